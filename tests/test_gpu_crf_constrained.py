"""Constrained Viterbi kernel (csrc/crf_constrained.hip) against the fp64
reference ops.reference.crf_decode_constrained on the CPU, against the fp32
reference bit for bit on exactly representable data, and against the
existing Viterbi kernels with open words.

Bound: TOL = 1e-3 absolute on path scores, the project's CRF figure
(test_gpu_crf_nbest.py). Each case prints its measured maxima before it
asserts. Measured on MI355X over all shapes: max|fp64(path) - ref optimum|
0.0, max|score - fp64(path)| 4.6e-4 at (3, 512, 20), below 7e-6 at L <= 40
(profiles/crf_constrained_r15.md). The score is an fp32 sum along the path:
with open words at (3, 512, 64) it reaches 1.9e3, where 512 roundings of
half an ulp (6e-5) add up to 1.1e-3, so the open-word test checks the
returned paths, not the fp32 score."""
import functools

import pytest
import torch

from chinesener_amd import ops
from chinesener_amd.ops import reference as ref

from test_gpu_kernels import _cuda
from test_gpu_crf_posterior import SHAPES, _inputs, _lens_for

pytestmark = pytest.mark.gpu

TOL = 1e-3
NINF = float("-inf")


def _word(bits):
    """A Python bit pattern as the signed value int64 holds."""
    bits &= (1 << 64) - 1
    return bits - (1 << 64) if bits >= 1 << 63 else bits


BIT = [_word(1 << i) for i in range(64)]      # singleton words


def _witness_words(B, L, T, seed):
    """Position words [B,L] and transition words [T] that admit a drawn
    witness path on every row: a third singletons, a third random supersets
    of the witness tag, a third zero; transition words hold the witness
    transitions plus random bits."""
    g = torch.Generator().manual_seed(seed)
    wit = torch.randint(0, T, (B, L), generator=g).tolist()
    kind = torch.randint(0, 3, (B, L), generator=g).tolist()
    extra = torch.randint(0, 2, (B, L, T), generator=g).tolist()
    words = []
    for b in range(B):
        row = []
        for t in range(L):
            w = 1 << wit[b][t]
            if kind[b][t] == 1:
                for j in range(T):
                    if extra[b][t][j]:
                        w |= 1 << j
            elif kind[b][t] == 2:
                w = 0
            row.append(_word(w))
        words.append(row)
    tbits = torch.randint(0, 2, (T, T), generator=g).tolist()
    tw = [0] * T
    for i in range(T):
        for j in range(T):
            if tbits[i][j]:
                tw[i] |= 1 << j
    for b in range(B):
        for t in range(L - 1):
            tw[wit[b][t]] |= 1 << wit[b][t + 1]
    return (torch.tensor(words, dtype=torch.int64).reshape(B, L),
            torch.tensor([_word(w) for w in tw], dtype=torch.int64))


@functools.lru_cache(maxsize=None)
def _case(B, L, T):
    """Float inputs of one shape on the GPU, the words, and the fp64 CPU
    reference result, computed once."""
    em, trans, lens, mask, _ = _inputs(B, L, T, seed=900 + L + T)
    allowed, tallowed = _witness_words(B, L, T, seed=77 + L + T)
    rp, rs = ref.crf_decode_constrained(em.double().cpu(), allowed,
                                        mask.cpu(), trans.double().cpu(),
                                        tallowed)
    return em, trans, lens, mask, allowed, tallowed, rp, rs


def _path_score64(em64, tr64, path, n):
    p = path[:n]
    s = em64[torch.arange(n), p].sum()
    if n > 1:
        s = s + tr64[p[:-1], p[1:]].sum()
    return s.item()


def _mask_of(lens, L):
    lens = torch.as_tensor(lens, device="cuda")
    return (torch.arange(L, device="cuda")[None, :] < lens[:, None]).long()


@pytest.mark.parametrize("B,L,T", SHAPES)
def test_constrained_matches_fp64_reference(B, L, T):
    _cuda()
    em, trans, lens, mask, allowed, tallowed, rp, rs = _case(B, L, T)
    assert torch.isfinite(rs).all(), "feasible by construction: no row left out"
    pred, score = ops.crf_viterbi_constrained(em, allowed.cuda(), mask, trans,
                                              tallowed.cuda())
    assert pred.dtype == torch.long and pred.shape == (B, L)
    assert score.dtype == torch.float32 and score.shape == (B,)
    pred, score = pred.cpu(), score.cpu()
    sets = ref.allowed_sets(allowed, T)
    tsets = ref.transition_sets(tallowed, T)
    em64, tr64 = em.double().cpu(), trans.double().cpu()
    err_ref = err_self = 0.0
    for b in range(B):
        n = int(lens[b])
        p = pred[b]
        assert sets[b, torch.arange(n), p[:n]].all(), b
        assert tsets[p[:n - 1], p[1:n]].all(), b
        assert torch.count_nonzero(p[n:]) == 0
        s64 = _path_score64(em64[b], tr64, p, n)
        err_ref = max(err_ref, abs(s64 - rs[b].item()))
        err_self = max(err_self, abs(score[b].item() - s64))
    print(f"crf_viterbi_constrained {(B, L, T)}: max|fp64(path) - ref optimum|"
          f" {err_ref:.3e}  max|score - fp64(path)| {err_self:.3e}")
    assert err_ref <= TOL
    assert err_self <= TOL


@pytest.mark.parametrize("B,L,T", SHAPES)
def test_constrained_small_integers_bitwise(B, L, T):
    """Values in [-2, 2] are exact in fp32 and so is every path score: the
    kernel must reproduce the fp32 reference bit for bit, ties included."""
    _cuda()
    g = torch.Generator().manual_seed(31 + L + T)
    em = torch.randint(-2, 3, (B, L, T), generator=g).float()
    trans = torch.randint(-2, 3, (T, T), generator=g).float()
    lens = torch.tensor(_lens_for(B, L))
    mask = (torch.arange(L)[None, :] < lens[:, None]).long()
    allowed, tallowed = _witness_words(B, L, T, seed=5 + L + T)
    rp, rs = ref.crf_decode_constrained(em, allowed, mask, trans, tallowed)
    assert torch.isfinite(rs).all()
    pred, score = ops.crf_viterbi_constrained(
        em.cuda(), allowed.cuda(), mask.cuda(), trans.cuda(), tallowed.cuda())
    assert torch.equal(pred.cpu(), rp)
    assert torch.equal(score.cpu(), rs)


# narrow crf.hip shapes, and the wide route (T > 20, and T = 20 at L = 512)
@pytest.mark.parametrize("B,L,T", [(7, 40, 10), (6, 33, 20), (5, 40, 21),
                                   (4, 37, 64), (3, 512, 20), (3, 512, 64)])
def test_open_words_agree_with_crf_viterbi(B, L, T):
    _cuda()
    em, trans, lens, mask, _ = _inputs(B, L, T, seed=300 + L + T)
    allowed = torch.zeros(B, L, dtype=torch.int64, device="cuda")
    pred, score = ops.crf_viterbi_constrained(em, allowed, mask, trans)
    vit = ops.crf_viterbi(em, mask, trans)
    em64, tr64 = em.double().cpu(), trans.double().cpu()
    gap = 0.0
    for b in range(B):
        n = int(lens[b])
        a = _path_score64(em64[b], tr64, pred[b].cpu(), n)
        v = _path_score64(em64[b], tr64, vit[b].cpu(), n)
        gap = max(gap, abs(a - v))
    assert torch.isfinite(score).all()
    print(f"open words {(B, L, T)}: max|fp64 score gap to crf_viterbi| "
          f"{gap:.3e}")
    assert gap <= TOL


def test_empty_batch():
    _cuda()
    em = torch.zeros(0, 5, 7, device="cuda")
    pred, score = ops.crf_viterbi_constrained(
        em, torch.zeros(0, 5, dtype=torch.int64, device="cuda"),
        torch.zeros(0, 5, dtype=torch.long, device="cuda"),
        torch.zeros(7, 7, device="cuda"))
    assert pred.shape == (0, 5) and score.shape == (0,)


@pytest.mark.parametrize("T", [10, 64])
def test_infeasible_row_leaves_neighbours_alone(T):
    """Row 2 is pinned to tag i then tag j with i -> j forbidden; row 4 is
    empty. Both get -inf and zeros; the rows sharing their block equal their
    own batch-1 results."""
    _cuda()
    B, L = 6, 9
    em, trans, _, _, _ = _inputs(B, L, T, seed=11 + T)
    lens = [L, 3, L, 5, 0, 1]
    mask = _mask_of(lens, L)
    i, j = 3, T - 1
    allowed = torch.zeros(B, L, dtype=torch.int64)
    allowed[2, 4], allowed[2, 5] = BIT[i], BIT[j]
    allowed[0, 2] = BIT[1]
    tw = [-1] * T
    tw[i] = _word(~(1 << j))
    tallowed = torch.tensor(tw, dtype=torch.int64).cuda()
    allowed = allowed.cuda()
    pred, score = ops.crf_viterbi_constrained(em, allowed, mask, trans,
                                              tallowed)
    for b in (2, 4):
        assert score[b].item() == NINF
        assert torch.count_nonzero(pred[b]) == 0
    for b in (0, 1, 3, 5):
        p1, s1 = ops.crf_viterbi_constrained(
            em[b:b + 1], allowed[b:b + 1], mask[b:b + 1], trans, tallowed)
        assert torch.equal(pred[b], p1[0]) and torch.equal(score[b], s1[0])
        assert torch.isfinite(score[b])
    assert pred[0, 2].item() == 1


def test_high_bits_and_bit_63():
    _cuda()
    # a word with only bits >= T set counts as open
    B, L, T = 3, 12, 10
    em, trans, _, _, _ = _inputs(B, L, T, seed=3)
    mask = _mask_of([L] * B, L)
    zero = torch.zeros(B, L, dtype=torch.int64, device="cuda")
    high = torch.full((B, L), _word(((1 << 64) - 1) & ~((1 << T) - 1)),
                      dtype=torch.int64, device="cuda")
    p0, s0 = ops.crf_viterbi_constrained(em, zero, mask, trans)
    p1, s1 = ops.crf_viterbi_constrained(em, high, mask, trans)
    assert torch.equal(p0, p1) and torch.equal(s0, s1)
    # bit 63 at T = 64: as a singleton, and as the only forbidden tag
    T = 64
    em, trans, _, _, _ = _inputs(B, L, T, seed=4)
    em[:, 5, 63] += 50.0          # free decoding takes tag 63 at t = 5
    free, _ = ops.crf_viterbi_constrained(em, zero, mask, trans)
    assert (free[:, 5] == 63).all()
    words = zero.clone()
    words[:, 5] = _word(~(1 << 63))
    pred, score = ops.crf_viterbi_constrained(em, words, mask, trans)
    assert (pred[:, 5] != 63).all() and torch.isfinite(score).all()
    words = zero.clone()
    words[:, 2] = BIT[63]
    pred, score = ops.crf_viterbi_constrained(em, words, mask, trans)
    assert (pred[:, 2] == 63).all() and torch.isfinite(score).all()
    rp, rs = ref.crf_decode_constrained(em.double().cpu(), words.cpu(),
                                        mask.cpu(), trans.double().cpu())
    for b in range(B):
        s64 = _path_score64(em[b].double().cpu(), trans.double().cpu(),
                            pred[b].cpu(), L)
        assert abs(s64 - rs[b].item()) <= TOL


def test_every_output_cell_written():
    """Two calls of one shape, the second with shorter rows: its cells at
    t >= len are 0, not what the first call (or the allocator) left."""
    _cuda()
    B, L, T = 5, 40, 21
    em, trans, _, _, _ = _inputs(B, L, T, seed=8)
    em = em + 3.0 * torch.nn.functional.one_hot(
        torch.full((B, L), 7), T).cuda()          # tag 7 nearly everywhere
    zero = torch.zeros(B, L, dtype=torch.int64, device="cuda")
    lens_a, lens_b = [L] * B, [3, 0, 17, 1, L]
    pa, _ = ops.crf_viterbi_constrained(em, zero, _mask_of(lens_a, L), trans)
    assert torch.count_nonzero(pa) > B * L // 2
    del pa
    pb, sb = ops.crf_viterbi_constrained(em, zero, _mask_of(lens_b, L), trans)
    for b, n in enumerate(lens_b):
        assert torch.count_nonzero(pb[b, n:]) == 0
    assert sb[1].item() == NINF
    raw_p, raw_s = ops.get_ext().crf_viterbi_constrained(
        em, zero, torch.tensor(lens_b, dtype=torch.int32, device="cuda"),
        trans, torch.full((T,), -1, dtype=torch.int64, device="cuda"))
    assert torch.equal(raw_p.long(), pb) and torch.equal(raw_s, sb)


def test_range_error():
    _cuda()
    em = torch.zeros(1, 4, 65, device="cuda")
    with pytest.raises(RuntimeError, match="outside the supported range"):
        ops.crf_viterbi_constrained(
            em, torch.zeros(1, 4, dtype=torch.int64, device="cuda"),
            torch.ones(1, 4, dtype=torch.long, device="cuda"),
            torch.zeros(65, 65, device="cuda"))


def test_graph_capture_replays_with_new_words():
    _cuda()
    B, L, T = 6, 33, 20
    em, trans, lens, mask, _ = _inputs(B, L, T, seed=21)
    lens32 = lens.to(torch.int32)
    tallowed = torch.full((T,), -1, dtype=torch.int64, device="cuda")
    words = [_witness_words(B, L, T, seed=s)[0].cuda() for s in (1, 2, 3)]
    fn = ops.get_ext().crf_viterbi_constrained
    eager = [fn(em, w, lens32, trans, tallowed) for w in words]
    static = words[0].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn(em, static, lens32, trans, tallowed)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn(em, static, lens32, trans, tallowed)
    for w, (ep, es) in list(zip(words, eager))[1:]:
        static.copy_(w)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], ep) and torch.equal(out[1], es)
