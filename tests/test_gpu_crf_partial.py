"""Partial-annotation CRF kernel (csrc/crf_partial.hip) through
ops.crf_partial_nll. Ground truth is ops.reference
.crf_partial_log_likelihood in fp64 on the same device; the tolerances are
the ones test_gpu_crf_wide.py holds the same scans to."""
import random

import numpy as np
import pytest
import torch

from chinesener_amd import ops
from chinesener_amd.ops import reference as ref

from conftest import make_tiny_params
from test_gpu_kernels import _cuda

pytestmark = pytest.mark.gpu

LL_TOL = dict(atol=1e-3, rtol=1e-4)
DEMIS_TOL = dict(atol=1e-3, rtol=1e-3)
DTRANS_TOL = dict(atol=1e-2, rtol=1e-3)


def _tmask(T):
    return (1 << T) - 1


def _to_i64(words, shape):
    """Python ints (64-bit patterns) -> int64 tensor, bit 63 included."""
    return torch.from_numpy(
        np.array(words, dtype=np.uint64).view(np.int64).reshape(shape).copy())


def _random_words(B, L, T, seed):
    """About half open, a third singletons, the rest random non-empty
    subsets; then some with stray bits >= T, some all-zero and, at T = 64,
    some with only bit 63."""
    rng = random.Random(seed)
    words = []
    for _ in range(B * L):
        r = rng.random()
        if r < 0.5:
            w = _tmask(T)
        elif r < 0.83:
            w = 1 << rng.randrange(T)
        else:
            w = (rng.getrandbits(T) & _tmask(T)) or (1 << rng.randrange(T))
        r = rng.random()
        if r < 0.10 and T < 64:
            w |= (rng.getrandbits(64 - T) or 1) << T
        elif r < 0.16:
            w = 0
        elif r < 0.22 and T == 64:
            w = 1 << 63
        words.append(w)
    return _to_i64(words, (B, L))


def _lens_for(B, L):
    """1, 2, L and an empty row wherever B has room for them."""
    if B >= 4:
        return ([1, 2, L, 0, L // 2, L - 1])[:B]
    if B == 3:
        return [L, 1, 0]
    return [L, 2]


def _inputs(B, L, T, seed, lens=None):
    g = torch.Generator().manual_seed(seed)
    em = torch.randn(B, L, T, generator=g).cuda()
    trans = torch.randn(T, T, generator=g).cuda()
    lens = torch.tensor(lens or _lens_for(B, L), device="cuda")
    assert lens.numel() == B
    mask = (torch.arange(L, device="cuda")[None, :] < lens[:, None]).long()
    allowed = _random_words(B, L, T, seed).cuda()
    w = torch.randn(B, generator=g).cuda()
    return em, trans, lens, mask, allowed, w


def _route(L, T):
    pair, nw, lds = ops.get_ext().crf_partial_route(L, T)
    return bool(pair), nw, lds


def _t64_edge():
    """(last L on the pair route, first on the split route) at T = 64."""
    last = max(L for L in range(1, 513) if _route(L, 64)[0])
    assert last < 512
    return last, last + 1


def _check_against_fp64(B, L, T, seed, lens=None):
    em, trans, lens, mask, allowed, w = _inputs(B, L, T, seed, lens)
    em64 = em.double().requires_grad_()
    tr64 = trans.double().requires_grad_()
    ll_ref = ref.crf_partial_log_likelihood(em64, allowed, mask, tr64,
                                            dtype=torch.float64)
    em2 = em.clone().requires_grad_()
    tr2 = trans.clone().requires_grad_()
    ll = ops.crf_partial_nll(em2, allowed, mask, tr2)
    print(f"({B},{L},{T}) route={_route(L, T)} "
          f"ll err={(ll.double() - ll_ref).abs().max().item():.3e}")
    torch.testing.assert_close(ll, ll_ref.float(), **LL_TOL)
    # ll <= 0; the slack is for rows where the constrained sum is the free one
    assert (ll <= LL_TOL["atol"]).all()

    (ll_ref * w.double()).sum().backward()
    (ll * w).sum().backward()
    print(f"  demis err={(em2.grad.double() - em64.grad).abs().max().item():.3e}"
          f" dtrans err={(tr2.grad.double() - tr64.grad).abs().max().item():.3e}")
    torch.testing.assert_close(em2.grad, em64.grad.float(), **DEMIS_TOL)
    torch.testing.assert_close(tr2.grad, tr64.grad.float(), **DTRANS_TOL)

    # raw kernel outputs: zeros past len and in empty rows, bitwise repeatable
    args = (em, allowed, lens.to(torch.int32), trans)
    out1 = ops.get_ext().crf_partial_fwd(*args)
    out2 = ops.get_ext().crf_partial_fwd(*args)
    for x, y in zip(out1, out2):
        assert torch.equal(x, y)
    ll_k, demis, dtrans = out1
    past = (mask == 0)[:, :, None].expand_as(demis)
    assert torch.count_nonzero(demis[past]) == 0
    for b in (lens == 0).nonzero().flatten().tolist():
        assert ll_k[b] == 0
        assert torch.count_nonzero(demis[b]) == 0
        assert torch.count_nonzero(dtrans[b]) == 0


# (5,40,10): the flagship width, TC = 12; (4,37,33): the first W=64 shape;
# (3,512,32): the largest pair-route W=32 shape; (2,512,64): the split route
@pytest.mark.parametrize("B,L,T", [(5, 40, 10), (6, 33, 24), (4, 37, 33),
                                   (3, 64, 64), (3, 512, 32), (2, 512, 64)])
def test_crf_partial_matches_fp64_reference(B, L, T):
    _cuda()
    _check_against_fp64(B, L, T, seed=100 + T)


def test_crf_partial_routes():
    _cuda()
    assert _route(40, 10)[0] and _route(150, 10)[0]
    assert _route(512, 32)[0]            # every W=32 shape pairs
    assert _route(64, 64)[0]
    assert not _route(512, 64)[0]
    for L, T in [(40, 10), (512, 32), (512, 64), (64, 64)]:
        pair, nw, lds = _route(L, T)
        assert lds <= 160 * 1024 and nw in (1, 2, 4)
        assert not pair or nw >= 2
    last, first = _t64_edge()
    assert _route(last, 64)[0] and not _route(first, 64)[0]


@pytest.mark.parametrize("side", ["last_pair", "first_split"])
def test_crf_partial_t64_route_edge(side):
    """T = 64 at the last L on the pair route and the first on the split
    route, as crf_partial_route reports them."""
    _cuda()
    last, first = _t64_edge()
    assert _route(last, 64)[0] != _route(first, 64)[0]
    L = last if side == "last_pair" else first
    _check_against_fp64(3, L, 64, seed=64, lens=[2, L, 0])


@pytest.mark.parametrize("B,L,T", [(5, 40, 10), (5, 33, 24), (5, 64, 64),
                                   (5, 512, 64)])
def test_crf_partial_open_rows_are_exactly_zero(B, L, T):
    """All-open and all-zero rows run the same arithmetic in both scans: ll,
    demis and dtrans are exactly 0, on the pair and on the split route."""
    _cuda()
    em, trans, lens, mask, allowed, _ = _inputs(
        B, L, T, seed=5, lens=[L, L, L - 1, L, 1])
    allowed[0] = _to_i64([_tmask(T)], (1,)).cuda()
    allowed[1] = 0
    # open below T, stray bits above it (at T = 64: all ones)
    allowed[2] = _to_i64([(1 << 64) - 1], (1,)).cuda()
    allowed[4] = 0
    ll, demis, dtrans = ops.get_ext().crf_partial_fwd(
        em, allowed, lens.to(torch.int32), trans)
    for b in (0, 1, 2, 4):
        assert ll[b] == 0
        assert torch.count_nonzero(demis[b]) == 0
        assert torch.count_nonzero(dtrans[b]) == 0
    assert ll[3] < 0 and torch.count_nonzero(demis[3]) > 0


@pytest.mark.parametrize("B,L,T", [(5, 40, 10), (4, 33, 24), (3, 64, 64),
                                   (2, 512, 64)])
def test_crf_partial_singletons_match_crf_nll(B, L, T):
    _cuda()
    g = torch.Generator().manual_seed(11 + T)
    em = torch.randn(B, L, T, generator=g).cuda()
    trans = torch.randn(T, T, generator=g).cuda()
    lens = torch.tensor(([L, 1, 2, L // 2, 3])[:B], device="cuda")
    mask = (torch.arange(L, device="cuda")[None, :] < lens[:, None]).long()
    tags = torch.randint(0, T, (B, L), generator=g).cuda()
    if T == 64:
        tags[:, ::5] = 63
    allowed = ops.allowed_from_tags(tags, torch.ones_like(tags, dtype=torch.bool),
                                    0)
    ll = ops.crf_partial_nll(em, allowed, mask, trans)
    ll_gold = ops.crf_nll(em, tags * mask, mask, trans)
    torch.testing.assert_close(ll, ll_gold, **LL_TOL)


def test_crf_partial_limits_raise():
    _cuda()
    ext = ops.get_ext()

    def args(L, T):
        return (torch.zeros(1, L, T, device="cuda"),
                torch.zeros(1, L, dtype=torch.int64, device="cuda"),
                torch.ones(1, dtype=torch.int32, device="cuda"),
                torch.zeros(T, T, device="cuda"))

    with pytest.raises(RuntimeError, match="64"):
        ext.crf_partial_fwd(*args(8, 65))
    with pytest.raises(RuntimeError, match="512"):
        ext.crf_partial_fwd(*args(513, 24))
    with pytest.raises(RuntimeError, match="512"):
        ext.crf_partial_route(513, 24)


def test_crf_partial_graph_capture_replay():
    """Forward plus autograd.grad under torch.cuda.graph: no host sync, and
    with no atomics a replay equals the eager call bit for bit."""
    _cuda()
    B, L, T = 4, 40, 10
    sets = [_inputs(B, L, T, seed=300 + i) for i in range(3)]
    _, _, _, mask, _, w = sets[0]

    def step(em, trans, allowed):
        ll = ops.crf_partial_nll(em, allowed, mask, trans)
        d_em, d_tr = torch.autograd.grad((ll * w).sum(), (em, trans))
        return ll, d_em, d_tr

    s_em = sets[0][0].clone().requires_grad_()
    s_tr = sets[0][1].clone().requires_grad_()
    s_al = sets[0][4].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(s_em, s_tr, s_al)
    torch.cuda.current_stream().wait_stream(side)

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s_out = step(s_em, s_tr, s_al)
    for em, trans, _, _, allowed, _ in sets[1:]:
        with torch.no_grad():
            s_em.copy_(em)
            s_tr.copy_(trans)
            s_al.copy_(allowed)
        graph.replay()
        e_out = step(em.clone().requires_grad_(),
                     trans.clone().requires_grad_(), allowed)
        for s, e in zip(s_out, e_out):
            assert torch.equal(s, e)


def test_bilstm_crf_trains_on_msra_partial_batch():
    """bilstm_crf on a synthetic msra_partial batch: 30 optimizer steps, the
    loss finite throughout and lower at the end than at the start."""
    _cuda()
    torch.manual_seed(0)
    from chinesener_amd.data.datasets import get_spec, load_data
    from chinesener_amd.data.loader import _to_tensors
    from chinesener_amd.data.preprocess import get_instance
    from chinesener_amd.models import build_model
    spec = get_spec("msra_partial")
    params = make_tiny_params("bilstm_crf")
    assert params["tag2idx"] == spec.tag2idx
    proc = get_instance("char", params["max_seq_len"], spec.tag2idx,
                        unknown_tag=spec.unknown_tag)
    params["vocab_size"] = len(proc.tokenizer.vocab)
    # no corpus files here: the synthetic, thinned-out train split
    sentences, tags = load_data("msra_partial", "no-such-dir/msra_partial",
                                "train")
    arrays = proc.stack([proc.build_seq_feature(s, t)
                         for s, t in zip(sentences[:6], tags[:6])])
    batch = _to_tensors(arrays, np.arange(6))
    assert batch["allowed_tags"].dtype == torch.int64
    open_word = 0b11111110          # O and the six entity tags
    assert (batch["allowed_tags"] == open_word).any()
    batch = {k: v.cuda() for k, v in batch.items()}
    model = build_model("bilstm_crf", params).to("cuda")
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    losses = []
    for _ in range(30):
        opt.zero_grad(set_to_none=True)
        out = model(batch)
        assert torch.isfinite(out.loss)
        losses.append(float(out.loss.detach()))
        out.loss.backward()
        opt.step()
    assert losses[-1] < losses[0]
