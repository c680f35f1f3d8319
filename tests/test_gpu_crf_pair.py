"""The CRF loss kernel (csrc/crf_pair.hip: forward and backward scans of a
row on two waves at once, then a combine that is parallel over t) and the
one-launch chain rule crf_grad_scale, at their edges: every scanned width,
partial blocks, B = 1, rows of one and two tokens, empty rows, rows of 512
tokens, confident logits, and both sides of the hand-over to crf_wide.hip.
Label sizes above 48 stay on crf_wide.hip; their cases (49 and 64 tags) are
kept, as the other side of that boundary.

Truth and tolerance are tests/test_gpu_crf_narrow.py's, imported from
there: an fp64 scan (at tiny shapes an enumeration of every path), and

    err_k <= 4 * err_32 + 16 * 2^-24 * (1 + M)

with ops.reference as the fp32 reference. Each figure is printed before it
is asserted. With one tag ops.reference is exact (err_32 = 0, M = 0 for
both gradients), so that case holds the kernel to 16 * 2^-24 on every
marginal and on a sum of L - 1 pair terms.

The labels that tests/test_gpu_crf_narrow.py prints ("x4", "x1", "wide")
name the routes crf_fwd had before this kernel; every case there that says
x4 or x1 now runs here. The hand-over lengths below are asked of
crf_fwd_route, not written down."""
import pytest
import torch

from chinesener_amd import ops

from test_gpu_kernels import _cuda
from test_gpu_crf_narrow import (_Report, _enumerate64, _inputs,
                                 _path_score64, _ref32, _ref64)

gpu = pytest.mark.gpu

EPS32 = 2.0 ** -24

# T at every edge of the scanned widths 12, 24, 32 | 48, 64; B = 5 leaves a
# partial block at one and at two sequences per block
EDGE_CASES = [(5, 33 + T % 8, T)
              for T in (1, 2, 12, 13, 24, 25, 32, 33, 48, 49, 64)]
SHAPE_CASES = [(1, 37, 10),              # B = 1
               (5, 1, 10), (5, 2, 10),   # no scan step; empty / one-term pairs
               (5, 1, 1), (5, 2, 33),
               (3, 512, 10), (2, 512, 32)]   # cancellation over long rows
SCALE8_CASES = [(5, 37, 12), (5, 34, 33), (3, 512, 10)]
HANDOVER_T = [48]       # the scanned width whose route ends below 512
PAIR_MAX_T = 48         # above it crf_fwd keeps crf_wide.hip at every L


def _lens(B, L, empty_last=False):
    """From {L, 1, 2, L/2, L-1, 0}."""
    base = [L, 1, 2, max(1, L // 2), max(1, L - 1)]
    out = [min(L, base[i % 5]) for i in range(B)]
    if empty_last:
        out[-1] = 0
    return out


def _junk(*sizes):
    """NaN-filled blocks of the output sizes, freed again: the allocator is
    likely to hand them to the at::empty outputs."""
    junk = [torch.full((n,), float("nan"), device="cuda")
            for n in sizes for _ in range(3)]
    del junk


def _raw(em, trans, lens, tags):
    B, L, T = em.shape
    _junk(B, B * L * T, B * T * T)
    out = ops.get_ext().crf_fwd(em.cuda(), tags.to(torch.int32).cuda(),
                                lens.to(torch.int32).cuda(), trans.cuda())
    return [o.cpu() for o in out]


def _check_raw(ll, demis, dtrans, lens, mask):
    """Every cell written: no NaN, zeros past len, zeros in empty rows."""
    B, L, T = demis.shape
    assert torch.isfinite(ll).all() and torch.isfinite(demis).all()
    assert torch.isfinite(dtrans).all()
    past = (mask == 0)[:, :, None].expand(B, L, T)
    assert torch.count_nonzero(demis[past]) == 0
    empty = lens == 0
    assert torch.count_nonzero(ll[empty]) == 0
    assert torch.count_nonzero(dtrans[empty]) == 0


def _check_case(B, L, T, scale=1.0, empty_last=False, label=""):
    em, trans, lens, mask, tags, w = _inputs(
        B, L, T, scale, lens=_lens(B, L, empty_last))
    ll64, logz64, dem64, dtr64 = _ref64(em, trans, lens, tags, w)
    keep = lens > 0
    ll32, dem32, dtr32 = _ref32(em[keep], trans, mask[keep], tags[keep],
                                w[keep])
    if L == 1:   # no transition is scored: autograd returns no gradient
        assert dtr64 is None and dtr32 is None
        dtr64 = torch.zeros(T, T, dtype=torch.float64)
        dtr32 = torch.zeros(T, T)
    ll_r, demis_r, dtrans_r = _raw(em, trans, lens, tags)
    _check_raw(ll_r, demis_r, dtrans_r, lens, mask)

    _junk(B, B * L * T, B * T * T, T * T)
    em_g = em.cuda().requires_grad_()
    tr_g = trans.cuda().requires_grad_()
    ll = ops.crf_nll(em_g, tags.cuda(), mask.cuda(), tr_g)
    (ll * w.cuda()).sum().backward()
    ll, dem, dtr = ll.detach().cpu(), em_g.grad.cpu(), tr_g.grad.cpu()
    assert torch.equal(ll, ll_r)

    route = ops.get_ext().crf_fwd_route(L, T)
    rep = _Report(f"({B},{L},{T}) scale={scale:g} route={route} {label}")
    rep.check("ll", ll[keep], ll64[keep], ll32,
              M=float(logz64[keep].abs().max()))
    rep.check("emissions.grad", dem[keep], dem64[keep], dem32)
    rep.check("transitions.grad", dtr, dtr64, dtr32)
    past = (mask == 0)[:, :, None].expand(B, L, T)
    assert torch.count_nonzero(dem[past]) == 0
    rep.finish()


@gpu
@pytest.mark.parametrize("B,L,T", EDGE_CASES + SHAPE_CASES)
def test_crf_pair_nll_and_grads(B, L, T):
    _cuda()
    assert ops.get_ext().crf_fwd_route(L, T)[0] == (1 if T <= PAIR_MAX_T else 0)
    _check_case(B, L, T)


@gpu
@pytest.mark.parametrize("B,L,T", [(5, 36, 12), (4, 34, 25), (3, 35, 48),
                                   (2, 1, 10)])
def test_crf_pair_last_row_empty(B, L, T):
    _cuda()
    _check_case(B, L, T, empty_last=True)


@gpu
@pytest.mark.parametrize("B,L,T", SCALE8_CASES)
def test_crf_pair_confident_logits(B, L, T):
    """The narrow file's scale-8 draw: alpha grows to tens of thousands."""
    _cuda()
    _check_case(B, L, T, scale=8.0)


def _last_pair_len(T):
    ext = ops.get_ext()
    fits = [L for L in range(1, 513) if ext.crf_fwd_route(L, T)[0] == 1]
    assert fits and fits == list(range(1, fits[-1] + 1))   # one interval
    return fits[-1]


@gpu
@pytest.mark.parametrize("side", ["last-on", "first-off"])
@pytest.mark.parametrize("T", HANDOVER_T)
def test_crf_pair_hand_over_to_wide(T, side):
    """The last L on the pair route and the first L off it, both from
    crf_fwd_route."""
    _cuda()
    ext = ops.get_ext()
    last = _last_pair_len(T)
    assert last < 512, f"T={T}: the pair route no longer ends below 512"
    L = last if side == "last-on" else last + 1
    pair, waves, lds = ext.crf_fwd_route(L, T)
    assert pair == (1 if side == "last-on" else 0)
    if pair:
        assert waves in (2, 4) and 0 < lds <= 160 * 1024
    _check_case(2, L, T, label=side)


@gpu
def test_crf_pair_route_covers_every_narrow_tagset():
    """Every T <= 32 is on the pair route up to L = 512; no T above 48 is
    on it at any L (that class measured slower than crf_wide.hip)."""
    _cuda()
    ext = ops.get_ext()
    for T in (49, 64):
        assert all(ext.crf_fwd_route(L, T)[0] == 0 for L in range(1, 513))
    for T in (1, 10, 12, 13, 20, 24, 25, 32):
        for L in (1, 128, 511, 512):
            pair, waves, lds = ext.crf_fwd_route(L, T)
            assert pair == 1 and lds <= 160 * 1024, (L, T)


@gpu
@pytest.mark.parametrize("B,L,T,lens", [(3, 4, 3, [4, 0, 2]),
                                        (2, 5, 2, [5, 1])])
def test_crf_pair_matches_enumeration(B, L, T, lens):
    _cuda()
    em, trans, lens, mask, tags, _ = _inputs(B, L, T, lens=lens)
    ll, demis, dtrans = _raw(em, trans, lens, tags)
    _check_raw(ll, demis, dtrans, lens, mask)
    rep = _Report(f"pair enumeration ({B},{L},{T})")
    for b in range(B):
        n = int(lens[b])
        if n == 0:
            continue
        log_z, marg, pair = _enumerate64(em[b], trans, n)
        gold = _path_score64(em[b], trans, tags[b].tolist(), n)
        onehot = torch.nn.functional.one_hot(tags[b, :n], T).double()
        counts = torch.zeros(T, T, dtype=torch.float64)
        for t in range(1, n):
            counts[tags[b, t - 1], tags[b, t]] += 1
        rep.check(f"row {b} ll", ll[b],
                  torch.tensor(gold - log_z, dtype=torch.float64), M=abs(log_z))
        rep.check(f"row {b} marginals", onehot - demis[b, :n].double(), marg)
        rep.check(f"row {b} pair counts", counts - dtrans[b].double(), pair)
    rep.finish()


@gpu
@pytest.mark.parametrize("B,L,T", [(5, 37, 12), (3, 40, 48), (5, 2, 10)])
def test_crf_pair_is_bitwise_reproducible(B, L, T):
    _cuda()
    em, trans, lens, mask, tags, _ = _inputs(B, L, T,
                                             lens=_lens(B, L, True))
    first = _raw(em, trans, lens, tags)
    second = _raw(em, trans, lens, tags)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


@gpu
@pytest.mark.parametrize("seqs", [1, 2])
def test_crf_pair_sequences_per_block_agree(seqs):
    """One and two sequences per block run the same arithmetic per row."""
    _cuda()
    B, L, T = 5, 37, 10
    em, trans, lens, mask, tags, _ = _inputs(B, L, T,
                                             lens=_lens(B, L, True))
    want = _raw(em, trans, lens, tags)
    _junk(B, B * L * T, B * T * T)
    got = ops.get_ext().crf_pair_fwd(
        em.cuda(), tags.to(torch.int32).cuda(), lens.to(torch.int32).cuda(),
        trans.cuda(), seqs_per_block=seqs)
    for a, b in zip(want, got):
        assert torch.equal(a, b.cpu())


@gpu
@pytest.mark.parametrize("B", [1, 7])
def test_crf_grad_scale_matches_fp64(B):
    """Against the torch expression in fp64. A cell of demis_out is one
    rounded product: |err| <= u |d w|. A cell of dtrans_out is B rounded
    products summed in fp32 in index order: |err| <= gamma_B sum_b |d_b w_b|
    with gamma_B = B u / (1 - B u), u = 2^-24 (Higham, Accuracy and
    Stability of Numerical Algorithms, section 4.2; a fused multiply-add
    only drops roundings)."""
    _cuda()
    L, T = 9, 5
    g = torch.Generator().manual_seed(7 + B)
    demis = torch.randn(B, L, T, generator=g)
    dtrans = torch.randn(B, T, T, generator=g) * 3
    dll = torch.randn(B, generator=g)
    dll[0] = -abs(dll[0]) - 0.5
    if B > 2:
        dll[2] = 0.0
        dll[B - 1] = 0.0
    d_g, t_g, w_g = demis.cuda(), dtrans.cuda(), dll.cuda()
    _junk(B * L * T, T * T)
    d_out, t_out = ops.get_ext().crf_grad_scale(d_g, t_g, w_g)
    assert d_out.data_ptr() != d_g.data_ptr()
    assert torch.equal(d_g.cpu(), demis) and torch.equal(t_g.cpu(), dtrans)
    assert tuple(d_out.shape) == (B, L, T) and tuple(t_out.shape) == (T, T)
    w64 = dll.double()[:, None, None]
    want_d = demis.double() * w64
    terms = dtrans.double() * w64
    want_t = terms.sum(0)
    u = EPS32
    err_d = (d_out.cpu().double() - want_d).abs()
    err_t = (t_out.cpu().double() - want_t).abs()
    bound_t = (B * u / (1 - B * u)) * terms.abs().sum(0)
    print(f"crf_grad_scale B={B}: demis err={float(err_d.max()):.3e} "
          f"dtrans err={float(err_t.max()):.3e} "
          f"dtrans bound>={float(bound_t.min()):.3e}")
    assert bool((err_d <= u * want_d.abs()).all())
    assert bool((err_t <= bound_t).all())
    if B > 2:   # an exact-zero weight gives an exact zero, either sign
        assert torch.count_nonzero(d_out[2]) == 0
    # an expanded scalar (what a summed loss hands backward) is read in place
    one = w_g[:1].expand(B)
    assert B == 1 or one.stride(0) == 0
    d_one, t_one = ops.get_ext().crf_grad_scale(d_g, t_g, one)
    d_ref, t_ref = ops.get_ext().crf_grad_scale(d_g, t_g, one.contiguous())
    assert torch.equal(d_one, d_ref) and torch.equal(t_one, t_ref)
    assert torch.equal(d_one.cpu(), demis * dll[0])


@gpu
def test_crf_nll_second_backward_sees_the_saved_tensors():
    """crf_grad_scale never scales in place."""
    _cuda()
    B, L, T = 3, 6, 4
    em, trans, lens, mask, tags, w = _inputs(B, L, T, lens=[6, 3, 1])
    em_g = em.cuda().requires_grad_()
    tr_g = trans.cuda().requires_grad_()
    ll = ops.crf_nll(em_g, tags.cuda(), mask.cuda(), tr_g)
    loss = (ll * w.cuda()).sum()
    first = torch.autograd.grad(loss, (em_g, tr_g), retain_graph=True)
    second = torch.autograd.grad(loss, (em_g, tr_g))
    for a, b in zip(first, second):
        assert torch.equal(a, b)
