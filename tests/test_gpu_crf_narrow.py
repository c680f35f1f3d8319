"""Narrow CRF kernels (csrc/crf.hip, at most 20 tags) at their edges:
partial 4-groups and blocks, T = 1, 2, 16, 17, 20, the full 160 KB of
dynamic LDS, the switch from four sequences per wave to one, the hand-over
to crf_wide.hip, empty rows and non-finite emissions.

The truth is a plain fp64 scan written here (and, at tiny shapes, an
enumeration of every path). ops.reference casts to fp32, so it is only the
fp32 reference: its own distance from the fp64 scan sets the tolerance,

    err_k <= 4 * err_32 + 16 * 2^-24 * (1 + M),

with err_k = max|kernel - ref64|, err_32 = max|ops.reference - ref64| on
the same inputs, and M = max|logZ64| for ll, max|ref64 value| for a
gradient. The factor 4 is the kernel's margin over the fp32 reference
(__expf/__logf are a few ulp against libm's one; the gold score is summed
in another order); the floor covers inputs on which the fp32 reference
happens to be exact (T = 1). Each figure is printed before it is asserted;
profiles/crf_narrow_tests.md has the measured table.

Both references run on the CPU, so the tolerance does not depend on the
device's fp32 library.

At T = 16 the four-per-wave kernel fits up to L = 159 (1024 + 64*159*16 is
exactly 160 KB), so (5, 158, 16) and (5, 159, 16) both run on it and
(5, 160, 16) is the T <= 16 case of the one-per-wave kernel."""
import itertools

import pytest
import torch

from chinesener_amd import ops
from chinesener_amd.ops import reference as ref

from test_gpu_kernels import _cuda

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24
LDS_BYTES = 160 * 1024


def _route(L, T):
    """Which kernel crf_fwd launches. Mirrors the host rule of crf_fwd in
    csrc/crf.hip (4 waves per block, fp32 alpha): keep the two in step."""
    if T <= 16 and 16 * 16 * 4 + 4 * 4 * L * T * 4 <= LDS_BYTES:
        return "x4"
    if T <= 20 and 20 * 20 * 4 + 4 * L * T * 4 <= LDS_BYTES:
        return "x1"
    return "wide"


def _route_viterbi(L, T):
    """The same for crf_viterbi (int8 backpointers, row stride 16 or 20)."""
    if T <= 16 and 16 * 16 * 4 + 4 * 4 * L * 16 <= LDS_BYTES:
        return "x4"
    if T <= 20 and 20 * 20 * 4 + 4 * L * 20 <= LDS_BYTES:
        return "x1"
    return "wide"


# (B, L, T) -> the route the case is here for
LOSS_CASES = {
    (5, 9, 1): "x4",        # T=1: ll is 0, every marginal is 1
    (6, 12, 2): "x4",
    (7, 40, 7): "x4",       # second wave has three of four groups
    (17, 33, 13): "x4",     # second block holds one row
    (5, 158, 16): "x4",     # T=16, all 16 lanes of a group, 162816 B of LDS
    (5, 159, 16): "x4",     # exactly 163840 B: the largest L that fits at T=16
    (5, 160, 16): "x1",     # T <= 16 on the one-per-wave kernel
    (3, 254, 10): "x4",     # the switch at the production tag count
    (3, 255, 10): "x1",
    (5, 30, 17): "x1",      # smallest T above 16
    (6, 45, 20): "x1",      # T=TMAX, two blocks, the second partial
    (2, 507, 20): "x1",     # exactly 163840 B of LDS
    (2, 508, 20): "wide",   # continuity across the hand-over
}
SCALE8_CASES = [(7, 40, 7), (5, 158, 16), (6, 45, 20)]

VITERBI_CASES = {
    (5, 9, 1): "x4", (6, 12, 2): "x4", (7, 40, 7): "x4", (17, 33, 13): "x4",
    (5, 158, 16): "x4", (3, 512, 16): "x4",
    (5, 30, 17): "x1", (6, 45, 20): "x1",
}


def _lens_for(B, L):
    base = [L, 1, 2, max(1, L // 2), 3, max(1, L - 1), 7]
    return [min(L, base[i % 7]) for i in range(B)]


def _inputs(B, L, T, scale=1.0, lens=None):
    """CPU fp32 inputs; the draw order is part of the test's definition."""
    g = torch.Generator().manual_seed(1000 + 100 * T + L)
    lens = torch.tensor(_lens_for(B, L) if lens is None else lens)
    assert lens.numel() == B
    mask = (torch.arange(L)[None, :] < lens[:, None]).long()
    em = torch.randn(B, L, T, generator=g) * scale
    trans = torch.randn(T, T, generator=g) * scale
    tags = torch.randint(0, T, (B, L), generator=g) * mask
    w = torch.randn(B, generator=g)
    return em, trans, lens, mask, tags, w


# ------------------------------------------------------------ fp64 truth
def _scan64(em, tags, lens, trans):
    """Forward algorithm in fp64. Returns (ll [B], logZ [B]); a row with
    lens == 0 has ll = 0 and takes no gradient."""
    assert em.dtype == torch.float64 and trans.dtype == torch.float64
    B, L, T = em.shape
    rows = torch.arange(B)
    alpha = em[:, 0]
    score = em[rows, 0, tags[:, 0]]
    for t in range(1, L):
        live = t < lens
        nxt = torch.logsumexp(alpha[:, :, None] + trans[None], dim=1) + em[:, t]
        alpha = torch.where(live[:, None], nxt, alpha)
        step = trans[tags[:, t - 1], tags[:, t]] + em[rows, t, tags[:, t]]
        score = score + torch.where(live, step, torch.zeros_like(step))
    log_z = torch.logsumexp(alpha, dim=1)
    ll = torch.where(lens > 0, score - log_z, torch.zeros_like(score))
    return ll, log_z


def _ref64(em, trans, lens, tags, w):
    """(ll, logZ, d_em, d_trans) of (ll * w).sum() in fp64."""
    em64 = em.double().requires_grad_()
    tr64 = trans.double().requires_grad_()
    ll, log_z = _scan64(em64, tags, lens, tr64)
    (ll * w.double()).sum().backward()
    return ll.detach(), log_z.detach(), em64.grad, tr64.grad


def _ref32(em, trans, mask, tags, w):
    """The same from ops.reference (fp32 inside). Rows must be non-empty."""
    em32 = em.clone().requires_grad_()
    tr32 = trans.clone().requires_grad_()
    ll = ref.crf_log_likelihood(em32, tags, mask, tr32)
    (ll * w).sum().backward()
    return ll.detach(), em32.grad, tr32.grad


def _path_score64(em, trans, path, n):
    em, trans = em.double(), trans.double()
    s = em[0, path[0]]
    for t in range(1, n):
        s = s + trans[path[t - 1], path[t]] + em[t, path[t]]
    return float(s)


def _viterbi64(em, lens, trans):
    """Plain fp64 Viterbi, row by row. Returns (pred [B,L] with zeros past
    len, optimum [B])."""
    em, trans = em.double(), trans.double()
    B, L, T = em.shape
    pred = torch.zeros(B, L, dtype=torch.long)
    opt = torch.zeros(B, dtype=torch.float64)
    for b in range(B):
        n = int(lens[b])
        if n == 0:
            continue
        delta = em[b, 0]
        back = []
        for t in range(1, n):
            best, idx = (delta[:, None] + trans).max(dim=0)
            delta = best + em[b, t]
            back.append(idx)
        cur = int(delta.argmax())
        opt[b] = delta[cur]
        pred[b, n - 1] = cur
        for t in range(n - 2, -1, -1):
            cur = int(back[t][cur])
            pred[b, t] = cur
    return pred, opt


def _enumerate64(em, trans, n):
    """Every path of one row in fp64: (logZ, marginals [n,T], expected
    transition counts [T,T]). Shares nothing with _scan64."""
    em, trans = em.double(), trans.double()
    T = em.shape[1]
    paths = list(itertools.product(range(T), repeat=n))
    scores = torch.tensor([_path_score64(em, trans, p, n) for p in paths],
                          dtype=torch.float64)
    log_z = torch.logsumexp(scores, dim=0)
    prob = (scores - log_z).exp()
    marg = torch.zeros(n, T, dtype=torch.float64)
    pair = torch.zeros(T, T, dtype=torch.float64)
    for p, pr in zip(paths, prob):
        for t in range(n):
            marg[t, p[t]] += pr
        for t in range(1, n):
            pair[p[t - 1], p[t]] += pr
    return float(log_z), marg, pair


# ------------------------------------------------------------- tolerance
class _Report:
    """Prints every figure, collects the misses, asserts once at the end."""

    def __init__(self, case):
        self.case = case
        self.missed = []

    def check(self, name, got, want64, got32=None, M=None):
        want64 = want64.double()
        err_k = float((got.double().cpu() - want64).abs().max())
        err_32 = (0.0 if got32 is None
                  else float((got32.double() - want64).abs().max()))
        if M is None:
            M = float(want64.abs().max())
        floor = 16 * EPS32 * (1 + M)
        bound = 4 * err_32 + floor
        ratio = err_k / err_32 if err_32 > 0 else float("inf" if err_k else 0)
        print(f"crf_narrow {self.case} {name}: err_k={err_k:.3e} "
              f"err_32={err_32:.3e} ratio={ratio:.2f} floor={floor:.3e} "
              f"bound={bound:.3e}")
        if not err_k <= bound:       # also catches NaN
            self.missed.append(f"{name}: {err_k:.3e} > {bound:.3e}")

    def finish(self):
        assert not self.missed, f"{self.case}: " + "; ".join(self.missed)


def _kernel_loss(em, trans, mask, tags, w):
    em_g = em.cuda().requires_grad_()
    tr_g = trans.cuda().requires_grad_()
    ll = ops.crf_nll(em_g, tags.cuda(), mask.cuda(), tr_g)
    (ll * w.cuda()).sum().backward()
    return ll.detach(), em_g.grad, tr_g.grad


def _check_loss_case(B, L, T, scale):
    em, trans, lens, mask, tags, w = _inputs(B, L, T, scale)
    if B >= 3:
        assert {L, 1, 2} <= set(lens.tolist())
    ll64, logz64, dem64, dtr64 = _ref64(em, trans, lens, tags, w)
    ll32, dem32, dtr32 = _ref32(em, trans, mask, tags, w)
    ll, dem, dtr = _kernel_loss(em, trans, mask, tags, w)
    rep = _Report(f"({B},{L},{T}) scale={scale:g} {_route(L, T)}")
    rep.check("ll", ll, ll64, ll32, M=float(logz64.abs().max()))
    rep.check("emissions.grad", dem, dem64, dem32)
    rep.check("transitions.grad", dtr, dtr64, dtr32)
    past = (mask == 0)[:, :, None].expand(B, L, T)
    assert torch.count_nonzero(dem.cpu()[past]) == 0
    rep.finish()


def test_case_list_covers_every_route():
    """A change of the host rule in crf.hip must show up here."""
    for table, route in ((LOSS_CASES, _route), (VITERBI_CASES, _route_viterbi)):
        for (B, L, T), want in table.items():
            assert route(L, T) == want, (B, L, T)
    routes = list(LOSS_CASES.values())
    assert routes.count("x4") >= 2 and routes.count("x1") >= 2
    assert routes.count("wide") >= 1
    assert _route(159, 16) == "x4" and 1024 + 64 * 159 * 16 == LDS_BYTES
    assert _route(507, 20) == "x1" and 1600 + 16 * 507 * 20 == LDS_BYTES
    assert all(_route(L, T) == "x4" for (_, L, T) in SCALE8_CASES[:2])
    assert _route(45, 20) == "x1"


@pytest.mark.parametrize("B,L,T", list(LOSS_CASES))
def test_crf_narrow_nll_and_grads(B, L, T):
    _cuda()
    _check_loss_case(B, L, T, 1.0)


@pytest.mark.parametrize("B,L,T", SCALE8_CASES)
def test_crf_narrow_nll_and_grads_confident_logits(B, L, T):
    """scale = 8: alpha grows to about 1e4 at L = 158."""
    _cuda()
    _check_loss_case(B, L, T, 8.0)


@pytest.mark.parametrize("B,L,T,lens", [(3, 4, 3, [4, 1, 3]),
                                        (2, 5, 2, None)])
def test_crf_narrow_matches_enumeration(B, L, T, lens):
    """ll, token marginals (onehot(tags) - demis) and expected transition
    counts (gold counts - dtrans) against a sum over every path."""
    _cuda()
    em, trans, lens, mask, tags, _ = _inputs(B, L, T, lens=lens)
    ll, demis, dtrans = ops.get_ext().crf_fwd(
        em.cuda(), tags.to(torch.int32).cuda(), lens.to(torch.int32).cuda(),
        trans.cuda())
    ll, demis, dtrans = ll.cpu(), demis.cpu(), dtrans.cpu()
    rep = _Report(f"enumeration ({B},{L},{T})")
    for b in range(B):
        n = int(lens[b])
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
        assert torch.count_nonzero(demis[b, n:]) == 0
    rep.finish()


@pytest.mark.parametrize("B,L,T", list(VITERBI_CASES))
def test_crf_narrow_viterbi_matches_fp64(B, L, T):
    _cuda()
    em, trans, lens, mask, _, _ = _inputs(B, L, T)
    pred64, opt64 = _viterbi64(em, lens, trans)
    # ties would be an input problem: the fp32 reference must already agree
    assert torch.equal(ref.crf_decode(em, mask, trans), pred64)
    pred = ops.crf_viterbi(em.cuda(), mask.cuda(), trans.cuda()).cpu()
    for b in range(B):
        n = int(lens[b])
        path = pred[b].clamp(0, T - 1).tolist()
        got = _path_score64(em[b], trans, path, n)
        tol = 16 * EPS32 * (1 + abs(float(opt64[b])))
        assert abs(got - float(opt64[b])) <= tol, \
            f"row {b}: path score {got} is below the optimum {float(opt64[b])}"
    assert torch.equal(pred, pred64)
    assert torch.count_nonzero(pred * (1 - mask)) == 0


@pytest.mark.parametrize("T", [7, 18])
def test_crf_narrow_viterbi_nonfinite_stays_in_range(T):
    """Both narrow decoders clamp the last argmax and every backpointer
    read; T=7 is the four-per-wave kernel, T=18 the one-per-wave one."""
    _cuda()
    L = 30
    assert _route_viterbi(L, 7) == "x4" and _route_viterbi(L, 18) == "x1"
    em, trans, _, mask, _, _ = _inputs(1, L, T)
    assert int(mask.sum()) == L
    em[0, 3, 5] = float("nan")
    em[0, 7, :] = float("inf")
    em[0, 11, 2] = float("-inf")
    em[0, 20, :] = float("nan")
    pred = ops.crf_viterbi(em.cuda(), mask.cuda(), trans.cuda())
    assert int(pred.min()) >= 0 and int(pred.max()) < T


EMPTY_LENS = [5, 0, 12, 0, 1, 0]


@pytest.mark.parametrize("T", [7, 18])
def test_crf_narrow_empty_rows(T):
    """Contract of crf_fwd / crf_viterbi for lens[b] == 0, the same as
    crf_wide.hip's: ll, both gradients and the decode of that row are zero.
    ops.reference.crf_log_likelihood treats position 0 as always real, so it
    does not return 0 for an empty row: the empty rows are held to the
    contract, and only the non-empty rows to the references."""
    _cuda()
    B, L = 6, 12
    assert _route(L, 7) == "x4" and _route(L, 18) == "x1"
    em, trans, lens, mask, tags, w = _inputs(B, L, T, lens=EMPTY_LENS)
    empty = lens == 0
    ext = ops.get_ext()
    em_g, tr_g = em.cuda(), trans.cuda()
    tags_g = tags.to(torch.int32).cuda()
    lens_g = lens.to(torch.int32).cuda()
    # the caching allocator is likely to hand ll one of these blocks
    junk = [torch.full((B,), float("nan"), device="cuda") for _ in range(8)]
    del junk
    ll, demis, dtrans = ext.crf_fwd(em_g, tags_g, lens_g, tr_g)
    ll, demis, dtrans = ll.cpu(), demis.cpu(), dtrans.cpu()
    print(f"crf_narrow empty rows T={T}: ll={ll.tolist()}")
    assert torch.isfinite(ll).all()
    assert torch.isfinite(demis).all() and torch.isfinite(dtrans).all()
    assert torch.equal(ll[empty], torch.zeros(int(empty.sum())))
    assert torch.count_nonzero(demis[empty]) == 0
    assert torch.count_nonzero(dtrans[empty]) == 0

    pred = ext.crf_viterbi(em_g, lens_g, tr_g).cpu().long()
    pred64, _ = _viterbi64(em, lens, trans)
    assert torch.count_nonzero(pred[empty]) == 0
    assert torch.equal(pred, pred64)

    # through the op, with all-zero mask rows
    junk = [torch.full((B,), float("nan"), device="cuda") for _ in range(8)]
    del junk
    em2 = em_g.clone().requires_grad_()
    tr2 = tr_g.clone().requires_grad_()
    ll_op = ops.crf_nll(em2, tags.cuda(), mask.cuda(), tr2)
    nll = -ll_op.sum()
    assert torch.isfinite(nll)
    d_em, d_tr = torch.autograd.grad((ll_op * w.cuda()).sum(), (em2, tr2))
    assert torch.isfinite(d_em).all() and torch.isfinite(d_tr).all()
    assert torch.count_nonzero(d_em.cpu()[empty]) == 0
    assert torch.equal(ll_op.detach().cpu(), ll)

    # non-empty rows against the references
    ll64, logz64, dem64, dtr64 = _ref64(em, trans, lens, tags, w)
    keep = ~empty
    ll32, dem32, dtr32 = _ref32(em[keep], trans, mask[keep], tags[keep], w[keep])
    rep = _Report(f"empty rows T={T} {_route(L, T)}")
    rep.check("ll", ll[keep], ll64[keep], ll32,
              M=float(logz64[keep].abs().max()))
    rep.check("emissions.grad", d_em.cpu()[keep], dem64[keep], dem32)
    rep.check("transitions.grad", d_tr, dtr64, dtr32)
    rep.finish()
