"""N-best CRF decode kernel (csrc/crf_nbest.hip) through ops.crf_nbest,
against the fp64 reference ops.reference.crf_nbest (run with k+1 ranks, so
the gap below the last returned rank is known) on the same inputs.

Bound: tol = 1e-3 absolute, no relative term, the project's CRF figure.
Scores are compared through the fp64 score recomputed from the returned
path, which does not depend on which of two near-tied paths the fp32 scan
preferred; paths are compared exactly wherever the reference separates a
rank from both neighbours by more than tol. Each case prints its measured
maxima before it asserts."""
import functools
import math

import pytest
import torch

from chinesener_amd import ops
from chinesener_amd.ops import reference as ref

from test_gpu_kernels import _cuda
from test_gpu_crf_posterior import SHAPES, _inputs, _lens_for

pytestmark = pytest.mark.gpu

TOL = 1e-3
KS = [1, 3, 4, 8]
NINF = float("-inf")


@functools.lru_cache(maxsize=None)
def _case(B, L, T):
    """Inputs of one shape (on the GPU) and their fp64 CPU copies + logZ."""
    em, trans, lens, mask, _ = _inputs(B, L, T, seed=900 + L + T)
    em64, tr64 = em.double().cpu(), trans.double().cpu()
    alpha = em64[:, 0]
    for t in range(1, L):
        nxt = torch.logsumexp(alpha[:, :, None] + tr64[None], dim=1) + em64[:, t]
        alpha = torch.where((t < lens.cpu())[:, None], nxt, alpha)
    return em, trans, lens, mask, em64, tr64, torch.logsumexp(alpha, dim=1)


@functools.lru_cache(maxsize=None)
def _reference(B, L, T, k):
    _, _, _, mask, em64, tr64, _ = _case(B, L, T)
    return ref.crf_nbest(em64, mask.cpu(), tr64, k + 1)


def _path_score64(em64, tr64, path, n):
    """fp64 score of path[:n]."""
    p = path[:n]
    s = em64[torch.arange(n), p].sum()
    if n > 1:
        s = s + tr64[p[:-1], p[1:]].sum()
    return s.item()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("B,L,T", SHAPES)
def test_nbest_matches_fp64_reference(B, L, T, k):
    _cuda()
    em, trans, lens, mask, em64, tr64, logz = _case(B, L, T)
    rpaths, rscores = _reference(B, L, T, k)
    paths, scores, logp = ops.crf_nbest(em, mask, trans, k)
    vit = ops.crf_viterbi(em, mask, trans).cpu()
    torch.cuda.synchronize()
    # 1. shapes, dtypes, padding, absent ranks
    assert paths.shape == (B, k, L) and paths.dtype == torch.long
    assert scores.shape == (B, k) and scores.dtype == torch.float32
    assert logp.shape == (B, k) and logp.dtype == torch.float64
    paths, scores, logp = paths.cpu(), scores.cpu(), logp.cpu()
    lens_l = lens.cpu().tolist()
    assert ((paths >= 0) & (paths < T)).all()
    err_self = err_ref = err_logp = 0.0
    compared = qualified = total = 0
    for b, n in enumerate(lens_l):
        assert torch.count_nonzero(paths[b, :, n:]) == 0
        npaths = min(k, T ** n)
        for r in range(npaths, k):
            assert scores[b, r].item() == NINF and logp[b, r].item() == NINF
            assert torch.count_nonzero(paths[b, r]) == 0
        assert torch.isfinite(scores[b, :npaths]).all()
        assert torch.isfinite(logp[b, :npaths]).all()
        seen = set()
        for r in range(npaths):
            total += 1
            # 2. the fp64 score of the returned path
            s64 = _path_score64(em64[b], tr64, paths[b, r], n)
            err_self = max(err_self, abs(s64 - scores[b, r].item()))
            err_ref = max(err_ref, abs(s64 - rscores[b, r].item()))
            # 3. distinct paths, non-increasing scores
            key = tuple(paths[b, r, :n].tolist())
            assert key not in seen, (b, r)
            seen.add(key)
            if r > 0:
                assert scores[b, r] <= scores[b, r - 1]
            # 4. exact path where the reference ranks it unambiguously
            gap_dn = (rscores[b, r] - rscores[b, r + 1]).item()
            gap_up = (rscores[b, r - 1] - rscores[b, r]).item() if r else math.inf
            if gap_dn > TOL and gap_up > TOL:
                qualified += 1
                assert torch.equal(paths[b, r], rpaths[b, r]), (b, r)
                compared += 1
            # 5. rank 0 is the Viterbi path when it is unambiguous
            if r == 0 and gap_dn > TOL:
                assert torch.equal(paths[b, 0], vit[b]), b
            # 6. logp = score - logZ
            err_logp = max(err_logp,
                           abs(logp[b, r].item() - (s64 - logz[b].item())))
        assert torch.exp(logp[b]).sum().item() <= 1.0 + TOL
    share = compared / max(total, 1)
    print(f"crf_nbest {(B, L, T)} k={k}: max|score - fp64(path)| "
          f"{err_self:.3e}  max|fp64(path) - ref| {err_ref:.3e}  "
          f"max|logp err| {err_logp:.3e}  paths compared {compared}/{total} "
          f"({100 * share:.0f}%)")
    assert err_self <= TOL
    assert err_ref <= TOL
    assert err_logp <= TOL
    if L <= 40:
        assert share >= 0.8


def test_nbest_routes():
    """The shapes above reach both backpointer routes: LDS for the serving
    shapes, the global workspace where one wave's table outgrows LDS."""
    _cuda()
    route = ops.get_ext().crf_nbest_route
    for k in KS:
        assert route(40, 10, k)[0] == 0
        assert route(150, 24, k)[0] == 0
        assert route(512, 20, k)[0] == 0
    assert route(512, 64, 8)[0] == 1
    assert route(512, 64, 4)[0] == 1
    assert route(512, 64, 1)[0] == 0
    assert route(37, 64, 8)[0] == 0
    # 4, 2, 1 waves per block as one wave's table grows
    assert [route(L, 32, 8)[1] for L in (40, 256, 512)] == [4, 2, 1]
    for L, T, k in [(40, 10, 4), (512, 20, 8), (512, 64, 8), (512, 32, 8)]:
        assert route(L, T, k)[2] <= 160 * 1024


def _tie_inputs(B, L, T, seed):
    g = torch.Generator().manual_seed(seed)
    em = torch.randint(-4, 5, (B, L, T), generator=g).float() / 4
    trans = torch.randint(-4, 5, (T, T), generator=g).float() / 4
    lens = torch.tensor(_lens_for(B, L))
    mask = (torch.arange(L)[None, :] < lens[:, None]).long()
    return em, trans, mask


@pytest.mark.parametrize("k", [4, 8])
@pytest.mark.parametrize("B,L,T", [(6, 12, 5), (4, 9, 33)])
def test_nbest_exact_ties_follow_the_reference(B, L, T, k):
    """Multiples of 0.25 make every sum exact in fp32, so ties are real
    ties; the kernel then has to break them exactly as the reference does.
    (No comparison with crf_viterbi: its cross-lane argmax does not pick
    the lowest tag under ties.)"""
    _cuda()
    em, trans, mask = _tie_inputs(B, L, T, seed=70 + T + k)
    rpaths, rscores = ref.crf_nbest(em, mask, trans, k)
    ties = sum(int((rscores[b, 1:] == rscores[b, :-1]).sum()) for b in range(B))
    assert ties > 0  # the inputs do tie
    paths, scores, _ = ops.crf_nbest(em.cuda(), mask.cuda(), trans.cuda(), k)
    assert torch.equal(scores.cpu(), rscores)
    assert torch.equal(paths.cpu(), rpaths)


def test_nbest_empty_row_and_batch_remainder():
    """An empty row among real ones; B = 7 is no multiple of 4, 2 waves."""
    _cuda()
    B, L, T, k = 7, 20, 24, 4
    g = torch.Generator().manual_seed(5)
    em = torch.randn(B, L, T, generator=g)
    trans = torch.randn(T, T, generator=g)
    lens = torch.tensor([5, 0, 20, 1, 0, 13, 2])
    mask = (torch.arange(L)[None, :] < lens[:, None]).long()
    paths, scores, logp = ops.crf_nbest(em.cuda(), mask.cuda(), trans.cuda(), k)
    paths, scores, logp = paths.cpu(), scores.cpu(), logp.cpu()
    rpaths, rscores = ref.crf_nbest(em.double(), mask, trans.double(), k)
    for b in (1, 4):
        assert (scores[b] == NINF).all() and (logp[b] == NINF).all()
        assert torch.count_nonzero(paths[b]) == 0
    assert torch.equal(torch.isfinite(scores), torch.isfinite(rscores))
    fin = torch.isfinite(rscores)
    torch.testing.assert_close(scores[fin].double(), rscores[fin],
                               atol=TOL, rtol=0)
    for b, n in enumerate(lens.tolist()):
        for r in range(k):
            if fin[b, r]:
                s64 = _path_score64(em[b].double(), trans.double(),
                                    paths[b, r], n)
                assert abs(s64 - rscores[b, r].item()) <= TOL
            assert torch.count_nonzero(paths[b, r, n:]) == 0


def test_nbest_limits_raise():
    _cuda()
    ext = ops.get_ext()
    lens = torch.ones(1, dtype=torch.int32, device="cuda")
    em, tr = torch.zeros(1, 8, 8, device="cuda"), torch.zeros(8, 8, device="cuda")
    for k in (0, 9):
        with pytest.raises(RuntimeError, match="k"):
            ext.crf_nbest(em, lens, tr, k)
        with pytest.raises(ValueError):
            ops.crf_nbest(em, torch.ones(1, 8, device="cuda"), tr, k)
    with pytest.raises(RuntimeError, match="64"):
        ext.crf_nbest(torch.zeros(1, 8, 65, device="cuda"), lens,
                      torch.zeros(65, 65, device="cuda"), 4)
    with pytest.raises(RuntimeError, match="512"):
        ext.crf_nbest(torch.zeros(1, 513, 8, device="cuda"), lens, tr, 4)
    paths, scores = ext.crf_nbest(em[:0], lens[:0], tr, 4)
    assert paths.shape == (0, 4, 8) and scores.shape == (0, 4)


def test_nbest_graph_capture():
    """ops.crf_nbest (kernel + path posterior) captures into a hipGraph;
    replays on inputs changed in place are bit-equal to the eager call."""
    _cuda()
    B, L, T, k = 4, 32, 10, 4
    sets = [_inputs(B, L, T, seed=s) for s in (31, 32, 33)]
    em_s, trans_s, _, mask_s, _ = (x.clone() for x in sets[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            ops.crf_nbest(em_s, mask_s, trans_s, k)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_s = ops.crf_nbest(em_s, mask_s, trans_s, k)
    for em, trans, _, mask, _ in sets[1:]:
        em_s.copy_(em)
        trans_s.copy_(trans)
        mask_s.copy_(mask)
        graph.replay()
        torch.cuda.synchronize()
        eager = ops.crf_nbest(em, mask, trans, k)
        for got, want in zip(out_s, eager):
            assert torch.equal(got, want)


def test_token_nbest_text_mask_matches_cpu():
    """ops.token_nbest with a mask that is no prefix (an MRC text_mask): the
    GPU result covers the masked positions and agrees with the CPU one."""
    _cuda()
    g = torch.Generator().manual_seed(15)
    B, L, T, k = 4, 24, 3, 4
    logits = torch.randn(B, L, T, generator=g) * 2
    pos = torch.arange(L)[None, :]
    start, end = torch.tensor([6, 9, 0, 23]), torch.tensor([24, 13, 5, 24])
    mask = ((pos >= start[:, None]) & (pos < end[:, None])).long()
    paths, scores, logp = ops.token_nbest(logits.cuda(), mask.cuda(), k)
    paths, scores, logp = paths.cpu(), scores.cpu(), logp.cpu()
    rp, rs, rl = ops.token_nbest(logits, mask, k)
    assert torch.equal(paths[:, 0], logits.argmax(-1) * mask)
    assert torch.count_nonzero(paths[(mask == 0)[:, None, :].expand_as(paths)]) == 0
    assert torch.equal(torch.isfinite(scores), torch.isfinite(rs))
    fin = torch.isfinite(rs)
    assert fin.sum() == 4 + 4 + 4 + 3      # the last row has T = 3 paths
    torch.testing.assert_close(scores[fin], rs[fin], atol=TOL, rtol=0)
    torch.testing.assert_close(logp[fin], rl[fin], atol=TOL, rtol=0)
    # every returned path scores what its rank says, in fp64
    lsm = torch.log_softmax(logits.double(), -1)
    own = (lsm.gather(2, paths.transpose(1, 2)).transpose(1, 2)
           * mask[:, None, :]).sum(2)
    torch.testing.assert_close(own[fin], rs[fin].double(), atol=TOL, rtol=0)
