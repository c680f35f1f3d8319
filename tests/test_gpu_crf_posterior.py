"""CRF path-posterior kernel (csrc/crf_posterior.hip) against the fp64
reference ops.reference.crf_path_posterior on the same inputs, and against
the existing CRF kernels.

Bound: atol=1e-3, rtol=0 on span_a and span_b separately, the absolute
figure the CRF tests already use for ll and demis. No relative term: at
L=512 the arrays reach +-1.4e3 and it would hide anything. The same
recurrences in plain fp32 without running offsets miss the bound at L=512
(0.9-1.4e-3), so it requires the offset scheme to work. Each case prints
its measured maxima before it asserts."""
import pytest
import torch

from chinesener_amd import ops
from chinesener_amd.ops import reference as ref

from test_gpu_kernels import _cuda

pytestmark = pytest.mark.gpu

SHAPES = [(5, 1, 1), (7, 2, 3), (7, 40, 10), (6, 33, 20), (5, 40, 21),
          (6, 37, 32), (4, 35, 33), (4, 37, 64), (3, 512, 20), (3, 512, 64)]


def _lens_for(B, L):
    """Rows of 1, 2, L and lengths in between; [512, 300, 1] at L=512."""
    if L == 512:
        return [512, 300, 1][:B]
    return [min(max(x, 1), L) for x in (1, 2, L, L // 2, 3, L - 1, 7)][:B]


def _inputs(B, L, T, seed):
    g = torch.Generator().manual_seed(seed)
    em = torch.randn(B, L, T, generator=g).cuda()
    trans = torch.randn(T, T, generator=g).cuda()
    lens = torch.tensor(_lens_for(B, L), device="cuda")
    assert lens.numel() == B
    mask = (torch.arange(L, device="cuda")[None, :] < lens[:, None]).long()
    rand_path = torch.randint(0, T, (B, L), generator=g).cuda()
    return em, trans, lens, mask, rand_path


def _check(em, trans, mask, path, what):
    a, b = ops.crf_path_posterior(em, mask, trans, path)
    ra, rb = ref.crf_path_posterior(em, mask, trans, path)
    assert a.dtype == torch.float64 and b.dtype == torch.float64
    assert a.shape == path.shape and b.shape == path.shape
    assert not a.requires_grad and not b.requires_grad
    err_a = (a - ra).abs().max().item()
    err_b = (b - rb).abs().max().item()
    print(f"crf_path_posterior {tuple(em.shape)} {what} path: "
          f"max|span_a err| {err_a:.3e}  max|span_b err| {err_b:.3e}")
    torch.testing.assert_close(a, ra, atol=1e-3, rtol=0)
    torch.testing.assert_close(b, rb, atol=1e-3, rtol=0)
    past = mask == 0
    assert torch.count_nonzero(a[past]) == 0
    assert torch.count_nonzero(b[past]) == 0


@pytest.mark.parametrize("B,L,T", SHAPES)
def test_posterior_matches_fp64_reference(B, L, T):
    _cuda()
    em, trans, lens, mask, rand_path = _inputs(B, L, T, seed=900 + L + T)
    _check(em, trans, mask, ops.crf_viterbi(em, mask, trans), "viterbi")
    _check(em, trans, mask, rand_path, "random")


@pytest.mark.parametrize("B,L,T", [(6, 33, 20), (4, 37, 64)])
def test_posterior_agrees_with_crf_fwd(B, L, T):
    """Sequence probability against crf_nll and token marginals against the
    emission gradient of crf_fwd (demis = onehot(tag) - marginal)."""
    _cuda()
    em, trans, lens, mask, path = _inputs(B, L, T, seed=40 + T)
    path = path * mask
    a, b = ops.crf_path_posterior(em, mask, trans, path)
    rows = torch.arange(B, device="cuda")
    seq = a[:, 0] + b[rows, lens - 1]
    ll = ops.crf_nll(em, path, mask, trans)
    torch.testing.assert_close(seq, ll.double(), atol=1e-3, rtol=0)

    _, demis, _ = ops.get_ext().crf_fwd(
        em, path.to(torch.int32), lens.to(torch.int32), trans)
    marg = 1.0 - demis.gather(2, path[:, :, None]).squeeze(2).double()
    valid = mask.bool()
    torch.testing.assert_close(torch.exp(a + b)[valid], marg[valid],
                               atol=1e-3, rtol=0)


def test_posterior_empty_row_is_zero():
    _cuda()
    B, L, T = 3, 20, 24
    g = torch.Generator().manual_seed(3)
    em = torch.randn(B, L, T, generator=g).cuda()
    trans = torch.randn(T, T, generator=g).cuda()
    lens = torch.tensor([5, 0, 20], dtype=torch.int32, device="cuda")
    path = torch.randint(0, T, (B, L), generator=g).to(torch.int32).cuda()
    a, b = ops.get_ext().crf_path_posterior(em, lens, trans, path)
    assert torch.count_nonzero(a[1]) == 0 and torch.count_nonzero(b[1]) == 0
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    mask = (torch.arange(L, device="cuda")[None, :] < lens[:, None]).long()
    ra, rb = ref.crf_path_posterior(em, mask, trans, path)
    torch.testing.assert_close(a, ra, atol=1e-3, rtol=0)
    torch.testing.assert_close(b, rb, atol=1e-3, rtol=0)


def test_posterior_limits_raise():
    """Outside 1 <= T <= 64, 1 <= L <= 512 the op refuses before launching."""
    _cuda()
    ext = ops.get_ext()
    lens = torch.ones(1, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="64"):
        ext.crf_path_posterior(
            torch.zeros(1, 8, 65, device="cuda"), lens,
            torch.zeros(65, 65, device="cuda"),
            torch.zeros(1, 8, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="512"):
        ext.crf_path_posterior(
            torch.zeros(1, 513, 8, device="cuda"), lens,
            torch.zeros(8, 8, device="cuda"),
            torch.zeros(1, 513, dtype=torch.int32, device="cuda"))
    a, b = ext.crf_path_posterior(
        torch.zeros(0, 8, 8, device="cuda"), lens[:0],
        torch.zeros(8, 8, device="cuda"),
        torch.zeros(0, 8, dtype=torch.int32, device="cuda"))
    assert a.shape == (0, 8) and b.shape == (0, 8)


def test_decode_scored_pred_is_viterbi():
    _cuda()
    em, trans, lens, mask, _ = _inputs(6, 33, 20, seed=11)
    pred, a, b = ops.crf_decode_scored(em, mask, trans)
    assert torch.equal(pred, ops.crf_viterbi(em, mask, trans))
    a2, b2 = ops.crf_path_posterior(em, mask, trans, pred)
    assert torch.equal(a, a2) and torch.equal(b, b2)


def test_decode_scored_graph_capture():
    """crf_decode_scored captures into a hipGraph (one chain on the capture
    stream); replays on fresh inputs are bit-equal to the eager call."""
    _cuda()
    B, L, T = 3, 64, 41
    sets = [_inputs(B, L, T, seed=s) for s in (21, 22, 23)]
    em_s, trans_s, _, mask_s, _ = (x.clone() for x in sets[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            ops.crf_decode_scored(em_s, mask_s, trans_s)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_s = ops.crf_decode_scored(em_s, mask_s, trans_s)
    for em, trans, _, mask, _ in sets[1:]:
        em_s.copy_(em)
        trans_s.copy_(trans)
        mask_s.copy_(mask)
        graph.replay()
        torch.cuda.synchronize()
        eager = ops.crf_decode_scored(em, mask, trans)
        for got, want in zip(out_s, eager):
            assert torch.equal(got, want)
