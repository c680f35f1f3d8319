"""Wide-tagset CRF kernels (csrc/crf_wide.hip): 21..64 tags, and <= 20
tags at lengths whose alpha the narrow kernels cannot hold in LDS. The
reference is ops.reference on the same device in fp32.

(3, 512, 20) is a wide case for the loss only: its int8 backpointers fit in
LDS, so crf_viterbi decodes it with the narrow one-per-wave
crf_viterbi_kernel of crf.hip. The other narrow cases are in
test_gpu_crf_narrow.py."""
import pytest
import torch

from chinesener_amd import ops
from chinesener_amd.ops import reference as ref

from conftest import make_tiny_batch, make_tiny_params
from test_gpu_kernels import _cuda

pytestmark = pytest.mark.gpu


def _lens_for(B, L):
    """Fixed lengths: rows of 1, 2 and L; [512, 300] plus a 1 at L=512."""
    if L == 512:
        return [512, 300, 1][:B]
    return [1, 2, L, L // 2, 3, L - 1, 7][:B]


def _inputs(B, L, T, seed):
    g = torch.Generator().manual_seed(seed)
    em = torch.randn(B, L, T, generator=g).cuda()
    trans = torch.randn(T, T, generator=g).cuda()
    lens = torch.tensor(_lens_for(B, L), device="cuda")
    assert lens.numel() == B
    mask = (torch.arange(L, device="cuda")[None, :] < lens[:, None]).long()
    tags = torch.randint(0, T, (B, L), generator=g).cuda() * mask
    w = torch.randn(B, generator=g).cuda()
    return em, trans, lens, mask, tags, w


@pytest.mark.parametrize("B,L,T", [(5, 40, 21), (6, 33, 24), (3, 64, 41),
                                   (4, 37, 64), (3, 512, 20), (2, 512, 64)])
def test_crf_wide_nll_and_grads(B, L, T):
    _cuda()
    em, trans, lens, mask, tags, w = _inputs(B, L, T, seed=100 + T)
    em32 = em.clone().requires_grad_()
    trans32 = trans.clone().requires_grad_()
    ll_ref = ref.crf_log_likelihood(em32, tags, mask, trans32)
    em2 = em.clone().requires_grad_()
    tr2 = trans.clone().requires_grad_()
    ll = ops.crf_nll(em2, tags, mask, tr2)
    torch.testing.assert_close(ll, ll_ref, atol=1e-3, rtol=1e-4)

    (ll_ref * w).sum().backward()
    (ll * w).sum().backward()
    torch.testing.assert_close(em2.grad, em32.grad, atol=1e-3, rtol=1e-3)
    torch.testing.assert_close(tr2.grad, trans32.grad, atol=1e-2, rtol=1e-3)
    past = (mask == 0)[:, :, None].expand_as(em2.grad)
    assert torch.count_nonzero(em2.grad[past]) == 0


def test_crf_wide_nll_three_rows_at_512x64():
    """(2, 512, 64) above has no room for the length-1 row; this adds it,
    with B=3 at one wave per block."""
    _cuda()
    B, L, T = 3, 512, 64
    em, trans, lens, mask, tags, w = _inputs(B, L, T, seed=7)
    assert lens.tolist() == [512, 300, 1]
    em32 = em.clone().requires_grad_()
    trans32 = trans.clone().requires_grad_()
    ll_ref = ref.crf_log_likelihood(em32, tags, mask, trans32)
    em2 = em.clone().requires_grad_()
    tr2 = trans.clone().requires_grad_()
    ll = ops.crf_nll(em2, tags, mask, tr2)
    torch.testing.assert_close(ll, ll_ref, atol=1e-3, rtol=1e-4)
    (ll_ref * w).sum().backward()
    (ll * w).sum().backward()
    torch.testing.assert_close(em2.grad, em32.grad, atol=1e-3, rtol=1e-3)
    torch.testing.assert_close(tr2.grad, trans32.grad, atol=1e-2, rtol=1e-3)


def test_crf_wide_empty_row_is_zero():
    """lens[b] == 0 leaves ll, both grads and the decode of that row zero."""
    _cuda()
    B, L, T = 3, 20, 24
    g = torch.Generator().manual_seed(3)
    em = torch.randn(B, L, T, generator=g).cuda()
    trans = torch.randn(T, T, generator=g).cuda()
    lens = torch.tensor([5, 0, 20], dtype=torch.int32, device="cuda")
    tags = torch.zeros(B, L, dtype=torch.int32, device="cuda")
    ll, demis, dtrans = ops.get_ext().crf_fwd(em, tags, lens, trans)
    assert ll[1] == 0 and torch.isfinite(ll).all()
    assert torch.count_nonzero(demis[1]) == 0
    assert torch.count_nonzero(dtrans[1]) == 0
    pred = ops.get_ext().crf_viterbi(em, lens, trans)
    assert torch.count_nonzero(pred[1]) == 0


# (3, 512, 20) runs crf.hip's crf_viterbi_kernel, not a wide kernel: the
# decode leaves crf.hip only for T > 20
@pytest.mark.parametrize("B,L,T", [(7, 50, 24), (5, 45, 64), (2, 512, 64),
                                   (3, 512, 20)])
def test_crf_wide_viterbi_matches_reference(B, L, T):
    _cuda()
    em, trans, lens, mask, _, _ = _inputs(B, L, T, seed=200 + T)
    if L == 512:        # lengths include 1 and L
        lens = torch.tensor(([512, 1, 300])[:B], device="cuda")
        mask = (torch.arange(L, device="cuda")[None, :] < lens[:, None]).long()
    assert 1 in lens.tolist() and L in lens.tolist()
    pred = ops.crf_viterbi(em, mask, trans)
    pred_ref = ref.crf_decode(em, mask, trans)
    assert torch.equal(pred.cpu(), pred_ref.cpu())
    assert torch.count_nonzero(pred * (1 - mask)) == 0


def test_crf_wide_viterbi_nonfinite_stays_in_range():
    _cuda()
    L, T = 30, 24
    g = torch.Generator().manual_seed(9)
    em = torch.randn(1, L, T, generator=g)
    em[0, 3, 5] = float("nan")
    em[0, 7, :] = float("inf")
    em[0, 11, 2] = float("-inf")
    em[0, 20, :] = float("nan")
    em = em.cuda()
    trans = torch.randn(T, T, generator=g).cuda()
    mask = torch.ones(1, L, dtype=torch.long, device="cuda")
    pred = ops.crf_viterbi(em, mask, trans)
    assert int(pred.min()) >= 0 and int(pred.max()) < T


def test_crf_wide_limits_raise():
    """Host-side range checks: nothing is launched."""
    _cuda()
    ext = ops.get_ext()

    def args(L, T):
        em = torch.zeros(1, L, T, device="cuda")
        return (em, torch.zeros(1, L, dtype=torch.int32, device="cuda"),
                torch.ones(1, dtype=torch.int32, device="cuda"),
                torch.zeros(T, T, device="cuda"))

    em, tags, lens, trans = args(8, 65)
    with pytest.raises(RuntimeError, match="64"):
        ext.crf_fwd(em, tags, lens, trans)
    with pytest.raises(RuntimeError, match="64"):
        ext.crf_viterbi(em, lens, trans)
    em, tags, lens, trans = args(513, 24)
    with pytest.raises(RuntimeError, match="512"):
        ext.crf_fwd(em, tags, lens, trans)
    with pytest.raises(RuntimeError, match="512"):
        ext.crf_viterbi(em, lens, trans)


def test_crf_wide_graph_capture_replay():
    """The graphed training step records these calls: no host sync, no
    allocation outside the torch allocator. The kernels use no atomics, so
    a replay equals the eager call bit for bit."""
    _cuda()
    B, L, T = 3, 64, 41
    sets = [_inputs(B, L, T, seed=300 + i) for i in range(3)]
    _, _, _, mask, tags, w = sets[0]

    def step(em, trans):
        ll = ops.crf_nll(em, tags, mask, trans)
        d_em, d_tr = torch.autograd.grad((ll * w).sum(), (em, trans))
        return ll, d_em, d_tr, ops.crf_viterbi(em.detach(), mask, trans.detach())

    s_em = sets[0][0].clone().requires_grad_()
    s_tr = sets[0][1].clone().requires_grad_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(s_em, s_tr)
    torch.cuda.current_stream().wait_stream(side)

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s_out = step(s_em, s_tr)
    for em, trans, *_ in sets[1:]:
        with torch.no_grad():
            s_em.copy_(em)
            s_tr.copy_(trans)
        graph.replay()
        e_out = step(em.clone().requires_grad_(), trans.clone().requires_grad_())
        for s, e in zip(s_out, e_out):
            assert torch.equal(s, e)


def test_bilstm_crf_trains_and_decodes_at_24_labels():
    _cuda()
    torch.manual_seed(0)
    from chinesener_amd.models import build_model
    model = build_model("bilstm_crf",
                        make_tiny_params("bilstm_crf", label_size=24)).to("cuda")
    batch = {k: (v.cuda() if isinstance(v, torch.Tensor) else v)
             for k, v in make_tiny_batch("bilstm_crf", label_size=24).items()}
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        out = model(batch)
        assert torch.isfinite(out.loss)
        out.loss.backward()
        opt.step()
    with torch.no_grad():
        pred = model.eval()(batch, compute_pred=True).pred_ids
    assert pred.shape == batch["token_ids"].shape
    assert int(pred.min()) >= 0 and int(pred.max()) < 24
