"""Backward wiring of the two CRF losses (ops/functional.py) on CPU. With a
stub extension whose crf_fwd / crf_partial_fwd / crf_grad_scale are torch
expressions and hip_enabled patched, both autograd functions hand
crf_grad_scale the saved tensors and dll, return its two results in the
gradient slots of emissions and transitions, and give what autograd gives
on ops.reference. Without the patch (the CPU path) crf_nll and
crf_partial_nll are ops.reference unchanged, and the chain rule itself is
the torch expression."""
import pytest
import torch

from chinesener_amd.ops import functional as fn
from chinesener_amd.ops import reference as ref


def _rowwise(ll_fn, emissions, lens, transitions):
    """(ll [B], d ll_b / d emissions [B,L,T], d ll_b / d transitions
    [B,T,T]) by autograd, one row at a time."""
    B, L, T = emissions.shape
    ll, demis, dtrans = [], [], []
    for b in range(B):
        em = emissions[b:b + 1].clone().requires_grad_()
        tr = transitions.clone().requires_grad_()
        mask = (torch.arange(L)[None, :] < lens[b]).long()
        with torch.enable_grad():   # called inside Function.forward
            val = ll_fn(em, b, mask, tr)
            g_em, g_tr = torch.autograd.grad(val.sum(), (em, tr))
        ll.append(val.detach()[0])
        demis.append(g_em[0])
        dtrans.append(g_tr)
    return [torch.stack(ll), torch.stack(demis), torch.stack(dtrans)]


class _Stub:
    def __init__(self):
        self.scale_calls = []

    def crf_fwd(self, emissions, tags, lens, transitions):
        return _rowwise(
            lambda em, b, mask, tr: ref.crf_log_likelihood(
                em, tags[b:b + 1].long(), mask, tr),
            emissions, lens, transitions)

    def crf_partial_fwd(self, emissions, allowed, lens, transitions):
        return _rowwise(
            lambda em, b, mask, tr: ref.crf_partial_log_likelihood(
                em, allowed[b:b + 1], mask, tr),
            emissions, lens, transitions)

    def crf_grad_scale(self, demis, dtrans, dll):
        self.scale_calls.append((demis, dtrans, dll))
        return [demis * dll[:, None, None],
                (dtrans * dll[:, None, None]).sum(0)]


@pytest.fixture
def stub(monkeypatch):
    s = _Stub()
    monkeypatch.setattr(fn, "get_ext", lambda: s)
    monkeypatch.setattr(fn, "hip_enabled", lambda t: True)
    return s


def _setup(B=4, L=6, T=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    lens = torch.tensor([L, 1, 3, L - 1][:B])
    mask = (torch.arange(L)[None, :] < lens[:, None]).long()
    em = torch.randn(B, L, T, generator=g)
    trans = torch.randn(T, T, generator=g)
    tags = torch.randint(0, T, (B, L), generator=g) * mask
    w = torch.randn(B, generator=g)
    w[1] = 0.0
    w[2] = -abs(w[2])
    return em, trans, mask, tags, w


def _reference_grads(ll_fn, em, trans, w):
    em2 = em.clone().requires_grad_()
    tr2 = trans.clone().requires_grad_()
    ll = ll_fn(em2, tr2)
    return (ll.detach(),) + torch.autograd.grad((ll * w).sum(), (em2, tr2))


def _allowed(tags, mask, T):
    # every other position known, the rest open
    known = mask.bool() & (torch.arange(tags.shape[1])[None, :] % 2 == 0)
    return torch.where(known, torch.ones_like(tags) << tags,
                       torch.zeros_like(tags)).to(torch.int64)


@pytest.mark.parametrize("loss", ["full", "partial"])
def test_hip_path_goes_through_crf_grad_scale(stub, loss):
    em, trans, mask, tags, w = _setup()
    T = em.shape[2]
    em_g, tr_g = em.clone().requires_grad_(), trans.clone().requires_grad_()
    if loss == "full":
        ll = fn.crf_nll(em_g, tags, mask, tr_g)
        want = _reference_grads(
            lambda e, t: ref.crf_log_likelihood(e, tags, mask, t),
            em, trans, w)
    else:
        allowed = _allowed(tags, mask, T)
        ll = fn.crf_partial_nll(em_g, allowed, mask, tr_g)
        want = _reference_grads(
            lambda e, t: ref.crf_partial_log_likelihood(e, allowed, mask, t),
            em, trans, w)
    assert "Crf" in type(ll.grad_fn).__name__
    d_em, d_tr = torch.autograd.grad((ll * w).sum(), (em_g, tr_g))
    (call,) = stub.scale_calls
    demis, dtrans, dll = call
    assert tuple(demis.shape) == tuple(em.shape)
    assert tuple(dtrans.shape) == (em.shape[0], T, T)
    assert dll.dtype == torch.float32
    assert torch.equal(dll, w)
    assert d_em.shape == em.shape and d_tr.shape == trans.shape
    torch.testing.assert_close(ll.detach(), want[0], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(d_em, want[1], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(d_tr, want[2], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("loss", ["full", "partial"])
def test_backward_returns_four_slots_and_keeps_the_saved_tensors(stub, loss):
    em, trans, mask, tags, w = _setup(seed=1)
    node = fn._CrfNllFn if loss == "full" else fn._CrfPartialFn

    class Ctx:
        saved_tensors = (torch.randn(4, 6, 3), torch.randn(4, 3, 3))

    before = [t.clone() for t in Ctx.saved_tensors]
    out = node.backward(Ctx, w)
    assert len(out) == 4 and out[1] is None and out[2] is None
    assert torch.equal(out[0], before[0] * w[:, None, None])
    assert torch.equal(out[3], (before[1] * w[:, None, None]).sum(0))
    for kept, was in zip(Ctx.saved_tensors, before):
        assert torch.equal(kept, was)


def test_cpu_path_is_the_reference_and_the_torch_chain_rule():
    em, trans, mask, tags, w = _setup(seed=2)
    T = em.shape[2]
    allowed = _allowed(tags, mask, T)
    for got_fn, ref_fn in (
            (lambda e, t: fn.crf_nll(e, tags, mask, t),
             lambda e, t: ref.crf_log_likelihood(e, tags, mask, t)),
            (lambda e, t: fn.crf_partial_nll(e, allowed, mask, t),
             lambda e, t: ref.crf_partial_log_likelihood(e, allowed, mask,
                                                         t))):
        got = _reference_grads(got_fn, em, trans, w)
        want = _reference_grads(ref_fn, em, trans, w)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    demis, dtrans = torch.randn(4, 6, 3), torch.randn(4, 3, 3)
    d_em, d_tr = fn._crf_grad_scale(demis, dtrans, w)
    assert torch.equal(d_em, demis * w[:, None, None])
    assert torch.equal(d_tr, (dtrans * w[:, None, None]).sum(0))
