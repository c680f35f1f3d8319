"""Backward wiring of the fused embedding gather (ops/functional.py) on
CPU, with a stub extension whose embed3_fwd / embed3_bwd are torch
expressions and hip_enabled patched: the node hands the kernel dy and the
ids as stored (no float copies), returns three gradients of the table
dtype and None for the ids, sends ineligible shapes and
CHINESENER_EMBED3_BWD=off to the torch code, and both routes give what
F.embedding's autograd gives on integer data."""
import pytest
import torch
import torch.nn.functional as F

from chinesener_amd.ops import functional as fn

BF = torch.bfloat16


class _Stub:
    limits = (16, 8, 32768, 1 << 32)   # chunk, segment cap, rows, V * rows

    def __init__(self):
        self.calls = []

    def embed3_bwd_limits(self):
        return list(self.limits)

    def embed3_fwd(self, w, p, t, ids, segs):
        L = ids.shape[1]
        return (w.float()[ids] + p.float()[:L] + t.float()[segs]).to(BF)

    def embed3_bwd(self, dy, ids, segs, V, P, S):
        self.calls.append((dy, ids, segs, V, P, S))
        B, L, H = dy.shape
        d = dy.reshape(-1, H).double()
        dw = torch.zeros(V, H, dtype=torch.float64).index_add_(
            0, ids.reshape(-1), d)
        dw[0] = 0
        dp = torch.zeros(P, H, dtype=torch.float64)
        dp[:L] = dy.double().sum(0)
        dt = torch.zeros(S, H, dtype=torch.float64).index_add_(
            0, segs.reshape(-1), d)
        return [dw.to(BF), dp.to(BF), dt.to(BF)]


@pytest.fixture
def stub(monkeypatch):
    s = _Stub()
    monkeypatch.setattr(fn, "get_ext", lambda: s)
    monkeypatch.setattr(fn, "hip_enabled", lambda t: True)
    monkeypatch.delenv("CHINESENER_EMBED3_BWD", raising=False)
    monkeypatch.delenv("CHINESENER_NO_EMBED3", raising=False)
    return s


def _ints(shape, seed, lo=-2, hi=4):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi, shape, generator=g).to(BF)


def _setup(V, P, S, H, B, L, seed):
    g = torch.Generator().manual_seed(seed)
    w = _ints((V, H), seed + 1).requires_grad_()
    p = _ints((P, H), seed + 2).requires_grad_()
    t = _ints((S, H), seed + 3).requires_grad_()
    ids = torch.randint(0, V, (B, L), generator=g)
    segs = torch.randint(0, S, (B, L), generator=g)
    dy = _ints((B, L, H), seed + 4)
    return w, p, t, ids, segs, dy


def _autograd_ref(w, p, t, ids, segs, dy):
    """F.embedding autograd in fp32 on the same values, rounded once."""
    w2, p2, t2 = (x.detach().float().requires_grad_() for x in (w, p, t))
    L = ids.shape[1]
    ref = (F.embedding(ids, w2, padding_idx=0) + p2[torch.arange(L)]
           + F.embedding(segs, t2))
    return [g.to(BF) for g in
            torch.autograd.grad(ref, (w2, p2, t2), dy.float())]


def _run(w, p, t, ids, segs, dy):
    out = fn.embed3(w, p, t, ids, segs)
    assert "Embed3" in type(out.grad_fn).__name__
    return torch.autograd.grad(out, (w, p, t), dy)


class _Ctx:
    """What _Embed3Fn.forward leaves for backward."""

    def __init__(self, w, p, t, ids, segs):
        self.saved_tensors = (ids, segs)
        self.shapes = (w.shape, p.shape, t.shape)


def test_eligible_shape_hands_the_kernel_the_stored_tensors(stub):
    w, p, t, ids, segs, dy = _setup(50, 12, 2, 16, 3, 7, seed=1)
    dw, dp, dt = _run(w, p, t, ids, segs, dy)
    (call,) = stub.calls
    raw = fn._Embed3Fn.backward(_Ctx(w, p, t, ids, segs), dy)
    assert len(raw) == 5 and raw[3] is None and raw[4] is None
    k_dy, k_ids, k_segs, V, P, S = call
    assert (V, P, S) == (50, 12, 2)
    # dy and the ids themselves: same storage, stored dtype, no copies
    assert k_dy.data_ptr() == dy.data_ptr() and k_dy.dtype == BF
    assert tuple(k_dy.shape) == (3, 7, 16)
    assert k_ids.data_ptr() == ids.data_ptr() and k_ids.dtype == torch.int64
    assert k_segs.data_ptr() == segs.data_ptr() and k_segs.dtype == torch.int64
    for got, table, ref in zip((dw, dp, dt), (w, p, t),
                               _autograd_ref(w, p, t, ids, segs, dy)):
        assert got.dtype == table.dtype and got.shape == table.shape
        assert torch.equal(got, ref)


def test_non_contiguous_dy_is_made_contiguous(stub):
    w, p, t, ids, segs, dy = _setup(50, 12, 2, 16, 3, 7, seed=2)
    dy_t = dy.transpose(0, 1).contiguous().transpose(0, 1)
    assert not dy_t.is_contiguous()
    grads = _run(w, p, t, ids, segs, dy_t)
    (call,) = stub.calls
    assert call[0].is_contiguous() and call[0].dtype == BF
    for got, ref in zip(grads, _autograd_ref(w, p, t, ids, segs, dy)):
        assert torch.equal(got, ref)


@pytest.mark.parametrize("why", ["S-over-cap", "H-not-8", "off", "rows",
                                 "key"])
def test_ineligible_goes_to_the_torch_code(stub, monkeypatch, why):
    V, P, S, H, B, L = 50, 12, 2, 16, 3, 7
    if why == "S-over-cap":
        S = stub.limits[1] + 1
    if why == "H-not-8":
        H = 12
    if why == "off":
        monkeypatch.setenv("CHINESENER_EMBED3_BWD", "off")
    if why == "rows":
        stub.limits = (16, 8, B * L - 1, 1 << 32)
    if why == "key":
        stub.limits = (16, 8, 32768, V * B * L - 1)
    w, p, t, ids, segs, dy = _setup(V, P, S, H, B, L, seed=3)
    if why == "H-not-8":
        # embed3() itself keeps such a width off the node; the node's own
        # check is what is under test
        out = fn._Embed3Fn.apply(w, p, t, ids, segs)
        grads = torch.autograd.grad(out, (w, p, t), dy)
    else:
        grads = _run(w, p, t, ids, segs, dy)
    assert not stub.calls
    for got, table, ref in zip(grads, (w, p, t),
                               _autograd_ref(w, p, t, ids, segs, dy)):
        assert got.dtype == table.dtype and got.shape == table.shape
        assert torch.equal(got, ref)


def test_limits_cover_the_long_flagship_batch(stub):
    # 64 x 512 rows of the 21128-row vocabulary must take the kernel
    # (the stub states the limits the extension is built with;
    # tests/test_gpu_embed_bwd.py holds the build to them)
    dy = torch.empty(64, 512, 8, dtype=BF)
    assert fn._embed3_bwd_eligible(dy, (21128, 8), (2, 8))
