"""Backward wiring of the linear layers (ops/functional.py) on CPU, with a
stub extension whose kernels are torch expressions and
CHINESENER_GEMM_NT=force: dW goes through gemm_tn(dy, x) and dx through
gemm_nn(dy, w) on the tensors as stored (no transposed copy), ineligible
shapes go to the library, and both give what F.linear's autograd gives."""
import pytest
import torch
import torch.nn.functional as F

from chinesener_amd.ops import functional as fn

BF = torch.bfloat16


class _Stub:
    """Torch stand-ins for the extension entries the two autograd nodes
    use; records the operands of every GEMM call."""

    def __init__(self):
        self.calls = []

    def gemm_nt(self, a, b, bias, fp32_out):
        self.calls.append(("gemm_nt", a, b))
        y = a.float() @ b.float().T
        if bias is not None:
            y = y + bias.float()
        return y if fp32_out else y.to(BF)

    def gemm_tn(self, a, b, split, fp32_out):
        assert a.is_contiguous() and b.is_contiguous() and split == 0
        self.calls.append(("gemm_tn", a, b))
        y = a.float().T @ b.float()
        return y if fp32_out else y.to(BF)

    def gemm_nn(self, a, b, fp32_out):
        assert a.is_contiguous() and b.is_contiguous()
        self.calls.append(("gemm_nn", a, b))
        y = a.float() @ b.float()
        return y if fp32_out else y.to(BF)

    def colsum(self, x):
        return x.float().sum(0).to(x.dtype)

    # LayerNorm(dropout(x) + res) and its backward, fp32 inside
    def dropout_add_ln_fwd(self, x, res, w, b, eps, keep, counter):
        g = torch.Generator().manual_seed(5)
        mask = (torch.rand(x.shape, generator=g) < keep).to(torch.uint8)
        s = x.float() * mask / keep + res.float()
        mean = s.mean(-1)
        rstd = (s.var(-1, unbiased=False) + eps).rsqrt()
        y = (s - mean[:, None]) * rstd[:, None] * w.float() + b.float()
        return y.to(BF), s.to(BF), mask, mean, rstd

    def dropout_add_ln_bwd(self, dy, s, w, mean, rstd, mask, keep, has_bias):
        xhat = (s.float() - mean[:, None]) * rstd[:, None]
        g = dy.float() * w.float()
        dsum = rstd[:, None] * (g - g.mean(-1, keepdim=True)
                                - xhat * (g * xhat).mean(-1, keepdim=True))
        dx_drop = (dsum * mask / keep).to(BF)
        self.dx_drop = dx_drop
        dbias = dx_drop.float().sum(0).to(BF) if has_bias else None
        return (dsum.to(BF), dx_drop, (dy.float() * xhat).sum(0).to(BF),
                dy.float().sum(0).to(BF), dbias)


@pytest.fixture
def stub(monkeypatch):
    s = _Stub()
    monkeypatch.setattr(fn, "get_ext", lambda: s)
    monkeypatch.setenv("CHINESENER_GEMM_NT", "force")
    return s


def _ints(shape, seed, lo=-2, hi=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi, shape, generator=g).to(BF)


def _linear_grads(x, w, dy):
    """F.linear autograd in fp32 on the same bf16 values, rounded once."""
    xf = x.float().requires_grad_()
    wf = w.float().requires_grad_()
    dx, dw = torch.autograd.grad(F.linear(xf, wf), (xf, wf), dy.float())
    return dx, dw


def _gemm_calls(stub, name):
    return [c for c in stub.calls if c[0] == name]


def test_linear_fn_eligible_uses_new_kernels_in_place(stub):
    # 3-D input, M = 2*64 = 128, N = 256, K = 128; integer operands make
    # every fp32 sum exact, so the comparison is bitwise
    x = _ints((2, 64, 128), 1).requires_grad_()
    w = _ints((256, 128), 2).requires_grad_()
    b = _ints((256,), 3).requires_grad_()
    dy = _ints((2, 64, 256), 4)
    y = fn._LinearFn.apply(x, w, b)
    y.backward(dy)
    dx_ref, dw_ref = _linear_grads(x.detach(), w.detach(), dy)
    assert torch.equal(x.grad, dx_ref.to(BF))
    assert torch.equal(w.grad, dw_ref.to(BF))
    assert torch.equal(b.grad, dy.reshape(-1, 256).float().sum(0).to(BF))

    (tn,), (nn,) = _gemm_calls(stub, "gemm_tn"), _gemm_calls(stub, "gemm_nn")
    # dy, x and w themselves: same storage, stored layout, no copies
    assert tuple(tn[1].shape) == (128, 256) and tuple(tn[2].shape) == (128, 128)
    assert tn[1].data_ptr() == dy.data_ptr()
    assert tn[2].data_ptr() == x.data_ptr()
    assert tuple(nn[1].shape) == (128, 256) and tuple(nn[2].shape) == (256, 128)
    assert nn[1].data_ptr() == dy.data_ptr()
    assert nn[2].data_ptr() == w.data_ptr()
    # the only gemm_nt call is the forward product
    assert len(_gemm_calls(stub, "gemm_nt")) == 1


def test_linear_fn_ineligible_goes_to_library(stub):
    # K = 96 is no multiple of 128 (and M = 96 none of 64): library path
    x = _ints((96, 96), 5).requires_grad_()
    w = _ints((128, 96), 6).requires_grad_()
    dy = _ints((96, 128), 7)
    y = fn._LinearFn.apply(x, w, None)
    y.backward(dy)
    assert not stub.calls
    dx_ref, dw_ref = _linear_grads(x.detach(), w.detach(), dy)
    assert torch.equal(x.grad, dx_ref.to(BF))
    assert torch.equal(w.grad, dw_ref.to(BF))


def test_wgrad_eligibility_is_n128_k128_m64(stub):
    # M = 64 (not 128): wgrad eligible, dgrad not
    x = _ints((64, 128), 8).requires_grad_()
    w = _ints((128, 128), 9).requires_grad_()
    dy = _ints((64, 128), 10)
    dyf = dy.contiguous()
    dw = fn._linear_wgrad(dyf, x.detach(), w.detach())
    dx = fn._linear_dgrad(dyf, x.detach(), w.detach())
    assert [c[0] for c in stub.calls] == ["gemm_tn"]
    dx_ref, dw_ref = _linear_grads(x.detach(), w.detach(), dy)
    assert torch.equal(dw, dw_ref.to(BF)) and torch.equal(dx, dx_ref.to(BF))


def test_mode_off_never_calls_the_extension_gemms(stub, monkeypatch):
    monkeypatch.setenv("CHINESENER_GEMM_NT", "off")
    x = _ints((128, 128), 11)
    w = _ints((128, 128), 12)
    dy = _ints((128, 128), 13)
    fn._linear_wgrad(dy, x, w)
    fn._linear_dgrad(dy, x, w)
    assert not stub.calls


@pytest.mark.parametrize("M,N,K", [(128, 128, 256), (96, 128, 96)])
def test_linear_dropout_add_ln_fn(stub, M, N, K):
    eligible = M % 128 == 0 and K % 128 == 0
    g = torch.Generator().manual_seed(20)
    x = _ints((M, K), 21).requires_grad_()
    w = _ints((N, K), 22).requires_grad_()
    b = _ints((N,), 23).requires_grad_()
    res = torch.randn(M, N, generator=g).to(BF).requires_grad_()
    ln_w = torch.randn(N, generator=g).to(BF).requires_grad_()
    ln_b = torch.randn(N, generator=g).to(BF).requires_grad_()
    dy = torch.randn(M, N, generator=g).to(BF)
    y = fn._LinearDropoutAddLNFn.apply(x, w, b, res, ln_w, ln_b, 1e-12, 0.9)
    y.backward(dy)

    # the linear's upstream gradient is the LN backward's dx_drop; given
    # that, dx and dw are F.linear's. Both sides sum the same fp32
    # products in another order (relative 2^-24 per term) and round to
    # bf16 once (half an ulp = 2^-9 each), so they agree to one bf16 ulp.
    dx_drop = stub.dx_drop
    dx_ref, dw_ref = _linear_grads(x.detach(), w.detach(), dx_drop)
    torch.testing.assert_close(x.grad.float(), dx_ref, rtol=2 ** -7,
                               atol=1e-4)
    torch.testing.assert_close(w.grad.float(), dw_ref, rtol=2 ** -7,
                               atol=1e-4)
    assert torch.equal(b.grad, dx_drop.float().sum(0).to(BF))

    if eligible:
        (tn,), (nn,) = (_gemm_calls(stub, "gemm_tn"),
                        _gemm_calls(stub, "gemm_nn"))
        assert tn[1].data_ptr() == dx_drop.data_ptr()
        assert tn[2].data_ptr() == x.data_ptr()
        assert nn[1].data_ptr() == dx_drop.data_ptr()
        assert nn[2].data_ptr() == w.data_ptr()
        assert tuple(nn[2].shape) == (N, K) and tuple(tn[2].shape) == (M, K)
    else:
        assert not _gemm_calls(stub, "gemm_tn")
        assert not _gemm_calls(stub, "gemm_nn")
