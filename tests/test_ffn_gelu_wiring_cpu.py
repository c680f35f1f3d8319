"""Wiring of ops.ffn_gelu_dropout_add_layernorm (ops/functional.py) on CPU,
with a stub extension whose kernels are torch expressions: the fused node
computes what the composed ops' autograd computes, hands the extension its
operands as stored, bumps the dropout RNG once, and every ineligible
condition lands on the composition."""
import pytest
import torch

from chinesener_amd.ops import functional as fn

BF = torch.bfloat16


def _gelu(u):
    return 0.5 * u * (1 + torch.tanh(0.7978845608 * (u + 0.044715 * u ** 3)))


def _dgelu(u):
    t = torch.tanh(0.7978845608 * (u + 0.044715 * u ** 3))
    da = 0.7978845608 * (1 + 3 * 0.044715 * u * u)
    return 0.5 * (1 + t) + 0.5 * u * (1 - t * t) * da


class _Stub:
    """Torch stand-ins for the extension entries the FFN node and the
    composed nodes use; records every call with its operands."""

    def __init__(self):
        self.calls = []

    def _names(self):
        return [c[0] for c in self.calls]

    def gemm_nt(self, a, b, bias, fp32_out):
        self.calls.append(("gemm_nt", a, b))
        y = a.float() @ b.float().T
        if bias is not None:
            y = y + bias.float()
        return y if fp32_out else y.to(BF)

    def gemm_tn(self, a, b, split, fp32_out):
        self.calls.append(("gemm_tn", a, b))
        return (a.float().T @ b.float()).to(BF)

    def gemm_nn(self, a, b, fp32_out):
        self.calls.append(("gemm_nn", a, b))
        return (a.float() @ b.float()).to(BF)

    def colsum(self, x):
        return x.float().sum(0).to(x.dtype)

    def bias_gelu_fwd(self, x, bias):
        self.calls.append(("bias_gelu_fwd", x, bias))
        return _gelu(x.float() + bias.float()).to(BF)

    def bias_gelu_bwd(self, dy, x, bias):
        self.calls.append(("bias_gelu_bwd", dy, x, bias))
        dx = (dy.float() * _dgelu(x.float() + bias.float())).to(BF)
        return [dx, dx.float().sum(0).to(bias.dtype)]

    def gemm_nt_bias_gelu(self, a, b, bias, save_pre):
        self.calls.append(("gemm_nt_bias_gelu", a, b, bias, save_pre))
        u = (a.float() @ b.float().T).to(BF)
        g = _gelu(u.float() + bias.float()).to(BF)
        self.u = u
        return [u if save_pre else None, g]

    def gemm_nn_dgelu(self, a, b, u, bias):
        self.calls.append(("gemm_nn_dgelu", a, b, u, bias))
        dh = (a.float() @ b.float()).to(BF)
        du = (dh.float() * _dgelu(u.float() + bias.float())).to(BF)
        return [du, du.float().sum(0).to(bias.dtype)]

    def dropout_add_ln_fwd(self, x, res, w, b, eps, keep, counter):
        self.calls.append(("dropout_add_ln_fwd", counter))
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
    monkeypatch.setattr(fn, "hip_enabled", lambda t: True)
    monkeypatch.setattr(fn, "_GEMM_NT_CHOICE", {})
    monkeypatch.setattr(fn, "_GEMM_NT_CALLS", {})
    monkeypatch.setenv("CHINESENER_GEMM_NT", "force")
    monkeypatch.setenv("CHINESENER_FUSED_GELU", "force")
    monkeypatch.delenv("CHINESENER_NO_FUSED_DROPOUT", raising=False)
    return s


M, H, FF = 128, 128, 256


def _operands(b1_dtype=BF, m=M):
    g = torch.Generator().manual_seed(31)

    def r(*shape, s=1.0):
        return (torch.randn(*shape, generator=g) * s).to(BF)

    t = {"x": r(2, m // 2, H), "w1": r(FF, H, s=0.1),
         "b1": r(FF).to(b1_dtype), "w2": r(H, FF, s=0.1), "b2": r(H),
         "ln_w": r(H), "ln_b": r(H)}
    for v in t.values():
        v.requires_grad_()
    t["dy"] = r(2, m // 2, H)
    return t


def _call(t, p=0.1, training=True):
    return fn.ffn_gelu_dropout_add_layernorm(
        t["x"], t["w1"], t["b1"], t["w2"], t["b2"], t["x"], t["ln_w"],
        t["ln_b"], 1e-12, p, training)


_PARAMS = ("x", "w1", "b1", "w2", "b2", "ln_w", "ln_b")


def _grads(t):
    return {k: t[k].grad for k in _PARAMS}


@pytest.mark.parametrize("b1_dtype", [BF, torch.float32])
def test_node_equals_composed_autograd(stub, monkeypatch, b1_dtype):
    t = _operands(b1_dtype)
    y = _call(t)
    y.backward(t["dy"])
    names = stub._names()
    assert names.count("gemm_nt_bias_gelu") == 1
    assert names.count("gemm_nn_dgelu") == 1
    assert "bias_gelu_fwd" not in names and "bias_gelu_bwd" not in names

    monkeypatch.setenv("CHINESENER_FUSED_GELU", "off")
    stub.calls.clear()
    c = _operands(b1_dtype)
    yc = _call(c)
    yc.backward(c["dy"])
    names = stub._names()
    assert "gemm_nt_bias_gelu" not in names and "gemm_nn_dgelu" not in names
    assert names.count("bias_gelu_fwd") == 1
    assert names.count("bias_gelu_bwd") == 1

    assert torch.equal(y, yc)
    got, want = _grads(t), _grads(c)
    for k in _PARAMS:
        assert got[k] is not None and got[k].dtype == want[k].dtype, k
        assert got[k].shape == want[k].shape, k
        assert torch.equal(got[k], want[k]), k


def test_operands_reach_the_extension_as_stored(stub):
    t = _operands()
    y = _call(t)
    y.backward(t["dy"])
    up = [c for c in stub.calls if c[0] == "gemm_nt_bias_gelu"][0]
    assert tuple(up[1].shape) == (M, H) and up[4] is True
    assert up[1].data_ptr() == t["x"].data_ptr()
    assert up[2].data_ptr() == t["w1"].data_ptr()
    assert up[3].data_ptr() == t["b1"].data_ptr()
    dn = [c for c in stub.calls if c[0] == "gemm_nn_dgelu"][0]
    assert dn[1].data_ptr() == stub.dx_drop.data_ptr()
    assert dn[2].data_ptr() == t["w2"].data_ptr()
    assert tuple(dn[2].shape) == (H, FF)
    assert dn[3].data_ptr() == stub.u.data_ptr()
    assert dn[4].data_ptr() == t["b1"].data_ptr()
    # FFN-down forward, two wgrads, one dgrad (FFN-up's); no other GEMM
    names = stub._names()
    assert names.count("gemm_nt") == 1 and names.count("gemm_tn") == 2
    assert names.count("gemm_nn") == 1


def test_one_rng_bump(stub):
    t = _operands()
    _call(t).backward(t["dy"])
    bumps = [c for c in stub.calls if c[0] == "dropout_add_ln_fwd"]
    assert len(bumps) == 1
    assert bumps[0][1] is fn._rng_counter_for(t["x"].device)


def test_no_grad_takes_the_forward_without_u(stub, monkeypatch):
    seen = []

    def tail(f, *a):
        seen.append(f)
        return f

    monkeypatch.setattr(fn, "linear_dropout_add_layernorm", tail)
    t = _operands()
    with torch.no_grad():
        f = _call(t, training=False)
    up = [c for c in stub.calls if c[0] == "gemm_nt_bias_gelu"]
    assert len(up) == 1 and up[0][4] is False
    assert tuple(f.shape) == (2, M // 2, FF) and seen[0] is f


def _composition_spy(monkeypatch):
    seen = []
    monkeypatch.setattr(fn, "linear",
                        lambda x, w, b=None: seen.append("linear") or x)
    monkeypatch.setattr(fn, "bias_gelu",
                        lambda x, b: seen.append("bias_gelu") or x)
    monkeypatch.setattr(fn, "linear_dropout_add_layernorm",
                        lambda f, *a: seen.append("tail") or f)
    return seen


@pytest.mark.parametrize("why", [
    "cpu", "fp32", "autocast", "rows", "fp16_bias", "p0", "eval_with_grad",
    "off", "no_fused_dropout"])
def test_fallbacks_take_the_composition(stub, monkeypatch, why):
    seen = _composition_spy(monkeypatch)
    t = _operands(m=96) if why == "rows" else _operands()
    p, training = 0.1, True
    if why == "cpu":
        monkeypatch.setattr(fn, "hip_enabled", lambda x: False)
    elif why == "fp32":
        t = {k: v.detach().float() for k, v in t.items()}
    elif why == "fp16_bias":
        t["b1"] = t["b1"].detach().to(torch.float16)
    elif why == "p0":
        p = 0.0
    elif why == "eval_with_grad":
        training = False
    elif why == "off":
        monkeypatch.setenv("CHINESENER_FUSED_GELU", "off")
    elif why == "no_fused_dropout":
        monkeypatch.setenv("CHINESENER_NO_FUSED_DROPOUT", "1")
    elif why == "autocast":
        # the GPU autocast state the op asks for; it cannot be entered
        # for real without a GPU
        monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    _call(t, p, training)
    assert seen == ["linear", "bias_gelu", "tail"]
    assert not stub.calls


def test_auto_waits_for_the_inner_key_and_decides_per_half(stub, monkeypatch):
    monkeypatch.setenv("CHINESENER_GEMM_NT", "auto")
    monkeypatch.setenv("CHINESENER_FUSED_GELU", "auto")
    raced = []

    def pick2(key, fused, pair, min_recur=None):
        if not key[0].startswith("ffn_"):
            return False                     # the node's own GEMMs: library
        raced.append(key)
        return key[0] == "ffn_up_gelu"       # forward wins, backward loses

    monkeypatch.setattr(fn, "_pick2", pick2)
    monkeypatch.setattr(fn, "_pick_gemm_nt", lambda x2, w, b: False)
    t = _operands()
    _call(t).backward(t["dy"])
    assert not raced                          # inner keys undecided
    names = stub._names()
    assert "gemm_nt_bias_gelu" not in names and "gemm_nn_dgelu" not in names
    assert names.count("bias_gelu_fwd") == 1
    assert names.count("bias_gelu_bwd") == 1

    fn._GEMM_NT_CHOICE[(M, FF, H, False)] = False
    fn._GEMM_NT_CHOICE[("dx", M, H, FF)] = False
    stub.calls.clear()
    t = _operands()
    _call(t).backward(t["dy"])
    assert ("ffn_up_gelu", M, FF, H) in raced
    assert ("ffn_dn_dgelu", M, H, FF) in raced
    names = stub._names()
    assert names.count("gemm_nt_bias_gelu") == 1      # fused forward
    assert "gemm_nn_dgelu" not in names               # unfused backward
    assert names.count("bias_gelu_bwd") == 1
    assert "bias_gelu_fwd" not in names
