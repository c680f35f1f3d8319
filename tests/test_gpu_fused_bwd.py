"""Fused backward glue: one-pass post-LN backward (dsum, dx_drop, dw, db,
dbias), bias_gelu backward with its bias grad, bf16 biases read in place,
and the linear_dropout_add_layernorm wiring.

Bias-grad rule used throughout: the kernel sums the stored bf16 values in
fp32 in its own fixed order and rounds once to the output dtype, so against
ref = values.float().sum(0) it may differ per column by the fp32 reordering
bound N * 2^-24 * sum|values| plus one ulp (of the output dtype) of ref.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from chinesener_amd import ops
from chinesener_amd.ops import functional as fn
from chinesener_amd.ops import reference as ref

KEEP = 0.8
EPS = 1e-12


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.ext_available(), "HIP extension must be built for GPU tests"


def _ulp(refv, dtype):
    """Spacing of `dtype` at |refv| (fp32 tensor), elementwise."""
    mant = 7 if dtype == torch.bfloat16 else 23
    a = refv.abs().clamp_min(torch.finfo(torch.float32).tiny)
    return torch.exp2(torch.floor(torch.log2(a)) - mant)


def _assert_colsum(got, values, label):
    """got [C] vs the column sum of values [N, C] under the module rule."""
    v = values.float()
    refv = v.sum(0)
    bound = v.shape[0] * 2.0 ** -24 * v.abs().sum(0) + _ulp(refv, got.dtype)
    err = (got.float() - refv).abs()
    worst = (err - bound).max().item()
    print(f"{label}: max err {err.max().item():.4g}, "
          f"max (err - bound) {worst:.4g}")
    assert (err <= bound).all(), (label, worst)


_LN_SHAPES = [(1, 8), (33, 40), (70, 520), (257, 768), (64, 1024)]
_ln_cache = {}


def _ln_case(N, H):
    """Inputs, kernel outputs of two identical calls and the fp32 torch
    reference for one shape; computed once, shared, never modified."""
    key = (N, H)
    if key in _ln_cache:
        return _ln_cache[key]
    g = torch.Generator(device="cuda").manual_seed(1000 + N * 7 + H)

    def rnd(*shape, dtype=torch.float32):
        return torch.randn(*shape, device="cuda", generator=g).to(dtype)

    x = rnd(N, H, dtype=torch.bfloat16)
    res = rnd(N, H, dtype=torch.bfloat16)
    w = rnd(H) * 0.5 + 1.0
    b = rnd(H)
    dy = rnd(N, H, dtype=torch.bfloat16)
    ext = ops.get_ext()
    ctr = torch.tensor([12345 + N], dtype=torch.int64, device="cuda")
    y, s, mask, mean, rstd = ext.dropout_add_ln_fwd(x, res, w, b, EPS, KEEP,
                                                    ctr)
    out1 = ext.dropout_add_ln_bwd(dy, s, w, mean, rstd, mask, KEEP, True)
    out2 = ext.dropout_add_ln_bwd(dy, s, w, mean, rstd, mask, KEEP, True)
    nodb = ext.dropout_add_ln_bwd(dy, s, w, mean, rstd, mask, KEEP, False)
    plain1 = ext.layernorm_bwd(dy, s, w, mean, rstd)
    plain2 = ext.layernorm_bwd(dy, s, w, mean, rstd)
    s32 = s.float().requires_grad_()
    w32 = w.clone().requires_grad_()
    b32 = b.clone().requires_grad_()
    F.layer_norm(s32, (H,), w32, b32, EPS).backward(dy.float())
    torch.cuda.synchronize()
    case = dict(s=s, mask=mask, w=w, dy=dy, out1=out1, out2=out2, nodb=nodb,
                plain1=plain1, plain2=plain2,
                ref=(s32.grad, w32.grad, b32.grad))
    _ln_cache[key] = case
    return case


@pytest.mark.parametrize("N,H", _LN_SHAPES)
def test_post_ln_bwd_matches_fp32_reference(N, H):
    _cuda()
    c = _ln_case(N, H)
    dsum, dx_drop, dw, db, dbias = c["out1"]
    dx_ref, dw_ref, db_ref = c["ref"]
    assert dsum.dtype == torch.bfloat16 and dsum.shape == (N, H)
    assert dw.dtype == c["w"].dtype and db.dtype == c["w"].dtype
    assert dbias.dtype == torch.bfloat16 and dbias.shape == (H,)
    torch.testing.assert_close(dsum.float(), dx_ref, atol=0.1, rtol=0.1)
    torch.testing.assert_close(dw, dw_ref, atol=0.5, rtol=0.05)
    torch.testing.assert_close(db, db_ref, atol=0.5, rtol=0.05)


@pytest.mark.parametrize("N,H", _LN_SHAPES)
def test_post_ln_bwd_dx_drop_bit_exact_and_dbias(N, H):
    _cuda()
    c = _ln_case(N, H)
    dsum, dx_drop, dw, db, dbias = c["out1"]
    want = (dsum.float() * c["mask"] * (1 / KEEP)).bfloat16()
    assert torch.equal(dx_drop, want)
    _assert_colsum(dbias, dx_drop, f"ln dbias N={N} H={H}")


@pytest.mark.parametrize("N,H", _LN_SHAPES)
def test_post_ln_bwd_reproducible(N, H):
    """No atomics: identical inputs give bit-identical reductions, and
    dropping the bias grad changes nothing else."""
    _cuda()
    c = _ln_case(N, H)
    for a, b in zip(c["out1"], c["out2"]):
        assert torch.equal(a, b)
    assert c["nodb"][4] is None
    # the two instantiations may contract fp32 operations differently
    # (a few 2^-23 relative steps on O(10) terms) ahead of one bf16
    # rounding (ulp <= 2^-7 relative)
    for a, b in zip(c["out1"][:4], c["nodb"][:4]):
        torch.testing.assert_close(a.float(), b.float(), atol=1e-5, rtol=2e-2)
    assert torch.equal(c["nodb"][1],
                       (c["nodb"][0].float() * c["mask"]
                        * (1 / KEEP)).bfloat16())


@pytest.mark.parametrize("N,H", _LN_SHAPES)
def test_layernorm_bwd_plain_path(N, H):
    """The no-dropout instantiation behind ext.layernorm_bwd: same
    return contract {dx, dw, db}, dw/db in the weight dtype."""
    _cuda()
    c = _ln_case(N, H)
    assert len(c["plain1"]) == 3
    dx, dw, db = c["plain1"]
    dx_ref, dw_ref, db_ref = c["ref"]
    assert dx.dtype == torch.bfloat16 and dx.shape == (N, H)
    assert dw.dtype == c["w"].dtype and dw.shape == (H,)
    assert db.dtype == c["w"].dtype and db.shape == (H,)
    torch.testing.assert_close(dx.float(), dx_ref, atol=0.1, rtol=0.1)
    torch.testing.assert_close(dw, dw_ref, atol=0.5, rtol=0.05)
    torch.testing.assert_close(db, db_ref, atol=0.5, rtol=0.05)
    for a, b in zip(c["plain1"], c["plain2"]):
        assert torch.equal(a, b)


def test_layernorm_bwd_bf16_weight_dtype():
    """bf16 LN params: the finisher writes dw/db as bf16 directly."""
    _cuda()
    c = _ln_case(33, 40)
    ext = ops.get_ext()
    s, dy = c["s"], c["dy"]
    mean = s.float().mean(1)
    rstd = torch.rsqrt(s.float().var(1, unbiased=False) + 1e-5)
    dx, dw, db = ext.layernorm_bwd(dy, s, c["w"].bfloat16(), mean, rstd)
    dx32, dw32, db32 = ext.layernorm_bwd(dy, s, c["w"].bfloat16().float(),
                                         mean, rstd)
    assert dw.dtype == torch.bfloat16 and db.dtype == torch.bfloat16
    assert torch.equal(dx, dx32)
    assert torch.equal(dw, dw32.bfloat16()) and torch.equal(db, db32.bfloat16())


# ------------------------------------------------------------ bias gelu
@pytest.mark.parametrize("bias_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("M,Fd", [(1, 8), (37, 24), (300, 264), (2049, 3072)])
def test_bias_gelu_bwd_fused_dbias(M, Fd, bias_dtype):
    _cuda()
    g = torch.Generator(device="cuda").manual_seed(2000 + M + Fd)
    x = torch.randn(M, Fd, device="cuda", generator=g).bfloat16()
    dy = torch.randn(M, Fd, device="cuda", generator=g).bfloat16()
    bias = torch.randn(Fd, device="cuda", generator=g).to(bias_dtype)
    ext = ops.get_ext()
    dx, dbias = ext.bias_gelu_bwd(dy, x, bias)
    dx2, dbias2 = ext.bias_gelu_bwd(dy, x, bias)
    assert dx.dtype == torch.bfloat16 and dbias.dtype == bias_dtype
    assert dbias.shape == (Fd,)
    x32 = x.float().requires_grad_()
    ref.bias_gelu(x32, bias.float()).backward(dy.float())
    torch.testing.assert_close(dx.float(), x32.grad, atol=0.05, rtol=0.05)
    _assert_colsum(dbias, dx, f"gelu dbias M={M} F={Fd} {bias_dtype}")
    assert torch.equal(dx, dx2) and torch.equal(dbias, dbias2)


# ------------------------------------------------------ bf16 bias in place
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (256, 384, 768)])
def test_gemm_nt_bf16_bias_bit_equal(M, N, K):
    _cuda()
    g = torch.Generator(device="cuda").manual_seed(3000 + N)
    a = torch.randn(M, K, device="cuda", generator=g).bfloat16()
    b = torch.randn(N, K, device="cuda", generator=g).bfloat16()
    bias = torch.randn(N, device="cuda", generator=g).bfloat16()
    ext = ops.get_ext()
    y16 = ext.gemm_nt(a, b, bias, False)
    y32 = ext.gemm_nt(a, b, bias.float(), False)
    assert torch.equal(y16, y32)
    want = a.float() @ b.float().T + bias.float()
    torch.testing.assert_close(y16.float(), want, atol=0.5, rtol=2e-2)


@pytest.mark.parametrize("M,Fd", [(37, 24), (300, 264)])
def test_bias_gelu_fwd_bf16_bias_bit_equal(M, Fd):
    _cuda()
    g = torch.Generator(device="cuda").manual_seed(4000 + Fd)
    x = torch.randn(M, Fd, device="cuda", generator=g).bfloat16()
    bias = torch.randn(Fd, device="cuda", generator=g).bfloat16()
    ext = ops.get_ext()
    y16 = ext.bias_gelu_fwd(x, bias)
    y32 = ext.bias_gelu_fwd(x, bias.float())
    assert torch.equal(y16, y32)
    torch.testing.assert_close(y16.float(),
                               ref.bias_gelu(x.float(), bias.float()),
                               atol=0.03, rtol=0.05)


# --------------------------------------------------------------- wiring
@pytest.mark.parametrize("shape,n_out,mode", [((4, 64, 128), 128, "force"),
                                              ((4, 10, 64), 96, "auto")])
def test_linear_dropout_add_layernorm_matches_composition(shape, n_out, mode,
                                                          monkeypatch):
    """Fused node vs dropout_add_layernorm(linear(.)) from the same RNG
    counter value: same outputs bit for bit, same grads, one bump each.
    'force' pins the in-tree GEMM so both forms take the same path."""
    _cuda()
    monkeypatch.setenv("CHINESENER_GEMM_NT", mode)
    monkeypatch.delenv("CHINESENER_NO_FUSED_DROPOUT", raising=False)
    torch.manual_seed(50)
    K = shape[-1]
    dev, bf = "cuda", torch.bfloat16
    x0 = torch.randn(*shape, device=dev, dtype=bf)
    w0 = (torch.randn(n_out, K, device=dev) / K ** 0.5).to(bf)
    b0 = torch.randn(n_out, device=dev, dtype=bf)
    r0 = torch.randn(*shape[:-1], n_out, device=dev, dtype=bf)
    lw0 = torch.randn(n_out, device=dev) * 0.5 + 1.0
    lb0 = torch.randn(n_out, device=dev)
    gy = torch.randn(*shape[:-1], n_out, device=dev, dtype=bf)
    ctr = fn._rng_counter_for(torch.device("cuda", torch.cuda.current_device()))
    c0 = ctr.clone()

    def leaves():
        return [t.clone().requires_grad_() for t in (x0, w0, b0, r0, lw0, lb0)]

    x, w, b, r, lw, lb = leaves()
    a = ops.linear(x, w, b)
    a.retain_grad()
    y_c = ops.dropout_add_layernorm(a, r, lw, lb, EPS, 0.1, True)
    y_c.backward(gy)
    assert int((ctr - c0).item()) == 1
    dx_drop = a.grad.reshape(-1, n_out)
    comp = [t.grad.clone() for t in (x, w, b, r, lw, lb)]

    ctr.copy_(c0)
    x, w, b, r, lw, lb = leaves()
    y_f = ops.linear_dropout_add_layernorm(x, w, b, r, lw, lb, EPS, 0.1, True)
    assert "LinearDropoutAddLN" in type(y_f.grad_fn).__name__ or \
        "LinearDropoutAddLN" in type(y_f.grad_fn.next_functions[0][0]).__name__
    y_f.backward(gy)
    assert int((ctr - c0).item()) == 1
    fused = [t.grad for t in (x, w, b, r, lw, lb)]

    assert y_f.shape == y_c.shape and torch.equal(y_f, y_c)
    torch.testing.assert_close(fused[0], comp[0], atol=1e-2, rtol=1e-2)
    torch.testing.assert_close(fused[3], comp[3], atol=1e-2, rtol=1e-2)
    torch.testing.assert_close(fused[1], comp[1], atol=1e-1, rtol=5e-2)
    torch.testing.assert_close(fused[4], comp[4], atol=2e-1, rtol=2e-2)
    torch.testing.assert_close(fused[5], comp[5], atol=2e-1, rtol=2e-2)
    assert fused[2].dtype == bf and fused[2].shape == (n_out,)
    _assert_colsum(fused[2], dx_drop, f"wiring dbias {shape}->{n_out}")
    _assert_colsum(comp[2], dx_drop, f"composed dbias {shape}->{n_out}")
