"""The FFN GEMMs with bias+GELU in their epilogues (csrc/gemm_nt.hip):
gemm_nt_bias_gelu and gemm_nn_dgelu against the kernel pairs they replace,
and the autograd node built on them against the composed ops.

The fused kernels keep the products, the K order and the bf16 rounding of
the plain GEMMs, so u has to equal gemm_nt's output bit for bit on any
data, and so has g to equal bias_gelu_fwd of it: the same GELU expression
(csrc/gelu.h) on the same rounded u, and measured equal in every case. du
comes from the same dgelu expression on the same rounded inputs; equality
is the target there too, but the compiler decides per call site which
a*b+c it contracts into an fma (it already does so differently for the
eight elements of one thread of bias_gelu_bwd_kernel), so an element may
land on the neighbouring bf16 value. Measured on MI355X: 0 to 8 elements
per case on random data and 72 of 98304 in the 256x384x192 integer case,
with either bias dtype, none by more than one step. Each backward case
prints its count; every element of du is held to one bf16 step from the
unfused value.

The bias gradient is summed in another order (per 128-row tile, then the
tiles; before: per 16-row chunk, then the chunks). Both are fixed-order
fp32 sums of bf16 values, so the new one is held to twice the old one's
largest error, each against an fp64 sum of its own du, and never to less
than one ulp of the output dtype at the largest column sum (the final
rounding alone can cost half an ulp on either side)."""
import functools
import math

import pytest
import torch

from chinesener_amd import ops
from chinesener_amd.ops import functional as fn

pytestmark = pytest.mark.gpu

BF = torch.bfloat16

# (M, N, K): one tile and one stage; 6 tiles (fewer workgroups than XCDs),
# three stages, M != N; 9 tiles (XCD remap with a remainder)
SHAPES = [(128, 128, 64), (256, 384, 192), (384, 384, 128)]
# data kind -> standard deviation of u (None: small integers). 8 and 25
# put max |u + bias| near 30 and 100, far into the saturated tanh.
KINDS = {"int": None, "rand": 1.0, "sat30": 8.0, "sat100": 25.0}
BIAS_DTYPES = [BF, torch.float32]


def _ext():
    return ops.get_ext()


def _pattern(rows, cols, mul_r, mul_c, div):
    """Integers in [-3, 3], another non-symmetric pattern per argument
    set, so that a row/column or an operand mix-up shows."""
    r = torch.arange(rows, device="cuda", dtype=torch.int64)[:, None]
    c = torch.arange(cols, device="cuda", dtype=torch.int64)[None, :]
    v = (r * mul_r + c * mul_c + (r // div) * c + (c // 5)) % 7 - 3
    return v.to(BF)


@functools.lru_cache(maxsize=None)
def _fwd_case(M, N, K, kind, bias_dtype):
    """Operands and the unfused results, computed once and shared."""
    sd = KINDS[kind]
    if sd is None:
        a, b = _pattern(M, K, 7, 3, 3), _pattern(N, K, 5, 11, 4)
        bias = _pattern(1, N, 1, 3, 2).reshape(N).to(bias_dtype)
    else:
        g = torch.Generator(device="cuda").manual_seed(M + 3 * N + 7 * K)
        a = torch.randn(M, K, generator=g, device="cuda").to(BF)
        b = (torch.randn(N, K, generator=g, device="cuda")
             * (sd / math.sqrt(K))).to(BF)
        bias = torch.randn(N, generator=g, device="cuda").to(bias_dtype)
    u = _ext().gemm_nt(a, b, None, False)
    g_ref = _ext().bias_gelu_fwd(u, bias)
    return a, b, bias, u, g_ref


@functools.lru_cache(maxsize=None)
def _bwd_case(M, N, K, kind, bias_dtype):
    sd = KINDS[kind]
    if sd is None:
        a, b = _pattern(M, K, 7, 3, 3), _pattern(K, N, 5, 11, 4)
        u = _pattern(M, N, 3, 5, 6)
        bias = _pattern(1, N, 1, 3, 2).reshape(N).to(bias_dtype)
    else:
        g = torch.Generator(device="cuda").manual_seed(2 * M + N + 5 * K)
        a = torch.randn(M, K, generator=g, device="cuda").to(BF)
        b = (torch.randn(K, N, generator=g, device="cuda")
             / math.sqrt(K)).to(BF)
        u = (torch.randn(M, N, generator=g, device="cuda") * sd).to(BF)
        bias = torch.randn(N, generator=g, device="cuda").to(bias_dtype)
    dh = _ext().gemm_nn(a, b, False)
    du_ref, dbias_old = _ext().bias_gelu_bwd(dh, u, bias)
    return a, b, u, bias, du_ref, dbias_old


def _reach(u, bias):
    return (u.float() + bias.float()).abs().max().item()


def _check_reach(kind, reach):
    if kind == "sat30":
        assert reach >= 25
    if kind == "sat100":
        assert reach >= 80


def _ulp(dtype, mag):
    bits = 7 if dtype == BF else 23
    return 2.0 ** (math.floor(math.log2(max(mag, 2.0 ** -126))) - bits)


def _steps(x, ref):
    """Distance of two bf16 tensors in representable values (+0 == -0)."""
    def key(t):
        b = t.contiguous().view(torch.int16).int()
        return torch.where(b < 0, -(b & 0x7FFF), b)
    return (key(x) - key(ref)).abs()


def _check_one_step(x, ref, what):
    assert x.dtype == BF and ref.dtype == BF and x.shape == ref.shape
    assert bool(torch.isfinite(x.float()).all())
    d = _steps(x, ref)
    print(f"{what}: {(d != 0).sum().item()} of {d.numel()} elements differ, "
          f"largest distance {d.max().item()} bf16 step(s)")
    assert d.max().item() <= 1


def _check_dbias(new, old, du_new, du_old, what):
    """Each dbias against the fp64 column sum of its own float(du): the
    new error at most twice the old kernel's largest, and at least one
    ulp of the dtype."""
    ref = du_new.float().double().sum(0)
    e_new = (new.double() - ref).abs().max().item()
    e_old = (old.double()
             - du_old.float().double().sum(0)).abs().max().item()
    bound = max(2 * e_old, _ulp(new.dtype, ref.abs().max().item()))
    print(f"dbias {what}: err new {e_new:.3e} old {e_old:.3e} "
          f"bound {bound:.3e}")
    assert new.dtype == old.dtype and new.shape == old.shape
    assert e_new <= bound


@pytest.mark.parametrize("bias_dtype", BIAS_DTYPES, ids=["bbf16", "bfp32"])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_fwd_equals_gemm_then_bias_gelu(M, N, K, kind, bias_dtype):
    a, b, bias, u_ref, g_ref = _fwd_case(M, N, K, kind, bias_dtype)
    _check_reach(kind, _reach(u_ref, bias))
    u, g = _ext().gemm_nt_bias_gelu(a, b, bias, True)
    assert u.dtype == BF and g.dtype == BF
    assert u.shape == (M, N) and g.shape == (M, N)
    assert u_ref.abs().max().item() > 0
    assert torch.equal(u, u_ref)
    assert torch.equal(g, g_ref)
    # a second call is bitwise the same; without save_pre only g comes back
    u2, g2 = _ext().gemm_nt_bias_gelu(a, b, bias, True)
    assert torch.equal(u2, u) and torch.equal(g2, g)
    u3, g3 = _ext().gemm_nt_bias_gelu(a, b, bias, False)
    assert u3 is None
    assert torch.equal(g3, g)


@pytest.mark.parametrize("bias_dtype", BIAS_DTYPES, ids=["bbf16", "bfp32"])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_bwd_equals_gemm_then_bias_gelu_bwd(M, N, K, kind, bias_dtype):
    a, b, u, bias, du_ref, dbias_old = _bwd_case(M, N, K, kind, bias_dtype)
    _check_reach(kind, _reach(u, bias))
    du, dbias = _ext().gemm_nn_dgelu(a, b, u, bias)
    assert du.dtype == BF and du.shape == (M, N)
    assert dbias.dtype == bias_dtype and dbias.shape == (N,)
    assert du_ref.abs().max().item() > 0
    _check_one_step(du, du_ref, f"bwd {M}x{N}x{K} {kind} du")
    _check_dbias(dbias, dbias_old, du, du_ref, f"{M}x{N}x{K} {kind}")
    du2, dbias2 = _ext().gemm_nn_dgelu(a, b, u, bias)
    assert torch.equal(du2, du) and torch.equal(dbias2, dbias)


def test_ineligible_operands_raise():
    e = _ext()

    def z(*shape, dtype=BF):
        return torch.zeros(*shape, dtype=dtype, device="cuda")

    bad_fwd = [
        (z(64, 64), z(128, 64), z(128)),              # M % 128
        (z(128, 64), z(192, 64), z(192)),             # N % 128
        (z(128, 96), z(128, 96), z(128)),             # K % 64
        (z(128, 64), z(128, 128), z(128)),            # K mismatch
        (z(128, 64, dtype=torch.float16), z(128, 64), z(128)),
        (z(128, 64), z(128, 64, dtype=torch.float32), z(128)),
        (z(128, 64), z(128, 64), z(64)),              # bias length
        (z(128, 64), z(128, 64), z(128, dtype=torch.float16)),
        (z(128, 128)[:, :64], z(128, 64), z(128)),    # strided a
    ]
    for a, b, bias in bad_fwd:
        with pytest.raises(RuntimeError):
            e.gemm_nt_bias_gelu(a, b, bias, True)
    bad_bwd = [
        (z(64, 64), z(64, 128), z(64, 128), z(128)),          # M % 128
        (z(128, 64), z(64, 192), z(128, 192), z(192)),        # N % 128
        (z(128, 96), z(96, 128), z(128, 128), z(128)),        # K % 64
        (z(128, 64), z(128, 128), z(128, 128), z(128)),       # K mismatch
        (z(128, 64), z(64, 128), z(128, 256), z(128)),        # u shape
        (z(128, 64), z(64, 128), z(128, 128, dtype=torch.float32), z(128)),
        (z(128, 64, dtype=torch.float16), z(64, 128), z(128, 128), z(128)),
        (z(128, 64), z(64, 128), z(128, 128), z(256)),        # bias length
        (z(128, 64), z(64, 128), z(128, 128), z(128, dtype=torch.float64)),
    ]
    for a, b, u, bias in bad_bwd:
        with pytest.raises(RuntimeError):
            e.gemm_nn_dgelu(a, b, u, bias)
    torch.cuda.synchronize()


def test_graph_capture_and_replays_equal_eager():
    M, N, K = SHAPES[1]
    a, b, bias, u_ref, g_ref = _fwd_case(M, N, K, "rand", BF)
    a2, b2, u_in, bias2, du_ref, _ = _bwd_case(M, N, K, "rand", BF)
    _, g_eager = _ext().gemm_nt_bias_gelu(a, b, bias, True)
    du_eager, dbias_eager = _ext().gemm_nn_dgelu(a2, b2, u_in, bias2)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):      # warm the allocator off-capture
        _ext().gemm_nt_bias_gelu(a, b, bias, True)
        _ext().gemm_nn_dgelu(a2, b2, u_in, bias2)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        u, g = _ext().gemm_nt_bias_gelu(a, b, bias, True)
        du, dbias = _ext().gemm_nn_dgelu(a2, b2, u_in, bias2)
    for _ in range(2):
        for t in (u, g, du, dbias):
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(u, u_ref) and torch.equal(g, g_eager)
        assert torch.equal(du, du_eager) and torch.equal(dbias, dbias_eager)


def _run_layer(monkeypatch, mode, record):
    """One forward + backward of a bf16 BertLayer (hidden 128, FFN 512,
    B=2, L=64) from a fixed seed; in-tree GEMMs on both sides, so that
    the unfused run launches exactly the pairs the fused kernels replace."""
    from chinesener_amd.models.bert import BertConfig, BertLayer
    monkeypatch.setenv("CHINESENER_GEMM_NT", "force")
    monkeypatch.setenv("CHINESENER_FUSED_GELU", mode)
    if mode == "force":
        orig = fn._ffn_dn

        def spy(dx_drop, w2, u, b1):
            out = orig(dx_drop, w2, u, b1)
            record["du"] = out[0]
            return out
        monkeypatch.setattr(fn, "_ffn_dn", spy)
    else:
        ext = ops.get_ext()

        class _Spy:                    # the extension, bias_gelu_bwd watched
            def __getattr__(self, name):
                return getattr(ext, name)

            def bias_gelu_bwd(self, dy, x, bias):
                out = ext.bias_gelu_bwd(dy, x, bias)
                record["du"] = out[0]
                return out
        monkeypatch.setattr(fn, "get_ext", lambda: _Spy())
    cfg = BertConfig(vocab_size=200, hidden_size=128, num_hidden_layers=1,
                     num_attention_heads=2, intermediate_size=512,
                     max_position_embeddings=64)
    torch.manual_seed(7)
    fn._rng_counter = None             # re-seeded from the line above
    layer = BertLayer(cfg).to("cuda").to(BF).train()
    with torch.no_grad():              # zeros would hide a bias mix-up
        layer.ffn_in_bias.copy_(torch.randn(512) * 0.5)
    x = torch.randn(2, 64, 128, device="cuda").to(BF).requires_grad_()
    mask = torch.ones(2, 64, dtype=torch.long, device="cuda")
    y = layer(x, mask, mask.sum(1))
    dy = torch.randn(y.shape, device="cuda").to(BF)
    y.backward(dy)
    grads = {n: p.grad for n, p in layer.named_parameters()}
    grads["x"] = x.grad
    return y.detach(), grads


def test_bert_layer_force_equals_off(monkeypatch):
    rec, rec_off = {}, {}
    y_f, g_f = _run_layer(monkeypatch, "force", rec)
    monkeypatch.undo()
    y_o, g_o = _run_layer(monkeypatch, "off", rec_off)
    assert "du" in rec                 # the fused node really ran
    assert "du" in rec_off             # and the unfused pair in the other
    assert torch.equal(y_f, y_o)
    assert set(g_f) == set(g_o)
    for name in g_o:
        assert g_f[name] is not None, name
        if name != "ffn_in_bias":
            assert torch.equal(g_f[name], g_o[name]), name
    _check_dbias(g_f["ffn_in_bias"], g_o["ffn_in_bias"], rec["du"],
                 rec_off["du"], "layer")


def test_no_grad_forward_skips_the_pre_activation(monkeypatch):
    """Under no_grad the op takes the fused forward without u and gives
    what the composition gives."""
    monkeypatch.setenv("CHINESENER_GEMM_NT", "force")
    g = torch.Generator(device="cuda").manual_seed(3)

    def r(*shape, s=1.0):
        return (torch.randn(*shape, generator=g, device="cuda") * s).to(BF)

    x, w1, b1 = r(2, 64, 128), r(512, 128, s=0.1), r(512)
    w2, b2, lw, lb = r(128, 512, s=0.05), r(128), r(128), r(128)
    outs = {}
    for mode in ("force", "off"):
        monkeypatch.setenv("CHINESENER_FUSED_GELU", mode)
        calls = []
        orig = fn._ffn_up

        def spy(x2, w, b, save_pre):
            calls.append(save_pre)
            return orig(x2, w, b, save_pre)
        monkeypatch.setattr(fn, "_ffn_up", spy)
        with torch.no_grad():
            outs[mode] = ops.ffn_gelu_dropout_add_layernorm(
                x, w1, b1, w2, b2, x, lw, lb, 1e-12, 0.1, False)
        monkeypatch.setattr(fn, "_ffn_up", orig)
        assert calls == ([False] if mode == "force" else [])
    assert torch.equal(outs["force"], outs["off"])
