"""CPU checks for the tiled attention feature: the dispatch function and
the pure-torch model of the online-softmax kernel (rescale algebra,
two-sweep backward, dropout placement) against the untiled reference in
fp64. No GPU needed."""
import math

import pytest
import torch

from chinesener_amd.ops import functional as fn
from chinesener_amd.ops import reference as ref

BF = torch.bfloat16


# ------------------------------------------------------------- dispatch
@pytest.mark.parametrize("L,D,dtype,on_gpu,expected", [
    (160, 64, BF, True, "lds"),
    (161, 64, BF, True, "tiled"),
    (176, 64, BF, True, "tiled"),
    (512, 64, BF, True, "tiled"),
    (513, 64, BF, True, "torch"),
    (200, 64, torch.float32, True, "torch"),
    (200, 64, BF, False, "torch"),
    (200, 128, BF, True, "torch"),
])
def test_attn_path_boundaries(monkeypatch, L, D, dtype, on_gpu, expected):
    monkeypatch.delenv("CHINESENER_ATTN_TILED", raising=False)
    assert fn._attn_path(L, D, dtype, on_gpu) == expected


def test_attn_path_env(monkeypatch):
    monkeypatch.setenv("CHINESENER_ATTN_TILED", "off")
    assert fn._attn_path(200, 64, BF, True) == "torch"
    assert fn._attn_path(160, 64, BF, True) == "lds"
    monkeypatch.setenv("CHINESENER_ATTN_TILED", "force")
    assert fn._attn_path(64, 64, BF, True) == "tiled"
    assert fn._attn_path(512, 64, BF, True) == "tiled"
    assert fn._attn_path(513, 64, BF, True) == "torch"
    assert fn._attn_path(64, 64, torch.float32, True) == "torch"
    assert fn._attn_path(64, 64, BF, False) == "torch"
    monkeypatch.delenv("CHINESENER_ATTN_TILED")
    assert fn._attn_path(64, 64, BF, True) == "lds"


def test_attention_qkv_packed_d128_is_torch_path():
    """The packed entry point keeps D in {32, 64}: D=128 on CPU goes
    through the reference and returns its result."""
    torch.manual_seed(0)
    qkv = torch.randn(1, 9, 3, 2, 128)
    out = fn.attention_qkv(qkv)
    q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
    torch.testing.assert_close(out, ref.attention(q, k, v).transpose(1, 2))


# ------------------------------------------------------------ CPU model
SHAPES = [33, 65, 130]
TILES = [(16, 16), (32, 64)]


def _inputs(L, seed=0, B=2, H=2, D=32):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, H, L, D, generator=g, dtype=torch.float64)
               for _ in range(3))
    lens = torch.tensor([L, 5])
    mask = (torch.arange(L)[None, :] < lens[:, None]).long()
    return q, k, v, lens, mask


def _untiled(q, k, v, mask, scale, keep=1.0, keep_mask=None):
    """softmax -> mask/keep -> @V, plus lse, in the dtype of q."""
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    s = s.masked_fill(~mask[:, None, None, :].bool(), float("-inf"))
    p = torch.softmax(s, -1)
    if keep < 1.0:
        p = p * keep_mask.to(p.dtype) / keep
    return torch.matmul(p, v), torch.logsumexp(s, -1)


def _check_fwd_bwd(q, k, v, lens, mask, tq, tk, keep=1.0, keep_mask=None,
                   tol_f=1e-9, tol_b=1e-8):
    L, D = q.shape[2], q.shape[3]
    scale = 1.0 / math.sqrt(D)
    out, lse = ref.attention_tiled(q, k, v, lens, scale, tq, tk, keep,
                                   keep_mask)
    qr, kr, vr = (t.clone().requires_grad_() for t in (q, k, v))
    out_ref, lse_ref = _untiled(qr, kr, vr, mask, scale, keep, keep_mask)
    mrow = mask[:, None, :, None].bool()
    torch.testing.assert_close(out * mrow, out_ref.detach() * mrow,
                               atol=tol_f, rtol=0)
    torch.testing.assert_close(lse, lse_ref.detach(), atol=tol_f, rtol=0)
    assert torch.isfinite(out).all()

    g = torch.randn(out.shape, dtype=out.dtype,
                    generator=torch.Generator().manual_seed(7))
    out_ref.backward(g)
    dq, dk, dv = ref.attention_tiled_bwd(g, q, k, v, out, lse, lens, scale,
                                         tq, tk, keep, keep_mask)
    torch.testing.assert_close(dq, qr.grad, atol=tol_b, rtol=0)
    torch.testing.assert_close(dk, kr.grad, atol=tol_b, rtol=0)
    torch.testing.assert_close(dv, vr.grad, atol=tol_b, rtol=0)
    kmask = ~mask[:, None, :, None].bool().expand_as(dk)
    assert (dk[kmask] == 0).all() and (dv[kmask] == 0).all()


@pytest.mark.parametrize("tq,tk", TILES)
@pytest.mark.parametrize("L", SHAPES)
def test_tiled_model_matches_reference_fp64(L, tq, tk):
    q, k, v, lens, mask = _inputs(L)
    # against ref.attention itself (forward), then fwd+bwd against the
    # same math with lse exposed
    out, _ = ref.attention_tiled(q, k, v, lens, 1.0 / math.sqrt(32), tq, tk)
    out_ref = ref.attention(q, k, v, mask)
    mrow = mask[:, None, :, None].bool()
    torch.testing.assert_close(out * mrow, out_ref * mrow, atol=1e-9, rtol=0)
    _check_fwd_bwd(q, k, v, lens, mask, tq, tk)


@pytest.mark.parametrize("tq,tk", TILES)
@pytest.mark.parametrize("L", SHAPES)
def test_tiled_model_bwd_matches_autograd_of_ref_attention(L, tq, tk):
    q, k, v, lens, mask = _inputs(L, seed=1)
    scale = 1.0 / math.sqrt(32)
    qr, kr, vr = (t.clone().requires_grad_() for t in (q, k, v))
    out_ref = ref.attention(qr, kr, vr, mask)
    g = torch.randn(out_ref.shape, dtype=torch.float64,
                    generator=torch.Generator().manual_seed(8))
    out_ref.backward(g)
    out, lse = ref.attention_tiled(q, k, v, lens, scale, tq, tk)
    dq, dk, dv = ref.attention_tiled_bwd(g, q, k, v, out, lse, lens, scale,
                                         tq, tk)
    torch.testing.assert_close(dq, qr.grad, atol=1e-8, rtol=0)
    torch.testing.assert_close(dk, kr.grad, atol=1e-8, rtol=0)
    torch.testing.assert_close(dv, vr.grad, atol=1e-8, rtol=0)
    assert (dk[1, :, 5:] == 0).all() and (dv[1, :, 5:] == 0).all()


@pytest.mark.parametrize("tq,tk", TILES)
@pytest.mark.parametrize("L", SHAPES)
def test_tiled_model_dropout_placement(L, tq, tk):
    q, k, v, lens, mask = _inputs(L, seed=2)
    keep_mask = torch.rand(2, 2, L, L,
                           generator=torch.Generator().manual_seed(3)) < 0.7
    _check_fwd_bwd(q, k, v, lens, mask, tq, tk, keep=0.7,
                   keep_mask=keep_mask)


def _spiked(L, lens, r0, jstar, seed):
    """Q[.., r0, :] = 16u and K[.., j*, :] = 16u for a unit vector u: the
    score of (r0, j*) is 256*scale above the others, so the running max
    of row r0 jumps at the tile holding j*."""
    g = torch.Generator().manual_seed(seed)
    B, H, D = 2, 2, 32
    q, k, v = (torch.randn(B, H, L, D, generator=g, dtype=torch.float64)
               for _ in range(3))
    u = torch.randn(D, generator=g, dtype=torch.float64)
    u = u / u.norm()
    q[:, :, r0] = 16 * u
    for b in range(B):
        k[b, :, jstar[b]] = 16 * u
    return q, k, v


@pytest.mark.parametrize("tq,tk", TILES)
@pytest.mark.parametrize("where", ["last", "first", "lens_edge"])
def test_tiled_model_forced_rescale(where, tq, tk):
    L = 130
    lens = torch.tensor([L, 70])      # 70: partly masked tile at 16 and 64
    mask = (torch.arange(L)[None, :] < lens[:, None]).long()
    jstar = {"last": [(n - 1) // tk * tk + 1 for n in (L, 70)],
             "first": [1, 1],
             "lens_edge": [L - 1, 69]}[where]
    q, k, v = _spiked(L, lens, r0=37, jstar=jstar, seed=11)
    _check_fwd_bwd(q, k, v, lens, mask, tq, tk, tol_f=1e-8, tol_b=1e-8)
