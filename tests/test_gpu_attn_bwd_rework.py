"""GPU numerics of the reworked full-LDS attention backward
(csrc/attention.hip): dq/dk/dv against an fp32 reference with the exact
dropout mask, both layouts, the QKV bias gradient emitted by the kernel,
run-to-run bit-reproducibility, old/new packed entry agreement and the fused
linear+attention autograd node. Gradient tolerances are those of
test_gpu_attention_tiled.py; the dbias bound is the fp32 summation bound."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chinesener_amd import ops
from chinesener_amd.ops import functional as fn

BF = torch.bfloat16
BWD_TOL = dict(atol=0.15, rtol=0.1)
SEED = 987654321
B, H = 2, 2
LS = [1, 17, 32, 48, 128, 160, 176]
CASES = [(L, D, keep) for D in (32, 64) for L in LS for keep in (1.0, 0.7)]


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.ext_available(), "HIP extension must be built for GPU tests"


def _splitmix_uniform(seed: int, idx):
    """Python replica of attn_hash_uniform (csrc/attn_common.h):
    splitmix64(seed, idx) -> [0,1)."""
    with np.errstate(over="ignore"):
        z = (np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)) ^ idx.astype(np.uint64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def _expected_kept(seed, BH, L, keep):
    bh = np.arange(BH, dtype=np.uint64)
    qi = np.arange(L, dtype=np.uint64)
    idx = ((bh[:, None, None] * np.uint64(L) + qi[None, :, None])
           * np.uint64(L) + qi[None, None, :])
    return _splitmix_uniform(seed, idx) < np.float32(keep)


def _pack(q, k, v):
    """[B,H,L,D] x3 -> [B,L,3,H,D]"""
    return torch.stack([t.transpose(1, 2) for t in (q, k, v)], 2).contiguous()


@functools.lru_cache(maxsize=None)
def _case(L, D, keep):
    """Random problem, the forward kernel's (out, lse) and the fp32
    autograd reference under the same dropout mask; computed once per
    case and never modified."""
    gen = torch.Generator(device="cuda").manual_seed(1000 * L + D)
    q, k, v = (torch.randn(B, H, L, D, device="cuda", generator=gen).to(BF)
               for _ in range(3))
    lens = torch.tensor([L, 1], device="cuda")          # len = L and len = 1
    kmask = torch.arange(L, device="cuda")[None, :] < lens[:, None]  # [B,L]
    g = (torch.randn(B, H, L, D, device="cuda", generator=gen)
         * kmask[:, None, :, None]).to(BF)
    scale = 1.0 / math.sqrt(D)
    seed = torch.tensor([SEED], dtype=torch.int64, device="cuda")
    if keep < 1.0:
        kept = torch.from_numpy(_expected_kept(SEED, B * H, L, np.float32(keep))
                                ).to("cuda").reshape(B, H, L, L)
        m = kept.float() / float(np.float32(keep))
    else:
        m = torch.ones(B, H, L, L, device="cuda")
    q32, k32, v32 = (t.float().requires_grad_() for t in (q, k, v))
    s = (q32 @ k32.transpose(-1, -2)) * scale
    s = s.masked_fill(~kmask[:, None, None, :], float("-inf"))
    out_ref = (torch.softmax(s, -1) * m) @ v32
    dq, dk, dv = torch.autograd.grad(out_ref, (q32, k32, v32), g.float())
    lens32 = lens.to(torch.int32)
    if L <= 160:
        out, lse = ops.get_ext().attn_fwd(q, k, v, lens32, scale, keep,
                                          seed if keep < 1.0 else None)
    else:
        # the forward binding stops at L = 160; the backward takes L <= 176
        out = out_ref.detach().to(BF)
        lse = torch.logsumexp(s.detach(), -1)
    return dict(q=q, k=k, v=v, g=g, lens32=lens32, scale=scale, keep=keep,
                seed=seed if keep < 1.0 else None, out=out, lse=lse,
                dq=dq, dk=dk, dv=dv)


def _packed_args(c):
    qkv = _pack(c["q"], c["k"], c["v"])
    return (c["g"].transpose(1, 2).contiguous(), qkv,
            c["out"].transpose(1, 2).contiguous(), c["lse"], c["lens32"],
            c["scale"], c["keep"], c["seed"])


def _dbias_bound(dqkv, out_dtype):
    """Per column of dqkv viewed as [n, C]: float64 sum and the fp32
    summation bound (n-1) 2^-24 sum|x|, plus half a bf16 ulp of the sum
    when the result is rounded to bf16."""
    x = dqkv.reshape(-1, dqkv.shape[2] * dqkv.shape[3] * dqkv.shape[4]).double()
    n = x.shape[0]
    exact = x.sum(0)
    bound = (n - 1) * 2.0 ** -24 * x.abs().sum(0)
    if out_dtype == BF:
        mag = exact.abs() + bound
        e = torch.floor(torch.log2(torch.clamp(mag, min=2.0 ** -126)))
        bound = bound + torch.where(mag > 0, 2.0 ** (e - 8),
                                    torch.zeros_like(mag))
    return exact, bound


@pytest.mark.parametrize("L,D,keep", CASES)
def test_bwd_matches_fp32_reference_both_layouts(L, D, keep):
    _cuda()
    ext = ops.get_ext()
    c = _case(L, D, keep)
    dq, dk, dv = ext.attn_bwd(c["g"], c["q"], c["k"], c["v"], c["out"],
                              c["lse"], c["lens32"], c["scale"], keep,
                              c["seed"])
    for got, want in ((dq, c["dq"]), (dk, c["dk"]), (dv, c["dv"])):
        torch.testing.assert_close(got.float(), want, **BWD_TOL)
    # keys at or beyond len get exactly zero gradient (batch 1 has len 1)
    assert (dk[1, :, 1:] == 0).all() and (dv[1, :, 1:] == 0).all()

    args = _packed_args(c)
    bias = torch.zeros(3 * H * D, device="cuda", dtype=BF)
    (dqkv_old,) = ext.attn_bwd_qkv(*args)
    dqkv, dbias = ext.attn_bwd_qkv_dbias(*args, bias)
    assert dqkv.shape == (B, L, 3, H, D) and dbias.shape == (3 * H * D,)
    assert dbias.dtype == BF
    # old and new packed entries: same dqkv bit for bit
    assert torch.equal(dqkv_old, dqkv)
    for i, want in enumerate((c["dq"], c["dk"], c["dv"])):
        torch.testing.assert_close(dqkv[:, :, i].transpose(1, 2).float(),
                                   want, **BWD_TOL)
    # the two layouts run the same arithmetic
    for i, d in enumerate((dq, dk, dv)):
        assert torch.equal(dqkv[:, :, i].transpose(1, 2), d)


@pytest.mark.parametrize("L,D,keep", CASES)
def test_dbias_is_column_sum_of_returned_dqkv(L, D, keep):
    _cuda()
    ext = ops.get_ext()
    args = _packed_args(_case(L, D, keep))
    for dt in (BF, torch.float32):
        bias = torch.zeros(3 * H * D, device="cuda", dtype=dt)
        dqkv, dbias = ext.attn_bwd_qkv_dbias(*args, bias)
        assert dbias.dtype == dt
        exact, bound = _dbias_bound(dqkv, dt)
        err = (dbias.double() - exact).abs()
        worst = float((err - bound).max())
        print(f"L={L} D={D} keep={keep} {dt}: max err {float(err.max()):.3e} "
              f"max (err - bound) {worst:.3e}")
        assert (err <= bound).all()


@pytest.mark.parametrize("L,D,keep", CASES)
def test_bwd_bit_reproducible(L, D, keep):
    _cuda()
    ext = ops.get_ext()
    args = _packed_args(_case(L, D, keep))
    bias = torch.zeros(3 * H * D, device="cuda", dtype=BF)
    a_dqkv, a_db = ext.attn_bwd_qkv_dbias(*args, bias)
    b_dqkv, b_db = ext.attn_bwd_qkv_dbias(*args, bias)
    assert torch.equal(a_dqkv, b_dqkv)
    assert torch.equal(a_db, b_db)


# ---------------------------------------------------- fused autograd node
def _tiny_layer():
    gen = torch.Generator(device="cuda").manual_seed(5)
    hid, heads, L = 64, 2, 32
    x = torch.randn(B, L, hid, device="cuda", generator=gen).to(BF)
    w = (torch.randn(3 * hid, hid, device="cuda", generator=gen)
         / math.sqrt(hid)).to(BF)
    b = (0.1 * torch.randn(3 * hid, device="cuda", generator=gen)).to(BF)
    lens = torch.tensor([L, 9], device="cuda")
    g = torch.randn(B, L, heads, hid // heads, device="cuda",
                    generator=gen).to(BF)
    return x, w, b, lens, g, heads


@pytest.mark.parametrize("training", [True, False])
def test_fused_node_matches_composition(monkeypatch, training):
    _cuda()
    monkeypatch.delenv("CHINESENER_ATTN_TILED", raising=False)
    monkeypatch.delenv("CHINESENER_NO_ATTN_DROP", raising=False)
    x, w, b, lens, g, heads = _tiny_layer()
    calls = []
    ext = ops.get_ext()

    class _Rec:
        def __getattr__(self, name):
            attr = getattr(ext, name)
            if not callable(attr):
                return attr

            def wrapped(*a, **kw):
                calls.append(name)
                return attr(*a, **kw)
            return wrapped

    monkeypatch.setattr(fn, "get_ext", lambda: _Rec())

    def run(fused):
        xs, ws, bs = (t.clone().requires_grad_() for t in (x, w, b))
        fn._rng_counter_for(x.device).fill_(SEED)
        keep_qkv = {}
        if fused:
            out = ops.linear_attention_qkv(xs, ws, bs, heads, lens=lens,
                                           p_drop=0.1, training=training)
        else:
            qkv = ops.linear(xs, ws, bs).reshape(B, x.shape[1], 3, heads, -1)
            qkv.retain_grad()
            keep_qkv["qkv"] = qkv
            out = ops.attention_qkv(qkv, lens=lens, p_drop=0.1,
                                    training=training)
        out.backward(g)
        ctr = int(fn._rng_counter_for(x.device).item())
        dqkv = keep_qkv["qkv"].grad if not fused else None
        return out.detach(), xs.grad, ws.grad, bs.grad, ctr, dqkv

    calls.clear()
    o1, dx1, dw1, db1, ctr1, _ = run(True)
    assert "attn_bwd_qkv_dbias" in calls and "colsum" not in calls
    calls.clear()
    o2, dx2, dw2, db2, ctr2, dqkv = run(False)
    assert "colsum" in calls
    assert torch.equal(o1, o2)
    assert ctr1 == ctr2
    torch.testing.assert_close(dx1.float(), dx2.float(), **BWD_TOL)
    torch.testing.assert_close(dw1.float(), dw2.float(), **BWD_TOL)
    torch.testing.assert_close(db1.float(), db2.float(), **BWD_TOL)
    exact, bound = _dbias_bound(dqkv, BF)
    assert ((db1.double() - exact).abs() <= bound).all()
    diff = (db1.double() - db2.double()).abs()
    print(f"training={training}: max |fused - colsum| {float(diff.max()):.3e}")
    assert (diff <= bound).all()
