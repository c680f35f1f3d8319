"""GPU numerics and wiring of the K/V-tiled attention kernels
(csrc/attention_tiled.hip): the four entry points, the ops-layer dispatch
for 161 <= L <= 512, lse, masking, forced online-softmax rescale, the
exact dropout mask, reproducibility, bounds, graph capture and a tiny
BERT encoder. Tolerances are those of test_attention_fwd_bwd."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chinesener_amd import ops
from chinesener_amd.ops import functional as fn
from chinesener_amd.ops import reference as ref

BF = torch.bfloat16
FWD_TOL = dict(atol=0.06, rtol=0.05)
BWD_TOL = dict(atol=0.15, rtol=0.1)


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.ext_available(), "HIP extension must be built for GPU tests"


class _Recorder:
    """Wraps the extension module and records which entry points ran."""

    def __init__(self, ext):
        self._ext = ext
        self.calls = []

    def __getattr__(self, name):
        attr = getattr(self._ext, name)
        if not callable(attr):
            return attr

        def wrapped(*a, **kw):
            self.calls.append(name)
            return attr(*a, **kw)
        return wrapped

    def tiled(self):
        return [c for c in self.calls if c.startswith("attn_tiled_")]


def _record(monkeypatch):
    rec = _Recorder(ops.get_ext())
    monkeypatch.setattr(fn, "get_ext", lambda: rec)
    return rec


@functools.lru_cache(maxsize=None)
def _case(L, D, B=2, H=2):
    """Random problem + fp32 autograd reference (the construction of
    test_attention_fwd_bwd), computed once per shape and never modified."""
    gen = torch.Generator(device="cuda").manual_seed(1000 * L + D)
    q32, k32, v32 = (torch.randn(B, H, L, D, device="cuda", generator=gen)
                     .requires_grad_() for _ in range(3))
    lens = torch.tensor([L, max(2, L - 41)], device="cuda")
    mask = (torch.arange(L, device="cuda")[None, :] < lens[:, None]).long()
    out_ref = ref.attention(q32, k32, v32, mask)
    g = torch.randn(B, H, L, D, device="cuda", generator=gen) \
        * mask[:, None, :, None]
    dq, dk, dv = torch.autograd.grad(out_ref, (q32, k32, v32), g)
    return dict(q=q32.detach().to(BF), k=k32.detach().to(BF),
                v=v32.detach().to(BF), lens=lens, mask=mask,
                lens32=lens.to(torch.int32), out=out_ref.detach(), g=g.to(BF),
                dq=dq, dk=dk, dv=dv, mrow=mask[:, None, :, None].bool())


def _pack(q, k, v):
    """[B,H,L,D] x3 -> [B,L,3,H,D]"""
    return torch.stack([t.transpose(1, 2) for t in (q, k, v)], 2).contiguous()


def _check_against_case(c, out, dq, dk, dv):
    """out, dq, dk, dv in [B,H,L,D]"""
    torch.testing.assert_close(out.float() * c["mrow"], c["out"] * c["mrow"],
                               **FWD_TOL)
    torch.testing.assert_close(dq.float(), c["dq"], **BWD_TOL)
    torch.testing.assert_close(dk.float(), c["dk"], **BWD_TOL)
    torch.testing.assert_close(dv.float(), c["dv"], **BWD_TOL)
    # masked keys get exactly zero gradient
    kz = ~c["mrow"].expand_as(dk)
    assert (dk[kz] == 0).all() and (dv[kz] == 0).all()


# ------------------------------------------------- direct extension calls
@pytest.mark.parametrize("L,D", [(33, 32), (65, 64), (130, 64), (192, 32)])
def test_entry_points(L, D):
    _cuda()
    ext = ops.get_ext()
    c = _case(L, D)
    scale = 1.0 / math.sqrt(D)
    out, lse = ext.attn_tiled_fwd(c["q"], c["k"], c["v"], c["lens32"], scale,
                                  1.0, None)
    dq, dk, dv = ext.attn_tiled_bwd(c["g"], c["q"], c["k"], c["v"], out, lse,
                                    c["lens32"], scale, 1.0, None)
    _check_against_case(c, out, dq, dk, dv)

    qkv = _pack(c["q"], c["k"], c["v"])
    out_p, lse_p = ext.attn_tiled_fwd_qkv(qkv, c["lens32"], scale, 1.0, None)
    (dqkv,) = ext.attn_tiled_bwd_qkv(c["g"].transpose(1, 2).contiguous(), qkv,
                                     out_p, lse_p, c["lens32"], scale, 1.0,
                                     None)
    assert out_p.shape == (2, L, 2, D) and dqkv.shape == qkv.shape
    # the two layouts run the same arithmetic: bitwise agreement
    assert torch.equal(out_p.transpose(1, 2), out)
    assert torch.equal(lse_p, lse)
    for i, d in enumerate((dq, dk, dv)):
        assert torch.equal(dqkv[:, :, i].transpose(1, 2), d)


# -------------------------------------------------------- through the ops
@pytest.mark.parametrize("L", [161, 170, 177, 256, 512])
def test_ops_dispatch_tiled(L, monkeypatch):
    _cuda()
    monkeypatch.delenv("CHINESENER_ATTN_TILED", raising=False)
    rec = _record(monkeypatch)
    c = _case(L, 64)

    q, k, v = (c[n].clone().requires_grad_() for n in "qkv")
    out = ops.attention(q, k, v, mask=c["mask"])
    out.backward(c["g"])
    assert set(rec.tiled()) == {"attn_tiled_fwd", "attn_tiled_bwd"}, rec.calls
    _check_against_case(c, out.detach(), q.grad, k.grad, v.grad)

    rec.calls.clear()
    qkv = _pack(c["q"], c["k"], c["v"]).requires_grad_()
    out_p = ops.attention_qkv(qkv, mask=c["mask"])
    out_p.backward(c["g"].transpose(1, 2))
    assert set(rec.tiled()) == {"attn_tiled_fwd_qkv", "attn_tiled_bwd_qkv"}, \
        rec.calls
    dq, dk, dv = (qkv.grad[:, :, i].transpose(1, 2) for i in range(3))
    _check_against_case(c, out_p.detach().transpose(1, 2), dq, dk, dv)


def test_ops_dispatch_l128_not_tiled(monkeypatch):
    _cuda()
    monkeypatch.delenv("CHINESENER_ATTN_TILED", raising=False)
    rec = _record(monkeypatch)
    c = _case(128, 64)
    q, k, v = (c[n].clone().requires_grad_() for n in "qkv")
    ops.attention(q, k, v, mask=c["mask"]).backward(c["g"])
    qkv = _pack(c["q"], c["k"], c["v"]).requires_grad_()
    ops.attention_qkv(qkv, mask=c["mask"]).backward(c["g"].transpose(1, 2))
    assert rec.tiled() == []
    assert {"attn_fwd", "attn_bwd", "attn_fwd_qkv", "attn_bwd_qkv"} \
        <= set(rec.calls)


# -------------------------------------------------------------------- lse
def test_lse_matches_full_lds_kernel_and_logsumexp():
    _cuda()
    ext = ops.get_ext()
    c = _case(128, 64)
    scale = 1.0 / math.sqrt(64)
    _, lse_t = ext.attn_tiled_fwd(c["q"], c["k"], c["v"], c["lens32"], scale,
                                  1.0, None)
    _, lse_l = ext.attn_fwd(c["q"], c["k"], c["v"], c["lens32"], scale, 1.0,
                            None)
    torch.testing.assert_close(lse_t, lse_l, atol=1e-2, rtol=0)
    s = torch.matmul(c["q"].float(), c["k"].float().transpose(-1, -2)) * scale
    s = s.masked_fill(~c["mask"][:, None, None, :].bool(), float("-inf"))
    # the kernel sums exact bf16 products in fp32 (<= 64 terms, |s| < ~10)
    # and uses the fast exp/log: a few 1e-5 absolute; 1e-3 leaves margin
    # without hiding a wrong max or a dropped tile (those move lse by >0.01)
    torch.testing.assert_close(lse_t, torch.logsumexp(s, -1), atol=1e-3,
                               rtol=0)


# ---------------------------------------------- masked keys, written rows
@pytest.mark.parametrize("short", [1, 65])
def test_masked_keys_zero_and_all_rows_finite(short):
    _cuda()
    ext = ops.get_ext()
    L, D = 192, 64
    c = _case(L, D)
    lens = torch.tensor([L, short], dtype=torch.int32, device="cuda")
    scale = 1.0 / math.sqrt(D)
    qkv = _pack(c["q"], c["k"], c["v"])
    out, lse = ext.attn_tiled_fwd_qkv(qkv, lens, scale, 1.0, None)
    dout = torch.randn(2, L, 2, D, device="cuda",
                       generator=torch.Generator(device="cuda").manual_seed(5)
                       ).to(BF)
    (dqkv,) = ext.attn_tiled_bwd_qkv(dout, qkv, out, lse, lens, scale, 1.0,
                                     None)
    assert torch.isfinite(out.float()).all()
    assert torch.isfinite(lse).all()
    assert torch.isfinite(dqkv.float()).all()
    assert (dqkv[1, short:, 1:] == 0).all()
    assert (dqkv[0, :, 1:] != 0).any(dim=-1).all()
    # a single real key: softmax is exactly 1 on it, out == V[0] on all rows
    if short == 1:
        assert torch.equal(out[1], qkv[1, 0:1, 2].expand(L, 2, D))


# ----------------------------------------- forced rescale (guide rule 26)
@functools.lru_cache(maxsize=None)
def _spike_base():
    L, D, B, H = 192, 64, 2, 2
    gen = torch.Generator().manual_seed(26)
    q, k, v, g = (torch.randn(B, H, L, D, generator=gen) for _ in range(4))
    u = torch.randn(D, generator=gen)
    return q, k, v, g, u / u.norm()


@pytest.mark.parametrize("where", ["last_tile", "first_tile", "lens_edge"])
def test_forced_rescale(where):
    """One K row spiked against one Q row (score 32 above the rest) so
    the running max of that row jumps at a chosen tile; fp64 host
    reference over the full tensor."""
    _cuda()
    ext = ops.get_ext()
    L, D = 192, 64
    lens_l = [L, 150]                 # batch 1: last tile 128..149 is partial
    jstar = {"last_tile": [130, 130], "first_tile": [1, 1],
             "lens_edge": [L - 1, 149]}[where]
    q, k, v, g, u = (t.clone() for t in _spike_base())
    r0 = 77
    q[:, :, r0] = 16 * u
    for b in range(2):
        k[b, :, jstar[b]] = 16 * u
    q, k, v, g = (t.to(BF) for t in (q, k, v, g))
    scale = 1.0 / math.sqrt(D)

    mask = (torch.arange(L)[None, :] < torch.tensor(lens_l)[:, None]).long()
    q64, k64, v64 = (t.double().requires_grad_() for t in (q, k, v))
    out_ref = ref.attention(q64, k64, v64, mask, scale)
    dq_r, dk_r, dv_r = torch.autograd.grad(out_ref, (q64, k64, v64),
                                           g.double())

    lens = torch.tensor(lens_l, dtype=torch.int32, device="cuda")
    qc, kc, vc, gc = (t.cuda() for t in (q, k, v, g))
    out, lse = ext.attn_tiled_fwd(qc, kc, vc, lens, scale, 1.0, None)
    dq, dk, dv = ext.attn_tiled_bwd(gc, qc, kc, vc, out, lse, lens, scale,
                                    1.0, None)
    torch.testing.assert_close(out.double().cpu(), out_ref.detach(),
                               **FWD_TOL)
    torch.testing.assert_close(dq.double().cpu(), dq_r, **BWD_TOL)
    torch.testing.assert_close(dk.double().cpu(), dk_r, **BWD_TOL)
    torch.testing.assert_close(dv.double().cpu(), dv_r, **BWD_TOL)
    # the spiked row really is dominated by the spiked key
    b_probe = out[1, :, r0].float().cpu()
    torch.testing.assert_close(b_probe, v[1, :, jstar[1]].float(),
                               atol=0.02, rtol=0.02)


# ---------------------------------------------------- exact dropout mask
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


SEED = 987654321


def _set_counter(device):
    fn._rng_counter_for(device).fill_(SEED)


def test_dropout_mask_exact_l192(monkeypatch):
    """V = identity on one 64-key block makes out[..., :64] that block of
    the dropped probability matrix; dout = identity on one 64-query block
    makes dV the backward-regenerated one. Through ops.attention_qkv with
    the shared device counter pinned to a known seed."""
    _cuda()
    monkeypatch.delenv("CHINESENER_ATTN_TILED", raising=False)
    monkeypatch.delenv("CHINESENER_NO_ATTN_DROP", raising=False)
    rec = _record(monkeypatch)
    B, L, H, D, keep = 2, 192, 1, 64, 0.7
    gen = torch.Generator(device="cuda").manual_seed(43)
    base = torch.randn(B, L, 3, H, D, device="cuda", generator=gen).to(BF)
    lens = torch.full((B,), L, dtype=torch.int32, device="cuda")
    eye = torch.eye(64, device="cuda", dtype=BF)

    p_fwd = np.zeros((B, L, L), np.float32)
    p_bwd = np.zeros((B, L, L), np.float32)
    for j in range(L // 64):
        qkv = base.clone()
        qkv[:, :, 2, 0, :] = 0
        qkv[:, j * 64:(j + 1) * 64, 2, 0, :] = eye
        qkv.requires_grad_()
        _set_counter(qkv.device)
        out = ops.attention_qkv(qkv, lens=lens, p_drop=0.3,
                                training=True)
        p_fwd[:, :, j * 64:(j + 1) * 64] = \
            out.detach()[:, :, 0].float().cpu().numpy()
        # query block j: dV[b, k, 0, i] = P'[b, j*64 + i, k]
        dout = torch.zeros(B, L, H, D, device="cuda", dtype=BF)
        dout[:, j * 64:(j + 1) * 64, 0, :] = eye
        out.backward(dout)
        dv = qkv.grad[:, :, 2, 0].float().cpu().numpy()       # [B, k, i]
        p_bwd[:, j * 64:(j + 1) * 64, :] = np.swapaxes(dv, 1, 2)
    assert "attn_tiled_fwd_qkv" in rec.calls
    assert "attn_tiled_bwd_qkv" in rec.calls

    kept_exp = _expected_kept(SEED, B * H, L, keep)
    kept_fwd = p_fwd != 0.0
    assert (kept_fwd == kept_exp).all(), \
        f"forward mask mismatch: {np.sum(kept_fwd != kept_exp)} cells"
    assert (p_fwd[kept_fwd] > 0).all()
    kept_bwd = p_bwd != 0.0
    assert (kept_bwd == kept_fwd).all(), \
        f"bwd-regenerated mask mismatch: {np.sum(kept_bwd != kept_fwd)} cells"
    np.testing.assert_allclose(p_bwd, p_fwd, atol=1e-2, rtol=1e-2)
    # rows of the dropped matrix sum to (kept mass)/keep: about 1
    assert abs(float(p_fwd.sum(-1).mean()) - 1.0) < 0.05


def test_dropout_mask_same_for_both_kernels_l64(monkeypatch):
    _cuda()
    monkeypatch.delenv("CHINESENER_NO_ATTN_DROP", raising=False)
    rec = _record(monkeypatch)
    B, L, H, D, keep = 2, 64, 1, 64, 0.7
    gen = torch.Generator(device="cuda").manual_seed(44)
    qkv = torch.randn(B, L, 3, H, D, device="cuda", generator=gen).to(BF)
    qkv[:, :, 2, 0, :] = torch.eye(64, device="cuda", dtype=BF)
    lens = torch.full((B,), L, dtype=torch.int32, device="cuda")
    pats = {}
    for mode in ("force", None):
        if mode:
            monkeypatch.setenv("CHINESENER_ATTN_TILED", mode)
        else:
            monkeypatch.delenv("CHINESENER_ATTN_TILED")
        rec.calls.clear()
        _set_counter(qkv.device)
        out = ops.attention_qkv(qkv, lens=lens, p_drop=0.3,
                                training=True)
        assert rec.calls.count("attn_tiled_fwd_qkv") == (1 if mode else 0)
        assert rec.calls.count("attn_fwd_qkv") == (0 if mode else 1)
        pats[mode] = out[:, :, 0].float().cpu().numpy() != 0.0
    assert (pats["force"] == pats[None]).all()
    assert (pats["force"] == _expected_kept(SEED, B * H, L, keep)).all()


# ------------------------------------------------------- reproducibility
def test_bitwise_reproducible():
    _cuda()
    ext = ops.get_ext()
    L, D, keep = 192, 64, 0.7
    c = _case(L, D)
    scale = 1.0 / math.sqrt(D)
    seed = torch.tensor([SEED], dtype=torch.int64, device="cuda")
    qkv = _pack(c["q"], c["k"], c["v"])
    dout = c["g"].transpose(1, 2).contiguous()
    runs = []
    for _ in range(2):
        out, lse = ext.attn_tiled_fwd_qkv(qkv, c["lens32"], scale, keep, seed)
        (dqkv,) = ext.attn_tiled_bwd_qkv(dout, qkv, out, lse, c["lens32"],
                                         scale, keep, seed)
        runs.append((out, lse, dqkv))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ----------------------------------------------------------------- bounds
def test_bounds(monkeypatch):
    _cuda()
    ext = ops.get_ext()
    lens = torch.tensor([513], dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError):
        ext.attn_tiled_fwd_qkv(
            torch.zeros(1, 513, 3, 1, 64, device="cuda", dtype=BF), lens,
            0.125, 1.0, None)
    with pytest.raises(RuntimeError):
        ext.attn_tiled_fwd_qkv(
            torch.zeros(1, 64, 3, 1, 128, device="cuda", dtype=BF),
            torch.tensor([64], dtype=torch.int32, device="cuda"), 0.125, 1.0,
            None)
    with pytest.raises(RuntimeError):
        ext.attn_tiled_fwd_qkv(
            torch.zeros(1, 64, 3, 1, 64, device="cuda"),     # fp32
            torch.tensor([64], dtype=torch.int32, device="cuda"), 0.125, 1.0,
            None)

    monkeypatch.delenv("CHINESENER_ATTN_TILED", raising=False)
    rec = _record(monkeypatch)
    gen = torch.Generator(device="cuda").manual_seed(9)
    qkv = torch.randn(1, 513, 3, 2, 64, device="cuda", generator=gen).to(BF)
    mask = torch.ones(1, 513, dtype=torch.long, device="cuda")
    out = ops.attention_qkv(qkv, mask=mask)
    assert not [c for c in rec.calls if c.startswith("attn_")]
    q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
    assert torch.equal(out, ref.attention(q, k, v, mask).transpose(1, 2))


# ---------------------------------------------------------- graph capture
def test_graph_capture_replay(monkeypatch):
    _cuda()
    monkeypatch.delenv("CHINESENER_ATTN_TILED", raising=False)
    L, D = 192, 64
    c = _case(L, D)
    lens = c["lens32"]
    gen = torch.Generator(device="cuda").manual_seed(12)
    inputs = [(torch.randn(2, L, 3, 2, D, device="cuda", generator=gen).to(BF),
               torch.randn(2, L, 2, D, device="cuda", generator=gen).to(BF))
              for _ in range(3)]

    def step(x, g):
        out = ops.attention_qkv(x, lens=lens)
        (dx,) = torch.autograd.grad(out, x, g)
        return out, dx

    sx = inputs[0][0].clone().requires_grad_()
    sg = inputs[0][1].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(sx, sg)
    torch.cuda.current_stream().wait_stream(side)

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s_out, s_dx = step(sx, sg)
    for x, g in inputs[1:]:
        with torch.no_grad():
            sx.copy_(x)
            sg.copy_(g)
        graph.replay()
        e_out, e_dx = step(x.clone().requires_grad_(), g)
        assert torch.equal(s_out, e_out)
        assert torch.equal(s_dx, e_dx)


# ------------------------------------------------------------ model level
def test_tiny_bert_l170_matches_torch_fallback(monkeypatch):
    """Two-layer encoder at the MRC length: default dispatch (tiled
    kernel) against CHINESENER_ATTN_TILED=off (the torch path). The bound
    is two layers' worth of the kernel-level forward tolerance; measured
    max difference is in profiles/attn_tiled_r03.md."""
    _cuda()
    from chinesener_amd.models.bert import BertConfig, BertModel
    from chinesener_amd.train.precision import convert_bf16_mixed
    torch.manual_seed(170)
    cfg = BertConfig(vocab_size=300, hidden_size=64, num_hidden_layers=2,
                     num_attention_heads=2, intermediate_size=128,
                     max_position_embeddings=256)
    model = convert_bf16_mixed(BertModel(cfg).cuda()).eval()
    B, L = 3, 170
    lens = torch.tensor([170, 163, 97], device="cuda")
    mask = (torch.arange(L, device="cuda")[None, :] < lens[:, None]).long()
    ids = torch.randint(1, 300, (B, L), device="cuda") * mask

    monkeypatch.delenv("CHINESENER_ATTN_TILED", raising=False)
    rec = _record(monkeypatch)
    with torch.no_grad():
        y_tiled = model(ids, mask)
    assert rec.calls.count("attn_tiled_fwd_qkv") == 2
    monkeypatch.setenv("CHINESENER_ATTN_TILED", "off")
    rec.calls.clear()
    with torch.no_grad():
        y_off = model(ids, mask)
    assert rec.tiled() == []
    m = mask[:, :, None].bool()
    diff = ((y_tiled.float() - y_off.float()) * m).abs().max().item()
    print(f"tiny BERT L=170 max |tiled - off| on real tokens: {diff:.5f}")
    torch.testing.assert_close(y_tiled.float() * m, y_off.float() * m,
                               atol=0.1, rtol=0.1)
