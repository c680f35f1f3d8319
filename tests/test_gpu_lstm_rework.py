"""BiLSTM recurrence kernels (csrc/lstm.hip) against a step-by-step fp32
model of the recurrence that rounds where the kernels round.

The extension entry points are called directly with given gates_x, so no
GEMM noise enters. The model (CPU, fp32): bf16 gates_x, bf16 weights,
h_{t-1} rounded to bf16 before the product, fp32 cell state, outputs zero
and state carried at t >= len. The backward model is the hand-written LSTM
backward in fp32 with dgates rounded to bf16 before the W_hh^T product; it
and the kernel are both fed the forward MODEL's cs and gates, so the
backward tests do not depend on the forward kernel.

Bounds. `PARENT_ERR` holds, per output and I/O dtype, the largest absolute
and relative error of the kernels of the commit before the compile-time-H
rework against this model, over exactly the cases below (table in
profiles/lstm_r06.md). A test allows twice that (FMA contraction may differ
between instantiations) and, for bf16 outputs, at least one bf16 ulp of the
model's value. No bound comes from the reworked kernels' own error.
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from chinesener_amd import ops
from chinesener_amd.ops import reference as ref

CLIP = 0.25        # small enough that cells reach it (asserted below)
CLIP_MARGIN = 1e-3
REL_FLOOR = 1e-2   # relative error is taken where |model| >= this

# (abs, rel) of the parent commit's kernels against the model.
PARENT_ERR = {
    ("hs", "bf16"): (7.094383e-03, 4.436866e-03),
    ("cs", "bf16"): (1.002252e-04, 4.447383e-03),
    ("gates", "bf16"): (2.029240e-04, 9.929492e-03),
    ("dgates_x", "bf16"): (7.600784e-03, 8.460474e-03),
    ("hs", "fp32"): (2.555847e-04, 7.031226e-03),
    ("cs", "fp32"): (4.515573e-04, 7.011455e-03),
    ("gates", "fp32"): (5.368590e-04, 1.001565e-02),
    ("dgates_x", "fp32"): (3.278255e-06, 6.937469e-05),
    # h = 200 through ops.bilstm (forward kernel's own cs/gates feed the
    # backward there)
    ("hs200", "bf16"): (1.945496e-03, 3.883835e-03),
    ("dgates_x200", "bf16"): (3.850341e-03, 4.043258e-03),
}

# kind: "fw"/"rv" = single-direction entry (reverse off/on, no clip in that
# binding), "bi" = bidirectional entry.
# (kind, H, B, L, activation, cell_clip, dtype)
CASES = [
    ("fw", 32, 5, 24, "tanh", 0.0, "bf16"),
    ("rv", 32, 17, 24, "relu", 0.0, "fp32"),
    ("fw", 64, 33, 24, "relu", 0.0, "bf16"),
    ("rv", 64, 5, 2, "tanh", 0.0, "bf16"),
    ("fw", 96, 17, 24, "tanh", 0.0, "fp32"),
    ("rv", 96, 33, 24, "relu", 0.0, "bf16"),
    ("fw", 128, 17, 24, "relu", 0.0, "bf16"),
    ("rv", 128, 33, 24, "tanh", 0.0, "bf16"),
    ("fw", 128, 5, 1, "tanh", 0.0, "fp32"),
    ("rv", 160, 5, 24, "tanh", 0.0, "bf16"),
    ("fw", 160, 17, 2, "relu", 0.0, "fp32"),
    ("fw", 256, 33, 24, "tanh", 0.0, "bf16"),
    ("rv", 256, 5, 24, "relu", 0.0, "fp32"),
    ("bi", 32, 33, 24, "relu", CLIP, "bf16"),
    ("bi", 64, 17, 24, "tanh", 0.0, "fp32"),
    ("bi", 96, 5, 24, "relu", CLIP, "fp32"),
    ("bi", 96, 17, 1, "tanh", CLIP, "bf16"),
    ("bi", 128, 33, 24, "relu", CLIP, "bf16"),
    ("bi", 128, 17, 24, "tanh", CLIP, "bf16"),
    ("bi", 128, 5, 2, "relu", 0.0, "fp32"),
    ("bi", 160, 33, 24, "relu", CLIP, "bf16"),
    ("bi", 160, 5, 24, "tanh", 0.0, "fp32"),
    ("bi", 256, 17, 24, "tanh", CLIP, "bf16"),
    ("bi", 256, 5, 1, "relu", CLIP, "fp32"),
]
CASE_IDS = ["-".join(str(v) for v in c) for c in CASES]


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.ext_available(), "HIP extension must be built for GPU tests"


def _bf(x):
    return x.to(torch.bfloat16).float()


def _act(x, relu):
    return torch.relu(x) if relu else torch.tanh(x)


def _dact_from_out(y, relu):
    return (y > 0).float() if relu else 1.0 - y * y


def _lens(B, L):
    """0, 1, L and values in between, whatever B and L are."""
    pat = [L, 0, 1, L // 2, L - 1, L // 3, L, (2 * L) // 3]
    return torch.tensor([min(max(pat[i % len(pat)], 0), L) for i in range(B)],
                        dtype=torch.int32)


# ------------------------------------------------------------------ model
def model_fwd(gx, w, lens, reverse, relu, clip):
    """One direction. gx [B,L,4H] fp32 holding bf16 values, w [H,4H] fp32
    holding bf16 values. Returns hs [B,L,H], cs [B,L,H], gates [B,L,H,4]
    (activated i, f, g, o, computed at every step like the kernel)."""
    B, L, H4 = gx.shape
    H = H4 // 4
    h = torch.zeros(B, H)
    c = torch.zeros(B, H)
    hs = torch.zeros(B, L, H)
    cs = torch.zeros(B, L, H)
    gates = torch.zeros(B, L, H, 4)
    order = range(L - 1, -1, -1) if reverse else range(L)
    for t in order:
        pre = gx[:, t] + _bf(h) @ w
        gi = 1.0 / (1.0 + torch.exp(-pre[:, 0 * H:1 * H]))
        gf = 1.0 / (1.0 + torch.exp(-pre[:, 1 * H:2 * H]))
        gg = _act(pre[:, 2 * H:3 * H], relu)
        go = 1.0 / (1.0 + torch.exp(-pre[:, 3 * H:4 * H]))
        c_new = gf * c + gi * gg
        if clip > 0:
            c_new = c_new.clamp(-clip, clip)
        h_new = go * _act(c_new, relu)
        valid = (t < lens).unsqueeze(1)
        c = torch.where(valid, c_new, c)
        h = torch.where(valid, _bf(h_new), h)  # carried as the bf16 operand
        hs[:, t] = torch.where(valid, h_new, torch.zeros_like(h_new))
        cs[:, t] = c
        gates[:, t] = torch.stack([gi, gf, gg, go], dim=-1)
    return hs, cs, gates


def model_bwd(dhs, cs, gates, w, lens, reverse, relu, clip):
    """dhs [B,L,H] fp32, cs/gates from model_fwd, w [H,4H]. Returns the
    pre-activation gate grads [B,L,4H]."""
    B, L, H = dhs.shape
    dh_c = torch.zeros(B, H)
    dc_c = torch.zeros(B, H)
    out = torch.zeros(B, L, 4 * H)
    order = range(L) if reverse else range(L - 1, -1, -1)
    for t in order:
        t_prev = t + 1 if reverse else t - 1
        valid = (t < lens).unsqueeze(1)
        gi, gf, gg, go = gates[:, t].unbind(-1)
        c_t = cs[:, t]
        if 0 <= t_prev < L:
            c_prev = torch.where((t_prev < lens).unsqueeze(1), cs[:, t_prev],
                                 torch.zeros_like(c_t))
        else:
            c_prev = torch.zeros_like(c_t)
        ac = _act(c_t, relu)
        dh = dh_c + dhs[:, t]
        dc = dc_c + dh * go * _dact_from_out(ac, relu)
        dgo = dh * ac * go * (1.0 - go)
        if clip > 0:
            dc = torch.where(c_t.abs() >= clip, torch.zeros_like(dc), dc)
        dgi = dc * gg * gi * (1.0 - gi)
        dgf = dc * c_prev * gf * (1.0 - gf)
        dgg = dc * gi * _dact_from_out(gg, relu)
        dg = torch.cat([dgi, dgf, dgg, dgo], dim=1)
        dg = torch.where(valid, dg, torch.zeros_like(dg))
        dc_c = torch.where(valid, dc * gf, dc_c)
        out[:, t] = dg
        dh_c = torch.where(valid, _bf(dg) @ w.t(), dh_c)
    return out


# ------------------------------------------------------------------ cases
def _near_clip(cs, lens, clip):
    """Valid, unclamped cells whose |c| lies within CLIP_MARGIN of the clip:
    a rounding difference there could flip the backward's |c| >= clip."""
    L = cs.shape[1]
    valid = (torch.arange(L).unsqueeze(0) < lens.unsqueeze(1)).unsqueeze(-1)
    a = cs.abs()
    return valid & (a < clip) & (a > clip - CLIP_MARGIN)


@functools.lru_cache(maxsize=None)
def make_case(kind, H, B, L, act, clip, dtype):
    """Seeded inputs and the model's outputs (CPU, computed once per case
    and shared by the forward and backward tests; never modified)."""
    seed = 1000 + CASES.index((kind, H, B, L, act, clip, dtype))
    g = torch.Generator().manual_seed(seed)
    D = 2 if kind == "bi" else 1
    relu = act == "relu"
    lens = _lens(B, L)
    gx = _bf(torch.randn(B, L, D * 4 * H, generator=g))
    w = [_bf(torch.randn(H, 4 * H, generator=g) * (0.5 / math.sqrt(H)))
         for _ in range(D)]
    dhs = _bf(torch.randn(B, L, D * H, generator=g))
    revs = [False, True] if kind == "bi" else [kind == "rv"]

    def run():
        return [model_fwd(gx[..., d * 4 * H:(d + 1) * 4 * H], w[d], lens,
                          revs[d], relu, clip) for d in range(D)]

    fw = run()
    if clip > 0:
        # Move cells that sit within CLIP_MARGIN below the clip away from
        # it: closing their input and forget gates (-20, exact in bf16)
        # leaves c ~ 0 there. Repeat, since later cells shift.
        for _ in range(20):
            bad = [_near_clip(fw[d][1], lens, clip) for d in range(D)]
            if not any(b.any() for b in bad):
                break
            for d in range(D):
                b_i, t_i, j_i = bad[d].nonzero(as_tuple=True)
                gx[b_i, t_i, d * 4 * H + 0 * H + j_i] = -20.0
                gx[b_i, t_i, d * 4 * H + 1 * H + j_i] = -20.0
            fw = run()
    bw = [model_bwd(dhs[..., d * H:(d + 1) * H], fw[d][1], fw[d][2], w[d],
                    lens, revs[d], relu, clip) for d in range(D)]
    return dict(D=D, H=H, B=B, L=L, relu=relu, clip=clip, lens=lens, gx=gx,
                w=w, dhs=dhs, revs=revs,
                hs=torch.cat([f[0] for f in fw], dim=-1),        # [B,L,D*H]
                cs=torch.stack([f[1] for f in fw]),              # [D,B,L,H]
                gates=torch.stack([f[2].reshape(B, L, 4 * H)     # [D,B,L,4H]
                                   for f in fw]),
                dgx=torch.cat(bw, dim=-1))                       # [B,L,D*4H]


def _tdtype(dtype):
    return torch.bfloat16 if dtype == "bf16" else torch.float32


def kernel_fwd(case, dtype):
    """hs [B,L,D*H], cs [D,B,L,H], gates [D,B,L,4H] from the extension."""
    ext = ops.get_ext()
    gx = case["gx"].to("cuda", _tdtype(dtype)).contiguous()
    lens = case["lens"].cuda()
    if case["D"] == 1:
        hs, cs, gates = ext.lstm_fwd(gx, case["w"][0].cuda(), lens,
                                     case["revs"][0], case["relu"])
        return hs, cs.unsqueeze(0), gates.unsqueeze(0)
    w_t2 = torch.stack([w.t() for w in case["w"]]).to(
        "cuda", torch.bfloat16).contiguous()
    hs, cs, gates = ext.bilstm_fwd(gx, w_t2, lens, case["relu"], case["clip"])
    return hs, cs, gates


def kernel_bwd(case, dtype):
    """dgates_x [B,L,D*4H] from the extension, fed the model's cs/gates."""
    ext = ops.get_ext()
    dhs = case["dhs"].to("cuda", _tdtype(dtype)).contiguous()
    lens = case["lens"].cuda()
    cs = case["cs"].cuda().contiguous()
    gates = case["gates"].cuda().contiguous()
    if case["D"] == 1:
        hs = case["hs"].to("cuda", _tdtype(dtype))
        (dgx,) = ext.lstm_bwd(dhs, hs, cs[0], gates[0], case["w"][0].cuda(),
                              lens, case["revs"][0], case["relu"])
        return dgx
    w2 = torch.stack(case["w"]).to("cuda", torch.bfloat16).contiguous()
    return ext.bilstm_bwd(dhs, cs, gates, w2, lens, case["relu"],
                          case["clip"])


# ------------------------------------------------------------- comparison
def errors(got, want):
    """Largest absolute error, and largest relative error over the
    elements with |want| >= REL_FLOOR."""
    got = got.detach().float().cpu()
    d = (got - want).abs()
    assert torch.isfinite(got).all()
    big = want.abs() >= REL_FLOOR
    rel = (d[big] / want.abs()[big]).max().item() if big.any() else 0.0
    return d.max().item() if d.numel() else 0.0, rel


def check(name, dtype, got, want, bf16_out):
    e_abs, e_rel = errors(got, want)
    p_abs, p_rel = PARENT_ERR[(name, dtype)]
    print(f"{name} {dtype}: abs {e_abs:.3e} (parent {p_abs:.3e}) "
          f"rel {e_rel:.3e} (parent {p_rel:.3e})")
    got = got.detach().float().cpu()
    d = (got - want).abs()
    bound = torch.full_like(want, 2 * p_abs)
    rel_bound = 2 * p_rel
    if bf16_out:
        # one bf16 ulp of the model's value: 2^(floor(log2|x|) - 7)
        ulp = torch.exp2(torch.floor(torch.log2(
            want.abs().clamp_min(1e-30))) - 7)
        bound = torch.maximum(bound, ulp)
        rel_bound = max(rel_bound, 2.0 ** -7)
    worst = (d - bound).max().item() if d.numel() else -1.0
    assert worst <= 0, f"{name}: |err| exceeds the bound by {worst:.3e}"
    big = want.abs() >= REL_FLOOR
    if big.any():
        r = (d[big] / want.abs()[big]).max().item()
        assert r <= rel_bound, f"{name}: rel err {r:.3e} > {rel_bound:.3e}"


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize("case_args", CASES, ids=CASE_IDS)
def test_case_inputs(case_args):
    """Conditions on the inputs, asserted on the model (CPU only)."""
    kind, H, B, L, act, clip, dtype = case_args
    case = make_case(*case_args)
    lens = case["lens"]
    valid = torch.arange(L).unsqueeze(0) < lens.unsqueeze(1)     # [B,L]
    assert (~valid).float().mean() >= 0.10
    assert int(lens.min()) == 0 and int(lens.max()) == L
    if L > 1:
        assert 1 in lens.tolist()
    if L > 2:
        assert any(1 < v < L for v in lens.tolist())
    if clip > 0:
        cs = case["cs"]                                          # [D,B,L,H]
        v = valid.unsqueeze(0).unsqueeze(-1).expand_as(cs)
        clamped = (cs.abs() == clip) & v
        assert clamped.sum().item() >= 0.05 * v.sum().item()
        for d in range(case["D"]):
            assert not _near_clip(cs[d], lens, clip).any()


@pytest.mark.parametrize("case_args", CASES, ids=CASE_IDS)
def test_forward_vs_model(case_args):
    _cuda()
    dtype = case_args[-1]
    case = make_case(*case_args)
    hs, cs, gates = kernel_fwd(case, dtype)
    torch.cuda.synchronize()
    check("hs", dtype, hs, case["hs"], bf16_out=dtype == "bf16")
    check("cs", dtype, cs, case["cs"], bf16_out=False)
    check("gates", dtype, gates, case["gates"], bf16_out=False)


@pytest.mark.parametrize("case_args", CASES, ids=CASE_IDS)
def test_backward_vs_model(case_args):
    _cuda()
    dtype = case_args[-1]
    case = make_case(*case_args)
    dgx = kernel_bwd(case, dtype)
    torch.cuda.synchronize()
    check("dgates_x", dtype, dgx, case["dgx"], bf16_out=dtype == "bf16")


def run_bilstm200():
    """h = 200 through ops.bilstm (zero-padded to 224). x is one-hot with
    a row of its own per (b, t) and the biases are zero, so the
    x-projection returns rows of W_ih exactly and W_ih.grad is dgates_x
    exactly: no GEMM rounding enters. Returns kernel and model (hs, dgx)."""
    from chinesener_amd.ops import functional as fn
    h, B, L = 200, 5, 24
    g = torch.Generator().manual_seed(4200)
    lens = _lens(B, L)
    w_ih = [_bf(torch.randn(B * L, 4 * h, generator=g)) for _ in range(2)]
    w_hh = [_bf(torch.randn(h, 4 * h, generator=g) * (0.5 / math.sqrt(h)))
            for _ in range(2)]
    dhs = _bf(torch.randn(B, L, 2 * h, generator=g))
    m_hs, m_dg = [], []
    for d in range(2):
        gx = w_ih[d].reshape(B, L, 4 * h)
        hs, cs, gates = model_fwd(gx, w_hh[d], lens, d == 1, False, 0.0)
        m_hs.append(hs)
        m_dg.append(model_bwd(dhs[..., d * h:(d + 1) * h], cs, gates,
                              w_hh[d], lens, d == 1, False, 0.0))
    x = torch.eye(B * L, device="cuda", dtype=torch.bfloat16) \
        .reshape(B, L, B * L)
    wi = [w.cuda().requires_grad_() for w in w_ih]
    wh = [w.cuda().requires_grad_() for w in w_hh]
    bs = [torch.zeros(4 * h, device="cuda") for _ in range(2)]
    out = fn.bilstm(x, wi[0], wh[0], bs[0], wi[1], wh[1], bs[1], lens.cuda(),
                    "tanh")
    assert out.shape == (B, L, 2 * h)
    out.backward(dhs.to("cuda", torch.bfloat16))
    k_dg = torch.cat([w.grad.reshape(B, L, 4 * h) for w in wi], dim=-1)
    return out, k_dg, torch.cat(m_hs, -1), torch.cat(m_dg, -1)


def test_bilstm_h200_padded_vs_model():
    _cuda()
    hs, dg, m_hs, m_dg = run_bilstm200()
    check("hs200", "bf16", hs, m_hs, bf16_out=True)
    check("dgates_x200", "bf16", dg, m_dg, bf16_out=True)


@pytest.mark.parametrize("h", [32, 128])
def test_bilstm_end_to_end_vs_reference(h):
    """fn.bilstm forward+backward against ref.bilstm_forward autograd in
    fp32, at the tolerances tests/test_gpu_kernels.py uses for the same
    comparison."""
    _cuda()
    torch.manual_seed(60 + h)
    from chinesener_amd.ops import functional as fn
    B, L, E = 4, 16, 16
    x32 = torch.randn(B, L, E, device="cuda") * 0.5
    ws = [(torch.randn(E, 4 * h, device="cuda") * 0.1).requires_grad_()
          for _ in range(2)]
    whs = [(torch.randn(h, 4 * h, device="cuda") * 0.1).requires_grad_()
           for _ in range(2)]
    bs = [(torch.randn(4 * h, device="cuda") * 0.1).requires_grad_()
          for _ in range(2)]
    lens = torch.tensor([16, 11, 3, 16], device="cuda")

    xr = x32.detach().clone().requires_grad_()
    out_ref = ref.bilstm_forward(xr, ws[0], whs[0], bs[0], ws[1], whs[1],
                                 bs[1], lens, "tanh")
    (out_ref ** 2).sum().backward()
    ref_grads = [t.grad.clone() for t in [xr] + ws + whs + bs]
    for t in ws + whs + bs:
        t.grad = None

    x2 = x32.detach().to(torch.bfloat16).requires_grad_()
    out = fn.bilstm(x2, ws[0], whs[0], bs[0], ws[1], whs[1], bs[1], lens,
                    "tanh")
    assert out.shape == (B, L, 2 * h)
    torch.testing.assert_close(out.float(), out_ref, atol=0.1, rtol=0.1)
    (out.float() ** 2).sum().backward()
    got = [x2.grad.float()] + [t.grad for t in ws + whs + bs]
    for g_, r_ in zip(got, ref_grads):
        torch.testing.assert_close(g_, r_, atol=0.5, rtol=0.2)
