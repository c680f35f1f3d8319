"""The rounding model of the TENER kernel (ops.reference.tener_attention_model)
and the acceptance rule that every TENER comparison uses, checked without a
GPU.

The rule (per tensor and per (b, h) slice; per head for du and dvb):

    e_kernel <= C_TENER * e_model + 2^-8 * max(s, 1)

with e_kernel = max|X_kernel - X_fp64|, e_model = max|X_model - X_fp64| and
s = max|X_fp64|. Inputs are bf16 values handed to every side, X_fp64 is
ops.reference.tener_attention in fp64, X_model the rounding model. The floor
is half a bf16 ulp at the result's scale (bf16 keeps 8 significant bits), the
output format itself; it carries the slices on which the model is exact.
C_TENER is measured on the GPU against the model, see
profiles/tener_tests.md.

tests/test_gpu_tener_edges.py imports the rule, the input builders and
C_TENER from here, so the mutation check below is a check of the very rule
the kernel is held to."""
import pytest
import torch

from chinesener_amd.ops import reference as ref

# kernel error / model error: the next power of two above the largest ratio
# measured over the sweep of tests/test_gpu_tener_edges.py on an MI355X,
# which is 1.00 (profiles/tener_tests.md)
C_TENER = 2.0
FLOOR = 2.0 ** -8
NAMES = ("out", "dq", "dk", "dv", "du", "dvb")


# ------------------------------------------------------------------ inputs
def make_inputs(B, H, L, D, table, seed, qk_std=0.5, device="cpu"):
    """bf16 q, k, v, u, vb, rel, dout, drawn in fp32 on the CPU (so a GPU run
    sees the same values) and rounded once. table: "random" is randn(2L, D),
    "sinus" is ref.relative_table(L, D)."""
    g = torch.Generator().manual_seed(seed)

    def draw(*shape, std=1.0):
        return (torch.randn(*shape, generator=g) * std).to(torch.bfloat16)

    inp = {
        "q": draw(B, H, L, D, std=qk_std), "k": draw(B, H, L, D, std=qk_std),
        "v": draw(B, H, L, D), "u": draw(H, D, std=0.1),
        "vb": draw(H, D, std=0.1),
        "rel": (draw(2 * L, D) if table == "random"
                else ref.relative_table(L, D).to(torch.bfloat16)),
        "dout": draw(B, H, L, D),
    }
    return {n: t.to(device) for n, t in inp.items()}


def sweep_lens(L):
    return [L, max(1, L // 2 + 1), 1]


def mask_of(lens, L, device="cpu"):
    lens = torch.as_tensor(lens, device=device)
    return (torch.arange(L, device=device)[None, :] < lens[:, None]).long()


def selection_inputs(L, device="cpu"):
    """Inputs on which head h attends to key i + delta_h and nothing else:
    q = u = 0, vb[h] = e_h, rel[m, h] = 30 at m = L-1+delta_h and 0 elsewhere
    (the other columns of rel are random), so a score is 30 on the target key
    and 0 on every other; exp(-30) vanishes against 1 in fp32. v rows are
    pairwise distinct, bf16-exact, entries in [1, 2). Returns (inputs, deltas,
    lens)."""
    B, H, D = 2, 5, 20
    g = torch.Generator().manual_seed(1000 + L)
    deltas = [-(L - 1), -1, 0, 1, L - 1]
    q = torch.zeros(B, H, L, D)
    k = torch.randn(B, H, L, D, generator=g)
    u = torch.zeros(H, D)
    vb = torch.zeros(H, D)
    rel = torch.randn(2 * L, D, generator=g)
    rel[:, :H] = 0.0
    for h, d in enumerate(deltas):
        vb[h, h] = 1.0
        rel[L - 1 + d, h] = 30.0
    # multiples of 1/128 in [1, 2) are bf16-exact; columns 0 and 1 number the
    # row, so no two rows of a (b, h) slice are equal
    v = 1.0 + torch.randint(0, 128, (B, H, L, D), generator=g) / 128.0
    j = torch.arange(L)
    v[..., 0] = 1.0 + (j % 128) / 128.0
    v[..., 1] = 1.0 + (j // 128) / 128.0
    inp = {"q": q, "k": k, "v": v, "u": u, "vb": vb, "rel": rel,
           "dout": torch.randn(B, H, L, D, generator=g)}
    inp = {n: t.to(torch.bfloat16).to(device) for n, t in inp.items()}
    return inp, deltas, [L, L // 2]


# -------------------------------------------------------------- references
def variant64(inp, mask, shift=0, flip=False, mask_delta=0, u_scale=1.0,
              vb_scale=1.0):
    """TENER attention and its gradients in fp64 by autograd, with optional
    defects: the gather offset moved by `shift` or mirrored (`flip`), the key
    mask longer or shorter by `mask_delta`, u or vb scaled. With no defect
    this is ops.reference.tener_attention (asserted below)."""
    leaves = {n: inp[n].double().requires_grad_()
              for n in ("q", "k", "v", "u", "vb")}
    q, k, v, u, vb = (leaves[n] for n in ("q", "k", "v", "u", "vb"))
    rel = inp["rel"].double()
    B, H, L, D = q.shape
    ar = torch.arange(L, device=q.device)
    rel_pos = ar[None, :] - ar[:, None]
    idx = ((-rel_pos if flip else rel_pos) + (L - 1) + shift).clamp(
        0, 2 * L - 1)
    s = torch.matmul(q + u_scale * u[None, :, None, :], k.transpose(-1, -2))
    bd = torch.matmul(q + vb_scale * vb[None, :, None, :], rel.t())
    s = s + bd.gather(-1, idx.expand(B, H, L, L))
    if mask is not None:
        lens = (mask.long().sum(1) + mask_delta).clamp(1, L)
        valid = (ar[None, :] < lens[:, None])[:, None, None, :]
        s = torch.where(valid, s, torch.full_like(s, ref.NEG_INF))
    out = torch.matmul(torch.softmax(s, -1), v)
    out.backward(inp["dout"].double())
    return (out.detach(),) + tuple(leaves[n].grad
                                   for n in ("q", "k", "v", "u", "vb"))


def reference64(inp, mask):
    """ops.reference.tener_attention in fp64 on the bf16 values; returns
    (out, dq, dk, dv, du, dvb)."""
    leaves = [inp[n].double().requires_grad_()
              for n in ("q", "k", "v", "u", "vb")]
    out = ref.tener_attention(*leaves, inp["rel"].double(), mask)
    out.backward(inp["dout"].double())
    return (out.detach(),) + tuple(t.grad for t in leaves)


def model(inp, mask):
    return ref.tener_attention_model(inp["q"], inp["k"], inp["v"], inp["u"],
                                     inp["vb"], inp["rel"], mask, inp["dout"])


# -------------------------------------------------------------------- rule
def slice_errors(x, x_model, x64, items):
    """(e_kernel, e_model, s) per (b, h) slice of the batch items `items`
    for a [B,H,L,D] tensor, per head for an [H,D] one."""
    x, x_model, x64 = (t.detach().double() for t in (x, x_model, x64))
    if x64.dim() == 4:
        x, x_model, x64 = x[items], x_model[items], x64[items]
        dims = (2, 3)
    else:
        dims = (1,)
    return ((x - x64).abs().amax(dims), (x_model - x64).abs().amax(dims),
            x64.abs().amax(dims))


def rule_failures(got, mdl, r64, lens, c=None, label="", report=None):
    """Apply the rule to the six tensors; batch items of length 0 are left
    out of the per-slice tensors. Prints every figure, returns the names of
    the tensors with a failing slice. `report`, a dict, collects per tensor
    the largest e_kernel/e_model (over slices whose model error is at least
    the floor, where the ratio means something) and the largest c that a
    slice would have needed."""
    c = C_TENER if c is None else c
    items = [b for b, n in enumerate(lens) if n >= 1]
    failed = []
    for name, x, xm, x64 in zip(NAMES, got, mdl, r64):
        assert x.shape == x64.shape, (name, x.shape, x64.shape)
        assert torch.isfinite(x.double()).all(), name
        e_k, e_m, s = slice_errors(x, xm, x64, items)
        floor = FLOOR * s.clamp(min=1.0)
        ok = e_k <= c * e_m + floor
        big = e_m >= floor
        ratio = float((e_k[big] / e_m[big]).max()) if big.any() else 0.0
        excess = (e_k - floor).clamp(min=0.0)
        need = torch.where(excess > 0, excess / e_m, torch.zeros_like(e_m))
        need = float(need.max())
        print(f"TENER {label} {name}: e_kernel {float(e_k.max()):.3e} "
              f"e_model {float(e_m.max()):.3e} scale {float(s.max()):.3e} "
              f"ratio {ratio:.3f} c_needed {need:.3f} "
              f"{'ok' if bool(ok.all()) else 'FAIL'}")
        if report is not None:
            old = report.get(name, (0.0, 0.0))
            report[name] = (max(old[0], ratio), max(old[1], need))
        if not bool(ok.all()):
            failed.append(name)
    return failed


# ------------------------------------------------------------------- tests
def test_variant_without_defect_is_the_reference():
    L = 37
    inp = make_inputs(2, 3, L, 20, "random", seed=1)
    mask = mask_of([L, 11], L)
    for a, b in zip(variant64(inp, mask), reference64(inp, mask)):
        torch.testing.assert_close(a, b, atol=1e-12, rtol=1e-12)


def test_model_within_existing_bounds_at_existing_shape():
    """Sanity of the model: at the shape of test_gpu_kernels.test_tener_fwd_bwd
    (sinusoidal table, upstream gradient masked as there) it sits inside
    that test's absolute bounds, by a wide margin."""
    B, H, L, D = 2, 2, 150, 20
    lens = [L, 97]
    inp = make_inputs(B, H, L, D, "sinus", seed=4)
    mask = mask_of(lens, L)
    inp["dout"] = inp["dout"] * mask[:, None, :, None].to(torch.bfloat16)
    mdl, r64 = model(inp, mask), reference64(inp, mask)
    row = mask[:, None, :, None].double()
    bounds = dict(out=0.12, dq=0.25, dk=0.25, dv=0.25, du=1.0, dvb=1.0)
    for name, xm, x64 in zip(NAMES, mdl, r64):
        w = row if name == "out" else 1.0
        err = float(((xm - x64) * w).abs().max())
        print(f"model vs fp64, {name}: {err:.4f} (bound {bounds[name]})")
        assert err <= bounds[name], name
        assert xm.dtype == torch.float64
        assert torch.equal(xm, xm.to(torch.bfloat16).double()), name


def test_model_follows_empty_and_unmasked_items():
    """mask=None equals an all-ones mask; an empty item is finite in the
    forward and has zero gradients."""
    L = 19
    inp = make_inputs(3, 2, L, 8, "random", seed=2)
    full = model(inp, mask_of([L, L, L], L))
    for a, b in zip(model(inp, None), full):
        assert torch.equal(a, b)
    inp["dout"][1] = 0
    out, dq, dk, dv, du, dvb = model(inp, mask_of([L, 0, 1], L))
    for t in (out, dq, dk, dv, du, dvb):
        assert torch.isfinite(t).all()
    for t in (dq, dk, dv):
        assert not t[1].any()


MUTANTS = {
    "offset+1": dict(shift=1),
    "offset-1": dict(shift=-1),
    "offset_sign": dict(flip=True),
    "mask+1": dict(mask_delta=1),
    "mask-1": dict(mask_delta=-1),
    "no_u": dict(u_scale=0.0),
    "no_vb": dict(vb_scale=0.0),
    "half_u": dict(u_scale=0.5),
}


@pytest.fixture(scope="module")
def largest_shape():
    """The sweep's largest shape (B = H = 3, L = 160, D = 32), random table:
    inputs, mask, lens, model and fp64 reference, computed once."""
    L = 160
    lens = sweep_lens(L)
    inp = make_inputs(3, 3, L, 32, "random", seed=160)
    mask = mask_of(lens, L)
    return inp, mask, lens, model(inp, mask), reference64(inp, mask)


def test_rule_accepts_the_model_itself(largest_shape):
    inp, mask, lens, mdl, r64 = largest_shape
    assert rule_failures(mdl, mdl, r64, lens, label="model") == []


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_rule_rejects_mutant(largest_shape, name):
    """The fp64 reference with one defect, in the place of the kernel, must
    fail the rule on at least one tensor."""
    inp, mask, lens, mdl, r64 = largest_shape
    bad = variant64(inp, mask, **MUTANTS[name])
    failed = rule_failures(bad, mdl, r64, lens, label=f"mutant {name}")
    assert failed, f"the rule accepts the defect {name}"


@pytest.mark.parametrize("L", [17, 160])
def test_model_exact_on_key_selection(L):
    """On the key-selection inputs the model returns the selected row of v
    bit for bit, so the GPU case may ask the same of the kernel."""
    inp, deltas, lens = selection_inputs(L)
    out = model(inp, mask_of(lens, L))[0]
    v = inp["v"].double()
    checked = 0
    for b, n in enumerate(lens):
        for h, d in enumerate(deltas):
            rows = [i for i in range(L) if 0 <= i + d < n]
            for i in rows:
                assert torch.equal(out[b, h, i], v[b, h, i + d]), (b, h, i)
            checked += len(rows)
    assert checked >= 3 * lens[1]
