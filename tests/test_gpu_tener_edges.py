"""csrc/tener.hip at its edges, through ops.tener_attention: rows that are
mostly padding, every Lpad step up to the 160-row limit, head dims 1 to 32,
one-token and empty items, mask=None, the model's own head count and call
layout, both ends of the relative table, and the fallback.

Every comparison uses the rule of tests/test_tener_model_cpu.py,

    e_kernel <= C_TENER * e_model + 2^-8 * max(s, 1)

per tensor and (b, h) slice (per head for du, dvb), against
ops.reference.tener_attention in fp64 on the same bf16 values, with the
rounding model ops.reference.tener_attention_model as the yardstick.
C_TENER and the measured ratios are in profiles/tener_tests.md; that file's
CPU half checks that the rule rejects eight wrong variants of the reference.
The upstream gradient is not masked: the kernel computes query rows past
len exactly as the reference does. The fp64 reference and the model run on
the GPU in fp64; each figure is printed before it is asserted."""
import pytest
import torch

from chinesener_amd import ops
from chinesener_amd.ops import reference as ref

from test_gpu_kernels import _cuda
from test_tener_model_cpu import (make_inputs, mask_of, model, reference64,
                                  rule_failures, selection_inputs, sweep_lens)

pytestmark = pytest.mark.gpu

SWEEP_L = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 129, 144, 145, 159,
           160]
SWEEP = ([(L, 20) for L in SWEEP_L]
         + [(L, D) for L in (17, 160) for D in (1, 8, 32)])


def run_kernel(inp, mask):
    """ops.tener_attention forward and backward on bf16 leaves; returns
    (out, dq, dk, dv, du, dvb)."""
    leaves = [inp[n].clone().requires_grad_()
              for n in ("q", "k", "v", "u", "vb")]
    out = ops.tener_attention(*leaves, inp["rel"], mask)
    assert out.dtype == torch.bfloat16 and out.shape == inp["q"].shape
    out.backward(inp["dout"])
    for t in leaves:
        assert t.grad.dtype == torch.bfloat16
    return (out.detach(),) + tuple(t.grad for t in leaves)


def check(inp, lens, label):
    L = inp["q"].shape[2]
    m = mask_of(lens, L, "cuda")
    got = run_kernel(inp, m)
    failed = rule_failures(got, model(inp, m), reference64(inp, m), lens,
                           label=label)
    assert not failed, f"{label}: {failed} outside the rule"
    return got


# ------------------------------------------------------------- shape sweep
@pytest.mark.parametrize("table", ["random", "sinus"])
@pytest.mark.parametrize("L,D", SWEEP)
def test_tener_shape_sweep(L, D, table):
    _cuda()
    inp = make_inputs(3, 3, L, D, table, seed=L * 64 + D, device="cuda")
    check(inp, sweep_lens(L), f"sweep L={L} D={D} {table}")


@pytest.mark.parametrize("table", ["random", "sinus"])
def test_tener_model_shape(table):
    """The encoder's own shape: 8 heads of 20, batch 4, L = 150."""
    _cuda()
    inp = make_inputs(4, 8, 150, 20, table, seed=150, device="cuda")
    check(inp, [150, 97, 33, 1], f"model-shape {table}")


@pytest.mark.parametrize("std", [0.5, 1.0, 2.0])
def test_tener_score_scale(std):
    """Unscaled attention at D = 32: score std about 1.4, 5.7 and 22. BD's
    bf16 rounding grows with the scores; the model's error grows with it and
    the rule must keep holding."""
    _cuda()
    inp = make_inputs(3, 3, 96, 32, "random", seed=int(std * 10),
                      qk_std=std, device="cuda")
    check(inp, sweep_lens(96), f"score-scale std={std}")


# ----------------------------------------------------- exact key selection
@pytest.mark.parametrize("L", [17, 160])
def test_tener_exact_key_selection(L):
    """Head h attends to key i + delta_h alone, delta = -(L-1), -1, 0, +1,
    L-1: table rows m = 0 and m = 2L-2 are each the one hot entry of a head,
    so a wrong end of the table or a mirrored offset returns another row of
    v. No tolerance: the model is exact on these inputs (CPU test)."""
    _cuda()
    inp, deltas, lens = selection_inputs(L, "cuda")
    out = ops.tener_attention(inp["q"], inp["k"], inp["v"], inp["u"],
                              inp["vb"], inp["rel"], mask_of(lens, L, "cuda"))
    checked = 0
    for b, n in enumerate(lens):
        for h, d in enumerate(deltas):
            lo, hi = max(0, -d), min(L, n - d)        # rows with 0 <= i+d < n
            if hi <= lo:
                continue
            want = inp["v"][b, h, lo + d:hi + d]
            assert torch.equal(out[b, h, lo:hi], want), (b, h, d)
            checked += hi - lo
    assert checked >= 3 * lens[1]


# ------------------------------------------------- the model's call layout
@pytest.mark.parametrize("masked", [True, False])
def test_tener_layer_call_layout(masked):
    """As TenerLayer calls it under autocast: q and v are transposed views of
    one [B, L, 2, H, D] bf16 projection, k is a view of the fp32 layer input,
    rel, u and vb are fp32. The gradients reach the two leaves in their own
    dtypes and pass the rule."""
    _cuda()
    B, H, L, D = 3, 3, 45, 20
    lens = sweep_lens(L) if masked else [L] * B
    inp = make_inputs(B, H, L, D, "random", seed=45, device="cuda")
    mask = mask_of(lens, L, "cuda") if masked else None

    qv = torch.stack([inp["q"].transpose(1, 2), inp["v"].transpose(1, 2)],
                     dim=2).contiguous().requires_grad_()      # [B,L,2,H,D]
    x = inp["k"].transpose(1, 2).reshape(B, L, H * D).float().requires_grad_()
    u = inp["u"].float().requires_grad_()
    vb = inp["vb"].float().requires_grad_()
    q, v = qv[:, :, 0].transpose(1, 2), qv[:, :, 1].transpose(1, 2)
    k = x.reshape(B, L, H, D).transpose(1, 2)
    assert not q.is_contiguous() and not k.is_contiguous()
    out = ops.tener_attention(q, k, v, u, vb, inp["rel"].float(), mask)
    out.backward(inp["dout"])

    assert qv.grad.dtype == torch.bfloat16 and qv.grad.shape == qv.shape
    assert x.grad.dtype == torch.float32 and x.grad.shape == x.shape
    assert u.grad.dtype == torch.float32 and vb.grad.dtype == torch.float32
    got = (out.detach(), qv.grad[:, :, 0].transpose(1, 2),
           x.grad.reshape(B, L, H, D).transpose(1, 2),
           qv.grad[:, :, 1].transpose(1, 2), u.grad, vb.grad)
    failed = rule_failures(got, model(inp, mask), reference64(inp, mask),
                           lens, label=f"layer-layout masked={masked}")
    assert not failed, failed


# ---------------------------------------- empty rows, independence, repeats
def _alone(inp, b, n):
    """Batch item b on its own."""
    one = {name: (t[b:b + 1] if t.dim() == 4 else t)
           for name, t in inp.items()}
    L = inp["q"].shape[2]
    return run_kernel(one, mask_of([n], L, "cuda"))


@pytest.mark.parametrize("L", [17, 160])
def test_tener_empty_and_one_token_items(L):
    """lens = [L, 0, 1] with a zero upstream gradient on the empty item:
    everything is finite, the empty item's dq, dk, dv are exactly zero, the
    other items pass the rule, and every item alone is bitwise the item in
    the batch."""
    _cuda()
    lens = [L, 0, 1]
    inp = make_inputs(3, 3, L, 20, "random", seed=7000 + L, device="cuda")
    inp["dout"][1] = 0
    got = check(inp, lens, f"empty-item L={L}")
    for name, t in zip(("out", "dq", "dk", "dv", "du", "dvb"), got):
        assert torch.isfinite(t.float()).all(), name
    for name, t in zip(("dq", "dk", "dv"), got[1:4]):
        assert not t[1].any(), f"{name} of the empty item"
    for b, n in enumerate(lens):
        for name, t, t1 in zip(("out", "dq", "dk", "dv"), got,
                               _alone(inp, b, n)):
            assert torch.equal(t[b:b + 1], t1), (name, b)


@pytest.mark.parametrize("L", [33, 145])
def test_tener_block_independence_and_reproducibility(L):
    """Beside the fp64 comparison of the same call: an item alone gives
    bitwise the out, dq, dk, dv it gives inside the batch (a block reads
    nothing of another's), and a second run of the call is bitwise the
    first, du and dvb included."""
    _cuda()
    lens = sweep_lens(L)
    inp = make_inputs(3, 3, L, 20, "random", seed=9000 + L, device="cuda")
    got = check(inp, lens, f"independence L={L}")
    again = run_kernel(inp, mask_of(lens, L, "cuda"))
    for name, a, b_ in zip(("out", "dq", "dk", "dv", "du", "dvb"), got,
                           again):
        assert torch.equal(a, b_), f"{name} differs between two runs"
    for b, n in enumerate(lens):
        for name, t, t1 in zip(("out", "dq", "dk", "dv"), got,
                               _alone(inp, b, n)):
            assert torch.equal(t[b:b + 1], t1), (name, b)


# ---------------------------------------------------------------- fallback
@pytest.mark.parametrize("L,D,dtype", [(161, 20, torch.bfloat16),
                                       (64, 40, torch.bfloat16),
                                       (64, 20, torch.float32)])
def test_tener_fallback_is_the_reference(L, D, dtype):
    """Past the kernel's limits (L > 160, D > 32, or fp32 q) the op is the
    reference itself, on the GPU, and does not raise."""
    _cuda()
    inp = make_inputs(2, 3, L, D, "random", seed=L + D, device="cuda")
    args = [inp[n].to(dtype) for n in ("q", "k", "v", "u", "vb", "rel")]
    mask = mask_of([L, L // 2], L, "cuda")
    out = ops.tener_attention(*args, mask)
    want = ref.tener_attention(*args, mask)
    assert out.dtype == dtype and torch.isfinite(out.float()).all()
    assert torch.equal(out, want)
