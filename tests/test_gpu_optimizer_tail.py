"""GPU tests for the end of the training step: balanced sum of squares +
clip finisher, AdamW with the clip folded in and grad addresses passed by
value, and the graphed step that uses them instead of ``p.grad`` copies.

Tolerances:
* sum of squares: relative 1e-5 against a float64 reference (an fp32 sum
  of at most a few 1e5 non-negative terms, accumulated per thread, per
  block and once more in the finisher);
* coef: rtol 1e-6 against the torch formula on the kernel's own sumsq
  (sqrt, add, divide in fp32: at most a few ulps of 1.2e-7);
* everything else is bitwise (``torch.equal``): no atomics anywhere, and
  the fused load does the arithmetic of scale-then-load.
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

B1, B2, EPS = 0.9, 0.999, 1e-6


def _ext():
    from chinesener_amd import ops
    assert ops.ext_available(), "HIP extension not built"
    return ops.get_ext()


def _edge_specs(ext):
    """(dtype, numel, kind): vector tails, a chunk + 5, two chunks exactly,
    both dtypes, one entry without a gradient and one bf16 grad that is a
    contiguous slice starting at an odd element of a larger buffer."""
    ch = ext.sumsq_chunk_elems()
    specs = []
    for dt in (torch.bfloat16, torch.float32):
        for n in (1, 3, 4, 7, ch + 5, 2 * ch):
            specs.append((dt, n, "plain"))
    specs.insert(3, (torch.bfloat16, 300, "null"))
    specs.insert(9, (torch.bfloat16, 1001, "odd"))
    return specs


def _make_grads(specs, scale, seed):
    """Per spec: the raw grad (None for 'null'), generated once per seed."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    raw = []
    for dt, n, kind in specs:
        if kind == "null":
            raw.append(None)
        elif kind == "odd":
            buf = (torch.randn(n + 9, device="cuda", generator=g)
                   * scale).to(dt)
            raw.append(buf[1:n + 1])
        else:
            raw.append((torch.randn(n, device="cuda", generator=g)
                        * scale).to(dt))
    return raw


def _ready(raw, specs):
    from chinesener_amd.train.optimizers import kernel_ready_grad
    likes = [torch.empty(0, dtype=dt, device="cuda") for dt, _, _ in specs]
    return [kernel_ready_grad(g, p) for g, p in zip(raw, likes)]


def _sumsq_coef(ext, specs, grads, max_norm=1.0):
    numels = [n for _, n, _ in specs]
    isbf = [int(dt == torch.bfloat16) for dt, _, _ in specs]
    ref = torch.empty(1, device="cuda")
    chunks = ext.sumsq_build_chunks(numels, isbf, ref)
    return ext.multi_tensor_sumsq_coef_run(chunks, numels, isbf, grads,
                                           max_norm)


def _ref_sumsq(raw):
    return sum(float(g.double().pow(2).sum()) for g in raw if g is not None)


def _check_coef(out, max_norm):
    want = (max_norm / (out[0:1].sqrt() + 1e-6)).clamp(max=1.0)
    torch.testing.assert_close(out[1:2], want, rtol=1e-6, atol=0)


@pytest.mark.parametrize("scale,clips", [(1.0, True), (1e-3, False)])
def test_sumsq_and_finisher_edges(scale, clips):
    ext = _ext()
    specs = _edge_specs(ext)
    raw = _make_grads(specs, scale, seed=1)
    odd = [g for g, s in zip(raw, specs) if s[2] == "odd"][0]
    assert odd.is_contiguous() and odd.data_ptr() % 16 != 0
    grads = _ready(raw, specs)
    routed = [g for g, s in zip(grads, specs) if s[2] == "odd"][0]
    assert routed.data_ptr() % 16 == 0 and torch.equal(routed, odd)
    # the native entry refuses what the vector loads cannot take
    with pytest.raises(RuntimeError, match="aligned"):
        _sumsq_coef(ext, specs, raw)

    out = _sumsq_coef(ext, specs, grads)
    ref = _ref_sumsq(raw)
    got = float(out[0])
    print(f"sumsq {got!r} ref {ref!r} rel {abs(got - ref) / ref:.3e} "
          f"coef {float(out[1])!r}")
    assert abs(got - ref) <= 1e-5 * ref
    _check_coef(out, 1.0)
    if clips:
        assert ref > 1.0 and float(out[1]) < 1.0
    else:
        assert ref < 1.0 and float(out[1]) == 1.0
    again = _sumsq_coef(ext, specs, grads)
    assert torch.equal(out, again)


def _tiny_specs(ext):
    n = ext.grad_table_slots() + 3
    return [(torch.bfloat16 if i % 3 else torch.float32, i % 5 + 1, "plain")
            for i in range(n)]


def test_sumsq_more_tensors_than_slots():
    ext = _ext()
    specs = _tiny_specs(ext)
    raw = _make_grads(specs, 1.0, seed=2)
    out = _sumsq_coef(ext, specs, _ready(raw, specs), max_norm=2.0)
    ref = _ref_sumsq(raw)
    got = float(out[0])
    print(f"sumsq {got!r} ref {ref!r} rel {abs(got - ref) / ref:.3e}")
    assert abs(got - ref) <= 1e-5 * ref
    _check_coef(out, 2.0)
    assert torch.equal(out, _sumsq_coef(ext, specs, _ready(raw, specs), 2.0))


def _adam_state(specs, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    dt = specs[0][0]
    ps = [(torch.randn(n, device="cuda", generator=g) * 0.1).to(dt)
          for _, n, _ in specs]
    masters = ([p.float().clone() for p in ps]
               if dt == torch.bfloat16 else [])
    ms = [torch.zeros(n, device="cuda") for _, n, _ in specs]
    vs = [torch.zeros(n, device="cuda") for _, n, _ in specs]
    return ps, masters, ms, vs


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("which", ["edges", "over_capacity"])
def test_fused_adamw_equals_scale_then_adamw(dtype, which):
    ext = _ext()
    if which == "edges":
        specs = [s for s in _edge_specs(ext) if s[0] == dtype]
        if dtype == torch.float32:   # the fp32 list gets a null entry too
            specs.insert(2, (torch.float32, 300, "null"))
    else:
        specs = [(dtype, n, k) for _, n, k in _tiny_specs(ext)]
    n = len(specs)
    lrs = [1e-3 * (1 + i % 7) for i in range(n)]
    wds = [0.01 * (i % 3) for i in range(n)]
    coef = torch.tensor([0.37], device="cuda")
    lr_mul = torch.tensor([0.5], device="cuda")

    old = _adam_state(specs, seed=3)
    new = copy.deepcopy(old)
    blob, info = ext.adamw_build_meta(new[0], [], new[1], new[2], new[3],
                                      lrs, wds)
    total, cnt, isbf = info.tolist()
    assert cnt == n and bool(isbf) == (dtype == torch.bfloat16)
    for step in range(3):
        raw = _make_grads(specs, 1.0, seed=10 + step)
        # old path: scale a copy in place, then the blob-less entry; the
        # parameter without a gradient is fed a zero grad
        scaled = [torch.zeros(s[1], dtype=dtype, device="cuda")
                  if g is None else g.clone() for g, s in zip(raw, specs)]
        ext.multi_tensor_scale(scaled, coef)
        ext.multi_tensor_adamw(old[0], scaled, old[1], old[2], old[3], lrs,
                               wds, B1, B2, EPS, lr_mul)
        ext.multi_tensor_adamw_tab_run(blob, total, cnt, bool(isbf), new[0],
                                       _ready(raw, specs), B1, B2, EPS,
                                       lr_mul, coef)
    torch.cuda.synchronize()
    for name, a, b in zip(("p", "master", "m", "v"), old, new):
        assert len(a) == len(b)
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), (name, i, specs[i])
    assert any(float(v.abs().max()) > 0 for v in new[3])


class _Out:
    def __init__(self, loss):
        self.loss = loss


class _TailNet(torch.nn.Module):
    """torch-only, so the backward is deterministic: two bf16 Linear, an
    fp32 LayerNorm, and one parameter the loss does not use."""

    def __init__(self):
        super().__init__()
        self.lin1 = torch.nn.Linear(32, 32).to(torch.bfloat16)
        self.lin2 = torch.nn.Linear(32, 32).to(torch.bfloat16)
        self.ln_out = torch.nn.LayerNorm(32)
        self.unused = torch.nn.Parameter(torch.randn(5))

    def forward(self, batch):
        h = torch.relu(self.lin1(batch["x"].to(torch.bfloat16)))
        y = self.ln_out(self.lin2(h).float() + batch["x"])
        return _Out((y * batch["x"]).pow(2).sum())


def _run_graphed(monkeypatch, mode, init, batches):
    from chinesener_amd.train.graph_step import GraphedTrainStep
    from chinesener_amd.train.optimizers import (
        AdamWeightDecay, LrSchedule, build_param_groups, clip_gradients)
    if mode == "off":
        monkeypatch.setenv("CHINESENER_FUSED_TAIL", "off")
    else:
        monkeypatch.delenv("CHINESENER_FUSED_TAIL", raising=False)
    model = _TailNet().cuda()
    model.load_state_dict(init)
    opt = AdamWeightDecay(build_param_groups(model, 1e-3, 0.01), lr=1e-3)
    sched = LrSchedule("bert", 1e-3, num_train_steps=100, warmup_steps=1)
    seen = []
    g = GraphedTrainStep(
        model, opt, sched,
        lambda m: seen.append(clip_gradients(m, "bert")))
    assert g.try_capture(batches[0], step=1)
    for s, b in enumerate(batches, start=1):
        g.replay(b, s)
    torch.cuda.synchronize()
    sumsq = float(seen[-1])           # the captured node's last replay
    params = {k: v.detach().clone() for k, v in model.named_parameters()}
    state = {k: {n: t.clone() for n, t in opt.state[p].items()}
             for k, p in model.named_parameters()}
    has_grad = [p.grad is not None for p in model.parameters()]
    g.release()
    return params, state, has_grad, sumsq


def test_graphed_step_fused_equals_off(monkeypatch):
    """Both modes take their norm from the new sum-of-squares kernel over
    the same chunk list (off mode runs it on the copied ``p.grad``), so
    coef is bitwise the same and the comparison is ``torch.equal``."""
    _ext()
    torch.manual_seed(0)
    init = copy.deepcopy(_TailNet().state_dict())
    gen = torch.Generator().manual_seed(4)
    batches = [{"x": (torch.randn(8, 32, generator=gen) * 3).cuda()}
               for _ in range(3)]
    fp, fs, fgrad, fsumsq = _run_graphed(monkeypatch, "fused", init, batches)
    op, os_, ograd, osumsq = _run_graphed(monkeypatch, "off", init, batches)
    print(f"sumsq fused {fsumsq!r} off {osumsq!r}")
    assert fsumsq > 1.0 and fsumsq == osumsq      # the clip is active
    assert not any(fgrad), "fused mode must not allocate p.grad"
    assert all(ograd), "off mode fills persistent p.grad buffers"
    for k in fp:
        assert torch.equal(fp[k], op[k]), k
        assert fs[k].keys() == os_[k].keys(), k
        for n in fs[k]:
            assert torch.equal(fs[k][n], os_[k][n]), (k, n)
    # the step did something, and the unused parameter only decayed
    assert not torch.equal(fp["lin1.weight"], init["lin1.weight"].cuda())
    assert float(fs["unused"]["m"].abs().max()) == 0.0
    assert not torch.equal(fp["unused"], init["unused"].cuda())
