"""CPU-side checks of the optimizer-tail hand-off: grad routing for the
by-value kernels, the publish/take protocol around ``clip_gradients`` and
the conditions under which GraphedTrainStep keeps filling ``p.grad``.
(The kernels themselves: tests/test_gpu_optimizer_tail.py.)"""
import torch

from chinesener_amd.train import optimizers as O
from chinesener_amd.train.graph_step import GraphedTrainStep


def test_kernel_ready_grad_routes():
    p = torch.zeros(8, dtype=torch.bfloat16)
    assert O.kernel_ready_grad(None, p) is None
    good = torch.ones(8, dtype=torch.bfloat16)
    assert good.data_ptr() % 16 == 0
    assert O.kernel_ready_grad(good, p) is good          # untouched
    wrong_dtype = torch.ones(8)
    r = O.kernel_ready_grad(wrong_dtype, p)
    assert r.dtype == torch.bfloat16 and r.is_contiguous()
    strided = torch.arange(16.).to(torch.bfloat16)[::2]
    r = O.kernel_ready_grad(strided, p)
    assert r.is_contiguous() and torch.equal(r, strided)
    odd = torch.arange(17.).to(torch.bfloat16)[1:9]      # contiguous, +2 B
    assert odd.is_contiguous() and odd.data_ptr() % 16 != 0
    r = O.kernel_ready_grad(odd, p)
    assert r.data_ptr() % 16 == 0 and torch.equal(r, odd)


def test_publication_is_withdrawn_when_not_consumed():
    m = torch.nn.Linear(2, 2)
    ps = list(m.parameters())
    O.publish_step_grads(m, ps, [torch.ones_like(p) for p in ps])
    # value clipping never consumes a publication: it clips p.grad
    for p in ps:
        p.grad = torch.full_like(p, 9.0)
    O.clip_gradients(m, "custom")
    assert all(float(p.grad.max()) == 5.0 for p in ps)
    assert O.take_step_coef(m) is None
    assert m._step_grads is None and m._step_coef is None
    assert O.take_step_coef(m) is None                   # idempotent


def test_fused_tail_needs_gpu_adamw_and_switch(monkeypatch):
    m = torch.nn.Linear(2, 2)
    opt = O.AdamWeightDecay(O.build_param_groups(m, 1e-3, 0.01))
    g = GraphedTrainStep(m, opt, None, lambda mm: None)
    assert not g._fused_tail()                           # CPU params
    sgd = torch.optim.SGD(m.parameters(), lr=0.1)
    assert not GraphedTrainStep(m, sgd, None, lambda mm: None)._fused_tail()
    monkeypatch.setenv("CHINESENER_FUSED_TAIL", "off")
    assert not O.fused_tail_enabled()
    monkeypatch.delenv("CHINESENER_FUSED_TAIL")
    assert O.fused_tail_enabled()
