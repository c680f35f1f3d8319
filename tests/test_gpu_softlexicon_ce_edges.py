"""csrc/softlexicon.hip and masked_ce_fwd/bwd of csrc/elementwise.hip at their
edges, against fp64 references.

softlexicon (one wave per token, 4 waves per block, lanes own columns):
token counts of every N % 4, E = 1, 7, 50 and 64, a two-row table whose
rows take about 20 N atomic adds each, weights as build_soft_lexicon pads
them (weight 0, id 0), a bf16 table, and the host check at E = 65. The
bounds are derived from the arithmetic, with eps = 2^-24 (fp32 unit
roundoff); a sum of n fp32 terms in any order is within (n-1) eps sum|x| of
the exact one (to first order), and the leading 2 covers the rounding of
each product and the second-order terms:

    out      10 products summed into a zero:         2 * 11 * eps * sum_s |w_s table[id_s, e]|
    dweights E <= 64 products through a 6-step
             butterfly over 64 lanes:                2 * (E + 6) * eps * sum_e |g_e table[id, e]|
    dtable   n atomic adds into a zero, n counted
             from ids:                               2 * (n + 1) * eps * sum |w g|

masked CE (one thread per row, 256 rows per block, loss and nvalid summed
across blocks by atomics): one, two, three and five blocks, T = 1, 2, 10 and
64, an all-masked batch, one valid row in the last block, logits times 40
and bf16 logits. Tolerance: CE_FACTOR times the error of the fp32
reference (CPU) against the fp64 one on the same inputs, plus 2^-23 |value|;
the factor is for __expf/__logf and the atomic summation order, the measured
ratio is in profiles/tener_tests.md."""
import pytest
import torch

from chinesener_amd import ops
from chinesener_amd.ops import reference as ref

from test_gpu_kernels import _cuda

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24
# bf16 keeps 8 significant bits: for |x| in [2^k, 2^(k+1)) half an ulp is
# 2^(k-8) <= 2^-8 |x|
HALF_ULP_BF16 = 2.0 ** -8
CE_FACTOR = 4.0


# ------------------------------------------------------------- softlexicon
def _lexicon_case(B, L, E, V, seed, padded=False):
    """table [V,E], int64 ids and weights [B,L,40], upstream gradient.
    padded: as build_soft_lexicon leaves them: id 0 is the pad word and is
    used with weight 0 only, most slots are padding, every third token has no
    word at all."""
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(V, E, generator=g)
    w = torch.rand(B, L, 40, generator=g)
    if padded:
        ids = torch.randint(1, V, (B, L, 40), generator=g)
        real = torch.rand(B, L, 40, generator=g) < 0.2
        real[:, ::3] = False
        ids = ids * real
        w = w * real
        w = w / w.sum(-1, keepdim=True).clamp(min=1e-30)
    else:
        ids = torch.randint(0, V, (B, L, 40), generator=g)
    dout = torch.randn(B, L, 4 * E, generator=g)
    return tuple(t.cuda() for t in (table, ids, w, dout))


def _lexicon_check(table, ids, w, dout, label):
    """Run the op on (table, ids, w), compare out and both gradients with
    ref.softlexicon_fuse in fp64 under the derived bounds. bf16 inputs add
    half a bf16 ulp of the rounded result."""
    B, L, _ = ids.shape
    V, E = table.shape
    dt = table.dtype
    t64 = table.double().requires_grad_()
    w64 = w.double().requires_grad_()
    g64 = dout.double()
    out64 = ref.softlexicon_fuse(t64, ids, w64)
    out64.backward(g64)

    emb = t64.detach()[ids]                                     # [B,L,40,E]
    wv = w64.detach()[..., None]
    g_slot = g64.view(B, L, 4, 1, E).expand(B, L, 4, 10, E).reshape(
        B, L, 40, E)
    b_out = 2 * 11 * EPS32 * (emb * wv).abs().view(B, L, 4, 10, E).sum(
        3).reshape(B, L, 4 * E)
    b_dw = 2 * (E + 6) * EPS32 * (emb * g_slot).abs().sum(-1)
    flat = ids.reshape(-1)
    n = torch.bincount(flat, minlength=V).double()[:, None]
    b_dt = 2 * (n + 1) * EPS32 * torch.zeros(V, E, dtype=torch.float64,
                                             device="cuda").index_add_(
        0, flat, (wv * g_slot).abs().reshape(-1, E))

    t2 = table.clone().requires_grad_()
    w2 = w.clone().requires_grad_()
    out = ops.softlexicon_fuse(t2, ids, w2)
    assert out.dtype == dt and out.shape == (B, L, 4 * E)
    out.backward(dout)
    assert t2.grad.dtype == dt and w2.grad.dtype == w.dtype
    worst = {}
    for name, x, x64, bound in (("out", out, out64, b_out),
                                ("dweights", w2.grad, w64.grad, b_dw),
                                ("dtable", t2.grad, t64.grad, b_dt)):
        x64 = x64.detach()
        if x.dtype == torch.bfloat16:
            bound = bound + HALF_ULP_BF16 * (x64.abs() + bound)
        err = (x.detach().double() - x64).abs()
        over = err > bound
        worst[name] = float((err / bound.clamp(min=1e-300)).max())
        print(f"softlexicon {label} {name}: max err {float(err.max()):.3e} "
              f"max err/bound {worst[name]:.3f}")
        assert torch.isfinite(x.float()).all(), name
        assert not over.any(), (f"{label} {name}: {int(over.sum())} elements "
                                f"over the bound, worst {worst[name]:.2f}x")
    return t2.grad, w2.grad


@pytest.mark.parametrize("E", [1, 7, 50, 64])
@pytest.mark.parametrize("B,L", [(1, 1), (1, 5), (3, 7), (1, 83)])
def test_softlexicon_shapes(B, L, E):
    """N = 1, 5, 21, 83 tokens: every N % 4, so the last block has one, two
    and three idle waves; E = 64 has every lane live, E = 1 one."""
    _cuda()
    _lexicon_check(*_lexicon_case(B, L, E, 37, seed=B * L * 100 + E),
                   label=f"N={B * L} E={E}")


def test_softlexicon_two_row_table():
    """V = 2: each table row takes about 20 N atomic adds per column."""
    _cuda()
    _lexicon_check(*_lexicon_case(1, 83, 50, 2, seed=2), label="V=2")


@pytest.mark.parametrize("B,L,E", [(3, 7, 50), (1, 83, 64)])
def test_softlexicon_padded_slots(B, L, E):
    """Padding slots (weight 0, id 0) add nothing: the pad row of dtable is
    exactly zero, a token without words gives an exactly zero output, and
    dweights of a padding slot is still the dot product with the pad row."""
    _cuda()
    table, ids, w, dout = _lexicon_case(B, L, E, 23, seed=E, padded=True)
    assert (w == 0).float().mean() > 0.7 and (w[:, ::3] == 0).all()
    dtable, dweights = _lexicon_check(table, ids, w, dout,
                                      label=f"padded N={B * L} E={E}")
    assert not dtable[0].any(), "zero-weight slots reached dtable"
    assert dweights[w == 0].abs().max() > 0.1
    out = ops.softlexicon_fuse(table, ids, w)
    assert not out[:, ::3].any()


@pytest.mark.parametrize("padded", [False, True])
def test_softlexicon_bf16_table(padded):
    """Pure-bf16 mode: a bf16 table and bf16 weights go through the fp32
    kernel; output and gradients come back in bf16."""
    _cuda()
    table, ids, w, dout = _lexicon_case(3, 7, 50, 23, seed=16, padded=padded)
    _lexicon_check(table.bfloat16(), ids, w.bfloat16(), dout.bfloat16(),
                   label=f"bf16 padded={padded}")


def test_softlexicon_rejects_wide_words():
    _cuda()
    table, ids, w, _ = _lexicon_case(1, 5, 65, 9, seed=65)
    with pytest.raises(RuntimeError, match="word dim > 64"):
        ops.softlexicon_fuse(table, ids, w)
    torch.cuda.synchronize()


# --------------------------------------------------------------- masked CE
def _ce_case(N, T, seed, scale=1.0, valid=None):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(N, T, generator=g) * scale
    labels = torch.randint(0, T, (N,), generator=g)
    mask = (torch.rand(N, generator=g) > 0.3).long()
    if valid is not None:
        mask = torch.zeros(N, dtype=torch.long)
        mask[valid] = 1
    return logits, labels, mask


def _ce_check(logits, labels, mask, label):
    """logits fp32 or bf16 on the CPU. Both references run on the CPU, so
    the tolerance does not depend on the device's fp32 library."""
    logits = logits.detach()
    l64 = logits.double().requires_grad_()
    loss64 = ref.masked_cross_entropy(l64, labels, mask)
    loss64.backward()
    l32 = logits.float().clone().requires_grad_()
    loss32 = ref.masked_cross_entropy(l32, labels, mask)
    loss32.backward()
    assert loss64.dtype == torch.float64 and loss32.dtype == torch.float32

    lk = logits.clone().cuda().requires_grad_()
    loss = ops.masked_cross_entropy(lk, labels.cuda(), mask.cuda())
    loss.backward()
    assert loss.dtype == torch.float32 and lk.grad.dtype == logits.dtype
    assert torch.isfinite(loss) and torch.isfinite(lk.grad.float()).all()

    ratios = []
    for name, x, x32, x64 in (("loss", loss, loss32, loss64),
                              ("dlogits", lk.grad, l32.grad, l64.grad)):
        x, x32, x64 = (t.detach().double().cpu() for t in (x, x32, x64))
        err32 = float((x32 - x64).abs().max())
        tol = CE_FACTOR * err32 + 2.0 ** -23 * x64.abs()
        if logits.dtype == torch.bfloat16 and name == "dlogits":
            # autograd rounds the fp32 gradient to the logits' bf16
            tol = tol + HALF_ULP_BF16 * (x64.abs() + tol)
        err = (x - x64).abs()
        ratio = float(err.max()) / err32 if err32 > 0 else float("inf")
        ratios.append(ratio)
        print(f"masked_ce {label} {name}: err_kernel {float(err.max()):.3e} "
              f"err_fp32 {err32:.3e} ratio {ratio:.2f}")
        assert not (err > tol).any(), (
            f"{label} {name}: err {float(err.max()):.3e}, fp32 reference "
            f"{err32:.3e}")
    # rows outside the mask get exactly zero gradient
    assert not lk.grad[mask.cuda() == 0].any()
    return loss, lk.grad


@pytest.mark.parametrize("T", [1, 2, 10, 64])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 600, 1025])
def test_masked_ce_blocks_and_tags(N, T):
    """One block exactly, one short of it, one over, three (a real batch of
    4 x 150) and five blocks; T = 1 has loss 0 and gradient 0."""
    _cuda()
    logits, labels, mask = _ce_case(N, T, seed=N * 100 + T)
    if N == 1:
        mask[:] = 1
    _ce_check(logits, labels, mask, f"N={N} T={T}")


@pytest.mark.parametrize("N,T", [(600, 10), (1025, 64)])
def test_masked_ce_all_masked(N, T):
    """nvalid = 0: the loss is exactly 0 and so is every gradient."""
    _cuda()
    logits, labels, mask = _ce_case(N, T, seed=3, valid=[])
    loss, grad = _ce_check(logits, labels, mask, f"all-masked N={N}")
    assert float(loss) == 0.0 and not grad.any()


@pytest.mark.parametrize("N,T", [(600, 10), (1025, 64)])
def test_masked_ce_one_valid_row_in_last_block(N, T):
    _cuda()
    logits, labels, mask = _ce_case(N, T, seed=4, valid=[N - 1])
    _, grad = _ce_check(logits, labels, mask, f"one-valid N={N}")
    assert grad[N - 1].any() and not grad[:N - 1].any()


@pytest.mark.parametrize("N,T", [(600, 10), (257, 64)])
def test_masked_ce_large_logits(N, T):
    """Logits times 40: the row maximum is subtracted before exp."""
    _cuda()
    logits, labels, mask = _ce_case(N, T, seed=5, scale=40.0)
    _ce_check(logits, labels, mask, f"x40 N={N} T={T}")


def test_masked_ce_bf16_logits():
    """bf16 logits in the model's [B, L, T] layout; the gradient comes back
    in bf16."""
    _cuda()
    logits, labels, mask = _ce_case(600, 10, seed=6)
    loss, grad = _ce_check(logits.bfloat16().view(4, 150, 10),
                           labels.view(4, 150), mask.view(4, 150), "bf16")
    assert grad.shape == (4, 150, 10)
