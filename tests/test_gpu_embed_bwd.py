"""Embedding backward as sorted segment sums (csrc/embed.hip embed3_bwd,
csrc/sorted_index.h) against a CPU fp64 reference rounded once to bf16:
called directly and through fn.embed3(...).backward.

Exact cases use small-integer dy, so every fp32 sum is exact in any order
and the comparison is bitwise over whole tensors, zero rows included; the
outputs come from at::empty, so NaN-filled blocks of the same sizes are
freed just before each call and an unwritten cell shows as NaN. Random dy
gets the a-priori bound of one bf16 rounding plus the fp32 summation
error of any order: |got - ref| <= 2^-8 |ref| + n 2^-24 sum|dy| over the
element's list of n rows."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from chinesener_amd import ops
from chinesener_amd.ops import functional as fn

BF = torch.bfloat16


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.ext_available(), "HIP extension must be built for GPU tests"


def _limits():
    chunk, cap, max_rows, max_keys = ops.get_ext().embed3_bwd_limits()
    return chunk, cap, max_rows, max_keys


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _make_ids(mode, V, B, L, g):
    R = B * L
    if mode == "rand":
        return torch.randint(0, V, (B, L), generator=g)
    if mode == "zero":
        return torch.zeros(B, L, dtype=torch.long)
    if mode == "seven":
        return torch.full((B, L), 7, dtype=torch.long)
    if mode == "distinct":      # V > R; ids 1 and V-1 among them
        assert V - 3 >= R - 2
        mid = torch.randperm(V - 3, generator=g)[:max(R - 2, 0)] + 2
        ids = torch.cat([torch.tensor([1, V - 1]), mid])[:R]
        return ids[torch.randperm(R, generator=g)].reshape(B, L)
    if mode == "half":          # one id on half the rows
        ids = torch.randint(1, V, (R,), generator=g)
        ids[torch.randperm(R, generator=g)[:R // 2]] = 11
        return ids.reshape(B, L)
    raise ValueError(mode)


def _make_segs(mode, S, B, L, g):
    if mode == "mixed":
        return torch.randint(0, S, (B, L), generator=g)
    return torch.full((B, L), {"zero": 0, "one": 1}[mode], dtype=torch.long)


def _ref64(dy, ids, segs, V, P, S):
    """(sums, sums of |dy|, list lengths) per table, fp64 on the CPU."""
    B, L, H = dy.shape
    d = dy.detach().double().cpu().reshape(-1, H)
    ids = ids.cpu().reshape(-1)
    segs = segs.cpu().reshape(-1)
    ones = torch.ones(B * L, dtype=torch.float64)
    out = []
    for x in (d, d.abs()):
        dw = torch.zeros(V, H, dtype=torch.float64).index_add_(0, ids, x)
        dw[0] = 0
        dp = torch.zeros(P, H, dtype=torch.float64)
        dp[:L] = x.reshape(B, L, H).sum(0)
        dt = torch.zeros(S, H, dtype=torch.float64).index_add_(0, segs, x)
        out.append((dw, dp, dt))
    nw = torch.zeros(V, dtype=torch.float64).index_add_(0, ids, ones)
    nw[0] = 0
    np_ = torch.zeros(P, dtype=torch.float64)
    np_[:L] = B
    nt = torch.zeros(S, dtype=torch.float64).index_add_(0, segs, ones)
    return out[0], out[1], (nw, np_, nt)


def _poison(V, P, S, H):
    """NaN-filled blocks of the output sizes, freed at once: the caching
    allocator hands them to the at::empty outputs of the next call."""
    for n in (V, P, S):
        torch.full((n, H), float("nan"), device="cuda", dtype=BF)
    torch.cuda.synchronize()


def _direct(dy, ids, segs, V, P, S):
    _poison(V, P, S, dy.shape[-1])
    return ops.get_ext().embed3_bwd(dy, ids, segs, V, P, S)


def _through_node(dy, ids, segs, V, P, S):
    H = dy.shape[-1]
    w = torch.zeros(V, H, device="cuda", dtype=BF, requires_grad=True)
    p = torch.zeros(P, H, device="cuda", dtype=BF, requires_grad=True)
    t = torch.zeros(S, H, device="cuda", dtype=BF, requires_grad=True)
    out = fn.embed3(w, p, t, ids, segs)
    assert out.grad_fn is not None and "Embed3" in type(out.grad_fn).__name__
    _poison(V, P, S, H)
    return torch.autograd.grad(out, (w, p, t), dy)


def _assert_bound(got, ref, absum, n, what):
    err = (got.double().cpu() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + n[:, None] * 2.0 ** -24 * absum
    bad = err > bound
    assert not bad.any(), (
        f"{what}: {int(bad.sum())} over the bound, worst excess "
        f"{float((err - bound).max()):.3e}")
    assert not torch.isnan(got).any(), what


def _case(V, P, S, H, B, L, ids="rand", segs="mixed"):
    return dict(V=V, P=P, S=S, H=H, B=B, L=L, ids=ids, segs=segs)


def _exact_cases():
    # S and the all-7 row counts are given in units of the build's limits
    # (segment cap, list chunk C) and resolved in the test
    cap = "cap"
    cs = {
        "existing-shape": _case(500, 64, 2, 96, 4, 33),
        "real-width-vocab": _case(21128, 512, 2, 768, 2, 128),
        "H8": _case(500, 64, 2, 8, 4, 33),
        "H264": _case(500, 64, 2, 264, 4, 33),
        "single-row": _case(500, 64, 2, 96, 1, 1),
        "L-eq-P": _case(500, 33, 2, 96, 4, 33),
        "L-lt-P": _case(500, 40, 2, 96, 4, 33),
        "all-pad": _case(500, 64, 2, 96, 4, 33, ids="zero"),
        "distinct": _case(300, 64, 2, 96, 4, 33, ids="distinct"),
        "V2": _case(2, 64, 2, 96, 4, 33),
        "seg-all-0": _case(500, 64, 2, 96, 4, 33, segs="zero"),
        "seg-all-1": _case(500, 64, 2, 96, 4, 33, segs="one"),
        "S1": _case(500, 64, 1, 96, 4, 33),
        "S-cap": _case(500, 64, cap, 96, 4, 33),
        "S-cap-plus-1": _case(500, 64, "cap+1", 96, 4, 33),
        # more rows than one slice of the rank kernel (512) and one tile (256)
        "two-slices": _case(700, 80, 2, 96, 9, 77),
    }
    # one list of R rows around the chunking edges: lists of fewer than 2C
    # rows are summed by one wave, n rows by n // C waves from 2C on; the
    # finisher adds the partial sums in 8 slices, so 5, 8, 9 and 21 chunks
    for mul, add in ((1, -1), (1, 0), (1, 1), (2, -1), (2, 0), (2, 1), (5, 3),
                     (8, 0), (9, 15), (21, 5)):
        cs[f"all-7-R-{mul}C{add:+d}"] = _case(500, (mul, add), 2, 96, 1,
                                              (mul, add), ids="seven")
    return cs


_EXACT = _exact_cases()


@pytest.mark.parametrize("name", list(_EXACT))
def test_exact_on_integer_dy(name):
    _cuda()
    C, cap, max_rows, max_keys = _limits()
    assert max_rows >= 64 * 512 and max_keys >= 21128 * 64 * 512
    c = dict(_EXACT[name])
    c["S"] = {"cap": cap, "cap+1": cap + 1}.get(c["S"], c["S"])
    for k in "PL":
        if isinstance(c[k], tuple):
            c[k] = c[k][0] * C + c[k][1]
    V, P, S, H, B, L = (c[k] for k in "VPSHBL")
    g = _gen(sum(map(ord, name)))
    dy = torch.randint(-2, 4, (B, L, H), generator=g).to(BF).cuda()
    ids = _make_ids(c["ids"], V, B, L, g).cuda()
    segs = _make_segs(c["segs"], S, B, L, g).cuda()
    ref, _, _ = _ref64(dy, ids, segs, V, P, S)
    ref = [r.to(BF) for r in ref]
    routes = [("node", _through_node)]
    if S <= cap:
        routes.append(("direct", _direct))
    for route, call in routes:
        got = call(dy, ids, segs, V, P, S)
        for nm, a, b in zip(("dw", "dp", "dt"), got, ref):
            assert a.dtype == BF and tuple(a.shape) == tuple(b.shape)
            assert torch.equal(a.cpu(), b), f"{name}/{route}/{nm}"


_RANDOM = {
    "existing-shape": _case(500, 64, 2, 96, 4, 33),
    "real-width-vocab": _case(21128, 512, 2, 768, 2, 128),
    "skewed": _case(500, 64, 2, 96, 8, 64, ids="half"),
}


def _random_inputs(name):
    c = _RANDOM[name]
    V, P, S, H, B, L = (c[k] for k in "VPSHBL")
    g = _gen(7 + len(name))
    dy = torch.randn(B, L, H, generator=g).to(BF).cuda()
    ids = _make_ids(c["ids"], V, B, L, g).cuda()
    segs = _make_segs(c["segs"], S, B, L, g).cuda()
    return dy, ids, segs, V, P, S


@pytest.mark.parametrize("name", list(_RANDOM))
def test_random_dy_within_apriori_bound(name):
    _cuda()
    dy, ids, segs, V, P, S = _random_inputs(name)
    ref, absum, n = _ref64(dy, ids, segs, V, P, S)
    for route, call in (("direct", _direct), ("node", _through_node)):
        got = call(dy, ids, segs, V, P, S)
        for nm, a, r, s, k in zip(("dw", "dp", "dt"), got, ref, absum, n):
            _assert_bound(a, r, s, k, f"{name}/{route}/{nm}")


def test_two_calls_are_bitwise_equal():
    _cuda()
    dy, ids, segs, V, P, S = _random_inputs("skewed")
    a = _direct(dy, ids, segs, V, P, S)
    b = _direct(dy, ids, segs, V, P, S)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16))


@pytest.mark.parametrize("pad_row", [False, True])
def test_nan_row_reaches_only_its_destinations(pad_row):
    _cuda()
    V, P, S, H, B, L = 500, 64, 2, 96, 4, 33
    g = _gen(31)
    dy = torch.randn(B, L, H, generator=g).to(BF)
    ids = torch.randint(1, V, (B, L), generator=g)
    segs = torch.randint(0, S, (B, L), generator=g)
    b0, l0 = 2, 17
    if pad_row:
        ids[b0, l0] = 0
    dy[b0, l0] = float("nan")
    dw, dp, dt = _direct(dy.cuda(), ids.cuda(), segs.cuda(), V, P, S)

    def nan_rows(t):
        m = torch.isnan(t).cpu()
        # a row is NaN in every column or in none
        assert torch.equal(m.any(1), m.all(1))
        return m.any(1).nonzero().flatten().tolist()

    assert nan_rows(dw) == ([] if pad_row else [int(ids[b0, l0])])
    assert nan_rows(dp) == [l0]
    assert nan_rows(dt) == [int(segs[b0, l0])]


def test_graph_capture_replays_with_new_ids():
    _cuda()
    V, P, S, H, B, L = 500, 64, 2, 96, 4, 33
    g = _gen(41)
    w = torch.randn(V, H, generator=g).to(BF).cuda().requires_grad_()
    p = torch.randn(P, H, generator=g).to(BF).cuda().requires_grad_()
    t = torch.randn(S, H, generator=g).to(BF).cuda().requires_grad_()
    dy = torch.randn(B, L, H, generator=g).to(BF).cuda()
    id_sets = [(_make_ids("rand", V, B, L, g).cuda(),
                _make_segs("mixed", S, B, L, g).cuda()),
               (_make_ids("half", V, B, L, g).cuda(),
                _make_segs("zero", S, B, L, g).cuda())]
    s_ids = id_sets[0][0].clone()
    s_segs = id_sets[0][1].clone()

    def step(ids, segs):
        out = fn.embed3(w, p, t, ids, segs)
        return (out,) + torch.autograd.grad(out, (w, p, t), dy)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(s_ids, s_segs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step(s_ids, s_segs)
    for ids, segs in reversed(id_sets):
        s_ids.copy_(ids)
        s_segs.copy_(segs)
        graph.replay()
        torch.cuda.synchronize()
        eager = step(ids, segs)
        for a, b in zip(captured, eager):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_switch_off_gives_the_torch_path(monkeypatch):
    _cuda()
    dy, ids, segs, V, P, S = _random_inputs("skewed")
    ref, absum, n = _ref64(dy, ids, segs, V, P, S)
    new = _through_node(dy, ids, segs, V, P, S)
    calls = []
    real = fn._embed3_bwd_torch
    monkeypatch.setattr(fn, "_embed3_bwd_torch",
                        lambda *a: calls.append(1) or real(*a))
    monkeypatch.setenv("CHINESENER_EMBED3_BWD", "off")
    old = _through_node(dy, ids, segs, V, P, S)
    assert calls == [1]
    for nm, a, b, r, s, k in zip(("dw", "dp", "dt"), new, old, ref, absum, n):
        _assert_bound(a, r, s, k, f"new/{nm}")
        _assert_bound(b, r, s, k, f"off/{nm}")
