"""Attention fwd+bwd timing through ops.attention_qkv at the BERT-base
head shape (B=64, H=12, D=64) on random data.

  L in {170, 256, 384, 512}: the tiled kernel (default dispatch) against
      CHINESENER_ATTN_TILED=off, the unfused torch path it replaces.
  L in {128, 160}: CHINESENER_ATTN_TILED=force against the full-LDS kernel
      (recorded only; the default dispatch keeps the full-LDS kernel).

The variants of one L are interleaved in one process (A B A B ...), each
sample is `--iters` fwd+bwd steps between two device events, and the
table reports the median and the min over `--reps` samples plus
torch.cuda.max_memory_allocated of one step of each variant. Correctness
is covered by tests/test_gpu_attention_tiled.py.

  python scripts/bench_attention.py [--out profiles/attn_tiled_r03.md]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from chinesener_amd.ops import functional as fn  # noqa: E402

ENV = "CHINESENER_ATTN_TILED"
# L -> [(label, env value or None)]; the first entry is the baseline
PLAN = {
    128: [("full-LDS", None), ("tiled (force)", "force")],
    160: [("full-LDS", None), ("tiled (force)", "force")],
    170: [("torch (off)", "off"), ("tiled", None)],
    256: [("torch (off)", "off"), ("tiled", None)],
    384: [("torch (off)", "off"), ("tiled", None)],
    512: [("torch (off)", "off"), ("tiled", None)],
}


def set_mode(value):
    if value is None:
        os.environ.pop(ENV, None)
    else:
        os.environ[ENV] = value


def bench_len(L, B, H, D, p_drop, reps, iters):
    torch.manual_seed(L)
    qkv = torch.randn(B, L, 3, H, D, device="cuda", dtype=torch.bfloat16,
                      requires_grad=True)
    dout = torch.randn(B, L, H, D, device="cuda", dtype=torch.bfloat16)
    lens = torch.full((B,), L, dtype=torch.int32, device="cuda")
    mask = torch.ones(B, L, dtype=torch.long, device="cuda")

    def step():
        out = fn.attention_qkv(qkv, mask=mask, lens=lens, p_drop=p_drop,
                               training=p_drop > 0)
        out.backward(dout)
        qkv.grad = None

    variants = PLAN[L]
    expect = {"full-LDS": "lds", "torch (off)": "torch"}
    peak = {}
    for label, mode in variants:          # warm-up + peak memory, per variant
        set_mode(mode)
        path = fn._attn_path(L, D, qkv.dtype, True)
        assert path == expect.get(label, "tiled"), (label, path)
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step()
        torch.cuda.synchronize()
        peak[label] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    times = {label: [] for label, _ in variants}
    for _ in range(reps):                 # interleaved samples
        for label, mode in variants:
            set_mode(mode)
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(iters):
                step()
            t1.record()
            t1.synchronize()
            times[label].append(t0.elapsed_time(t1) / iters)
    set_mode(None)
    return [(label, statistics.median(times[label]), min(times[label]),
             peak[label]) for label, _ in variants]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--lens", type=int, nargs="*", default=sorted(PLAN))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--head_dim", type=int, default=64)
    ap.add_argument("--p_drop", type=float, default=0.0)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None, help="append the table here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_attention.py needs a GPU")

    lines = [
        f"B={args.batch} H={args.heads} D={args.head_dim} p_drop={args.p_drop}"
        f"; fwd+bwd per step, {args.reps} interleaved samples x {args.iters} "
        "steps, device events",
        "",
        "| L | variant | median ms | min ms | vs baseline (median) | "
        "peak MiB above inputs |",
        "|---|---|---|---|---|---|",
    ]
    for L in args.lens:
        rows = bench_len(L, args.batch, args.heads, args.head_dim,
                         args.p_drop, args.reps, args.iters)
        base = rows[0][1]
        for label, med, mn, pk in rows:
            lines.append(f"| {L} | {label} | {med:.3f} | {mn:.3f} | "
                         f"{base / med:.2f}x | {pk:.0f} |")
        print("\n".join(lines[-len(rows):]), flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
