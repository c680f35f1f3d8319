"""crf_fwd's loss kernel (csrc/crf_pair.hip) at one and at two sequences per
block, on the same inputs, the two taking turns window by window. The route
(csrc/crf_pair_route.h) fixes one of them; this is the measurement behind
that choice. Shapes whose two-sequence carve does not fit LDS print n/a.

Method: scripts/bench_crf_partial.py's (device events around N back-to-back
calls after warm-up, R windows, median and min..max in microseconds).

    python scripts/bench_crf_pair.py [--out table.md]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from chinesener_amd import ops  # noqa: E402

SHAPES = [(64, 128, 10), (64, 128, 24), (64, 128, 32), (64, 128, 41),
          (64, 512, 24), (8, 150, 10), (1, 150, 10), (512, 128, 10)]


def window(fn, n):
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / n


def fmt(ws):
    if not ws:
        return "n/a"
    return f"{statistics.median(ws):.1f} ({min(ws):.1f}..{max(ws):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table here")
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_crf_pair.py needs a GPU"
    ext = ops.get_ext()
    gen = torch.Generator().manual_seed(0)
    lines = ["| B | L | T | 1 sequence / block us | 2 sequences / block us |",
             "|---|---|---|---|---|"]
    print(torch.cuda.get_device_name(0), flush=True)
    for B, L, T in SHAPES:
        em = torch.randn(B, L, T, generator=gen).cuda()
        trans = torch.randn(T, T, generator=gen).cuda()
        lens = torch.full((B,), L, dtype=torch.int32, device="cuda")
        tags = torch.randint(0, T, (B, L), generator=gen).to(torch.int32).cuda()
        fns = {}
        for seqs in (1, 2):
            def fn(seqs=seqs):
                return ext.crf_pair_fwd(em, tags, lens, trans,
                                        seqs_per_block=seqs)
            try:
                for _ in range(10):
                    fn()
                fns[seqs] = fn
            except RuntimeError as e:
                print(f"  {seqs}/block refused: {str(e).splitlines()[0]}",
                      flush=True)
        torch.cuda.synchronize()
        n = 400 if L <= 150 else 100
        ws = {1: [], 2: []}
        for _ in range(args.reps):
            for seqs, fn in fns.items():
                ws[seqs].append(window(fn, n))
        row = f"| {B} | {L} | {T} | {fmt(ws[1])} | {fmt(ws[2])} |"
        print(row, flush=True)
        lines.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
