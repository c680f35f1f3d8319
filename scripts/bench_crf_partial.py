"""Partial-annotation CRF timing: crf_partial_fwd next to crf_fwd on the same
emissions and lengths, at the training widths (10, 24, 64 tags), one serving
row and the split-route shape (8, 512, 64). crf_fwd is one forward-backward
scan plus the gold score; crf_partial_fwd is two scans (free and
constrained) and their difference, on two waves of a block (pair route) or
in two launches (split route). The last column is partial / crf_fwd.
Correctness is covered by tests/test_gpu_crf_partial.py; this times the
extension entry points only (output allocation included, as a caller pays).

Method: device events around N back-to-back calls after warm-up; the two
ops take turns, window by window, so drift hits both alike; R windows each;
the table reports the median window and the min..max spread in microseconds
per call. About half the positions carry an open word, a third a singleton,
the rest a random subset.

    python scripts/bench_crf_partial.py [--out table.md]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from chinesener_amd import ops  # noqa: E402

SHAPES = [(64, 128, 10), (64, 128, 24), (64, 128, 64), (1, 150, 10),
          (8, 512, 64)]


def random_words(B, L, T, gen):
    """int64 [B,L] on the CPU: ~1/2 open, ~1/3 singletons, rest subsets."""
    tags = torch.randint(0, T, (B, L), generator=gen)
    single = ops.allowed_from_tags(tags, torch.ones(B, L, dtype=torch.bool), 0)
    lo = torch.randint(0, 1 << min(T, 32), (B, L), generator=gen)
    hi = torch.randint(0, 1 << max(min(T, 63) - 32, 1), (B, L),
                       generator=gen) << 32
    subset = (lo | hi if T > 32 else lo) | single
    r = torch.rand(B, L, generator=gen)
    words = torch.where(r < 0.5, torch.zeros_like(single),   # 0 = all tags
                        torch.where(r < 0.83, single, subset))
    return words


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
    return f"{statistics.median(ws):.1f} ({min(ws):.1f}..{max(ws):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table here")
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_crf_partial.py needs a GPU"
    ext = ops.get_ext()
    gen = torch.Generator().manual_seed(0)

    lines = ["| B | L | T | route | waves/block | LDS bytes | "
             "crf_partial_fwd us | crf_fwd us | partial / crf_fwd |",
             "|---|---|---|---|---|---|---|---|---|"]
    print(torch.cuda.get_device_name(0), flush=True)
    for B, L, T in SHAPES:
        em = torch.randn(B, L, T, generator=gen).cuda()
        trans = torch.randn(T, T, generator=gen).cuda()
        lens = torch.full((B,), L, dtype=torch.int32, device="cuda")
        tags32 = torch.randint(0, T, (B, L), generator=gen).to(torch.int32).cuda()
        allowed = random_words(B, L, T, gen).cuda()
        pair, nw, lds = ext.crf_partial_route(L, T)

        def part():
            return ext.crf_partial_fwd(em, allowed, lens, trans)

        def full():
            return ext.crf_fwd(em, tags32, lens, trans)

        n = 400 if L <= 150 else 100
        for fn in (part, full):
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        wp, wf = [], []
        for _ in range(args.reps):
            wp.append(window(part, n))
            wf.append(window(full, n))
        ratio = statistics.median(wp) / statistics.median(wf)
        row = (f"| {B} | {L} | {T} | {'pair' if pair else 'split'} | {nw} | "
               f"{lds} | {fmt(wp)} | {fmt(wf)} | {ratio:.2f}x |")
        print(row, flush=True)
        lines.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
