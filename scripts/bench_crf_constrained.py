"""Constrained Viterbi timing: crf_viterbi_constrained next to crf_viterbi
on the same emissions and lengths, and next to the host composition it
replaces (expand the words with torch, torch.where the emissions to -1e30
outside the sets, call crf_viterbi), at the training widths (10, 24, 64
tags), one serving row and the largest carve (8, 512, 64). The composition
honours the position words only, not transition words, and feeds -1e30 into
kernels that were never specified for it; it is timed, not checked.
Correctness is covered by tests/test_gpu_crf_constrained.py; this times the
extension entry points (output allocation included, as a caller pays).

Method (scripts/bench_crf_partial.py): device events around N back-to-back
calls after warm-up; the three take turns, window by window, so drift hits
all alike; R windows each; the table reports the median window and the
min..max spread in microseconds per call. About half the positions carry an
open word, a third a singleton, the rest a random subset.

    python scripts/bench_crf_constrained.py [--out table.md]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from chinesener_amd import ops  # noqa: E402
from chinesener_amd.ops import reference as ref  # noqa: E402

from bench_crf_partial import SHAPES, fmt, random_words, window  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table here")
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_crf_constrained.py needs a GPU"
    ext = ops.get_ext()
    gen = torch.Generator().manual_seed(0)

    lines = ["| B | L | T | crf_viterbi_constrained us | crf_viterbi us | "
             "host composition us | constrained / crf_viterbi | "
             "constrained / composition |",
             "|---|---|---|---|---|---|---|---|"]
    print(torch.cuda.get_device_name(0), flush=True)
    for B, L, T in SHAPES:
        em = torch.randn(B, L, T, generator=gen).cuda()
        trans = torch.randn(T, T, generator=gen).cuda()
        lens = torch.full((B,), L, dtype=torch.int32, device="cuda")
        allowed = random_words(B, L, T, gen).cuda()
        tallowed = torch.full((T,), -1, dtype=torch.int64, device="cuda")
        neg = torch.full((), -1e30, device="cuda")

        def con():
            return ext.crf_viterbi_constrained(em, allowed, lens, trans,
                                               tallowed)

        def vit():
            return ext.crf_viterbi(em, lens, trans)

        def comp():
            masked = torch.where(ref.allowed_sets(allowed, T), em, neg)
            return ext.crf_viterbi(masked, lens, trans)

        n = 400 if L <= 150 else 100
        for fn in (con, vit, comp):
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        wc, wv, wh = [], [], []
        for _ in range(args.reps):
            wc.append(window(con, n))
            wv.append(window(vit, n))
            wh.append(window(comp, n))
        mc = statistics.median(wc)
        row = (f"| {B} | {L} | {T} | {fmt(wc)} | {fmt(wv)} | {fmt(wh)} | "
               f"{mc / statistics.median(wv):.2f}x | "
               f"{mc / statistics.median(wh):.2f}x |")
        print(row, flush=True)
        lines.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
