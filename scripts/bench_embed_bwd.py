"""Embedding backward timing: the sorted-segment-sum kernels
(ext.embed3_bwd, csrc/embed.hip) next to the torch scatter code they
replace (ops.functional._embed3_bwd_torch: fp32 casts, zero fills,
index_add_ with float atomics, casts back) on the same GPU and inputs, at
the flagship tables (V=21128, P=512, S=2, H=768) for B=64 with L=128 and
L=512, on two id distributions:

  synthetic  ids as data.loader.make_synthetic_batch draws them (uniform
             over the vocabulary, CLS/SEP once per row, a PAD tail),
             all rows in segment 0
  skewed     Zipf-like ids (weight 1/k over 5000 ids), whose most frequent
             id is on about 11 % of the rows; no PAD; all rows in segment 0

The last column is skewed / synthetic for the kernels: the list chunking
is there to keep it near 1. Correctness is covered by
tests/test_gpu_embed_bwd.py; this times the two entry points only.

Method: device events around N back-to-back calls, after warm-up; R such
windows per shape; the table reports the median window and the min..max
spread, in microseconds per call.

    python scripts/bench_embed_bwd.py [--out table.md]
        [--ids synthetic|skewed] [--no-torch]    (one input, kernels only:
                                                  for a per-kernel trace)
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from chinesener_amd import ops  # noqa: E402
from chinesener_amd.data.loader import make_synthetic_batch  # noqa: E402
from chinesener_amd.ops import functional as fn  # noqa: E402

V, P, S, H = 21128, 512, 2, 768
SHAPES = [(64, 128), (64, 512)]


def windows(f, n, reps, warmup):
    """[us per call] for `reps` windows of `n` calls each."""
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(n):
            f()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1) * 1e3 / n)
    return out


def fmt(ws):
    return f"{statistics.median(ws):.1f} ({min(ws):.1f}..{max(ws):.1f})"


def skewed_ids(B, L, seed=0):
    """Zipf-like: rank k drawn with weight 1/k over 5000 ids. The head of
    that law is the one heavy id: 1 / H(5000) = 11 % of the rows."""
    g = torch.Generator().manual_seed(seed)
    w = 1.0 / torch.arange(1, 5001, dtype=torch.float64)
    ids = torch.multinomial(w, B * L, replacement=True, generator=g) + 106
    return ids.reshape(B, L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table here")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ids", choices=["synthetic", "skewed"], default=None,
                    help="time this input only")
    ap.add_argument("--no-torch", action="store_true",
                    help="skip the torch column")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_embed_bwd.py needs a GPU"
    ext = ops.get_ext()
    print(torch.cuda.get_device_name(0), flush=True)
    lines = ["| B | L | ids | longest list | torch us | embed3_bwd us | "
             "torch / kernels | skewed / synthetic |",
             "|---|---|---|---|---|---|---|---|"]
    for B, L in SHAPES:
        g = torch.Generator().manual_seed(1)
        dy = torch.randn(B, L, H, generator=g).to(torch.bfloat16).cuda()
        segs = torch.zeros(B, L, dtype=torch.long, device="cuda")
        base = None
        for name, ids in (
                ("synthetic", make_synthetic_batch(B, L)["token_ids"]),
                ("skewed", skewed_ids(B, L))):
            if args.ids and name != args.ids:
                continue
            longest = int(torch.bincount(ids.flatten())[1:].max())
            ids = ids.cuda()
            old = None
            if not args.no_torch:
                old = windows(lambda: fn._embed3_bwd_torch(
                    dy, ids, segs, (V, H), (P, H), (S, H)), 20, args.reps, 5)
            new = windows(lambda: ext.embed3_bwd(dy, ids, segs, V, P, S),
                          20, args.reps, 5)
            m_new = statistics.median(new)
            if base is None:
                base = m_new
            ratio = f"{statistics.median(old) / m_new:.1f}x" if old else "n/a"
            row = (f"| {B} | {L} | {name} | {longest} | "
                   f"{fmt(old) if old else 'n/a'} | "
                   f"{fmt(new)} | {ratio} | "
                   f"{m_new / base:.2f}x |")
            print(row, flush=True)
            lines.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
