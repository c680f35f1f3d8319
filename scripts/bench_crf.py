"""CRF kernel timing: crf_fwd (loss + grads in one pass), crf_viterbi,
crf_path_posterior and crf_nbest (k = 4, 8) at B=64 over the tag counts
either side of the narrow/wide boundary and at the serving shapes (B = 1,
8), next to ops.reference (fwd+bwd / decode) on the same GPU and the same
inputs.
crf_fwd and crf_path_posterior both get the Viterbi path as their tags:
crf_fwd runs the same two scans plus the alpha table and both gradients, so
it is the yardstick the posterior kernel must not exceed. crf_nbest is the
kernel alone (no path posterior); its yardstick is crf_viterbi on the same
inputs, and the last column is that ratio. (64, 512, 64) is the shape whose
backpointers go through the global workspace.
Correctness is covered by tests/test_gpu_kernels.py,
tests/test_gpu_crf_wide.py, tests/test_gpu_crf_posterior.py and
tests/test_gpu_crf_nbest.py; this times
the extension entry points only.

Method: device events around N back-to-back calls, after warm-up; R such
windows per shape; the table reports the median window and the min..max
spread, in microseconds per call. A shape the extension refuses, or an op
it does not have, prints n/a, so the same script runs on a commit without
the wide kernels, without crf_path_posterior or without crf_nbest.

    python scripts/bench_crf.py [--out table.md] [--no-ref]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from chinesener_amd import ops  # noqa: E402
from chinesener_amd.ops import reference as ref  # noqa: E402

SHAPES = [(64, 128, 10), (64, 128, 20), (64, 128, 24), (64, 128, 41),
          (64, 128, 64), (64, 512, 24), (64, 512, 64),
          # serving: one request and one full bucket
          (1, 150, 10), (8, 150, 10), (1, 128, 24), (8, 128, 24)]


def windows(fn, n, reps, warmup):
    """[us per call] for `reps` windows of `n` calls each."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(n):
            fn()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1) * 1e3 / n)
    return out


def fmt(ws):
    if ws is None:
        return "n/a"
    return f"{statistics.median(ws):.1f} ({min(ws):.1f}..{max(ws):.1f})"


def try_windows(fn, n, reps, warmup):
    try:
        return windows(fn, n, reps, warmup)
    except RuntimeError as e:  # shape outside this build's kernels
        print(f"  refused: {str(e).splitlines()[0]}", flush=True)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table here")
    ap.add_argument("--no-ref", action="store_true",
                    help="skip the torch reference columns")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_crf.py needs a GPU"
    ext = ops.get_ext()
    torch.manual_seed(0)

    lines = ["| B | L | T | crf_fwd route | crf_fwd us | ref fwd+bwd us | crf_viterbi us | "
             "ref decode us | crf_path_posterior us | crf_nbest k=4 us | "
             "crf_nbest k=8 us | nbest/viterbi k=4, k=8 |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    print(torch.cuda.get_device_name(0), flush=True)
    for B, L, T in SHAPES:
        em = torch.randn(B, L, T, device="cuda")
        trans = torch.randn(T, T, device="cuda")
        lens = torch.full((B,), L, dtype=torch.int32, device="cuda")
        mask = torch.ones(B, L, dtype=torch.long, device="cuda")
        tags = torch.randint(0, T, (B, L), device="cuda")
        tags32 = tags.to(torch.int32)
        n = 50 if L <= 150 else 20
        try:  # the decoded path, where this build can decode the shape
            tags32 = ext.crf_viterbi(em, lens, trans)
            tags = tags32.long()
        except RuntimeError:
            pass

        fwd = try_windows(lambda: ext.crf_fwd(em, tags32, lens, trans),
                          n, args.reps, 5)
        vit = try_windows(lambda: ext.crf_viterbi(em, lens, trans),
                          n, args.reps, 5)
        post = None
        if hasattr(ext, "crf_path_posterior"):
            post = try_windows(
                lambda: ext.crf_path_posterior(em, lens, trans, tags32),
                n, args.reps, 5)
        nb = {4: None, 8: None}
        if hasattr(ext, "crf_nbest"):
            for k in nb:
                nb[k] = try_windows(
                    lambda: ext.crf_nbest(em, lens, trans, k), n, args.reps, 5)
        ratio = "n/a"
        if vit and nb[4] and nb[8]:
            v = statistics.median(vit)
            ratio = (f"{statistics.median(nb[4]) / v:.1f}x, "
                     f"{statistics.median(nb[8]) / v:.1f}x")
        rfwd = rvit = None
        if not args.no_ref:
            em_g = em.clone().requires_grad_()
            tr_g = trans.clone().requires_grad_()

            def ref_step():
                ll = ref.crf_log_likelihood(em_g, tags, mask, tr_g)
                ll.sum().backward()
                em_g.grad = None
                tr_g.grad = None

            def ref_dec():
                with torch.no_grad():
                    ref.crf_decode(em, mask, trans)

            rfwd = windows(ref_step, 2, 3, 1)
            rvit = windows(ref_dec, 2, 3, 1)
        route = "n/a"   # a build without the query has the former routes
        if hasattr(ext, "crf_fwd_route"):
            pair, waves, lds = ext.crf_fwd_route(L, T)
            route = f"pair {waves}w {lds} B" if pair else "wide"
        row = (f"| {B} | {L} | {T} | {route} | {fmt(fwd)} | {fmt(rfwd)} | {fmt(vit)} | "
               f"{fmt(rvit)} | {fmt(post)} | {fmt(nb[4])} | {fmt(nb[8])} | "
               f"{ratio} |")
        print(row, flush=True)
        lines.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
