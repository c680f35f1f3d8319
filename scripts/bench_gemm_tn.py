"""gemm_tn / gemm_nn (csrc/gemm_nt.hip) vs the library on the BERT backward
shapes at T = 8192: the four wgrad products dW[N,K] = dy^T x per split
(1, 2, 3, 4, 6, 8 and the host rule, split 0) and the four dgrad products
dx = dy w. Device events over 20 calls, min of 5 rounds.
Prints the table; `--out FILE` also writes it there."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from chinesener_amd import ops  # noqa: E402

ext = ops.get_ext()
torch.manual_seed(0)
lines = []
T = 8192
# linear layers as (out N, in K): QKV, attention out, FFN up, FFN down
LAYERS = [(2304, 768), (768, 768), (3072, 768), (768, 3072)]
SPLITS = [1, 2, 3, 4, 6, 8, 0]


def bench(fn, calls=20, rounds=5):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(rounds):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / calls)
    return best


def emit(line):
    print(line, flush=True)
    lines.append(line)


for N, K in LAYERS:
    dy = torch.randn(T, N, device="cuda", dtype=torch.bfloat16)
    x = torch.randn(T, K, device="cuda", dtype=torch.bfloat16)
    fl = 2.0 * T * N * K
    t_lib = bench(lambda: dy.T @ x)
    parts = []
    for s in SPLITS:
        t = bench(lambda: ext.gemm_tn(dy, x, s, False))
        parts.append(f"s{s} {t:6.1f}us ({fl / t / 1e6:4.0f})")
    emit(f"wgrad dW[{N:4d},{K:4d}] T={T}: lib {t_lib:6.1f}us "
         f"({fl / t_lib / 1e6:4.0f} TF/s) | " + "  ".join(parts))

for N, K in LAYERS:
    dy = torch.randn(T, N, device="cuda", dtype=torch.bfloat16)
    w = torch.randn(N, K, device="cuda", dtype=torch.bfloat16)
    fl = 2.0 * T * N * K
    t_lib = bench(lambda: dy @ w)
    t = bench(lambda: ext.gemm_nn(dy, w, False))
    emit(f"dgrad dx[{T},{K:4d}] N={N:4d}: lib {t_lib:6.1f}us "
         f"({fl / t_lib / 1e6:4.0f} TF/s) | ours {t:6.1f}us "
         f"({fl / t / 1e6:4.0f} TF/s)  ratio {t_lib / t:.2f}x")

if "--out" in sys.argv:
    out = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
