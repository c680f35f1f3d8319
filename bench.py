#!/usr/bin/env python3
"""Flagship training benchmark (driver contract).

Measures training samples/sec of bert_bilstm_crf (BERT-base encoder +
BiLSTM + CRF, the BASELINE.json headline config) on MSRA-shaped
synthetic data, bf16, random-init weights. Weak scaling: per-GPU batch
fixed; `value` is the whole-job aggregate samples/sec.

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
  (N>1 is launched by the driver via torch.distributed.run, one rank/GPU)

A plain run sets up, warms up, times the K steps and prints one JSON
line. --dump-outputs DIR additionally writes the last timed step's
results as DIR/*.npy (inputs are seeded, so two builds can be compared
output for output). --full is where any measurement beyond the headline
figure belongs; there is none today.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

# TunableOp GEMM tuning (env must be set BEFORE torch init) is a
# measured net LOSS on this stack now (17.55 ms/step without vs 17.82
# with, plus ~45 s tuning per process that multi-rank SCALE runs cannot
# afford) — opt-in via CHINESENER_TUNABLE=1.
if os.environ.get("CHINESENER_TUNABLE") == "1":
    _rank_tag = os.environ.get("RANK", "0")
    os.environ.setdefault("PYTORCH_TUNABLEOP_ENABLED", "1")
    os.environ.setdefault("PYTORCH_TUNABLEOP_TUNING", "1")
    # multi-rank: bound per-solution tuning time harder (ranks tune the
    # same shapes in lockstep between collectives; the slowest gates all)
    _dur = "100" if os.environ.get("WORLD_SIZE", "1") == "1" else "30"
    os.environ.setdefault("PYTORCH_TUNABLEOP_MAX_TUNING_DURATION_MS", _dur)
    # per-rank filename: concurrent ranks must not clobber one CSV
    os.environ.setdefault("PYTORCH_TUNABLEOP_FILENAME",
                          f"/tmp/chinesener_tunableop_r{_rank_tag}_.csv")
# a dead peer must raise in surviving ranks, not hang the driver window
os.environ.setdefault("TORCH_NCCL_ASYNC_ERROR_HANDLING", "1")

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from chinesener_amd.config import resolve_params
from chinesener_amd.data.loader import make_synthetic_batch
from chinesener_amd.models import build_model, model_params, optimizer_family
from chinesener_amd.train.optimizers import build_optimizer, clip_gradients


DUMP_PER_PARAM = 4096   # elements sampled from each parameter tensor


def dump_outputs(out_dir, loss, model):
    """Write what the last timed training step produced: its loss, and
    the parameters it updated. A BERT-base parameter set is ~440 MB in
    fp32, so each tensor contributes a fixed, seeded sample of at most
    DUMP_PER_PARAM elements (~3 MB in all), concatenated in
    named_parameters() order. The sample indices depend only on the
    parameter shapes, so two builds are comparable element for element."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "loss.npy"),
            loss.detach().float().cpu().numpy().reshape(-1))
    gen = torch.Generator().manual_seed(20240531)
    chunks = []
    with torch.no_grad():
        for _, p in model.named_parameters():
            flat = p.detach().reshape(-1)
            if flat.numel() > DUMP_PER_PARAM:
                idx = torch.randint(flat.numel(), (DUMP_PER_PARAM,),
                                    generator=gen)
                flat = flat[idx.to(flat.device)]
            chunks.append(flat.float().cpu())
    np.save(os.path.join(out_dir, "params_sample.npy"),
            torch.cat(chunks).numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch_size", type=int, default=64,
                    help="per-GPU batch (weak scaling; global=batch*gpus)")
    ap.add_argument("--seq_len", type=int, default=128)
    ap.add_argument("--model", default="bert_bilstm_crf")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed "
                         "step produced (loss + a fixed seeded sample of "
                         "the updated parameters) as DIR/<name>.npy, float32")
    ap.add_argument("--full", action="store_true",
                    help="also run the measurements and checks beyond the "
                         "headline figure (none today: a plain run already "
                         "does only setup, warmup, the timed steps and the "
                         "result line)")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if args.gpus > 1 and world == 1:
        print(f"[bench] --gpus {args.gpus} requested but WORLD_SIZE=1 — "
              f"launch via torch.distributed.run for multi-GPU; "
              f"measuring 1 GPU and reporting n_gpus=1", file=sys.stderr)
    local_rank = int(os.environ.get("LOCAL_RANK", rank))
    use_gpu = torch.cuda.is_available()
    # modulo lets a 2-rank RCCL smoke run on a 1-GPU box (oversubscribed)
    dev_idx = local_rank % max(1, torch.cuda.device_count()) if use_gpu else 0
    device = f"cuda:{dev_idx}" if use_gpu else "cpu"
    dist = None
    if world > 1:
        from datetime import timedelta
        import torch.distributed as dist_mod
        dist = dist_mod
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if use_gpu:
            torch.cuda.set_device(dev_idx)
        # bounded collective timeout: a desynced rank fails the job fast
        # with a diagnostic instead of eating the driver's SCALE window.
        # CHINESENER_DP_BACKEND=gloo lets a multi-rank smoke share one
        # GPU (RCCL refuses two ranks on one device).
        backend = os.environ.get("CHINESENER_DP_BACKEND") or (
            "nccl" if use_gpu else "gloo")
        dist.init_process_group(backend, timeout=timedelta(minutes=5))

    torch.manual_seed(1234 + rank)
    # MSRA-shaped config: vocab 21128, 10 BIO labels, BERT-base encoder
    params = resolve_params(model_params(args.model), {
        "vocab_size": 21128, "label_size": 10,
        "num_train_steps": 100000, "step_per_epoch": 1000,
    })
    if use_gpu:
        from chinesener_amd.ops.tunable import freeze, load_tuned_gemm_table
        if os.environ.get("CHINESENER_TUNABLE") == "1":
            load_tuned_gemm_table(tune=True)
    model = build_model(args.model, params).to(device)
    use_bf16 = use_gpu and params.get("dtype", "bf16") == "bf16"
    if use_bf16:
        # pure-bf16 weights + fp32 masters in the fused optimizer
        from chinesener_amd.train.precision import convert_bf16_mixed
        convert_bf16_mixed(model)
    dp = None
    if world > 1:
        from chinesener_amd.dist import BucketedDataParallel
        dp = BucketedDataParallel(model)
    family = optimizer_family(args.model)
    opt, schedule = build_optimizer(model, family, params)

    from chinesener_amd.data.preprocess import extract_prefix_surfix
    enhance, _ = extract_prefix_surfix(args.model)
    batches = [make_synthetic_batch(args.batch_size, args.seq_len, 10,
                                    word_enhance=enhance, seed=rank * 100 + i,
                                    device=device)
               for i in range(8)]

    step_num = 0

    def cast(b):
        if not use_bf16:
            return b
        return {k: v.to(torch.bfloat16) if v.is_floating_point() else v
                for k, v in b.items()}

    def train_step(batch):
        nonlocal step_num
        if dp is not None:
            dp.zero_grad()
        else:
            opt.zero_grad(set_to_none=True)
        out = model(cast(batch))
        out.loss.backward()
        if dp is not None:
            dp.finalize_backward()
        clip_gradients(model, family)
        step_num += 1
        schedule.apply(opt, step_num)
        opt.step()
        return out.loss

    t_w0 = time.perf_counter()
    for i in range(args.warmup):
        train_step(batches[i % len(batches)])
    if use_gpu:
        freeze()
        if rank == 0 and os.environ.get("CHINESENER_BENCH_DEBUG"):
            import torch.cuda.tunable as _tun
            print(f"[debug] warmup {time.perf_counter() - t_w0:.1f}s, "
                  f"tunable enabled={_tun.is_enabled()} "
                  f"results={len(_tun.get_results())}", file=sys.stderr)

    # hipGraph-capture the whole training step (see train/graph_step.py).
    # Gated on an RCCL backend when DP is active: gloo collectives
    # invalidate the capture AND leave the stream wedged in capture state
    # (verified on hardware) — RCCL supports capture.
    graphed = None
    capture_safe = dist is None or dist.get_backend() == "nccl"
    if (use_gpu and capture_safe
            and os.environ.get("CHINESENER_NO_STEPGRAPH") != "1"):
        import logging
        logging.basicConfig(level=logging.INFO, stream=sys.stderr)
        from chinesener_amd.train.graph_step import GraphedTrainStep
        from chinesener_amd.train.optimizers import clip_gradients as _clip
        g = GraphedTrainStep(model, opt, schedule,
                             lambda m: _clip(m, family), dp=dp, cast=cast)
        ok = g.try_capture(batches[0])
        if dist is not None:
            # every rank must agree graph-vs-eager or the collective
            # schedules diverge and the job deadlocks
            flag = torch.tensor([1 if ok else 0], device=device)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            if not bool(flag.item()):
                if ok:
                    g.release()          # drops graph + graph-mode caches
                else:
                    opt.lr_dev = None
                ok = False
                # a rank whose capture FAILED skipped the post-capture
                # param restore (its warmup passes applied real updates)
                # — re-sync params from rank 0 and restart optimizer
                # state so all ranks continue identically
                with torch.no_grad():
                    for p in model.parameters():
                        dist.broadcast(p.data, src=0)
                opt.state.clear()
                if hasattr(opt, "_meta_cache"):
                    opt._meta_cache = {}
                if hasattr(model, "_clip_meta"):
                    model._clip_meta = None
        if ok and dist is not None and world > 1:
            # The captured DP body end-launches its collectives
            # (autograd.grad fires no hooks), losing backward/comm
            # overlap; eager keeps the bucket-hook overlap. Measure both
            # and keep the faster — every rank sees the same reduced
            # timings, so the choice stays collective-consistent.
            def _timed(fn, n=5):
                dist.barrier()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(n):
                    fn(batches[i % len(batches)])
                dist.barrier()
                torch.cuda.synchronize()
                t = torch.tensor([time.perf_counter() - t0], device=device)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                return float(t.item())

            t_graph = _timed(lambda b: g.replay(b, 1))
            t_eager = _timed(train_step)
            if t_eager < t_graph:
                g.release()
                ok = False
                if rank == 0:
                    print(f"[bench] eager DP ({t_eager:.3f}s/5) beats "
                          f"graphed ({t_graph:.3f}s/5); using eager",
                          file=sys.stderr)
        if ok:
            graphed = g

    def graph_train_step(batch):
        nonlocal step_num
        step_num += 1
        return graphed.replay(batch, step_num)

    if graphed is not None:
        train_step = graph_train_step
    if dist is not None:
        dist.barrier()
    if use_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    last_loss = None
    for i in range(args.steps):
        last_loss = train_step(batches[i % len(batches)])
    if dist is not None:
        dist.barrier()
    if use_gpu:
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    # max over ranks
    if dist is not None:
        t = torch.tensor([elapsed], device=device if use_gpu else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    if rank == 0:
        if args.dump_outputs and last_loss is not None:
            dump_outputs(args.dump_outputs, last_loss, model)
        total_samples = args.steps * args.batch_size * world
        result = {
            "metric": f"training samples/sec, {args.model} (BERT-base + BiLSTM + CRF), msra-shaped"
                      if args.model == "bert_bilstm_crf"
                      else f"training samples/sec, {args.model}, msra-shaped",
            "value": round(total_samples / elapsed, 2),
            "unit": "samples/sec",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1000, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16" if use_bf16 else "fp32",
            "data": "synthetic",
            "config": {"model": args.model,
                       "global_batch": args.batch_size * world,
                       "seq_len": args.seq_len,
                       "parallelism": f"dp{world}"},
        }
        print(json.dumps(result))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
