"""Gradient-norm pass of the fused clipping (optim.hip gradnorm_partial_kernel +
gradnorm_finalize_kernel) against the project's own streaming yardstick and against torch, in
one process on the same buffers.

Per flat gradient size (GPT-2-small 124.4 M elements, a Llama-3-8B 1/8 ZeRO shard 1.004 G,
ResNet-18 11.7 M):

  norm   the new pass: per-chunk partial sums + finalize        reads 4 B / element
  adamw  ext.adamw on the same buffers (the existing update)     moves 30 B / element
  vnorm  torch.linalg.vector_norm(flat_grad)                     reads 4 B / element
  clip   torch.nn.utils.clip_grad_norm_ over the per-parameter   12 B / element (reads the
         views (what a user would otherwise call)                gradients, then read-modify-writes)

then the time of a whole GPT-2-small optimizer step (real parameter shapes) with clipping
off, on, and off + clip_grad_norm_ in front.  Times are device-event times of `reps`
back-to-back calls after a warm-up; the variants alternate within each of `--rounds` rounds and
the median over the rounds is reported with the min..max spread.

    python benchmarks/gradnorm_bench.py [--sizes 124.4e6,1.004e9,11.7e6] [--rounds 7]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _ab(variants: dict, rounds: int, window_ms: float = 60.0) -> dict:
    """{name: (median ms, min ms, max ms, reps)}; every variant warmed up, reps sized so one
    timed window is ~window_ms, variants alternating within each round."""
    reps = {}
    for name, fn in variants.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        est = _time(fn, 5)
        reps[name] = max(5, min(2000, int(window_ms / max(est, 1e-3))))
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(_time(fn, reps[name]))
    return {name: (statistics.median(t), min(t), max(t), reps[name]) for name, t in times.items()}


def bench_size(n: int, rounds: int) -> None:
    from ray_torch_distributed_checkpoint_amd.ops._ext import gpu_ext
    from ray_torch_distributed_checkpoint_amd.optim import FusedAdamW

    dev = torch.device("cuda", 0)
    ext = gpu_ext()
    # parameter shapes like a transformer's: ~n/64 elements each (benchmarks/optim_bench.py)
    per = max(1 << 16, n // 64)
    shapes, left = [], n
    while left > 0:
        k = min(per, left)
        shapes.append(k)
        left -= k
    params = [torch.nn.Parameter(torch.randn(k, device=dev) * 0.02) for k in shapes]
    opt = FusedAdamW(params, lr=1e-4, weight_decay=0.1)
    for p in params:
        p.grad = torch.randn_like(p)
    opt.step()  # builds the flat space and the state; p.grad become views of the flat buffer
    sp = opt.flat_space
    chunks, nch = sp.chunk_table(params, [True] * len(params))
    partial = torch.zeros(nch, dtype=torch.float64, device=dev)  # (the kernels carry the sums in fp64)
    out = torch.zeros(2, dtype=torch.float32, device=dev)
    m, v = opt._bufs["exp_avg"], opt._bufs["exp_avg_sq"]
    flat = sp.grad[:sp.numel]

    def norm():
        ext.gradnorm_partial(chunks, nch, sp.grad, partial, 0)
        ext.gradnorm_finalize(partial, nch, 1.0, 1.0, out)

    def adamw():
        ext.adamw(chunks, nch, sp.data, sp.grad, m, v, sp.shadow, 1e-4, 0.9, 0.999, 1e-8, 0.1, 0.1,
                  math.sqrt(0.001), 1.0, 0)

    def vnorm():
        torch.linalg.vector_norm(flat)

    def clip():  # (max_norm far above the norm: the gradients keep their values; torch multiplies anyway)
        torch.nn.utils.clip_grad_norm_(params, 1e9)

    norm()
    torch.cuda.synchronize()
    ref = float(torch.linalg.vector_norm(flat.double()))
    got = float(out[0])
    res = _ab({"norm": norm, "adamw": adamw, "vnorm": vnorm, "clip": clip}, rounds)
    bytes_per = {"norm": 4.0, "adamw": 30.0, "vnorm": 4.0, "clip": 12.0}
    print(f"# flat gradient of {n} elements ({len(params)} parameters, {nch} chunks); "
          f"norm {got:.6f} vs float64 {ref:.6f} (rel {abs(got - ref) / ref:.1e})", flush=True)
    for name, (med, lo, hi, reps) in res.items():
        gbs = bytes_per[name] * n / (med * 1e-3) / 1e9
        print(json.dumps({"elements": n, "pass": name, "ms": round(med, 4), "ms_min": round(lo, 4),
                          "ms_max": round(hi, 4), "reps": reps, "bytes_per_element": bytes_per[name],
                          "GBps": round(gbs, 1)}), flush=True)
    del params, opt, sp, m, v, flat, partial
    torch.cuda.empty_cache()


def bench_gpt2_step(rounds: int) -> None:
    from ray_torch_distributed_checkpoint_amd.models import GPT2, GPT2Config
    from ray_torch_distributed_checkpoint_amd.optim import FusedAdamW

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = GPT2(GPT2Config.named("gpt2-small")).to(dev)
    params = list(model.parameters())
    opt = FusedAdamW(params, lr=1e-4, betas=(0.9, 0.95), weight_decay=0.1)
    for p in params:
        p.grad = torch.randn_like(p) * 0.01
    opt.step()

    def off():
        opt.max_grad_norm = None
        opt.step()

    def on():
        opt.max_grad_norm = 1.0
        opt.step()

    def off_torch_clip():
        opt.max_grad_norm = None
        torch.nn.utils.clip_grad_norm_(params, 1e9)
        opt.step()

    res = _ab({"step_clip_off": off, "step_clip_on": on, "step_clip_off+clip_grad_norm_": off_torch_clip}, rounds)
    n = sum(p.numel() for p in params)
    print(f"# GPT-2-small optimizer step, {n} parameters in {len(params)} tensors (host work included)", flush=True)
    for name, (med, lo, hi, reps) in res.items():
        print(json.dumps({"step": name, "ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                          "reps": reps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="124.4e6,1.004e9,11.7e6")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gradnorm_bench needs a GPU")
    print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}", flush=True)
    for n in (int(float(x)) for x in args.sizes.split(",")):
        bench_size(n, args.rounds)
    if not args.no_step:
        bench_gpt2_step(args.rounds)


if __name__ == "__main__":
    main()
