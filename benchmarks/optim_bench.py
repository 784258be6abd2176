"""Fused AdamW step over a flat parameter space (optim/fused.py FusedAdamW, optim.hip
adamw_kernel / adamw_bf16state_kernel): time per step and the HBM rate it reaches.  Bytes per
parameter: 30 with fp32 state (read p, g, m, v; write p, m, v and the bf16 shadow), 22 with
bf16 state (m and v are 2 B each way).  Sizes: GPT-2-small (124.4 M) and Llama-3-8B (8.03 B).

    python benchmarks/optim_bench.py [--params 124.4e6,8.03e9] [--reps 10] [--state-dtype fp32|bf16|both]

`--state-dtype both`: an A/B in one process - two optimizers over the SAME parameter, gradient
and shadow buffers (each with its own state) stepped in alternating timed windows of at least
`--window-ms`, `--rounds` rounds; per variant the median and the min-max spread over the rounds.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BYTES = {"fp32": 30.0, "bf16": 22.0}
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _window(opt, reps, ev):
    ev[0].record()
    for _ in range(reps):
        opt.step()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", default="124.4e6,8.03e9")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--state-dtype", default="fp32", choices=["fp32", "bf16", "both"])
    ap.add_argument("--rounds", type=int, default=7, help="A/B rounds (--state-dtype both)")
    ap.add_argument("--window-ms", type=float, default=120.0, help="least length of a timed A/B window")
    args = ap.parse_args()
    from ray_torch_distributed_checkpoint_amd.optim import FusedAdamW

    dev = torch.device("cuda", 0)
    kinds = ["fp32", "bf16"] if args.state_dtype == "both" else [args.state_dtype]
    for n in (int(float(x)) for x in args.params.split(",")):
        # parameter shapes like a transformer's: square-ish matrices of ~n/64 elements
        per = max(1 << 16, n // 64)
        shapes, left = [], n
        while left > 0:
            k = min(per, left)
            shapes.append(k)
            left -= k
        params = [torch.nn.Parameter(torch.randn(k, device=dev) * 0.02) for k in shapes]
        opts = {k: FusedAdamW(params, lr=1e-4, weight_decay=0.1, state_dtype=DTYPES[k]) for k in kinds}
        for p in params:
            p.grad = torch.randn_like(p)
        for opt in opts.values():
            opt.step()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        if len(kinds) == 1:
            (kind, opt), = opts.items()
            best = min(_window(opt, args.reps, ev) for _ in range(3))
            row = {"params": n, "state": kind, "ms": round(best, 3),
                   "TBps": round(BYTES[kind] * n / (best * 1e-3) / 1e12, 2)}
            print(json.dumps(row), flush=True)
        else:
            reps = {k: max(args.reps, int(args.window_ms / _window(o, 3, ev)) + 1) for k, o in opts.items()}
            ms = {k: [] for k in kinds}
            for _ in range(args.rounds):
                for k in kinds:
                    ms[k].append(_window(opts[k], reps[k], ev))
            for k in kinds:
                med = statistics.median(ms[k])
                row = {"params": n, "state": k, "ms": round(med, 4), "ms_min": round(min(ms[k]), 4),
                       "ms_max": round(max(ms[k]), 4), "spread_pct": round(100 * (max(ms[k]) - min(ms[k])) / med, 2),
                       "TBps": round(BYTES[k] * n / (med * 1e-3) / 1e12, 3), "bytes_per_param": BYTES[k],
                       "reps": reps[k], "rounds": args.rounds}
                print(json.dumps(row), flush=True)
            a, b = statistics.median(ms["fp32"]), statistics.median(ms["bf16"])
            print(json.dumps({"params": n, "bf16_over_fp32_time": round(b / a, 4), "bytes_ratio": round(22 / 30, 4)}),
                  flush=True)
        del params, opts
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
