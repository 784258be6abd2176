"""Fused AdamW step over a flat parameter space (optim/fused.py FusedAdamW, optim.hip
adamw_kernel / adamw_bf16state_kernel): time per step and the HBM rate it reaches.  Bytes per
parameter: 30 with fp32 state (read p, g, m, v; write p, m, v and the bf16 shadow), 22 with
bf16 state (m and v are 2 B each way).  Sizes: GPT-2-small (124.4 M) and Llama-3-8B (8.03 B).

    python benchmarks/optim_bench.py [--params 124.4e6,8.03e9] [--reps 10] [--state-dtype fp32|bf16|both]

`--state-dtype both`: an A/B in one process - two optimizers over the SAME parameter, gradient
and shadow buffers (each with its own state) stepped in alternating timed windows of at least
`--window-ms`, `--rounds` rounds; per variant the median and the min-max spread over the rounds.

`--capturable both`: an alternating A/B of the host-scalar kernel and the device-table kernel
(capturable=True: lr and the bias corrections read from tables by a device step counter) over one
optimizer's buffers, with and without the one-thread counter increment that ends a capturable
step; fp32 state unless `--state-dtype bf16`.
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


def _capturable_ab(args, n, params, kind):
    """Alternating A/B of the host-scalar and the device-table kernel over the SAME buffers (one
    optimizer's parameters, gradients, state, shadow and chunk table): `host` = ext.adamw with
    lr and the bias corrections by value, `dev` = ext.adamw_dev reading them from the tables,
    `dev+advance` = the same followed by the counter increment that ends a capturable step."""
    import math

    from ray_torch_distributed_checkpoint_amd.ops._ext import gpu_ext
    from ray_torch_distributed_checkpoint_amd.optim import FusedAdamW, LRSchedule

    b1, b2, eps, wd, t = 0.9, 0.95, 1e-8, 0.1, 2
    opt = FusedAdamW(params, lr=1e-4, betas=(b1, b2), eps=eps, weight_decay=wd, state_dtype=DTYPES[kind],
                     lr_schedule=LRSchedule.warmup_cosine(100, 100000), capturable=True)
    for p in params:
        p.grad = torch.randn_like(p)
    opt.step()  # state, chunk table, device tables; the device counter now holds 1
    ext, sp, dv = gpu_ext(), opt.flat_space, opt._dev
    chunks, nc = sp.chunk_table(params, [True] * len(params))
    m, v = opt._bufs["exp_avg"], opt._bufs["exp_avg_sq"]
    lr = opt.lr_schedule.lr(1e-4, t)

    def host():
        ext.adamw(chunks, nc, sp.data, sp.grad, m, v, sp.shadow, lr, b1, b2, eps, wd, 1 - b1 ** t,
                  math.sqrt(1 - b2 ** t), 1.0, 0, 0, 0, t)

    def dev():
        ext.adamw_dev(chunks, nc, sp.data, sp.grad, m, v, sp.shadow, dv["count"], dv["lr"], 0, dv["bc"][(b1, b2)], 0,
                      b1, b2, eps, wd, 1.0, 0, 0, 0)

    def dev_advance():
        dev()
        ext.optim_step_advance(dv["count"])

    fns = {"host": host, "dev": dev, "dev+advance": dev_advance}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def window(fn, reps):
        dv["count"].fill_(1)  # every window computes step 2 (the same table rows as `host`)
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / reps

    reps = {k: max(args.reps, int(args.window_ms / window(f, 3)) + 1) for k, f in fns.items()}
    ms = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, f in fns.items():
            ms[k].append(window(f, reps[k]))
    med = {k: statistics.median(x) for k, x in ms.items()}
    for k in fns:
        print(json.dumps({"params": n, "state": kind, "path": k, "ms": round(med[k], 4), "ms_min": round(min(ms[k]), 4),
                          "ms_max": round(max(ms[k]), 4),
                          "spread_pct": round(100 * (max(ms[k]) - min(ms[k])) / med[k], 2),
                          "TBps": round(BYTES[kind] * n / (med[k] * 1e-3) / 1e12, 3), "reps": reps[k],
                          "rounds": args.rounds}), flush=True)
    print(json.dumps({"params": n, "state": kind,
                      "dev_minus_host_pct": round(100 * (med["dev"] - med["host"]) / med["host"], 3),
                      "dev_advance_minus_host_pct": round(100 * (med["dev+advance"] - med["host"]) / med["host"], 3),
                      "dev_advance_minus_host_us": round(1e3 * (med["dev+advance"] - med["host"]), 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", default="124.4e6,8.03e9")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--state-dtype", default="fp32", choices=["fp32", "bf16", "both"])
    ap.add_argument("--capturable", default="off", choices=["off", "both"],
                    help="both: A/B of the host-scalar and the device-table (capturable=True) step")
    ap.add_argument("--rounds", type=int, default=7, help="A/B rounds (--state-dtype both, --capturable both)")
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
        if args.capturable == "both":
            _capturable_ab(args, n, params, "fp32" if args.state_dtype == "both" else args.state_dtype)
            del params
            torch.cuda.empty_cache()
            continue
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
