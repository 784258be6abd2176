"""Fused LM-head cross-entropy kernel on the GPT-2 logits shape ([16384, 50304] bf16, 50257
real columns, gradient written in place): register-resident single-read kernel vs the
two-pass kernel (RTDC_XENT_TWO_PASS=1), interleaved rounds in one process.

    python benchmarks/xent_bench.py [--rows 16384] [--reps 20]

`--aux` instead alternates the plain kernel and the one with label smoothing + z-loss
(xent.hip, AUX instantiations) on ONE buffer, in place, in one process: `--rounds` rounds, every
timed window at least `--window-ms` (both kernels are warmed, then one `reps` for both grows until
each one's window is that long; every window's length is printed and a short one is an error); per
kernel the median and the min-max spread over the rounds, then the ratio of the medians.  The two
move the same bytes.

    python benchmarks/xent_bench.py --aux                                   # GPT-2: 16384 x 50304, V 50257
    python benchmarks/xent_bench.py --aux --rows 2048 --V 128256 --ld 128256   # Llama-3
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ray_torch_distributed_checkpoint_amd.ops._ext import gpu_ext  # noqa: E402


def aux_ab(a):
    """plain vs label smoothing + z-loss, alternating on the same buffer"""
    torch.manual_seed(0)
    x0 = (torch.randn(a.rows, a.ld, device="cuda") * 2).bfloat16()
    tgt = torch.randint(0, a.V, (a.rows,), device="cuda")
    loss = torch.empty(a.rows, device="cuda")
    ce = torch.empty(a.rows, device="cuda")
    ext = gpu_ext()
    buf = x0.clone()
    gs = 1.0 / a.rows

    def plain():
        ext.xent(buf, buf, tgt, loss, None, None, a.rows, a.V, a.ld, gs, -100)

    def aux():
        ext.xent(buf, buf, tgt, loss, None, None, a.rows, a.V, a.ld, gs, -100, label_smoothing=a.label_smoothing,
                 z_loss=a.z_loss, ce=ce)

    fns = {"plain": plain, "aux": aux}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def window(fn, reps):
        """(us per call, ms of the whole window)"""
        buf.copy_(x0)  # every window starts from the logits (a call leaves its gradient in the buffer)
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        t = ev[0].elapsed_time(ev[1])
        return t / reps, t

    # Both kernels are loaded and warm before anything is sized.  `reps` is ONE number for both arms (the
    # slower arm's warmed estimate plus 10 %), grown until each arm's calibration window reaches window_ms;
    # every timed window's own length is kept and checked below.
    for f in fns.values():
        window(f, 10)
    reps = max(a.reps, int(1.1 * a.window_ms / min(window(f, 10)[0] for f in fns.values())) + 1)
    while min(window(f, reps)[1] for f in fns.values()) < a.window_ms:
        reps = int(reps * 1.25) + 1
    ms = {k: [] for k in fns}
    win = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, f in fns.items():
            per, t = window(f, reps)
            ms[k].append(per)
            win[k].append(t)
    med = {k: statistics.median(v) for k, v in ms.items()}
    nbytes = 2 * a.rows * a.ld * 2
    for k in fns:
        print(json.dumps({"rows": a.rows, "V": a.V, "ld": a.ld, "kernel": k, "us": round(med[k] * 1e3, 2),
                          "us_min": round(min(ms[k]) * 1e3, 2), "us_max": round(max(ms[k]) * 1e3, 2),
                          "spread_pct": round(100 * (max(ms[k]) - min(ms[k])) / med[k], 2),
                          "TBps_rw": round(nbytes / (med[k] * 1e-3) / 1e12, 3), "reps": reps,
                          "rounds": a.rounds, "window_ms_min": round(min(win[k]), 1),
                          "window_ms_max": round(max(win[k]), 1)}), flush=True)
    print(json.dumps({"rows": a.rows, "V": a.V, "ld": a.ld, "label_smoothing": a.label_smoothing, "z_loss": a.z_loss,
                      "aux_over_plain": round(med["aux"] / med["plain"], 4),
                      "aux_minus_plain_pct": round(100 * (med["aux"] - med["plain"]) / med["plain"], 3)}), flush=True)
    short = {k: round(min(v), 1) for k, v in win.items() if min(v) < a.window_ms}
    if short:
        raise SystemExit(f"timed window shorter than {a.window_ms} ms: {short}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--V", type=int, default=50257)
    ap.add_argument("--ld", type=int, default=50304)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--aux", action="store_true", help="A/B of the plain kernel and the label-smoothing + z-loss one")
    ap.add_argument("--label-smoothing", type=float, default=0.1)
    ap.add_argument("--z-loss", type=float, default=1e-4)
    ap.add_argument("--rounds", type=int, default=7, help="A/B rounds (--aux)")
    ap.add_argument("--window-ms", type=float, default=120.0, help="least length of a timed window (--aux)")
    a = ap.parse_args()
    if a.aux:
        return aux_ab(a)
    torch.manual_seed(0)
    x0 = (torch.randn(a.rows, a.ld, device="cuda") * 2).bfloat16()
    tgt = torch.randint(0, a.V, (a.rows,), device="cuda")
    loss = torch.empty(a.rows, device="cuda")
    ext = gpu_ext()
    res = {"rows": a.rows, "ld": a.ld}
    bufs = {k: x0.clone() for k in ("reg", "two_pass")}
    times = {k: [] for k in bufs}
    for _ in range(5):
        for k, buf in bufs.items():
            if k == "two_pass":
                os.environ["RTDC_XENT_TWO_PASS"] = "1"
            else:
                os.environ.pop("RTDC_XENT_TWO_PASS", None)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                buf.copy_(x0) if False else None
                ext.xent(buf, buf, tgt, loss, None, None, a.rows, a.V, a.ld, 1.0 / a.rows, -100)
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.reps * 1e3)
    os.environ.pop("RTDC_XENT_TWO_PASS", None)
    nbytes = 2 * a.rows * a.ld * 2
    for k, ts in times.items():
        t = sorted(ts)[len(ts) // 2]
        res[f"{k}_us"] = round(t, 1)
        res[f"{k}_TBps_rw"] = round(nbytes / (t * 1e-6) / 1e12, 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
