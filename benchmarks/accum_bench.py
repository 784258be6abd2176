"""Cost of in-place gradient accumulation (optim.GradAccumulator), A/B in one process on the
same buffers: the variants alternate within each of `--rounds` rounds, every timed window is
at least 120 ms of device-event time, the median over the rounds is reported with min..max.

(a) the grouped weight-gradient launch (gemm_bf16_grouped), overwriting vs accumulating:
    GPT-2's eight products of two layers at M = 16384 tokens, and the four products of a
    Llama-3-8B layer at M = 2048;
(b) one micro-batch forward + backward of gpt2-small (16 x 1024) and llama3-1b (1 x 2048):
    fresh    the single-backward step of today (gradients written into the flat buffer)
    inplace  a later micro-batch of an accumulated step (kernels add into the flat buffer)
    legacy   a second backward with p.grad kept: every op allocates, autograd adds
    with torch.cuda.max_memory_allocated over one such backward for the last two.

    python benchmarks/accum_bench.py [--rounds 7] [--part a|b|ab] [--models gpt2-small,llama3-1b]
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

WINDOW_MS = 120.0


def _time(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _ab(variants: dict, rounds: int) -> dict:
    """variants: {name: (setup or None, body)}; setup runs untimed before every window of its
    variant.  {name: (median ms, min ms, max ms, reps)}."""
    reps = {}
    for name, (setup, fn) in variants.items():
        if setup:
            setup()
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        est = _time(fn, 3)
        reps[name] = max(3, int(math.ceil(WINDOW_MS / max(est, 1e-3))))
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, (setup, fn) in variants.items():
            if setup:
                setup()
                torch.cuda.synchronize()
            times[name].append(_time(fn, reps[name]))
    return {name: (statistics.median(t), min(t), max(t), reps[name]) for name, t in times.items()}


def _row(tag, name, res, **extra):
    med, lo, hi, reps = res
    print(json.dumps({"bench": tag, "variant": name, "ms": round(med, 4), "ms_min": round(lo, 4),
                      "ms_max": round(hi, 4), "reps": reps, **extra}), flush=True)


GPT2_SHAPES = [(2304, 768), (768, 768), (3072, 768), (768, 3072)]
LLAMA8B_SHAPES = [(6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336)]  # wqkv, wo, w13, w2


def bench_grouped(tag, shapes, M, rounds):
    from ray_torch_distributed_checkpoint_amd.ops._ext import gpu_ext

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    dys = [torch.randn(M, n, device=dev).bfloat16() for n, _ in shapes]
    xs = [(torch.randn(M, k, device=dev) * 0.01).bfloat16() for _, k in shapes]
    outs = [torch.zeros(n, k, device=dev) for n, k in shapes]
    dims = []
    for n, k in shapes:
        dims += [n, k, M, n, k, k]
    ext = gpu_ext()
    ones = [1] * len(shapes)
    res = _ab({"overwrite": (None, lambda: ext.gemm_bf16_grouped(dys, xs, outs, dims, False, False)),
               "accumulate": (None, lambda: ext.gemm_bf16_grouped(dys, xs, outs, dims, False, False, ones))}, rounds)
    tiles = sum(((n + 255) // 256) * ((k + 255) // 256) for n, k in shapes)
    flops = 2.0 * M * sum(n * k for n, k in shapes)
    for name, r in res.items():
        _row(tag, name, r, M=M, products=len(shapes), tiles=tiles, TFLOPs=round(flops / (r[0] * 1e-3) / 1e12, 1))


def bench_micro_batch(model_name, rounds):
    from ray_torch_distributed_checkpoint_amd.ops.gemm import flush_wgrads
    from ray_torch_distributed_checkpoint_amd.optim import FlatParamSpace

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    if model_name.startswith("gpt2"):
        from ray_torch_distributed_checkpoint_amd.models import GPT2, GPT2Config

        cfg = GPT2Config.named(model_name)
        model, B, T, vocab = GPT2(cfg).to(dev), 16, 1024, cfg.vocab_size
    else:
        from ray_torch_distributed_checkpoint_amd.models import Llama, LlamaConfig

        cfg = LlamaConfig.named(model_name)
        model, B, T, vocab = Llama(cfg, device=dev), 1, 2048, cfg.vocab_size
    sp = FlatParamSpace(list(reversed(list(model.parameters()))))
    data = torch.randint(0, vocab, (B, T + 1), device=dev)
    x, y = data[:, :-1].contiguous(), data[:, 1:].contiguous()

    def fwd_bwd():
        model(x, y).backward()

    def first():  # the first micro-batch of a step: gradients written, p.grad attached
        flush_wgrads()
        sp.zero_grad(set_to_none=True)
        fwd_bwd()

    def inplace():
        sp.next_micro_step()
        fwd_bwd()
        flush_wgrads()
        sp.fold_grads()

    res = _ab({"fresh": (None, first), "inplace": (first, inplace), "legacy": (first, fwd_bwd)}, rounds)
    peaks = {}
    for name in ("inplace", "legacy"):  # memory over the second BACKWARD alone (forward done, peak reset)
        first()
        if name == "inplace":
            sp.next_micro_step()
        loss = model(x, y)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        total0 = torch.cuda.memory_stats(dev)["allocated_bytes.all.allocated"]
        loss.backward()
        if name == "inplace":
            flush_wgrads()
            sp.fold_grads()
        torch.cuda.synchronize()
        del loss
        # (peak: the largest live set; requested: every byte the caching allocator handed out)
        peaks[name] = (torch.cuda.max_memory_allocated(dev), base,
                       torch.cuda.memory_stats(dev)["allocated_bytes.all.allocated"] - total0)
    sp.zero_grad(set_to_none=True)
    for name, r in res.items():
        extra = {}
        if name in peaks:
            peak, base, req = peaks[name]
            extra = {"peak_alloc_MiB": round(peak / 2 ** 20, 1), "peak_over_start_MiB": round((peak - base) / 2 ** 20, 1),
                     "requested_MiB": round(req / 2 ** 20, 1)}
        _row("micro_batch " + model_name, name, r, batch=B, seq_len=T, **extra)
    print(json.dumps({"bench": "micro_batch " + model_name,
                      "inplace_minus_fresh_ms": round(res["inplace"][0] - res["fresh"][0], 4),
                      "inplace_minus_legacy_ms": round(res["inplace"][0] - res["legacy"][0], 4),
                      "fresh_spread_ms": round(res["fresh"][2] - res["fresh"][1], 4)}), flush=True)
    del model, sp
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--part", default="ab")
    ap.add_argument("--models", default="gpt2-small,llama3-1b")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("accum_bench needs a GPU")
    print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}", flush=True)
    if "a" in args.part:
        bench_grouped("grouped gpt2 2 layers", GPT2_SHAPES * 2, 16384, args.rounds)
        bench_grouped("grouped llama3-8b layer", LLAMA8B_SHAPES, 2048, args.rounds)
    if "b" in args.part:
        for m in args.models.split(","):
            bench_micro_batch(m, args.rounds)


if __name__ == "__main__":
    main()
