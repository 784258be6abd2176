"""Decode attention (split-KV kernel, csrc/kernels/attn_decode.hip, bf16 and FP8 cache) and generate() benchmark.

    python benchmarks/decode_bench.py [--rounds 7] [--window-ms 20] [--only llama8b] [--no-generate] [--out FILE]
    python benchmarks/decode_bench.py --fast [--fast-out FILE]      # the few-row / captured tables only

Kernel part: one decode launch (the decode kernel and its merge) per shape, next to
F.scaled_dot_product_attention on the same cache - one process, same buffers, the two arms
alternating over --rounds rounds, every timed window at least --window-ms long; median and minimum
per arm.  Achieved bytes/s = the K and V bytes of the cached keys (read once) / time, reported as
a share of this box's device-to-device copy rate (read + write bytes of a 1 GiB copy / time), which
is measured first in the same process.
Model part: tokens per second of generate() for gpt2-small and llama3-1b (random weights), and
the attention share of one decode step: the step's decode_attention calls timed alone at the same
cache length against the whole step.
--fast adds (and --fast-only runs alone) the two tables of profiles/decode_fast.md:
(a) per linear, `linear_few_rows` against `linear_fwd` on rows padded to a multiple of 8, alternating
on the same buffers, for every distinct (N, K) of a gpt2-small, llama3-1b and llama3-8b decode step
at M = 1, 8, 16: microseconds (median, and the min .. max spread over the rounds), weight bytes /
time and its share of the copy rate (both arms allocate their output per call); a shape where the few-row median is not below the tile
median by more than the larger of the two spreads is marked lost;
(b) per decode step and generate() tokens/s for gpt2-small and llama3-1b at B = 1 and 8, four arms:
eager / captured x tile / few-row (eager-tile is the path of the tables above);
(c) the FP8 tables of profiles/decode_fast_fp8.md: in (a)'s loop `linear_few_rows_fp8` on the per-row
e4m3 image of the same weight alternates with the bf16 few-row kernel and with a second arm of that
same bf16 kernel (its ratio to the first is the spread a ratio has to beat); weight bytes are
N K + 4 N (codes and scales) against 2 N K; in (b)'s loop two more arms, eager / captured with
weights="fp8".
--kv-cache fp8 runs the tables of profiles/decode_fp8_kv.md alone (--kv-out FILE): per SHAPES row the
FP8-cache decode kernel (the same file's e4m3 instantiations) alternating with the bf16 kernel on the same
values (the FP8 cache is the quantised bf16 one), bytes = the cached keys' K and V bytes plus, for FP8,
their scales, over the copy rate; then per decode step and generate() tokens/s of gpt2-small and
llama3-1b at B = 1 and 8 with the bf16 and the FP8 cache, eager, and together with captured few-row
weights="fp8".  An FP8 median not below the bf16 median by more than the larger spread is marked LOST.
Prints one JSON line per measurement and a markdown table at the end (--out: also to a file).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from statistics import median

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ray_torch_distributed_checkpoint_amd.ops._ext import gpu_ext  # noqa: E402
from ray_torch_distributed_checkpoint_amd.ops.decode import decode_splits  # noqa: E402
from ray_torch_distributed_checkpoint_amd.ops.llama_ops import rope_tables  # noqa: E402

# name, B, cached length, H, Hkv, Dh, rope
SHAPES = [("llama8b", 1, 2048, 32, 8, 128, True), ("llama8b", 1, 8192, 32, 8, 128, True),
          ("llama8b", 8, 2048, 32, 8, 128, True), ("llama8b", 8, 8192, 32, 8, 128, True),
          ("gpt2", 16, 1024, 12, 12, 64, False)]
DEV = "cuda"


def window(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e-3 / reps


def reps_for(fn, window_ms):
    fn()
    torch.cuda.synchronize()
    t = window(fn, 5)
    return max(5, int(window_ms * 1e-3 / max(t, 1e-7)) + 1)


def ab(arms: dict, rounds, window_ms):
    """alternating rounds; {arm: (median s, min s, reps)}"""
    reps = {k: reps_for(f, window_ms) for k, f in arms.items()}
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, f in arms.items():
            times[k].append(window(f, reps[k]))
    return {k: (median(v), min(v), reps[k], max(v)) for k, v in times.items()}


def copy_rate(rounds, window_ms):
    n = 1 << 30
    a = torch.empty(n, dtype=torch.uint8, device=DEV)
    b = torch.empty_like(a)
    med = ab({"copy": lambda: b.copy_(a)}, rounds, window_ms)["copy"][0]
    return 2 * n / med


def kernel_rows(args, rate):
    ext = gpu_ext()
    rows = []
    for name, B, L, H, Hkv, Dh, rope in SHAPES:
        if args.only and name != args.only:
            continue
        Tmax = L + 64
        W = (H + 2 * Hkv) * Dh
        qkv_new = (torch.randn(B, W, device=DEV) * 0.5).bfloat16()
        cache = (torch.randn(B, Tmax, 2 * Hkv * Dh, device=DEV) * 0.5).bfloat16()
        pos = torch.full((B,), L, dtype=torch.int32, device=DEV)
        ns = decode_splits(B, Hkv, Tmax, torch.device(DEV))
        part = torch.empty(B * H * ns * (Dh + 2), dtype=torch.float32, device=DEV)
        out = torch.empty((B, H * Dh), dtype=torch.bfloat16, device=DEV)
        cos, sin = rope_tables(Tmax, Dh, 500000.0, DEV) if rope else (None, None)
        scale = Dh ** -0.5

        def native():
            ext.decode_attn(qkv_new, cache, pos, cos, sin, out, part, H, Hkv, 0, ns, scale)

        # SDPA on the same cache: strided views, keys 0 .. L (the new row is already stored)
        native()
        q = qkv_new[:, : H * Dh].view(B, H, 1, Dh)
        k = cache[:, : L + 1, : Hkv * Dh].view(B, L + 1, Hkv, Dh).transpose(1, 2)
        v = cache[:, : L + 1, Hkv * Dh:].view(B, L + 1, Hkv, Dh).transpose(1, 2)
        how = "enable_gqa"
        try:
            F.scaled_dot_product_attention(q, k, v, enable_gqa=True)

            def sdpa():
                F.scaled_dot_product_attention(q, k, v, enable_gqa=True)
        except (TypeError, RuntimeError):
            how = "k, v expanded to H heads beforehand"
            ke, ve = (t.repeat_interleave(H // Hkv, dim=1) for t in (k, v))

            def sdpa():
                F.scaled_dot_product_attention(q, ke, ve)
        r = ab({"native": native, "sdpa": sdpa}, args.rounds, args.window_ms)
        nbytes = B * L * 2 * Hkv * Dh * 2
        row = {"bench": "decode_attn", "shape": name, "B": B, "cached": L, "H": H, "Hkv": Hkv, "Dh": Dh, "nsplit": ns,
               "native_us_med": r["native"][0] * 1e6, "native_us_min": r["native"][1] * 1e6,
               "sdpa_us_med": r["sdpa"][0] * 1e6, "sdpa_us_min": r["sdpa"][1] * 1e6, "sdpa_how": how,
               "kv_bytes": nbytes, "native_GBps": nbytes / r["native"][0] * 1e-9,
               "share_of_copy_rate": nbytes / r["native"][0] / rate, "reps": [r["native"][2], r["sdpa"][2]]}
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def generate_rows(args):
    from ray_torch_distributed_checkpoint_amd.generate import build_model
    from ray_torch_distributed_checkpoint_amd.models.generation import new_cache
    from ray_torch_distributed_checkpoint_amd.ops import decode_attention

    rows = []
    for name, B, P, N in (("gpt2-small", 1, 64, 192), ("gpt2-small", 8, 64, 192), ("llama3-1b", 1, 64, 192),
                          ("llama3-1b", 8, 64, 192)):
        torch.manual_seed(0)
        model = build_model(name, DEV).eval()
        idx = torch.randint(0, model.cfg.vocab_size, (B, P), device=DEV)
        model.generate(idx, 8)                                   # warm-up: shadows, workspaces
        torch.cuda.synchronize()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            model.generate(idx, N)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        # one decode step at position P + N / 2, and its attention calls alone
        cache = new_cache(model, B, P + N, DEV)
        model.prefill(idx, cache)
        cache.pos.fill_(P + N // 2)
        cache.length = P + N // 2
        tok = idx[:, 0].contiguous()

        def step():
            model.decode_step(tok, cache)
            cache.advance(-1)

        c = model.cfg
        llama = hasattr(c, "n_kv_heads")
        H, Hkv, Dh, nl = ((c.n_heads, c.n_kv_heads, c.head_dim, c.n_layers) if llama
                          else (c.n_head, c.n_head, c.n_embd // c.n_head, c.n_layer))
        qkv = (torch.randn(B, (H + 2 * Hkv) * Dh, device=DEV) * 0.5).bfloat16()
        rope = rope_tables(cache.Tmax, Dh, c.rope_theta, DEV) if llama else None

        def attn():
            for li in range(nl):
                decode_attention(qkv, cache, li, H, Hkv, rope=rope)

        r = ab({"step": step, "attn": attn}, args.rounds, args.window_ms)
        row = {"bench": "generate", "model": name, "B": B, "prompt": P, "new_tokens": N,
               "tokens_per_s": B * N / median(ts), "s_per_generate_med": median(ts),
               "decode_step_us": r["step"][0] * 1e6, "attention_us": r["attn"][0] * 1e6,
               "attention_share": r["attn"][0] / r["step"][0]}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del model, cache
        torch.cuda.empty_cache()
    return rows


def linear_shapes():
    """(model, layer, N, K) of every linear of a decode step, one row per distinct (N, K) of a model"""
    from ray_torch_distributed_checkpoint_amd.models import GPT2Config, LlamaConfig

    out = []
    g = GPT2Config.named("gpt2-small")
    C = g.n_embd
    out += [("gpt2-small", n, N, K) for n, N, K in (("c_attn", 3 * C, C), ("attn c_proj", C, C), ("c_fc", 4 * C, C),
                                                    ("mlp c_proj", C, 4 * C), ("lm head", g.padded_vocab, C))]
    for name in ("llama3-1b", "llama3-8b"):
        c = LlamaConfig.named(name)
        D, Dh = c.dim, c.head_dim
        out += [(name, n, N, K) for n, N, K in (("wqkv", (c.n_heads + 2 * c.n_kv_heads) * Dh, D), ("wo", D, c.n_heads * Dh),
                                                ("w13", 2 * c.ffn_dim, D), ("w2", D, c.ffn_dim),
                                                ("output", c.padded_vocab, D))]
    seen, rows = set(), []
    for r in out:
        if (r[0], r[2], r[3]) not in seen:
            seen.add((r[0], r[2], r[3]))
            rows.append(r)
    return rows


def linear_rows(args, rate):
    from ray_torch_distributed_checkpoint_amd import ops
    from ray_torch_distributed_checkpoint_amd.ops import gemm as G

    rows = []
    for model, layer, N, K in linear_shapes():
        w = (torch.randn(N, K, device=DEV) * K ** -0.5).bfloat16()
        q, qs = ops.quantize_fp8_rows(w)
        for M in (1, 8, 16):
            Mp = -(-M // 8) * 8
            xp = torch.zeros(Mp, K, dtype=torch.bfloat16, device=DEV)
            xp[:M] = torch.randn(M, K, device=DEV).bfloat16()
            x = xp[:M]
            # both arms allocate their output per call, as the decode step does
            r = ab({"few": lambda: G.linear_few_rows(x, w), "tile": lambda: G.linear_fwd(xp, w),
                    "fp8": lambda: ops.linear_few_rows_fp8(x, q, qs), "few2": lambda: G.linear_few_rows(x, w)},
                   args.rounds, args.window_ms)
            (pm, pmin, preps, pmax), f2 = r["fp8"], r["few2"][0]
            fp8_bytes = N * K + 4 * N
            (fm, fmin, _, fmax), (tm, tmin, _, tmax) = r["few"], r["tile"]
            spread = max(fmax - fmin, tmax - tmin)
            row = {"bench": "few_rows_linear", "model": model, "layer": layer, "N": N, "K": K, "M": M,
                   "waves_per": list(gpu_ext().few_rows_plan(N, K)),
                   "few_us": [fm * 1e6, fmin * 1e6, fmax * 1e6], "tile_us": [tm * 1e6, tmin * 1e6, tmax * 1e6],
                   "weight_bytes": 2 * N * K, "few_GBps": 2 * N * K / fm * 1e-9, "tile_GBps": 2 * N * K / tm * 1e-9,
                   "few_share_of_copy_rate": 2 * N * K / fm / rate, "tile_share_of_copy_rate": 2 * N * K / tm / rate,
                   "lost": not fm < tm - spread,
                   "fp8_plan": list(gpu_ext().few_rows_fp8_plan(N, K)), "fp8_us": [pm * 1e6, pmin * 1e6, pmax * 1e6],
                   "fp8_weight_bytes": fp8_bytes, "fp8_GBps": fp8_bytes / pm * 1e-9,
                   "fp8_share_of_copy_rate": fp8_bytes / pm / rate, "few_over_fp8": fm / pm, "few_over_few2": fm / f2,
                   "fp8_window_ms": [pm * preps * 1e3, fm * r["few"][2] * 1e3],
                   "fp8_lost": not pm < fm - max(fmax - fmin, pmax - pmin)}
            print(json.dumps(row), flush=True)
            rows.append(row)
        del w, q, qs
        torch.cuda.empty_cache()
    return rows


# arm, few_row, captured, weights
ARMS = (("eager tile", False, False, "bf16"), ("eager few-row", True, False, "bf16"),
        ("captured tile", False, True, "bf16"), ("captured few-row", True, True, "bf16"),
        ("eager few-row fp8", True, False, "fp8"), ("captured few-row fp8", True, True, "fp8"))


def fast_rows(args):
    """per decode step and generate() tokens/s, eager / captured x tile / few-row"""
    from ray_torch_distributed_checkpoint_amd.generate import build_model
    from ray_torch_distributed_checkpoint_amd.models.generation import CapturedDecode, new_cache

    rows = []
    for name, B, P, N in (("gpt2-small", 1, 64, 192), ("gpt2-small", 8, 64, 192), ("llama3-1b", 1, 64, 192),
                          ("llama3-1b", 8, 64, 192)):
        torch.manual_seed(0)
        model = build_model(name, DEV).eval()
        idx = torch.randint(0, model.cfg.vocab_size, (B, P), device=DEV)
        tok = idx[:, 0].contiguous()
        cache = new_cache(model, B, P + N, DEV)
        model.prefill(idx, cache)
        cache.pos.fill_(P + N // 2)
        cache.length = P + N // 2
        steps, keep = {}, []
        for arm, few, cap, wts in ARMS:
            if cap:
                sess = CapturedDecode(model, cache, few_row=few, weights=wts)
                keep.append(sess)

                def step(sess=sess):
                    sess.step(tok)
                    cache.advance(-1)
            else:
                def step(few=few, wts=wts):
                    model.decode_step(tok, cache, few_row=few, weights=wts)
                    cache.advance(-1)
            steps[arm] = step
        r = ab(steps, args.rounds, args.window_ms)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(2000):
            keep[0]._check_weights()
        guard_us = (time.perf_counter() - t0) / 2000 * 1e6    # host cost of the per-step weight guard
        for arm, few, cap, wts in ARMS:
            model.generate(idx, 8, few_row=few, captured=cap, weights=wts)       # warm-up
            torch.cuda.synchronize()
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                model.generate(idx, N, few_row=few, captured=cap, weights=wts)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            med, mn, _, mx = r[arm]
            row = {"bench": "decode_fast", "model": name, "B": B, "prompt": P, "new_tokens": N, "arm": arm,
                   "step_us": [med * 1e6, mn * 1e6, mx * 1e6], "tokens_per_s": B * N / median(ts),
                   "guard_host_us": guard_us if cap else None,
                   "tokens_per_s_range": [B * N / max(ts), B * N / min(ts)]}
            print(json.dumps(row), flush=True)
            rows.append(row)
        del model, cache, keep, steps
        torch.cuda.empty_cache()
    return rows


def fast_table(rate, lrows, frows):
    out = [f"device-to-device copy rate (1 GiB, read + write bytes): {rate * 1e-12:.2f} TB/s", ""]
    if lrows:
        out += ["| model | linear | N | K | M | waves, chunks/wave | few-row us med (min .. max) | tile us med (min .. max) | "
                "few-row GB/s | share of copy rate | tile GB/s | tile / few-row | |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in lrows:
            f, t = r["few_us"], r["tile_us"]
            out.append(f"| {r['model']} | {r['layer']} | {r['N']} | {r['K']} | {r['M']} | {r['waves_per'][0]}, {r['waves_per'][1]} | "
                       f"{f[0]:.1f} ({f[1]:.1f} .. {f[2]:.1f}) | {t[0]:.1f} ({t[1]:.1f} .. {t[2]:.1f}) | {r['few_GBps']:.0f} | "
                       f"{100 * r['few_share_of_copy_rate']:.1f} % | {r['tile_GBps']:.0f} | {t[0] / f[0]:.2f} | "
                       f"{'LOST' if r['lost'] else ''} |")
        lost = [r for r in lrows if r["lost"]]
        out += ["", "lost shapes (few-row median not below the tile median by more than the larger spread): "
                + (", ".join(f"{r['model']} {r['layer']} M={r['M']}" for r in lost) if lost else "none"), ""]
        out += ["FP8 weights: `linear_few_rows_fp8` against the bf16 few-row kernel on the same x "
                "(bytes: N K + 4 N against 2 N K)", "",
                "| model | linear | N | K | M | T, waves, chunks/wave | fp8 us med (min .. max) | bf16 few-row us med (min .. max) | "
                "fp8 weight GB/s | share of copy rate | bf16 / fp8 | bf16 / bf16 again | windows ms (fp8, bf16) | |",
                "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in lrows:
            f, t, pl, wm = r["fp8_us"], r["few_us"], r["fp8_plan"], r["fp8_window_ms"]
            out.append(f"| {r['model']} | {r['layer']} | {r['N']} | {r['K']} | {r['M']} | {pl[0]}, {pl[1]}, {pl[2]} | "
                       f"{f[0]:.1f} ({f[1]:.1f} .. {f[2]:.1f}) | {t[0]:.1f} ({t[1]:.1f} .. {t[2]:.1f}) | {r['fp8_GBps']:.0f} | "
                       f"{100 * r['fp8_share_of_copy_rate']:.1f} % | {r['few_over_fp8']:.2f} | {r['few_over_few2']:.2f} | "
                       f"{wm[0]:.0f}, {wm[1]:.0f} | {'LOST' if r['fp8_lost'] else ''} |")
        lost = [r for r in lrows if r["fp8_lost"]]
        out += ["", "FP8 lost shapes (fp8 median not below the bf16 few-row median by more than the larger spread): "
                + (", ".join(f"{r['model']} {r['layer']} M={r['M']}" for r in lost) if lost else "none"), ""]
    if frows:
        out += ["| model | B | arm | decode step us med (min .. max) | generate() tokens/s med (min .. max) | step vs eager tile | "
                "weight guard, host us per step |", "|---|---|---|---|---|---|---|"]
        base = {(r["model"], r["B"]): r["step_us"][0] for r in frows if r["arm"] == "eager tile"}
        for r in frows:
            s, g = r["step_us"], r["tokens_per_s_range"]
            out.append(f"| {r['model']} | {r['B']} | {r['arm']} | {s[0]:.0f} ({s[1]:.0f} .. {s[2]:.0f}) | "
                       f"{r['tokens_per_s']:.0f} ({g[0]:.0f} .. {g[1]:.0f}) | {base[(r['model'], r['B'])] / s[0]:.2f} x | "
                       f"{'' if r['guard_host_us'] is None else '%.1f' % r['guard_host_us']} |")
    return "\n".join(out)


def kv_kernel_rows(args, rate):
    """the bf16 and the FP8-cache decode kernels alternating on the same cached values"""
    from ray_torch_distributed_checkpoint_amd.ops import KVCache

    ext, rows = gpu_ext(), []
    for name, B, L, H, Hkv, Dh, rope in SHAPES:
        if args.only and name != args.only:
            continue
        Tmax = L + 64
        qkv_new = (torch.randn(B, (H + 2 * Hkv) * Dh, device=DEV) * 0.5).bfloat16()
        cache = (torch.randn(B, Tmax, 2 * Hkv * Dh, device=DEV) * 0.5).bfloat16()
        kvc = KVCache(1, B, Tmax, Hkv, Dh, DEV, kv_dtype="fp8")
        filler = torch.zeros((B, Tmax, (H + 2 * Hkv) * Dh), dtype=torch.bfloat16, device=DEV)
        filler[:, :, H * Dh:] = cache
        kvc.fill(0, filler, H, Tmax)
        del filler
        cq, cs = kvc.layers[0], kvc.scales[0]
        pos = torch.full((B,), L, dtype=torch.int32, device=DEV)
        ns = decode_splits(B, Hkv, Tmax, torch.device(DEV))
        part = torch.empty(B * H * ns * (Dh + 2), dtype=torch.float32, device=DEV)
        out = torch.empty((B, H * Dh), dtype=torch.bfloat16, device=DEV)
        cos, sin = rope_tables(Tmax, Dh, 500000.0, DEV) if rope else (None, None)
        scale = Dh ** -0.5
        r = ab({"bf16": lambda: ext.decode_attn(qkv_new, cache, pos, cos, sin, out, part, H, Hkv, 0, ns, scale),
                "fp8": lambda: ext.decode_attn(qkv_new, cq, pos, cos, sin, out, part, H, Hkv, 0, ns, scale, cache_scale=cs)},
               args.rounds, args.window_ms)
        (bm, bmin, _, bmax), (fm, fmin, _, fmax) = r["bf16"], r["fp8"]
        bb, fb = B * L * 2 * Hkv * Dh * 2, B * L * 2 * Hkv * (Dh + 4)
        row = {"bench": "decode_attn_fp8kv", "shape": name, "B": B, "cached": L, "H": H, "Hkv": Hkv, "Dh": Dh, "nsplit": ns,
               "bf16_us": [bm * 1e6, bmin * 1e6, bmax * 1e6], "fp8_us": [fm * 1e6, fmin * 1e6, fmax * 1e6],
               "bf16_bytes": bb, "fp8_bytes": fb, "bf16_share": bb / bm / rate, "fp8_share": fb / fm / rate,
               "bf16_over_fp8": bm / fm, "lost": not fm < bm - max(bmax - bmin, fmax - fmin)}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del cache, kvc, cq, cs
        torch.cuda.empty_cache()
    return rows


# arm, kv_cache, few_row, captured, weights
KV_ARMS = (("bf16 cache", "bf16", False, False, "bf16"), ("fp8 cache", "fp8", False, False, "bf16"),
           ("bf16 cache, captured few-row fp8 weights", "bf16", True, True, "fp8"),
           ("fp8 cache, captured few-row fp8 weights", "fp8", True, True, "fp8"))


def kv_step_rows(args):
    from ray_torch_distributed_checkpoint_amd.generate import build_model
    from ray_torch_distributed_checkpoint_amd.models.generation import CapturedDecode, new_cache

    rows = []
    for name, B, P, N in (("gpt2-small", 1, 64, 192), ("gpt2-small", 8, 64, 192), ("llama3-1b", 1, 64, 192),
                          ("llama3-1b", 8, 64, 192)):
        torch.manual_seed(0)
        model = build_model(name, DEV).eval()
        idx = torch.randint(0, model.cfg.vocab_size, (B, P), device=DEV)
        tok = idx[:, 0].contiguous()
        steps, keep = {}, []
        for arm, kvd, few, cap, wts in KV_ARMS:
            cache = new_cache(model, B, P + N, DEV, kv_cache=kvd)
            model.prefill(idx, cache, few_row=few, weights=wts)
            cache.pos.fill_(P + N // 2)
            cache.length = P + N // 2
            sess = CapturedDecode(model, cache, few_row=few, weights=wts) if cap else None
            keep.append((cache, sess))

            def step(cache=cache, sess=sess, few=few, wts=wts):
                if sess is not None:
                    sess.step(tok)
                else:
                    model.decode_step(tok, cache, few_row=few, weights=wts)
                cache.advance(-1)
            steps[arm] = step
        r = ab(steps, args.rounds, args.window_ms)
        for arm, kvd, few, cap, wts in KV_ARMS:
            kw = dict(few_row=few, captured=cap, weights=wts, kv_cache=kvd)
            model.generate(idx, 8, **kw)       # warm-up
            torch.cuda.synchronize()
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                model.generate(idx, N, **kw)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            med, mn, _, mx = r[arm]
            row = {"bench": "decode_fp8kv_step", "model": name, "B": B, "prompt": P, "new_tokens": N, "arm": arm,
                   "step_us": [med * 1e6, mn * 1e6, mx * 1e6], "tokens_per_s": B * N / median(ts),
                   "tokens_per_s_range": [B * N / max(ts), B * N / min(ts)]}
            print(json.dumps(row), flush=True)
            rows.append(row)
        del model, keep, steps
        torch.cuda.empty_cache()
    return rows


def kv_table(rate, krows, srows):
    out = [f"device-to-device copy rate (1 GiB, read + write bytes): {rate * 1e-12:.2f} TB/s", ""]
    if krows:
        out += ["| shape | B | cached keys | nsplit | bf16 kernel us med (min .. max) | fp8 kernel us med (min .. max) | "
                "bf16 share of copy rate | fp8 share of copy rate | bf16 / fp8 | |", "|---|---|---|---|---|---|---|---|---|---|"]
        for r in krows:
            b, f = r["bf16_us"], r["fp8_us"]
            out.append(f"| {r['shape']} H{r['H']} Hkv{r['Hkv']} Dh{r['Dh']} | {r['B']} | {r['cached']} | {r['nsplit']} | "
                       f"{b[0]:.1f} ({b[1]:.1f} .. {b[2]:.1f}) | {f[0]:.1f} ({f[1]:.1f} .. {f[2]:.1f}) | "
                       f"{100 * r['bf16_share']:.1f} % | {100 * r['fp8_share']:.1f} % | {r['bf16_over_fp8']:.2f} | "
                       f"{'LOST' if r['lost'] else ''} |")
        out.append("")
    if srows:
        out += ["| model | B | arm | decode step us med (min .. max) | generate() tokens/s med (min .. max) | "
                "step vs the bf16 cache | |", "|---|---|---|---|---|---|---|"]
        by = {(r["model"], r["B"], r["arm"]): r["step_us"] for r in srows}
        for r in srows:
            s, g = r["step_us"], r["tokens_per_s_range"]
            base = by[(r["model"], r["B"], r["arm"].replace("fp8 cache", "bf16 cache"))]
            lost = r["arm"].startswith("fp8") and not s[0] < base[0] - max(s[2] - s[1], base[2] - base[1])
            out.append(f"| {r['model']} | {r['B']} | {r['arm']} | {s[0]:.0f} ({s[1]:.0f} .. {s[2]:.0f}) | "
                       f"{r['tokens_per_s']:.0f} ({g[0]:.0f} .. {g[1]:.0f}) | {base[0] / s[0]:.2f} x | {'LOST' if lost else ''} |")
    return "\n".join(out)


def table(rate, krows, grows):
    out = [f"device-to-device copy rate (1 GiB, read + write bytes): {rate * 1e-12:.2f} TB/s", ""]
    if krows:
        out += ["| shape | B | cached keys | nsplit | decode kernel us (med / min) | SDPA us (med / min) | K+V GB/s | "
                "share of copy rate | SDPA / kernel |", "|---|---|---|---|---|---|---|---|---|"]
        for r in krows:
            out.append(f"| {r['shape']} H{r['H']} Hkv{r['Hkv']} Dh{r['Dh']} | {r['B']} | {r['cached']} | {r['nsplit']} | "
                       f"{r['native_us_med']:.1f} / {r['native_us_min']:.1f} | {r['sdpa_us_med']:.1f} / "
                       f"{r['sdpa_us_min']:.1f} | {r['native_GBps']:.0f} | {100 * r['share_of_copy_rate']:.1f} % | "
                       f"{r['sdpa_us_med'] / r['native_us_med']:.2f} |")
        out.append("")
    if grows:
        out += ["| model | B | prompt + new | tokens/s | decode step us | attention us | attention share |",
                "|---|---|---|---|---|---|---|"]
        for r in grows:
            out.append(f"| {r['model']} | {r['B']} | {r['prompt']} + {r['new_tokens']} | {r['tokens_per_s']:.0f} | "
                       f"{r['decode_step_us']:.0f} | {r['attention_us']:.0f} | {100 * r['attention_share']:.1f} % |")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-generate", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--fast", action="store_true", help="also the few-row / captured tables")
    ap.add_argument("--fast-only", action="store_true", help="only the few-row / captured tables")
    ap.add_argument("--fast-part", default="both", choices=("both", "linear", "step"))
    ap.add_argument("--fast-out", default=None)
    ap.add_argument("--kv-cache", default=None, choices=("fp8",), help="only the FP8 KV-cache tables")
    ap.add_argument("--kv-part", default="both", choices=("both", "kernel", "step"))
    ap.add_argument("--kv-out", default=None)
    args = ap.parse_args()
    rate = copy_rate(args.rounds, args.window_ms)
    print(json.dumps({"bench": "copy_rate", "bytes_per_s": rate}), flush=True)
    if args.kv_cache:
        krows = kv_kernel_rows(args, rate) if args.kv_part in ("both", "kernel") else []
        srows = kv_step_rows(args) if args.kv_part in ("both", "step") else []
        text = kv_table(rate, krows, srows)
        print(text)
        if args.kv_out:
            with open(args.kv_out, "w") as f:
                f.write(text + "\n")
        return
    if not args.fast_only:
        krows = kernel_rows(args, rate)
        grows = [] if args.no_generate else generate_rows(args)
        text = table(rate, krows, grows)
        print(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
    if args.fast or args.fast_only:
        lrows = linear_rows(args, rate) if args.fast_part in ("both", "linear") else []
        frows = fast_rows(args) if args.fast_part in ("both", "step") else []
        text = fast_table(rate, lrows, frows)
        print(text)
        if args.fast_out:
            with open(args.fast_out, "w") as f:
                f.write(text + "\n")


if __name__ == "__main__":
    main()
