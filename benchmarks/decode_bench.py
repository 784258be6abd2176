"""Decode attention (split-KV kernel, csrc/kernels/attn_decode.hip) and generate() benchmark.

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
eager / captured x tile / few-row (eager-tile is the path of the tables above).
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
    from ray_torch_distributed_checkpoint_amd.ops import gemm as G

    rows = []
    for model, layer, N, K in linear_shapes():
        w = (torch.randn(N, K, device=DEV) * K ** -0.5).bfloat16()
        for M in (1, 8, 16):
            Mp = -(-M // 8) * 8
            xp = torch.zeros(Mp, K, dtype=torch.bfloat16, device=DEV)
            xp[:M] = torch.randn(M, K, device=DEV).bfloat16()
            x = xp[:M]
            # both arms allocate their output per call, as the decode step does
            r = ab({"few": lambda: G.linear_few_rows(x, w), "tile": lambda: G.linear_fwd(xp, w)},
                   args.rounds, args.window_ms)
            (fm, fmin, _, fmax), (tm, tmin, _, tmax) = r["few"], r["tile"]
            spread = max(fmax - fmin, tmax - tmin)
            row = {"bench": "few_rows_linear", "model": model, "layer": layer, "N": N, "K": K, "M": M,
                   "waves_per": list(gpu_ext().few_rows_plan(N, K)),
                   "few_us": [fm * 1e6, fmin * 1e6, fmax * 1e6], "tile_us": [tm * 1e6, tmin * 1e6, tmax * 1e6],
                   "weight_bytes": 2 * N * K, "few_GBps": 2 * N * K / fm * 1e-9, "tile_GBps": 2 * N * K / tm * 1e-9,
                   "few_share_of_copy_rate": 2 * N * K / fm / rate, "tile_share_of_copy_rate": 2 * N * K / tm / rate,
                   "lost": not fm < tm - spread}
            print(json.dumps(row), flush=True)
            rows.append(row)
        del w
        torch.cuda.empty_cache()
    return rows


ARMS = (("eager tile", False, False), ("eager few-row", True, False), ("captured tile", False, True),
        ("captured few-row", True, True))


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
        for arm, few, cap in ARMS:
            if cap:
                sess = CapturedDecode(model, cache, few_row=few)
                keep.append(sess)

                def step(sess=sess):
                    sess.step(tok)
                    cache.advance(-1)
            else:
                def step(few=few):
                    model.decode_step(tok, cache, few_row=few)
                    cache.advance(-1)
            steps[arm] = step
        r = ab(steps, args.rounds, args.window_ms)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(2000):
            keep[0]._check_weights()
        guard_us = (time.perf_counter() - t0) / 2000 * 1e6    # host cost of the per-step weight guard
        for arm, few, cap in ARMS:
            model.generate(idx, 8, few_row=few, captured=cap)       # warm-up
            torch.cuda.synchronize()
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                model.generate(idx, N, few_row=few, captured=cap)
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
    args = ap.parse_args()
    rate = copy_rate(args.rounds, args.window_ms)
    print(json.dumps({"bench": "copy_rate", "bytes_per_s": rate}), flush=True)
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
