"""Causal flash attention microbenchmark (native fwd/bwd vs torch SDPA) on the GPT-2-small and
Llama-3-8B shapes; random operands, one process, interleaved repetitions.

    python benchmarks/attn_bench.py [--reps 20]
    python benchmarks/attn_bench.py --doc-len T T/8 100 [--only gpt2] [--rounds 7]
    python benchmarks/attn_bench.py --variants default 1,1,1 [--rounds 1]
    python benchmarks/attn_bench.py --window T/8 T/4 T/2 [--only llama8b_t8k] [--rounds 7]
    python benchmarks/attn_bench.py --dropout 0.1 [--only gpt2] [--rounds 7]

--doc-len L times the document-masked kernels (packed sequences: equal documents of length L, the
last one shorter when L does not divide T) next to the plain causal kernels on the same shape and
operands: kernel calls alone (the dK/dV head split chosen as the op chooses it), every timed
window at least --window-ms long, plain and masked alternating over --rounds rounds in one
process, median and minimum per arm and the plain arm's own run-to-run spread.  L = T (one document) is
the cost of the mask code with nothing to skip; L is an integer, `T` or `T/<n>`.

--window W times the sliding-window kernels the same way (same buffers, alternating rounds, every
window's length recorded), three arms per pass: the plain causal kernels, the window kernels, and
the document-mask kernels fed the band as clipped [B, T] arrays (what a window costs without
kernels of its own).  Next to the times it prints the share of key tiles the band visits, counted
from the kernels' loop bounds.  It adds a long shape (T = 8192) to the two of --doc-len.

--dropout P times the attention-dropout kernels (flash_fwd_drop / flash_bwd_drop, plain causal
mask) next to the plain kernels the same way: same buffers, alternating rounds, every timed
window's length recorded, median / minimum per arm, the plain arm's own spread and the ratio.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ray_torch_distributed_checkpoint_amd.ops._ext import gpu_ext  # noqa: E402
from ray_torch_distributed_checkpoint_amd.ops.attention import causal_attention  # noqa: E402

SHAPES = [("gpt2", 16, 1024, 12, 12, 64), ("llama8b", 1, 2048, 32, 8, 128), ("llama8b_b4", 4, 2048, 32, 8, 128)]


def timeit(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    fn()
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps * 1e-3


def _doc_len(spec: str, T: int) -> int:
    if spec.upper().startswith("T"):
        return T // int(spec[2:]) if len(spec) > 1 else T
    return int(spec)


def doc_mask_ab(args):
    """Plain vs document-masked kernels, forward and backward, per shape and document length."""
    from statistics import median

    from ray_torch_distributed_checkpoint_amd.ops import DocLayout
    from ray_torch_distributed_checkpoint_amd.ops.attention import _dkdv_head_split

    ext = gpu_ext()
    for name, B, T, H, Hkv, Dh in SHAPES[:2]:
        if args.only and name != args.only:
            continue
        W = (H + 2 * Hkv) * Dh
        scale = Dh ** -0.5
        q_ = (torch.randn(B, T, W, device="cuda") * 0.5).bfloat16()
        o_ = torch.empty((B, T, H * Dh), dtype=torch.bfloat16, device="cuda")
        lse = torch.empty((B * H, T), dtype=torch.float32, device="cuda")
        dy = torch.randn_like(o_)
        dqkv = torch.empty_like(q_)
        delta = torch.empty((B * H, T), dtype=torch.float32, device="cuda")
        # the GQA head split of dK/dV and its fp32 partials, chosen as causal_attention chooses them
        qs = _dkdv_head_split(B, T, H, Hkv, q_.device)
        part = torch.empty(qs * B * T * Hkv * 2 * Dh, dtype=torch.float32, device="cuda") if qs > 1 else None
        for spec in args.doc_len:
            L = _doc_len(spec, T)
            if not 1 <= L <= T:
                raise SystemExit(f"--doc-len {spec}: need 1 <= L <= T = {T}")
            row = [L] * (T // L) + ([T % L] if T % L else [])
            d = DocLayout.from_lengths([row] * B, T, "cuda")
            arms = {
                "plain_fwd": lambda: ext.flash_fwd(q_, o_, lse, B, T, H, Hkv, Dh, scale),
                "doc_fwd": lambda: ext.flash_fwd_doc(q_, o_, lse, d.start, d.end, B, T, H, Hkv, Dh, scale),
                "plain_bwd": lambda: ext.flash_bwd(q_, o_, dy, lse, delta, dqkv, B, T, H, Hkv, Dh, scale, None, part,
                                                   qs),
                "doc_bwd": lambda: ext.flash_bwd_doc(q_, o_, dy, lse, delta, dqkv, d.start, d.end, B, T, H, Hkv, Dh,
                                                     scale, None, part, qs),
            }
            # repetitions per arm so that every timed window is at least --window-ms long (a few ms
            # measure the clock ramp and the scheduler as much as the kernel)
            # (calibrated on 200 warm calls, with a quarter to spare for a faster clock later on)
            reps = {k: max(args.reps, int(1.25 * args.window_ms * 1e-3 / timeit(fn, 200)) + 1) for k, fn in arms.items()}
            # an arm's forward runs right before its backward, which so reads the o / lse of its
            # own mask
            t = {k: [] for k in arms}
            for _ in range(args.rounds):
                for kind in ("plain", "doc"):
                    t[kind + "_fwd"].append(timeit(arms[kind + "_fwd"], reps[kind + "_fwd"]) * 1e6)
                    t[kind + "_bwd"].append(timeit(arms[kind + "_bwd"], reps[kind + "_bwd"]) * 1e6)
            res = {"shape": name, "B": B, "T": T, "H": H, "Hkv": Hkv, "Dh": Dh, "doc_len": L, "docs_per_row": len(row),
                   "dkdv_head_split": qs, "reps": reps, "window_ms": args.window_ms, "rounds": args.rounds}
            for k, v in t.items():
                res[k + "_us_median"], res[k + "_us_min"] = round(median(v), 2), round(min(v), 2)
            for ph in ("fwd", "bwd"):
                pm, dm = median(t["plain_" + ph]), median(t["doc_" + ph])
                res[f"plain_{ph}_spread_pct"] = round(100 * (max(t["plain_" + ph]) - min(t["plain_" + ph])) / pm, 2)
                res[f"doc_vs_plain_{ph}_pct"] = round(100 * (dm - pm) / pm, 2)
            print(json.dumps(res), flush=True)


WINDOW_SHAPES = SHAPES[:2] + [("llama8b_t8k", 1, 8192, 32, 8, 128)]


def _tile_counts(T, Dh, W):
    """Key (query) tiles of 64 the loops of one (batch, head) visit, plain causal and under a window
    W, from the loop bounds of attn_flash.hip at the default rows per wave: forward and dQ blocks of
    64 G rows run tiles lo[first row] / 64 .. (last row) / 64, dK/dV blocks of 64 G keys the query
    tiles (first key) / 64 .. (hi[last key] - 1) / 64."""
    two = T % 128 == 0
    g_fwd, g_dq, g_kv = (2 if Dh == 128 and two else 1), (2 if two else 1), (2 if Dh == 64 and two else 1)

    def rows(G):  # (plain, band) over the query-row blocks
        blk = 64 * G
        plain = sum((qb + 1) * G for qb in range(T // blk))
        return plain, sum((qb + 1) * G - max(qb * blk - W + 1, 0) // 64 for qb in range(T // blk))

    def keys(G):
        blk = 64 * G
        plain = sum(T // 64 - kb * G for kb in range(T // blk))
        return plain, sum((min(kb * blk + blk - 1 + W, T) - 1) // 64 - kb * G + 1 for kb in range(T // blk))

    f, dq, kv = rows(g_fwd), rows(g_dq), keys(g_kv)
    return {"fwd": f, "bwd": (dq[0] + kv[0], dq[1] + kv[1])}


def window_ab(args):
    """Plain vs sliding-window kernels vs the DOC kernels on clipped arrays, forward and backward,
    per shape and window."""
    from statistics import median

    from ray_torch_distributed_checkpoint_amd.ops.attention import _dkdv_head_split

    ext = gpu_ext()
    for name, B, T, H, Hkv, Dh in WINDOW_SHAPES:
        if args.only and name != args.only:
            continue
        Wd, scale = (H + 2 * Hkv) * Dh, Dh ** -0.5
        q_ = (torch.randn(B, T, Wd, device="cuda") * 0.5).bfloat16()
        o_ = torch.empty((B, T, H * Dh), dtype=torch.bfloat16, device="cuda")
        lse = torch.empty((B * H, T), dtype=torch.float32, device="cuda")
        dy = torch.randn_like(o_)
        dqkv = torch.empty_like(q_)
        delta = torch.empty((B * H, T), dtype=torch.float32, device="cuda")
        qs = _dkdv_head_split(B, T, H, Hkv, q_.device)
        part = torch.empty(qs * B * T * Hkv * 2 * Dh, dtype=torch.float32, device="cuda") if qs > 1 else None
        for spec in args.window:
            W = _doc_len(spec, T)
            if not 1 <= W <= T:
                raise SystemExit(f"--window {spec}: need 1 <= W <= T = {T}")
            t_ = torch.arange(T, device="cuda", dtype=torch.int32)[None, :].expand(B, T)
            cs, ce = (t_ - W + 1).clamp_min(0).contiguous(), (t_ + W).clamp_max(T).contiguous()
            arms = {
                "plain_fwd": lambda: ext.flash_fwd(q_, o_, lse, B, T, H, Hkv, Dh, scale),
                "win_fwd": lambda: ext.flash_fwd_win(q_, o_, lse, W, None, None, B, T, H, Hkv, Dh, scale),
                "clip_fwd": lambda: ext.flash_fwd_doc(q_, o_, lse, cs, ce, B, T, H, Hkv, Dh, scale),
                "plain_bwd": lambda: ext.flash_bwd(q_, o_, dy, lse, delta, dqkv, B, T, H, Hkv, Dh, scale, None, part,
                                                   qs),
                "win_bwd": lambda: ext.flash_bwd_win(q_, o_, dy, lse, delta, dqkv, W, None, None, B, T, H, Hkv, Dh,
                                                     scale, None, part, qs),
                "clip_bwd": lambda: ext.flash_bwd_doc(q_, o_, dy, lse, delta, dqkv, cs, ce, B, T, H, Hkv, Dh, scale,
                                                      None, part, qs),
            }
            # (as --doc-len: windows of at least --window-ms, calibrated on warm calls; an arm's
            # forward runs right before its backward, which so reads the o / lse of its own mask)
            reps = {k: max(args.reps, int(1.25 * args.window_ms * 1e-3 / timeit(fn, 100)) + 1) for k, fn in arms.items()}
            t = {k: [] for k in arms}
            for _ in range(args.rounds):
                for kind in ("plain", "win", "clip"):
                    t[kind + "_fwd"].append(timeit(arms[kind + "_fwd"], reps[kind + "_fwd"]) * 1e6)
                    t[kind + "_bwd"].append(timeit(arms[kind + "_bwd"], reps[kind + "_bwd"]) * 1e6)
            tiles = _tile_counts(T, Dh, W)
            res = {"shape": name, "B": B, "T": T, "H": H, "Hkv": Hkv, "Dh": Dh, "window": W, "dkdv_head_split": qs,
                   "reps": reps, "window_ms": args.window_ms, "rounds": args.rounds}
            for k, v in t.items():
                res[k + "_us_median"], res[k + "_us_min"] = round(median(v), 2), round(min(v), 2)
                res[k + "_timed_ms"] = [round(x * reps[k] * 1e-3, 1) for x in v]  # every timed window's length
            for ph in ("fwd", "bwd"):
                pm, wm, cm = (median(t[a + "_" + ph]) for a in ("plain", "win", "clip"))
                res[f"plain_{ph}_spread_pct"] = round(100 * (max(t["plain_" + ph]) - min(t["plain_" + ph])) / pm, 2)
                res[f"win_over_plain_{ph}_time"] = round(wm / pm, 3)
                res[f"band_over_triangle_{ph}_tiles"] = round(tiles[ph][1] / tiles[ph][0], 3)
                res[f"win_vs_clip_{ph}_pct"] = round(100 * (wm - cm) / cm, 2)
            print(json.dumps(res), flush=True)


def dropout_ab(args):
    """Plain vs attention-dropout kernels, forward and backward, per shape and probability."""
    from statistics import median

    from ray_torch_distributed_checkpoint_amd.ops.attention import _dkdv_head_split, attention_dropout_keep

    ext = gpu_ext()
    for name, B, T, H, Hkv, Dh in SHAPES[:2]:
        if args.only and name != args.only:
            continue
        Wd, scale = (H + 2 * Hkv) * Dh, Dh ** -0.5
        q_ = (torch.randn(B, T, Wd, device="cuda") * 0.5).bfloat16()
        o_ = torch.empty((B, T, H * Dh), dtype=torch.bfloat16, device="cuda")
        lse = torch.empty((B * H, T), dtype=torch.float32, device="cuda")
        dy = torch.randn_like(o_)
        dqkv = torch.empty_like(q_)
        delta = torch.empty((B * H, T), dtype=torch.float32, device="cuda")
        qs = _dkdv_head_split(B, T, H, Hkv, q_.device)
        part = torch.empty(qs * B * T * Hkv * 2 * Dh, dtype=torch.float32, device="cuda") if qs > 1 else None
        for p in args.dropout:
            thr, _ = attention_dropout_keep(p)
            seed, off = 0x5EED, 12345
            arms = {
                "plain_fwd": lambda: ext.flash_fwd(q_, o_, lse, B, T, H, Hkv, Dh, scale),
                "drop_fwd": lambda: ext.flash_fwd_drop(q_, o_, lse, 0, None, None, thr, seed, off, None, B, T, H, Hkv,
                                                       Dh, scale),
                "plain_bwd": lambda: ext.flash_bwd(q_, o_, dy, lse, delta, dqkv, B, T, H, Hkv, Dh, scale, None, part,
                                                   qs),
                "drop_bwd": lambda: ext.flash_bwd_drop(q_, o_, dy, lse, delta, dqkv, 0, None, None, thr, seed, off,
                                                       None, B, T, H, Hkv, Dh, scale, None, part, qs),
            }
            # (as --doc-len: windows of at least --window-ms, calibrated on warm calls; an arm's
            # forward runs right before its backward, which so reads the o / lse of its own mask)
            reps = {k: max(args.reps, int(1.25 * args.window_ms * 1e-3 / timeit(fn, 100)) + 1) for k, fn in arms.items()}
            t = {k: [] for k in arms}
            for _ in range(args.rounds):
                for kind in ("plain", "drop"):
                    t[kind + "_fwd"].append(timeit(arms[kind + "_fwd"], reps[kind + "_fwd"]) * 1e6)
                    t[kind + "_bwd"].append(timeit(arms[kind + "_bwd"], reps[kind + "_bwd"]) * 1e6)
            res = {"shape": name, "B": B, "T": T, "H": H, "Hkv": Hkv, "Dh": Dh, "dropout_p": p, "thr": thr,
                   "dkdv_head_split": qs, "reps": reps, "window_ms": args.window_ms, "rounds": args.rounds}
            for k, v in t.items():
                res[k + "_us_median"], res[k + "_us_min"] = round(median(v), 2), round(min(v), 2)
                res[k + "_timed_ms"] = [round(x * reps[k] * 1e-3, 1) for x in v]  # every timed window's length
            for ph in ("fwd", "bwd"):
                pm, dm = median(t["plain_" + ph]), median(t["drop_" + ph])
                res[f"plain_{ph}_spread_pct"] = round(100 * (max(t["plain_" + ph]) - min(t["plain_" + ph])) / pm, 2)
                res[f"drop_over_plain_{ph}_time"] = round(dm / pm, 3)
            print(json.dumps(res), flush=True)


def variants_ab(args):
    """The forward and the backward kernel calls, timed apart, at each rows-per-wave setting: one
    JSON line per (shape, setting) with the time of every round.  Two builds are compared by running
    this in alternating processes (RTDC_EXT_SO), one round each."""
    from ray_torch_distributed_checkpoint_amd.ops.attention import _dkdv_head_split

    ext = gpu_ext()
    knobs = ("RTDC_FA_FWD", "RTDC_FA_DQ", "RTDC_FA_DKDV")
    for name, B, T, H, Hkv, Dh in SHAPES[:2]:
        if args.only and name != args.only:
            continue
        W, scale = (H + 2 * Hkv) * Dh, Dh ** -0.5
        q_ = (torch.randn(B, T, W, device="cuda") * 0.5).bfloat16()
        o_ = torch.empty((B, T, H * Dh), dtype=torch.bfloat16, device="cuda")
        lse = torch.empty((B * H, T), dtype=torch.float32, device="cuda")
        dy = torch.randn_like(o_)
        dqkv = torch.empty_like(q_)
        delta = torch.empty_like(lse)
        qs = _dkdv_head_split(B, T, H, Hkv, q_.device)
        part = torch.empty(qs * B * T * Hkv * 2 * Dh, dtype=torch.float32, device="cuda") if qs > 1 else None
        arms = {"fwd": lambda: ext.flash_fwd(q_, o_, lse, B, T, H, Hkv, Dh, scale),
                "bwd": lambda: ext.flash_bwd(q_, o_, dy, lse, delta, dqkv, B, T, H, Hkv, Dh, scale, None, part, qs)}
        for spec in args.variants:
            for k, v in zip(knobs, spec.split(",") if spec != "default" else (None,) * 3):
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v
            arms["fwd"]()  # the backward reads this setting's o / lse
            # repetitions so that every timed window is at least --window-ms long (as --doc-len)
            reps = {k: max(args.reps, int(1.25 * args.window_ms * 1e-3 / timeit(fn, 200)) + 1) for k, fn in arms.items()}
            t = {k: [round(timeit(fn, reps[k]) * 1e6, 2) for _ in range(args.rounds)] for k, fn in arms.items()}
            print(json.dumps({"shape": name, "B": B, "T": T, "H": H, "Hkv": Hkv, "Dh": Dh, "variant": spec,
                              "dkdv_head_split": qs, "reps": reps, "window_ms": args.window_ms,
                              "fwd_us": t["fwd"], "bwd_us": t["bwd"]}), flush=True)
        for k in knobs:
            os.environ.pop(k, None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", nargs="+", default=None, metavar="F,Q,K",
                    help="time the forward and backward kernel calls at each RTDC_FA_FWD,RTDC_FA_DQ,RTDC_FA_DKDV "
                         "setting (`default` = all unset), --rounds windows of --window-ms each")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default=None)
    ap.add_argument("--doc-len", nargs="+", default=None, metavar="L",
                    help="time the document-masked kernels with equal documents of length L (an integer, T or "
                         "T/<n>; several allowed) next to the plain ones")
    ap.add_argument("--window", nargs="+", default=None, metavar="W",
                    help="time the sliding-window kernels with a window of W keys (an integer, T or T/<n>; several "
                         "allowed) next to the plain ones and to the document-mask kernels on clipped arrays")
    ap.add_argument("--dropout", nargs="+", type=float, default=None, metavar="P",
                    help="time the attention-dropout kernels at probability P (several allowed) next to the plain "
                         "ones")
    ap.add_argument("--rounds", type=int, default=7, help="--doc-len / --window: alternating plain / masked rounds")
    ap.add_argument("--window-ms", type=float, default=120.0,
                    help="--doc-len / --window: least length of every timed window (repetitions are scaled to it)")
    args = ap.parse_args()
    torch.manual_seed(0)
    from gemm_bench import warm_up_clocks

    warm_up_clocks()
    if args.doc_len:
        return doc_mask_ab(args)
    if args.window:
        return window_ab(args)
    if args.dropout:
        return dropout_ab(args)
    if args.variants:
        return variants_ab(args)
    for name, B, T, H, Hkv, Dh in SHAPES:
        if args.only and name != args.only:
            continue
        W = (H + 2 * Hkv) * Dh
        qkv = (torch.randn(B, T, W, device="cuda") * 0.5).bfloat16().requires_grad_(True)
        flops_f = 2 * 2 * B * H * T * T * Dh / 2  # causal
        y = causal_attention(qkv, H, Hkv)
        dy = torch.randn_like(y)
        t_f = min(timeit(lambda: causal_attention(qkv, H, Hkv), args.reps) for _ in range(3))

        def fb():
            out = causal_attention(qkv, H, Hkv)
            out.backward(dy)

        t_fb = min(timeit(fb, args.reps) for _ in range(3))
        # the kernels alone (what a training step pays; the autograd round trip above adds host
        # overhead the GPU can wait on in an isolated loop): flash_fwd, flash_bwd (dQ + dK/dV)
        ext = gpu_ext()
        scale = Dh ** -0.5
        q_ = qkv.detach()
        o_ = torch.empty((B, T, H * Dh), dtype=torch.bfloat16, device="cuda")
        lse = torch.empty((B * H, T), dtype=torch.float32, device="cuda")
        ext.flash_fwd(q_, o_, lse, B, T, H, Hkv, Dh, scale)
        dqkv = torch.empty_like(q_)
        delta = torch.empty((B * H, T), dtype=torch.float32, device="cuda")
        dyc = dy.contiguous()
        t_kf = min(timeit(lambda: ext.flash_fwd(q_, o_, lse, B, T, H, Hkv, Dh, scale), args.reps) for _ in range(3))
        t_kb = min(timeit(lambda: ext.flash_bwd(q_, o_, dyc, lse, delta, dqkv, B, T, H, Hkv, Dh, scale, None), args.reps)
                   for _ in range(3))
        q = qkv.detach()[..., : H * Dh].view(B, T, H, Dh).transpose(1, 2).contiguous().requires_grad_(True)
        k = qkv.detach()[..., H * Dh:(H + Hkv) * Dh].view(B, T, Hkv, Dh).transpose(1, 2)
        v = qkv.detach()[..., (H + Hkv) * Dh:].view(B, T, Hkv, Dh).transpose(1, 2)
        k = k.repeat_interleave(H // Hkv, 1).contiguous().requires_grad_(True)
        v = v.repeat_interleave(H // Hkv, 1).contiguous().requires_grad_(True)
        t_sf = min(timeit(lambda: F.scaled_dot_product_attention(q, k, v, is_causal=True), args.reps) for _ in range(3))
        do = torch.randn(B, H, T, Dh, device="cuda", dtype=torch.bfloat16)

        def sfb():
            F.scaled_dot_product_attention(q, k, v, is_causal=True).backward(do)

        t_sfb = min(timeit(sfb, args.reps) for _ in range(3))
        print(json.dumps({"shape": name, "B": B, "T": T, "H": H, "Hkv": Hkv, "Dh": Dh,
                          "fwd_us": round(t_f * 1e6, 1), "fwd_TF": round(flops_f / t_f / 1e12, 1),
                          "bwd_us": round((t_fb - t_f) * 1e6, 1),
                          "bwd_TF": round(2.5 * flops_f / (t_fb - t_f) / 1e12, 1),
                          "kernel_fwd_us": round(t_kf * 1e6, 1), "kernel_fwd_TF": round(flops_f / t_kf / 1e12, 1),
                          "kernel_bwd_us": round(t_kb * 1e6, 1),
                          "kernel_bwd_TF": round(2.5 * flops_f / t_kb / 1e12, 1),
                          "sdpa_fwd_us": round(t_sf * 1e6, 1), "sdpa_fwd_TF": round(flops_f / t_sf / 1e12, 1),
                          "sdpa_bwd_us": round((t_sfb - t_sf) * 1e6, 1)}), flush=True)


if __name__ == "__main__":
    main()
