"""Yardstick of the decode attention kernel (csrc/kernels/attn_decode.hip), in the manner of the
attention section of tests/ulp.py, whose helpers it reuses unchanged.

`decode_ref` in float64 is the reference: for row b the keys max(0, pos - window + 1) .. pos, key
pos being the new token itself, softmax(scale q.k) and o = sum p v, on inputs that are exact bf16
values (with RoPE: the rotated, bf16-rounded new row, which the kernel reproduces bit for bit and
the GPU test checks separately).  It returns the per-element allowance of `out`.  The same
function in float32 with the kernel's one bf16 rounding in place is the twin.
"""
from __future__ import annotations

import math

import torch

from tests import ulp as U

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
DECODE_MUTANTS = ("own_key_dropped", "window_off_by_one")

TMAX = 320
HEADS = ((1, 1, 64), (4, 2, 128), (8, 1, 64), (8, 2, 128), (12, 12, 64))      # (H, Hkv, Dh)
POS_SETS = ((0, 319, 64), (1, 62, 128), (63, 65, 127))                        # ragged within one launch
WINDOWS = (1, 5, 64, 100, None)
SPLITS = (1, 2, 5)
GENS = ("randn", "peaky")


def decode_inputs(gen, B, Tmax, H, Hkv, Dh, seed=0, dev="cpu"):
    """(qkv_new [B, W], cache [B, Tmax, 2 Hkv Dh]) in bf16 from the "randn" / "peaky" generators of
    tests/ulp.py: rows 0 .. Tmax - 1 of a packed qkv give the cache, row Tmax the new token."""
    x = U.attn_inputs(gen, B, Tmax + 1, H, Hkv, Dh, seed=seed)["qkv"]
    return x[:, Tmax].contiguous().to(dev), x[:, :Tmax, H * Dh:].contiguous().to(dev)


def decode_ref(dtype, qkv_new, cache, pos, H, Hkv, Dh, window=None, twin=False, mutant=""):
    """qkv_new [B, (H + 2 Hkv) Dh] (already rotated where RoPE applies), cache [B, Tmax, 2 Hkv Dh],
    pos int [B].  Returns {"out": [B, H Dh]} and, for the float64 reference, "allow_out".
    Rows of the cache outside lo .. pos - 1 are never looked at (they may hold anything).

    The roundings of attn_decode.hip, counted from its source, one allowance term each:
      * a score: 8 products per lane in 4 chained v_dot2_f32_bf16, log2(Dh / 8) DPP adds, one
        multiply by scale * log2(e), the subtraction of the running maximum and the v_exp_f32:
        fp32 only, F(Dh) = U._f32_terms(Dh) of sum_d |q_d k_d| scale, a relative error r_j of
        e_j; the same errors reach the normaliser l, weighted by p: r_j + sum_i p_i r_i per key
      * the weighted sum o and l: one fma per key and slot, a rescale per 4 keys, the merge of the
        key slots and of the splits, the division: fp32 only, F(T) of sum_j p_j |v_j|, T = Tmax
      * probabilities stay fp32: no bf16 term (unlike attn_flash.hip's e)
      * out stored as bf16: U._stored, half a bf16 spacing
    twin=True (float32): fp32 arithmetic with `out` rounded to bf16.  `mutant`: a deliberate error."""
    assert mutant == "" or mutant in DECODE_MUTANTS
    B, Tmax = cache.shape[0], cache.shape[1]
    G, dev = H // Hkv, cache.device
    p = torch.as_tensor(pos, device=dev).long()
    scale = U._f32(1.0 / math.sqrt(Dh))
    x = qkv_new.to(dtype).reshape(B, H + 2 * Hkv, Dh)
    q = x[:, :H].reshape(B, Hkv, G, Dh)
    kv = cache.to(dtype).clone()
    kv[torch.arange(B, device=dev), p] = x[:, H:].reshape(B, -1)
    t = torch.arange(Tmax, device=dev)
    if window is None:
        lo = torch.zeros_like(p)
    else:
        lo = (p - window + (0 if mutant == "window_off_by_one" else 1)).clamp_min(0)
    allowed = (t[None] <= p[:, None]) & (t[None] >= lo[:, None])
    if mutant == "own_key_dropped":
        allowed = allowed & (t[None] != p[:, None])
    zero = torch.zeros((), dtype=dtype, device=dev)
    am = allowed[:, :, None, None]
    K = torch.where(am, kv[..., : Hkv * Dh].reshape(B, Tmax, Hkv, Dh), zero)
    V = torch.where(am, kv[..., Hkv * Dh:].reshape(B, Tmax, Hkv, Dh), zero)
    keep = allowed[:, None, None, :]
    S = torch.einsum("bhgd,bthd->bhgt", q, K) * scale
    Sm = torch.where(keep, S, torch.full_like(S, -math.inf))
    e = torch.exp(Sm - Sm.amax(-1, keepdim=True))
    l = e.sum(-1, keepdim=True)
    O = U._rb(torch.einsum("bhgt,bthd->bhgd", e, V) / l, twin)
    res = {"out": O.reshape(B, H * Dh)}
    if dtype != F64 or twin or mutant:
        return res
    P = e / l
    Fd, Ft = U._f32_terms(Dh), U._f32_terms(Tmax)
    r = Fd * scale * torch.einsum("bhgd,bthd->bhgt", q.abs(), K.abs())
    r = torch.where(keep, r, zero)
    w = P * (r + (P * r).sum(-1, keepdim=True))
    A = torch.einsum("bhgt,bthd->bhgd", w + Ft * P, V.abs())
    res["allow_out"] = U._stored(O, A).reshape(B, H * Dh)
    return res


def split_ranges(Tmax, nsplit):
    """key ranges of rtdc_decode_attn: chunk = ceil(Tmax / nsplit) rounded up to a multiple of 64"""
    chunk = (-(-Tmax // nsplit) + 63) // 64 * 64
    return [(s * chunk, min(Tmax, (s + 1) * chunk)) for s in range(nsplit)]
