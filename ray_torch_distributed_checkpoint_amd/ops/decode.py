"""KV cache and decode attention: one new token per batch row against the cached keys.

The cache of a layer is [B, Tmax, 2 * Hkv * Dh]: the k|v tail of the packed qkv rows (K heads,
then V heads), so a prefill fills it with one strided copy of the qkv activations.  `pos`
(int32 [B], on the device) is the index of the next token of each row; rows may differ.

`decode_attention` is the attention part of one decode step: on the GPU one launch of the
split-KV kernel (csrc/kernels/attn_decode.hip) rotates the new q and k heads (RoPE tables
given), stores the new k|v row at `pos` and attends to the keys max(0, pos - window + 1) .. pos;
on the CPU the same math in torch.  It does not advance `pos`: every layer of a step shares it
and the model calls `KVCache.advance()` once the step is done.
"""
from __future__ import annotations

import math
import os

import torch

from ._ext import gpu_ext, require_dtype


class KVCache:
    """One [B, Tmax, 2 * Hkv * Dh] cache tensor per layer, `pos` (int32 [B] on the device) and
    `length`, the host's copy of the largest position (no device read is needed to know it)."""

    def __init__(self, n_layers: int, B: int, Tmax: int, Hkv: int, Dh: int, device=None, dtype=None):
        device = torch.device(device if device is not None else "cpu")
        if dtype is None:
            dtype = torch.bfloat16 if device.type == "cuda" else torch.float32
        if min(n_layers, B, Tmax, Hkv, Dh) < 1:
            raise ValueError("KVCache: every dimension must be >= 1")
        self.B, self.Tmax, self.Hkv, self.Dh = B, Tmax, Hkv, Dh
        self.layers = [torch.zeros((B, Tmax, 2 * Hkv * Dh), dtype=dtype, device=device) for _ in range(n_layers)]
        self.pos = torch.zeros(B, dtype=torch.int32, device=device)
        self.length = 0
        self._part = None

    @property
    def device(self):
        return self.pos.device

    def advance(self, n: int = 1) -> None:
        self.pos += n
        self.length += n

    def reset(self) -> None:
        self.pos.zero_()
        self.length = 0

    def fill(self, layer: int, qkv: torch.Tensor, n_head: int, rows: int) -> None:
        """Prefill: copy the k|v tail of rows [0, rows) of qkv [B, T, (H + 2 Hkv) Dh] into the
        layer's cache (one strided copy per batch row on the GPU)."""
        B, T, W = qkv.shape
        kvw = 2 * self.Hkv * self.Dh
        if B != self.B or W != n_head * self.Dh + kvw or rows > min(T, self.Tmax):
            raise ValueError(f"KVCache.fill: qkv {tuple(qkv.shape)} / rows {rows} do not fit the cache "
                             f"[{self.B}, {self.Tmax}, {kvw}]")
        dst = self.layers[layer]
        if qkv.is_cuda and qkv.is_contiguous() and qkv.dtype == dst.dtype:
            es = qkv.element_size()
            ext = gpu_ext()
            for b in range(B):
                ext.copy2d(dst[b], qkv[b].reshape(-1)[n_head * self.Dh:], rows, kvw * es, kvw * es, W * es)
        else:
            dst[:, :rows] = qkv[:, :rows, n_head * self.Dh:].to(dst.dtype)


def decode_splits(B: int, Hkv: int, Tmax: int, device) -> int:
    """Key splits of one decode launch.  A block serves one (split, kv-head, row) and streams
    its keys once, so with few (kv-head, row) pairs (Llama-3-8B at B = 1: 8) the split over keys
    carries the parallelism: enough splits for 4 blocks per CU, none shorter than 64 keys.  It
    depends on (B, Hkv, Tmax, CU count) only, never on pos, so it is constant over a generation.
    RTDC_DECODE_SPLITS forces a value (clamped to 1 .. Tmax / 64)."""
    most = max(1, Tmax // 64)
    forced = int(os.environ.get("RTDC_DECODE_SPLITS", "0"))
    if forced > 0:
        return min(forced, most)
    from .gemm import _num_cus

    want = -(-4 * _num_cus(device) // (B * Hkv))
    return max(1, min(want, most))


def _decode_ref(qkv_new, kv, pos, H, Hkv, Dh, rope, window, scale):
    B = qkv_new.shape[0]
    G = H // Hkv
    Tmax = kv.shape[1]
    x = qkv_new.reshape(B, H + 2 * Hkv, Dh)
    p = pos.long()
    if rope is not None:
        cos, sin = rope
        c, s = cos[p][:, None, :], sin[p][:, None, :]
        rot = x[:, : H + Hkv].float()
        x1, x2 = rot[..., : Dh // 2], rot[..., Dh // 2:]
        rot = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).to(x.dtype)
        x = torch.cat([rot, x[:, H + Hkv:]], dim=1)
    kv[torch.arange(B, device=kv.device), p] = x[:, H:].reshape(B, -1).to(kv.dtype)
    t = torch.arange(Tmax, device=kv.device)
    lo = (p - window + 1).clamp_min(0) if window else torch.zeros_like(p)
    allowed = (t[None, :] <= p[:, None]) & (t[None, :] >= lo[:, None])            # [B, Tmax]
    keys = kv[..., : Hkv * Dh].reshape(B, Tmax, Hkv, Dh).float()
    vals = kv[..., Hkv * Dh:].reshape(B, Tmax, Hkv, Dh).float()
    zero = torch.zeros((), dtype=keys.dtype, device=kv.device)
    keys = torch.where(allowed[:, :, None, None], keys, zero)    # rows outside the range are never looked at
    vals = torch.where(allowed[:, :, None, None], vals, zero)
    q = x[:, :H].reshape(B, Hkv, G, Dh).float()
    s = torch.einsum("bhgd,bthd->bhgt", q, keys) * scale
    s = s.masked_fill(~allowed[:, None, None, :], -math.inf)
    o = torch.einsum("bhgt,bthd->bhgd", torch.softmax(s, dim=-1), vals)
    return o.reshape(B, H * Dh).to(qkv_new.dtype)


def decode_attention(qkv_new: torch.Tensor, cache: KVCache, layer: int, n_head: int, n_kv_head: int | None = None,
                     rope=None, window: int | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """qkv_new [B, (H + 2 Hkv) Dh], the new token's packed row before RoPE -> [B, H Dh].
    rope: (cos, sin) of ops.llama_ops.rope_tables with at least Tmax rows (None: no rotation).
    window (None = off): the keys max(0, pos - window + 1) .. pos.  out: an optional [B, H Dh]
    destination.  Stores the new k|v row (k rotated) at cache.layers[layer][b, pos[b]]."""
    Hkv = n_kv_head or n_head
    if qkv_new.dim() != 2 or qkv_new.shape[1] % (n_head + 2 * Hkv) or n_head % Hkv:
        raise ValueError(f"decode_attention: qkv_new must be [B, (H + 2 Hkv) Dh], got {tuple(qkv_new.shape)} "
                         f"with H={n_head}, Hkv={Hkv}")
    B, W = qkv_new.shape
    Dh = W // (n_head + 2 * Hkv)
    kv = cache.layers[layer]
    if (B, Hkv, Dh) != (cache.B, cache.Hkv, cache.Dh):
        raise ValueError(f"decode_attention: qkv_new (B={B}, Hkv={Hkv}, Dh={Dh}) does not match the cache "
                         f"(B={cache.B}, Hkv={cache.Hkv}, Dh={cache.Dh})")
    if qkv_new.device != kv.device or qkv_new.dtype != kv.dtype:
        raise ValueError(f"decode_attention: qkv_new is {qkv_new.dtype} on {qkv_new.device}, the cache "
                         f"{kv.dtype} on {kv.device}")
    if cache.length >= cache.Tmax:
        raise ValueError(f"decode_attention: the cache is full ({cache.length} of {cache.Tmax} positions)")
    if window is not None:
        window = int(window)
        if window < 1:
            raise ValueError(f"decode_attention: window must be >= 1 (None = off), got {window}")
    if rope is not None:
        cos, sin = rope
        if cos.device != kv.device or cos.shape != sin.shape or cos.shape[0] < cache.Tmax or cos.shape[1] != Dh // 2:
            raise ValueError(f"decode_attention: rope tables {tuple(cos.shape)} on {cos.device} do not cover "
                             f"[{cache.Tmax}, {Dh // 2}] on {kv.device}")
    if out is not None and (out.shape != (B, n_head * Dh) or out.dtype != qkv_new.dtype or out.device != kv.device
                            or not out.is_contiguous()):
        raise ValueError("decode_attention: out must be a contiguous [B, H Dh] tensor like qkv_new")
    scale = 1.0 / math.sqrt(Dh)
    if not qkv_new.is_cuda:
        y = _decode_ref(qkv_new, kv, cache.pos, n_head, Hkv, Dh, rope, window, scale)
        if out is not None:
            out.copy_(y)
            return out
        return y
    require_dtype(qkv_new, "decode_attention")
    if Dh not in (64, 128):
        raise ValueError(f"decode_attention: the decode kernel takes Dh in (64, 128), got {Dh}")
    if cache.Tmax % 64 or n_head // Hkv > 8:
        raise ValueError(f"decode_attention: the decode kernel needs Tmax % 64 == 0 and H / Hkv <= 8, got "
                         f"Tmax={cache.Tmax}, H={n_head}, Hkv={Hkv}")
    if not qkv_new.is_contiguous() or not kv.is_contiguous():
        raise ValueError("decode_attention: contiguous qkv_new and cache expected")
    nsplit = decode_splits(B, Hkv, cache.Tmax, kv.device)
    need = B * n_head * nsplit * (Dh + 2)
    part = cache._part
    if part is None or part.numel() < need or part.device != kv.device:
        part = cache._part = torch.empty(need, dtype=torch.float32, device=kv.device)
    if out is None:
        out = torch.empty((B, n_head * Dh), dtype=torch.bfloat16, device=kv.device)
    cos, sin = rope if rope is not None else (None, None)
    gpu_ext().decode_attn(qkv_new, kv, cache.pos, cos, sin, out, part, n_head, Hkv, window or 0, nsplit, scale)
    return out
