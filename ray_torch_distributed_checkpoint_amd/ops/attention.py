"""Causal multi-head self-attention composed from the native batched MFMA GEMM + row softmax.

Inputs are the packed QKV activations [B, T, 3C] written by the c_attn GEMM, read in place
through batch strides (no split/transpose copies): per (b, h)

    S  = (Q K^T) / sqrt(Dh)        GEMM, tiles above the diagonal skipped       (causal=1)
    P  = softmax_causal(S)         wave64 row kernel, writes exact zeros above the diagonal
    O  = P V                       GEMM, k-range limited to the causal prefix    (causal=2)

backward:  dP = dO V^T (causal=1) -> dS = P*(dP - rowsum(P*dP)) -> dQ = dS K / sqrt(Dh)
(causal=2), dK = dS^T Q / sqrt(Dh) and dV = P^T dO (causal=3: k >= the key tile).

The probability matrix is materialised (B*H*T*T bf16 per layer) - affordable in 288 GB of
HBM and it keeps every product on the well-tested GEMM; a flash-style fused kernel replaces
this path when T grows.  GQA (Llama) reuses it with per-head K/V strides.
"""
from __future__ import annotations

import math
import os

import torch
import torch.nn.functional as F

from . import gemm as G
from ._ext import gpu_ext, require_dtype
from .random import PhiloxStream, default_stream, philox4x32


def _qkv_layout(B, T, H, Hkv, Dh):
    C = H * Dh
    row = C + 2 * Hkv * Dh  # qkv row width
    return C, row


class _CausalAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, B, T, H, Hkv, Dh):
        C, row = _qkv_layout(B, T, H, Hkv, Dh)
        qkv = qkv.contiguous()
        dev = qkv.device
        alpha = 1.0 / math.sqrt(Dh)
        grp = H // Hkv
        P = torch.empty((B, H, T, T), dtype=torch.bfloat16, device=dev)
        q = qkv
        k = qkv[..., C:]
        v = qkv[..., C + Hkv * Dh:]
        # GQA: head h reads kv head h // grp -> inner stride over heads is Dh/grp per q-head...
        # expressed with batch_inner = H and explicit strides: kv offset = (h // grp) * Dh.
        if grp == 1:
            kstride = Dh
        else:
            kstride = None
        out = torch.empty((B, T, C), dtype=torch.bfloat16, device=dev)
        if kstride is not None:
            G.gemm_bf16(q, k, P, T, T, Dh, row, row, T, True, True, alpha=alpha, causal=G.CAUSAL_SKIP_UPPER,
                        batch=B * H, batch_inner=H, strides=(T * row, Dh, T * row, Dh, H * T * T, T * T))
            gpu_ext().softmax_fwd(P, P, None, B * H * T, T, True)
            G.gemm_bf16(P, v, out, T, Dh, T, T, row, C, True, False, causal=G.CAUSAL_K_UPTO_M,
                        batch=B * H, batch_inner=H, strides=(H * T * T, T * T, T * row, Dh, T * C, Dh))
        else:
            for g in range(grp):  # q heads h = j*grp + g share kv head j
                G.gemm_bf16(q[..., g * Dh:], k, P[:, g::grp], T, T, Dh, row, row, T, True, True, alpha=alpha,
                            causal=G.CAUSAL_SKIP_UPPER, batch=B * Hkv, batch_inner=Hkv,
                            strides=(T * row, grp * Dh, T * row, Dh, H * T * T, grp * T * T))
            gpu_ext().softmax_fwd(P, P, None, B * H * T, T, True)
            for g in range(grp):
                G.gemm_bf16(P[:, g::grp], v, out[..., g * Dh:], T, Dh, T, T, row, C, True, False,
                            causal=G.CAUSAL_K_UPTO_M, batch=B * Hkv, batch_inner=Hkv,
                            strides=(H * T * T, grp * T * T, T * row, Dh, T * C, grp * Dh))
        ctx.save_for_backward(qkv, P)
        ctx.dims = (B, T, H, Hkv, Dh)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, P = ctx.saved_tensors
        B, T, H, Hkv, Dh = ctx.dims
        C, row = _qkv_layout(B, T, H, Hkv, Dh)
        grp = H // Hkv
        alpha = 1.0 / math.sqrt(Dh)
        dout = dout.contiguous()
        dev = qkv.device
        q, k, v = qkv, qkv[..., C:], qkv[..., C + Hkv * Dh:]
        dqkv = torch.empty_like(qkv)
        dq, dk, dv = dqkv, dqkv[..., C:], dqkv[..., C + Hkv * Dh:]
        dP = torch.empty((B, H, T, T), dtype=torch.bfloat16, device=dev)
        for g in range(grp):
            # dP = dO V^T
            G.gemm_bf16(dout[..., g * Dh:], v, dP[:, g::grp], T, T, Dh, C, row, T, True, True,
                        causal=G.CAUSAL_SKIP_UPPER, batch=B * Hkv, batch_inner=Hkv,
                        strides=(T * C, grp * Dh, T * row, Dh, H * T * T, grp * T * T))
        gpu_ext().softmax_bwd(P, dP, dP, B * H * T, T, True)
        for g in range(grp):
            # dQ = alpha * dS K
            G.gemm_bf16(dP[:, g::grp], k, dq[..., g * Dh:], T, Dh, T, T, row, row, True, False, alpha=alpha,
                        causal=G.CAUSAL_K_UPTO_M, batch=B * Hkv, batch_inner=Hkv,
                        strides=(H * T * T, grp * T * T, T * row, Dh, T * row, grp * Dh))
        # dK, dV sum over the q-heads of a group: first group writes, the rest accumulate
        for g in range(grp):
            acc = g > 0
            G.gemm_bf16(dP[:, g::grp], q[..., g * Dh:], dk, T, Dh, T, T, row, row, False, False, alpha=alpha,
                        Cin=dk if acc else None, beta=1.0 if acc else 0.0, causal=G.CAUSAL_K_FROM_M,
                        batch=B * Hkv, batch_inner=Hkv,
                        strides=(H * T * T, grp * T * T, T * row, grp * Dh, T * row, Dh))
            G.gemm_bf16(P[:, g::grp], dout[..., g * Dh:], dv, T, Dh, T, T, C, row, False, False,
                        Cin=dv if acc else None, beta=1.0 if acc else 0.0, causal=G.CAUSAL_K_FROM_M,
                        batch=B * Hkv, batch_inner=Hkv,
                        strides=(H * T * T, grp * T * T, T * C, grp * Dh, T * row, Dh))
        return dqkv, None, None, None, None, None


class DocLayout:
    """Document layout of packed sequences: each row of `T` tokens is a concatenation of
    documents and a token attends only to earlier tokens of its own document.

    Two contiguous int32 [B, T] tensors: `start[b, t]` = index of the first token of t's document,
    `end[b, t]` = one past its last.  Every constructor goes through start flags - a position
    starts a document iff it is 0 or flagged; `start` is the running maximum of the flagged
    positions and `end` the reverse running minimum of the next one (or T) - so the arrays are
    valid for any input: both non-decreasing along t, constant within a document, and
    start[t] <= t < end[t].  The attention kernels rely on that and never validate or clamp.
    Build it once per batch; every layer shares it.  On the GPU the flags -> (start, end) step is
    one native launch (`data_ops.hip` doc_layout_kernel); the CPU path is the same scans in torch.
    """

    __slots__ = ("start", "end")

    def __init__(self, start: torch.Tensor, end: torch.Tensor):
        self.start, self.end = start, end

    @property
    def device(self):
        return self.start.device

    @property
    def shape(self):
        return tuple(self.start.shape)

    def to(self, device) -> "DocLayout":
        return DocLayout(self.start.to(device), self.end.to(device))

    @classmethod
    def from_flags(cls, flags: torch.Tensor) -> "DocLayout":
        """flags: [B, T], non-zero where a document starts (position 0 always does)."""
        if flags.dim() != 2:
            raise ValueError("DocLayout: start flags must be [B, T]")
        B, T = flags.shape
        f = (flags != 0).to(torch.uint8).contiguous()
        start = torch.empty((B, T), dtype=torch.int32, device=f.device)
        end = torch.empty_like(start)
        if f.is_cuda:
            gpu_ext().doc_layout(f, start, end)
            return cls(start, end)
        pos = torch.arange(T, dtype=torch.int64, device=f.device).expand(B, T)
        fb = f.bool().clone()
        fb[:, 0] = True
        st = torch.cummax(torch.where(fb, pos, torch.zeros_like(pos)), dim=1).values
        # the next start strictly after t: reverse running minimum of the flagged positions > t
        nxt = torch.where(fb, pos, torch.full_like(pos, T))
        nxt = torch.cat([nxt[:, 1:], torch.full((B, 1), T, dtype=torch.int64, device=f.device)], dim=1)
        en = torch.flip(torch.cummin(torch.flip(nxt, dims=[1]), dim=1).values, dims=[1])
        return cls(st.to(torch.int32).contiguous(), en.to(torch.int32).contiguous())

    @classmethod
    def from_lengths(cls, lengths, T: int, device=None) -> "DocLayout":
        """lengths: one list of document lengths per row, each summing to T."""
        flags = torch.zeros((len(lengths), T), dtype=torch.uint8)
        for b, row in enumerate(lengths):
            if any(int(n) <= 0 for n in row) or sum(int(n) for n in row) != T:
                raise ValueError(f"DocLayout.from_lengths: row {b} lengths must be positive and sum to {T}")
            at = 0
            for n in row:
                flags[b, at] = 1
                at += int(n)
        return cls.from_flags(flags.to(device) if device is not None else flags)

    @classmethod
    def from_eos(cls, tokens: torch.Tensor, eos_id: int) -> "DocLayout":
        """The token after an EOS starts a document; position 0 always starts one."""
        flags = torch.zeros(tokens.shape, dtype=torch.uint8, device=tokens.device)
        flags[:, 1:] = (tokens[:, :-1] == eos_id).to(torch.uint8)
        return cls.from_flags(flags)

    @classmethod
    def from_doc_start(cls, t: torch.Tensor) -> "DocLayout":
        """t[b, i] = index of the first token of i's document.  Position i counts as a start iff
        t[b, i] == i, so an input that is not a valid layout still yields a valid one."""
        pos = torch.arange(t.shape[1], device=t.device, dtype=t.dtype)
        return cls.from_flags(t == pos[None, :])

    def mask(self) -> torch.Tensor:
        """Boolean [B, T, T]: query q may attend to key k iff start[q] <= k <= q."""
        T = self.start.shape[1]
        k = torch.arange(T, device=self.start.device)
        return (k[None, None, :] >= self.start[:, :, None].long()) & (k[None, None, :] <= k[None, :, None])


class _FlashAttention(torch.autograd.Function):
    """Fused causal flash attention (csrc/kernels/attn_flash.hip): no T x T matrix in HBM."""

    @staticmethod
    def forward(ctx, qkv, B, T, H, Hkv, Dh, docs=None, window=None, drop=None):
        """window (int, 1 <= window < T, or None): the sliding-window kernels, with or without docs.
        drop (None, or (thr, seed, offset, device_base)): the dropout kernels, under any mask; the
        backward regenerates the mask from the same stream position."""
        qkv = qkv.contiguous()
        out = torch.empty((B, T, H * Dh), dtype=torch.bfloat16, device=qkv.device)
        lse = torch.empty((B * H, T), dtype=torch.float32, device=qkv.device)
        scale = 1.0 / math.sqrt(Dh)
        if drop is not None:
            thr, seed, offset, base = drop
            gpu_ext().flash_fwd_drop(qkv, out, lse, window or 0, docs.start if docs is not None else None,
                                     docs.end if docs is not None else None, thr, seed, offset, base,
                                     B, T, H, Hkv, Dh, scale)
        elif window is not None:
            gpu_ext().flash_fwd_win(qkv, out, lse, window, docs.start if docs is not None else None,
                                    docs.end if docs is not None else None, B, T, H, Hkv, Dh, scale)
        elif docs is None:
            gpu_ext().flash_fwd(qkv, out, lse, B, T, H, Hkv, Dh, scale)
        else:
            gpu_ext().flash_fwd_doc(qkv, out, lse, docs.start, docs.end, B, T, H, Hkv, Dh, scale)
        ctx.save_for_backward(qkv, out, lse)
        ctx.dims = (B, T, H, Hkv, Dh, scale)
        ctx.docs = docs  # (int32 layout tensors: no gradient, shared by every layer of the step)
        ctx.window = window
        ctx.drop = drop
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        B, T, H, Hkv, Dh, scale = ctx.dims
        dqkv = torch.empty_like(qkv)
        delta = torch.empty((B * H, T), dtype=torch.float32, device=qkv.device)
        # the column sums of dqkv (the qkv projection's bias gradient) as per-16-row partials
        # written by the kernels on the way out, offered to that projection's colsum()
        Wd = qkv.shape[-1]
        cs = torch.empty((B * T // 16, Wd), dtype=torch.float32, device=qkv.device) if G.partials_wanted() else None
        qs = _dkdv_head_split(B, T, H, Hkv, qkv.device)
        part = torch.empty(qs * B * T * Hkv * 2 * Dh, dtype=torch.float32, device=qkv.device) if qs > 1 else None
        dout = dout.contiguous()
        docs = ctx.docs
        if ctx.drop is not None:
            thr, seed, offset, base = ctx.drop
            gpu_ext().flash_bwd_drop(qkv, out, dout, lse, delta, dqkv, ctx.window or 0,
                                     docs.start if docs is not None else None,
                                     docs.end if docs is not None else None, thr, seed, offset, base,
                                     B, T, H, Hkv, Dh, scale, cs, part, qs)
        elif ctx.window is not None:
            gpu_ext().flash_bwd_win(qkv, out, dout, lse, delta, dqkv, ctx.window,
                                    docs.start if docs is not None else None,
                                    docs.end if docs is not None else None, B, T, H, Hkv, Dh, scale, cs, part, qs)
        elif docs is None:
            gpu_ext().flash_bwd(qkv, out, dout, lse, delta, dqkv, B, T, H, Hkv, Dh, scale, cs, part, qs)
        else:
            gpu_ext().flash_bwd_doc(qkv, out, dout, lse, delta, dqkv, docs.start, docs.end, B, T, H, Hkv, Dh, scale,
                                    cs, part, qs)
        if cs is not None:
            G.offer_colsum_partials(dqkv, cs)
        return dqkv, None, None, None, None, None, None, None, None


def _dkdv_head_split(B: int, T: int, H: int, Hkv: int, device) -> int:
    """q-head subsets per GQA group for the dK/dV pass.  One dK/dV block owns 64 keys of one
    kv-head and loops over every q-head of its group, so a short batch (Llama-3-8B at B=1,
    T=2048: 8 kv-heads x 32 key blocks = 256 blocks, the heaviest with 4x32 steps) fills one
    block per CU with a 2:1 load imbalance.  Splitting the group over `qs` blocks multiplies the
    block count (partials summed in a fixed order by dkdv_reduce_kernel: deterministic) and lets
    the heavy-first order balance them.  RTDC_FA_QS forces a value (1 = no split)."""
    grp = H // Hkv
    forced = int(os.environ.get("RTDC_FA_QS", "0"))
    if forced:
        return forced if grp % forced == 0 else 1
    from .gemm import _num_cus

    blocks, cus = B * Hkv * (T // 64), _num_cus(device)
    qs = 1
    while grp % (qs * 2) == 0 and blocks * qs < 4 * cus:
        qs *= 2
    return qs


def flash_supported(T: int, Dh: int) -> bool:
    return T % 64 == 0 and Dh in (64, 128)


def window_mask(T: int, window: int, device=None) -> torch.Tensor:
    """Boolean [T, T]: query q may attend to key k iff q - window < k <= q (its last `window` keys)."""
    t = torch.arange(T, device=device)
    return (t[None, :] <= t[:, None]) & (t[None, :] > t[:, None] - window)


def attention_dropout_keep(p: float) -> tuple[int, float]:
    """(thr, inv_keep) of attention dropout at probability p.  The drop probability is quantised
    to 1/256: thr = round(256 p) must lie in 1..255, an element is dropped with probability
    thr / 256 (p = 0.1 -> 26 / 256) and the survivors are scaled by inv_keep = 256 / (256 - thr),
    the realised keep probability, so the expectation is exact."""
    thr = int(round(256.0 * float(p)))
    if not 1 <= thr <= 255:
        raise ValueError(f"attention dropout: round(256 * p) must lie in 1..255, got p={p} (thr={thr})")
    return thr, 256.0 / (256 - thr)


def attention_dropout_counters(B: int, H: int, T: int) -> int:
    """Philox counters one attention dropout forward reserves: one per 4 x 4 block of every
    (b, h) score matrix, the blocks above the diagonal included."""
    if T % 4:
        raise ValueError(f"attention dropout needs T % 4 == 0, got T={T}")
    return B * H * (T // 4) ** 2


def attention_dropout_mask(seed: int, offset: int, B: int, H: int, T: int, p: float) -> torch.Tensor:
    """The keep mask of the flash kernels (attn_flash.hip drop_keep16) as a bool [B, H, T, T] CPU
    tensor, built in numpy on `philox4x32`: block = ((b H + h) nb + q // 4) nb + key // 4 with
    nb = T / 4, words = Philox(seed, 0, offset + block); word q % 4, byte key % 4 (little end
    first) decides element (q, key), kept iff byte >= thr."""
    import numpy as np

    thr, _ = attention_dropout_keep(p)
    n, nb = attention_dropout_counters(B, H, T), T // 4
    ctr = (np.arange(n, dtype=np.uint64) + np.uint64(int(offset) & ((1 << 64) - 1)))  # (wraps mod 2^64)
    words = philox4x32(seed, 0, ctr)                                         # [n, 4]: word = q % 4
    shifts = np.array([0, 8, 16, 24], dtype=np.uint32)
    byte = (words[:, :, None] >> shifts[None, None, :]) & np.uint32(0xFF)     # [n, q % 4, key % 4]
    keep = (byte >= np.uint32(thr)).reshape(B, H, nb, nb, 4, 4).transpose(0, 1, 2, 4, 3, 5).reshape(B, H, T, T)
    return torch.from_numpy(np.ascontiguousarray(keep))


def causal_attention_ref(qkv, B, T, H, Hkv, Dh, docs=None, window=None, keep=None, inv_keep=1.0):
    """keep (bool [B, H, T, T], attention_dropout_mask) with inv_keep: attention dropout, through an
    explicit softmax - P is normalised over every allowed key, then the kept entries are scaled."""
    C = H * Dh
    q = qkv[..., :C].reshape(B, T, H, Dh).transpose(1, 2)
    k = qkv[..., C:C + Hkv * Dh].reshape(B, T, Hkv, Dh).transpose(1, 2)
    v = qkv[..., C + Hkv * Dh:].reshape(B, T, Hkv, Dh).transpose(1, 2)
    if Hkv != H:
        k = k.repeat_interleave(H // Hkv, dim=1)
        v = v.repeat_interleave(H // Hkv, dim=1)
    if keep is not None:
        allowed = window_mask(T, window if window is not None else T, qkv.device)[None, None]
        if docs is not None:
            allowed = allowed & docs.mask()[:, None]
        s = (q.float() @ k.float().transpose(-1, -2)) * (1.0 / math.sqrt(Dh))
        pm = torch.softmax(s.masked_fill(~allowed, -math.inf), dim=-1)
        pm = pm * (keep.to(qkv.device).to(pm.dtype) * inv_keep)
        o = (pm @ v.float()).to(qkv.dtype)
        return o.transpose(1, 2).reshape(B, T, C)
    if window is not None:  # boolean band mask, inside the document when both are given
        band = window_mask(T, window, qkv.device)[None, None]
        o = F.scaled_dot_product_attention(q, k, v, attn_mask=band if docs is None else band & docs.mask()[:, None])
    elif docs is None:
        o = F.scaled_dot_product_attention(q, k, v, is_causal=True)
    else:  # boolean mask start[q] <= key <= q: the oracle of the document-masked kernels
        o = F.scaled_dot_product_attention(q, k, v, attn_mask=docs.mask()[:, None])
    return o.transpose(1, 2).reshape(B, T, C)


def causal_attention(qkv: torch.Tensor, n_head: int, n_kv_head: int | None = None,
                     docs: DocLayout | None = None, window: int | None = None, dropout_p: float = 0.0,
                     training: bool = True, stream: PhiloxStream | None = None) -> torch.Tensor:
    """qkv: [B, T, (H + 2*Hkv) * Dh] -> [B, T, H*Dh].  docs (packed sequences): row q attends to
    the keys start[q] <= key <= q of its own document only; it needs the flash path - there is
    no unmasked fallback.  window (sliding-window attention, None = off): row q attends to its
    last `window` keys only, max(0, q - window + 1) <= key <= q, within its document when docs is
    given; window >= T masks nothing and runs the kernels that run without it.  Like docs it needs
    the flash path on the GPU.  Without docs and window any T runs: the composed path pads T to a
    multiple of 64.
    dropout_p (attention dropout, active when training and dropout_p != 0): the probabilities are
    dropped after the softmax with the quantised probability of attention_dropout_keep, under any
    mask.  The keep mask is drawn inside the flash kernels from B * H * (T/4)^2 counters reserved
    from `stream` (default: the default stream) and regenerated in the backward; the CPU path draws
    the same mask from the same stream state (attention_dropout_mask).  Like docs and window it
    needs the flash path on the GPU."""
    B, T, W = qkv.shape
    Hkv = n_kv_head or n_head
    Dh = W // (n_head + 2 * Hkv)
    if window is not None:
        window = int(window)
        if window < 1:
            raise ValueError(f"causal_attention: window must be >= 1 (None = off), got {window}")
        if window >= T:
            window = None
    if docs is not None:
        if docs.shape != (B, T):
            raise ValueError(f"causal_attention: docs layout is {docs.shape}, qkv is [{B}, {T}, ...]")
        if docs.device != qkv.device:
            raise ValueError(f"causal_attention: docs on {docs.device}, qkv on {qkv.device}")
    thr = 0
    if training and dropout_p != 0.0:
        thr, inv_keep = attention_dropout_keep(dropout_p)
        ncnt = attention_dropout_counters(B, n_head, T)
    if qkv.is_cuda:
        require_dtype(qkv, "causal_attention")
    elif thr:
        seed, offset = (stream or default_stream()).reserve_counters(ncnt)
        keep = attention_dropout_mask(seed, offset, B, n_head, T, dropout_p)
        return causal_attention_ref(qkv, B, T, n_head, Hkv, Dh, docs, window, keep, inv_keep)
    else:
        return causal_attention_ref(qkv, B, T, n_head, Hkv, Dh, docs, window)
    impl = os.environ.get("RTDC_ATTN", "flash")
    if thr:
        if impl != "flash" or not flash_supported(T, Dh):
            raise RuntimeError(
                f"causal_attention: attention dropout needs the flash kernels (T % 64 == 0, Dh in (64, 128), "
                f"RTDC_ATTN=flash); got T={T}, Dh={Dh}, RTDC_ATTN={impl}")
        st = stream or default_stream()
        seed, offset = st.reserve_counters(ncnt)
        return _FlashAttention.apply(qkv, B, T, n_head, Hkv, Dh, docs, window, (thr, seed, offset, st.device_base()))
    if window is not None:
        if impl != "flash" or not flash_supported(T, Dh):
            raise RuntimeError(
                f"causal_attention: a sliding window needs the flash kernels (T % 64 == 0, Dh in (64, 128), "
                f"RTDC_ATTN=flash); got T={T}, Dh={Dh}, RTDC_ATTN={impl}")
        return _FlashAttention.apply(qkv, B, T, n_head, Hkv, Dh, docs, window)
    if docs is not None:
        if impl != "flash" or not flash_supported(T, Dh):
            raise RuntimeError(
                f"causal_attention: document masking needs the flash kernels (T % 64 == 0, Dh in (64, 128), "
                f"RTDC_ATTN=flash); got T={T}, Dh={Dh}, RTDC_ATTN={impl}")
        return _FlashAttention.apply(qkv, B, T, n_head, Hkv, Dh, docs)
    if impl == "flash" and flash_supported(T, Dh):
        return _FlashAttention.apply(qkv, B, T, n_head, Hkv, Dh)
    if T % 64:
        # the composed GEMMs take T as a reduction length and as the row pitch of P (gemm_bf16 needs
        # K % 64 == 0): zero rows are appended.  Causality keeps them out of every real row, and their
        # dO is zero in the backward (the slice's gradient), so they add nothing to dK / dV either.
        pad = -T % 64
        return _CausalAttention.apply(F.pad(qkv, (0, 0, 0, pad)), B, T + pad, n_head, Hkv, Dh)[:, :T]
    return _CausalAttention.apply(qkv, B, T, n_head, Hkv, Dh)
