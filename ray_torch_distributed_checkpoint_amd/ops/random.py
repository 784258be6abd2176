"""Checkpointable counter-based (Philox4x32-10) RNG stream for the native dropout kernels.

Every dropout launch consumes a contiguous counter range [offset, offset + ceil(n/4)) of the
stream (seed).  The state is two integers, saved in checkpoints and restored on resume so the
masks after a restart are bit-identical (BASELINE config 5); the backward pass regenerates a
mask from the (seed, offset) recorded by its forward instead of storing it.
"""
from __future__ import annotations

import threading


class PhiloxStream:
    """In graph mode (a captured hipGraph step, utils/graphs.py) the counter base lives in a
    device int64 (`device_base`): kernels add it to the step-relative offsets recorded at
    capture time, and the captured step ends with `base += consumed`, so every replay draws
    fresh masks while the host never runs."""

    def __init__(self, seed: int = 0x5EED, offset: int = 0):
        self.seed = int(seed) & ((1 << 64) - 1)
        self.offset = int(offset)
        self._lock = threading.Lock()
        self._base = None  # device counter base in graph mode
        self._graph_users = 0  # live captured steps sharing _base (acquire/release_graph_mode)

    def device_base(self):
        return self._base

    def enter_graph_mode(self, device) -> None:
        import torch

        self._base = torch.tensor([self.offset], dtype=torch.int64, device=device)
        self.offset = 0

    def end_graph_step(self) -> None:
        """Called inside the capture after the step's last dropout: advance the device base."""
        self._base.add_(self.offset)
        self.offset = 0

    def exit_graph_mode(self) -> None:
        if self._base is not None:
            self.offset = int(self._base.item()) + self.offset
            self._base = None
        self._graph_users = 0

    def acquire_graph_mode(self, device) -> None:
        """A captured step starts using the device base: the first user enters graph mode, the
        others share it (each of their graphs ends with base += consumed)."""
        if self._base is None:
            self.enter_graph_mode(device)
            self._graph_users = 0
        self._graph_users += 1

    def release_graph_mode(self) -> None:
        """A captured step is closed: graph mode ends with the LAST user, so no live graph ever
        replays against a freed device base (or a host offset that overlaps its counter)."""
        if self._graph_users > 0:
            self._graph_users -= 1
            if self._graph_users == 0:
                self.exit_graph_mode()

    def reserve(self, numel: int) -> tuple[int, int]:
        """Reserve counters for `numel` elements; returns (seed, offset)."""
        n = (int(numel) + 3) // 4
        with self._lock:
            off = self.offset
            self.offset += n
        return self.seed, off

    def reserve_counters(self, n: int) -> tuple[int, int]:
        """Reserve `n` consecutive counters (Philox calls, not elements); returns (seed, offset).
        Attention dropout takes one counter per 4 x 4 block of the score matrix."""
        n = int(n)
        if n < 0:
            raise ValueError(f"reserve_counters: n must be >= 0, got {n}")
        with self._lock:
            off = self.offset
            self.offset += n
        return self.seed, off

    def state_dict(self) -> dict:
        off = self.offset if self._base is None else int(self._base.item()) + self.offset
        return {"seed": self.seed, "offset": off}

    def load_state_dict(self, sd: dict) -> None:
        self.seed = int(sd["seed"])
        if self._base is not None:
            self._base.fill_(int(sd["offset"]))
            self.offset = 0
        else:
            self.offset = int(sd["offset"])


_default = PhiloxStream()


def default_stream() -> PhiloxStream:
    return _default


def manual_seed(seed: int) -> None:
    _default.seed = int(seed) & ((1 << 64) - 1)
    _default.offset = 0


# ---- stochastic rounding of bf16 optimizer state (optim/fused.py FusedAdamW(state_dtype=bfloat16)) ----
# NumPy twins of `Philox::gen` (csrc/kernels/common.h) and `sr_bf16` (csrc/kernels/optim.hip): the
# CPU reference path and the tests draw exactly the bits the kernel draws.

_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK32 = 0xFFFFFFFF


def philox4x32(seed: int, ctr_hi: int, ctr_lo):
    """Philox4x32-10 in the layout of `Philox::gen(seed, ctr_hi, ctr_lo)`: key = seed's two
    words, counter = (ctr_lo low, ctr_lo high, ctr_hi low, ctr_hi high).  `ctr_lo`: an integer
    or an array of them; returns uint32 [..., 4]."""
    import numpy as np

    lo = np.asarray(ctr_lo, dtype=np.uint64)
    seed, ctr_hi = int(seed) & ((1 << 64) - 1), int(ctr_hi) & ((1 << 64) - 1)
    m32 = np.uint64(_MASK32)
    s32 = np.uint64(32)
    c0, c1 = lo & m32, lo >> s32
    c2 = np.full_like(lo, ctr_hi & _MASK32)
    c3 = np.full_like(lo, ctr_hi >> 32)
    k0, k1 = seed & _MASK32, seed >> 32
    for _ in range(10):
        p0 = np.uint64(_M0) * c0  # (two uint32 factors: the product fits uint64)
        p1 = np.uint64(_M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + _W0) & _MASK32, (k1 + _W1) & _MASK32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def sr_words(seed: int, step: int, start: int, n: int):
    """The uint32 word of each flat element in [start, start + n): element e draws
    `philox4x32(seed, step, e >> 2)[e & 3]`.  exp_avg rounds with its low 16 bits, exp_avg_sq
    with its high 16."""
    import numpy as np

    if n <= 0:
        return np.zeros(0, dtype=np.uint32)
    g0, g1 = start >> 2, (start + n - 1) >> 2
    r = philox4x32(seed, step, np.arange(g0, g1 + 1, dtype=np.uint64)).reshape(-1)
    off = start - (g0 << 2)
    return r[off:off + n]


def sr_bf16_bits(x, r16):
    """Stochastic rounding of fp32 `x` (array) to bf16 with 16 random bits per element; returns
    the bf16 bit patterns (uint16).  On the sign-magnitude bits b of x: (b + r16) >> 16, so the
    result is the bf16 neighbour away from zero with probability (b & 0xFFFF) / 65536 - unbiased
    for both signs, exact for a bf16-representable x.  Inf / NaN pass through (b >> 16) and a
    finite x is never carried to infinity."""
    import numpy as np

    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    u = b + np.asarray(r16).astype(np.uint32)  # (wraps only for NaN patterns, which keep b)
    exp = np.uint32(0x7F800000)
    keep = ((b & exp) == exp) | ((u & exp) == exp)
    return (np.where(keep, b, u) >> np.uint32(16)).astype(np.uint16)


def sr_bf16(x, r16):
    """`sr_bf16_bits` on torch tensors: fp32 `x` -> bfloat16 tensor of the same shape (CPU)."""
    import numpy as np
    import torch

    bits = sr_bf16_bits(x.detach().float().contiguous().numpy(), np.asarray(r16))
    return torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16).reshape(x.shape)
