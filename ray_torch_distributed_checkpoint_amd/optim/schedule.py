"""Learning-rate schedules for the fused optimizers, and the host-built tables of their
capturable (device-resident) step.

A schedule is a pure function of the optimizer-step number: no RNG, no hidden state, so a resumed
run needs only the step count that already comes back with the optimizer state.  The convention is
torch's `LambdaLR` called after every `opt.step()`: the n-th optimizer step (n = 1, 2, ...) uses

    lr_g(n) = base_lr_g * f(n - 1)                      (Python doubles)

with the multiplier f(k), k = 0, 1, ...:

    warmup      f(k) = (k + 1) / warmup_steps                           k < warmup_steps
    decay       p = (k - s) / (total_steps - 1 - s),  s = max(warmup_steps - 1, 0)
      cosine    f(k) = r + (1 - r) * 0.5 * (1 + cos(pi * p))            r = min_lr_ratio
      linear    f(k) = r + (1 - r) * (1 - p)
    after       f(k) = f(total_steps - 1)                               k >= total_steps

so the decay starts from 1 at the last warmup step (the first step when there is no warmup) and
reaches `min_lr_ratio` exactly at k = total_steps - 1, the `total_steps`-th optimizer step.

`FusedAdamW(..., lr_schedule=s)` / `FusedSGD(..., lr_schedule=s)` (or `opt.lr_schedule = s` later)
attach one; optim/fused.py writes `group["lr"]` from it at the start of every step, so a scheduled
run is bit for bit a run whose caller set `group["lr"]` by hand.  With `capturable=True` the kernels
read the same values from the tables built here:

* `lr_table`: fp32 [n_groups, L], row g = float32(base_g * f(k)), k = 0 .. L - 1 (L = total_steps;
  1 for a constant schedule) - the kernel reads column min(completed steps, L - 1);
* `bias_correction_table(b1, b2)`: fp32 [Lbc, 2], row t - 1 = {float32(1 - b1**t),
  float32(sqrt(1 - b2**t))}, the expressions the host path passes by value; Lbc is the first t at
  which both are exactly 1.0f (they stay there), the kernel reads row min(t, Lbc).

Both hold the very doubles the host path rounds to fp32, so the device path is the host path bit
for bit; nothing is recomputed on the device (its pow / cos are not correctly rounded).
"""
from __future__ import annotations

import functools
import math

import numpy as np

MAX_BC_ROWS = 1 << 22  # bias-correction rows a capturable AdamW may need (16 B / row pair: 32 MB)


class LRSchedule:
    """Multiplier f(k) of the (k + 1)-th optimizer step; constant from k = total_steps - 1 on."""

    def __init__(self, kind: str, fn, total_steps: int):
        total_steps = int(total_steps)
        if total_steps < 1:
            raise ValueError(f"total_steps must be >= 1, got {total_steps}")
        self.kind = kind
        self.total_steps = total_steps
        self._fn = fn

    # -- constructors --------------------------------------------------------------------------
    @classmethod
    def constant(cls) -> "LRSchedule":
        return cls("constant", lambda k: 1.0, 1)

    @classmethod
    def warmup_cosine(cls, warmup_steps: int, total_steps: int, min_lr_ratio: float = 0.0) -> "LRSchedule":
        return cls._warmup_decay("cosine", warmup_steps, total_steps, min_lr_ratio)

    @classmethod
    def warmup_linear(cls, warmup_steps: int, total_steps: int, min_lr_ratio: float = 0.0) -> "LRSchedule":
        return cls._warmup_decay("linear", warmup_steps, total_steps, min_lr_ratio)

    @classmethod
    def from_fn(cls, fn, total_steps: int) -> "LRSchedule":
        """`fn(k)`, k = 0 .. total_steps - 1, returns the multiplier of the (k + 1)-th optimizer
        step as a Python float (the lambda a `LambdaLR` would be given)."""
        return cls("fn", lambda k: float(fn(k)), total_steps)

    @classmethod
    def _warmup_decay(cls, kind, warmup_steps, total_steps, min_lr_ratio) -> "LRSchedule":
        w, total, r = int(warmup_steps), int(total_steps), float(min_lr_ratio)
        if total < 1:
            raise ValueError(f"total_steps must be >= 1, got {total}")
        if w < 0 or w > total:
            raise ValueError(f"warmup_steps must be in [0, total_steps = {total}], got {w}")
        if not 0.0 <= r <= 1.0:
            raise ValueError(f"min_lr_ratio must be in [0, 1], got {min_lr_ratio}")
        s = max(w - 1, 0)
        span = total - 1 - s

        def f(k: int) -> float:
            if k < w:
                return (k + 1) / w
            p = (k - s) / span if span > 0 else 0.0
            if kind == "cosine":
                return r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * p))
            return r + (1.0 - r) * (1.0 - p)

        sch = cls(kind, f, total)
        sch.warmup_steps, sch.min_lr_ratio = w, r
        return sch

    # -- values --------------------------------------------------------------------------------
    @property
    def is_constant(self) -> bool:
        return self.kind == "constant"

    def multiplier(self, k: int) -> float:
        """f(k): the multiplier of the (k + 1)-th optimizer step."""
        return self._fn(min(max(int(k), 0), self.total_steps - 1))

    __call__ = multiplier

    def lr(self, base_lr: float, n: int) -> float:
        """Learning rate of the n-th optimizer step (n >= 1)."""
        return base_lr * self.multiplier(n - 1)

    def lr_table(self, base_lrs) -> np.ndarray:
        return lr_table(base_lrs, self)

    def __repr__(self) -> str:
        extra = "".join(f", {k}={getattr(self, k)}" for k in ("warmup_steps", "min_lr_ratio") if hasattr(self, k))
        return f"LRSchedule({self.kind}, total_steps={self.total_steps}{extra})"


class ScheduleBinding:
    """A schedule attached to an optimizer: the schedule and the groups' base learning rates
    (their `lr` at the moment of attaching).  Lives on the optimizer, not in `param_groups`."""

    def __init__(self, schedule: LRSchedule, base_lrs):
        self.schedule = schedule
        self.base_lrs = [float(b) for b in base_lrs]

    def lrs(self, n: int) -> list:
        """Every group's learning rate of the n-th optimizer step."""
        f = self.schedule.multiplier(n - 1)
        return [b * f for b in self.base_lrs]


def lr_table(base_lrs, schedule: LRSchedule | None = None) -> np.ndarray:
    """fp32 [n_groups, L]: row g = float32(base_g * f(k)), k = 0 .. L - 1; L = 1 without a schedule."""
    if schedule is None or schedule.is_constant:
        mult = [1.0] if schedule is None else [schedule.multiplier(0)]
    else:
        mult = [schedule.multiplier(k) for k in range(schedule.total_steps)]
    return np.array([[np.float32(float(b) * f) for f in mult] for b in base_lrs], dtype=np.float32).reshape(
        len(base_lrs), len(mult))


def _bc_row(b1: float, b2: float, t: int):
    return np.float32(1 - b1 ** t), np.float32(math.sqrt(1 - b2 ** t))


@functools.lru_cache(maxsize=16)
def bias_correction_table(b1: float, b2: float, max_rows: int = MAX_BC_ROWS) -> np.ndarray:
    """fp32 [Lbc, 2]: row t - 1 = {float32(1 - b1**t), float32(sqrt(1 - b2**t))} for t = 1 .. Lbc,
    Lbc the first t at which both are exactly 1.0f (b**t only shrinks: they stay 1.0f).  Raises
    ValueError for betas that need more than `max_rows` rows."""
    b1, b2 = float(b1), float(b2)
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError(f"betas must be in [0, 1), got ({b1}, {b2})")
    one = np.float32(1.0)
    if _bc_row(b1, b2, max_rows) != (one, one):
        raise ValueError(f"betas ({b1}, {b2}): the bias corrections are not yet 1.0f after {max_rows} steps - "
                         "too many table rows for a capturable optimizer (use capturable=False)")
    rows = []
    t = 1
    while True:
        row = _bc_row(b1, b2, t)
        rows.append(row)
        if row == (one, one):
            break
        t += 1
    tab = np.array(rows, dtype=np.float32).reshape(len(rows), 2)
    tab.setflags(write=False)
    return tab
