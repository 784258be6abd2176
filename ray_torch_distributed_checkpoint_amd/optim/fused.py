"""Fused AdamW / SGD: one native launch per param group over the model's flat buffers.

API and `state_dict()` format match `torch.optim.AdamW` / `torch.optim.SGD` (state keys
`step`, `exp_avg`, `exp_avg_sq` / `momentum_buffer`), so checkpoints interoperate with stock
torch.  On the GPU the state tensors are views into flat fp32 buffers and the step is the
chunk-table kernel in csrc/kernels/optim.hip, which also refreshes the bf16 compute shadows.
On the CPU the same math runs per tensor with torch ops (reference path).

Host cost per step is O(#params) Python dict work and nothing else: AdamW step counts are
plain host integers (torch keeps one CPU tensor per parameter and does `step += 1` plus a
`float()` on each - ~150 tensor ops per GPT-2 step that left the GPU idle before the
optimizer launch); the per-parameter `step` tensors are materialised only by
`state_dict()` and parsed back by `load_state_dict()`, so checkpoints stay torch-compatible.
Like torch.optim, parameters without a gradient this step are skipped entirely (no weight
decay, no momentum), and the chunk table is built only from parameters that have one.

Global gradient-norm clipping (`max_grad_norm`, off by default) is fused into the step: a
read-only pass over the same chunk tables writes one sum of squares per chunk, a single-block
kernel turns them into `{total_norm, coef}` on the device, and the update kernels fold `coef`
into the gradient multiply they already do - one extra read of the gradients, no write, no
host sync, no atomics.  The norm is over every parameter of every param group that has a
gradient this step (`clip_grad_norm_(model.parameters())`); under ZeRO-1 each rank sums its
owned shards and the ranks' sums are all-gathered and added in rank order, so every rank gets
the same bits.  Determinism: for a fixed configuration (world size, ZeRO stage, bucket plan,
tail split) the chunk tables and every summation order are fixed, so the norm is bitwise
reproducible from run to run and across a restart.  Across configurations the chunk cuts
differ, and only agreement to fp32 rounding is promised.  The GPU kernels carry the sums of
squares in fp64 and round once, at the norm, so in practice two cuts of the same gradient give
the same fp32 norm (their fp64 sums agree to ~1e-15; the norms differ only if the exact value
lies that close to an fp32 rounding boundary) - with fp32 sums a ZeRO-1 and a replicated run
got coefficients one ulp apart, which bf16 compute amplifies to visibly different parameters
within a few steps.  The CPU reference paths sum in fp32.

bf16 moment state (`FusedAdamW(state_dtype=torch.bfloat16)`, off by default): `exp_avg` and
`exp_avg_sq` live in bf16 flat buffers and are rounded stochastically after every update, with
Philox bits that are a pure function of (rounding_seed, step, flat element index) - the rule and
its NumPy twin are in ops/random.py, the kernel is `adamw_bf16state_kernel`.  With bf16 state the
CPU also steps over the flat buffers (every element needs its flat index).

Learning-rate schedules (`lr_schedule=`, optim/schedule.py; off by default): `step()` first writes
`group["lr"] = base_lr * f(step_count)` and then runs the code above unchanged.  `capturable=True`
(off by default) replaces the per-step host scalars of the native launches - lr, AdamW's two bias
corrections, the bf16-state kernel's step word - by device tables indexed with a device step
counter that a one-thread kernel increments after the last update launch of every step, so a
step captured into a hipGraph keeps stepping them; the results are the host path's bit for bit.
"""
from __future__ import annotations

import math

import torch

from ..ops._ext import gpu_ext
from ..ops.random import sr_bf16, sr_words
from ..ops.shadow import bump_generation
from .flat import FlatParamSpace, space_of


class _FlatOptimizer(torch.optim.Optimizer):
    _state_keys: tuple = ()
    _counts_steps = False  # the state carries a per-parameter `step` (AdamW)

    def __init__(self, params, defaults, max_grad_norm=None, lr_schedule=None, capturable=False):
        super().__init__(params, defaults)
        # number of step() calls (host int; AdamW's load_state_dict restores it from the loaded
        # per-parameter steps, FusedSGD's state has none: set `opt.step_count` after a load)
        self._step_count = 0
        # learning-rate schedule (optim/schedule.py): `group["lr"]` is rewritten from it at the
        # start of every step.  Attributes, not param-group options: state_dict() and checkpoints
        # keep their keys.
        self._sched = None
        # capturable=True (GPU): lr, bias corrections and the step number are read by the kernels
        # from device tables indexed by a device step counter, so a step captured into a hipGraph
        # keeps stepping them on replay.  `_dev` holds that state, `_captured` the parameters of
        # captured launches (None: never captured - then nothing is ever read back).
        self.capturable = bool(capturable)
        self._dev = None
        self._captured = None
        self.lr_schedule = lr_schedule
        # clip the global gradient norm to this value inside the step (None / 0: off).  An
        # attribute, not a param-group option: state_dict() and checkpoints do not change.
        # Unlike torch.nn.utils.clip_grad_norm_, `p.grad` is left UNSCALED - the coefficient is
        # applied inside the update.
        self.max_grad_norm = max_grad_norm
        # pre-clip global norm of the last clipped step: a 0-dim fp32 tensor on the parameters'
        # device (a view of the clip workspace: reading it is the caller's sync, the step has
        # none); None before the first clipped step
        self.grad_norm = None
        self._clip_ws = None
        self._space: FlatParamSpace | None = None
        self._bufs: dict[str, torch.Tensor] = {}
        self._steps: dict = {}  # param -> number of optimizer steps taken (host int)
        self._bound: set = set()
        self._have = None  # parameters with a gradient this step (set by the native step)
        self._overlap = None  # optim.overlap.BackwardOverlap (updates run during backward)
        # dtype of the flat optimizer-state buffers (FusedAdamW(state_dtype=...) may set bfloat16)
        self.state_dtype = torch.float32
        # DistributedDataParallel(zero_stage=1) leaves p.grad reduced only on this rank's shards:
        # only these optimizers (which update exactly the owned shards) may step such a model
        for p in self._all_params():
            p._rtdc_zero_capable = True

    # -- flat setup ------------------------------------------------------------------------
    def _all_params(self):
        return [p for g in self.param_groups for p in g["params"]]

    def _ensure_space(self):
        if self._space is not None:
            return self._space
        params = self._all_params()
        sp = space_of(params)
        if sp is None or any(p not in set(sp.params) for p in params):
            saved = [p.grad.detach().clone() if p.grad is not None else None for p in params]
            sp = FlatParamSpace(params)
            for p, g in zip(params, saved):
                if g is not None:
                    p.grad.copy_(g)
                else:
                    p.grad = None
        self._space = sp
        # optimizer state: the whole flat space, or (ZeRO-1) only this rank's owned shards,
        # back to back - 1/world of the bytes (FlatParamSpace.state_numel)
        for k in self._state_keys:
            self._bufs[k] = torch.zeros(sp.state_numel, dtype=self.state_dtype, device=sp.device)
        # adopt any state that already exists (e.g. loaded before the first step)
        for p in params:
            st = self.state.get(p)
            if st is None:
                continue
            for k in self._state_keys:
                if k in st and st[k] is not None:
                    self._adopt(p, k, st[k])
                    st[k] = self._state_value(p, k)
        return sp

    # -- per-parameter state views -------------------------------------------------------------
    def _state_value(self, p, k):
        """What `self.state[p][k]` holds: a view of the flat state buffer, or under ZeRO-1 a
        `FlatShardedTensor` over this rank's compact slices (checkpoint/sharded.py) - the value
        a sharded checkpoint writes and reads without any all-gather."""
        sp = self._space
        seg = sp.segment_of(p)
        z = sp.zero
        if z is None:
            return FlatParamSpace.view(self._bufs[k], seg)
        from ..checkpoint.sharded import FlatShardedTensor

        buf = self._bufs[k]
        local = [(a - seg.offset, buf[so:so + (b - a)]) for a, b, so in sp.owned_ranges(seg)]
        lo, hi = seg.offset, seg.offset + seg.numel
        ranges = []
        for r in range(z.world):
            rr = []
            for oa, ob in z.owned_by(r):
                a, b = max(lo, oa), min(hi, ob)
                if a < b:
                    rr.append((a - lo, b - lo))
            ranges.append(rr)
        return FlatShardedTensor(seg.shape, buf.dtype, local, ranges, z.rank)

    def _adopt(self, p, k, v) -> None:
        """Copy a loaded/pre-existing state value into this optimizer's buffers (no-op when it
        already views them).  `v`: a full tensor of the parameter's shape, or a
        FlatShardedTensor whose local pieces cover this rank's owned ranges."""
        from ..checkpoint.sharded import FlatShardedTensor

        sp = self._space
        seg = sp.segment_of(p)
        buf = self._bufs[k]
        if isinstance(v, FlatShardedTensor):
            have = {s: t for s, t in v.local}
            for a, b, so in sp.owned_ranges(seg):
                t = have.get(a - seg.offset)
                if t is None or t.numel() != b - a:
                    raise ValueError(f"optimizer state {k!r}: sharded value does not cover owned range {a}-{b}")
                dst = buf[so:so + (b - a)]
                if t.data_ptr() != dst.data_ptr():
                    with torch.no_grad():
                        dst.copy_(t.reshape(-1).to(dst.device, dst.dtype))
            return
        if not torch.is_tensor(v):
            return
        if sp.zero is None:
            dst = FlatParamSpace.view(buf, seg)
            if v.data_ptr() != dst.data_ptr():
                with torch.no_grad():
                    dst.copy_(v.to(dst.device, dst.dtype))
            return
        # a full (replicated-layout) tensor: keep the owned ranges of its storage-order elements
        full = v.detach().to(buf.device, buf.dtype)
        if seg.channels_last:
            o, i, kh, kw = seg.shape
            full = full.permute(0, 2, 3, 1).contiguous()
        flat = full.reshape(-1)
        with torch.no_grad():
            for a, b, so in sp.owned_ranges(seg):
                buf[so:so + (b - a)].copy_(flat[a - seg.offset:b - seg.offset])

    def _bind_state(self, p):
        if p in self._bound:
            return self.state[p]
        st = self.state[p]
        for k in self._state_keys:
            if k not in st:
                st[k] = self._state_value(p, k)
        self._bound.add(p)
        return st

    def _flat_mode(self) -> bool:
        """Updates run over the flat buffers' chunk tables: always on the GPU (native kernels),
        and on the CPU under ZeRO-1 (owned shards only, compact state - reference path) or with
        bf16 state (the rounding bits are keyed by the flat element index)."""
        if self._use_native() or self.state_dtype != torch.float32:
            return True
        sp = space_of(self._all_params())
        return sp is not None and sp.zero is not None

    @torch.no_grad()
    def init_state(self) -> None:
        """Materialise every per-parameter state entry (zeros, step 0) without stepping, so
        `state_dict()` has its full structure before the first step - what a sharded
        checkpoint load fills in place (torch.distributed.checkpoint.state_dict does the same
        with a zero-grad step, T/distributed/checkpoint/state_dict.py `_init_optim_state`).
        Numerically a no-op for AdamW; for SGD a zero momentum buffer equals torch's
        first-step `buf = g` whenever dampening == 0."""
        flat = self._flat_mode()
        for p in self._all_params():
            st = self.state[p]
            if flat:
                self._ensure_space()
                self._bind_state(p)
            else:
                for k in self._state_keys:
                    if k not in st:
                        st[k] = torch.zeros_like(p, memory_format=torch.preserve_format)
            self._init_extra(p, st)
        self._materialize_steps()

    def _init_extra(self, p, st) -> None:
        pass

    # -- learning-rate schedule, step count, device-resident step state --------------------------
    @property
    def lr_schedule(self):
        return None if self._sched is None else self._sched.schedule

    @lr_schedule.setter
    def lr_schedule(self, schedule) -> None:
        """Attach (or with None detach) an `LRSchedule`; the groups' current `lr` become its base
        learning rates."""
        if schedule is None:
            self._sched = None
            return
        from .schedule import LRSchedule, ScheduleBinding

        if not isinstance(schedule, LRSchedule):
            raise TypeError(f"lr_schedule must be an optim.schedule.LRSchedule, got {type(schedule).__name__}")
        self._sched = ScheduleBinding(schedule, [g["lr"] for g in self.param_groups])

    @property
    def step_count(self) -> int:
        return self._step_count

    @step_count.setter
    def step_count(self, n: int) -> None:
        self._step_count = int(n)
        if self._dev is not None:
            self._dev["count"].fill_(self._step_count)

    def get_last_lr(self) -> list:
        return [g["lr"] for g in self.param_groups]

    def _apply_schedule(self, n: int) -> None:
        """group["lr"] of the n-th optimizer step."""
        for g, lr in zip(self.param_groups, self._sched.lrs(n)):
            g["lr"] = lr

    def _begin_step(self, capturing: bool = False) -> None:
        """Before the first launch of a step (`step()`; BackwardOverlap's first early update):
        bring the host counters up to date with captured replays, write the scheduled `lr`, and
        keep the device tables of a capturable optimizer current.  Idempotent within a step."""
        if self._captured is not None and not capturing:
            self._reconcile()
        if self._sched is not None:
            self._apply_schedule(self._step_count + 1)
        if self.capturable and self._use_native():
            self._ensure_dev(capturing)

    def _ensure_dev(self, capturing: bool = False) -> dict:
        """The device step state: `count` (int64, completed optimizer steps), `lr` (fp32
        [n_groups, L]) and per (b1, b2) the bias-correction table.  Uploaded outside capture only;
        a table a captured graph reads is updated in place or kept alive, never freed."""
        from .schedule import bias_correction_table, lr_table

        dev = self._dev
        b = self._sched
        # without a schedule the (one-column) table follows `group["lr"]`, which the caller may edit
        key = (b.schedule, tuple(b.base_lrs)) if b is not None else (None, tuple(g["lr"] for g in self.param_groups))
        if dev is not None and dev["lr_key"] == key:
            return dev
        if capturing:
            raise RuntimeError("capturable optimizer: the device lr / bias-correction tables must be uploaded "
                               "before capture - run an eager step first (utils.graphs.CapturedStep(warmup >= 1))")
        device = self._all_params()[0].device
        if dev is None:
            dev = self._dev = {"count": torch.full((1,), self._step_count, dtype=torch.int64, device=device),
                               "lr": None, "lr_key": None, "bc": {}, "retired": []}
            for g in self.param_groups:
                if "betas" in g and tuple(g["betas"]) not in dev["bc"]:
                    b1, b2 = g["betas"]
                    dev["bc"][(b1, b2)] = torch.from_numpy(bias_correction_table(b1, b2).copy()).to(device)
        tab = torch.from_numpy(lr_table(key[1], key[0]))
        if dev["lr"] is not None and dev["lr"].shape == tab.shape:
            dev["lr"].copy_(tab)
        else:
            if dev["lr"] is not None:
                dev["retired"].append(dev["lr"])
            dev["lr"] = tab.to(device)
        dev["lr_key"] = key
        return dev

    def _group_index(self, group) -> int:
        for i, g in enumerate(self.param_groups):
            if g is group:
                return i
        raise ValueError("param group does not belong to this optimizer")

    def _end_step(self, capturing: bool, steps_before) -> None:
        """After the last launch of `step()`.  `capturing`: the step was captured by a capturable
        optimizer.  It ran nothing: the host counters go back to what the device holds, and the
        replays are added by `_reconcile`."""
        if not capturing:
            self._step_count += 1
            return
        cap = self._captured if self._captured is not None else set()
        if steps_before is not None:
            for p, n in list(self._steps.items()):
                if n != steps_before.get(p, 0):
                    cap.add(p)
                    self._steps[p] = steps_before.get(p, 0)
        self._captured = cap

    def _reconcile(self) -> None:
        """Replays of a captured step advance only the device counter: read it back (8 bytes) and
        add the difference to `step_count` and to the steps of the parameters in the captured
        launches; `group["lr"]` becomes the last step's."""
        if self._dev is None or torch.cuda.is_current_stream_capturing():
            return
        n = int(self._dev["count"].item())
        d = n - self._step_count
        if d:
            self._step_count = n
            for p in self._captured:
                if p in self._steps:
                    self._steps[p] += d
        if self._sched is not None and n > 0:
            self._apply_schedule(n)

    # -- torch-compatible state dict -------------------------------------------------------
    def _materialize_steps(self) -> None:
        """Write the host step counters into the per-parameter `step` tensors torch keeps."""
        if self._captured is not None:
            self._reconcile()
        for p, n in self._steps.items():
            st = self.state.get(p)
            if st is not None:
                st["step"] = torch.tensor(float(n))

    def checkpoint_value(self, p, k, v):
        """The value a sharded checkpoint stores for state `k` of `p`: `v` itself, except a
        ZeRO-1 shard of a channels-last (ResNet conv) weight - its flat order is the storage
        order [O, KH, KW, I], not the torch shape's row-major order - which is consolidated
        into a full tensor (a sum of zero-filled shards: exact; collective over the group)."""
        from ..checkpoint.sharded import FlatShardedTensor

        if not isinstance(v, FlatShardedTensor):
            return v
        seg = self._space.segment_of(p)
        if not seg.channels_last:
            return v
        import torch.distributed as dist

        full = torch.zeros(seg.numel, dtype=v.dtype, device=self._space.device)
        for s0, t in v.local:
            full[s0:s0 + t.numel()].copy_(t)
        dist.all_reduce(full, group=self._space.zero.group)
        o, i, kh, kw = seg.shape
        return full.view(o, kh, kw, i).permute(0, 3, 1, 2)

    def consolidate_state(self) -> dict | None:
        """ZeRO-1: {state key: full flat buffer} all-gathered from every rank's compact shards
        (collective: call on every rank); None without ZeRO.  Only the torch-format
        `state_dict()` needs this - sharded checkpoints write the shards as they are."""
        sp = self._space
        if sp is None or sp.zero is None:
            return None
        full = {}
        for k, buf in self._bufs.items():
            f = torch.zeros(sp.numel, dtype=buf.dtype, device=buf.device)
            sp.zero.gather_compact(buf, f)
            full[k] = f
        return full

    def state_dict(self):
        """torch.optim format.  Under ZeRO-1 this is a collective that returns FULL state
        tensors (gathered copies); `checkpoint.state_dict.get_optimizer_state_dict` returns
        the sharded form instead."""
        full = self.consolidate_state()
        self._materialize_steps()
        sd = super().state_dict()
        if full is None:
            return sd
        # torch packs the live per-parameter dicts: replace the sharded values in copies
        ids = [i for g in sd["param_groups"] for i in g["params"]]
        state = {}
        for i, p in zip(ids, self._all_params()):
            st = sd["state"].get(i)
            if st is None:
                continue
            st = dict(st)
            seg = self._space.segment_of(p)
            for k in self._state_keys:
                if k in st:
                    st[k] = FlatParamSpace.view(full[k], seg)
            state[i] = st
        sd["state"] = state
        return sd

    def zero_grad(self, set_to_none: bool = True):
        from ..ops.gemm import flush_wgrads

        flush_wgrads()  # (a deferred weight gradient must not land after the reset)
        if self._space is not None and self._space.grad is not None:
            self._space.zero_grad(set_to_none=set_to_none)
        else:
            super().zero_grad(set_to_none=set_to_none)
            sp = space_of(self._all_params())
            if sp is not None and sp.accumulating:
                # the per-tensor CPU step over a space someone else built (a DDP wrap): the
                # accumulated step ends here too
                sp.zero_grad(set_to_none=set_to_none)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._steps = {}
        self._bound = set()
        for p in self._all_params():
            st = self.state.get(p)
            if st and "step" in st:
                self._steps[p] = int(float(st["step"]))
        if self._counts_steps:  # (also rewrites the device counter of a capturable optimizer)
            self.step_count = max(self._steps.values(), default=0)
        if self._space is not None:
            for p in self._all_params():
                st = self.state.get(p)
                if not st:
                    continue
                for k in self._state_keys:
                    if k in st and st[k] is not None:
                        self._adopt(p, k, st[k])
                        st[k] = self._state_value(p, k)

    @torch.no_grad()
    def step(self, closure=None):
        from ..ops.gemm import flush_wgrads

        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        flush_wgrads()  # weight gradients deferred into a grouped launch (normally flushed by backward's end)
        if self._flat_mode():
            capturing = self._use_native() and torch.cuda.is_current_stream_capturing()
            if capturing:
                self._check_capture()
            self._begin_step(capturing)
            # Only a capturable optimizer counts its replays (on the device, read back by
            # `_reconcile`).  Any other captured step - a constant-lr FusedSGD - counts like an
            # eager one: once, when it is captured.
            replayed = capturing and self.capturable
            before = dict(self._steps) if replayed else None
            self._flat_step()
            self._end_step(replayed, before)
            return loss
        self._begin_step()
        self._step_count += 1
        coef = self._plain_prelude()
        for group in self.param_groups:
            self._plain_update(group, self._with_grad(group), coef)
        return loss

    # What a subclass supplies: `_check_capture()` raises if its step must not be captured into a
    # hipGraph; `_plain_update(group, ps, coef)` is the per-tensor CPU step of one param group (`coef`:
    # the factor on every gradient, None: 1); `_native_launches` / `_cpu_launches(group, ps)` give the
    # flat step's [(params, decay_flags, fn(chunks, n[, clip]))].

    def _flat_step(self) -> None:
        """One step over the flat buffers: native chunk-table kernels on the GPU, the same
        chunk walk with torch ops on the CPU (ZeRO-1 reference path); then, under ZeRO-1, the
        parameter all-gather."""
        sp = self._ensure_space()
        have = sp.ensure_grad_views()
        self._have = None if len(have) == len(sp.params) else set(have)
        ov = self._overlap
        clip = self._clip_on()
        if clip and ov is not None:
            raise ValueError("max_grad_norm with BackwardOverlap: the updates that ran during backward cannot be "
                             "clipped (the global norm is known only after the whole backward)")
        done = ov.updated if ov is not None else ()
        native = self._use_native()
        launches = []
        for group in self.param_groups:
            ps = [p for p in self._with_grad(group) if p not in done]
            if ps:
                launches += self._native_launches(group, ps) if native else self._cpu_launches(group, ps)
        if clip:
            self._launch_clipped(sp, launches, native)
        else:
            self._launch_split(sp, launches)
        if ov is not None:
            ov.end_step()  # the compute stream waits for the updates that ran during backward
        if native and self.capturable:
            gpu_ext().optim_step_advance(self._dev["count"])  # behind every launch that read the counter
        sp.after_step()  # ZeRO-1: gather the updated shards
        bump_generation()  # masters / shadows changed in place: K-major weight images are stale

    @staticmethod
    def _rows(chunks, n):
        for start, lend, so in chunks[:n].tolist():
            yield start, lend & 0xFFFFFFFF, bool(lend >> 32), so

    @staticmethod
    def _tail_plan(sp, launches):
        """launches: [(params, decay_flags, fn)] -> (parts, waits): per launch `(tables, fn)` with
        one chunk table per entry of `waits` plus one.  Without a pending last-bucket all-reduce
        (DDP defer_tail_to_optimizer; `sp.pending_tail`, cleared here) that is the whole chunk
        table and no wait; with one, table 0 holds everything below the first in-flight piece and
        table i + 1 the piece that `waits[i]` makes the stream wait for."""
        tail, sp.pending_tail = sp.pending_tail, None
        if tail is None:
            return [((sp.chunk_table(ps, flags),), fn) for ps, flags, fn in launches], []
        starts = [off for off, _ in tail]
        return ([(sp.chunk_table_splits(ps, flags, starts), fn) for ps, flags, fn in launches],
                [wait for _, wait in tail])

    @staticmethod
    def _walk(parts, waits, wait: bool = True):
        """(chunks, n, fn) of every non-empty table, piece-major; before piece i + 1 its collective
        is waited for (also when nothing is launched), unless `wait` is off."""
        for i in range(len(waits) + 1):
            if i and wait:
                waits[i - 1]()
            for tables, fn in parts:
                chunks, n = tables[i]
                if n:
                    yield chunks, n, fn

    def _launch_split(self, sp, launches) -> None:
        """launches: [(params, decay_flags, fn(chunks, n))].  With a pending last-bucket
        all-reduce, update everything below its slice first, stream-wait for the collective,
        then the slice itself.

        Gradient clipping (`_launch_clipped`) gives up this tail/update overlap: every update
        needs the clip coefficient, which needs the whole gradient, so only the norm pass of the
        early part overlaps the tail's transfer."""
        for chunks, n, fn in self._walk(*self._tail_plan(sp, launches)):
            fn(chunks, n)

    # -- global gradient-norm clipping ---------------------------------------------------------
    def _clip_on(self) -> bool:
        m = self.max_grad_norm
        return m is not None and m > 0

    def _clip_buffers(self, device, need: int = 0, floor: int = 0, world: int = 1) -> dict:
        """The clip workspace, allocated once (never inside a launch, so a step stays
        capturable): `out` = {total_norm, coef}, `local` = this rank's sum of squares (ZeRO-1;
        the CPU paths' accumulator), `gather` = every rank's sum, `partial` = one sum per chunk
        (`floor`: the largest chunk count of the space; `need`: this step's).  `out` is fp32; the
        sums are fp64 on the GPU (what the kernels carry them in), fp32 on the CPU paths."""
        ws = self._clip_ws
        sums = torch.float64 if torch.device(device).type == "cuda" else torch.float32
        if ws is None:
            ws = self._clip_ws = {k: torch.zeros(n, dtype=dt, device=device)
                                  for k, n, dt in (("out", 2, torch.float32), ("local", 1, sums),
                                                   ("gather", world, sums), ("partial", 0, sums))}
        if ws["gather"].numel() != world:
            ws["gather"] = torch.zeros(world, dtype=sums, device=device)
        if ws["partial"].numel() < need:
            ws["partial"] = torch.zeros(max(need, floor), dtype=sums, device=device)
        if self.grad_norm is None:
            self.grad_norm = ws["out"][0]
        return ws

    @staticmethod
    def _write_clip(out, sumsq, scale: float, max_norm: float) -> float:
        """torch twin of the finalize kernel: out = {scale * sqrt(sumsq), min(1, max_norm / (norm + 1e-6))}
        in fp32 (torch.clamp keeps a NaN, like clip_grad_norm_); returns the coefficient."""
        total = sumsq.reshape(()).sqrt() * scale
        out[0] = total
        out[1] = torch.clamp(max_norm / (total + 1e-6), max=1.0)
        return float(out[1])

    def _launch_clipped(self, sp, launches, native: bool) -> None:
        """`_launch_split` with clipping: the per-chunk sums of squares of every launch's chunk
        table (each its own slice of the partials buffer, in launch order), the norm and the clip
        coefficient, then the updates with it.  With a pending DDP tail: the sums of everything
        below the first in-flight piece, then per piece wait + its sums, the norm, all updates."""
        parts, waits = self._tail_plan(sp, launches)
        ws = self._clip_buffers(sp.device, sum(n for tables, _ in parts for _, n in tables), sp.max_chunks(),
                                1 if sp.zero is None else sp.zero.world)
        pieces = self._walk(parts, waits)
        if native:
            clip = self._norm_native(sp, ws, self._sums_native(sp, ws, pieces))
        else:
            self._add_sumsq(ws, (sp.grad[start:start + ln] for chunks, n, _ in pieces
                                 for start, ln, _, _ in self._rows(chunks, n)))
            clip = self._norm_cpu(sp, ws)
        for chunks, n, fn in self._walk(parts, waits, wait=False):
            fn(chunks, n, clip)

    @staticmethod
    def _sums_native(sp, ws, pieces) -> int:
        """partial[k] = sum of squares of the k-th chunk, in fp64; returns the number of chunks."""
        ext, total = gpu_ext(), 0
        for chunks, n, _ in pieces:
            ext.gradnorm_partial(chunks, n, sp.grad, ws["partial"], total)
            total += n
        return total

    def _norm_native(self, sp, ws, total: int) -> int:
        """out = {norm, coef} from the per-chunk sums, on the device; the address the update
        kernels read the coefficient from."""
        ext, z, max_norm = gpu_ext(), sp.zero, float(self.max_grad_norm)
        ext.gradnorm_finalize(ws["partial"], total, sp.grad_scale, max_norm, ws["out"],
                              None if z is None else ws["local"])
        if z is not None:
            self._gather_sums(z, ws)
            ext.gradnorm_combine(ws["gather"], z.world, sp.grad_scale, max_norm, ws["out"])
        return ws["out"].data_ptr()

    @staticmethod
    def _add_sumsq(ws, grads) -> None:
        """CPU reference: local = sum over `grads` of sum(g * g), in fp32, added in the order given
        (the chunk tables' / the parameters')."""
        ws["local"].zero_()
        for g in grads:
            ws["local"] += (g * g).sum()

    def _norm_cpu(self, sp, ws) -> float:
        """`_norm_native` with torch ops; returns the coefficient as a host float."""
        z = sp.zero
        s = ws["local"][0]
        if z is not None:
            self._gather_sums(z, ws)
            s = ws["gather"][0]
            for r in range(1, z.world):
                s = s + ws["gather"][r]
        return self._write_clip(ws["out"], s, sp.grad_scale, float(self.max_grad_norm))

    @staticmethod
    def _gather_sums(z, ws) -> None:
        """ZeRO-1: every rank's local sum -> `gather` on every rank."""
        import torch.distributed as dist

        # all-gather (not all-reduce) + a rank-order sum: the same bits on every rank
        dist.all_gather_into_tensor(ws["gather"], ws["local"], group=z.group)

    def _plain_clip(self):
        """Clip coefficient of the per-tensor CPU step (None: clipping off): the same
        semantics with torch ops - per-tensor sum(g * g) in fp32, added in parameter order."""
        if not self._clip_on():
            return None
        ps = [p for group in self.param_groups for p in self._with_grad(group)]
        dev = ps[0].device if ps else self._all_params()[0].device
        ws = self._clip_buffers(dev)
        self._add_sumsq(ws, (p.grad.float() for p in ps))
        sp = space_of(self._all_params())
        return self._write_clip(ws["out"], ws["local"][0], 1.0 if sp is None else sp.grad_scale,
                                float(self.max_grad_norm))

    def _plain_prelude(self):
        """Start of the per-tensor CPU step: wait for a deferred collective, bring an
        accumulated step's gradients into their slices (FlatParamSpace.ensure_grad_views: the
        add fold-back, and the views of parameters only an earlier micro-batch touched), and
        return the factor on every gradient (clip coefficient x the space's grad_scale; None: 1)."""
        sp = space_of(self._all_params())
        gs = 1.0
        if sp is not None:
            sp.wait_pending_tail()
            if sp.accumulating:
                sp.ensure_grad_views()
            gs = sp.grad_scale
        coef = self._plain_clip()
        if coef is None:
            return None if gs == 1.0 else gs
        return coef * gs

    def _use_native(self):
        ps = self._all_params()
        return bool(ps) and ps[0].is_cuda

    def _with_grad(self, group) -> list:
        have = self._have
        if have is None:
            return [p for p in group["params"] if p.grad is not None]
        return [p for p in group["params"] if p in have]

    @property
    def flat_space(self):
        return self._space


class FusedAdamW(_FlatOptimizer):
    _state_keys = ("exp_avg", "exp_avg_sq")
    _counts_steps = True

    def _init_extra(self, p, st) -> None:
        self._steps.setdefault(p, 0)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False,
                 maximize=False, max_grad_norm=None, state_dtype=torch.float32, rounding_seed=0,
                 lr_schedule=None, capturable=False):
        """`max_grad_norm`: clip the global gradient norm inside the step (None / 0: off; settable
        later as `opt.max_grad_norm`).  `opt.grad_norm` then holds the pre-clip norm of the last
        step.  `p.grad` is left unscaled - the one visible difference from
        `torch.nn.utils.clip_grad_norm_`, which rewrites the gradients.

        `state_dtype`: torch.float32 (default) or torch.bfloat16.  With bfloat16, `exp_avg` and
        `exp_avg_sq` are STORED in bf16 (half the state memory and checkpoint bytes, 22 instead of
        30 B moved per parameter and step) and rounded stochastically - round-to-nearest would
        freeze `exp_avg_sq` at beta2 = 0.999.  The update of a step uses the fp32 moments before
        rounding.  The random bits are Philox4x32-10 of (`rounding_seed`, the parameter's step
        number, the element's offset in the flat parameter space): no RNG state exists, runs and
        resumes are bit-identical, and the bits do not depend on how the chunk tables are cut.
        They do depend on the flat layout, so a replicated and a ZeRO-1 run (whose buckets are
        padded) are not promised equal bits.  Both are attributes, not param-group options:
        `state_dict()` keeps torch's keys; a checkpoint resumes into the same `state_dtype`.

        `lr_schedule`: an `optim.schedule.LRSchedule` (settable later as `opt.lr_schedule`): the
        n-th step runs with `group["lr"] = base_lr * f(n - 1)`, written at the start of `step()` -
        bit for bit a run whose caller set `group["lr"]` by hand.  The base rates are the groups'
        `lr` when the schedule is attached; nothing is added to `param_groups` or the state.

        `capturable=True` (GPU; the CPU accepts it and runs the host path): the kernels read lr,
        `1 - b1**t`, `sqrt(1 - b2**t)` and the step number from device tables indexed by a device
        step counter instead of host scalars (optim/schedule.py builds the tables from the same
        doubles, so the results are the same bits), and the step may be captured into a hipGraph
        (`utils.graphs.CapturedStep`) with the schedule and the bias corrections advancing on every
        replay.  Replays advance only the device counter; `state_dict()`, `load_state_dict()` and the
        next eager step read it back (8 bytes) and bring `step_count`, the per-parameter steps and
        `group["lr"]` up to date.  Betas whose bias corrections need more than 2^22 table rows to
        reach 1.0f raise ValueError."""
        if amsgrad or maximize:
            raise NotImplementedError("amsgrad/maximize are not supported by the fused kernel")
        if state_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"FusedAdamW state_dtype must be torch.float32 or torch.bfloat16, got {state_dtype!r}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False,
                                      maximize=False, foreach=None, capturable=False, differentiable=False,
                                      fused=None), max_grad_norm, lr_schedule, capturable)
        if capturable:  # (host tables, cached per betas: refuses betas that need too many rows)
            from .schedule import bias_correction_table

            for g in self.param_groups:
                bias_correction_table(*g["betas"])
        self.state_dtype = state_dtype
        self.rounding_seed = int(rounding_seed) & ((1 << 64) - 1)

    def _native_launches(self, group, ps) -> list:
        """[(params, decay_flags, fn(chunks, n))] of one param group's native update of `ps`
        (advances their step counters)."""
        sp, ext = self._space, gpu_ext()
        for p in ps:
            self._bind_state(p)
        b1, b2 = group["betas"]
        wd = group["weight_decay"]
        cap = self.capturable
        if cap:
            # device path: lr = table[group][count], bias corrections = row t, t = count + 1 + off
            dev, gi = self._dev, self._group_index(group)
            bc = dev["bc"].get((b1, b2))
            if bc is None:
                raise RuntimeError(f"capturable FusedAdamW: betas {(b1, b2)} changed after construction")
            now = self._step_count + 1  # the optimizer step these launches belong to
        out = []
        for step, sub in self._count(ps).items():
            def fn(chunks, n, clip=0, step=step):
                bufs = (chunks, n, sp.data, sp.grad, self._bufs["exp_avg"], self._bufs["exp_avg_sq"], sp.shadow)
                if cap:
                    ext.adamw_dev(*bufs, dev["count"], dev["lr"], gi, bc, step - now, b1, b2, group["eps"], wd,
                                  sp.grad_scale, sp.skip_ptr, clip, self.rounding_seed)
                else:
                    ext.adamw(*bufs, group["lr"], b1, b2, group["eps"], wd, 1 - b1 ** step,
                              math.sqrt(1 - b2 ** step), sp.grad_scale, sp.skip_ptr, clip, self.rounding_seed, step)

            out.append((sub, [wd != 0.0] * len(sub), fn))
        return out

    @staticmethod
    def _torch_update(p, g, m, v, step: int, lr, b1, b2, eps, wd, decay: bool) -> None:
        """torch.optim.AdamW's update of one tensor - a whole parameter or a slice of the flat
        buffers - in place; `g` is the gradient with every factor applied."""
        if decay:
            p.mul_(1 - lr * wd)
        m.lerp_(g, 1 - b1)
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
        denom = (v.sqrt() / math.sqrt(1 - b2 ** step)).add_(eps)
        p.addcdiv_(m, denom, value=-lr / (1 - b1 ** step))

    def _cpu_launches(self, group, ps) -> list:
        """CPU twin of `_native_launches` (ZeRO-1 on gloo): the per-tensor reference math of
        `_torch_update`, applied chunk by chunk to the owned flat slices and the compact state.  With
        bf16 state the parameter update is that same math on the widened moments (so step 1 equals the
        fp32-state optimizer bit for bit), while the moments that are rounded and stored are
        computed with the kernel's own operation order: a few fp32 ulps from the former, and the
        same bits as the GPU keeps."""
        sp = self._space
        for p in ps:
            self._bind_state(p)
        b1, b2 = group["betas"]
        wd, lr, eps = group["weight_decay"], group["lr"], group["eps"]
        m_all, v_all = self._bufs["exp_avg"], self._bufs["exp_avg_sq"]
        bf16_state = m_all.dtype == torch.bfloat16
        if bf16_state:  # the kernel's fp32 coefficients: (float)b and 1.f - (float)b
            f32 = torch.float32
            b1f, b2f = torch.tensor(b1, dtype=f32), torch.tensor(b2, dtype=f32)
            c1f, c2f = 1 - b1f, 1 - b2f
        out = []
        for step, sub in self._count(ps).items():
            def fn(chunks, n, clip=None, step=step):
                gs = sp.grad_scale if clip is None else sp.grad_scale * clip
                if bf16_state:  # (the kernel multiplies grad_scale and the coefficient in fp32)
                    gsf = torch.tensor(sp.grad_scale, dtype=f32)
                    if clip is not None:
                        gsf = gsf * torch.tensor(clip, dtype=f32)
                for start, ln, decay, so in self._rows(chunks, n):
                    p = sp.data[start:start + ln]
                    g = sp.grad[start:start + ln]
                    ms, vs = m_all[so:so + ln], v_all[so:so + ln]
                    # bf16 state: widen, do the fp32 math, update p from the unrounded moments
                    m, v = (ms.float(), vs.float()) if bf16_state else (ms, vs)
                    if bf16_state:
                        # What is STORED repeats adamw_bf16state_kernel's operations bit for bit, so the
                        # two paths keep the same state (one bf16 ulp of difference in a stored moment
                        # would move the next update by lr * 2^-7): gr = g * gs; m = fma(1 - b1, gr, b1 * m);
                        # v = fma(b2, v, ((1 - b2) * gr) * gr), every product and constant in fp32.  A
                        # product of two fp32 values is exact in fp64, so fp64 multiply-add + one rounding
                        # to fp32 is the fused operation (but for a double rounding, ~2^-29 of the cases).
                        gr = g * gsf
                        m_st = (c1f.double() * gr.double() + (b1f * m).double()).float()
                        v_st = (b2f.double() * v.double() + ((c2f * gr) * gr).double()).float()
                    if gs != 1.0:
                        g = g * gs
                    self._torch_update(p, g, m, v, step, lr, b1, b2, eps, wd, decay)
                    if bf16_state:  # the kernel's rounding: bits keyed by (seed, step, flat index)
                        w = sr_words(self.rounding_seed, step, start, ln)
                        ms.copy_(sr_bf16(m_st, w & 0xFFFF))
                        vs.copy_(sr_bf16(v_st, w >> 16))

            out.append((sub, [wd != 0.0] * len(sub), fn))
        return out

    def _count(self, ps) -> dict:
        """Advance the step counter of every parameter in `ps`; {step: [params]}."""
        steps = self._steps
        by = {}
        for p in ps:
            n = steps.get(p, 0) + 1
            steps[p] = n
            by.setdefault(n, []).append(p)
        return by

    def _check_capture(self) -> None:
        if not self.capturable:
            raise RuntimeError("FusedAdamW computes bias corrections on the host per step: not graph-capturable "
                               "(construct it with capturable=True, use eager steps, or FusedSGD inside "
                               "utils.graphs.CapturedStep)")

    def _plain_update(self, group, ps, coef) -> None:
        b1, b2 = group["betas"]
        for step, sub in self._count(ps).items():
            for p in sub:
                st = self.state[p]
                if "exp_avg" not in st:
                    st["exp_avg"] = torch.zeros_like(p)
                    st["exp_avg_sq"] = torch.zeros_like(p)
                g = p.grad if coef is None else p.grad * coef
                # (decays unconditionally: with weight_decay = 0 a multiply by 1.0)
                self._torch_update(p, g, st["exp_avg"], st["exp_avg_sq"], step, group["lr"], b1, b2, group["eps"],
                                   group["weight_decay"], True)


class FusedSGD(_FlatOptimizer):
    _state_keys = ("momentum_buffer",)

    def init_state(self) -> None:
        if all(g["momentum"] != 0.0 for g in self.param_groups):
            super().init_state()

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False,
                 maximize=False, max_grad_norm=None, lr_schedule=None, capturable=False):
        """`max_grad_norm`: as in `FusedAdamW` (clipping inside the step, `p.grad` left unscaled);
        a clipped FusedSGD step stays capturable in `utils.graphs.CapturedStep`.  `lr_schedule`,
        `capturable`: as in `FusedAdamW`.  A constant-lr step captures either way; with a
        non-constant schedule only `capturable=True` does (a host `lr` would freeze in the graph).
        SGD's state has no step number: after `load_state_dict` set `opt.step_count` yourself."""
        if maximize:
            raise NotImplementedError("maximize is not supported by the fused kernel")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=nesterov, maximize=False, foreach=None, differentiable=False,
                                      fused=None), max_grad_norm, lr_schedule, capturable)

    def _first_parts(self, group, ps) -> list:
        """[(params, first)]: torch's first momentum step is `buf = d` (a clone), so parameters
        without a buffer yet form their own launch with first=True (and get their buffer here)."""
        if group["momentum"] == 0.0:
            return [(ps, False)]
        fresh = [p for p in ps if "momentum_buffer" not in self.state[p]]
        if not fresh:
            return [(ps, False)]
        old = [p for p in ps if "momentum_buffer" in self.state[p]]
        for p in fresh:
            self._bind_state(p)
        return [(fresh, True)] + ([(old, False)] if old else [])

    def _native_launches(self, group, ps) -> list:
        sp, ext = self._space, gpu_ext()
        mom = group["momentum"]
        wd = group["weight_decay"]
        cap = self.capturable
        if cap:  # device path: lr = table[group][count]
            dev, gi = self._dev, self._group_index(group)
        out = []
        for sub, first in self._first_parts(group, ps):
            def fn(chunks, n, clip=0, first=first):
                bufs = (chunks, n, sp.data, sp.grad, self._bufs["momentum_buffer"] if mom != 0.0 else None, sp.shadow)
                rest = (mom, group["dampening"], wd, group["nesterov"], first, sp.grad_scale, sp.skip_ptr, clip)
                if cap:
                    ext.sgd_dev(*bufs, dev["count"], dev["lr"], gi, *rest)
                else:
                    ext.sgd(*bufs, group["lr"], *rest)

            out.append((sub, [wd != 0.0] * len(sub), fn))
        return out

    @staticmethod
    def _torch_update(p, d, buf, first: bool, lr, mom, damp, wd, nest):
        """torch.optim.SGD's update of one tensor - a whole parameter or a slice of the flat
        buffers - in place; `d` is the gradient with every factor applied.  `buf`: the momentum
        buffer (None: torch's first step clones one; `first`: an existing one takes `d`).  Returns
        the buffer."""
        if wd != 0:
            d = d.add(p, alpha=wd)
        if mom != 0:
            if buf is None:
                buf = torch.clone(d).detach()
            elif first:
                buf.copy_(d)
            else:
                buf.mul_(mom).add_(d, alpha=1 - damp)
            d = d.add(buf, alpha=mom) if nest else buf
        p.add_(d, alpha=-lr)
        return buf

    def _cpu_launches(self, group, ps) -> list:
        """CPU twin of `_native_launches` (ZeRO-1 on gloo), torch.optim.SGD's math per chunk."""
        sp = self._space
        mom, wd, lr, damp, nest = (group["momentum"], group["weight_decay"], group["lr"], group["dampening"],
                                   group["nesterov"])
        parts = self._first_parts(group, ps)
        buf_all = self._bufs.get("momentum_buffer")
        out = []
        for sub, first in parts:
            def fn(chunks, n, clip=None, first=first):
                gs = sp.grad_scale if clip is None else sp.grad_scale * clip
                for start, ln, decay, so in self._rows(chunks, n):
                    d = sp.grad[start:start + ln]
                    if gs != 1.0:
                        d = d * gs
                    self._torch_update(sp.data[start:start + ln], d, buf_all[so:so + ln] if mom != 0 else None, first,
                                       lr, mom, damp, wd if decay else 0, nest)

            out.append((sub, [wd != 0.0] * len(sub), fn))
        return out

    def _check_capture(self) -> None:
        if not self.capturable and self._sched is not None and not self._sched.schedule.is_constant:
            raise RuntimeError("FusedSGD with a learning-rate schedule: a captured step would freeze lr "
                               "(construct it with capturable=True)")

    def _plain_update(self, group, ps, coef) -> None:
        mom = group["momentum"]
        for p in ps:
            d = p.grad if coef is None else p.grad * coef
            buf = self._torch_update(p, d, self.state[p].get("momentum_buffer") if mom != 0 else None, False,
                                     group["lr"], mom, group["dampening"], group["weight_decay"], group["nesterov"])
            if mom != 0:
                self.state[p]["momentum_buffer"] = buf
