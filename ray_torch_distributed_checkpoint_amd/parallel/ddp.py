"""Data-parallel wrapper: bucketed gradient all-reduce over RCCL (xGMI) overlapped with backward.

What the reference gets from `ray.train.torch.prepare_model` -> torch DDP
(R/my_ray_module.py:135; torch/nn/parallel/distributed.py, c10d reducer.hpp), re-designed for
MI355X:

* Gradients live in ONE flat fp32 buffer (FlatParamSpace) laid out in reverse registration
  order (~ backward order).  A bucket is a contiguous slice of it, so the all-reduce runs in
  place on the gradients: no copy-in, no copy-out, no per-bucket flatten (reducer.hpp:329,499).
* Bucket plan is static: a small first bucket (so the first collective starts early in
  backward, reducer.hpp:30-31) then `bucket_cap_mb` buckets.  The default cap (32 MiB) is
  sized for RCCL on 8 fully-connected MI355X: a ring all-reduce of a B-byte bucket moves
  2*(7/8)*B per GPU split over RCCL's channels (one per xGMI link), so 32 MiB gives each of
  7 links >= 4 MiB per step - past the per-message latency knee - while keeping ~15 buckets
  of overlap for GPT-2-small.
* Collectives are launched strictly in bucket order (identical on every rank) from the
  autograd post-accumulate hooks; RCCL runs them on its own stream, overlapped with the rest
  of backward; the end-of-backward callback only makes the compute stream wait.
* Averaging is folded into the collective (ReduceOp.AVG on RCCL - no divide kernel); gloo
  (CPU tests) uses SUM + one in-place scale of the flat buffer.
* `grad_comm_dtype="bf16"` halves the bytes on xGMI: each ready bucket is rounded into a bf16
  twin of the flat gradient buffer on the compute stream, all-reduced in bf16, and widened back
  into the fp32 master gradients on a side stream as soon as its collective lands (the
  compute stream waits for that stream once, at the end of backward).  `bucket_cap_mb` counts
  communicated bytes, like torch DDP's bucket_cap_mb counts bytes of the gradient dtype.
* With `defer_tail_to_optimizer`, backward returns with the LAST bucket's all-reduce still in
  flight (on RCCL): the fused optimizer steps every other parameter first and stream-waits for
  it only before the last slice, hiding the step's exposed collective tail (GPT-2: the tied
  154 MB token table, whose gradient completes at the very end of backward).  That bucket is
  issued as collectives of <= `tail_piece_mb` (32 MB: >= 4 MB per xGMI link at 8 ranks), and
  the optimizer waits for and updates them piece by piece, so only the first piece's transfer
  and the last piece's update stay exposed.
* `zero_stage=1` (ZeRO-1) shards the optimizer work: every bucket is padded to a multiple of
  64 x world elements and REDUCE-SCATTERED in place (rank r receives the averaged shard r), the
  fused optimizer updates only this rank's shards (1/world of the AdamW traffic - 40 of 150 ms
  per Llama-3-8B step on one GPU) and keeps optimizer state for them alone (compact buffers:
  1/world of the exp_avg/exp_avg_sq bytes), and the updated fp32 shards are all-gathered back
  after the step (same bytes on xGMI as the all-reduce).  Sharded checkpoints write each
  rank's state shards as DCP chunks of the torch-shaped state tensors - no consolidation
  (checkpoint/sharded.py).  `p.grad` is reduced only on the owned shards, so only
  FusedAdamW / FusedSGD may step a ZeRO-1 model (checked at the first backward).
* Parameters and buffers are broadcast from rank 0 once at construction as ONE flat tensor;
  module buffers (BatchNorm running stats) are broadcast before each forward when
  `broadcast_buffers` (distributed.py:1557-1558 semantics) as one coalesced flat tensor.
"""
from __future__ import annotations

import contextlib
import os

import torch
import torch.distributed as dist
import torch.nn as nn

from ..ops.gemm import flush_wgrads, when_grad_ready
from ..optim.flat import FlatParamSpace


class _Bucket:
    __slots__ = ("index", "start", "end", "params", "pending", "work", "launched")

    def __init__(self, index, start, end, params):
        self.index, self.start, self.end, self.params = index, start, end, params
        self.pending = len(params)
        self.work = None
        self.launched = False


class DistributedDataParallel(nn.Module):
    def __init__(self, module: nn.Module, process_group=None, bucket_cap_mb: float = 32.0,
                 first_bucket_mb: float = 2.0, broadcast_buffers: bool = True, device_ids=None,
                 output_device=None, find_unused_parameters: bool = False, gradient_as_bucket_view: bool = True,
                 defer_tail_to_optimizer: bool = False, grad_comm_dtype: str = "fp32", p2p_max_kb: float = 0.0,
                 zero_stage: int = 0, p2p_timeout_s: float = 30.0, force_collectives: bool = False,
                 tail_piece_mb: float = 32.0):
        super().__init__()
        if grad_comm_dtype not in ("fp32", "bf16"):
            raise ValueError("grad_comm_dtype must be 'fp32' or 'bf16'")
        if zero_stage not in (0, 1):
            raise ValueError("zero_stage must be 0 (replicated optimizer) or 1 (sharded optimizer state)")
        self.grad_comm_dtype = grad_comm_dtype
        self.bucket_cap_mb = bucket_cap_mb
        self.module = module
        # the last bucket's all-reduce stays in flight after backward; the fused optimizer
        # updates every other parameter first and waits for it only before the last bucket's
        # slice (FlatParamSpace.pending_tail) - overlaps the step's exposed collective tail
        self.defer_tail = defer_tail_to_optimizer
        self.process_group = process_group
        self.world_size = dist.get_world_size(process_group) if dist.is_initialized() else 1
        # force_collectives: run the whole communication path (native engine, RCCL all-reduce
        # of every bucket, buffer broadcasts) even in a 1-rank group - a one-GPU rehearsal of the
        # multi-GPU code path against the real backend (an all-reduce over one rank is the identity)
        self._collective = self.world_size > 1 or (force_collectives and dist.is_initialized())
        self.broadcast_buffers = broadcast_buffers
        params = [p for p in module.parameters() if p.requires_grad]
        self.zero = zero_stage == 1 and self.world_size > 1
        if self.zero:
            self.defer_tail = False  # the optimizer needs every owned shard reduced first
        esz = 2 if grad_comm_dtype == "bf16" else 4
        cap = int(bucket_cap_mb * (1 << 20) / esz)
        first_cap = int(first_bucket_mb * (1 << 20) / esz)
        existing = getattr(params[0], "_rtdc_space", None) if params else None
        groups = None
        if existing is not None and all(getattr(p, "_rtdc_space", None) is existing for p in params):
            if self.zero:
                raise ValueError("DistributedDataParallel(zero_stage=1) lays out the flat parameter space itself: "
                                 "wrap the model before the optimizer takes its first step")
            self.space = existing
        else:
            order = list(reversed(params))
            align = None
            if self.zero:
                # bucket plan first; each bucket then ends on a multiple of 64 x world elements
                # so it splits into `world` equal, aligned ZeRO shards
                groups = self._plan([p.numel() for p in order], first_cap, cap)
                align = {g[-1]: 64 * self.world_size for g in groups}
            self.space = FlatParamSpace(order, align_after=align)
        dev = self.space.device
        backend = dist.get_backend(process_group) if dist.is_initialized() else "gloo"
        # RCCL averages inside the collective (ReduceOp.AVG = PreMulSum).  On a 1-rank group
        # (force_collectives rehearsal) the average is the identity, but RCCL still runs its
        # oneRankReduce<PreMulSum> pass over every bucket (measured 0.87 ms per GPT-2 step in
        # bf16, profiles/comm_bf16_1rank_r4.txt): SUM there, which RCCL treats as in-place no-op.
        self._use_avg = backend == "nccl" and self.world_size > 1
        # one flat broadcast of all parameters from rank 0
        if self._collective:
            dist.broadcast(self.space.data, src=0, group=process_group)
            self.space.refresh_shadows()
        self._bufspace = None
        bufs = [b for b in module.buffers() if b is not None and b.numel() > 0 and b.dtype.is_floating_point]
        if bufs:
            n = sum(b.numel() for b in bufs)
            flat = torch.empty(n, dtype=torch.float32, device=dev)
            off = 0
            views = []
            with torch.no_grad():
                for b in bufs:
                    v = flat[off:off + b.numel()]
                    v.copy_(b.reshape(-1).float())
                    views.append(v)
                    off += b.numel()
            if all(b.dtype == torch.float32 for b in bufs):
                for b, v in zip(bufs, views):
                    b.data = v.view(b.shape)
                self._bufspace = (flat, None)
            else:
                self._bufspace = (flat, list(zip(bufs, views)))
            if self._collective:
                self._sync_buffers()
        # static bucket plan over the flat gradient buffer (caps in communicated bytes)
        self.buckets: list[_Bucket] = []
        sp = self.space
        if groups is None:
            groups = self._plan([s.numel for s in sp.segments], first_cap, cap)
        for k, g in enumerate(groups):
            start = sp.segments[g[0]].offset
            last = sp.segments[g[-1]]
            end = sp.segments[groups[k + 1][0]].offset if self.zero and k + 1 < len(groups) else \
                (sp.numel if self.zero else last.offset + (last.numel + 63) // 64 * 64)
            self.buckets.append(_Bucket(k, start, end, [sp.params[i] for i in g]))
        if self.zero:
            from ..optim.flat import ZeroLayout

            sp.set_zero(ZeroLayout([(b.start, b.end) for b in self.buckets], dist.get_rank(process_group),
                                   self.world_size, process_group))
        self._bucket_of = {}
        for b in self.buckets:
            for p in b.params:
                self._bucket_of[id(p)] = b
        self._next = 0
        self._require_sync = True
        self._callback_queued = False
        self._hooks = []
        self._pidx = {id(p): i for i, p in enumerate(self.space.params)}
        self._engine = None
        self._check = os.environ.get("RTDC_COLLECTIVE_CHECK", "0") == "1"
        self._steps = 0
        self._zero_checked = False
        self._p2p_timeout_s = float(p2p_timeout_s)
        self._comm = None
        self.p2p = None
        self.p2p_max_bytes = 0
        if self._collective and grad_comm_dtype == "bf16":
            self._comm = torch.empty(self.space.numel, dtype=torch.bfloat16, device=dev)
        if self._collective:
            self._engine = self._native_engine(process_group)
            # the deferred last bucket (GPT-2: the 154 MB tied token table) as collectives of
            # <= tail_piece_mb communicated bytes: the optimizer updates piece i while pieces
            # i+1.. are still on the wire (see FlatParamSpace.pending_tail)
            tail_max = int(tail_piece_mb * (1 << 20) / esz) \
                if self._engine is not None and self.defer_tail and tail_piece_mb > 0 else 0
            # everything that shapes the sequence of collectives must agree before the first one
            self._verify_plan_across_ranks(tail_max, p2p_max_kb)
            if tail_max:
                self._engine.set_tail_split(tail_max)
            self._attach_p2p(process_group, p2p_max_kb)
            for p in self.space.params:
                self._hooks.append(p.register_post_accumulate_grad_hook(self._on_grad_ready))

    @staticmethod
    def _plan(numels, first_cap: int, cap: int) -> list:
        """Bucket plan in layout order: lists of parameter indices; the first bucket holds at
        most first_cap elements (so its collective starts early in backward), the others cap
        (a parameter's extent counts its 64-element alignment padding from the next one on)."""
        groups, cur, cur_size = [], [], 0
        sizes = []
        for i, n in enumerate(numels):
            limit = first_cap if not groups else cap
            if cur and cur_size + n > limit:
                groups.append(cur)
                sizes.append(cur_size)
                cur, cur_size = [], 0
            cur.append(i)
            cur_size += (n + 63) // 64 * 64
        if cur:
            groups.append(cur)
            sizes.append(cur_size)
        # a degenerate first bucket (GPT-2: only ln_f, 6 KB, because the next parameter alone
        # exceeds first_cap) is a latency-only collective: fold it into the second bucket
        if len(groups) > 1 and sizes[0] < min(first_cap, cap) // 4:
            groups = [groups[0] + groups[1]] + groups[2:]
        return groups

    def _agree(self, value: int, what: str) -> None:
        """All ranks must hold the same integer (MIN == MAX all-reduce); raise otherwise."""
        t = torch.tensor([value, -value], dtype=torch.int64, device=self.space.device)
        dist.all_reduce(t, op=dist.ReduceOp.MIN, group=self.process_group)
        if int(t[0].item()) != -int(t[1].item()):
            raise RuntimeError(f"DDP {what} differs across ranks (rank {dist.get_rank(self.process_group)} has "
                               f"{value}): collectives would deadlock or mix unrelated buffers")

    def _verify_plan_across_ranks(self, tail_max: int = 0, p2p_max_kb: float = 0.0) -> None:
        """Parameter shapes + bucket plan fingerprint identical on every rank (the role of torch
        DDP's _verify_param_shape_across_processes) - including every knob that
        changes the number or sizes of the collectives: the deferred tail's piece split, the
        communicated dtype, ZeRO, the engine and the P2P threshold.  Ranks that disagree on any
        of them would issue different collective sequences (hang, or sums over mismatched
        ranges); this raises before the first one instead."""
        import zlib

        desc = ";".join(f"{tuple(s.shape)}@{s.offset}" for s in self.space.segments)
        desc += "|" + ",".join(f"{b.start}-{b.end}" for b in self.buckets)
        desc += (f"|tail={tail_max}|defer={int(bool(self.defer_tail))}|comm={self.grad_comm_dtype}"
                 f"|zero={int(self.zero)}|engine={'native' if self._engine is not None else 'python'}"
                 f"|p2p={float(p2p_max_kb)}")
        self._agree(zlib.crc32(desc.encode()) & 0x7FFFFFFF, "parameter/bucket plan")

    def _native_engine(self, process_group):
        """C++ bucket engine (csrc/runtime/reducer.cpp); RTDC_DDP_ENGINE=python keeps the
        Python reference implementation of the same protocol."""
        if os.environ.get("RTDC_DDP_ENGINE", "native") == "python":
            if self.zero:
                raise ValueError("zero_stage=1 needs the native bucket engine (RTDC_DDP_ENGINE=native)")
            return None
        from ..ops._ext import ext

        mod = ext()
        if mod is None or not hasattr(mod, "GradBucketEngine"):
            if self.zero:
                raise RuntimeError("zero_stage=1 needs the native bucket engine (extension not built)")
            return None
        for a, b in zip(self.buckets, self.buckets[1:]):
            assert a.end == b.start, "buckets must tile the flat gradient buffer"
        bounds = [b.start for b in self.buckets] + [self.buckets[-1].end]
        param_bucket = [self._bucket_of[id(p)].index for p in self.space.params]
        segs = [(s.offset, s.numel) for s in self.space.segments]
        pg = process_group if process_group is not None else dist.distributed_c10d._get_default_group()
        return mod.GradBucketEngine(self.space.grad, bounds, param_bucket, segs, pg, self._use_avg,
                                    1.0 / self.world_size, self._comm,
                                    self.world_size if self.zero else 0, dist.get_rank(process_group))

    def _attach_p2p(self, process_group, max_kb: float) -> None:
        """Buckets of at most max_kb KiB (communicated bytes) go through the one-shot hipIpc
        all-reduce (parallel/p2p.py) instead of RCCL: latency-bound small buckets (the toy MLP's
        1-2 MB, every model's small first bucket) take one xGMI hop to all peers at once.
        Opt-in (0 = off); needs the native engine, device gradients and <= 8 ranks."""
        self.p2p = None
        self.p2p_max_bytes = 0
        # a re-wrap reuses the flat space: never keep a previous communicator's error word
        # (freed with it, or set by its timeout) as this wrap's optimizer skip flag
        self.space.skip_ptr = 0
        if max_kb <= 0 or self._engine is None or self.space.device.type != "cuda" or self.world_size > 8 \
                or self.zero:
            return
        from .p2p import P2PAllReduce

        esz = 2 if self.grad_comm_dtype == "bf16" else 4
        small = [(b.end - b.start) * esz for b in self.buckets if (b.end - b.start) * esz <= max_kb * 1024]
        if not small:
            return
        cap_mb = max(small) / (1 << 20) + 0.01
        self.p2p = P2PAllReduce(process_group, capacity_mb=cap_mb, device=self.space.device,
                                timeout_s=self._p2p_timeout_s)
        self.p2p_max_bytes = int(max_kb * 1024)
        self._engine.set_p2p(self.p2p.comm, self.p2p_max_bytes)
        # a timed-out bucket is NaN-filled on the device: the fused optimizer kernels read the
        # error word and skip the update, so no NaN ever reaches a parameter (parallel/health.py)
        self.space.skip_ptr = self.p2p.error_ptr()

    def comm_plan(self) -> dict:
        """Self-description of the gradient all-reduce (what a multi-GPU bench reports)."""
        sizes = self.bucket_sizes_bytes()
        return {"world_size": self.world_size, "grad_comm_dtype": self.grad_comm_dtype,
                "bucket_cap_mb": self.bucket_cap_mb, "buckets": len(sizes),
                "bucket_mb": [round(b / (1 << 20), 2) for b in sizes],
                "allreduce_bytes_per_step": int(sum(sizes)),
                "engine": "native" if self._engine is not None else "python",
                "defer_tail_to_optimizer": self.defer_tail,
                "zero_stage": 1 if self.zero else 0,
                "p2p_buckets": ([i for i, v in enumerate(self._engine.p2p_buckets()) if v]
                                if getattr(self, "p2p", None) is not None else [])}

    # ------------------------------------------------------------------ buffers
    def _sync_buffers(self):
        flat, pairs = self._bufspace
        if pairs is not None:
            with torch.no_grad():
                for b, v in pairs:
                    v.copy_(b.reshape(-1).float())
        dist.broadcast(flat, src=0, group=self.process_group)
        if pairs is not None:
            with torch.no_grad():
                for b, v in pairs:
                    b.copy_(v.view(b.shape).to(b.dtype))

    # ------------------------------------------------------------------ forward
    def wait_tail(self) -> None:
        """Stream-order a deferred last-bucket all-reduce (no-op when none is pending)."""
        self.space.wait_pending_tail()

    def forward(self, *args, **kwargs):
        self.space.wait_pending_tail()
        if self._collective and self.broadcast_buffers and self._bufspace is not None and self.training:
            self._sync_buffers()
        return self.module(*args, **kwargs)

    @contextlib.contextmanager
    def no_sync(self):
        old = self._require_sync
        self._require_sync = False
        try:
            yield
        finally:
            self._require_sync = old

    # ------------------------------------------------------------------ reducer
    def _on_grad_ready(self, p):
        if not self._require_sync:
            return
        if not self._callback_queued:
            self._callback_queued = True
            torch.autograd.Variable._execution_engine.queue_callback(self._finalize)
        # a weight gradient deferred into a grouped GEMM launch is written at its flush: the
        # bucket may only count it (and launch its collective) after that kernel is enqueued
        when_grad_ready(p, lambda: self._grad_final(p))

    def _grad_final(self, p):
        g = p.grad
        seg_view = None
        if g is not None:
            b = self._bucket_of[id(p)]
            # AccumulateGrad may have replaced the view (zero_grad(set_to_none=True)): fold back
            sp = self.space
            s = sp.segment_of(p) if g.data_ptr() < sp.grad.data_ptr() or \
                g.data_ptr() >= sp.grad.data_ptr() + sp.grad.numel() * 4 else None
            if s is not None:
                # (added to the earlier micro-batches' sum in accumulate mode, copied otherwise)
                sp._fold(p, s)
        if self._engine is not None:
            self._engine.mark_ready(self._pidx[id(p)])
            return
        b = self._bucket_of[id(p)]
        b.pending -= 1
        self._launch_ready()

    def _launch(self, b: _Bucket):
        view = self.space.grad[b.start:b.end]
        if self._comm is not None:
            lp = self._comm[b.start:b.end]
            lp.copy_(view)
            view = lp
        op = dist.ReduceOp.AVG if self._use_avg else dist.ReduceOp.SUM
        b.work = dist.all_reduce(view, op=op, group=self.process_group, async_op=True)
        b.launched = True

    def _launch_ready(self):
        while self._next < len(self.buckets) and self.buckets[self._next].pending <= 0:
            self._launch(self.buckets[self._next])
            self._next += 1

    def _finalize(self):
        self._callback_queued = False
        flush_wgrads()  # deferred weight gradients (and the bucket marks waiting on them) first
        self._steps += 1
        if self._engine is not None:
            if self.p2p is not None and self.p2p.error():
                # an earlier one-shot all-reduce timed out waiting for a peer (its bucket was
                # poisoned with NaN): fail the step on the host as soon as the flag is visible
                raise RuntimeError("P2P all-reduce timed out waiting for a peer rank (gradients poisoned with NaN); "
                                   f"p2p_timeout_s={self._p2p_timeout_s}")
            self._engine.finalize(self.defer_tail)
            if self._engine.tail_pending():
                starts = self._engine.tail_piece_starts()
                if starts:
                    eng = self._engine
                    self.space.pending_tail = [(s, (lambda i=i: eng.wait_tail_piece(i))) for i, s in enumerate(starts)]
                else:
                    self.space.pending_tail = [(self._engine.tail_start(), self._engine.wait_tail)]
            if self._check:  # RTDC_COLLECTIVE_CHECK=1: desync detector (one tiny all-reduce per step)
                self._agree(self._steps * 1000003 + self._engine.launched() + len(self.buckets), "step sequence")
            if self.zero and not self._zero_checked:
                self._check_zero_optimizer()
            self.space.attach_grad_views()
            return
        # params that produced no gradient this step: zero-filled grads, still reduced
        while self._next < len(self.buckets):
            b = self.buckets[self._next]
            self._launch(b)
            self._next += 1
        for b in self.buckets:
            if b.work is not None:
                b.work.wait()
                if self._comm is not None:
                    with torch.no_grad():
                        self.space.grad[b.start:b.end].copy_(self._comm[b.start:b.end])
            b.work = None
            b.launched = False
            b.pending = len(b.params)
        if not self._use_avg and self.world_size > 1:
            with torch.no_grad():
                self.space.grad.mul_(1.0 / self.world_size)
        self.space.attach_grad_views()
        self._next = 0
        self._callback_queued = False

    def _check_zero_optimizer(self) -> None:
        """ZeRO-1 leaves `p.grad` reduced only on this rank's owned shards (the rest is this
        rank's local, un-averaged gradient).  Only FusedAdamW / FusedSGD, which update exactly
        the owned shards and then all-gather the parameters, may step such a model: a stock
        torch optimizer - or grad clipping / grad-norm logging on p.grad - would silently apply
        rank-dependent updates.  Fail loudly at the end of the first backward instead."""
        self._zero_checked = True
        bad = [i for i, p in enumerate(self.space.params) if not getattr(p, "_rtdc_zero_capable", False)]
        if bad:
            raise RuntimeError(
                f"DistributedDataParallel(zero_stage=1): {len(bad)} parameter(s) are not owned by a FusedAdamW / "
                "FusedSGD optimizer.  Under ZeRO-1 p.grad holds the averaged gradient only on this rank's shards, "
                "so stock torch optimizers (and grad clipping on p.grad) would diverge across ranks; construct "
                "ray_torch_distributed_checkpoint_amd.optim.FusedAdamW/FusedSGD over model.parameters() "
                "or use zero_stage=0.")

    def detach(self) -> None:
        """Remove this wrapper's gradient hooks (e.g. before re-wrapping the same model with
        another bucket plan, as bench.py's bucket sweep does).  The model keeps its flat space."""
        self.space.wait_pending_tail()
        for h in self._hooks:
            h.remove()
        self._hooks = []
        self._engine = None
        if self.p2p is not None:
            from . import health

            health.unregister(self.p2p)
            self.space.skip_ptr = 0
            self.p2p = None

    # ------------------------------------------------------------------ passthrough
    def state_dict(self, *args, **kwargs):
        return super().state_dict(*args, **kwargs)

    def bucket_sizes_bytes(self):
        esz = 2 if self._comm is not None else 4
        return [(b.end - b.start) * esz for b in self.buckets]
