"""The BASELINE bf16 data-parallel workloads as `TorchTrainer` per-worker loops with periodic
sharded asynchronous checkpoints and exact resume.

This is the reference's product - a per-worker loop that checkpoints and `report`s into
`RunConfig(storage_path)` and can be restored with `--from-run` (R/my_ray_module.py:115-213,
:253-264; R/train_flow.py:65-77) - applied to the BASELINE.json configs beyond the toy MLP:

  config 2  resnet18      DDP bf16, sharded DCP save every N steps
  config 3  gpt2-small    DDP, RCCL all-reduce overlapped with the async checkpoint write
  config 4  llama3-8b     sharded state_dict (per-rank `__<r>_0.distcp` shards, 288 GB sizing)
  config 5  any model     kill at step K (RTDC_FAIL_AT_STEP), restart / --from-run, bit-equal

(+ `gpt2-tiny`, `llama3-tiny`, `resnet18-tiny` with the same code paths for CPU/gloo tests.)

Every `ckpt_every_n_steps` steps the loop calls
    h = dcp.async_save(state, train.get_context().next_checkpoint_dir())
    train.report(metrics, checkpoint=Checkpoint.from_async_save(h))
which returns as soon as the HBM snapshot is enqueued: the native engine drains it through the
pinned ring while the next steps run, and the session commits `checkpoint_NNNNNN/`
(`.metadata` + one `__<rank>_0.distcp` per rank) in the background once every rank's shard is
durable; retention (`CheckpointConfig.num_to_keep`) applies on commit.

The checkpointed state is the full train state - model (incl. BatchNorm buffers), optimizer
(FQN-keyed, torch-compatible), step, epoch, sampler position, and every rank's CPU / device /
Philox / numpy RNG state - so a restart (`train.get_checkpoint()`, FailureConfig) or
`--from-run ... --resume_mode exact` continues with losses bit-identical to an uninterrupted
run (deterministic kernels, fixed bucket order).  `resume_mode="weights"` loads only the model
(the reference's warm start).

Data is synthetic and index-addressed (a sample is a pure function of its index), sharded by
`DistributedSampler`'s seed+epoch permutation contract, and generated on the device.
"""
from __future__ import annotations

import argparse
import json
import time
from dataclasses import asdict, dataclass
from typing import Optional

import numpy as np
import torch
import torch.distributed as dist

from . import ops
from . import train
from .checkpoint import dcp
from .checkpoint.state_dict import get_state_dict, set_state_dict
from .ops.xent import IGNORE_INDEX, check_loss_coeffs
from .optim import FusedAdamW, FusedSGD, GradAccumulator
from .parallel.sampler import DistributedSampler
from .utils.profiling import phase


# ---------------------------------------------------------------------------------- config
@dataclass
class WorkloadConfig:
    model: str = "gpt2-tiny"
    steps: int = 20                       # total optimizer steps (global)
    batch_size_per_worker: Optional[int] = None
    seq_len: Optional[int] = None         # tokens (LMs) or image side (ResNet)
    lr: Optional[float] = None
    ckpt_every_n_steps: Optional[int] = None   # None -> CheckpointConfig.ckpt_every_n_steps
    report_every_n_steps: Optional[int] = None  # None -> ckpt interval
    seed: int = 1234
    dataset_size: int = 1 << 20
    resume_mode: str = "exact"            # exact | weights (for an explicit `checkpoint`)
    checkpoint: object = None             # upstream Checkpoint (--from-run / --from-task)
    async_checkpoint: Optional[bool] = None  # None -> CheckpointConfig.async_checkpoint
    num_classes: int = 10
    max_grad_norm: Optional[float] = None  # clip the global gradient norm inside the fused step (None / 0: off)
    doc_len: Optional[int] = None  # LMs: packed sequences of documents of this mean length (None / 0: off)
    sliding_window: Optional[int] = None  # LMs: every attention sees its last N keys only (None / 0: off)
    attn_dropout: Optional[float] = None  # LMs: dropout on the attention probabilities (None / 0: off)
    # LMs: dtype the fused AdamW stores exp_avg / exp_avg_sq in: "fp32" | "bf16" (bf16: stochastically
    # rounded with bits keyed by `seed`; a checkpoint resumes into the same setting)
    opt_state_dtype: str = "fp32"
    # micro-batches per optimizer step (optim.GradAccumulator): each step draws this many batches,
    # adds their gradients in place in the flat buffer and applies their mean
    grad_accum_steps: int = 1
    # learning-rate schedule over the optimizer steps (optim/schedule.py): "constant" | "cosine" |
    # "linear", with `warmup_steps` of linear warmup and a decay to min_lr_ratio x lr that ends at step
    # `lr_total_steps` (None: `steps`).  "constant" without warmup attaches no schedule at all.
    lr_schedule: str = "constant"
    warmup_steps: int = 0
    min_lr_ratio: float = 0.0
    lr_total_steps: Optional[int] = None
    # GPU: build the fused optimizer with capturable=True (lr, bias corrections and the step number read
    # from device tables by a device step counter: the same bits, and the step may be captured into a
    # hipGraph).  Off by default: the device-table kernels measured 0.5 us (about 1 %) behind the
    # host-scalar ones at ResNet-18 size, and a step ends with one more tiny launch
    # (profiles/adamw_capturable_ab.md).
    opt_capturable: bool = False
    # optional terms of the fused cross-entropy kernels (ops/xent.py), every workload: the auxiliary
    # z-loss z * logsumexp^2 per row and label smoothing in [0, 1) (None / 0: off).  With either on
    # the report rows also carry ce_loss / ce_losses, the plain cross-entropy of the same steps.
    z_loss: Optional[float] = None
    label_smoothing: Optional[float] = None

    @classmethod
    def from_dict(cls, d: dict) -> "WorkloadConfig":
        known = {f for f in cls.__dataclass_fields__}
        return cls(**{k: v for k, v in d.items() if k in known})


_OPT_STATE_DTYPES = {"fp32": "float32", "bf16": "bfloat16"}  # option value -> torch dtype name

_LR_SCHEDULES = ("constant", "cosine", "linear")


def make_schedule(cfg: WorkloadConfig):
    """The `LRSchedule` of a config; None for the default (constant, no warmup): then no schedule
    object exists and the optimizer runs exactly as before."""
    from .optim import LRSchedule

    if cfg.lr_schedule not in _LR_SCHEDULES:
        raise ValueError(f"lr_schedule must be one of {list(_LR_SCHEDULES)}, got {cfg.lr_schedule!r}")
    w = int(cfg.warmup_steps or 0)
    if cfg.lr_schedule == "constant" and w == 0:
        return None
    total = int(cfg.lr_total_steps or cfg.steps)
    if cfg.lr_schedule == "cosine":
        return LRSchedule.warmup_cosine(w, total, cfg.min_lr_ratio)
    if cfg.lr_schedule == "linear":
        return LRSchedule.warmup_linear(w, total, cfg.min_lr_ratio)
    return LRSchedule.warmup_linear(w, total, 1.0)  # constant after the warmup


_DEFAULTS = {
    # name prefix: (batch/worker, seq_len or image side, lr)
    "gpt2-tiny": (4, 64, 1e-3), "gpt2": (16, 1024, 6e-4),
    "llama3-tiny": (2, 64, 1e-3), "llama3": (1, 2048, 3e-4),
    "resnet18-tiny": (8, 32, 0.05), "resnet18": (256, 224, 0.1),
}


def _defaults(name: str):
    for k in sorted(_DEFAULTS, key=len, reverse=True):
        if name.startswith(k):
            return _DEFAULTS[k]
    raise ValueError(f"unknown workload model {name!r}")


# ---------------------------------------------------------------------------------- data
def _mix_add(x: torch.Tensor, add: int) -> torch.Tensor:
    """Deterministic integer hash of x + add (values stay < 2^31: no signed overflow on any
    device); `data_ops.hip` mix31 is the same function."""
    x = (x + add) & 0x7FFFFFFF
    for _ in range(3):
        x = ((x ^ (x >> 13)) * 1103515245 + 12345) & 0x7FFFFFFF
    return x


def _mix(x: torch.Tensor, seed: int) -> torch.Tensor:
    """The token hash: `_mix_add` under the first seed constant."""
    return _mix_add(x, seed * 7919 + 1)


class SyntheticTokens:
    """`n` sequences of `seq_len + 1` random tokens; sequence i is a function of (seed, i).

    doc_len = L packs documents into each sequence: position p > 0 of sequence i starts a
    document iff `_mix_add` of (i, p) under a second seed constant is 0 mod L (mean length L).  The
    layout is stateless - a function of (seed, i, p) - so exact resume needs no new state.
    `batch()` then returns (inputs, targets, docs) with the target of each document's last token
    IGNORE_INDEX (the next token belongs to another document)."""

    def __init__(self, n: int, seq_len: int, vocab: int, seed: int = 0, doc_len: int | None = None):
        self.n, self.seq_len, self.vocab, self.seed = n, seq_len, vocab, seed
        self.doc_len = int(doc_len) if doc_len else None

    def _doc_seed_add(self) -> int:
        return self.seed * 104729 + 17  # (tokens: seed * 7919 + 1)

    def _docs(self, idx: torch.Tensor, tgt: torch.Tensor):
        """(targets with document ends ignored, DocLayout) of the sequences idx."""
        B, T = tgt.shape
        if idx.is_cuda:
            from .ops._ext import gpu_ext

            flags = torch.empty((B, T), dtype=torch.uint8, device=idx.device)
            gpu_ext().synth_doc_flags(idx.to(torch.int64).contiguous(), flags, self.doc_len, self._doc_seed_add())
        else:
            pos = torch.arange(T, device=idx.device, dtype=torch.int64)
            h = _mix_add(idx.to(torch.int64)[:, None] * (T + 1) + pos, self._doc_seed_add())
            flags = ((h % self.doc_len == 0) & (pos > 0)[None, :]).to(torch.uint8)
        docs = ops.DocLayout.from_flags(flags)
        pos = torch.arange(T, device=idx.device, dtype=torch.int32)
        last = docs.end == (pos + 1)[None, :]
        return tgt.masked_fill(last, IGNORE_INDEX), docs

    def __len__(self):
        return self.n

    def batch(self, idx: torch.Tensor):
        """(inputs, targets), contiguous [B, seq_len] int64.  On the GPU one native kernel
        (`data_ops.hip` synth_tokens) writes both; the CPU path is the same hash in ATen."""
        if idx.is_cuda:
            from .ops._ext import gpu_ext

            ids = idx.to(torch.int64).contiguous()
            B = ids.numel()
            inp = torch.empty((B, self.seq_len), dtype=torch.int64, device=idx.device)
            tgt = torch.empty_like(inp)
            gpu_ext().synth_tokens(ids, inp, tgt, self.vocab, self.seed * 7919 + 1)
            if self.doc_len:
                return (inp, *self._docs(ids, tgt))
            return inp, tgt
        pos = torch.arange(self.seq_len + 1, device=idx.device, dtype=torch.int64)
        tok = _mix(idx.to(torch.int64)[:, None] * (self.seq_len + 1) + pos, self.seed) % self.vocab
        if self.doc_len:
            return (tok[:, :-1].contiguous(), *self._docs(idx, tok[:, 1:].contiguous()))
        return tok[:, :-1].contiguous(), tok[:, 1:].contiguous()


class SyntheticImages:
    """`n` labelled images; image i = prototype (i mod P) of a fixed pool, label = its class."""

    def __init__(self, n: int, hw: int, classes: int, device, seed: int = 0, pool: int = 64):
        g = torch.Generator().manual_seed(seed)
        self.n, self.classes = n, classes
        self.x = torch.randn(pool, 3, hw, hw, generator=g).to(device)
        self.y = (torch.arange(pool) % classes).to(device)

    def __len__(self):
        return self.n

    def batch(self, idx: torch.Tensor):
        j = idx % self.x.shape[0]
        return self.x.index_select(0, j), self.y.index_select(0, j)


class ShardedStream:
    """Batches of this rank's shard in sampler order with an exact, checkpointable position
    (epoch, pos): `DistributedSampler`'s seed+epoch permutation, strided by rank."""

    def __init__(self, dataset, batch: int, world: int, rank: int, seed: int, device):
        self.ds, self.B, self.device = dataset, batch, device
        self.sampler = DistributedSampler(dataset, num_replicas=world, rank=rank, shuffle=True, seed=seed,
                                          drop_last=True)
        self.epoch, self.pos, self._ids, self._ids_epoch = 0, 0, None, None

    def _epoch_ids(self):
        if self._ids_epoch != self.epoch:
            self.sampler.set_epoch(self.epoch)
            self._ids = torch.tensor(self.sampler.indices(), dtype=torch.int64, device=self.device)
            self._ids_epoch = self.epoch
        return self._ids

    def next(self):
        ids = self._epoch_ids()
        if self.pos + self.B > ids.numel():
            self.epoch, self.pos = self.epoch + 1, 0
            ids = self._epoch_ids()
        j = ids[self.pos:self.pos + self.B]
        self.pos += self.B
        return self.ds.batch(j)

    def state_dict(self):
        return {"epoch": self.epoch, "pos": self.pos}

    def load_state_dict(self, sd):
        self.epoch, self.pos = int(sd["epoch"]), int(sd["pos"])


# ---------------------------------------------------------------------------------- model
@dataclass
class Workload:
    model: torch.nn.Module
    optimizer: torch.optim.Optimizer
    data: object
    batch: int
    seq_len: int
    tokens_per_sample: int = 0
    flops_per_sample: float = 0.0
    loss_fn: object = None


def build(cfg: WorkloadConfig, device) -> Workload:
    """Model (same random init on every rank: seeded), optimizer, synthetic dataset."""
    B0, S0, lr0 = _defaults(cfg.model)
    B = cfg.batch_size_per_worker or B0
    S = cfg.seq_len or S0
    lr = cfg.lr or lr0
    clip = cfg.max_grad_norm or None
    # the schedule rewrites group["lr"] on the host before every step (host-scalar kernels);
    # opt_capturable moves lr, the bias corrections and the step number into device tables (GPU only)
    sched = make_schedule(cfg)
    sched_kw = {} if sched is None else {"lr_schedule": sched}
    if cfg.opt_capturable and torch.device(device).type == "cuda":
        sched_kw["capturable"] = True
    ls, zl = check_loss_coeffs(cfg.label_smoothing, cfg.z_loss)
    aux = bool(ls or zl)  # the loss function then returns (loss, plain cross-entropy)
    torch.manual_seed(cfg.seed)
    name = cfg.model
    if name.startswith("resnet18"):
        from .models import ResNet18

        # "-tiny" = the full network on 32x32 images (the GEMM tiles need >= 64 channels)
        model = ResNet18(num_classes=cfg.num_classes).to(device)
        opt = FusedSGD(model.parameters(), lr=lr, momentum=0.9, weight_decay=5e-5, max_grad_norm=clip, **sched_kw)
        data = SyntheticImages(cfg.dataset_size, S, cfg.num_classes, device, seed=cfg.seed)
        if aux:
            return Workload(model, opt, data, B, S, 0, model.flops_per_sample(S),
                            lambda net, x, y: ops.cross_entropy(net(x), y, label_smoothing=ls, z_loss=zl,
                                                                return_ce=True))
        return Workload(model, opt, data, B, S, 0, model.flops_per_sample(S),
                        lambda net, x, y: ops.cross_entropy(net(x), y))
    if name.startswith("llama"):
        from .models import Llama, LlamaConfig

        mc = LlamaConfig.named(name)
        S = min(S, mc.max_seq_len)
        model = Llama(mc, device=device)
    elif name.startswith("gpt2"):
        from .models import GPT2, GPT2Config

        mc = GPT2Config.named(name)
        S = min(S, mc.n_positions)
        model = GPT2(mc).to(device)
    else:
        raise ValueError(f"unknown workload model {name!r}")
    opt = FusedAdamW(model.parameters(), lr=lr, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1, max_grad_norm=clip,
                     state_dtype=getattr(torch, _OPT_STATE_DTYPES[cfg.opt_state_dtype]), rounding_seed=cfg.seed, **sched_kw)
    data = SyntheticTokens(cfg.dataset_size, S, mc.vocab_size, seed=cfg.seed, doc_len=cfg.doc_len or None)
    # (with documents the batch is (x, y, docs); flops_per_token still counts the full causal triangle,
    # under a sliding window too)
    model.sliding_window = int(cfg.sliding_window) if cfg.sliding_window else None
    model.attn_dropout = float(cfg.attn_dropout) if cfg.attn_dropout else 0.0
    if aux:
        model.z_loss, model.label_smoothing = zl, ls  # forward() leaves the plain cross-entropy in last_ce

        def lm_loss(net, x, y, docs=None):
            loss = net(x, y) if docs is None else net(x, y, docs)
            return loss, _unwrap(net).last_ce

        return Workload(model, opt, data, B, S, S, model.flops_per_token(S) * S, lm_loss)
    return Workload(model, opt, data, B, S, S, model.flops_per_token(S) * S,
                    lambda net, x, y, docs=None: net(x, y) if docs is None else net(x, y, docs))


# ---------------------------------------------------------------------------------- RNG state
def _pack(obj) -> bytes:
    """Deterministic byte encoding of a nested dict of tensors / JSON scalars (a JSON header +
    raw tensor bytes): equal states give equal bytes on every rank, so the replicated,
    deduplicated sharded save stores the value once and any rank may be its writer."""
    tensors = []

    def enc(o):
        if torch.is_tensor(o):
            tensors.append(o.detach().cpu().contiguous())
            return {"__t": len(tensors) - 1, "dtype": str(o.dtype).replace("torch.", ""), "shape": list(o.shape)}
        if isinstance(o, dict):
            return {str(k): enc(v) for k, v in o.items()}
        return o

    head = json.dumps(enc(obj), sort_keys=True).encode()
    body = b"".join(t.reshape(-1).view(torch.uint8).numpy().tobytes() for t in tensors)
    return len(head).to_bytes(8, "little") + head + body


def _unpack(blob: bytes):
    n = int.from_bytes(blob[:8], "little")
    head = json.loads(blob[8:8 + n].decode())
    body = memoryview(blob)[8 + n:]
    metas = []

    def walk(o):
        if isinstance(o, dict):
            if "__t" in o:
                metas.append(o)
            else:
                for v in o.values():
                    walk(v)

    walk(head)
    offs, at = {}, 0
    for m in sorted(metas, key=lambda m: m["__t"]):
        dt = getattr(torch, m["dtype"])
        nb = int(np.prod(m["shape"], dtype=np.int64)) * torch.empty((), dtype=dt).element_size()
        offs[m["__t"]] = (at, nb, dt, m["shape"])
        at += nb

    def dec(o):
        if isinstance(o, dict):
            if "__t" in o:
                off, nb, dt, shape = offs[o["__t"]]
                raw = torch.frombuffer(bytearray(body[off:off + nb]), dtype=torch.uint8)
                return raw.view(dt).reshape(shape)
            return {k: dec(v) for k, v in o.items()}
        return o

    return dec(head)


def _rng_blob(device) -> bytes:
    """Every rank's RNG states (CPU, device, Philox dropout stream, numpy) gathered to all
    ranks and packed into one `bytes` value (identical on every rank)."""
    _, keys, pos, has_gauss, gauss = np.random.get_state()
    mine = {"torch_cpu": torch.get_rng_state(), "philox": ops.default_stream().state_dict(),
            "numpy": {"keys": torch.from_numpy(keys.astype(np.int64)), "pos": int(pos),
                      "has_gauss": int(has_gauss), "gauss": float(gauss)}}
    if device.type == "cuda":
        mine["torch_cuda"] = torch.cuda.get_rng_state(device)
    world = dist.get_world_size() if dist.is_initialized() else 1
    parts = [None] * world
    if world > 1:
        dist.all_gather_object(parts, mine)
    else:
        parts = [mine]
    return _pack({f"rank{r}": p for r, p in enumerate(parts)})


def _set_rng(blob: bytes, rank: int, device) -> bool:
    if not blob:
        return False
    st = _unpack(blob).get(f"rank{rank}")
    if st is None:  # resumed at a different world size: this rank has no recorded stream
        return False
    torch.set_rng_state(st["torch_cpu"].cpu())
    ops.default_stream().load_state_dict(st["philox"])
    n = st["numpy"]
    np.random.set_state(("MT19937", n["keys"].cpu().numpy().astype(np.uint32), n["pos"], n["has_gauss"],
                         n["gauss"]))
    if device.type == "cuda" and "torch_cuda" in st:
        torch.cuda.set_rng_state(st["torch_cuda"].cpu(), device)
    return True


# ---------------------------------------------------------------------------------- loop
def samples_per_s(steps: int, grad_accum_steps: int, batch: int, world: int, dt: float) -> float:
    """Samples per second of `steps` optimizer steps in dt seconds: each step consumes
    grad_accum_steps micro-batches of `batch` samples on each of `world` workers."""
    return round(steps * grad_accum_steps * batch * world / max(dt, 1e-9), 3)


def _unwrap(m):
    return m.module if hasattr(m, "module") else m


def _train_state(core, opt, stream, step, rng: bytes):
    msd, osd = get_state_dict(core, opt)
    return {"model": msd, "optim": osd,
            "trainer": {"step": int(step), "epoch": stream.epoch, "pos": stream.pos, "rng": rng}}


def restore(core, opt, stream, checkpoint, mode: str, device, rank: int) -> int:
    """Load a sharded checkpoint into the live model/optimizer; returns the step to resume at
    (0 for a weights-only warm start)."""
    with checkpoint.as_directory() as path:
        if mode == "weights":
            msd, _ = get_state_dict(core, None)
            sd = dcp.load({"model": msd}, path)
            set_state_dict(core, None, model_state_dict=sd["model"])
            step = 0
        else:
            sd = _train_state(core, opt, stream, 0, b"")
            dcp.load(sd, path)
            set_state_dict(core, opt, model_state_dict=sd["model"], optim_state_dict=sd["optim"])
            tr = sd["trainer"]
            stream.load_state_dict(tr)
            if not _set_rng(tr["rng"], rank, device):
                torch.manual_seed(int(tr["step"]) * 1000003 + rank)
            step = int(tr["step"])
            if not getattr(opt, "_counts_steps", True):
                opt.step_count = step  # (SGD's state carries no step number: the schedule resumes from the trainer's)
    sp = getattr(opt, "flat_space", None) or getattr(core.parameters().__next__(), "_rtdc_space", None)
    if sp is not None:
        sp.refresh_shadows()  # bf16 compute copies of the restored fp32 masters
    return step


def train_loop_per_worker(config: dict):
    cfg = WorkloadConfig.from_dict(config)
    ctx = train.get_context()
    ccfg = ctx.get_checkpoint_config()
    every = cfg.ckpt_every_n_steps or ccfg.ckpt_every_n_steps
    report_every = cfg.report_every_n_steps or every or max(1, cfg.steps)
    use_async = ccfg.async_checkpoint if cfg.async_checkpoint is None else cfg.async_checkpoint
    dev = train.torch.get_device()
    world, rank = ctx.get_world_size(), ctx.get_world_rank()
    train.torch.enable_reproducibility(cfg.seed)

    wl = build(cfg, dev)
    if cfg.attn_dropout:
        # every rank's default Philox stream starts at the same seed and would draw the same masks:
        # seeded per (seed, rank) before the first step; an exact resume then restores the position
        # from the checkpoint's RNG state.  With attn_dropout off nothing is seeded.
        ops.manual_seed(int(cfg.seed) * 1000003 + rank)
    # fused optimizers wait for the deferred last bucket themselves (DDP defer_tail_to_optimizer)
    net = train.torch.prepare_model(wl.model, parallel_strategy_kwargs={"defer_tail_to_optimizer": True})
    core, opt = _unwrap(net), wl.optimizer
    stream = ShardedStream(wl.data, wl.batch, world, rank, cfg.seed, dev)

    start = 0
    restart = train.get_checkpoint()  # set when the trainer restarted this gang after a failure
    if restart is not None:
        start = restore(core, opt, stream, restart, "exact", dev, rank)
        print(f"[workload] rank {rank}: restarted from {restart.path} at step {start}", flush=True)
    elif cfg.checkpoint is not None:
        start = restore(core, opt, stream, cfg.checkpoint, cfg.resume_mode, dev, rank)
        print(f"[workload] rank {rank}: resumed ({cfg.resume_mode}) from {cfg.checkpoint.path} at step {start}",
              flush=True)

    pending = None  # this rank's in-flight async save (at most one: bounded snapshot memory)
    losses = []
    clipping = bool(cfg.max_grad_norm)
    scheduled = getattr(opt, "lr_schedule", None) is not None
    norms = []  # per-step pre-clip gradient norms (device scalars, read with the losses)
    aux = bool(cfg.z_loss or cfg.label_smoothing)  # the loss function returns (loss, plain cross-entropy)
    ces = []  # aux: per-step plain cross-entropy (device scalars, read with the losses)
    t_last, n_last = time.perf_counter(), 0
    k = int(cfg.grad_accum_steps or 1)
    if k < 1:
        raise ValueError(f"grad_accum_steps must be >= 1, got {k}")
    # k > 1: every optimizer step draws k batches; only the last backward reduces across ranks
    acc = GradAccumulator(opt, steps=k, ddp=net if hasattr(net, "no_sync") else None) if k > 1 else None
    for step in range(start, cfg.steps):
        train.report_progress(step)
        if acc is None:
            batch = stream.next()  # (x, y), or (x, y, docs) for packed sequences (doc_len)
            with phase("fwd"):
                loss = wl.loss_fn(net, *batch)
                if aux:
                    loss, ce = loss
            with phase("bwd"):
                loss.backward()
            loss = loss.detach()
        else:
            micro, micro_ce = [], []
            for i in range(k):
                batch = stream.next()
                with acc.micro_step(i):
                    with phase("fwd"):
                        li = wl.loss_fn(net, *batch)
                        if aux:
                            li, ci = li
                            micro_ce.append(ci)
                    with phase("bwd"):
                        li.backward()
                micro.append(li.detach())
            loss = torch.stack(micro).float().mean()  # (on the device: still one host sync per report)
            if aux:
                ce = torch.stack(micro_ce).float().mean()
        with phase("opt"):
            opt.step()
            opt.zero_grad(set_to_none=True)
        losses.append(loss)
        if clipping:
            norms.append(opt.grad_norm.clone())
        if aux:
            ces.append(ce)
        n_last += 1
        done = step + 1
        do_ckpt = bool(every) and (done % every == 0 or done == cfg.steps)
        if not (do_ckpt or done % report_every == 0 or done == cfg.steps):
            continue
        vals = torch.stack(losses).float()
        if clipping:
            vals = torch.cat([vals, torch.stack(norms)])
        if aux:
            vals = torch.cat([vals, torch.stack(ces).float()])
        vals = vals.tolist()  # the one host sync per report
        n = len(losses)
        vals, gnorms, cvals = vals[:n], vals[n:n + len(norms)], vals[n + len(norms):]
        dt = time.perf_counter() - t_last
        metrics = {"step": done, "loss": vals[-1], "losses": vals, "epoch": stream.epoch,
                   "samples_per_s": samples_per_s(n_last, k, wl.batch, world, dt)}
        if wl.tokens_per_sample:
            metrics["tokens_per_s"] = round(metrics["samples_per_s"] * wl.tokens_per_sample, 1)
        if clipping:
            metrics["grad_norm"], metrics["grad_norms"] = gnorms[-1], gnorms
        if scheduled:
            metrics["lr"] = opt.get_last_lr()[0]  # the last step's, group 0
        if aux:
            metrics["ce_loss"], metrics["ce_losses"] = cvals[-1], cvals
        losses, norms, ces, n_last = [], [], [], 0
        ck = None
        if do_ckpt:
            with phase("ckpt"):
                if pending is not None:
                    pending.wait()
                state = _train_state(core, opt, stream, done, _rng_blob(dev))
                if use_async:
                    pending = dcp.async_save(state, ctx.next_checkpoint_dir())
                    ck = train.Checkpoint.from_async_save(pending)
                    metrics["ckpt_snapshot_s"] = round(pending.t_return, 6)
                else:
                    t0 = time.perf_counter()
                    d = ctx.next_checkpoint_dir()
                    dcp.save(state, d)
                    ck = train.Checkpoint.from_directory(d)
                    metrics["ckpt_save_s"] = round(time.perf_counter() - t0, 6)
        train.report(metrics, checkpoint=ck)
        t_last = time.perf_counter()
    if pending is not None:
        pending.wait()


# ---------------------------------------------------------------------------------- driver
def default_zero_stage(model: str, world: int) -> int:
    """ZeRO-1 by default where the replicated optimizer dominates: Llama-3-8B's AdamW streams
    ~241 GB per step (40 of 147 ms on one MI355X); sharded over W ranks each moves 1/W of it,
    and the state checkpoint is written as owner shards with no all-gather.  The small models
    keep the replicated step (their update is < 1 ms)."""
    return 1 if model.startswith("llama") and world > 1 else 0


def train_workload(model: str = "gpt2-tiny", steps: int = 20, num_workers: int = 1, use_gpu: bool = False,
                   batch_size_per_worker: int | None = None, seq_len: int | None = None, lr: float | None = None,
                   ckpt_every_n_steps: int | None = 5, num_checkpoints_to_keep: int | None = 2,
                   checkpoint_storage_path: str | None = None, checkpoint=None, resume_mode: str = "exact",
                   max_failures: int = 0, seed: int = 1234, grad_comm_dtype: str = "fp32",
                   bucket_cap_mb: float = 32.0, zero_stage: int = -1, progress_timeout_s: float | None = 300.0,
                   dataset_size: int = 1 << 20, name: str | None = None, verbose: int = 1,
                   report_every_n_steps: int | None = None, max_grad_norm: float | None = None,
                   doc_len: int | None = None, sliding_window: int | None = None,
                   attn_dropout: float | None = None, opt_state_dtype: str = "fp32", grad_accum_steps: int = 1,
                   lr_schedule: str = "constant", warmup_steps: int = 0, min_lr_ratio: float = 0.0,
                   lr_total_steps: int | None = None, opt_capturable: bool = False, z_loss: float | None = None,
                   label_smoothing: float | None = None):
    """`train_fashion_mnist`'s counterpart for the bf16 workloads (R/my_ray_module.py:216-251).
    zero_stage -1: `default_zero_stage(model, num_workers)`.  max_grad_norm: clip the global
    gradient norm inside the fused optimizer step (None / 0: off); the report rows then carry
    `grad_norm` / `grad_norms` (pre-clip).  doc_len (LMs): train on packed sequences of synthetic
    documents of that mean length, attention and RoPE positions restricted to each document
    (None / 0: off; the report rows are unchanged).  sliding_window (LMs): every attention layer
    sees the last N keys only, within the document under doc_len (None / 0: off; nothing new is
    checkpointed - a resume passes the same value).  attn_dropout (LMs; None / 0: off): dropout on
    the attention probabilities of every block, drawn inside the flash kernels
    (ops.causal_attention dropout_p=; the probability is quantised to 1/256).  Each rank's default
    Philox stream is then seeded from (seed, rank) before the first step; its position is part of
    the RNG state every checkpoint already carries, so an exact resume with the same value is
    bit-identical and nothing new is checkpointed.  Off: nothing is seeded, rows, checkpoints and
    bits are unchanged.  opt_state_dtype (LMs): "fp32" | "bf16" - the
    dtype FusedAdamW stores its moments in (bf16: half the optimizer memory and checkpoint bytes,
    stochastic rounding keyed by `seed`; the report rows are unchanged).  grad_accum_steps = k:
    every optimizer step accumulates k micro-batches in place (optim.GradAccumulator) and applies
    their mean; `steps` stays optimizer steps, a row's loss is the mean over its k micro-batches
    and samples_per_s / tokens_per_s count k x the batch.  lr_schedule "constant" | "cosine" |
    "linear" with `warmup_steps` of linear warmup and a decay to `min_lr_ratio` x lr that ends at
    optimizer step `lr_total_steps` (None: `steps`): the report rows then carry `lr` (the row's last
    step, group 0).  The schedule is a function of the step count that comes back with the optimizer
    state, so an exact resume needs the same arguments and nothing else - resuming into a longer
    `steps` needs the original `lr_total_steps` given explicitly.  The default (constant, no warmup)
    attaches nothing: rows, checkpoints and bits are unchanged.  opt_capturable (GPU): the fused
    optimizer reads lr, the bias corrections and the step number from device tables
    (`capturable=True`): the same bits as the host path, and a step that may be captured.
    z_loss / label_smoothing (every workload; None / 0: off): the auxiliary z-loss
    z * logsumexp(logits)^2 per row and label smoothing in [0, 1), both computed inside the fused
    cross-entropy kernels (ops/xent.py).  `loss` / `losses` stay the optimised objective; with either
    term on the rows also carry `ce_loss` / `ce_losses`, the plain cross-entropy of the same steps
    (the mean over the micro-batches under grad_accum_steps).  Nothing new is checkpointed: an
    exact resume with the same two arguments is bit-identical; with both off rows, checkpoints and
    bits are unchanged."""
    if int(grad_accum_steps) < 1:
        raise ValueError(f"grad_accum_steps must be >= 1, got {grad_accum_steps}")
    if opt_state_dtype not in _OPT_STATE_DTYPES:
        raise ValueError(f"opt_state_dtype must be one of {sorted(_OPT_STATE_DTYPES)}, got {opt_state_dtype!r}")
    check_loss_coeffs(label_smoothing, z_loss)  # (argument errors here, not in the workers)
    if sliding_window and int(sliding_window) < 1:
        raise ValueError(f"sliding_window must be >= 1 (None / 0: off), got {sliding_window}")
    if attn_dropout:
        ops.attention_dropout_keep(attn_dropout)  # (ValueError here, not in the workers)
    if zero_stage < 0:
        zero_stage = default_zero_stage(model, num_workers)
    cfg = WorkloadConfig(model=model, steps=steps, batch_size_per_worker=batch_size_per_worker, seq_len=seq_len,
                         lr=lr, ckpt_every_n_steps=ckpt_every_n_steps, seed=seed, resume_mode=resume_mode,
                         checkpoint=checkpoint, dataset_size=dataset_size, report_every_n_steps=report_every_n_steps,
                         max_grad_norm=max_grad_norm or None, doc_len=doc_len or None,
                         sliding_window=int(sliding_window) if sliding_window else None,
                         attn_dropout=float(attn_dropout) if attn_dropout else None,
                         opt_state_dtype=opt_state_dtype, grad_accum_steps=int(grad_accum_steps),
                         lr_schedule=lr_schedule, warmup_steps=int(warmup_steps or 0),
                         min_lr_ratio=float(min_lr_ratio or 0.0), lr_total_steps=lr_total_steps or None,
                         opt_capturable=bool(opt_capturable), z_loss=float(z_loss) if z_loss else None,
                         label_smoothing=float(label_smoothing) if label_smoothing else None)
    make_schedule(cfg)  # (argument errors here, not in the workers)
    run_config = train.RunConfig(
        name=name, storage_path=checkpoint_storage_path, verbose=verbose,
        checkpoint_config=train.CheckpointConfig(num_to_keep=num_checkpoints_to_keep,
                                                 ckpt_every_n_steps=ckpt_every_n_steps),
        failure_config=train.FailureConfig(max_failures=max_failures),
        progress_timeout_s=progress_timeout_s)
    trainer = train.TorchTrainer(
        train_loop_per_worker, train_loop_config={k: v for k, v in asdict(cfg).items() if v is not None},
        scaling_config=train.ScalingConfig(num_workers=num_workers, use_gpu=use_gpu),
        torch_config=train.TorchConfig(grad_comm_dtype=grad_comm_dtype, bucket_cap_mb=bucket_cap_mb,
                                       zero_stage=zero_stage),
        run_config=run_config)
    return trainer.fit()


def main(argv=None):
    ap = argparse.ArgumentParser(description="bf16 DDP workload with sharded async checkpoints")
    ap.add_argument("--model", default="gpt2-tiny")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--num-workers", type=int, default=1)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--seq-len", type=int, default=None)
    ap.add_argument("--ckpt-every", type=int, default=5)
    ap.add_argument("--keep", type=int, default=2)
    ap.add_argument("--storage", default=None)
    ap.add_argument("--max-failures", type=int, default=0)
    ap.add_argument("--grad-comm-dtype", default="fp32")
    ap.add_argument("--zero-stage", type=int, default=-1, choices=[-1, 0, 1],
                    help="-1: ZeRO-1 for llama* at more than one worker, else replicated")
    ap.add_argument("--max-grad-norm", type=float, default=None,
                    help="clip the global gradient norm inside the fused optimizer step (default: off)")
    ap.add_argument("--doc-len", type=int, default=None,
                    help="LMs: packed sequences of synthetic documents of this mean length, attention and "
                         "RoPE positions per document (default: off)")
    ap.add_argument("--sliding-window", type=int, default=None,
                    help="LMs: sliding-window attention, every layer sees its last N keys only (default: off)")
    ap.add_argument("--attn-dropout", type=float, default=None,
                    help="LMs: dropout on the attention probabilities, inside the flash kernels (default: off)")
    ap.add_argument("--opt-state-dtype", default="fp32", choices=sorted(_OPT_STATE_DTYPES),
                    help="LMs: dtype of the fused AdamW's stored moments (bf16: stochastically rounded)")
    ap.add_argument("--grad-accum-steps", type=int, default=1,
                    help="micro-batches accumulated in place per optimizer step (default 1: off)")
    ap.add_argument("--lr-schedule", default="constant", choices=list(_LR_SCHEDULES),
                    help="learning-rate schedule over the optimizer steps (default: constant)")
    ap.add_argument("--warmup-steps", type=int, default=0, help="linear warmup steps of the schedule")
    ap.add_argument("--min-lr-ratio", type=float, default=0.0,
                    help="the schedule decays to this fraction of the learning rate")
    ap.add_argument("--lr-total-steps", type=int, default=None,
                    help="step at which the decay ends (default: --steps; give it explicitly when resuming into a "
                         "longer --steps)")
    ap.add_argument("--opt-capturable", action="store_true",
                    help="GPU: fused optimizer with device-resident step count, lr and bias-correction tables "
                         "(capturable=True; same bits as the default host path)")
    ap.add_argument("--z-loss", type=float, default=None,
                    help="auxiliary z-loss z * logsumexp(logits)^2 per row, inside the fused cross-entropy kernels "
                         "(default: off); rows then also carry the plain ce_loss")
    ap.add_argument("--label-smoothing", type=float, default=None,
                    help="label smoothing of the training cross-entropy, in [0, 1) (default: off)")
    ap.add_argument("--cpu", action="store_true")
    a = ap.parse_args(argv)
    use_gpu = torch.cuda.is_available() and not a.cpu
    res = train_workload(a.model, a.steps, a.num_workers, use_gpu, a.batch, a.seq_len, None, a.ckpt_every, a.keep,
                         a.storage, max_failures=a.max_failures, grad_comm_dtype=a.grad_comm_dtype,
                         zero_stage=a.zero_stage, max_grad_norm=a.max_grad_norm, doc_len=a.doc_len,
                         sliding_window=a.sliding_window, attn_dropout=a.attn_dropout,
                         opt_state_dtype=a.opt_state_dtype, grad_accum_steps=a.grad_accum_steps,
                         lr_schedule=a.lr_schedule, warmup_steps=a.warmup_steps, min_lr_ratio=a.min_lr_ratio,
                         lr_total_steps=a.lr_total_steps, opt_capturable=a.opt_capturable, z_loss=a.z_loss,
                         label_smoothing=a.label_smoothing)
    print(res)


if __name__ == "__main__":
    # run the importable module's main: the training loop is then pickled for the workers by
    # reference (as `python -m`'s __main__ it would be pickled by value, globals included, which
    # fails on the torch namespaces among them)
    from ray_torch_distributed_checkpoint_amd.workloads import main as _main

    _main()
