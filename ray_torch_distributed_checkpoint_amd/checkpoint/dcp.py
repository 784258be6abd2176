"""Sharded checkpoints in the `torch.distributed.checkpoint` (DCP) on-disk format, natively.

Format (identical to torch DCP 2.x, so `torch.distributed.checkpoint.load` reads what we
write and we read what it writes - torch/distributed/checkpoint/filesystem.py:97,319-372,763):
  <dir>/__{rank}_0.distcp   back-to-back items: a torch.save zip archive per tensor chunk,
                            torch.save bytes per non-tensor value (BYTE_IO)
  <dir>/.metadata           pickled `Metadata` (tensor sizes/chunks, storage (file, off, len)),
                            written by rank 0 via .tmp + fsync + rename (atomic commit)

What is different from torch DCP, MI355X-first:
* **Planning needs no collectives.**  Data-parallel state is replicated, so every rank
  flattens the same state_dict, computes the same size-balanced owner assignment (the
  dedup of _dedup_save_plans.py, but greedy by bytes) and the same file layouts (item sizes
  are deterministic), so rank 0 can write `.metadata` without gather/scatter of plans.
* **Snapshot in HBM, write in the background.**  Owned tensors are cloned on the compute
  stream (a few D2D copies: ~0.1 ms per 100 MB at HBM rate; 288 GB leaves room for a full
  copy of even the Llama-3-8B per-rank shard), then the C++ engine drains them through a
  bounded pinned ring on its own copy stream to writer threads.  Training continues at once;
  stream order protects the snapshot from the next optimizer step - no fence needed.
* **Restore reads each byte once.**  Items are assigned to reader ranks (balanced), read
  with parallel pread into pinned memory, copied H2D and broadcast over RCCL/xGMI, instead
  of every rank reading the whole checkpoint.  Works across world sizes (resharding).
"""
from __future__ import annotations

import dataclasses
import io
import os
import pickle
import struct
import threading
import time
import uuid

import torch
import torch.distributed as dist
from torch.distributed.checkpoint._nested_dict import flatten_state_dict
from torch.distributed.checkpoint.filesystem import _StorageInfo
from torch.distributed.checkpoint.metadata import (BytesStorageMetadata, ChunkStorageMetadata, Metadata,
                                                   MetadataIndex, StorageMeta, TensorProperties,
                                                   TensorStorageMetadata)

from ..ops import _ext
from . import snapshot, torchsave

METADATA_FN = ".metadata"
DCP_VERSION = "1.0.0"


# ------------------------------------------------------------------------------ helpers
def _world(pg=None):
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(pg), dist.get_rank(pg)
    return 1, 0


def _resolve_stateful(state_dict: dict) -> dict:
    out = {}
    for k, v in state_dict.items():
        if hasattr(v, "state_dict") and callable(v.state_dict) and not torch.is_tensor(v):
            out[k] = v.state_dict()
        else:
            out[k] = v
    return out


def _bytes_of(obj) -> bytes:
    buf = io.BytesIO()
    torch.save(obj, buf)
    return buf.getvalue()


def _balanced_owner(items: list[tuple[str, int]], world: int) -> dict[str, int]:
    """Deterministic greedy bin packing by bytes (largest first, ties by fqn)."""
    load = [0] * world
    owner = {}
    for fqn, n in sorted(items, key=lambda x: (-x[1], x[0])):
        r = min(range(world), key=lambda i: (load[i], i))
        owner[fqn] = r
        load[r] += max(n, 1)
    return owner


_pkl_cache: dict = {}


def _shape_tensor(dtype, shape):
    return torch.empty(shape, dtype=dtype, device="meta")


def _pkl_for(dtype, shape) -> bytes:
    key = (dtype, tuple(shape))
    v = _pkl_cache.get(key)
    if v is None:
        v, _ = torchsave.pickle_state(_shape_tensor(dtype, shape))
        _pkl_cache[key] = v
    return v


# ------------------------------------------------------------------------------ save
@dataclasses.dataclass
class _Item:
    fqn: str
    kind: str  # "tensor" | "bytes"
    nbytes: int
    tensor: torch.Tensor | None = None
    data: bytes | None = None
    chunk: tuple | None = None        # (offsets, sizes, global shape) of a shard of a sharded value
    owner: int | None = None          # writer rank fixed by the value's layout (sharded values)


def _collect(state_dict, world: int = 1, rank: int = 0):
    """Flatten a state dict into write items.  Replicated tensors / bytes get their owner from
    the balanced plan later; `FlatShardedTensor` values (ZeRO-1 optimizer state) expand into
    one item per hyper-rectangular piece of every rank's flat ranges, owned by that rank -
    other ranks' pieces carry meta tensors (shape + dtype are all the file layout needs)."""
    from .sharded import FlatShardedTensor

    sd = _resolve_stateful(state_dict)
    flat, mapping = flatten_state_dict(sd)
    items = []
    for fqn, v in flat.items():
        if isinstance(v, FlatShardedTensor):
            if v.world != world:
                raise ValueError(f"{fqn}: sharded over {v.world} ranks but saving with world size {world}")
            esz = torch.empty((), dtype=v.dtype).element_size()
            mine = {tuple(off): t for off, _sz, t in v.local_piece_tensors()}
            for r in range(world):
                for off, sz, _fs, n in v.pieces_of(r):
                    t = mine[tuple(off)].detach() if r == rank else torch.empty(sz, dtype=v.dtype, device="meta")
                    items.append(_Item(fqn, "tensor", n * esz, tensor=t, chunk=(tuple(off), tuple(sz), tuple(v.shape)),
                                       owner=r))
        elif torch.is_tensor(v):
            t = v.detach()
            items.append(_Item(fqn, "tensor", t.numel() * t.element_size(), tensor=t))
        else:
            b = _bytes_of(v)
            items.append(_Item(fqn, "bytes", len(b), data=b))
    return items, mapping


def _archives_for(items: list[_Item], with_ptrs: bool):
    arcs = []
    for it in items:
        if it.kind == "tensor":
            t = it.tensor
            ptr = t.data_ptr() if with_ptrs else 1
            if it.nbytes == 0:
                arcs.append((False, torchsave.build_records(_pkl_for(t.dtype, t.shape), [(0, 0, False)])))
            else:
                arcs.append((False, torchsave.build_records(_pkl_for(t.dtype, t.shape),
                                                            [(ptr, it.nbytes, t.is_cuda and with_ptrs)])))
        else:
            arcs.append((True, [("bytes", it.data, 0, 0, False)]))
    return arcs


class AsyncSave:
    """Handle of an in-flight sharded save on this rank."""

    def __init__(self, checkpoint_id, handle, metadata, rank, t_start, t_return, nbytes, pg):
        self.checkpoint_id, self._h, self._metadata = checkpoint_id, handle, metadata
        self.rank, self.t_start, self.t_return, self.nbytes, self.pg = rank, t_start, t_return, nbytes, pg
        self.write_s = None
        self.d2h_s = None  # seconds until the snapshot's last byte reached the pinned ring
        self._h_timings = getattr(handle, "d2h_seconds", None)
        self._lease = None
        self._error: BaseException | None = None
        # waited on by the training loop and by the session's committer thread
        self._lock = threading.Lock()

    def wait(self) -> float:
        """Local shard durable.  Returns seconds since the save call.  The outcome is cached
        under a lock: concurrent and repeated waiters all get the same result, and a failed
        write (or verify) raises for every one of them."""
        with self._lock:
            if self._error is None and self.write_s is None:
                try:
                    if self._h is not None:
                        self._h.wait()  # raises CommPoisonedError from the words captured at the snapshot
                    from ..parallel import health

                    if health.poisoned(getattr(self, "_words", None)):  # (also when this rank wrote nothing)
                        raise health.CommPoisonedError(
                            "refusing checkpoint commit: a P2P gradient all-reduce timed out before the snapshot")
                    if getattr(self, "_verify", None):
                        _verify_written(self._verify)
                        self._verify = None
                    self._lease = None
                    self.write_s = time.perf_counter() - self.t_start
                    if self._h_timings is not None:
                        self.d2h_s = self._h_timings()
                except BaseException as e:  # noqa: BLE001
                    self._error = e
                finally:
                    self._h = None
                    self._lease = None
            if self._error is not None:
                from ..parallel.health import CommPoisonedError

                if isinstance(self._error, CommPoisonedError):
                    raise CommPoisonedError(str(self._error)) from self._error
                raise IOError(f"sharded save to {self.checkpoint_id} failed: {self._error}") from self._error
            return self.write_s

    def _finish(self):
        """Rank 0 (or a simulated rank): write `.metadata` atomically (call after every rank's
        wait())."""
        if self._metadata is not None:
            write_metadata(self.checkpoint_id, self._metadata)

    def result(self):
        """wait + barrier + metadata commit + barrier (collective on `pg`)."""
        self.wait()
        w, _ = _world(self.pg)
        if w > 1:
            dist.barrier(group=self.pg)
        self._finish()
        if w > 1:
            dist.barrier(group=self.pg)
        return self


def _verify_written(entries) -> None:
    """RTDC_CKPT_VERIFY=1 debug mode: read every tensor record this rank wrote
    back from disk and compare it byte for byte with the snapshot that was staged."""
    for path, base, size, t in entries:
        off, n = _zip_data_record(path, base, size)
        with open(path, "rb") as f:
            f.seek(off)
            disk = f.read(n)
        host = t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy().tobytes()
        if disk != host:
            raise IOError(f"checkpoint verify failed: {path}@{off} ({n} bytes) differs from the staged tensor")


def write_metadata(checkpoint_id: str, md: Metadata):
    tmp = os.path.join(checkpoint_id, METADATA_FN + ".tmp")
    with open(tmp, "wb") as f:
        pickle.dump(md, f)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, os.path.join(checkpoint_id, METADATA_FN))
    from ..train.storage import fsync_dir

    fsync_dir(checkpoint_id)


SIMULATED_TAG = "rtdc:simulated"  # StorageMeta.modules marker of a simulated (one-rank) save


def _simulated(simulate):
    """(world, rank) this process plays in a SIMULATED multi-rank save/load, or None.
    `simulate=(W, r)`: plan exactly as rank r of a W-rank data-parallel job (owner plan, file
    layout, `.metadata` for all W ranks) but write / read only rank r's share, with no
    collectives - how one GPU measures a per-rank shard of an 8-GPU job (e.g. Llama-3-8B's
    ~12 GB train-state shard).  The result on disk is one rank's file plus the full metadata: a
    measurement artifact, not a restorable checkpoint, so its metadata carries SIMULATED_TAG
    and a non-simulated load refuses it.  Only the explicit argument enables this (an
    environment switch could silently turn a trainer's real checkpoints into artifacts)."""
    if simulate is None:
        return None
    w, r = int(simulate[0]), int(simulate[1])
    if not (0 <= r < w):
        raise ValueError(f"simulate=({w}, {r}): rank out of range")
    if _world(None)[0] != 1:
        raise ValueError("a simulated multi-rank save/load runs in a single process (no process group)")
    return w, r


def _merge_rank_metadata(metadata: Metadata, parts: list) -> None:
    """Fold the other ranks' metadata of a non-replicated save into rank 0's.  A key present on
    several ranks (a FlatShardedTensor: one TensorStorageMetadata per rank, each listing that
    rank's chunks) gets the union of their chunk lists, and its storage entries are re-indexed
    to the merged list - a plain dict.update would keep only the last rank's chunks while the
    storage entries of every rank survive, and a load would then miss chunk sizes."""
    sd_md, storage = metadata.state_dict_metadata, metadata.storage_data
    for p in parts:
        for fqn, m in p.state_dict_metadata.items():
            mine = sd_md.get(fqn)
            if mine is None:
                sd_md[fqn] = m
                remap = {i: i for i in range(len(getattr(m, "chunks", []) or []))}
            elif isinstance(m, TensorStorageMetadata) and isinstance(mine, TensorStorageMetadata):
                if tuple(mine.size) != tuple(m.size):
                    raise ValueError(f"{fqn}: ranks disagree on the global shape ({tuple(mine.size)} vs {tuple(m.size)})")
                remap = {}
                for i, c in enumerate(m.chunks):
                    remap[i] = len(mine.chunks)
                    mine.chunks.append(c)
            else:
                raise ValueError(f"{fqn}: saved by several ranks with replicated=False but is not a sharded tensor")
            for idx, info in p.storage_data.items():
                if idx.fqn != fqn:
                    continue
                i = remap.get(idx.index, idx.index) if idx.index is not None else None
                storage[MetadataIndex(fqn, idx.offset, i)] = info
        for idx, info in p.storage_data.items():
            if idx.fqn not in p.state_dict_metadata:
                storage[idx] = info
        metadata.planner_data.update(p.planner_data)


def _plan_save(state_dict, process_group, replicated, sim):
    """(world, rank, items, flatten mapping, {rank: owned items}) of a save - deterministic on
    every rank, no collectives."""
    world, rank = sim if sim else _world(process_group)
    items, mapping = _collect(state_dict, world, rank)
    rep = [it for it in items if it.owner is None]
    if replicated:
        owner = _balanced_owner([(it.fqn, it.nbytes) for it in rep], world)
    else:
        # per-rank state (e.g. per-rank shards): every rank writes its own items; fqns must be unique
        owner = {it.fqn: rank for it in rep}
    for it in rep:
        it.owner = owner[it.fqn]
    per_rank: dict[int, list[_Item]] = {r: [] for r in range(world)}
    for it in items:
        per_rank[it.owner].append(it)
    return world, rank, items, mapping, per_rank


def prepare_async(state_dict: dict, process_group=None, *, replicated: bool = True, simulate=None) -> int:
    """Startup-time allocation for async saves of `state_dict`-shaped state: the native engine
    (pinned ring, writer threads) and this rank's HBM snapshot arena, so that the first
    checkpoint of a run allocates nothing between two training steps (a trainer calls this
    once; the session does for its registered state).  Returns the arena bytes."""
    sim = _simulated(simulate)
    _w, rank, _items, _m, per_rank = _plan_save(state_dict, process_group, replicated, sim)
    torchsave.get_engine()
    return snapshot.reserve([it.tensor for it in per_rank[rank] if it.kind == "tensor"])


def async_save(state_dict: dict, checkpoint_id: str, process_group=None, *, fsync: bool = True,
               crc: bool = True, replicated: bool = True, simulate=None) -> AsyncSave:
    """Start a sharded save; returns once the HBM snapshot is enqueued (non-blocking).
    `simulate=(W, r)`: see `_simulated`."""
    t0 = time.perf_counter()
    from ..parallel import health

    # a timed-out P2P collective left NaN gradients behind: never snapshot that state.  No
    # device sync here (that would drain the compute stream on the non-blocking path): the
    # communicators' words are also captured right after the snapshot copies, in stream order,
    # and wait() decides commit-or-refuse from that captured value (not the live sticky word)
    health.assert_healthy("checkpoint save", sync=False)
    sim = _simulated(simulate)
    world, rank, items, mapping, per_rank = _plan_save(state_dict, process_group, replicated, sim)
    os.makedirs(checkpoint_id, exist_ok=True)
    mine = per_rank[rank]
    # HBM / host snapshot of owned tensors, in stream order on the compute stream: into a
    # reused arena, one copy per flat storage (checkpoint/snapshot.py)
    owned_t = [it for it in mine if it.kind == "tensor"]
    lease, snaps = snapshot.take([it.tensor for it in owned_t])
    for it, t in zip(owned_t, snaps):
        it.tensor = t
    words = health.capture_error_words()
    ready = None
    if any(it.kind == "tensor" and it.tensor.is_cuda for it in mine):
        ready = torch.cuda.Event()
        ready.record()
    ext = _ext.ext()
    # this rank's records, built once: the engine writes them and - the layout depends on record
    # names and sizes only - they also plan this rank's file for the metadata and the verify pass
    arcs_mine = _archives_for(mine, with_ptrs=True) if mine else []
    lay_mine = None
    metadata = None
    if rank == 0 or not replicated or sim:
        sd_md = {}
        storage = {}
        ranks = range(world) if replicated else [rank]
        for r in ranks:
            fname = f"__{r}_0.distcp"
            if r == rank:
                _, lay = lay_mine = ext.plan_layout(arcs_mine)
            else:
                _, lay = ext.plan_layout(_archives_for(per_rank[r], with_ptrs=False))
            for it, (base, size, _recs) in zip(per_rank[r], lay):
                if it.kind == "tensor" and it.chunk is not None:
                    offs, sizes, gshape = it.chunk
                    m = sd_md.get(it.fqn)
                    if m is None:
                        m = sd_md[it.fqn] = TensorStorageMetadata(
                            properties=TensorProperties(dtype=it.tensor.dtype), size=torch.Size(gshape), chunks=[])
                    storage[MetadataIndex(it.fqn, torch.Size(offs), len(m.chunks))] = _StorageInfo(fname, base, size)
                    m.chunks.append(ChunkStorageMetadata(offsets=torch.Size(offs), sizes=torch.Size(sizes)))
                elif it.kind == "tensor":
                    t = it.tensor
                    zeros = torch.Size([0] * t.dim())
                    sd_md[it.fqn] = TensorStorageMetadata(
                        properties=TensorProperties(dtype=t.dtype), size=torch.Size(t.shape),
                        chunks=[ChunkStorageMetadata(offsets=zeros, sizes=torch.Size(t.shape))])
                    storage[MetadataIndex(it.fqn, zeros, 0)] = _StorageInfo(fname, base, size)
                else:
                    sd_md[it.fqn] = BytesStorageMetadata()
                    storage[MetadataIndex(it.fqn)] = _StorageInfo(fname, base, size)
        metadata = Metadata(state_dict_metadata=sd_md, planner_data=mapping, storage_data=storage,
                            storage_meta=StorageMeta(checkpoint_id=checkpoint_id, save_id=str(uuid.uuid4()),
                                                     modules=[SIMULATED_TAG] if sim else []),
                            version=DCP_VERSION)
        if not replicated and world > 1 and not sim:
            # gather per-rank metadata on rank 0 (CPU object collective)
            parts = [None] * world
            dist.all_gather_object(parts, metadata, group=process_group)
            if rank == 0:
                _merge_rank_metadata(metadata, parts[1:])
            else:
                metadata = None
    elif not replicated and world > 1:
        pass
    handle = None
    nbytes = sum(it.nbytes for it in mine)
    verify = []
    if mine:
        path = os.path.join(checkpoint_id, f"__{rank}_0.distcp")
        handle = torchsave.submit_files([(path, fsync, crc, arcs_mine)],
                                        [lease] + [it.tensor for it in mine if it.tensor is not None], nbytes, ready,
                                        words)
        if os.environ.get("RTDC_CKPT_VERIFY", "0") == "1":
            _, lay = lay_mine or ext.plan_layout(arcs_mine)
            verify = [(path, base, size, it.tensor) for it, (base, size, _r) in zip(mine, lay) if it.kind == "tensor"]
    h = AsyncSave(checkpoint_id, handle, metadata, rank, t0, time.perf_counter() - t0, nbytes, process_group)
    h._verify = verify
    h._words = words
    h._lease = lease if verify else None  # the verify pass reads the snapshot after the drain
    return h


def save(state_dict: dict, checkpoint_id: str, process_group=None, **kw) -> AsyncSave:
    """Blocking sharded save (collective): returns after `.metadata` is committed."""
    return async_save(state_dict, checkpoint_id, process_group, **kw).result()


# ------------------------------------------------------------------------------ load
class _SafeUnpickler(pickle.Unpickler):
    """Only the DCP metadata dataclasses and torch/builtin value types - no arbitrary code."""

    _ALLOWED = {
        ("torch.distributed.checkpoint.metadata", n) for n in (
            "Metadata", "MetadataIndex", "TensorStorageMetadata", "BytesStorageMetadata", "ChunkStorageMetadata",
            "TensorProperties", "StorageMeta", "_MEM_FORMAT_ENCODING")
    } | {("torch.distributed.checkpoint.filesystem", "_StorageInfo"), ("torch", "Size"), ("torch", "strided"),
         ("collections", "OrderedDict"), ("pathlib", "PosixPath"), ("torch", "device"),
         ("torch.serialization", "_get_layout"),
         ("torch.distributed.checkpoint._extension", "StreamTransformExtension")}

    def find_class(self, module, name):
        if (module, name) in self._ALLOWED:
            return super().find_class(module, name)
        if module == "torch" and isinstance(getattr(torch, name, None), torch.dtype):
            return getattr(torch, name)
        if module == "torch" and name in ("layout",):
            return getattr(torch, name)
        raise pickle.UnpicklingError(f"disallowed global in checkpoint metadata: {module}.{name}")


def read_metadata(checkpoint_id: str) -> Metadata:
    with open(os.path.join(checkpoint_id, METADATA_FN), "rb") as f:
        return _SafeUnpickler(f).load()


def _zip_data_record(path: str, base: int, length: int, f=None) -> tuple[int, int]:
    """(absolute data offset, size) of the tensor record '<prefix>/data/0' in a zip slice.
    Handles ZIP64 (records >= 4 GiB, offsets past 4 GiB, zip64 end-of-central-directory).
    Reads only the archive's tail (a one-tensor archive's central directory is < 1 KiB) and
    the record's local header; pass an open file `f` to reuse it across items."""
    if f is None:
        with open(path, "rb") as fh:
            return _zip_data_record(path, base, length, fh)
    tail = b""
    for tail_len in (min(length, 2048), min(length, 1 << 16)):
        f.seek(base + length - tail_len)
        tail = f.read(tail_len)
        eocd = tail.rfind(b"PK\x05\x06")
        if eocd >= 0:
            n_, cd_size_, cd_off_ = struct.unpack("<HII", tail[eocd + 10:eocd + 20])
            z64 = n_ == 0xFFFF or cd_size_ == 0xFFFFFFFF or cd_off_ == 0xFFFFFFFF
            if z64 or cd_off_ >= length - tail_len:  # central directory inside what was read
                break
    if eocd < 0:
        raise IOError(f"{path}@{base}: no zip end record")
    n, cd_size, cd_off = struct.unpack("<HII", tail[eocd + 10:eocd + 20])
    if n == 0xFFFF or cd_size == 0xFFFFFFFF or cd_off == 0xFFFFFFFF:
        loc = eocd - 20
        if loc < 0 or tail[loc:loc + 4] != b"PK\x06\x07":
            raise IOError(f"{path}@{base}: zip64 locator missing")
        (z64_off,) = struct.unpack("<Q", tail[loc + 8:loc + 16])
        f.seek(base + z64_off)
        rec = f.read(56)
        if rec[:4] != b"PK\x06\x06":
            raise IOError(f"{path}@{base}: bad zip64 end record")
        n, _n2, cd_size, cd_off = struct.unpack("<QQQQ", rec[24:56])
    if cd_off >= length - len(tail):
        cd = tail[cd_off - (length - len(tail)):cd_off - (length - len(tail)) + cd_size]
    else:
        f.seek(base + cd_off)
        cd = f.read(cd_size)
    pos = 0
    for _ in range(n):
        (sig,) = struct.unpack("<I", cd[pos:pos + 4])
        if sig != 0x02014B50:
            raise IOError(f"{path}@{base}: corrupt central directory")
        csize, usize = struct.unpack("<II", cd[pos + 20:pos + 28])
        nlen, elen, clen = struct.unpack("<HHH", cd[pos + 28:pos + 34])
        lho, = struct.unpack("<I", cd[pos + 42:pos + 46])
        name = cd[pos + 46:pos + 46 + nlen].decode()
        if name.endswith("/data/0"):
            if 0xFFFFFFFF in (csize, usize, lho):
                extra = cd[pos + 46 + nlen:pos + 46 + nlen + elen]
                e = 0
                while e + 4 <= len(extra):
                    tag, sz = struct.unpack("<HH", extra[e:e + 4])
                    if tag == 1:
                        vals = list(struct.unpack("<" + "Q" * (sz // 8), extra[e + 4:e + 4 + sz]))
                        if usize == 0xFFFFFFFF:
                            usize = vals.pop(0)
                        if csize == 0xFFFFFFFF:
                            csize = vals.pop(0)
                        if lho == 0xFFFFFFFF:
                            lho = vals.pop(0)
                        break
                    e += 4 + sz
            f.seek(base + lho)
            lh = f.read(30)
            lnlen, lelen = struct.unpack("<HH", lh[26:30])
            return base + lho + 30 + lnlen + lelen, csize
        pos += 46 + nlen + elen + clen
    raise IOError(f"{path}@{base}: no tensor data record")


def _data_records(items, threads: int = 8) -> list[tuple[int, int]]:
    """(data offset, size) of the tensor record of each (path, base, length) zip slice, in
    order: one native call per file (csrc/runtime/ckpt_engine.cpp zip_data_records - parallel
    preads, no per-item Python I/O).  RTDC_ZIP_PARSE=py keeps the Python parser (A/B)."""
    out: list = [None] * len(items)
    if os.environ.get("RTDC_ZIP_PARSE", "native") == "py":
        handles: dict = {}
        try:
            for i, (path, base, length) in enumerate(items):
                fh = handles.get(path)
                if fh is None:
                    fh = handles[path] = open(path, "rb", buffering=0)
                out[i] = _zip_data_record(path, base, length, fh)
        finally:
            for fh in handles.values():
                fh.close()
        return out
    by_path: dict[str, list[int]] = {}
    for i, (path, _b, _l) in enumerate(items):
        by_path.setdefault(path, []).append(i)
    ext = _ext.ext()
    for path, ids in by_path.items():
        res = ext.zip_data_records(path, [items[i][1] for i in ids], [items[i][2] for i in ids], threads)
        for i, r in zip(ids, res):
            out[i] = (int(r[0]), int(r[1]))
    return out


def _pinned(n: int) -> torch.Tensor:
    t = torch.empty(n, dtype=torch.uint8)
    if torch.cuda.is_available():
        t = t.pin_memory()
    return t


def load(state_dict: dict, checkpoint_id: str, process_group=None, *, broadcast: bool = True,
         pinned_mb: int = 1024, threads: int = 8, simulate=None) -> dict:
    """Load a DCP-format checkpoint IN PLACE into `state_dict` (tensors copied into, Stateful
    objects get load_state_dict).  Collective when a process group is initialised.
    Reader plan: a checkpoint saved by the same number of ranks is read back by its writers
    (each rank reads the file it wrote - no cross-rank file access, page-cache local);
    otherwise readers are balanced by bytes.  Every tensor is then broadcast from its reader
    (coalesced).  `simulate=(W, r)`: read only rank r's share of a W-rank plan, no collectives."""
    sim = _simulated(simulate)
    world, rank = sim if sim else _world(process_group)
    md = read_metadata(checkpoint_id)
    sm = getattr(md, "storage_meta", None)
    if not sim and sm is not None and SIMULATED_TAG in (getattr(sm, "modules", None) or []):
        # a simulated save writes one rank's file: restorable only once every rank's file exists
        missing_files = sorted({i.relative_path for i in md.storage_data.values()
                                if not os.path.exists(os.path.join(checkpoint_id, i.relative_path))})
        if missing_files:
            raise ValueError(f"{checkpoint_id} is a simulated one-rank measurement artifact (saved with simulate=...): "
                             f"{len(missing_files)} rank file(s) such as {missing_files[0]} were never written, so it "
                             "cannot be restored")
    resolved = _resolve_stateful(state_dict)
    flat, mapping = flatten_state_dict(resolved)
    ext = _ext.ext()
    # index storage entries per fqn
    chunks_of: dict[str, list] = {}
    for idx, info in md.storage_data.items():
        chunks_of.setdefault(idx.fqn, []).append((idx, info))
    tensor_fqns = [k for k, v in flat.items() if torch.is_tensor(v)]
    missing = [k for k in flat if k not in md.state_dict_metadata]
    if missing:
        raise KeyError(f"checkpoint {checkpoint_id} is missing keys: {missing[:5]}{'...' if len(missing) > 5 else ''}")
    from .sharded import FlatShardedTensor

    sharded_fqns = [k for k, v in flat.items() if isinstance(v, FlatShardedTensor)]
    if sharded_fqns:
        # every rank reads exactly the bytes of its own shards (no broadcast, any saved layout)
        _load_sharded(flat, sharded_fqns, md, chunks_of, checkpoint_id, ext, threads)
    sizes = []
    for k in tensor_fqns:
        m = md.state_dict_metadata[k]
        n = 1
        for s in m.size:
            n *= s
        sizes.append((k, n * flat[k].element_size()))
    reader = _reader_plan(md, chunks_of, sizes, world) if broadcast else {k: rank for k in tensor_fqns}
    my = [k for k in tensor_fqns if reader[k] == rank]
    # ---- read my items: (dest tensor, chunk offsets, chunk sizes, file, data offset, nbytes)
    reqs = []
    need = []
    for k in my:
        dest = flat[k]
        mdt = md.state_dict_metadata[k]
        if tuple(mdt.size) != tuple(dest.shape):
            raise ValueError(f"{k}: checkpoint shape {tuple(mdt.size)} != destination {tuple(dest.shape)}")
        if mdt.properties.dtype != dest.dtype:  # (never cast or reinterpret: e.g. bf16 optimizer state)
            raise ValueError(f"{k}: checkpoint dtype {mdt.properties.dtype} != destination {dest.dtype}")
        for idx, info in chunks_of[k]:
            need.append((k, idx, info, os.path.join(checkpoint_id, info.relative_path)))
    recs = _data_records([(path, info.offset, info.length) for _k, _i, info, path in need], threads)
    for (k, idx, info, path), (off, n) in zip(need, recs):
        dest = flat[k]
        mdt = md.state_dict_metadata[k]
        csizes = None
        for c in mdt.chunks:
            if tuple(c.offsets) == tuple(idx.offset):
                csizes = tuple(c.sizes)
        reqs.append((dest, tuple(idx.offset), csizes or tuple(dest.shape), path, off, n, mdt.properties.dtype))
    # device destinations whose region is one contiguous run of the same dtype stream straight
    # from the file: native pread -> pinned ring -> H2D on the engine's copy stream, pipelined
    # (torchsave.get_engine().read_to_device); anything else (host destinations, resharded
    # chunks) goes through a pinned staging buffer + copy_
    direct: dict[str, tuple[list, list, list]] = {}
    staged = []
    for r in reqs:
        dest, offs, csz, path, off, n, dt = r
        region = dest
        for dim, (o, sz) in enumerate(zip(offs, csz)):
            region = region.narrow(dim, o, sz)
        if (dest.is_cuda and region.is_contiguous() and region.dtype == dt
                and region.numel() * region.element_size() == n and torch.cuda.is_available()):
            o_, l_, d_ = direct.setdefault(path, ([], [], []))
            o_.append(off)
            l_.append(n)
            d_.append(region.data_ptr())
        else:
            staged.append(r)
    if direct:
        from . import torchsave

        eng = torchsave.get_engine()
        torch.cuda.current_stream().synchronize()  # destinations may still be read by queued kernels
        for path, (o, l, d) in direct.items():
            eng.read_to_device(path, o, l, d, threads)
    reqs = staged
    # batched: parallel pread into a pinned buffer, then copy into the destination
    cap = max(pinned_mb << 20, max([r[5] for r in reqs], default=0))
    staging = _pinned(min(cap, sum(r[5] for r in reqs))) if reqs else None
    i = 0
    while i < len(reqs):
        batch, used = [], 0
        while i < len(reqs) and (not batch or used + reqs[i][5] <= cap):
            batch.append((reqs[i], used))
            used += reqs[i][5]
            i += 1
        by_file: dict[str, tuple[list, list, list]] = {}
        base_ptr = staging.data_ptr()
        for (dest, offs, csz, path, off, n, dt), at in batch:
            o, l, d = by_file.setdefault(path, ([], [], []))
            o.append(off)
            l.append(n)
            d.append(base_ptr + at)
        for path, (o, l, d) in by_file.items():
            ext.read_ranges(path, o, l, d, threads)
        for (dest, offs, csz, path, off, n, dt), at in batch:
            src = staging[at:at + n].view(dt).view(csz)
            region = dest
            for dim, (o, s_) in enumerate(zip(offs, csz)):
                region = region.narrow(dim, o, s_)
            with torch.no_grad():
                region.copy_(src, non_blocking=dest.is_cuda)
        if dest_is_cuda(batch):
            torch.cuda.current_stream().synchronize()  # staging reuse
    # ---- broadcast from readers, coalesced: each reader's tensors packed into <= 256 MB flat
    # buffers per dtype (GPT-2's train state: ~450 per-tensor broadcasts -> a handful)
    if broadcast and world > 1 and not sim:
        _coalesced_broadcast([(flat[k], reader[k]) for k in tensor_fqns], world, process_group)
    # ---- non-tensor values (rank 0 reads, broadcasts as objects)
    obj_keys = [k for k in flat if not torch.is_tensor(flat[k]) and not isinstance(flat[k], FlatShardedTensor)]
    values = {}
    if obj_keys:
        if rank == 0 or not broadcast or sim:
            for k in obj_keys:
                (idx, info), = chunks_of[k]
                if sim and not os.path.exists(os.path.join(checkpoint_id, info.relative_path)):
                    continue  # another simulated rank's file
                with open(os.path.join(checkpoint_id, info.relative_path), "rb") as f:
                    f.seek(info.offset)
                    values[k] = torch.load(io.BytesIO(f.read(info.length)), weights_only=True)
        if broadcast and world > 1 and not sim:
            box = [values]
            dist.broadcast_object_list(box, src=_global_rank(0, process_group), group=process_group)
            values = box[0]
    for k, v in values.items():
        _set_path(resolved, mapping[k], v)
    # Stateful objects
    for key, v in state_dict.items():
        if hasattr(v, "load_state_dict") and not torch.is_tensor(v):
            v.load_state_dict(resolved[key])
        else:
            state_dict[key] = resolved[key]
    if flat and any(torch.is_tensor(v) and v.is_cuda for v in flat.values()):
        torch.cuda.current_stream().synchronize()
    return state_dict


def _load_sharded(flat, fqns, md, chunks_of, checkpoint_id, ext, threads) -> None:
    """Fill each FlatShardedTensor's local slices from the saved chunks that intersect them.
    Saved chunks must be contiguous in row-major order (a whole tensor, or the pieces a
    sharded save writes); the intersection is one byte range of the chunk's data record."""
    from .sharded import chunk_flat_range

    dev_reads: dict[str, tuple[list, list, list]] = {}
    host_reads: dict[str, tuple[list, list, list]] = {}
    # pass 1: the (chunk, local slice) intersections; pass 2 reads the data records they need
    hits = []  # (path, info, [(dst tensor, byte offset in the record, bytes)])
    for k in fqns:
        v = flat[k]
        mdt = md.state_dict_metadata[k]
        if tuple(mdt.size) != tuple(v.shape):
            raise ValueError(f"{k}: checkpoint shape {tuple(mdt.size)} != destination {tuple(v.shape)}")
        if mdt.properties.dtype != v.dtype:
            raise ValueError(f"{k}: checkpoint dtype {mdt.properties.dtype} != destination {v.dtype}")
        esz = torch.empty((), dtype=v.dtype).element_size()
        sizes_of = {tuple(c.offsets): tuple(c.sizes) for c in mdt.chunks}
        covered = 0
        for idx, info in chunks_of[k]:
            fr = chunk_flat_range(idx.offset, sizes_of[tuple(idx.offset)], v.shape)
            if fr is None:
                raise ValueError(f"{k}: chunk at {tuple(idx.offset)} is not contiguous in row-major order; a "
                                 f"flat-sharded destination cannot read it")
            cs, cn = fr
            parts = []
            for s0, t in v.local:
                lo, hi = max(s0, cs), min(s0 + t.numel(), cs + cn)
                if lo >= hi:
                    continue
                parts.append((t[lo - s0:hi - s0], (lo - cs) * esz, (hi - lo) * esz))
                covered += hi - lo
            if parts:
                hits.append((os.path.join(checkpoint_id, info.relative_path), info, parts))
        if covered != v.local_numel():
            raise ValueError(f"{k}: checkpoint chunks cover {covered} of this rank's {v.local_numel()} elements")
    recs = _data_records([(path, info.offset, info.length) for path, info, _p in hits], threads)
    for (path, _info, parts), rec in zip(hits, recs):
        for dst, at, nb in parts:
            group = dev_reads if (dst.is_cuda and torch.cuda.is_available()) else host_reads
            o, l_, d = group.setdefault(path, ([], [], []))
            o.append(rec[0] + at)
            l_.append(nb)
            d.append(dst.data_ptr())
    if dev_reads:
        from . import torchsave

        eng = torchsave.get_engine()
        torch.cuda.current_stream().synchronize()
        for path, (o, l_, d) in dev_reads.items():
            eng.read_to_device(path, o, l_, d, threads)
    for path, (o, l_, d) in host_reads.items():
        ext.read_ranges(path, o, l_, d, threads)


def _reader_plan(md, chunks_of, sizes, world) -> dict:
    """fqn -> reader rank.  Same world as the save: the rank whose file holds the tensor (its
    writer); otherwise (or for multi-file tensors) byte-balanced."""
    import re

    files = {info.relative_path for info in md.storage_data.values()}
    ranks = {int(m.group(1)) for f in files for m in [re.match(r"__(\d+)_\d+\.distcp$", f)] if m}
    if ranks and max(ranks) + 1 == world:
        out, rest = {}, []
        for k, n in sizes:
            fs = {info.relative_path for _idx, info in chunks_of[k]}
            m = re.match(r"__(\d+)_\d+\.distcp$", next(iter(fs))) if len(fs) == 1 else None
            if m:
                out[k] = int(m.group(1))
            else:
                rest.append((k, n))
        out.update(_balanced_owner(rest, world) if rest else {})
        return out
    return _balanced_owner(sizes, world)


BCAST_CAP_BYTES = 256 << 20


def _coalesced_broadcast(pairs, world, pg, cap: int = BCAST_CAP_BYTES) -> int:
    """Broadcast each tensor from its reader rank, packing the tensors of one (reader, dtype,
    device) into flat buffers of at most `cap` bytes (one collective each; tensors larger than
    `cap` go alone, in place).  Order is identical on every rank.  Returns the number of
    collectives issued."""
    n_coll = 0
    for src in range(world):
        groups: dict = {}
        for t, r in pairs:
            if r == src:
                groups.setdefault((t.dtype, t.device), []).append(t)
        g_src = _global_rank(src, pg)
        me = dist.get_rank(pg)
        for (dtype, device), ts in groups.items():
            esz = torch.empty((), dtype=dtype).element_size()
            batch, used = [], 0

            def flush(batch):
                if not batch:
                    return 0
                if len(batch) == 1 and batch[0].is_contiguous():
                    dist.broadcast(batch[0], src=g_src, group=pg)
                    return 1
                total = sum(x.numel() for x in batch)
                buf = torch.empty(total, dtype=dtype, device=device)
                if me == src:
                    off = 0
                    with torch.no_grad():
                        for x in batch:
                            buf[off:off + x.numel()].copy_(x.reshape(-1))
                            off += x.numel()
                dist.broadcast(buf, src=g_src, group=pg)
                if me != src:
                    off = 0
                    with torch.no_grad():
                        for x in batch:
                            x.copy_(buf[off:off + x.numel()].view(x.shape))
                            off += x.numel()
                return 1

            for t in ts:
                nb = t.numel() * esz
                if nb >= cap:
                    if t.is_contiguous():
                        dist.broadcast(t, src=g_src, group=pg)
                    else:
                        tmp = t.contiguous()
                        dist.broadcast(tmp, src=g_src, group=pg)
                        if me != src:
                            with torch.no_grad():
                                t.copy_(tmp)
                    n_coll += 1
                    continue
                if used + nb > cap:
                    n_coll += flush(batch)
                    batch, used = [], 0
                batch.append(t)
                used += nb
            n_coll += flush(batch)
    global LAST_LOAD_COLLECTIVES
    LAST_LOAD_COLLECTIVES = n_coll
    return n_coll


LAST_LOAD_COLLECTIVES = 0


def dest_is_cuda(batch) -> bool:
    return any(b[0][0].is_cuda for b in batch)


def _global_rank(group_rank: int, pg) -> int:
    if pg is None:
        return group_rank
    return dist.get_global_rank(pg, group_rank)


def _set_path(root, path, value):
    cur = root
    for p in path[:-1]:
        cur = cur[p]
    cur[path[-1]] = value
