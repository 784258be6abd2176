"""Global gradient-norm clipping fused into the flat optimizers (csrc/kernels/optim.hip
gradnorm_* kernels, optim/fused.py `max_grad_norm`) on the GPU.

The single-process cases run over one synthetic parameter set that reaches every kernel path:
parameters of 1, 3 and 67 elements (scalar tail, len % 4 != 0), one of 16384 + 67 (two chunks),
4200 parameters of 3 elements (more chunks than the grid: the grid-stride loop; more than 1024
partials: the finalize kernel's serial part), one parameter without a gradient, and two param
groups with different lr / weight decay.

Norm tolerance: the terms are non-negative and every element passes through fewer than 64
additions at these shapes (<= 16 per lane accumulator, 2 to combine the accumulators, 10 in
the block reduction, 5 serial + 14 in the finalize), so even an fp32 sum is within
64 x 2^-24 ~ 4e-6 relative of the exact one and the root within half that: 1e-5 relative
against the float64 norm (the kernels sum in fp64 and round once, so they are far inside it).  Fused-vs-torch is `rtol=1e-5, atol=1e-6` as in tests/test_optim.py.
"""
import copy
import os
import socket
import sys
import traceback

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

NGPU = torch.cuda.device_count() if torch.cuda.is_available() else 0
N_TINY = 4200
SIZES = [1, 3, 67, 16384 + 67] + [3] * N_TINY + [5]  # the last one never gets a gradient
SPLIT = 4  # group 0: the four odd-sized parameters; group 1: the tiny ones (one launch of > 4096 chunks)


def _build(kind, clip, seed=0):
    """(params, optimizer) over a flat space on the GPU.  Gradients are views of the flat
    gradient buffer and are set by `_set_grads`; the last parameter keeps `grad = None`."""
    from ray_torch_distributed_checkpoint_amd.optim import FlatParamSpace, FusedAdamW, FusedSGD

    g = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(n, generator=g).cuda()) for n in SIZES]
    sp = FlatParamSpace(params)
    for p in params[:-1]:
        p.grad = sp.grad_view(p)
    groups = [{"params": params[:SPLIT], "lr": 2e-3, "weight_decay": 0.0},
              {"params": params[SPLIT:], "lr": 1e-3, "weight_decay": 0.1}]
    if kind == "adamw":
        opt = FusedAdamW(groups, max_grad_norm=clip)
    else:
        opt = FusedSGD(groups, momentum=0.9, max_grad_norm=clip)
    assert opt._ensure_space() is sp  # (opt.flat_space is set from here on)
    return params, opt


def _grads(step, seed=0):
    """Per-parameter gradient values of step `step` (CPU), the same for every optimizer."""
    g = torch.Generator().manual_seed(1000 * seed + 17 + step)
    return [torch.randn(n, generator=g) * (0.5 + 0.25 * step) for n in SIZES[:-1]]


def _set_grads(params, grads):
    with torch.no_grad():
        for p, v in zip(params, grads):
            p.grad.copy_(v)
    assert params[-1].grad is None


def _ref_norm(grads) -> float:
    return float(torch.linalg.vector_norm(torch.cat(grads).double()))


def _state(params, opt):
    sp = opt.flat_space
    out = {"p": sp.data.clone(), "shadow": sp.shadow.clone()}
    for k, b in opt._bufs.items():
        out[k] = b.clone()
    return out


def _equal(a: dict, b: dict) -> bool:
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


_norm1 = {}


def _measured_norm(kind="adamw") -> float:
    """The norm the kernels report for the step-0 gradients (computed once, shared)."""
    if "v" not in _norm1:
        params, opt = _build(kind, 1e9)
        _set_grads(params, _grads(0))
        opt.step()
        _norm1["v"] = float(opt.grad_norm)
    return _norm1["v"]


def test_norm_value_and_chunk_paths():
    params, opt = _build("adamw", 1e9)
    assert opt.grad_norm is None
    gr = _grads(0)
    _set_grads(params, gr)
    opt.step()
    sp = opt.flat_space
    nchunks = [n for (_t, n) in sp._chunk_cache.values()]
    assert max(nchunks) > 4096 and sum(nchunks) == N_TINY + 5, nchunks  # grid-stride loop, finalize's serial part
    gn = opt.grad_norm
    assert gn.dim() == 0 and gn.dtype == torch.float32 and gn.is_cuda
    assert gn.data_ptr() == opt._clip_ws["out"].data_ptr()  # a view of out[0]: no copy, no sync
    ref = _ref_norm(gr)  # the gradless parameter is not part of it
    got = float(gn)
    print("grad_norm", got, "float64 reference", ref, "relative error", abs(got - ref) / ref)
    assert abs(got - ref) <= 1e-5 * ref
    assert float(opt._clip_ws["out"][1]) == 1.0  # far below max_grad_norm: coefficient exactly 1
    # p.grad is left unscaled
    assert all(torch.equal(p.grad.cpu(), v) for p, v in zip(params, gr))


def test_partial_kernel_unaligned_chunks_and_bounds():
    """Chunks cut at odd offsets (as chunk_table_splits can) take the scalar path; every chunk's
    partial equals the float64 sum of squares of exactly its elements."""
    from ray_torch_distributed_checkpoint_amd.ops._ext import gpu_ext

    g = torch.randn(70000, generator=torch.Generator().manual_seed(5)).cuda()
    rows = [(0, 5, 0), (5, 3, 0), (9, 16384, 0), (16393, 4099, 0), (20492, 1030, 0), (21524, 1, 0), (30001, 2047, 0),
            (32048, 16384, 0), (48432, 16383, 0), (64815, 5185, 0)]
    chunks = torch.tensor(rows, dtype=torch.int64).cuda()
    partial = torch.full((len(rows) + 3,), -1.0, device="cuda", dtype=torch.float64)
    gpu_ext().gradnorm_partial(chunks, len(rows), g, partial, 2)
    assert partial[0] == -1 and partial[1] == -1 and partial[-1] == -1  # only its slice is written
    gd = g.double()
    for i, (s, n, _) in enumerate(rows):
        ref = float((gd[s:s + n] ** 2).sum())
        assert abs(float(partial[2 + i]) - ref) <= 4e-6 * ref, (i, s, n)
    with pytest.raises(RuntimeError):
        gpu_ext().gradnorm_partial(chunks, len(rows), g, partial, 4)  # would write past the buffer


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_coefficient_applied_exactly(kind):
    """The clipped step is bitwise the unclipped step with grad_scale = the coefficient read
    back: parameters, optimizer state and bf16 shadows (two steps: SGD's first and later form)."""
    m = 0.5 * _measured_norm()
    pa, oa = _build(kind, m)
    pb, ob = _build(kind, None)
    for step in range(2):
        gr = _grads(step)
        _set_grads(pa, gr)
        _set_grads(pb, gr)
        oa.step()
        coef = float(oa._clip_ws["out"][1])
        assert 0.0 < coef < 1.0, coef
        assert abs(coef - m / (float(oa.grad_norm) + 1e-6)) <= 1e-6 * coef
        ob.flat_space.grad_scale = coef
        ob.step()
        assert _equal(_state(pa, oa), _state(pb, ob)), (kind, step)
    assert ob.grad_norm is None


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_inactive_clip_is_the_unclipped_step(kind):
    m = 2.0 * _measured_norm()
    pa, oa = _build(kind, m)
    pb, ob = _build(kind, None)
    gr = _grads(0)
    _set_grads(pa, gr)
    _set_grads(pb, gr)
    oa.step()
    ob.step()
    assert float(oa._clip_ws["out"][1]) == 1.0
    assert _equal(_state(pa, oa), _state(pb, ob))


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_active_clip_matches_torch(kind):
    m = 0.5 * _measured_norm()
    params, opt = _build(kind, m)
    ref_p = [torch.nn.Parameter(p.detach().cpu().clone()) for p in params]
    groups = [{"params": ref_p[:SPLIT], "lr": 2e-3, "weight_decay": 0.0},
              {"params": ref_p[SPLIT:], "lr": 1e-3, "weight_decay": 0.1}]
    ref = torch.optim.AdamW(groups) if kind == "adamw" else torch.optim.SGD(groups, momentum=0.9)
    for step in range(3):
        gr = _grads(step)
        _set_grads(params, gr)
        for p, v in zip(ref_p, gr):
            p.grad = v.clone()
        norm = float(torch.nn.utils.clip_grad_norm_(ref_p, m))
        assert norm > m
        opt.step()
        ref.step()
        assert abs(float(opt.grad_norm) - norm) <= 1e-5 * norm
    keys = ("exp_avg", "exp_avg_sq") if kind == "adamw" else ("momentum_buffer",)
    for p, r in zip(params[:-1], ref_p):
        torch.testing.assert_close(p.detach().cpu(), r.detach(), rtol=1e-5, atol=1e-6)
        for k in keys:
            torch.testing.assert_close(opt.state[p][k].cpu(), ref.state[r][k], rtol=1e-5, atol=1e-6)
    assert torch.equal(params[-1].detach().cpu(), ref_p[-1].detach())  # no gradient: untouched


def test_run_to_run_determinism():
    m = 0.5 * _measured_norm()
    runs = []
    for _ in range(2):
        params, opt = _build("adamw", m)
        norms = []
        for step in range(3):
            _set_grads(params, _grads(step))
            opt.step()
            norms.append(opt.grad_norm.clone())
        runs.append((torch.stack(norms), _state(params, opt)))
    assert torch.equal(runs[0][0], runs[1][0])
    assert _equal(runs[0][1], runs[1][1])


def test_captured_sgd_step_with_clip_replays_bitwise():
    """FusedSGD (momentum) with an active clip on the toy MLP inside CapturedStep: five replays
    equal five eager steps bit for bit - parameters and grad_norm (no host read in step())."""
    from ray_torch_distributed_checkpoint_amd import ops
    from ray_torch_distributed_checkpoint_amd.models import NeuralNetwork
    from ray_torch_distributed_checkpoint_amd.optim import FusedSGD
    from ray_torch_distributed_checkpoint_amd.utils.graphs import CapturedStep

    clip = 0.05
    torch.manual_seed(0)
    base = NeuralNetwork()
    xs = torch.randn(8, 16, 1, 28, 28, device="cuda")
    ys = torch.randint(0, 10, (8, 16), device="cuda")

    def run(graph):
        m = copy.deepcopy(base).cuda()
        opt = FusedSGD(m.parameters(), lr=1e-2, momentum=0.9, max_grad_norm=clip)
        ops.manual_seed(77)
        x, y = xs[0].clone(), ys[0].clone()

        def step():
            opt.zero_grad()
            loss = ops.cross_entropy(m(x), y)
            loss.backward()
            opt.step()
            return loss.detach()

        norms = []
        if graph:
            cs = CapturedStep(step, warmup=3)  # the 3 warm-up steps consume batch 0
            for i in range(3, 8):
                x.copy_(xs[i])
                y.copy_(ys[i])
                cs.replay()
                norms.append(opt.grad_norm.clone())
            cs.close()
        else:
            for i in range(8):
                x.copy_(xs[0] if i < 3 else xs[i])
                y.copy_(ys[0] if i < 3 else ys[i])
                step()
                if i >= 3:
                    norms.append(opt.grad_norm.clone())
        return torch.stack(norms), [p.detach().clone() for p in m.parameters()]

    ne, pe = run(False)
    ng, pg = run(True)
    assert bool((ne > clip).all()), ne  # the clip is active at every compared step
    assert torch.equal(ne, ng), (ne, ng)
    assert all(torch.equal(a, b) for a, b in zip(pe, pg))


def test_backward_overlap_with_clip_raises():
    from ray_torch_distributed_checkpoint_amd.optim import FusedAdamW
    from ray_torch_distributed_checkpoint_amd.optim.overlap import BackwardOverlap

    def make(clip):
        torch.manual_seed(0)
        ps = [torch.nn.Parameter(torch.randn(100, device="cuda")) for _ in range(3)]
        return ps, FusedAdamW(ps, lr=1e-3, max_grad_norm=clip)

    _, opt = make(1.0)
    with pytest.raises(ValueError):
        BackwardOverlap(opt)
    ps, opt = make(None)
    ov = BackwardOverlap(opt)
    opt.max_grad_norm = 1.0
    before = [p.detach().clone() for p in ps]
    for p in ps:
        p.grad = torch.ones_like(p)
    with pytest.raises(ValueError):
        opt.step()
    assert all(torch.equal(p.detach(), b) for p, b in zip(ps, before))
    ov.remove()


def test_workload_exact_resume_with_clip_gpu(tmp_path, monkeypatch):
    from tests.test_gradclip_cpu import run_resume_case

    for k in ("RTDC_FAIL_AT_STEP", "RTDC_HANG_AT_STEP", "RTDC_FORCE_CPU", "RTDC_FAIL_AT_REPORT"):
        monkeypatch.delenv(k, raising=False)
    run_resume_case(tmp_path, use_gpu=True)


# ------------------------------------------------------------------ two ranks
CLIP2 = 0.5
B, T = 2, 64


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _two_rank_worker(rank, world, port, backend, q):
    """gpt2-tiny, 3 AdamW steps with an active clip: replicated DDP (deferred tail in small
    pieces: the clipped step's piecewise norm pass) and ZeRO-1."""
    try:
        import torch.distributed as dist

        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world))
        dev = torch.device("cuda", rank % torch.cuda.device_count())
        torch.cuda.set_device(dev)
        kw = {"device_id": dev} if backend == "nccl" else {}
        dist.init_process_group(backend, rank=rank, world_size=world, **kw)
        from ray_torch_distributed_checkpoint_amd.models import GPT2, GPT2Config
        from ray_torch_distributed_checkpoint_amd.optim import FusedAdamW
        from ray_torch_distributed_checkpoint_amd.parallel.ddp import DistributedDataParallel

        out = {}
        for zero in (0, 1):
            torch.manual_seed(0)
            model = GPT2(GPT2Config.named("gpt2-tiny")).to(dev)
            extra = {} if zero else {"defer_tail_to_optimizer": True, "tail_piece_mb": 0.02}
            net = DistributedDataParallel(model, bucket_cap_mb=0.25, first_bucket_mb=0.05, zero_stage=zero, **extra)
            opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.1, max_grad_norm=CLIP2)
            norms, pieces = [], []
            for k in range(3):
                g = torch.Generator().manual_seed(11 + k)
                data = torch.randint(0, 1000, (world * B, T + 1), generator=g).to(dev)[rank * B:(rank + 1) * B]
                net(data[:, :-1], data[:, 1:]).backward()
                pieces.append(len(net.space.pending_tail) if net.space.pending_tail else 0)
                opt.step()
                opt.zero_grad()
                norms.append(opt.grad_norm.clone())
            torch.cuda.synchronize()
            out[zero] = (torch.stack(norms).cpu().numpy(),
                         {n: p.detach().float().cpu().numpy() for n, p in model.named_parameters()}, pieces)
            dist.barrier()
        q.put((rank, "ok", out))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        q.put((rank, "err", traceback.format_exc()))


def _spawn_two_ranks(backend, world):
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_two_rank_worker, args=(r, world, port, backend, q)) for r in range(world)]
    # ranks sharing one device: one HIP hardware queue each (as tests/test_multigpu_gpu.py pins
    # its shared-device rehearsal); set in the parent, a spawned child initialises HIP on import
    old_q = os.environ.get("GPU_MAX_HW_QUEUES")
    if backend == "gloo":
        os.environ["GPU_MAX_HW_QUEUES"] = "1"
    try:
        for p in ps:
            p.start()
    finally:
        if backend == "gloo":
            if old_q is None:
                os.environ.pop("GPU_MAX_HW_QUEUES", None)
            else:
                os.environ["GPU_MAX_HW_QUEUES"] = old_q
    out = {}
    try:
        for _ in range(world):
            r, st, v = q.get(timeout=300)
            assert st == "ok", f"rank {r}:\n{v}"
            out[r] = v
    finally:
        for p in ps:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    return out


@pytest.mark.parametrize("backend", [
    pytest.param("nccl", marks=pytest.mark.skipif(NGPU < 2, reason="one rank per GPU needs >= 2 GPUs"), id="rccl"),
    pytest.param("gloo", id="gloo_standin")])
def test_zero1_with_clip_matches_replicated(backend):
    """ZeRO-1 with an active clip: the norm is bitwise equal on both ranks, equals the
    replicated run's at relative 1e-5 at every step, and the parameters after 3 steps match the
    replicated run.

    Parameter tolerance: rtol=2e-5, atol=2e-6, the numeric tolerance of
    tests/test_multigpu_gpu.py::test_zero1_equals_replicated_optimizer.  gpt2-tiny computes in
    bf16, which amplifies even a 1-ulp difference of the clip coefficient far beyond that
    within 3 steps (with fp32 sums of squares: up to 1.9e-3 off, 16 % of the elements outside),
    so this bound holds only because the kernels carry the sums in fp64 and both chunk cuts
    round to the same fp32 norm."""
    world = 2
    out = _spawn_two_ranks(backend, world)
    rep_n, rep_p, rep_pieces = out[0][0]
    assert all(n >= 3 for n in rep_pieces), rep_pieces  # the replicated step saw a piecewise tail
    for r in range(world):
        zn, zp, _ = out[r][1]
        print("rank", r, "replicated norms", out[r][0][0].tolist(), "ZeRO-1 norms", zn.tolist())
        assert (zn > CLIP2).all(), zn  # active at every step
        assert np.array_equal(zn, out[0][1][0]), "ZeRO-1 norm differs across ranks"
        assert np.array_equal(out[r][0][0], rep_n), "replicated norm differs across ranks"
        np.testing.assert_allclose(zn, rep_n, rtol=1e-5, atol=0)
        for n in rep_p:
            assert np.array_equal(zp[n], out[0][1][1][n]), (r, n)  # identical on every rank
            assert np.array_equal(out[r][0][1][n], rep_p[n]), (r, n)
    zp = out[0][1][1]
    worst = max(float(np.abs(zp[n] - v).max()) for n, v in rep_p.items())
    print("max abs parameter difference ZeRO-1 vs replicated after 3 steps", worst)
    for n, v in rep_p.items():
        np.testing.assert_allclose(zp[n], v, rtol=2e-5, atol=2e-6, err_msg=n)
