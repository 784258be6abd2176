"""In-place gradient accumulation over micro-batches on the GPU (optim.GradAccumulator).

* the grouped weight-gradient kernels' accumulating store is bitwise `prev + fresh`, touches
  nothing outside its outputs, and a group may mix adding and overwriting products;
* an accumulated backward leaves every gradient at its own slice of the flat buffer, equal to
  the sum of the micro-batches' single-backward gradients - bitwise wherever the accumulating
  kernel does one IEEE add per element, within a derived bound where a gradient is itself the
  sum of two partial products (tied table, alpha_dev LM head);
* a parameter that gets its first gradient in a later micro-batch is written, not added to;
* whole optimizer steps against legacy accumulation (autograd adds into a kept p.grad);
* clipping sees the averaged gradient; DDP reduces once per step; the workload resumes exactly;
* ResNet's unconverted gradients accumulate through the add fold-back.
"""
import functools
import os
import socket
import sys
import traceback

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

SHAPES = [(2304, 768), (768, 768), (3072, 768), (768, 3072)]  # tests/test_wgrad_group_gpu.py
GUARD = 64
SENTINEL = -12345.0

# (name, [(N, K, M tokens)]): one block per tile / persistent with one tile per block; persistent
# over 332 tiles (several tiles per block, products switching mid-run, ragged edges); products
# of different K - the one-block-per-tile kernel (gemm8g_kernel) itself
GROUPS = [
    ("gpt2_two_layers", [(n, k, 4096) for n, k in SHAPES * 2]),
    ("persistent_ragged", [(n, k, 2048) for n, k in [(4096, 4096), (1000, 2736), (2048, 1024)]]),
    ("mixed_k", [(768, 768, 4096), (1000, 520, 2048), (2304, 768, 1024)]),
]


def _guarded(n, k, dev):
    """An [n, k] fp32 output with GUARD sentinel elements on either side."""
    buf = torch.full((n * k + 2 * GUARD,), SENTINEL, device=dev)
    return buf, buf[GUARD:GUARD + n * k].view(n, k)


@pytest.mark.parametrize("name,group", GROUPS, ids=[g[0] for g in GROUPS])
def test_grouped_accumulate_is_bitwise_prev_plus_fresh(name, group):
    from ray_torch_distributed_checkpoint_amd.ops._ext import gpu_ext

    torch.manual_seed(7)
    dev = torch.device("cuda", 0)
    dys, xs, dims = [], [], []
    for n, k, m in group:
        dys.append(torch.randn(m, n, device=dev).bfloat16())
        xs.append(torch.randn(m, k, device=dev).bfloat16())
        dims += [n, k, m, n, k, k]
    fresh = [torch.full((n, k), float("nan"), device=dev) for n, k, _ in group]
    gpu_ext().gemm_bf16_grouped(dys, xs, fresh, dims, False, False)
    prev = [torch.randn(n, k, device=dev) * 50.0 for n, k, _ in group]
    for flags in ([1] * len(group), [i % 2 for i in range(len(group))]):
        runs = []
        for _ in range(2):
            bufs, outs = zip(*[_guarded(n, k, dev) for n, k, _ in group])
            for o, p in zip(outs, prev):
                o.copy_(p)
            gpu_ext().gemm_bf16_grouped(dys, xs, list(outs), dims, False, False, flags)
            torch.cuda.synchronize()
            for i, (b, o) in enumerate(zip(bufs, outs)):
                want = prev[i] + fresh[i] if flags[i] else fresh[i]
                assert torch.isfinite(o).all()
                assert torch.equal(o, want), f"{name} product {i} flag {flags[i]}: {(o - want).abs().max().item():.3e}"
                assert bool((b[:GUARD] == SENTINEL).all()) and bool((b[-GUARD:] == SENTINEL).all()), \
                    f"{name} product {i}: guard band overwritten"
            runs.append([o.clone() for o in outs])
        assert all(torch.equal(a, b) for a, b in zip(*runs))  # run to run


# ---------------------------------------------------------------- accumulated backward passes
def _gpt2(dev):
    from ray_torch_distributed_checkpoint_amd.models import GPT2, GPT2Config

    torch.manual_seed(0)
    cfg = GPT2Config(vocab_size=1024, n_positions=1024, n_embd=768, n_layer=2, n_head=12)
    return GPT2(cfg).to(dev)


def _llama(dev):
    from ray_torch_distributed_checkpoint_amd.models import Llama, LlamaConfig

    torch.manual_seed(0)
    return Llama(LlamaConfig.named("llama3-tiny"), device=dev)  # Dh 64, RMSNorm, SwiGLU, untied head


def _batches(kind, n, seed=3):
    g = torch.Generator().manual_seed(seed)
    shape = (4, 1025) if kind == "gpt2" else (8, 513)  # 4096 tokens: groupable weight gradients
    return [torch.randint(0, 1024, shape, generator=g).cuda() for _ in range(n)]


def _clone_grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


@functools.lru_cache(maxsize=None)
def _accumulated(kind):
    """(g1, g2, G, status, launched): single-backward gradients of two micro-batches and the
    accumulated pass over both, `_grad_status` before the step, (form, accumulate flags) of
    the deferred weight-gradient launches of the second micro-batch."""
    from ray_torch_distributed_checkpoint_amd.ops import gemm as G_

    if kind == "gpt2_nodefer":
        # column sums reduced immediately (RTDC_COLSUM_DEFER=0): LayerNorm's backward then cannot
        # add into its slots and hands its sums to the fold-back / the projection's colsum()
        old = G_._DEFER_ON
        G_._DEFER_ON = False
        try:
            return _accumulated_impl("gpt2")
        finally:
            G_._DEFER_ON = old
    return _accumulated_impl(kind)


def _accumulated_impl(kind):
    from ray_torch_distributed_checkpoint_amd.ops import gemm as G_
    from ray_torch_distributed_checkpoint_amd.optim import FusedAdamW, GradAccumulator

    dev = torch.device("cuda", 0)
    model = (_gpt2 if kind == "gpt2" else _llama)(dev)
    opt = FusedAdamW(model.parameters(), lr=1e-3)
    sp = opt._ensure_space()
    b1, b2 = _batches(kind, 2)
    singles = []
    for b in (b1, b2):
        opt.zero_grad(set_to_none=True)
        model(b[:, :-1], b[:, 1:]).backward()
        torch.cuda.synchronize()
        singles.append(_clone_grads(model))
    opt.zero_grad(set_to_none=True)
    acc = GradAccumulator(opt, steps=2, average=False)
    launched = []
    orig, orig_split = G_._WgradGroup._launch, G_._WgradGroup._launch_split

    def spy(self, items):
        launched.append(("grouped", [bool(it[5]) for it in items]))
        return orig(self, items)

    def spy_split(self, items):  # a remainder far below a round: one split-K launch per product
        launched.append(("split", [bool(it[5]) for it in items]))
        return orig_split(self, items)

    with acc.micro_step(0):
        model(b1[:, :-1], b1[:, 1:]).backward()
    G_._WgradGroup._launch, G_._WgradGroup._launch_split = spy, spy_split
    try:
        with acc.micro_step(1):
            model(b2[:, :-1], b2[:, 1:]).backward()
    finally:
        G_._WgradGroup._launch, G_._WgradGroup._launch_split = orig, orig_split
    torch.cuda.synchronize()
    status = list(sp._grad_status(sp.grad.data_ptr()))
    total = _clone_grads(model)
    opt.zero_grad(set_to_none=True)
    assert not sp.accumulating
    return singles[0], singles[1], total, status, launched


def _derived_bound_ok(G, g1, g2):
    """|G - (g1 + g2 in fp64)| <= 8 * 2^-24 * (|g1| + |g2| + |G|) elementwise: each path rounds
    at most three partial sums of those magnitudes."""
    ref = g1.double() + g2.double()
    bound = 8.0 * 2.0 ** -24 * (g1.double().abs() + g2.double().abs() + G.double().abs())
    return bool(((G.double() - ref).abs() <= bound).all())


@pytest.mark.parametrize("kind,bounded", [("gpt2", ("wte",)), ("llama", ("output",)), ("gpt2_nodefer", ("wte",))])
def test_accumulated_backward_lands_in_the_slices(kind, bounded):
    g1, g2, total, status, launched = _accumulated(kind)
    assert status and all(s == 1 for s in status), status  # every p.grad is its own flat slice
    # the second micro-batch's weight gradients were deferred as in a single backward, adding:
    # the GPT-2 layers' 216 tiles as one grouped launch, llama3-tiny's few tiles split-K each
    assert launched and all(all(flags) for _, flags in launched), launched
    assert {form for form, _ in launched} == ({"split"} if kind == "llama" else {"grouped"}), launched
    assert set(total) == set(g1) == set(g2)
    for n in total:
        assert torch.isfinite(total[n]).all(), n
        if n in bounded:
            assert _derived_bound_ok(total[n], g1[n], g2[n]), f"{n}: outside the derived bound"
        else:
            assert torch.equal(total[n], g1[n] + g2[n]), \
                f"{n}: max |G - (g1 + g2)| = {(total[n] - (g1[n] + g2[n])).abs().max().item():.3e}"


def test_first_touch_in_a_later_micro_batch_writes():
    from ray_torch_distributed_checkpoint_amd import ops
    from ray_torch_distributed_checkpoint_amd.optim import FusedAdamW, GradAccumulator

    dev = torch.device("cuda", 0)
    torch.manual_seed(5)
    wa = torch.nn.Parameter(torch.randn(1024, 1024, device=dev) * 0.03)
    wb = torch.nn.Parameter(torch.randn(1024, 1024, device=dev) * 0.03)
    x1 = torch.randn(4096, 1024, device=dev).bfloat16()
    x2 = torch.randn(4096, 1024, device=dev).bfloat16()
    opt = FusedAdamW([wa, wb], lr=1e-3)
    sp = opt._ensure_space()

    def loss(x, both):
        h = ops.linear(x, wa)
        if both:
            h = ops.linear(h, wb)
        return h.float().square().mean()

    opt.zero_grad(set_to_none=True)
    loss(x1, False).backward()
    ga1 = wa.grad.detach().clone()
    opt.zero_grad(set_to_none=True)
    loss(x2, True).backward()
    torch.cuda.synchronize()
    ga2, gb2 = wa.grad.detach().clone(), wb.grad.detach().clone()
    opt.zero_grad(set_to_none=True)
    sp.grad_view(wb).fill_(float("nan"))  # what a stale slice must not leak into the sum
    acc = GradAccumulator(opt, steps=2, average=False)
    with acc.micro_step(0):
        loss(x1, False).backward()
    assert wb.grad is None
    with acc.micro_step(1):
        loss(x2, True).backward()
    torch.cuda.synchronize()
    assert torch.isfinite(wa.grad).all() and torch.isfinite(wb.grad).all()
    assert torch.equal(wb.grad, gb2)
    assert torch.equal(wa.grad, ga1 + ga2)
    assert all(s == 1 for s in sp._grad_status(sp.grad.data_ptr()))


# ---------------------------------------------------------------- whole steps
def _tiny(kind, dev):
    from ray_torch_distributed_checkpoint_amd.models import GPT2, GPT2Config, Llama, LlamaConfig

    torch.manual_seed(0)
    if kind == "gpt2-tiny":
        return GPT2(GPT2Config.named("gpt2-tiny")).to(dev)
    return Llama(LlamaConfig.named("llama3-tiny"), device=dev)


def _tiny_batches(n, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 1000, (4, 65), generator=g).cuda() for _ in range(n)]


def _train(kind, k, mode, steps=3, clip=None):
    """mode "accum": GradAccumulator; "legacy": p.grad kept between the backwards (autograd
    adds) with grad_scale = 1/k; "plain": the single-backward loop (k = 1)."""
    from ray_torch_distributed_checkpoint_amd.optim import FusedAdamW, GradAccumulator

    dev = torch.device("cuda", 0)
    model = _tiny(kind, dev)
    opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.1, max_grad_norm=clip)
    sp = opt._ensure_space()
    acc = GradAccumulator(opt, steps=k) if mode == "accum" else None
    if mode == "legacy":
        sp.grad_scale = 1.0 / k
    opt.zero_grad(set_to_none=True)
    norms, sums = [], []
    for s in range(steps):
        bs = _tiny_batches(k, 100 + s)
        for i, b in enumerate(bs):
            if acc is not None:
                with acc.micro_step(i):
                    model(b[:, :-1], b[:, 1:]).backward()
            else:
                model(b[:, :-1], b[:, 1:]).backward()
        opt.step()
        if clip:
            norms.append(opt.grad_norm.clone())
            sums.append({n: p.grad.detach().clone() for n, p in model.named_parameters()})
        opt.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    return {n: p.detach().clone() for n, p in model.named_parameters()}, norms, sums


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("kind", ["gpt2-tiny", "llama3-tiny"])
def test_steps_match_legacy_accumulation(kind, k):
    got, _, _ = _train(kind, k, "accum")
    ref, _, _ = _train(kind, k, "legacy")
    for n in ref:
        # (the fused-optimizer-vs-torch tolerance of tests/test_optim.py)
        torch.testing.assert_close(got[n], ref[n], rtol=1e-5, atol=1e-6, msg=lambda m, n=n: f"{n}: {m}")


@pytest.mark.parametrize("kind", ["gpt2-tiny", "llama3-tiny"])
def test_one_micro_batch_is_the_plain_loop(kind):
    got, _, _ = _train(kind, 1, "accum")
    ref, _, _ = _train(kind, 1, "plain")
    for n in ref:
        assert torch.equal(got[n], ref[n]), n


def test_clipping_sees_the_averaged_gradient():
    _, norms, sums = _train("gpt2-tiny", 2, "accum", steps=2, clip=0.05)
    for norm, grads in zip(norms, sums):
        # p.grad holds the unscaled sum g1 + g2; the step clips the norm of its mean
        want = sum((g.double() / 2).square().sum() for g in grads.values()).sqrt()
        assert abs(norm.double().item() - want.item()) <= 4 * 2.0 ** -24 * want.item(), (norm.item(), want.item())
        assert want.item() > 0.05  # the clip was active


# ---------------------------------------------------------------- two ranks on one device
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


DDP_B, DDP_T = 2, 64


def _ddp_batch(world, rank, step, i):
    g = torch.Generator().manual_seed(1000 + 10 * step + i)
    data = torch.randint(0, 1000, (world * DDP_B, DDP_T + 1), generator=g)
    return data[rank * DDP_B:(rank + 1) * DDP_B].cuda()


def _ddp_worker(rank, world, port, q):
    try:
        import torch.distributed as dist

        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world))
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from ray_torch_distributed_checkpoint_amd.optim import FusedAdamW, GradAccumulator
        from ray_torch_distributed_checkpoint_amd.parallel.ddp import DistributedDataParallel

        out = {}
        # replicated: gradients of one accumulated step, and when the collectives were launched
        model = _tiny("gpt2-tiny", dev)
        net = DistributedDataParallel(model, bucket_cap_mb=0.25, first_bucket_mb=0.05)
        opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.1)
        acc = GradAccumulator(opt, steps=2, ddp=net, average=False)
        opt.zero_grad(set_to_none=True)
        launched = []
        for i in range(2):
            b = _ddp_batch(world, rank, 0, i)
            with acc.micro_step(i):
                net(b[:, :-1], b[:, 1:]).backward()
            # (_steps counts the backward passes that ran the bucket engine - each launches every
            # bucket's collective exactly once and resets its per-step launch counter)
            launched.append(int(net._steps))
        net.wait_tail()
        torch.cuda.synchronize()
        out["grads"] = {n: p.grad.detach().float().cpu().numpy() for n, p in model.named_parameters()}
        out["launched"] = launched
        opt.zero_grad(set_to_none=True)
        net.detach()
        dist.barrier()
        # ZeRO-1: two accumulated steps, twice
        runs = []
        for _ in range(2):
            model = _tiny("gpt2-tiny", dev)
            net = DistributedDataParallel(model, bucket_cap_mb=0.25, first_bucket_mb=0.05, zero_stage=1)
            opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.1)
            acc = GradAccumulator(opt, steps=2, ddp=net)
            opt.zero_grad(set_to_none=True)
            for s in range(2):
                for i in range(2):
                    b = _ddp_batch(world, rank, s, i)
                    with acc.micro_step(i):
                        net(b[:, :-1], b[:, 1:]).backward()
                opt.step()
                opt.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            runs.append({n: p.detach().float().cpu().numpy() for n, p in model.named_parameters()})
            net.detach()
            dist.barrier()
        out["zero"] = runs
        q.put((rank, "ok", out))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        q.put((rank, "err", traceback.format_exc()))


def test_ddp_reduces_once_per_accumulated_step():
    import numpy as np
    import torch.multiprocessing as mp

    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_ddp_worker, args=(r, world, port, q)) for r in range(world)]
    # ranks sharing one device: one HIP hardware queue each (set in the parent: a spawned child
    # initialises HIP on import)
    old_q = os.environ.get("GPU_MAX_HW_QUEUES")
    os.environ["GPU_MAX_HW_QUEUES"] = "1"
    try:
        for p in ps:
            p.start()
    finally:
        if old_q is None:
            os.environ.pop("GPU_MAX_HW_QUEUES", None)
        else:
            os.environ["GPU_MAX_HW_QUEUES"] = old_q
    out = {}
    try:
        for _ in range(world):
            r, st, v = q.get(timeout=240)
            assert st == "ok", f"rank {r}:\n{v}"
            out[r] = v
    finally:
        for p in ps:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for r in range(world):
        assert out[r]["launched"] == [0, 1], out[r]["launched"]  # once, in the last micro-batch
    # single-process g1 + g2 of each rank's micro-batches
    dev = torch.device("cuda", 0)
    from ray_torch_distributed_checkpoint_amd.optim import FusedAdamW

    per_rank = []
    for r in range(world):
        model = _tiny("gpt2-tiny", dev)
        opt = FusedAdamW(model.parameters(), lr=1e-3)
        opt._ensure_space()
        gs = []
        for i in range(2):
            opt.zero_grad(set_to_none=True)
            b = _ddp_batch(world, r, 0, i)
            model(b[:, :-1], b[:, 1:]).backward()
            torch.cuda.synchronize()
            gs.append({n: p.grad.detach().double().cpu() for n, p in model.named_parameters()})
        opt.zero_grad(set_to_none=True)
        per_rank.append(gs)
    for n, g0 in out[0]["grads"].items():
        assert np.array_equal(g0, out[1]["grads"][n]), f"ranks differ on {n}"
        parts = [per_rank[r][i][n] for r in range(world) for i in range(2)]
        ref = sum(parts) / world
        got = torch.from_numpy(g0).double()
        # the derived bound of the single-process test over four partial gradients, halved
        bound = 8.0 * 2.0 ** -24 * (sum(p.abs() for p in parts) / world + got.abs())
        assert bool(((got - ref).abs() <= bound).all()), f"{n}: {((got - ref).abs() - bound).max().item():.3e} over"
    for r in range(world):
        a, b = out[r]["zero"]
        assert all(np.array_equal(a[n], b[n]) for n in a), "ZeRO-1 accumulated steps differ run to run"
    assert all(np.array_equal(out[0]["zero"][0][n], out[1]["zero"][0][n]) for n in out[0]["zero"][0])


# ---------------------------------------------------------------- workload
def test_workload_accumulates_and_resumes_exactly_gpu(tmp_path, monkeypatch):
    from tests.test_grad_accum_cpu import run_accum_resume_case

    for k in ("RTDC_FAIL_AT_STEP", "RTDC_HANG_AT_STEP", "RTDC_FORCE_CPU", "RTDC_FAIL_AT_REPORT"):
        monkeypatch.delenv(k, raising=False)
    run_accum_resume_case(tmp_path, model="llama3-tiny", use_gpu=True)


# ---------------------------------------------------------------- ResNet: the add fold-back
def test_resnet_accumulates_through_the_fold_back():
    from ray_torch_distributed_checkpoint_amd import ops
    from ray_torch_distributed_checkpoint_amd.models import ResNet18
    from ray_torch_distributed_checkpoint_amd.optim import FusedSGD, GradAccumulator

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = ResNet18(num_classes=10).to(dev)
    opt = FusedSGD(model.parameters(), lr=0.05, momentum=0.9)
    sp = opt._ensure_space()
    g = torch.Generator().manual_seed(2)
    xs = [torch.randn(8, 3, 32, 32, generator=g).to(dev) for _ in range(2)]
    ys = [torch.randint(0, 10, (8,), generator=g).to(dev) for _ in range(2)]
    bufs = {n: b.detach().clone() for n, b in model.named_buffers()}

    def reset_buffers():  # BatchNorm running statistics: every pass starts from the same model
        with torch.no_grad():
            for n, b in model.named_buffers():
                b.copy_(bufs[n])

    singles = []
    for x, y in zip(xs, ys):
        opt.zero_grad(set_to_none=True)
        ops.cross_entropy(model(x), y).backward()
        torch.cuda.synchronize()
        singles.append(_clone_grads(model))
    g1, g2 = singles
    reset_buffers()
    opt.zero_grad(set_to_none=True)
    acc = GradAccumulator(opt, steps=2, average=False)
    for i, (x, y) in enumerate(zip(xs, ys)):
        with acc.micro_step(i):
            ops.cross_entropy(model(x), y).backward()
    torch.cuda.synchronize()
    assert all(s == 1 for s in sp._grad_status(sp.grad.data_ptr()))
    for n, p in model.named_parameters():
        want = g1[n] + g2[n]
        # one fp32 add of a fresh tensor: bitwise, or within 1 ulp of the sum
        ulp = torch.ldexp(torch.ones_like(want), torch.frexp(want)[1] - 24)
        assert bool(((p.grad - want).abs() <= ulp).all()), f"{n}: {(p.grad - want).abs().max().item():.3e}"
    opt.zero_grad(set_to_none=True)
