"""Capturable fused optimizers (FusedAdamW / FusedSGD capturable=True): the kernels read lr, the
bias corrections and the step number from device tables indexed by a device step counter.

* the device path equals the host-scalar path bit for bit after every step - across both table
  clamps, with a parameter that joins late (a non-zero step offset), with fp32 and bf16 state
  (the Philox step word), momentum SGD, an active clip and a gradient scale;
* BackwardOverlap with a capturable, scheduled AdamW stays bitwise equal to the plain step;
* a scheduled, clipped AdamW step captured into a hipGraph replays to the bits of eager steps,
  and the host counters are reconciled from the device counter afterwards;
* what must still refuse capture does; a scheduled GPU workload (device path) resumes exactly.
"""
import copy
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

# 1 and 7: the scalar tail loop only; 65 x 3: vector body + tail; 128 x 64: one full chunk's worth
# of vector iterations; 20000: a parameter cut into two chunks (16384 elements each at most)
SHAPES = [(1,), (7,), (65, 3), (128, 64), (20000,)]
LATE = (33,)  # first gradient at step 3: its Adam step number trails the optimizer's by 2
STEPS = 30  # betas (0.5, 0.5): bias-correction rows end at 25; warmup_cosine(2, 6): lr rows end at 6


@pytest.fixture(autouse=True)
def _default_philox_out_of_graph_mode():
    """A captured step that an earlier test never closed keeps the default dropout stream in
    graph mode, where eager steps do not advance its counter: start every test from host mode."""
    from ray_torch_distributed_checkpoint_amd import ops

    torch.cuda.synchronize()
    ops.default_stream().exit_graph_mode()
    yield


def _make(kind, capturable, clip=None):
    from ray_torch_distributed_checkpoint_amd.optim import FusedAdamW, FusedSGD, LRSchedule

    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(s, device=DEV)) for s in SHAPES + [LATE]]
    sch = LRSchedule.warmup_cosine(2, 6)
    if kind == "sgd":
        opt = FusedSGD(ps, lr=0.05, momentum=0.9, nesterov=True, weight_decay=0.01, max_grad_norm=clip,
                       lr_schedule=sch, capturable=capturable)
    else:
        opt = FusedAdamW(ps, lr=0.05, betas=(0.5, 0.5), weight_decay=0.1, max_grad_norm=clip, lr_schedule=sch,
                         capturable=capturable, rounding_seed=5,
                         state_dtype=torch.bfloat16 if kind == "adamw_bf16" else torch.float32)
    return ps, opt


def _snapshot(opt):
    sp = opt.flat_space
    return [sp.data.clone(), sp.shadow.clone()] + [b.clone() for b in opt._bufs.values()]


@pytest.fixture(scope="module")
def grads():
    g = torch.Generator(device=DEV).manual_seed(1)
    return [[torch.randn(s, device=DEV, generator=g) for s in SHAPES + [LATE]] for _ in range(STEPS)]


@pytest.mark.parametrize("kind,clip,grad_scale", [
    ("adamw", None, 1.0), ("adamw_bf16", None, 1.0), ("sgd", None, 1.0), ("adamw", 0.5, 1.0),
    ("adamw_bf16", 0.5, 0.25), ("sgd", 0.5, 0.25), ("adamw", None, 0.25)])
def test_device_path_equals_host_path_bitwise_every_step(grads, kind, clip, grad_scale):
    from ray_torch_distributed_checkpoint_amd.optim import schedule as S

    (ph, host), (pd, dev) = _make(kind, False, clip), _make(kind, True, clip)
    for n in range(1, STEPS + 1):
        for ps, opt in ((ph, host), (pd, dev)):
            for i, (p, g) in enumerate(zip(ps, grads[n - 1])):
                p.grad = None if (i == len(SHAPES) and n < 3) else g.clone()
            opt._ensure_space().grad_scale = grad_scale
            opt.step()
        a, b = _snapshot(host), _snapshot(dev)
        assert len(a) == len(b) == (3 if kind == "sgd" else 4)
        for x, y in zip(a, b):
            assert torch.equal(x, y), (kind, n)
        assert host.get_last_lr() == dev.get_last_lr() and dev.step_count == n
        if clip:
            assert torch.equal(host.grad_norm, dev.grad_norm) and float(dev.grad_norm) > clip
    assert int(dev._dev["count"].item()) == STEPS  # the device counter kept step with the host's
    assert dev._dev["lr"].shape == (1, 6) and dev._captured is None
    if kind != "sgd":
        assert dev._dev["bc"][(0.5, 0.5)].shape == (25, 2)
        assert torch.equal(dev._dev["bc"][(0.5, 0.5)].cpu(), torch.from_numpy(S.bias_correction_table(0.5, 0.5).copy()))
        sd = dev.state_dict()["state"]
        assert float(sd[0]["step"]) == STEPS and float(sd[len(SHAPES)]["step"]) == STEPS - 2
    fresh, _ = _make(kind, True)
    assert all(not torch.equal(p.detach(), q.detach()) for p, q in zip(pd, fresh))  # every parameter moved


def _gpt2_run(overlap: bool, capturable: bool, steps: int = 4):
    from ray_torch_distributed_checkpoint_amd.models import GPT2, GPT2Config
    from ray_torch_distributed_checkpoint_amd.optim import BackwardOverlap, FusedAdamW, LRSchedule

    torch.manual_seed(0)
    model = GPT2(GPT2Config.named("gpt2-tiny")).to(DEV)
    opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.1, capturable=capturable,
                     lr_schedule=LRSchedule.warmup_cosine(2, 4, 0.1))
    if overlap:
        ov = BackwardOverlap(opt, bucket_mb=0.05)
        assert len(ov.groups) > 2
    g = torch.Generator(device=DEV).manual_seed(1)
    losses = []
    for _ in range(steps):
        data = torch.randint(0, 1000, (4, 65), device=DEV, generator=g)
        loss = model(data[:, :-1], data[:, 1:])
        loss.backward()
        opt.step()
        opt.zero_grad()
        losses.append(loss.item())
    torch.cuda.synchronize()
    return losses, [p.detach().clone() for p in model.parameters()], opt._bufs["exp_avg_sq"].clone()


def test_backward_overlap_with_capturable_adamw_bitwise_equal():
    l0, p0, v0 = _gpt2_run(False, False)  # plain step, host scalars
    for overlap, capturable in ((False, True), (True, True), (True, False)):
        l1, p1, v1 = _gpt2_run(overlap, capturable)
        assert l0 == l1, (overlap, capturable)
        assert all(torch.equal(a, b) for a, b in zip(p0, p1)), (overlap, capturable)
        assert torch.equal(v0, v1), (overlap, capturable)


@pytest.mark.parametrize("state_dtype", [torch.float32, torch.bfloat16])
def test_captured_adamw_step_replays_bitwise_and_reconciles(state_dtype):
    """Scheduled, clipped AdamW on the toy MLP inside CapturedStep(warmup=3): 6 replays equal 9
    eager steps bit for bit; the host counters then come back from the device counter."""
    from ray_torch_distributed_checkpoint_amd import ops
    from ray_torch_distributed_checkpoint_amd.models import NeuralNetwork
    from ray_torch_distributed_checkpoint_amd.optim import FusedAdamW, LRSchedule
    from ray_torch_distributed_checkpoint_amd.utils.graphs import CapturedStep

    clip = 0.05
    torch.manual_seed(0)
    base = NeuralNetwork()
    xs = torch.randn(10, 16, 1, 28, 28, device="cuda")
    ys = torch.randint(0, 10, (10, 16), device="cuda")
    sch = LRSchedule.warmup_cosine(2, 8)

    def run(graph):
        m = copy.deepcopy(base).cuda()
        opt = FusedAdamW(m.parameters(), lr=1e-2, betas=(0.9, 0.95), weight_decay=0.1, max_grad_norm=clip,
                         lr_schedule=sch, capturable=True, state_dtype=state_dtype, rounding_seed=3)
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
            assert opt.step_count == 3  # the captured step ran nothing
            for i in range(3, 9):
                x.copy_(xs[i])
                y.copy_(ys[i])
                cs.replay()
                norms.append(opt.grad_norm.clone())
            cs.close()
        else:
            for i in range(9):
                x.copy_(xs[0] if i < 3 else xs[i])
                y.copy_(ys[0] if i < 3 else ys[i])
                step()
                if i >= 3:
                    norms.append(opt.grad_norm.clone())
        torch.cuda.synchronize()
        state = [p.detach().clone() for p in m.parameters()] + [b.clone() for b in opt._bufs.values()]
        # reconciliation: state_dict() reads the device counter back
        sd = opt.state_dict()
        assert [float(st["step"]) for st in sd["state"].values()] == [9.0] * len(list(m.parameters()))
        assert opt.step_count == 9 and opt.get_last_lr() == [sch.lr(1e-2, 9)]
        assert (opt._captured is not None) == graph
        # one further eager step on both copies
        x.copy_(xs[9])
        y.copy_(ys[9])
        step()
        torch.cuda.synchronize()
        assert opt.step_count == 10 and opt.get_last_lr() == [sch.lr(1e-2, 10)]
        after = [p.detach().clone() for p in m.parameters()] + [b.clone() for b in opt._bufs.values()]
        return torch.stack(norms), state, after

    ne, se, ae = run(False)
    ng, sg, ag = run(True)
    assert bool((ne > clip).all()), ne  # the clip is active at every compared step
    assert torch.equal(ne, ng), (ne, ng)
    assert all(torch.equal(a, b) for a, b in zip(se, sg))
    assert all(torch.equal(a, b) for a, b in zip(ae, ag))
    assert se[-1].dtype == state_dtype


def test_capture_refusals():
    from ray_torch_distributed_checkpoint_amd.optim import FusedAdamW, FusedSGD, LRSchedule

    def capture(opt, ps):
        for p in ps:
            p.grad = torch.ones_like(p)
        opt.step()  # eager: state, workspaces
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.graph(g, stream=s):
            ps[0].grad.mul_(1.0)  # (a refused step leaves a graph that is not empty)
            opt.step()
        return g

    def params():
        torch.manual_seed(0)
        return [torch.nn.Parameter(torch.randn(100, device=DEV)) for _ in range(3)]

    ps = params()
    with pytest.raises(RuntimeError, match="capturable=True"):
        capture(FusedAdamW(ps, lr=1e-3), ps)
    ps = params()
    with pytest.raises(RuntimeError, match="capturable=True"):
        capture(FusedSGD(ps, lr=1e-2, momentum=0.9, lr_schedule=LRSchedule.warmup_linear(1, 4)), ps)
    for kw in ({}, {"lr_schedule": LRSchedule.constant()}):  # constant lr: captures as before
        ps = params()
        opt = FusedSGD(ps, lr=1e-2, momentum=0.9, **kw)
        g = capture(opt, ps)
        before = [p.detach().clone() for p in ps]
        g.replay()
        torch.cuda.synchronize()
        assert all(not torch.equal(p.detach(), b) for p, b in zip(ps, before))
        assert opt._captured is None  # host-scalar path: nothing to read back


def _rows(path):
    return [json.loads(line) for line in open(os.path.join(path, "result.json"))]


def _by_step(rows, key):
    out = {}
    for row in rows:
        for i, v in enumerate(reversed(row[key])):
            out[row["step"] - i] = v
    return out


def test_workload_exact_resume_with_schedule_gpu(tmp_path, monkeypatch):
    """gpt2-tiny with the cosine schedule on the GPU (device-table kernels): 6 steps with a
    checkpoint every 3; an exact resume from step 3 reproduces steps 4-6 bit for bit."""
    from ray_torch_distributed_checkpoint_amd import train
    from ray_torch_distributed_checkpoint_amd import workloads as W
    from ray_torch_distributed_checkpoint_amd.optim import LRSchedule

    for k in ("RTDC_FAIL_AT_STEP", "RTDC_HANG_AT_STEP", "RTDC_FORCE_CPU", "RTDC_FAIL_AT_REPORT"):
        monkeypatch.delenv(k, raising=False)
    wl = W.build(W.WorkloadConfig(model="gpt2-tiny", steps=6, lr_schedule="cosine", warmup_steps=2,
                                  opt_capturable=True), DEV)
    assert wl.optimizer.capturable and wl.optimizer.lr_schedule is not None  # opted in: the device path
    wl = W.build(W.WorkloadConfig(model="gpt2-tiny", steps=6, lr_schedule="cosine", warmup_steps=2), DEV)
    assert not wl.optimizer.capturable and wl.optimizer.lr_schedule is not None  # the default stays on the host path
    del wl
    kw = dict(steps=6, num_workers=1, use_gpu=True, ckpt_every_n_steps=3, verbose=0, lr_schedule="cosine",
              warmup_steps=2, min_lr_ratio=0.1, opt_capturable=True)
    a = W.train_workload("gpt2-tiny", checkpoint_storage_path=str(tmp_path / "a"), **kw)
    rows = _rows(a.path)
    sch = LRSchedule.warmup_cosine(2, 6, 0.1)
    assert [(r["step"], r["lr"]) for r in rows] == [(3, sch.lr(1e-3, 3)), (6, sch.lr(1e-3, 6))]
    la = _by_step(rows, "losses")
    cks = sorted(d for d in os.listdir(a.path) if d.startswith("checkpoint_"))
    assert len(cks) == 2
    ck = train.Checkpoint.from_directory(os.path.join(a.path, cks[0]))
    b = W.train_workload("gpt2-tiny", checkpoint_storage_path=str(tmp_path / "b"), checkpoint=ck,
                         resume_mode="exact", **kw)
    rows_b = _rows(b.path)
    assert _by_step(rows_b, "losses") == {k: la[k] for k in (4, 5, 6)}
    assert rows_b[-1]["lr"] == rows[-1]["lr"]
