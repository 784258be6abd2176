"""Gradient accumulation over micro-batches without a GPU: the flat space's micro-step protocol,
GradAccumulator + DDP against torch DDP's no_sync() recipe on two gloo ranks, and the workload /
CLI plumbing (rows, exact resume)."""
import copy
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import mp_util  # noqa: E402


# ---------------------------------------------------------------- space protocol
def _space():
    from ray_torch_distributed_checkpoint_amd.optim import FlatParamSpace

    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(s)) for s in [(5, 3), (7,), (4, 4)]]
    sp = FlatParamSpace(ps)
    sp.zero_grad(set_to_none=True)
    return ps, sp


def test_next_micro_step_records_touched_and_detaches():
    from ray_torch_distributed_checkpoint_amd.ops.gradbuf import grad_slot, grad_target

    ps, sp = _space()
    assert not sp.accumulating and not any(sp.touched(p) for p in ps)
    v0, a0 = grad_slot(ps[0])
    assert not a0 and v0.data_ptr() == sp.grad_view(ps[0]).data_ptr()
    v0.fill_(1.0)
    ps[0].grad = v0                      # what AccumulateGrad does with the returned view
    ps[1].grad = torch.full((7,), 2.0)   # a gradient allocated outside the buffer
    sid = sp.step_id
    sp.next_micro_step()
    assert sp.accumulating and sp.fresh and sp.step_id == sid + 1
    assert all(p.grad is None for p in ps)
    assert [sp.touched(p) for p in ps] == [True, True, False]
    assert torch.equal(sp.grad_view(ps[1]), torch.full((7,), 2.0))  # folded (copied: first micro-batch)
    # touched: the slot adds; a first touch in a later micro-batch writes
    v, a = grad_slot(ps[0])
    assert a and v.data_ptr() == sp.grad_view(ps[0]).data_ptr()
    v2, a2 = grad_slot(ps[2])
    assert not a2 and v2.data_ptr() == sp.grad_view(ps[2]).data_ptr()
    # a call site that cannot add gets no view for a touched parameter
    assert grad_target(ps[1]) is None
    # handed out twice in one micro-batch (tied weight): the second use allocates
    assert grad_slot(ps[0]) == (None, False)


def test_fold_back_adds_and_step_reattaches():
    from ray_torch_distributed_checkpoint_amd.optim import FusedSGD

    ps, sp = _space()
    opt = FusedSGD(ps, lr=0.5)
    before = [p.detach().clone() for p in ps]
    g0 = [torch.randn(p.shape) for p in ps]
    g1 = [torch.randn(p.shape) for p in ps]
    for p, g in zip(ps, g0):
        p.grad = g.clone()
    sp.next_micro_step()
    ps[0].grad = g1[0].clone()  # foreign gradient for a touched parameter: added
    # ps[1], ps[2]: no gradient in the last micro-batch
    sp.fold_grads()
    assert ps[0].grad.data_ptr() == sp.grad_view(ps[0]).data_ptr()
    assert torch.equal(ps[0].grad, g0[0] + g1[0])
    sp.grad_scale = 0.5
    opt.step()
    assert all(p.grad is not None and p.grad.data_ptr() == sp.grad_view(p).data_ptr() for p in ps)  # re-attached
    want = [before[0] - 0.5 * 0.5 * (g0[0] + g1[0]), before[1] - 0.5 * 0.5 * g0[1], before[2] - 0.5 * 0.5 * g0[2]]
    for p, w in zip(ps, want):
        torch.testing.assert_close(p.detach(), w, rtol=1e-6, atol=1e-7)
    opt.zero_grad(set_to_none=True)
    assert not sp.accumulating and not any(sp.touched(p) for p in ps) and all(p.grad is None for p in ps)
    # outside accumulate mode the fold-back copies, as before
    sp.grad_view(ps[0]).fill_(9.0)
    ps[0].grad = g1[0].clone()
    sp.ensure_grad_views()
    assert torch.equal(ps[0].grad, g1[0])


def test_accumulator_contract():
    from ray_torch_distributed_checkpoint_amd.optim import FusedSGD, GradAccumulator

    ps, sp = _space()
    opt = FusedSGD(ps, lr=0.1)
    one = GradAccumulator(opt, steps=1)
    with one.micro_step(0):
        pass
    assert sp.grad_scale == 1.0 and not sp.accumulating and one.space is None  # k = 1 calls nothing
    acc = GradAccumulator(opt, steps=4)
    assert sp.grad_scale == 0.25
    with pytest.raises(IndexError):
        with acc.micro_step(4):
            pass
    acc.close()
    assert sp.grad_scale == 1.0
    with pytest.raises(ValueError):
        GradAccumulator(opt, steps=0)
    opt._overlap = object()  # a BackwardOverlap is attached
    with pytest.raises(RuntimeError, match="BackwardOverlap"):
        GradAccumulator(opt, steps=2)


# ---------------------------------------------------------------- two gloo ranks vs torch DDP
def _ddp_accum(rank, world, k):
    from ray_torch_distributed_checkpoint_amd.models import GPT2, GPT2Config
    from ray_torch_distributed_checkpoint_amd.optim import FusedAdamW, GradAccumulator
    from ray_torch_distributed_checkpoint_amd.parallel.ddp import DistributedDataParallel

    torch.manual_seed(0)
    base = GPT2(GPT2Config.named("gpt2-tiny"))
    ours_m, ref_m = copy.deepcopy(base), copy.deepcopy(base)
    ours = DistributedDataParallel(ours_m, bucket_cap_mb=0.25, first_bucket_mb=0.05, defer_tail_to_optimizer=True)
    ref = torch.nn.parallel.DistributedDataParallel(ref_m)
    opt_o = FusedAdamW(ours_m.parameters(), lr=1e-3, weight_decay=0.1)
    opt_r = torch.optim.AdamW(ref_m.parameters(), lr=1e-3, weight_decay=0.1, foreach=False)
    acc = GradAccumulator(opt_o, steps=k, ddp=ours)
    opt_o.zero_grad(set_to_none=True)
    opt_r.zero_grad(set_to_none=True)
    g = torch.Generator().manual_seed(100 + rank)
    reduced = []
    for _ in range(3):
        data = [torch.randint(0, 1000, (2, 33), generator=g) for _ in range(k)]
        for i, d in enumerate(data):
            with acc.micro_step(i):
                ours(d[:, :-1], d[:, 1:]).backward()
            reduced.append(ours.space.pending_tail is not None)
            if i < k - 1:
                with ref.no_sync():
                    (ref(d[:, :-1], d[:, 1:]) / k).backward()
            else:
                (ref(d[:, :-1], d[:, 1:]) / k).backward()
        opt_o.step()
        opt_o.zero_grad(set_to_none=True)
        opt_r.step()
        opt_r.zero_grad(set_to_none=True)
    # only the last micro-batch of each step left a deferred collective behind
    assert reduced == ([False] * (k - 1) + [True]) * 3, reduced
    named = dict(ref_m.named_parameters())
    err = max(float((p.detach() - named[n].detach()).abs().max()) for n, p in ours_m.named_parameters())
    return err


@pytest.mark.parametrize("k", [2, 4])
def test_accumulator_with_ddp_is_bitwise_torch_ddp_no_sync(k):
    """fp32 communication, k a power of two: 1/k commutes with every rounding (no underflow with
    this data), so the accumulated sum scaled once equals torch's sum of scaled gradients."""
    assert mp_util.run(_ddp_accum, 2, k) == [0.0, 0.0]


def test_accumulator_with_ddp_k3_matches_torch():
    out = mp_util.run(_ddp_accum, 2, 3)
    assert max(out) < 5e-3, out  # (the bf16-communication tolerance of tests/test_distributed_cpu.py)


# ---------------------------------------------------------------- workload and CLIs
def _rows(path):
    return [json.loads(line) for line in open(os.path.join(path, "result.json"))]


def _losses(path):
    out = {}
    for row in _rows(path):
        for i, v in enumerate(reversed(row["losses"])):
            k = row["step"] - i
            assert out.setdefault(k, v) == v, f"step {k} logged twice with different losses"
    return out


def _final_model(model, ckpt_path):
    import torch.distributed.checkpoint as tdcp

    from ray_torch_distributed_checkpoint_amd.models import GPT2, GPT2Config, Llama, LlamaConfig

    m = GPT2(GPT2Config.named(model)) if model.startswith("gpt2") else Llama(LlamaConfig.named(model))
    sd = {"model": m.state_dict()}
    tdcp.load(sd, checkpoint_id=ckpt_path)
    return sd["model"]


def run_accum_resume_case(tmp_path, model: str, use_gpu: bool):
    """4 optimizer steps of 2 micro-batches with a checkpoint every 2; a run killed at step 3
    and restarted from the step-2 checkpoint logs the same losses and ends with the same
    parameters, bit for bit."""
    from ray_torch_distributed_checkpoint_amd import workloads as W

    kw = dict(steps=4, num_workers=1, use_gpu=use_gpu, ckpt_every_n_steps=2, verbose=0, grad_accum_steps=2)
    a = W.train_workload(model, checkpoint_storage_path=str(tmp_path / "a"), **kw)
    rows = _rows(a.path)
    assert [r["step"] for r in rows] == [2, 4]
    assert all(r["samples_per_s"] > 0 and len(r["losses"]) == 2 for r in rows)
    os.environ["RTDC_FAIL_AT_STEP"] = "3:0"
    try:
        b = W.train_workload(model, checkpoint_storage_path=str(tmp_path / "b"), max_failures=1, **kw)
    finally:
        os.environ.pop("RTDC_FAIL_AT_STEP", None)
    la, lb = _losses(a.path), _losses(b.path)
    assert sorted(la) == [1, 2, 3, 4] and la == lb
    assert b.metrics["step"] == 4
    pa, pb = _final_model(model, a.checkpoint.path), _final_model(model, b.checkpoint.path)
    assert all(torch.equal(pa[n], pb[n]) for n in pa)
    return a


@pytest.fixture
def _cpu(monkeypatch):
    monkeypatch.setenv("RTDC_FORCE_CPU", "1")
    for k in ("RTDC_FAIL_AT_STEP", "RTDC_HANG_AT_STEP", "RTDC_FAIL_AT_REPORT"):
        monkeypatch.delenv(k, raising=False)


def test_workload_exact_resume_with_accumulation_cpu(tmp_path, _cpu):
    run_accum_resume_case(tmp_path, model="gpt2-tiny", use_gpu=False)


def test_workload_rows_with_accumulation_cpu(tmp_path, _cpu):
    from ray_torch_distributed_checkpoint_amd import workloads as W

    kw = dict(steps=2, num_workers=1, use_gpu=False, ckpt_every_n_steps=2, verbose=0)
    # the loss of an accumulated step is the mean of its micro-batch losses: before the first
    # update, step 1 of k = 2 sees the batches of steps 1 and 2 of ... a model that step 1 of
    # the plain run already changed; so take a learning rate of ~0, under which both are one model
    plain = W.train_workload("gpt2-tiny", checkpoint_storage_path=str(tmp_path / "p"), lr=1e-30, **dict(kw, steps=4))
    accum = W.train_workload("gpt2-tiny", checkpoint_storage_path=str(tmp_path / "q"), lr=1e-30, grad_accum_steps=2,
                             **kw)
    lp, lq = _losses(plain.path), _losses(accum.path)
    assert sorted(lq) == [1, 2]
    for s in (1, 2):
        mean = (torch.tensor(lp[2 * s - 1], dtype=torch.float32) + torch.tensor(lp[2 * s], dtype=torch.float32)) / 2
        assert abs(lq[s] - float(mean)) <= 2e-6 * abs(float(mean)), (s, lq[s], float(mean))
    # grad_accum_steps=1 is the run without the option
    one = W.train_workload("gpt2-tiny", checkpoint_storage_path=str(tmp_path / "o"), grad_accum_steps=1, **kw)
    ref = W.train_workload("gpt2-tiny", checkpoint_storage_path=str(tmp_path / "r"), **kw)
    strip = lambda rows: [{k: v for k, v in r.items() if k == "step" or "loss" in k or k == "epoch"} for r in rows]
    assert strip(_rows(one.path)) == strip(_rows(ref.path))
    assert set(_rows(one.path)[0]) == set(_rows(ref.path)[0])


def test_throughput_counts_every_micro_batch():
    from ray_torch_distributed_checkpoint_amd import workloads as W

    assert W.samples_per_s(3, 1, 4, 2, 1.5) == 16.0
    assert W.samples_per_s(3, 2, 4, 2, 1.5) == 32.0  # k x the batch


def test_config_and_clis_carry_grad_accum_steps():
    import subprocess

    from ray_torch_distributed_checkpoint_amd import workloads as W

    assert W.WorkloadConfig().grad_accum_steps == 1
    assert W.WorkloadConfig.from_dict({"grad_accum_steps": 4, "unknown": 1}).grad_accum_steps == 4
    with pytest.raises(ValueError):
        W.train_workload("gpt2-tiny", steps=1, grad_accum_steps=0)
    env = dict(os.environ, PYTHONPATH=ROOT, RTDC_FORCE_CPU="1", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-m", "ray_torch_distributed_checkpoint_amd.workloads", "--help"], env=env,
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "--grad-accum-steps" in r.stdout, r.stderr[-2000:]
    src = open(os.path.join(ROOT, "train_flow.py")).read()
    assert 'Parameter("grad_accum_steps", default=1' in src
    assert "grad_accum_steps=int(self.grad_accum_steps)" in src
