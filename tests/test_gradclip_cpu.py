"""Global gradient-norm clipping fused into FusedAdamW / FusedSGD (`max_grad_norm`), CPU paths:
the per-tensor reference step, the flat ZeRO-1 reference step over gloo, the DDP deferred tail,
the workload plumbing (report rows, exact resume) and the unchanged checkpoint format.

Tolerances: fused-vs-torch is `rtol=1e-5, atol=1e-6`, what tests/test_optim.py uses for the
unclipped optimizers; clipping adds one fp32 multiply per gradient element and an fp32 norm
whose rounding error (a sum of non-negative terms) is far below that.
"""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import mp_util  # noqa: E402

RTOL, ATOL = 1e-5, 1e-6


def _mlp(seed=7):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(20, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64), torch.nn.ReLU(),
                               torch.nn.Linear(64, 5))


def _close(a, b) -> bool:
    return bool(torch.allclose(a, b, rtol=RTOL, atol=ATOL))


# ------------------------------------------------------------------ single process, per-tensor path
@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_plain_cpu_step_matches_torch_clip(kind):
    """Two param groups, one parameter without a gradient: norm, parameters and state follow
    clip_grad_norm_ + the torch optimizer; p.grad is left unscaled."""
    from ray_torch_distributed_checkpoint_amd.optim import FusedAdamW, FusedSGD

    ours_m, ref_m = _mlp(), _mlp()
    extra_o, extra_r = torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(3))  # never gets a gradient

    def groups(m, extra):
        ps = list(m.parameters())
        return [{"params": ps[:2], "lr": 2e-2, "weight_decay": 0.0},
                {"params": ps[2:] + [extra], "lr": 1e-2, "weight_decay": 0.1}]

    if kind == "adamw":
        ours = FusedAdamW(groups(ours_m, extra_o), max_grad_norm=0.05)
        ref = torch.optim.AdamW(groups(ref_m, extra_r))
    else:
        ours = FusedSGD(groups(ours_m, extra_o), momentum=0.9, max_grad_norm=0.05)
        ref = torch.optim.SGD(groups(ref_m, extra_r), momentum=0.9)
    assert ours.grad_norm is None
    g = torch.Generator().manual_seed(3)
    for _ in range(3):
        x, y = torch.randn(8, 20, generator=g), torch.randint(0, 5, (8,), generator=g)
        for m, opt in ((ours_m, ours), (ref_m, ref)):
            opt.zero_grad()
            torch.nn.functional.cross_entropy(m(x), y).backward()
        raw = [p.grad.clone() for p in ours_m.parameters()]
        norm = torch.nn.utils.clip_grad_norm_(list(ref_m.parameters()) + [extra_r], 0.05)
        ours.step()
        ref.step()
        assert float(norm) > 0.05  # the clip is active
        assert abs(float(ours.grad_norm) - float(norm)) <= 1e-5 * float(norm)
        assert all(torch.equal(p.grad, r) for p, r in zip(ours_m.parameters(), raw)), "p.grad must stay unscaled"
    assert ours.grad_norm.dim() == 0 and ours.grad_norm.dtype == torch.float32
    for a, b in zip(ours_m.parameters(), ref_m.parameters()):
        assert _close(a, b)
        for k, v in ref.state[b].items():
            if k != "step":
                assert _close(ours.state[a][k], v), k
    assert torch.equal(extra_o, extra_r)


def test_inactive_and_disabled_clip_are_the_unclipped_step():
    from ray_torch_distributed_checkpoint_amd.optim import FusedAdamW

    ms = [_mlp() for _ in range(3)]
    opts = [FusedAdamW(ms[0].parameters(), lr=1e-2), FusedAdamW(ms[1].parameters(), lr=1e-2, max_grad_norm=1e6),
            FusedAdamW(ms[2].parameters(), lr=1e-2, max_grad_norm=0)]
    x, y = torch.randn(8, 20), torch.randint(0, 5, (8,))
    for m, opt in zip(ms, opts):
        torch.nn.functional.cross_entropy(m(x), y).backward()
        opt.step()
    for a, b, c in zip(*(m.parameters() for m in ms)):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert opts[0].grad_norm is None and opts[2].grad_norm is None and opts[1].grad_norm is not None
    opts[0].max_grad_norm = 0.01  # settable later
    torch.nn.functional.cross_entropy(ms[0](x), y).backward()
    opts[0].step()
    assert float(opts[0].grad_norm) > 0.01


def test_state_dict_format_unchanged():
    """max_grad_norm is an attribute, not a param-group option: the checkpoint keys are today's."""
    from ray_torch_distributed_checkpoint_amd.optim import FusedAdamW, FusedSGD

    for cls, kw in ((FusedAdamW, {}), (FusedSGD, {"momentum": 0.9})):
        sds = []
        for clip in (None, 0.05):
            m = _mlp()
            opt = cls(m.parameters(), lr=1e-2, max_grad_norm=clip, **kw)
            torch.manual_seed(0)
            torch.nn.functional.cross_entropy(m(torch.randn(8, 20)), torch.randint(0, 5, (8,))).backward()
            opt.step()
            sds.append(opt.state_dict())
        a, b = sds
        assert a.keys() == b.keys()
        assert [g.keys() for g in a["param_groups"]] == [g.keys() for g in b["param_groups"]]
        assert "max_grad_norm" not in b["param_groups"][0] and "max_grad_norm" not in opt.defaults
        assert a["state"].keys() == b["state"].keys()
        assert all(a["state"][k].keys() == b["state"][k].keys() for k in a["state"])


# ------------------------------------------------------------------ two ranks over gloo
def _ddp_tail_clip(rank, world, comm):
    """defer_tail_to_optimizer with >= 3 tail pieces and an active clip vs torch DDP (with
    torch's own bf16 compression hook for bf16 communication: at 2 ranks its pre-division by
    the world size is exact, so both sides communicate the same bf16 values) +
    clip_grad_norm_ + torch AdamW, compared after every one of 3 steps.

    fp32 communication: the two runs are independent over the 3 steps.  bf16 communication: the
    reference takes over our parameters and Adam state after every comparison, so each step
    starts from a common state.  Rounding a gradient to bf16 is discontinuous: a 1-ulp fp32
    difference in the parameters (the two norms sum in different orders) flips the bf16
    rounding of some later gradient elements, a 2^-8 relative change that no fp32 tolerance
    covers (the unclipped bf16 test in tests/test_distributed_cpu.py allows 5e-3 for it)."""
    from ray_torch_distributed_checkpoint_amd.optim import FusedAdamW
    from ray_torch_distributed_checkpoint_amd.parallel.ddp import DistributedDataParallel

    base = _mlp()
    ours_m, ref_m = copy.deepcopy(base), copy.deepcopy(base)
    ours = DistributedDataParallel(ours_m, bucket_cap_mb=0.01, first_bucket_mb=0.005, defer_tail_to_optimizer=True,
                                   tail_piece_mb=0.002 if comm == "fp32" else 0.001, grad_comm_dtype=comm)
    ref = torch.nn.parallel.DistributedDataParallel(ref_m)
    if comm == "bf16":
        from torch.distributed.algorithms.ddp_comm_hooks import default_hooks

        ref.register_comm_hook(None, default_hooks.bf16_compress_hook)
    clip = 0.05
    opt_o = FusedAdamW(ours.parameters(), lr=1e-2, weight_decay=0.1, max_grad_norm=clip)
    opt_r = torch.optim.AdamW(ref.parameters(), lr=1e-2, weight_decay=0.1)
    g = torch.Generator().manual_seed(100 + rank)
    pieces, norms = [], []
    ok, err = True, 0.0
    for _ in range(3):
        x = torch.randn(8, 20, generator=g)
        y = torch.randint(0, 5, (8,), generator=g)
        for m, opt in ((ours, opt_o), (ref, opt_r)):
            opt.zero_grad()
            torch.nn.functional.cross_entropy(m(x), y).backward()
        pieces.append(len(ours.space.pending_tail) if ours.space.pending_tail else 0)
        opt_o.step()
        assert ours.space.pending_tail is None
        norms.append((float(opt_o.grad_norm), float(torch.nn.utils.clip_grad_norm_(ref.parameters(), clip))))
        opt_r.step()
        with torch.no_grad():
            for a, b in zip(ours_m.parameters(), ref_m.parameters()):
                ok = ok and _close(a, b)
                err = max(err, float((a - b).abs().max()))
                for k in ("exp_avg", "exp_avg_sq"):
                    ok = ok and _close(opt_o.state[a][k], opt_r.state[b][k])
                    if comm == "bf16":
                        opt_r.state[b][k].copy_(opt_o.state[a][k])
                if comm == "bf16":
                    b.copy_(a)
    return ok, err, pieces, norms


@pytest.mark.parametrize("comm", ["fp32", "bf16"])
def test_ddp_deferred_tail_with_clip_matches_torch(comm):
    out = mp_util.run(_ddp_tail_clip, 2, comm)
    for ok, err, pieces, norms in out:
        print(comm, "max abs parameter difference", err, "tail pieces", pieces, "norms", norms)
    for ok, err, pieces, norms in out:
        assert all(n >= 3 for n in pieces), pieces
        assert all(theirs > 0.05 for _, theirs in norms), norms  # active at every step
        assert all(abs(mine - theirs) <= 1e-5 * theirs for mine, theirs in norms), norms
        assert ok, err
    assert out[0][3] == out[1][3]


def _zero_clip(rank, world):
    """ZeRO-1 (flat CPU reference path: owned shards, all-gathered local sums) vs the replicated
    two-rank run, clip active."""
    from ray_torch_distributed_checkpoint_amd.models import GPT2, GPT2Config
    from ray_torch_distributed_checkpoint_amd.optim import FusedAdamW
    from ray_torch_distributed_checkpoint_amd.parallel.ddp import DistributedDataParallel

    out = {}
    for zero in (0, 1):
        torch.manual_seed(0)
        model = GPT2(GPT2Config.named("gpt2-tiny"))
        net = DistributedDataParallel(model, bucket_cap_mb=0.25, first_bucket_mb=0.05, zero_stage=zero)
        opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.1, max_grad_norm=0.05)
        norms = []
        for k in range(3):
            g = torch.Generator().manual_seed(11 + k)
            data = torch.randint(0, 1000, (2 * world, 33), generator=g)[2 * rank:2 * rank + 2]
            net(data[:, :-1], data[:, 1:]).backward()
            opt.step()
            opt.zero_grad()
            norms.append(opt.grad_norm.clone())
        assert (net.space.zero is not None) == bool(zero)
        # (numpy: a tensor in the result queue would be shared memory owned by an exiting process)
        out[zero] = (torch.stack(norms).numpy(), [p.detach().numpy().copy() for p in model.parameters()])
    return out


def test_zero1_with_clip_matches_replicated():
    out = mp_util.run(_zero_clip, 2)
    for r in range(2):
        (n0, p0), (n1, p1) = out[r][0], out[r][1]
        print("rank", r, "replicated norms", n0.tolist(), "zero norms", n1.tolist())
        assert (n0 > 0.05).all()
        assert np.array_equal(n1, out[0][1][0]), "the ZeRO-1 norm must be bitwise equal on both ranks"
        np.testing.assert_allclose(n1, n0, rtol=1e-5, atol=0)
        for a, b in zip(p1, p0):
            np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL)
        for a, b in zip(p1, out[0][1][1]):
            assert np.array_equal(a, b)


# ------------------------------------------------------------------ workload plumbing
def _rows(path):
    return [json.loads(line) for line in open(os.path.join(path, "result.json"))]


def _by_step(rows, key):
    out = {}
    for row in rows:
        for i, v in enumerate(reversed(row[key])):
            out[row["step"] - i] = v
    return out


def run_resume_case(tmp_path, use_gpu: bool):
    """6 steps with a checkpoint every 3 and a clip below every step's norm; an exact resume
    from the step-3 checkpoint reproduces losses and norms of steps 4-6 bit for bit."""
    from ray_torch_distributed_checkpoint_amd import train
    from ray_torch_distributed_checkpoint_amd import workloads as W

    m = 0.05
    kw = dict(steps=6, num_workers=1, use_gpu=use_gpu, ckpt_every_n_steps=3, verbose=0, max_grad_norm=m)
    a = W.train_workload("gpt2-tiny", checkpoint_storage_path=str(tmp_path / "a"), **kw)
    rows = _rows(a.path)
    assert [r["step"] for r in rows] == [3, 6]
    assert all(r["grad_norm"] == r["grad_norms"][-1] and len(r["grad_norms"]) == len(r["losses"]) for r in rows)
    na, la = _by_step(rows, "grad_norms"), _by_step(rows, "losses")
    assert sorted(na) == list(range(1, 7))
    print("grad norms", na)
    assert min(na.values()) > m, na  # the clip is active at every step
    cks = sorted(d for d in os.listdir(a.path) if d.startswith("checkpoint_"))
    assert len(cks) == 2
    ck = train.Checkpoint.from_directory(os.path.join(a.path, cks[0]))
    b = W.train_workload("gpt2-tiny", checkpoint_storage_path=str(tmp_path / "b"), checkpoint=ck,
                         resume_mode="exact", **kw)
    rows_b = _rows(b.path)
    nb, lb = _by_step(rows_b, "grad_norms"), _by_step(rows_b, "losses")
    assert sorted(nb) == [4, 5, 6]
    assert nb == {k: na[k] for k in (4, 5, 6)}
    assert lb == {k: la[k] for k in (4, 5, 6)}
    return a


def test_workload_rows_and_exact_resume_cpu(tmp_path, monkeypatch):
    from ray_torch_distributed_checkpoint_amd import workloads as W

    monkeypatch.setenv("RTDC_FORCE_CPU", "1")
    for k in ("RTDC_FAIL_AT_STEP", "RTDC_HANG_AT_STEP", "RTDC_FAIL_AT_REPORT"):
        monkeypatch.delenv(k, raising=False)
    run_resume_case(tmp_path, use_gpu=False)
    # clipping off: the rows are what they were
    c = W.train_workload("gpt2-tiny", steps=2, num_workers=1, use_gpu=False, ckpt_every_n_steps=2, verbose=0,
                         checkpoint_storage_path=str(tmp_path / "c"))
    for row in _rows(c.path):
        assert "grad_norm" not in row and "grad_norms" not in row


def test_workload_config_and_cli_carry_the_knob():
    from ray_torch_distributed_checkpoint_amd import workloads as W

    assert W.WorkloadConfig().max_grad_norm is None
    assert W.WorkloadConfig.from_dict({"max_grad_norm": 1.0}).max_grad_norm == 1.0
    wl = W.build(W.WorkloadConfig(model="gpt2-tiny", max_grad_norm=1.0), torch.device("cpu"))
    assert wl.optimizer.max_grad_norm == 1.0
    assert W.build(W.WorkloadConfig(model="gpt2-tiny"), torch.device("cpu")).optimizer.max_grad_norm is None
