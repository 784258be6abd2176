"""Learning-rate schedules (optim/schedule.py) on the CPU: the multipliers against their closed
form and torch's LambdaLR, a scheduled fused optimizer against torch and - bitwise - against the
same optimizer whose `group["lr"]` the caller sets by hand, the host-built tables of the capturable
step, state_dict / reload, the workload rows and kill-restart, ZeRO-1 on gloo, argument errors."""
import json
import math
import os
import socket
import sys
import traceback

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ray_torch_distributed_checkpoint_amd.optim import FusedAdamW, FusedSGD, LRSchedule  # noqa: E402
from ray_torch_distributed_checkpoint_amd.optim import schedule as S  # noqa: E402


# ------------------------------------------------------------------------------- closed form
def _closed(kind, w, total, r, k):
    """The documented multiplier of the (k + 1)-th optimizer step, written out independently."""
    k = min(k, total - 1)
    if k < w:
        return (k + 1) / w
    s = max(w - 1, 0)
    p = (k - s) / (total - 1 - s)
    if kind == "cosine":
        return r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * p))
    return r + (1.0 - r) * (1.0 - p)


def _make(kind, w=3, total=10, r=0.1):
    return LRSchedule.warmup_cosine(w, total, r) if kind == "cosine" else LRSchedule.warmup_linear(w, total, r)


@pytest.mark.parametrize("kind", ["cosine", "linear"])
def test_multipliers_equal_closed_form_and_lambdalr(kind):
    s = _make(kind)
    base = 3e-3
    q = torch.nn.Parameter(torch.zeros(3))
    ref = torch.optim.AdamW([q], lr=base)
    lam = torch.optim.lr_scheduler.LambdaLR(ref, lambda k: _closed(kind, 3, 10, 0.1, k))
    for n in range(1, 15):  # four steps past the end
        f = s.multiplier(n - 1)
        assert f == _closed(kind, 3, 10, 0.1, n - 1), n
        assert s.lr(base, n) == base * f
        assert lam.get_last_lr() == [base * f], n  # the lr torch's step n runs with
        q.grad = torch.ones(3)
        ref.step()
        lam.step()
    # shape of the schedule: warmup 1/3, 2/3, 1; min_lr_ratio exactly at step total_steps, kept afterwards
    assert [s(k) for k in range(3)] == [1 / 3, 2 / 3, 1.0]
    assert s(9) == 0.1 and s(10) == 0.1 and s(1000) == 0.1
    assert all(s(k) > s(k + 1) for k in range(2, 9))
    assert LRSchedule.constant()(0) == 1.0 and LRSchedule.constant()(99) == 1.0
    sq = LRSchedule.from_fn(lambda k: 1.0 / (k + 1), 4)
    assert [sq(k) for k in range(6)] == [1.0, 0.5, 1 / 3, 0.25, 0.25, 0.25]


# ------------------------------------------------------------------- optimizers against torch
def _params(seed=0):
    torch.manual_seed(seed)
    return [torch.randn(s) for s in [(33, 17), (17,), (64, 8), (5,)]]


def _grads(n_steps, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(b.shape, generator=g) for b in _params()] for _ in range(n_steps)]


def _adamw(ps, **kw):
    return FusedAdamW(ps, lr=0.01, betas=(0.9, 0.95), weight_decay=0.1, **kw)


def _sgd(ps, **kw):
    return FusedSGD(ps, lr=0.01, momentum=0.9, nesterov=True, weight_decay=0.05, **kw)


def _step(opt, ps, grads):
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    opt.step()
    opt.zero_grad(set_to_none=True)


def _bits_equal(a, b):
    return all(torch.equal(x.detach(), y.detach()) for x, y in zip(a, b))


@pytest.mark.parametrize("make", [_adamw, _sgd])
def test_scheduled_optimizer_is_bitwise_hand_set_lr(make):
    sch = LRSchedule.warmup_cosine(3, 10, 0.1)
    grads = _grads(12)
    ps = [torch.nn.Parameter(b.clone()) for b in _params()]
    qs = [torch.nn.Parameter(b.clone()) for b in _params()]
    opt, hand = make(ps, lr_schedule=sch), make(qs)
    assert opt.lr_schedule is sch and hand.lr_schedule is None
    for n in range(1, 13):
        for g in hand.param_groups:
            g["lr"] = 0.01 * _closed("cosine", 3, 10, 0.1, n - 1)
        _step(opt, ps, grads[n - 1])
        _step(hand, qs, grads[n - 1])
        assert opt.step_count == n
        assert opt.get_last_lr() == [0.01 * _closed("cosine", 3, 10, 0.1, n - 1)]
        assert _bits_equal(ps, qs), n
    sa, sb = opt.state_dict()["state"], hand.state_dict()["state"]
    for i in sa:
        for k, v in sa[i].items():
            assert torch.equal(v, sb[i][k]), (i, k)


def test_scheduled_adamw_against_torch_lambdalr():
    sch = LRSchedule.warmup_cosine(3, 10, 0.1)
    grads = _grads(12)
    ps = [torch.nn.Parameter(b.clone()) for b in _params()]
    qs = [torch.nn.Parameter(b.clone()) for b in _params()]
    opt = _adamw(ps, lr_schedule=sch)
    ref = torch.optim.AdamW(qs, lr=0.01, betas=(0.9, 0.95), weight_decay=0.1, foreach=False)
    lam = torch.optim.lr_scheduler.LambdaLR(ref, sch.multiplier)
    for n in range(12):
        _step(opt, ps, grads[n])
        _step(ref, qs, grads[n])
        assert opt.get_last_lr() == lam.get_last_lr()
        lam.step()
    for p, q in zip(ps, qs):
        torch.testing.assert_close(p.detach(), q.detach(), rtol=1e-5, atol=1e-6)


def test_schedule_set_later_and_flat_cpu_path():
    """`opt.lr_schedule = s` after construction; the flat CPU step (bf16 state) takes the same lr."""
    sch = LRSchedule.warmup_linear(2, 6)
    grads = _grads(7)
    ps = [torch.nn.Parameter(b.clone()) for b in _params()]
    qs = [torch.nn.Parameter(b.clone()) for b in _params()]
    opt = _adamw(ps, state_dtype=torch.bfloat16, capturable=True)  # (the CPU accepts capturable: host path)
    opt.lr_schedule = sch
    hand = _adamw(qs, state_dtype=torch.bfloat16)
    for n in range(1, 8):
        hand.param_groups[0]["lr"] = 0.01 * _closed("linear", 2, 6, 0.0, n - 1)
        _step(opt, ps, grads[n - 1])
        _step(hand, qs, grads[n - 1])
        assert _bits_equal(ps, qs), n
    assert opt.get_last_lr() == [0.0]


# ------------------------------------------------------------------------------------ tables
def test_lr_and_bias_correction_tables():
    sch = LRSchedule.warmup_cosine(3, 10, 0.1)
    bases = [0.01, 3e-4]
    tab = S.lr_table(bases, sch)
    assert tab.dtype == np.float32 and tab.shape == (2, 10)
    for g, b in enumerate(bases):
        for k in range(10):
            assert tab[g, k] == np.float32(b * sch.multiplier(k))
    assert S.lr_table(bases).shape == (2, 1) and S.lr_table(bases)[1, 0] == np.float32(3e-4)
    assert S.lr_table(bases, LRSchedule.constant()).shape == (2, 1)
    for (b1, b2), rows in (((0.5, 0.5), 25), ((0.9, 0.95), 325)):
        bc = S.bias_correction_table(b1, b2)
        assert bc.dtype == np.float32 and bc.shape == (rows, 2)
        for t in range(1, rows + 1):
            assert bc[t - 1, 0] == np.float32(1 - b1 ** t) and bc[t - 1, 1] == np.float32(math.sqrt(1 - b2 ** t)), t
        assert tuple(bc[-1]) == (1.0, 1.0) and tuple(bc[-2]) != (1.0, 1.0)
        for t in (rows + 1, 10 * rows):  # they stay 1.0f
            assert np.float32(1 - b1 ** t) == 1.0 and np.float32(math.sqrt(1 - b2 ** t)) == 1.0
    assert 16000 < S.bias_correction_table(0.9, 0.999).shape[0] < 17500
    with pytest.raises(ValueError):
        S.bias_correction_table(0.9, 0.9999999)  # ~1.7e8 rows
    with pytest.raises(ValueError):
        FusedAdamW([torch.nn.Parameter(torch.zeros(3))], betas=(0.9, 0.9999999), capturable=True)
    FusedAdamW([torch.nn.Parameter(torch.zeros(3))], betas=(0.9, 0.9999999))  # the host path takes any betas


# ------------------------------------------------------------------------ state dict, reload
@pytest.mark.parametrize("make", [_adamw, _sgd])
def test_state_dict_keys_unchanged_and_reload_continues_bitwise(make):
    sch = LRSchedule.warmup_cosine(3, 10, 0.1)
    grads = _grads(8)
    ps = [torch.nn.Parameter(b.clone()) for b in _params()]
    qs = [torch.nn.Parameter(b.clone()) for b in _params()]
    us = [torch.nn.Parameter(b.clone()) for b in _params()]
    opt, full, plain = make(ps, lr_schedule=sch), make(qs, lr_schedule=sch), make(us)
    for n in range(5):
        _step(opt, ps, grads[n])
        _step(full, qs, grads[n])
        _step(plain, us, grads[n])
    sd, psd = opt.state_dict(), plain.state_dict()
    assert sorted(sd) == sorted(psd)
    assert [sorted(g) for g in sd["param_groups"]] == [sorted(g) for g in psd["param_groups"]]
    assert sorted(sd["state"]) == sorted(psd["state"])
    for i in sd["state"]:
        assert sorted(sd["state"][i]) == sorted(psd["state"][i])
    # a fresh optimizer and schedule, loaded: the step number comes back with the state
    rs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt2 = make(rs, lr_schedule=LRSchedule.warmup_cosine(3, 10, 0.1))
    opt2.load_state_dict(sd)
    if make is _adamw:
        assert opt2.step_count == 5
    else:  # torch's SGD state has no step number: the caller supplies it
        opt2.step_count = 5
    for n in range(5, 8):
        _step(opt2, rs, grads[n])
        _step(full, qs, grads[n])
        assert _bits_equal(rs, qs), n
    assert opt2.step_count == 8 and opt2.get_last_lr() == full.get_last_lr()


# -------------------------------------------------------------------------- workload rows
@pytest.fixture
def _cpu_workload(monkeypatch):
    monkeypatch.setenv("RTDC_FORCE_CPU", "1")
    for k in ("RTDC_FAIL_AT_STEP", "RTDC_HANG_AT_STEP", "RTDC_FAIL_AT_REPORT"):
        monkeypatch.delenv(k, raising=False)


def _rows(result_path):
    return [json.loads(line) for line in open(os.path.join(result_path, "result.json"))]


def _losses(result_path) -> dict:
    out = {}
    for row in _rows(result_path):
        for i, v in enumerate(reversed(row["losses"])):
            k = row["step"] - i
            assert out.get(k, v) == v, f"step {k} logged twice with different losses"
            out[k] = v
    return out


def _fit(tmp, name, steps=8, workers=2, **kw):
    from ray_torch_distributed_checkpoint_amd import workloads as W

    return W.train_workload("gpt2-tiny", steps=steps, num_workers=workers, ckpt_every_n_steps=2,
                            checkpoint_storage_path=str(tmp / name), verbose=0, **kw)


def test_workload_rows_carry_lr_and_kill_restart_is_bit_equal(tmp_path, monkeypatch, _cpu_workload):
    kw = dict(lr_schedule="cosine", warmup_steps=3)
    a = _fit(tmp_path, "a", **kw)
    rows = _rows(a.path)
    assert [r["step"] for r in rows] == [2, 4, 6, 8]
    for r in rows:  # gpt2-tiny's lr is 1e-3; the decay ends at `steps`
        assert r["lr"] == 1e-3 * _closed("cosine", 3, 8, 0.0, r["step"] - 1)
    assert rows[-1]["lr"] == 0.0
    monkeypatch.setenv("RTDC_FAIL_AT_STEP", "5:1")
    b = _fit(tmp_path, "b", max_failures=1, **kw)
    la, lb = _losses(a.path), _losses(b.path)
    assert sorted(la) == list(range(1, 9)) and la == lb
    assert [r["lr"] for r in _rows(b.path) if r["step"] == 8] == [0.0]
    monkeypatch.delenv("RTDC_FAIL_AT_STEP")
    c = _fit(tmp_path, "c", steps=4)  # the defaults: no schedule, today's row keys
    assert all("lr" not in r for r in _rows(c.path))
    d = _fit(tmp_path, "d", steps=4, lr_schedule="constant", warmup_steps=0, min_lr_ratio=0.0)
    assert [sorted(r) for r in _rows(d.path)] == [sorted(r) for r in _rows(c.path)]
    assert _losses(c.path) == _losses(d.path)
    assert _losses(c.path)[2] != la[2]  # (the schedule really changed the run: step 1 ran at lr / 3)


# ------------------------------------------------------------------------------ ZeRO-1, gloo
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(37, 129)
        self.b = torch.nn.Linear(129, 65)
        self.c = torch.nn.Linear(65, 10)

    def forward(self, x):
        return self.c(torch.relu(self.b(torch.relu(self.a(x)))))


def _zero_worker(rank, world, port, zero, q):
    try:
        import torch.distributed as dist

        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.set_num_threads(1)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from ray_torch_distributed_checkpoint_amd.parallel.ddp import DistributedDataParallel

        torch.manual_seed(0)
        model = _Net()
        net = DistributedDataParallel(model, bucket_cap_mb=0.02, first_bucket_mb=0.005, zero_stage=zero)
        opt = FusedAdamW(model.parameters(), lr=1e-2, weight_decay=0.1, lr_schedule=LRSchedule.warmup_cosine(2, 5, 0.1))
        g = torch.Generator().manual_seed(rank + 11)
        lrs = []
        for _ in range(6):
            net(torch.randn(8, 37, generator=g)).square().mean().backward()
            opt.step()
            opt.zero_grad()
            lrs.append(opt.get_last_lr()[0])
        sd = opt.state_dict()
        state = {k: {n: v.numpy().copy() for n, v in st.items() if torch.is_tensor(v)} for k, st in sd["state"].items()}
        params = {n: p.detach().numpy().copy() for n, p in model.named_parameters()}
        q.put((rank, "ok", (params, state, lrs, opt.step_count)))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        q.put((rank, "err", traceback.format_exc()))


def _zero_run(world, zero):
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_zero_worker, args=(r, world, port, zero, q)) for r in range(world)]
    for p in ps:
        p.start()
    out = {}
    try:
        for _ in range(world):
            r, st, v = q.get(timeout=180)
            assert st == "ok", v
            out[r] = v
    finally:
        for p in ps:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    return out


def test_zero1_scheduled_equals_replicated_scheduled():
    """Two ranks: bitwise, as tests/test_zero_cpu.py asserts for the unscheduled comparison."""
    base, z = _zero_run(2, 0), _zero_run(2, 1)
    want = [1e-2 * _closed("cosine", 2, 5, 0.1, k) for k in range(6)]
    for r in range(2):
        assert z[r][2] == want and base[r][2] == want and z[r][3] == 6
        for n, v in base[0][0].items():
            assert np.array_equal(z[r][0][n], v), (r, n)
        for k, st in base[0][1].items():
            for name, v in st.items():
                assert np.array_equal(z[r][1][k][name], v), (r, k, name)


# --------------------------------------------------------------------------- argument errors
def test_argument_errors():
    for ctor in (LRSchedule.warmup_cosine, LRSchedule.warmup_linear):
        with pytest.raises(ValueError):
            ctor(11, 10)  # warmup_steps > total_steps
        with pytest.raises(ValueError):
            ctor(0, 0)  # total_steps < 1
        with pytest.raises(ValueError):
            ctor(2, 10, -0.1)
        with pytest.raises(ValueError):
            ctor(2, 10, 1.5)
        ctor(10, 10)
        ctor(0, 1, 1.0)
    with pytest.raises(ValueError):
        LRSchedule.from_fn(lambda k: 1.0, 0)
    with pytest.raises(TypeError):
        FusedAdamW([torch.nn.Parameter(torch.zeros(3))], lr_schedule=lambda k: 1.0)
    from ray_torch_distributed_checkpoint_amd import workloads as W

    with pytest.raises(ValueError):
        W.train_workload("gpt2-tiny", steps=4, lr_schedule="exponential")
    with pytest.raises(ValueError):
        W.train_workload("gpt2-tiny", steps=4, lr_schedule="cosine", warmup_steps=5)
