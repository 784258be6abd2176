"""Label smoothing and z-loss in the cross-entropy, checked without a GPU:

* the reference of tests/xent_aux_ref.py: the twin condition on its whole (e, z) table (which fixes
  FLOOR_XENT_AUX_U: half of it leaves the ceiling), bit-equality with ulp.xent_ref at e = z = 0,
  agreement with autograd through torch's own label-smoothed cross-entropy, and five deliberate
  errors that each leave the allowance a kernel is given;
* the CPU paths of ops.cross_entropy / ops.lm_head_cross_entropy: values, the (loss, ce) contract,
  the ValueErrors;
* the workload plumbing: rows, exact resume, accumulation, the command lines.
"""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import ulp as U  # noqa: E402
from tests import xent_aux_ref as A  # noqa: E402

F64, F32 = U.F64, U.F32


# ------------------------------------------------------------------------------- the reference
def test_twin_condition_on_the_whole_table():
    """every (e, z) of the table x every dispatch arm x random / planted rows x both grad scales:
    the fp32 twin stays under its ceilings for grad, loss, ce and lse (Judge.check fails otherwise)"""
    J = U.Judge()
    for e, z in A.XENT_AUX_TABLE:
        for dt, V, ld, arm in U.XENT_ARMS:
            for planted in (False, True):
                c = U.xent_inputs(dt, V, ld, planted)
                for gs in (1.0, 1.0 / 7):
                    A.judge_xent_aux(J, "xent-aux", (arm, V, ld, "planted" if planted else "randn", round(gs, 3), e, z),
                                     c, gs, e, z, {}, threads=U.xent_threads(arm))
    J.check()


def test_floor_is_the_smallest_power_of_two_that_holds_the_ceiling():
    tab = A.twin_table(candidates=(-8, -7))
    assert max(w[1] for w in tab.values()) <= U.TWIN_ULP_CEIL          # 2^-7 holds on every (e, z)
    assert max(w[0] for w in tab.values()) > U.TWIN_ULP_CEIL           # 2^-8 does not
    assert A.FLOOR_XENT_AUX_U == 2.0 ** -7


@pytest.mark.parametrize("dtype", [F64, F32])
def test_zero_coefficients_give_xent_ref_bit_for_bit(dtype):
    for dt, V, ld, _ in U.XENT_ARMS:
        for planted in (False, True):
            c = U.xent_inputs(dt, V, ld, planted)
            for gs in (1.0, 1.0 / 7):
                a = A.xent_aux_ref(dtype, c["logits"], c["target"], V, gs, 0.0, 0.0)
                r = U.xent_ref(dtype, c["logits"], c["target"], V, gs)
                for k in ("grad", "loss", "lse", "lse_scale", "loss_scale", "tmask"):
                    assert torch.equal(a[k], r[k]), (k, V, ld, planted, gs)
                assert torch.equal(a["ce"], r["loss"])


@pytest.mark.parametrize("e,z", A.XENT_AUX_TABLE)
def test_float64_reference_agrees_with_autograd(e, z):
    """F.cross_entropy(label_smoothing=e, ignore_index=-100) + z * logsumexp^2 averaged over the
    valid rows, differentiated by autograd, against the written-out formulas: 1e-12"""
    ef, zf = U._f32(e), U._f32(z)   # the coefficients the helper uses
    for dt, V, ld, planted in ((U.BF16, 333, 333, False), (U.BF16, 8185, 8192, True), (F32, 10, 16, False)):
        c = U.xent_inputs(dt, V, ld, planted)
        x = c["logits"][:, :V].double().requires_grad_(True)
        keep = c["target"] != U.IGNORE_INDEX
        n = int(keep.sum())
        lse = torch.logsumexp(x, 1)
        loss = F.cross_entropy(x, c["target"], ignore_index=U.IGNORE_INDEX, label_smoothing=ef) + \
            zf * (lse * lse)[keep].sum() / n
        loss.backward()
        gs = 1.0 / n
        r = A.xent_aux_ref(F64, c["logits"], c["target"], V, gs, e, z)
        gsf = U._f32(gs)    # the helper's grad_scale is an fp32 value: take it out again
        assert (r["grad"] / gsf * gs - x.grad).abs().max().item() <= 1e-12 * max(1.0, x.grad.abs().max().item())
        assert abs((r["loss"].sum() / n - loss.detach()).item()) <= 1e-12 * abs(loss.item())
        assert (r["grad"][~keep] == 0).all() and (r["loss"][~keep] == 0).all() and (r["ce"][~keep] == 0).all()
        plain = F.cross_entropy(x.detach(), c["target"], ignore_index=U.IGNORE_INDEX)
        assert abs((r["ce"].sum() / n - plain).item()) <= 1e-12 * abs(plain.item())


def _caught(mutant, e, z, V=333, ld=344, gs=1.0 / 7):
    """(grad caught, loss caught): the mutant's fp32 outputs - the gradient rounded to bf16 like a
    kernel's - against the allowance a kernel is given on the same case"""
    c = U.xent_inputs(U.BF16, V, ld, planted=False)
    a = (c["logits"], c["target"], V, gs, e, z)
    r, t, m = A.xent_aux_ref(F64, *a), A.xent_aux_ref(F32, *a), A.xent_aux_ref(F32, *a, mutant=mutant)
    fl = A.xent_aux_grad_floor(r, V, gs, e)
    allow = U.allow_bf16(U.ulp_err(t["grad"], r["grad"], fl), 1)
    assert U.ulp_err(t["grad"].to(U.BF16), r["grad"], fl) <= allow      # the honest twin is inside
    g = U.ulp_err(m["grad"].to(U.BF16), r["grad"], fl) > allow
    R = -(-ld // 256)
    la = U.allow_f32(U.rel_err(t["loss"], r["loss"], r["loss_scale"]), R)
    return g, U.rel_err(m["loss"], r["loss"], r["loss_scale"]) > la


@pytest.mark.parametrize("mutant,e,z,where", [("u_ld", 0.1, 1e-4, "grad"), ("a_half", 0.0, 1e-2, "grad"),
                                              ("a_half", 0.1, 1e-2, "grad"), ("hot_one", 0.1, 0.0, "grad"),
                                              ("ignored_u", 0.1, 1e-4, "grad"), ("pad_sum", 0.1, 1e-4, "loss")])
def test_deliberate_errors_leave_the_allowance(mutant, e, z, where):
    g, l = _caught(mutant, e, z)
    assert g if where == "grad" else l, (mutant, g, l)
    if mutant == "pad_sum":
        assert not g   # the row sum enters the loss alone


# ------------------------------------------------------------------------------- CPU paths of the ops
def _torch_loss(x, t, e, z):
    keep = t != U.IGNORE_INDEX
    lse = torch.logsumexp(x, 1)
    return F.cross_entropy(x, t, ignore_index=U.IGNORE_INDEX, label_smoothing=e) + \
        z * (lse * lse)[keep].sum() / max(int(keep.sum()), 1)


@pytest.mark.parametrize("e,z", [(0.1, 0.0), (0.0, 1e-2), (0.1, 1e-2)])
def test_cpu_paths_follow_torch(e, z):
    from ray_torch_distributed_checkpoint_amd import ops

    torch.manual_seed(3)
    M, V = 12, 37
    x = (torch.randn(M, V) * 2).requires_grad_(True)
    t = torch.randint(0, V, (M,))
    t[3] = U.IGNORE_INDEX
    want = _torch_loss(x, t, e, z)
    gw, = torch.autograd.grad(want, x)
    loss, ce = ops.cross_entropy(x, t, label_smoothing=e, z_loss=z, return_ce=True)
    gl, = torch.autograd.grad(loss, x)
    assert torch.allclose(loss, want, rtol=1e-6, atol=0) and torch.allclose(gl, gw, rtol=1e-5, atol=1e-8)
    assert ce.dim() == 0 and ce.dtype == torch.float32 and not ce.requires_grad
    assert torch.allclose(ce, F.cross_entropy(x.detach(), t, ignore_index=U.IGNORE_INDEX), rtol=1e-6, atol=0)
    assert torch.equal(ops.cross_entropy(x, t, label_smoothing=e, z_loss=z), loss)   # the loss alone
    # the LM head: a padded vocabulary matrix, the targets over the first V rows of it
    C, Vp = 16, 40
    h = torch.randn(2, 6, C, requires_grad=True)
    w = torch.randn(Vp, C, requires_grad=True)
    tt = torch.randint(0, V, (2, 6))
    tt[0, 2] = U.IGNORE_INDEX
    want = _torch_loss(F.linear(h, w)[..., :V].reshape(-1, V), tt.reshape(-1), e, z)
    loss, ce = ops.lm_head_cross_entropy(h, w, tt, V, label_smoothing=e, z_loss=z, return_ce=True)
    assert torch.allclose(loss, want, rtol=1e-6, atol=0)
    gh, gw_ = torch.autograd.grad(loss, (h, w))
    wh, ww = torch.autograd.grad(want, (h, w))
    assert torch.allclose(gh, wh, rtol=1e-5, atol=1e-8) and torch.allclose(gw_, ww, rtol=1e-5, atol=1e-8)
    assert (gw_[V:] == 0).all()
    assert ce.dim() == 0 and not ce.requires_grad
    plain = ops.lm_head_cross_entropy(h, w, tt, V)
    assert torch.allclose(ce, plain.detach(), rtol=1e-6, atol=0)


def test_defaults_are_the_plain_loss_and_bad_coefficients_raise():
    from ray_torch_distributed_checkpoint_amd import ops

    torch.manual_seed(4)
    x, t = torch.randn(9, 11), torch.randint(0, 11, (9,))
    plain = F.cross_entropy(x, t, ignore_index=U.IGNORE_INDEX)
    assert torch.equal(ops.cross_entropy(x, t), plain)
    assert torch.equal(ops.cross_entropy(x, t, label_smoothing=0.0, z_loss=0.0), plain)
    loss, ce = ops.cross_entropy(x, t, return_ce=True)
    assert torch.equal(loss, plain) and torch.equal(ce, plain) and not ce.requires_grad
    h, w = torch.randn(3, 4), torch.randn(11, 4)
    for bad in ({"label_smoothing": 1.0}, {"label_smoothing": -0.1}, {"z_loss": -1e-4}, {"label_smoothing": float("nan")}):
        with pytest.raises(ValueError):
            ops.cross_entropy(x, t, **bad)
        with pytest.raises(ValueError):
            ops.lm_head_cross_entropy(h, w, t[:3], 11, **bad)


def test_native_bindings_check_the_coefficients_and_keep_the_positional_calls():
    """the checks run ahead of every device check, so they answer without a GPU; a positional call
    without the keywords still reaches the device check (RuntimeError: no GPU tensor)"""
    from ray_torch_distributed_checkpoint_amd.ops._ext import ext

    m = ext()
    x = torch.randn(4, 8)
    t = torch.zeros(4, dtype=torch.int64)
    f = torch.zeros(4)
    for bad in ({"label_smoothing": 1.0}, {"label_smoothing": -0.5}, {"z_loss": -1.0}):
        with pytest.raises(ValueError):
            m.xent(x, None, t, f, None, None, 4, 8, 8, 1.0, U.IGNORE_INDEX, **bad)
        with pytest.raises(ValueError):
            m.xent_bwd(x, x.clone(), t, f, f[:1], f[:1], U.IGNORE_INDEX, **bad)
    with pytest.raises(RuntimeError, match="GPU"):
        m.xent(x, None, t, f, None, None, 4, 8, 8, 1.0, U.IGNORE_INDEX)
    with pytest.raises(RuntimeError, match="GPU"):
        m.xent(x, None, t, f, None, None, 4, 8, 8, 1.0, U.IGNORE_INDEX, label_smoothing=0.1, z_loss=1e-4, ce=f)


# ------------------------------------------------------------------------------- models and workloads
def test_models_take_the_terms_as_plain_attributes():
    from ray_torch_distributed_checkpoint_amd.models import GPT2, GPT2Config, Llama, LlamaConfig

    for make in (lambda **kw: GPT2(GPT2Config.named("gpt2-tiny"), **kw),
                 lambda **kw: Llama(LlamaConfig.named("llama3-tiny"), **kw)):
        torch.manual_seed(0)
        m = make()
        assert m.z_loss == 0.0 and m.label_smoothing == 0.0 and m.last_ce is None
        keys = set(m.state_dict())
        assert not any("z_loss" in k or "smoothing" in k or "last_ce" in k for k in keys)
        V = m.cfg.vocab_size
        idx = torch.randint(0, V, (2, 17))
        plain = m(idx[:, :-1], idx[:, 1:])
        assert m.last_ce is None                       # both off: nothing new is made
        m.z_loss, m.label_smoothing = 1e-2, 0.1        # settable after construction
        loss = m(idx[:, :-1], idx[:, 1:])
        assert loss.dim() == 0 and loss.requires_grad
        assert m.last_ce.dim() == 0 and not m.last_ce.requires_grad
        assert torch.allclose(m.last_ce, plain.detach(), rtol=1e-6, atol=0)
        assert set(m.state_dict()) == keys
        m2 = make(z_loss=1e-2, label_smoothing=0.1)
        m2.load_state_dict(m.state_dict())
        assert torch.equal(m2(idx[:, :-1], idx[:, 1:]), loss)
        m.z_loss, m.label_smoothing = 0.0, 0.0         # switched off again: no stale last_ce
        assert torch.equal(m(idx[:, :-1], idx[:, 1:]), plain) and m.last_ce is None


def _rows(path):
    return [json.loads(line) for line in open(os.path.join(path, "result.json"))]


def _series(path, key):
    out = {}
    for row in _rows(path):
        for i, v in enumerate(reversed(row[key])):
            k = row["step"] - i
            assert out.setdefault(k, v) == v, f"step {k} logged twice with different {key}"
    return out


def run_aux_resume_case(tmp_path, model: str, use_gpu: bool, **extra):
    """4 optimizer steps with both terms and a checkpoint every 2; a run killed at step 3 and
    restarted from the step-2 checkpoint logs the same losses and plain cross-entropies, bit for bit"""
    from ray_torch_distributed_checkpoint_amd import workloads as W

    kw = dict(steps=4, num_workers=1, use_gpu=use_gpu, ckpt_every_n_steps=2, verbose=0, z_loss=1e-4,
              label_smoothing=0.1, **extra)
    a = W.train_workload(model, checkpoint_storage_path=str(tmp_path / "a"), **kw)
    rows = _rows(a.path)
    assert [r["step"] for r in rows] == [2, 4]
    for r in rows:
        assert len(r["ce_losses"]) == len(r["losses"]) == 2 and r["ce_loss"] == r["ce_losses"][-1]
        assert r["loss"] == r["losses"][-1] and all(v == v and v > 0 for v in r["ce_losses"])
    os.environ["RTDC_FAIL_AT_STEP"] = "3:0"
    try:
        b = W.train_workload(model, checkpoint_storage_path=str(tmp_path / "b"), max_failures=1, **kw)
    finally:
        os.environ.pop("RTDC_FAIL_AT_STEP", None)
    for key in ("losses", "ce_losses"):
        sa, sb = _series(a.path, key), _series(b.path, key)
        assert sorted(sa) == [1, 2, 3, 4] and sa == sb, key
    assert b.metrics["step"] == 4
    return a


@pytest.fixture
def _cpu(monkeypatch):
    monkeypatch.setenv("RTDC_FORCE_CPU", "1")
    for k in ("RTDC_FAIL_AT_STEP", "RTDC_HANG_AT_STEP", "RTDC_FAIL_AT_REPORT"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("model", ["gpt2-tiny", "resnet18-tiny"])
def test_workload_rows_and_kill_restart_with_both_terms_cpu(tmp_path, _cpu, model):
    run_aux_resume_case(tmp_path, model, use_gpu=False)


def test_workload_rows_z_loss_alone_and_accumulation_cpu(tmp_path, _cpu):
    from ray_torch_distributed_checkpoint_amd import workloads as W

    kw = dict(num_workers=1, use_gpu=False, ckpt_every_n_steps=2, verbose=0, z_loss=1e-3, lr=1e-30)
    # (a learning rate of ~0: the k = 2 run's step s then sees the plain run's steps 2s - 1 and 2s on one model)
    plain = W.train_workload("gpt2-tiny", steps=4, checkpoint_storage_path=str(tmp_path / "p"), **kw)
    accum = W.train_workload("gpt2-tiny", steps=2, checkpoint_storage_path=str(tmp_path / "q"), grad_accum_steps=2, **kw)
    for key in ("losses", "ce_losses"):
        sp, sq = _series(plain.path, key), _series(accum.path, key)
        assert sorted(sp) == [1, 2, 3, 4] and sorted(sq) == [1, 2]
        for s in (1, 2):
            mean = float((torch.tensor(sp[2 * s - 1], dtype=F32) + torch.tensor(sp[2 * s], dtype=F32)) / 2)
            assert abs(sq[s] - mean) <= 2e-6 * abs(mean), (key, s, sq[s], mean)
    # z > 0, e = 0: the objective is the plain cross-entropy plus z * mean(lse^2) > 0
    for path in (plain.path, accum.path):
        for r in _rows(path):
            assert all(c < l for c, l in zip(r["ce_losses"], r["losses"])), r


def test_workload_rows_without_the_terms_are_todays_cpu(tmp_path, _cpu):
    from ray_torch_distributed_checkpoint_amd import workloads as W

    kw = dict(steps=2, num_workers=1, use_gpu=False, ckpt_every_n_steps=2, verbose=0)
    ref = W.train_workload("gpt2-tiny", checkpoint_storage_path=str(tmp_path / "r"), **kw)
    off = W.train_workload("gpt2-tiny", checkpoint_storage_path=str(tmp_path / "o"), z_loss=0.0, label_smoothing=0.0,
                           **kw)
    on = W.train_workload("gpt2-tiny", checkpoint_storage_path=str(tmp_path / "n"), z_loss=1e-4, **kw)
    r0, o0, n0 = _rows(ref.path)[0], _rows(off.path)[0], _rows(on.path)[0]
    assert set(o0) == set(r0) and not any(k.startswith("ce_") for k in r0)
    assert {"step", "loss", "losses", "epoch", "samples_per_s", "tokens_per_s"} <= set(r0)
    assert o0["losses"] == r0["losses"]                       # and the same bits
    assert set(n0) == set(r0) | {"ce_loss", "ce_losses"}
    assert n0["ce_losses"][0] == r0["losses"][0]              # step 1: the same model, the plain loss itself


def test_config_and_clis_carry_the_two_terms():
    from ray_torch_distributed_checkpoint_amd import workloads as W

    c = W.WorkloadConfig()
    assert c.z_loss is None and c.label_smoothing is None
    c = W.WorkloadConfig.from_dict({"z_loss": 1e-4, "label_smoothing": 0.1, "unknown": 1})
    assert (c.z_loss, c.label_smoothing) == (1e-4, 0.1)
    for bad in ({"z_loss": -1.0}, {"label_smoothing": 1.0}):
        with pytest.raises(ValueError):
            W.train_workload("gpt2-tiny", steps=1, **bad)
    env = dict(os.environ, PYTHONPATH=ROOT, RTDC_FORCE_CPU="1", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-m", "ray_torch_distributed_checkpoint_amd.workloads", "--help"], env=env,
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "--z-loss" in r.stdout and "--label-smoothing" in r.stdout, r.stderr[-2000:]
    r = subprocess.run([sys.executable, "-m", "ray_torch_distributed_checkpoint_amd.workloads", "--z-loss", "x"],
                       env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 2 and "--z-loss" in r.stderr    # a float is parsed
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_flow.py"), "run", "--help"], env=env,
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "--z_loss" in r.stdout and "--label_smoothing" in r.stdout, r.stderr[-2000:]
