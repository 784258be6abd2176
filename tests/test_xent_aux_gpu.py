"""Label smoothing and z-loss in the fused cross-entropy kernels, on the GPU.

The yardstick is tests/ulp.py with the reference and floors of tests/xent_aux_ref.py: per element
against fp64, the allowance measured from the fp32 twin on the same case.  The shapes are ulp's
(`XENT_ARMS`: one (V, ld) per dispatch arm and boundary of the launcher ladder, M = 5; `XENT_WRAPPER`
at M = 63), which are the arm boundaries and the partly padded last chunk; the AUX ladder of
xent.hip is the plain one, so the same table reaches every AUX instantiation:

  xent_reg_kernel<NT, NCH, ARG, true>   the nine XR rows of XENT_ARMS, with / without argmax
  xent_kernel<T, VEC, true>             (131073, 131080) bf16, (333, 333) bf16, (10, 16) / (4100, 4104) / (10, 10) fp32
  xent_bwd_kernel<T, VEC, true>         cross_entropy at V = 333, 50257 (scalar form), 1000 (16-B form), bf16 and fp32
  xent_finalize_ce_kernel               every cross_entropy(return_ce=True) and the LM head

Each judged output prints one line; the WORST lines of one run are kept in profiles/xent_aux_ulp.md.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

from tests import ulp as U
from tests import xent_aux_ref as A

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32, BF16 = U.F64, U.F32, U.BF16
NAN = float("nan")
ARM_IDS = [f"{str(a[0])[6:]}-{a[1]}-{a[2]}" for a in U.XENT_ARMS]


def _ext():
    from ray_torch_distributed_checkpoint_amd.ops._ext import gpu_ext

    return gpu_ext()


def _close(out, ref, rel):
    err = (out.float() - ref.float()).abs().max().item()
    mag = ref.float().abs().max().item() + 1e-6
    assert err <= rel * mag, f"max err {err} vs {rel}*{mag}"


def _bits(x):
    """the tensor's bit patterns (torch.equal on floats takes -0 for +0 and no NaN for itself)"""
    return x.view(torch.int16) if x.dtype == BF16 else x.view(torch.int32) if x.dtype == F32 else x


def _pos_zero(x):
    """every element is +0.0 (`== 0` would take -0.0 too)"""
    return bool((_bits(x) == 0).all())


def _guarded(M, *tail, dtype=F32, fill=NAN):
    """(buffer with one guard row on each side, its M inner rows)"""
    buf = torch.full((M + 2, *tail), fill, dtype=dtype, device=DEV)
    return buf, buf[1:M + 1]


def _direct(c, in_place, grad_scale, with_arg, kw=None, positional=False):
    """one xent launch; out-of-place outputs are NaN-filled with a guard row on each side"""
    lg = c["logits"].clone()
    M, ld = lg.shape
    gbuf, dl = (None, lg) if in_place else _guarded(M, ld, dtype=lg.dtype)
    lbuf, loss = _guarded(M)
    sbuf, lse = _guarded(M) if with_arg else (None, None)
    abuf, am = _guarded(M, dtype=torch.int64, fill=-1) if with_arg else (None, None)
    cbuf, ce = (None, None) if positional else _guarded(M)
    if positional:
        _ext().xent(lg, dl, c["target"], loss, lse, am, M, c["V"], ld, grad_scale, U.IGNORE_INDEX)
    else:
        _ext().xent(lg, dl, c["target"], loss, lse, am, M, c["V"], ld, grad_scale, U.IGNORE_INDEX, ce=ce, **kw)
    for buf in (gbuf, lbuf, sbuf, cbuf):   # the guard rows stay NaN
        assert buf is None or (torch.isnan(buf[0]).all() and torch.isnan(buf[-1]).all())
    assert abuf is None or (abuf[0] == -1 and abuf[-1] == -1)
    out = {"grad": dl, "loss": loss}
    if ce is not None:
        out["ce"] = ce
    if with_arg:
        out.update(lse=lse, argmax=am)
    return out


# ------------------------------------------------------------------------------- the row kernels
@pytest.mark.parametrize("dtype,V,ld,arm", U.XENT_ARMS, ids=ARM_IDS)
def test_dispatch_arms(dtype, V, ld, arm):
    """every arm, random and planted rows, each out of place / in place, grad_scale 1 and 1/7,
    with and without argmax / lse, for (e, z) = (0.1, 0), (0, 1e-4), (0.1, 1e-4)"""
    J = U.Judge()
    for planted in (False, True):
        c = U.xent_inputs(dtype, V, ld, planted, dev=DEV)
        ignored = c["target"] == U.IGNORE_INDEX
        assert int(ignored.sum()) == 1
        first = U.first_argmax(c["logits"], V)
        for e, z in A.XENT_AUX_GPU:
            refs = {gs: A.xent_aux_refs(c, gs, e, z) for gs in {w[1] for w in U.XENT_WAYS}}
            for in_place, gs, with_arg in U.XENT_WAYS:
                o = _direct(c, in_place, gs, with_arg, {"label_smoothing": e, "z_loss": z})
                shape = (arm, V, ld, "planted" if planted else "randn", "inplace" if in_place else "", round(gs, 3),
                         "arg" if with_arg else "", e, z)
                A.judge_xent_aux(J, "xent-aux", shape, c, gs, e, z, o, threads=U.xent_threads(arm),
                                 k=1 if dtype == BF16 else 0, refs=refs[gs])
                g = o["grad"]
                assert torch.isfinite(g).all(), shape
                assert _pos_zero(g[:, V:].contiguous()), shape            # padding columns: exactly +0.0
                assert _pos_zero(g[ignored]) and _pos_zero(o["loss"][ignored]) and _pos_zero(o["ce"][ignored]), shape
                if with_arg:
                    assert torch.equal(o["argmax"], first), (shape, o["argmax"].tolist(), first.tolist())
    J.check()


@pytest.mark.parametrize("dtype,V,ld,arm", U.XENT_ARMS, ids=ARM_IDS)
def test_zero_coefficients_are_the_plain_call_bit_for_bit(dtype, V, ld, arm):
    """e = z = 0 passed as keywords runs the plain instantiations: every output bitwise equal to
    the positional call without them, and ce is the loss"""
    for planted in (False, True):
        c = U.xent_inputs(dtype, V, ld, planted, dev=DEV)
        for in_place, gs, with_arg in U.XENT_WAYS:
            a = _direct(c, in_place, gs, with_arg, positional=True)
            b = _direct(c, in_place, gs, with_arg, {"label_smoothing": 0.0, "z_loss": 0.0})
            for k in a:
                assert torch.equal(_bits(a[k]), _bits(b[k])), (k, arm, planted, in_place, gs)
            assert torch.equal(_bits(b["ce"]), _bits(b["loss"]))


@pytest.mark.parametrize("dtype,V,ld,arm", U.XENT_ARMS, ids=ARM_IDS)
def test_two_runs_are_bitwise_equal(dtype, V, ld, arm):
    """the row sum is a fixed-order reduction (no atomics): run to run the same bits"""
    kw = {"label_smoothing": 0.1, "z_loss": 1e-4}
    for planted in (False, True):
        c = U.xent_inputs(dtype, V, ld, planted, dev=DEV)
        for in_place, gs, with_arg in U.XENT_WAYS:   # with and without argmax: every AUX instantiation
            a, b = _direct(c, in_place, gs, with_arg, kw), _direct(c, in_place, gs, with_arg, kw)
            assert all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a), (arm, planted, in_place, with_arg)


# ------------------------------------------------------------------------------- the wrappers
@pytest.mark.parametrize("dtype,V", U.XENT_WRAPPER, ids=[f"{str(d)[6:]}-{v}" for d, v in U.XENT_WRAPPER])
def test_cross_entropy_wrapper(dtype, V):
    """cross_entropy(label_smoothing, z_loss, return_ce) at M = 63: the backward kernel forms
    upstream / divisor * dL/dx from the logits and the saved logsumexp and rounds it once (k = 1);
    the mean loss and the returned ce come from one finalize launch"""
    from ray_torch_distributed_checkpoint_amd.ops import cross_entropy

    e, z = 0.1, 1e-4
    J = U.Judge()
    c = U.xent_wrapper_inputs(dtype, V, dev=DEV)
    M = c["logits"].shape[0]
    n_counted = int((c["target"] != U.IGNORE_INDEX).sum())
    assert 0 < n_counted < M
    for n_valid, upstream in ((None, 1.0), (50, 1.0), (50, 3.0)):
        n = n_valid or n_counted
        lg = c["logits"].clone().requires_grad_(True)
        loss, ce = cross_entropy(lg, c["target"], n_valid, label_smoothing=e, z_loss=z, return_ce=True)
        assert ce.dim() == 0 and ce.dtype == F32 and ce.is_cuda and not ce.requires_grad
        (loss * upstream).backward()
        shape = (str(dtype)[6:], V, f"n_valid={n_valid}", f"upstream={upstream}", e, z)
        gs = (torch.tensor(upstream, dtype=F32) / n).item()   # the kernel's g[0] / den[0], an fp32 division
        r = A.judge_xent_aux(J, "cross_entropy()", shape, c, gs, e, z, {"grad": lg.grad}, k=1 if dtype == BF16 else 0)
        assert _pos_zero(lg.grad[c["target"] == U.IGNORE_INDEX])
        for what, out in (("loss", loss.detach()), ("ce", ce)):
            # the mean of the reference rows in fp64 and in fp32; scale: the mean of the rows' sums of
            # |terms| (loss_scale / ce_scale of the reference), R: the rows a finalize thread adds
            (m64, _), (m32, _) = U.mean_loss_ref(F64, r[what], n), U.mean_loss_ref(F32, r[what], n)
            J.rel("cross_entropy()", shape, "mean " + what, out, m64, m32, r[what + "_scale"].sum() / n, -(-M // 1024))
        # the loss alone is the same tensor's value
        assert torch.equal(cross_entropy(c["logits"], c["target"], n_valid, label_smoothing=e, z_loss=z), loss.detach())
    J.check()


def test_xent_bwd_unaligned_view_takes_the_scalar_form():
    """xent_bwd with the two terms on a contiguous view that starts 2 B off a 16-B boundary,
    V % 8 == 0: the same numbers as the aligned call, bit for bit"""
    J = U.Judge()
    M, V, e, z = 5, 1000, 0.1, 1e-4
    c = U.xent_inputs(BF16, V, V, planted=False, dev=DEV)
    refs = A.xent_aux_refs(c, 1.0 / 7, e, z)
    lse = refs[0]["lse"].float()
    g, den = torch.ones(1, device=DEV), torch.full((1,), 7.0, device=DEV)
    buf = torch.zeros(M * V + 8, dtype=BF16, device=DEV)
    view = buf[1:1 + M * V].view(M, V)
    view.copy_(c["logits"])
    assert view.is_contiguous() and view.data_ptr() % 16 == 2 and c["logits"].data_ptr() % 16 == 0
    outs = []
    for lg in (view, c["logits"]):
        dl = torch.full((M, V), NAN, dtype=BF16, device=DEV)
        _ext().xent_bwd(lg, dl, c["target"], lse, g, den, U.IGNORE_INDEX, label_smoothing=e, z_loss=z)
        outs.append(dl)
        A.judge_xent_aux(J, "xent_bwd-aux", (M, V, f"base % 16 = {lg.data_ptr() % 16}"), c, 1.0 / 7, e, z, {"grad": dl},
                         refs=refs)
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    assert buf[0] == 0 and (buf[1 + M * V:] == 0).all()
    J.check()


def _lm_head_case():
    from ray_torch_distributed_checkpoint_amd.ops import lm_head_cross_entropy

    e, z = 0.1, 1e-4
    torch.manual_seed(8)
    M, C, V, Vp = 128, 64, 50257, 50304
    x = (torch.randn(M, C, device=DEV)).to(BF16).requires_grad_(True)
    w = (torch.randn(Vp, C, device=DEV) * 0.1).requires_grad_(True)
    tgt = torch.randint(0, V, (M,), device=DEV)
    tgt[3::17] = U.IGNORE_INDEX
    loss, ce = lm_head_cross_entropy(x, w, tgt, V, label_smoothing=e, z_loss=z, return_ce=True)
    loss.backward()
    xr = x.detach().float().requires_grad_(True)
    wr = w.detach().bfloat16().float().requires_grad_(True)
    lg = F.linear(xr, wr)[:, :V]
    keep = tgt != U.IGNORE_INDEX
    ref = F.cross_entropy(lg, tgt, ignore_index=U.IGNORE_INDEX, label_smoothing=e) + \
        z * (torch.logsumexp(lg, 1) ** 2)[keep].sum() / keep.sum()
    ref.backward()
    plain = F.cross_entropy(lg.detach(), tgt, ignore_index=U.IGNORE_INDEX)
    print(f"lm head (0.1, 1e-4): loss {loss.item():.6f} ref {ref.item():.6f}  ce {ce.item():.6f} ref {plain.item():.6f}")
    assert abs(loss.item() - ref.item()) < 2e-2
    assert abs(ce.item() - plain.item()) < 2e-2 and not ce.requires_grad
    _close(x.grad, xr.grad, 3e-2)
    _close(w.grad, wr.grad, 3e-2)
    assert w.grad[V:].abs().max().item() == 0.0


def test_lm_head_cross_entropy_gpt2_vocab():
    """GPT-2's arm, in place (XR(256,25)): vocab 50257 padded to 50304, both terms.  The GEMM in front
    sets the error: the figures of the plain test of tests/test_row_kernels_gpu.py"""
    _lm_head_case()


def test_lm_head_cross_entropy_gpt2_vocab_two_pass(monkeypatch):
    """the same through xent_kernel<bf16, true, true> (RTDC_XENT_TWO_PASS in the environment)"""
    monkeypatch.setenv("RTDC_XENT_TWO_PASS", "1")
    _lm_head_case()


def test_lm_head_row_chunks_carry_the_terms(monkeypatch):
    """the RTDC_LMHEAD_CHUNK_MB path (two chunks of 256 rows, out of place): the same loss, ce and
    gradients as the unchunked in-place path, up to the other GEMM's rounding"""
    from ray_torch_distributed_checkpoint_amd.ops import lm_head_cross_entropy
    from ray_torch_distributed_checkpoint_amd.ops import xent as X

    e, z = 0.1, 1e-4
    M, C, V, Vp = 512, 64, 50257, 50304
    torch.manual_seed(9)
    x0 = torch.randn(M, C, device=DEV).to(BF16)
    w0 = torch.randn(Vp, C, device=DEV) * 0.1
    tgt = torch.randint(0, V, (M,), device=DEV)
    tgt[3::17] = U.IGNORE_INDEX
    res = []
    for mb in (0.0, 26.0):
        monkeypatch.setattr(X, "_LM_CHUNK_MB", mb)
        assert X._lm_chunk_rows(M, Vp) == (M if mb == 0 else 256)
        x, w = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
        loss, ce = lm_head_cross_entropy(x, w, tgt, V, label_smoothing=e, z_loss=z, return_ce=True)
        loss.backward()
        res.append((loss.item(), ce.item(), x.grad, w.grad))
    (l0, c0, gx0, gw0), (l1, c1, gx1, gw1) = res
    print(f"lm head chunks: loss {l0:.6f} / {l1:.6f}  ce {c0:.6f} / {c1:.6f}")
    assert abs(l0 - l1) < 2e-3 and abs(c0 - c1) < 2e-3
    assert l0 != c0   # the terms are in the loss and not in ce
    _close(gx1, gx0, 3e-2)
    _close(gw1, gw0, 3e-2)
    assert gw1[V:].abs().max().item() == 0.0


# ------------------------------------------------------------------------------- models, workload
@pytest.mark.parametrize("name", ["gpt2-tiny", "llama3-tiny"])
def test_model_loss_matches_the_cpu_path(name):
    """B2 T128, (e, z) = (0.1, 1e-4): the GPU loss against the model's fp32 CPU path, within 1.5 x the
    same error of the plain loss measured here; model.last_ce is the plain run's loss to that error"""
    from ray_torch_distributed_checkpoint_amd.models import GPT2, GPT2Config, Llama, LlamaConfig

    torch.manual_seed(0)
    ref = Llama(LlamaConfig.named(name)) if name.startswith("llama") else GPT2(GPT2Config.named(name))
    gpu = copy.deepcopy(ref).cuda()
    torch.manual_seed(2)
    idx = torch.randint(0, ref.cfg.vocab_size, (2, 129))
    x, y = idx[:, :-1].contiguous(), idx[:, 1:].contiguous()
    with torch.no_grad():
        plain_gpu, plain_cpu = gpu(x.cuda(), y.cuda()), ref(x, y)
        assert gpu.last_ce is None
        for m in (ref, gpu):
            m.label_smoothing, m.z_loss = 0.1, 1e-4
        aux_gpu, aux_cpu = gpu(x.cuda(), y.cuda()), ref(x, y)
    plain = abs(plain_gpu.item() - plain_cpu.item())
    aux = abs(aux_gpu.item() - aux_cpu.item())
    ce = abs(gpu.last_ce.item() - plain_gpu.item())
    print(f"{name}: GPU-vs-CPU loss error plain {plain:.4e}, with both terms {aux:.4e}; "
          f"|last_ce - plain loss| {ce:.4e}; terms add {aux_cpu.item() - plain_cpu.item():.4e}")
    assert gpu.last_ce.dim() == 0 and gpu.last_ce.is_cuda and not gpu.last_ce.requires_grad
    assert abs(aux_cpu.item() - plain_cpu.item()) > 10 * plain   # the terms do move the loss beyond the parity error
    assert aux <= 1.5 * plain, (aux, plain)
    assert ce <= plain, (ce, plain)


def test_workload_with_both_terms_resumes_exactly_gpu(tmp_path, monkeypatch):
    from tests.test_xent_aux_cpu import run_aux_resume_case

    for k in ("RTDC_FAIL_AT_STEP", "RTDC_HANG_AT_STEP", "RTDC_FORCE_CPU", "RTDC_FAIL_AT_REPORT"):
        monkeypatch.delenv(k, raising=False)
    run_aux_resume_case(tmp_path, model="llama3-tiny", use_gpu=True, grad_accum_steps=2)
