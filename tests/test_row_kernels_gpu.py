"""Every dispatch variant of the memory-bound row kernels against fp64, to the ulp (GPU only).

The yardstick is tests/ulp.py: each op's reference runs in float64 (the reference) and in float32
(the "twin") on the kernel's own bf16 inputs; a kernel output may differ from the reference by
the rounding(s) to bf16 plus 16 x the twin's error, measured on the same case.  Each judged
output prints one line (op, shape, kernel error, twin error, allowance); the lines of one run are
kept in profiles/row_kernels_ulp.md.

Launcher branch -> the case that reaches it (check against the `if` ladders of the .hip files):

  xent.hip      XR(256,4)    ld <= 8192     (V, ld) = (8185, 8192), (8192, 8192)
                XR(256,8)    ld <= 16384    (8193, 8200), (16384, 16384)
                XR(256,16)   ld <= 32768    (20001, 20008)
                XR(256,25)   ld <= 51200    (50257, 50304); lm_head_cross_entropy at vocab 50257
                XR(512,16)   ld <= 65536    (51201, 51208), (65536, 65536)
                XR(1024,16)  ld <= 131072   (131072, 131072)
                xent_kernel<bf16,true>   ld > 131072, ld % 8 == 0      (131073, 131080)
                xent_kernel<bf16,false>  ld % 8 != 0    (333, 333); cross_entropy at bf16 V = 333, 50257
                xent_kernel<float,true>  fp32, ld % 8 == 0             (10, 16), (4100, 4104)
                xent_kernel<float,false> fp32, ld % 8 != 0             (10, 10); cross_entropy at fp32 V = 333
                each with ARG true / false (with / without argmax), in and out of place
                xent_bwd_kernel<T,false>: cross_entropy at M = 63, V = 333 (bf16, fp32), 50257 (bf16);
                xent_bwd_kernel<T,true> (V % 8 == 0): V = 1000 (bf16, fp32); xent_finalize: all of these;
                V % 8 == 0 on an unaligned base -> <T,false>: test_xent_bwd_unaligned_view_takes_the_scalar_form
  norm.hip fwd  CPL 1   D <= 512: 8, 200, 256, 512      CPL 2   D = 520, 768, 1024
                CPL 4   D = 2048    CPL 8   D = 4096    CPL 16  D = 8192    else (D = 8200): refused
  norm.hip bwd  8-B form cpl4 1  D = 256      cpl4 3  D = 768
                16-B form CPL 1  D = 8, 200, 512   CPL 2  D = 520, 1024   CPL 4  D = 2048   CPL 8  D = 4096
                else (D = 8192): refused;   CS true / false: with / without the dx column sums
                row loop (fetch(row + nw)): M = 67 at 16 waves, D = 256, 768, 1024, 2048;
                RTDC_NORM_BWD_VW4=0 (D = 256, 768 in the 16-B form: idle lanes, a partial chunk) and
                RTDC_COLSUM_WIDE=0 (colsum_ws_kernel): a fresh child process, both knobs are read once;
                grid capped at the resident slots: (M, D) = (9001, 768), (4101, 4096)
  attn_softmax  CPL 1  T = 8, 64     CPL 2  T = 520, 1024     CPL 4  T = 1032, 2048     CPL 8  T = 4096
                else (T = 4104): refused;  causal and not, with and without lse, in and out of place
  llama_ops     swiglu stride loop, second iteration: (M, F) = (2100, 16384); first: the other shapes
                rope: Dh 16 / 64 / 128 (1, 4, 8 chunks per head), rotated and copied heads, tok % T wraps
                (the second iteration of rope's stride loop needs 67 M elements and is not reached)
"""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from tests import ulp as U

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32, BF16 = U.F64, U.F32, U.BF16


def _ext():
    from ray_torch_distributed_checkpoint_amd.ops._ext import gpu_ext

    return gpu_ext()


def _close(out, ref, rel):
    err = (out.float() - ref.float()).abs().max().item()
    mag = ref.float().abs().max().item() + 1e-6
    assert err <= rel * mag, f"max err {err} vs {rel}*{mag}"


# ------------------------------------------------------------------------------- norms
def _norm_fwd(c, eps, rms):
    x = c["x"]
    M = x.shape[0]
    y = torch.empty_like(x)
    rstd = torch.empty(M, dtype=F32, device=DEV)
    if rms:
        _ext().rmsnorm_fwd(x, c["g"], y, rstd, eps)
        return {"y": y, "rstd": rstd}
    mean = torch.empty(M, dtype=F32, device=DEV)
    _ext().layernorm_fwd(x, c["g"], c["b"], y, mean, rstd, eps)
    return {"y": y, "mean": mean, "rstd": rstd}


def _norm_bwd(c, fwd, rms, want_sum):
    """the backward on the forward's own saved statistics; returns the outputs and the waves"""
    from ray_torch_distributed_checkpoint_amd.ops import norm as N

    x = c["x"]
    M, D = x.shape
    nw = N._bwd_waves(M)
    ws = torch.empty(N._bwd_ws_elems(nw, D), dtype=F32, device=DEV)
    dx = torch.full_like(x, float("nan"))
    dg, db = (torch.full((D,), float("nan"), dtype=F32, device=DEV) for _ in range(2))
    dxsum = torch.full((D,), float("nan"), dtype=F32, device=DEV) if want_sum else None
    if rms:
        _ext().rmsnorm_bwd(c["dy"], x, c["g"], fwd["rstd"], c["dres"], dx, ws, dg, nw)
        out = {"dx": dx, "dgamma": dg}
    else:
        _ext().layernorm_bwd(c["dy"], x, c["g"], fwd["mean"], fwd["rstd"], c["dres"], dx, ws, dg, db, dxsum, nw, False)
        out = {"dx": dx, "dgamma": dg, "dbeta": db}
    if want_sum and not rms:
        out["dxsum"] = dxsum
    return out, nw


@pytest.mark.parametrize("rms", [False, True], ids=["layernorm", "rmsnorm"])
def test_norm_widths_and_row_counts(rms):
    """every width instantiation x M = 1, 3, 5, 64 (and eps 1e-6 at M = 5); D = 8192 forward only"""
    op = "rmsnorm" if rms else "layernorm"
    J = U.Judge()
    for M, D, eps in U.norm_cases():
        if M >= 67:
            continue
        c = U.norm_inputs(M, D, dres=True, dev=DEV)
        outs = _norm_fwd(c, eps, rms)
        bwd = D <= 4096
        if bwd:
            outs.update(_norm_bwd(c, outs, rms, want_sum=not rms)[0])
        U.judge_norm(J, op, (M, D, eps), c, eps, rms, outs, bwd=bwd, rows_per_wave=1)
        if not rms and c["const_row"] is not None:  # variance 0: y is beta, bit for bit
            assert torch.equal(outs["y"][c["const_row"]], c["b"]), (M, D)
    J.check()


@pytest.mark.parametrize("rms", [False, True], ids=["layernorm", "rmsnorm"])
@pytest.mark.parametrize("M,D,waves", [(67, D, 16) for D in U.NORM_LOOP_WIDTHS] + [(M, D, None) for M, D in U.NORM_LOOP_BIG])
def test_norm_backward_row_loop(monkeypatch, rms, M, D, waves):
    """a backward wave owns several rows in sequence (the software-pipelined fetch(row + nw)):
    with and without dres, with and without the dx column sums"""
    from ray_torch_distributed_checkpoint_amd.ops import norm as N

    if waves is not None:
        monkeypatch.setattr(N, "_BWD_WAVES", waves)
    op = "rmsnorm" if rms else "layernorm"
    J = U.Judge()
    for dres in (False, True):
        c = U.norm_inputs(M, D, dres=dres, dev=DEV)
        fwd = _norm_fwd(c, 1e-5, rms)
        for want_sum in ((False,) if rms else (False, True)):
            bw, nw = _norm_bwd(c, fwd, rms, want_sum)
            assert nw == (waves or 4096)
            # a wave adds at least ceil(M / nw) rows serially (more where the grid is capped)
            U.judge_norm(J, op, (M, D, "dres" if dres else "", "colsum" if want_sum else ""), c, 1e-5, rms,
                         {**fwd, **bw}, rows_per_wave=-(-M // nw))
    J.check()


def _knobs_off_child():
    """what test_norm_backward_knobs_off runs in its child process"""
    from ray_torch_distributed_checkpoint_amd.ops import norm as N

    assert os.environ["RTDC_NORM_BWD_VW4"] == "0" and os.environ["RTDC_COLSUM_WIDE"] == "0" and N._BWD_WAVES == 16
    J = U.Judge()
    for rms in (False, True):
        for M, D in ((67, 256), (67, 768)):
            for dres in (False, True):
                c = U.norm_inputs(M, D, dres=dres, dev=DEV)
                fwd = _norm_fwd(c, 1e-5, rms)
                for want_sum in ((False,) if rms else (False, True)):
                    bw, nw = _norm_bwd(c, fwd, rms, want_sum)
                    assert nw == 16
                    U.judge_norm(J, "rmsnorm" if rms else "layernorm",
                                 (M, D, "dres" if dres else "", "colsum" if want_sum else "", "knobs off"), c, 1e-5, rms,
                                 {**fwd, **bw}, rows_per_wave=-(-M // nw))
    J.check()


def test_norm_backward_knobs_off():
    """RTDC_NORM_BWD_VW4=0 and RTDC_COLSUM_WIDE=0, which the library reads once per process, so in a
    fresh child: D = 256 and 768 go through the 16-B form (64 and 32 of a chunk row's lanes idle, the
    `c < nch` guard on a partial chunk) and every reduction through the two-launch colsum_ws_kernel;
    LayerNorm and RMSNorm at M = 67 on 16 waves, with and without dres and the dx column sums,
    judged as test_norm_backward_row_loop judges them"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RTDC_NORM_BWD_VW4="0", RTDC_COLSUM_WIDE="0", RTDC_NORM_BWD_WAVES="16", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", "from tests.test_row_kernels_gpu import _knobs_off_child as f; f()"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("ULP ") >= 12 * 2  # 12 backward calls, dx and dgamma at the least of each


class _Producer(torch.autograd.Function):
    """Stands for the projection that wrote x: its backward asks colsum() for the column sums of
    the gradient it receives, as the projection's bias gradient does.  (A leaf's .grad would not
    do: AccumulateGrad detaches the tensor, and the offer is keyed to the tensor autograd passes.)"""

    @staticmethod
    def forward(ctx, x, bias):
        return x.clone()

    @staticmethod
    def backward(ctx, dy):
        from ray_torch_distributed_checkpoint_amd.ops import gemm as G

        taken = G._take_colsum(dy.view(-1, dy.shape[-1]))
        return dy, taken


@pytest.mark.parametrize("M,D,waves", [(67, 768, 16), (67, 2048, 16), (5, 200, None)])
def test_norm_autograd_wrappers(monkeypatch, M, D, waves):
    """layer_norm / rms_norm plumbing: passthrough (the residual gradient enters as dres), the
    dx column sums offered to colsum() (grad_sum_into), and the plain form"""
    from ray_torch_distributed_checkpoint_amd.ops import layer_norm, rms_norm
    from ray_torch_distributed_checkpoint_amd.ops import norm as N

    if waves is not None:
        monkeypatch.setattr(N, "_BWD_WAVES", waves)
    rpw = -(-M // N._bwd_waves(M))
    J = U.Judge()
    for rms in (False, True):
        for passthrough in (True, False):
            c = U.norm_inputs(M, D, dres=passthrough, dev=DEV)
            x0 = c["x"].clone().requires_grad_(True)
            bias = torch.zeros(D, device=DEV, requires_grad=True)
            x = _Producer.apply(x0, bias)
            w = c["g"].float().requires_grad_(True)   # bf16-representable masters: the shadow is exact
            b = c["b"].float().requires_grad_(True)
            outs = {}
            if rms:
                res = rms_norm(x, w, 1e-5, passthrough=passthrough)
            else:
                res = layer_norm(x, w, b, 1e-5, passthrough=passthrough, grad_sum_into=bias if passthrough else None)
            if passthrough:
                y, xp = res
                assert torch.equal(xp, x)
                torch.autograd.backward([y, xp], [c["dy"], c["dres"]])
            else:
                y = res
                y.backward(c["dy"])
            outs.update(y=y.detach(), dx=x0.grad, dgamma=w.grad)
            if not rms:
                outs["dbeta"] = b.grad
            if passthrough and not rms:
                assert bias.grad is not None, "the backward did not offer the dx column sums"
                outs["dxsum"] = bias.grad
            else:
                assert bias.grad is None
            U.judge_norm(J, "rms_norm()" if rms else "layer_norm()", (M, D, "passthrough" if passthrough else "plain"),
                         c, 1e-5, rms, outs, rows_per_wave=rpw)
    J.check()


def test_norm_unsupported_widths_refuse_cleanly():
    """backward at D = 8192 and forward at D = 8200 raise, and the next supported call is right"""
    J = U.Judge()
    c = U.norm_inputs(5, 8192, dres=True, dev=DEV)
    for rms in (False, True):
        fwd = _norm_fwd(c, 1e-5, rms)
        with pytest.raises(RuntimeError, match="unsupported shape"):
            _norm_bwd(c, fwd, rms, want_sum=False)
    c2 = U.norm_inputs(5, 8200, dev=DEV)
    for rms in (False, True):
        with pytest.raises(RuntimeError, match="unsupported shape"):
            _norm_fwd(c2, 1e-5, rms)
    for rms in (False, True):
        c3 = U.norm_inputs(5, 520, dres=True, dev=DEV)
        outs = _norm_fwd(c3, 1e-5, rms)
        outs.update(_norm_bwd(c3, outs, rms, want_sum=not rms)[0])
        U.judge_norm(J, "rmsnorm" if rms else "layernorm", (5, 520, "after a refusal"), c3, 1e-5, rms, outs)
    J.check()


# ------------------------------------------------------------------------------- cross-entropy
def _xent_direct(c, in_place, grad_scale, with_arg):
    lg = c["logits"].clone()
    M, ld = lg.shape
    dl = lg if in_place else torch.full_like(lg, float("nan"))
    loss = torch.full((M,), float("nan"), dtype=F32, device=DEV)
    lse = torch.full((M,), float("nan"), dtype=F32, device=DEV) if with_arg else None
    am = torch.full((M,), -1, dtype=torch.int64, device=DEV) if with_arg else None
    _ext().xent(lg, dl, c["target"], loss, lse, am, M, c["V"], ld, grad_scale, U.IGNORE_INDEX)
    out = {"grad": dl, "loss": loss}
    if with_arg:
        out.update(lse=lse, argmax=am)
    return out


@pytest.mark.parametrize("dtype,V,ld,arm", U.XENT_ARMS, ids=[f"{str(a[0])[6:]}-{a[1]}-{a[2]}" for a in U.XENT_ARMS])
def test_xent_dispatch_arms(dtype, V, ld, arm):
    """one (V, ld) per dispatch arm and boundary, M = 5: random and planted rows, each out of
    place / in place, grad_scale 1 and 1/7, with and without the argmax / lse outputs"""
    J = U.Judge()
    for planted in (False, True):
        c = U.xent_inputs(dtype, V, ld, planted, dev=DEV)
        ignored = c["target"] == U.IGNORE_INDEX
        assert int(ignored.sum()) == 1
        first = U.first_argmax(c["logits"], V)
        for in_place, gs, with_arg in U.XENT_WAYS:
            o = _xent_direct(c, in_place, gs, with_arg)
            shape = (arm, V, ld, "planted" if planted else "randn", "inplace" if in_place else "", round(gs, 3),
                     "arg" if with_arg else "")
            U.judge_xent(J, "xent", shape, c, gs, o, threads=U.xent_threads(arm), k=1 if dtype == BF16 else 0)
            g = o["grad"]
            assert torch.isfinite(g).all(), shape
            assert (g[:, V:] == 0).all(), shape                       # padding columns: exactly 0
            assert (g[ignored] == 0).all() and (o["loss"][ignored] == 0).all(), shape
            if with_arg:
                assert torch.equal(o["argmax"], first), (shape, o["argmax"].tolist(), first.tolist())
    J.check()


@pytest.mark.parametrize("dtype,V", U.XENT_WRAPPER, ids=[f"{str(d)[6:]}-{v}" for d, v in U.XENT_WRAPPER])
def test_xent_wrappers(dtype, V):
    """cross_entropy / xent_metrics at M = 63: xent_finalize with ignored rows and with n_valid
    given, and the backward kernel, which forms upstream / divisor * (softmax - onehot) from the
    logits and the saved logsumexp and rounds it once (k = 1; a stored bf16 gradient scaled
    afterwards was rounded twice and reached 1.117 ulp at divisor 50, above the 1.016 of k = 2)."""
    from ray_torch_distributed_checkpoint_amd.ops import cross_entropy, xent_metrics

    J = U.Judge()
    c = U.xent_wrapper_inputs(dtype, V, dev=DEV)
    M = c["logits"].shape[0]
    n_counted = int((c["target"] != U.IGNORE_INDEX).sum())
    assert 0 < n_counted < M
    for n_valid, upstream in ((None, 1.0), (50, 1.0), (50, 3.0)):
        n = n_valid or n_counted
        lg = c["logits"].clone().requires_grad_(True)
        loss = cross_entropy(lg, c["target"], n_valid)
        (loss * upstream).backward()
        shape = (str(dtype)[6:], V, f"n_valid={n_valid}", f"upstream={upstream}")
        gs = (torch.tensor(upstream, dtype=F32) / n).item()   # the kernel's g[0] / den[0], an fp32 division
        r = U.judge_xent(J, "cross_entropy()", shape, c, gs, {"grad": lg.grad}, k=1 if dtype == BF16 else 0)
        assert (lg.grad[c["target"] == U.IGNORE_INDEX] == 0).all()
        (m64, sc), (m32, _) = U.mean_loss_ref(F64, r["loss"], n), U.mean_loss_ref(F32, r["loss"], n)
        J.rel("cross_entropy()", shape, "mean", loss.detach(), m64, m32, sc, -(-M // 1024))
    tgt = torch.where(c["target"] == U.IGNORE_INDEX, torch.zeros_like(c["target"]), c["target"])
    ls, nc = xent_metrics(c["logits"], tgt)
    r = U.xent_ref(F64, c["logits"], tgt, V)
    t = U.xent_ref(F32, c["logits"], tgt, V)
    J.rel("xent_metrics()", (str(dtype)[6:], V), "sum", ls, r["loss"].sum(), t["loss"].sum(), r["loss"].abs().sum(), 1)
    assert nc.item() == int((U.first_argmax(c["logits"], V) == tgt).sum())
    J.check()


def test_xent_bwd_unaligned_view_takes_the_scalar_form():
    """xent_bwd on a contiguous view that starts 2 B off a 16-B boundary, V % 8 == 0: the launcher
    must not take the 16-B-per-lane form there; same numbers as the aligned call, bit for bit"""
    J = U.Judge()
    M, V = 5, 1000
    c = U.xent_inputs(BF16, V, V, planted=False, dev=DEV)
    r = U.xent_ref(F64, c["logits"], c["target"], V, 1.0 / 7)
    lse = r["lse"].float()
    g, den = torch.ones(1, device=DEV), torch.full((1,), 7.0, device=DEV)
    buf = torch.zeros(M * V + 8, dtype=BF16, device=DEV)
    view = buf[1:1 + M * V].view(M, V)
    view.copy_(c["logits"])
    assert view.is_contiguous() and view.data_ptr() % 16 == 2 and c["logits"].data_ptr() % 16 == 0
    outs = []
    for lg in (view, c["logits"]):
        dl = torch.full((M, V), float("nan"), dtype=BF16, device=DEV)
        _ext().xent_bwd(lg, dl, c["target"], lse, g, den, U.IGNORE_INDEX)
        outs.append(dl)
        U.judge_xent(J, "xent_bwd", (M, V, f"base % 16 = {lg.data_ptr() % 16}"), c, 1.0 / 7, {"grad": dl})
    assert torch.equal(outs[0], outs[1]) and buf[0] == 0 and (buf[1 + M * V:] == 0).all()
    J.check()


def test_lm_head_cross_entropy_gpt2_vocab():
    """GPT-2's arm, in place: vocab 50257 padded to 50304.  The GEMM in front sets the error, so
    this one keeps the figures of test_lm_head_cross_entropy_padded_vocab."""
    from ray_torch_distributed_checkpoint_amd.ops import lm_head_cross_entropy

    torch.manual_seed(8)
    M, C, V, Vp = 128, 64, 50257, 50304
    x = (torch.randn(M, C, device=DEV)).to(BF16).requires_grad_(True)
    w = (torch.randn(Vp, C, device=DEV) * 0.1).requires_grad_(True)
    tgt = torch.randint(0, V, (M,), device=DEV)
    tgt[3::17] = U.IGNORE_INDEX
    loss = lm_head_cross_entropy(x, w, tgt, V)
    loss.backward()
    xr = x.detach().float().requires_grad_(True)
    wr = w.detach().bfloat16().float().requires_grad_(True)
    ref = F.cross_entropy(F.linear(xr, wr)[:, :V], tgt, ignore_index=U.IGNORE_INDEX)
    ref.backward()
    assert abs(loss.item() - ref.item()) < 2e-2
    _close(x.grad, xr.grad, 3e-2)
    _close(w.grad, wr.grad, 3e-2)
    assert w.grad[V:].abs().max().item() == 0.0


# ------------------------------------------------------------------------------- causal softmax
@pytest.mark.parametrize("rows,T,causal", U.SOFTMAX_CASES)
def test_softmax_forward_backward(rows, T, causal):
    """direct softmax_fwd / softmax_bwd: out of place with lse, then in place without (as the
    attention path calls it).  Causal inputs are NaN above the diagonal: never read, written 0."""
    J = U.Judge()
    c = U.softmax_inputs(rows, T, causal, dev=DEV)
    shape = (rows, T, "causal" if causal else "full")
    keep = U._causal_mask(rows, T, DEV) if causal else torch.ones(rows, T, dtype=torch.bool, device=DEV)
    P = torch.full_like(c["S"], float("nan"))
    lse = torch.full((rows,), float("nan"), dtype=F32, device=DEV)
    _ext().softmax_fwd(c["S"], P, lse, rows, T, causal)
    U.judge_softmax_fwd(J, shape, c, T, causal, {"P": P, "lse": lse})
    P2 = c["S"].clone()
    _ext().softmax_fwd(P2, P2, None, rows, T, causal)
    U.judge_softmax_fwd(J, shape + ("inplace",), c, T, causal, {"P": P2})
    for p in (P, P2):
        assert torch.isfinite(p).all() and (p[~keep] == 0).all(), shape
    dS = torch.full_like(P, float("nan"))
    _ext().softmax_bwd(P, c["dP"], dS, rows, T, causal)
    U.judge_softmax_bwd(J, shape, P, c["dP"], T, causal, dS)
    dS2 = c["dP"].clone()
    _ext().softmax_bwd(P, dS2, dS2, rows, T, causal)
    U.judge_softmax_bwd(J, shape + ("inplace",), P, c["dP"], T, causal, dS2)
    for d in (dS, dS2):
        assert torch.isfinite(d).all() and (d[~keep] == 0).all(), shape
    J.check()


def test_softmax_unsupported_width_refuses_cleanly():
    T = 4104
    S = torch.randn(4, T, device=DEV).to(BF16)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        _ext().softmax_fwd(S, torch.empty_like(S), None, 4, T, False)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        _ext().softmax_bwd(S, S, torch.empty_like(S), 4, T, False)
    J = U.Judge()
    c = U.softmax_inputs(7, 64, False, dev=DEV)
    P = torch.empty_like(c["S"])
    _ext().softmax_fwd(c["S"], P, None, 7, 64, False)
    U.judge_softmax_fwd(J, (7, 64, "after a refusal"), c, 64, False, {"P": P})
    J.check()


# ------------------------------------------------------------------------------- SwiGLU
@pytest.mark.parametrize("M,Fd", U.SWIGLU_CASES)
def test_swiglu_forward_backward(M, Fd):
    """direct swiglu_fwd / swiglu_bwd; gates 0, +-30, +-100 next to random ones; (2100, 16384)
    is more work than the 16384 x 256 grid, so the stride loop runs twice"""
    if (M, Fd) == U.SWIGLU_CASES[-1]:
        assert M * Fd // 8 > 16384 * 256
    J = U.Judge()
    c = U.swiglu_inputs(M, Fd, dev=DEV)
    h = torch.full((M, Fd), float("nan"), dtype=BF16, device=DEV)
    dgu = torch.full_like(c["gu"], float("nan"))
    _ext().swiglu_fwd(c["gu"], h)
    _ext().swiglu_bwd(c["gu"], c["dh"], dgu)
    assert torch.isfinite(h).all() and torch.isfinite(dgu).all()
    U.judge_swiglu(J, (M, Fd), c, {"h": h, "dgu": dgu})
    J.check()


# ------------------------------------------------------------------------------- RoPE
@pytest.mark.parametrize("Dh,H,Hkv", U.ROPE_CASES)
def test_rope_forward_inverse_and_autograd(Dh, H, Hkv):
    """direct rope, forward and inverse, against fp64 cos / sin computed in the reference (so
    rope_tables' fp32 tables are judged too); B = 2, T = 37: tok % T wraps; the V heads are
    bit-identical copies; apply_rope's backward against fp64 autograd"""
    from ray_torch_distributed_checkpoint_amd.ops.llama_ops import apply_rope, rope_tables

    J = U.Judge()
    c = U.rope_inputs(Dh, H, Hkv, dev=DEV)
    x = c["x"]
    B, T = x.shape[:2]
    cos, sin = rope_tables(T, Dh, U.ROPE_THETA, x.device)
    for inverse in (False, True):
        y = torch.full_like(x, float("nan"))
        _ext().rope(x, y, cos, sin, T, H + Hkv, H + 2 * Hkv, Dh, inverse)
        U.judge_rope(J, (Dh, H, Hkv, "inv" if inverse else "fwd"), x, H, Hkv, Dh, inverse, y)
        heads = lambda t: t.view(B, T, H + 2 * Hkv, Dh)  # noqa: E731
        assert torch.equal(heads(y)[:, :, H + Hkv:], heads(x)[:, :, H + Hkv:])
    xg = x.clone().requires_grad_(True)
    apply_rope(xg, H, Hkv, U.ROPE_THETA).backward(c["dy"])
    grads = []
    for dt in (F64, F32):
        xr = x.to(dt).requires_grad_(True)
        out = U.rope_ref(dt, xr, T, H, Hkv, Dh)
        out.backward(c["dy"].to(dt).view(out.shape))
        grads.append(xr.grad.view(out.shape))
    J.ulp("apply_rope()", (Dh, H, Hkv), "dx", xg.grad.view(grads[0].shape), grads[0], grads[1],
          U.row_floor(grads[0], U.FLOOR_ROPE))
    J.check()
