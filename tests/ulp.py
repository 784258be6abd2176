"""Per-element yardstick for the memory-bound row kernels (norm / xent / attn_softmax / llama_ops).

Pure torch, importable without a GPU.  Three parts:

* the metric: `ulp_err` (bf16 outputs, in units of the last place of the fp64 reference) and
  `rel_err` (fp32 outputs, relative to the fp64 sum of |terms| of a reduction, or to |ref|);
* one reference function per op, a function of `dtype`: run in float64 it is the reference, run
  in float32 (never rounded to bf16) it is the "twin".  Both see exactly what the kernel sees:
  bf16 activations and bf16-rounded parameters;
* the allowance, measured at run time from the twin on the same inputs (`allow_bf16`,
  `allow_f32`); no constant here is tuned against a kernel.

`floor` (the FLOOR_* constants, times the row maximum of |ref|; two of them times another scale,
said where they stand) keeps elements that are the
difference of two nearly equal quantities from being judged in units of their own, arbitrarily
small, last place: below the floor an element is judged in ulps of the floor.  Each constant is
the smallest power of two for which the fp32 twin stays <= 2^-4 ulp on every case generator in
this file (tests/test_ulp_cpu.py holds that condition); what cancels is said next to it.

The case generators at the bottom are shared by tests/test_ulp_cpu.py (twin condition, mutant
sensitivity) and tests/test_row_kernels_gpu.py (the kernels).

The last section does the same for the attention kernels (attn_flash.hip and the composed path),
with one difference said there: those kernels round to bf16 inside the computation, so their
allowance is a per-element tensor derived from those roundings (`attn_ref`, `Judge.within`), not
a multiple of an unrounded twin's error.  tests/test_attn_ulp_gpu.py runs the kernels against it.

The GEMM section (at the end) puts the bf16 MFMA GEMMs and their fused epilogues (gemm_bf16.hip,
gemm_8ph.h/.hip, gemm4b.hip, gemm8b.hip, gemm_f32.hip) under the first yardstick again - they
accumulate in fp32 and round every output to bf16 once, split-K included (its slabs are fp32):
* `gemm_ref` in float64 is the reference, in float32 (nothing rounded to bf16) the twin; the
  epilogue is written in the kernels' order - bias, then beta * Cin, then the activation - with the
  GELU of common.h (`gelu_sigmoid_arg`); it returns every output of the call (C, the saved
  pre-activation or gelu', the column sums) and S, the sum of |terms| at the leaves;
* bf16 outputs: `Judge.ulp`, k = 1, floor = FLOOR_GEMM x S (an element is a sum of K signed
  products: |ref| / S has a median of a few percent and no lower bound); fp32 outputs:
  `Judge.rel`, scale = S, R = K;
* column sums: the fused arm (8-wave / one-barrier kernels, act 3 / 6, bf16 C) adds the fp32 values
  before they are packed and is judged against the fp64 column sum of the unrounded product with
  R = the rows a lane adds serially (GEMM_CS_ROWS, counted from tile_epilogue_bf16); every other
  arm reduces the stored C and is judged against the fp64 column sum of the kernel's own C;
* the case table (GEMM_*) is data shared by tests/test_ulp_cpu.py (twin condition, mutants) and
  tests/test_gemm_ulp_gpu.py (the kernels).

The CNN section (the last) does the same for the ResNet path - cnn.hip, the implicit-GEMM
convolution modes, conv3x3_wgrad_kernel and the statistics epilogues of gemm_bf16.hip: `conv_ref`,
`bn_ref` and the pool references, the index formulas of the kernels that only move data, the
generators (randn, offset, planted) and the CNN_* tables; tests/test_cnn_ulp_gpu.py runs the kernels.

The optimizer section (the last) does it for optim.hip and the arithmetic of elementwise.hip: `adamw_ref`
and `sgd_ref` (one step in the kernels' order, every scalar rounded to fp32 as a launcher receives it),
`optim_inputs` and the chunk tables, `embed_ref` / `embed_bwd_ref`, and the dropout mask from the Philox
twin of ops/random.py; tests/test_optim_ulp_gpu.py and tests/test_elementwise_ulp_gpu.py run the kernels.

The reductions section (the last) covers the stand-alone reduction kernels - the column sums of norm.hip, the
gradient-norm kernels of optim.hip, the loss finalisation of xent.hip: references that mirror each kernel's
partition, an integer generator on which every summation order is exact (the kernel must match bit for bit) and
an offset one judged by `Judge.rel` / `Judge.rel64`; tests/test_reduce_ulp_gpu.py runs the kernels.
"""
from __future__ import annotations

import math

import torch

IGNORE_INDEX = -100
BF16 = torch.bfloat16
TWIN_ULP_CEIL = 2.0 ** -4    # condition on the inputs: the fp32 twin is this close to fp64
TWIN_REL_CEIL = 2.0 ** -18
TINY = 2.0 ** -126


# ------------------------------------------------------------------------------- the metric
def ulp_bf16(v: torch.Tensor) -> torch.Tensor:
    """2^(floor(log2 v) - 7) for v > 0 (float64): the spacing of bf16 numbers in v's binade."""
    _, e = torch.frexp(v.double())  # v = m * 2^e, m in [0.5, 1)  ->  floor(log2 v) = e - 1
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - 8)


def ulp_err(out: torch.Tensor, ref64: torch.Tensor, floor) -> float:
    """max over all elements of |out - ref| / ulp_bf16(max(|ref|, floor)); floor broadcasts."""
    ref = ref64.double()
    fl = torch.as_tensor(floor, dtype=torch.float64, device=ref.device).clamp_min(TINY)
    den = ulp_bf16(torch.maximum(ref.abs(), fl))
    e = (out.double() - ref).abs() / den
    return float("nan") if bool(torch.isnan(e).any()) else e.max().item()


def rel_err(out: torch.Tensor, ref64: torch.Tensor, scale) -> float:
    """max |out - ref| / scale for fp32 outputs (an exact match scores 0 whatever the scale)."""
    ref = ref64.double()
    d = (out.double() - ref).abs()
    sc = torch.as_tensor(scale, dtype=torch.float64, device=ref.device).abs().expand_as(d)
    e = torch.where(d == 0, torch.zeros_like(d), d / sc)
    return float("nan") if bool(torch.isnan(e).any()) else e.max().item()


def row_floor(ref64: torch.Tensor, k: float) -> torch.Tensor:
    """k times the maximum of |ref| over the last axis (one floor per row)."""
    return ref64.double().abs().amax(-1, keepdim=True) * k


def allow_bf16(t: float, k: int = 1) -> float:
    """ulps allowed to a kernel output rounded k times to bf16, t = the twin's ulp_err: 0.5 per
    round-to-nearest conversion; 16 x the twin for another summation order and the hardware
    v_exp / v_rsq / v_rcp (a few fp32 ulp each); t floored at 2^-10 (64 fp32 roundings)."""
    return 0.5 * k + 16.0 * max(t, 2.0 ** -10)


def allow_f32(t_rel: float, R: int) -> float:
    """relative error allowed to an fp32 output, R = terms the kernel adds serially before its
    tree combine."""
    return max(16.0 * t_rel, (R + 16) * 2.0 ** -24)


class Judge:
    """Prints one line per judged output (op, shape, kernel error, twin error, allowance) and
    collects what misses: a twin above its ceiling (the inputs are ill-conditioned), or a kernel
    output above the allowance measured from the twin.  `out=None` judges the twin alone."""

    def __init__(self):
        self.failed = []
        self.worst = {}

    def _note(self, op, shape, what, unit, kerr, terr, allow, ceil):
        k = "-" if kerr is None else f"{kerr:.4g}"
        ln = f"ULP {op:<12s} {str(shape):<40s} {what:<7s} kernel {k:<10s} twin {terr:<10.4g} allow {allow:<10.4g} {unit}"
        print(ln)
        if not terr <= ceil:
            self.failed.append(ln + "   <- twin above its ceiling")
        if kerr is not None:
            if not kerr <= allow:   # also catches NaN
                self.failed.append(ln + "   <- kernel above the allowance")
            w = self.worst.get((op, what, unit))
            if w is None or not kerr <= w[0]:
                self.worst[(op, what, unit)] = (kerr, terr, allow, shape)

    def ulp(self, op, shape, what, out, ref64, twin, floor, k=1):
        t = ulp_err(twin, ref64, floor)
        self._note(op, shape, what, "ulp", None if out is None else ulp_err(out, ref64, floor), t,
                   allow_bf16(t, k), TWIN_ULP_CEIL)

    def rel(self, op, shape, what, out, ref64, twin, scale, R):
        t = rel_err(twin, ref64, scale)
        self._note(op, shape, what, "rel", None if out is None else rel_err(out, ref64, scale), t,
                   allow_f32(t, R), TWIN_REL_CEIL)

    def within(self, op, shape, what, out, ref64, twin, allow):
        """a per-element allowance tensor (attn_ref): max |out - ref| / allowance <= 1, the twin too"""
        self._note(op, shape, what, "x allowance", None if out is None else allow_err(out, ref64, allow),
                   allow_err(twin, ref64, allow), 1.0, 1.0)

    def check(self):
        for (op, what, unit), (k, t, a, shape) in sorted(self.worst.items()):
            print(f"WORST {op:<12s} {what:<7s} kernel {k:.4g} twin {t:.4g} allow {a:.4g} {unit} at {shape}")
        assert not self.failed, "\n" + "\n".join(self.failed)


def _f32(v: float) -> float:
    return torch.tensor(v, dtype=torch.float32).item()


# ------------------------------------------------------------------------------- norms
# LayerNorm y: x - mean loses the row offset (+30 rows), and xhat*gamma lands near -beta.
FLOOR_LN_Y = 2.0 ** -10
# RMSNorm y is a product: nothing cancels, and 2^-40 of the row maximum is below every element.
FLOOR_RMS_Y = 2.0 ** -40
# dx: the backward subtracts two row means (mean(dxhat), xhat*mean(dxhat*xhat)) from dxhat.
FLOOR_NORM_DX = 2.0 ** -12


def norm_ref(dtype, x, g, b, eps, dy=None, dres=None, rms=False, mutant=""):
    """LayerNorm (RMSNorm with rms=True) forward and, with dy, backward.  `mutant` names a
    deliberate error, used only by the sensitivity checks of tests/test_ulp_cpu.py."""
    x, g = x.to(dtype), g.to(dtype)
    D = x.shape[-1]
    eps = _f32(1e-4 if mutant == "eps" else eps)  # the kernel takes eps as a float
    mean = torch.zeros_like(x[:, :1]) if rms else x.sum(-1, keepdim=True) / D   # a true division, as the kernel's
    xc = x - mean
    var = (xc * xc).sum(-1, keepdim=True) / ((D - 1) if mutant == "var" else D)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = xc * rstd
    y = xhat * g
    if not rms:
        y = y + b.to(dtype) * (0.75 if mutant == "beta" else 1.0)
    out = {"y": y, "mean": mean[:, 0], "rstd": rstd[:, 0], "mean_scale": x.abs().sum(-1) / D}
    if dy is None:
        return out
    dy = dy.to(dtype)
    dxhat = dy * g
    m1 = torch.zeros_like(mean) if (rms or mutant == "m1") else dxhat.sum(-1, keepdim=True) / D
    m2 = (dxhat * xhat).sum(-1, keepdim=True) / D
    dx = rstd * (dxhat - m1 - xhat * m2)
    if dres is not None:
        r = dres.to(dtype)
        if mutant == "dres":
            r = r.clone()
            r[-1] = 0
        dx = dx + r
    tg = dy * xhat
    if mutant == "dgamma":
        tg = tg[:-1]
    # dgamma / dbeta: the sum of |terms| as they stand.  colsum(dx): with the terms taken at the
    # leaves - a dx is itself dxhat - m1 - xhat m2 (+ dres), so the column sum of one or three rows
    # is not judged against a residue (within 1.05 x of sum |dx| from M = 5 on)
    dx_terms = rstd * (dxhat.abs() + m1.abs() + (xhat * m2).abs()) + (0 if dres is None else dres.to(dtype).abs())
    out.update(dx=dx, dgamma=tg.sum(0), dgamma_scale=(dy * xhat).abs().sum(0),
               dbeta=dy.sum(0), dbeta_scale=dy.abs().sum(0), dxsum=dx.sum(0), dxsum_scale=dx_terms.sum(0))
    return out


def norm_inputs(M, D, seed=0, dres=False, dev="cpu"):
    """randn*2 rows, plus: rows offset by +30 (the mean dominates), one constant row (variance 0,
    y == beta bit for bit), one row of magnitude 2^-20."""
    gen = torch.Generator().manual_seed(1000 * D + M + seed)
    x = torch.randn(M, D, generator=gen) * 2
    if M >= 3:
        x[2] = 1.5  # every partial sum k * 1.5 is exact in fp32, so mean == 1.5 exactly
    if M >= 5:
        # not at M = 3: with two rows in a column sum, sum |dy xhat| can be a thousandth of one
        # term's |dy| (|x| + |mean|) rstd, and the fp32 x - mean of the offset row shows in dgamma
        x[1::7] += 30
        x[3] = torch.randn(D, generator=gen) * 2.0 ** -20
    c = {"x": x.to(BF16), "g": (1 + 0.1 * torch.randn(D, generator=gen)).to(BF16),
         "b": (0.1 * torch.randn(D, generator=gen)).to(BF16), "dy": torch.randn(M, D, generator=gen).to(BF16),
         "dres": torch.randn(M, D, generator=gen).to(BF16) if dres else None,
         "const_row": 2 if M >= 3 else None}
    return {k: v.to(dev) if torch.is_tensor(v) else v for k, v in c.items()}


NORM_WIDTHS = (8, 200, 256, 512, 520, 768, 1024, 2048, 4096)
NORM_ROWS = (1, 3, 5, 64)
NORM_LOOP_WIDTHS = (256, 768, 1024, 2048)   # M = 67 at 16 waves: 4-5 rows per wave
NORM_LOOP_BIG = ((9001, 768), (4101, 4096))  # default wave count, grid capped at the slots


def norm_cases():
    """(M, D, eps) of every norm case; the row-loop cases are run with and without dres."""
    out = [(M, D, 1e-5) for D in NORM_WIDTHS for M in NORM_ROWS]
    out += [(5, D, 1e-6) for D in NORM_WIDTHS]
    out += [(M, 8192, 1e-5) for M in NORM_ROWS]  # forward only
    out += [(67, D, 1e-5) for D in NORM_LOOP_WIDTHS] + [(M, D, 1e-5) for M, D in NORM_LOOP_BIG]
    return out


# ------------------------------------------------------------------------------- cross-entropy
# off the target column nothing cancels: every probability above 2^-40 of the row maximum is
# judged in its own last place (below lie only the far columns of the shifted row, ~e^-80).
FLOOR_XENT = 2.0 ** -40
# the target column is grad_scale * (p - 1): on a saturated row (target +12 above the rest) p is
# within 2^-10 of 1 and the whole gradient row is that residue, so this floor is taken times
# |grad_scale| (the 1 that is subtracted), not times the row maximum.
FLOOR_XENT_TARGET = 2.0 ** -8


def first_argmax(logits, V):
    """smallest index holding the row maximum, from the stored values (ties are planted)."""
    x = logits[:, :V].double()
    idx = torch.arange(V, device=x.device).expand_as(x)
    return torch.where(x == x.amax(1, keepdim=True), idx, torch.full_like(idx, V)).amin(1)


def last_argmax(logits, V):  # the mutant
    x = logits[:, :V].double()
    idx = torch.arange(V, device=x.device).expand_as(x)
    return torch.where(x == x.amax(1, keepdim=True), idx, torch.full_like(idx, -1)).amax(1)


def xent_ref(dtype, logits, target, V, grad_scale=1.0, mutant=""):
    """per-row loss, logsumexp and gradient grad_scale * (softmax - onehot) of logits[:, :V]
    (lse = max + log(sum exp(x - max)), p = exp(x - lse), as nn.CrossEntropyLoss computes it)."""
    M, ld = logits.shape
    x = logits.to(dtype) if mutant == "padding" else logits[:, :V].to(dtype)
    m = x.amax(1, keepdim=True)
    s = torch.exp(x - m).sum(1, keepdim=True)
    lse = m + torch.log(s)
    p = torch.exp(x[:, :V] - lse)
    valid = target != IGNORE_INDEX
    if mutant == "ignored":
        valid = torch.ones_like(valid)
    t = torch.where(target != IGNORE_INDEX, target, torch.zeros_like(target))
    hot = torch.zeros_like(p)
    hot.scatter_(1, ((t + 1) % V if mutant == "onehot" else t)[:, None], 1.0)
    gs = torch.tensor(grad_scale, dtype=torch.float32, device=x.device).to(dtype)  # a float in the kernel
    grad = gs * (p - hot) * valid[:, None].to(dtype)
    xt = x.gather(1, t[:, None])
    tmask = torch.zeros_like(p, dtype=torch.bool)
    tmask.scatter_(1, t[:, None], True)
    return {"grad": grad, "loss": torch.where(valid, (lse - xt)[:, 0], torch.zeros_like(lse[:, 0])),
            "lse": lse[:, 0], "lse_scale": (m.abs() + torch.log(s).abs())[:, 0],
            "loss_scale": (lse.abs() + xt.abs())[:, 0], "tmask": tmask & valid[:, None]}


def xent_grad_floor(ref, grad_scale):
    g = ref["grad"].double()
    return torch.where(ref["tmask"], torch.full_like(g, abs(_f32(grad_scale)) * FLOOR_XENT_TARGET),
                       row_floor(g, FLOOR_XENT))


# (dtype, V, ld, arm): one per dispatch arm and boundary of rtdc_xent
XENT_ARMS = [
    (BF16, 8185, 8192, "XR(256,4)"), (BF16, 8192, 8192, "XR(256,4)"), (BF16, 8193, 8200, "XR(256,8)"),
    (BF16, 16384, 16384, "XR(256,8)"), (BF16, 20001, 20008, "XR(256,16)"), (BF16, 50257, 50304, "XR(256,25)"),
    (BF16, 51201, 51208, "XR(512,16)"), (BF16, 65536, 65536, "XR(512,16)"), (BF16, 131072, 131072, "XR(1024,16)"),
    (BF16, 131073, 131080, "xent_kernel<bf16,true>"), (BF16, 333, 333, "xent_kernel<bf16,false>"),
    (torch.float32, 10, 16, "xent_kernel<float,true>"), (torch.float32, 4100, 4104, "xent_kernel<float,true>"),
    (torch.float32, 10, 10, "xent_kernel<float,false>"),
]


def xent_threads(arm: str) -> int:
    return int(arm[3:].split(",")[0]) if arm.startswith("XR(") else 256


def xent_targets(V, ld):
    """0, V-1, a column of the last (partly padded) 16-B chunk, a mid column, ignored."""
    return [0, V - 1, max(0, (V - 1) // 8 * 8), V // 2, IGNORE_INDEX]


def xent_inputs(dtype, V, ld, planted, seed=0, dev="cpu"):
    """M = 5 rows [M, ld]; the padding [V, ld) holds large finite junk that must not be read as
    logits.  planted=False: randn*3.  planted=True, by row: two equal maxima in different threads'
    chunks (ignored row); two equal maxima in different waves, the later column in the earlier
    thread where the row is long enough; a row shifted by -3000 with its maximum in column V-1
    (one bf16 step, 16, above the rest: the target is another column, so p - 1 does not cancel);
    an all-equal row; the target, column V-1, +12 above the rest."""
    gen = torch.Generator().manual_seed(V * 7 + ld + seed)
    x = torch.randn(5, ld, generator=gen) * (1.0 if planted else 3.0)
    tg = xent_targets(V, ld)
    if planted:
        tg = [IGNORE_INDEX, 0, V // 2, max(0, (V - 1) // 8 * 8), V - 1]
        top = 6.0
        a, b_ = (9, 26) if V > 26 else (2, 7)           # threads 1 and 3 (vector) / 2 and 7 (scalar)
        x[0, a] = x[0, b_] = top
        if V > 2100:
            c, d = 800, 2048                             # thread 100 | thread 0 (NT 256) or 256
        elif V > 200:
            c, d = 5, 200                                # scalar: threads 5 and 200
        else:
            c, d = 1, V - 2
        x[1, c] = x[1, d] = top
        x[2] = x[2] * 4 - 3008.0                        # bf16 spacing is 16 here: the rest is <= -2992
        x[2, V - 1] = -2976.0
        x[3] = 0.75
        x[4, tg[4]] = x[4].abs().max() + 12.0
    x[:, V:] = 50.0
    x = x.to(dtype)
    return {"logits": x.to(dev), "target": torch.tensor(tg, dtype=torch.int64, device=dev), "V": V, "ld": ld}


# (in place, grad_scale, with argmax/lse)
XENT_WAYS = [(False, 1.0, True), (True, 1.0 / 7, True), (True, 1.0, False), (False, 1.0 / 7, False)]
XENT_WRAPPER = [(BF16, 333), (torch.float32, 333), (BF16, 50257), (BF16, 1000), (torch.float32, 1000)]   # M = 63


def xent_wrapper_inputs(dtype, V, seed=0, dev="cpu"):
    gen = torch.Generator().manual_seed(V + seed)
    M = 63
    x = (torch.randn(M, V, generator=gen) * 3).to(dtype)
    t = torch.randint(0, V, (M,), generator=gen)
    t[5::9] = IGNORE_INDEX
    return {"logits": x.to(dev), "target": t.to(dev), "V": V}


def mean_loss_ref(dtype, loss_rows, n):
    """mean of the per-row losses over n, and its sum of |terms| / n."""
    v = loss_rows.to(dtype)
    return v.sum() / n, v.abs().sum() / n


# ------------------------------------------------------------------------------- causal softmax
# dS = P * (dP - sum_j P dP): dP minus the row's weighted mean of dP.  A row whose P is (nearly)
# one-hot - every short causal row, every saturated one - is that residue in all its elements,
# so this floor is taken times the row maximum of |P dP| (the terms), not of |dS|.  2^-10 misses
# the ceiling on one case, the causal T = 4096.
FLOOR_SOFTMAX_DS = 2.0 ** -9
FLOOR_SOFTMAX_P = 2.0 ** -40   # nothing cancels; below every probability of the cases


def _causal_mask(rows, T, device):
    i = (torch.arange(rows, device=device) % T)[:, None]
    return torch.arange(T, device=device)[None, :] <= i


def softmax_ref(dtype, S, T, causal, mutant=""):
    """row softmax of S [rows, T]; causal: row r keeps columns [0, r % T].  Masked entries of S
    are never looked at (they may hold NaN) and come out as exact zeros."""
    rows = S.shape[0]
    keep = _causal_mask(rows, T, S.device) if causal else torch.ones_like(S, dtype=torch.bool)
    if mutant == "diag":
        keep = keep & ~(torch.arange(T, device=S.device)[None, :] == (torch.arange(rows, device=S.device) % T)[:, None])
        keep[::T, 0] = True
    s = torch.where(keep, S.to(dtype), torch.full_like(S, -math.inf, dtype=dtype))
    m = s.amax(1, keepdim=True)
    e = torch.exp(s - m)
    z = e.sum(1, keepdim=True)
    return {"P": e * (1.0 / z), "lse": (m + torch.log(z))[:, 0], "lse_scale": (m.abs() + torch.log(z).abs())[:, 0],
            "keep": keep}


def softmax_bwd_ref(dtype, P, dP, T, causal):
    """dS = P * (dP - sum_j P dP) from the bf16 P the forward wrote."""
    rows = P.shape[0]
    keep = _causal_mask(rows, T, P.device) if causal else torch.ones_like(P, dtype=torch.bool)
    p = torch.where(keep, P.to(dtype), torch.zeros_like(P, dtype=dtype))
    d = torch.where(keep, dP.to(dtype), torch.zeros_like(dP, dtype=dtype))
    return {"dS": p * (d - (p * d).sum(1, keepdim=True)),
            "floor": (p * d).double().abs().amax(1, keepdim=True) * FLOOR_SOFTMAX_DS}


# (rows, T, causal): three (batch*head) below T = 2048, one above; a row count that is no
# multiple of 4, non-causal
SOFTMAX_CASES = [(3 * T, T, c) for T in (8, 64, 520, 1024, 1032) for c in (True, False)] + \
                [(T, T, True) for T in (2048, 4096)] + [(5, 2048, False), (5, 4096, False), (7, 64, False)]


def softmax_inputs(rows, T, causal, seed=0, dev="cpu"):
    """randn*2 scores, every 5th row with one entry +12 above the rest (saturated); above the
    diagonal NaN when causal (S and dP)."""
    gen = torch.Generator().manual_seed(T * 3 + rows + seed)
    S = torch.randn(rows, T, generator=gen) * 2
    keep = _causal_mask(rows, T, "cpu") if causal else torch.ones(rows, T, dtype=torch.bool)
    i = torch.arange(rows) % T
    hot = torch.arange(rows)[::5]
    top = torch.where(keep, S, torch.full_like(S, -math.inf)).amax(1)
    S[hot, (i[hot] // 2)] = top[hot] + 12.0
    dP = torch.randn(rows, T, generator=gen)
    if causal:
        S = torch.where(keep, S, torch.full_like(S, math.nan))
        dP = torch.where(keep, dP, torch.full_like(dP, math.nan))
    return {"S": S.to(BF16).to(dev), "dP": dP.to(BF16).to(dev)}


# ------------------------------------------------------------------------------- SwiGLU
# products: nothing cancels (1 + g (1 - sg) of silu' crosses zero at g = -1.278, but no bf16 gate
# is within 2^-9 of that root); below 2^-40 of the row maximum lie only the outputs of the
# planted -30 and +-100 gates.
FLOOR_SWIGLU = 2.0 ** -40

SWIGLU_CASES = [(3, 8), (5, 520), (64, 14336), (2100, 16384)]   # the last: the stride loop runs twice
SWIGLU_GATES = (0.0, 30.0, -30.0, 100.0, -100.0)


def swiglu_ref(dtype, gu, dh=None, mutant=""):
    """gu = [gate | up] [M, 2F]: h = silu(gate) * up; with dh also dgu = [dh up silu'(gate) | dh silu(gate)]."""
    F = gu.shape[1] // 2
    g, u = gu[:, :F].to(dtype), gu[:, F:].to(dtype)
    sg = 1.0 / (1.0 + torch.exp(-g))
    out = {"h": g * sg * u}
    if dh is not None:
        d = dh.to(dtype)
        dg, du = d * u * (sg * (1.0 + g * (1.0 - sg))), d * (g * sg)
        out["dgu"] = torch.cat([du, dg] if mutant == "swap" else [dg, du], 1)
    return out


def swiglu_inputs(M, F, seed=0, dev="cpu"):
    gen = torch.Generator().manual_seed(M * 31 + F + seed)
    gu = torch.randn(M, 2 * F, generator=gen) * 2
    for j, v in enumerate(SWIGLU_GATES):   # exactly representable gates, next to random ones
        gu[j % M, (3 * j) % F] = v
        gu[M - 1 - j % M, F - 1 - (3 * j) % F] = v
    return {"gu": gu.to(BF16).to(dev), "dh": torch.randn(M, F, generator=gen).to(BF16).to(dev)}


def swiglu_chunks(M, F):
    """row ranges of at most 2^22 elements, so the fp64 reference of the large case stays small"""
    step = max(1, (1 << 22) // F)
    return [(r, min(M, r + step)) for r in range(0, M, step)]


# ------------------------------------------------------------------------------- RoPE
# y1 = x1 cos - x2 sin, y2 = x2 cos + x1 sin: a difference (sum) of two products per element.
FLOOR_ROPE = 2.0 ** -7

ROPE_CASES = [(Dh, H, Hkv) for Dh in (16, 64, 128) for H, Hkv in ((4, 2), (3, 3))]   # B = 2, T = 37
ROPE_B, ROPE_T, ROPE_THETA = 2, 37, 500000.0


def rope_ref(dtype, x, T, H, Hkv, Dh, theta=ROPE_THETA, inverse=False, mutant=""):
    """rotate-half RoPE on packed qkv [B, T, (H + 2 Hkv) Dh]: q and k heads rotated by the angle
    of t = token % T (by its negative with inverse), v heads copied.  cos / sin are computed here
    in `dtype`, so the kernel's fp32 tables are judged too."""
    B = x.shape[0]
    xh = x.reshape(B, -1, H + 2 * Hkv, Dh).to(dtype)
    ntok = xh.shape[1]
    inv = 1.0 / (torch.tensor(theta, dtype=dtype, device=x.device) **
                 (torch.arange(0, Dh, 2, dtype=dtype, device=x.device) / Dh))
    t = torch.arange(ntok, device=x.device)
    if mutant == "nowrap":
        t = t[None, :] + T * torch.arange(B, device=x.device)[:, None]
    else:
        t = (t % T)[None, :].expand(B, -1)
    ang = t.to(dtype)[..., None] * inv
    c, s = torch.cos(ang)[:, :, None, :], torch.sin(ang)[:, :, None, :]
    if inverse:
        s = -s
    s = s.expand(B, ntok, H + Hkv, Dh // 2)
    if mutant == "ksign":
        s = torch.cat([s[:, :, :H], -s[:, :, H:]], 2)
    rot = xh[:, :, : H + Hkv]
    x1, x2 = rot[..., : Dh // 2], rot[..., Dh // 2:]
    out = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)
    return torch.cat([out, xh[:, :, H + Hkv:]], 2)   # [B, T, heads, Dh]: a "row" is one head


def rope_inputs(Dh, H, Hkv, seed=0, dev="cpu"):
    gen = torch.Generator().manual_seed(Dh * 100 + H * 10 + Hkv + seed)
    W = (H + 2 * Hkv) * Dh
    return {"x": torch.randn(ROPE_B, ROPE_T, W, generator=gen).to(BF16).to(dev),
            "dy": torch.randn(ROPE_B, ROPE_T, W, generator=gen).to(BF16).to(dev)}


# ------------------------------------------------------------------------------- judging one case
# `outs` holds the kernel's outputs by name; a missing name is judged for the twin alone (all of
# them on the CPU, where tests/test_ulp_cpu.py holds the twin condition).
F64, F32 = torch.float64, torch.float32


def judge_norm(J, op, shape, c, eps, rms, outs, bwd=True, rows_per_wave=1):
    """rows_per_wave: the rows a backward wave adds serially into dgamma / dbeta / colsum(dx)."""
    D = c["x"].shape[-1]
    a = (c["x"], c["g"], c["b"], eps, c["dy"] if bwd else None, c["dres"] if bwd else None, rms)
    r, t = norm_ref(F64, *a), norm_ref(F32, *a)
    lane_terms = 8 * ((D // 8 + 63) // 64)   # a lane adds its CPL x 8 elements before the wave tree
    J.ulp(op, shape, "y", outs.get("y"), r["y"], t["y"], row_floor(r["y"], FLOOR_RMS_Y if rms else FLOOR_LN_Y))
    if not rms:
        J.rel(op, shape, "mean", outs.get("mean"), r["mean"], t["mean"], r["mean_scale"], lane_terms)
    J.rel(op, shape, "rstd", outs.get("rstd"), r["rstd"], t["rstd"], r["rstd"].abs(), lane_terms)
    if bwd:
        J.ulp(op, shape, "dx", outs.get("dx"), r["dx"], t["dx"], row_floor(r["dx"], FLOOR_NORM_DX))
        for n in ("dgamma",) + (() if rms else ("dbeta", "dxsum")):
            J.rel(op, shape, n, outs.get(n), r[n], t[n], r[n + "_scale"], rows_per_wave)
    return r


def judge_xent(J, op, shape, c, grad_scale, outs, threads=256, k=1):
    V = c["V"]
    r = xent_ref(F64, c["logits"], c["target"], V, grad_scale)
    t = xent_ref(F32, c["logits"], c["target"], V, grad_scale)
    R = -(-c["logits"].shape[1] // threads)   # columns a thread adds serially
    g = outs.get("grad")
    J.ulp(op, shape, "grad", None if g is None else g[:, :V], r["grad"], t["grad"], xent_grad_floor(r, grad_scale), k)
    J.rel(op, shape, "loss", outs.get("loss"), r["loss"], t["loss"], r["loss_scale"], R)
    J.rel(op, shape, "lse", outs.get("lse"), r["lse"], t["lse"], r["lse_scale"], R)
    return r


def judge_softmax_fwd(J, shape, c, T, causal, outs):
    r, t = softmax_ref(F64, c["S"], T, causal), softmax_ref(F32, c["S"], T, causal)
    lane_terms = 8 * ((T // 8 + 63) // 64)
    J.ulp("softmax", shape, "P", outs.get("P"), r["P"], t["P"], row_floor(r["P"], FLOOR_SOFTMAX_P))
    J.rel("softmax", shape, "lse", outs.get("lse"), r["lse"], t["lse"], r["lse_scale"], lane_terms)
    return r, t


def judge_softmax_bwd(J, shape, P, dP, T, causal, out):
    r, t = softmax_bwd_ref(F64, P, dP, T, causal), softmax_bwd_ref(F32, P, dP, T, causal)
    J.ulp("softmax", shape, "dS", out, r["dS"], t["dS"], r["floor"])


def judge_swiglu(J, shape, c, outs):
    """in row chunks, so the fp64 reference of the large case stays small"""
    M, F = c["dh"].shape
    for a, b in swiglu_chunks(M, F):
        r, t = swiglu_ref(F64, c["gu"][a:b], c["dh"][a:b]), swiglu_ref(F32, c["gu"][a:b], c["dh"][a:b])
        sh = shape if (a, b) == (0, M) else f"{shape} rows {a}:{b}"
        for n in ("h", "dgu"):
            o = outs.get(n)
            J.ulp("swiglu", sh, n, None if o is None else o[a:b], r[n], t[n], row_floor(r[n], FLOOR_SWIGLU))


def judge_rope(J, shape, x, H, Hkv, Dh, inverse, out, what="y"):
    a = (x, ROPE_T, H, Hkv, Dh, ROPE_THETA, inverse)
    r, t = rope_ref(F64, *a), rope_ref(F32, *a)
    J.ulp("rope", shape, what, None if out is None else out.reshape(r.shape), r, t, row_floor(r, FLOOR_ROPE))
    return r


# ------------------------------------------------------------------------------- flash attention
# attn_flash.hip (fwd_kernel and bwd_dq_kernel with one and two 16-row groups per wave, G = 1 | 2;
# bwd_dkdv_kernel, bwd_dkdv2_kernel, dkdv_reduce_kernel) and the composed
# GEMM + softmax path of ops/attention.py, judged per element against an explicit fp64 forward and
# backward.  Unlike the row kernels these round to bf16 INSIDE the computation (the probabilities
# feed MFMAs as bf16 operands), so the allowance is not measured from an unrounded twin: it is the
# first-order bound of those roundings, counted from the source, each term taken with the absolute
# values of its leaves.  The twin applies the same roundings in fp32 and has to stay inside it
# (tests/test_ulp_cpu.py); no coefficient is tuned against a kernel.
# Relative error of one round-to-nearest conversion to bf16 (8 significant bits): half a spacing,
# 2^-8 of the binade's lower end.  (2^-9 is its value at the upper end; with it the twin, which
# only rounds where the kernels do, left the allowance on dV by up to 1.29 x and on out by 1.04 x.)
U_BF16 = 2.0 ** -8
U2 = (1.0 + U_BF16) ** 2 - 1.0     # two such roundings in a product chain (2u + u^2)
LOG2E = 1.4426950408889634
ATTN_OUTPUTS = ("out", "lse", "delta", "dq", "dk", "dv")
ATTN_MUTANTS = ("diag_upper", "diag_wave_last", "drop_key", "scores_x102", "bwd_p_x102", "l_low", "dout_dropped",
                "group_first_only", "doc_start_low", "doc_end_low")


def _f32_terms(n: int) -> float:
    """the fp32 share of an allowance: n serially added terms + 64 (v_exp / v_log / v_rcp, the MFMA's
    own accumulation, another summation order), in units of 2^-24 of the sum of |terms|"""
    return (n + 64) * 2.0 ** -24


def _rb(x: torch.Tensor, on: bool) -> torch.Tensor:
    return x.to(BF16).to(x.dtype) if on else x


def _stored(ref: torch.Tensor, a: torch.Tensor) -> torch.Tensor:
    """allowance of a value the kernel stores as bf16, a = the allowance before that rounding: the
    value rounded is within a of ref, so the rounding adds at most half a spacing of |ref| + a"""
    return a + 0.5 * ulp_bf16((ref.abs() + a).clamp_min(TINY))


def doc_arrays(lengths, T, dev="cpu"):
    """(start, end) int64 [B, T] of a list of document lengths per batch row (what DocLayout holds)."""
    st, en = [], []
    for row in lengths:
        assert sum(row) == T and min(row) > 0
        s, e, at = [], [], 0
        for n in row:
            s += [at] * n
            e += [at + n] * n
            at += n
        st.append(s)
        en.append(e)
    return torch.tensor(st, device=dev), torch.tensor(en, device=dev)


def attn_masks(B, T, docs, dev, mutant=""):
    """keep_q [B, Tq, Tk]: start[q] <= k <= q, as the query-row kernels (fwd, dQ) test it;
    keep_kv: k <= q < end[k], as the key-row kernels (dK/dV) do.  The same set for a valid layout."""
    pos = torch.arange(T, device=dev)
    if docs is None:
        start, end = torch.zeros(B, T, dtype=torch.int64, device=dev), torch.full((B, T), T, device=dev)
    else:
        start, end = docs[0].long().clone(), docs[1].long().clone()
    if mutant in ("doc_start_low", "doc_end_low"):
        # the longest document of batch row 0 that does not begin the row
        s0 = start[0]
        cand = torch.unique(s0[s0 > 0])
        assert cand.numel(), "the mutant needs a second document"
        first = cand[torch.stack([(s0 == c).sum() for c in cand]).argmax()]
        if mutant == "doc_start_low":
            start[0, s0 == first] -= 1
        else:
            end[0, s0 == first] -= 1
    q, k = pos[None, :, None], pos[None, None, :]
    keep_q = (k >= start[:, :, None]) & (k <= q)
    keep_kv = (k <= q) & (q < end[:, None, :])
    if mutant in ("diag_upper", "diag_wave_last", "drop_key"):
        if mutant == "diag_upper":
            hit = (k == q) & (q >= T // 2)
        elif mutant == "diag_wave_last":
            hit = (k == q) & (q >= T - 64) & (q % 16 == 15)
        else:
            hit = (k == T // 2 - 3) & (q >= T - 64)
        keep_q = keep_q & ~hit
        keep_kv = keep_kv & ~hit
    return keep_q, keep_kv, mutant != "doc_end_low"


def attn_ref(dtype, qkv, dout, B, T, H, Hkv, Dh, docs=None, twin=False, mutant="", path="flash"):
    """Causal (document-masked with docs = (start, end)) attention on packed qkv [B, T, (H + 2 Hkv) Dh]
    with GQA, forward and backward written out: S, m, e, l, O, lse | delta, P, dP, dS, dQ, dK, dV.

    dtype float64, twin False: the reference; it also returns the per-element allowance of every
    output ("allow_<name>").  twin=True (float32): the kernel's bf16 roundings where attn_flash.hip
    places them - e ahead of P.V and of the row sum (pack_pair in fwd_kernel; with G = 2 it sums the
    unrounded e, one rounding fewer), O as stored and as delta reads it, P ahead of dV, dS ahead of
    dQ / dK, each stored gradient once after the fp32 sum over the group (registers, or the
    head-split partials).  path="gemm": the composed path of ops/attention.py, which also stores
    S, P, dP and dS as bf16 matrices and adds the group's dK / dV in bf16.
    Masked entries are never looked at.  `mutant`: a deliberate error (ATTN_MUTANTS)."""
    assert mutant == "" or mutant in ATTN_MUTANTS
    dev, G, C = qkv.device, H // Hkv, H * Dh
    gemm = path == "gemm"
    rq = twin and not gemm   # the flash kernels' roundings
    rg = twin and gemm       # the composed path's
    scale = _f32(1.0 / math.sqrt(Dh))   # a float in the kernels
    x = qkv.to(dtype)
    heads = lambda t, n, g: t.reshape(B, T, n, g, Dh).permute(0, 2, 3, 1, 4)   # [B, n, g, T, Dh]; head = n * G + g
    q, k, v = heads(x[..., :C], Hkv, G), heads(x[..., C:C + Hkv * Dh], Hkv, 1), heads(x[..., C + Hkv * Dh:], Hkv, 1)
    do = heads(dout.to(dtype), Hkv, G)
    keep_q, keep_kv, same = attn_masks(B, T, docs, dev, mutant)
    kq, kkv = keep_q[:, None, None], keep_kv[:, None, None]
    tr = lambda t: t.transpose(-1, -2)
    zero = torch.zeros((), dtype=dtype, device=dev)

    # ---- forward
    S = _rb((q @ tr(k)) * scale, rg)                      # [B, Hkv, G, Tq, Tk]
    if mutant == "scores_x102":
        S[..., T // 2:, :] *= 1.02
    Sm = torch.where(kq, S, torch.full_like(S, -math.inf))
    m = Sm.amax(-1, keepdim=True)
    e = _rb(torch.exp(Sm - m), rq)
    l = e.sum(-1, keepdim=True)
    if mutant == "l_low":
        l[..., T - 64:, :] *= 1.0 - 2.0 ** -6
    if gemm:
        Pf = _rb(e / l, rg)                               # the stored bf16 P, which the backward re-reads
        O = _rb(Pf @ v, rg)
    else:
        O = _rb((e @ v) / l, rq)
    lse = m + torch.log(l)

    # ---- backward
    dob = do
    if mutant == "dout_dropped":
        dob = do.clone()
        dob[:, -1, -1, T - 16:] = 0
    dP = dob @ tr(v)
    if gemm:
        dP = _rb(dP, rg)
        Praw = Pf
        delta = torch.where(kq, Pf * dP, zero).sum(-1, keepdim=True)   # softmax_bwd's row term
    else:
        Praw = torch.exp(S - lse)
        delta = (dob * O).sum(-1, keepdim=True)
    if mutant == "bwd_p_x102":
        Praw = Praw.clone()
        Praw[..., 64:, :] *= 1.02
    P = torch.where(kq, Praw, zero)
    dS = _rb(P * (torch.where(kq, dP, zero) - delta), twin)
    if same:
        Pk, dSk = P, dS
    else:
        Pk = torch.where(kkv, Praw, zero)
        dSk = _rb(Pk * (torch.where(kkv, dP, zero) - delta), twin)
    dQ = _rb((dS @ k) * scale, twin)
    dVg, dKg = tr(_rb(Pk, rq)) @ dob, (tr(dSk) @ q) * scale    # per q-head [B, Hkv, G, Tk, Dh]
    if mutant == "group_first_only":
        dVg[:, :, 1:, T - 64:] = 0
        dKg[:, :, 1:, T - 64:] = 0
    if rg:   # beta = 1 GEMMs: every q-head of the group is added to the stored bf16 rows
        dV, dK = _rb(dVg[:, :, 0], True), _rb(dKg[:, :, 0], True)
        for g in range(1, G):
            dV, dK = _rb(dV + dVg[:, :, g], True), _rb(dK + dKg[:, :, g], True)
    else:
        dV, dK = _rb(dVg.sum(2), twin), _rb(dKg.sum(2), twin)

    rows = lambda t: t.permute(0, 3, 1, 2, 4).reshape(B, T, -1)      # [B, n, g, T, Dh] -> [B, T, n g Dh]
    kvrows = lambda t: t.permute(0, 2, 1, 3).reshape(B, T, -1)       # [B, Hkv, T, Dh]
    vec = lambda t: t[..., 0].reshape(B * H, T)
    res = {"out": rows(O), "lse": vec(lse) * LOG2E, "delta": vec(delta), "dq": rows(dQ), "dk": kvrows(dK),
           "dv": kvrows(dV)}
    if dtype != F64 or twin or mutant:
        return res

    # ---- the allowance (u = U_BF16; F(n) = _f32_terms(n) of the sum of |terms| at the leaves)
    u, Fk, Fg, Fd = U_BF16, _f32_terms(T), _f32_terms(G * T), _f32_terms(Dh)
    av, ak, aq, ado = v.abs(), k.abs(), q.abs(), do.abs()
    pv, pk = P @ av, P @ ak
    dterms = (do * O).abs().sum(-1, keepdim=True)             # the leaves of delta
    dpl = torch.where(kq, ado @ tr(av), zero) + dterms        # the leaves of dP - delta
    Wt = P * (torch.where(kq, dP, zero) - delta).abs()        # |dS|
    if not gemm:
        # out: e rounded (numerator) and l the sum of rounded e (denominator): U2; O stored as bf16
        A_o = _stored(O, (U2 + Fk) * pv)
        # delta = sum_d dO * O(stored)
        E_d = (ado * A_o).sum(-1, keepdim=True) + Fd * dterms
        # lse = m + log2 l, l within u (sum of rounded e); the lazy rescale keeps the kernel's m
        # within 8 below the row maximum, so |m| + |log2 l| is up to 16 above the reference's
        A_lse = LOG2E * u + Fk * (LOG2E * (m.abs() + torch.log(l).abs()) + 16.0)
        # dV: P = 2^(s c - lse) inherits u from lse and is rounded by pack_pair: U2; dV stored as bf16
        A_dv = _stored(dV, (U2 + Fg) * (tr(P) @ ado).sum(2))
        # dQ: u from lse in P, dS rounded by pack_pair: U2; P x (error of delta); dQ stored as bf16
        A_dq = _stored(dQ, scale * (U2 * (Wt @ ak) + Fk * ((P * dpl) @ ak) + E_d * pk))
        # dK: the mirror image, summed over the group in fp32 and stored once
        A_dk = _stored(dK, scale * (U2 * (tr(Wt) @ aq) + Fg * (tr(P * dpl) @ aq) + tr(P * E_d) @ aq).sum(2))
    else:
        # gemm_bf16 stores S = bf16(alpha Q K^T): e carries u |s|, and so does l, p-weighted; the
        # softmax stores P = bf16(e / l): relative error of p_ij
        sabs = torch.where(kq, S, zero).abs()
        r = u * (1.0 + sabs + (P * sabs).sum(-1, keepdim=True)) + Fk
        A_o = (P * r) @ av + (u + Fk) * pv                      # + O rounded when stored
        # dP = bf16(dO V^T); the row term sum_j P dP is formed from the stored P and dP
        adp = torch.where(kq, dP, zero).abs()
        E_d = (P * (r + u) * adp).sum(-1, keepdim=True) + Fk * (P * adp).sum(-1, keepdim=True)
        A_lse = torch.zeros_like(lse)                           # the composed path keeps no lse
        # dS = bf16(P (dP - row term)): error of P, of dP, of the row term, its own rounding
        E_s = P * (r * (adp + delta.abs()) + u * adp + E_d) + u * Wt + Fd * P * dpl
        A_dq = scale * (E_s @ ak + (u + Fk) * (Wt @ ak))        # + dQ rounded when stored
        # dK / dV: one bf16 rounding per q-head added (beta = 1 re-reads the stored rows)
        gV, gK = tr(P) @ ado, scale * (tr(Wt) @ aq)             # per q-head sums of |terms|
        cum = lambda t: sum(t[:, :, : g + 1].sum(2) for g in range(G))   # |partial sum| after each add
        A_dv = (tr(P * r) @ ado).sum(2) + u * cum(gV) + Fk * gV.sum(2)
        A_dk = scale * (tr(E_s) @ aq).sum(2) + u * cum(gK) + Fk * gK.sum(2)
    res.update(allow_out=rows(A_o), allow_lse=vec(A_lse), allow_delta=vec(E_d), allow_dq=rows(A_dq),
               allow_dk=kvrows(A_dk), allow_dv=kvrows(A_dv))
    return res


def allow_err(out, ref64, allow) -> float:
    """max |out - ref| / allowance, elementwise (an exact match scores 0 whatever the allowance)."""
    d = (out.double() - ref64.double()).abs()
    e = torch.where(d == 0, torch.zeros_like(d), d / allow.double())
    return float("nan") if bool(torch.isnan(e).any()) else e.max().item()


def old_yardstick(out, ref64, rel) -> bool:
    """`_close` of tests/test_kernels_gpu.py and tests/test_attn_docmask_gpu.py: the largest error of the
    tensor against rel x the largest magnitude of the tensor"""
    return (out.double() - ref64).abs().max().item() <= rel * (ref64.abs().max().item() + 1e-6)


# -- inputs
ATTN_GENS = ("randn", "peaky", "spikes", "offset")
SPIKE_A, SPIKE_B = 8.25, 22.0   # log2-domain scores of the two planted keys (tile 1, tile 2)


def attn_inputs(gen, B, T, H, Hkv, Dh, seed=0, dev="cpu"):
    """qkv [B, T, (H + 2 Hkv) Dh] and dout [B, T, H Dh], bf16.
    randn: plain.  peaky: q and k x 3 (rows near one-hot).
    spikes (T >= 256): the rows of the last 64-row block are one +-1 direction w plus a little
    noise, and two keys are multiples of w - one in key tile 1 scoring SPIKE_A, one in tile 2
    scoring SPIKE_B in the log2 domain - so every row's running maximum rises by clearly less than
    8 at tile 1 (no rescale, e up to 2^7) and by clearly more at tile 2 (rescale): the
    `mx * c > m + 8` test of the forward kernels (attn_spike_rises measures it).
    offset: dimension 0 of every key is 16; q-head 0 has the matching value that puts all its
    scores near +60 in the log2 domain, the last q-head (H > 1) near -40."""
    gen_ = torch.Generator().manual_seed(7919 * T + 131 * Dh + 17 * H + 3 * Hkv + B + seed)
    C, KV = H * Dh, Hkv * Dh
    x = torch.randn(B, T, C + 2 * KV, generator=gen_)
    dout = torch.randn(B, T, C, generator=gen_)
    qv, kv_ = x[..., :C].view(B, T, H, Dh), x[..., C:C + KV].view(B, T, Hkv, Dh)
    if gen == "peaky":
        qv *= 3
        kv_ *= 3
    elif gen == "spikes":
        assert T >= 256
        w = torch.where(torch.rand(Dh, generator=gen_) < 0.5, -1.0, 1.0)
        qv[:, T - 64:] = w + 0.125 * qv[:, T - 64:]
        # scale * (w . gamma w) = gamma sqrt(Dh) in natural units
        kv_[:, 64 + 5] = w * (SPIKE_A / LOG2E / math.sqrt(Dh))
        kv_[:, 128 + 37] = w * (SPIKE_B / LOG2E / math.sqrt(Dh))
    elif gen == "offset":
        kv_[..., 0] = 16.0
        qv[:, :, 0, 0] = 60.0 / LOG2E * math.sqrt(Dh) / 16.0
        if H > 1:
            qv[:, :, H - 1, 0] = -40.0 / LOG2E * math.sqrt(Dh) / 16.0
    else:
        assert gen == "randn"
    return {"qkv": x.to(BF16).to(dev), "dout": dout.to(BF16).to(dev)}


def attn_spike_rises(qkv, B, T, H, Hkv, Dh):
    """per row of the last 64-row block (plain causal): the rise of the running maximum over the
    tile-0 maximum at key tile 1 and at key tile 2, log2 domain - what the lazy rescale tests"""
    C, G = H * Dh, H // Hkv
    x = qkv.double()
    q = x[..., :C].reshape(B, T, Hkv, G, Dh).permute(0, 2, 3, 1, 4)[..., T - 64:, :]
    k = x[..., C:C + Hkv * Dh].reshape(B, T, Hkv, 1, Dh).permute(0, 2, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * (LOG2E / math.sqrt(Dh))
    m0, m1, m2 = (s[..., 64 * t:64 * t + 64].amax(-1) for t in range(3))
    return m1 - m0, m2 - torch.maximum(m0, m1), m2 - m0


# -- document layouts (lengths per batch row).  A: a boundary inside the first wave (5), one
# mid-wave, two documents of length 1, later blocks that continue a document from an earlier key
# tile; batch row 1 a single document, row 2 the reverse of row 0.  T = 192 and 256 are LAYOUT_A
# of tests/test_attn_docmask_gpu.py.
_LAYOUT_A = {64: [5, 35, 1, 1, 22], 128: [5, 65, 1, 1, 56], 192: [5, 65, 1, 1, 58, 62],
             256: [5, 65, 1, 1, 58, 126], 384: [5, 65, 1, 1, 58, 126, 70, 58]}
_ALIGNED = {64: [64], 128: [64, 64], 192: [64, 128], 256: [64, 128, 64], 384: [64, 128, 64, 128]}
ATTN_LAYOUTS = ("A", "aligned", "ones")


def attn_layout(name, T, B):
    if name == "ones":
        return [[1] * T for _ in range(B)]
    if name == "aligned":
        a = _ALIGNED[T]
        return [a, a[::-1], [64] * (T // 64)][:B]
    a = _LAYOUT_A[T]
    return [a, [T], a[::-1]][:B]


# -- the case table: (B, T, H, Hkv, Dh, generator).  T = 64 one tile; 128 the first size of the
# 32-row kernels; 192 forces the 64-row kernels and wraps the NS = 2 ring; 256 two 128-row blocks
# and four key tiles; 384 three 128-row blocks.  Group sizes 1, 2, 4, 8; B chosen so that every
# launch grid meets every branch of xcd_grid (test_attn_grids_meet_every_xcd_branch).
ATTN_CASES = [
    (1, 64, 1, 1, 64, "randn"),
    (3, 64, 4, 2, 128, "peaky"),
    (2, 128, 4, 4, 64, "randn"),
    (1, 128, 8, 2, 128, "offset"),
    (3, 128, 8, 1, 64, "offset"),
    (2, 192, 4, 2, 64, "randn"),
    (1, 192, 8, 1, 128, "peaky"),
    (2, 256, 4, 2, 64, "spikes"),
    (1, 256, 4, 4, 128, "randn"),
    (1, 384, 1, 1, 64, "randn"),
    (2, 384, 4, 2, 128, "peaky"),
]
ATTN_VARIANTS = [(1, 1, 1), (2, 2, 2), (1, 2, 1), (2, 1, 2)]   # (RTDC_FA_FWD, RTDC_FA_DQ, RTDC_FA_DKDV)
ATTN_DIRECT = [ATTN_CASES[7], ATTN_CASES[3]]                   # the cases the GPU test also launches directly
ATTN_GEMM = [(2, 100, 4, 2, 64, "randn"), (1, 128, 8, 2, 128, "peaky")]   # RTDC_ATTN=gemm


def attn_case_id(c):
    return "B%d-T%d-H%d-Hkv%d-Dh%d-%s" % c


def attn_head_splits(H, Hkv):
    """the RTDC_FA_QS values ops/attention.py honours for this group size"""
    return [qs for qs in (1, 2, 4) if (H // Hkv) % qs == 0]


def attn_launches(B, T, H, Hkv, Dh, v, qs):
    """(kernel, gridDim.x, gridDim.y) of the three launches, from flash_fwd_launch / flash_bwd_launch
    with all three variant knobs set (so Dh = 128 takes bwd_dkdv2 when asked).  "fwd2" and "dq2" are
    fwd_kernel and bwd_dq_kernel with G = 2 (32 rows per wave, 128-row blocks), the bare names G = 1."""
    two = T % 128 == 0
    f, d, kv = (x == 2 and two for x in v)
    return [("fwd2" if f else "fwd", T // (128 if f else 64), B * H),
            ("dq2" if d else "dq", T // (128 if d else 64), B * H),
            ("dkdv2" if kv else "dkdv", T // (128 if kv else 64), B * Hkv * qs)]


def xcd_branch(gx, gy):
    """the branch of xcd_grid (common.h, x_major) a grid takes"""
    n = gx * gy
    return "rows" if gy % 8 == 0 else ("even" if n % 8 == 0 else ("ragged<8" if n < 8 else "ragged"))


def judge_attn(J, fams, shape, ref, twin, outs, names=("out", "dq", "dk", "dv")):
    """fams: the kernel that wrote each output, by output name (the WORST lines go by it)"""
    for n in names:
        J.within(fams[n], shape, n, outs.get(n), ref[n], twin[n], ref["allow_" + n])


# ------------------------------------------------------------------------------- GEMM
# C = act(alpha A.B + bias + beta Cin): an element is a sum of K signed products (plus the bias and
# the residual), so it can be arbitrarily small against S = sum |terms|: what cancels is the K-term
# sum itself.  Below FLOOR_GEMM x S an element is judged in ulps of that floor.  Measured on the
# whole case table (tests/test_ulp_cpu.py::test_twin_gemm): the twin's worst error is 0.0107 ulp
# at 2^-10, 0.0426 at 2^-12 and 0.164 at 2^-14, so 2^-12 is the smallest power of two under 2^-4.
FLOOR_GEMM = 2.0 ** -12

GEMM_MUTANTS = ("truncate", "drop_k_last", "cols_scaled", "bias_shift", "slab_bf16", "res_after_act",
                "gelu_of_rounded", "colsum_rounded")
GELU_ROOT = -0.75     # the bf16 number nearest the root of gelu' (-0.7518); its neighbours are +-2^-8
GEMM_AUX_PLANTED = (GELU_ROOT, GELU_ROOT - 2.0 ** -8, GELU_ROOT + 2.0 ** -8, 0.0, 6.0, -6.0, 20.0, -20.0)


def gelu_parts(x):
    """(sigmoid, gelu') of the tanh-form GELU as common.h writes it: gelu_sigmoid_arg, gelu_tanh_grad"""
    k0, k1 = _f32(0.7978845608028654), _f32(0.044715)
    u = k0 * (k1 * x * x * x + x)
    s = 1.0 / (1.0 + torch.exp(-2.0 * u))
    return s, 2.0 * x * s * (1.0 - s) * k0 * (3.0 * k1 * x * x + 1.0) + s


def gemm_alpha(alpha, alpha_dev=None) -> float:
    """alpha as the kernels form it: a float, times the device scalar in fp32"""
    a = _f32(alpha)
    return a if alpha_dev is None else _f32(a * float(alpha_dev.float().reshape(-1)[0]))


def _truncate_bf16(x):
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(x.dtype)


def gemm_ref(dtype, A, B, a_kmajor=True, b_kmajor=True, *, alpha=1.0, alpha_dev=None, bias=None, Cin=None, beta=0.0,
             act=0, aux_in=None, mutant="", slabs=4):
    """gemm_bf16 / gemm_f32 with the fused epilogue.  A, B as stored: K-major [M, K] / [N, K] or
    MN-major [K, M] / [K, N], leading batch dimensions allowed.  The order is epilogue4's and
    tile_epilogue_bf16's: alpha x the sum, + bias, + beta Cin, then the activation (1 relu, 2 gelu
    with the pre-activation as aux_out, 5 gelu with gelu' as aux_out, 3 / 6 / 4 x gelu'(aux_in) /
    aux_in / [aux_in > 0]).  act 2 stores the rounded pre-activation but applies GELU to the
    unrounded one (gemm_common.h epilogue4: store4 of v, then gelu_tanh(v)).
    Returns C, aux_out, the column sums of C, and S = |alpha| |A| |B| + |bias| + |beta Cin| (x the
    activation factor of act 3 / 6 / 4), with S_aux for aux_out, colsum_scale = colsum(S) and
    S_rel, the scale of an fp32 C (S, but for act 3: see there).
    `mutant`: a deliberate error (GEMM_MUTANTS), used only by tests/test_ulp_cpu.py."""
    assert mutant == "" or mutant in GEMM_MUTANTS
    tr = lambda t: t.transpose(-1, -2)
    a = A.to(dtype) if a_kmajor else tr(A.to(dtype))   # [.., M, K]
    b = tr(B.to(dtype)) if b_kmajor else B.to(dtype)   # [.., K, N]
    K = a.shape[-1]
    al = gemm_alpha(alpha, alpha_dev)
    S = abs(al) * (a.abs() @ b.abs())
    if mutant == "drop_k_last":
        a = a.clone()
        a[..., -8:, K - 1] = 0
    if mutant == "slab_bf16":
        per = -(-(K // 64) // slabs) * 64
        v = sum(_rb(al * (a[..., k0:k0 + per] @ b[..., k0:k0 + per, :]), True) for k0 in range(0, K, per))
    else:
        v = al * (a @ b)
    if bias is not None:
        bb = bias.to(dtype)
        S = S + bb.abs()
        if mutant == "bias_shift":
            bb = bb.clone()
            bb[-8:] = bb[-16:-8]
        v = v + bb
    res = None
    if Cin is not None and beta != 0.0:
        res = _f32(beta) * Cin.to(dtype)
        S = S + res.abs()
        if mutant != "res_after_act":
            v = v + res
    aux_out = S_aux = S_rel = None
    if act == 1:
        C, aux_out, S_aux = v.clamp_min(0), v, S          # (gemm_f32 stores the pre-activation)
    elif act == 2:
        x = _rb(v, True) if mutant == "gelu_of_rounded" else v
        C, aux_out, S_aux = x * gelu_parts(x)[0], v, S
    elif act == 5:
        s, g = gelu_parts(v)
        # gelu' = s + x (...): terms of size <= 1 next to what v's own error moves (|gelu''| < 1.2)
        C, aux_out, S_aux = v * s, g, S + 1.0
    elif act in (3, 4, 6):
        h = aux_in.to(dtype)
        if act == 3:
            s, f = gelu_parts(h)
            # gelu' = s + x (...) is itself a sum of two terms that cancel at its root (-0.7518):
            # next to it the fp32 twin is 1.3e-5 of S |gelu'| - above TWIN_REL_CEIL - so an fp32
            # output is judged against S x the two terms' magnitudes (S_rel).  A bf16 output keeps
            # S |gelu'| under its floor: the twin stays below 2^-4 ulp there.
            S_rel = S * (s.abs() + (f - s).abs())
        else:
            f = h if act == 6 else (h > 0).to(dtype)
        C, S = v * f, S * f.abs()
    else:
        assert act == 0
        C = v
    if mutant == "res_after_act" and res is not None:
        C = C + res
    if mutant == "cols_scaled":
        C = C.clone()
        C[..., -8:] *= 1.0 + 2.0 ** -7
    if mutant == "truncate":
        C = _truncate_bf16(C)
    cs = (_rb(C, True) if mutant == "colsum_rounded" else C).sum(-2)
    return {"C": C, "S": S, "S_rel": S if S_rel is None else S_rel, "aux_out": aux_out, "S_aux": S_aux, "colsum": cs,
            "colsum_scale": S.sum(-2)}


# -- inputs
GEMM_GENS = ("randn", "range")


def gemm_inputs(gen, M, N, K, seed=0, dev="cpu", bscale=1.0, batch=(), dtype=BF16):
    """the logical operands a [.., M, K] and b [.., K, N] (`gemm_store` lays them out).
    randn: plain (b x bscale).  range: row M // 3 of a x 2^-20, column 2 N // 3 of b x 2^10, and
    (from two K-tiles on) one K-tile of a all zero - rows and columns that a whole-tensor
    criterion does not see."""
    g = torch.Generator().manual_seed(1009 * M + 31 * N + K + 7 * len(gen) + seed)
    a = torch.randn(*batch, M, K, generator=g)
    b = torch.randn(*batch, K, N, generator=g) * bscale
    if gen == "range":
        a[..., M // 3, :] *= 2.0 ** -20
        b[..., :, 2 * N // 3] *= 2.0 ** 10
        if K >= 128:
            kt = (K // 64) // 2
            a[..., :, 64 * kt:64 * kt + 64] = 0
    else:
        assert gen == "randn"
    return a.to(dtype).to(dev), b.to(dtype).to(dev)


def gemm_store(a, b, a_kmajor, b_kmajor):
    """(A, B) as the kernel reads them: K-major [M, K] / [N, K] or MN-major [K, M] / [K, N]"""
    tr = lambda t: t.transpose(-1, -2).contiguous()
    return (a if a_kmajor else tr(a)), (tr(b) if b_kmajor else b)


def gemm_aux_in(M, N, seed=0, dev="cpu"):
    """randn with the bf16 numbers around the root of gelu' and 0, +-6, +-20 planted (twice each)"""
    g = torch.Generator().manual_seed(977 * M + N + seed)
    h = torch.randn(M, N, generator=g)
    for j, v in enumerate(GEMM_AUX_PLANTED):
        h[(7 * j) % M, (13 * j + 1) % N] = v
        h[M - 1 - (5 * j) % M, N - 1 - (11 * j) % N] = v
    return h.to(BF16).to(dev)


# -- the epilogue variants: name -> what the call gets.  bias "bf16" / "f32"; cin "alias" (Cin is
# C) / "sep"; colsum: also colsum_out.  "mul" (act 6) takes as aux_in the gelu' that the act-5
# call of the same kernel stored (the saved-derivative round trip; on the CPU the twin's, rounded).
GEMM_EPILOGUES = {
    "plain": {},
    "bias_bf16": {"bias": "bf16"},
    "bias_f32": {"bias": "f32"},
    "alpha": {"alpha": 0.5},
    "alpha_dev": {"alpha": 0.5, "alpha_dev": 0.75},
    "cin_alias": {"cin": "alias", "beta": 0.5},
    "accumulate": {"cin": "alias", "beta": 1.0},
    "cin_sep": {"cin": "sep", "beta": 0.5, "bias": "bf16"},
    "relu": {"bias": "f32", "act": 1},
    "gelu": {"bias": "bf16", "act": 2},
    "gelu_save_grad": {"bias": "bf16", "act": 5},
    "mul": {"act": 6, "colsum": True},
    "gelu_bwd": {"act": 3, "colsum": True},
    "relu_bwd": {"act": 4},
    "gelu_bwd_res": {"act": 3, "cin": "sep", "beta": 1.0},   # the launcher sends it to cfg 0
}
GEMM_BWD_ACTS = (3, 4, 6)


def gemm_case(gen, M, N, K, epi="plain", out_fp32=False, dev="cpu", bscale=None, aux_in=None, dtype=BF16):
    """operands and epilogue inputs of one case, and the keyword arguments of gemm_ref for it.
    With an activation b is scaled by K^-1/2 so that the pre-activations are O(1)."""
    e = GEMM_EPILOGUES[epi]
    act = e.get("act", 0)
    if bscale is None:
        bscale = K ** -0.5 if act else 1.0
    a, b = gemm_inputs(gen, M, N, K, dev=dev, bscale=bscale, dtype=dtype)
    g = torch.Generator().manual_seed(M + 3 * N + 5 * K + len(epi))
    odt = F32 if out_fp32 else BF16
    c = {"a": a, "b": b, "M": M, "N": N, "K": K, "epi": epi, "out_fp32": out_fp32, "act": act,
         "colsum": bool(e.get("colsum")), "cin": e.get("cin"),
         "alpha": e.get("alpha", 1.0), "beta": e.get("beta", 0.0), "bias": None, "Cin": None, "alpha_dev": None,
         "aux_in": None}
    if e.get("bias"):
        bias = torch.randn(N, generator=g)
        c["bias"] = (bias if e["bias"] == "f32" else bias.to(BF16)).to(dev)
    if e.get("cin"):
        c["Cin"] = torch.randn(M, N, generator=g).to(odt).to(dev)
    if e.get("alpha_dev") is not None:
        c["alpha_dev"] = torch.tensor([e["alpha_dev"]], dtype=F32, device=dev)
    if act in GEMM_BWD_ACTS:
        c["aux_in"] = gemm_aux_in(M, N, dev=dev).to(BF16 if dtype == BF16 else F32) if aux_in is None else aux_in
    return c


def gemm_ref_of(dtype, c, mutant=""):
    return gemm_ref(dtype, c["a"], c["b"], True, False, alpha=c["alpha"], alpha_dev=c["alpha_dev"], bias=c["bias"],
                    Cin=c["Cin"], beta=c["beta"], act=c["act"], aux_in=c["aux_in"], mutant=mutant)


# -- the kernels' shapes (gemm_bf16.hip header, rtdc_gemm_bf16)
GEMM_TILES = {0: (128, 128), 1: (256, 128), 2: (128, 256), 3: (256, 256), 4: (256, 64), 5: (64, 256),
              6: (256, 256), 7: (256, 192), 8: (256, 256), 9: (256, 192), 10: (256, 256), 11: (256, 128),
              12: (256, 256), 13: (256, 256)}
GEMM_LAYOUTS = ((True, True), (True, False), (False, False), (False, True))   # (a_kmajor, b_kmajor)
GEMM_KS = (64, 128, 192, 320)   # one K-tile, two, the peeled tails of cfg 12 / 13, five
# rows a lane adds serially into the fused column sums: 2 (qa) x TMQ pairs per column run in
# tile_epilogue_bf16; TMQ = SA / 16 with SA = 128 / WA and WA = the partial rows per row tile that
# rtdc_gemm_bf16 reduces (2 at 256 columns, 4 at 192 / 128)
GEMM_CS_ROWS = {6: 8, 8: 8, 10: 8, 12: 8, 13: 8, 7: 4, 9: 4, 11: 4}


def gemm_tile_shapes(cfg):
    """one axis ends in a tile of 8, the other in a tile that is 8 short"""
    BM, BN = GEMM_TILES[cfg]
    return [(BM + 8, 2 * BN - 8), (2 * BM - 8, BN + 8)]


def gemm_cfg_runs_as(cfg, a_k, b_k, out_fp32, K=128):
    """the configuration a forced tile_cfg runs as (the documented fall-backs of rtdc_gemm_bf16:
    cfg 13 is forward only, cfg 11 needs a K-major A and a bf16 output - both then run as cfg 6),
    or None where the launcher refuses (the persistent form needs two K-tiles)."""
    if cfg == 13 and not (a_k and b_k):
        cfg = 6
    if cfg == 11 and (out_fp32 or not a_k):
        cfg = 6
    if cfg in (8, 9) and K < 128:
        return None
    return cfg


def gemm_colsum_fallback_rows(M):
    """rows a wave of colsum_partial_kernel (norm.hip) adds serially: M / 64 blocks (1..256), 4 waves"""
    nblk = min(256, max(1, M // 64))
    return -(-(-(-M // nblk)) // 4)


GEMM_SPLITK_SHAPES = ((264, 264), (520, 392))
GEMM_SPLITK_KS = (2048, 1984)                    # 32 K-tiles: split; 31: never
GEMM_SPLITK_CFGS = (-1, 0, 6, 7, 10, 11, 12, 13)
GEMM_PERSIST_MN = (4392, 4160)                   # 18 x 17 (22) tiles, the last row and column partial
GEMM_PERSIST_KS = (128, 320)
GEMM_EPI_SHAPE = (520, 392, 192)
GEMM_EPI_CFGS = (0, 6, 7, 8, 10, 11, 12, 13)
# automatic routes under the default knobs: (name, M, N, K, layout, epilogue, fp32 out, the forced
# configuration it must equal bit for bit), worked out from pick_cfg / pick_cfg_few_rows
GEMM_ROUTES = [
    ("tail_split", 2048, 19200, 1024, (True, True), "plain", False, 12),       # 600 tiles: 2 rounds + 88 tiles
    ("tail_split_bias", 2048, 19200, 1024, (True, True), "bias_bf16", False, 12),
    ("few_rows_13", 2048, 4352, 512, (True, True), "plain", False, 13),        # 136 tiles: one partial round
    ("few_rows_0", 512, 512, 512, (True, True), "plain", False, 0),            # at most half a round, K <= 4096
    ("few_rows_7", 2048, 8448, 1024, (True, True), "plain", False, 7),         # 352 x 192-wide tiles
    ("few_rows_6", 2048, 6400, 512, (True, False), "plain", False, 6),         # dgrad layout, 200 tiles
    ("few_rows_11", 256, 384, 4160, (True, False), "plain", False, 11),        # K > 4096: 256x128 tiles
    ("long_k_12", 512, 512, 2048, (True, True), "plain", True, 12),            # K >= 2048 forward
]
GEMM_BATCH = (3, 2, 136, 136, 128)               # outer, inner, M, N, K on cfg 0
# grouped weight gradients dW[N, K] = dY[T, N]^T X[T, K]: (N, K) of each product
GEMM_GROUP_SMALL = ((1000, 2736), (512, 768), (264, 520))     # 56 tiles: under one round
GEMM_GROUP_BIG = ((4096, 4096), (1000, 2736), (2048, 1024))   # 332 tiles: the persistent grouped kernel
GEMM_GROUP_TOKENS = (192, 2048)
GEMM_F32_SHAPES = ((16, 512, 784), (16, 10, 512), (37, 70, 100), (37, 130, 100))   # (M, N, K)
GEMM_F32_EPIS = ("plain", "relu", "relu_bwd", "accumulate")


def gemm_cpu_cases():
    """(label, gen, M, N, K, epilogue, fp32 out) of every case of the table, for the twin condition.
    The multi-tile cases - persistent, automatic routes, grouped - are cut down to one 256x256
    tile (the twin's error depends on K, the epilogue and the generator, not on the tile count)."""
    out = []
    tiles = sorted({s for cfg in GEMM_TILES for s in gemm_tile_shapes(cfg)})
    for gen in GEMM_GENS:
        for f32 in (False, True):
            out += [("tile", gen, M, N, K, "plain", f32) for M, N in tiles for K in GEMM_KS]
            out += [("splitk", gen, M, N, K, e, f32) for M, N in GEMM_SPLITK_SHAPES for K in GEMM_SPLITK_KS
                    for e in ("plain", "accumulate")]
            out += [("persist", gen, 256, 256, K, "plain", f32) for K in GEMM_PERSIST_KS]
            out += [("epilogue", gen, *GEMM_EPI_SHAPE, e, f32) for e in GEMM_EPILOGUES]
        out += [("route", gen, 256, 256, K, e, f32) for _, _, _, K, _, e, f32, _ in GEMM_ROUTES]
        out += [("batch", gen, *GEMM_BATCH[2:], "plain", f32) for f32 in (False, True)]
        out += [("group", gen, 256, 256, T, e, True) for T in GEMM_GROUP_TOKENS for e in ("plain", "accumulate")]
        out += [("f32", gen, M, N, K, e, True) for M, N, K in GEMM_F32_SHAPES for e in GEMM_F32_EPIS]   # fp32 operands
    return out


def gemm_cpu_case(label, gen, M, N, K, epi, f32, dev="cpu"):
    """the case of one row of gemm_cpu_cases; act 6 reads the gelu' its act-5 twin stored"""
    aux = None
    if epi == "mul":
        aux = gemm_ref_of(F32, gemm_case(gen, M, N, K, "gelu_save_grad", f32, dev))["aux_out"].to(BF16)
    return gemm_case(gen, M, N, K, epi, f32, dev, aux_in=aux, dtype=F32 if label == "f32" else BF16)


def judge_gemm(J, op, shape, c, r, t, outs, cs_rows=None, aux_fp32=False):
    """C, aux_out and (where the call asks for them) the column sums of one call.  cs_rows: the
    fused arm's serial rows; None: the arm that reduces the stored C (judged against the kernel's
    own C - on the CPU against the twin's, rounded)."""
    K, C = c["K"], outs.get("C")
    if c["out_fp32"]:
        # (the clamp as in ulp_err: gelu'(-20) is 1e-258 in fp64 and 0 in fp32)
        J.rel(op, shape, "C", C, r["C"], t["C"], r["S_rel"].clamp_min(TINY), K)
    else:
        J.ulp(op, shape, "C", C, r["C"], t["C"], FLOOR_GEMM * r["S"])
    if r["aux_out"] is not None and (not outs or "aux_out" in outs):
        if aux_fp32:
            J.rel(op, shape, "aux", outs.get("aux_out"), r["aux_out"], t["aux_out"], r["S_aux"], K)
        else:
            J.ulp(op, shape, "aux", outs.get("aux_out"), r["aux_out"], t["aux_out"], FLOOR_GEMM * r["S_aux"])
    if c["colsum"]:
        if cs_rows is not None:
            J.rel(op, shape, "colsum", outs.get("colsum"), r["colsum"], t["colsum"], r["colsum_scale"], cs_rows)
        else:
            st = (C if C is not None else t["C"].to(F32 if c["out_fp32"] else BF16))
            J.rel(op, shape, "colsum*", outs.get("colsum"), st.double().sum(-2), st.float().sum(-2),
                  st.double().abs().sum(-2), gemm_colsum_fallback_rows(c["M"]))


# ------------------------------------------------------------------------------- CNN (ResNet path)
# cnn.hip, the implicit-GEMM convolution modes of rtdc_conv_gemm, conv3x3_wgrad_kernel and the
# conv_tile_stats / bnb_tile_stats epilogues of gemm_bf16.hip, under the first yardstick where the
# kernel accumulates in fp32 and rounds once (conv y, implicit dgrad, BatchNorm, pools), and under
# a per-element allowance where bf16 values are summed (dgrad through linear_dgrad + col2im).
# No reference here calls a convolution library: windows are explicit tap loops over a padded
# image and the products are matmuls, so every one runs in float64 on either device.
# * `conv_ref`: y / dx / dw and S, the sum of |terms| at the leaves;
# * `bn_ref`: forward (y, mean, var, running statistics) and backward (dx, dgamma, dbeta, dres);
#   the backward takes the ReLU mask as an input (an element within an fp32 rounding of the
#   boundary flips dbeta by a whole gradient value: the GPU tests pass `stored y > 0`);
# * `maxpool_ref` / `maxpool_bwd_ref` / `avgpool_ref`, and the index formulas of the kernels that
#   only move data (`im2col_ref`, `w_flip_t_ref`, `s2d_ref`, `stem_w_s2d_ref`, `stem_dw_ref`);
# * the case tables (CNN_*) are data shared by tests/test_ulp_cpu.py and tests/test_cnn_ulp_gpu.py;
#   every shape has H != W.
#
# BatchNorm y = x ka + (beta - mean ka) (+ res), ka = rstd gamma: x ka and mean ka cancel (the
# `offset` generator puts the channel mean at 8 standard deviations), and y lands near -res.
# Times S_y = |x ka| + (sum |x| / N) |ka| + |beta| + |res|: the leaves of the kernel's fma, the mean
# taken at its own leaves (it is a sum of N signed terms).
FLOOR_BN_Y = 2.0 ** -11
# BatchNorm dx = gr (g - dbeta / N - xhat dgamma / N), gr = gamma rstd, formed by the kernel as
# gr g + kB x + (kD - kB mean): g and the two channel means cancel, and so do kB x and kB mean.
# Times S_dx = |gr| (|g| + sum |g| / N + rstd (|x| + sum |x| / N) sum |g| rstd (|x| + sum |x| / N) / N):
# the leaves.  The smallest power of two at which the twin holds both as the CPU computes it and as the
# device does (the GPU tests compute theirs there, with the device's division and square root): at 2^-13
# the CPU's still passes (0.050 ulp), the device's does not (0.075 at 35 x 2056, planted), and at 2^-14
# the CPU's has left the ceiling too (0.10).  tests/test_ulp_cpu.py holds the CPU's half of that,
# tests/test_cnn_ulp_gpu.py::test_floor_bn_dx_on_the_device the device's.
FLOOR_BN_DX = 2.0 ** -12
# The pools take no floor (every element is judged in its own last place): max-pool backward adds at
# most K^2 bf16 values in fp32 - exact but for an exponent spread above 16 bits - and rounds once, the
# global average adds HW = 35 bf16 values the same way, and its backward is one product.

CONV_MUTANTS = ("pad_clamp", "khkw_swapped", "hw_swapped", "col2im_phase", "dw_last_row", "truncate", "addend_after")
BN_MUTANTS = ("biased_var", "eps", "mask_ge", "mask_pre_res", "dbeta_dropped", "dres_unmasked")
POOL_MUTANTS = ("last_argmax", "pad_zero", "bwd_window_dropped")
# terms a lane adds serially.  Tile statistics (conv_tile_stats): a lane adds its TM <= 4 rows, then
# the 16-lane tree, then WM <= 8 waves in order.  BatchNorm partial rows (bn_reduce_kernel): see
# bn_serial_rows.  Weight gradients: one MFMA accumulator takes every pixel of its split serially
# (gemm_bf16_kernel mode 2: K = the padded pixel count; conv3x3_wgrad_kernel: per x KP pixels), so
# R = the pixel count, as gemm's R = K.
CNN_STATS_ROWS = 4 + 8


def out_hw(H, W, KH, KW, stride, pad):
    return (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1


def _windows(x, KH, KW, stride, pad, fill=0.0, clamp=False):
    """[B, Ho, Wo, KH * KW, C] of an NHWC tensor: tap (kh, kw) of output pixel (ho, wo) is input
    pixel (ho s - p + kh, wo s - p + kw), `fill` outside the image (clamp: the border pixel)."""
    B, H, W, C = x.shape
    Ho, Wo = out_hw(H, W, KH, KW, stride, pad)
    if clamp:
        hi = torch.arange(-pad, H + pad, device=x.device).clamp(0, H - 1)
        wi = torch.arange(-pad, W + pad, device=x.device).clamp(0, W - 1)
        xp = x[:, hi][:, :, wi]
    else:
        xp = torch.full((B, H + 2 * pad, W + 2 * pad, C), fill, dtype=x.dtype, device=x.device)
        xp[:, pad:pad + H, pad:pad + W] = x
    taps = [xp[:, kh:kh + stride * (Ho - 1) + 1:stride, kw:kw + stride * (Wo - 1) + 1:stride]
            for kh in range(KH) for kw in range(KW)]
    return torch.stack(taps, 3)


def _col2im(dcols, B, H, W, C, KH, KW, stride, pad, phase=True):
    """gather form of col2im_kernel: dx[b, h, w] = sum over taps with (h + p - kh) % s == 0 of
    dcols[(b, (h + p - kh) / s, (w + p - kw) / s)][(kh, kw)]; returns the [T, B, H, W, C] terms
    (zero where a tap does not reach).  phase=False drops the `% s` test (a mutant)."""
    Ho, Wo = out_hw(H, W, KH, KW, stride, pad)
    dc = dcols.reshape(B, Ho, Wo, KH * KW, C)
    hh, ww = torch.arange(H, device=dcols.device), torch.arange(W, device=dcols.device)
    out = []
    for kh in range(KH):
        hs = hh + pad - kh
        okh = (hs >= 0) & (hs // stride < Ho) & ((hs % stride == 0) if phase else True)
        for kw in range(KW):
            ws = ww + pad - kw
            okw = (ws >= 0) & (ws // stride < Wo) & ((ws % stride == 0) if phase else True)
            v = dc[:, (hs // stride).clamp(0, Ho - 1)][:, :, (ws // stride).clamp(0, Wo - 1)][:, :, :, kh * KW + kw]
            out.append(v * (okh[:, None] & okw[None, :])[None, :, :, None].to(v.dtype))
    return torch.stack(out)


def conv_ref(dtype, x, w, stride, pad, dy=None, addend=None, mutant="", path="implicit", twin=False):
    """NHWC convolution x [B, H, W, C] (bf16) * w [Cout, C, KH, KW] (rounded to bf16 here, as the
    kernels' shadow is), no bias: y [B, Ho, Wo, Cout]; with dy also dw [Cout, C, KH, KW] and dx.
    S_* = the sum of |terms| at the leaves.  addend: the GradStash tensor, added to dx in fp32 ahead
    of the single rounding.  path="cols" (float64, no mutant): dx as linear_dgrad + col2im forms it -
    every column value is stored as bf16 and up to ceil(KH / s) ceil(KW / s) of them are added - with
    allow_dx, the per-element allowance counted from those roundings; twin=True applies them in
    `dtype`.  `mutant`: a deliberate error (CONV_MUTANTS)."""
    assert mutant == "" or mutant in CONV_MUTANTS
    B, H, W, C = x.shape
    Cout, _, KH, KW = w.shape
    Ho, Wo = out_hw(H, W, KH, KW, stride, pad)
    M, K = B * Ho * Wo, KH * KW * C
    xs = x.to(dtype)
    wb = w.to(BF16).to(dtype)
    if mutant == "khkw_swapped":
        wb = wb.transpose(2, 3)
    wm = wb.permute(0, 2, 3, 1).reshape(Cout, K)           # k = (kh KW + kw) C + c
    cols = _windows(xs, KH, KW, stride, pad, clamp=mutant == "pad_clamp").reshape(M, K)
    y = cols @ wm.T
    out = {"S_y": (cols.abs() @ wm.abs().T).view(B, Ho, Wo, Cout)}
    if mutant == "hw_swapped":
        y = y.view(B, Wo, Ho, Cout).transpose(1, 2).reshape(M, Cout)
    if mutant == "truncate":
        y = _truncate_bf16(y)
    out["y"] = y.view(B, Ho, Wo, Cout)
    if dy is None:
        return out
    g = dy.to(dtype).reshape(M, Cout)
    gw = g
    if mutant == "dw_last_row":
        gw = g.clone()
        gw[-1] = 0
    back = lambda m: m.view(Cout, KH, KW, C).permute(0, 3, 1, 2)
    out.update(dw=back(gw.T @ cols), S_dw=back(g.abs().T @ cols.abs()))
    dcols = g @ wm
    S_dc = g.abs() @ wm.abs()
    rounded = path == "cols" and twin
    terms = _col2im(_rb(dcols, rounded), B, H, W, C, KH, KW, stride, pad, phase=mutant != "col2im_phase")
    dx, S_dx = terms.sum(0), _col2im(S_dc, B, H, W, C, KH, KW, stride, pad).sum(0)
    if addend is not None:
        a = addend.to(dtype)
        S_dx = S_dx + a.abs()
        dx = _rb(dx, True) + a if mutant == "addend_after" else dx + a
    out.update(dx=_rb(dx, rounded), S_dx=S_dx)
    if path == "cols" and dtype == F64 and not twin and not mutant:
        # a column value is within F(Cout) S of its fp64 value before linear_dgrad stores it as
        # bf16; col2im adds the stored values (and the addend) in fp32 and rounds the sum once
        a_col = _stored(dcols, _f32_terms(Cout) * S_dc)
        A = _col2im(a_col, B, H, W, C, KH, KW, stride, pad)
        live = _col2im(torch.ones_like(dcols), B, H, W, C, KH, KW, stride, pad)
        out["allow_dx"] = _stored(dx, (A * live).sum(0) + _f32_terms(KH * KW + 1) * S_dx)
    return out


def bn_serial_rows(N, C, nblk):
    """terms a thread of bn_reduce_kernel adds serially (its share of a row-block), plus the row
    lanes and the partials a thread of the finalize adds in order"""
    cg = C // 8
    rl = 256 // min(256, cg)
    R = -(-N // nblk)
    return -(-R // rl) + rl + -(-nblk // 256)


def bn_ref(dtype, x, gamma, beta, eps, momentum, rm, rv, res=None, relu=False, mask=None, dy=None, training=True,
           mutant=""):
    """BatchNorm over the rows of x [N, C] (bf16; an NHWC tensor flattened), fp32 gamma / beta and
    running statistics, in the kernels' form: ka = rstd gamma, y = x ka + (beta - mean ka) (+ res),
    ReLU.  Returns y, mean, var, running_mean, running_var (unbiased, n / (n - 1)) and their scales;
    with dy the backward: g = dy where mask (given, or `y > 0` of this forward), dbeta = sum g,
    dgamma = sum g xhat, dx = gamma rstd (g - dbeta / N - xhat dgamma / N), dres = g.
    `mutant`: a deliberate error (BN_MUTANTS)."""
    assert mutant == "" or mutant in BN_MUTANTS
    N, C = x.shape
    xs, ga, be = x.to(dtype), gamma.to(dtype), beta.to(dtype)
    e = torch.tensor(_f32(1e-4 if mutant == "eps" else eps), dtype=dtype, device=x.device)
    mo = torch.tensor(_f32(momentum), dtype=dtype, device=x.device)
    out = {}
    if training:
        mean = xs.sum(0) / N
        m2 = ((xs - mean) ** 2).sum(0)
        var = m2 / N
        out.update(running_mean=(1 - mo) * rm.to(dtype) + mo * mean,
                   running_mean_scale=(1 - mo) * rm.to(dtype).abs() + mo * xs.abs().sum(0) / N,
                   running_var=(1 - mo) * rv.to(dtype) + mo * (var if mutant == "biased_var" else m2 / max(N - 1, 1)),
                   mean_scale=xs.abs().sum(0) / N)
        out["running_var_scale"] = (1 - mo) * rv.to(dtype).abs() + mo * m2 / max(N - 1, 1)
    else:
        mean, var = rm.to(dtype), rv.to(dtype)
    # the mean at its leaves: a batch mean is a sum of N signed terms, in error by fp32 roundings of
    # sum |x| / N however small it comes out itself
    am = out["mean_scale"] if training else mean.abs()
    rstd = 1.0 / torch.sqrt(var + e)
    ka = rstd * ga
    t0 = xs * ka + (be - mean * ka)
    t = t0 if res is None else t0 + res.to(dtype)
    y = t.clamp_min(0) if relu else t
    S_y = (xs * ka).abs() + am * ka.abs() + be.abs() + (0 if res is None else res.to(dtype).abs())
    out.update(y=y, mean=mean, var=var, rstd=rstd, S_y=S_y.expand_as(y))
    if dy is None:
        return out
    g = dy.to(dtype)
    if relu:
        if mutant == "mask_ge":
            mk = y >= 0
        elif mutant == "mask_pre_res":
            mk = t0 > 0
        else:
            mk = (y > 0) if mask is None else mask
        gm = torch.where(mk, g, torch.zeros_like(g))
    else:
        gm = g
    xhat = (xs - mean) * rstd
    dbeta, dgamma = gm.sum(0), (gm * xhat).sum(0)
    gr = ga * rstd
    dx = gr * (gm - (0 if mutant == "dbeta_dropped" else dbeta / N) - xhat * dgamma / N)
    # the leaves: dbeta and dgamma are themselves sums of N signed terms, taken with their |terms|
    sb, sg = gm.abs().sum(0), (gm * rstd).abs().mul(xs.abs() + am).sum(0)
    S_dx = gr.abs() * (gm.abs() + sb / N + rstd * (xs.abs() + am) * sg / N)
    out.update(dx=dx, S_dx=S_dx, dbeta=dbeta, dbeta_scale=sb, dgamma=dgamma, dgamma_scale=sg,
               dres=g if mutant == "dres_unmasked" else gm)
    return out


def tile_stats_ref(dtype, y, bm):
    """(mean, M2) of every bm-row tile of the stored y [M, C] as conv_tile_stats forms them, and the
    leaf terms its one-pass form sums: sum |v| / n for the mean, sum v^2 for M2 = Q - S mean"""
    M, C = y.shape
    v = y.to(dtype)
    nt = -(-M // bm)
    vp = torch.zeros(nt * bm, C, dtype=dtype, device=y.device)
    vp[:M] = v
    vp = vp.view(nt, bm, C)
    n = torch.tensor([min(bm, M - i * bm) for i in range(nt)], dtype=dtype, device=y.device)[:, None]
    live = (torch.arange(bm, device=y.device)[None, :, None] < n[:, :, None]).to(dtype)
    mean = vp.sum(1) / n
    return {"mean": mean, "m2": (((vp - mean[:, None]) * live) ** 2).sum(1), "mean_scale": vp.abs().sum(1) / n,
            "m2_scale": (vp * vp).sum(1)}


def first_max_tap(win, last=False):
    """index of the first (last: the mutant) maximum along the tap axis 3 of [B, Ho, Wo, T, C]"""
    T = win.shape[3]
    idx = torch.arange(T, device=win.device)[None, None, None, :, None].expand_as(win)
    hit = win == win.amax(3, keepdim=True)
    if last:
        return torch.where(hit, idx, torch.full_like(idx, -1)).amax(3)
    return torch.where(hit, idx, torch.full_like(idx, T)).amin(3)


def maxpool_ref(x, k, s, p, mutant=""):
    """max-pool of an NHWC bf16 tensor: y (the stored bits of the first maximum in (kh, kw) order,
    the sign of a zero included) and arg, its tap index kh K + kw (uint8); padding never competes"""
    assert mutant == "" or mutant in POOL_MUTANTS
    win = _windows(x.double(), k, k, s, p, fill=0.0 if mutant == "pad_zero" else -math.inf)
    arg = first_max_tap(win, last=mutant == "last_argmax")
    raw = _windows(x, k, k, s, p, fill=0.0)
    return {"y": raw.gather(3, arg[:, :, :, None]).squeeze(3), "arg": arg.to(torch.uint8)}


def maxpool_bwd_ref(dtype, dy, arg, H, W, k, s, p, mutant=""):
    """dx[b, h, w] = sum of dy over the windows whose argmax tap is (h, w): at most K^2 values (4 for
    3x3 / 2), one rounding.  S_dx the sum of their magnitudes."""
    B, Ho, Wo, C = dy.shape
    g = dy.to(dtype)
    if mutant == "bwd_window_dropped":
        g = g.clone()
        g[:, Ho - 1, Wo - 1] = 0
    hot = torch.zeros(B, Ho, Wo, k * k, C, dtype=dtype, device=dy.device)
    hot.scatter_(3, arg.long()[:, :, :, None], 1.0)
    cols = lambda v: (hot * v[:, :, :, None]).reshape(B * Ho * Wo, k * k * C)
    return {"dx": _col2im(cols(g), B, H, W, C, k, k, s, p).sum(0),
            "S_dx": _col2im(cols(dy.to(dtype).abs()), B, H, W, C, k, k, s, p).sum(0)}


def avgpool_ref(dtype, x, dy=None):
    """global average [B, H, W, C] -> [B, C] (the sum over HW, divided by HW) and its backward dy / HW"""
    B, C = x.shape[0], x.shape[-1]
    v = x.to(dtype).reshape(B, -1, C)
    HW = v.shape[1]
    out = {"y": v.sum(1) / HW, "S_y": v.abs().sum(1) / HW}
    if dy is not None:
        out["dx"] = (dy.to(dtype) / HW)[:, None, :].expand(B, HW, C).reshape(x.shape)
    return out


# -- kernels that only move data: the index formula each must match bit for bit
def im2col_ref(x, KH, KW, stride, pad, Kp, Mp):
    """cols [Mp, Kp]: k = (kh KW + kw) C + c, zero for padding taps, for k >= K and for rows M..Mp"""
    B, H, W, C = x.shape
    win = _windows(x, KH, KW, stride, pad)
    M, K = B * win.shape[1] * win.shape[2], KH * KW * C
    cols = torch.zeros(Mp, Kp, dtype=x.dtype, device=x.device)
    cols[:M, :K] = win.reshape(M, K)
    return cols


def w_flip_t_ref(wm, Cout, KH, KW, C):
    """out[c][(kh, kw, co)] = wm[co][(KH - 1 - kh, KW - 1 - kw, c)] (the stride-1 dgrad operand)"""
    return wm.view(Cout, KH, KW, C).flip(1, 2).permute(3, 1, 2, 0).reshape(C, KH * KW * Cout).contiguous()


def nhwc_bf16_ref(x):
    return x.permute(0, 2, 3, 1).to(BF16).contiguous()


def s2d_ref(x):
    """X'[b][i][j][(2 di + dj) 3 + c] = X[b][c][2 i + di][2 j + dj], channels 12..15 zero"""
    B, _, H, W = x.shape
    v = x.view(B, 3, H // 2, 2, W // 2, 2).permute(0, 2, 4, 3, 5, 1).reshape(B, H // 2, W // 2, 12)
    return torch.cat([v, torch.zeros_like(v[..., :4])], -1).to(BF16).contiguous()


def _stem_index():
    """for k = (a 4 + bb) 16 + q of the 4x4x16 space-to-depth weight: its (kh, kw, c) in the 7x7x3
    weight, or -1 (q >= 12, or kh / kw = 2 a + di - 1 / 2 bb + dj - 1 = -1)"""
    idx = torch.full((256,), -1, dtype=torch.int64)
    for k in range(256):
        a, bb, q = k >> 6, (k >> 4) & 3, k & 15
        if q < 12:
            di, dj, c = q // 6, (q // 3) & 1, q % 3
            kh, kw = 2 * a + di - 1, 2 * bb + dj - 1
            if kh >= 0 and kw >= 0:
                idx[k] = (kh * 7 + kw) * 3 + c
    return idx


def stem_w_s2d_ref(wm):
    """[Cout, 147] (kh, kw, c) -> [Cout, 256]"""
    idx = _stem_index().to(wm.device)
    out = wm[:, idx.clamp_min(0)]
    return torch.where(idx[None, :] >= 0, out, torch.zeros_like(out))


def stem_dw_ref(dwp):
    """[Cout, 256] -> [Cout, 147]: the inverse gather"""
    idx = _stem_index()
    inv = torch.empty(147, dtype=torch.int64)
    inv[idx[idx >= 0]] = torch.nonzero(idx >= 0)[:, 0]
    return dwp[:, inv.to(dwp.device)]


# -- inputs
CNN_GENS = ("randn", "offset")


def conv_inputs(gen, B, H, W, C, Cout, KH, KW, stride, pad, seed=0, dev="cpu", addend=False):
    """x, w, dy (and the GradStash addend).  offset: input channel 0 is the constant 4 and reaches
    every filter through its centre tap alone (never a padding tap) with weight 2, next to K - 9
    random products of variance 1 / K, so that an OUTPUT channel's mean is 8 x its standard deviation
    at every pixel, the border included (tests/test_ulp_cpu.py holds the ratio): what the fused
    statistics of the epilogue then see."""
    g = torch.Generator().manual_seed(97 * H + 31 * W + 7 * C + Cout + 3 * KH + stride + len(gen) + seed)
    K = KH * KW * C
    x = torch.randn(B, H, W, C, generator=g)
    w = torch.randn(Cout, C, KH, KW, generator=g) * K ** -0.5
    if gen == "offset":
        x[..., 0] = 4.0
        w[:, 0] = 0.0
        w[:, 0, KH // 2, KW // 2] = 2.0
    else:
        assert gen == "randn"
    Ho, Wo = out_hw(H, W, KH, KW, stride, pad)
    c = {"x": x.to(BF16), "w": w, "dy": torch.randn(B, Ho, Wo, Cout, generator=g).to(BF16),
         "addend": torch.randn(B, H, W, C, generator=g).to(BF16) if addend else None}
    return {k: v.to(dev) if torch.is_tensor(v) else v for k, v in c.items()}


def bn_inputs(gen, N, C, seed=0, dev="cpu", res=False):
    """x [N, C], gamma, beta, running statistics, dy (and a residual).  offset: channel mean = 8 x
    the channel's standard deviation.  planted: channel 0 constant (variance 0), channel 1 with
    gamma = 0, channel 2 at magnitude 2^-20."""
    g = torch.Generator().manual_seed(1013 * C + N + 5 * len(gen) + seed)
    sd = 0.5 + torch.rand(C, generator=g)
    x = torch.randn(N, C, generator=g) * sd
    gamma = 0.5 + torch.rand(C, generator=g)
    gamma[C // 2:] *= -1          # negative gammas too
    if gen == "offset":
        x += 8 * sd
    elif gen == "planted":
        x[:, 0] = 1.5
        gamma[1] = 0.0
        x[:, 2] *= 2.0 ** -20
    else:
        assert gen == "randn"
    c = {"x": x.to(BF16), "gamma": gamma, "beta": 0.3 * torch.randn(C, generator=g),
         "rm": 0.1 * torch.randn(C, generator=g), "rv": 0.5 + torch.rand(C, generator=g),
         "dy": torch.randn(N, C, generator=g).to(BF16),
         "res": torch.randn(N, C, generator=g).to(BF16) if res else None}
    return {k: v.to(dev) if torch.is_tensor(v) else v for k, v in c.items()}


def pool_inputs(gen, B, H, W, C, k, s, p, seed=0, dev="cpu"):
    """x [B, H, W, C] and dy.  planted: constant 2x2 and 3x3 patches (ties inside a window), +0 and
    -0 next to each other in an otherwise negative window, and an all-negative border ring (rows 0
    and H - 1, columns 0 and W - 1), where padding read as zero would win."""
    g = torch.Generator().manual_seed(131 * H + 17 * W + C + k + seed)
    x = torch.randn(B, H, W, C, generator=g)
    if gen == "planted":
        x[:, 0] = -x[:, 0].abs() - 0.5
        x[:, H - 1] = -x[:, H - 1].abs() - 0.5
        x[:, :, 0] = -x[:, :, 0].abs() - 0.5
        x[:, :, W - 1] = -x[:, :, W - 1].abs() - 0.5
        x[:, 1:2, 1:2] = -x[:, 1:2, 1:2].abs() - 0.5          # window (0, 0) of 3x3/2/1 is all negative
        x[:, 2:4, 2:4] = 3.0                                   # 2x2 tie
        x[:, H - 5:H - 2, W - 5:W - 2] = 2.5                   # 3x3 tie
        x[:, 4:7, 0:3] = -x[:, 4:7, 0:3].abs() - 0.5
        x[:, 5, 1, 0::2] = 0.0
        x[:, 5, 2, 0::2] = -0.0
        x[:, 5, 1, 1::2] = -0.0
        x[:, 5, 2, 1::2] = 0.0
    else:
        assert gen == "randn"
    Ho, Wo = out_hw(H, W, k, k, s, p)
    return {"x": x.to(BF16).to(dev), "dy": torch.randn(B, Ho, Wo, C, generator=g).to(BF16).to(dev)}


# -- the case tables.  Convolutions: (name, B, H, W, C, Cout, KH, stride, pad); every H != W
CNN_CONV_IMPLICIT = [
    ("c64", 1, 17, 19, 64, 64, 3, 1, 1),         # 323 pixels: two 256-row tiles, the last partial, M % 8 != 0
    ("c128", 1, 17, 19, 64, 128, 3, 1, 1),       # 128x128 tiles
    ("c192", 2, 9, 11, 128, 192, 3, 1, 1),       # partial second column tile, two k-tiles per tap, > 4 wgrad tiles
    ("s2", 2, 9, 11, 64, 128, 3, 2, 1),          # strided: dgrad through linear_dgrad + col2im
    ("p1x1s2", 2, 9, 11, 64, 128, 1, 2, 0),      # projection shortcut
    ("k5", 1, 9, 11, 64, 64, 5, 1, 2),           # 5x5: mode-2 weight gradient
    ("s2odd", 1, 10, 13, 64, 64, 3, 2, 1),       # stride 2, even / odd size
]
# 3x3 / 1 / 1 weight gradients on conv3x3_wgrad_kernel, B = 3: (name, H, W, C, Cout)
CNN_WGRAD3 = [
    ("img", 5, 7, 64, 64),        # the whole image in one partial chunk (35 of 64 pixels)
    ("rows3", 17, 19, 64, 64),    # 3 rows of 19 per chunk, 6 chunks per image, the last partial
    ("w33", 4, 33, 64, 128),      # one row of 33 of 64 pixels per chunk
    ("w64", 3, 64, 64, 64),       # one full row per chunk
    ("uneven", 23, 33, 128, 128),  # four tiles, 69 chunks over 64 splits: two chunks a block, the last one
]
CNN_WGRAD3_KP128 = [("w33x3", 5, 33, 64, 64), ("w40x3", 4, 40, 64, 64)]   # 99 and 120 of 128 pixels
# fused statistics (GM 3): 256-row tiles (323 rows: the last partial) and 128-row tiles (CNN_BN_BIG's rows)
CNN_CONV_STATS = [("st64", 1, 17, 19, 64, 64, 3, 1, 1), ("st128", 3, 31, 35, 64, 128, 3, 1, 1)]
CNN_WGRAD_SPLITK =("k5long", 2, 33, 35, 64, 64, 5, 1, 2)               # 2310 pixels: 37 k-tiles, pick_splitk splits
# BatchNorm: (N, C); N = 3 x 7 x 11 and others that are no multiple of 4 x the row lanes
CNN_BN = [(231, 64), (231, 192), (77, 512), (35, 2056)]
CNN_BN_BIG = (3 * 31 * 35, 128)     # 3255 rows: 26 tiles of 128 (S = 4 splits of 7, 7, 7, 5); default nblk = 6
CNN_BN_MANY = (3255, 192)           # _BN_LOADS = 1: 305 row-blocks of 11 rows, the last 9 empty
CNN_POOLS = [(2, 9, 12, 64, 3, 2, 1), (2, 10, 7, 64, 3, 2, 1), (2, 9, 12, 128, 3, 2, 1), (2, 10, 7, 128, 3, 2, 1),
             (2, 10, 12, 64, 2, 2, 0), (1, 9, 12, 128, 2, 2, 0)]
CNN_AVGPOOL = (3, 5, 7, 512)        # HW = 35
CNN_STEM_S2D = [(2, 12, 20), (1, 10, 36)]
CNN_STEM_COLS = [("small", 2, 10, 14), ("stem224", 1, 8, 224)]


def conv_case_id(c):
    return c[0]


# -- grid arithmetic of the launchers (mirrors, for the branch-coverage test)
def bn_blocks(N, C, loads=32):
    """_bn_blocks of ops/cnn.py"""
    return max(1, min(2048, (N * C) // (256 * 8 * loads)))


def bn_reduce_branches(N, C, nblk):
    """the paths of bn_reduce_kernel / bn_finalize_kernel / the apply kernels this launch takes"""
    cg = C // 8
    R = -(-N // nblk)
    out = set()
    grid = max(1, min(16384, -(-(N * cg) // 256)))
    out.add("apply_hoisted" if (grid * 256) % cg == 0 else "apply_generic")
    if 256 % min(256, cg) != 0:
        out.add("idle_lanes")
    if cg > 256:
        out.add("second_gbase")
    for b in range(nblk):
        n = max(0, min(N, (b + 1) * R) - b * R)
        if n == 0:
            out.add("empty_block")
        rl = 256 // min(256, cg)
        rows0 = len(range(0, n, rl))           # rows of lane 0
        if rows0 >= 4:
            out.add("unrolled")
        if rows0 % 4 or n % rl:
            out.add("remainder")
    if nblk > 256:
        out.add("finalize_wraps")
    return out


def bn_split(p_nblk, C, nblk, enabled=True):
    """(S, per) of the split merge of rtdc_bn_fwd, or None where the finalize runs alone"""
    cg = (C + 63) // 64
    S = min((512 + cg - 1) // cg, (p_nblk + 7) // 8, nblk)
    if S < 4 or not enabled:
        return None
    per = -(-p_nblk // S)
    return -(-p_nblk // per), per


def conv3_wgrad_plan(B, H, W, Cin, Cout, kp_env=64, ws_elems=1 << 40):
    """(KP, RC, cpi, S, per) of launch_conv3x3_wgrad, or None where it hands the shape back"""
    if Cin % 64 or Cout % 64 or W < 1 or W > 64 or H < 1:
        return None
    max_halo = {128: (4 * 768 - 128 * 8) // 8, 64: (3 * 768 - 64 * 8) // 8}
    KP, RC = 128, min(128 // W, H)
    if kp_env == 64 or RC * W * 4 < 3 * 128 or (RC + 2) * (W + 2) > max_halo[128]:
        KP, RC = 64, min(64 // W, H)
    if KP == 64 and (RC + 2) * (W + 2) > max_halo[64]:
        return None
    cpi = -(-H // RC)
    nchunks = B * cpi
    tiles = (Cout // 64) * (Cin // 64)
    if tiles > 4:
        return None
    S = max(1, min(256 // tiles, nchunks))
    slab = Cout * 9 * Cin
    if S > 1 and S * slab > ws_elems:
        S = max(1, ws_elems // slab)
    per = -(-nchunks // S)
    return KP, RC, cpi, -(-nchunks // per), per


def pick_splitk(M, N, K, tiles, ws_elems, slots=512, t_ktile_us=1.8):
    """pick_splitk of gemm_bf16.hip: the slab count of a mode-2 product [M, N] over K (padded) pixels"""
    ktiles = K // 64
    if tiles >= 200 or ktiles < 32:
        return 1
    slab_us = M * N * 8.0 / 4.0e6
    best, best_t = 1, 1e30
    for s in range(1, 1025):
        if ktiles // s < 8 or s * M * N > ws_elems:
            break
        waves = -(-tiles * s // slots)
        t = waves * -(-ktiles // s) * t_ktile_us + (s * slab_us if s > 1 else 0.0)
        if t < best_t - 1e-9:
            best, best_t = s, t
    return best


def judge_conv(J, op, shape, r, t, outs, names=("y", "dx", "dw"), pixels=0):
    """y and implicit-GEMM dx: Judge.ulp, k = 1, FLOOR_GEMM x S; dw: Judge.rel, R = the pixels"""
    for n in names:
        o = outs.get(n)
        if n == "dw":
            J.rel(op, shape, n, o, r[n], t[n], r["S_dw"].clamp_min(TINY), pixels)
        else:
            J.ulp(op, shape, n, o, r[n], t[n], FLOOR_GEMM * r["S_" + n])


def judge_bn(J, op, shape, r, t, outs, R, fwd=("y", "running_mean", "running_var"), bwd=()):
    for n in fwd + bwd:
        o = outs.get(n)
        if n == "y":
            J.ulp(op, shape, n, o, r[n], t[n], FLOOR_BN_Y * r["S_y"])
        elif n == "dx":
            J.ulp(op, shape, n, o, r[n], t[n], FLOOR_BN_DX * r["S_dx"])
        else:
            J.rel(op, shape, n, o, r[n], t[n], r[n + "_scale"].clamp_min(TINY), R)


# ------------------------------------------------------------------------------- optimizers, embedding, dropout
# optim.hip (adamw_kernel, adamw_bf16state_kernel's parameter, sgd_kernel) and the arithmetic of
# elementwise.hip (embedding, dropout, ReLU-dropout) under the first yardstick: every output is fp32
# (or one bf16 rounding of an fp32 value) and a short chain of fp32 operations per element.
# * `adamw_ref` / `sgd_ref`: ONE step written out in the kernels' order.  Every scalar argument is
#   rounded to fp32 first, as the launcher receives it (`bc1 = 1 - b1**step` and `bc2_sqrt` as
#   optim/fused.py computes them, in Python doubles, then rounded); what the kernel derives from
#   them (grad_scale x coef, 1 - lr wd, lr / bc1, 1 - b1 ...) is computed in `dtype`, so those
#   roundings are the kernel's error, not the reference's.  They return the new p and state and S,
#   the sum of |terms| of each: |p decay| + |update| for AdamW's p, |b1 m| + |(1 - b1) gr| for m, v
#   itself (nothing cancels); SGD is linear in its leaves p, g and buf, so its S is the same chain
#   over the absolute values.  `normal`: every intermediate is a normal number or exactly zero
#   (the twin asserts it on the CPU: no result depends on how a device treats denormals).
# * R, the fp32 roundings of the kernel's chain per output, counted from the statements of
#   adamw_kernel / sgd_kernel (quoted at OPTIM_R).
# * `optim_inputs`: p with one exact zero per aligned quad (there the new p is the update itself,
#   judged in its own last place), g = randn x exp(4 randn) with planted runs of exact zeros and of
#   +-2^-30 and +-2^-27, where eps = 1e-8 dominates AdamW's denominator.  A multi-step case keeps g
#   and takes m, v / buf from the kernel's previous launch: m then never cancels (b1 m and
#   (1 - b1) gr have one sign).  With a fresh gradient every step they cancel on some element of
#   100 k to 2^-16, and the update there - the whole of p where p = 0 - has that many fewer good
#   bits in ANY fp32 evaluation, the twin's included: an input condition, not a kernel property.
# * `embed_ref` / `embed_bwd_ref`, `dropout_keep` (the mask from ops/random.py's Philox twin),
#   `dropout_ref`, `relu_dropout_ref`.
ADAMW_MUTANTS = ("eps_inside", "coupled_wd", "decay_flag_ignored", "coef_dropped", "bc_step_off_by_one")
SGD_MUTANTS = ("nesterov_off", "first_dampened", "wd_after_momentum", "grad_scale_on_wd")
# `upd` of adamw_kernel, one definition for the scalar and the vector branch, and what precedes it:
#   gs = grad_scale * clip[1]                                  1
#   gr = gv * gs                                               1
#   me = fmaf(1.f - b1, gr, b1 * me)                           3   -> m: 5 with gs, gr
#   ve = fmaf(b2, ve, ((1.f - b2) * gr) * gr)                  4   -> v: 6 with gs, gr
#   denom = sqrtf(ve) / bc2_sqrt + eps                         3
#   decay = 1.f - lr * wd ; step_size = lr / bc1               3
#   pe = fmaf(pe, decay, -(step_size * me / denom))            3   -> p: 18
# `upd` of sgd_kernel:
#   gs ; d = fmaf(gs, gv, w * pe)                              3
#   b = fmaf(momentum, b, (1.f - dampening) * d)               3   -> buf: 6
#   d = fmaf(momentum, b, d) ; pe = fmaf(-lr, d, pe)           2   -> p: 8
# OPTIM_R_TORCH: the same chains in separate torch operations, every product and sum rounded
# (`_torch_update` of optim/fused.py, whose scalars are Python doubles rounded once by the operation).
OPTIM_R = {"adamw": {"p": 18, "m": 5, "v": 6}, "sgd": {"p": 8, "buf": 6}}
OPTIM_R_TORCH = {"adamw": {"p": 21, "m": 6, "v": 7}, "sgd": {"p": 12, "buf": 8}}
OPTIM_SGD_OPTIONS = [(0.0, 0.0, False, 0.0), (0.9, 0.0, False, 0.05), (0.9, 0.5, False, 0.0), (0.9, 0.0, True, 0.05)]
OPTIM_LR = 1e-3


def _normal(*xs) -> bool:
    return all(bool(((x == 0) | (x.abs() >= TINY)).all()) for x in xs if x is not None)


def _scalars(dtype, dev, *vals, f32=True):
    return [torch.tensor(_f32(v) if f32 else v, dtype=dtype, device=dev) for v in vals]


def adamw_ref(dtype, p, g, m, v, decay_mask, lr, b1, b2, eps, wd, step, grad_scale, coef=None, mutant="",
              f32_scalars=True):
    """one AdamW step; m / v may be bf16 (the bf16-state kernel widens what it stored); coef: the clip
    coefficient the kernel read (None: no clip pointer); f32_scalars=False leaves the scalars the doubles
    they are (the cross-check against torch.optim in float64)"""
    dev = p.device
    t = step + 1 if mutant == "bc_step_off_by_one" else step
    sd = dtype if f32_scalars else F64   # what is derived from the scalars: in the kernel's fp32, or in doubles
    lr_, b1_, b2_, eps_, wd_, gsc, cf = _scalars(sd, dev, lr, b1, b2, eps, wd, grad_scale,
                                                 1.0 if coef is None else coef, f32=f32_scalars)
    bc1, bc2s = _scalars(sd, dev, 1 - b1 ** t, math.sqrt(1 - b2 ** t), f32=f32_scalars)
    one = torch.ones((), dtype=sd, device=dev)
    gs = gsc if mutant == "coef_dropped" else gsc * cf
    b1_, b2_, eps_, wd_, bc2s, gs, dk, c1, c2, ss, one = (x.to(dtype) for x in (
        b1_, b2_, eps_, wd_, bc2s, gs, one - lr_ * wd_, one - b1_, one - b2_, lr_ / bc1, one))
    p_, g_, m_, v_ = (x.to(dtype) for x in (p, g, m, v))
    mask = torch.ones_like(decay_mask, dtype=torch.bool) if mutant == "decay_flag_ignored" else decay_mask.bool()
    gr = g_ * gs
    if mutant == "coupled_wd":   # torch.optim.Adam's L2 term instead of the decoupled decay
        gr = gr + torch.where(mask, wd_ * p_, torch.zeros_like(p_))
        decay = one.expand_as(p_)
    else:
        decay = torch.where(mask, dk, one)
    pd = p_ * decay
    a, b = b1_ * m_, c1 * gr
    mn = a + b
    c, d1 = b2_ * v_, c2 * gr
    d = d1 * gr
    vn = c + d
    rt = vn.sqrt()
    q = rt / bc2s
    denom = (rt + eps_) / bc2s if mutant == "eps_inside" else q + eps_
    num = ss * mn
    upd = num / denom
    pn = pd - upd
    return {"p": pn, "m": mn, "v": vn, "S_p": pd.abs() + upd.abs(), "S_m": a.abs() + b.abs(), "S_v": vn,
            "normal": _normal(gr, pd, a, b, mn, c, d1, d, vn, rt, q, denom, num, upd, pn)}


def sgd_ref(dtype, p, g, buf, decay_mask, lr, momentum, dampening, wd, nesterov, first, grad_scale, coef=None,
            mutant="", f32_scalars=True):
    """one SGD step (the comment above sgd_kernel); buf is None and stays None when momentum == 0"""
    dev = p.device
    sd = dtype if f32_scalars else F64
    lr_, mom, damp, wd_, gsc, cf = _scalars(sd, dev, lr, momentum, dampening, wd, grad_scale,
                                            1.0 if coef is None else coef, f32=f32_scalars)
    one = torch.ones((), dtype=sd, device=dev)
    lr_, mom, wd_, gs, undamp = (x.to(dtype) for x in (lr_, mom, wd_, gsc * cf, one - damp))
    p_, g_ = p.to(dtype), g.to(dtype)
    w = torch.where(decay_mask.bool(), wd_, torch.zeros((), dtype=dtype, device=dev))
    d0 = g_ * gs
    wp = w * p_ * gs if mutant == "grad_scale_on_wd" else w * p_
    seen = [d0, wp]

    def chain(d0, wp, b0):
        late = mutant == "wd_after_momentum"
        d = d0 if late else d0 + wp
        b = None
        if momentum != 0:
            if first:
                b = undamp * d if mutant == "first_dampened" else d
            else:
                x, y = mom * b0, undamp * d
                b = x + y
                seen.extend((x, y))
            if nesterov and mutant != "nesterov_off":
                z = mom * b
                seen.append(z)
                d = d + z
            else:
                d = b
            seen.append(b)
        if late:
            d = d + wp
        e = lr_ * d
        seen.extend((d, e))
        return b, e

    b0 = None if (momentum == 0 or first) else buf.to(dtype)
    bn, e = chain(d0, wp, b0)
    values = list(seen)
    bS, eS = chain(d0.abs(), wp.abs(), None if b0 is None else b0.abs())
    pn = p_ - e
    return {"p": pn, "buf": bn, "S_p": p_.abs() + eS, "S_buf": bS, "normal": _normal(pn, *values)}


def optim_planted(n, dev="cpu"):
    """(zeros, 2^-30, 2^-27) masks of the planted gradient runs: five elements each in every 97 (a
    prime period, so the runs meet every alignment and every chunk of a table)"""
    r = torch.arange(n, device=dev) % 97
    return r < 5, (r >= 30) & (r < 35), (r >= 60) & (r < 65)


def optim_inputs(n, seed=0, state=None, dev="cpu"):
    """p, g (fp32) and the state: zeros (first step) or `state`, the kernel's own previous output
    ({"m", "v"} or {"buf"}), taken as it is"""
    gen = torch.Generator().manual_seed(1000 + seed)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * torch.exp(4 * torch.randn(n, generator=gen))
    i = torch.arange(n)
    p[(i & 3) == ((i >> 2) & 3)] = 0.0   # one exact zero per aligned quad, on every lane in turn
    sign = torch.where((i & 1) == 0, 1.0, -1.0)
    z, s30, s27 = optim_planted(n)
    g[z] = 0.0
    g[s30] = sign[s30] * 2.0 ** -30
    g[s27] = sign[s27] * 2.0 ** -27
    c = {"p": p.to(dev), "g": g.to(dev)}
    for k in ("m", "v", "buf"):
        c[k] = torch.zeros(n, device=dev) if state is None or k not in state else state[k]
    return c


OPTIM_LENS = (1, 3, 4, 5, 7, 63, 64, 65, 1027)


def optim_table_rows():
    """the chunk table of tests/test_optim_ulp_gpu.py as [(start, len, sstart, decay)], and the elements it
    spans: aligned starts, odd-offset pieces, the compact state layout, a full chunk and one of 16384 - 3,
    mixed decay flags, gaps between the chunks"""
    rows, at = [], 0

    def add(s, ln, so):
        rows.append((s, ln, so, (len(rows) * 5 // 3) % 2))

    for ln in OPTIM_LENS:
        add(at, ln, at)
        at += (ln + 63) // 64 * 64
    for off in (1, 2, 3, 5, 6, 7):   # what chunk_table_splits emits: a piece that starts anywhere
        for ln in (1, 3, 4, 5, 64, 1027 - off):
            add(at + off, ln, at + off)
            at += 1152
    # the state of these lives elsewhere (ZeRO-1: shards back to back); (20000, 1922): `vec` false through
    # sstart alone; (24002, 2180): through start alone
    for s, ln, so in ((4096, 1027, 0), (8192 + 64, 65, 1088), (12288, 7, 1216), (16384, 640, 1280),
                      (20000, 256, 1922), (24002, 256, 2180)):
        add(at + s, ln, at + so)
    at += 24320
    add(at, 16384, at)
    at += 16384 + 64
    add(at, 16384 - 3, at)
    return rows, at + 16384


def optim_many_rows():
    """5000 chunks: more than the 4096 blocks the grid is capped at"""
    lens = [8, 5, 64, 3]
    return [(64 * i, lens[i % 4], 64 * i, int(i % 3 == 0)) for i in range(5000)], 64 * 5000


def optim_rows_index(rows, n_p, n_s):
    """(flat p / g / shadow indices, state indices, decay flag) of every element of the table, in table
    order; checks first that the chunks lie inside the buffers and do not overlap"""
    pi, si, dm = [], [], []
    for s, ln, so, d in rows:
        assert ln > 0 and 0 <= s and s + ln <= n_p and 0 <= so and so + ln <= n_s, (s, ln, so)
        pi.append(torch.arange(s, s + ln))
        si.append(torch.arange(so, so + ln))
        dm.append(torch.full((ln,), bool(d)))
    pi, si, dm = torch.cat(pi), torch.cat(si), torch.cat(dm)
    assert pi.unique().numel() == pi.numel() and si.unique().numel() == si.numel()
    return pi, si, dm


OPTIM_CLASS_SHAPES = [(64, 33), (7,), (1027,), (3, 5, 9), (16384 + 5,)]
OPTIM_CLASS_MAX_NORM = 0.5


def optim_class_inputs(seed=0):
    """flat p and g for the parameters of OPTIM_CLASS_SHAPES (the FusedAdamW / FusedSGD tests): p is
    optim_inputs', g is randn x exp(1.5 randn) with only the zero runs planted.  Not optim_inputs' g: with
    max_grad_norm = 0.5 the clip coefficient is max_norm / |g|, and exp(4 randn) puts the norm near 1e8, so
    the 2^-30 run times a coefficient of 5e-9 squares to 2^-115 and (1 - b2) times that is a denormal - the
    twin condition (every intermediate normal or zero) cannot hold.  Here the norm is about 1e3 and every
    gr^2 stays above 1e-30; tests/test_ulp_cpu.py holds the twin conditions on these inputs too."""
    total = sum(math.prod(s) for s in OPTIM_CLASS_SHAPES)
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(total, generator=gen) * torch.exp(1.5 * torch.randn(total, generator=gen))
    g[optim_planted(total)[0]] = 0.0
    return {"p": optim_inputs(total, seed)["p"], "g": g}


def optim_class_grad_factor(k):
    """the gradient of step k is g times this: one sign on every step (see the head of this section)"""
    return 1.0 + 0.5 * k


def judge_adamw(J, shape, r, t, outs, names=("p", "m", "v"), R=OPTIM_R):
    """r, t: adamw_ref in float64 / float32 over the elements judged; R: OPTIM_R, counted from `upd` of
    adamw_kernel (OPTIM_R_TORCH for the CPU path)"""
    for n in names:
        J.rel("adamw", shape, n, outs.get(n), r[n], t[n], r["S_" + n].clamp_min(TINY), R["adamw"][n])


def judge_sgd(J, shape, r, t, outs, R=OPTIM_R):
    """R: OPTIM_R, counted from `upd` of sgd_kernel; no buffer without momentum"""
    for n in ("p", "buf"):
        if r[n] is not None:
            J.rel("sgd", shape, n, outs.get(n), r[n], t[n], r["S_" + n].clamp_min(TINY), R["sgd"][n])


# -- embedding
EMBED_WIDTHS = (8, 128, 520, 1024)   # 1 lane of 64 busy; 16; the column loop twice (8 lanes the second time); twice, full
EMBED_BT = ((1, 1), (3, 5), (2, 37))
EMBED_V = 50


def embed_inputs(B, T, D, seed=0, dev="cpu"):
    gen = torch.Generator().manual_seed(2000 + seed)
    idx = torch.randint(0, EMBED_V, (B, T), generator=gen)
    flat = idx.view(-1)
    flat[0] = EMBED_V - 1
    flat[-1] = 0 if flat.numel() > 1 else EMBED_V - 1
    wte = torch.randn(EMBED_V, D, generator=gen).to(BF16)
    wpe = torch.randn(T, D, generator=gen).to(BF16)
    return {"idx": idx.to(dev), "wte": wte.to(dev), "wpe": wpe.to(dev)}


def embed_ref(dtype, idx, wte, wpe, T):
    """out[t] = wte[idx[t]] + wpe[t % T] over the flattened tokens"""
    flat = idx.reshape(-1)
    out = wte.to(dtype)[flat]
    if wpe is not None:
        out = out + wpe.to(dtype)[torch.arange(flat.numel(), device=flat.device) % T]
    return out


def embed_bwd_inputs(D, distinct, seed=0, dev="cpu"):
    """B = 2, T = 64: ids from 7 values (runs of about 18 that cross the 4-token blocks), or all distinct;
    V = 160 rows, so most rows are used by no token"""
    B, T, V = 2, 64, 160
    gen = torch.Generator().manual_seed(3000 + seed)
    if distinct:
        idx = torch.randperm(V, generator=gen)[:B * T].view(B, T)
    else:
        idx = torch.tensor([3, 17, 18, 64, 100, 158, 159])[torch.randint(0, 7, (B, T), generator=gen)]
    dout = torch.randn(B, T, D, generator=gen).to(BF16)
    dwte0 = torch.randn(V, D, generator=gen)
    dwpe0 = torch.randn(T, D, generator=gen)
    return {"idx": idx.to(dev), "dout": dout.to(dev), "dwte0": dwte0.to(dev), "dwpe0": dwpe0.to(dev), "V": V}


def embed_bwd_ref(dtype, idx, dout, dwte0, dwpe0, acc_wte, acc_wpe):
    """dwte (+)= index_add of dout rows by token id, dwpe (+)= sum over the batch; S: the sum of |terms|,
    the prior content included; `used`: the rows some token uses; `run`: the longest run of one id"""
    B, T = idx.shape
    V, D = dwte0.shape
    flat = idx.reshape(-1)
    do = dout.to(dtype).reshape(B * T, D)
    zero = torch.zeros(V, D, dtype=dtype, device=dout.device)
    dwte, S_wte = zero.index_add(0, flat, do), zero.index_add(0, flat, do.abs())
    dwpe, S_wpe = do.view(B, T, D).sum(0), do.abs().view(B, T, D).sum(0)
    if acc_wte:
        dwte, S_wte = dwte + dwte0.to(dtype), S_wte + dwte0.to(dtype).abs()
    if acc_wpe:
        dwpe, S_wpe = dwpe + dwpe0.to(dtype), S_wpe + dwpe0.to(dtype).abs()
    count = torch.bincount(flat, minlength=V)
    return {"dwte": dwte, "dwpe": dwpe, "S_dwte": S_wte, "S_dwpe": S_wpe, "used": count > 0, "run": int(count.max())}


# -- dropout
DROPOUT_SIZES = (1, 3, 5, 1027, 8192 * 1024 + 5)   # the last: the grid is capped at 8192 blocks, a second sweep
_keep_words: dict = {}


def dropout_words(seed, counter, n):
    """the uint32 word of each of n elements: element 4 q + e takes word e of
    philox4x32(seed, 0, counter + q); cached (int64 tensor on the CPU)"""
    import numpy as np

    from ray_torch_distributed_checkpoint_amd.ops.random import philox4x32

    key = (seed, counter, n)
    if key not in _keep_words:
        q = np.arange((n + 3) // 4, dtype=np.uint64) + np.uint64(counter)
        _keep_words.clear()   # (one at a time: the large case holds 8.4 M words)
        _keep_words[key] = torch.from_numpy(philox4x32(seed, 0, q).reshape(-1)[:n].astype(np.int64))
    return _keep_words[key]


def dropout_keep(seed, counter, n, p):
    """keep = (r >> 8) * 2^-24 >= float32(p): both sides exact in float64"""
    return (dropout_words(seed, counter, n) >> 8).double() * 2.0 ** -24 >= _f32(p)


def dropout_ref(dtype, x, keep, p):
    """y = keep ? x / (1 - p) : 0, p the fp32 number the kernel holds (the kernel multiplies by 1.f / (1.f - p))"""
    one, p_ = _scalars(dtype, x.device, 1.0, p)
    xs = x.to(dtype)
    y = xs * (one / (one - p_)) if dtype == F32 else xs / (one - p_)
    return torch.where(keep, y, torch.zeros_like(y))


def relu_dropout_ref(dtype, h, keep, p, dy=None):
    """forward (dy None): h m; backward: dy m; m = (keep and h > 0) ? 1 / (1 - p) : 0, and 1 at p = 0"""
    one, p_ = _scalars(dtype, h.device, 1.0, p)
    scale = one / (one - p_) if p > 0 else one
    src = (h if dy is None else dy).to(dtype)
    return torch.where(keep & (h > 0), src * scale, torch.zeros_like(src))


# ------------------------------------------------------------------------------- reductions
# The stand-alone reduction kernels: colsum_partial_kernel, colsum_ws_kernel, colsum_wide_kernel and
# colsum_multi_kernel (norm.hip), gradnorm_partial / finalize / combine_kernel (optim.hip), xent_finalize_kernel
# and xent_alpha_kernel (xent.hip).  A reference here mirrors a kernel's PARTITION - which rows, columns, chunk
# elements and jobs land in which output - and not its summation order: in float64 it is the reference, in
# float32 the twin.  Two generators:
# * `ints`: non-zero integers small enough that every partial and total sum is exactly representable in the
#   kernel's accumulator (fp32: |x| <= 64 and rows x 64 < 2^24, the tables stop at 4160 rows; the fp64 grad-norm
#   sums: |x| <= 2^10, squares <= 2^20, 2^14 of them).  Any summation order is then exact, so a kernel must equal
#   the float64 reference bit for bit, and one dropped, duplicated or misplaced element changes the result
#   (no element is zero).
# * `offset`: randn + 1, judged with `Judge.rel` against the fp64 sum of |terms| with `allow_f32(twin, R)`, R the
#   terms a lane adds serially (the reduce_R_* helpers, each counted from the kernel named next to it).  The
#   grad-norm kernels sum in fp64: `Judge.rel64`, the same form with 2^-53 for 2^-24, against `math.fsum` of the
#   squares (the product of two fp32 numbers is exact in fp64), the twin being torch's float64 sum.
# tests/test_ulp_cpu.py holds the twin condition and the mutants, tests/test_reduce_ulp_gpu.py runs the kernels.
REDUCE_MUTANTS = ("drop_last_row", "no_min", "pad_read", "tail_dropped", "acc_ignored", "job_shift", "no_clamp",
                  "f32_acc")
REDUCE_GENS = ("ints", "offset")
TWIN_REL64_CEIL = 2.0 ** -47   # the fp64 twin: the same 2^6 roundings as TWIN_REL_CEIL allows in fp32

REDUCE_PARTIAL_MN = ((1, 1), (3, 8), (9, 8), (67, 4), (261, 4))   # (M, nblk): (3, 8) and (9, 8) leave empty blocks
REDUCE_PARTIAL_N = (8, 72, 100, 7, 512, 520, 1032)                # 100 and 7: the scalar arm
REDUCE_PARTIAL_PAD = (0, 8, 3)                                    # ld - N; 3 forces the scalar arm
REDUCE_WIDE_W = (1, 15, 16, 17, 191, 192, 193, 385, 4096)         # 16 waves, 16 * kWideU = 192 rows a step
REDUCE_WIDE_D = (1, 63, 64, 65, 200)
REDUCE_TWO_LAUNCH_W = (4097, 4160)                                # > kWideMaxRows: S = 64 stage-1 blocks of R = 65
REDUCE_KNOBS_OFF_W = (1, 17, 63, 64, 193)                         # RTDC_COLSUM_WIDE=0: S = 1, 1, 1, 2, 6
REDUCE_MULTI_5 = ((192, 65, 0), (1, 1, 1), (17, 64, 1), (4096, 200, 0), (3, 130, 1))   # (W, D, accumulate)
REDUCE_MULTI_32 = tuple((5, 8 + j, int(j % 2 == 1 or j == 31)) for j in range(32))
REDUCE_GRADNORM_LENS = (1, 2, 3, 4, 5, 1023, 1024, 1025, 4099, 16384)
REDUCE_FINALIZE_N = (0, 1, 1023, 1024, 1025, 5000)
REDUCE_GRAD_SCALES = (1.0, 0.125, 3.0)
REDUCE_WORLDS = (1, 2, 8)
REDUCE_XENT_M = (1, 1023, 1024, 1025, 3000)
REDUCE_XENT_FORMS = ("some_ignored", "none_ignored", "all_ignored", "fixed_n")


def reduce_rpb(M, nblk):
    """rows per block of launch_colsum_partial: rpb = (M + nblk - 1) / nblk"""
    return -(-M // nblk)


def reduce_R_partial(M, nblk):
    """colsum_partial_kernel: `for (r = r0 + wv; r < r1; r += 4)` - a lane adds every 4th row of its block"""
    return -(-reduce_rpb(M, nblk) // 4)


def reduce_R_wide(W):
    """colsum_wide_cols: wave wv adds rows wv, wv + 16, ... into one accumulator"""
    return -(-W // 16)


def reduce_ws_plan(W):
    """colsum_ws_reduce without the wide kernel -> (S, R): S = clamp(W / 32, 1, 64) stage-1 blocks of R rows"""
    S = min(64, max(1, W // 32))
    return S, -(-W // S)


def reduce_R_ws(W):
    """colsum_ws_kernel: the 4 waves stride the R rows of a block (`w = r0 + wv`, steps of 4); two stages
    (S > 1) add the S stage-1 rows the same way"""
    S, R = reduce_ws_plan(W)
    return -(-R // 4) + (-(-S // 4) if S > 1 else 0)


def reduce_R_gradnorm(ln):
    """gradnorm_partial_kernel: lane t takes elements (or quads) t, t + 256, ..."""
    return -(-ln // 256)


def reduce_R_finalize(n):
    """gradnorm_finalize_kernel / xent_finalize_kernel: `for (i = threadIdx.x; i < n; i += 1024)`"""
    return -(-n // 1024)


def allow_f64(t_rel: float, R: int) -> float:
    """`allow_f32` for a kernel that accumulates in fp64"""
    return max(16.0 * t_rel, (R + 16) * 2.0 ** -53)


def ulp_f32(v: float) -> float:
    """the spacing of fp32 numbers in the binade of the normal number v"""
    return 2.0 ** (math.frexp(abs(v))[1] - 1 - 23)


def _judge_rel64(self, op, shape, what, out, ref64, twin, scale, R):
    t = rel_err(twin, ref64, scale)
    self._note(op, shape, what, "rel64", None if out is None else rel_err(out, ref64, scale), t, allow_f64(t, R),
               TWIN_REL64_CEIL)


Judge.rel64 = _judge_rel64


def reduce_gen(gen, shape, seed, dtype=F32, dev="cpu", bound=64):
    """`ints`: integers in [-bound, -1] u [1, bound]; `offset`: randn + 1 (rounded to `dtype` once)"""
    g = torch.Generator().manual_seed(seed)
    if gen == "ints":
        v = torch.randint(1, bound + 1, shape, generator=g) * (2 * torch.randint(0, 2, shape, generator=g) - 1)
        return v.to(dtype).to(dev)
    assert gen == "offset"
    return (torch.randn(shape, generator=g, dtype=F64 if dtype == F64 else F32) + 1.0).to(dtype).to(dev)


def colsum_partial_ref(dtype, X, M, N, ld, nblk, mutant=""):
    """-> [nblk][N]: row x = the sum of rows [x rpb, min(M, (x + 1) rpb)) of X[:, :N]; a block past M is exactly
    0.  X is the 2-D view the kernel is given (its row stride is the kernel's ld; columns >= N are padding).  The
    `no_min` mutant reads the rows X holds past M, as the kernel would read what follows the matrix."""
    assert X.dim() == 2 and X.shape[0] >= M and X.shape[1] >= N and ld >= N
    rpb = reduce_rpb(M, nblk)
    rows = min(nblk * rpb, X.shape[0]) if mutant == "no_min" else M
    v = X[:rows, :N].to(dtype)
    if mutant == "drop_last_row":   # `r < r1 - 1`
        r = torch.arange(rows, device=X.device)
        v = v * (~((r % rpb == rpb - 1) | (r == M - 1))).to(dtype)[:, None]
    if mutant == "pad_read":        # the last column also takes the first padding column
        v = torch.cat([v[:, :N - 1], v[:, N - 1:] + X[:rows, N:N + 1].to(dtype)], 1)
    v = torch.cat([v, torch.zeros(nblk * rpb - rows, N, dtype=dtype, device=X.device)])
    return v.view(nblk, rpb, N).sum(1)


def colsum_rows_ref(dtype, ws, W, D, base=None, accumulate=False, mutant=""):
    """out[d] (+)= sum over the W rows of ws [W][D] (colsum_ws_kernel / colsum_wide_cols); `base` is what out
    held before the launch"""
    s = ws[:W, :D].to(dtype).sum(0)
    return s + base[:D].to(dtype) if accumulate and mutant != "acc_ignored" else s


def colsum_multi_ref(dtype, jobs, mutant=""):
    """jobs [(ws, W, D, base, accumulate)] -> the n outputs of one colsum_multi launch"""
    outs = [colsum_rows_ref(dtype, *j, mutant=mutant) for j in jobs]
    if mutant == "job_shift":   # job j's columns land in job j + 1's output (the rest keeps what it held)
        n, shifted = len(jobs), []
        for j, job in enumerate(jobs):
            prev, k = outs[j - 1], min(job[2], jobs[j - 1][2])
            keep = job[3][:job[2]].to(dtype).clone()
            keep[:k] = prev[:k]
            shifted.append(keep)
        return shifted if n > 1 else outs
    return outs


def gradnorm_chunks(lens=REDUCE_GRADNORM_LENS):
    """[(start, len)]: every length at start & 3 = 0, 1, 2, 3, gaps of 4 to 7 elements between the chunks;
    -> the table and the length of the gradient buffer"""
    rows, at = [], 0
    for ln in lens:
        for k in range(4):
            at = (at + 3) // 4 * 4 + 4 + k
            rows.append((at, ln))
            at += ln
    return rows, at + 5


def gradnorm_partial_ref(dtype, g, chunks, mutant=""):
    """partial[ci] = the sum of squares of chunk ci's elements, squared and added in `dtype` (float64: what the
    kernel does, the twin of `gradnorm_partial_exact`; float32: the `f32_acc` mutant)"""
    out = []
    for s, ln in chunks:
        if mutant == "tail_dropped" and s % 4 == 0:   # the vector path without `if (i < c.len)`
            ln -= ln % 4
        out.append(g[s:s + ln].to(dtype).square().sum())
    return torch.stack(out)


def gradnorm_partial_exact(g, chunks):
    """the correctly rounded sums (math.fsum of the exact fp64 squares), float64 on the CPU"""
    gl = g.double().cpu().tolist()
    return torch.tensor([math.fsum(x * x for x in gl[s:s + ln]) for s, ln in chunks], dtype=F64)


def fsum64(v):
    return math.fsum(v.double().cpu().tolist())


def clip_ref(total_sq, grad_scale, max_norm, total=None):
    """`write_clip` of optim.hip in its fp32 arithmetic -> (total_norm, coef) as Python floats holding fp32
    values: total = grad_scale * (float)sqrt(sum); c = max_norm / (total + 1e-6f); coef = c < 1 ? c : (c != c ? c
    : 1).  `total`: take the kernel's own total_norm in place of the first line."""
    f = lambda x: torch.tensor(x, dtype=F32)   # noqa: E731
    if total is None:
        total = f(grad_scale) * torch.tensor(total_sq, dtype=F64).sqrt().float()
    else:
        total = f(total)
    c = f(max_norm) / (total + f(1e-6))
    coef = c if bool(c < 1) else (c if bool(c != c) else f(1.0))
    return total.item(), coef.item()


def xent_finalize_ref(dtype, loss, ce, target, fixed_n, mutant=""):
    """out[0] = sum(loss) / n, out[1] = n, out[2] = sum(ce) / n (ce given); n = max(number of targets that are
    not IGNORE_INDEX, 1), or fixed_n without targets.  In float32 the quotient is the fp32 division the kernel
    performs; on `ints` its operands are exact, so it is the kernel's result bit for bit."""
    if target is None:
        n = torch.tensor(_f32(fixed_n), dtype=dtype, device=loss.device)
    else:
        n = (target != IGNORE_INDEX).to(dtype).sum()
        if mutant != "no_clamp":
            n = n.clamp_min(1.0)
    out = [loss.to(dtype).sum() / n, n]
    if ce is not None:
        out.append(ce.to(dtype).sum() / n)
    return torch.stack(out)


def xent_finalize_scale(loss, ce, n):
    """the fp64 sums of |terms| over the divisor, per output (out[1] is a count: exact)"""
    s = [loss.double().abs().sum() / n, torch.tensor(1.0, dtype=F64, device=loss.device)]
    if ce is not None:
        s.append(ce.double().abs().sum() / n)
    return torch.stack(s).clamp_min(TINY)


def xent_finalize_targets(M, form, seed=0, dev="cpu"):
    """int64 targets for REDUCE_XENT_FORMS (None for `fixed_n`): every third ignored (from row 1 on, so M = 1
    keeps its row), none, all"""
    if form == "fixed_n":
        return None
    t = torch.randint(0, 1000, (M,), generator=torch.Generator().manual_seed(seed))
    if form == "some_ignored":
        t[1::3] = IGNORE_INDEX
    elif form == "all_ignored":
        t[:] = IGNORE_INDEX
    return t.to(dev)


def reduce_partial_cases():
    """(M, nblk, N, ld) of the colsum_partial table"""
    return [(M, nblk, N, N + pad) for M, nblk in REDUCE_PARTIAL_MN for N in REDUCE_PARTIAL_N for pad in REDUCE_PARTIAL_PAD]


def reduce_partial_input(gen, dtype, M, N, ld, seed=0, dev="cpu", extra_rows=0, pad=float("nan")):
    """X [M + extra_rows][ld] with NaN (or `pad`) in the padding columns; the data of the extra rows is 1"""
    X = reduce_gen(gen, (M + extra_rows, ld), seed, dtype, dev)
    X[M:] = 1.0
    X[:, N:] = pad
    return X
