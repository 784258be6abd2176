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
