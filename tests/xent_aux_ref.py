"""Reference, floors and judging for the cross-entropy kernels with label smoothing e and z-loss z
(xent.hip, AUX instantiations).  It extends tests/ulp.py, which it imports and does not change:
the metric, the allowances (`allow_bf16`, `allow_f32`), `Judge` and the case generators
(`XENT_ARMS`, `xent_inputs`, `XENT_WAYS`, `XENT_WRAPPER`) are that file's.

Per row with a valid target t, over the real columns j < V:

    L        = lse - (1 - e) x_t - (e / V) sum_j x_j + z lse^2
    dL/dx_j  = (1 + 2 z lse) softmax_j - e / V - (1 - e) [j == t]

`xent_aux_ref` in float64 is the reference, in float32 the twin.  At e = z = 0 it returns
`ulp.xent_ref`'s tensors bit for bit (tests/test_xent_aux_cpu.py holds that).

Floors, by the rule of tests/ulp.py (the smallest power of two for which the fp32 twin stays at or
under 2^-4 ulp on every case):

* the target column: |grad_scale| * FLOOR_XENT_TARGET * max(1, |a|), a = 1 + 2 z lse - the element
  is grad_scale * (a p - u - (1 - e)), a residue of terms of size |a| and 1;
* off the target: the larger of ulp's row floor (FLOOR_XENT x the row maximum) and
  |grad_scale| * (e / V) * FLOOR_XENT_AUX_U.  An element a p_j - u cancels to nothing where
  p_j ~ 1 / V; the twin's own error there is that of x - lse at lse ~ 12, about 2^-20 u.

FLOOR_XENT_AUX_U, measured (`python -m tests.xent_aux_ref` prints this table): the worst twin error
of the gradient in bf16 ulps over all of XENT_ARMS, random and planted rows, grad_scale 1 and 1/7,
by (e, z) and candidate F:

    (e, z)          2^-10    2^-9     2^-8     2^-7     2^-6
    (0.1, 0)        0.167    0.115    0.0577   0.0298   0.0298
    (0.1, 1e-4)     0.17     0.126    0.0632   0.0316   0.0275
    (0.01, 1e-4)    0.215    0.108    0.0543   0.0388   0.0275
    (0.3, 1e-3)     0.149    0.0746   0.0433   0.0216   0.0211
    (0, 1e-4)       0.0397   0.0397   0.0397   0.0397   0.0397
    (0, 1e-2)       0.0294   0.0294   0.0294   0.0294   0.0294

2^-8 leaves the ceiling (0.0632 > 0.0625) and 2^-7 holds it (0.0388 at worst), so F = 2^-7.  With
e = 0 the term is absent and ulp's own floors hold the twin at 0.0397.
"""
from __future__ import annotations

import torch

from tests import ulp as U

FLOOR_XENT_AUX_U = 2.0 ** -7

# (e, z) of the twin condition; the GPU tests run the first three of XENT_AUX_GPU
XENT_AUX_TABLE = [(0.1, 0.0), (0.1, 1e-4), (0.01, 1e-4), (0.3, 1e-3), (0.0, 1e-4), (0.0, 1e-2)]
XENT_AUX_GPU = [(0.1, 0.0), (0.0, 1e-4), (0.1, 1e-4)]
XENT_AUX_MUTANTS = ("u_ld", "a_half", "hot_one", "ignored_u", "pad_sum")


def xent_aux_ref(dtype, logits, target, V, grad_scale=1.0, e=0.0, z=0.0, mutant=""):
    """per-row loss L, plain cross-entropy ce, logsumexp and gradient grad_scale * dL/dx of
    logits[:, :V], written as the formulas above; e, z and grad_scale are floats in the kernel
    (rounded to fp32 first, then taken in `dtype`).  `mutant`: a deliberate error
    (XENT_AUX_MUTANTS), for the sensitivity checks only."""
    assert mutant == "" or mutant in XENT_AUX_MUTANTS
    M, ld = logits.shape
    x = logits[:, :V].to(dtype)
    m = x.amax(1, keepdim=True)
    s = torch.exp(x - m).sum(1, keepdim=True)
    lse = m + torch.log(s)
    p = torch.exp(x - lse)
    valid = target != U.IGNORE_INDEX
    t = torch.where(valid, target, torch.zeros_like(target))
    hot = torch.zeros_like(p)
    hot.scatter_(1, t[:, None], 1.0)
    f = lambda v: torch.tensor(v, dtype=torch.float32, device=x.device).to(dtype)   # a float in the kernel
    gs, ef, zf = f(grad_scale), f(e), f(z)
    u = ef / (ld if mutant == "u_ld" else V)            # a true division, as the kernel's
    a = 1.0 + (1.0 if mutant == "a_half" else 2.0) * zf * lse
    keep = valid[:, None].to(dtype)
    grad = gs * (a * p - u - hot * (1.0 if mutant == "hot_one" else 1.0 - ef)) * keep
    if mutant == "ignored_u":
        grad = grad - gs * u * (1.0 - keep)
    xt = x.gather(1, t[:, None])
    xs = logits.to(dtype) if mutant == "pad_sum" else x
    sumx = xs.sum(1, keepdim=True)
    zero = torch.zeros_like(lse[:, 0])
    loss = (lse - (1.0 - ef) * xt - u * sumx + zf * lse * lse)[:, 0]
    tmask = torch.zeros_like(p, dtype=torch.bool)
    tmask.scatter_(1, t[:, None], True)
    return {"grad": grad, "loss": torch.where(valid, loss, zero), "ce": torch.where(valid, (lse - xt)[:, 0], zero),
            "lse": lse[:, 0], "lse_scale": (m.abs() + torch.log(s).abs())[:, 0],
            "loss_scale": (lse.abs() + (1.0 - ef) * xt.abs() + u * x.abs().sum(1, keepdim=True) + zf * lse * lse)[:, 0],
            "ce_scale": (lse.abs() + xt.abs())[:, 0], "a": a, "tmask": tmask & valid[:, None]}


def xent_aux_grad_floor(ref, V, grad_scale, e, u_floor=FLOOR_XENT_AUX_U):
    g = ref["grad"].double()
    gs = abs(U._f32(grad_scale))
    tgt = gs * U.FLOOR_XENT_TARGET * ref["a"].double().abs().clamp_min(1.0)
    off = torch.maximum(U.row_floor(g, U.FLOOR_XENT), torch.full_like(g[:, :1], gs * (U._f32(e) / V) * u_floor))
    return torch.where(ref["tmask"], tgt.expand_as(g), off.expand_as(g))


def xent_aux_refs(c, grad_scale, e, z):
    """(reference, twin) of one case: computed once and shared by the calls that judge it"""
    a = (c["logits"], c["target"], c["V"], grad_scale, e, z)
    return xent_aux_ref(U.F64, *a), xent_aux_ref(U.F32, *a)


def judge_xent_aux(J, op, shape, c, grad_scale, e, z, outs, threads=256, k=1, u_floor=FLOOR_XENT_AUX_U, refs=None):
    """as ulp.judge_xent, plus `ce`; a name missing from `outs` is judged for the twin alone;
    refs: `xent_aux_refs` of the same case, if the caller holds them"""
    V = c["V"]
    r, t = refs or xent_aux_refs(c, grad_scale, e, z)
    R = -(-c["logits"].shape[1] // threads)   # columns a thread adds serially
    g = outs.get("grad")
    J.ulp(op, shape, "grad", None if g is None else g[:, :V], r["grad"], t["grad"],
          xent_aux_grad_floor(r, V, grad_scale, e, u_floor), k)
    J.rel(op, shape, "loss", outs.get("loss"), r["loss"], t["loss"], r["loss_scale"], R)
    J.rel(op, shape, "ce", outs.get("ce"), r["ce"], t["ce"], r["ce_scale"], R)
    J.rel(op, shape, "lse", outs.get("lse"), r["lse"], t["lse"], r["lse_scale"], R)
    return r


def twin_table(candidates=(-10, -9, -8, -7, -6)):
    """{(e, z): [worst twin ulp error of the gradient per candidate exponent of F]} over XENT_ARMS,
    random and planted rows, grad_scale 1 and 1/7"""
    out = {}
    for e, z in XENT_AUX_TABLE:
        worst = [0.0] * len(candidates)
        for dt, V, ld, _ in U.XENT_ARMS:
            for planted in (False, True):
                c = U.xent_inputs(dt, V, ld, planted)
                for gs in (1.0, 1.0 / 7):
                    r = xent_aux_ref(U.F64, c["logits"], c["target"], V, gs, e, z)
                    t = xent_aux_ref(U.F32, c["logits"], c["target"], V, gs, e, z)
                    for i, x in enumerate(candidates):
                        worst[i] = max(worst[i], U.ulp_err(t["grad"], r["grad"],
                                                           xent_aux_grad_floor(r, V, gs, e, 2.0 ** x)))
        out[(e, z)] = worst
    return out


if __name__ == "__main__":
    cand = (-10, -9, -8, -7, -6)
    print("%-15s %s" % ("(e, z)", "".join("%-9s" % f"2^{x}" for x in cand)))
    for (e, z), w in twin_table(cand).items():
        print("%-15s %s" % (f"({e:g}, {z:g})", "".join("%-9.3g" % v for v in w)))
