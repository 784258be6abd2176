"""The fused optimizer kernels and the cast / fill kernels judged per element (GPU only).

The yardstick is the optimizer section of tests/ulp.py: `adamw_ref` / `sgd_ref` write ONE step out in the
kernels' order with every scalar rounded to fp32 as the launcher receives it; in float64 they are the
reference, in float32 the twin, both computed on the device over the elements of the chunk table.  An fp32
output is held to max(16 x the twin, (R + 16) 2^-24) of the sum of |terms| (R counted from `upd` of each
kernel: OPTIM_R), the bf16 shadow to `p.bfloat16()` of the same launch bit for bit, everything outside the
chunks - gaps, the 64 guard elements behind every buffer - to its initial bits.  A multi-step case restarts
p from the generator (its planted zeros are judged every step) and takes the state the kernel left behind.
The casts and the fill are exact.  Each judged output prints one ULP line, each test its WORST lines; those
of one run are kept in profiles/optim_ulp_worst.txt.

Arm -> the test that reaches it:

  adamw_kernel<false>: vector path, scalar tail (len & 3), len < 4, `vec` false through
  `start` (offsets 1 .. 7) and through `sstart` alone, `sstart != start`, 16 iterations per
  lane (a full chunk), decay flag 0 / 1, clip pointer null / set, grad_scale 1 / 1/8,
  steps 1, 2, 7, betas (0.5, 0.75) with eps 1e-3, planted zero / tiny gradients, p = 0       test_adamw_table
  the grid cap (5000 chunks on 4096 blocks: the chunk loop runs twice)                       test_adamw_many_chunks, test_sgd_many_chunks
  adamw_bf16state_kernel<false>: p and the shadow over the same table (its stored moments:
  tests/test_optim_state_bf16_gpu.py)                                                        test_adamw_bf16_state_p_and_shadow
  sgd_kernel<false>: momentum 0 (no buffer) / 0.9, dampening 0 / 0.5, nesterov, weight decay
  with the per-chunk flag, first 1 (the buffer is not read) then 0, clip, grad_scale         test_sgd_table
  the shadow store, 8-B and scalar, of all three kernels                                     every test above
  `skip` word 1 (nothing moves) and 0 (== no pointer), all three kernels                     test_skip_word
  a chunk cut at offsets 1, 2, 3 mod 4 == the uncut chunk bit for bit, AdamW and SGD         test_cut_invariance
  FusedAdamW / FusedSGD: the launch parameters the classes derive (bias corrections, first,
  decay flags from the chunk table, grad_scale, the clip coefficient), a gradless parameter  test_fused_adamw_class, test_fused_sgd_class
  f32_to_bf16_kernel / bf16_to_f32_kernel: 16-B path, tail loop, n < 4, the second sweep of
  the capped grid, special values, scale 1 / 1/8                                             test_f32_to_bf16, test_bf16_to_f32
  f32_to_bf16_t_kernel: both `& 3` fallbacks, partial tiles on both axes                     test_f32_to_bf16_t
  fill_f32_kernel: n < 4, tail, the second sweep; a misaligned pointer is refused            test_fill_f32

Not run: adamw_kernel<true>, adamw_bf16state_kernel<true> and sgd_kernel<true> (the device-table variants
`adamw_dev` / `sgd_dev`) - tests/test_optim_capturable_gpu.py holds them to the host path bit for bit at
every step, table ends included, so what is judged here carries over.
"""
import math

import pytest
import torch

from tests import ulp as U

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F64, F32, BF16 = U.F64, U.F32, U.BF16
NAN = float("nan")
PAD = 64   # untouched guard elements behind every buffer's used part
LR = U.OPTIM_LR
ADAMW = dict(b1=0.9, b2=0.999, eps=1e-8, wd=0.1)
WAYS = [(None, 1.0), (0.37, 1.0), (None, 0.125), (0.37, 0.125)]   # (clip coefficient, grad_scale)
SEED = 0x1234_5678_9ABC_DEF0


def _ext():
    from ray_torch_distributed_checkpoint_amd.ops._ext import gpu_ext

    return gpu_ext()


def _bits(t):
    return t.contiguous().view({F32: torch.int32, BF16: torch.int16}[t.dtype])


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _table(rows):
    """rows [(start, len, sstart, decay)] -> (int64 [n, 3] GPU tensor, n): the row encoding of
    FlatParamSpace.chunk_table (tests/test_optim_state_bf16_gpu.py `_table`)"""
    t = [(r[0], r[1] | (r[3] << 32), r[2]) for r in rows]
    return torch.tensor(t, dtype=torch.int64, device=DEV), len(t)


def _index(rows, n_p, n_s):
    """U.optim_rows_index (which checks that the chunks lie inside the buffers and do not overlap) on the device"""
    return tuple(x.to(DEV) for x in U.optim_rows_index(rows, n_p, n_s))


def _outside(idx, n):
    o = torch.ones(n, dtype=torch.bool, device=DEV)
    o[idx] = False
    return o


_big_rows, _many_rows = U.optim_table_rows, U.optim_many_rows


def _clip(coef):
    return None if coef is None else torch.tensor([2.0, coef], device=DEV)


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _state(n, si, dtype=F32, fill=0.0):
    """a state buffer: `fill` on the chunks, NaN everywhere else"""
    b = torch.full((n + PAD,), NAN, dtype=dtype, device=DEV)
    b[si] = fill
    return b


# ------------------------------------------------------------------------------- AdamW
def _adamw_case(J, label, rows, n, coef, gs, steps=(1, 2, 7), state_dtype=F32, seed=0, **hyper):
    h = {**ADAMW, **hyper}
    chunks, nc = _table(rows)
    pi, si, dm = _index(rows, n, n)
    out_p, out_s = _outside(pi, n + PAD), _outside(si, n + PAD)
    c = U.optim_inputs(n + PAD, seed, dev=DEV)
    p0, g = c["p"], c["g"]
    m, v = _state(n, si, state_dtype), _state(n, si, state_dtype)
    clip = _clip(coef)
    names = ("p", "m", "v") if state_dtype == F32 else ("p",)
    for step in steps:
        p, shadow = p0.clone(), torch.full((n + PAD,), NAN, dtype=BF16, device=DEV)
        m_in, v_in = m.clone(), v.clone()
        _ext().adamw(chunks, nc, p, g, m, v, shadow, LR, h["b1"], h["b2"], h["eps"], h["wd"], 1 - h["b1"] ** step,
                     math.sqrt(1 - h["b2"] ** step), gs, 0, _ptr(clip), SEED, step)
        a = (p0[pi], g[pi], m_in[si], v_in[si], dm, LR, h["b1"], h["b2"], h["eps"], h["wd"], step, gs, coef)
        r, t = U.adamw_ref(F64, *a), U.adamw_ref(F32, *a)
        U.judge_adamw(J, (label, step, coef, gs), r, t, {"p": p[pi], "m": m[si], "v": v[si]}, names)
        assert _same(shadow[pi], p[pi].bfloat16()), (label, step)
        assert _same(p[out_p], p0[out_p]) and _same(shadow[out_p], torch.full_like(shadow[out_p], NAN))
        assert _same(m[out_s], m_in[out_s]) and _same(v[out_s], v_in[out_s])
        if state_dtype == BF16:
            assert not m[si].float().isnan().any() and (v[si].float() >= 0).all()


@pytest.mark.parametrize("coef,gs", WAYS)
def test_adamw_table(coef, gs):
    J = U.Judge()
    rows, n = _big_rows()
    _adamw_case(J, "table", rows, n, coef, gs)
    if coef is None and gs == 1.0:
        _adamw_case(J, "betas", rows, n, coef, gs, b1=0.5, b2=0.75, eps=1e-3)
    J.check()


def test_adamw_many_chunks():
    J = U.Judge()
    rows, n = _many_rows()
    _adamw_case(J, "5000", rows, n, 0.37, 0.125, steps=(1, 2), seed=1)
    J.check()


def test_adamw_bf16_state_p_and_shadow():
    """the reference reads the bf16 moments the kernel stored; the stored moments themselves are judged by
    tests/test_optim_state_bf16_gpu.py"""
    J = U.Judge()
    rows, n = _big_rows()
    for coef, gs in WAYS:
        _adamw_case(J, "bf16state", rows, n, coef, gs, state_dtype=BF16, seed=2)
    J.check()


# ------------------------------------------------------------------------------- SGD
def _sgd_case(J, label, rows, n, opt, coef, gs, seed=3):
    mom, damp, nest, wd = opt
    chunks, nc = _table(rows)
    pi, si, dm = _index(rows, n, n)
    out_p, out_s = _outside(pi, n + PAD), _outside(si, n + PAD)
    c = U.optim_inputs(n + PAD, seed, dev=DEV)
    p0, g = c["p"], c["g"]
    buf = None if mom == 0 else _state(n, si, fill=NAN)   # first = 1 must not read it
    clip = _clip(coef)
    for first in (True, False):
        p, shadow = p0.clone(), torch.full((n + PAD,), NAN, dtype=BF16, device=DEV)
        b_in = None if buf is None else buf.clone()
        _ext().sgd(chunks, nc, p, g, buf, shadow, LR, mom, damp, wd, nest, first, gs, 0, _ptr(clip))
        a = (p0[pi], g[pi], None if buf is None else b_in[si], dm, LR, mom, damp, wd, nest, first, gs, coef)
        r, t = U.sgd_ref(F64, *a), U.sgd_ref(F32, *a)
        U.judge_sgd(J, (label, opt, first, coef, gs), r, t, {"p": p[pi], "buf": None if buf is None else buf[si]})
        assert _same(shadow[pi], p[pi].bfloat16()), (label, opt, first)
        assert _same(p[out_p], p0[out_p]) and _same(shadow[out_p], torch.full_like(shadow[out_p], NAN))
        assert buf is None or _same(buf[out_s], b_in[out_s])


@pytest.mark.parametrize("opt", U.OPTIM_SGD_OPTIONS, ids=["plain", "momentum_wd", "dampening", "nesterov_wd"])
def test_sgd_table(opt):
    J = U.Judge()
    rows, n = _big_rows()
    for coef, gs in WAYS:
        _sgd_case(J, "table", rows, n, opt, coef, gs)
    J.check()


def test_sgd_many_chunks():
    J = U.Judge()
    rows, n = _many_rows()
    _sgd_case(J, "5000", rows, n, (0.9, 0.0, True, 0.05), 0.37, 0.125, seed=4)
    J.check()


# ------------------------------------------------------------------------------- skip, cuts
def _generic(n, seed):
    """buffers of generic values (nothing exactly representable in fewer bits)"""
    gen = torch.Generator().manual_seed(seed)
    r = lambda: torch.randn(n + PAD, generator=gen)   # noqa: E731
    return {"p": r().to(DEV), "g": r().to(DEV), "m": (0.1 * r()).to(DEV), "v": (0.1 * r()).square().to(DEV),
            "buf": r().to(DEV)}


def _launch(kind, rows, c, skip=0):
    """one launch of `kind` over clones of the buffers c; -> every buffer it may write"""
    chunks, nc = _table(rows)
    clip = _clip(0.37)
    p, sh = c["p"].clone(), torch.full_like(c["p"], NAN, dtype=BF16)
    if kind == "sgd":
        buf = c["buf"].clone()
        _ext().sgd(chunks, nc, p, c["g"], buf, sh, LR, 0.9, 0.0, 0.05, True, False, 0.125, skip, _ptr(clip))
        return {"p": p, "buf": buf, "shadow": sh}
    m, v = c["m"].clone(), c["v"].clone()
    if kind == "adamw_bf16":
        m, v = m.bfloat16(), v.bfloat16()
    _ext().adamw(chunks, nc, p, c["g"], m, v, sh, LR, 0.9, 0.999, 1e-8, 0.1, 1 - 0.9 ** 3, math.sqrt(1 - 0.999 ** 3),
                 0.125, skip, _ptr(clip), SEED, 3)
    return {"p": p, "m": m, "v": v, "shadow": sh}


@pytest.mark.parametrize("kind", ["adamw", "adamw_bf16", "sgd"])
def test_skip_word(kind):
    """the communicator health word: set, no bit of p, the state or the shadow moves; clear, the launch is
    the launch without a pointer"""
    rows, n = _big_rows()
    _index(rows, n, n)
    c = _generic(n, 5)
    word = torch.ones(1, dtype=torch.int32, device=DEV)
    before = {"p": c["p"], "m": c["m"], "v": c["v"], "buf": c["buf"], "shadow": torch.full_like(c["p"], NAN, dtype=BF16)}
    if kind == "adamw_bf16":
        before["m"], before["v"] = c["m"].bfloat16(), c["v"].bfloat16()
    for k, t in _launch(kind, rows, c, word.data_ptr()).items():
        assert _same(t, before[k]), k
    word.zero_()
    plain, cleared = _launch(kind, rows, c), _launch(kind, rows, c, word.data_ptr())
    assert not _same(plain["p"], c["p"])
    for k in plain:
        assert _same(plain[k], cleared[k]), k


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_cut_invariance(kind):
    """64-aligned chunks, and the same elements cut at offsets 1, 2 and 3 mod 4 (`sstart` moved alike): the
    first piece ends on the vector path's scalar tail, the second runs the scalar path throughout.  p, the
    state and the shadow are the uncut launch's bit for bit."""
    whole = [(0, 1027, 0, 1), (1088, 65, 1088, 0), (1216, 7, 1216, 1), (1280, 640, 1280, 1), (2048, 16384, 2048, 0),
             (18432, 16384 - 3, 18432, 1)]
    n = 18432 + 16384
    _index(whole, n, n)
    c = _generic(n, 6)
    base = _launch(kind, whole, c)
    assert not _same(base["p"], c["p"])
    for r in (1, 2, 3):
        cut = []
        for s, ln, so, d in whole:
            at = r if ln <= 8 else r + 4 * (ln // 8)
            cut += [(s, at, so, d), (s + at, ln - at, so + at, d)]
        _index(cut, n, n)
        got = _launch(kind, cut, c)
        for k in base:
            assert _same(got[k], base[k]), (r, k, int((_bits(got[k]) != _bits(base[k])).sum()))


# ------------------------------------------------------------------------------- the optimizer classes
SHAPES = U.OPTIM_CLASS_SHAPES
NO_GRAD = 3   # this parameter never receives a gradient


def _class_params(seed):
    """parameters and gradients of U.optim_class_inputs (why its gradients are tamer than optim_inputs': there)"""
    c = U.optim_class_inputs(seed)
    ps, gs, at = [], [], 0
    for s in SHAPES:
        k = math.prod(s)
        ps.append(torch.nn.Parameter(c["p"][at:at + k].view(s).clone().to(DEV)))
        gs.append(c["g"][at:at + k].view(s).to(DEV))
        at += k
    return ps, gs


def _class_steps(J, kind, opt, ps, grads, ref_of, grad_scale=1.0):
    """three steps; each judged from the buffers read before and after it"""
    sp = opt._ensure_space()
    sp.grad_scale = grad_scale
    live = [p for i, p in enumerate(ps) if i != NO_GRAD]
    for k in range(3):
        for i, (p, g) in enumerate(zip(ps, grads)):
            if i != NO_GRAD:
                p.grad = g * U.optim_class_grad_factor(k)   # one sign on every step: exp_avg never cancels (tests/ulp.py)
        before = {"p": sp.data.clone(), "shadow": sp.shadow.clone(), **{n: b.clone() for n, b in opt._bufs.items()}}
        opt.step()
        coef = float(opt._clip_ws["out"][1]) if opt.max_grad_norm else None
        assert coef is None or 0.0 < coef < 1.0
        wd = opt.param_groups[0]["weight_decay"]
        chunks, nc = sp.chunk_table(live, [wd != 0.0] * len(live))
        rows = [(s, ln, so, int(d)) for s, ln, d, so in opt._rows(chunks, nc)]
        pi, si, dm = _index(rows, sp.data.numel(), sp.state_numel)
        r, t, outs = ref_of(before, sp.grad, pi, si, dm, k, grad_scale, coef)
        (U.judge_adamw if kind == "adamw" else U.judge_sgd)(J, (kind, k + 1, coef, grad_scale), r, t, outs(pi, si))
        assert _same(sp.shadow[pi], sp.data[pi].bfloat16())
        out_p, out_s = _outside(pi, sp.data.numel()), _outside(si, sp.state_numel)
        assert _same(sp.data[out_p], before["p"][out_p])   # the gradless parameter and the padding
        assert _same(sp.shadow[out_p], before["shadow"][out_p])
        for n, b in opt._bufs.items():
            assert _same(b[out_s], before[n][out_s]), n
        seg = sp.segment_of(ps[NO_GRAD])
        assert bool(out_p[seg.offset:seg.offset + seg.numel].all())
        opt.zero_grad()


@pytest.mark.parametrize("wd,max_norm,grad_scale", [(0.0, None, 1.0), (0.1, None, 1.0), (0.0, 0.5, 1.0), (0.1, 0.5, 1.0),
                                                    (0.1, 0.5, 0.125)])
def test_fused_adamw_class(wd, max_norm, grad_scale):
    from ray_torch_distributed_checkpoint_amd.optim import FusedAdamW

    J = U.Judge()
    ps, grads = _class_params(7)
    opt = FusedAdamW(ps, lr=LR, weight_decay=wd, max_grad_norm=max_norm)

    def ref_of(before, g, pi, si, dm, k, gs, coef):
        a = (before["p"][pi], g[pi], before["exp_avg"][si], before["exp_avg_sq"][si], dm, LR, 0.9, 0.999, 1e-8, wd,
             k + 1, gs, coef)
        bufs = opt._bufs
        return (U.adamw_ref(F64, *a), U.adamw_ref(F32, *a),
                lambda pi, si: {"p": opt.flat_space.data[pi], "m": bufs["exp_avg"][si], "v": bufs["exp_avg_sq"][si]})

    _class_steps(J, "adamw", opt, ps, grads, ref_of, grad_scale)
    J.check()


@pytest.mark.parametrize("opts,max_norm,grad_scale", [(o, None, 1.0) for o in U.OPTIM_SGD_OPTIONS] +
                         [(U.OPTIM_SGD_OPTIONS[3], 0.5, 1.0), (U.OPTIM_SGD_OPTIONS[3], 0.5, 0.125)])
def test_fused_sgd_class(opts, max_norm, grad_scale):
    from ray_torch_distributed_checkpoint_amd.optim import FusedSGD

    J = U.Judge()
    mom, damp, nest, wd = opts
    ps, grads = _class_params(8)
    opt = FusedSGD(ps, lr=LR, momentum=mom, dampening=damp, nesterov=nest, weight_decay=wd, max_grad_norm=max_norm)

    def ref_of(before, g, pi, si, dm, k, gs, coef):
        a = (before["p"][pi], g[pi], before["momentum_buffer"][si] if mom else None, dm, LR, mom, damp, wd, nest,
             k == 0, gs, coef)
        return (U.sgd_ref(F64, *a), U.sgd_ref(F32, *a),
                lambda pi, si: {"p": opt.flat_space.data[pi], "buf": opt._bufs["momentum_buffer"][si] if mom else None})

    _class_steps(J, "sgd", opt, ps, grads, ref_of, grad_scale)
    if mom == 0:   # no buffer is passed to the kernel: the allocated one stays zero
        assert not opt._bufs["momentum_buffer"].any()
    J.check()


# ------------------------------------------------------------------------------- casts and fill
def _from_bits(bits, dtype):
    it = torch.int32 if dtype == F32 else torch.int16
    return torch.tensor([b - (1 << (32 if dtype == F32 else 16)) if b >> (31 if dtype == F32 else 15) else b for b in bits],
                        dtype=it).view(dtype)


# +-0, +-inf, a quiet and a signalling NaN, the largest finite value (rounds to inf), ties between two bf16
# neighbours with an even and an odd lower one (both signs), denormals: the smallest, the largest, a tie
# between 0 and the smallest bf16 denormal, a tie that rounds up, a bf16 denormal
SPECIAL_F32 = _from_bits([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0x7F7FFFFF, 0xFF7FFFFF,
                          0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x00000001, 0x007FFFFF,
                          0x80000001, 0x00008000, 0x00018000, 0x00010000, 0x807F8000], F32)
SPECIAL_BF16 = _from_bits([0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0x7F7F, 0xFF7F, 0x0001, 0x007F, 0x8001, 0x0080, 0x8080,
                           0x3F80, 0x0400], BF16)
CAST_SIZES = (1, 3, 4, 5, 1023, 1027, 8192 * 1024 + 7)   # the last: the grid is capped at 8192 blocks


def _with_specials(n, special, seed):
    """randn with the special values planted at the front, in the middle and in the tail (rotated by n, so
    the short sizes take different ones)"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=gen).to(special.dtype)
    sp = special.roll(n % special.numel())
    k = min(n, sp.numel())
    x[:k] = sp[:k]
    x[n - k:] = sp[sp.numel() - k:]
    if n > 4 * sp.numel():
        x[n // 2:n // 2 + k] = sp
    return x


def _equal_or_both_nan(got, want):
    """bit for bit, but any NaN for a NaN"""
    g, w = got.cpu(), want.cpu()
    nan = w.float().isnan()
    assert torch.equal(g.float().isnan(), nan)
    ok = (_bits(g) == _bits(w)) | nan
    assert bool(ok.all()), (int((~ok).sum()), _bits(g)[~ok][:8].tolist(), _bits(w)[~ok][:8].tolist())


def _guarded(n, dtype, fill=NAN):
    buf = torch.full((n + PAD,), fill, dtype=dtype, device=DEV)
    return buf, buf[:n]


@pytest.mark.parametrize("n", CAST_SIZES)
def test_f32_to_bf16(n):
    x = _with_specials(n, SPECIAL_F32, n)
    buf, y = _guarded(n, BF16, 3.0)
    _ext().f32_to_bf16(x.to(DEV), y)
    _equal_or_both_nan(y, x.bfloat16())
    assert bool((buf[n:] == 3.0).all())


@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("n", CAST_SIZES)
def test_bf16_to_f32(n, scale):
    x = _with_specials(n, SPECIAL_BF16, n + 1)
    buf, y = _guarded(n, F32, 3.0)
    _ext().bf16_to_f32(x.to(DEV), y, scale)
    _equal_or_both_nan(y, x.float() * scale)
    assert bool((buf[n:] == 3.0).all())


@pytest.mark.parametrize("R,C", [(64, 64), (65, 130), (100, 72), (7, 3), (4, 1028), (1028, 4)])
def test_f32_to_bf16_t(R, C):
    x = _with_specials(R * C, SPECIAL_F32, R).view(R, C)
    buf, y = _guarded(R * C, BF16, 3.0)
    _ext().f32_to_bf16_t(x.to(DEV), y.view(C, R))
    _equal_or_both_nan(y.view(C, R), x.t().contiguous().bfloat16())
    assert bool((buf[R * C:] == 3.0).all())


@pytest.mark.parametrize("value", [0.0, -1.5])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, 2048 * 1024 + 7])   # the last: the grid is capped at 2048 blocks
def test_fill_f32(n, value):
    buf, x = _guarded(n, F32)
    _ext().fill_f32(x, value)
    assert _same(x, torch.full((n,), value, device=DEV))
    assert bool(buf[n:].isnan().all())
    if n > 1:   # a view at offset 1 is 4 bytes past a 16-B boundary
        with pytest.raises(RuntimeError, match="16-B aligned"):
            _ext().fill_f32(buf[1:n], value)
        assert _same(x, torch.full((n,), value, device=DEV))
