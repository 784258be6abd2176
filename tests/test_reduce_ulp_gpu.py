"""The stand-alone reduction kernels judged exactly (GPU only): the column sums of norm.hip, the gradient-norm
kernels of optim.hip and the loss finalisation of xent.hip, each called through its binding.

The yardstick is the reductions section of tests/ulp.py.  A reference mirrors the kernel's partition, not its
summation order.  On `ints` (non-zero integers whose every partial and total sum is exact in the kernel's
accumulator) a kernel must equal the float64 reference BIT FOR BIT: one dropped, duplicated or misplaced row,
column, tail element or job changes the result.  On `offset` (randn + 1) an fp32 sum is held to
max(16 x the twin, (R + 16) 2^-24) of the fp64 sum of |terms|, an fp64 sum (gradnorm_*) to the same with 2^-53
against math.fsum of the exact squares; R is the number of terms a lane adds serially (U.reduce_R_*).  Every
output is pre-filled with NaN and followed by 64 guard elements that must still be NaN; padding columns, gaps
between chunks and whatever follows an input are NaN too.  Each judged output prints one ULP line, each test its
WORST lines; those of one run are kept in profiles/reduce_ulp_worst.txt.

Arm -> the test that reaches it:

  colsum_partial_kernel<bf16 / float, VEC>: N = 8, 72, 512, 520, 1032 at ld = N, N + 8 (the second and third
  512-column block with one lane busy and with all); <.., scalar>: N = 100, 7 and every ld = N + 3; M < nblk
  (empty blocks: exactly 0), rows_per_block 1, 2, 17, 66 (the waves' row counts unequal), `min(M, .)`      test_colsum_partial
  launch_colsum_partial: N % 8 == 0 and ld % 8 == 0 on a pointer that is not 16-B aligned -> scalar arm    test_colsum_partial_misaligned_view
  colsum / colsum_partial bindings: CPU tensors, a dtype that is neither bf16 nor fp32, M / N / nblk < 1,
  ld < N, X shorter than (M - 1) ld + N, ws / out of the wrong dtype or too small                          test_colsum_bindings_refuse
  colsum_wide_kernel (colsum_wide_cols): W = 1 .. 4096 around the 16-wave and the 16 x kWideU = 192-row
  steps, D = 1 .. 200 (one lane, a partial and a second 64-column block), accumulate 0 / 1, twice bitwise   test_colsum_wide
  colsum_ws_kernel, two launches (W = 4097, 4160 > kWideMaxRows: S = 64, R = 65, the last stage-1 block
  partial / full, the `w < r1` tail add, accumulate only in the second launch)                             test_colsum_two_launch
  colsum_ws_kernel with RTDC_COLSUM_WIDE=0: single stage (W = 1, 17, 63; `accumulate && gridDim.y == 1`),
  two stages at small W (64: S = 2; 193: S = 6, the last block partial)                                    test_colsum_knobs_off
  colsum_multi_kernel: 1, 5 and 32 jobs, irregular start[] (a 1-column job after a 2-block job, D < 64),
  accumulate bit 31, each job bitwise the immediate colsum                                                 test_colsum_multi
  rtdc_colsum_multi refusals (n = 0, 33; W = 0, 4097; D = 0): nothing written                              test_colsum_multi_refuses
  gradnorm_partial_kernel: vector path with the 4-deep loop (`j + 768 < nv`: len 4099, 16384), the single
  loop and the scalar tail (len % 4 = 1, 2, 3), scalar path (start & 3 != 0) with both loops, len < 4,
  the `offset` into partial                                                                                test_gradnorm_partial
  gradnorm_finalize_kernel: n = 0, 1, around 1024 (the serial part runs 0, 1, 2, 5 times), `local` set
  (out untouched) / null (write_clip: clip active / inactive, grad_scale 1, 1/8, 3, NaN and inf sums)      test_gradnorm_finalize_local, test_gradnorm_finalize_clip
  gradnorm_combine_kernel: world 1, 2, 8 == finalize over the same numbers bit for bit                     test_gradnorm_combine
  xent_finalize_kernel<false / true>: M = 1, around 1024, 3000; some / no / all targets ignored (divisor
  clamped to 1), no targets (fixed_n); out[2] with ce, untouched without                                   test_xent_finalize
  xent_alpha_kernel: the fp32 quotient, den = 1                                                            test_xent_alpha

out[1] of write_clip (the clip coefficient) is computed from the kernel's own out[0] and held to 1 fp32 ulp of
`U.clip_ref`.  It is NOT that number bit for bit: on the MI355X 69 of the 72 cases of test_gradnorm_finalize_clip
are, and the three that sit one ulp off all have grad_scale = 3, the one scale whose product with the root is
not exact.  The compiler contracts `total + 1e-6f` with the product before it into one fma, so the divisor is
formed from the unrounded product while out[0] holds the rounded one; at most half an ulp of the divisor, hence
at most one of the quotient.  The division itself is the correctly rounded one: the quotients of xent_finalize
(exact operands on `ints`) and xent_alpha equal the CPU's fp32 division bit for bit, and that is asserted.
"""
import math
import os
import subprocess
import sys

import pytest
import torch

from tests import ulp as U

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F64, F32, BF16 = U.F64, U.F32, U.BF16
NAN = float("nan")
PAD = 64   # untouched guard elements behind every output
GENS = U.REDUCE_GENS
DTYPES = [BF16, F32]


def _ext():
    from ray_torch_distributed_checkpoint_amd.ops._ext import gpu_ext

    return gpu_ext()


def _name(dtype):
    return str(dtype)[6:]


def _guarded(n, dtype=F32, fill=NAN):
    """(buffer of n + PAD elements, its first n): the call gets the view, the guards are checked on the buffer"""
    buf = torch.full((n + PAD,), fill, dtype=dtype, device=DEV)
    return buf, buf[:n]


def _untouched(buf, n=0):
    return bool(buf[n:].isnan().all())


def _bits(t):
    return t.contiguous().view({F32: torch.int32, F64: torch.int64}[t.dtype])


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _judge(J, gen, op, shape, what, out, r, t, scale, R):
    """one ULP line; on `ints` the output is the float64 reference bit for bit"""
    J.rel(op, shape, what, out, r, t, scale, R)
    if gen == "ints":
        bad = out.double() != r
        assert not bool(bad.any()), (op, shape, what, int(bad.sum()), bad.nonzero()[:4].tolist())


# ------------------------------------------------------------------------------- colsum_partial
def _partial_case(J, gen, dtype, X, M, N, ld, nblk, label=()):
    buf, ws = _guarded(nblk * N)
    _ext().colsum_partial(X, M, N, ld, ws, nblk)
    a = (M, N, ld, nblk)
    r, t = U.colsum_partial_ref(F64, X, *a), U.colsum_partial_ref(F32, X, *a)
    sc = U.colsum_partial_ref(F64, X.abs(), *a).clamp_min(U.TINY)
    got = ws.view(nblk, N)
    _judge(J, gen, "colsum_part", (_name(dtype), gen) + a + label, "ws", got, r, t, sc, U.reduce_R_partial(M, nblk))
    empty = got[-(-M // U.reduce_rpb(M, nblk)):]
    assert not bool(empty.any()) and not bool(empty.isnan().any()), a   # a block without rows: exactly 0
    assert _untouched(buf, nblk * N), a


@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_colsum_partial(dtype, gen):
    J = U.Judge()
    for M, nblk, N, ld in U.reduce_partial_cases():
        X = U.reduce_partial_input(gen, dtype, M, N, ld, seed=N + M, dev=DEV)   # the padding columns are NaN
        _partial_case(J, gen, dtype, X, M, N, ld, nblk)
    J.check()


@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_colsum_partial_misaligned_view(dtype, gen):
    """X[:, 1:9] of a [M, 16] buffer: N % 8 == 0 and ld % 8 == 0, but the pointer is 2 (bf16) or 4 (fp32) bytes
    past a 16-B boundary.  The launcher must not take the 16-B loads on it; the sums are right either way."""
    J = U.Judge()
    for M, nblk in U.REDUCE_PARTIAL_MN:
        whole = U.reduce_gen(gen, (M, 16), M, dtype, DEV)
        whole[:, 0] = NAN
        whole[:, 9:] = NAN
        X = whole[:, 1:9]
        assert X.data_ptr() % 16 == whole.element_size() and X.stride(0) == 16
        _partial_case(J, gen, dtype, X, M, 8, 16, nblk, ("view",))
    J.check()


def test_colsum_bindings_refuse():
    """a refused call raises, launches nothing and leaves ws and out as they were"""
    M, N, nblk = 9, 8, 4
    X = torch.ones(M, N, device=DEV)
    wbuf, ws = _guarded((nblk + 64) * N)
    obuf, out = _guarded(N)
    ok = dict(X=X, M=M, N=N, ld=N, ws=ws, nblk=nblk, out=out)
    bad = [dict(X=X.cpu()), dict(ws=ws.cpu()), dict(out=out.cpu()),
           dict(X=X.half()), dict(X=X.double()), dict(X=X.int()),
           dict(M=0), dict(N=0), dict(nblk=0), dict(M=-1), dict(ld=N - 1),
           dict(M=M + 1),                                   # X holds 9 rows
           dict(X=X.view(-1)[1:].view(-1), M=M),            # one element short of (M - 1) ld + N from its pointer
           dict(ld=N + 1),                                  # (M - 1) (N + 1) + N > M N
           dict(ws=ws.double()), dict(ws=ws.bfloat16()), dict(ws=ws[:nblk * N - 1]),
           dict(out=out.bfloat16()), dict(out=out.double()), dict(out=out[:N - 1])]
    for kw in bad:
        a = {**ok, **kw}
        if "out" not in kw:
            with pytest.raises(RuntimeError):
                _ext().colsum_partial(a["X"], a["M"], a["N"], a["ld"], a["ws"][:nblk * N], a["nblk"])
        if "ws" in kw and kw["ws"].dtype == F32 and kw["ws"].is_cuda:
            a["ws"] = ws[:(nblk + 64) * N - 1]               # big enough for the partials, not for the level-2 rows
        with pytest.raises(RuntimeError):
            _ext().colsum(a["X"], a["M"], a["N"], a["ld"], a["ws"], a["nblk"], a["out"], False)
    torch.cuda.synchronize()
    assert _untouched(wbuf) and _untouched(obuf)
    _ext().colsum(X, M, N, N, ws, nblk, out, False)          # and the call they all vary is a good one
    assert torch.equal(out, torch.full((N,), float(M), device=DEV)) and _untouched(obuf, N)


# ------------------------------------------------------------------------------- wide / two-launch / knobs off
def _base(gen, D, acc, seed):
    """what `out` holds before the launch: an integer / offset base when accumulating, else NaN"""
    return U.reduce_gen(gen, (D,), seed, F32, DEV) if acc else torch.full((D,), NAN, device=DEV)


def _rows_case(J, gen, op, W, D, acc, R):
    """colsum of an fp32 [W][D] matrix with nblk = W: rows_per_block = 1, so stage 1 copies X into ws and the
    reduction under test sums exactly the rows of X"""
    X = U.reduce_gen(gen, (W, D), W + D, F32, DEV)
    base = _base(gen, D, acc, W + D + 1)
    got = []
    for _ in range(2):
        ws = torch.full(((W + 64) * D,), NAN, device=DEV)
        buf, out = _guarded(D)
        out.copy_(base)
        _ext().colsum(X, W, D, D, ws, W, out, bool(acc))
        assert _same(ws[:W * D].view(W, D), X), (W, D)
        assert _untouched(buf, D), (W, D)
        got.append(out)
    a = (X, W, D, base, bool(acc))
    sc = U.colsum_rows_ref(F64, X.abs(), W, D, base.abs(), bool(acc)).clamp_min(U.TINY)
    _judge(J, gen, op, (gen, W, D, acc), "out", got[0], U.colsum_rows_ref(F64, *a), U.colsum_rows_ref(F32, *a), sc, R + acc)
    assert _same(got[0], got[1]), (W, D, acc)
    return X, base, got[0]


@pytest.mark.parametrize("gen", GENS)
def test_colsum_wide(gen):
    J = U.Judge()
    for W in U.REDUCE_WIDE_W:
        for D in U.REDUCE_WIDE_D:
            for acc in (0, 1):
                _rows_case(J, gen, "colsum_wide", W, D, acc, U.reduce_R_wide(W))
    J.check()


@pytest.mark.parametrize("gen", GENS)
def test_colsum_two_launch(gen):
    J = U.Judge()
    for W in U.REDUCE_TWO_LAUNCH_W:
        assert U.reduce_ws_plan(W) == (64, 65)
        for D in U.REDUCE_WIDE_D:
            for acc in (0, 1):
                _rows_case(J, gen, "colsum_ws2", W, D, acc, U.reduce_R_ws(W))
    J.check()


def _knobs_off_child():
    """what test_colsum_knobs_off runs in its child process"""
    assert os.environ["RTDC_COLSUM_WIDE"] == "0"
    J = U.Judge()
    for gen in GENS:
        for W in U.REDUCE_KNOBS_OFF_W:
            for D in U.REDUCE_WIDE_D:
                for acc in (0, 1):
                    _rows_case(J, gen, "colsum_ws", W, D, acc, U.reduce_R_ws(W))
    J.check()


def test_colsum_knobs_off():
    """RTDC_COLSUM_WIDE=0, which the library reads once per process, so in a fresh child: the wide cases at
    W = 1, 17, 63 (one colsum_ws_kernel launch, accumulating in it), 64 and 193 (two launches, S = 2 and 6)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RTDC_COLSUM_WIDE="0", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", "from tests.test_reduce_ulp_gpu import _knobs_off_child as f; f()"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("ULP ") == len(GENS) * len(U.REDUCE_KNOBS_OFF_W) * len(U.REDUCE_WIDE_D) * 2


# ------------------------------------------------------------------------------- colsum_multi
def _multi_case(J, gen, table, seed):
    jobs, bufs, outs = [], [], []
    for j, (W, D, acc) in enumerate(table):
        ws = U.reduce_gen(gen, (W, D), seed + 2 * j, F32, DEV)
        base = _base(gen, D, acc, seed + 2 * j + 1)
        buf, out = _guarded(D)
        out.copy_(base)
        jobs.append((ws, W, D, base, bool(acc)))
        bufs.append(buf)
        outs.append(out)
    _ext().colsum_multi([j[0].view(-1) for j in jobs], outs, [j[1] for j in jobs], [j[2] for j in jobs],
                        [int(j[4]) for j in jobs])
    r, t = U.colsum_multi_ref(F64, jobs), U.colsum_multi_ref(F32, jobs)
    sc = U.colsum_multi_ref(F64, [(ws.abs(), W, D, b.abs(), a) for ws, W, D, b, a in jobs])
    for j, (ws, W, D, base, acc) in enumerate(jobs):
        _judge(J, gen, "colsum_multi", (gen, len(table), j, W, D, int(acc)), "out", outs[j], r[j], t[j],
               sc[j].clamp_min(U.TINY), U.reduce_R_wide(W) + acc)
        assert _untouched(bufs[j], D), j
        # the immediate form over the same rows: the same bits, asserted and not assumed
        scratch = torch.full(((W + 64) * D,), NAN, device=DEV)
        now = base.clone()
        _ext().colsum(ws, W, D, D, scratch, W, now, acc)
        assert _same(outs[j], now), (len(table), j, W, D)


@pytest.mark.parametrize("gen", GENS)
def test_colsum_multi(gen):
    J = U.Judge()
    _multi_case(J, gen, ((193, 65, 0),), 1)
    _multi_case(J, gen, ((17, 64, 1),), 2)
    _multi_case(J, gen, U.REDUCE_MULTI_5, 3)
    assert len(U.REDUCE_MULTI_32) == 32 and U.REDUCE_MULTI_32[31][2] == 1
    _multi_case(J, gen, U.REDUCE_MULTI_32, 4)
    J.check()


def test_colsum_multi_refuses():
    good = torch.ones(4097 * 8, device=DEV)
    b0, o0 = _guarded(8)
    b1, o1 = _guarded(8)
    m = _ext().colsum_multi
    with pytest.raises(RuntimeError):
        m([], [], [], [], [])
    with pytest.raises(RuntimeError):
        m([good] * 33, [o0] * 33, [5] * 33, [8] * 33, [0] * 33)
    for W, D in ((0, 8), (4097, 8), (5, 0)):
        with pytest.raises(RuntimeError):
            m([good, good], [o0, o1], [5, W], [8, D], [0, 0])     # the first job is a good one: it must not run
    torch.cuda.synchronize()
    assert _untouched(b0) and _untouched(b1)
    m([good, good], [o0, o1], [5, 4096], [8, 8], [0, 0])
    assert torch.equal(o0, torch.full((8,), 5.0, device=DEV)) and torch.equal(o1, torch.full((8,), 4096.0, device=DEV))
    assert _untouched(b0, 8) and _untouched(b1, 8)


# ------------------------------------------------------------------------------- gradnorm
def _chunk_table(rows):
    """[(start, len)] -> the int64 [n, 3] table (start, len | decay << 32, sstart)"""
    return torch.tensor([(s, ln, 0) for s, ln in rows], dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("gen", GENS)
def test_gradnorm_partial(gen):
    J = U.Judge()
    rows, n = U.gradnorm_chunks()
    vals = U.reduce_gen(gen, (n,), 3, bound=1 << 10)
    g = torch.full((n + PAD,), NAN)
    for s, ln in rows:                      # the gaps between the chunks stay NaN
        g[s:s + ln] = vals[s:s + ln]
    ex, tw = U.gradnorm_partial_exact(g, rows), U.gradnorm_partial_ref(F64, g, rows)
    off, nc = 3, len(rows)
    buf, partial = _guarded(off + nc + 5, F64)
    _ext().gradnorm_partial(_chunk_table(rows), nc, g.to(DEV), partial, off)
    got = partial[off:off + nc].cpu()
    for i, (s, ln) in enumerate(rows):
        J.rel64("gradnorm_part", (gen, s & 3, ln), "partial", got[i], ex[i], tw[i], ex[i], U.reduce_R_gradnorm(ln))
        if gen == "ints":
            assert got[i] == ex[i], (s, ln, got[i].item(), ex[i].item())
    assert _untouched(partial[:off]) and _untouched(buf, off + nc)
    J.check()


def _partials(gen, n, seed):
    """n fp64 partial sums: integers up to 2^30, or squares of randn + 1 with full fp64 mantissas"""
    if gen == "ints":
        return torch.randint(1, 1 << 30, (n,), generator=torch.Generator().manual_seed(seed)).double()
    return U.reduce_gen("offset", (n,), seed, F64).square()


def _with_nan_behind(p):
    """the numbers on the device, NaN behind them (a read past n poisons the sum)"""
    buf = torch.full((p.numel() + PAD,), NAN, dtype=F64, device=DEV)
    buf[:p.numel()] = p
    return buf


@pytest.mark.parametrize("gen", GENS)
def test_gradnorm_finalize_local(gen):
    J = U.Judge()
    for n in U.REDUCE_FINALIZE_N:
        p = _partials(gen, n, n)
        ex = torch.tensor(U.fsum64(p), dtype=F64)
        lbuf, local = _guarded(1, F64)
        obuf, out = _guarded(2)
        _ext().gradnorm_finalize(_with_nan_behind(p), n, 1.0, 1.0, out, local)
        got = local.cpu()[0]
        if n == 0 or gen == "ints":
            assert got == ex, (n, got.item(), ex.item())
        if n:
            J.rel64("gradnorm_fin", (gen, n), "local", got, ex, p.sum(), ex, U.reduce_R_finalize(n))
        assert _untouched(lbuf, 1) and _untouched(obuf)   # with `local` the clip pair is not written
    J.check()


def _clip_judge(J, shape, out, total_sq, gs, max_norm):
    """out[0] within 1.5 fp32 ulp of the fp64 grad_scale x sqrt(sum) (the cast of the root and the product round
    once each); out[1] within 1 ulp of clip_ref over the kernel's own out[0] (not bitwise: the module docstring)
    -> whether it is that bit for bit"""
    total, coef = out[0].item(), out[1].item()
    ref = U._f32(gs) * math.sqrt(total_sq)
    if ref == 0.0:
        assert total == 0.0
    else:
        J._note("write_clip", shape, "total", "ulp32", abs(total - ref) / U.ulp_f32(ref),
                abs(U.clip_ref(total_sq, gs, max_norm)[0] - ref) / U.ulp_f32(ref), 1.5, 1.5)
    want = U.clip_ref(total_sq, gs, max_norm, total=total)[1]
    J._note("write_clip", shape, "coef", "ulp32", abs(coef - want) / U.ulp_f32(want), 0.0, 1.0, 0.0)
    return coef == want


@pytest.mark.parametrize("gen", GENS)
def test_gradnorm_finalize_clip(gen):
    """an active clip (max_norm = half the norm: coef < 1) and an inactive one (twice the norm: coef == 1) at
    every n and grad_scale; a NaN sum gives a NaN pair, an infinite one (inf, 0)"""
    J = U.Judge()
    bitwise = []
    for n in U.REDUCE_FINALIZE_N:
        p = _partials(gen, n, n + 7)
        ex = U.fsum64(p)
        dev_p = _with_nan_behind(p)
        for gs in U.REDUCE_GRAD_SCALES:
            norm = gs * math.sqrt(ex)
            for active in (True, False):
                max_norm = U._f32((0.5 if active else 2.0) * norm) if n else 1.0
                obuf, out = _guarded(2)
                _ext().gradnorm_finalize(dev_p, n, gs, max_norm, out, None)
                o = out.cpu()
                bitwise.append(_clip_judge(J, (gen, n, gs, "active" if active else "inactive"), o, ex, gs, max_norm))
                assert (0.0 < o[1] < 1.0) if (active and n) else o[1] == 1.0, (n, gs, active, o.tolist())
                assert _untouched(obuf, 2)
    print("write_clip: coef bit for bit in", sum(bitwise), "of", len(bitwise))
    for bad, want in ((NAN, (NAN, NAN)), (float("inf"), (float("inf"), 0.0))):
        p = torch.tensor([1.0, bad, 2.0], dtype=F64)
        obuf, out = _guarded(2)
        _ext().gradnorm_finalize(_with_nan_behind(p), 3, 1.0, 1.0, out, None)
        o = out.cpu().tolist()
        assert all((a != a and b != b) or a == b for a, b in zip(o, want)), (bad, o)
        assert all((a != a and b != b) or a == b for a, b in zip(o, U.clip_ref(bad, 1.0, 1.0))), (bad, o)
        assert _untouched(obuf, 2)
    J.check()


@pytest.mark.parametrize("gen", GENS)
def test_gradnorm_combine(gen):
    J = U.Judge()
    for world in U.REDUCE_WORLDS:
        p = _partials(gen, world, world + 11)
        ex = U.fsum64(p)
        dev_p = _with_nan_behind(p)
        for gs in U.REDUCE_GRAD_SCALES:
            max_norm = U._f32(0.5 * gs * math.sqrt(ex))
            cbuf, comb = _guarded(2)
            fbuf, fin = _guarded(2)
            _ext().gradnorm_combine(dev_p, world, gs, max_norm, comb)
            _ext().gradnorm_finalize(dev_p, world, gs, max_norm, fin, None)
            _clip_judge(J, (gen, "combine", world, gs), comb.cpu(), ex, gs, max_norm)
            assert _same(comb, fin), (world, gs, comb.tolist(), fin.tolist())
            assert _untouched(cbuf, 2) and _untouched(fbuf, 2)
    J.check()


# ------------------------------------------------------------------------------- xent_finalize / xent_alpha
def _rows_in(v):
    """fp32 rows on the device with NaN behind them"""
    buf = torch.full((v.numel() + PAD,), NAN, device=DEV)
    buf[:v.numel()] = v
    return buf[:v.numel()]


@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("with_ce", [False, True], ids=["plain", "ce"])
def test_xent_finalize(with_ce, gen):
    J = U.Judge()
    for M in U.REDUCE_XENT_M:
        loss = _rows_in(U.reduce_gen(gen, (M,), M))
        ce = _rows_in(U.reduce_gen(gen, (M,), M + 1)) if with_ce else None
        for form in U.REDUCE_XENT_FORMS:
            tg = U.xent_finalize_targets(M, form, dev=DEV)
            fixed_n = M + 2.0
            obuf, out3 = _guarded(3)
            out = out3 if with_ce else out3[:2]
            _ext().xent_finalize(loss, tg, fixed_n, out, ce)
            # on the CPU: its fp32 division is the correctly rounded one
            a = (loss.cpu(), None if ce is None else ce.cpu(), None if tg is None else tg.cpu(), fixed_n)
            out = out.cpu()
            r, t = U.xent_finalize_ref(F64, *a), U.xent_finalize_ref(F32, *a)
            assert r[1] == {"all_ignored": 1, "none_ignored": M, "fixed_n": fixed_n}.get(form, r[1])
            J.rel("xent_finalize", (gen, M, form, with_ce), "out", out, r, t, U.xent_finalize_scale(a[0], a[1], r[1]),
                  U.reduce_R_finalize(M) + 1)
            assert out[1].item() == r[1].item()
            if gen == "ints":   # exact sums: the fp32 quotient of the twin is the kernel's, bit for bit
                assert _same(out, t), (M, form, out.tolist(), t.tolist())
            assert _untouched(obuf, 3 if with_ce else 2), (M, form)
    J.check()


def test_xent_alpha():
    for g, den in ((0.37, 3.0), (1.0, 1.0), (-2.5, 1.0), (1.0, 1023.0), (1.0 / 7, 2998.0)):
        gt, dt = torch.tensor([g, NAN], device=DEV), torch.tensor([den, NAN], device=DEV)
        obuf, out = _guarded(1)
        _ext().xent_alpha(gt[:1], dt[:1], out)
        want = torch.tensor([g]) / torch.tensor([den])   # the correctly rounded fp32 quotient
        assert _same(out.cpu(), want), (g, den, out.item(), want.item())
        assert _untouched(obuf, 1)
