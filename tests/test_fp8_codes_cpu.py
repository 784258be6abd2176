"""The e4m3 code space on the CPU: the reference of tests/fp8_codes.py against torch's cast, the torch
formulas of ops/fp8.py on every rounding boundary and on tiny rows, and the teeth of the comparisons that
tests/test_fp8_codes_gpu.py makes.

Sensitivity, in the manner of tests/test_ulp_cpu.py and DECODE_MUTANTS: every mutant of FP8_MUTANTS is
rejected by the comparison the GPU test uses at that site (equal codes on the anchored runs, equal
numbers on the one-hot few-row calls and on the one-key decode case, decode_ref's allowance on a cache
of subnormal codes), with the CPU path standing in for the kernel.  The gap these tests close is stated
as a test of the inputs: on the `randn` inputs of the older FP8 tests the two subnormal mutants stay far
inside the per-element allowances.
"""
import math

import pytest
import torch

from ray_torch_distributed_checkpoint_amd import ops
from tests import decode_ref as D
from tests import fp8_codes as C
from tests import ulp as U

F64, F32, BF16, U8, FP8 = C.F64, C.F32, C.BF16, C.U8, torch.float8_e4m3fn
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])


def _cpu_quant(w):
    q, s = ops.quantize_fp8_rows(w)
    return q.view(U8), s


@DTYPES
def test_reference_is_torchs_cast_on_every_boundary(dtype):
    v = C.boundary_values(dtype)
    assert v.dtype == dtype and v.numel() == 1516 and v.double().abs().max().item() == 448.0
    assert torch.equal(v.double(), v.to(BF16).double()) == (dtype == BF16)
    got = C.rne_e4m3(v.double())
    assert torch.equal(got, v.to(FP8).view(U8))
    assert set(got.tolist()) == set(C.FINITE_CODES.tolist())        # every finite code is somebody's nearest
    table = torch.arange(256, dtype=U8).view(FP8).double()
    assert torch.equal(table.nan_to_num(nan=-1.0), C.E4M3_VALUES.nan_to_num(nan=-1.0))
    assert int(torch.isnan(C.E4M3_VALUES).sum()) == 2 and C.E4M3_VALUES[0x7E].item() == 448.0


def test_reference_ties_signs_and_overflow():
    x = torch.tensor([2.0 ** -10, -2.0 ** -10, 3 * 2.0 ** -10, 0.0, -0.0, 17.0, 19.0, 463.99, 464.0, -1e9, float("nan")])
    want = [0x00, 0x80, 0x02, 0x00, 0x80, 0x58, 0x5A, 0x7E, 0x7F, 0x7F, 0x7F]      # 17 -> 16, 19 -> 20: ties to even
    assert C.rne_e4m3(x.double()).tolist() == want


@DTYPES
@pytest.mark.parametrize("run", [64, 1536])
def test_cpu_quantiser_on_anchored_rows(run, dtype):
    w, codes, scales = C.anchored_runs(C.boundary_values(dtype), run, C.ANCHOR_JS)
    q, s = _cpu_quant(w)
    assert torch.equal(s, scales) and torch.equal(q, codes)
    assert bool((s == torch.ldexp(torch.ones(()), torch.tensor(C.ANCHOR_JS))[torch.arange(len(s)) % 5]).all())


@pytest.mark.parametrize("mutant", C.QUANT_MUTANTS)
def test_quantising_mutants_fail_the_anchored_comparison(mutant):
    """the GPU test asserts equal codes on these runs, at every quantising site; each mutant differs from
    the CPU path's codes, and exactly where it should"""
    for dtype in (F32, BF16):
        for run in (64, 128, 1536):
            w, codes, scales = C.anchored_runs(C.boundary_values(dtype), run, C.ANCHOR_JS)
            q, _ = _cpu_quant(w)
            t = w.double() / scales.double()[:, None]
            bad = C.rne_e4m3(t, mutant)
            assert not torch.equal(q, bad)
            differs, a = q != bad, t.abs()
            lo = (torch.searchsorted(C._POS, a.contiguous(), right=True) - 1).clamp(0, 126)
            mid = (C._POS[lo] + C._POS[(lo + 1).clamp_max(126)]) / 2
            where = {"half_away": (a == mid) & (lo % 2 == 0) & (lo < 126), "truncate": (a > mid) | ((a == mid) & (lo % 2 == 1)),
                     "subnormal_quotient_flushed": (a < 2.0 ** -6) & (a > 2.0 ** -10), "zero_sign_dropped": torch.signbit(t) & (a <= 2.0 ** -10)}
            assert torch.equal(differs, where[mutant]) and int(differs.sum()) >= 4, (mutant, dtype, run)


def _few_rows_cpu(q, scale, k0):
    return ops.linear_few_rows_fp8(C.one_hot_rows(q.shape[1], k0), q.view(FP8), scale)


def test_widening_mutant_fails_the_exact_comparisons():
    """few-row: the CPU path gives value * scale as numbers at every k, the mutant's expectation does not, and
    a NaN byte makes its column NaN; decode: the CPU path on the one-key case gives value * vscale exactly"""
    q, scale = C.few_rows_codes(128)
    assert all(int((q[:, k] == c).sum()) >= 1 for k in (0, 77, 127) for c in C.FINITE_CODES.tolist())
    for k0 in range(0, 128, 16):
        y = _few_rows_cpu(q, scale, k0)
        assert y.dtype == BF16 and torch.equal(y.double(), C.few_rows_expected(q, scale, k0))
        assert not torch.equal(y.double(), C.few_rows_expected(q, scale, k0, "subnormal_widened_zero"))
    q[5, 40] = C.NANB
    y = _few_rows_cpu(q, scale, 32).double()
    assert bool(torch.isnan(y[:, 5]).all()) and bool(torch.isfinite(y[:, :5]).all()) and bool(torch.isfinite(y[:, 6:]).all())
    for H in (4, 8):
        qkv_new, codes, scales, want = C.v_codes_case(H)
        kvc = ops.KVCache(1, 4, 320, 4, 64, kv_dtype="fp8")
        kvc.layers[0].view(U8).copy_(codes)
        kvc.scales[0].copy_(scales)
        kvc.pos.copy_(torch.tensor((1, 64, 130, 319), dtype=torch.int32))
        kvc.length = 319
        out = ops.decode_attention(qkv_new, kvc, 0, H, 4, window=2)
        assert torch.equal(out.double(), want)
        assert set(codes[:, :, 256:][scales[:, :, 4:].isfinite().repeat_interleave(64, 2)].tolist()) == set(C.FINITE_CODES.tolist())
        bad = C.widen(codes[scales[:, :, 0].isfinite()][:, 256:], "subnormal_widened_zero").view(4, 4, 64)
        bad = (bad * scales[scales[:, :, 0].isfinite()][:, 4:].double()[..., None]).repeat_interleave(H // 4, 1).view(4, -1)
        assert not torch.equal(out.double(), bad)


@pytest.mark.parametrize("H,Hkv,Dh", [(4, 2, 128), (8, 1, 64)])
def test_subnormal_mutants_pass_randn_and_fail_the_code_caches(H, Hkv, Dh):
    """The gap, as a test of the inputs.  On the `randn` cache of tests/test_decode_fp8kv_gpu.py, quantised as
    that test quantises it, a handful of codes are subnormal and not every byte value occurs; flushing the
    subnormal quotients (at the quantiser) or the subnormal codes (at the widening) moves no element of `out`
    by a tenth of decode_ref's allowance.  On code_cache("subnormal") the widening mutant is far outside it."""
    pos, window = (63, 65, 127), None
    q, cache = D.decode_inputs("randn", 3, D.TMAX, H, Hkv, Dh)
    cq, cs = C.quant_runs(cache, Dh)
    assert torch.equal(cq, ops.quantize_fp8_rows(cache.reshape(-1, Dh).contiguous())[0].view(U8).view(cq.shape))
    sub = ((cq & 0x78) == 0) & ((cq & 0x07) != 0)
    print(f"randn cache: subnormal share {sub.float().mean().item():.3g}, {torch.unique(cq).numel()} byte values")
    assert 0 < sub.float().mean().item() < 1e-3
    nq, ns = C.quant_runs(q[:, H * Dh:], Dh)
    new64 = torch.cat([q[:, : H * Dh].double(), C.dequant(nq, ns, Dh)], dim=1)
    ref = D.decode_ref(F64, new64, C.dequant(cq, cs, Dh), pos, H, Hkv, Dh, window)
    flushed = D.decode_ref(F64, new64, C.dequant(C.quant_runs(cache, Dh, "subnormal_quotient_flushed")[0], cs, Dh),
                           pos, H, Hkv, Dh, window)["out"]
    zeroed = D.decode_ref(F64, new64, C.dequant(cq, cs, Dh, "subnormal_widened_zero"), pos, H, Hkv, Dh, window)["out"]
    for name, bad in (("flushed", flushed), ("zeroed", zeroed)):
        e = U.allow_err(bad, ref["out"], ref["allow_out"])
        print(f"randn cache, subnormal {name}: {e:.3g} x allowance")
        assert e < 0.1
    cq, cs, nq, ns, ref, _ = C.decode_code_case("subnormal", q, H, Hkv, Dh, pos, window, D.TMAX)
    new64 = torch.cat([q[:, : H * Dh].double(), C.dequant(nq, ns, Dh)], dim=1)
    bad = D.decode_ref(F64, new64, C.dequant(cq, cs, Dh, "subnormal_widened_zero"), pos, H, Hkv, Dh, window)["out"]
    e = U.allow_err(bad, ref["out"], ref["allow_out"])
    print(f"code_cache(subnormal), subnormal zeroed: {e:.3g} x allowance")
    assert e > 10.0


def test_subnormal_mutants_pass_the_randn_weights():
    """the quantiser test's [37, 2080] randn weight has subnormal codes in fewer than 2 of 10 000 elements;
    on a few-row case of the same kind (x, w randn; 16 x 136 x 384) both subnormal mutants move y by less than
    a tenth of the least the GEMM yardstick ever allows (half a bf16 place and 16 x 2^-10)"""
    w = torch.randn(37, 2080, generator=torch.Generator().manual_seed(5))
    q, _ = C.quant_runs(w, 2080)
    sub = ((q & 0x78) == 0) & ((q & 0x07) != 0)
    assert 0 < int(sub.sum()) < 2e-4 * q.numel()
    g = torch.Generator().manual_seed(136 + 384)
    x, w = torch.randn(16, 384, generator=g).to(BF16).double(), torch.randn(136, 384, generator=g)
    q, s = C.quant_runs(w, 384)
    wd = C.dequant(q, s, 384)
    ref, S = x @ wd.t(), x.abs() @ wd.abs().t()
    for bad in (C.dequant(C.quant_runs(w, 384, "subnormal_quotient_flushed")[0], s, 384), C.dequant(q, s, 384, "subnormal_widened_zero")):
        e = U.ulp_err(x @ bad.t(), ref, U.FLOOR_GEMM * S)
        print(f"randn weight, subnormal mutant: {e:.3g} ulp of {U.allow_bf16(0.0):.3g} allowed at the least")
        assert e < 0.1 * U.allow_bf16(0.0)


@pytest.mark.parametrize("kind", ["codes", "subnormal"])
@pytest.mark.parametrize("H,Hkv,Dh", [(4, 2, 128), (8, 1, 64), (12, 12, 64)])
def test_twin_inside_the_allowance_on_code_caches(H, Hkv, Dh, kind):
    """the condition on the inputs of the GPU test: decode_ref's fp32 twin stays inside decode_ref's unchanged
    allowance on caches of given codes, the new token quantised by the CPU formula"""
    J = U.Judge()
    q, _ = D.decode_inputs("randn", 3, D.TMAX, H, Hkv, Dh)
    for pos in D.POS_SETS:
        for window in (5, None):
            _, _, _, _, ref, twin = C.decode_code_case(kind, q, H, Hkv, Dh, pos, window, D.TMAX)
            assert bool((ref["allow_out"] > 0).all())
            J.within("decode_codes", (kind, pos, window), "out", None, ref["out"], twin, ref["allow_out"])
    J.check()


@pytest.mark.parametrize("name,w", C.tiny_rows(64), ids=[n for n, _ in C.tiny_rows(64)])
def test_tiny_rows_stay_finite(name, w):
    """a row whose amax / 448 underflows to zero gets scale 1.0 and zero codes, not a division by zero; a
    subnormal scale is coarse but finite; a normal scale keeps the rounding bound of the format"""
    q, s = _cpu_quant(w)
    C.check_tiny(w, q, s)
    if name == "fp32_1e-44":
        assert s.item() == 1.0 and not bool((q & 0x7F).any())
    assert math.isfinite(s.item())
