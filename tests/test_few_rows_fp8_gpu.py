"""The FP8 few-row linear and its quantiser (csrc/kernels/gemm_few_rows_fp8.hip) on the GPU.

The linear is judged per element by the GEMM yardstick of tests/ulp.py, unchanged: `gemm_ref` on x and
the dequantised weights q * scale in float64 is the reference, in float32 on the device the twin.
PLANS: (N, K) -> the (T column tiles per block, W waves, chunks of 128 k per wave) with which the case
reaches its arm, asserted on the extension's plan.  Every call gets x inside a 16-row NaN buffer, q
followed by a row of e4m3 NaN bytes, scale and bias followed by a NaN, and writes y into a NaN-filled
[M + 1, N] buffer whose last row must keep its bits.
"""
import pytest
import torch

from ray_torch_distributed_checkpoint_amd import ops
from ray_torch_distributed_checkpoint_amd.ops._ext import gpu_ext
from tests import ulp as U

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32, BF16, FP8, NAN = torch.float64, torch.float32, torch.bfloat16, torch.float8_e4m3fn, float("nan")
PLANS = {(8, 128): (1, 1, 1),        # one chunk on one wave; 8 real weight rows
         (24, 128): (1, 1, 1),       # two blocks, the second partial
         (16, 256): (1, 2, 1),       # the LDS combine, one chunk per wave
         (136, 384): (1, 2, 2),      # 3 chunks that do not divide among the 2 waves
         (1000, 640): (1, 4, 2),     # last tile partial; 5 chunks on 4 waves: 2 + 2 + 1 + 0 (an idle wave)
         (40, 3072): (1, 16, 2),     # many k steps; a load group with 2 of its 4 chunks live
         (4088, 1024): (2, 8, 1),    # the smallest weight with T = 2 (256 tiles, 8 waves), last tile partial
         (8200, 1024): (4, 8, 1)}    # the smallest with T = 4 and a column tile wholly beyond N (513 tiles)
EPIS = ("plain", "bias_bf16", "bias_f32_gelu", "bias_res_gelu")
_refs: dict = {}   # (M, N, K, epi) -> the case, its fp64 reference and fp32 twin; dropped by the last test


def _torch_quant(w):   # the formula in torch (tensor divisors: true fp32 divisions)
    amax = w.float().abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / torch.full_like(amax, 448.0), torch.ones_like(amax))
    return (w.float() / scale[:, None]).to(FP8), scale


def _guarded(t, rows, fill=NAN):
    buf = torch.full((rows,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=DEV)
    buf[: t.shape[0]] = t
    return buf[: t.shape[0]]


def _case(M, N, K, epi):
    if (M, N, K, epi) not in _refs:
        g = torch.Generator().manual_seed(1009 * M + 31 * N + K + len(epi))
        gelu = epi.endswith("gelu")
        x = torch.randn(M, K, generator=g).to(BF16)
        q, scale = _torch_quant(torch.randn(N, K, generator=g) * (K ** -0.5 if gelu else 1.0))
        bias = torch.randn(N, generator=g).to(F32 if epi == "bias_f32_gelu" else BF16) if epi != "plain" else None
        c = {"M": M, "N": N, "K": K, "out_fp32": False, "colsum": False, "act": 2 if gelu else 0,
             "x": _guarded(x, 16), "q": _guarded(q.view(torch.uint8), N + 1, 0x7F).view(FP8),
             "scale": _guarded(scale, N + 1), "bias": None if bias is None else _guarded(bias, N + 1),
             "res": torch.randn(M, N, generator=g).to(BF16).to(DEV) if epi == "bias_res_gelu" else None}
        ref = lambda dt: U.gemm_ref(dt, c["x"], (c["q"].float().to(dt) * c["scale"].to(dt)[:, None]).t(), True, False,
                                    bias=c["bias"], Cin=c["res"], beta=1.0, act=c["act"])
        _refs[(M, N, K, epi)] = (c, ref(F64), ref(F32))
    return _refs[(M, N, K, epi)]


def _run(c, x=None, res=None):
    x, res = (c["x"], c["res"]) if x is None else (x, res)
    M, N = x.shape[0], c["N"]
    buf = torch.full((M + 1, N), NAN, dtype=BF16, device=DEV)
    y = ops.linear_few_rows_fp8(x, c["q"], c["scale"], bias=c["bias"], act=c["act"], residual=res, out=buf[:M])
    torch.cuda.synchronize()
    assert y.data_ptr() == buf.data_ptr() and bool(torch.isnan(buf[M]).all()), "a store below the last row"
    assert bool(torch.isfinite(buf[:M]).all()), "a masked row, column, scale or bias reached the output"
    return buf[:M]


@pytest.mark.parametrize("shape", list(PLANS), ids=lambda s: "%dx%d" % s)
def test_against_fp64(shape):   # M in 1, 7, 16 x the four epilogues; the plan reaches the arm PLANS names
    N, K = shape
    assert tuple(gpu_ext().few_rows_fp8_plan(N, K)) == PLANS[shape]
    J = U.Judge()
    for M in (1, 7, 16):
        for epi in EPIS:
            c, r, t = _case(M, N, K, epi)
            U.judge_gemm(J, "few_rows_fp8", "%dx%dx%d %s" % (M, N, K, epi), c, r, t, {"C": _run(c)})
    J.check()


@pytest.mark.parametrize("shape", [(8, 128), (16, 256), (8200, 1024)], ids=lambda s: "%dx%d" % s)
def test_row_invariance_and_determinism(shape):   # rows 0, 5, 15 of an M = 16 call against M = 1 calls on them
    bits = lambda t: t.contiguous().view(torch.int16)
    for epi in EPIS:
        c = _case(16, *shape, epi)[0]
        y16 = _run(c)
        assert torch.equal(bits(y16), bits(_run(c))), "two calls differ"
        for m in (0, 5, 15):
            y1 = _run(c, _guarded(c["x"][m:m + 1], 16), None if c["res"] is None else c["res"][m:m + 1].contiguous())
            assert torch.equal(bits(y1[0]), bits(y16[m])), (epi, m)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["randn", "zero_row", "boundary", "out"])
def test_quantiser_is_bitwise_the_torch_formula(kind, dtype):
    """[37, 2080]: the last block not full, a row loop of three steps, the last with idle lanes.  boundary:
    every row's maximum is 1.0234375, a bf16 number whose quotient by its own scale is not exactly 448."""
    w = torch.randn(37, 2080, generator=torch.Generator().manual_seed(5))
    if kind == "zero_row":
        w[11] = 0
    if kind == "boundary":
        w = w.clamp(-1.0, 1.0)
        w[:, 1029], w[3, 7] = 1.0234375, -1.0234375
    w = w.to(dtype).to(DEV)
    want_q, want_s = _torch_quant(w.cpu())
    assert bool(torch.isfinite(want_q.float()).all()) and want_q.float().abs().max().item() == 448.0
    out = (torch.empty((37, 2080), dtype=FP8, device=DEV), torch.empty(37, dtype=F32, device=DEV)) if kind == "out" else None
    q, s = ops.quantize_fp8_rows(w, out=out)
    assert out is None or (q.data_ptr() == out[0].data_ptr() and s.data_ptr() == out[1].data_ptr())
    assert torch.equal(s.cpu().view(torch.int32), want_s.view(torch.int32))
    assert torch.equal(q.cpu().view(torch.uint8), want_q.view(torch.uint8))


def test_refused_calls_raise_before_a_launch():   # in the op and in the binding itself; the output untouched
    _refs.clear()
    mk = lambda *s, dt=BF16: torch.ones(s, dtype=dt, device=DEV)
    q8 = lambda *s: mk(*s).to(FP8)
    for x, q, scale in ((mk(4, 192), q8(16, 192), mk(16, dt=F32)),              # K = 192
                        (mk(17, 128), q8(16, 128), mk(16, dt=F32)),             # M = 17
                        (mk(4, 128), q8(12, 128), mk(12, dt=F32)),              # N = 12
                        (mk(4, 128), mk(16, 128), mk(16, dt=F32)),              # bf16 q
                        (mk(4, 128), q8(16, 128), mk(16, dt=torch.float16)),    # fp16 scale
                        (mk(4, 128), q8(16, 128), mk(8, dt=F32)),               # scale of the wrong length
                        (mk(4, 128), q8(32, 128)[::2], mk(16, dt=F32))):        # strided q
        out = torch.full((x.shape[0], q.shape[0]), NAN, dtype=BF16, device=DEV)
        with pytest.raises((RuntimeError, ValueError, TypeError)):
            ops.linear_few_rows_fp8(x, q, scale, out=out)
        with pytest.raises((RuntimeError, ValueError, TypeError)):
            gpu_ext().gemm_few_rows_fp8(x, q, scale, None, None, out, 0)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())
