"""The few-row linear kernel (csrc/kernels/gemm_few_rows.hip) judged per element against fp64.

The yardstick is the GEMM section of tests/ulp.py, unchanged: `gemm_ref` in float64 is the
reference, in float32 the twin (computed on the device, once per case, shared); the bf16 output is
held to 0.5 ulp + 16 x the twin's error with a floor of FLOOR_GEMM x the sum of |terms|.  The case
table and the arm each (N, K) reaches are in tests/few_rows_cases.py; test_plan_reaches_the_named_arms
asserts each arm on the extension's own launch plan.

Every call gets x as the first M rows of a 16-row buffer whose other rows are NaN, w as the first
N rows of a buffer with a NaN row after them, and writes y into the first M rows of a NaN-filled
[M + 1, N] buffer whose last row must keep its bits: a read of a masked row or a store outside
y[:M, :N] shows.  Each test prints its WORST lines; those of one run are kept in
profiles/decode_fast.md.
"""
import pytest
import torch

from tests import few_rows_cases as FR
from tests import ulp as U

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32, BF16 = U.F64, U.F32, U.BF16
NAN = float("nan")
_refs: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_refs():
    yield
    _refs.clear()


def _ext():
    from ray_torch_distributed_checkpoint_amd.ops._ext import gpu_ext

    return gpu_ext()


def _G():
    from ray_torch_distributed_checkpoint_amd.ops import gemm as G

    return G


def _case(gen, M, N, K, epi, keep=True):
    """case, fp64 reference and twin: computed once, shared, never modified"""
    key = (gen, M, N, K, epi)
    if key not in _refs:
        c = FR.case(gen, M, N, K, epi, DEV)
        got = (c, *FR.refs(c))
        if not keep:
            return got
        _refs[key] = got
    return _refs[key]


def _operands(c):
    """x [M, K] inside a 16-row NaN buffer, w [N, K] with a NaN row after it"""
    M, N, K = c["M"], c["N"], c["K"]
    xb = torch.full((16, K), NAN, dtype=BF16, device=DEV)
    xb[:M] = c["a"]
    wb = torch.full((N + 1, K), NAN, dtype=BF16, device=DEV)
    wb[:N] = c["b"].t()
    return xb[:M], wb[:N]


def _run(c, x=None, w=None):
    """one linear_few_rows call on a case; y is [M, N] of a NaN-filled [M + 1, N] buffer"""
    M, N = c["M"], c["N"]
    if x is None:
        x, w = _operands(c)
    buf = torch.full((M + 1, N), NAN, dtype=BF16, device=DEV)
    res = c["Cin"] if c["cin"] else None
    assert res is None or c["beta"] == 1.0
    y = _G().linear_few_rows(x, w, bias=c["bias"], act=c["act"], residual=res, out=buf[:M])
    torch.cuda.synchronize()
    assert y.data_ptr() == buf.data_ptr()
    assert bool(torch.isnan(buf[M]).all()), "a store below the last row"
    assert bool(torch.isfinite(buf[:M]).all()), "a masked row or column reached the output"
    return buf[:M]


def test_plan_reaches_the_named_arms():
    """the extension's launch plan for every (N, K) of the table has the property its line in
    tests/few_rows_cases.py names, covers every chunk, and the table meets every wave count"""
    seen = set()
    for (N, K), arm in FR.ARMS.items():
        W, per = _ext().few_rows_plan(N, K)
        ch, bl = K // 64, -(-N // 16)
        assert 1 <= W <= 16 and W <= ch and W * per >= ch, (N, K, W, per)
        assert arm(W, per, ch, bl), (N, K, W, per)
        seen.add(W)
    assert set(FR.ARMS) == set(FR.SHAPES) and seen == {1, 2, 4, 8, 16}


@pytest.mark.parametrize("shape", FR.SHAPES, ids=FR.shape_id)
def test_against_fp64(shape):
    """M in 1, 2, 7, 8, 15, 16 x both generators x plain, bias_bf16, bias_f32, gelu, bias + residual,
    bias + residual + gelu on one (N, K) of the table, masked operands, guard row"""
    J = U.Judge()
    keep = shape[0] < 4096
    for gen, M, N, K, epi in FR.cases([shape]):
        c, r, t = _case(gen, M, N, K, epi, keep)
        U.judge_gemm(J, "few_rows", "%dx%dx%d %s %s" % (M, N, K, gen, epi), c, r, t, {"C": _run(c)})
    J.check()


@pytest.mark.parametrize("shape", FR.SHAPES, ids=FR.shape_id)
def test_row_invariance_and_determinism(shape):
    """row m of an M = 16 call is bit for bit the M = 1 call on that row (the summation order
    depends on (N, K) alone), for every epilogue; two calls give equal bits"""
    N, K = shape
    J = U.Judge()
    for epi in FR.EPIS:
        c, r, t = _case("randn", 16, N, K, epi, N < 4096)
        x, w = _operands(c)
        y16 = _run(c, x, w)
        assert torch.equal(FR.bits(y16), FR.bits(_run(c, x, w))), "two calls differ"
        for m in (0, 5, 15):
            c1 = dict(c, M=1, Cin=None if c["Cin"] is None else c["Cin"][m:m + 1].contiguous())
            xb = torch.full((16, K), NAN, dtype=BF16, device=DEV)
            xb[0] = c["a"][m]
            y1 = _run(c1, xb[:1], w)
            assert torch.equal(FR.bits(y1[0]), FR.bits(y16[m])), (epi, m)
        U.judge_gemm(J, "few_rows", "16x%dx%d randn %s" % (N, K, epi), c, r, t, {"C": y16})
    J.check()


def test_refused_shapes_raise_before_a_launch():
    """M = 17, K = 96, N = 12, fp32 x, a strided x, and a few more: each raises in the binding (or
    in the op, for the row count) and leaves the output untouched"""
    G = _G()
    mk = lambda *s, dt=BF16: torch.ones(s, dtype=dt, device=DEV)
    out = torch.full((16, 16), NAN, dtype=BF16, device=DEV)

    def refused(x, w, o=None, **kw):
        with pytest.raises((RuntimeError, ValueError, TypeError)):
            G.linear_few_rows(x, w, out=out[: x.shape[0], : w.shape[0]] if o is None else o, **kw)
        with pytest.raises((RuntimeError, ValueError, TypeError)):   # the binding itself, without the op's checks
            _ext().gemm_few_rows(x, w, kw.get("bias"), kw.get("residual"),
                                 torch.full((x.shape[0], w.shape[0]), NAN, dtype=BF16, device=DEV), kw.get("act", 0))
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())

    refused(mk(17, 64), mk(16, 64), o=torch.full((17, 16), NAN, dtype=BF16, device=DEV))   # M = 17
    refused(mk(4, 96), mk(16, 96))                                    # K = 96
    refused(mk(4, 64), mk(12, 64), o=torch.full((4, 12), NAN, dtype=BF16, device=DEV))     # N = 12
    refused(mk(4, 64, dt=F32), mk(16, 64))                            # fp32 x
    refused(mk(4, 128)[:, ::2], mk(16, 64))                           # strided x
    refused(mk(4, 64), mk(16, 64, dt=F32))                            # fp32 w
    refused(mk(4, 64), mk(32, 64)[::2])                               # strided w
    refused(mk(4, 64), mk(16, 128))                                   # K mismatch
    refused(mk(4, 72)[:, 8:], mk(16, 64))                             # x off its rows
    refused(mk(4, 64), mk(16, 64), bias=mk(16, dt=torch.float16))     # bias dtype
    refused(mk(4, 64), mk(16, 64), bias=mk(8))                        # bias length
    refused(mk(4, 64), mk(16, 64), residual=mk(4, 16, dt=F32))        # residual dtype
    refused(mk(4, 64), mk(16, 64), act=1)                             # relu is not an epilogue of this kernel
    with pytest.raises((RuntimeError, ValueError)):                   # out of the wrong shape
        _ext().gemm_few_rows(mk(4, 64), mk(16, 64), None, None, mk(4, 24), 0)
    with pytest.raises((RuntimeError, ValueError)):                   # x only 8-byte aligned
        _ext().gemm_few_rows(mk(4 * 64 + 4)[4:].view(4, 64), mk(16, 64), None, None, mk(4, 16), 0)
