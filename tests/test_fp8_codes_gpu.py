"""Every e4m3 code through every FP8 site of the generation path on the GPU (csrc/kernels/fp8.h and its
users), against tests/fp8_codes.py; tests/test_fp8_codes_cpu.py holds the reference and shows that these
comparisons reject its mutants.

Quantising sites, bit for bit on the rounding boundaries (every code value, every midpoint of two neighbours,
one place of the source type either side, both signs, in runs whose scale is exactly a power of two):
quant_fp8_rows_kernel, kv_fill_fp8_kernel and the decode owner's KvFp8::store_new; tiny rows, whose scale
underflows.  Widening sites, exact numbers for all 254 finite codes: fp8_widen2 into the few-row MFMA (one-hot
x rows, every byte lane), cvt_pk_f32_fp8 for V (one cached key with all the weight); then fp8_widen2 into the
decode score and V again on caches of given codes, judged per element against decode_ref in fp64.

The per-element test keeps decode_ref's allowance as it stands (Dh + 64 and Tmax + 64 terms where the FP8 kernel,
counted from its source in tests/test_decode_fp8kv_gpu.py, has Dh + 65 and Tmax + 65).  WORST lines of one run, the
plans reached and the tiny-row results: profiles/fp8_code_space.md.
"""
import pytest
import torch

from ray_torch_distributed_checkpoint_amd import ops
from tests import decode_ref as D
from tests import fp8_codes as C
from tests import ulp as U
from tests.test_decode_fp8kv_gpu import _guarded, _guards_intact, _launch
from tests.test_decode_gpu import DEV, NAN, _ext

pytestmark = pytest.mark.gpu

F32, BF16, U8, FP8 = C.F32, C.BF16, C.U8, torch.float8_e4m3fn
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
K_ROWS = 1536   # quant_fp8_rows_kernel: a full step of 64 lanes x 16 elements and one of 32 lanes
_cases: dict = {}


def _gpu_quant(w):
    """ops.quantize_fp8_rows into storage followed by a NaN row and a NaN scale, which must keep their bits"""
    N, K = w.shape
    qbuf = torch.full((N + 1, K), C.NANB, dtype=U8, device=DEV)
    sbuf = torch.full((N + 1,), NAN, dtype=F32, device=DEV)
    ops.quantize_fp8_rows(w.to(DEV), out=(qbuf[:N].view(FP8), sbuf[:N]))
    torch.cuda.synchronize()
    assert bool((qbuf[N] == C.NANB).all()) and bool(torch.isnan(sbuf[N])), "a store beyond the last row"
    return qbuf[:N].cpu(), sbuf[:N].cpu()


def _same_bits(s, want):
    return torch.equal(s.view(torch.int32), want.view(torch.int32))


def _rolled(v):
    """the boundary values five times, each copy started elsewhere: every value meets several lanes and byte
    positions, and the rows fill one block of four and start a second"""
    return torch.cat([v.roll(311 * i) for i in range(5)])


@DTYPES
@pytest.mark.parametrize("j", C.ANCHOR_JS, ids=lambda j: f"j{j}")
def test_quantize_rows_on_every_boundary(j, dtype):
    w, codes, scales = C.anchored_runs(_rolled(C.boundary_values(dtype)), K_ROWS, j)
    assert w.shape == (5, K_ROWS)
    q, s = _gpu_quant(w)
    assert _same_bits(s, scales) and torch.equal(q, codes)


@DTYPES
def test_quantize_rows_off_the_boundaries(dtype):
    """the same rows times 1.37 (rounded to the source type): no quotient is exact any more; the CPU formula"""
    w, _, _ = C.anchored_runs(_rolled(C.boundary_values(dtype)), K_ROWS, C.ANCHOR_JS)
    w = (w.float() * 1.37).to(dtype)
    want_q, want_s = ops.quantize_fp8_rows(w)
    q, s = _gpu_quant(w)
    assert _same_bits(s, want_s) and torch.equal(q, want_q.view(U8))


@pytest.mark.parametrize("name,w", C.tiny_rows(K_ROWS), ids=[n for n, _ in C.tiny_rows(K_ROWS)])
def test_quantize_tiny_rows(name, w):
    """finite codes and a finite scale > 0 whatever the maximum, and the CPU formula's bits"""
    q, s = _gpu_quant(w)
    print(f"TINY {name:<20s} scale {s.item():.9g} largest |code| {C.widen(q).abs().max().item():g}")
    C.check_tiny(w, q, s)
    want_q, want_s = ops.quantize_fp8_rows(w)
    assert _same_bits(s, want_s) and torch.equal(q, want_q.view(U8))


def _kv_runs(Dh):
    """the boundary values in bf16 as anchored runs of Dh (a multiple of 8 of them), the scales cycling through
    ANCHOR_JS: once, shared by the fill and the owner test, never modified"""
    if Dh not in _cases:
        _cases[Dh] = C.anchored_runs(C.boundary_values(BF16), Dh, C.ANCHOR_JS, multiple=8)
    return _cases[Dh]


@pytest.mark.parametrize("Dh", [64, 128])
def test_kv_fill_on_every_boundary(Dh):
    """kv_fill_fp8 on a packed bf16 qkv [2, T, (H + 2 Hkv) Dh], H = 3, Hkv = 2, whose k|v tails are the runs:
    codes and scales bit for bit; the q heads hold NaN and are never read; guard slabs and rows >= T intact"""
    B, H, Hkv = 2, 3, 2
    w, codes, scales = _kv_runs(Dh)
    T = w.shape[0] // (2 * Hkv * B)
    qkv = torch.full((B, T, (H + 2 * Hkv) * Dh), NAN, dtype=BF16)
    qkv[:, :, H * Dh:] = w.view(B, T, 2 * Hkv * Dh)
    qbuf, sbuf = _guarded(B, T + 1, Hkv, Dh)
    _ext().kv_fill_fp8(qkv.to(DEV), qbuf[1:B + 1].view(FP8), sbuf[1:B + 1], H, T)
    torch.cuda.synchronize()
    assert _guards_intact(qbuf, sbuf, B), "guard slab was written"
    assert bool((qbuf[1:B + 1, T] == C.NANB).all()) and bool(torch.isnan(sbuf[1:B + 1, T]).all())
    assert torch.equal(qbuf[1:B + 1, :T].cpu(), codes.view(B, T, 2 * Hkv * Dh))
    assert _same_bits(sbuf[1:B + 1, :T].cpu().contiguous(), scales.view(B, T, 2 * Hkv))


@pytest.mark.parametrize("Dh", [64, 128])
def test_decode_owner_stores_every_boundary(Dh):
    """The runs as the k and v heads of qkv_new (H = Hkv = 2, q = 0, no RoPE), one launch for all rows, pos
    spread over the cache: with nsplit = 5 the owner is split 0 for some rows and a later split for others.
    The bytes and the two scales stored at pos are the expectation; every other row and scale is untouched.
    `out` is not looked at."""
    H = Hkv = 2
    w, codes, scales = _kv_runs(Dh)
    B = w.shape[0] // (2 * Hkv)
    spread = (0, 319, 64, 130, 200, 63, 5)
    pos = tuple(spread[b % len(spread)] for b in range(B))
    assert {p // 64 for p in pos} >= {0, 1, 4}
    qkv_new = torch.cat([torch.zeros((B, H * Dh), dtype=BF16), w.view(B, 2 * Hkv * Dh)], dim=1).to(DEV)
    cq0 = torch.zeros((B, D.TMAX, 2 * Hkv * Dh), dtype=U8, device=DEV)          # the rows below pos: zero codes, scale 1
    cs0 = torch.ones((B, D.TMAX, 2 * Hkv), dtype=F32, device=DEV)
    rows, p = torch.arange(B, device=DEV), torch.tensor(pos, device=DEV)
    t = torch.arange(D.TMAX, device=DEV)[None]
    for nsplit in (1, 5):
        _, cq, cs = _launch(qkv_new, cq0, cs0, pos, H, Hkv, Dh, None, False, nsplit)
        assert torch.equal(cq[rows, p].cpu(), codes.view(B, 2 * Hkv * Dh)), nsplit
        assert _same_bits(cs[rows, p].cpu().contiguous(), scales.view(B, 2 * Hkv)), nsplit
        below, above = (t < p[:, None])[:, :, None], (t > p[:, None])[:, :, None]
        assert not bool(torch.where(below, cq, 0).any()) and bool((torch.where(below, cs, 1.0) == 1.0).all())
        assert bool((cq[above.expand_as(cq)] == C.NANB).all()) and bool(torch.isnan(cs[above.expand_as(cs)]).all())


def _few_rows(q, scale, x):
    """one call with q followed by a row of NaN bytes, scale by a NaN, and y inside a NaN-filled [17, N] buffer"""
    N, K = q.shape
    qbuf = torch.full((N + 1, K), C.NANB, dtype=U8, device=DEV)
    qbuf[:N] = q.to(DEV)
    sbuf = torch.full((N + 1,), NAN, dtype=F32, device=DEV)
    sbuf[:N] = scale.to(DEV)
    ybuf = torch.full((17, N), NAN, dtype=BF16, device=DEV)
    y = ops.linear_few_rows_fp8(x.to(DEV), qbuf[:N].view(FP8), sbuf[:N], out=ybuf[:16])
    torch.cuda.synchronize()
    assert y.data_ptr() == ybuf.data_ptr() and bool(torch.isnan(ybuf[16]).all()), "a store below the last row"
    return ybuf[:16].cpu()


@pytest.mark.parametrize("K,many_waves", [(128, False), (384, True)], ids=["K128_W1", "K384_W2"])
def test_few_rows_widens_every_code_in_every_byte_lane(K, many_waves):
    """x is 16 one-hot rows at k0 .. k0 + 15, k0 swept over K; column k of q holds every finite code: y[m, n] is
    value(q[n, k0 + m]) * scale[n] as a number, no tolerance.  K = 128 is one chunk on one wave; K = 384 is
    three chunks on two waves (2 + 1) and the LDS combine.  Then one NaN byte: its whole column is NaN (0 x NaN)."""
    T, W, per = _ext().few_rows_fp8_plan(C.FEW_ROWS_N, K)
    print(f"PLAN few_rows_fp8 N {C.FEW_ROWS_N} K {K}: T {T} W {W} per {per}")
    assert (W > 1) == many_waves and (T, W, per) == ((1, 2, 2) if many_waves else (1, 1, 1))
    q, scale = C.few_rows_codes(K)
    for k0 in range(0, K, 16):
        y = _few_rows(q, scale, C.one_hot_rows(K, k0))
        assert torch.equal(y.double(), C.few_rows_expected(q, scale, k0)), k0
    k0 = K - 32
    q[37, k0 + 9] = C.NANB
    y = _few_rows(q, scale, C.one_hot_rows(K, k0)).double()
    want = C.few_rows_expected(q, scale, k0)
    assert bool(torch.isnan(y[:, 37]).all())
    keep = torch.arange(C.FEW_ROWS_N) != 37
    assert torch.equal(y[:, keep], want[:, keep])


@pytest.mark.parametrize("H", [4, 8])
def test_decode_widens_every_v_code_exactly(H):
    """tests/fp8_codes.py v_codes_case: one cached key carries weight exactly 1 and its V runs hold every finite
    code; out = value * vscale as numbers for 1, 2 and 5 splits (pos = 64: the key and the owner in two splits)"""
    Hkv, Dh, pos = 4, 64, (1, 64, 130, 319)
    qkv_new, codes, scales, want = C.v_codes_case(H, Hkv, Dh, pos, D.TMAX)
    for nsplit in D.SPLITS:
        out, _, _ = _launch(qkv_new.to(DEV), codes.to(DEV), scales.to(DEV), pos, H, Hkv, Dh, 2, False, nsplit)
        assert torch.equal(out.cpu().double(), want), nsplit


def _code_case(kind, H, Hkv, Dh, pos, window, rope):
    """a case of tests/fp8_codes.py decode_code_case, the new row rotated by the rope kernel where RoPE is on"""
    from ray_torch_distributed_checkpoint_amd.ops.llama_ops import apply_rope

    B = len(pos)
    qkv_new, _ = D.decode_inputs("randn", B, D.TMAX, H, Hkv, Dh, dev=DEV)
    rot = qkv_new
    if rope:
        full = torch.zeros((B, D.TMAX, qkv_new.shape[1]), dtype=BF16, device=DEV)
        full[torch.arange(B), list(pos)] = qkv_new
        rot = apply_rope(full, H, Hkv)[torch.arange(B), list(pos)].contiguous()
    cq, cs, nq, ns, ref, twin = C.decode_code_case(kind, rot.cpu(), H, Hkv, Dh, pos, window, D.TMAX)
    return qkv_new, cq.to(DEV), cs.to(DEV), nq.to(DEV), ns.to(DEV), ref, twin


@pytest.mark.parametrize("H,Hkv,Dh", [(4, 2, 128), (8, 1, 64), (12, 12, 64)])
def test_decode_per_element_on_the_code_space(H, Hkv, Dh):
    """test_decode_per_element_and_stored_row's loop on caches of given codes: all 254 finite bytes, and the 16
    subnormal ones alone (where a widening that flushed them would leave `out` zero)"""
    J = U.Judge()
    i = 0
    for kind in ("codes", "subnormal"):
        for pos in D.POS_SETS:
            for window in D.WINDOWS:
                rope = bool(i % 2)
                i += 1
                qkv_new, cq0, cs0, nq, ns, ref, twin = _code_case(kind, H, Hkv, Dh, pos, window, rope)
                rows, p = torch.arange(len(pos), device=DEV), torch.tensor(pos, device=DEV)
                for nsplit in D.SPLITS:
                    out, cq, cs = _launch(qkv_new, cq0, cs0, pos, H, Hkv, Dh, window, rope, nsplit)
                    shape = (kind, pos, window, "rope" if rope else "-", nsplit)
                    J.within("decode_codes", shape, "out", out.cpu(), ref["out"], twin, ref["allow_out"])
                    assert torch.equal(cq[rows, p], nq) and torch.equal(cs[rows, p], ns)
    J.check()
