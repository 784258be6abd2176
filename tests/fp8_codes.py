"""The OCP e4m3 code space, written out: what tests/test_fp8_codes_cpu.py and tests/test_fp8_codes_gpu.py
hold the three quantising sites (quant_fp8_rows_kernel, kv_fill_fp8_kernel, the decode owner's
KvFp8::store_new) and the three widening sites (fp8_widen2 into the few-row MFMA and into the decode
score, cvt_pk_f32_fp8 for V) of csrc/kernels/fp8.h against.  Pure torch, importable without a GPU.

Nothing here goes through `.to(torch.float8_e4m3fn)`: the 256 decoded values are computed from the bit
fields and `rne_e4m3` picks the nearest of them.  The CPU test then shows that torch's cast agrees on
`boundary_values`, so the two references check each other.

A byte is s eeee mmm: e = 0 is the subnormal m * 2^-9, e > 0 is (1 + m / 8) * 2^(e - 7), 0x7F and 0xFF
are NaN, there is no infinity, the largest magnitude is 448 (0x7E).

FP8_MUTANTS are deliberate errors of the reference, in the manner of DECODE_MUTANTS: the CPU test
shows that the comparisons of the GPU test reject every one of them.
"""
from __future__ import annotations

import torch

F64, F32, BF16, U8 = torch.float64, torch.float32, torch.bfloat16, torch.uint8
NANB = 0x7F
QUANT_MUTANTS = ("half_away", "truncate", "subnormal_quotient_flushed", "zero_sign_dropped")
WIDEN_MUTANTS = ("subnormal_widened_zero",)
FP8_MUTANTS = QUANT_MUTANTS + WIDEN_MUTANTS
ANCHOR_JS = (-20, -3, 0, 5, 100)   # scales 2^j of the anchored runs: tiny, small, one, large, huge
# row maxima of `tiny_rows`: fp32 rows whose amax / 448 underflows to zero (1e-44), is a subnormal
# fp32 (5e-43 .. 1.2e-38, the last with a normal maximum), is just normal (6e-36), and a row near the
# top of fp32 (3e38)
TINY_MAXIMA = (1e-44, 5e-43, 1e-41, 1.2e-38, 6e-36, 3e38)
BF16_MIN_SUBNORMAL = 2.0 ** -133


def _decoded():
    b = torch.arange(256)
    e, m = (b >> 3) & 15, (b & 7).double()
    mag = torch.where(e == 0, m * 2.0 ** -9, (1 + m / 8) * torch.ldexp(torch.ones(256, dtype=F64), e - 7))
    v = torch.where(b >= 128, -mag, mag)
    v[(b & 0x7F) == 0x7F] = float("nan")
    return v


E4M3_VALUES = _decoded()                         # [256] float64, 0x7F and 0xFF NaN
_POS = E4M3_VALUES[:127].clone()                 # the finite non-negative values, ascending with the code
FINITE_CODES = torch.tensor([b for b in range(256) if b & 0x7F != 0x7F], dtype=U8)   # [254]
SUBNORMAL_CODES = torch.tensor(list(range(8)) + list(range(0x80, 0x88)), dtype=U8)   # [16], the zeros included


def widen(codes: torch.Tensor, mutant: str = "") -> torch.Tensor:
    """uint8 codes -> their float64 values (NaN codes NaN).  mutant "subnormal_widened_zero": the
    codes 0x01 .. 0x07 and 0x81 .. 0x87 give zero."""
    assert mutant == "" or mutant in WIDEN_MUTANTS
    v = E4M3_VALUES[codes.long()]
    if mutant == "subnormal_widened_zero":
        v = torch.where((codes & 0x78) == 0, torch.zeros_like(v), v)
    return v


def rne_e4m3(x64: torch.Tensor, mutant: str = "") -> torch.Tensor:
    """float64 -> the uint8 code of the nearest finite e4m3 value; a tie goes to the even code; the
    sign is kept, on a zero result too; |x| >= 464 (half a step beyond 448) and NaN give the NaN code
    0x7F.  (No quotient of the project's formula exceeds 448 (1 + 2^-23), so nothing judged here depends
    on the convention at and above 464.)  `mutant`: one of QUANT_MUTANTS."""
    assert mutant == "" or mutant in QUANT_MUTANTS
    x = x64.double()
    a = x.abs()
    lo = (torch.searchsorted(_POS, a.nan_to_num(nan=0.0).contiguous(), right=True) - 1).clamp(0, 126)
    hi = (lo + 1).clamp_max(126)
    mid = (_POS[lo] + _POS[hi]) / 2              # exact: neighbours differ in the last of 3 mantissa bits
    up = (a > mid) | ((a == mid) & (lo % 2 == 1))
    if mutant == "half_away":
        up = a >= mid
    if mutant == "truncate":
        up = torch.zeros_like(up)
    code = torch.where(up, hi, lo)
    if mutant == "subnormal_quotient_flushed":
        code = torch.where(a < 2.0 ** -6, torch.zeros_like(code), code)
    neg = torch.signbit(x)
    if mutant == "zero_sign_dropped":
        neg = neg & (code != 0)
    code = code + 128 * neg.long()
    code = torch.where((a >= 464) | torch.isnan(x), torch.full_like(code, NANB), code)
    return code.to(U8)


def _step(v: torch.Tensor, up: bool) -> torch.Tensor:
    """the neighbour of every non-negative v one place of its own dtype up, or down (below zero: the
    smallest negative subnormal)"""
    it = torch.int32 if v.dtype == F32 else torch.int16
    bits = v.contiguous().view(it).clone()
    if up:
        return (bits + 1).view(v.dtype)
    zero = bits == 0
    bits = torch.where(zero, torch.full_like(bits, torch.iinfo(it).min + 1), bits - 1)
    return bits.view(v.dtype)


def boundary_values(dtype) -> torch.Tensor:
    """Where a quantiser can go wrong, as exact values of `dtype` (fp32 or bf16): the 127 finite
    non-negative code values, the 126 midpoints of two neighbours (2^-10, half the smallest subnormal and
    a tie to zero, is the first of them), and each of those 253 one place of `dtype` up and down, |v| <=
    448; then all of it negated.  758 + 758 = 1516 values (0 - one place is already negative, so the
    smallest subnormal of `dtype` appears twice with either sign)."""
    assert dtype in (F32, BF16)
    exact = torch.cat([_POS, (_POS[:-1] + _POS[1:]) / 2])
    pts = exact.to(dtype)
    assert torch.equal(pts.double(), exact)
    v = torch.cat([pts, _step(pts, True), _step(pts, False)])
    v = v[v.double().abs() <= 448]
    return torch.cat([v, -v])


def anchored_runs(values: torch.Tensor, run: int, j, multiple: int = 1):
    """`values` (exact in their dtype, |v| <= 448) packed into runs of length `run`: run r holds run - 1
    of them times 2^j and one anchor, +448 * 2^j (r even) or -448 * 2^j (r odd) at element (7 r + 3) % run,
    so its maximum is 448 * 2^j, its scale exactly 2^j and every quotient exact.  j: an int, or a
    sequence that the runs cycle through.  The values are repeated from the start to fill the last run
    and to make the number of runs a multiple of `multiple`.
    Returns (w [runs, run] in the dtype of `values`, codes uint8 [runs, run], scales fp32 [runs]): the
    expected codes are rne_e4m3 of what a run holds over 2^j (the value itself, or a zero of its sign
    where the value times 2^j underflowed), the expected scale is 2^j."""
    js = (j,) if isinstance(j, int) else tuple(j)
    n = -(-values.numel() // (run - 1))
    n = -(-n // multiple) * multiple
    pay = values.repeat(-(-n * (run - 1) // values.numel()))[: n * (run - 1)].view(n, run - 1)
    jr = torch.tensor([js[r % len(js)] for r in range(n)])
    two_j = torch.ldexp(torch.ones(n, dtype=F64), jr)
    w = torch.empty((n, run), dtype=F64)
    for r in range(n):
        at = (7 * r + 3) % run
        w[r, :at], w[r, at + 1:] = pay[r, :at].double(), pay[r, at:].double()
        w[r, at] = -448.0 if r % 2 else 448.0
    w = (w * two_j[:, None]).to(values.dtype)    # a power of two: exact unless it underflows
    assert bool((w.double().abs().amax(1) == 448 * two_j).all())
    return w, rne_e4m3(w.double() / two_j[:, None]), two_j.to(F32)


def tiny_rows(K: int):
    """[(name, w [1, K])]: one fp32 row per TINY_MAXIMA, holding every finite e4m3 value / 448 times the
    maximum (rounded to fp32) and the maximum itself with either sign; one bf16 row of 0 and +-2^-133, the
    smallest bf16 subnormal"""
    frac = (E4M3_VALUES[FINITE_CODES.long()] / 448).repeat(-(-K // 254))[:K]
    rows = []
    for m in TINY_MAXIMA:
        w = (frac * m).to(F32)
        w[0], w[K - 1] = m, -m
        rows.append((f"fp32_{m:g}", w.view(1, K)))
    w = (torch.arange(K) % 3 - 1).double() * BF16_MIN_SUBNORMAL
    rows.append(("bf16_min_subnormal", w.to(BF16).view(1, K)))
    assert rows[-1][1].double().abs().max().item() == BF16_MIN_SUBNORMAL
    return rows


def check_tiny(w: torch.Tensor, codes: torch.Tensor, scale: torch.Tensor) -> None:
    """what holds for any finite row: finite codes, a finite scale > 0; where the scale is a normal
    fp32 number, |code * scale - w| <= half the e4m3 spacing at |w| / scale, times the scale, plus one
    fp32 rounding of the quotient (2^-24 |w|).  The spacing at a quotient t is 2^(max(floor(log2 t), -6) - 3),
    in the top binade (t >= 256, the quotient of the maximum may pass 448 by one rounding) 32."""
    assert bool((codes & 0x7F != NANB).all()), "a NaN code"
    s = scale.double()
    assert bool(torch.isfinite(s).all()) and bool((s > 0).all()), scale
    for r in range(w.shape[0]):
        if s[r].item() < 2.0 ** -126:
            continue
        w64 = w[r].double()
        t = w64.abs() / s[r]
        _, e = torch.frexp(t)                    # t = m 2^e, m in [0.5, 1): floor(log2 t) = e - 1 (t = 0: e = 0)
        e = torch.where(t == 0, torch.full_like(e, -100), e)
        spacing = torch.ldexp(torch.ones_like(t), (e - 1).clamp(-6, 8) - 3)
        err = (widen(codes[r]) * s[r] - w64).abs()
        assert bool((err <= 0.5 * spacing * s[r] + 2.0 ** -24 * w64.abs()).all()), (r, err.max().item())


def code_cache(kind: str, B: int, Tmax: int, Hkv: int, Dh: int, seed: int = 0):
    """An FP8 KV cache given directly, not by quantising: (codes uint8 [B, Tmax, 2 Hkv Dh], scales fp32
    [B, Tmax, 2 Hkv]).  "codes": uniform over the 254 finite bytes, scales 2^-8 (1 + u); "subnormal":
    uniform over 0x00 .. 0x07 and 0x80 .. 0x87, scales 64 (1 + u); u uniform in [0, 1)."""
    pool, base = {"codes": (FINITE_CODES, 2.0 ** -8), "subnormal": (SUBNORMAL_CODES, 64.0)}[kind]
    g = torch.Generator().manual_seed(8191 * seed + 127 * Dh + 31 * Hkv + 7 * B + len(kind))
    codes = pool[torch.randint(0, pool.numel(), (B, Tmax, 2 * Hkv * Dh), generator=g)]
    scales = (base * (1 + torch.rand((B, Tmax, 2 * Hkv), generator=g, dtype=F64))).to(F32)
    return codes, scales


def dequant(codes: torch.Tensor, scales: torch.Tensor, Dh: int, mutant: str = "") -> torch.Tensor:
    """code * scale in float64 (exact), runs of Dh on the last axis of `codes`, one scale each"""
    return (widen(codes, mutant).view(*scales.shape, Dh) * scales.double()[..., None]).view(codes.shape)


def quant_runs(x: torch.Tensor, Dh: int, mutant: str = ""):
    """The project's formula on the last axis cut into runs of Dh, from this file's table:
    scale = amax / 448 as an fp32 division (1.0 where that is not > 0), code = rne_e4m3 of the fp32
    quotient.  (codes uint8 like x, scales fp32 [..., runs])"""
    r = x.float().reshape(-1, Dh)
    amax = r.abs().amax(dim=1)
    s = amax / torch.full_like(amax, 448.0)
    s = torch.where(s > 0, s, torch.ones_like(s))
    return (rne_e4m3((r / s[:, None]).double(), mutant).view(x.shape),
            s.view(*x.shape[:-1], x.shape[-1] // Dh))


def decode_code_case(kind, rot, H, Hkv, Dh, pos, window, Tmax, seed=0):
    """One decode case on a `code_cache`: rot is the new token's row (bf16, rotated where RoPE applies),
    its k and v heads quantised by the CPU formula (ops.quantize_fp8_rows).  Returns (codes, scales) of the
    cache, (codes, scales) of the new row, decode_ref(F64) on the dequantised values with its allowance
    as it stands, and the fp32 twin's `out`."""
    from ray_torch_distributed_checkpoint_amd import ops
    from tests import decode_ref as D

    B = len(pos)
    cq, cs = code_cache(kind, B, Tmax, Hkv, Dh, seed)
    nq, ns = ops.quantize_fp8_rows(rot[:, H * Dh:].reshape(-1, Dh).contiguous())
    nq, ns = nq.view(U8).view(B, 2 * Hkv * Dh), ns.view(B, 2 * Hkv)
    new64 = torch.cat([rot[:, : H * Dh].double(), dequant(nq, ns, Dh)], dim=1)
    kv64 = dequant(cq, cs, Dh)
    ref = D.decode_ref(D.F64, new64, kv64, pos, H, Hkv, Dh, window)
    twin = D.decode_ref(D.F32, new64, kv64, pos, H, Hkv, Dh, window, twin=True)["out"]
    return cq, cs, nq, ns, ref, twin


# ---- the few-row linear on one-hot rows: every code in every byte lane of the weight
FEW_ROWS_N = 256
FEW_ROWS_SCALES = (2.0 ** -3, 1.0, 2.0 ** 5)


def few_rows_codes(K: int):
    """q[n, k] = FINITE_CODES[(n + k) % 254] (uint8 [256, K]) and scale[n] cycling through 2^-3, 1, 2^5:
    column k of q holds every finite code, so every code passes through every byte position of a lane's
    loads."""
    n, k = torch.arange(FEW_ROWS_N)[:, None], torch.arange(K)[None]
    scale = torch.tensor([FEW_ROWS_SCALES[i % 3] for i in range(FEW_ROWS_N)], dtype=F32)
    return FINITE_CODES[(n + k) % 254], scale


def one_hot_rows(K: int, k0: int) -> torch.Tensor:
    """x bf16 [16, K]: row m is 1.0 at k0 + m"""
    x = torch.zeros((16, K), dtype=BF16)
    x[torch.arange(16), k0 + torch.arange(16)] = 1.0
    return x


def few_rows_expected(q: torch.Tensor, scale: torch.Tensor, k0: int, mutant: str = "") -> torch.Tensor:
    """y[m, n] = value(q[n, k0 + m]) * scale[n], float64 [16, N]: a 3-bit mantissa times a power of two,
    exact in bf16"""
    return (widen(q[:, k0:k0 + 16], mutant) * scale.double()[:, None]).t().contiguous()


# ---- decode: one cached key that takes all the weight, its V run holding every code
def v_codes_case(H: int, Hkv: int = 4, Dh: int = 64, pos=(1, 64, 130, 319), Tmax: int = 320):
    """Window 2, no RoPE: row b attends to the cached key pos[b] - 1 and to the new token.  The cached
    key's K run is 0x7E (448) throughout at scale 2^-6, so k = 7; the new token has q = 4 and k = -7
    everywhere (quantised: scale 2^-6 exactly, code 0xFE).  The scores are +-Dh * 28 / sqrt(Dh) = +-224,
    646 apart in the log2 domain, so the new key's weight 2^-646 is exactly 0 in fp32 and l = 1.  The cached
    key's V run of (b, kv-head) holds FINITE_CODES[(64 b + e + kvh) % 254] at a power-of-two scale, the new v
    is zero: out[b, h, e] = value * vscale exactly.  Every other cache row holds NaN bytes and NaN scales.
    Returns (qkv_new bf16, codes, scales, expected out float64 [B, H Dh])."""
    B, G = len(pos), H // Hkv
    codes = torch.full((B, Tmax, 2 * Hkv * Dh), NANB, dtype=U8)
    scales = torch.full((B, Tmax, 2 * Hkv), float("nan"), dtype=F32)
    b, kvh, e = torch.arange(B)[:, None, None], torch.arange(Hkv)[None, :, None], torch.arange(Dh)[None, None]
    vcode = FINITE_CODES[(64 * b + e + kvh) % 254]                                   # [B, Hkv, Dh]
    vscale = torch.ldexp(torch.ones((B, Hkv), dtype=F32), (3 * torch.arange(B)[:, None] + torch.arange(Hkv)[None]) % 7 - 3)
    for i, p in enumerate(pos):
        codes[i, p - 1, : Hkv * Dh] = 0x7E
        codes[i, p - 1, Hkv * Dh:] = vcode[i].reshape(-1)
        scales[i, p - 1, :Hkv] = 2.0 ** -6
        scales[i, p - 1, Hkv:] = vscale[i]
    qkv_new = torch.cat([torch.full((B, H * Dh), 4.0), torch.full((B, Hkv * Dh), -7.0), torch.zeros((B, Hkv * Dh))], 1)
    want = (widen(vcode) * vscale.double()[..., None]).repeat_interleave(G, dim=1).reshape(B, H * Dh)
    return qkv_new.to(BF16), codes, scales, want
