"""The FP8 KV cache kernels (csrc/kernels/attn_decode.hip, the e4m3 cache format) on the GPU, on the shapes of
tests/decode_ref.py: the quantising fill and the stored row bit for bit against the CPU formula
(ops.quantize_fp8_rows of the [*, Dh] view), `out` per element against fp64, bitwise properties.

The reference of `out` is decode_ref(F64) on the dequantised cache, the new row dequantised too
(code * scale is exact in fp64), so it already holds the quantised values and the kernel adds no
bf16 term.  Counted from the source as decode_ref's docstring counts, the kernel adds two fp32
roundings to the bf16 cache's: one multiply per score (the group sum times kscale * scale * log2 e,
itself one rounding per key in place of the host's scale * log2 e) and one per key and head
(p * vscale).  That is Dh + 65 and Tmax + 65 terms where decode_ref allows Dh + 64 and Tmax + 64; the
test keeps decode_ref's allowance as it is, the narrower of the two.  WORST lines of one run:
profiles/decode_fp8_kv.md.
"""
import math

import pytest
import torch

from ray_torch_distributed_checkpoint_amd import ops
from tests import decode_ref as D
from tests import ulp as U
from tests.test_decode_gpu import DEV, NAN, _ext, _tables

pytestmark = pytest.mark.gpu

U8, F8 = torch.uint8, torch.float8_e4m3fn
NANB = 0x7F   # the e4m3 NaN byte
IDS = [f"H{h}_Hkv{k}_Dh{d}" for h, k, d in D.HEADS]
_refs: dict = {}


def _quant(x, Dh):
    """the CPU formula on the last axis cut into runs of Dh: (codes as uint8 like x, scales [..., runs])"""
    q, s = ops.quantize_fp8_rows(x.cpu().reshape(-1, Dh).contiguous())
    return q.view(U8).view(x.shape), s.view(*x.shape[:-1], x.shape[-1] // Dh)


def _deq(q, s, Dh):
    return (q.view(F8).float().double().view(*s.shape, Dh) * s.double()[..., None]).view(q.shape)


def _case(H, Hkv, Dh, gen, pos, window, rope):
    """(qkv_new, codes, scales of the cache) on the GPU, (codes, scales) of the rotated new row, the
    fp64 reference on the dequantised values with its allowance, the twin: once, shared, never modified"""
    from ray_torch_distributed_checkpoint_amd.ops.llama_ops import apply_rope

    key = (H, Hkv, Dh, gen, pos, window, rope)
    if key not in _refs:
        B = len(pos)
        qkv_new, cache = D.decode_inputs(gen, B, D.TMAX, H, Hkv, Dh, dev=DEV)
        rot = qkv_new
        if rope:
            full = torch.zeros((B, D.TMAX, qkv_new.shape[1]), dtype=U.BF16, device=DEV)
            full[torch.arange(B), list(pos)] = qkv_new
            rot = apply_rope(full, H, Hkv)[torch.arange(B), list(pos)].contiguous()
        cq, cs = _quant(cache, Dh)
        nq, ns = _quant(rot[:, H * Dh:], Dh)
        new64 = torch.cat([rot[:, : H * Dh].cpu().double(), _deq(nq, ns, Dh)], dim=1)
        ref = D.decode_ref(D.F64, new64, _deq(cq, cs, Dh), pos, H, Hkv, Dh, window)
        twin = D.decode_ref(D.F32, new64, _deq(cq, cs, Dh), pos, H, Hkv, Dh, window, twin=True)["out"]
        _refs[key] = (qkv_new, cq.to(DEV), cs.to(DEV), nq.to(DEV), ns.to(DEV), ref, twin)
    return _refs[key]


def _guarded(B, Tmax, Hkv, Dh):
    """(codes, scales) [B + 2, ...] full of NaN bytes / NaN: rows 1 .. B are the cache, 0 and B + 1 guards"""
    return (torch.full((B + 2, Tmax, 2 * Hkv * Dh), NANB, dtype=U8, device=DEV),
            torch.full((B + 2, Tmax, 2 * Hkv), NAN, dtype=torch.float32, device=DEV))


def _guards_intact(qbuf, sbuf, B):
    return all(bool((qbuf[i] == NANB).all()) and bool(torch.isnan(sbuf[i]).all()) for i in (0, B + 1))


def _launch(qkv_new, cq0, cs0, pos, H, Hkv, Dh, window, rope, nsplit, fill=NANB):
    """one direct launch on guarded buffers, rows at or beyond pos holding `fill` bytes and NaN scales;
    returns (out, codes, scales after the call)"""
    B, Tmax = len(pos), cq0.shape[1]
    qbuf, sbuf = _guarded(B, Tmax, Hkv, Dh)
    p = torch.tensor(pos, dtype=torch.int32, device=DEV)
    used = (torch.arange(Tmax, device=DEV)[None] < p[:, None])[:, :, None]
    qbuf[1:B + 1] = torch.where(used, cq0, torch.full_like(cq0, fill))
    sbuf[1:B + 1] = torch.where(used, cs0, torch.full_like(cs0, NAN))
    obuf = torch.full((B + 2, H * Dh), NAN, dtype=U.BF16, device=DEV)
    pbuf = torch.full((3, B * H * nsplit * (Dh + 2)), NAN, dtype=torch.float32, device=DEV)
    cos, sin = _tables(Dh) if rope else (None, None)
    _ext().decode_attn(qkv_new, qbuf[1:B + 1].view(F8), p, cos, sin, obuf[1:B + 1], pbuf[1],
                       H, Hkv, window or 0, nsplit, 1.0 / math.sqrt(Dh), cache_scale=sbuf[1:B + 1])
    torch.cuda.synchronize()
    assert _guards_intact(qbuf, sbuf, B), "guard slab of the cache was written"
    assert all(bool(torch.isnan(t).all()) for t in (obuf[0], obuf[B + 1], pbuf[0], pbuf[2])), "guard slab written"
    out = obuf[1:B + 1].clone()
    assert bool(torch.isfinite(out.float()).all())
    return out, qbuf[1:B + 1].clone(), sbuf[1:B + 1].clone()


@pytest.mark.parametrize("H,Hkv,Dh", D.HEADS, ids=IDS)
def test_fill_is_the_cpu_formula_bitwise(H, Hkv, Dh):
    """kv_fill_fp8 on rows (1, 63, 64, 320) of a T = 320 prompt, B = 3, into a Tmax = 384 cache: codes
    and scales of the rows below `rows` equal the CPU formula, everything else stays NaN"""
    B, T, Tmax = 3, D.TMAX, D.TMAX + 64
    qkv = U.attn_inputs("randn", B, T, H, Hkv, Dh)["qkv"]
    qkv[1, 0, H * Dh: (H + 1) * Dh] = 0.0   # an all-zero run: scale 1.0
    wq, ws = _quant(qkv[:, :, H * Dh:], Dh)
    assert ws[1, 0, 0].item() == 1.0
    for rows in (1, 63, 64, 320):
        qbuf, sbuf = _guarded(B, Tmax, Hkv, Dh)
        _ext().kv_fill_fp8(qkv.to(DEV), qbuf[1:B + 1].view(F8), sbuf[1:B + 1], H, rows)
        torch.cuda.synchronize()
        assert _guards_intact(qbuf, sbuf, B), "guard slab was written"
        assert torch.equal(qbuf[1:B + 1, :rows].cpu(), wq[:, :rows]), rows
        assert torch.equal(sbuf[1:B + 1, :rows].cpu(), ws[:, :rows]), rows
        assert bool((qbuf[1:B + 1, rows:] == NANB).all()) and bool(torch.isnan(sbuf[1:B + 1, rows:]).all()), rows


@pytest.mark.parametrize("H,Hkv,Dh", D.HEADS, ids=IDS)
def test_decode_per_element_and_stored_row(H, Hkv, Dh):
    """every element of out within decode_ref's allowance for every split count; the bytes and scales
    at pos are the CPU formula on the rotated new row, every other row and scale is unchanged"""
    J = U.Judge()
    i = 0
    for gen in D.GENS:
        for pos in D.POS_SETS:
            for window in D.WINDOWS:
                rope = bool(i % 2)
                i += 1
                qkv_new, cq0, cs0, nq, ns, ref, twin = _case(H, Hkv, Dh, gen, pos, window, rope)
                rows, p = torch.arange(len(pos), device=DEV), torch.tensor(pos, device=DEV)
                keep = (torch.arange(D.TMAX, device=DEV)[None] < p[:, None])[:, :, None]
                for nsplit in D.SPLITS:
                    out, cq, cs = _launch(qkv_new, cq0, cs0, pos, H, Hkv, Dh, window, rope, nsplit)
                    shape = (gen, pos, window, "rope" if rope else "-", nsplit)
                    J.within("decode_fp8kv", shape, "out", out.cpu(), ref["out"], twin, ref["allow_out"])
                    assert torch.equal(cq[rows, p], nq) and torch.equal(cs[rows, p], ns)
                    assert torch.equal(torch.where(keep, cq, 0), torch.where(keep, cq0, 0))
                    assert torch.equal(torch.where(keep, cs, 0.0), torch.where(keep, cs0, 0.0))
                    after = (torch.arange(D.TMAX, device=DEV)[None] > p[:, None])[:, :, None]
                    assert bool((cq[after.expand_as(cq)] == NANB).all())
                    assert bool(torch.isnan(cs[after.expand_as(cs)]).all())
    J.check()


@pytest.mark.parametrize("H,Hkv,Dh", [(4, 2, 128), (8, 1, 64)])
def test_decode_bitwise(H, Hkv, Dh):
    """equal bits: a repeated launch; unused rows holding zero or NaN bytes (NaN scales either way); a
    row of a ragged batch and its own B = 1 launch (split count pinned)"""
    for pos, window, rope in (((0, 319, 64), None, True), ((63, 65, 127), 5, False), ((1, 62, 128), 100, True)):
        qkv_new, cq0, cs0, _, _, _, _ = _case(H, Hkv, Dh, "randn", pos, window, rope)
        for nsplit in D.SPLITS:
            out, cq, cs = _launch(qkv_new, cq0, cs0, pos, H, Hkv, Dh, window, rope, nsplit)
            out2, cq2, cs2 = _launch(qkv_new, cq0, cs0, pos, H, Hkv, Dh, window, rope, nsplit)
            assert torch.equal(out, out2) and torch.equal(cq, cq2) and torch.equal(cs.view(torch.int32), cs2.view(torch.int32))
            assert torch.equal(out, _launch(qkv_new, cq0, cs0, pos, H, Hkv, Dh, window, rope, nsplit, fill=0)[0])
            for b in range(len(pos)):
                o1, _, _ = _launch(qkv_new[b:b + 1].contiguous(), cq0[b:b + 1].contiguous(), cs0[b:b + 1].contiguous(),
                                   pos[b:b + 1], H, Hkv, Dh, window, rope, nsplit)
                assert torch.equal(out[b:b + 1], o1), (pos, b, nsplit)


def test_operator_follows_the_cache_and_refuses_bad_tensors():
    """ops.KVCache(kv_dtype="fp8"): fill and decode_attention reach the FP8 kernels; a cache tensor of
    the wrong dtype or shape is refused in the binding, before a launch"""
    H, Hkv, Dh, pos, window = 8, 2, 128, (63, 65, 127), 100
    qkv_new, cq0, cs0, nq, ns, ref, _ = _case(H, Hkv, Dh, "randn", pos, window, True)
    kvc = ops.KVCache(2, 3, D.TMAX, Hkv, Dh, DEV, kv_dtype="fp8")
    qkv = U.attn_inputs("randn", 3, 64, H, Hkv, Dh)["qkv"].to(DEV)
    kvc.fill(0, qkv, H, 40)
    wq, ws = _quant(qkv[:, :40, H * Dh:], Dh)
    assert torch.equal(kvc.layers[0][:, :40].view(U8).cpu(), wq) and torch.equal(kvc.scales[0][:, :40].cpu(), ws)
    kvc.layers[1].view(U8).copy_(cq0)
    kvc.scales[1].copy_(cs0)
    kvc.pos.copy_(torch.tensor(pos, dtype=torch.int32))
    kvc.length = max(pos)
    out = ops.decode_attention(qkv_new, kvc, 1, H, Hkv, rope=_tables(Dh), window=window)
    assert U.allow_err(out.cpu(), ref["out"], ref["allow_out"]) <= 1.0
    assert torch.equal(kvc.layers[1].view(U8)[torch.arange(3), list(pos)], nq)
    p = kvc.pos
    part = torch.zeros(3 * H * (Dh + 2), dtype=torch.float32, device=DEV)
    o = torch.zeros((3, H * Dh), dtype=U.BF16, device=DEV)
    for bad_q, bad_s in ((cq0, cs0), (cq0.view(F8), cs0.double()), (cq0.view(F8)[:, :, :Dh].contiguous(), cs0),
                         (cq0.view(F8), cs0[:, :64].contiguous())):
        with pytest.raises(RuntimeError, match="cache_q"):
            _ext().decode_attn(qkv_new, bad_q, p, None, None, o, part, H, Hkv, 0, 1, 0.1, cache_scale=bad_s)
        with pytest.raises(RuntimeError, match="cache_q"):
            _ext().kv_fill_fp8(qkv, bad_q, bad_s, H, 1)
    with pytest.raises(RuntimeError, match="needs its cache_scale"):       # an FP8 cache without its scales
        _ext().decode_attn(qkv_new, cq0.view(F8), p, None, None, o, part, H, Hkv, 0, 1, 0.1)
    with pytest.raises(RuntimeError, match="float8_e4m3fn cache_q"):       # a bf16 cache with scales
        _ext().decode_attn(qkv_new, torch.zeros(cq0.shape, dtype=U.BF16, device=DEV), p, None, None, o, part,
                           H, Hkv, 0, 1, 0.1, cache_scale=cs0)
