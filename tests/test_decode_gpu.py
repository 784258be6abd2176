"""The split-KV decode attention kernel on the GPU: judged per element against fp64, bitwise
properties, guard slabs, unsupported shapes.

The yardstick is tests/decode_ref.py (reference, allowance, twin; tests/test_decode_cpu.py holds
the twin inside the allowance and the mutants outside).  Shapes: Tmax = 320, B = 3 ragged rows
per launch (pos = 0 next to pos = 319), RTDC_DECODE_SPLITS in {1, 2, 5} - with 5 splits pos = 0
leaves four of them empty.  Each head layout prints its WORST line; those of one run are kept in
profiles/decode_bench.md.
"""
import math

import pytest
import torch

from tests import decode_ref as D
from tests import ulp as U

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
_refs: dict = {}


def _ext():
    from ray_torch_distributed_checkpoint_amd.ops._ext import gpu_ext

    return gpu_ext()


def _tables(Dh):
    from ray_torch_distributed_checkpoint_amd.ops.llama_ops import rope_tables

    return rope_tables(D.TMAX, Dh, 500000.0, DEV)


def _case(H, Hkv, Dh, gen, pos, window, rope):
    """inputs (on the GPU), the rotated new row, fp64 reference with its allowance: computed once,
    shared, never modified"""
    from ray_torch_distributed_checkpoint_amd.ops.llama_ops import apply_rope

    key = (H, Hkv, Dh, gen, pos, window, rope)
    if key not in _refs:
        B = len(pos)
        qkv_new, cache = D.decode_inputs(gen, B, D.TMAX, H, Hkv, Dh, dev=DEV)
        rot = qkv_new
        if rope:
            # the rotated row as the existing rope kernel writes it: the new row placed at pos[b]
            full = torch.zeros((B, D.TMAX, qkv_new.shape[1]), dtype=U.BF16, device=DEV)
            full[torch.arange(B), list(pos)] = qkv_new
            rot = apply_rope(full, H, Hkv)[torch.arange(B), list(pos)].contiguous()
        ref = D.decode_ref(D.F64, rot.cpu(), cache.cpu(), pos, H, Hkv, Dh, window)
        twin = D.decode_ref(D.F32, rot.cpu(), cache.cpu(), pos, H, Hkv, Dh, window, twin=True)
        _refs[key] = (qkv_new, cache, rot, ref, twin["out"])
    return _refs[key]


def _launch(qkv_new, cache_init, pos, H, Hkv, Dh, window, rope, nsplit, fill=NAN):
    """One direct launch with out, part and cache as dim-0 slices of NaN-filled buffers; checks the
    guard slabs and returns (out, cache after the call)."""
    B = len(pos)
    Tmax = cache_init.shape[1]
    cbuf = torch.full((B + 2, Tmax, 2 * Hkv * Dh), NAN, dtype=U.BF16, device=DEV)
    cache = cbuf[1:B + 1]
    p = torch.tensor(pos, dtype=torch.int32, device=DEV)
    t = torch.arange(Tmax, device=DEV)
    used = t[None] < p[:, None]
    cache.copy_(torch.where(used[:, :, None], cache_init, torch.full_like(cache_init, fill)))
    obuf = torch.full((B + 2, H * Dh), NAN, dtype=U.BF16, device=DEV)
    n = B * H * nsplit * (Dh + 2)
    pbuf = torch.full((3, n), NAN, dtype=torch.float32, device=DEV)
    cos, sin = _tables(Dh) if rope else (None, None)
    _ext().decode_attn(qkv_new, cache, p, cos, sin, obuf[1:B + 1], pbuf[1], H, Hkv, window or 0, nsplit,
                       1.0 / math.sqrt(Dh))
    torch.cuda.synchronize()
    for name, slab in (("out", obuf[0]), ("out", obuf[B + 1]), ("part", pbuf[0]), ("part", pbuf[2]),
                       ("cache", cbuf[0]), ("cache", cbuf[B + 1])):
        assert bool(torch.isnan(slab).all()), f"guard slab of {name} was written"
    out = obuf[1:B + 1].clone()
    assert bool(torch.isfinite(out.float()).all())
    return out, cache.clone()


@pytest.mark.parametrize("H,Hkv,Dh", D.HEADS, ids=[f"H{h}_Hkv{k}_Dh{d}" for h, k, d in D.HEADS])
def test_decode_per_element(H, Hkv, Dh):
    """every element of out within the allowance of the fp64 reference, for every split count;
    the cache row at pos holds the new k|v (k rotated), every other row is unchanged"""
    J = U.Judge()
    i = 0
    for gen in D.GENS:
        for pos in D.POS_SETS:
            for window in D.WINDOWS:
                rope = bool(i % 2)
                i += 1
                qkv_new, cache0, rot, ref, twin = _case(H, Hkv, Dh, gen, pos, window, rope)
                B = len(pos)
                for ns in D.SPLITS:
                    out, cache = _launch(qkv_new, cache0, pos, H, Hkv, Dh, window, rope, ns)
                    shape = (gen, pos, window, "rope" if rope else "-", ns)
                    J.within("decode_attn", shape, "out", out.cpu(), ref["out"], twin, ref["allow_out"])
                    # the stored row: bits of the rotated k and the untouched v; the rest as it was
                    rows = torch.arange(B, device=DEV)
                    p = torch.tensor(pos, device=DEV)
                    assert torch.equal(cache[rows, p], rot[:, H * Dh:])
                    t = torch.arange(D.TMAX, device=DEV)
                    before = (t[None] < p[:, None])[:, :, None]
                    assert torch.equal(torch.where(before, cache, torch.zeros_like(cache)),
                                       torch.where(before, cache0, torch.zeros_like(cache)))
                    after = (t[None] > p[:, None])[:, :, None].expand_as(cache)
                    assert bool(torch.isnan(cache[after]).all())
    J.check()


@pytest.mark.parametrize("H,Hkv,Dh", [(4, 2, 128), (8, 1, 64)])
def test_decode_bitwise(H, Hkv, Dh):
    """equal bits: a repeated launch; a row of a ragged batch and its own B = 1 launch (split count
    pinned); unused cache rows holding zeros or NaN"""
    for pos, window, rope in (((0, 319, 64), None, True), ((63, 65, 127), 5, False), ((1, 62, 128), 100, True)):
        qkv_new, cache0, _, _, _ = _case(H, Hkv, Dh, "randn", pos, window, rope)
        for ns in D.SPLITS:
            out, cache = _launch(qkv_new, cache0, pos, H, Hkv, Dh, window, rope, ns)
            out2, cache2 = _launch(qkv_new, cache0, pos, H, Hkv, Dh, window, rope, ns)
            assert torch.equal(out, out2) and torch.equal(cache.view(torch.int16), cache2.view(torch.int16))
            outz, cachez = _launch(qkv_new, cache0, pos, H, Hkv, Dh, window, rope, ns, fill=0.0)
            assert torch.equal(out, outz)
            t = torch.arange(D.TMAX, device=DEV)
            upto = (t[None] <= torch.tensor(pos, device=DEV)[:, None])[:, :, None]
            zero = torch.zeros_like(cache)
            assert torch.equal(torch.where(upto, cache, zero), torch.where(upto, cachez, zero))
            for b in range(len(pos)):
                o1, _ = _launch(qkv_new[b:b + 1].contiguous(), cache0[b:b + 1].contiguous(), pos[b:b + 1], H, Hkv, Dh,
                                window, rope, ns)
                assert torch.equal(out[b:b + 1], o1), (pos, b, ns)


def test_decode_operator_and_splits(monkeypatch):
    """ops.decode_attention: the knob reaches the launch, the default split rule runs, and both
    agree with the reference; it does not advance pos"""
    from ray_torch_distributed_checkpoint_amd.ops import KVCache, decode_attention
    from ray_torch_distributed_checkpoint_amd.ops.decode import decode_splits

    H, Hkv, Dh, pos, window = 8, 2, 128, (0, 319, 64), 100
    qkv_new, cache0, rot, ref, _ = _case(H, Hkv, Dh, "randn", pos, window, True)
    for forced in ("", "1", "5", "99"):
        monkeypatch.setenv("RTDC_DECODE_SPLITS", forced or "0")
        ns = decode_splits(3, Hkv, D.TMAX, torch.device(DEV))
        assert ns == (min(int(forced), 5) if forced else 5)   # 4 blocks per CU wanted, 64 keys at least: 5
        kvc = KVCache(2, 3, D.TMAX, Hkv, Dh, DEV)
        kvc.layers[1].copy_(cache0)
        kvc.pos.copy_(torch.tensor(pos, dtype=torch.int32))
        kvc.length = max(pos)
        out = decode_attention(qkv_new, kvc, 1, H, Hkv, rope=_tables(Dh), window=window)
        assert U.allow_err(out.cpu(), ref["out"], ref["allow_out"]) <= 1.0
        assert kvc.pos.tolist() == list(pos) and kvc.length == max(pos)
        assert torch.equal(kvc.layers[1][torch.arange(3), list(pos)], rot[:, H * Dh:])
        assert not bool(kvc.layers[0].any())


def test_decode_unsupported_raises():
    """unsupported shapes raise and do not launch"""
    from ray_torch_distributed_checkpoint_amd.ops import KVCache, decode_attention

    def run(H, Hkv, Dh, Tmax, length=0, dtype=U.BF16, dev=DEV, **kw):
        kvc = KVCache(1, 2, Tmax, Hkv, Dh, DEV)
        kvc.length = length
        x = torch.zeros((2, (H + 2 * Hkv) * Dh), dtype=dtype, device=dev)
        before = kvc.layers[0].clone()
        try:
            return decode_attention(x, kvc, 0, H, Hkv, **kw)
        finally:
            assert torch.equal(kvc.layers[0], before)

    run(2, 1, 64, 64)
    with pytest.raises(ValueError, match="Dh"):
        run(2, 1, 32, 64)
    with pytest.raises(ValueError, match="full"):
        run(2, 1, 64, 64, length=64)
    with pytest.raises(ValueError, match="Tmax"):
        run(2, 1, 64, 100)
    with pytest.raises(ValueError, match="H / Hkv"):
        run(16, 1, 64, 64)
    with pytest.raises(ValueError, match="window"):
        run(2, 1, 64, 64, window=0)
    with pytest.raises(ValueError, match="cache"):
        run(2, 1, 64, 64, dev="cpu", dtype=torch.float32)
    with pytest.raises(ValueError, match="rope"):
        run(2, 1, 64, 64, rope=_tables(128))
    ext = _ext()
    x = torch.zeros((2, 4 * 64), dtype=U.BF16, device=DEV)
    c = torch.zeros((2, 64, 128), dtype=U.BF16, device=DEV)
    p = torch.zeros(2, dtype=torch.int32, device=DEV)
    o = torch.zeros((2, 128), dtype=U.BF16, device=DEV)
    part = torch.zeros(2 * 2 * 66, dtype=torch.float32, device=DEV)
    ext.decode_attn(x, c, p, None, None, o, part, 2, 1, 0, 1, 0.125)
    with pytest.raises(RuntimeError, match="unsupported shape"):   # nsplit beyond Tmax / 64
        ext.decode_attn(x, c, p, None, None, o, torch.zeros(2 * 2 * 2 * 66, device=DEV), 2, 1, 0, 2, 0.125)
    with pytest.raises(RuntimeError, match="part workspace"):
        ext.decode_attn(x, c, p, None, None, o, part[:-1], 2, 1, 0, 1, 0.125)
    with pytest.raises(RuntimeError, match="int32"):
        ext.decode_attn(x, c, p.long(), None, None, o, part, 2, 1, 0, 1, 0.125)
    with pytest.raises(RuntimeError, match="do not match"):
        ext.decode_attn(x, c[:, :, :64].contiguous(), p, None, None, o, part, 2, 1, 0, 1, 0.125)
