"""The yardstick of the decode attention kernel and the CPU path of ops.decode_attention.

tests/decode_ref.py: the float32 twin (the kernel's one bf16 rounding in place) has to stay inside
the per-element allowance of the float64 reference on every case the GPU test launches, and two
mutants of the reference have to land outside it - the yardstick has teeth.  The CPU path of
`decode_attention` has to agree with row `pos` of `causal_attention_ref` over pos + 1 tokens.
"""
import pytest
import torch

from tests import decode_ref as D
from tests import ulp as U


@pytest.mark.parametrize("H,Hkv,Dh", D.HEADS, ids=[f"H{h}_Hkv{k}_Dh{d}" for h, k, d in D.HEADS])
def test_twin_inside_the_allowance(H, Hkv, Dh):
    J = U.Judge()
    for gen in D.GENS:
        q, c = D.decode_inputs(gen, 3, D.TMAX, H, Hkv, Dh)
        for pos in D.POS_SETS:
            for window in D.WINDOWS:
                ref = D.decode_ref(D.F64, q, c, pos, H, Hkv, Dh, window)
                twin = D.decode_ref(D.F32, q, c, pos, H, Hkv, Dh, window, twin=True)
                assert bool((ref["allow_out"] > 0).all())
                J.within("decode_attn", (gen, pos, window), "out", None, ref["out"], twin["out"], ref["allow_out"])
    J.check()


@pytest.mark.parametrize("mutant,pos,window", [("own_key_dropped", (1, 62, 128), None),
                                               ("own_key_dropped", (63, 65, 127), 64),
                                               ("window_off_by_one", (62, 128, 319), 5),
                                               ("window_off_by_one", (65, 127, 128), 64)])
def test_mutants_leave_the_allowance(mutant, pos, window):
    """randn inputs, where every key in range carries weight: the mutant moves most elements of
    every row by more than the allowance"""
    for H, Hkv, Dh in ((4, 2, 128), (8, 1, 64)):
        q, c = D.decode_inputs("randn", 3, D.TMAX, H, Hkv, Dh)
        ref = D.decode_ref(D.F64, q, c, pos, H, Hkv, Dh, window)
        bad = D.decode_ref(D.F64, q, c, pos, H, Hkv, Dh, window, mutant=mutant)["out"]
        over = (bad - ref["out"]).abs() > ref["allow_out"]
        assert bool((over.float().mean(dim=1) > 0.5).all()), over.float().mean(dim=1)
        assert U.allow_err(bad, ref["out"], ref["allow_out"]) > 10.0


def test_nan_outside_the_range_changes_nothing():
    q, c = D.decode_inputs("randn", 3, D.TMAX, 4, 2, 128)
    pos, window = (5, 64, 200), 64
    ref = D.decode_ref(D.F64, q, c, pos, 4, 2, 128, window)
    dirty = c.clone()
    t = torch.arange(D.TMAX)
    p = torch.tensor(pos)
    outside = (t[None] >= p[:, None]) | (t[None] < (p - window + 1)[:, None])
    dirty[outside] = float("nan")
    got = D.decode_ref(D.F64, q, dirty, pos, 4, 2, 128, window)
    assert torch.equal(got["out"], ref["out"]) and torch.equal(got["allow_out"], ref["allow_out"])


def test_split_ranges_cover_the_cache():
    for Tmax in (64, 320, 8192):
        for ns in (1, 2, 5, Tmax // 64):
            if ns <= Tmax // 64:
                r = D.split_ranges(Tmax, ns)
                keys = [k for a, b in r for k in range(a, b)]
                assert keys == list(range(Tmax)) and all(a % 64 == 0 for a, _ in r)


@pytest.mark.parametrize("H,Hkv,Dh", [(4, 2, 16), (2, 2, 8), (8, 1, 64)])
@pytest.mark.parametrize("window", [None, 1, 5])
@pytest.mark.parametrize("rope", [False, True])
def test_cpu_path_matches_causal_attention(H, Hkv, Dh, window, rope):
    """token by token: decode_attention on a growing cache == the last row of the causal
    attention over the tokens so far (after apply_rope when the tables are given), fp32"""
    from ray_torch_distributed_checkpoint_amd.ops import KVCache, decode_attention
    from ray_torch_distributed_checkpoint_amd.ops.attention import causal_attention_ref
    from ray_torch_distributed_checkpoint_amd.ops.llama_ops import apply_rope, rope_tables

    B, T = 2, 12
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(B, T, (H + 2 * Hkv) * Dh, generator=g)
    cache = KVCache(1, B, T, Hkv, Dh, "cpu")
    cache.layers[0].fill_(float("nan"))          # rows not yet written must not matter
    tables = rope_tables(T, Dh, 500000.0, "cpu") if rope else None
    full = apply_rope(qkv, H, Hkv) if rope else qkv
    for t in range(T):
        out = decode_attention(qkv[:, t].contiguous(), cache, 0, H, Hkv, rope=tables, window=window)
        w = window if window is not None and window < t + 1 else None
        want = causal_attention_ref(full[:, : t + 1], B, t + 1, H, Hkv, Dh, window=w)[:, t]
        assert torch.allclose(out, want, rtol=1e-5, atol=1e-6), (t, (out - want).abs().max())
        assert torch.equal(cache.layers[0][:, t], full[:, t, H * Dh:])
        assert cache.length == t and cache.pos.tolist() == [t] * B
        cache.advance()
    with pytest.raises(ValueError, match="full"):
        decode_attention(qkv[:, 0].contiguous(), cache, 0, H, Hkv, rope=tables, window=window)


def test_cpu_path_ragged_and_errors():
    from ray_torch_distributed_checkpoint_amd.ops import KVCache, decode_attention

    H, Hkv, Dh = 4, 2, 64
    q, c = D.decode_inputs("randn", 3, 64, H, Hkv, Dh)
    pos = (0, 63, 17)
    cache = KVCache(1, 3, 64, Hkv, Dh, "cpu")
    cache.layers[0].copy_(c.float())
    cache.pos.copy_(torch.tensor(pos, dtype=torch.int32))
    cache.length = max(pos)
    out = decode_attention(q.float(), cache, 0, H, Hkv, window=20)
    ref = D.decode_ref(D.F64, q, c, pos, H, Hkv, Dh, 20)
    assert U.allow_err(out, ref["out"], ref["allow_out"]) <= 1.0
    with pytest.raises(ValueError, match="window"):
        decode_attention(q.float(), cache, 0, H, Hkv, window=0)
    with pytest.raises(ValueError, match="does not match the cache"):
        decode_attention(q.float()[:2], cache, 0, H, Hkv)
    with pytest.raises(ValueError, match="the cache"):
        decode_attention(q, cache, 0, H, Hkv)          # bf16 rows, fp32 cache
    with pytest.raises(ValueError, match="qkv_new must be"):
        decode_attention(q.float(), cache, 0, 3, 2)
