"""The FP8 (e4m3) KV cache on the CPU: `KVCache(kv_dtype="fp8")`, its `fill`, the row store and the
math of `decode_attention`, and `generate(kv_cache="fp8")`.

The contract: the cache viewed as [B Tmax 2 Hkv, Dh] is ops.quantize_fp8_rows of the bf16 / fp32 cache
in the same view, bit for bit (k after RoPE), and the step attends to code * scale, the new key included.
"""
import pytest
import torch

from ray_torch_distributed_checkpoint_amd import ops
from ray_torch_distributed_checkpoint_amd.generate import build_model
from ray_torch_distributed_checkpoint_amd.models.generation import new_cache
from ray_torch_distributed_checkpoint_amd.ops.llama_ops import rope_tables

U8 = torch.uint8


@pytest.mark.parametrize("H,Hkv,Dh,rope", [(2, 2, 16, False), (4, 2, 64, True), (8, 1, 128, True)])
def test_fill_and_row_store_are_quantize_fp8_rows(H, Hkv, Dh, rope):
    B, T, Tmax, rows = 3, 9, 12, 7
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn((B, T + 1, (H + 2 * Hkv) * Dh), generator=g)
    qkv[1, 2, H * Dh: (H + 1) * Dh] = 0.0                       # an all-zero k head
    tables = rope_tables(Tmax, Dh, 500000.0, "cpu") if rope else None
    plain = ops.KVCache(1, B, Tmax, Hkv, Dh)                    # the fp32 cache: the values to quantise
    cache = ops.KVCache(1, B, Tmax, Hkv, Dh, kv_dtype="fp8")
    assert cache.layers[0].dtype == torch.float8_e4m3fn and cache.scales[0].shape == (B, Tmax, 2 * Hkv)
    for c in (plain, cache):
        c.fill(0, qkv[:, :T], H, rows)
        c.pos.fill_(rows)
        c.length = rows
    q, s = ops.quantize_fp8_rows(plain.layers[0][:, :rows].reshape(-1, Dh).contiguous())
    assert torch.equal(cache.layers[0][:, :rows].reshape(-1, Dh).view(U8), q.view(U8))
    assert torch.equal(cache.scales[0][:, :rows].reshape(-1), s)
    assert cache.scales[0][1, 2, 0].item() == 1.0 and not bool(cache.layers[0][1, 2, :Dh].view(U8).any())
    assert not bool(cache.layers[0][:, rows:].view(U8).any())   # rows >= rows: untouched

    new = qkv[:, T].contiguous()
    before = cache.layers[0].view(U8).clone()
    ops.decode_attention(new, plain, 0, H, Hkv, rope=tables)    # stores the rotated fp32 row
    out = ops.decode_attention(new, cache, 0, H, Hkv, rope=tables, window=5)
    q, s = ops.quantize_fp8_rows(plain.layers[0][:, rows].reshape(-1, Dh).contiguous())
    assert torch.equal(cache.layers[0][:, rows].reshape(-1, Dh).view(U8), q.view(U8))
    assert torch.equal(cache.scales[0][:, rows].reshape(-1), s)
    after = cache.layers[0].view(U8).clone()
    after[:, rows] = before[:, rows]
    assert torch.equal(after, before)                           # every other row unchanged
    # the output: plain attention over code * scale, the new key through its code too
    deq = ops.KVCache(1, B, Tmax, Hkv, Dh)
    deq.layers[0].copy_((cache.layers[0].float().view(B, Tmax, 2 * Hkv, Dh) * cache.scales[0][..., None]).flatten(2))
    deq.pos.fill_(rows)
    deq.length = rows
    rot = new.clone()
    if rope:  # the q heads rotated at pos, as the step rotates them
        from ray_torch_distributed_checkpoint_amd.ops.decode import _rotate_new
        rot = _rotate_new(new, deq.pos, H, Hkv, Dh, tables).reshape(B, -1).clone()
    rot[:, H * Dh:] = deq.layers[0][:, rows]
    assert torch.equal(out, ops.decode_attention(rot, deq, 0, H, Hkv, window=5))


@pytest.mark.parametrize("name", ["gpt2-tiny", "llama3-tiny"])
def test_generate_with_an_fp8_cache_runs(name):
    torch.manual_seed(0)
    model = build_model(name, "cpu").eval()
    idx = torch.randint(0, model.cfg.vocab_size, (2, 5))
    out = model.generate(idx, 4, kv_cache="fp8")
    assert out.shape == (2, 9) and torch.equal(out[:, :5], idx) and int(out.max()) < model.cfg.vocab_size
    assert torch.equal(out, model.generate(idx, 4, kv_cache="fp8", few_row=True, weights="bf16"))
    assert model.generate(idx, 4, kv_cache="fp8", few_row=True, weights="fp8").shape == (2, 9)
    assert new_cache(model, 2, 9, "cpu", kv_cache="fp8").kv_dtype == "fp8"
    assert new_cache(model, 2, 9, "cpu").scales is None


def test_a_bad_kv_cache_raises():
    model = build_model("gpt2-tiny", "cpu").eval()
    idx = torch.zeros((1, 3), dtype=torch.int64)
    with pytest.raises(ValueError, match="kv_cache"):
        model.generate(idx, 2, kv_cache="int8")
    with pytest.raises(ValueError, match="kv_cache"):
        new_cache(model, 1, 8, "cpu", kv_cache="fp16")
    with pytest.raises(ValueError, match="kv_dtype"):
        ops.KVCache(1, 1, 8, 1, 16, kv_dtype="e5m2")
