"""KV-cache generation shared by GPT2 and Llama: prefill, one-token decode steps and sampling.

`prefill` is the model's forward over the prompt (ops.causal_attention, dropout off) that also
copies each layer's k|v rows into an ops.KVCache and sends only the last position through the
LM head.  `decode_step` runs one token per batch row: the same GEMMs, norms and fused epilogues
on few rows, with ops.decode_attention in place of the causal attention.  Everything runs under
torch.no_grad().  On the GPU the prompt is right-padded to a multiple of 64 tokens for the flash
kernels (causality keeps the padding out of every real row; only the real rows reach the cache)
and the batch of a decode step to a multiple of 8 rows for the GEMMs.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .. import ops
from ..ops.llama_ops import rope_tables, swiglu_mlp


def _pad_prompt(idx: torch.Tensor) -> torch.Tensor:
    pad = -idx.shape[1] % 64 if idx.is_cuda else 0
    return F.pad(idx, (0, pad)) if pad else idx


def _rows8(x: torch.Tensor) -> torch.Tensor:
    pad = -x.shape[0] % 8 if x.is_cuda else 0
    return F.pad(x, (0, 0, 0, pad)) if pad else x


def _check_prefill(idx, cache, limit, what):
    B, P = idx.shape
    if cache.length != 0:
        raise ValueError("prefill: the cache is not empty (KVCache.reset() first)")
    if B != cache.B or P < 1 or P > cache.Tmax or idx.device != cache.device:
        raise ValueError(f"prefill: prompt {tuple(idx.shape)} on {idx.device} does not fit the cache "
                         f"(B={cache.B}, Tmax={cache.Tmax}) on {cache.device}")
    if P > limit:
        raise ValueError(f"prefill: prompt of {P} tokens exceeds {what}={limit}")


def _finish_prefill(cache, P):
    cache.pos.fill_(P)
    cache.length = P


def _attend(qkv, B, cache, li, n_head, n_kv_head, rope, window, y):
    """decode attention of the B real rows of a (row-padded) qkv; y: the padded destination."""
    if y is None:
        return ops.decode_attention(qkv, cache, li, n_head, n_kv_head, rope=rope, window=window)
    ops.decode_attention(qkv[:B], cache, li, n_head, n_kv_head, rope=rope, window=window, out=y[:B])
    return y


# ---------------------------------------------------------------------------------- GPT-2
@torch.no_grad()
def gpt2_prefill(model, idx: torch.Tensor, cache) -> torch.Tensor:
    c = model.cfg
    _check_prefill(idx, cache, c.n_positions, "n_positions")
    B, P = idx.shape
    x = ops.embedding(_pad_prompt(idx), model.wte, model.wpe)
    win = model.sliding_window or None
    for li, blk in enumerate(model.h):
        h, x = blk.ln_1(x, passthrough=True)
        qkv = blk.attn.c_attn(h)
        cache.fill(li, qkv, c.n_head, P)
        y = ops.causal_attention(qkv, c.n_head, window=win, training=False)
        x = blk.attn.c_proj(y, residual=x)
        h, x = blk.ln_2(x, passthrough=True)
        x = blk.mlp(h, residual=x)
    _finish_prefill(cache, P)
    last = _rows8(x[:, P - 1].contiguous())
    return ops.linear(model.ln_f(last), model.wte)[:B, : c.vocab_size]


@torch.no_grad()
def gpt2_decode_step(model, tok: torch.Tensor, cache) -> torch.Tensor:
    c = model.cfg
    B = tok.shape[0]
    if cache.length >= min(cache.Tmax, c.n_positions):
        raise ValueError(f"decode_step: position {cache.length} is beyond the cache (Tmax={cache.Tmax}) or "
                         f"n_positions={c.n_positions}")
    pos = cache.pos.long()
    if tok.is_cuda:  # the embedding kernel's sum: bf16 tables added in fp32, rounded once
        x = (ops.shadow_of(model.wte)[tok].float() + ops.shadow_of(model.wpe)[pos].float()).to(torch.bfloat16)
    else:
        x = model.wte[tok] + model.wpe[pos]
    x = _rows8(x)
    y = x.new_zeros((x.shape[0], c.n_embd)) if x.shape[0] != B else None
    win = model.sliding_window or None
    for li, blk in enumerate(model.h):
        h, x = blk.ln_1(x, passthrough=True)
        qkv = blk.attn.c_attn(h)
        a = _attend(qkv, B, cache, li, c.n_head, c.n_head, None, win, y)
        x = blk.attn.c_proj(a, residual=x)
        h, x = blk.ln_2(x, passthrough=True)
        x = blk.mlp(h, residual=x)
    cache.advance()
    return ops.linear(model.ln_f(x), model.wte)[:B, : c.vocab_size]


# ---------------------------------------------------------------------------------- Llama
@torch.no_grad()
def llama_prefill(model, idx: torch.Tensor, cache) -> torch.Tensor:
    from ..ops.llama_ops import apply_rope

    c = model.cfg
    _check_prefill(idx, cache, c.max_seq_len, "max_seq_len")
    B, P = idx.shape
    x = ops.embedding(_pad_prompt(idx), model.tok_embeddings)
    win = model.sliding_window or None
    for li, blk in enumerate(model.layers):
        h, x = blk.attention_norm(x, passthrough=True)
        qkv = apply_rope(ops.linear(h, blk.attention.wqkv), c.n_heads, c.n_kv_heads, c.rope_theta)
        cache.fill(li, qkv, c.n_heads, P)
        y = ops.causal_attention(qkv, c.n_heads, c.n_kv_heads, window=win, training=False)
        x = ops.linear(y, blk.attention.wo, residual=x)
        h, x = blk.ffn_norm(x, passthrough=True)
        x = blk.feed_forward(h, residual=x)
    _finish_prefill(cache, P)
    last = _rows8(x[:, P - 1].contiguous())
    return ops.linear(model.norm(last), model.output)[:B, : c.vocab_size]


@torch.no_grad()
def llama_decode_step(model, tok: torch.Tensor, cache) -> torch.Tensor:
    c = model.cfg
    B = tok.shape[0]
    if cache.length >= min(cache.Tmax, c.max_seq_len):
        raise ValueError(f"decode_step: position {cache.length} is beyond the cache (Tmax={cache.Tmax}) or "
                         f"max_seq_len={c.max_seq_len}")
    pad = -B % 8 if tok.is_cuda else 0
    x = ops.embedding(F.pad(tok, (0, pad))[:, None], model.tok_embeddings)[:, 0]
    y = x.new_zeros((x.shape[0], c.n_heads * c.head_dim)) if pad else None
    rope = rope_tables(cache.Tmax, c.head_dim, c.rope_theta, tok.device)
    win = model.sliding_window or None
    for li, blk in enumerate(model.layers):
        h, x = blk.attention_norm(x, passthrough=True)
        qkv = ops.linear(h, blk.attention.wqkv)
        a = _attend(qkv, B, cache, li, c.n_heads, c.n_kv_heads, rope, win, y)
        x = ops.linear(a, blk.attention.wo, residual=x)
        h, x = blk.ffn_norm(x, passthrough=True)
        x = swiglu_mlp(h, blk.feed_forward.w13, blk.feed_forward.w2, x)
    cache.advance()
    return ops.linear(model.norm(x), model.output)[:B, : c.vocab_size]


# ---------------------------------------------------------------------------------- sampling
def new_cache(model, B: int, length: int, device):
    """An ops.KVCache for `length` positions of this model (GPU: rounded up to a multiple of 64)."""
    c = model.cfg
    if hasattr(c, "n_kv_heads"):
        n_layers, Hkv, Dh = c.n_layers, c.n_kv_heads, c.head_dim
    else:
        n_layers, Hkv, Dh = c.n_layer, c.n_head, c.n_embd // c.n_head
    device = torch.device(device)
    Tmax = -(-length // 64) * 64 if device.type == "cuda" else length
    return ops.KVCache(n_layers, B, Tmax, Hkv, Dh, device)


def sample(logits: torch.Tensor, temperature: float, top_k: int | None, gen) -> torch.Tensor:
    """One token per row of logits [B, vocab_size] (padded vocabulary columns already cut off):
    argmax at temperature 0, else a draw from softmax(logits / temperature) over the top_k."""
    if temperature == 0.0:
        return logits.argmax(dim=-1)
    z = logits.float() / temperature
    if top_k is not None and top_k < z.shape[-1]:
        kth = torch.topk(z, top_k, dim=-1).values[:, -1:]
        z = z.masked_fill(z < kth, float("-inf"))
    return torch.multinomial(torch.softmax(z, dim=-1), 1, generator=gen)[:, 0]


@torch.no_grad()
def generate(model, idx: torch.Tensor, max_new_tokens: int, temperature: float = 0.0, top_k: int | None = None,
             seed: int = 0, eos_id: int | None = None) -> torch.Tensor:
    """idx [B, P] -> [B, P + max_new_tokens].  One prefill, then one decode step per token; the
    loop has no host read of device data: a row that emitted eos_id keeps emitting it through a
    device-side mask and there is no early exit."""
    limit = getattr(model.cfg, "n_positions", None) or model.cfg.max_seq_len
    B, P = idx.shape
    N = int(max_new_tokens)
    if N < 0 or temperature < 0.0 or (top_k is not None and top_k < 1):
        raise ValueError("generate: max_new_tokens >= 0, temperature >= 0 and top_k >= 1 expected")
    if P + N > limit:
        raise ValueError(f"generate: prompt {P} + max_new_tokens {N} exceeds the model's {limit} positions")
    if N == 0:
        return idx.clone()
    gen = None
    if temperature != 0.0:
        gen = torch.Generator(device=idx.device)
        gen.manual_seed(int(seed))
    cache = new_cache(model, B, P + N, idx.device)
    out = torch.empty((B, P + N), dtype=idx.dtype, device=idx.device)
    out[:, :P] = idx
    done = torch.zeros(B, dtype=torch.bool, device=idx.device)
    logits = model.prefill(idx, cache)
    for i in range(N):
        tok = sample(logits, float(temperature), top_k, gen).to(idx.dtype)
        if eos_id is not None:
            tok = torch.where(done, torch.full_like(tok, eos_id), tok)
            done = done | (tok == eos_id)
        out[:, P + i] = tok
        if i + 1 < N:
            logits = model.decode_step(tok, cache)
    return out
