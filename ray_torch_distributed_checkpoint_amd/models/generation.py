"""KV-cache generation shared by GPT2 and Llama: prefill, one-token decode steps and sampling.

`prefill` is the model's forward over the prompt (ops.causal_attention, dropout off) that also
copies each layer's k|v rows into an ops.KVCache and sends only the last position through the
LM head.  `decode_step` runs one token per batch row: the same GEMMs, norms and fused epilogues
on few rows, with ops.decode_attention in place of the causal attention.  Everything runs under
torch.no_grad().  On the GPU the prompt is right-padded to a multiple of 64 tokens for the flash
kernels (causality keeps the padding out of every real row; only the real rows reach the cache)
and the batch of a decode step to a multiple of 8 rows for the GEMMs.

Two switches, both off by default (a call without them runs the code above unchanged):
`few_row=True` sends every linear of a decode step, and the last-position LM head of the prefill,
to ops.linear_few_rows on the B real rows (B <= 16; no row padding); `CapturedDecode` /
`generate(captured=True)` records one decode step as a hipGraph and replays it per token.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .. import ops
from ..ops import gemm as G
from ..ops._ext import gpu_ext
from ..ops.llama_ops import rope_tables, swiglu_mlp


def _pad_prompt(idx: torch.Tensor) -> torch.Tensor:
    pad = -idx.shape[1] % 64 if idx.is_cuda else 0
    return F.pad(idx, (0, pad)) if pad else idx


def _rows8(x: torch.Tensor) -> torch.Tensor:
    pad = -x.shape[0] % 8 if x.is_cuda else 0
    return F.pad(x, (0, 0, 0, pad)) if pad else x


def _check_few_row(B: int) -> None:
    if B > G.FEW_ROWS_MAX:
        raise ValueError(f"few_row=True takes at most {G.FEW_ROWS_MAX} batch rows, got {B}")


def _few(x, w, bias=None, act=G.ACT_NONE, residual=None):
    """one linear of a few-row decode step: the weight's bf16 shadow through ops.linear_few_rows"""
    return G.linear_few_rows(x, ops.shadow_of(w), bias=bias, act=act, residual=residual)


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
def gpt2_prefill(model, idx: torch.Tensor, cache, few_row: bool = False) -> torch.Tensor:
    c = model.cfg
    _check_prefill(idx, cache, c.n_positions, "n_positions")
    B, P = idx.shape
    if few_row:
        _check_few_row(B)
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
    if few_row and idx.is_cuda:
        return _few(model.ln_f(x[:, P - 1].contiguous()), model.wte)[:, : c.vocab_size]
    last = _rows8(x[:, P - 1].contiguous())
    return ops.linear(model.ln_f(last), model.wte)[:B, : c.vocab_size]


@torch.no_grad()
def gpt2_decode_step(model, tok: torch.Tensor, cache, few_row: bool = False) -> torch.Tensor:
    c = model.cfg
    B = tok.shape[0]
    if few_row:
        _check_few_row(B)
    if cache.length >= min(cache.Tmax, c.n_positions):
        raise ValueError(f"decode_step: position {cache.length} is beyond the cache (Tmax={cache.Tmax}) or "
                         f"n_positions={c.n_positions}")
    pos = cache.pos.long()
    if tok.is_cuda:  # the embedding kernel's sum: bf16 tables added in fp32, rounded once
        x = (ops.shadow_of(model.wte)[tok].float() + ops.shadow_of(model.wpe)[pos].float()).to(torch.bfloat16)
    else:
        x = model.wte[tok] + model.wpe[pos]
    if few_row and tok.is_cuda:
        return _gpt2_decode_few(model, x, cache)
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


def _gpt2_decode_few(model, x, cache):
    """the decode step on the B real rows: five few-row linears per block and the LM head"""
    c = model.cfg
    win = model.sliding_window or None
    for li, blk in enumerate(model.h):
        h, x = blk.ln_1(x, passthrough=True)
        qkv = _few(h, blk.attn.c_attn.weight, blk.attn.c_attn.bias)
        a = ops.decode_attention(qkv, cache, li, c.n_head, c.n_head, rope=None, window=win)
        x = _few(a, blk.attn.c_proj.weight, blk.attn.c_proj.bias, residual=x)
        h, x = blk.ln_2(x, passthrough=True)
        g = _few(h, blk.mlp.c_fc.weight, blk.mlp.c_fc.bias, act=G.ACT_GELU)
        x = _few(g, blk.mlp.c_proj.weight, blk.mlp.c_proj.bias, residual=x)
    cache.advance()
    return _few(model.ln_f(x), model.wte)[:, : c.vocab_size]


# ---------------------------------------------------------------------------------- Llama
@torch.no_grad()
def llama_prefill(model, idx: torch.Tensor, cache, few_row: bool = False) -> torch.Tensor:
    from ..ops.llama_ops import apply_rope

    c = model.cfg
    _check_prefill(idx, cache, c.max_seq_len, "max_seq_len")
    B, P = idx.shape
    if few_row:
        _check_few_row(B)
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
    if few_row and idx.is_cuda:
        return _few(model.norm(x[:, P - 1].contiguous()), model.output)[:, : c.vocab_size]
    last = _rows8(x[:, P - 1].contiguous())
    return ops.linear(model.norm(last), model.output)[:B, : c.vocab_size]


@torch.no_grad()
def llama_decode_step(model, tok: torch.Tensor, cache, few_row: bool = False) -> torch.Tensor:
    c = model.cfg
    B = tok.shape[0]
    if few_row:
        _check_few_row(B)
    if cache.length >= min(cache.Tmax, c.max_seq_len):
        raise ValueError(f"decode_step: position {cache.length} is beyond the cache (Tmax={cache.Tmax}) or "
                         f"max_seq_len={c.max_seq_len}")
    if few_row and tok.is_cuda:
        return _llama_decode_few(model, tok, cache)
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


def _llama_decode_few(model, tok, cache):
    """the decode step on the B real rows: wqkv, wo, w13 (then the swiglu_fwd launch), w2, output"""
    c = model.cfg
    x = ops.embedding(tok[:, None], model.tok_embeddings)[:, 0]
    rope = rope_tables(cache.Tmax, c.head_dim, c.rope_theta, tok.device)
    win = model.sliding_window or None
    for li, blk in enumerate(model.layers):
        h, x = blk.attention_norm(x, passthrough=True)
        qkv = _few(h, blk.attention.wqkv)
        a = ops.decode_attention(qkv, cache, li, c.n_heads, c.n_kv_heads, rope=rope, window=win)
        x = _few(a, blk.attention.wo, residual=x)
        h, x = blk.ffn_norm(x, passthrough=True)
        gu = _few(h, blk.feed_forward.w13)
        hh = torch.empty((gu.shape[0], gu.shape[1] // 2), dtype=torch.bfloat16, device=gu.device)
        gpu_ext().swiglu_fwd(gu, hh)
        x = _few(hh, blk.feed_forward.w2, residual=x)
    cache.advance()
    return _few(model.norm(x), model.output)[:, : c.vocab_size]


# ---------------------------------------------------------------------------------- captured decode
class CapturedDecode:
    """One decode step of `model` on `cache`, recorded once as a hipGraph and replayed per token.

        sess = CapturedDecode(model, cache, few_row=True)     # after model.prefill(idx, cache)
        logits = sess.step(tok)                               # [B, vocab_size], static: use it
                                                              # before the next step

    The step was written for this: the key splits never depend on the position, `cache.pos` lives
    on the device and the captured step ends with `pos += 1`, so one capture serves every later
    position and every later prompt on the same cache (`cache.reset()`, `prefill`, `step` again).
    `cache.length`, the host's copy, is checked against Tmax and the model's position limit and
    bumped by `step`; at the limit `step` raises before any replay.

    Construction runs one eager step on the "capture" side stream (lazy allocations, shadows, rope
    tables), then captures on that stream: one chain, no fork inside.  It then puts `cache.pos` and
    `cache.length` back: they and every cache row below `length` keep their bits; the warm-up leaves
    its k|v row at position `length`, which the first real step overwrites before any read.  A full
    cache cannot be warmed up and is refused.

    What the graph bakes in, and how `step` guards it:
    * `model.sliding_window` and `few_row` are recorded; `step` raises if either differs.
    * the addresses of every parameter and of every bf16 weight shadow.  ops.shadow_of refreshes a
      stale shadow in place (same storage), but only when it is called, and a replay calls nothing:
      `step` compares every parameter's version counter and, where one moved (load_state_dict, a
      torch optimizer), refreshes the shadow on the current stream before the replay.  A shadow's
      storage can be replaced (shadow_of after a device or shape change, ops.shadow.bind_shadow of
      a flat optimizer buffer) and so can a parameter's (`p.data = ...`): `step` raises then, and a
      new session has to be built.  The fused optimizers write master and shadow in the same kernel
      pass without a version bump: the guard does not see such an update and does not need to,
      since both storages are the ones the graph reads and nothing is left to refresh.
      The guard is one pass over the parameters on the host per step (three attribute reads each;
      its measured cost is in profiles/decode_fast.md) and runs while the previous replay executes.
    """

    def __init__(self, model, cache, few_row: bool = False):
        if not (torch.cuda.is_available() and cache.device.type == "cuda"):
            raise RuntimeError("CapturedDecode: hipGraph capture needs the model and the cache on a GPU")
        from ..ops.streams import side_stream

        self.model, self.cache, self.few_row = model, cache, bool(few_row)
        self.window = model.sliding_window or None
        self.limit = min(cache.Tmax, getattr(model.cfg, "n_positions", None) or model.cfg.max_seq_len)
        if few_row:
            _check_few_row(cache.B)
        if cache.length >= self.limit:
            raise ValueError(f"CapturedDecode: the cache is full ({cache.length} of {self.limit} positions): "
                             f"nothing to warm up on")
        dev = cache.device
        self.tok = torch.zeros(cache.B, dtype=torch.int64, device=dev)
        length0, pos0 = cache.length, cache.pos.clone()
        cur = torch.cuda.current_stream(dev)
        side = side_stream(dev, "capture")
        try:
            with torch.no_grad():
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    model.decode_step(self.tok, cache, few_row=self.few_row)
                cur.wait_stream(side)
                cache.pos.copy_(pos0)      # the capture below sees the position it was built at
                cache.length = length0
                torch.cuda.synchronize(dev)
                self.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph, stream=side):
                    self.logits = model.decode_step(self.tok, cache, few_row=self.few_row)
        finally:
            cache.pos.copy_(pos0)
            cache.length = length0
        self._guard = [(p, p._version, p.data_ptr(), getattr(p, "_rtdc_shadow", None)) for p in model.parameters()]
        self._shadow_ptrs = [None if s is None else s.data_ptr() for _, _, _, s in self._guard]
        self.replays = 0

    def _check_weights(self) -> None:
        for i, (p, ver, ptr, s) in enumerate(self._guard):
            if p._version == ver and getattr(p, "_rtdc_shadow", None) is s and p.data_ptr() == ptr:
                continue
            if p.data_ptr() != ptr:
                raise RuntimeError("CapturedDecode: a parameter's storage was replaced after capture; "
                                   "build a new session")
            if s is not None and (ops.shadow_of(p) is not s or s.data_ptr() != self._shadow_ptrs[i]):
                raise RuntimeError("CapturedDecode: a weight shadow's storage was replaced after capture; "
                                   "build a new session")
            self._guard[i] = (p, p._version, ptr, s)

    def step(self, tok: torch.Tensor) -> torch.Tensor:
        c = self.cache
        if (self.model.sliding_window or None) != self.window:
            raise RuntimeError(f"CapturedDecode: model.sliding_window changed after capture "
                               f"({self.window} -> {self.model.sliding_window}); build a new session")
        if tok.shape != self.tok.shape:
            raise ValueError(f"CapturedDecode.step: tok must be [{c.B}], got {tuple(tok.shape)}")
        if c.length >= self.limit:
            raise ValueError(f"decode_step: position {c.length} is beyond the cache (Tmax={c.Tmax}) or the "
                             f"model's position limit ({self.limit})")
        self._check_weights()
        self.tok.copy_(tok)
        self.graph.replay()
        c.length += 1
        self.replays += 1
        return self.logits


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
             seed: int = 0, eos_id: int | None = None, few_row: bool = False, captured: bool = False) -> torch.Tensor:
    """idx [B, P] -> [B, P + max_new_tokens].  One prefill, then one decode step per token; the
    loop has no host read of device data: a row that emitted eos_id keeps emitting it through a
    device-side mask and there is no early exit.
    few_row: the decode linears and the prefill's LM head on ops.linear_few_rows (B <= 16; on the
    CPU the reference math is the same either way).  captured (GPU only): the decode step is
    replayed from a CapturedDecode built on this call's cache; sampling and the eos mask stay
    eager, on the same generator, so the tokens are those of the eager loop."""
    limit = getattr(model.cfg, "n_positions", None) or model.cfg.max_seq_len
    B, P = idx.shape
    N = int(max_new_tokens)
    if N < 0 or temperature < 0.0 or (top_k is not None and top_k < 1):
        raise ValueError("generate: max_new_tokens >= 0, temperature >= 0 and top_k >= 1 expected")
    if P + N > limit:
        raise ValueError(f"generate: prompt {P} + max_new_tokens {N} exceeds the model's {limit} positions")
    if few_row:
        _check_few_row(B)
    if captured and not idx.is_cuda:
        raise ValueError("generate: captured=True needs the GPU (a hipGraph replays the decode step)")
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
    logits = model.prefill(idx, cache, few_row=few_row)
    sess = CapturedDecode(model, cache, few_row=few_row) if captured and N > 1 else None
    for i in range(N):
        tok = sample(logits, float(temperature), top_k, gen).to(idx.dtype)
        if eos_id is not None:
            tok = torch.where(done, torch.full_like(tok, eos_id), tok)
            done = done | (tok == eos_id)
        out[:, P + i] = tok
        if i + 1 < N:
            logits = sess.step(tok) if sess is not None else model.decode_step(tok, cache, few_row=few_row)
    return out
