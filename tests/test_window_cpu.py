"""Sliding-window attention without a GPU: the band semantics of `causal_attention(window=)` on
the CPU path (alone and with documents), the argument checks, the receptive field of the tiny
models with `sliding_window`, and exact resume of the LM workloads with a window on."""
import json
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LENGTHS = [5, 35, 1, 1, 54]


def _heads(qkv, H, Hkv, Dh):
    B, T, _ = qkv.shape
    C = H * Dh
    q = qkv[..., :C].reshape(B, T, H, Dh)
    k = qkv[..., C:C + Hkv * Dh].reshape(B, T, Hkv, Dh).repeat_interleave(H // Hkv, dim=2)
    v = qkv[..., C + Hkv * Dh:].reshape(B, T, Hkv, Dh).repeat_interleave(H // Hkv, dim=2)
    return q, k, v


@pytest.mark.parametrize("W", [1, 17, 96, 200])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (4, 2)])
def test_window_is_attention_over_the_last_w_keys(H, Hkv, W):
    """Row by row: softmax over the keys max(0, t - W + 1) .. t, nothing else."""
    from ray_torch_distributed_checkpoint_amd.ops import causal_attention

    torch.manual_seed(0)
    B, T, Dh = 2, 96, 16
    qkv = torch.randn(B, T, (H + 2 * Hkv) * Dh)
    out = causal_attention(qkv, H, Hkv, window=W).reshape(B, T, H, Dh)
    q, k, v = _heads(qkv, H, Hkv, Dh)
    for t in range(T):
        lo = max(0, t - W + 1)
        s = torch.einsum("bhd,bkhd->bhk", q[:, t], k[:, lo:t + 1]) / math.sqrt(Dh)
        ref = torch.einsum("bhk,bkhd->bhd", torch.softmax(s, dim=-1), v[:, lo:t + 1])
        assert torch.allclose(out[:, t], ref, atol=1e-5, rtol=1e-5), t


@pytest.mark.parametrize("W", [96, 97, 200])
def test_window_of_the_whole_row_is_plain_causal(W):
    """W >= T masks nothing: the result of window=None, exactly - without and with documents."""
    from ray_torch_distributed_checkpoint_amd.ops import DocLayout, causal_attention

    torch.manual_seed(1)
    H, Hkv, Dh, T = 4, 2, 16, 96
    qkv = torch.randn(2, T, (H + 2 * Hkv) * Dh)
    assert torch.equal(causal_attention(qkv, H, Hkv, window=W), causal_attention(qkv, H, Hkv))
    docs = DocLayout.from_lengths([LENGTHS, [T]], T)
    assert torch.equal(causal_attention(qkv, H, Hkv, docs=docs, window=W), causal_attention(qkv, H, Hkv, docs=docs))


@pytest.mark.parametrize("W", [1, 17, 40])
def test_window_with_docs_is_sdpa_under_both_masks(W):
    from ray_torch_distributed_checkpoint_amd.ops import DocLayout, causal_attention

    torch.manual_seed(2)
    H, Hkv, Dh, T, B = 4, 2, 16, 96, 2
    qkv = torch.randn(B, T, (H + 2 * Hkv) * Dh)
    docs = DocLayout.from_lengths([LENGTHS, [T]], T)
    out = causal_attention(qkv, H, Hkv, docs=docs, window=W)
    t = torch.arange(T)
    band = (t[None, :] <= t[:, None]) & (t[None, :] >= t[:, None] - W + 1)
    q, k, v = (x.transpose(1, 2) for x in _heads(qkv, H, Hkv, Dh))
    ref = F.scaled_dot_product_attention(q, k, v, attn_mask=(docs.mask() & band[None])[:, None])
    assert torch.allclose(out, ref.transpose(1, 2).reshape(B, T, H * Dh), atol=1e-5, rtol=1e-5)
    # both masks bite: neither one alone gives this result (at W = 1 a row sees itself alone,
    # which no document can narrow)
    assert not torch.allclose(out, causal_attention(qkv, H, Hkv, docs=docs), atol=1e-3)
    assert W == 1 or not torch.allclose(out, causal_attention(qkv, H, Hkv, window=W), atol=1e-3)


@pytest.mark.parametrize("W", [0, -1, -64])
def test_window_below_one_is_an_error(W):
    from ray_torch_distributed_checkpoint_amd.ops import causal_attention

    with pytest.raises(ValueError, match="window"):
        causal_attention(torch.randn(1, 64, 3 * 2 * 16), 2, window=W)


def _model(name, **kw):
    from ray_torch_distributed_checkpoint_amd.models import GPT2, GPT2Config, Llama, LlamaConfig

    torch.manual_seed(0)
    if name.startswith("llama"):
        cfg = LlamaConfig.named(name)
        return cfg, Llama(cfg, **kw), cfg.n_layers
    cfg = GPT2Config.named(name)
    return cfg, GPT2(cfg, **kw), cfg.n_layer


@pytest.mark.parametrize("name", ["gpt2-tiny", "llama3-tiny"])
def test_model_receptive_field(name):
    """With sliding_window = W a layer moves information at most W - 1 positions, so the logits at
    position t depend on the tokens t - L (W - 1) .. t alone.  Without the window they see all."""
    W, T = 8, 64
    cfg, net, L = _model(name, sliding_window=W)
    assert net.sliding_window == W and "sliding_window" not in "".join(net.state_dict())
    reach = L * (W - 1)
    t0 = 40  # positions >= t0 must not see the tokens before t0 - reach
    torch.manual_seed(1)
    idx = torch.randint(0, cfg.vocab_size, (2, T))
    idx2 = idx.clone()
    idx2[:, : t0 - reach] = torch.randint(0, cfg.vocab_size, (2, t0 - reach))
    with torch.no_grad():
        a, b = net(idx), net(idx2)
        assert torch.equal(a[:, t0:], b[:, t0:])
        assert not torch.equal(a[:, t0 - reach - 1], b[:, t0 - reach - 1])  # (an edited position itself)
        net.sliding_window = None  # a plain attribute, settable later
        a, b = net(idx), net(idx2)
        assert not torch.equal(a[:, t0:], b[:, t0:])
        assert all(not torch.equal(a[:, t], b[:, t]) for t in range(t0, T))


def _losses(result_path) -> dict:
    out = {}
    for line in open(os.path.join(result_path, "result.json")):
        row = json.loads(line)
        for i, v in enumerate(reversed(row["losses"])):
            out[row["step"] - i] = v
    return out


@pytest.mark.parametrize("model", ["llama3-tiny", "gpt2-tiny"])
def test_workload_with_window_resumes_exactly(tmp_path, monkeypatch, model):
    from ray_torch_distributed_checkpoint_amd import workloads as W

    monkeypatch.setenv("RTDC_FORCE_CPU", "1")

    def fit(name, steps, **kw):
        return W.train_workload(model, steps=steps, num_workers=1, ckpt_every_n_steps=2, sliding_window=16,
                                checkpoint_storage_path=str(tmp_path / name), verbose=0, **kw)

    full = _losses(fit("full", 4).path)
    assert sorted(full) == [1, 2, 3, 4] and all(torch.isfinite(torch.tensor(v)) for v in full.values())
    first = fit("first", 2)
    rest = _losses(fit("rest", 4, checkpoint=first.checkpoint, resume_mode="exact").path)
    assert _losses(first.path) == {k: full[k] for k in (1, 2)}
    assert rest == {k: full[k] for k in (3, 4)}
    # the window does change what is computed
    plain = W.train_workload(model, steps=1, num_workers=1, ckpt_every_n_steps=2,
                             checkpoint_storage_path=str(tmp_path / "plain"), verbose=0)
    assert _losses(plain.path)[1] != full[1]


def test_workload_window_argument():
    from ray_torch_distributed_checkpoint_amd import workloads as W

    assert W.WorkloadConfig(model="gpt2-tiny").sliding_window is None
    with pytest.raises(ValueError, match="sliding_window"):
        W.train_workload("gpt2-tiny", steps=1, num_workers=1, sliding_window=-3, verbose=0)
