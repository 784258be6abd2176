"""Packed sequences through the whole model on the GPU: Llama (document mask + per-document RoPE
positions) and GPT-2 (document mask; learned positions stay absolute)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

B, T, LENGTHS = 2, 128, [50, 78]


def _model(name):
    from ray_torch_distributed_checkpoint_amd.models import GPT2, GPT2Config, Llama, LlamaConfig

    torch.manual_seed(0)
    if name.startswith("llama"):
        cfg = LlamaConfig.named(name)
        return cfg, Llama(cfg)
    cfg = GPT2Config.named(name)
    return cfg, GPT2(cfg)


def _docs(device):
    from ray_torch_distributed_checkpoint_amd.ops import DocLayout

    return DocLayout.from_lengths([LENGTHS] * B, T, device)


@pytest.mark.parametrize("name", ["llama3-tiny", "gpt2-tiny"])
def test_document_isolation_through_the_model(name):
    """Other token ids in document 1 leave the logits of document 2's rows bit-identical: no
    attention across the boundary in any layer and, for Llama, positions that restart (with
    absolute positions the rows would still match - the mask alone proves nothing about RoPE -
    so the Llama rows are also compared with the document run alone, as rows 0..77)."""
    cfg, ref = _model(name)
    gpu = ref.cuda()
    docs = _docs("cuda")
    torch.manual_seed(1)
    idx = torch.randint(0, cfg.vocab_size, (B, T), device="cuda")
    idx2 = idx.clone()
    idx2[:, : LENGTHS[0]] = torch.randint(0, cfg.vocab_size, (B, LENGTHS[0]), device="cuda")
    with torch.no_grad():
        a = gpu(idx, docs=docs)
        b = gpu(idx2, docs=docs)
    assert torch.isfinite(a.float()).all()
    assert torch.equal(a[:, LENGTHS[0]:], b[:, LENGTHS[0]:])
    assert not torch.equal(a[:, : LENGTHS[0]], b[:, : LENGTHS[0]])
    if name.startswith("llama"):
        # position reset: document 2 alone, padded with a second document to keep T % 64 == 0
        from ray_torch_distributed_checkpoint_amd.ops import DocLayout

        n2 = LENGTHS[1]
        alone = torch.cat([idx[:, LENGTHS[0]:], idx[:, : LENGTHS[0]]], dim=1)
        with torch.no_grad():
            c = gpu(alone, docs=DocLayout.from_lengths([[n2, T - n2]] * B, T, "cuda"))
        err = (c[:, :n2].float() - a[:, LENGTHS[0]:].float()).abs().max().item()
        mag = a.float().abs().max().item()
        assert err <= 2e-2 * mag, (err, mag)  # (other tile phase: equal up to bf16 rounding)


@pytest.mark.parametrize("name", ["llama3-tiny", "gpt2-tiny"])
def test_packed_logits_match_the_cpu_path(name):
    """GPU logits of the packed input against the model's fp32 CPU path with the same docs.  The
    bound is measured here: the same GPU-vs-CPU error of the plain forward (existing
    behaviour) of the same model and input; packed may be at most 1.5x that - room for shorter
    softmax rows changing the rounding pattern, not for a wrong mask."""
    cfg, ref = _model(name)
    gpu = copy.deepcopy(ref).cuda()
    torch.manual_seed(2)
    idx = torch.randint(0, cfg.vocab_size, (B, T))
    with torch.no_grad():
        plain = (gpu(idx.cuda()).float().cpu() - ref(idx).float()).abs().max().item()
        packed = (gpu(idx.cuda(), docs=_docs("cuda")).float().cpu() - ref(idx, docs=_docs("cpu")).float()).abs().max().item()
        moved = (ref(idx, docs=_docs("cpu")).float() - ref(idx).float()).abs().max().item()
    print(f"{name}: GPU-vs-CPU max logit error plain {plain:.4e}, packed {packed:.4e} (mask effect {moved:.3e})")
    assert moved > 10 * plain  # the mask does change the logits, far beyond the parity error
    assert packed <= 1.5 * plain, (packed, plain)


def test_llama_step_with_documents():
    """One optimizer step on packed sequences: finite loss and gradients, and the targets of
    the documents' last tokens (-100) give exactly zero rows in the LM-head gradient."""
    from ray_torch_distributed_checkpoint_amd.optim import FusedAdamW

    cfg, ref = _model("llama3-tiny")
    gpu = ref.cuda()
    docs = _docs("cuda")
    torch.manual_seed(3)
    tok = torch.randint(0, cfg.vocab_size, (B, T + 1), device="cuda")
    pos = torch.arange(T, device="cuda", dtype=torch.int32)
    last = docs.end == (pos + 1)[None, :]
    assert int(last.sum()) == B * len(LENGTHS)
    tgt = tok[:, 1:].masked_fill(last, -100)
    opt = FusedAdamW(gpu.parameters(), lr=1e-3, weight_decay=0.0)
    loss = gpu(tok[:, :-1].contiguous(), tgt.contiguous(), docs)
    # ops/xent.py _LMHeadXent.forward: ctx.save_for_backward(x2, ws, logits, cnt), and on the
    # unchunked path (RTDC_LMHEAD_CHUNK_MB off, the default) the xent kernel has overwritten
    # `logits` with the softmax gradient - saved tensor 2 is dlogits [B*T, padded vocab]
    saved = loss.grad_fn.saved_tensors
    assert len(saved) == 4 and saved[2].shape[0] == B * T and saved[2].dtype == torch.bfloat16
    dlogits = saved[2]
    rows = dlogits.view(B * T, -1)
    assert (rows[last.view(-1)] == 0).all()
    assert (rows[~last.view(-1)] != 0).any(dim=1).all()
    loss.backward()
    assert torch.isfinite(loss).item()
    for n, p in gpu.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad.float()).all(), n
    opt.step()
    assert all(torch.isfinite(p.float()).all() for p in gpu.parameters())
