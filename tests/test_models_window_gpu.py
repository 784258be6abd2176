"""Sliding-window attention through the whole model on the GPU: GPT-2 and Llama with
`sliding_window`, alone and together with packed documents."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

B, T, W, LENGTHS = 2, 128, 24, [50, 78]


def _model(name):
    from ray_torch_distributed_checkpoint_amd.models import GPT2, GPT2Config, Llama, LlamaConfig

    torch.manual_seed(0)
    if name.startswith("llama"):
        cfg = LlamaConfig.named(name)
        return cfg, Llama(cfg, sliding_window=W)
    cfg = GPT2Config.named(name)
    return cfg, GPT2(cfg, sliding_window=W)


def _docs(device):
    from ray_torch_distributed_checkpoint_amd.ops import DocLayout

    return DocLayout.from_lengths([LENGTHS] * B, T, device)


@pytest.mark.parametrize("name", ["llama3-tiny", "gpt2-tiny"])
def test_windowed_logits_match_the_cpu_path(name):
    """GPU logits with sliding_window against the model's fp32 CPU path with the same window.
    The bound is the one of the packed-documents test: the GPU-vs-CPU error of the plain forward
    of the same model and input; windowed may be at most 1.5x that - room for shorter softmax
    rows changing the rounding pattern, not for a wrong mask."""
    cfg, ref = _model(name)
    gpu = copy.deepcopy(ref).cuda()
    torch.manual_seed(2)
    idx = torch.randint(0, cfg.vocab_size, (B, T))
    with torch.no_grad():
        win = (gpu(idx.cuda()).float().cpu() - ref(idx).float()).abs().max().item()
        wref = ref(idx).float()
        gpu.sliding_window = ref.sliding_window = None
        plain = (gpu(idx.cuda()).float().cpu() - ref(idx).float()).abs().max().item()
        moved = (wref - ref(idx).float()).abs().max().item()
    print(f"{name}: GPU-vs-CPU max logit error plain {plain:.4e}, window {win:.4e} (mask effect {moved:.3e})")
    assert moved > 10 * plain  # the window does change the logits, far beyond the parity error
    assert win <= 1.5 * plain, (win, plain)


def test_llama_step_with_window_and_documents():
    """One optimizer step with sliding_window on packed sequences: finite loss and gradients."""
    from ray_torch_distributed_checkpoint_amd.optim import FusedAdamW

    cfg, ref = _model("llama3-tiny")
    gpu = ref.cuda()
    docs = _docs("cuda")
    torch.manual_seed(3)
    tok = torch.randint(0, cfg.vocab_size, (B, T + 1), device="cuda")
    pos = torch.arange(T, device="cuda", dtype=torch.int32)
    tgt = tok[:, 1:].masked_fill(docs.end == (pos + 1)[None, :], -100)
    opt = FusedAdamW(gpu.parameters(), lr=1e-3, weight_decay=0.0)
    loss = gpu(tok[:, :-1].contiguous(), tgt.contiguous(), docs)
    loss.backward()
    assert torch.isfinite(loss).item()
    for n, p in gpu.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad.float()).all(), n
    opt.step()
    assert all(torch.isfinite(p.float()).all() for p in gpu.parameters())
    # the window reached the kernels: without it the same step has another loss
    gpu2 = _model("llama3-tiny")[1].cuda()
    gpu2.sliding_window = None
    assert gpu2(tok[:, :-1].contiguous(), tgt.contiguous(), docs).item() != loss.item()
