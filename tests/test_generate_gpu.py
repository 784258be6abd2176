"""KV-cache generation on the GPU: the cached path (padded prefill + decode steps on the split-KV
kernel) against the CPU fp32 forward of the same weights, no worse than twice the error of the
existing GPU full forward; generate() reproducible bit for bit.

B = 2, prompt P = 40 (the prefill pads it to 64), then 30 teacher-forced decode steps, which
cross the 64 boundary.  The masters are rounded to bf16-representable values first, so the CPU
reference multiplies the same weights.  Both paths round activations to bf16 at the same places;
the factor 2 covers the different summation order inside attention.  The two numbers of one run
are kept in profiles/decode_parity.md.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, P, STEPS = 2, 40, 30
_built: dict = {}


def _models(name):
    """(CPU fp32 model, its GPU copy, tokens [B, P + STEPS], CPU reference logits) - built once"""
    from ray_torch_distributed_checkpoint_amd.generate import build_model
    from ray_torch_distributed_checkpoint_amd.models import Llama, LlamaConfig

    if name not in _built:
        torch.manual_seed(20)
        if name == "llama-dh128":
            cpu = Llama(LlamaConfig(vocab_size=1024, dim=256, n_layers=2, n_heads=2, n_kv_heads=1, ffn_dim=512,
                                    max_seq_len=512))
        else:
            cpu = build_model(name, "cpu")
        cpu.eval()
        with torch.no_grad():
            for p in cpu.parameters():
                p.copy_(p.bfloat16().float())
        g = torch.Generator().manual_seed(3)
        idx = torch.randint(0, cpu.cfg.vocab_size, (B, P + STEPS), generator=g)
        _built[name] = (cpu, copy.deepcopy(cpu).to(DEV).eval(), idx)
    return _built[name]


def _parity(name, window):
    from ray_torch_distributed_checkpoint_amd.models.generation import new_cache

    cpu, gpu, idx = _models(name)
    cpu.sliding_window = gpu.sliding_window = window
    T = P + STEPS
    try:
        with torch.no_grad():
            ref = cpu(idx)[:, P - 1:]                                      # positions P - 1 .. T - 1
            # the existing GPU forward, on the flash kernels: T padded to a multiple of 64 (causal)
            full = gpu(F.pad(idx, (0, -T % 64)).to(DEV))[:, P - 1:T].float().cpu()
        cache = new_cache(gpu, B, T, DEV)
        dev_idx = idx.to(DEV)
        rows = [gpu.prefill(dev_idx[:, :P], cache)]
        for t in range(P, T - 1):
            rows.append(gpu.decode_step(dev_idx[:, t], cache))
        rows.append(gpu.decode_step(dev_idx[:, T - 1], cache))
        assert cache.length == T
        dec = torch.stack(rows, dim=1).float().cpu()
    finally:
        cpu.sliding_window = gpu.sliding_window = None
    assert dec.shape == ref.shape == full.shape
    assert bool(torch.isfinite(dec).all())
    e_full = (full - ref).abs().max().item()
    e_dec = (dec - ref).abs().max().item()
    per_pos = (dec - ref).abs().amax(dim=(0, 2))
    print(f"PARITY {name:<12s} window {window!s:<5s} e_full {e_full:.4g} e_dec {e_dec:.4g} "
          f"ratio {e_dec / e_full:.3f} logit scale {ref.abs().max().item():.4g} "
          f"worst decode position {P - 1 + int(per_pos.argmax())}")
    return e_full, e_dec


@pytest.mark.parametrize("name,window", [("gpt2-tiny", None), ("llama3-tiny", None), ("llama-dh128", None),
                                         ("llama-dh128", 16), ("llama3-tiny", 16)])
def test_cached_path_no_worse_than_twice_the_full_forward(name, window):
    e_full, e_dec = _parity(name, window)
    assert e_full > 0
    assert e_dec <= 2.0 * e_full, (e_dec, e_full)


@pytest.mark.parametrize("name", ["gpt2-tiny", "llama3-tiny", "llama-dh128"])
def test_generate_is_reproducible_bit_for_bit(name):
    _, gpu, idx = _models(name)
    prompt = idx[:, :P].to(DEV)
    V = gpu.cfg.vocab_size
    a = gpu.generate(prompt, STEPS, temperature=0.8, top_k=50, seed=7)
    b = gpu.generate(prompt, STEPS, temperature=0.8, top_k=50, seed=7)
    assert a.shape == (B, P + STEPS) and torch.equal(a, b) and torch.equal(a[:, :P], prompt)
    assert int(a.max()) < V and int(a.min()) >= 0
    g1, g2 = gpu.generate(prompt, STEPS), gpu.generate(prompt, STEPS)
    assert torch.equal(g1, g2) and int(g1.max()) < V
    eos = int(g1[0, P + 2])
    e = gpu.generate(prompt, STEPS, eos_id=eos)
    assert set(e[0, P + 2:].tolist()) == {eos}
    gpu.sliding_window = 16
    try:
        w1, w2 = gpu.generate(prompt, STEPS, temperature=0.8, seed=7), gpu.generate(prompt, STEPS, temperature=0.8, seed=7)
    finally:
        gpu.sliding_window = None
    assert torch.equal(w1, w2)
