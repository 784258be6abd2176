"""`weights="fp8"` on the GPU, on the models, tokens and sizes of tests/test_generate_fast_gpu.py.  Every
linear master (the tied wte included) is snapped once through quantise -> dequantise in fp32, on the
CPU model and its GPU copy alike: a snapped master quantises to its own codes, so the CPU fp32 forward
is the reference of the FP8 path.  The bound is the existing one, unchanged: e_dec <= 2 x e_full, the
error of the GPU bf16 full forward of the same model (PARITY lines: profiles/decode_fast_fp8.md).
"""
import copy

import pytest
import torch
import torch.nn.functional as F

from ray_torch_distributed_checkpoint_amd import ops
from ray_torch_distributed_checkpoint_amd.models.generation import CapturedDecode
from tests.test_generate_fast_gpu import DEV, NAMES, STEPS, P, T, _bits, _cache
from tests.test_generate_fast_gpu import _models as _bf16_models

pytestmark = pytest.mark.gpu

FP8 = dict(few_row=True, weights="fp8")
_built: dict = {}


def _models(name):
    if name not in _built:
        cpu, idx = copy.deepcopy(_bf16_models(name)[0]), _bf16_models(name)[2]
        with torch.no_grad():
            for n, p in cpu.named_parameters():
                if p.dim() == 2 and "wpe" not in n and "tok_embeddings" not in n:
                    q, s = ops.quantize_fp8_rows(p.detach().contiguous())
                    p.copy_(q.float() * s[:, None])
        _built[name] = (cpu, copy.deepcopy(cpu).to(DEV).eval(), idx)
    return _built[name]


def _eager(gpu, idx, **kw):
    cache = _cache(gpu, idx.shape[0])
    rows = [gpu.prefill(idx[:, :P], cache, **kw).clone()]
    for t in range(P, T):
        rows.append(gpu.decode_step(idx[:, t], cache, **kw).clone())
    return rows, cache


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("name", NAMES)
def test_fp8_path_no_worse_than_twice_the_full_forward(name, B):
    cpu, gpu, idx = _models(name)
    idx = idx[:B]
    with torch.no_grad():
        ref = cpu(idx)[:, P - 1:]
        full = gpu(F.pad(idx, (0, -T % 64)).to(DEV))[:, P - 1:T].float().cpu()
    rows, cache = _eager(gpu, idx.to(DEV), **FP8)
    dec = torch.stack(rows, dim=1).float().cpu()
    assert cache.length == T and dec.shape == ref.shape == full.shape and bool(torch.isfinite(dec).all())
    e_full, e_dec = (full - ref).abs().max().item(), (dec - ref).abs().max().item()
    print(f"PARITY fp8 {name:<12s} B {B} e_full {e_full:.4g} e_dec {e_dec:.4g} ratio {e_dec / e_full:.3f} "
          f"logit scale {ref.abs().max().item():.4g}")
    assert e_dec <= 2.0 * e_full, (e_dec, e_full)


@pytest.mark.parametrize("name", NAMES)
def test_captured_equals_eager_bitwise(name):
    """also: a session refuses a step that names another `weights`; fp8 without few_row raises"""
    _, gpu, idx = _models(name)
    for B in (2, 3):
        dev_idx = idx[:B].to(DEV)
        want, _ = _eager(gpu, dev_idx, **FP8)
        cache = _cache(gpu, B)
        assert torch.equal(_bits(gpu.prefill(dev_idx[:, :P], cache, **FP8)), _bits(want[0]))
        sess = CapturedDecode(gpu, cache, **FP8)
        for i, t in enumerate(range(P, T)):
            assert torch.equal(_bits(sess.step(dev_idx[:, t], weights="fp8")), _bits(want[i + 1])), t
        prompt = dev_idx[:, :P]
        for kw in (FP8, dict(temperature=0.8, top_k=50, seed=7, **FP8)):
            s = gpu.generate(prompt, STEPS, **kw)
            assert torch.equal(s, gpu.generate(prompt, STEPS, captured=True, **kw))
            assert s.shape == (B, T) and int(s.max()) < gpu.cfg.vocab_size
    cache.reset()
    gpu.prefill(prompt, cache, **FP8)
    with pytest.raises(RuntimeError, match="weights"):
        sess.step(dev_idx[:, P], weights="bf16")
    with pytest.raises(RuntimeError, match="weights"):
        CapturedDecode(gpu, cache, few_row=True).step(dev_idx[:, P], weights="fp8")
    for call in (lambda: gpu.prefill(prompt, _cache(gpu, B), weights="fp8"),
                 lambda: gpu.decode_step(dev_idx[:, P], cache, weights="fp8"),
                 lambda: gpu.generate(prompt, 4, weights="fp8"), lambda: CapturedDecode(gpu, cache, weights="fp8")):
        with pytest.raises(ValueError, match="few_row"):
            call()


def test_a_moved_version_requantises_in_place_and_a_replaced_image_raises():
    gpu, idx = copy.deepcopy(_models("gpt2-tiny")[1]), _models("gpt2-tiny")[2][:2].to(DEV)
    cache = _cache(gpu, 2)
    gpu.prefill(idx[:, :P], cache, **FP8)
    sess = CapturedDecode(gpu, cache, **FP8)
    sess.step(idx[:, P])
    w = gpu.h[0].mlp.c_fc.weight
    q_ptr, q_old = w._rtdc_fp8[0].data_ptr(), w._rtdc_fp8[0].view(torch.uint8).clone()
    with torch.no_grad():
        w.mul_(torch.linspace(0.5, 1.5, w.shape[1], device=DEV))
    got = sess.step(idx[:, P + 1]).clone()
    assert w._rtdc_fp8[0].data_ptr() == q_ptr and not torch.equal(w._rtdc_fp8[0].view(torch.uint8), q_old)
    c2 = _cache(gpu, 2)
    gpu.prefill(idx[:, :P], c2, **FP8)
    for l2, l1 in zip(c2.layers, cache.layers):
        l2.copy_(l1)                 # the cache rows as the session saw them
    c2.pos.fill_(P + 1)
    c2.length = P + 1
    assert torch.equal(_bits(got), _bits(gpu.decode_step(idx[:, P + 1], c2, **FP8)))
    w._rtdc_fp8 = (w._rtdc_fp8[0].clone(), w._rtdc_fp8[1])
    with pytest.raises(RuntimeError, match="FP8"):
        sess.step(idx[:, P + 2])
