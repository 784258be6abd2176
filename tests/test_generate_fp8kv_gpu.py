"""`kv_cache="fp8"` on the GPU, on the models, tokens and sizes of tests/test_generate_fast_gpu.py.

Captured against eager is bitwise, with the FP8 cache alone and together with few_row=True,
weights="fp8".  Parity: the reference is the CPU fp32 full forward without any quantisation; e_full is
the GPU bf16 full forward's error, e_q the error of the CPU fp32 model run through prefill /
decode_step on a CPU FP8 cache (pure quantisation error, plain torch), and the GPU FP8-cache path is
held to e_dec <= 2 e_full + 2 e_q: the project's allowance for the bf16 path plus the same factor of
two on the quantisation error, for codes that flip because the GPU's bf16 k|v differ from the CPU's
fp32 ones.  PARITY lines of one run: profiles/decode_fp8_kv.md.
"""
import pytest
import torch
import torch.nn.functional as F

from ray_torch_distributed_checkpoint_amd.models.generation import CapturedDecode, new_cache
from tests.test_generate_fast_gpu import DEV, NAMES, STEPS, P, T, _bits, _models
from tests.test_generate_fp8_gpu import _models as _snapped_models

pytestmark = pytest.mark.gpu

CONFIGS = {"cache": {}, "cache+fp8w": dict(few_row=True, weights="fp8")}


def _run(model, idx, dev, **kw):
    """[prefill logits, then one row per teacher-forced step] on a fresh FP8 cache, and the cache"""
    cache = new_cache(model, idx.shape[0], T, dev, kv_cache="fp8")
    rows = [model.prefill(idx[:, :P], cache, **kw).clone()]
    for t in range(P, T):
        rows.append(model.decode_step(idx[:, t], cache, **kw).clone())
    return rows, cache


@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("name", NAMES)
def test_captured_equals_eager_bitwise(name, cfg):
    """also: the session keeps working after cache.reset() and a new prefill; generate(captured=True)
    gives the eager tokens"""
    kw = CONFIGS[cfg]
    _, gpu, idx = _models(name)
    for B in (2, 3):
        dev_idx = idx[:B].to(DEV)
        want, ecache = _run(gpu, dev_idx, DEV, **kw)
        cache = new_cache(gpu, B, T, DEV, kv_cache="fp8")
        assert torch.equal(_bits(gpu.prefill(dev_idx[:, :P], cache, **kw)), _bits(want[0]))
        sess = CapturedDecode(gpu, cache, **kw)
        for again in range(2):
            for i, t in enumerate(range(P, T)):
                assert torch.equal(_bits(sess.step(dev_idx[:, t])), _bits(want[i + 1])), (again, t)
            for a, b, sa, sb in zip(cache.layers, ecache.layers, cache.scales, ecache.scales):
                assert torch.equal(a[:, :T].view(torch.uint8), b[:, :T].view(torch.uint8))
                assert torch.equal(sa[:, :T], sb[:, :T])
            cache.reset()
            gpu.prefill(dev_idx[:, :P], cache, **kw)
        s = gpu.generate(dev_idx[:, :P], STEPS, kv_cache="fp8", **kw)
        assert torch.equal(s, gpu.generate(dev_idx[:, :P], STEPS, kv_cache="fp8", captured=True, **kw))
        assert s.shape == (B, T) and int(s.max()) < gpu.cfg.vocab_size


@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("name", NAMES)
def test_fp8_cache_parity(name, B, cfg):
    cpu, gpu, idx = (_models if cfg == "cache" else _snapped_models)(name)
    idx = idx[:B]
    with torch.no_grad():
        ref = cpu(idx)[:, P - 1:]
        full = gpu(F.pad(idx, (0, -T % 64)).to(DEV))[:, P - 1:T].float().cpu()
    quant = torch.stack(_run(cpu, idx, "cpu")[0], dim=1)
    rows, cache = _run(gpu, idx.to(DEV), DEV, **CONFIGS[cfg])
    dec = torch.stack(rows, dim=1).float().cpu()
    assert cache.length == T and dec.shape == ref.shape == full.shape and bool(torch.isfinite(dec).all())
    e_full, e_q = (full - ref).abs().max().item(), (quant - ref).abs().max().item()
    err = (dec - ref).abs()
    e_dec, at = err.max().item(), [int(i) for i in torch.unravel_index(err.argmax(), err.shape)]
    print(f"PARITY fp8kv {cfg:<10s} {name:<12s} B {B} e_full {e_full:.4g} e_q {e_q:.4g} e_q/e_full {e_q / e_full:.3f} "
          f"e_dec {e_dec:.4g} bound {2 * e_full + 2 * e_q:.4g} used {e_dec / (2 * e_full + 2 * e_q):.3f} "
          f"worst (row, position, logit) ({at[0]}, {P - 1 + at[1]}, {at[2]}) logit scale {ref.abs().max().item():.4g}")
    assert e_full > 0 and e_q > 0
    assert e_dec <= 2.0 * e_full + 2.0 * e_q, (e_dec, e_full, e_q)
