"""The fast decode switches on the GPU: `few_row=True` (every decode linear on the few-row kernel)
and `CapturedDecode` / `generate(captured=True)` (the decode step replayed from a hipGraph).

Models, weights and sizes as in tests/test_generate_gpu.py: gpt2-tiny, llama3-tiny and a Dh-128
Llama, masters rounded to bf16; prompt P = 40 (the prefill pads it to 64), then 30 teacher-forced
steps across the 64 boundary; B = 2 and 3; sliding_window None and 16.

Captured against eager is bitwise: the graph replays the kernels the eager step launches, on the
same inputs.  Parity with the CPU fp32 forward keeps the existing test's bound, twice the error
of the GPU full forward, now with few_row=True; the PARITY lines of one run are appended to
profiles/decode_parity.md.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
P, STEPS = 40, 30
T = P + STEPS
NAMES = ["gpt2-tiny", "llama3-tiny", "llama-dh128"]
_built: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_models():
    yield
    _built.clear()


def _models(name):
    """(CPU fp32 model, its GPU copy, tokens [3, P + STEPS]) - built once"""
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
        idx = torch.randint(0, cpu.cfg.vocab_size, (3, T), generator=g)
        _built[name] = (cpu, copy.deepcopy(cpu).to(DEV).eval(), idx)
    return _built[name]


def _cache(gpu, B, length=T):
    from ray_torch_distributed_checkpoint_amd.models.generation import new_cache

    return new_cache(gpu, B, length, DEV)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _eager(gpu, idx, few_row, start=P):
    """[prefill logits, then one row of logits per teacher-forced step], and the cache"""
    cache = _cache(gpu, idx.shape[0])
    rows = [gpu.prefill(idx[:, :start], cache, few_row=few_row).clone()]
    for t in range(start, T):
        rows.append(gpu.decode_step(idx[:, t], cache, few_row=few_row).clone())
    return rows, cache


@pytest.mark.parametrize("window", [None, 16])
@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("name", NAMES)
def test_captured_step_is_bitwise_the_eager_step(name, B, window):
    """both few_row values; also: building the session leaves pos, length and the cache rows below
    length bit for bit, and the keyword-less decode_step is bitwise few_row=False"""
    from ray_torch_distributed_checkpoint_amd.models.generation import CapturedDecode

    _, gpu, idx = _models(name)
    idx = idx[:B].to(DEV)
    gpu.sliding_window = window
    try:
        for few_row in (False, True):
            want, ecache = _eager(gpu, idx, few_row)
            cache = _cache(gpu, B)
            first = gpu.prefill(idx[:, :P], cache, few_row=few_row)
            assert torch.equal(_bits(first), _bits(want[0]))
            before = [l[:, :P].clone() for l in cache.layers]
            sess = CapturedDecode(gpu, cache, few_row=few_row)
            torch.cuda.synchronize()
            assert cache.length == P and cache.pos.tolist() == [P] * B
            assert all(torch.equal(_bits(l[:, :P]), _bits(b)) for l, b in zip(cache.layers, before))
            for i, t in enumerate(range(P, T)):
                got = sess.step(idx[:, t])
                assert got.shape == want[i + 1].shape == (B, gpu.cfg.vocab_size)
                assert torch.equal(_bits(got), _bits(want[i + 1])), (few_row, t)
            assert cache.length == T == ecache.length and cache.pos.tolist() == ecache.pos.tolist() == [T] * B
            assert sess.replays == STEPS
            assert all(torch.equal(_bits(a[:, :T]), _bits(b[:, :T])) for a, b in zip(cache.layers, ecache.layers))
            if not few_row:   # the defaults: no keyword is few_row=False, bit for bit
                c2 = _cache(gpu, B)
                assert torch.equal(_bits(gpu.prefill(idx[:, :P], c2)), _bits(want[0]))
                for i, t in enumerate(range(P, P + 3)):
                    assert torch.equal(_bits(gpu.decode_step(idx[:, t], c2)), _bits(want[i + 1]))
    finally:
        gpu.sliding_window = None


@pytest.mark.parametrize("name,window", [("gpt2-tiny", None), ("llama3-tiny", None), ("llama-dh128", None),
                                         ("llama-dh128", 16), ("llama3-tiny", 16)])
@pytest.mark.parametrize("B", [2, 3])
def test_few_row_path_no_worse_than_twice_the_full_forward(name, window, B):
    """the bound of tests/test_generate_gpu.py, unchanged, on the few_row=True cached path"""
    cpu, gpu, idx = _models(name)
    idx = idx[:B]
    cpu.sliding_window = gpu.sliding_window = window
    try:
        with torch.no_grad():
            ref = cpu(idx)[:, P - 1:]
            full = gpu(F.pad(idx, (0, -T % 64)).to(DEV))[:, P - 1:T].float().cpu()
        dev_idx = idx.to(DEV)
        rows, cache = _eager(gpu, dev_idx, True)
        assert cache.length == T
        dec = torch.stack(rows, dim=1).float().cpu()
        tile = torch.stack(_eager(gpu, dev_idx, False)[0], dim=1).float().cpu()
    finally:
        cpu.sliding_window = gpu.sliding_window = None
    assert dec.shape == ref.shape == full.shape
    assert bool(torch.isfinite(dec).all())
    e_full = (full - ref).abs().max().item()
    e_dec = (dec - ref).abs().max().item()
    e_tile = (tile - ref).abs().max().item()
    per_pos = (dec - ref).abs().amax(dim=(0, 2))
    print(f"PARITY few_row {name:<12s} B {B} window {window!s:<5s} e_full {e_full:.4g} e_dec {e_dec:.4g} "
          f"ratio {e_dec / e_full:.3f} (tile route: e_dec {e_tile:.4g} ratio {e_tile / e_full:.3f}) "
          f"logit scale {ref.abs().max().item():.4g} worst decode position {P - 1 + int(per_pos.argmax())}")
    assert e_full > 0
    assert e_dec <= 2.0 * e_full, (e_dec, e_full)


@pytest.mark.parametrize("few_row", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_generate_captured_equals_eager(name, few_row):
    """token for token: greedy, temperature 0.8 / top_k 50 / seed 7, with eos_id, with a window"""
    _, gpu, idx = _models(name)
    for B in (2, 3):
        prompt = idx[:B, :P].to(DEV)
        g = gpu.generate(prompt, STEPS, few_row=few_row)
        assert torch.equal(g, gpu.generate(prompt, STEPS, few_row=few_row, captured=True))
        kw = dict(temperature=0.8, top_k=50, seed=7, few_row=few_row)
        s = gpu.generate(prompt, STEPS, **kw)
        assert torch.equal(s, gpu.generate(prompt, STEPS, captured=True, **kw))
        assert s.shape == (B, T) and torch.equal(s[:, :P], prompt) and int(s.max()) < gpu.cfg.vocab_size
        eos = int(g[0, P + 2])
        e = gpu.generate(prompt, STEPS, eos_id=eos, few_row=few_row, captured=True)
        assert torch.equal(e, gpu.generate(prompt, STEPS, eos_id=eos, few_row=few_row))
        assert set(e[0, P + 2:].tolist()) == {eos}
    gpu.sliding_window = 16
    try:
        assert torch.equal(gpu.generate(prompt, STEPS, captured=True, **kw), gpu.generate(prompt, STEPS, **kw))
    finally:
        gpu.sliding_window = None


@pytest.mark.parametrize("few_row", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_one_capture_serves_many_prompts(name, few_row):
    """a session built on an empty cache's first prompt is reused after cache.reset() and the prefill
    of another prompt of another length: bitwise a fresh eager run"""
    from ray_torch_distributed_checkpoint_amd.models.generation import CapturedDecode

    _, gpu, idx = _models(name)
    idx = idx[:2].to(DEV)
    cache = _cache(gpu, 2)
    gpu.prefill(idx[:, :P], cache, few_row=few_row)
    sess = CapturedDecode(gpu, cache, few_row=few_row)
    for t in range(P, P + 4):
        sess.step(idx[:, t])
    other = idx.flip(1).contiguous()
    start = 23
    want, _ = _eager(gpu, other, few_row, start=start)
    cache.reset()
    first = gpu.prefill(other[:, :start], cache, few_row=few_row)
    assert torch.equal(_bits(first), _bits(want[0]))
    for i, t in enumerate(range(start, T)):
        assert torch.equal(_bits(sess.step(other[:, t])), _bits(want[i + 1])), t
    assert cache.length == T


@pytest.mark.parametrize("name", ["gpt2-tiny", "llama-dh128"])
def test_overflow_and_changed_window_raise_before_a_replay(name):
    from ray_torch_distributed_checkpoint_amd.models.generation import CapturedDecode

    _, gpu, idx = _models(name)
    idx = idx[:2].to(DEV)
    cache = _cache(gpu, 2, 64)     # Tmax = 64: the position limit of this cache
    gpu.prefill(idx[:, :62], cache)
    sess = CapturedDecode(gpu, cache)
    sess.step(idx[:, 62])
    sess.step(idx[:, 63])
    assert cache.length == 64 and sess.replays == 2
    torch.cuda.synchronize()
    snap = [l.clone() for l in cache.layers]
    with pytest.raises(ValueError):
        sess.step(idx[:, 64])
    torch.cuda.synchronize()
    assert sess.replays == 2 and cache.length == 64 and cache.pos.tolist() == [64, 64]
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(cache.layers, snap))
    with pytest.raises(ValueError):          # a full cache cannot be warmed up
        CapturedDecode(gpu, cache)
    # a window changed after capture
    cache.reset()
    gpu.prefill(idx[:, :P], cache)
    gpu.sliding_window = 16
    try:
        with pytest.raises(RuntimeError, match="sliding_window"):
            sess.step(idx[:, P])
    finally:
        gpu.sliding_window = None
    assert sess.replays == 2 and cache.length == P
    sess.step(idx[:, P])                     # and back: the session works again
    assert cache.length == P + 1
    with pytest.raises(ValueError, match="at most 16"):
        gpu.decode_step(torch.zeros(17, dtype=torch.int64, device=DEV), _cache(gpu, 17, 64), few_row=True)


def test_replaced_weight_storage_is_detected_and_a_refreshed_shadow_is_read():
    """an in-place update of a master (version bump) reaches the replay through the refreshed
    shadow; a shadow or a parameter whose storage was replaced raises"""
    from ray_torch_distributed_checkpoint_amd.models.generation import CapturedDecode

    _, base, idx = _models("gpt2-tiny")
    gpu = copy.deepcopy(base)
    idx = idx[:2].to(DEV)
    cache = _cache(gpu, 2)
    gpu.prefill(idx[:, :P], cache)
    sess = CapturedDecode(gpu, cache)
    sess.step(idx[:, P])
    w = gpu.h[0].mlp.c_fc.weight
    with torch.no_grad():
        w.mul_(0.5)
    got = sess.step(idx[:, P + 1]).clone()
    c2 = _cache(gpu, 2)
    gpu.prefill(idx[:, :P], c2)      # (c_fc changed: the cache rows of layer 1 differ, so rebuild them ...)
    for l2, l1 in zip(c2.layers, cache.layers):
        l2.copy_(l1)                 # ... as the session saw them
    c2.pos.fill_(P + 1)
    c2.length = P + 1
    assert torch.equal(_bits(got), _bits(gpu.decode_step(idx[:, P + 1], c2)))
    w._rtdc_shadow = w._rtdc_shadow.clone()
    with pytest.raises(RuntimeError, match="shadow"):
        sess.step(idx[:, P + 2])
