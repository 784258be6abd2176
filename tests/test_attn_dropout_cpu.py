"""Attention dropout without a GPU: the reference of tests/attn_dropout_ref.py (its fp32 twin stays
inside its own allowance, the mutants leave it), the mask function, the CPU path of
ops.causal_attention and exact resume of a workload with attn_dropout on."""
import json
import math
import os

import pytest
import torch

from tests import ulp as U
from tests.attn_dropout_ref import DROP_MUTANTS, attn_drop_ref, clipped

F64, F32 = U.F64, U.F32
CASES = [(2, 64, 2, 2, 64), (2, 128, 4, 2, 64), (1, 192, 4, 1, 128)]
SEED, OFFSET = 0x5EED, 12345
OUTS = ("out", "lse", "delta", "dq", "dk", "dv")


def _docs(mode, B, T):
    arr = U.doc_arrays(U.attn_layout("A", T, B), T) if mode == "A" else None
    return clipped(B, T, 48 if mode == "W48" else None, arr)


@pytest.mark.parametrize("mode", ["plain", "A", "W48"])
@pytest.mark.parametrize("gen", ["randn", "peaky"])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("c", CASES, ids=lambda c: "B%d-T%d-H%d-Hkv%d-Dh%d" % c)
def test_twin_stays_inside_the_allowance(c, p, gen, mode):
    B, T, H, Hkv, Dh = c
    x = U.attn_inputs(gen, B, T, H, Hkv, Dh)
    a = (x["qkv"], x["dout"], B, T, H, Hkv, Dh, SEED, OFFSET, p, _docs(mode, B, T))
    ref, twin = attn_drop_ref(F64, *a), attn_drop_ref(F32, *a, twin=True)
    for n in OUTS:
        score = U.allow_err(twin[n], ref[n], ref["allow_" + n])
        print(f"{c} p={p} {gen} {mode} {n}: twin score {score:.3f}")
        assert score <= 1.0, (n, score)


@pytest.fixture(scope="module")
def mutant_case():
    B, T, H, Hkv, Dh = CASES[1]
    x = U.attn_inputs("randn", B, T, H, Hkv, Dh)
    a = (x["qkv"], x["dout"], B, T, H, Hkv, Dh, SEED, OFFSET, 0.1)
    return a, attn_drop_ref(F64, *a)


@pytest.mark.parametrize("mutant", DROP_MUTANTS)
def test_mutants_leave_the_allowance(mutant_case, mutant):
    """a kernel with the error (the fp32 twin carrying it) scores > 1 on at least one output"""
    a, ref = mutant_case
    bad = attn_drop_ref(F32, *a, twin=True, mutant=mutant)
    scores = {n: U.allow_err(bad[n], ref[n], ref["allow_" + n]) for n in OUTS}
    print(mutant, {n: round(s, 2) for n, s in scores.items()})
    # (a NaN score - l_kept_only divides by 0 where a row's only key is dropped - is outside as well)
    assert any(not s <= 1.0 for s in scores.values()), scores


def test_mask_properties():
    from ray_torch_distributed_checkpoint_amd.ops import attention_dropout_keep, attention_dropout_mask

    B, H, T = 2, 4, 128
    nb = T // 4
    tri = torch.tril(torch.ones(T, T, dtype=torch.bool))
    for p in (0.1, 0.25, 0.5):
        thr, inv_keep = attention_dropout_keep(p)
        assert thr == round(256 * p) and inv_keep == 256 / (256 - thr)
        m = attention_dropout_mask(SEED, OFFSET, B, H, T, p)
        assert m.shape == (B, H, T, T) and m.dtype == torch.bool
        n = int(tri.sum()) * B * H
        keep = (256 - thr) / 256
        sigma = math.sqrt(keep * (1 - keep) / n)
        frac = m[:, :, tri].float().mean().item()
        print(f"p={p}: kept {frac:.5f}, expected {keep:.5f}, {abs(frac - keep) / sigma:.2f} sigma")
        assert abs(frac - keep) <= 5 * sigma
        assert torch.equal(m, attention_dropout_mask(SEED, OFFSET, B, H, T, p))
    # offset and offset + B H nb nb reserve disjoint counter ranges: the second draw is the tail of
    # a draw of twice the batch that starts at the first
    n = B * H * nb * nb
    both = attention_dropout_mask(SEED, OFFSET, 2 * B, H, T, 0.5)
    first, second = attention_dropout_mask(SEED, OFFSET, B, H, T, 0.5), attention_dropout_mask(SEED, OFFSET + n, B, H, T, 0.5)
    assert torch.equal(both[:B], first) and torch.equal(both[B:], second)
    agree = (first == second).float().mean().item()
    assert abs(agree - 0.5) < 5 * 0.5 / math.sqrt(first.numel())  # independent draws agree by chance only
    for p in (0.0, 0.001, 0.999, 1.0, -0.1):
        with pytest.raises(ValueError):
            attention_dropout_keep(p)
    with pytest.raises(ValueError):
        attention_dropout_mask(SEED, OFFSET, B, H, T, 0.999)


def test_cpu_causal_attention_consumes_the_stream():
    from ray_torch_distributed_checkpoint_amd.ops import (PhiloxStream, attention_dropout_keep, attention_dropout_mask,
                                                          causal_attention)

    B, T, H, Hkv, Dh = 2, 64, 4, 2, 16
    nb = T // 4
    torch.manual_seed(0)
    qkv = torch.randn(B, T, (H + 2 * Hkv) * Dh)
    st = PhiloxStream(seed=11, offset=7)
    plain = causal_attention(qkv, H, Hkv)
    assert torch.equal(causal_attention(qkv, H, Hkv, dropout_p=0.1, training=False, stream=st), plain)
    assert torch.equal(causal_attention(qkv, H, Hkv, dropout_p=0.0, stream=st), plain)
    assert st.offset == 7  # neither call drew anything
    out = causal_attention(qkv, H, Hkv, dropout_p=0.1, stream=st)
    assert st.offset == 7 + B * H * nb * nb
    causal_attention(qkv, H, Hkv, dropout_p=0.5, window=16, stream=st)
    assert st.offset == 7 + 2 * B * H * nb * nb
    # what it computed: softmax over every allowed key, then the kept entries scaled
    thr, ik = attention_dropout_keep(0.1)
    M = attention_dropout_mask(11, 7, B, H, T, 0.1)
    q = qkv[..., :H * Dh].reshape(B, T, H, Dh).transpose(1, 2)
    k = qkv[..., H * Dh:(H + Hkv) * Dh].reshape(B, T, Hkv, Dh).transpose(1, 2).repeat_interleave(H // Hkv, 1)
    v = qkv[..., (H + Hkv) * Dh:].reshape(B, T, Hkv, Dh).transpose(1, 2).repeat_interleave(H // Hkv, 1)
    s = (q @ k.transpose(-1, -2)) / math.sqrt(Dh)
    s = s.masked_fill(~torch.tril(torch.ones(T, T, dtype=torch.bool)), -math.inf)
    ref = ((torch.softmax(s, -1) * M * ik) @ v).transpose(1, 2).reshape(B, T, H * Dh)
    assert torch.allclose(out, ref, atol=1e-5, rtol=1e-5)
    with pytest.raises(ValueError):
        causal_attention(qkv, H, Hkv, dropout_p=0.999, stream=st)
    # gradients flow through the CPU path
    g = qkv.clone().requires_grad_(True)
    causal_attention(g, H, Hkv, dropout_p=0.1, stream=PhiloxStream(11, 7)).sum().backward()
    assert torch.isfinite(g.grad).all() and g.grad.abs().sum() > 0


def test_reserve_counters():
    from ray_torch_distributed_checkpoint_amd.ops import PhiloxStream

    st = PhiloxStream(3, 10)
    assert st.reserve_counters(5) == (3, 10) and st.offset == 15
    assert st.reserve(5) == (3, 15) and st.offset == 17  # reserve(numel) stays: ceil(numel / 4) counters


def test_models_take_attn_dropout_as_a_plain_attribute():
    from ray_torch_distributed_checkpoint_amd import ops
    from ray_torch_distributed_checkpoint_amd.models import GPT2, GPT2Config, Llama, LlamaConfig

    for net, vocab in ((GPT2(GPT2Config.named("gpt2-tiny"), attn_dropout=0.1), 1000),
                       (Llama(LlamaConfig.named("llama3-tiny"), attn_dropout=0.1), 1024)):
        assert net.attn_dropout == 0.1 and "attn_dropout" not in "".join(net.state_dict())
        torch.manual_seed(1)
        idx = torch.randint(0, vocab, (2, 65))
        x, y = idx[:, :-1], idx[:, 1:]
        ops.manual_seed(5)
        a = net(x, y).item()
        assert ops.default_stream().offset > 0
        ops.manual_seed(5)
        assert net(x, y).item() == a  # the same stream state, the same masks
        net.eval()
        off = ops.default_stream().offset
        e = net(x, y).item()
        assert ops.default_stream().offset == off and e != a  # eval draws nothing
        net.train()
        net.attn_dropout = 0.0
        assert net(x, y).item() == e and ops.default_stream().offset == off


def _losses(result_path) -> dict:
    out = {}
    for line in open(os.path.join(result_path, "result.json")):
        row = json.loads(line)
        for i, v in enumerate(reversed(row["losses"])):
            out[row["step"] - i] = v
    return out


def test_workload_with_attn_dropout_resumes_exactly(tmp_path, monkeypatch):
    """gpt2-tiny with attn_dropout = 0.1: the losses of an exact resume are bit-identical to the
    uninterrupted run's (the mask stream's position comes back with the checkpoint's RNG state).
    With attn_dropout unset the run is the run it was: the same rows as attn_dropout = 0, and the
    default stream is neither seeded nor advanced."""
    from ray_torch_distributed_checkpoint_amd import ops
    from ray_torch_distributed_checkpoint_amd import workloads as W

    monkeypatch.setenv("RTDC_FORCE_CPU", "1")

    def fit(name, steps, p=0.1, **kw):
        return W.train_workload("gpt2-tiny", steps=steps, num_workers=1, ckpt_every_n_steps=2, attn_dropout=p,
                                checkpoint_storage_path=str(tmp_path / name), verbose=0, **kw)

    full = _losses(fit("full", 4).path)
    assert sorted(full) == [1, 2, 3, 4] and all(torch.isfinite(torch.tensor(v)) for v in full.values())
    first = fit("first", 2)
    rest = _losses(fit("rest", 4, checkpoint=first.checkpoint, resume_mode="exact").path)
    assert _losses(first.path) == {k: full[k] for k in (1, 2)}
    assert rest == {k: full[k] for k in (3, 4)}

    ops.manual_seed(0x5EED)
    before = ops.default_stream().state_dict()
    off = _losses(fit("off", 2, p=None).path)
    assert ops.default_stream().state_dict() == before
    assert off == _losses(fit("zero", 2, p=0.0).path)
    assert off[1] != full[1]  # dropout does change what is computed
    assert W.WorkloadConfig(model="gpt2-tiny").attn_dropout is None
    with pytest.raises(ValueError):
        W.train_workload("gpt2-tiny", steps=1, num_workers=1, attn_dropout=0.999, verbose=0)
