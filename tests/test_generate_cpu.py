"""KV-cache generation of GPT-2 and Llama on the CPU path (fp32): prefill + decode_step against
the full forward, generate() against the naive loop, sampling, eos, limits, and the command line
on a committed checkpoint."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = {"gpt2-tiny": 0, "llama3-tiny": 0}   # chosen on the CPU: the greedy top-two gap stays > 1e-3 (asserted)
P, N = 9, 14


def _model(name, seed=None):
    from ray_torch_distributed_checkpoint_amd.generate import build_model

    torch.manual_seed(SEED[name] if seed is None else seed)
    return build_model(name, "cpu").eval()


def _prompt(model, B=2, n=P, seed=11):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, model.cfg.vocab_size, (B, n), generator=g)


def _naive(model, idx, n):
    """full forward, argmax, append; also the smallest top-two logit gap met on the way"""
    gap = float("inf")
    with torch.no_grad():
        for _ in range(n):
            last = model(idx)[:, -1]
            top = torch.topk(last, 2, dim=-1).values
            gap = min(gap, (top[:, 0] - top[:, 1]).min().item())
            idx = torch.cat([idx, last.argmax(-1, keepdim=True)], dim=1)
    return idx, gap


@pytest.mark.parametrize("name", ["gpt2-tiny", "llama3-tiny"])
@pytest.mark.parametrize("window", [None, 6])
def test_teacher_forced_logits_match_full_forward(name, window):
    from ray_torch_distributed_checkpoint_amd.models.generation import new_cache

    model = _model(name)
    model.sliding_window = window
    idx = _prompt(model, n=P + N)
    with torch.no_grad():
        full = model(idx)
    scale = full.abs().max().item()
    cache = new_cache(model, 2, P + N, "cpu")
    lg = model.prefill(idx[:, :P], cache)
    assert lg.shape == (2, model.cfg.vocab_size) and cache.length == P
    worst = (lg - full[:, P - 1]).abs().max().item()
    for t in range(P, P + N):
        lg = model.decode_step(idx[:, t], cache)
        worst = max(worst, (lg - full[:, t]).abs().max().item())
    assert cache.length == P + N and cache.pos.tolist() == [P + N] * 2
    assert worst <= 1e-4 * scale, (worst, scale)
    with pytest.raises(ValueError):
        model.decode_step(idx[:, 0], cache)      # the cache is full


@pytest.mark.parametrize("name", ["gpt2-tiny", "llama3-tiny"])
def test_greedy_generate_equals_naive_loop(name):
    model = _model(name)
    idx = _prompt(model)
    want, gap = _naive(model, idx, N)
    assert gap > 1e-3, f"seed {SEED[name]}: top-two gap {gap} - choose another committed seed"
    got = model.generate(idx, N)
    assert got.shape == (2, P + N) and got.dtype == idx.dtype
    assert torch.equal(got, want)
    assert torch.equal(model.generate(idx, N, temperature=0.7, top_k=1, seed=5), want)   # top_k = 1 is greedy
    assert torch.equal(model.generate(idx, 0), idx)


@pytest.mark.parametrize("name", ["gpt2-tiny", "llama3-tiny"])
def test_sampling(name):
    model = _model(name)
    V = model.cfg.vocab_size
    idx = _prompt(model)
    a = model.generate(idx, N, temperature=1.5, seed=3)
    b = model.generate(idx, N, temperature=1.5, seed=3)
    c = model.generate(idx, N, temperature=1.5, seed=4)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert int(a.max()) < V and int(c.max()) < V and int(a.min()) >= 0
    # the padded vocabulary columns can never be drawn, however attractive their weights are
    # (gpt2-tiny: 1000 of 1024 columns real; llama3-tiny has no padded column, the rows below are empty)
    table = model.wte if name.startswith("gpt2") else model.output
    assert table.shape[0] > V or name == "llama3-tiny"
    with torch.no_grad():
        table[V:] = 50.0 * table[:V].abs().max()
    d = model.generate(idx, N, temperature=1.0, seed=1)
    assert int(d.max()) < V
    k = model.generate(idx, N, temperature=1.0, top_k=3, seed=1)
    assert int(k.max()) < V


def test_rows_stay_at_eos_after_emitting_it():
    model = _model("gpt2-tiny")
    idx = _prompt(model)
    free = model.generate(idx, N)
    eos = int(free[0, P + 3])                   # what row 0 emits as its 4th token
    got = model.generate(idx, N, eos_id=eos)
    for b in range(2):
        row, ref = got[b, P:].tolist(), free[b, P:].tolist()
        first = ref.index(eos) if eos in ref else None
        if first is None:
            assert row == ref
        else:
            assert row[: first + 1] == ref[: first + 1] and set(row[first:]) == {eos}
    assert set(got[0, P + 3:].tolist()) == {eos}


def test_length_overflow_raises():
    g, l = _model("gpt2-tiny"), _model("llama3-tiny")
    with pytest.raises(ValueError, match="exceeds"):
        g.generate(_prompt(g, n=250), 7)         # n_positions = 256
    with pytest.raises(ValueError, match="exceeds"):
        l.generate(_prompt(l, n=500), 13)        # max_seq_len = 512
    assert g.generate(_prompt(g, n=250), 6).shape == (2, 256)


def test_command_line_on_a_committed_checkpoint(tmp_path, monkeypatch):
    """2 training steps of gpt2-tiny, checkpoint committed; the command line's tokens equal
    generate() of a model loaded by hand from the same directory"""
    monkeypatch.setenv("RTDC_FORCE_CPU", "1")
    from ray_torch_distributed_checkpoint_amd import workloads as W
    from ray_torch_distributed_checkpoint_amd.generate import build_model, load_weights

    r = W.train_workload("gpt2-tiny", steps=2, num_workers=1, ckpt_every_n_steps=2,
                         checkpoint_storage_path=str(tmp_path / "run"), verbose=0)
    ckpt = r.checkpoint.path
    env = dict(os.environ, RTDC_FORCE_CPU="1", PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "ray_torch_distributed_checkpoint_amd.generate", "--model", "gpt2-tiny",
           "--checkpoint", ckpt, "--prompt-ids", "5,17,900,3", "--max-new-tokens", "12", "--batch", "2",
           "--device", "cpu"]
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=300)
    assert out.returncode == 0, out.stderr
    row = json.loads(out.stdout.strip().splitlines()[-1])
    assert row["tokens_per_s"] > 0 and row["new_tokens"] == 12
    torch.manual_seed(99)                        # another init: the weights must come from the checkpoint
    model = build_model("gpt2-tiny", "cpu").eval()
    before = model.h[0].attn.c_attn.weight.clone()
    load_weights(model, ckpt)
    assert not torch.equal(before, model.h[0].attn.c_attn.weight)
    want = model.generate(torch.tensor([[5, 17, 900, 3]] * 2), 12)
    assert row["tokens"] == want.tolist()
    # sampled, from synthetic prompt rows
    cmd2 = cmd[:7] + ["--prompt-len", "8", "--max-new-tokens", "5", "--temperature", "0.9", "--top-k", "20", "--seed",
                      "7", "--batch", "3", "--device", "cpu"]
    out2 = subprocess.run(cmd2, capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=300)
    assert out2.returncode == 0, out2.stderr
    row2 = json.loads(out2.stdout.strip().splitlines()[-1])
    assert len(row2["tokens"]) == 3 and all(len(t) == 13 for t in row2["tokens"])
    assert max(max(t) for t in row2["tokens"]) < model.cfg.vocab_size
