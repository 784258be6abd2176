"""Packed sequences without a GPU: the document layout and its constructors, the CPU oracle of
document-masked attention and per-document RoPE, the synthetic document stream, and exact
resume of the LM workloads with documents on."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LENGTHS = [5, 65, 1, 1, 58, 126]
STARTS = [0, 5, 70, 71, 72, 130]


def _valid(d):
    """The invariants the kernels rely on."""
    B, T = d.start.shape
    pos = torch.arange(T, dtype=torch.int32)[None, :]
    assert d.start.dtype == torch.int32 and d.end.dtype == torch.int32
    assert d.start.is_contiguous() and d.end.is_contiguous()
    assert (d.start <= pos).all() and (pos < d.end).all() and (d.end <= T).all() and (d.start >= 0).all()
    assert (d.start[:, 1:] >= d.start[:, :-1]).all() and (d.end[:, 1:] >= d.end[:, :-1]).all()
    for b in range(B):
        for t in range(T):  # constant within a document, and the document is [start, end)
            s, e = int(d.start[b, t]), int(d.end[b, t])
            assert (d.start[b, s:e] == s).all() and (d.end[b, s:e] == e).all()


def test_layout_constructors_agree():
    from ray_torch_distributed_checkpoint_amd.ops import DocLayout

    T = 256
    a = DocLayout.from_lengths([LENGTHS], T)
    assert sorted(set(a.start[0].tolist())) == STARTS
    assert sorted(set(a.end[0].tolist())) == STARTS[1:] + [T]
    _valid(a)
    # the same layout from EOS tokens (an EOS ends each document but the last) ...
    tok = torch.randint(1, 50, (1, T))
    for s in STARTS[1:]:
        tok[0, s - 1] = 0
    b = DocLayout.from_eos(tok, 0)
    # ... and from its own start array
    c = DocLayout.from_doc_start(a.start)
    for o in (b, c):
        assert torch.equal(o.start, a.start) and torch.equal(o.end, a.end)
    # not a layout at all (decreasing, out of range, position 0 unflagged): still a valid one
    junk = torch.randint(-5, T + 5, (3, T))
    junk[0] = torch.arange(T).flip(0)
    _valid(DocLayout.from_doc_start(junk))
    _valid(DocLayout.from_eos(torch.zeros(2, 17, dtype=torch.int64), 0))  # all EOS: documents of length 1
    with pytest.raises(ValueError):
        DocLayout.from_lengths([[5, 6]], 12)


@pytest.mark.parametrize("H,Hkv", [(4, 4), (4, 2)])
def test_cpu_attention_with_docs_is_per_document_attention(H, Hkv):
    from ray_torch_distributed_checkpoint_amd.ops import DocLayout, causal_attention
    from ray_torch_distributed_checkpoint_amd.ops.attention import causal_attention_ref

    torch.manual_seed(0)
    B, T, Dh = 2, 256, 16
    rows = [LENGTHS, [256]]
    qkv = torch.randn(B, T, (H + 2 * Hkv) * Dh)
    out = causal_attention(qkv, H, Hkv, docs=DocLayout.from_lengths(rows, T))
    for b, row in enumerate(rows):
        at = 0
        for n in row:
            ref = causal_attention_ref(qkv[b:b + 1, at:at + n], 1, n, H, Hkv, Dh)
            assert torch.allclose(out[b:b + 1, at:at + n], ref, atol=1e-5, rtol=1e-5), (b, at, n)
            at += n


def test_rope_ref_with_docs_is_per_document_rope():
    from ray_torch_distributed_checkpoint_amd.ops import DocLayout
    from ray_torch_distributed_checkpoint_amd.ops.llama_ops import apply_rope, rope_ref

    torch.manual_seed(1)
    H, Hkv, Dh, T = 4, 2, 16, 256
    rows = [LENGTHS, [256]]
    x = torch.randn(2, T, (H + 2 * Hkv) * Dh)
    docs = DocLayout.from_lengths(rows, T)
    y = rope_ref(x, H, Hkv, 500000.0, docs)
    assert torch.equal(y, apply_rope(x, H, Hkv, 500000.0, docs=docs))
    for b, row in enumerate(rows):
        at = 0
        for n in row:
            assert torch.equal(y[b:b + 1, at:at + n], rope_ref(x[b:b + 1, at:at + n].contiguous(), H, Hkv, 500000.0))
            at += n


def test_synthetic_tokens_with_documents():
    from ray_torch_distributed_checkpoint_amd.workloads import SyntheticTokens, _mix

    idx = torch.tensor([3, 77, 1000, 4])
    plain = SyntheticTokens(1 << 12, 64, 1000, seed=5)
    packed = SyntheticTokens(1 << 12, 64, 1000, seed=5, doc_len=16)
    out = plain.batch(idx)
    assert isinstance(out, tuple) and len(out) == 2
    # without doc_len: the hash stream of before, bit for bit
    pos = torch.arange(65, dtype=torch.int64)
    tok = _mix(idx[:, None] * 65 + pos, 5) % 1000
    assert torch.equal(out[0], tok[:, :-1]) and torch.equal(out[1], tok[:, 1:])
    x, y, docs = packed.batch(idx)
    x2, y2, docs2 = packed.batch(idx)
    assert torch.equal(x, x2) and torch.equal(y, y2) and torch.equal(docs.start, docs2.start)  # reproducible
    assert torch.equal(x, out[0])  # the tokens themselves do not change
    _valid(docs)
    # a row of the batch is a function of its sequence index alone
    x1, y1, d1 = packed.batch(idx[1:2])
    assert torch.equal(y1[0], y[1]) and torch.equal(d1.start[0], docs.start[1])
    # targets are -100 exactly at the documents' last tokens
    t = torch.arange(64, dtype=torch.int32)[None, :]
    last = docs.end == t + 1
    assert torch.equal(y == -100, last) and torch.equal(y[~last], out[1][~last])
    # the layout is the one the start flags define
    flags = docs.start == t
    assert flags[:, 0].all() and 1 < int(flags.sum()) < flags.numel()
    from ray_torch_distributed_checkpoint_amd.ops import DocLayout

    again = DocLayout.from_flags(flags)
    assert torch.equal(again.start, docs.start) and torch.equal(again.end, docs.end)


def _losses(result_path) -> dict:
    out = {}
    for line in open(os.path.join(result_path, "result.json")):
        row = json.loads(line)
        for i, v in enumerate(reversed(row["losses"])):
            out[row["step"] - i] = v
    return out


@pytest.mark.parametrize("model", ["llama3-tiny", "gpt2-tiny"])
def test_workload_with_documents_resumes_exactly(tmp_path, monkeypatch, model):
    from ray_torch_distributed_checkpoint_amd import workloads as W

    monkeypatch.setenv("RTDC_FORCE_CPU", "1")

    def fit(name, steps, **kw):
        return W.train_workload(model, steps=steps, num_workers=1, ckpt_every_n_steps=2, doc_len=16,
                                checkpoint_storage_path=str(tmp_path / name), verbose=0, **kw)

    full = _losses(fit("full", 4).path)
    assert sorted(full) == [1, 2, 3, 4] and all(torch.isfinite(torch.tensor(v)) for v in full.values())
    first = fit("first", 2)
    rest = _losses(fit("rest", 4, checkpoint=first.checkpoint, resume_mode="exact").path)
    assert _losses(first.path) == {k: full[k] for k in (1, 2)}
    assert rest == {k: full[k] for k in (3, 4)}
    # documents do change what is trained on
    plain = W.train_workload(model, steps=1, num_workers=1, ckpt_every_n_steps=2,
                             checkpoint_storage_path=str(tmp_path / "plain"), verbose=0)
    assert _losses(plain.path)[1] != full[1]
