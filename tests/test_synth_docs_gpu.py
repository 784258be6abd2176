"""The synthetic document stream on the GPU: the native flag kernel + layout kernel give the CPU
path's arrays bit for bit, and the packed LM workload trains and resumes exactly on the GPU."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.mark.parametrize("T,vocab,L", [(1024, 50257, 100), (64, 1000, 7), (200, 333, 1)])
def test_synth_documents_match_cpu(T, vocab, L):
    """SyntheticTokens(doc_len=L).batch() on the GPU (synth_tokens, synth_doc_flags, doc_layout
    kernels) equals the CPU hash path: inputs, targets incl. the -100 positions, start, end.
    doc_len values that are no power of two, ids up to dataset_size - 1."""
    from ray_torch_distributed_checkpoint_amd.workloads import SyntheticTokens

    n = 1 << 20
    ds = SyntheticTokens(n, T, vocab, seed=1234, doc_len=L)
    ids = torch.tensor([0, 5, 1 << 19, n - 1, n - 2, 77], dtype=torch.int64)
    ci, ct, cd = ds.batch(ids)
    gi, gt, gd = ds.batch(ids.to(DEV))
    assert gi.is_contiguous() and gt.is_contiguous()
    assert gd.start.is_cuda and gd.start.dtype == torch.int32 and gd.end.dtype == torch.int32
    assert torch.equal(gi.cpu(), ci) and torch.equal(gt.cpu(), ct)
    assert torch.equal(gd.start.cpu(), cd.start) and torch.equal(gd.end.cpu(), cd.end)
    pos = torch.arange(T, dtype=torch.int32)[None, :]
    assert torch.equal(gt.cpu() == -100, cd.end == pos + 1)
    if L > 1:
        assert 1 < int((cd.start == pos).sum()) < ids.numel() * T  # some boundaries, not all
    else:
        assert torch.equal(cd.start, pos.expand_as(cd.start))  # every token its own document


def _losses(result_path) -> dict:
    out = {}
    for line in open(os.path.join(result_path, "result.json")):
        row = json.loads(line)
        for i, v in enumerate(reversed(row["losses"])):
            out[row["step"] - i] = v
    return out


def test_packed_workload_trains_and_resumes_exactly_on_gpu(tmp_path, monkeypatch):
    """`workloads.py --doc-len` end to end on the GPU: the 3-tuple batch, the CUDA layout through
    RoPE and the document-masked flash kernels of every layer, -100 targets in the LM head; a run
    resumed from its step-2 checkpoint repeats steps 3 and 4 bit for bit."""
    from ray_torch_distributed_checkpoint_amd import train
    from ray_torch_distributed_checkpoint_amd import workloads as W

    for k in ("RTDC_FAIL_AT_STEP", "RTDC_HANG_AT_STEP", "RTDC_FORCE_CPU"):
        monkeypatch.delenv(k, raising=False)
    kw = dict(steps=4, num_workers=1, use_gpu=True, ckpt_every_n_steps=2, verbose=0, doc_len=16)
    a = W.train_workload("llama3-tiny", checkpoint_storage_path=str(tmp_path / "a"), **kw)
    la = _losses(a.path)
    assert sorted(la) == [1, 2, 3, 4] and all(v == v and abs(v) < 1e4 for v in la.values())
    ck = train.Checkpoint.from_directory(os.path.join(a.path, "checkpoint_000000"))  # after step 2
    b = W.train_workload("llama3-tiny", checkpoint_storage_path=str(tmp_path / "b"), checkpoint=ck,
                         resume_mode="exact", **kw)
    assert _losses(b.path) == {3: la[3], 4: la[4]}
