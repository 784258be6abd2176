"""Document-masked causal flash attention (packed sequences) on the GPU: all six DOC kernels of
attn_flash.hip at both head sizes, against fp32 SDPA under the boolean mask start[q] <= k <= q,
plus the bitwise properties a mask leak, a wrong ring base or a NaN from a fully masked tile
would break.  RTDC_FA_FWD / RTDC_FA_DQ / RTDC_FA_DKDV are read per call, so one process runs
the 16- and the 32-row variants; T = 192 forces the 64-row kernels.
"""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(4, 4, 64), (4, 2, 128)]  # (H, Hkv, Dh)
B = 2
# layout A (batch row 0): a boundary inside the first wave (5); one at 70, so rows 64-69 of the
# second block continue a document from tile 0 while rows 72+ of the same wave see tile 0 fully
# masked with the running max still at its start value; two documents of length 1; a boundary
# (130) mid-wave in a block whose first key tile is 1.  Batch row 1 is a single document, which
# catches a layout indexed without the batch.
LAYOUT_A = {256: [[5, 65, 1, 1, 58, 126], [256]], 192: [[5, 65, 1, 1, 58, 62], [192]]}
VARIANTS = list(itertools.product((1, 2), repeat=3))  # (FWD, DQ, DKDV)


def _bf(*shape):
    return torch.randn(*shape, device=DEV).to(torch.bfloat16)


def _close(out, ref, rel):
    err = (out.float() - ref.float()).abs().max().item()
    mag = ref.float().abs().max().item() + 1e-6
    assert err <= rel * mag, f"max err {err} vs {rel}*{mag}"


def _set_variant(monkeypatch, v):
    fwd, dq, dkdv = v
    monkeypatch.setenv("RTDC_FA_FWD", str(fwd))
    monkeypatch.setenv("RTDC_FA_DQ", str(dq))
    monkeypatch.setenv("RTDC_FA_DKDV", str(dkdv))


def _docs(lengths, T):
    from ray_torch_distributed_checkpoint_amd.ops import DocLayout

    return DocLayout.from_lengths(lengths, T, DEV)


_cases: dict = {}


def _case(H, Hkv, Dh, T, name, lengths):
    """Inputs and the fp32 oracle of one (shape, layout): computed once, shared, never modified."""
    from ray_torch_distributed_checkpoint_amd.ops.attention import causal_attention_ref

    key = (H, Hkv, Dh, T, name)
    c = _cases.get(key)
    if c is None:
        torch.manual_seed(11 + Dh + T)
        W = (H + 2 * Hkv) * Dh
        qkv, g = _bf(B, T, W), _bf(B, T, H * Dh)
        docs = _docs(lengths, T)
        qr = qkv.float().requires_grad_(True)
        ref = causal_attention_ref(qr, B, T, H, Hkv, Dh, docs)
        ref.backward(g.float())
        c = _cases[key] = (qkv, g, docs, ref.detach(), qr.grad.detach())
    return c


def _run(qkv, g, H, Hkv, docs):
    from ray_torch_distributed_checkpoint_amd.ops import causal_attention

    x = qkv.clone().requires_grad_(True)
    out = causal_attention(x, H, Hkv, docs=docs)
    out.backward(g)
    torch.cuda.synchronize()
    return out.detach(), x.grad


def _check_oracle(H, Hkv, Dh, T, name, lengths):
    qkv, g, docs, ref, rgrad = _case(H, Hkv, Dh, T, name, lengths)
    out, grad = _run(qkv, g, H, Hkv, docs)
    assert torch.isfinite(out.float()).all() and torch.isfinite(grad.float()).all()
    _close(out, ref, 2e-2)
    _close(grad, rgrad, 3e-2)


@pytest.mark.parametrize("v", VARIANTS, ids=lambda v: "fwd%d-dq%d-dkdv%d" % v)
@pytest.mark.parametrize("H,Hkv,Dh", SHAPES)
def test_oracle_layout_a(monkeypatch, H, Hkv, Dh, v):
    _set_variant(monkeypatch, v)
    _check_oracle(H, Hkv, Dh, 256, "A", LAYOUT_A[256])


@pytest.mark.parametrize("H,Hkv,Dh", SHAPES)
def test_oracle_layout_a_64row(H, Hkv, Dh):
    """T = 192 is no multiple of 128: the 64-row kernels run whatever the variant asks for."""
    _check_oracle(H, Hkv, Dh, 192, "A", LAYOUT_A[192])


@pytest.mark.parametrize("v", [(1, 1, 1), (2, 2, 2)], ids=["v1", "v2"])
@pytest.mark.parametrize("T", [256, 192])
@pytest.mark.parametrize("H,Hkv,Dh", SHAPES)
def test_single_document_is_plain_causal(monkeypatch, H, Hkv, Dh, T, v):
    """start = 0 everywhere: the same tiles in the same order and masks that never fire, so the
    DOC kernels give the bits of the plain ones."""
    from ray_torch_distributed_checkpoint_amd.ops import causal_attention

    _set_variant(monkeypatch, v)
    qkv, g = _case(H, Hkv, Dh, T, "A", LAYOUT_A[T])[:2]
    out, grad = _run(qkv, g, H, Hkv, _docs([[T], [T]], T))
    x = qkv.clone().requires_grad_(True)
    pout = causal_attention(x, H, Hkv)
    pout.backward(g)
    assert torch.equal(out, pout.detach())
    assert torch.equal(grad, x.grad)


@pytest.mark.parametrize("v", [(1, 1, 1), (2, 2, 2)], ids=["v1", "v2"])
@pytest.mark.parametrize("T", [256, 192])
@pytest.mark.parametrize("H,Hkv,Dh", SHAPES)
def test_isolation_bitwise(monkeypatch, H, Hkv, Dh, T, v):
    """New values in the document at rows 5-69 (inputs and upstream gradient) leave every bit
    of every other row alone; one leaked masked score would change bits."""
    _set_variant(monkeypatch, v)
    qkv, g, docs = _case(H, Hkv, Dh, T, "A", LAYOUT_A[T])[:3]
    out, grad = _run(qkv, g, H, Hkv, docs)
    torch.manual_seed(99)
    q2, g2 = qkv.clone(), g.clone()
    q2[0, 5:70] = _bf(65, qkv.shape[-1])
    g2[0, 5:70] = _bf(65, g.shape[-1])
    out2, grad2 = _run(q2, g2, H, Hkv, docs)
    keep = torch.ones(B, T, dtype=torch.bool, device=DEV)
    keep[0, 5:70] = False
    assert torch.equal(out[keep], out2[keep])
    assert torch.equal(grad[keep], grad2[keep])
    assert not torch.equal(out[~keep], out2[~keep])  # (the edit did reach its own document)


@pytest.mark.parametrize("v", [(1, 1, 1), (2, 2, 2)], ids=["v1", "v2"])
@pytest.mark.parametrize("H,Hkv,Dh", SHAPES)
def test_tile_aligned_documents(monkeypatch, H, Hkv, Dh, v):
    """Pure block skipping: no tile needs the low mask."""
    _set_variant(monkeypatch, v)
    _check_oracle(H, Hkv, Dh, 256, "aligned", [[64, 128, 64], [128, 64, 64]])


@pytest.mark.parametrize("v", [(1, 1, 1), (2, 2, 2)], ids=["v1", "v2"])
@pytest.mark.parametrize("H,Hkv,Dh", SHAPES)
def test_all_documents_of_length_one(monkeypatch, H, Hkv, Dh, v):
    """Every row attends to itself alone: p = 1 and l = 1, so out is the V head the q-head maps
    to, bit for bit; dQ and dK vanish."""
    _set_variant(monkeypatch, v)
    T = 256
    qkv, g, docs, ref, rgrad = _case(H, Hkv, Dh, T, "ones", [[1] * T, [1] * T])
    out, grad = _run(qkv, g, H, Hkv, docs)
    C = H * Dh
    vheads = qkv[..., C + Hkv * Dh:].view(B, T, Hkv, Dh).repeat_interleave(H // Hkv, dim=2)
    assert torch.equal(out.view(B, T, H, Dh), vheads)
    _close(grad, rgrad, 3e-2)
    bound = 3e-2 * (rgrad.abs().max().item() + 1e-6)
    assert grad[..., : C + Hkv * Dh].float().abs().max().item() <= bound


@pytest.mark.parametrize("v", [(1, 1, 1), (2, 2, 2)], ids=["v1", "v2"])
@pytest.mark.parametrize("H,Hkv,Dh", SHAPES)
def test_deterministic(monkeypatch, H, Hkv, Dh, v):
    _set_variant(monkeypatch, v)
    qkv, g, docs = _case(H, Hkv, Dh, 256, "A", LAYOUT_A[256])[:3]
    a = _run(qkv, g, H, Hkv, docs)
    b = _run(qkv, g, H, Hkv, docs)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("v", [(1, 1, 1), (2, 2, 2)], ids=["v1", "v2"])
@pytest.mark.parametrize("H,Hkv,Dh", SHAPES)
def test_colsum_partials(monkeypatch, H, Hkv, Dh, v):
    """The per-16-row column sums the DOC backward offers equal those of the dqkv it stored."""
    from ray_torch_distributed_checkpoint_amd.ops import causal_attention
    from ray_torch_distributed_checkpoint_amd.ops import gemm as G

    _set_variant(monkeypatch, v)
    qkv, g, docs = _case(H, Hkv, Dh, 256, "A", LAYOUT_A[256])[:3]
    # the consumer of dqkv in a model is the qkv projection's backward, which sees the tensor
    # the attention backward returned; a hook on a non-leaf input sees that same tensor
    x = qkv.clone().requires_grad_(True) * 1
    got = []
    x.register_hook(got.append)
    monkeypatch.setattr(G, "partials_wanted", lambda: True)
    causal_attention(x, H, Hkv, docs=docs).backward(g)
    d2 = got[0].view(-1, x.shape[-1])
    ref = d2.float().sum(0)
    rows = G._take_partials(d2)
    assert rows is not None  # the DOC backward did offer them
    _close(rows.sum(0), ref, 1e-5)
    G.offer_colsum_partials(got[0], rows)
    cs = G.colsum(d2)
    torch.cuda.synchronize()
    _close(cs, ref, 1e-5)
    assert G._take_partials(d2) is None  # consumed: the partials were offered and used


@pytest.mark.parametrize("H,Hkv,Dh", SHAPES)
def test_rope_per_document(H, Hkv, Dh):
    """apply_rope with docs, forward and backward, is bit for bit apply_rope of each document as
    a [1, L, W] tensor of its own."""
    from ray_torch_distributed_checkpoint_amd.ops.llama_ops import apply_rope

    T, theta = 256, 500000.0
    W = (H + 2 * Hkv) * Dh
    torch.manual_seed(21)
    x, g = _bf(B, T, W), _bf(B, T, W)
    lengths = LAYOUT_A[T]
    xd = x.clone().requires_grad_(True)
    y = apply_rope(xd, H, Hkv, theta, docs=_docs(lengths, T))
    y.backward(g)
    for b, row in enumerate(lengths):
        at = 0
        for n in row:
            xs = x[b:b + 1, at:at + n].clone().requires_grad_(True)
            ys = apply_rope(xs, H, Hkv, theta)
            ys.backward(g[b:b + 1, at:at + n].contiguous())
            assert torch.equal(y[b:b + 1, at:at + n], ys), (b, at, n)
            assert torch.equal(xd.grad[b:b + 1, at:at + n], xs.grad), (b, at, n)
            at += n


def test_layout_kernel_matches_cpu():
    """The one-launch flags -> (start, end) kernel against the torch scans, at sizes around its
    per-thread chunking (T below, at and above the block size; odd T)."""
    from ray_torch_distributed_checkpoint_amd.ops import DocLayout

    torch.manual_seed(3)
    for T in (1, 7, 255, 256, 257, 1000, 2048):
        flags = (torch.rand(3, T) < 0.05).to(torch.uint8)
        flags[1] = 0
        flags[2] = 1
        cpu, gpu = DocLayout.from_flags(flags), DocLayout.from_flags(flags.to(DEV))
        assert torch.equal(cpu.start, gpu.start.cpu()) and torch.equal(cpu.end, gpu.end.cpu()), T


def test_docs_need_the_flash_path(monkeypatch):
    from ray_torch_distributed_checkpoint_amd.ops import causal_attention

    H, Dh = 4, 64
    with pytest.raises(RuntimeError, match="document masking"):
        causal_attention(_bf(1, 100, 3 * H * Dh), H, docs=_docs([[40, 60]], 100))
    monkeypatch.setenv("RTDC_ATTN", "gemm")
    with pytest.raises(RuntimeError, match="document masking"):
        causal_attention(_bf(1, 128, 3 * H * Dh), H, docs=_docs([[40, 88]], 128))
