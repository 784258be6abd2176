"""Sliding-window causal flash attention on the GPU, alone and with packed documents: the twelve
MASK_WIN instantiations of attn_flash.hip.

A window W gives row q the low bound lo[q] = max(start[q], q - W + 1) and key k the high bound
hi[k] = min(end[k], k + W): bounds of the same shape as a document layout's.  So the yardstick is
the one of the document mask, tests/ulp.py::attn_ref with the clipped arrays (start', end') as
its `docs`, every output judged per element against fp64 (score <= 1); and the DOC kernels fed
those arrays as a DocLayout must give the same bits, since the live arithmetic is the same.
The rest are the properties a window adds: tiles outside the band are skipped (never read), W = 1
returns V, W >= T is the unwindowed call.

RTDC_FA_FWD / RTDC_FA_DQ / RTDC_FA_DKDV are read per call, so one process runs the 16- and the
32-row variants; T = 192 forces the 64-row kernels.  The WORST lines of one run are kept in
profiles/attn_window_ulp.md.
"""
import math

import pytest
import torch

from tests import ulp as U

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32 = U.F64, U.F32
CASES = [U.ATTN_CASES[i] for i in (2, 5, 7, 8, 10)]
LAYOUTS = (None, "A")
KNOBS = [(1, 1, 1), (2, 2, 2)]
_refs: dict = {}


def _windows(T):
    return [1, 17, 64, 65, 100, T - 1]


def _ext():
    from ray_torch_distributed_checkpoint_amd.ops._ext import gpu_ext

    return gpu_ext()


def _clipped(B, T, W, arr):
    """(start', end') int64 [B, T]: the document bounds (0 / T without documents) clipped to the band"""
    t = torch.arange(T, device=DEV)[None, :].expand(B, T)
    start = torch.zeros_like(t) if arr is None else arr[0]
    end = torch.full_like(t, T) if arr is None else arr[1]
    return torch.maximum(start, t - W + 1), torch.minimum(end, t + W)


def _case(c, layout, W):
    """inputs, document layout, the clipped layout, fp64 reference (with the allowance) and twin of
    one (case, layout, W): computed once, shared, never modified"""
    from ray_torch_distributed_checkpoint_amd.ops import DocLayout

    key = (c, layout, W)
    if key not in _refs:
        B, T, H, Hkv, Dh, gen = c
        x = U.attn_inputs(gen, B, T, H, Hkv, Dh, dev=DEV)
        docs = arr = None
        if layout is not None:
            lengths = U.attn_layout(layout, T, B)
            docs, arr = DocLayout.from_lengths(lengths, T, DEV), U.doc_arrays(lengths, T, DEV)
        clip = _clipped(B, T, W, arr)
        cdocs = DocLayout(clip[0].to(torch.int32).contiguous(), clip[1].to(torch.int32).contiguous())
        a = (x["qkv"], x["dout"], B, T, H, Hkv, Dh, clip)
        _refs[key] = (x, docs, cdocs, U.attn_ref(F64, *a), U.attn_ref(F32, *a, twin=True))
    return _refs[key]


def _set_knobs(monkeypatch, v, qs):
    for name, val in zip(("RTDC_FA_FWD", "RTDC_FA_DQ", "RTDC_FA_DKDV"), v):
        monkeypatch.setenv(name, str(val))
    monkeypatch.setenv("RTDC_FA_QS", str(qs))


def _families(c, v, qs):
    f, d, kv = (fam + "_win" for fam, _, _ in U.attn_launches(*c[:5], v, qs))
    return {"out": f, "lse": f, "delta": d, "dq": d, "dk": kv, "dv": kv}


def _split(grad, H, Hkv, Dh):
    C, KV = H * Dh, Hkv * Dh
    return {"dq": grad[..., :C], "dk": grad[..., C:C + KV], "dv": grad[..., C + KV:]}


def _run(qkv, dout, H, Hkv, finite=True, **kw):
    from ray_torch_distributed_checkpoint_amd.ops import causal_attention

    q = qkv.clone().requires_grad_(True)
    out = causal_attention(q, H, Hkv, **kw)
    out.backward(dout)
    torch.cuda.synchronize()
    if finite:
        assert torch.isfinite(out.float()).all() and torch.isfinite(q.grad.float()).all()
    return out.detach(), q.grad


@pytest.mark.parametrize("layout", LAYOUTS, ids=["plain", "A"])
@pytest.mark.parametrize("c", CASES, ids=U.attn_case_id)
def test_window_per_element(monkeypatch, c, layout):
    """causal_attention(window=W[, docs]) + backward: every W x variant knobs x head split, each of
    out, dQ, dK, dV inside its per-element allowance under the clipped bounds"""
    B, T, H, Hkv, Dh, _ = c
    monkeypatch.delenv("RTDC_ATTN", raising=False)
    J = U.Judge()
    for W in _windows(T):
        x, docs, _, ref, twin = _case(c, layout, W)
        for v in KNOBS:
            for qs in U.attn_head_splits(H, Hkv):
                _set_knobs(monkeypatch, v, qs)
                out, grad = _run(x["qkv"], x["dout"], H, Hkv, docs=docs, window=W)
                shape = "%s %s W%d v%d%d%d qs%d" % (U.attn_case_id(c), layout or "plain", W, *v, qs)
                U.judge_attn(J, _families(c, v, qs), shape, ref, twin, {"out": out, **_split(grad, H, Hkv, Dh)})
    J.check()


def _guarded(n0, rest, dtype):
    """a [n0, *rest] dim-0 slice of a NaN-filled buffer with one guard slab on either side"""
    big = torch.full((n0 + 2, *rest), float("nan"), dtype=dtype, device=DEV)
    return big, big[1:n0 + 1]


@pytest.mark.parametrize("layout", LAYOUTS, ids=["plain", "A"])
def test_launchers_guarded(monkeypatch, layout):
    """flash_fwd_win / flash_bwd_win called directly, both row variants, qs 1 and 2: lse and delta
    judged as well; every output is a slice of a NaN-filled buffer - inside everything is written,
    outside nothing is"""
    c, W = U.ATTN_CASES[7], 100
    B, T, H, Hkv, Dh, _ = c
    Wd, C, scale = (H + 2 * Hkv) * Dh, H * Dh, 1.0 / math.sqrt(Dh)
    x, docs, _, ref, twin = _case(c, layout, W)
    st, en = (docs.start, docs.end) if docs is not None else (None, None)
    J = U.Judge()
    for v in KNOBS:
        for qs in (1, 2):
            _set_knobs(monkeypatch, v, qs)
            bufs = {"out": _guarded(B, (T, C), U.BF16), "lse": _guarded(B * H, (T,), F32),
                    "delta": _guarded(B * H, (T,), F32), "dqkv": _guarded(B, (T, Wd), U.BF16)}
            out, lse, delta, dqkv = (bufs[n][1] for n in ("out", "lse", "delta", "dqkv"))
            part = torch.empty(qs * B * T * Hkv * 2 * Dh, dtype=F32, device=DEV) if qs > 1 else None
            _ext().flash_fwd_win(x["qkv"], out, lse, W, st, en, B, T, H, Hkv, Dh, scale)
            _ext().flash_bwd_win(x["qkv"], out, x["dout"], lse, delta, dqkv, W, st, en, B, T, H, Hkv, Dh, scale,
                                 None, part, qs)
            torch.cuda.synchronize()
            for name, (big, inner) in bufs.items():
                assert torch.isfinite(inner.float()).all(), f"{name}: an element no block wrote (or a non-finite value)"
                assert torch.isnan(big[0]).all() and torch.isnan(big[-1]).all(), f"{name}: a store outside the tensor"
            outs = {"out": out, "lse": lse, "delta": delta, **_split(dqkv, H, Hkv, Dh)}
            shape = "%s %s W%d v%d%d%d qs%d direct" % (U.attn_case_id(c), layout or "plain", W, *v, qs)
            U.judge_attn(J, _families(c, v, qs), shape, ref, twin, outs, U.ATTN_OUTPUTS)
    J.check()


def test_launcher_argument_checks():
    """window >= 1, and the layout arrays both or neither"""
    c = U.ATTN_CASES[2]
    B, T, H, Hkv, Dh, _ = c
    x, docs, _, _, _ = _case(c, "A", 17)
    out = torch.empty(B, T, H * Dh, dtype=U.BF16, device=DEV)
    lse = torch.empty(B * H, T, dtype=F32, device=DEV)
    with pytest.raises(RuntimeError, match="window"):
        _ext().flash_fwd_win(x["qkv"], out, lse, 0, None, None, B, T, H, Hkv, Dh, 0.125)
    with pytest.raises(RuntimeError, match="together"):
        _ext().flash_fwd_win(x["qkv"], out, lse, 17, docs.start, None, B, T, H, Hkv, Dh, 0.125)


@pytest.mark.parametrize("layout", LAYOUTS, ids=["plain", "A"])
@pytest.mark.parametrize("c", CASES, ids=U.attn_case_id)
def test_bitwise_against_doc_kernels_on_clipped_layouts(monkeypatch, c, layout):
    """The DOC kernels fed (start', end') do the same arithmetic on the live elements, and a fully
    masked tile adds exact zeros: out and dqkv agree bit for bit."""
    B, T, H, Hkv, Dh, _ = c
    monkeypatch.delenv("RTDC_ATTN", raising=False)
    for W in _windows(T):
        x, docs, cdocs, _, _ = _case(c, layout, W)
        for v in KNOBS:
            for qs in U.attn_head_splits(H, Hkv):
                _set_knobs(monkeypatch, v, qs)
                out, grad = _run(x["qkv"], x["dout"], H, Hkv, docs=docs, window=W)
                dout, dgrad = _run(x["qkv"], x["dout"], H, Hkv, docs=cdocs)
                assert torch.equal(out, dout), (W, v, qs)
                assert torch.equal(grad, dgrad), (W, v, qs)


@pytest.mark.parametrize("v", KNOBS, ids=["v1", "v2"])
@pytest.mark.parametrize("H,Hkv,Dh", [(4, 4, 64), (4, 2, 128)])
def test_tiles_outside_the_band_are_never_read(monkeypatch, H, Hkv, Dh, v):
    """T = 384, W = 64.  Rows >= 256 see keys >= 193 only: their blocks (128 rows, or 64) start the
    key loop at tile 3, so NaN in the K / V rows of tile 0 cannot reach them - a tile that is
    visited and masked would spread it through 0 x NaN in the MFMA.  Likewise keys < 128 are seen
    by rows < 191 only: their blocks end the query loop at tile 2, and NaN in dout rows >= 256
    stays out of their dK / dV."""
    _set_knobs(monkeypatch, v, 1)
    B, T, W = 2, 384, 64
    C, KV = H * Dh, Hkv * Dh
    x = U.attn_inputs("randn", B, T, H, Hkv, Dh, dev=DEV)
    qkv = x["qkv"].clone()
    qkv[:, :64, C:] = float("nan")
    out, grad = _run(qkv, x["dout"], H, Hkv, finite=False, window=W)
    assert torch.isfinite(out[:, 256:].float()).all()
    assert torch.isfinite(grad[:, 256:, :C].float()).all()
    assert torch.isnan(out[:, :64].float()).any()  # (the NaN rows are read where the band holds them)
    dout = x["dout"].clone()
    dout[:, 256:] = float("nan")
    out, grad = _run(x["qkv"], dout, H, Hkv, finite=False, window=W)
    assert torch.isfinite(out.float()).all()
    assert torch.isfinite(grad[:, :128, C:].float()).all()
    assert torch.isnan(grad[:, 256:, C:].float()).any()


@pytest.mark.parametrize("v", KNOBS, ids=["v1", "v2"])
@pytest.mark.parametrize("c", [U.ATTN_CASES[5], U.ATTN_CASES[8], U.ATTN_CASES[10]], ids=U.attn_case_id)
def test_window_of_one_returns_v(monkeypatch, c, v):
    """Every row attends to itself alone: p = 1 and l = 1, so out is the V head the q-head maps to"""
    B, T, H, Hkv, Dh, _ = c
    _set_knobs(monkeypatch, v, 1)
    x = _case(c, None, 1)[0]
    out, _ = _run(x["qkv"], x["dout"], H, Hkv, window=1)
    vheads = x["qkv"][..., (H + Hkv) * Dh:].view(B, T, Hkv, Dh).repeat_interleave(H // Hkv, dim=2)
    assert torch.equal(out.view(B, T, H, Dh), vheads)


@pytest.mark.parametrize("v", KNOBS, ids=["v1", "v2"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=["plain", "A"])
@pytest.mark.parametrize("c", [U.ATTN_CASES[5], U.ATTN_CASES[8]], ids=U.attn_case_id)
def test_window_of_the_whole_row_is_the_call_without(monkeypatch, c, layout, v):
    B, T, H, Hkv, Dh, _ = c
    _set_knobs(monkeypatch, v, 1)
    x, docs = _case(c, layout, 17)[:2]
    ref = _run(x["qkv"], x["dout"], H, Hkv, docs=docs)
    for W in (T, T + 5):
        got = _run(x["qkv"], x["dout"], H, Hkv, docs=docs, window=W)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), W


@pytest.mark.parametrize("v", KNOBS, ids=["v1", "v2"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=["plain", "A"])
@pytest.mark.parametrize("c", [U.ATTN_CASES[7], U.ATTN_CASES[8]], ids=U.attn_case_id)
def test_deterministic(monkeypatch, c, layout, v):
    B, T, H, Hkv, Dh, _ = c
    x, docs = _case(c, layout, 100)[:2]
    for qs in U.attn_head_splits(H, Hkv):
        _set_knobs(monkeypatch, v, qs)
        a = _run(x["qkv"], x["dout"], H, Hkv, docs=docs, window=100)
        b = _run(x["qkv"], x["dout"], H, Hkv, docs=docs, window=100)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _close(out, ref, rel):
    err = (out.float() - ref.float()).abs().max().item()
    mag = ref.float().abs().max().item() + 1e-6
    assert err <= rel * mag, f"max err {err} vs {rel}*{mag}"


@pytest.mark.parametrize("v", KNOBS, ids=["v1", "v2"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=["plain", "A"])
@pytest.mark.parametrize("c", [U.ATTN_CASES[7], U.ATTN_CASES[8]], ids=U.attn_case_id)
def test_colsum_partials(monkeypatch, c, layout, v):
    """The per-16-row column sums the window backward offers equal those of the dqkv it stored
    (qs 1: written by the dK/dV kernel; qs 2: by the head-split reduction)."""
    from ray_torch_distributed_checkpoint_amd.ops import causal_attention
    from ray_torch_distributed_checkpoint_amd.ops import gemm as G

    B, T, H, Hkv, Dh, _ = c
    x, docs = _case(c, layout, 100)[:2]
    monkeypatch.setattr(G, "partials_wanted", lambda: True)
    for qs in U.attn_head_splits(H, Hkv)[:2]:
        _set_knobs(monkeypatch, v, qs)
        # the consumer of dqkv in a model is the qkv projection's backward, which sees the tensor
        # the attention backward returned; a hook on a non-leaf input sees that same tensor
        q = x["qkv"].clone().requires_grad_(True) * 1
        got = []
        q.register_hook(got.append)
        causal_attention(q, H, Hkv, docs=docs, window=100).backward(x["dout"])
        d2 = got[0].view(-1, q.shape[-1])
        ref = d2.float().sum(0)
        rows = G._take_partials(d2)
        assert rows is not None  # the window backward did offer them
        _close(rows.sum(0), ref, 1e-5)
        G.offer_colsum_partials(got[0], rows)
        cs = G.colsum(d2)
        torch.cuda.synchronize()
        _close(cs, ref, 1e-5)
        assert G._take_partials(d2) is None  # consumed: the partials were offered and used


def test_window_needs_the_flash_path(monkeypatch):
    from ray_torch_distributed_checkpoint_amd.ops import causal_attention

    H, Dh = 4, 64
    monkeypatch.delenv("RTDC_ATTN", raising=False)
    qkv = torch.randn(1, 100, 3 * H * Dh, device=DEV).to(torch.bfloat16)
    with pytest.raises(RuntimeError, match="sliding window"):
        causal_attention(qkv, H, window=32)
    monkeypatch.setenv("RTDC_ATTN", "gemm")
    qkv = torch.randn(1, 128, 3 * H * Dh, device=DEV).to(torch.bfloat16)
    with pytest.raises(RuntimeError, match="sliding window"):
        causal_attention(qkv, H, window=32)
    with pytest.raises(ValueError, match="window"):
        causal_attention(qkv, H, window=0)
