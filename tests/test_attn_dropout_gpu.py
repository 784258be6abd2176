"""Attention dropout in the flash kernels on the GPU (the DROP instantiations of attn_flash.hip).

The mask is read back exactly through inputs that make the output a picture of it; out, dQ, dK, dV
(and lse, delta through the launchers) are judged per element against the fp64 reference of
tests/attn_dropout_ref.py (score <= 1); and the bitwise properties: reproducible from the stream
state, one mask under every variant knob and head split, off = the plain call, host / device split
of the counter base, hipGraph replays.

RTDC_FA_FWD / RTDC_FA_DQ / RTDC_FA_DKDV / RTDC_FA_QS are read per call, so one process runs every
variant; T = 64 and 192 force the 64-row kernels.  The WORST lines of one run are kept in
profiles/attn_dropout_ulp.txt.
"""
import math

import pytest
import torch

from tests import ulp as U
from tests.attn_dropout_ref import attn_drop_ref, clipped

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32 = U.F64, U.F32
KNOBS = [(1, 1, 1), (2, 2, 2)]
SEED = 0x1234ABCD5EED
# (B, T, H, Hkv, Dh, generator): T = 64 one tile, 128 the first size of the 32-row kernels, 192 the
# 64-row kernels with a wrapped ring, 256 two 128-row blocks; both head sizes; groups of 2 and 4
CASES = [(2, 64, 4, 2, 64, "randn"), (2, 128, 4, 1, 128, "peaky"), (2, 192, 4, 2, 128, "randn"),
         (2, 256, 4, 1, 64, "randn"), (1, 256, 4, 2, 128, "peaky")]
MODES = ("plain", "A", "W48", "A+W48")
_refs: dict = {}


def _ext():
    from ray_torch_distributed_checkpoint_amd.ops._ext import gpu_ext

    return gpu_ext()


def _stream(offset):
    from ray_torch_distributed_checkpoint_amd.ops import PhiloxStream

    return PhiloxStream(SEED, offset)


def _set_knobs(monkeypatch, v, qs):
    for name, val in zip(("RTDC_FA_FWD", "RTDC_FA_DQ", "RTDC_FA_DKDV"), v):
        monkeypatch.setenv(name, str(val))
    monkeypatch.setenv("RTDC_FA_QS", str(qs))


def _mode(mode, B, T):
    """(DocLayout or None, window or None, the clipped arrays the reference takes as docs)"""
    from ray_torch_distributed_checkpoint_amd.ops import DocLayout

    docs = arr = None
    if mode.startswith("A"):
        lengths = U.attn_layout("A", T, B)
        docs, arr = DocLayout.from_lengths(lengths, T, DEV), U.doc_arrays(lengths, T, DEV)
    W = 48 if mode.endswith("W48") else None
    return docs, W, clipped(B, T, W, arr, DEV)


def _case(c, mode, p, offset):
    """inputs, layout, window, fp64 reference (with the allowance) and twin: computed once, shared,
    never modified"""
    key = (c, mode, p, offset)
    if key not in _refs:
        B, T, H, Hkv, Dh, gen = c
        x = U.attn_inputs(gen, B, T, H, Hkv, Dh, dev=DEV)
        docs, W, clip = _mode(mode, B, T)
        a = (x["qkv"], x["dout"], B, T, H, Hkv, Dh, SEED, offset, p, clip)
        _refs[key] = (x, docs, W, attn_drop_ref(F64, *a), attn_drop_ref(F32, *a, twin=True))
    return _refs[key]


def _families(c, v, qs):
    f, d, kv = (fam + "_drop" for fam, _, _ in U.attn_launches(*c[:5], v, qs))
    return {"out": f, "lse": f, "delta": d, "dq": d, "dk": kv, "dv": kv}


def _split(grad, H, Hkv, Dh):
    C, KV = H * Dh, Hkv * Dh
    return {"dq": grad[..., :C], "dk": grad[..., C:C + KV], "dv": grad[..., C + KV:]}


def _run(qkv, dout, H, Hkv, **kw):
    from ray_torch_distributed_checkpoint_amd.ops import causal_attention

    q = qkv.clone().requires_grad_(True)
    out = causal_attention(q, H, Hkv, **kw)
    out.backward(dout)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all() and torch.isfinite(q.grad.float()).all()
    return out.detach(), q.grad


# ---------------------------------------------------------------- 1. the mask, read back exactly
@pytest.mark.parametrize("qs", [1, 2])
@pytest.mark.parametrize("v", KNOBS, ids=["v111", "v222"])
@pytest.mark.parametrize("T", [64, 128])
def test_mask_read_back_exactly(monkeypatch, T, v, qs):
    """q = k = 0 makes P uniform over the causal prefix and V = I (T = Dh) makes out[q, j] = P Z:
    non-zero iff (q, j) is kept.  dO = I on one q-head of each group makes dV[j, q] the same
    picture of that head.  Both equal attention_dropout_mask exactly, for every b and h, with a
    counter base that carries across the 32-bit word - under every variant knob and head split,
    so they all draw one mask."""
    from ray_torch_distributed_checkpoint_amd.ops import attention_dropout_mask, causal_attention

    B, H, Hkv, Dh, p, off = 2, 4, 2, T, 0.1, 2 ** 32 - 5
    grp, C, KV = H // Hkv, H * Dh, Hkv * Dh
    _set_knobs(monkeypatch, v, qs)
    eye = torch.eye(T, device=DEV)
    qkv = torch.zeros(B, T, C + 2 * KV, device=DEV)
    qkv[..., C + KV:] = eye.repeat(1, Hkv)[None]
    qkv = qkv.to(U.BF16)
    tri = torch.tril(torch.ones(T, T, dtype=torch.bool, device=DEV))
    M = attention_dropout_mask(SEED, off, B, H, T, p).to(DEV) & tri
    assert 0.85 < M[:, :, tri].float().mean().item() < 0.95
    for g in range(grp):
        dout = torch.zeros(B, T, H, Dh, device=DEV)
        dout[:, :, g::grp] = eye[None, :, None, :]
        x = qkv.clone().requires_grad_(True)
        out = causal_attention(x, H, Hkv, dropout_p=p, stream=_stream(off))
        out.backward(dout.reshape(B, T, C).to(U.BF16))
        torch.cuda.synchronize()
        got = out.detach().view(B, T, H, Dh).permute(0, 2, 1, 3) != 0          # [B, H, q, j]
        assert torch.equal(got, M), (v, qs, "out")
        dv = x.grad[..., C + KV:].view(B, T, Hkv, Dh).permute(0, 2, 3, 1) != 0   # [B, Hkv, q, j]
        assert torch.equal(dv, M[:, g::grp]), (v, qs, g, "dV")


# ---------------------------------------------------------------- 2. the per-element judge
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", CASES, ids=U.attn_case_id)
def test_dropout_per_element(monkeypatch, c, mode):
    """causal_attention(dropout_p=) + backward: p x variant knobs x head split, each of out, dQ, dK,
    dV inside its per-element allowance"""
    B, T, H, Hkv, Dh, _ = c
    monkeypatch.delenv("RTDC_ATTN", raising=False)
    J = U.Judge()
    for p in (0.1, 0.5):
        x, docs, W, ref, twin = _case(c, mode, p, 1000)
        for v in KNOBS:
            for qs in (1, 2):
                _set_knobs(monkeypatch, v, qs)
                out, grad = _run(x["qkv"], x["dout"], H, Hkv, docs=docs, window=W, dropout_p=p, stream=_stream(1000))
                shape = "%s %s p%.1f v%d%d%d qs%d" % (U.attn_case_id(c), mode, p, *v, qs)
                U.judge_attn(J, _families(c, v, qs), shape, ref, twin, {"out": out, **_split(grad, H, Hkv, Dh)})
    J.check()


def _guarded(n0, rest, dtype):
    """a [n0, *rest] dim-0 slice of a NaN-filled buffer with one guard slab on either side"""
    big = torch.full((n0 + 2, *rest), float("nan"), dtype=dtype, device=DEV)
    return big, big[1:n0 + 1]


@pytest.mark.parametrize("mode", ["plain", "A+W48"])
def test_launchers_guarded(monkeypatch, mode):
    """flash_fwd_drop / flash_bwd_drop called directly, both row variants, qs 1 and 2: lse and delta
    judged as well; every output is a slice of a NaN-filled buffer - inside everything is written,
    outside nothing is"""
    from ray_torch_distributed_checkpoint_amd.ops import attention_dropout_keep

    c, p, off = (2, 256, 4, 2, 64, "randn"), 0.1, 77
    B, T, H, Hkv, Dh, _ = c
    Wd, C, scale = (H + 2 * Hkv) * Dh, H * Dh, 1.0 / math.sqrt(Dh)
    thr = attention_dropout_keep(p)[0]
    x, docs, W, ref, twin = _case(c, mode, p, off)
    st, en = (docs.start, docs.end) if docs is not None else (None, None)
    J = U.Judge()
    for v in KNOBS:
        for qs in (1, 2):
            _set_knobs(monkeypatch, v, qs)
            bufs = {"out": _guarded(B, (T, C), U.BF16), "lse": _guarded(B * H, (T,), F32),
                    "delta": _guarded(B * H, (T,), F32), "dqkv": _guarded(B, (T, Wd), U.BF16)}
            out, lse, delta, dqkv = (bufs[n][1] for n in ("out", "lse", "delta", "dqkv"))
            part = torch.empty(qs * B * T * Hkv * 2 * Dh, dtype=F32, device=DEV) if qs > 1 else None
            _ext().flash_fwd_drop(x["qkv"], out, lse, W or 0, st, en, thr, SEED, off, None, B, T, H, Hkv, Dh, scale)
            _ext().flash_bwd_drop(x["qkv"], out, x["dout"], lse, delta, dqkv, W or 0, st, en, thr, SEED, off, None,
                                  B, T, H, Hkv, Dh, scale, None, part, qs)
            torch.cuda.synchronize()
            for name, (big, inner) in bufs.items():
                assert torch.isfinite(inner.float()).all(), f"{name}: an element no block wrote (or a non-finite value)"
                assert torch.isnan(big[0]).all() and torch.isnan(big[-1]).all(), f"{name}: a store outside the tensor"
            outs = {"out": out, "lse": lse, "delta": delta, **_split(dqkv, H, Hkv, Dh)}
            shape = "%s %s p%.1f v%d%d%d qs%d direct" % (U.attn_case_id(c), mode, p, *v, qs)
            U.judge_attn(J, _families(c, v, qs), shape, ref, twin, outs, U.ATTN_OUTPUTS)
    J.check()


def test_launcher_argument_checks():
    c = CASES[0]
    B, T, H, Hkv, Dh, _ = c
    x = U.attn_inputs("randn", B, T, H, Hkv, Dh, dev=DEV)
    out = torch.empty(B, T, H * Dh, dtype=U.BF16, device=DEV)
    lse = torch.empty(B * H, T, dtype=F32, device=DEV)
    for thr in (0, 256):
        with pytest.raises(RuntimeError, match="thr"):
            _ext().flash_fwd_drop(x["qkv"], out, lse, 0, None, None, thr, 1, 0, None, B, T, H, Hkv, Dh, 0.125)
    with pytest.raises(RuntimeError, match="off_dev"):
        _ext().flash_fwd_drop(x["qkv"], out, lse, 0, None, None, 26, 1, 0, torch.zeros(1, dtype=torch.int64),
                              B, T, H, Hkv, Dh, 0.125)
    with pytest.raises(RuntimeError, match="off_dev"):
        _ext().flash_fwd_drop(x["qkv"], out, lse, 0, None, None, 26, 1, 0, torch.zeros(1, dtype=torch.int32, device=DEV),
                              B, T, H, Hkv, Dh, 0.125)


# ---------------------------------------------------------------- 3. bitwise
@pytest.mark.parametrize("v", KNOBS, ids=["v111", "v222"])
@pytest.mark.parametrize("mode", ["plain", "A+W48"])
def test_same_stream_state_same_bits(monkeypatch, mode, v):
    c = CASES[3]
    B, T, H, Hkv, Dh, _ = c
    x, docs, W, _, _ = _case(c, mode, 0.1, 1000)
    for qs in (1, 2):
        _set_knobs(monkeypatch, v, qs)
        a = _run(x["qkv"], x["dout"], H, Hkv, docs=docs, window=W, dropout_p=0.1, stream=_stream(1000))
        b = _run(x["qkv"], x["dout"], H, Hkv, docs=docs, window=W, dropout_p=0.1, stream=_stream(1000))
        o = _run(x["qkv"], x["dout"], H, Hkv, docs=docs, window=W, dropout_p=0.1, stream=_stream(1001))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert not torch.equal(a[0], o[0])  # another stream position, another mask


@pytest.mark.parametrize("mode", MODES)
def test_off_is_the_plain_call(monkeypatch, mode):
    c = CASES[3]
    B, T, H, Hkv, Dh, _ = c
    x, docs, W, _, _ = _case(c, mode, 0.1, 1000)
    st = _stream(5)
    plain = _run(x["qkv"], x["dout"], H, Hkv, docs=docs, window=W)
    for kw in ({"dropout_p": 0.1, "training": False}, {"dropout_p": 0.0}):
        got = _run(x["qkv"], x["dout"], H, Hkv, docs=docs, window=W, stream=st, **kw)
        assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
    assert st.offset == 5


def test_counter_base_split_between_host_and_device(monkeypatch):
    """offset = host part + *off_dev: any split gives the bits of the all-host offset"""
    from ray_torch_distributed_checkpoint_amd.ops import attention_dropout_keep

    c, p, off = CASES[3], 0.1, 2 ** 32 - 5
    B, T, H, Hkv, Dh, _ = c
    Wd, C, scale = (H + 2 * Hkv) * Dh, H * Dh, 1.0 / math.sqrt(Dh)
    thr = attention_dropout_keep(p)[0]
    x = U.attn_inputs("randn", B, T, H, Hkv, Dh, dev=DEV)
    res = []
    for host, dev in ((off, None), (0, off), (off - 12345, 12345), (7, off - 7)):
        base = None if dev is None else torch.tensor([dev], dtype=torch.int64, device=DEV)
        out = torch.empty(B, T, C, dtype=U.BF16, device=DEV)
        lse, delta = torch.empty(B * H, T, dtype=F32, device=DEV), torch.empty(B * H, T, dtype=F32, device=DEV)
        dqkv = torch.empty(B, T, Wd, dtype=U.BF16, device=DEV)
        _ext().flash_fwd_drop(x["qkv"], out, lse, 0, None, None, thr, SEED, host, base, B, T, H, Hkv, Dh, scale)
        _ext().flash_bwd_drop(x["qkv"], out, x["dout"], lse, delta, dqkv, 0, None, None, thr, SEED, host, base,
                              B, T, H, Hkv, Dh, scale, None, None, 1)
        torch.cuda.synchronize()
        res.append((out, lse, delta, dqkv))
    for r in res[1:]:
        assert all(torch.equal(a, b) for a, b in zip(res[0], r))


def test_dropout_needs_the_flash_path(monkeypatch):
    from ray_torch_distributed_checkpoint_amd.ops import causal_attention

    H, Dh = 4, 64
    monkeypatch.delenv("RTDC_ATTN", raising=False)
    st = _stream(3)
    qkv = torch.randn(1, 100, 3 * H * Dh, device=DEV).to(torch.bfloat16)
    with pytest.raises(RuntimeError, match="dropout"):
        causal_attention(qkv, H, dropout_p=0.1, stream=st)
    monkeypatch.setenv("RTDC_ATTN", "gemm")
    qkv = torch.randn(1, 128, 3 * H * Dh, device=DEV).to(torch.bfloat16)
    with pytest.raises(RuntimeError, match="dropout"):
        causal_attention(qkv, H, dropout_p=0.1, stream=st)
    with pytest.raises(ValueError):
        causal_attention(qkv, H, dropout_p=0.999, stream=st)
    assert st.offset == 3  # a refused call reserves nothing


# ---------------------------------------------------------------- 4. hipGraph
def test_graph_replays_draw_fresh_masks():
    """forward + backward with dropout captured in a hipGraph: the counter base lives on the device
    and every replay advances it, so two replays draw different masks, each the mask of the eager
    call made at the same stream offset - bit for bit"""
    from ray_torch_distributed_checkpoint_amd.ops import causal_attention
    from ray_torch_distributed_checkpoint_amd.utils.graphs import CapturedStep

    B, T, H, Hkv, Dh, p, off0 = 2, 128, 4, 4, 64, 0.1, 40
    n = B * H * (T // 4) ** 2
    x = U.attn_inputs("randn", B, T, H, Hkv, Dh, dev=DEV)
    q = x["qkv"].clone().requires_grad_(True)
    st = _stream(off0)

    def step():
        q.grad = None
        out = causal_attention(q, H, Hkv, dropout_p=p, stream=st)
        out.backward(x["dout"])
        return out.detach(), q.grad

    cs = CapturedStep(step, warmup=1, philox=st)  # the warm-up call draws [off0, off0 + n)
    try:
        got = []
        for _ in range(2):
            out, grad = cs.replay()
            torch.cuda.synchronize()
            got.append((out.clone(), grad.clone()))
    finally:
        cs.close()
    assert st.offset == off0 + 3 * n  # the host counter resumes where the replays left it
    assert not torch.equal(got[0][0], got[1][0])
    for i, (out, grad) in enumerate(got):
        e_out, e_grad = _run(x["qkv"], x["dout"], H, Hkv, dropout_p=p, stream=_stream(off0 + (i + 1) * n))
        assert torch.equal(out, e_out) and torch.equal(grad, e_grad), i
