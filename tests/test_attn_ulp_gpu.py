"""The attention kernels judged per element against fp64 (GPU only).

The yardstick is the attention section of tests/ulp.py: `attn_ref` in float64 is the reference
and returns, for every element of out, lse, delta, dQ, dK and dV, the error the kernel's own bf16
roundings can cause (counted from attn_flash.hip, terms at the leaves) plus a stated fp32 term;
the same function in float32 with those roundings in place is the twin, which
tests/test_ulp_cpu.py holds inside the allowance.  A kernel output scores
max |out - ref| / allowance and has to stay <= 1.  Each judged output prints one ULP line, each
test its WORST lines; those of one run are kept in profiles/attn_ulp_worst.txt.

Kernel -> the cases that reach it (U.attn_launches mirrors flash_fwd_launch / flash_bwd_launch;
tests/test_ulp_cpu.py::test_attn_grids_meet_every_xcd_branch checks the grids):

  fwd / bwd_dq with G = 1, bwd_dkdv    RTDC_FA_* = 1 at every T; whatever the knob at T = 64 and 192
  fwd / bwd_dq with G = 2, bwd_dkdv2   RTDC_FA_* = 2 at T = 128, 256, 384 (Dh = 128 dkdv2: opt-in, set here)
  dkdv_reduce                  RTDC_FA_QS = 2, 4 where the group size allows
  DOC instantiations           layouts A, aligned, ones; the plain ones with docs=None
  composed GEMM + softmax      T = 100 (no flash kernel), T = 128 with RTDC_ATTN=gemm

The fp64 reference of a (case, layout) is computed once and shared by every variant.
"""
import math

import pytest
import torch

from tests import ulp as U

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32 = U.F64, U.F32
_refs: dict = {}


def _ext():
    from ray_torch_distributed_checkpoint_amd.ops._ext import gpu_ext

    return gpu_ext()


def _case(c, layout=None, path="flash"):
    """inputs, document layout, fp64 reference (with the allowance) and twin of one case:
    computed once, shared, never modified"""
    from ray_torch_distributed_checkpoint_amd.ops import DocLayout

    key = (c, layout, path)
    if key not in _refs:
        B, T, H, Hkv, Dh, gen = c
        x = U.attn_inputs(gen, B, T, H, Hkv, Dh, dev=DEV)
        docs = arr = None
        if layout is not None:
            lengths = U.attn_layout(layout, T, B)
            docs, arr = DocLayout.from_lengths(lengths, T, DEV), U.doc_arrays(lengths, T, DEV)
            assert torch.equal(docs.start.long(), arr[0]) and torch.equal(docs.end.long(), arr[1])
        a = (x["qkv"], x["dout"], B, T, H, Hkv, Dh, arr)
        _refs[key] = (x, docs, U.attn_ref(F64, *a, path=path), U.attn_ref(F32, *a, twin=True, path=path))
    return _refs[key]


def _set_knobs(monkeypatch, v, qs):
    for name, val in zip(("RTDC_FA_FWD", "RTDC_FA_DQ", "RTDC_FA_DKDV"), v):
        monkeypatch.setenv(name, str(val))
    monkeypatch.setenv("RTDC_FA_QS", str(qs))


def _families(c, v, qs):
    f, d, kv = (fam for fam, _, _ in U.attn_launches(*c[:5], v, qs))
    return {"out": f, "lse": f, "delta": d, "dq": d, "dk": kv, "dv": kv}


def _split(grad, H, Hkv, Dh):
    C, KV = H * Dh, Hkv * Dh
    return {"dq": grad[..., :C], "dk": grad[..., C:C + KV], "dv": grad[..., C + KV:]}


def _run(x, H, Hkv, Dh, docs):
    from ray_torch_distributed_checkpoint_amd.ops import causal_attention

    q = x["qkv"].clone().requires_grad_(True)
    out = causal_attention(q, H, Hkv, docs=docs)
    out.backward(x["dout"])
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all() and torch.isfinite(q.grad.float()).all()
    return {"out": out.detach(), **_split(q.grad, H, Hkv, Dh)}


def _variants(T):
    return U.ATTN_VARIANTS if T % 128 == 0 else [(1, 1, 1), (2, 2, 2)]   # the knobs are ignored at T = 64, 192


@pytest.mark.parametrize("c", U.ATTN_CASES, ids=U.attn_case_id)
def test_attention_per_element(monkeypatch, c):
    """causal_attention + backward: every case x {plain, layout A, aligned, ones} x variant knobs x
    head split, each of out, dQ, dK, dV inside its per-element allowance"""
    B, T, H, Hkv, Dh, _ = c
    monkeypatch.delenv("RTDC_ATTN", raising=False)
    J = U.Judge()
    for layout in (None,) + U.ATTN_LAYOUTS:
        x, docs, ref, twin = _case(c, layout)
        for v in _variants(T):
            for qs in U.attn_head_splits(H, Hkv):
                _set_knobs(monkeypatch, v, qs)
                outs = _run(x, H, Hkv, Dh, docs)
                shape = "%s %s v%d%d%d qs%d" % (U.attn_case_id(c), layout or "plain", *v, qs)
                U.judge_attn(J, _families(c, v, qs), shape, ref, twin, outs)
    J.check()


def _guarded(n0, rest, dtype):
    """a [n0, *rest] dim-0 slice of a NaN-filled buffer with one guard slab on either side"""
    big = torch.full((n0 + 2, *rest), float("nan"), dtype=dtype, device=DEV)
    return big, big[1:n0 + 1]


def _check_guards(bufs):
    for name, (big, inner) in bufs.items():
        assert torch.isfinite(inner.float()).all(), f"{name}: an element no block wrote (or a non-finite value)"
        assert torch.isnan(big[0]).all() and torch.isnan(big[-1]).all(), f"{name}: a store outside the tensor"


@pytest.mark.parametrize("doc", [False, True], ids=["plain", "doc"])
@pytest.mark.parametrize("c", U.ATTN_DIRECT, ids=U.attn_case_id)
def test_launchers_guarded(monkeypatch, c, doc):
    """flash_fwd(_doc) / flash_bwd(_doc) called directly, both row variants, qs 1 and 2: lse and
    delta judged as well; every output is a slice of a NaN-filled buffer - inside everything is
    written, outside nothing is"""
    B, T, H, Hkv, Dh, _ = c
    W, C, scale = (H + 2 * Hkv) * Dh, H * Dh, 1.0 / math.sqrt(Dh)
    x, docs, ref, twin = _case(c, "A" if doc else None)
    J = U.Judge()
    for v in [(1, 1, 1), (2, 2, 2)]:
        for qs in (1, 2):
            _set_knobs(monkeypatch, v, qs)
            bufs = {"out": _guarded(B, (T, C), U.BF16), "lse": _guarded(B * H, (T,), F32),
                    "delta": _guarded(B * H, (T,), F32), "dqkv": _guarded(B, (T, W), U.BF16)}
            out, lse, delta, dqkv = (bufs[n][1] for n in ("out", "lse", "delta", "dqkv"))
            part = torch.empty(qs * B * T * Hkv * 2 * Dh, dtype=F32, device=DEV) if qs > 1 else None
            if doc:
                _ext().flash_fwd_doc(x["qkv"], out, lse, docs.start, docs.end, B, T, H, Hkv, Dh, scale)
                _ext().flash_bwd_doc(x["qkv"], out, x["dout"], lse, delta, dqkv, docs.start, docs.end, B, T, H, Hkv,
                                     Dh, scale, None, part, qs)
            else:
                _ext().flash_fwd(x["qkv"], out, lse, B, T, H, Hkv, Dh, scale)
                _ext().flash_bwd(x["qkv"], out, x["dout"], lse, delta, dqkv, B, T, H, Hkv, Dh, scale, None, part, qs)
            torch.cuda.synchronize()
            _check_guards(bufs)
            outs = {"out": out, "lse": lse, "delta": delta, **_split(dqkv, H, Hkv, Dh)}
            shape = "%s %s v%d%d%d qs%d direct" % (U.attn_case_id(c), "A" if doc else "plain", *v, qs)
            U.judge_attn(J, _families(c, v, qs), shape, ref, twin, outs, U.ATTN_OUTPUTS)
    J.check()


@pytest.mark.parametrize("c", U.ATTN_GEMM, ids=U.attn_case_id)
def test_composed_path_per_element(monkeypatch, c):
    """the GEMM + row-softmax path (the only one at T % 64 != 0): its allowance also carries the
    bf16 S, P, dP and dS matrices and the bf16 accumulation of dK / dV over the group"""
    B, T, H, Hkv, Dh, _ = c
    monkeypatch.setenv("RTDC_ATTN", "gemm")
    x, _, ref, twin = _case(c, None, "gemm")
    outs = _run(x, H, Hkv, Dh, None)
    J = U.Judge()
    U.judge_attn(J, dict.fromkeys(U.ATTN_OUTPUTS, "gemm"), U.attn_case_id(c), ref, twin, outs)
    J.check()
