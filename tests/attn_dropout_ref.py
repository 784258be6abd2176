"""Reference of flash attention with attention dropout: the flash branch of tests/ulp.py::attn_ref
with the scaled keep mask Z = M * inv_keep carried in (a helper, not a test).

M is `ops.attention_dropout_mask(seed, offset, B, H, T, p)`, Z = M * inv_keep with inv_keep the
realised 256 / (256 - thr) (a float in the kernels, like the score scale).

    forward : l and lse sum the UNDROPPED e;  O = ((e o M) V) * inv_keep / l
    backward: delta = sum dO O;  dV = (P o M)^T dO * inv_keep;  dP = Z o (dO V^T);
              dS = P o (dP - delta);  dQ = dS K scale;  dK = dS^T Q scale

dtype float64, twin False: the reference, with the per-element allowance of every output.
twin=True (float32): the kernels' bf16 roundings where attn_flash.hip places them - e ahead of the
row sum and (then masked) of P.V, O as stored, P ahead of dV (then masked), dS ahead of dQ / dK,
every stored gradient once.  The mask zeroes 16-bit halves of words that are already rounded, so it
adds no rounding; P and dS are rounded exactly where they are without dropout.

The allowance terms are attn_ref's with Z at the leaves: A_o from (P o Z) |v|, A_dv from
(P o Z)^T |dO|, dpl = Z o (|dO| |v|^T) + dterms, Wt = |dS|; the fp32 multiply by inv_keep adds
one to each F count.  No coefficient is fitted to a kernel.

`window` is given as in tests/test_attn_window_gpu.py: the document bounds clipped to the band are
a document layout of the same shape, so it goes in as `docs` (clipped()).
"""
import math

import torch

from tests.ulp import F64, LOG2E, U2, U_BF16, _f32, _f32_terms, _rb, _stored, attn_masks

DROP_MUTANTS = ("mask_transposed", "head0_mask", "inv_keep_one", "bwd_offset_plus_1", "dv_undropped", "l_kept_only")


def clipped(B, T, W, arr, dev="cpu"):
    """(start', end') int64 [B, T]: the document bounds (0 / T without documents) clipped to the band
    of a window W (None: the bounds themselves, or None without documents)"""
    if W is None:
        return arr
    t = torch.arange(T, device=dev)[None, :].expand(B, T)
    start = torch.zeros_like(t) if arr is None else arr[0]
    end = torch.full_like(t, T) if arr is None else arr[1]
    return torch.maximum(start, t - W + 1), torch.minimum(end, t + W)


def attn_drop_ref(dtype, qkv, dout, B, T, H, Hkv, Dh, seed, offset, p, docs=None, twin=False, mutant=""):
    from ray_torch_distributed_checkpoint_amd.ops import attention_dropout_keep, attention_dropout_mask

    assert mutant == "" or mutant in DROP_MUTANTS
    dev, G, C = qkv.device, H // Hkv, H * Dh
    rq = twin
    scale = _f32(1.0 / math.sqrt(Dh))
    thr, ik = attention_dropout_keep(p)
    ik = 1.0 if mutant == "inv_keep_one" else _f32(ik)
    M = attention_dropout_mask(seed, offset, B, H, T, p)
    if mutant == "mask_transposed":
        M = M.transpose(-1, -2)
    elif mutant == "head0_mask":
        M = M[:, :1].expand(B, H, T, T)
    Mb = attention_dropout_mask(seed, offset + 1, B, H, T, p) if mutant == "bwd_offset_plus_1" else M
    grouped = lambda t: t.reshape(B, Hkv, G, T, T).to(dev).to(dtype)         # head = n * G + g
    M, Mb = grouped(M), grouped(Mb)
    Z, Zb = M * ik, Mb * ik

    x = qkv.to(dtype)
    heads = lambda t, n, g: t.reshape(B, T, n, g, Dh).permute(0, 2, 3, 1, 4)   # [B, n, g, T, Dh]
    q, k, v = heads(x[..., :C], Hkv, G), heads(x[..., C:C + Hkv * Dh], Hkv, 1), heads(x[..., C + Hkv * Dh:], Hkv, 1)
    do = heads(dout.to(dtype), Hkv, G)
    keep_q, _, _ = attn_masks(B, T, docs, dev)
    kq = keep_q[:, None, None]
    tr = lambda t: t.transpose(-1, -2)
    zero = torch.zeros((), dtype=dtype, device=dev)

    # ---- forward
    S = (q @ tr(k)) * scale                                # [B, Hkv, G, Tq, Tk]
    Sm = torch.where(kq, S, torch.full_like(S, -math.inf))
    m = Sm.amax(-1, keepdim=True)
    e = _rb(torch.exp(Sm - m), rq)
    l = ((e * M) if mutant == "l_kept_only" else e).sum(-1, keepdim=True)
    O = _rb(((e * M) @ v) * (ik / l), rq)
    lse = m + torch.log(l)

    # ---- backward
    dPraw = do @ tr(v)
    dP = Zb * dPraw
    Praw = torch.exp(S - lse)
    delta = (do * O).sum(-1, keepdim=True)
    P = torch.where(kq, Praw, zero)
    dS = _rb(P * (torch.where(kq, dP, zero) - delta), twin)
    dQ = _rb((dS @ k) * scale, twin)
    Pdv = _rb(P, rq) if mutant == "dv_undropped" else _rb(P, rq) * Mb
    dVg, dKg = (tr(Pdv) @ do) * ik, (tr(dS) @ q) * scale   # per q-head [B, Hkv, G, Tk, Dh]
    dV, dK = _rb(dVg.sum(2), twin), _rb(dKg.sum(2), twin)

    rows = lambda t: t.permute(0, 3, 1, 2, 4).reshape(B, T, -1)
    kvrows = lambda t: t.permute(0, 2, 1, 3).reshape(B, T, -1)
    vec = lambda t: t[..., 0].reshape(B * H, T)
    res = {"out": rows(O), "lse": vec(lse) * LOG2E, "delta": vec(delta), "dq": rows(dQ), "dk": kvrows(dK),
           "dv": kvrows(dV)}
    if dtype != F64 or twin or mutant:
        return res

    # ---- the allowance: attn_ref's flash branch with Z at the leaves, one more fp32 term per count
    u, Fk, Fg, Fd = U_BF16, _f32_terms(T + 1), _f32_terms(G * T + 1), _f32_terms(Dh + 1)
    av, ak, aq, ado = v.abs(), k.abs(), q.abs(), do.abs()
    PZ = P * Z
    pv, pk = PZ @ av, P @ ak
    dterms = (do * O).abs().sum(-1, keepdim=True)
    dpl = Z * torch.where(kq, ado @ tr(av), zero) + dterms
    Wt = P * (torch.where(kq, dP, zero) - delta).abs()
    A_o = _stored(O, (U2 + Fk) * pv)
    E_d = (ado * A_o).sum(-1, keepdim=True) + Fd * dterms
    A_lse = LOG2E * u + Fk * (LOG2E * (m.abs() + torch.log(l).abs()) + 16.0)
    A_dv = _stored(dV, (U2 + Fg) * (tr(PZ) @ ado).sum(2))
    A_dq = _stored(dQ, scale * (U2 * (Wt @ ak) + Fk * ((P * dpl) @ ak) + E_d * pk))
    A_dk = _stored(dK, scale * (U2 * (tr(Wt) @ aq) + Fg * (tr(P * dpl) @ aq) + tr(P * E_d) @ aq).sum(2))
    res.update(allow_out=rows(A_o), allow_lse=vec(A_lse), allow_delta=vec(E_d), allow_dq=rows(A_dq),
               allow_dk=kvrows(A_dk), allow_dv=kvrows(A_dv))
    return res
