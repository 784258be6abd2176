"""FP8 (OCP e4m3) weight images for generation: the per-row quantiser, the few-row linear that
reads them (csrc/kernels/gemm_few_rows_fp8.hip) and the cache of a parameter's image.

Weight-only: activations, the KV cache, norms, biases and embeddings stay as they are.  The
quantisation of a weight w [N, K], per row n:

    scale[n] = max_k |w[n, k]| / 448        (fp32 division; 1.0 where the quotient is not > 0)
    q[n, k]  = rne_e4m3(float(w[n, k]) / scale[n])      (a true fp32 division)

The scale is 1.0 for an all-zero row and for a row so small that the division underflows to zero
(a maximum of about 3e-43 or less: its codes are all zero), so it is never zero: no finite row divides
by zero.  For a finite row no quotient exceeds 448 by more than an fp32 rounding, so no code saturates or is
NaN; a row whose scale is a subnormal fp32 (a maximum below about 5e-36) is quantised more coarsely.  A row
that holds inf or NaN is not defined here.  The GPU kernels and the torch formulas below give the same bits.
"""
from __future__ import annotations

import torch

from ._ext import gpu_ext
from .gemm import ACT_GELU, ACT_NONE, FEW_ROWS_MAX
from .shadow import _GEN

FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0


def quantize_fp8_rows(w: torch.Tensor, out=None):
    """w [N, K] contiguous, fp32 or bf16 -> (q [N, K] float8_e4m3fn, scale [N] fp32) by the formula
    of this module; out=(q, scale) writes into existing storage.  On the GPU one launch of
    quant_fp8_rows_kernel (K % 16 == 0); on the CPU the formula in torch.  Finite weights only: what a
    row that holds inf or NaN gives is not defined."""
    if w.dim() != 2 or w.dtype not in (torch.float32, torch.bfloat16) or not w.is_contiguous():
        raise ValueError("quantize_fp8_rows: a contiguous fp32 or bf16 [N, K] weight expected")
    N, K = w.shape
    if out is None:
        out = (torch.empty((N, K), dtype=FP8, device=w.device), torch.empty((N,), dtype=torch.float32, device=w.device))
    q, scale = out
    if q.shape != w.shape or q.dtype != FP8 or scale.shape != (N,) or scale.dtype != torch.float32:
        raise ValueError("quantize_fp8_rows: out must be (float8_e4m3fn [N, K], fp32 [N])")
    with torch.no_grad():
        if w.is_cuda:
            gpu_ext().quantize_fp8_rows(w.detach(), q, scale)
        else:
            wf = w.detach().float()
            amax = wf.abs().amax(dim=1)
            # (a tensor divisor: a Python scalar would be turned into a multiplication by 1 / 448)
            s = amax / torch.full_like(amax, FP8_MAX)
            s = torch.where(s > 0, s, torch.ones_like(s))   # a zero row, or a quotient that underflowed
            scale.copy_(s)
            q.copy_((wf / s[:, None]).to(FP8))
    return q, scale


def linear_few_rows_fp8(x2d: torch.Tensor, q: torch.Tensor, scale: torch.Tensor, bias=None, act=ACT_NONE,
                        residual=None, out=None):
    """y[M,N] = act((x[M,K] @ q[N,K]^T) * scale[n] + bias + residual) for 1 <= M <= 16 rows: one launch
    of the FP8 weight-streaming kernel, which widens the e4m3 weights to bf16 in registers on their
    way into the MFMA.  On the GPU x and residual are bf16, q float8_e4m3fn, scale fp32 [N], bias
    bf16 or fp32, K % 128 == 0, N % 8 == 0, every operand contiguous and 16-byte aligned: anything
    else raises in the binding before a launch.  On the CPU the same math in fp32, rounded once."""
    if act not in (ACT_NONE, ACT_GELU):
        raise ValueError(f"linear_few_rows_fp8: act must be ACT_NONE or ACT_GELU, got {act}")
    if x2d.dim() != 2 or q.dim() != 2:
        raise ValueError("linear_few_rows_fp8: x [M, K] and q [N, K] expected")
    M, N = x2d.shape[0], q.shape[0]
    if not 1 <= M <= FEW_ROWS_MAX:
        raise ValueError(f"linear_few_rows_fp8: 1 <= M <= {FEW_ROWS_MAX} rows expected, got {M}")
    if not x2d.is_cuda:
        if q.dtype != FP8 or scale.dtype != torch.float32 or scale.shape != (N,):
            raise ValueError("linear_few_rows_fp8: q float8_e4m3fn [N, K] and scale fp32 [N] expected")
        y = x2d.float() @ (q.float() * scale[:, None]).t()
        if bias is not None:
            y = y + bias.float()
        if residual is not None:
            y = y + residual.float()
        if act == ACT_GELU:
            y = torch.nn.functional.gelu(y, approximate="tanh")
        y = y.to(x2d.dtype)
        if out is not None:
            out.copy_(y)
            return out
        return y
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=x2d.device)
    gpu_ext().gemm_few_rows_fp8(x2d, q, scale, bias, residual, out, act)
    return out


def few_rows_fp8_plan(N: int, K: int):
    """(column tiles of 16 per block, waves per block, chunks of 128 k per wave) of the launch for (N, K)"""
    return tuple(gpu_ext().few_rows_fp8_plan(N, K))


def fp8_stamp(p: torch.Tensor):
    """what an image of p is valid for: p's version counter and the fused optimizers' generation"""
    return (p._version, _GEN[0])


def fp8_rows_of(p: torch.Tensor):
    """The (q, scale) image of a 2-D parameter, cached on it with its version counter and quantised
    from the parameter's own values (fp32 master or bf16).  When the version moves (any in-place
    torch update), or a fused optimizer reports an update of the masters (ops.shadow.bump_generation),
    the image is refreshed in place, in the same storage: a captured decode step that baked its
    addresses in keeps reading the right bytes."""
    img = getattr(p, "_rtdc_fp8", None)
    ver = fp8_stamp(p)
    fresh = img is None or img[0].device != p.device or img[0].shape != p.shape
    if fresh or getattr(p, "_rtdc_fp8_ver", None) != ver:
        src = p.detach()
        src = src if src.is_contiguous() else src.contiguous()
        if fresh:
            img = quantize_fp8_rows(src)
        else:
            quantize_fp8_rows(src, out=img)   # (the same tuple, the same storage)
        p._rtdc_fp8 = img
        p._rtdc_fp8_ver = ver
    return img
