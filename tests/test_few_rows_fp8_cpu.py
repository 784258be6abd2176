"""The CPU (torch) paths of ops.quantize_fp8_rows and ops.linear_few_rows_fp8 against float64, and
generate(..., weights="fp8") on the CPU.  Bounds, from the formats alone: e4m3 has 3 mantissa bits
and subnormals spaced 2^-9, so a quotient rounds by at most max(2^-4 |v|, 2^-10) (x 1 + 2^-20 for the two
fp32 divisions); an fp32 sum of K products + bias + residual is within (K + 16) 2^-24 of the sum of |terms|.
"""
import pytest
import torch

from ray_torch_distributed_checkpoint_amd import ops
from ray_torch_distributed_checkpoint_amd.generate import build_model


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,N,K", [(3, 24, 128), (16, 136, 384)])
def test_quantiser_and_linear_against_fp64(M, N, K, dtype):
    g = torch.Generator().manual_seed(N + K)
    w = torch.randn(N, K, generator=g)
    w[N // 2] = 0
    w[1] *= 2.0 ** -20
    w = w.to(dtype)
    q, scale = ops.quantize_fp8_rows(w)
    assert q.dtype == torch.float8_e4m3fn and scale.dtype == torch.float32 and scale.shape == (N,)
    w64, s64, q64 = w.double(), scale.double(), q.float().double()
    amax = w64.abs().amax(dim=1)
    assert scale[N // 2].item() == 1.0 and not bool(q64[N // 2].any())
    assert bool(((s64 - amax / 448.0).abs() <= 2.0 ** -24 * amax / 448.0)[amax > 0].all())
    assert bool(torch.isfinite(q64).all()) and q64.abs().max().item() == 448.0
    allow = torch.maximum(2.0 ** -4 * w64.abs(), 2.0 ** -10 * s64[:, None]) * (1 + 2.0 ** -20)
    assert bool(((q64 * s64[:, None] - w64).abs() <= allow).all())
    out = (torch.empty_like(q), torch.empty_like(scale))   # out=, and idempotent on its own dequantised output
    assert ops.quantize_fp8_rows(q.float() * scale[:, None], out=out)[0] is out[0]
    assert torch.equal(out[0].view(torch.uint8), q.view(torch.uint8)) and torch.equal(out[1], scale)
    x, bias, res = torch.randn(M, K, generator=g), torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    wd = q64 * s64[:, None]
    for b, r in ((None, None), (bias, res)):
        y = ops.linear_few_rows_fp8(x, q, scale, bias=b, residual=r)
        ref, S = x.double() @ wd.t(), x.double().abs() @ wd.abs().t()
        if b is not None:
            ref, S = ref + b.double() + r.double(), S + b.double().abs() + r.double().abs()
        assert y.dtype == torch.float32 and bool(((y.double() - ref).abs() <= (K + 16) * 2.0 ** -24 * S).all())
        gelu = ops.linear_few_rows_fp8(x, q, scale, bias=b, residual=r, act=2)
        assert torch.equal(gelu, torch.nn.functional.gelu(y, approximate="tanh"))
    with pytest.raises(ValueError):
        ops.linear_few_rows_fp8(torch.zeros(17, K), q, scale)


def test_generate_fp8_on_the_cpu():
    m = build_model("gpt2-tiny", "cpu").eval()
    idx = torch.randint(0, m.cfg.vocab_size, (2, 12), generator=torch.Generator().manual_seed(1))
    for kw in ({}, dict(temperature=0.8, top_k=50, seed=7)):
        a = m.generate(idx, 8, few_row=True, weights="fp8", **kw)
        assert a.shape == (2, 20) and torch.equal(a[:, :12], idx) and int(a.max()) < m.cfg.vocab_size
        assert torch.equal(a, m.generate(idx, 8, few_row=True, weights="fp8", **kw))
    assert getattr(m.h[0].mlp.c_fc.weight, "_rtdc_fp8", None) is not None   # the images were used
    with pytest.raises(ValueError):
        m.generate(idx, 8, weights="fp8")
