"""The case table of the few-row linear kernel, shared by tests/test_few_rows_cpu.py (twin
condition, mutants) and tests/test_few_rows_gpu.py (the kernel).  The yardstick is the GEMM
section of tests/ulp.py, unchanged.

(N, K) -> the arm of csrc/kernels/gemm_few_rows.hip it reaches.  The kernel runs W waves per
16-column block and gives each `per` chunks of 64 k, loaded 4 chunks at a time; W and per come from
the extension (`few_rows_plan`), and the GPU test asserts each case's property (ARMS below) on
what the extension answers, so a retuned plan that no longer reaches an arm fails there:

  (8, 64)        one k-step on one wave; one block of 8 real weight rows
  (24, 64)       two blocks, the second partial
  (16, 128)      the LDS combine, one chunk per wave
  (136, 192)     9 blocks; 3 chunks that do not divide evenly among the waves, no wave idle
  (384, 128)     24 blocks with the LDS combine
  (1000, 320)    63 blocks, the last partial; 5 chunks on 4 waves: 2 + 2 + 1 + 0 (an idle wave)
  (40, 3072)     many k-steps; a load group with fewer than its 4 chunks live
  (16, 576)      (added) the 8-wave instance, with idle waves
  (8, 4160)      (added) the load-group loop runs more than once
  (32776, 128)   (added) 2049 blocks: W capped by the block count, below the chunk count
"""
import torch

from tests import ulp as U

MS = (1, 2, 7, 8, 15, 16)
SHAPES = ((8, 64), (24, 64), (16, 128), (136, 192), (384, 128), (1000, 320), (40, 3072),
          (16, 576), (8, 4160), (32776, 128))
# (W, per, chunks, blocks) -> the property that makes the case what its line above says
ARMS = {
    (8, 64): lambda W, per, ch, bl: W == 1 and ch == 1 and bl == 1,
    (24, 64): lambda W, per, ch, bl: W == 1 and bl == 2,
    (16, 128): lambda W, per, ch, bl: W > 1 and per == 1,
    (136, 192): lambda W, per, ch, bl: W > 1 and (W - 1) * per < ch < W * per,
    (384, 128): lambda W, per, ch, bl: W > 1 and bl == 24,
    (1000, 320): lambda W, per, ch, bl: W > 1 and (W - 1) * per >= ch,
    (40, 3072): lambda W, per, ch, bl: ch == 48 and per % 4 != 0,
    (16, 576): lambda W, per, ch, bl: W == 8 and (W - 1) * per >= ch,
    (8, 4160): lambda W, per, ch, bl: per > 4,
    (32776, 128): lambda W, per, ch, bl: W == 1 and W < ch,
}
# plain, the two bias types, bias + GELU, bias + residual (beta 1), and - the order "residual, then
# the activation" - bias + residual + GELU
EPIS = ("plain", "bias_bf16", "bias_f32", "gelu", "bias_res", "gelu_res")
ACT_NONE, ACT_GELU = 0, 2


def case(gen, M, N, K, epi, dev="cpu"):
    """U.gemm_case of one row of the table; the residual epilogues are the `cin_sep` case with
    beta set to 1 (and, for gelu_res, act 2 on O(1) pre-activations) before any reference is taken"""
    if epi == "bias_res":
        c = U.gemm_case(gen, M, N, K, "cin_sep", dev=dev)
        c["beta"] = 1.0
    elif epi == "gelu_res":
        c = U.gemm_case(gen, M, N, K, "cin_sep", dev=dev, bscale=K ** -0.5)
        c["beta"], c["act"] = 1.0, ACT_GELU
    else:
        c = U.gemm_case(gen, M, N, K, epi, dev=dev)
    c["epi"] = epi
    assert c["alpha"] == 1.0 and c["alpha_dev"] is None and c["aux_in"] is None and c["act"] in (ACT_NONE, ACT_GELU)
    return c


def refs(c):
    return U.gemm_ref_of(U.F64, c), U.gemm_ref_of(U.F32, c)


def cases(shapes=SHAPES):
    for N, K in shapes:
        for M in MS:
            for gen in U.GEMM_GENS:
                for epi in EPIS:
                    yield gen, M, N, K, epi


def shape_id(s):
    return "%dx%d" % s


def bits(t):
    return t.contiguous().view(torch.int16)
