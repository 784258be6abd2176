// OCP e4m3 for gfx950, the one formula every FP8 kernel of this project quantises and widens by:
//   scale = amax / 448 (a true fp32 division), or 1.0 where that quotient is not > 0: an all-zero
//   run, and a run so small (amax <= 448 * 2^-150, about 3e-43) that the quotient underflows to
//   zero, whose codes are then all zero; code = rne_e4m3(x / scale),
// and every e4m3 value is a bf16 value, so the widening is exact.  The scale is never zero, so no
// finite run divides by it into NaN codes.  quant_fp8_rows_kernel (gemm_few_rows_fp8.hip),
// kv_fill_fp8_kernel and the decode kernel's owner (attn_decode.hip) must agree bit for bit: they
// all come here.
#pragma once
#include "common.h"

namespace rtdc {

typedef __attribute__((ext_vector_type(2))) __bf16 fp8_bf16x2;

// the scale of a run from its largest magnitude
__device__ __forceinline__ float fp8_scale(float amax) {
  const float s = __fdiv_rn(amax, 448.f);
  return s > 0.f ? s : 1.f;
}

// v[0 .. 3] / s -> four e4m3 bytes, v[0] in the lowest (v_cvt_pk_fp8_f32 twice)
__device__ __forceinline__ uint32_t fp8_pack4(const float* v, float s) {
  int p = __builtin_amdgcn_cvt_pk_fp8_f32(__fdiv_rn(v[0], s), __fdiv_rn(v[1], s), 0, false);
  p = __builtin_amdgcn_cvt_pk_fp8_f32(__fdiv_rn(v[2], s), __fdiv_rn(v[3], s), p, true);
  return (uint32_t)p;
}

// the low (HI = false) or high pair of e4m3 bytes of w -> bf16x2, exactly
// (v_cvt_scalef32_pk_bf16_fp8 at scale 1.0)
template <bool HI>
__device__ __forceinline__ fp8_bf16x2 fp8_widen2(uint32_t w) {
  return __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, HI);
}

}  // namespace rtdc
