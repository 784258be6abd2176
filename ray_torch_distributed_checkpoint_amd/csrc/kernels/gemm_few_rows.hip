// Few-row linear for gfx950: y[M, N] = act(x[M, K] . w[N, K]^T + bias + residual), 1 <= M <= 16.
//
// A decode step multiplies 1..16 token rows by every weight of the model: the product is a read
// of the weights and nothing else, and a 128x128 / 256x256 MFMA tile that stages 8 padded rows
// through LDS cannot stream them.  Here the weights go from global memory straight into the MFMA.
//
// v_mfma_f32_16x16x32_bf16 computes D[i][j] = sum_k A[i][k] B[k][j] with lane l (r = l & 15,
// g = l >> 4) holding A[r][8g .. 8g+7] and B[8g .. 8g+7][r] and ending with D[4g .. 4g+3][r].
// w is the A operand: one 16-byte load per lane is the fragment of 16 weight rows n0 + r, and the
// lane ends with 4 consecutive n of token row m = r (one 8-byte store).  x is the B operand, its
// fragment the same 16-byte load from row m of x (x is at most 16 K bf16: it stays in the L2).
//
// K is walked in chunks of 64 (K % 64 == 0): two MFMAs, the first on k = 64c + 8g + j, the second
// on k = 64c + 32 + 8g + j, whose two loads a wave issues back to back - together the whole
// 128-byte line of each weight row.  A wave keeps kFrU chunks (2 kFrU KiB of weights) in flight.
//
// few_rows_kernel<W>, grid ceil(N / 16), W waves: the block owns 16 output columns; wave v
// accumulates the chunks [v * per, (v + 1) * per) in ascending order into one accumulator, the W
// partial accumulators meet in LDS and wave 0 adds them in wave order, applies the epilogue and
// stores.  One launch, no workspace, no atomics.  W and per come from the host as a function of
// (N, K) alone (few_rows_plan), so the summation order of an output element never depends on M
// or on the other rows: each MFMA column is computed on its own.
//
// Rows >= M of the x fragment and weight rows >= N are never loaded: the lane's fragment is zero
// by select.  Lanes with m >= M or n >= N store nothing.
//
// Epilogue, in the order of gemm_common.h's epilogue4: sum, + bias (bf16 or fp32), + residual
// (bf16), then none | tanh-form GELU of the unrounded value; rounded to bf16 once.
#include "common.h"

namespace rtdc {

constexpr int kFrU = 4;        // chunks of 64 k a wave loads before it multiplies them
constexpr int kFrMaxWaves = 16;

struct FewRowsArgs {
  const bf16_t* x;
  const bf16_t* w;
  const void* bias;
  const bf16_t* res;
  bf16_t* y;
  int M, N, K;
  int bias_type;  // 0 none, 1 bf16, 2 fp32
  int act;        // 0 none, 2 gelu_tanh
  int chunks;     // K / 64
  int per;        // chunks per wave
};

__device__ __forceinline__ void fr_load4_bf16(const bf16_t* p, float* v) {
  const uint2 x = *(const uint2*)p;
  v[0] = __uint_as_float(x.x << 16); v[1] = __uint_as_float(x.x & 0xffff0000u);
  v[2] = __uint_as_float(x.y << 16); v[3] = __uint_as_float(x.y & 0xffff0000u);
}

template <int W>
__global__ __launch_bounds__(W * 64) void few_rows_kernel(FewRowsArgs a) {
  __shared__ f32x4 red[W][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const bool w_ok = n0 + r < a.N, x_ok = r < a.M;
  // (a masked lane's pointer stays inside the operand; it is never dereferenced)
  const bf16_t* wp = a.w + (long long)(w_ok ? n0 + r : 0) * a.K + 8 * g;
  const bf16_t* xp = a.x + (long long)(x_ok ? r : 0) * a.K + 8 * g;
  const int c_begin = wave * a.per, c_end = min(c_begin + a.per, a.chunks);

  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int c0 = c_begin; c0 < c_end; c0 += kFrU) {
    bf16x8 wf[kFrU][2], xf[kFrU][2];
#pragma unroll
    for (int u = 0; u < kFrU; ++u) {
      const bool live = c0 + u < c_end;  // wave-uniform
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const long long k = (long long)(c0 + u) * 64 + 32 * h;
        wf[u][h] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        xf[u][h] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (live && w_ok) wf[u][h] = *(const bf16x8*)(wp + k);
        if (live && x_ok) xf[u][h] = *(const bf16x8*)(xp + k);
      }
    }
#pragma unroll
    for (int u = 0; u < kFrU; ++u) {
      if (c0 + u < c_end) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[u][0], xf[u][0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[u][1], xf[u][1], acc, 0, 0, 0);
      }
    }
  }

  if (W > 1) {
    red[wave][lane] = acc;
    __syncthreads();
    if (wave != 0) return;
    acc = red[0][lane];
#pragma unroll
    for (int v = 1; v < W; ++v) {
      const f32x4 p = red[v][lane];
      acc[0] += p[0]; acc[1] += p[1]; acc[2] += p[2]; acc[3] += p[3];
    }
  }

  const int m = r, n = n0 + 4 * g;
  if (m >= a.M || n >= a.N) return;  // (N % 8 == 0: the 4 columns of a lane are inside together)
  float v[4] = {acc[0], acc[1], acc[2], acc[3]};
  if (a.bias_type == 1) {
    float bb[4];
    fr_load4_bf16((const bf16_t*)a.bias + n, bb);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] += bb[i];
  } else if (a.bias_type == 2) {
    const f32x4 bb = *(const f32x4*)((const float*)a.bias + n);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] += bb[i];
  }
  const long long off = (long long)m * a.N + n;
  if (a.res) {
    float c[4];
    fr_load4_bf16(a.res + off, c);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] += c[i];
  }
  if (a.act == 2) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = gelu_tanh(v[i]);
  }
  *(uint2*)(a.y + off) = make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
}

}  // namespace rtdc

using namespace rtdc;

// The launch plan, a function of (N, K) alone: W waves per 16-column block (a power of two,
// 1 .. 16) and `per` chunks of 64 k per wave.  Few column blocks (N small) get many waves so
// that the chip still has ~16 waves per CU of loads in flight; a wave never gets less than one
// chunk where there is one to give, and W never exceeds the chunk count.
extern "C" void rtdc_few_rows_plan(long long N, long long K, int* waves, int* per) {
  const long long tiles = (N + 15) / 16, chunks = K / 64;
  int W = 1;
  while (W < kFrMaxWaves && tiles * (2 * W) <= 4096 && 2 * W <= chunks) W *= 2;
  *waves = W;
  *per = (int)((chunks + W - 1) / W);
}

extern "C" int rtdc_gemm_few_rows(const void* x, const void* w, const void* bias, int bias_type, const void* res,
                                  void* y, int M, int N, int K, int act, hipStream_t st) {
  if (M < 1 || M > 16 || N < 8 || N % 8 != 0 || K < 64 || K % 64 != 0) return 1;
  if ((act != 0 && act != 2) || bias_type < 0 || bias_type > 2 || (bias_type != 0) != (bias != nullptr)) return 1;
  FewRowsArgs a;
  a.x = (const bf16_t*)x;
  a.w = (const bf16_t*)w;
  a.bias = bias;
  a.res = (const bf16_t*)res;
  a.y = (bf16_t*)y;
  a.M = M;
  a.N = N;
  a.K = K;
  a.bias_type = bias_type;
  a.act = act;
  a.chunks = K / 64;
  int W = 1;
  rtdc_few_rows_plan(N, K, &W, &a.per);
  const dim3 grid((N + 15) / 16);
#define RTDC_FR_CASE(w) \
  case w: hipLaunchKernelGGL((few_rows_kernel<w>), grid, dim3(w * 64), 0, st, a); break;
  switch (W) {
    RTDC_FR_CASE(1) RTDC_FR_CASE(2) RTDC_FR_CASE(4) RTDC_FR_CASE(8) RTDC_FR_CASE(16)
    default: return 1;
  }
#undef RTDC_FR_CASE
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
