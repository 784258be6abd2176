// FP8-weight few-row linear for gfx950:
//   y[M, N] = act((x[M, K] . q[N, K]^T) * scale[n] + bias + residual), 1 <= M <= 16,
// q OCP e4m3 (one byte per weight), scale fp32 per weight row, x / residual / y bf16, and the
// quantiser that makes (q, scale) from a weight:  scale[n] = max_k |w[n, k]| / 448 (1 where that
// is not > 0: fp8.h), q[n, k] = rne_e4m3(w[n, k] / scale[n]), both divisions true fp32 divisions.
//
// A decode step's linear is a read of its weights; a bf16 kernel cannot go below its bytes, so
// this one reads half of them.  Every e4m3 value is a bf16 value: the weights are widened in
// registers (fp8.h: v_cvt_scalef32_pk_bf16_fp8 at scale 1.0, two bytes per VALU op) and fed to the same
// v_mfma_f32_16x16x32_bf16 as gemm_few_rows.hip, so against the dequantised weights the only error
// is the fp32 accumulation.  The row scale multiplies the fp32 sum in the epilogue.
//
// The MFMA: D[i][j] = sum_k A[i][k] B[k][j]; lane l (r = l & 15, g = l >> 4) holds 8 k of row r
// of A and of column r of B and ends with D[4g .. 4g+3][r].  q is the A operand (row n0 + r), x
// the B operand (token row m = r).  Which 8 k a lane feeds into which MFMA is free as long as both
// operands agree; the k mapping of this file:
//
//   K is walked in chunks of 128 (K % 128 == 0): one 128-byte line of every weight row.  Lane
//   (r, g) loads bytes [16g, 16g + 16) and [64 + 16g, 64 + 16g + 16) of the line of row n0 + r, two
//   16-byte loads issued back to back (h = 0, 1) that together with the other three g cover the
//   line.  Each load is two fragments (j = 0, 1: its low and high 8 bytes), so a chunk is four
//   MFMAs, and MFMA (h, j) sums, in lane group g,   k = 128 c + 64 h + 16 g + 8 j + i, i = 0 .. 7.
//   The x fragment of (h, j) is the 16-byte bf16 load at that k of row m: two loads per 16 k.
//
// few_rows_fp8_kernel<T, W>, grid ceil(N / 16 T), W waves: the block owns T column tiles of 16.
// A wave loads the x fragments of a k chunk once and multiplies them with the fragments of the T
// weight tiles into T accumulators: the L2 re-reads of x, which at one byte per weight and M = 16
// are twice the weight traffic of a 16-column block, are divided by T.  A tile wholly beyond N is
// never loaded and never stored.  A wave keeps U chunks of all T tiles (2 T U KiB of weights) in
// flight before the first conversion (U = 2 at T = 4, else 4).  K is split over the W waves: wave
// v accumulates the chunks [v per, (v + 1) per) in ascending order, the partials meet in LDS and
// wave 0 adds them in wave order, applies the epilogue and stores.  One launch, no workspace, no
// atomics.  (T, W, per) come from the host as a function of (N, K) alone (rtdc_few_rows_fp8_plan),
// so the summation order of an output element never depends on M or on the other rows.
//
// Rows >= M of x and weight rows >= N are never loaded (the fragment is zero by select); scale and
// bias are read only for n < N; lanes with m >= M or n >= N store nothing.
//
// Epilogue, in the order of gemm_common.h's epilogue4: sum * scale, + bias (bf16 or fp32),
// + residual (bf16), then none | tanh-form GELU of the unrounded value; rounded to bf16 once.
//
// quant_fp8_rows_kernel: one wave per weight row (4 rows per block), 16 elements per lane and
// step.  Pass 1 takes the row maximum (DPP / row-swap wave_max of common.h), pass 2 re-reads the
// row (it is in the L2), divides, converts with v_cvt_pk_fp8_f32 and stores 16 bytes per lane, by
// fp8.h's formula, which the FP8 KV cache (attn_decode.hip) shares.
#include "common.h"
#include "fp8.h"

namespace rtdc {

constexpr int kF8MaxWaves = 16;
constexpr int kF8MaxWavesT = 8;    // T > 1: the fragments in flight need more than the 128 VGPRs of a 16-wave block
constexpr int kF8InFlight = 16384; // (tile, wave) load streams x chunks each keeps in flight, at 2 KiB: 32 MiB
__host__ __device__ constexpr int f8_group(int T) { return T == 4 ? 2 : 4; }

struct FewRowsFp8Args {
  const bf16_t* x;
  const uint8_t* q;
  const float* scale;
  const void* bias;
  const bf16_t* res;
  bf16_t* y;
  int M, N, K;
  int bias_type;  // 0 none, 1 bf16, 2 fp32
  int act;        // 0 none, 2 gelu_tanh
  int chunks;     // K / 128
  int per;        // chunks per wave
};

__device__ __forceinline__ void f8_load4_bf16(const bf16_t* p, float* v) {
  const uint2 x = *(const uint2*)p;
  v[0] = __uint_as_float(x.x << 16); v[1] = __uint_as_float(x.x & 0xffff0000u);
  v[2] = __uint_as_float(x.y << 16); v[3] = __uint_as_float(x.y & 0xffff0000u);
}

// 8 e4m3 bytes (k ascending with the byte address) -> one bf16x8 MFMA fragment, exactly
__device__ __forceinline__ bf16x8 f8_widen8(uint32_t lo, uint32_t hi) {
  union { fp8_bf16x2 p[4]; bf16x8 v; } u;
  u.p[0] = fp8_widen2<false>(lo);
  u.p[1] = fp8_widen2<true>(lo);
  u.p[2] = fp8_widen2<false>(hi);
  u.p[3] = fp8_widen2<true>(hi);
  return u.v;
}

template <int T, int W>
__global__ __launch_bounds__(W * 64) void few_rows_fp8_kernel(FewRowsFp8Args a) {
  constexpr int U = f8_group(T);  // chunks of 128 k a wave loads before it converts them
  __shared__ f32x4 red[W > 1 ? W : 1][T][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * (16 * T);
  const bool x_ok = r < a.M;
  bool w_ok[T];
  const uint8_t* qp[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    // (a masked lane's pointer stays inside the operand; it is never dereferenced)
    w_ok[t] = n0 + 16 * t + r < a.N;
    qp[t] = a.q + (long long)(w_ok[t] ? n0 + 16 * t + r : 0) * a.K + 16 * g;
  }
  const bf16_t* xp = a.x + (long long)(x_ok ? r : 0) * a.K + 16 * g;
  const int c_begin = wave * a.per, c_end = min(c_begin + a.per, a.chunks);

  f32x4 acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int c0 = c_begin; c0 < c_end; c0 += U) {
    uint4 wq[U][T][2];
    bf16x8 xf[U][2][2];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool live = c0 + u < c_end;  // wave-uniform
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const long long k = (long long)(c0 + u) * 128 + 64 * h;
#pragma unroll
        for (int t = 0; t < T; ++t) {
          wq[u][t][h] = make_uint4(0u, 0u, 0u, 0u);
          if (live && w_ok[t]) wq[u][t][h] = *(const uint4*)(qp[t] + k);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          xf[u][h][j] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
          if (live && x_ok) xf[u][h][j] = *(const bf16x8*)(xp + k + 8 * j);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (c0 + u < c_end) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
          for (int t = 0; t < T; ++t) {
            const uint4 b = wq[u][t][h];
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f8_widen8(b.x, b.y), xf[u][h][0], acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f8_widen8(b.z, b.w), xf[u][h][1], acc[t], 0, 0, 0);
          }
        }
      }
    }
  }

  if (W > 1) {
#pragma unroll
    for (int t = 0; t < T; ++t) red[wave][t][lane] = acc[t];
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      acc[t] = red[0][t][lane];
#pragma unroll
      for (int v = 1; v < W; ++v) {
        const f32x4 p = red[v][t][lane];
        acc[t][0] += p[0]; acc[t][1] += p[1]; acc[t][2] += p[2]; acc[t][3] += p[3];
      }
    }
  }

  const int m = r;
  if (m >= a.M) return;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int n = n0 + 16 * t + 4 * g;
    if (n >= a.N) continue;  // (N % 8 == 0: the 4 columns of a lane are inside together)
    const f32x4 sc = *(const f32x4*)(a.scale + n);
    float v[4] = {acc[t][0] * sc[0], acc[t][1] * sc[1], acc[t][2] * sc[2], acc[t][3] * sc[3]};
    if (a.bias_type == 1) {
      float bb[4];
      f8_load4_bf16((const bf16_t*)a.bias + n, bb);
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
      f8_load4_bf16(a.res + off, c);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] += c[i];
    }
    if (a.act == 2) {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = gelu_tanh(v[i]);
    }
    *(uint2*)(a.y + off) = make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
  }
}

// ---- the quantiser
__device__ __forceinline__ void f8_load16(const float* p, float* v) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x4 x = *(const f32x4*)(p + 4 * i);
    v[4 * i] = x[0]; v[4 * i + 1] = x[1]; v[4 * i + 2] = x[2]; v[4 * i + 3] = x[3];
  }
}
__device__ __forceinline__ void f8_load16(const bf16_t* p, float* v) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const uint4 x = *(const uint4*)(p + 8 * i);
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[8 * i + 2 * j] = __uint_as_float(w[j] << 16);
      v[8 * i + 2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
    }
  }
}

constexpr int kQuantRows = 4;  // rows (waves) per block

template <typename TW>
__global__ __launch_bounds__(kQuantRows * 64) void quant_fp8_rows_kernel(const TW* __restrict__ w,
                                                                         uint8_t* __restrict__ q,
                                                                         float* __restrict__ scale, int N, int K) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * kQuantRows + (threadIdx.x >> 6);
  if (n >= N) return;  // (wave-uniform; no barrier below)
  const TW* row = w + (long long)n * K;
  float v[16], amax = 0.f;
  for (int k = 16 * lane; k < K; k += 16 * 64) {
    f8_load16(row + k, v);
#pragma unroll
    for (int i = 0; i < 16; ++i) amax = fmaxf(amax, fabsf(v[i]));
  }
  amax = wave_max(amax);
  const float s = fp8_scale(amax);
  if (lane == 0) scale[n] = s;
  uint8_t* qrow = q + (long long)n * K;
  for (int k = 16 * lane; k < K; k += 16 * 64) {
    f8_load16(row + k, v);
    *(uint4*)(qrow + k) = make_uint4(fp8_pack4(v, s), fp8_pack4(v + 4, s), fp8_pack4(v + 8, s), fp8_pack4(v + 12, s));
  }
}

}  // namespace rtdc

using namespace rtdc;

// The launch plan, a function of (N, K) alone: T column tiles of 16 per block, W waves per block
// (a power of two; at most 8 where T > 1) and `per` chunks of 128 k per wave.  A (tile, wave) pair
// is one stream of loads with U chunks of 2 KiB in flight.  The chip wants 16 .. 32 MiB in flight
// (~64 .. 128 KiB per CU, what gemm_few_rows.hip keeps): a weight that still reaches 16 MiB with
// T = 4 (then T = 2) has streams to spare and spends them on x reuse; small weights keep T = 1
// and take many waves.  W grows while the bytes in flight stay under 32 MiB; a wave never gets
// less than one chunk where there is one to give, and W never exceeds the chunk count.
extern "C" void rtdc_few_rows_fp8_plan(long long N, long long K, int* tiles_per_block, int* waves, int* per) {
  const long long tiles = (N + 15) / 16, chunks = K / 128;
  int wcap = 1;
  while (wcap < kF8MaxWavesT && 2 * wcap <= chunks) wcap *= 2;
  int T = 1;
  if (tiles * wcap * f8_group(4) * 2 >= kF8InFlight) T = 4;
  else if (tiles * wcap * f8_group(2) * 2 >= kF8InFlight) T = 2;
  const long long blocks = (tiles + T - 1) / T;
  const int wmax = T == 1 ? kF8MaxWaves : kF8MaxWavesT;
  int W = 1;
  while (W < wmax && blocks * T * f8_group(T) * (2 * W) <= kF8InFlight && 2 * W <= chunks) W *= 2;
  *tiles_per_block = T;
  *waves = W;
  *per = (int)((chunks + W - 1) / W);
}

extern "C" int rtdc_gemm_few_rows_fp8(const void* x, const void* q, const void* scale, const void* bias,
                                      int bias_type, const void* res, void* y, int M, int N, int K, int act,
                                      hipStream_t st) {
  if (M < 1 || M > 16 || N < 8 || N % 8 != 0 || K < 128 || K % 128 != 0) return 1;
  if ((act != 0 && act != 2) || bias_type < 0 || bias_type > 2 || (bias_type != 0) != (bias != nullptr)) return 1;
  if (!x || !q || !scale || !y) return 1;
  FewRowsFp8Args a;
  a.x = (const bf16_t*)x;
  a.q = (const uint8_t*)q;
  a.scale = (const float*)scale;
  a.bias = bias;
  a.res = (const bf16_t*)res;
  a.y = (bf16_t*)y;
  a.M = M;
  a.N = N;
  a.K = K;
  a.bias_type = bias_type;
  a.act = act;
  a.chunks = K / 128;
  int T = 1, W = 1;
  rtdc_few_rows_fp8_plan(N, K, &T, &W, &a.per);
  const dim3 grid((unsigned)((N + 16 * T - 1) / (16 * T)));
#define RTDC_F8_CASE(t, w) \
  case 100 * t + w: hipLaunchKernelGGL((few_rows_fp8_kernel<t, w>), grid, dim3(w * 64), 0, st, a); break;
  switch (100 * T + W) {
    RTDC_F8_CASE(1, 1) RTDC_F8_CASE(1, 2) RTDC_F8_CASE(1, 4) RTDC_F8_CASE(1, 8) RTDC_F8_CASE(1, 16)
    RTDC_F8_CASE(2, 1) RTDC_F8_CASE(2, 2) RTDC_F8_CASE(2, 4) RTDC_F8_CASE(2, 8)
    RTDC_F8_CASE(4, 1) RTDC_F8_CASE(4, 2) RTDC_F8_CASE(4, 4) RTDC_F8_CASE(4, 8)
    default: return 1;
  }
#undef RTDC_F8_CASE
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

// w [N, K] contiguous, fp32 (src_bf16 = 0) or bf16; K % 16 == 0 (16 elements per lane and step)
extern "C" int rtdc_quantize_fp8_rows(const void* w, int src_bf16, void* q, void* scale, long long N, long long K,
                                      hipStream_t st) {
  if (N < 1 || K < 16 || K % 16 != 0 || N > INT32_MAX || K > INT32_MAX || !w || !q || !scale) return 1;
  const dim3 grid((unsigned)((N + kQuantRows - 1) / kQuantRows)), block(kQuantRows * 64);
  if (src_bf16)
    hipLaunchKernelGGL((quant_fp8_rows_kernel<bf16_t>), grid, block, 0, st, (const bf16_t*)w, (uint8_t*)q,
                       (float*)scale, (int)N, (int)K);
  else
    hipLaunchKernelGGL((quant_fp8_rows_kernel<float>), grid, block, 0, st, (const float*)w, (uint8_t*)q,
                       (float*)scale, (int)N, (int)K);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
