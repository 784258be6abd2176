// LayerNorm / RMSNorm forward + backward for bf16 activations (gfx950).
//
// One wave64 per row; each lane owns CPL 16-B chunks (8 bf16) of the row, so the row lives in
// registers between the statistics pass and the normalisation pass (one HBM read, one write).
// Backward fuses the residual-gradient add (dx = dres + LN'(dy)) and writes per-wave partial
// dgamma/dbeta rows to a workspace that a second kernel reduces in a fixed order, so the
// parameter gradients are bitwise reproducible (no float atomics, MI355X_MICROARCH.md §Global
// float atomics).
#include "gemm_common.h"

#include <cstdint>
#include <cstdlib>

namespace rtdc {

__device__ __forceinline__ void ld8(const bf16_t* p, float* v) {
  uint4 x = *(const uint4*)p;
  uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = __uint_as_float(w[i] << 16);
    v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}
__device__ __forceinline__ void st8(bf16_t* p, const float* v) {
  uint4 x = make_uint4(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]),
                       pack_bf2(v[6], v[7]));
  *(uint4*)p = x;
}

// red4[q] = (add ? red4[q] + v : v) for the 4 floats v (per-block partial-sum combine in LDS)
__device__ __forceinline__ void red_acc4(float* red, int q, const float* v, int add) {
  f32x4* p = (f32x4*)red + q;
  f32x4 a = {v[0], v[1], v[2], v[3]};
  if (add) a = *p + a;
  *p = a;
}

template <int CPL, bool RMS>
__global__ __launch_bounds__(256) void norm_fwd_kernel(const bf16_t* __restrict__ x,
                                                      const bf16_t* __restrict__ g,
                                                      const bf16_t* __restrict__ b,
                                                      bf16_t* __restrict__ y, float* __restrict__ mean_out,
                                                      float* __restrict__ rstd_out, int M, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int nch = D >> 3;
  const bf16_t* xr = x + (long long)row * D;
  float v[CPL][8];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const int c = lane + 64 * i;
    if (c < nch) {
      ld8(xr + c * 8, v[i]);
#pragma unroll
      for (int e = 0; e < 8; ++e) s += v[i][e];
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[i][e] = 0.f;
    }
  }
  float mean = 0.f;
  if (!RMS) mean = wave_sum(s) / D;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const int c = lane + 64 * i;
    if (c < nch) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float d = v[i][e] - mean;
        ss += d * d;
      }
    }
  }
  const float rstd = rsqrtf(wave_sum(ss) / D + eps);
  if (lane == 0) {
    if (mean_out) mean_out[row] = mean;
    rstd_out[row] = rstd;
  }
  bf16_t* yr = y + (long long)row * D;
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const int c = lane + 64 * i;
    if (c < nch) {
      float gg[8], bb[8], o[8];
      ld8(g + c * 8, gg);
      if (!RMS) ld8(b + c * 8, bb);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (v[i][e] - mean) * rstd * gg[e] + (RMS ? 0.f : bb[e]);
      st8(yr + c * 8, o);
    }
  }
}

// A lane's chunk of VW bf16: 16 B (VW = 8) or 8 B (VW = 4), as the backward kernel loads, unpacks
// and stores it.  The 16-B chunk goes in by reference and through unpack8bf, the 8-B one by value:
// the kernel's row loop is compiled with floating-point contraction on, which multiply-adds the
// compiler fuses there follows details like these, and the bits of dx and of its column sums
// follow the fusing (profiles/norm_bwd_merge.md: a by-value 16-B chunk changed them at D >= 2048).
template <int VW>
struct BfChunk;
template <>
struct BfChunk<8> {
  using raw = uint4;
  static __device__ __forceinline__ void unpack(const uint4& q, float* v) {
    unpack8bf(u32x4{q.x, q.y, q.z, q.w}, v);
  }
  static __device__ __forceinline__ void store(bf16_t* p, const float* v) { st8(p, v); }
};
template <>
struct BfChunk<4> {
  using raw = uint2;
  static __device__ __forceinline__ void unpack(uint2 q, float* v) {
    v[0] = __uint_as_float(q.x << 16);
    v[1] = __uint_as_float(q.x & 0xffff0000u);
    v[2] = __uint_as_float(q.y << 16);
    v[3] = __uint_as_float(q.y & 0xffff0000u);
  }
  static __device__ __forceinline__ void store(bf16_t* p, const float* v) {
    *(uint2*)p = make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
  }
};

// dxhat = dy*g ; dx = rstd * (dxhat - mean(dxhat) - xhat * mean(dxhat*xhat))   (LayerNorm)
// dx = rstd * (dxhat - xhat * mean(dxhat*xhat))                                  (RMSNorm)
// CS: also the column sums of dx itself (the residual-stream gradient this kernel produces is
// the output gradient of the block's residual projection, whose bias gradient is exactly that
// colsum - computed here on the way out instead of re-reading dx in a separate reduction).
// Partial rows per block: ws_dg [nblk][D], ws_db = ws_dg + nblk*D, ws_cs = ws_db + nblk*D.
// VW: elements per lane chunk.  8 (16-B chunks) for every width; 4 (8-B chunks) for widths whose
// 16-B chunk count is not a multiple of 64 (GPT-2: D = 768 -> 96 chunks of 8, so the 16-B form
// leaves half the lanes idle in its second chunk and carries [2][8] accumulators; 192 chunks of
// 4 = 3 per lane, every lane busy, [3][4] accumulators: fewer VGPRs, more waves per SIMD for this
// latency-bound stream).  Same math, same per-block partial rows.
template <int VW, int CPL, bool RMS, bool CS>
__global__ __launch_bounds__(256) void norm_bwd_kernel(
    const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x, const bf16_t* __restrict__ g,
    const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
    const bf16_t* __restrict__ dres, bf16_t* __restrict__ dx, float* __restrict__ ws_dg,
    float* __restrict__ ws_db, float* __restrict__ ws_cs, int M, int D) {
  using Chunk = BfChunk<VW>;
  using raw_t = typename Chunk::raw;
  const int lane = threadIdx.x & 63;
  const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nw = gridDim.x * 4;
  const int nch = D >> (VW == 8 ? 3 : 2);
  float adg[CPL][VW], adb[CPL][VW], acs[CS ? CPL : 1][VW];
#pragma unroll
  for (int i = 0; i < CPL; ++i)
#pragma unroll
    for (int e = 0; e < VW; ++e) adg[i][e] = adb[i][e] = 0.f;
#pragma unroll
  for (int i = 0; i < (CS ? CPL : 1); ++i)
#pragma unroll
    for (int e = 0; e < VW; ++e) acs[i][e] = 0.f;

  float gg[CPL][VW];
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const int c = lane + 64 * i;
    if (c < nch) Chunk::unpack(*(const raw_t*)(g + c * VW), gg[i]);
  }

  // rows are software-pipelined: the next row's x / dy / dres (and its statistics) are in
  // flight while this row is reduced and written (a wave owns M/nw rows in sequence)
  raw_t px[CPL], pd[CPL], pr[CPL];
  float pmean = 0.f, prstd = 0.f;
  auto fetch = [&](int r) {
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const int c = lane + 64 * i;
      if (c < nch) {
        px[i] = *(const raw_t*)(x + (long long)r * D + c * VW);
        pd[i] = *(const raw_t*)(dy + (long long)r * D + c * VW);
        if (dres) pr[i] = *(const raw_t*)(dres + (long long)r * D + c * VW);
      }
    }
    pmean = RMS ? 0.f : mean_in[r];
    prstd = rstd_in[r];
  };
  if (gw < M) fetch(gw);
  for (int row = gw; row < M; row += nw) {
    const float mean = pmean;
    const float rstd = prstd;
    raw_t cx[CPL], cd[CPL], rraw[CPL];
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      cx[i] = px[i];
      cd[i] = pd[i];
      rraw[i] = pr[i];
    }
    if (row + nw < M) fetch(row + nw);
    float xh[CPL][VW], dxh[CPL][VW];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const int c = lane + 64 * i;
      if (c < nch) {
        float xv[VW], dv[VW];
        Chunk::unpack(cx[i], xv);
        Chunk::unpack(cd[i], dv);
#pragma unroll
        for (int e = 0; e < VW; ++e) {
          xh[i][e] = (xv[e] - mean) * rstd;
          dxh[i][e] = dv[e] * gg[i][e];
          s1 += dxh[i][e];
          s2 += dxh[i][e] * xh[i][e];
          adg[i][e] += dv[e] * xh[i][e];
          adb[i][e] += dv[e];
        }
      }
    }
    const float m1 = RMS ? 0.f : wave_sum(s1) / D;
    const float m2 = wave_sum(s2) / D;
    bf16_t* dxr = dx + (long long)row * D;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const int c = lane + 64 * i;
      if (c < nch) {
        float o[VW], r[VW];
        if (dres) Chunk::unpack(rraw[i], r);
#pragma unroll
        for (int e = 0; e < VW; ++e) {
          o[e] = rstd * (dxh[i][e] - m1 - xh[i][e] * m2);
          if (dres) o[e] += r[e];
          if constexpr (CS) acs[i][e] += o[e];
        }
        Chunk::store(dxr + c * VW, o);
      }
    }
  }
  // combine the block's 4 waves in LDS (fixed wave order), one partial row per block
  extern __shared__ float red[];  // [D] dgamma (+ [D] dbeta) (+ [D] colsum(dx))
  constexpr int KCS = RMS ? 1 : 2;
  const int wv = threadIdx.x >> 6;
  for (int w = 0; w < 4; ++w) {
    if (wv == w) {
#pragma unroll
      for (int i = 0; i < CPL; ++i) {
        const int c = lane + 64 * i;
        if (c < nch) {
          // 16-B LDS accesses (scalar ones at a lane stride of a whole chunk were 8-way (VW = 8)
          // and 4-way (VW = 4) bank conflicts)
#pragma unroll
          for (int h = 0; h < VW / 4; ++h) {
            red_acc4(red, c * (VW / 4) + h, adg[i] + 4 * h, w);
            if (!RMS) red_acc4(red, D / 4 + c * (VW / 4) + h, adb[i] + 4 * h, w);
            if constexpr (CS) red_acc4(red, KCS * D / 4 + c * (VW / 4) + h, acs[i] + 4 * h, w);
          }
        }
      }
    }
    __syncthreads();
  }
  for (int d = threadIdx.x; d < D; d += 256) {
    ws_dg[(long long)blockIdx.x * D + d] = red[d];
    if (!RMS) ws_db[(long long)blockIdx.x * D + d] = red[D + d];
    if constexpr (CS) ws_cs[(long long)blockIdx.x * D + d] = red[KCS * D + d];
  }
}

// out[d] (+)= sum_w ws[w][d], fixed summation order.  A block owns 64 columns; its 4 waves
// stride over the W partial rows (coalesced 256-B rows per wave) and combine through LDS,
// so a 1024 x 768 workspace is 12 blocks x 256 loads per lane instead of 768 serial chains.
// Sum W partial rows of ws [W][D] -> out[S][D] where block (x, y) reduces rows
// [y*R, (y+1)*R) of 64 columns; 4 waves stride the rows, combined in LDS in fixed order.
// Run twice (W -> S -> 1) so every thread keeps only a few independent loads in flight and
// the reduction order is fixed (deterministic).
struct OutPtrs {
  float* p[4];
};
// out: tmp + z * out_z when tmp is set (first of two stages), else outs.p[z]
__global__ __launch_bounds__(256) void colsum_ws_kernel(const float* __restrict__ ws, float* __restrict__ tmp,
                                                       OutPtrs outs, int W, int D, int R, int accumulate,
                                                       long long ws_z, long long out_z) {
  __shared__ float part[4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  ws += blockIdx.z * ws_z;  // z = independent reductions batched into one launch
  float* out = tmp ? tmp + blockIdx.z * out_z : outs.p[blockIdx.z];
  const int d = blockIdx.x * 64 + lane;
  const int r0 = blockIdx.y * R, r1 = min(W, r0 + R);
  float s0 = 0.f, s1 = 0.f;
  if (d < D) {
    int w = r0 + wv;
    for (; w + 4 < r1; w += 8) {
      s0 += ws[(long long)w * D + d];
      s1 += ws[(long long)(w + 4) * D + d];
    }
    if (w < r1) s0 += ws[(long long)w * D + d];
  }
  part[wv][lane] = s0 + s1;
  __syncthreads();
  if (wv == 0 && d < D) {
    const float t = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
    float* o = out + (long long)blockIdx.y * D + d;
    *o = (accumulate && gridDim.y == 1) ? *o + t : t;
  }
}

// One launch for up to kWideMaxRows partial rows: a 1024-thread block owns 64 columns; its 16
// waves stride the rows (wave w: rows w, w+16, ...) with kWideU loads in flight per lane, and
// the 16 wave partials are added in wave order in LDS - a fixed order for a given W
// (bitwise reproducible).  The two-launch form (W -> W/32 -> 1) paid a second launch and a
// kernel-boundary drain per reduction (~50 per GPT-2 step).
constexpr int kWideU = 12, kWideMaxRows = 4096;
// The calling 1024-thread block reduces columns [d0, d0 + 64) of one job: out[d] (+)= sum_w ws[w][d].
// The one body of colsum_wide_kernel and colsum_multi_kernel.
__device__ __forceinline__ void colsum_wide_cols(const float* __restrict__ ws, float* out, int W, int D, int d0,
                                                 bool accumulate) {
  __shared__ float part[16][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int d = d0 + lane;
  float acc = 0.f;
  if (d < D) {
    for (int w0 = wv; w0 < W; w0 += 16 * kWideU) {
      float v[kWideU];
#pragma unroll
      for (int u = 0; u < kWideU; ++u) {
        const int w = w0 + 16 * u;
        v[u] = w < W ? ws[(long long)w * D + d] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < kWideU; ++u) acc += v[u];
    }
  }
  part[wv][lane] = acc;
  __syncthreads();
  if (wv == 0 && d < D) {
    float t = part[0][lane];
#pragma unroll
    for (int i = 1; i < 16; ++i) t += part[i][lane];
    float* o = out + d;
    *o = accumulate ? *o + t : t;
  }
}

// z = independent reductions batched into one launch: ws + z*ws_z [W][D] -> outs.p[z]
__global__ __launch_bounds__(1024) void colsum_wide_kernel(const float* __restrict__ ws, OutPtrs outs, int W, int D,
                                                          int accumulate, long long ws_z) {
  colsum_wide_cols(ws + blockIdx.z * ws_z, outs.p[blockIdx.z], W, D, blockIdx.x * 64, accumulate);
}

// Deferred column-sum reductions of one backward window in ONE launch (ops/gemm.py: the bias /
// LayerNorm-parameter gradients of two layers flushed with their grouped weight gradients):
// job j = ws_j [W_j][D_j] partial rows -> out_j [D_j]; block b works on 64 columns of the job
// whose block range holds b.  Per job it runs colsum_wide_cols, the very function
// colsum_wide_kernel runs, so the result is bitwise the non-deferred one by construction.
constexpr int kMultiJobs = 32;
struct ColsumJobs {
  const float* ws[kMultiJobs];
  float* out[kMultiJobs];
  int W[kMultiJobs];
  int D[kMultiJobs];
  int start[kMultiJobs + 1];
  unsigned accumulate;  // bit j: out_j += sum
  int n;
};
static_assert(sizeof(ColsumJobs) <= 4096, "kernel argument segment");

__global__ __launch_bounds__(1024) void colsum_multi_kernel(ColsumJobs jobs) {
  const int b = blockIdx.x;
  int j = 0;
#pragma unroll
  for (int i = 1; i < kMultiJobs; ++i) j += (i < jobs.n && b >= jobs.start[i]) ? 1 : 0;
  j = __builtin_amdgcn_readfirstlane(j);
  colsum_wide_cols(jobs.ws[j], jobs.out[j], jobs.W[j], jobs.D[j], (b - jobs.start[j]) * 64, (jobs.accumulate >> j) & 1u);
}

static bool colsum_wide_enabled() {
  static int v = -1;  // RTDC_COLSUM_WIDE=0: the two-launch form (A/B)
  if (v < 0) {
    const char* e = getenv("RTDC_COLSUM_WIDE");
    v = (e && e[0] == '0') ? 0 : 1;
  }
  return v == 1;
}

// nz <= 4 independent reductions ws + z*ws_z [W][D] (W partial rows) -> outs.p[z] [D];
// tmp holds nz x S intermediate rows (nz * 64 * D floats).
static void colsum_ws_reduce(const float* ws, int W, int D, float* tmp, OutPtrs outs, int accumulate,
                             hipStream_t st, int nz = 1, long long ws_z = 0) {
  int S = W / 32;
  S = S < 1 ? 1 : (S > 64 ? 64 : S);
  // every W the wide kernel takes goes through it - also a handful of rows: the deferred form
  // (colsum_multi_kernel) sums in its order, so a reduction's bits must not depend on whether
  // its target was a deferrable gradient slot
  if (W <= kWideMaxRows && colsum_wide_enabled()) {
    hipLaunchKernelGGL(colsum_wide_kernel, dim3((D + 63) / 64, 1, nz), dim3(1024), 0, st, ws, outs, W, D, accumulate,
                       ws_z);
  } else if (S > 1 && tmp) {
    const int R = (W + S - 1) / S;
    hipLaunchKernelGGL(colsum_ws_kernel, dim3((D + 63) / 64, S, nz), dim3(256), 0, st, ws, tmp, outs, W, D, R, 0,
                       ws_z, 64LL * D);
    hipLaunchKernelGGL(colsum_ws_kernel, dim3((D + 63) / 64, 1, nz), dim3(256), 0, st, (const float*)tmp,
                       (float*)nullptr, outs, S, D, S, accumulate, 64LL * D, 0LL);
  } else {
    hipLaunchKernelGGL(colsum_ws_kernel, dim3((D + 63) / 64, 1, nz), dim3(256), 0, st, ws, (float*)nullptr, outs, W,
                       D, W, accumulate, ws_z, 0LL);
  }
}
static OutPtrs outs1(float* a, float* b = nullptr, float* c = nullptr) { return OutPtrs{{a, b, c, nullptr}}; }

// Column sums of a [M][N] matrix (bias gradient), stage 1: block (x, y) reduces rows
// [x*R, (x+1)*R) of columns [y*512, y*512+512): lane = 8 columns (16-B loads for bf16), the 4
// waves stride the rows and are combined in LDS -> ws[x][N].  Stage 2 = colsum_ws_reduce.
__device__ __forceinline__ float as_f(bf16_t v) { return bf2f(v); }
__device__ __forceinline__ float as_f(float v) { return v; }
template <typename T>
__device__ __forceinline__ void ld8c(const T* p, float* v);
template <>
__device__ __forceinline__ void ld8c<bf16_t>(const bf16_t* p, float* v) { ld8(p, v); }
template <>
__device__ __forceinline__ void ld8c<float>(const float* p, float* v) {
  const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void colsum_partial_kernel(const T* __restrict__ X, int M, int N, int ld,
                                                            int rows_per_block, float* __restrict__ ws) {
  __shared__ float part[4][512];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int c = blockIdx.y * 512 + lane * 8;
  const int r0 = blockIdx.x * rows_per_block;
  const int r1 = min(M, r0 + rows_per_block);
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (c < N) {
    for (int r = r0 + wv; r < r1; r += 4) {
      float v[8];
      if constexpr (VEC) {
        ld8c<T>(X + (long long)r * ld + c, v);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = c + e < N ? as_f(X[(long long)r * ld + c + e]) : 0.f;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] += v[e];
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) part[wv][lane * 8 + e] = a[e];
  __syncthreads();
  for (int j = threadIdx.x; j < 512; j += 256) {
    const int n = blockIdx.y * 512 + j;
    if (n < N) ws[(long long)blockIdx.x * N + n] = (part[0][j] + part[1][j]) + (part[2][j] + part[3][j]);
  }
}

}  // namespace rtdc

using namespace rtdc;

template <bool RMS>
static int launch_norm_fwd(const void* x, const void* g, const void* b, void* y, float* mean,
                           float* rstd, int M, int D, float eps, hipStream_t st) {
  if (D % 8 != 0) return 1;
  const int cpl = (D / 8 + 63) / 64;
  dim3 grid((M + 3) / 4), block(256);
#define L(C)                                                                                  \
  hipLaunchKernelGGL((norm_fwd_kernel<C, RMS>), grid, block, 0, st, (const bf16_t*)x,         \
                     (const bf16_t*)g, (const bf16_t*)b, (bf16_t*)y, mean, rstd, M, D, eps)
  if (cpl <= 1) L(1);
  else if (cpl <= 2) L(2);
  else if (cpl <= 4) L(4);
  else if (cpl <= 8) L(8);
  else if (cpl <= 16) L(16);
  else return 1;
#undef L
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

// The norm_bwd_kernel instantiation that runs a width, handed to f as a Kernel<...> tag: the one
// place that picks it, so the occupancy query and the launch (both inside f) name the same kernel.
// Returns f's result, 1 for an unsupported width.
template <auto K>
struct Kernel {
  static constexpr auto fn = K;
};
template <int VW, int CPL, bool RMS, typename F>
static int with_norm_bwd_cs(bool cs, F& f) {
  if constexpr (!RMS) {  // (RMSNorm never takes the dx column sums)
    if (cs) return f(Kernel<norm_bwd_kernel<VW, CPL, RMS, true>>{});
  }
  return f(Kernel<norm_bwd_kernel<VW, CPL, RMS, false>>{});
}
template <bool RMS, typename F>
static int with_norm_bwd_kernel(int D, bool cs, F f) {
  static int vw4_env = -1;
  if (vw4_env < 0) {
    const char* e = getenv("RTDC_NORM_BWD_VW4");
    vw4_env = (e && e[0] == '0') ? 0 : 1;
  }
  // 8-B chunks when they fill every lane (D/4 a multiple of 64) and 16-B ones would not, up to 4
  // chunks per lane: D/4 = 64 * odd and <= 256, so D is 256 or 768 and a lane owns 1 or 3 chunks
  if (vw4_env && (D / 8) % 64 != 0 && (D / 4) % 64 == 0 && D / 4 <= 64 * 4)
    return D / 4 == 64 ? with_norm_bwd_cs<4, 1, RMS>(cs, f) : with_norm_bwd_cs<4, 3, RMS>(cs, f);
  const int cpl = (D / 8 + 63) / 64;
  if (cpl <= 1) return with_norm_bwd_cs<8, 1, RMS>(cs, f);
  if (cpl <= 2) return with_norm_bwd_cs<8, 2, RMS>(cs, f);
  if (cpl <= 4) return with_norm_bwd_cs<8, 4, RMS>(cs, f);
  if (cpl <= 8) return with_norm_bwd_cs<8, 8, RMS>(cs, f);
  return 1;
}

// resident 256-thread blocks of kernel K on this device (cached per kernel)
template <auto K>
static int resident_blocks(size_t lds) {
  static int cus = 0, occ = 0;
  static size_t occ_lds = ~(size_t)0;
  if (cus == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      cus = 256;
  }
  if (lds != occ_lds) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, K, 256, lds) != hipSuccess || occ <= 0) occ = 1;
    occ_lds = lds;
  }
  return cus * occ;
}

// ws layout: [nz][nblk][D] partials (dgamma | dbeta | colsum(dx)) | nz x [64][D] level-2 rows,
// nz = (RMS ? 1 : 2) + (dxsum != nullptr).  The outputs are written, never accumulated.
template <bool RMS>
static int launch_norm_bwd(const void* dy, const void* x, const void* g, const float* mean,
                           const float* rstd, const void* dres, void* dx, float* ws, float* dg,
                           float* db, float* dxsum, int M, int D, int nwaves, hipStream_t st,
                           int* nblk_out = nullptr) {
  if (D % 8 != 0 || nwaves % 4 != 0) return 1;
  const bool cs = dxsum != nullptr;
  const int nz = (RMS ? 1 : 2) + (cs ? 1 : 0);
  const size_t lds = (size_t)nz * D * sizeof(float);
  if (lds > 160 * 1024) return 1;
  int nblk = 0;
  const int rc = with_norm_bwd_kernel<RMS>(D, cs, [&](auto k) {
    // one wave of blocks: a grid past the resident block slots leaves a partial second wave
    // (GPT-2: 1024 blocks on 768 slots ran 0.94 ms/step of LayerNorm backward, 768 blocks 0.67)
    constexpr auto kernel = decltype(k)::fn;
    const int slots = resident_blocks<kernel>(lds);
    nblk = nwaves / 4 < slots ? nwaves / 4 : slots;
    const long long part = (long long)nblk * D;
    hipLaunchKernelGGL(kernel, dim3(nblk), dim3(256), lds, st, (const bf16_t*)dy, (const bf16_t*)x,
                       (const bf16_t*)g, mean, rstd, (const bf16_t*)dres, (bf16_t*)dx, ws, ws + part,
                       ws + (RMS ? 1 : 2) * part, M, D);
    return 0;
  });
  if (rc) return rc;
  if (nblk_out) {  // deferred: the caller reduces the [nz][nblk][D] partials (rtdc_colsum_multi)
    *nblk_out = nblk;
    return hipGetLastError() == hipSuccess ? 0 : 2;
  }
  // one reduction launch (pair) for all of them
  const long long part = (long long)nblk * D;
  const OutPtrs o = RMS ? outs1(dg) : outs1(dg, db, dxsum);
  colsum_ws_reduce(ws, nblk, D, ws + nz * part, o, 0, st, nz, part);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

extern "C" int rtdc_layernorm_fwd(const void* x, const void* g, const void* b, void* y, float* mean,
                                  float* rstd, int M, int D, float eps, hipStream_t st) {
  return launch_norm_fwd<false>(x, g, b, y, mean, rstd, M, D, eps, st);
}
extern "C" int rtdc_rmsnorm_fwd(const void* x, const void* g, void* y, float* rstd, int M, int D,
                                float eps, hipStream_t st) {
  return launch_norm_fwd<true>(x, g, nullptr, y, nullptr, rstd, M, D, eps, st);
}
extern "C" int rtdc_layernorm_bwd(const void* dy, const void* x, const void* g, const float* mean,
                                  const float* rstd, const void* dres, void* dx, float* ws,
                                  float* dg, float* db, float* dxsum, int M, int D, int nwaves,
                                  hipStream_t st, int* nblk_out) {
  return launch_norm_bwd<false>(dy, x, g, mean, rstd, dres, dx, ws, dg, db, dxsum, M, D, nwaves, st, nblk_out);
}
extern "C" int rtdc_rmsnorm_bwd(const void* dy, const void* x, const void* g, const float* rstd,
                                const void* dres, void* dx, float* ws, float* dg, int M, int D, int nwaves,
                                hipStream_t st) {
  return launch_norm_bwd<true>(dy, x, g, nullptr, rstd, dres, dx, ws, dg, nullptr, nullptr, M, D, nwaves, st);
}
// out[D] (+)= sum of W partial rows ws[W][D] (tmp: 64 * D floats of scratch); called by the GEMM
// launcher (gemm_bf16.hip) on the partial rows its gelu-backward epilogue leaves
extern "C" int rtdc_colsum_rows(const float* ws, int W, int D, float* tmp, float* out, int accumulate,
                                hipStream_t st) {
  colsum_ws_reduce(ws, W, D, tmp, outs1(out), accumulate, st);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
// n <= 32 deferred reductions (see colsum_multi_kernel); every W_j <= kWideMaxRows
extern "C" int rtdc_colsum_multi(const float* const* ws, float* const* out, const int* W, const int* D,
                                 const int* accumulate, int n, hipStream_t st) {
  if (n < 1 || n > kMultiJobs) return 1;
  ColsumJobs jobs{};
  int blocks = 0;
  for (int i = 0; i < n; ++i) {
    if (W[i] < 1 || W[i] > kWideMaxRows || D[i] < 1) return 1;
    jobs.ws[i] = ws[i];
    jobs.out[i] = out[i];
    jobs.W[i] = W[i];
    jobs.D[i] = D[i];
    jobs.start[i] = blocks;
    if (accumulate[i]) jobs.accumulate |= 1u << i;
    blocks += (D[i] + 63) / 64;
  }
  jobs.start[n] = blocks;
  jobs.n = n;
  hipLaunchKernelGGL(colsum_multi_kernel, dim3((unsigned)blocks), dim3(1024), 0, st, jobs);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

// stage 1 of a column sum: the partial rows ws [nblk][N] of X [M][N]
static void launch_colsum_partial(const void* X, int M, int N, int ld, float* ws, int nblk, int is_bf16,
                                  hipStream_t st) {
  // the 16-B loads need the pointer aligned too (a view that starts inside a row is not)
  const bool vec = N % 8 == 0 && ld % 8 == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
  const int rpb = (M + nblk - 1) / nblk;
  dim3 grid(nblk, (N + 511) / 512), block(256);
#define CS(T, V) hipLaunchKernelGGL((colsum_partial_kernel<T, V>), grid, block, 0, st, (const T*)X, M, N, ld, rpb, ws)
  if (is_bf16) {
    if (vec) CS(bf16_t, true); else CS(bf16_t, false);
  } else {
    if (vec) CS(float, true); else CS(float, false);
  }
#undef CS
}

// stage 1 only; the reduction is deferred to rtdc_colsum_multi
extern "C" int rtdc_colsum_partial(const void* X, int M, int N, int ld, float* ws, int nblk, int is_bf16,
                                   hipStream_t st) {
  launch_colsum_partial(X, M, N, ld, ws, nblk, is_bf16, st);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

extern "C" int rtdc_colsum(const void* X, int M, int N, int ld, float* ws, int nblk, float* out,
                           int accumulate, int is_bf16, hipStream_t st) {
  // ws: [nblk][N] partials followed by [64][N] level-2 rows
  launch_colsum_partial(X, M, N, ld, ws, nblk, is_bf16, st);
  colsum_ws_reduce(ws, nblk, N, ws + (long long)nblk * N, outs1(out), accumulate, st);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
