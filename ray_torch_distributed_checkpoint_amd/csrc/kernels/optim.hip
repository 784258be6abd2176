// Fused optimizers over FLAT parameter/state buffers (gfx950).
//
// The framework keeps every parameter, gradient and optimizer state of a model in one
// contiguous buffer per kind (FlatParamSpace), so an optimizer step is ONE launch over a
// chunk table instead of ATen's multi-tensor-apply foreach chain (reference: SGD(momentum=0.9)
// at R/my_ray_module.py:142,160 -> torch/optim/sgd.py _multi_tensor_sgd).  A chunk is a slice
// of one parameter (never crossing parameters) carrying that parameter's weight-decay flag;
// segments are 64-element aligned so every lane moves 16 B per load.
//
// AdamW: fp32 master + m + v, optional bf16 shadow written in the same pass (the copy the
// bf16 MFMA kernels read).  grad_scale folds the DDP 1/world pre-divide into the step.
// A chunk carries two offsets: `start` into the flat parameter / gradient / shadow buffers and
// `sstart` into the optimizer-state buffers.  Without ZeRO they are equal; under ZeRO-1 the
// state buffers hold only this rank's owned shards back to back (1/world of the bytes), so
// `sstart` is the chunk's position in that compact buffer.
// Semantics follow torch.optim.AdamW / SGD (decoupled weight decay; SGD first-step clone).
//
// `skip` (optional): a communicator health word (the one-shot P2P all-reduce's host-coherent
// error flag, csrc/runtime/p2p_comm.cpp).  When a gradient collective earlier on this stream
// timed out it poisoned its bucket with NaN and set the word; the update then becomes a no-op,
// so a NaN gradient can never reach the parameters or the optimizer state - also inside a
// replayed hipGraph, where no host code runs between the collective and the step.
//
// Host side: two launchers, rtdc_adamw and rtdc_sgd, each taking one argument struct (args.h).
#include "args.h"
#include "common.h"

namespace rtdc {

__device__ __forceinline__ bool comm_poisoned(const int* skip) {
  return skip != nullptr && __hip_atomic_load(skip, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0;
}

struct Chunk {
  long long start;   // offset into p / g / shadow
  int len;
  int decay;
  long long sstart;  // offset into the optimizer state (m, v / momentum buffer)
};
static_assert(sizeof(Chunk) == 24, "chunk table rows are 3 x int64");

// ---- device-resident step state (DevStep, args.h) ---------------------------------------------
// Read once per block, before the chunk loop (wave-uniform addresses: scalar loads).  Both indices
// are clamped into their tables whatever the counter holds.
__device__ __forceinline__ long long dev_step(const DevStep& ds, float& lr) {
  const long long n = *ds.count;
  const long long k = n < 0 ? 0 : (n < ds.L ? n : ds.L - 1);
  lr = ds.lr[k];
  return n + 1 + ds.step_off;  // the Adam step number t of this launch's parameters
}
__device__ __forceinline__ void dev_bias(const DevStep& ds, long long t, float& bc1, float& bc2_sqrt) {
  const long long r = (t < 1 ? 1 : (t < ds.Lbc ? t : ds.Lbc)) - 1;
  bc1 = ds.bc[2 * r];
  bc2_sqrt = ds.bc[2 * r + 1];
}

__global__ void optim_step_advance_kernel(long long* count) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *count += 1;
}

template <bool DEV>
__global__ __launch_bounds__(256) void adamw_kernel(const Chunk* __restrict__ chunks, int nchunks,
                                                   float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v,
                                                   bf16_t* __restrict__ shadow, float lr, float b1,
                                                   float b2, float eps, float wd, float bc1,
                                                   float bc2_sqrt, float grad_scale, const int* skip,
                                                   const float* __restrict__ clip, const DevStep ds) {
  if (comm_poisoned(skip)) return;
  if constexpr (DEV) dev_bias(ds, dev_step(ds, lr), bc1, bc2_sqrt);
  // clip (optional): {total_norm, coef} of gradnorm_finalize_kernel - the clip coefficient folds
  // into the gradient multiply
  const float gs = clip ? grad_scale * clip[1] : grad_scale;
  const float step_size = lr / bc1;
  for (int ci = blockIdx.x; ci < nchunks; ci += gridDim.x) {
    const Chunk c = chunks[ci];
    const float decay = c.decay ? (1.f - lr * wd) : 1.f;
    // One definition of the element update for the vector and the scalar path, with the fused
    // multiply-adds written out and contraction off (as in adamw_bf16state_kernel below): left to
    // the compiler, the vector copy became v = fma(b2, v, ((1 - b2) gr) gr) and the scalar copy
    // v = fma(gr, (1 - b2) gr, b2 v), so a chunk cut at an odd offset changed exp_avg_sq in the
    // last bit.  The fusions are the ones the vector path compiled to: every element of an
    // aligned chunk keeps its bits but the last len & 3 (the scalar tail), which now follow them.
    // Measured against the build before: profiles/optim_aligned_vs_parent.txt.
    auto upd = [&](float gv, float& pe, float& me, float& ve) {
#pragma clang fp contract(off)
      const float gr = gv * gs;
      me = fmaf(1.f - b1, gr, b1 * me);
      ve = fmaf(b2, ve, ((1.f - b2) * gr) * gr);
      const float denom = sqrtf(ve) / bc2_sqrt + eps;
      pe = fmaf(pe, decay, -(step_size * me / denom));
    };
    // 16-B accesses only where both offsets allow them: a chunk cut at an odd offset (a deferred-
    // tail piece, a ZeRO-1 shard boundary) takes the scalar path, as in the two kernels below
    const bool vec = (c.start & 3) == 0 && (c.sstart & 3) == 0;
    for (int i = threadIdx.x * 4; i < c.len; i += 256 * 4) {
      const long long o = c.start + i, so = c.sstart + i;
      if (vec && i + 4 <= c.len) {
        f32x4 pp = *(f32x4*)(p + o), gg = *(const f32x4*)(g + o);
        f32x4 mm = *(f32x4*)(m + so), vv = *(f32x4*)(v + so);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float pe = pp[e], me = mm[e], ve = vv[e];
          upd(gg[e], pe, me, ve);
          pp[e] = pe;
          mm[e] = me;
          vv[e] = ve;
        }
        *(f32x4*)(p + o) = pp;
        *(f32x4*)(m + so) = mm;
        *(f32x4*)(v + so) = vv;
        if (shadow) *(uint2*)(shadow + o) = make_uint2(pack_bf2(pp[0], pp[1]), pack_bf2(pp[2], pp[3]));
      } else {
        for (int e = 0; e < 4 && i + e < c.len; ++e) {
          const long long oe = o + e, se = so + e;
          float pe = p[oe], me = m[se], ve = v[se];
          upd(g[oe], pe, me, ve);
          p[oe] = pe;
          m[se] = me;
          v[se] = ve;
          if (shadow) shadow[oe] = f2bf(pe);
        }
      }
    }
  }
}

// ---- AdamW with bf16 moment state (FusedAdamW(state_dtype=torch.bfloat16)) ------------------
// m and v are STORED in bf16: 22 B per parameter and step instead of 30.  Round-to-nearest would
// freeze v (beta2 = 0.999 moves it by less than bf16's half ulp), so the stored state is rounded
// stochastically with Philox bits that are a pure function of (seed, step, flat element index):
// element e = chunk.start + i draws Philox::gen(seed, step, e >> 2)[e & 3]; exp_avg takes the low
// 16 bits of that word, exp_avg_sq the high 16.  No RNG state exists, and any cut of the chunk
// tables (deferred tail pieces, ZeRO-1 shards) gives the same bits.  The parameter update uses
// the fp32 m and v BEFORE rounding (ops/random.py holds the Python twin of both functions).
__device__ __forceinline__ uint32_t sr_bf16(float x, uint32_t r16) {
  const uint32_t b = __float_as_uint(x);
  const uint32_t u = b + r16;  // sign-magnitude bits: rounds away from zero with probability low16 / 65536
  // inf / NaN pass through; a finite value is never carried into exponent 0xFF
  const bool keep = (b & 0x7f800000u) == 0x7f800000u || (u & 0x7f800000u) == 0x7f800000u;
  return (keep ? b : u) >> 16;
}

__device__ __forceinline__ uint32_t philox_word(const uint4 r, int w) {
  return w == 0 ? r.x : (w == 1 ? r.y : (w == 2 ? r.z : r.w));
}

template <bool DEV>
__global__ __launch_bounds__(256) void adamw_bf16state_kernel(
    const Chunk* __restrict__ chunks, int nchunks, float* __restrict__ p, const float* __restrict__ g,
    bf16_t* __restrict__ m, bf16_t* __restrict__ v, bf16_t* __restrict__ shadow, float lr, float b1, float b2,
    float eps, float wd, float bc1, float bc2_sqrt, float grad_scale, const int* skip,
    const float* __restrict__ clip, uint64_t seed, uint64_t step, const DevStep ds) {
  if (comm_poisoned(skip)) return;
  if constexpr (DEV) {
    const long long t = dev_step(ds, lr);
    dev_bias(ds, t, bc1, bc2_sqrt);
    step = (uint64_t)t;  // the Philox step word: the same number the host path passes
  }
  const float gs = clip ? grad_scale * clip[1] : grad_scale;
  const float step_size = lr / bc1;
  for (int ci = blockIdx.x; ci < nchunks; ci += gridDim.x) {
    const Chunk c = chunks[ci];
    const float decay = c.decay ? (1.f - lr * wd) : 1.f;
    // One definition of the element update for the vector and the scalar path, with the fused
    // multiply-adds written out and contraction off: left to the compiler, the two inlined
    // copies were contracted differently (b1*m + c*g has two fusions), and a chunk cut at an
    // odd offset changed the result in the last bit.  The fusions are the ones adamw_kernel's
    // vector path compiles to.
    auto upd = [&](float gv, float& pe, float& me, float& ve) {
#pragma clang fp contract(off)
      const float gr = gv * gs;
      me = fmaf(1.f - b1, gr, b1 * me);
      ve = fmaf(b2, ve, ((1.f - b2) * gr) * gr);
      const float denom = sqrtf(ve) / bc2_sqrt + eps;
      pe = fmaf(pe, decay, -(step_size * me / denom));
    };
    // four elements that share one Philox call (o is a multiple of 4): pp, mu, vu updated in place
    auto calc4 = [&](long long o, f32x4& pp, const f32x4 gg, uint2& mu, uint2& vu) {
      const uint4 r = Philox::gen(seed, step, (uint64_t)o >> 2);
      const uint32_t rw[4] = {r.x, r.y, r.z, r.w};
      const uint32_t mi[4] = {mu.x << 16, mu.x & 0xffff0000u, mu.y << 16, mu.y & 0xffff0000u};
      const uint32_t vi[4] = {vu.x << 16, vu.x & 0xffff0000u, vu.y << 16, vu.y & 0xffff0000u};
      uint32_t ms[4], vs[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = pp[e], me = __uint_as_float(mi[e]), ve = __uint_as_float(vi[e]);
        upd(gg[e], pe, me, ve);
        pp[e] = pe;
        ms[e] = sr_bf16(me, rw[e] & 0xffffu);
        vs[e] = sr_bf16(ve, rw[e] >> 16);
      }
      mu = make_uint2(ms[0] | (ms[1] << 16), ms[2] | (ms[3] << 16));
      vu = make_uint2(vs[0] | (vs[1] << 16), vs[2] | (vs[3] << 16));
    };
    // 16-B accesses of p and g, 8-B accesses of m, v and the shadow (16-B state accesses, 8
    // elements per lane and iteration, measured equal within 0.3 %: profiles/adamw_bf16_state.md).
    // One Philox call serves four elements that share e >> 2; chunks cut at an odd offset (a
    // deferred-tail piece) take the scalar path, which draws the same word per element.
    const bool vec = (c.start & 3) == 0 && (c.sstart & 3) == 0;
    for (int i = threadIdx.x * 4; i < c.len; i += 256 * 4) {
      const long long o = c.start + i, so = c.sstart + i;
      if (vec && i + 4 <= c.len) {
        f32x4 pp = *(f32x4*)(p + o);
        const f32x4 gg = *(const f32x4*)(g + o);
        uint2 mu = *(const uint2*)(m + so), vu = *(const uint2*)(v + so);
        calc4(o, pp, gg, mu, vu);
        *(f32x4*)(p + o) = pp;
        *(uint2*)(m + so) = mu;
        *(uint2*)(v + so) = vu;
        if (shadow) *(uint2*)(shadow + o) = make_uint2(pack_bf2(pp[0], pp[1]), pack_bf2(pp[2], pp[3]));
      } else {
        for (int e = 0; e < 4 && i + e < c.len; ++e) {
          const long long oe = o + e, se = so + e;
          const uint32_t w = philox_word(Philox::gen(seed, step, (uint64_t)oe >> 2), (int)(oe & 3));
          float pe = p[oe], me = bf2f(m[se]), ve = bf2f(v[se]);
          upd(g[oe], pe, me, ve);
          p[oe] = pe;
          m[se] = (bf16_t)sr_bf16(me, w & 0xffffu);
          v[se] = (bf16_t)sr_bf16(ve, w >> 16);
          if (shadow) shadow[oe] = f2bf(pe);
        }
      }
    }
  }
}

// torch SGD: d = g*s + wd*p ; buf = first ? d : mom*buf + (1-damp)*d ; d = nesterov ? d + mom*buf : buf
// p -= lr*d
template <bool DEV>
__global__ __launch_bounds__(256) void sgd_kernel(const Chunk* __restrict__ chunks, int nchunks,
                                                 float* __restrict__ p, const float* __restrict__ g,
                                                 float* __restrict__ buf, bf16_t* __restrict__ shadow,
                                                 float lr, float momentum, float dampening, float wd,
                                                 int nesterov, int first, float grad_scale, const int* skip,
                                                 const float* __restrict__ clip, const DevStep ds) {
  if (comm_poisoned(skip)) return;
  if constexpr (DEV) dev_step(ds, lr);
  const float gs = clip ? grad_scale * clip[1] : grad_scale;
  for (int ci = blockIdx.x; ci < nchunks; ci += gridDim.x) {
    const Chunk c = chunks[ci];
    const float w = c.decay ? wd : 0.f;
    // the fused multiply-adds written out and contraction off, as in the AdamW kernels: left to the
    // compiler, the vector copy became d = fma(gs, g, w p) and the scalar copy d = fma(w, p, gs g), so
    // with weight decay a chunk cut at an odd offset changed the last bit.  The fusions are the ones
    // the vector path compiled to.
    auto upd = [&](float gv, float& pe, float& b) {
#pragma clang fp contract(off)
      float d = fmaf(gs, gv, w * pe);
      if (momentum != 0.f) {
        b = first ? d : fmaf(momentum, b, (1.f - dampening) * d);
        d = nesterov ? fmaf(momentum, b, d) : b;
      }
      pe = fmaf(-lr, d, pe);
    };
    const bool vec = (c.start & 3) == 0 && (c.sstart & 3) == 0;
    // 4 elements per lane and iteration (16-B loads of p, g and the momentum buffer)
    for (int i = threadIdx.x * 4; i < c.len; i += 256 * 4) {
      const long long o = c.start + i, so = c.sstart + i;
      if (vec && i + 4 <= c.len) {
        f32x4 pp = *(f32x4*)(p + o);
        const f32x4 gg = *(const f32x4*)(g + o);
        f32x4 bb = (momentum != 0.f && !first) ? *(f32x4*)(buf + so) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float pe = pp[e], b = bb[e];
          upd(gg[e], pe, b);
          pp[e] = pe;
          bb[e] = b;
        }
        *(f32x4*)(p + o) = pp;
        if (momentum != 0.f) *(f32x4*)(buf + so) = bb;
        if (shadow) *(uint2*)(shadow + o) = make_uint2(pack_bf2(pp[0], pp[1]), pack_bf2(pp[2], pp[3]));
      } else {
        for (int e = 0; e < 4 && i + e < c.len; ++e) {
          const long long oe = o + e, se = so + e;
          float pe = p[oe], b = (momentum != 0.f && !first) ? buf[se] : 0.f;
          upd(g[oe], pe, b);
          if (momentum != 0.f) buf[se] = b;
          p[oe] = pe;
          if (shadow) shadow[oe] = f2bf(pe);
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void f32_to_bf16_kernel(const float* __restrict__ x, bf16_t* __restrict__ y,
                                                         long long n) {
  for (long long i = (blockIdx.x * 256LL + threadIdx.x) * 4; i < n; i += gridDim.x * 256LL * 4) {
    if (i + 4 <= n) {
      f32x4 v = *(const f32x4*)(x + i);
      *(uint2*)(y + i) = make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
    } else {
      for (long long e = i; e < n; ++e) y[e] = f2bf(x[e]);
    }
  }
}

// y[c][r] = bf16(x[r][c]) for a row-major fp32 [R][C] matrix: the K-major image of a weight for
// the products that read it transposed (ops/shadow.py shadow_t_of).  64x64 tiles through LDS
// (padded rows: conflict-free column reads), 16-B loads, 8-B stores.
__global__ __launch_bounds__(256) void f32_to_bf16_t_kernel(const float* __restrict__ x, bf16_t* __restrict__ y,
                                                           int R, int C) {
  __shared__ float t[64][65];
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rr = ty + 16 * i, r = r0 + rr, c = c0 + 4 * tx;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (r < R) {
      if (c + 4 <= C && (C & 3) == 0) {
        const f32x4 q = *(const f32x4*)(x + (long long)r * C + c);
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = c + e < C ? x[(long long)r * C + c + e] : 0.f;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) t[rr][4 * tx + e] = v[e];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int cc = ty + 16 * i, c = c0 + cc, r = r0 + 4 * tx;
    if (c >= C) continue;
    bf16_t* o = y + (long long)c * R + r;
    if (r + 4 <= R && (R & 3) == 0) {
      *(uint2*)o = make_uint2(pack_bf2(t[4 * tx][cc], t[4 * tx + 1][cc]), pack_bf2(t[4 * tx + 2][cc], t[4 * tx + 3][cc]));
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (r + e < R) o[e] = f2bf(t[4 * tx + e][cc]);
    }
  }
}

__global__ __launch_bounds__(256) void bf16_to_f32_kernel(const bf16_t* __restrict__ x, float* __restrict__ y,
                                                         long long n, float scale) {
  for (long long i = (blockIdx.x * 256LL + threadIdx.x) * 4; i < n; i += gridDim.x * 256LL * 4) {
    if (i + 4 <= n) {
      const uint2 u = *(const uint2*)(x + i);
      f32x4 v;
      v[0] = __uint_as_float(u.x << 16) * scale;
      v[1] = __uint_as_float(u.x & 0xffff0000u) * scale;
      v[2] = __uint_as_float(u.y << 16) * scale;
      v[3] = __uint_as_float(u.y & 0xffff0000u) * scale;
      *(f32x4*)(y + i) = v;
    } else {
      for (long long e = i; e < n; ++e) y[e] = bf2f(x[e]) * scale;
    }
  }
}

// ---- global gradient-norm clipping (optim/fused.py max_grad_norm) -------------------------
// Three small kernels produce clip[0] = total_norm, clip[1] = coef on the device; the update
// kernels above fold clip[1] into their gradient multiply, so clipping costs one extra read of
// the gradients, no write and no host sync.  No atomics: every sum has a fixed order, so the
// norm is bitwise reproducible for a fixed chunk table.
//
// All sums of squares are carried in fp64 (the square of an fp32 value is exact in fp64; the
// kernel stays memory-bound, CDNA's fp64 FMA is full rate) and rounded to fp32 once, at the
// norm.  With fp32 sums the norm depended on where the chunks are cut in its last bit, so a
// ZeRO-1 run (chunks cut at shard boundaries) and a replicated run got clip coefficients one
// ulp apart - which bf16 compute amplifies to visibly different parameters within a few
// steps.  fp64 sums of two different cuts agree to ~1e-15, so the fp32 norm is the same
// unless the exact value lies that close to an fp32 rounding boundary.
//
// partial[ci] = sum of squares of chunk ci.  One chunk per block iteration; the value depends
// only on the chunk's (start, len) and the data (the block is always 256 lanes), not on the
// grid.  16-B loads when `start` is 4-aligned (always, except chunks cut at an odd offset),
// four independent loads in flight per lane, each into its own accumulator.
__device__ __forceinline__ double sqd(float x) { return (double)x * (double)x; }
__device__ __forceinline__ double sq4(const f32x4 x) { return (sqd(x[0]) + sqd(x[1])) + (sqd(x[2]) + sqd(x[3])); }

// block_sum (common.h) for fp64: a fixed-order butterfly inside each wave, then the waves' sums
// in wave order.  `red` must hold NT/64 doubles.
template <int NT>
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  if (l == 0) red[w] = v;
  __syncthreads();
  double r = 0.0;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) r += red[i];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void gradnorm_partial_kernel(const Chunk* __restrict__ chunks, int nchunks,
                                                              const float* __restrict__ g,
                                                              double* __restrict__ partial) {
  __shared__ double red[4];
  for (int ci = blockIdx.x; ci < nchunks; ci += gridDim.x) {
    const Chunk c = chunks[ci];
    const float* gc = g + c.start;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if ((c.start & 3) == 0) {
      const f32x4* gv = (const f32x4*)gc;
      const int nv = c.len >> 2;
      int j = threadIdx.x;
      for (; j + 768 < nv; j += 1024) {
        const f32x4 x0 = gv[j], x1 = gv[j + 256], x2 = gv[j + 512], x3 = gv[j + 768];
        a0 += sq4(x0);
        a1 += sq4(x1);
        a2 += sq4(x2);
        a3 += sq4(x3);
      }
      for (; j < nv; j += 256) a0 += sq4(gv[j]);
      // scalar tail: the last len % 4 elements
      const int i = (nv << 2) + threadIdx.x;
      if (i < c.len) a1 += sqd(gc[i]);
    } else {
      int i = threadIdx.x;
      for (; i + 768 < c.len; i += 1024) {
        const float x0 = gc[i], x1 = gc[i + 256], x2 = gc[i + 512], x3 = gc[i + 768];
        a0 += sqd(x0);
        a1 += sqd(x1);
        a2 += sqd(x2);
        a3 += sqd(x3);
      }
      for (; i < c.len; i += 256) a0 += sqd(gc[i]);
    }
    const double s = block_sum_f64<256>((a0 + a1) + (a2 + a3), red);
    if (threadIdx.x == 0) partial[ci] = s;
  }
}

// out[0] = total_norm = grad_scale * sqrt(sum), out[1] = coef = min(1, max_norm / (total_norm + 1e-6))
// (torch.nn.utils.clip_grad_norm_; a NaN norm gives a NaN coefficient, as torch's clamp does)
__device__ __forceinline__ void write_clip(double sum, float grad_scale, float max_norm, float* out) {
  const float total = grad_scale * (float)sqrt(sum);
  const float c = max_norm / (total + 1e-6f);
  out[0] = total;
  out[1] = c < 1.f ? c : (c != c ? c : 1.f);
}

// One block: lane t sums partial[t], partial[t + 1024], ... serially, then a fixed-order block
// reduction.  local != nullptr (ZeRO-1): only the local sum is written - the ranks' sums are
// all-gathered and combined by gradnorm_combine_kernel.
__global__ __launch_bounds__(1024) void gradnorm_finalize_kernel(const double* __restrict__ partial, int n,
                                                                float grad_scale, float max_norm,
                                                                float* __restrict__ out, double* __restrict__ local) {
  __shared__ double red[16];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) s += partial[i];
  s = block_sum_f64<1024>(s, red);
  if (threadIdx.x == 0) {
    if (local != nullptr)
      local[0] = s;
    else
      write_clip(s, grad_scale, max_norm, out);
  }
}

// ZeRO-1: the ranks' local sums (all-gathered: every rank holds the same `world` doubles) are
// added in rank order, so every rank computes the same bits.
__global__ void gradnorm_combine_kernel(const double* __restrict__ sums, int world, float grad_scale, float max_norm,
                                        float* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s = 0.0;
  for (int r = 0; r < world; ++r) s += sums[r];
  write_clip(s, grad_scale, max_norm, out);
}

}  // namespace rtdc

using namespace rtdc;

static inline int grid_for(int nchunks) { return nchunks < 4096 ? nchunks : 4096; }

// One update launch over a chunk table: `rest` are the kernel's parameters after (chunks, nchunks,
// p, g).  An empty table launches nothing; device tables that cannot be indexed are refused (1).
template <typename... KP, typename... A>
static int launch_update(void (*kernel)(KP...), const OptimArgs& o, bool bc_table, hipStream_t st, A... rest) {
  if (o.nchunks <= 0) return 0;
  const DevStep& ds = o.ds;
  if (ds.count != nullptr && (ds.lr == nullptr || ds.L < 1 || (bc_table && (ds.bc == nullptr || ds.Lbc < 1)))) return 1;
  hipLaunchKernelGGL(kernel, dim3(grid_for(o.nchunks)), dim3(256), 0, st, (const Chunk*)o.chunks, o.nchunks, o.p, o.g,
                     rest...);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

// a->ds.count != nullptr (capturable): lr, the bias corrections and the step number - also the
// bf16-state kernel's Philox step word - come from the device tables, not from a->lr / bc1 / bc2_sqrt / step
extern "C" int rtdc_adamw(const AdamwArgs* a, hipStream_t st) {
  const bool dev = a->ds.count != nullptr;
  bf16_t* shadow = (bf16_t*)a->shadow;
  if (a->state_bf16)
    return launch_update(dev ? adamw_bf16state_kernel<true> : adamw_bf16state_kernel<false>, *a, true, st,
                         (bf16_t*)a->m, (bf16_t*)a->v, shadow, a->lr, a->b1, a->b2, a->eps, a->wd, a->bc1, a->bc2_sqrt,
                         a->grad_scale, a->skip, a->clip, (uint64_t)a->seed, (uint64_t)a->step, a->ds);
  return launch_update(dev ? adamw_kernel<true> : adamw_kernel<false>, *a, true, st, (float*)a->m, (float*)a->v, shadow,
                       a->lr, a->b1, a->b2, a->eps, a->wd, a->bc1, a->bc2_sqrt, a->grad_scale, a->skip, a->clip, a->ds);
}

extern "C" int rtdc_sgd(const SgdArgs* a, hipStream_t st) {
  return launch_update(a->ds.count != nullptr ? sgd_kernel<true> : sgd_kernel<false>, *a, false, st, a->buf,
                       (bf16_t*)a->shadow, a->lr, a->momentum, a->dampening, a->wd, a->nesterov, a->first,
                       a->grad_scale, a->skip, a->clip, a->ds);
}

// count += 1 on stream st: the last launch of a capturable optimizer step
extern "C" int rtdc_optim_step_advance(long long* count, hipStream_t st) {
  if (count == nullptr) return 1;
  hipLaunchKernelGGL(optim_step_advance_kernel, dim3(1), dim3(64), 0, st, count);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

extern "C" int rtdc_f32_to_bf16(const float* x, void* y, long long n, hipStream_t st) {
  long long blocks = (n / 4 + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(f32_to_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, (bf16_t*)y, n);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

extern "C" int rtdc_f32_to_bf16_t(const float* x, void* y, int R, int C, hipStream_t st) {
  if (R <= 0 || C <= 0) return 0;
  hipLaunchKernelGGL(f32_to_bf16_t_kernel, dim3((unsigned)((C + 63) / 64), (unsigned)((R + 63) / 64)), dim3(256), 0,
                     st, x, (bf16_t*)y, R, C);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

// ---- batched bf16 transpose: dst[c][r] = src[r][c] for up to kTMaxJobs row-major [R][C]
// matrices in one launch (the K-major images of a model's weights, ops/shadow.py
// kmajor_refresh).  Block = one 64x64 tile of one job: 16-B loads of 8 rows x 8 columns per
// pass into an LDS tile padded by one 16-B chunk per row, 16-B stores of 8 consecutive output
// columns gathered from one LDS column.  Requires R % 8 == 0 and C % 8 == 0.
typedef __attribute__((ext_vector_type(4))) unsigned int tu32x4;
constexpr int kTMaxJobs = 96;
struct TJobs {
  const bf16_t* src[kTMaxJobs];
  bf16_t* dst[kTMaxJobs];
  int R[kTMaxJobs], C[kTMaxJobs];
  int start[kTMaxJobs + 1];  // first tile of each job (prefix sums)
  int n;
};

__global__ __launch_bounds__(256) void bf16_transpose_multi_kernel(const TJobs* __restrict__ jobs) {
  __shared__ __attribute__((aligned(16))) bf16_t t[64][72];
  const int b = blockIdx.x;
  int j = 0;
  {  // job of this tile: the last job whose start <= b (n <= 96: a short scalar scan)
    const int n = jobs->n;
    for (int i = 1; i < n; ++i) j = jobs->start[i] <= b ? i : j;
  }
  const int R = jobs->R[j], C = jobs->C[j];
  const int tiles_c = (C + 63) / 64;
  const int tile = b - jobs->start[j];
  const int r0 = (tile / tiles_c) * 64, c0 = (tile % tiles_c) * 64;
  const bf16_t* src = jobs->src[j];
  bf16_t* dst = jobs->dst[j];
  const int tid = threadIdx.x;
  // load: thread -> (row tid / 8 + 32 p, 8 columns at 8 * (tid % 8))
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int rr = tid / 8 + 32 * p, cc = 8 * (tid % 8);
    tu32x4 v = {0u, 0u, 0u, 0u};
    if (r0 + rr < R && c0 + cc < C) v = *(const tu32x4*)(src + (long long)(r0 + rr) * C + c0 + cc);
    *(tu32x4*)&t[rr][cc] = v;
  }
  __syncthreads();
  // store: thread -> (output row = input column tid / 8 + 32 p, 8 output columns = input rows)
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int oc = tid / 8 + 32 * p, orr = 8 * (tid % 8);
    if (c0 + oc >= C || r0 + orr >= R) continue;
    uint32_t w[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
      w[e] = (uint32_t)t[orr + 2 * e][oc] | ((uint32_t)t[orr + 2 * e + 1][oc] << 16);
    *(tu32x4*)(dst + (long long)(c0 + oc) * R + r0 + orr) = tu32x4{w[0], w[1], w[2], w[3]};
  }
}

extern "C" int rtdc_bf16_transpose_multi(const void* const* src, void* const* dst, const int* R, const int* C, int n,
                                         void* jobs_dev, hipStream_t st) {
  if (n <= 0) return 0;
  if (n > kTMaxJobs) return 1;
  TJobs h{};
  int tiles = 0;
  for (int i = 0; i < n; ++i) {
    if (R[i] % 8 || C[i] % 8) return 1;
    h.src[i] = (const bf16_t*)src[i];
    h.dst[i] = (bf16_t*)dst[i];
    h.R[i] = R[i];
    h.C[i] = C[i];
    h.start[i] = tiles;
    tiles += ((R[i] + 63) / 64) * ((C[i] + 63) / 64);
  }
  h.start[n] = tiles;
  h.n = n;
  // the table goes to device memory ahead of the kernel on the same stream (larger than the
  // kernel-argument segment)
  if (hipMemcpyAsync(jobs_dev, &h, sizeof(TJobs), hipMemcpyHostToDevice, st) != hipSuccess) return 2;
  hipLaunchKernelGGL(bf16_transpose_multi_kernel, dim3((unsigned)tiles), dim3(256), 0, st, (const TJobs*)jobs_dev);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

extern "C" int rtdc_bf16_transpose_jobs_bytes() { return (int)sizeof(TJobs); }

// memory-bound read pass: at most 256 CUs x 8 blocks, the rest by the grid-stride loop
static inline int grid_for_read(int nchunks) { return nchunks < 2048 ? nchunks : 2048; }

extern "C" int rtdc_gradnorm_partial(const void* chunks, int nchunks, const float* g, double* partial,
                                     hipStream_t st) {
  if (nchunks <= 0) return 0;
  hipLaunchKernelGGL(gradnorm_partial_kernel, dim3(grid_for_read(nchunks)), dim3(256), 0, st, (const Chunk*)chunks,
                     nchunks, g, partial);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

extern "C" int rtdc_gradnorm_finalize(const double* partial, int n, float grad_scale, float max_norm, float* out,
                                      double* local, hipStream_t st) {
  hipLaunchKernelGGL(gradnorm_finalize_kernel, dim3(1), dim3(1024), 0, st, partial, n, grad_scale, max_norm, out,
                     local);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

extern "C" int rtdc_gradnorm_combine(const double* sums, int world, float grad_scale, float max_norm, float* out,
                                     hipStream_t st) {
  hipLaunchKernelGGL(gradnorm_combine_kernel, dim3(1), dim3(64), 0, st, sums, world, grad_scale, max_norm, out);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

extern "C" int rtdc_bf16_to_f32(const void* x, float* y, long long n, float scale, hipStream_t st) {
  long long blocks = (n / 4 + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(bf16_to_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const bf16_t*)x, y, n, scale);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
