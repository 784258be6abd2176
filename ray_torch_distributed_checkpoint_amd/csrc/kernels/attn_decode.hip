// Decode attention for gfx950: one new query token per batch row against a KV cache.
//
// qkv_new [B, (H + 2 Hkv) Dh] is the new token's packed row as the qkv GEMM wrote it (before
// RoPE); cache [B, Tmax, 2 Hkv Dh] holds the k|v tail of the earlier tokens' rows (K heads, then
// V heads); pos[b] (device int32) is the new token's index.  Row b attends to the keys
// lo .. pos[b] with lo = window ? max(0, pos[b] - window + 1) : 0; the keys below pos[b] come
// from the cache, key pos[b] is the new token itself, taken from qkv_new.
//
// decode_attn_kernel, grid (nsplit, Hkv, B), 256 threads: a block serves all G = H / Hkv query
// heads of its kv-head over the keys of its split, [split * chunk, (split + 1) * chunk) cut to
// [lo, pos[b]), so every K and V byte is read once per step.  Dh / 8 lanes share one key row
// (16 B each: a wave load covers 64 * 16 B of whole rows), a wave holds 64 / (Dh / 8) key
// slots and the block 4 times that; a thread walks the keys of its slot 4 at a time.  Scores
// are v_dot2_f32_bf16 chains reduced over the row's lanes by DPP; the online softmax is per key
// slot, fp32, log2 domain, the bare v_exp_f32; probabilities stay fp32.  At the end the slots
// are merged through LDS in slot order and (m, l, o[Dh]) per query head goes to `part`.
// The split that contains pos[b] owns the new token: it adds the key from registers and is the
// one block of its (b, kv-head) that stores the k|v row into cache[b, pos[b]]; no block reads
// that row.  Rows at or beyond pos[b], or below the window, are never loaded.
// With cos/sin tables the new q and k heads are rotated at table row pos[b] by rope_kernel's
// fp32 formula (llama_ops.hip) and rounded to bf16 where that kernel rounds.
//
// decode_merge_kernel, grid B * H, Dh threads: combines the nsplit partials in split order
// (an empty split, m = -inf, gets weight exactly 0 and its exponent is never formed) and writes
// out = o / l as bf16.  No atomics anywhere: the result is a pure function of the inputs and
// nsplit.  nsplit and chunk come from the host and do not depend on pos.
#include "common.h"

namespace rtdc {

constexpr float kDecLog2e = 1.4426950408889634f;
typedef __attribute__((ext_vector_type(2))) __bf16 dec_bf16x2;

struct DecodeArgs {
  const bf16_t* qkv;
  bf16_t* cache;
  const int* pos;
  const float* cosb;
  const float* sinb;
  float* part;
  int Tmax, H, Hkv, window, nsplit, chunk;
  float scale;
};

__device__ __forceinline__ float dec_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

__device__ __forceinline__ float dec_dot2(uint32_t a, uint32_t b, float c) {
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(dec_bf16x2, a), __builtin_bit_cast(dec_bf16x2, b), c, false);
}
__device__ __forceinline__ float dec_dot8(const uint4& a, const uint4& b) {
  float s = dec_dot2(a.x, b.x, 0.f);
  s = dec_dot2(a.y, b.y, s);
  s = dec_dot2(a.z, b.z, s);
  return dec_dot2(a.w, b.w, s);
}

// sum over the LPR (8 or 16) adjacent lanes that share a key row; every lane active
template <int LPR>
__device__ __forceinline__ float dec_group_sum(float v) {
  v += dpp_f<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_f<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_f<0x141>(v);  // row_half_mirror: the other quad of the 8 lanes
  if (LPR == 16) v += dpp_f<0x140>(v);  // row_mirror: the other half of the 16
  return v;
}

__device__ __forceinline__ void dec_unpack8(const uint4& x, float* v) {
  const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = __uint_as_float(w[i] << 16);
    v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}

// U keys of this thread's slot against the G query heads: one rescale per call.  Called by
// every lane of the block (the DPP sums need them); an invalid key scores -inf and its
// exponential is exactly 0.  A slot that has seen no valid key keeps m = -inf and is skipped,
// so -inf - -inf is never formed.
template <int G, int LPR, int U>
__device__ __forceinline__ void dec_step(const uint4* qv, const uint4* kx, const uint4* vx, const bool* valid,
                                         float c, float* m, float* l, float (*o)[8]) {
  float vf[U][8];
#pragma unroll
  for (int j = 0; j < U; ++j) dec_unpack8(vx[j], vf[j]);
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float s[U];
    float mn = m[g];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const float d = dec_group_sum<LPR>(dec_dot8(qv[g], kx[j])) * c;
      s[j] = valid[j] ? d : -INFINITY;
      mn = fmaxf(mn, s[j]);
    }
    if (mn > -INFINITY) {
      const float alpha = dec_exp2(m[g] - mn);  // m = -inf: 0
      float p[U], ps = 0.f;
#pragma unroll
      for (int j = 0; j < U; ++j) {
        p[j] = dec_exp2(s[j] - mn);
        ps += p[j];
      }
      l[g] = fmaf(l[g], alpha, ps);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float acc = o[g][e] * alpha;
#pragma unroll
        for (int j = 0; j < U; ++j) acc = fmaf(p[j], vf[j][e], acc);
        o[g][e] = acc;
      }
      m[g] = mn;
    }
  }
}

template <int DH, int G>
__global__ __launch_bounds__(256) void decode_attn_kernel(DecodeArgs a) {
  constexpr int LPR = DH / 8, KPW = 64 / LPR, SLOTS = 4 * KPW, U = 4, HALF = DH / 2;
  __shared__ __attribute__((aligned(16))) bf16_t sq[G + 2][DH];  // rotated q heads, rotated k, v
  __shared__ __attribute__((aligned(16))) float so[SLOTS][DH];
  __shared__ float sml[SLOTS][2];

  const int split = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c8 = lane % LPR, slot = wave * KPW + lane / LPR;
  const int p = a.pos[b];
  const bool pos_ok = p >= 0 && p < a.Tmax;  // (a position outside the cache: every split empty)
  const int W = (a.H + 2 * a.Hkv) * DH;
  const bf16_t* x = a.qkv + (long long)b * W;

  // ---- the new token: q heads of this group and the k head rotated into LDS, v copied
  if (pos_ok) {
    for (int w = tid; w < (G + 1) * HALF; w += 256) {
      const int hd = w / HALF, i = w - hd * HALF;
      const bf16_t* src = x + (long long)(hd < G ? kvh * G + hd : a.H + kvh) * DH;
      const float x1 = bf2f(src[i]), x2 = bf2f(src[i + HALF]);
      float o1 = x1, o2 = x2;
      if (a.cosb) {
        const float cs = a.cosb[(long long)p * HALF + i], sn = a.sinb[(long long)p * HALF + i];
        o1 = x1 * cs - x2 * sn;
        o2 = x2 * cs + x1 * sn;
      }
      sq[hd][i] = f2bf(o1);
      sq[hd][i + HALF] = f2bf(o2);
    }
    for (int w = tid; w < DH; w += 256) sq[G + 1][w] = x[(long long)(a.H + a.Hkv + kvh) * DH + w];
  }
  __syncthreads();

  const int k_begin = split * a.chunk, k_end = k_begin + a.chunk;
  const bool own = pos_ok && p >= k_begin && p < k_end;
  bf16_t* crow = a.cache + (long long)b * a.Tmax * 2 * a.Hkv * DH + (long long)kvh * DH;  // + key * 2 Hkv DH (+ Hkv DH: v)
  const long long pitch = 2LL * a.Hkv * DH, voff = (long long)a.Hkv * DH;
  if (own && tid < 2 * LPR) {
    const int which = tid / LPR, cc = tid - which * LPR;
    *(uint4*)(crow + p * pitch + which * voff + cc * 8) = *(const uint4*)&sq[G + which][cc * 8];
  }

  uint4 qv[G];
#pragma unroll
  for (int g = 0; g < G; ++g) qv[g] = *(const uint4*)&sq[g][c8 * 8];
  float m[G], l[G], o[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = -INFINITY;
    l[g] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[g][e] = 0.f;
  }
  const float c = a.scale * kDecLog2e;

  if (pos_ok) {
    const int lo = a.window > 0 ? max(0, p - a.window + 1) : 0;
    const int ka = max(lo, k_begin), kb = min(p, k_end);  // cached keys of this split: [ka, kb)
    for (int k0 = ka; k0 < kb; k0 += U * SLOTS) {
      uint4 kx[U], vx[U];
      bool valid[U];
#pragma unroll
      for (int j = 0; j < U; ++j) {
        const int key = k0 + j * SLOTS + slot;
        valid[j] = key < kb;
        kx[j] = make_uint4(0, 0, 0, 0);
        vx[j] = make_uint4(0, 0, 0, 0);
        if (valid[j]) {
          const bf16_t* kp = crow + key * pitch + c8 * 8;
          kx[j] = *(const uint4*)kp;
          vx[j] = *(const uint4*)(kp + voff);
        }
      }
      dec_step<G, LPR, U>(qv, kx, vx, valid, c, m, l, o);
    }
    if (own) {  // the new token's own key, from LDS, in slot 0
      const uint4 kx = *(const uint4*)&sq[G][c8 * 8], vx = *(const uint4*)&sq[G + 1][c8 * 8];
      const bool valid = slot == 0;
      dec_step<G, LPR, 1>(qv, &kx, &vx, &valid, c, m, l, o);
    }
  }

  // ---- merge the key slots in slot order, one query head at a time
  for (int g = 0; g < G; ++g) {
#pragma unroll
    for (int gg = 0; gg < G; ++gg) {  // (static register index)
      if (gg == g) {
        *(float4*)&so[slot][c8 * 8] = make_float4(o[gg][0], o[gg][1], o[gg][2], o[gg][3]);
        *(float4*)&so[slot][c8 * 8 + 4] = make_float4(o[gg][4], o[gg][5], o[gg][6], o[gg][7]);
        if (c8 == 0) {
          sml[slot][0] = m[gg];
          sml[slot][1] = l[gg];
        }
      }
    }
    __syncthreads();
    if (tid < DH) {
      float M = -INFINITY;
      for (int s = 0; s < SLOTS; ++s) M = fmaxf(M, sml[s][0]);
      float L = 0.f, O = 0.f;
      if (M > -INFINITY) {
        for (int s = 0; s < SLOTS; ++s) {
          const float ms = sml[s][0];
          if (ms > -INFINITY) {
            const float w = dec_exp2(ms - M);
            L = fmaf(w, sml[s][1], L);
            O = fmaf(w, so[s][tid], O);
          }
        }
      }
      float* pr = a.part + (((long long)b * a.H + kvh * G + g) * a.nsplit + split) * (DH + 2);
      if (tid == 0) {
        pr[0] = M;
        pr[1] = L;
      }
      pr[2 + tid] = O;
    }
    __syncthreads();
  }
}

template <int DH>
__global__ __launch_bounds__(DH) void decode_merge_kernel(const float* __restrict__ part, bf16_t* __restrict__ out,
                                                         int nsplit) {
  const float* pr = part + (long long)blockIdx.x * nsplit * (DH + 2);
  const int col = threadIdx.x;
  float M = -INFINITY;
  for (int s = 0; s < nsplit; ++s) M = fmaxf(M, pr[s * (DH + 2)]);
  float L = 0.f, O = 0.f;
  if (M > -INFINITY) {
    for (int s = 0; s < nsplit; ++s) {
      const float ms = pr[s * (DH + 2)];
      if (ms > -INFINITY) {  // an empty split: weight exactly 0, no exponent formed
        const float w = dec_exp2(ms - M);
        L = fmaf(w, pr[s * (DH + 2) + 1], L);
        O = fmaf(w, pr[s * (DH + 2) + 2 + col], O);
      }
    }
  }
  out[(long long)blockIdx.x * DH + col] = f2bf(L > 0.f ? O / L : 0.f);
}

}  // namespace rtdc

using namespace rtdc;

template <int DH>
static void launch_decode(int G, dim3 grid, hipStream_t st, const DecodeArgs& a) {
#define RTDC_DEC_CASE(g) \
  case g: hipLaunchKernelGGL((decode_attn_kernel<DH, g>), grid, dim3(256), 0, st, a); break;
  switch (G) {
    RTDC_DEC_CASE(1) RTDC_DEC_CASE(2) RTDC_DEC_CASE(3) RTDC_DEC_CASE(4)
    RTDC_DEC_CASE(5) RTDC_DEC_CASE(6) RTDC_DEC_CASE(7) RTDC_DEC_CASE(8)
  }
#undef RTDC_DEC_CASE
}

// part: B * H * nsplit * (Dh + 2) floats.  nsplit in 1 .. Tmax / 64; split s covers the keys
// [s * chunk, (s + 1) * chunk) with chunk = ceil(Tmax / nsplit) rounded up to a multiple of 64.
extern "C" int rtdc_decode_attn(const void* qkv_new, void* cache, const int* pos, const float* cosb, const float* sinb,
                                void* out, float* part, int B, int Tmax, int H, int Hkv, int Dh, int window,
                                int nsplit, float scale, hipStream_t st) {
  if (Dh != 64 && Dh != 128) return 1;
  if (B < 1 || Tmax < 64 || Tmax % 64 != 0 || Hkv < 1 || H % Hkv != 0 || H / Hkv > 8 || window < 0) return 1;
  if (nsplit < 1 || nsplit > Tmax / 64 || nsplit > 65535 || Hkv > 65535 || B > 65535) return 1;
  if ((cosb == nullptr) != (sinb == nullptr)) return 1;
  DecodeArgs a;
  a.qkv = (const bf16_t*)qkv_new;
  a.cache = (bf16_t*)cache;
  a.pos = pos;
  a.cosb = cosb;
  a.sinb = sinb;
  a.part = part;
  a.Tmax = Tmax;
  a.H = H;
  a.Hkv = Hkv;
  a.window = window;
  a.nsplit = nsplit;
  a.chunk = ((Tmax + nsplit - 1) / nsplit + 63) / 64 * 64;
  a.scale = scale;
  const dim3 grid(nsplit, Hkv, B);
  if (Dh == 64) launch_decode<64>(H / Hkv, grid, st, a);
  else launch_decode<128>(H / Hkv, grid, st, a);
  if (hipGetLastError() != hipSuccess) return 2;
  if (Dh == 64)
    hipLaunchKernelGGL(decode_merge_kernel<64>, dim3(B * H), dim3(64), 0, st, part, (bf16_t*)out, nsplit);
  else
    hipLaunchKernelGGL(decode_merge_kernel<128>, dim3(B * H), dim3(128), 0, st, part, (bf16_t*)out, nsplit);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
