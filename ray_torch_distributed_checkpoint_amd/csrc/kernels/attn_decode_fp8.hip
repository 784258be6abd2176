// Decode attention on an FP8 (OCP e4m3) KV cache for gfx950, and the prefill's quantising fill.
//
// The cache of a layer is two tensors: q [B, Tmax, 2 Hkv Dh] e4m3 bytes in the layout of the bf16
// cache (K heads, then V heads) and scale [B, Tmax, 2 Hkv] fp32 in the same head order.  A run of
// Dh elements (one head of one token, k or v) is quantised as ops/fp8.py quantises a weight row:
//   scale = amax / 448 (a true fp32 division; 1.0 for an all-zero run), code = rne_e4m3(x / scale),
// so the cache viewed as [B Tmax 2 Hkv, Dh] is quant_fp8_rows_kernel's image of the bf16 cache in
// the same view, bit for bit.  K is quantised after RoPE.  2 Dh + 8 bytes per key and kv-head
// against the 4 Dh of the bf16 cache.
//
// kv_fill_fp8_kernel, one launch for all batch rows: Dh / 8 lanes share a head of a token of the
// packed qkv [B, T, (H + 2 Hkv) Dh], read in place with one 16-byte load each; the head maximum
// is a DPP group reduction, each lane divides, converts with v_cvt_pk_fp8_f32 and stores 8 bytes;
// lane 0 of the group stores the scale.  The grid runs over the (token, head) groups of the rows
// t < rows of all B batch rows; nothing else is written.
//
// decode_attn_fp8_kernel, grid (nsplit, Hkv, B), 256 threads: the contract of decode_attn_kernel
// (attn_decode.hip) - the same split ranges, the split that contains pos[b] owns the new token,
// the same in-order LDS slot merge, the same `part` layout, merged by rtdc_decode_merge; no
// atomics; launch parameters from (B, Hkv, Tmax) and the host's nsplit alone.  The work split is
// this kernel's own: a lane loads 16 bytes = 16 e4m3 values of a key row, so Dh / 16 lanes share
// a row (4 or 8), a wave holds 16 or 8 key slots and the block 64 or 32: twice the keys of the
// bf16 kernel on the same number of loads.  A thread has 4 keys of its slot in flight (K bytes,
// V bytes and the two scales of each, loaded by every lane of the group) and sends them through
// the softmax U at a time.  A lane holds 16 elements of q per head (two uint4 of bf16) and 16 of
// o.  K bytes are widened to bf16 exactly (v_cvt_scalef32_pk_bf16_fp8 at scale 1.0) into the
// v_dot2_f32_bf16 chains of the bf16 kernel; after the DPP group sum the score is multiplied by
// kscale * (scale * log2 e), formed once per key.  V bytes are widened to fp32
// (v_cvt_pk_f32_fp8); the key's v-scale is folded into the probability once per key and head
// (p * vscale) ahead of the fma chain, not once per element.
//
// U per G (all at 16 values per lane; no instantiation uses scratch - the compiler's resource
// table of the gfx950 build is in profiles/decode_fp8_kv.md): G = 1: 4, G <= 4: 2, else 1.
//
// The new token: q and k heads rotated as in the bf16 kernel (rope_kernel's fp32 formula, rounded
// to bf16), then the owning block quantises the k head and the v head from LDS by the formula
// above, stores the two runs of Dh bytes and the two scales at pos[b], and attends to the new key
// through code * scale like to any cached key: the output is a pure function of what the cache
// holds after the step.  Rows at or beyond pos[b], or below the window, are never loaded: their
// bytes and scales may be NaN.
#include "common.h"

namespace rtdc {

constexpr float kDec8Log2e = 1.4426950408889634f;
constexpr int kDec8Flight = 4;  // keys of a slot in flight
typedef __attribute__((ext_vector_type(2))) __bf16 dec8_bf16x2;
typedef __attribute__((ext_vector_type(2))) float dec8_f32x2;

__host__ __device__ constexpr int dec8_unroll(int G) { return G == 1 ? 4 : G <= 4 ? 2 : 1; }

struct DecodeFp8Args {
  const bf16_t* qkv;
  uint8_t* cq;
  float* cs;
  const int* pos;
  const float* cosb;
  const float* sinb;
  float* part;
  int Tmax, H, Hkv, window, nsplit, chunk;
  float scale;
};

// ---- the quantiser of one head run: LPG = Dh / 8 adjacent lanes, 8 bf16 values each
template <int LPG>
__device__ __forceinline__ float f8kv_group_max(float v) {
  v = fmaxf(v, dpp_f<0xB1>(v));   // quad_perm [1,0,3,2]
  v = fmaxf(v, dpp_f<0x4E>(v));   // quad_perm [2,3,0,1]
  v = fmaxf(v, dpp_f<0x141>(v));  // row_half_mirror: the other quad of the 8 lanes
  if (LPG == 16) v = fmaxf(v, dpp_f<0x140>(v));  // row_mirror: the other half of the 16
  return v;
}

// every lane of the group active; s: the run's scale, the same bits in every lane of the group
template <int LPG>
__device__ __forceinline__ uint2 f8kv_quant8(const uint4& x, float& s) {
  const uint32_t w[4] = {x.x, x.y, x.z, x.w};
  float v[8], amax = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = __uint_as_float(w[i] << 16);
    v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    amax = fmaxf(amax, fmaxf(fabsf(v[2 * i]), fabsf(v[2 * i + 1])));
  }
  amax = f8kv_group_max<LPG>(amax);
  s = amax > 0.f ? __fdiv_rn(amax, 448.f) : 1.f;
  uint32_t o[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int p = __builtin_amdgcn_cvt_pk_fp8_f32(__fdiv_rn(v[4 * i], s), __fdiv_rn(v[4 * i + 1], s), 0, false);
    p = __builtin_amdgcn_cvt_pk_fp8_f32(__fdiv_rn(v[4 * i + 2], s), __fdiv_rn(v[4 * i + 3], s), p, true);
    o[i] = (uint32_t)p;
  }
  return make_uint2(o[0], o[1]);
}

template <int DH>
__global__ __launch_bounds__(256) void kv_fill_fp8_kernel(const bf16_t* __restrict__ qkv, uint8_t* __restrict__ cq,
                                                          float* __restrict__ cs, int T, int Tmax, int H, int Hkv,
                                                          int rows, long long groups) {
  constexpr int LPG = DH / 8;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long grp = gid / LPG;
  const int c = (int)(gid % LPG);
  const bool ok = grp < groups;  // (whole groups: the lanes of a group are in or out together)
  uint4 x = make_uint4(0, 0, 0, 0);
  long long dst = 0;
  if (ok) {
    const int hd = (int)(grp % (2 * Hkv));
    const long long bt = grp / (2 * Hkv);
    const long long t = bt % rows, b = bt / rows;
    x = *(const uint4*)(qkv + ((b * T + t) * (H + 2 * Hkv) + H + hd) * DH + c * 8);
    dst = (b * Tmax + t) * (2 * Hkv) + hd;
  }
  float s;
  const uint2 code = f8kv_quant8<LPG>(x, s);
  if (ok) {
    *(uint2*)(cq + dst * DH + c * 8) = code;
    if (c == 0) cs[dst] = s;
  }
}

// ---- the decode step
__device__ __forceinline__ float dec8_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

__device__ __forceinline__ float dec8_dot2(uint32_t a, dec8_bf16x2 b, float c) {
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(dec8_bf16x2, a), b, c, false);
}

// 16 e4m3 bytes of a key row (element index ascending with the byte address) against 16 bf16 of q
__device__ __forceinline__ float dec8_dot16(const uint4* q, const uint4& k) {
  const uint32_t a[8] = {q[0].x, q[0].y, q[0].z, q[0].w, q[1].x, q[1].y, q[1].z, q[1].w};
  const uint32_t w[4] = {k.x, k.y, k.z, k.w};
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    s = dec8_dot2(a[2 * i], __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[i], 1.0f, false), s);
    s = dec8_dot2(a[2 * i + 1], __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[i], 1.0f, true), s);
  }
  return s;
}

__device__ __forceinline__ void dec8_unpack16(const uint4& x, float* v) {
  const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const dec8_f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
    const dec8_f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
    v[4 * i] = lo[0]; v[4 * i + 1] = lo[1];
    v[4 * i + 2] = hi[0]; v[4 * i + 3] = hi[1];
  }
}

// sum over the LPR (4 or 8) adjacent lanes that share a key row; every lane active
template <int LPR>
__device__ __forceinline__ float dec8_group_sum(float v) {
  v += dpp_f<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_f<0x4E>(v);   // quad_perm [2,3,0,1]
  if (LPR == 8) v += dpp_f<0x141>(v);  // row_half_mirror: the other quad of the 8 lanes
  return v;
}

// U keys of this thread's slot against the G query heads: one rescale per call.  Called by every
// lane of the block (the DPP sums need them).  ksc = kscale * scale * log2(e) and vs = vscale of
// each key; an invalid key has zero bytes and zero scales, scores -inf and its exponential is
// exactly 0.  A slot that has seen no valid key keeps m = -inf and is skipped.
template <int G, int LPR, int U>
__device__ __forceinline__ void dec8_step(const uint4 (*qv)[2], const uint4* kx, const uint4* vx, const float* ksc,
                                          const float* vs, const bool* valid, float* m, float* l, float (*o)[16]) {
  float vf[U][16];
#pragma unroll
  for (int j = 0; j < U; ++j) dec8_unpack16(vx[j], vf[j]);
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float s[U];
    float mn = m[g];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const float d = dec8_group_sum<LPR>(dec8_dot16(qv[g], kx[j])) * ksc[j];
      s[j] = valid[j] ? d : -INFINITY;
      mn = fmaxf(mn, s[j]);
    }
    if (mn > -INFINITY) {
      const float alpha = dec8_exp2(m[g] - mn);  // m = -inf: 0
      float pv[U], ps = 0.f;
#pragma unroll
      for (int j = 0; j < U; ++j) {
        const float p = dec8_exp2(s[j] - mn);
        ps += p;
        pv[j] = p * vs[j];
      }
      l[g] = fmaf(l[g], alpha, ps);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        float acc = o[g][e] * alpha;
#pragma unroll
        for (int j = 0; j < U; ++j) acc = fmaf(pv[j], vf[j][e], acc);
        o[g][e] = acc;
      }
      m[g] = mn;
    }
  }
}

template <int DH, int G>
__global__ __launch_bounds__(256) void decode_attn_fp8_kernel(DecodeFp8Args a) {
  constexpr int LPR = DH / 16, KPW = 64 / LPR, SLOTS = 4 * KPW, U = dec8_unroll(G), F = kDec8Flight;
  constexpr int HALF = DH / 2, LPG = DH / 8;
  __shared__ __attribute__((aligned(16))) bf16_t sq[G + 2][DH];  // rotated q heads, rotated k, v
  __shared__ __attribute__((aligned(16))) uint8_t snq[2][DH];    // the new k and v heads' codes
  __shared__ float sns[2];                                       // and their scales
  __shared__ __attribute__((aligned(16))) float so[SLOTS][DH];
  __shared__ float sml[SLOTS][2];

  const int split = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c16 = lane % LPR, slot = wave * KPW + lane / LPR;
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
  const long long pitch = 2LL * a.Hkv * DH, voff = (long long)a.Hkv * DH;  // (elements = bytes)
  uint8_t* crow = a.cq + (long long)b * a.Tmax * pitch + (long long)kvh * DH;  // + key * pitch (+ voff: v)
  float* srow = a.cs + (long long)b * a.Tmax * 2 * a.Hkv + kvh;               // + key * 2 Hkv (+ Hkv: v)
  // ---- the owner quantises the new k and v heads: wave 0, LPG lanes per head (the lanes beyond
  // the two heads repeat them and store nothing)
  if (own && wave == 0) {
    const int which = (lane / LPG) & 1, cc = lane % LPG;
    float s;
    const uint2 code = f8kv_quant8<LPG>(*(const uint4*)&sq[G + which][cc * 8], s);
    if (lane < 2 * LPG) {
      *(uint2*)&snq[which][cc * 8] = code;
      *(uint2*)(crow + p * pitch + which * voff + cc * 8) = code;
      if (cc == 0) {
        sns[which] = s;
        srow[(long long)p * 2 * a.Hkv + which * a.Hkv] = s;
      }
    }
  }
  __syncthreads();

  uint4 qv[G][2];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    qv[g][0] = *(const uint4*)&sq[g][c16 * 16];
    qv[g][1] = *(const uint4*)&sq[g][c16 * 16 + 8];
  }
  float m[G], l[G], o[G][16];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = -INFINITY;
    l[g] = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) o[g][e] = 0.f;
  }
  const float c = a.scale * kDec8Log2e;

  if (pos_ok) {
    const int lo = a.window > 0 ? max(0, p - a.window + 1) : 0;
    const int ka = max(lo, k_begin), kb = min(p, k_end);  // cached keys of this split: [ka, kb)
    for (int k0 = ka; k0 < kb; k0 += F * SLOTS) {
      uint4 kx[F], vx[F];
      float ksc[F], vs[F];
      bool valid[F];
#pragma unroll
      for (int j = 0; j < F; ++j) {
        const int key = k0 + j * SLOTS + slot;
        valid[j] = key < kb;
        kx[j] = make_uint4(0, 0, 0, 0);
        vx[j] = make_uint4(0, 0, 0, 0);
        ksc[j] = 0.f;
        vs[j] = 0.f;
        if (valid[j]) {
          const uint8_t* kp = crow + key * pitch + c16 * 16;
          const float* sp = srow + (long long)key * 2 * a.Hkv;
          kx[j] = *(const uint4*)kp;
          vx[j] = *(const uint4*)(kp + voff);
          ksc[j] = sp[0];
          vs[j] = sp[a.Hkv];
        }
      }
#pragma unroll
      for (int j = 0; j < F; ++j) ksc[j] *= c;
#pragma unroll
      for (int j = 0; j < F; j += U) dec8_step<G, LPR, U>(qv, kx + j, vx + j, ksc + j, vs + j, valid + j, m, l, o);
    }
    if (own) {  // the new token's own key, its codes and scales from LDS, in slot 0
      const uint4 kx = *(const uint4*)&snq[0][c16 * 16], vx = *(const uint4*)&snq[1][c16 * 16];
      const float ksc = sns[0] * c, vs = sns[1];
      const bool valid = slot == 0;
      dec8_step<G, LPR, 1>(qv, &kx, &vx, &ksc, &vs, &valid, m, l, o);
    }
  }

  // ---- merge the key slots in slot order, one query head at a time
  for (int g = 0; g < G; ++g) {
#pragma unroll
    for (int gg = 0; gg < G; ++gg) {  // (static register index)
      if (gg == g) {
#pragma unroll
        for (int e = 0; e < 16; e += 4)
          *(float4*)&so[slot][c16 * 16 + e] = make_float4(o[gg][e], o[gg][e + 1], o[gg][e + 2], o[gg][e + 3]);
        if (c16 == 0) {
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
            const float w = dec8_exp2(ms - M);
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

}  // namespace rtdc

using namespace rtdc;

extern "C" int rtdc_decode_merge(const float* part, void* out, int B, int H, int Dh, int nsplit, hipStream_t st);

template <int DH>
static void launch_decode_fp8(int G, dim3 grid, hipStream_t st, const DecodeFp8Args& a) {
#define RTDC_DEC8_CASE(g) \
  case g: hipLaunchKernelGGL((decode_attn_fp8_kernel<DH, g>), grid, dim3(256), 0, st, a); break;
  switch (G) {
    RTDC_DEC8_CASE(1) RTDC_DEC8_CASE(2) RTDC_DEC8_CASE(3) RTDC_DEC8_CASE(4)
    RTDC_DEC8_CASE(5) RTDC_DEC8_CASE(6) RTDC_DEC8_CASE(7) RTDC_DEC8_CASE(8)
  }
#undef RTDC_DEC8_CASE
}

// The refusals, split ranges and `part` of rtdc_decode_attn; cache_q [B, Tmax, 2 Hkv Dh] e4m3
// bytes, cache_scale [B, Tmax, 2 Hkv] fp32.
extern "C" int rtdc_decode_attn_fp8kv(const void* qkv_new, void* cache_q, float* cache_scale, const int* pos,
                                      const float* cosb, const float* sinb, void* out, float* part, int B, int Tmax,
                                      int H, int Hkv, int Dh, int window, int nsplit, float scale, hipStream_t st) {
  if (Dh != 64 && Dh != 128) return 1;
  if (B < 1 || Tmax < 64 || Tmax % 64 != 0 || Hkv < 1 || H % Hkv != 0 || H / Hkv > 8 || window < 0) return 1;
  if (nsplit < 1 || nsplit > Tmax / 64 || nsplit > 65535 || Hkv > 65535 || B > 65535) return 1;
  if ((cosb == nullptr) != (sinb == nullptr)) return 1;
  DecodeFp8Args a;
  a.qkv = (const bf16_t*)qkv_new;
  a.cq = (uint8_t*)cache_q;
  a.cs = cache_scale;
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
  if (Dh == 64) launch_decode_fp8<64>(H / Hkv, grid, st, a);
  else launch_decode_fp8<128>(H / Hkv, grid, st, a);
  if (hipGetLastError() != hipSuccess) return 2;
  return rtdc_decode_merge(part, out, B, H, Dh, nsplit, st);
}

// qkv [B, T, (H + 2 Hkv) Dh] bf16 -> rows t < rows of cache_q / cache_scale (Tmax rows per batch row)
extern "C" int rtdc_kv_fill_fp8(const void* qkv, void* cache_q, float* cache_scale, int B, int T, int Tmax, int H,
                                int Hkv, int Dh, int rows, hipStream_t st) {
  if (Dh != 64 && Dh != 128) return 1;
  if (B < 1 || T < 1 || Tmax < 1 || H < 1 || Hkv < 1 || rows < 0 || rows > T || rows > Tmax) return 1;
  if (rows == 0) return 0;
  const long long groups = (long long)B * rows * 2 * Hkv;
  const long long blocks = (groups * (Dh / 8) + 255) / 256;
  if (blocks > INT32_MAX) return 1;
  if (Dh == 64)
    hipLaunchKernelGGL(kv_fill_fp8_kernel<64>, dim3((unsigned)blocks), dim3(256), 0, st, (const bf16_t*)qkv,
                       (uint8_t*)cache_q, cache_scale, T, Tmax, H, Hkv, rows, groups);
  else
    hipLaunchKernelGGL(kv_fill_fp8_kernel<128>, dim3((unsigned)blocks), dim3(256), 0, st, (const bf16_t*)qkv,
                       (uint8_t*)cache_q, cache_scale, T, Tmax, H, Hkv, rows, groups);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
