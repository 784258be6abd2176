// Decode attention for gfx950: one new query token per batch row against a KV cache, bf16 or FP8
// (OCP e4m3), and the FP8 cache's quantising prefill fill.
//
// qkv_new [B, (H + 2 Hkv) Dh] is the new token's packed row as the qkv GEMM wrote it (before
// RoPE); cache [B, Tmax, 2 Hkv Dh] holds the k|v tail of the earlier tokens' rows (K heads, then
// V heads); pos[b] (device int32) is the new token's index.  Row b attends to the keys
// lo .. pos[b] with lo = window ? max(0, pos[b] - window + 1) : 0; the keys below pos[b] come
// from the cache, key pos[b] is the new token itself.
//
// The FP8 cache is two tensors: e4m3 bytes in the layout above and scale [B, Tmax, 2 Hkv] fp32 in
// the same head order.  A run of Dh elements (one head of one token, k or v) is quantised by fp8.h's
// formula, as ops/fp8.py quantises a weight row, so the cache viewed as [B Tmax 2 Hkv, Dh] is
// quant_fp8_rows_kernel's image of the bf16 cache in the same view, bit for bit.  K is quantised
// after RoPE.  2 Dh + 8 bytes per key and kv-head against the 4 Dh of the bf16 cache.
//
// decode_attn_kernel<KV, Dh, G>, grid (nsplit, Hkv, B), 256 threads: a block serves all G = H / Hkv
// query heads of its kv-head over the keys of its split, [split * chunk, (split + 1) * chunk) cut to
// [lo, pos[b]), so every K and V byte is read once per step.  A lane loads 16 bytes of a key row,
// KV::EPL elements (8 bf16 or 16 e4m3), so LPR = Dh / EPL lanes share a row, a wave holds 64 / LPR
// key slots and the block 4 times that; a thread has KV::F keys of its slot in flight and sends them
// through the softmax KV::unroll(G) at a time.  Scores are v_dot2_f32_bf16 chains (e4m3 K bytes are
// widened to bf16 exactly) reduced over the row's lanes by DPP; the online softmax is per key slot,
// fp32, log2 domain, the bare v_exp_f32; probabilities stay fp32.  With scales the score is
// multiplied by kscale * (scale * log2 e), formed once per key, and the key's v-scale is folded
// into the probability once per key and head (p * vscale) ahead of the fma chain.  At the end the
// slots are merged through LDS in slot order and (m, l, o[Dh]) per query head goes to `part`.
//
// The split that contains pos[b] owns the new token: its block is the one of its (b, kv-head) that
// stores the k|v row into cache[b, pos[b]] (no block reads that row), and it adds the new key in
// slot 0.  bf16: the row is copied and the key taken from LDS as rotated.  FP8: the block quantises
// the k head and the v head from LDS, stores the two runs of Dh bytes and the two scales, and attends
// to the new key through code * scale like to any cached key, so the output is a pure function of
// what the cache holds after the step.  Rows at or beyond pos[b], or below the window, are never
// loaded: they may hold NaN.  With cos/sin tables the new q and k heads are rotated at table row
// pos[b] by rope_kernel's fp32 formula (llama_ops.hip) and rounded to bf16 where that kernel rounds.
//
// The FP8 instantiations' registers (none uses scratch) are in profiles/decode_fp8_kv.md.
//
// decode_merge_kernel, grid B * H, Dh threads: combines the nsplit partials in split order
// (an empty split, m = -inf, gets weight exactly 0 and its exponent is never formed) and writes
// out = o / l as bf16.  No atomics anywhere: the result is a pure function of the inputs and
// nsplit.  nsplit and chunk come from the host and do not depend on pos.
//
// kv_fill_fp8_kernel, one launch for all batch rows: Dh / 8 lanes share a head of a token of the
// packed qkv [B, T, (H + 2 Hkv) Dh], read in place with one 16-byte load each; the head maximum
// is a DPP group reduction, each lane divides, converts and stores 8 bytes; lane 0 of the group
// stores the scale.  The grid runs over the (token, head) groups of the rows t < rows of all B
// batch rows; nothing else is written.
#include "common.h"
#include "fp8.h"

namespace rtdc {

constexpr float kDecLog2e = 1.4426950408889634f;
typedef __attribute__((ext_vector_type(2))) float dec_f32x2;

struct DecodeArgs {
  const bf16_t* qkv;
  void* cache;  // KV::elem [B, Tmax, 2 Hkv Dh]
  const int* pos;
  const float* cosb;
  const float* sinb;
  float* part;
  int Tmax, H, Hkv, window, nsplit, chunk;
  float scale;
  float* cache_scale;  // [B, Tmax, 2 Hkv]; null: a bf16 cache
};

__device__ __forceinline__ float dec_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

__device__ __forceinline__ float dec_dot2(uint32_t a, fp8_bf16x2 b, float c) {
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(fp8_bf16x2, a), b, c, false);
}

// reduction over the LPR (4, 8 or 16) adjacent lanes that share a row; every lane active
template <int LPR, typename OP>
__device__ __forceinline__ float dec_group_reduce(float v, OP op) {
  v = op(v, dpp_f<0xB1>(v));                   // quad_perm [1,0,3,2]
  v = op(v, dpp_f<0x4E>(v));                   // quad_perm [2,3,0,1]
  if (LPR >= 8) v = op(v, dpp_f<0x141>(v));    // row_half_mirror: the other quad of the 8 lanes
  if (LPR == 16) v = op(v, dpp_f<0x140>(v));   // row_mirror: the other half of the 16
  return v;
}

// ---- the quantiser of one head run: LPG = Dh / 8 adjacent lanes, 8 bf16 values each; every lane
// of the group active; s: the run's scale, the same bits in every lane of the group
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
  s = fp8_scale(dec_group_reduce<LPG>(amax, [](float a, float b) { return fmaxf(a, b); }));
  return make_uint2(fp8_pack4(v, s), fp8_pack4(v + 4, s));
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

// ---- what a cache format supplies to decode_attn_kernel.  elem: a cache element; EPL: the elements
// of a lane's 16 bytes of a key row; kScaled: two fp32 scales per key; F keys of a slot in flight,
// unroll(G) of them per softmax call; dot(): the lane's q fragment (EPL bf16) against its 16 K bytes;
// widen(): its 16 V bytes as EPL floats; store_new(): the owner's store of the new token's k and v
// heads (sq[G], sq[G + 1], rotated) at the cache row `dst` = key p, by the threads tid < 64.
struct DecNone {};

struct KvBf16 {
  typedef bf16_t elem;
  static constexpr int EPL = 8, F = 4;
  static constexpr bool kScaled = false;
  static constexpr int unroll(int) { return 4; }
  template <int DH> using NewCodes = DecNone;
  typedef DecNone NewScales;

  static __device__ __forceinline__ float dot(const uint4* q, const uint4& k) {
    float s = dec_dot2(q[0].x, __builtin_bit_cast(fp8_bf16x2, k.x), 0.f);
    s = dec_dot2(q[0].y, __builtin_bit_cast(fp8_bf16x2, k.y), s);
    s = dec_dot2(q[0].z, __builtin_bit_cast(fp8_bf16x2, k.z), s);
    return dec_dot2(q[0].w, __builtin_bit_cast(fp8_bf16x2, k.w), s);
  }
  static __device__ __forceinline__ void widen(const uint4& x, float* v) {
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = __uint_as_float(w[i] << 16);
      v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
  }
  // a copy
  template <int DH>
  static __device__ __forceinline__ void store_new(const bf16_t (*kv)[DH], bf16_t* dst, long long voff, float*, int,
                                                   int, DecNone&, DecNone&, int tid) {
    constexpr int LPG = DH / 8;
    if (tid < 2 * LPG) {
      const int which = tid / LPG, cc = tid - which * LPG;
      *(uint4*)(dst + which * voff + cc * 8) = *(const uint4*)&kv[which][cc * 8];
    }
  }
};

struct KvFp8 {
  typedef uint8_t elem;
  static constexpr int EPL = 16, F = 4;
  static constexpr bool kScaled = true;
  // (no instantiation uses scratch at these: profiles/decode_fp8_kv.md)
  static constexpr int unroll(int G) { return G == 1 ? 4 : G <= 4 ? 2 : 1; }
  template <int DH> using NewCodes = uint8_t[2][DH];  // the new k and v heads' codes in LDS
  typedef float NewScales[2];                         // and their scales

  // element index ascending with the byte address
  static __device__ __forceinline__ float dot(const uint4* q, const uint4& k) {
    const uint32_t a[8] = {q[0].x, q[0].y, q[0].z, q[0].w, q[1].x, q[1].y, q[1].z, q[1].w};
    const uint32_t w[4] = {k.x, k.y, k.z, k.w};
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      s = dec_dot2(a[2 * i], fp8_widen2<false>(w[i]), s);
      s = dec_dot2(a[2 * i + 1], fp8_widen2<true>(w[i]), s);
    }
    return s;
  }
  static __device__ __forceinline__ void widen(const uint4& x, float* v) {
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const dec_f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
      const dec_f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
      v[4 * i] = lo[0]; v[4 * i + 1] = lo[1];
      v[4 * i + 2] = hi[0]; v[4 * i + 3] = hi[1];
    }
  }
  // quantise, then store codes and scales to the cache and to LDS: wave 0, LPG lanes per head (the
  // lanes beyond the two heads repeat them and store nothing)
  template <int DH>
  static __device__ __forceinline__ void store_new(const bf16_t (*kv)[DH], uint8_t* dst, long long voff, float* srow,
                                                   int p, int Hkv, uint8_t (&snq)[2][DH], float (&sns)[2], int tid) {
    constexpr int LPG = DH / 8;
    const int which = (tid / LPG) & 1, cc = tid % LPG;
    float s;
    const uint2 code = f8kv_quant8<LPG>(*(const uint4*)&kv[which][cc * 8], s);
    if (tid < 2 * LPG) {
      *(uint2*)&snq[which][cc * 8] = code;
      *(uint2*)(dst + which * voff + cc * 8) = code;
      if (cc == 0) {
        sns[which] = s;
        srow[(long long)p * 2 * Hkv + which * Hkv] = s;
      }
    }
  }
};

// U keys of this thread's slot against the G query heads: one rescale per call.  Called by
// every lane of the block (the DPP sums need them).  With scales, ksc = kscale * scale * log2(e)
// and vs = vscale of each key; without, c = scale * log2(e).  An invalid key (zero bytes, zero
// scales) scores -inf and its exponential is exactly 0.  A slot that has seen no valid key keeps
// m = -inf and is skipped, so -inf - -inf is never formed.
template <typename KV, int G, int LPR, int U>
__device__ __forceinline__ void dec_step(const uint4 (*qv)[KV::EPL / 8], const uint4* kx, const uint4* vx,
                                         const float* ksc, const float* vs, const bool* valid, float c, float* m,
                                         float* l, float (*o)[KV::EPL]) {
  float vf[U][KV::EPL];
#pragma unroll
  for (int j = 0; j < U; ++j) KV::widen(vx[j], vf[j]);
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float s[U];
    float mn = m[g];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      float cj = c;
      if constexpr (KV::kScaled) cj = ksc[j];
      const float d = dec_group_reduce<LPR>(KV::dot(qv[g], kx[j]), [](float a, float b) { return a + b; }) * cj;
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
        if constexpr (KV::kScaled) p[j] = p[j] * vs[j];
      }
      l[g] = fmaf(l[g], alpha, ps);
#pragma unroll
      for (int e = 0; e < KV::EPL; ++e) {
        float acc = o[g][e] * alpha;
#pragma unroll
        for (int j = 0; j < U; ++j) acc = fmaf(p[j], vf[j][e], acc);
        o[g][e] = acc;
      }
      m[g] = mn;
    }
  }
}

template <typename KV, int DH, int G>
__global__ __launch_bounds__(256) void decode_attn_kernel(DecodeArgs a) {
  typedef typename KV::elem elem;
  constexpr int EPL = KV::EPL, LPR = DH / EPL, KPW = 64 / LPR, SLOTS = 4 * KPW, HALF = DH / 2;
  constexpr int F = KV::F, U = KV::unroll(G);
  __shared__ __attribute__((aligned(16))) bf16_t sq[G + 2][DH];  // rotated q heads, rotated k, v
  // the owner's quantised new k and v heads: only a cache with scales has them (else empty, unused)
  __shared__ __attribute__((aligned(16))) typename KV::template NewCodes<DH> snq;
  __shared__ typename KV::NewScales sns;
  __shared__ __attribute__((aligned(16))) float so[SLOTS][DH];
  __shared__ float sml[SLOTS][2];

  const int split = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ce = lane % LPR, slot = wave * KPW + lane / LPR;
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
  elem* crow = (elem*)a.cache + (long long)b * a.Tmax * 2 * a.Hkv * DH + (long long)kvh * DH;  // + key * pitch (+ voff: v)
  const long long pitch = 2LL * a.Hkv * DH, voff = (long long)a.Hkv * DH;                      // (elements)
  float* srow = nullptr;
  if constexpr (KV::kScaled) srow = a.cache_scale + (long long)b * a.Tmax * 2 * a.Hkv + kvh;  // + key * 2 Hkv (+ Hkv: v)
  if (own && wave == 0)
    KV::template store_new<DH>(sq + G, crow + p * pitch, voff, srow, p, a.Hkv, snq, sns, lane);
  if constexpr (KV::kScaled) __syncthreads();  // (the owner reads its codes back from LDS)

  uint4 qv[G][EPL / 8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
#pragma unroll
    for (int i = 0; i < EPL / 8; ++i) qv[g][i] = *(const uint4*)&sq[g][ce * EPL + 8 * i];
  }
  float m[G], l[G], o[G][EPL];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = -INFINITY;
    l[g] = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e) o[g][e] = 0.f;
  }
  const float c = a.scale * kDecLog2e;

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
          const elem* kp = crow + key * pitch + ce * EPL;
          kx[j] = *(const uint4*)kp;
          vx[j] = *(const uint4*)(kp + voff);
          if constexpr (KV::kScaled) {
            const float* sp = srow + (long long)key * 2 * a.Hkv;
            ksc[j] = sp[0];
            vs[j] = sp[a.Hkv];
          }
        }
      }
      if constexpr (KV::kScaled) {
#pragma unroll
        for (int j = 0; j < F; ++j) ksc[j] *= c;
      }
#pragma unroll
      for (int j = 0; j < F; j += U)
        dec_step<KV, G, LPR, U>(qv, kx + j, vx + j, ksc + j, vs + j, valid + j, c, m, l, o);
    }
    if (own) {  // the new token's own key in slot 0: as rotated, or its codes and scales, from LDS
      const elem* nk;
      float ksc = 0.f, vs = 0.f;
      if constexpr (KV::kScaled) {
        nk = &snq[0][0];
        ksc = sns[0] * c;
        vs = sns[1];
      } else {
        nk = &sq[G][0];
      }
      const uint4 kx = *(const uint4*)(nk + ce * EPL), vx = *(const uint4*)(nk + DH + ce * EPL);
      const bool valid = slot == 0;
      dec_step<KV, G, LPR, 1>(qv, &kx, &vx, &ksc, &vs, &valid, c, m, l, o);
    }
  }

  // ---- merge the key slots in slot order, one query head at a time
  for (int g = 0; g < G; ++g) {
#pragma unroll
    for (int gg = 0; gg < G; ++gg) {  // (static register index)
      if (gg == g) {
#pragma unroll
        for (int e = 0; e < EPL; e += 4)
          *(float4*)&so[slot][ce * EPL + e] = make_float4(o[gg][e], o[gg][e + 1], o[gg][e + 2], o[gg][e + 3]);
        if (ce == 0) {
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

template <typename KV, int DH>
static void launch_decode(int G, dim3 grid, hipStream_t st, const DecodeArgs& a) {
#define RTDC_DEC_CASE(g) \
  case g: hipLaunchKernelGGL((decode_attn_kernel<KV, DH, g>), grid, dim3(256), 0, st, a); break;
  switch (G) {
    RTDC_DEC_CASE(1) RTDC_DEC_CASE(2) RTDC_DEC_CASE(3) RTDC_DEC_CASE(4)
    RTDC_DEC_CASE(5) RTDC_DEC_CASE(6) RTDC_DEC_CASE(7) RTDC_DEC_CASE(8)
  }
#undef RTDC_DEC_CASE
}

template <int DH>
static int launch_decode_steps(const DecodeArgs& a, bf16_t* out, int B, hipStream_t st) {
  const dim3 grid(a.nsplit, a.Hkv, B);
  if (a.cache_scale) launch_decode<KvFp8, DH>(a.H / a.Hkv, grid, st, a);
  else launch_decode<KvBf16, DH>(a.H / a.Hkv, grid, st, a);
  if (hipGetLastError() != hipSuccess) return 2;
  hipLaunchKernelGGL(decode_merge_kernel<DH>, dim3(B * a.H), dim3(DH), 0, st, a.part, out, a.nsplit);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

// cache_scale null: cache is bf16 [B, Tmax, 2 Hkv Dh]; else cache holds e4m3 bytes in that layout
// and cache_scale [B, Tmax, 2 Hkv] fp32.  part: B * H * nsplit * (Dh + 2) floats.  nsplit in
// 1 .. Tmax / 64; split s covers the keys [s * chunk, (s + 1) * chunk) with chunk =
// ceil(Tmax / nsplit) rounded up to a multiple of 64.
extern "C" int rtdc_decode_attn(const void* qkv_new, void* cache, float* cache_scale, const int* pos, const float* cosb,
                                const float* sinb, void* out, float* part, int B, int Tmax, int H, int Hkv, int Dh,
                                int window, int nsplit, float scale, hipStream_t st) {
  if (Dh != 64 && Dh != 128) return 1;
  if (B < 1 || Tmax < 64 || Tmax % 64 != 0 || Hkv < 1 || H % Hkv != 0 || H / Hkv > 8 || window < 0) return 1;
  if (nsplit < 1 || nsplit > Tmax / 64 || nsplit > 65535 || Hkv > 65535 || B > 65535) return 1;
  if ((cosb == nullptr) != (sinb == nullptr)) return 1;
  DecodeArgs a;
  a.qkv = (const bf16_t*)qkv_new;
  a.cache = cache;
  a.cache_scale = cache_scale;
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
  return Dh == 64 ? launch_decode_steps<64>(a, (bf16_t*)out, B, st) : launch_decode_steps<128>(a, (bf16_t*)out, B, st);
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
