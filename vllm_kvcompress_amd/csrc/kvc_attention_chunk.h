// The kernels of the query-block ("chunk") attention, instantiated by two translation units: kvc_attention_chunk.hip
// (KVD = 0: caches in the query's dtype; the description of the two kernels is there) and kvc_attention_chunk_fp8.hip
// (KVD = 1 / 2: e4m3 / e5m2 caches; the description of the fp8 stage is there).  The compute loops, the LDS tile
// formats and the metric rule are one text for both; what depends on KVD is the global -> register -> LDS stage of
// the output pass, the K operand load of the metric pass and the v_scale factor of the last multiply.
#pragma once
#include "kvc_common.h"
#include "../../include/kvc_mi355x.h"

#include <math.h>

namespace kvc {
namespace {

typedef _Float16 cf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 cbf16x8 __attribute__((ext_vector_type(8)));
typedef float cf32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t cu32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t cu32x2 __attribute__((ext_vector_type(2)));

template <typename T> struct Mma16;
template <> struct Mma16<_Float16> {
  using V8 = cf16x8;
  static __device__ __forceinline__ cf32x4 mma(V8 a, V8 b, cf32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
};
template <> struct Mma16<__bf16> {
  using V8 = cbf16x8;
  static __device__ __forceinline__ cf32x4 mma(V8 a, V8 b, cf32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
};

// fp8 bytes -> T, exact (every e4m3 / e5m2 value is an fp16 and a bf16 value).  The scale operand of the conversion
// instructions contributes its exponent only: it is the literal 1.0 here, k_scale / v_scale never go through it.
template <typename T, bool E5M2>
__device__ __forceinline__ cu32x2 cvt8x4(uint32_t w) {          // bytes 0 .. 3 of w -> four T, order kept
  if constexpr (__is_same(T, _Float16) && E5M2) {                // e5m2 is the top byte of an fp16
    return cu32x2{((w & 0xFFu) << 8) | ((w & 0xFF00u) << 16), ((w >> 8) & 0xFF00u) | (w & 0xFF000000u)};
  } else if constexpr (__is_same(T, _Float16)) {
    return cu32x2{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, false)),
                  __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, true))};
  } else if constexpr (E5M2) {
    return cu32x2{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_bf8(w, 1.0f, false)),
                  __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_bf8(w, 1.0f, true))};
  } else {
    return cu32x2{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false)),
                  __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true))};
  }
}
template <typename T, bool E5M2>
__device__ __forceinline__ cu32x4 cvt8x8(uint32_t w0, uint32_t w1) {
  const cu32x2 a = cvt8x4<T, E5M2>(w0), b = cvt8x4<T, E5M2>(w1);
  return cu32x4{a[0], a[1], b[0], b[1]};
}

constexpr int CH_TQ = 16;          // query tokens per workgroup of the output pass (one MFMA tile per query head)
constexpr int CH_KT = 32;          // keys per LDS tile of the output pass
constexpr int CH_HG = 16;          // query heads per workgroup of the output pass
constexpr int CH_MW = 64;          // keys a wave of the metric pass keeps in registers
constexpr int CH_MP = 4 * CH_MW;   // keys per workgroup of the metric pass
constexpr int CH_RT = 4;           // query row tiles the metric pass stages per barrier
constexpr float CH_LOG2E = 1.4426950408889634f;

struct ChunkArgs {
  void* out;
  const void* q;
  const void* k_cache;
  const void* v_cache;
  const int32_t* block_tables;
  const int32_t* context_lens;
  const int32_t* kv_position;
  const int32_t* qsl;
  const int32_t* qpos;
  const int32_t* buf_len;
  float* metrics;
  float* stats;                    // [num_tokens, num_heads, 2]: row max (log2 domain), 1 / row sum
  int64_t q_stride, o_stride, kv_block_stride;
  float scale;                     // fp8 caches: scale * k_scale
  int32_t num_heads, num_kv_heads, qpk, head_groups, max_blocks, max_ctx, max_q, bs, bs_log2, slot_major;
  float v_scale;                   // fp8 caches only; last, so that the KVD = 0 kernels' argument offsets stay
};

// what both kernels know about their (sequence, KV head)
struct HeadView {
  int q0, nq, ctx;
  const int32_t* bt;
  __device__ __forceinline__ HeadView(const ChunkArgs& a, int s, int hk) {
    q0 = a.qsl[s];
    nq = min(a.qsl[s + 1] - q0, a.max_q);
    ctx = max(0, min(min(a.context_lens[s * a.num_kv_heads + hk], a.max_ctx), a.max_blocks * a.bs));
    bt = a.block_tables + ((int64_t)s * a.num_kv_heads + hk) * a.max_blocks;
  }
  // slots token j sees: i < limit(j)
  __device__ __forceinline__ int limit(int j) const { return max(0, ctx - (nq - 1 - j)); }
};

// The tree rule of the TREE kernel variants (kvc_attention_chunk_tree.hip): with base = ctx - nq (signed), a token
// with mask word W sees slot i < ctx iff e = i - base < 0 (the cached prefix) or bit e of W is set (e < nq: one of
// the new tokens).  tree_word clears the bits from nq up, so that a set bit alone says "a slot below ctx".
__device__ __forceinline__ uint64_t tree_word(const uint64_t* tree, int idx, int nq) {
  const uint64_t wd = tree[idx];
  return nq >= 64 ? wd : wd & ((1ull << (nq & 63)) - 1ull);
}
// The rule for 32 consecutive slots at once: bit b says whether a token with (cleared) word W sees the slot with
// e = e0 + b -- ones below e = 0, the word's bits from there, zeros from e = 64.  A lane's keys of a step lie within
// 20 slots, so one 64-bit shift serves all its weights.  Every shift amount is masked behind the compare that bounds
// it: never the operand's width or more.
__device__ __forceinline__ uint32_t tree_window(uint64_t word, int e0) {
  if (e0 <= -32) return 0xFFFFFFFFu;
  if (e0 < 0) return (uint32_t)(word << (-e0 & 31)) | ((1u << (-e0 & 31)) - 1u);      // -e0 = 1 .. 31
  return e0 < 64 ? (uint32_t)(word >> (e0 & 63)) : 0u;
}

// ---------------------------------------------------------------------------------- 1. output pass
template <typename T, int HD, int NT, int KVD>
__global__ __launch_bounds__(256) void chunk_out_kernel(ChunkArgs a) {
  using M = Mma16<T>;
  using V8 = typename M::V8;
  constexpr int PP = HD / 8;                  // 16-byte pieces per K row
  constexpr int PP_LOG2 = HD == 128 ? 4 : 3;
  constexpr int KS = HD / 32;                 // MFMA k-steps of QK^T
  constexpr int DT = HD / 16;                 // 16-dim output tiles of P.V
  constexpr int KU = CH_KT + 1;               // K tile: units per piece row
  constexpr int VS = CH_KT + 8;               // V tile: elements per dim row (80 bytes: rows stay 16-byte aligned)
  constexpr int CPT = CH_KT * PP / 256;       // 16-byte chunks per thread and tile, of K and of V
  constexpr bool E5M2 = KVD == 2;
  constexpr int U = HD / 16;                  // fp8: 16-byte chunks per K row (16 dims each)
  constexpr int U_LOG2 = HD == 128 ? 3 : 2;
  static_assert(HD == 64 || HD == 128, "chunk attention: head sizes 64 and 128");
  __shared__ __attribute__((aligned(16))) cu32x4 ktile[2][PP * KU];
  __shared__ __attribute__((aligned(16))) T vtile[2][HD * VS];

  const int s = blockIdx.z;
  const int hk = blockIdx.y / a.head_groups, hg = blockIdx.y % a.head_groups;
  const HeadView hv(a, s, hk);
  const int j0 = blockIdx.x * CH_TQ;
  if (j0 >= hv.nq) return;                                       // (uniform: before any barrier)
  const int lim_max = hv.limit(min(hv.nq, j0 + CH_TQ) - 1);     // the tile's last token sees the most
  const int lim_min = hv.limit(j0);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;
  const int nh = min(CH_HG, a.qpk - hg * CH_HG);                // query heads of this group
  const int h0 = hk * a.qpk + hg * CH_HG;
  const int tok = j0 + c;                                        // the lane's query token (MFMA column)
  const bool tok_ok = tok < hv.nq;
  const int lim = tok_ok ? hv.limit(tok) : 0;
  const T* kc = reinterpret_cast<const T*>(a.k_cache);
  const T* vc = reinterpret_cast<const T*>(a.v_cache);
  const int bs = a.bs, bsl = a.bs_log2;
  // fp8: a tile is CH_KT * U chunks of K and as many of V -- at HD 128 one of each per thread, at HD 64 waves 0, 1
  // take K and waves 2, 3 take V (wave-uniform: no divergence, and either half keeps its coalesced order)
  const uint8_t* kc8 = reinterpret_cast<const uint8_t*>(a.k_cache);
  const uint8_t* vc8 = reinterpret_cast<const uint8_t*>(a.v_cache);
  const int id8 = HD == 128 ? tid : (tid & 127);
  const bool k_mine = HD == 128 || tid < 128, v_mine = HD == 128 || tid >= 128;

  V8 bq[NT][KS];                                                 // Q operands: token c, dims 32 ks + 8 g ..
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int hi = w + 4 * nt;
    const T* qp = reinterpret_cast<const T*>(a.q) + (int64_t)(hv.q0 + tok) * a.q_stride + (int64_t)(h0 + hi) * HD + 8 * g;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      cu32x4 raw = {0u, 0u, 0u, 0u};
      if (tok_ok && hi < nh) raw = *reinterpret_cast<const cu32x4*>(qp + 32 * ks);
      bq[nt][ks] = __builtin_bit_cast(V8, raw);
    }
  }

  cu32x4 kreg[CPT], vreg[CPT];
  // global -> registers: keys k0 .. k0 + 31 of the head.  A block is read if its first key is visible (the block
  // exists then); V elements of keys nobody sees are zeroed (0 * garbage could be NaN), K needs no such care (masked logits)
  auto fetch = [&](int k0) {
    if constexpr (KVD != 0) {
      // raw bytes, the same chunk order in both layouts for K (chunk r of a block lies at byte 16 r)
      const int b = id8 >> (bsl + U_LOG2), r = id8 & ((U << bsl) - 1);       // block of the tile, chunk of the block
      const int kb = k0 + (b << bsl);
      kreg[0] = cu32x4{0u, 0u, 0u, 0u};
      vreg[0] = cu32x4{0u, 0u, 0u, 0u};
      if (k_mine && kb < lim_max)
        kreg[0] = *reinterpret_cast<const cu32x4*>(kc8 + (int64_t)hv.bt[kb >> bsl] * a.kv_block_stride + 16 * r);
      if (v_mine && !a.slot_major) {                             // [hd][bs]: chunk r = 16 keys of dim r / (bs / 16)
        const int key = kb + 16 * (r & ((bs >> 4) - 1));
        if (kb < lim_max && key < lim_max) {
          cu32x4 v = *reinterpret_cast<const cu32x4*>(vc8 + (int64_t)hv.bt[kb >> bsl] * a.kv_block_stride + 16 * r);
          if (key + 16 > lim_max) {                              // byte 0 is +0 in e4m3 and in e5m2
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int nb = lim_max - key - 4 * e;              // bytes of word e that belong to visible keys
              if (nb <= 0) v[e] = 0u;
              else if (nb < 4) v[e] &= (1u << (8 * nb)) - 1u;
            }
          }
          vreg[0] = v;
        }
      } else if (v_mine) {                                       // [bs][hd]: key fastest over the lanes (see park)
        const int key = k0 + (id8 & (CH_KT - 1)), u = id8 >> 5;
        if (key < lim_max)
          vreg[0] = *reinterpret_cast<const cu32x4*>(vc8 + (int64_t)hv.bt[key >> bsl] * a.kv_block_stride +
                                                     (int64_t)(key & (bs - 1)) * HD + 16 * u);
      }
      return;
    }
#pragma unroll
    for (int x = 0; x < CPT; ++x) {
      const int id = tid + 256 * x;
      const int b = id >> (bsl + PP_LOG2), r = id & ((PP << bsl) - 1);      // block of the tile, chunk of the block
      const int kb = k0 + (b << bsl);
      kreg[x] = cu32x4{0u, 0u, 0u, 0u};
      if (kb < lim_max) kreg[x] = *reinterpret_cast<const cu32x4*>(kc + (int64_t)hv.bt[kb >> bsl] * a.kv_block_stride + 8 * r);
      vreg[x] = cu32x4{0u, 0u, 0u, 0u};
      if (!a.slot_major) {                                       // [hd][bs]: chunk r = 8 keys of dim r / (bs / 8)
        const int key = kb + 8 * (r & ((bs >> 3) - 1));
        if (kb < lim_max && key < lim_max) {
          cu32x4 v = *reinterpret_cast<const cu32x4*>(vc + (int64_t)hv.bt[kb >> bsl] * a.kv_block_stride + 8 * r);
          if (key + 8 > lim_max) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              if (key + 2 * e >= lim_max) v[e] = 0u;
              else if (key + 2 * e + 1 >= lim_max) v[e] &= 0xFFFFu;
            }
          }
          vreg[x] = v;
        }
      } else {                                                   // [bs][hd]: key fastest over the lanes (see park)
        const int kt = id & (CH_KT - 1), p = id >> 5;
        const int key = k0 + kt;
        if (key < lim_max)
          vreg[x] = *reinterpret_cast<const cu32x4*>(vc + (int64_t)hv.bt[key >> bsl] * a.kv_block_stride +
                                                     (int64_t)(key & (bs - 1)) * HD + 8 * p);
      }
    }
  };
  auto park = [&](int buf) {
    if constexpr (KVD != 0) {
      // dequantised once per workgroup, on the way into the tiles the compute loop reads as T
      const int b = id8 >> (bsl + U_LOG2), r = id8 & ((U << bsl) - 1);
      if (k_mine) {                                              // 16 dims of one key: pieces 2 u and 2 u + 1
        int u, kt;
        if (!a.slot_major) { u = r >> bsl; kt = (b << bsl) + (r & (bs - 1)); }       // K [hd/16][bs][16]
        else { u = r & (U - 1); kt = (b << bsl) + (r >> U_LOG2); }                   // K [bs][hd]
        ktile[buf][(2 * u) * KU + kt] = cvt8x8<T, E5M2>(kreg[0][0], kreg[0][1]);
        ktile[buf][(2 * u + 1) * KU + kt] = cvt8x8<T, E5M2>(kreg[0][2], kreg[0][3]);
      }
      if (v_mine && !a.slot_major) {                             // 16 keys of one dim: two 16-byte row stores
        const int d = r >> (bsl - 4), k16 = (b << bsl) + 16 * (r & ((bs >> 4) - 1));
        cu32x4* row = reinterpret_cast<cu32x4*>(&vtile[buf][d * VS + k16]);
        row[0] = cvt8x8<T, E5M2>(vreg[0][0], vreg[0][1]);
        row[1] = cvt8x8<T, E5M2>(vreg[0][2], vreg[0][3]);
      } else if (v_mine) {                                       // 16 dims of one key: transposed, 2-byte stores
        const int vk = id8 & (CH_KT - 1), u = id8 >> 5;
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          const V8 v = __builtin_bit_cast(V8, cvt8x8<T, E5M2>(vreg[0][2 * hf], vreg[0][2 * hf + 1]));
#pragma unroll
          for (int e = 0; e < 8; ++e) vtile[buf][(16 * u + 8 * hf + e) * VS + vk] = v[e];
        }
      }
      return;
    }
#pragma unroll
    for (int x = 0; x < CPT; ++x) {
      const int id = tid + 256 * x;
      const int b = id >> (bsl + PP_LOG2), r = id & ((PP << bsl) - 1);
      int p, kt;
      if (!a.slot_major) { p = r >> bsl; kt = (b << bsl) + (r & (bs - 1)); }       // K [hd/8][bs][8]
      else { p = r & (PP - 1); kt = (b << bsl) + (r >> PP_LOG2); }                 // K [bs][hd]
      ktile[buf][p * KU + kt] = kreg[x];
      if (!a.slot_major) {
        const int d = r >> (bsl - 3), k8 = (b << bsl) + 8 * (r & ((bs >> 3) - 1));
        *reinterpret_cast<cu32x4*>(&vtile[buf][d * VS + k8]) = vreg[x];
      } else {
        const int vk = id & (CH_KT - 1), vp = id >> 5;
        const V8 v = __builtin_bit_cast(V8, vreg[x]);
#pragma unroll
        for (int e = 0; e < 8; ++e) vtile[buf][(8 * vp + e) * VS + vk] = v[e];
      }
    }
  };

  float m[NT], l[NT];
  cf32x4 O[NT][DT];                                              // O^T: dims 16 dt + 4 g + i of token c
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    m[nt] = -INFINITY; l[nt] = 0.0f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) O[nt][dt] = cf32x4{0.f, 0.f, 0.f, 0.f};
  }
  const float sc = a.scale * CH_LOG2E;
  const int ntiles = (lim_max + CH_KT - 1) / CH_KT;
  if (ntiles > 0) { fetch(0); park(0); }
  __syncthreads();
  for (int t = 0; t < ntiles; ++t) {
    const int k0 = t * CH_KT, buf = t & 1;
    const bool more = t + 1 < ntiles;
    if (more) fetch(k0 + CH_KT);
    if (w < nh) {
      V8 ak[2][KS], av[DT];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) ak[kt][ks] = __builtin_bit_cast(V8, ktile[buf][(4 * ks + g) * KU + 16 * kt + c]);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {                          // dim 16 dt + c, keys 4 g .. + 3 and 16 + 4 g .. + 3
        const T* row = &vtile[buf][(16 * dt + c) * VS + 4 * g];
        const cu32x2 lo = *reinterpret_cast<const cu32x2*>(row), hi = *reinterpret_cast<const cu32x2*>(row + 16);
        av[dt] = __builtin_bit_cast(V8, cu32x4{lo[0], lo[1], hi[0], hi[1]});
      }
      const bool masked = k0 + CH_KT > lim_min;                  // only the last nq slots (and the ragged end) need the mask
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        if (w + 4 * nt >= nh) continue;                          // (wave-uniform)
        cf32x4 sa[2] = {cf32x4{0.f, 0.f, 0.f, 0.f}, cf32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) sa[kt] = M::mma(ak[kt][ks], bq[nt][ks], sa[kt]);
        float tv[8], tmax = -INFINITY;
#pragma unroll
        for (int j = 0; j < 8; ++j) {                            // key k0 + 16 (j / 4) + 4 g + j % 4 of token c
          float t = sa[j >> 2][j & 3] * sc;
          if (masked && k0 + 16 * (j >> 2) + 4 * g + (j & 3) >= lim) t = -INFINITY;
          tv[j] = t;
          tmax = fmaxf(tmax, t);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float mn = fmaxf(m[nt], tmax);
        const float ms = mn == -INFINITY ? 0.0f : mn;            // (a row that has seen nothing yet: every weight 0)
        const float alpha = __builtin_amdgcn_exp2f(m[nt] - ms);
        float psum = 0.0f;
        V8 pb;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float p = __builtin_amdgcn_exp2f(tv[j] - ms);
          psum += p;
          pb[j] = (T)p;
        }
        psum += __shfl_xor(psum, 16, 64);
        psum += __shfl_xor(psum, 32, 64);
        l[nt] = l[nt] * alpha + psum;
        m[nt] = mn;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          O[nt][dt] *= alpha;
          O[nt][dt] = M::mma(av[dt], pb, O[nt][dt]);
        }
      }
    }
    if (more) park(buf ^ 1);
    __syncthreads();
  }
  if (!tok_ok) return;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int hi = w + 4 * nt;
    if (hi >= nh) continue;
    const float inv = l[nt] > 0.0f ? 1.0f / l[nt] : 0.0f;
    float fin = inv;                                             // fp8: v_scale goes into the last multiply (fp32)
    if constexpr (KVD != 0) fin = inv * a.v_scale;
    T* o = reinterpret_cast<T*>(a.out) + (int64_t)(hv.q0 + tok) * a.o_stride + (int64_t)(h0 + hi) * HD + 4 * g;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      typedef T T4 __attribute__((ext_vector_type(4)));
      T4 r;
#pragma unroll
      for (int i = 0; i < 4; ++i) r[i] = (T)(O[nt][dt][i] * fin);
      *reinterpret_cast<T4*>(o + 16 * dt) = r;
    }
    if (g == 0) {
      float* st = a.stats + ((int64_t)(hv.q0 + tok) * a.num_heads + h0 + hi) * 2;
      st[0] = l[nt] > 0.0f ? m[nt] : 0.0f;
      st[1] = inv;
    }
  }
}

// ---------------------------------------------------------------------------------- 2. metric pass
template <typename T, int HD, bool L2, int KVD>
__global__ __launch_bounds__(256) void chunk_metric_kernel(ChunkArgs a) {
  using M = Mma16<T>;
  using V8 = typename M::V8;
  constexpr int PP = HD / 8, KS = HD / 32, NKT = CH_MW / 16;
  constexpr int QU = 17;                                         // Q tile: 16-byte unit (piece p, token) at p * 17 + token
  __shared__ __attribute__((aligned(16))) cu32x4 qtile[2][CH_RT][PP * QU];

  const int s = blockIdx.z, hk = blockIdx.y;
  const HeadView hv(a, s, hk);
  const int kp0 = blockIdx.x * CH_MP;
  if (hv.nq <= 0 || kp0 >= hv.ctx) return;                       // (uniform: before any barrier)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;
  const int kw0 = kp0 + CH_MW * w;                               // the wave's first key
  const int bs = a.bs, bsl = a.bs_log2;
  const T* kc = reinterpret_cast<const T*>(a.k_cache);
  const int buflen = a.buf_len[s];

  V8 ak[NKT][KS];                                                // K operands: key kw0 + 16 kt + c, dims 32 ks + 8 g ..
  int kpos[NKT][4];                                              // positions of the keys of the lane's results
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    const int key = kw0 + 16 * kt + c;
    const int64_t blk = key < hv.ctx ? (int64_t)hv.bt[key >> bsl] * a.kv_block_stride : 0;
    const int ko = key & (bs - 1);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int p = 4 * ks + g;
      cu32x4 raw = {0u, 0u, 0u, 0u};
      if constexpr (KVD != 0) {                                  // 8 bytes: half of the 16-dim chunk (key, p / 2)
        cu32x2 raw8 = {0u, 0u};
        if (key < hv.ctx)
          raw8 = *reinterpret_cast<const cu32x2*>(reinterpret_cast<const uint8_t*>(a.k_cache) + blk +
                                                  (a.slot_major ? ko * HD + 8 * p : (((p >> 1) << bsl) + ko) * 16 + 8 * (p & 1)));
        raw = cvt8x8<T, KVD == 2>(raw8[0], raw8[1]);
      } else {
        if (key < hv.ctx) raw = *reinterpret_cast<const cu32x4*>(kc + blk + (a.slot_major ? ko * HD + 8 * p : ((p << bsl) + ko) * 8));
      }
      ak[kt][ks] = __builtin_bit_cast(V8, raw);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int kr = kw0 + 16 * kt + 4 * g + i;
      kpos[kt][i] = kr < hv.ctx ? a.kv_position[(int64_t)hv.bt[kr >> bsl] * bs + (kr & (bs - 1))] : 0x7FFFFFFF;
    }
  }

  // row tiles: rt = token tile * qpk + query head, from the first token that sees the partition's first key
  const int rt_begin = max(0, kp0 - hv.ctx + hv.nq) / 16 * a.qpk;
  const int rt_end = (hv.nq + 15) / 16 * a.qpk;
  cu32x4 qreg[CH_RT];
  auto fetch = [&](int rt0) {
    const int row = tid / PP, p = tid % PP;
#pragma unroll
    for (int x = 0; x < CH_RT; ++x) {
      const int rt = rt0 + x, tt = rt / a.qpk, hq = rt - tt * a.qpk;
      const int tok = 16 * tt + row;
      qreg[x] = cu32x4{0u, 0u, 0u, 0u};
      if (tid < 16 * PP && rt < rt_end && tok < hv.nq)
        qreg[x] = *reinterpret_cast<const cu32x4*>(reinterpret_cast<const T*>(a.q) + (int64_t)(hv.q0 + tok) * a.q_stride +
                                                   (int64_t)(hk * a.qpk + hq) * HD + 8 * p);
    }
  };
  auto park = [&](int buf) {
    const int row = tid / PP, p = tid % PP;
    if (tid < 16 * PP) {
#pragma unroll
      for (int x = 0; x < CH_RT; ++x) qtile[buf][x][p * QU + row] = qreg[x];
    }
  };

  float acc[NKT][4];
  uint32_t touched = 0u;                                         // bit 4 kt + i: some query passed both masks
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[kt][i] = 0.0f;
  const float sc = a.scale * CH_LOG2E;
  fetch(rt_begin);
  park(0);
  __syncthreads();
  int buf = 0;
  for (int rt0 = rt_begin; rt0 < rt_end; rt0 += CH_RT, buf ^= 1) {
    const bool more = rt0 + CH_RT < rt_end;
    if (more) fetch(rt0 + CH_RT);
    if (kw0 < hv.ctx) {
#pragma unroll
      for (int x = 0; x < CH_RT; ++x) {
        const int rt = rt0 + x, tt = rt / a.qpk, hq = rt - tt * a.qpk;
        // (wave-uniform) past the end, or not even the tile's last token sees the wave's first key
        if (rt >= rt_end || hv.limit(min(hv.nq, 16 * tt + 16) - 1) <= kw0) continue;
        const int tok = 16 * tt + c;
        const bool ok = tok < hv.nq;
        const int vis = ok ? hv.limit(tok) : 0;
        const int win = ok ? a.qpos[hv.q0 + tok] - buflen : (int)0x80000000;
        float rmax = 0.0f, rinv = 0.0f;
        if (ok) {
          const float* st = a.stats + ((int64_t)(hv.q0 + tok) * a.num_heads + hk * a.qpk + hq) * 2;
          rmax = st[0]; rinv = st[1];
        }
        V8 bq[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) bq[ks] = __builtin_bit_cast(V8, qtile[buf][x][(4 * ks + g) * QU + c]);
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
          cf32x4 sa = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) sa = M::mma(ak[kt][ks], bq[ks], sa);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const bool pass = kw0 + 16 * kt + 4 * g + i < vis && kpos[kt][i] <= win;
            const float p = pass ? __builtin_amdgcn_exp2f(sa[i] * sc - rmax) * rinv : 0.0f;
            if constexpr (L2) acc[kt][i] = __builtin_fmaf(p, p, acc[kt][i]);
            else acc[kt][i] += p;
            touched |= (pass ? 1u : 0u) << (4 * kt + i);
          }
        }
      }
    }
    if (more) park(buf ^ 1);
    __syncthreads();
  }
  if (kw0 >= hv.ctx) return;
  // sum over the 16 tokens held by the lanes of each group (a fixed butterfly: every lane ends with the same sum);
  // lane c of group g then owns key kw0 + 16 (c / 4) + 4 g + c % 4
#pragma unroll
  for (int d = 1; d < 16; d <<= 1) touched |= (uint32_t)__shfl_xor((int)touched, d, 64);
  float mine = 0.0f;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v = acc[kt][i];
#pragma unroll
      for (int d = 1; d < 16; d <<= 1) v += __shfl_xor(v, d, 64);
      if (c == 4 * kt + i) mine = v;
    }
  const int key = kw0 + 16 * (c >> 2) + 4 * g + (c & 3);
  if (key < hv.ctx && ((touched >> c) & 1u)) {
    float* dst = a.metrics + (int64_t)hv.bt[key >> bsl] * bs + (key & (bs - 1));
    *dst = *dst + mine;
  }
}

template <typename T, int HD, int KVD>
int launch_chunk(const ChunkArgs& a, int num_seqs, int use_l2, hipStream_t s) {
  const int nh = a.qpk < CH_HG ? a.qpk : CH_HG;
  const dim3 grid((a.max_q + CH_TQ - 1) / CH_TQ, a.num_kv_heads * a.head_groups, num_seqs);
  if (nh <= 4) hipLaunchKernelGGL((chunk_out_kernel<T, HD, 1, KVD>), grid, dim3(256), 0, s, a);
  else if (nh <= 8) hipLaunchKernelGGL((chunk_out_kernel<T, HD, 2, KVD>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((chunk_out_kernel<T, HD, 4, KVD>), grid, dim3(256), 0, s, a);
  if (a.metrics != nullptr) {
    const dim3 mgrid((a.max_ctx + CH_MP - 1) / CH_MP, a.num_kv_heads, num_seqs);
    if (use_l2) hipLaunchKernelGGL((chunk_metric_kernel<T, HD, true, KVD>), mgrid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((chunk_metric_kernel<T, HD, false, KVD>), mgrid, dim3(256), 0, s, a);
  }
  return check_launch("paged_attention_chunk");
}

// The checks of F5 that do not depend on the cache dtype (include/kvc_mi355x.h), then the kernel arguments.
// false: nothing is to be launched and *rc is the entry's result.  stride_mult: what kv_block_stride must be a
// multiple of (its unit is the cache element: 8 two-byte elements or 16 bytes -- 16-byte blocks either way).
inline bool chunk_prepare(const kvc_attention_chunk_params* p, int64_t stride_mult, ChunkArgs& a, int* rc) {
  auto refuse = [&](const std::string& msg) { *rc = fail_invalid(msg); return false; };
  if (p->alibi_slopes != nullptr) return refuse("paged_attention_chunk: ALiBi slopes are not supported");
  if (p->dtype != 0 && p->dtype != 1) return refuse("Unsupported data type of query");
  if (p->head_size != 64 && p->head_size != 128) return refuse("Unsupported head size: " + std::to_string(p->head_size));
  if (p->block_size != 16 && p->block_size != 32) return refuse("Unsupported block size: " + std::to_string(p->block_size));
  if (p->num_kv_heads < 1 || p->num_heads < 1 || p->num_heads % p->num_kv_heads != 0)
    return refuse("paged_attention_chunk: num_heads must be a multiple of num_kv_heads");
  if (p->block_layout != KVC_LAYOUT_REFERENCE && p->block_layout != KVC_LAYOUT_SLOT_MAJOR)
    return refuse("Unsupported block layout: " + std::to_string(p->block_layout));
  if (p->num_seqs <= 0 || p->num_tokens <= 0 || p->max_query_len <= 0) { *rc = KVC_OK; return false; }
  if ((reinterpret_cast<uintptr_t>(p->query) & 15) || (p->q_stride % 8) || (reinterpret_cast<uintptr_t>(p->out) & 7) ||
      (p->out_stride % 4))
    return refuse("paged_attention_chunk: query rows must be 16-byte aligned (output rows 8-byte)");
  if ((reinterpret_cast<uintptr_t>(p->key_cache) & 15) || (reinterpret_cast<uintptr_t>(p->value_cache) & 15) ||
      (p->kv_block_stride % stride_mult))
    return refuse("paged_attention_chunk: cache blocks must be 16-byte aligned");
  if (p->workspace == nullptr || (reinterpret_cast<uintptr_t>(p->workspace) & 7) ||
      p->workspace_bytes < kvc_paged_attention_chunk_workspace_bytes(p->num_tokens, p->num_heads))
    return refuse("paged_attention_chunk: workspace too small");
  a.out = p->out; a.q = p->query; a.k_cache = p->key_cache; a.v_cache = p->value_cache;
  a.block_tables = p->block_tables; a.context_lens = p->context_lens; a.kv_position = p->kv_position;
  a.qsl = p->query_start_loc; a.qpos = p->query_positions; a.buf_len = p->kv_metric_buffer_len;
  a.metrics = p->metrics; a.stats = reinterpret_cast<float*>(p->workspace);
  a.q_stride = p->q_stride; a.o_stride = p->out_stride; a.kv_block_stride = p->kv_block_stride;
  a.scale = p->scale; a.v_scale = 1.0f;
  a.num_heads = p->num_heads; a.num_kv_heads = p->num_kv_heads; a.qpk = p->num_heads / p->num_kv_heads;
  a.head_groups = (a.qpk + CH_HG - 1) / CH_HG;
  a.max_blocks = p->max_num_blocks_per_seq;
  a.max_ctx = p->max_context_len > 0 ? p->max_context_len : 0;
  a.max_q = p->max_query_len;
  a.bs = p->block_size; a.bs_log2 = p->block_size == 16 ? 4 : 5;
  a.slot_major = p->block_layout == KVC_LAYOUT_SLOT_MAJOR ? 1 : 0;
  if (p->num_seqs > 65535 || (int64_t)a.num_kv_heads * a.head_groups > 65535)
    return refuse("paged_attention_chunk: at most 65535 sequences and 65535 (KV head, head group) pairs per call");
  if (a.metrics != nullptr && a.max_ctx == 0) a.metrics = nullptr;       // nothing cached: nothing to add
  return true;
}

}  // namespace
}  // namespace kvc
