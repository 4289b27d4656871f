// The kernels of the "split" schedule of the query-block attention, instantiated by two translation units:
// kvc_attention_chunk_split.hip (KVD = 0: caches in the query's dtype; the description of the schedule, the partition
// rule and the C entry are there) and kvc_attention_chunk_split_fp8.hip (KVD = 1 / 2: e4m3 / e5m2 caches).  The data
// path of a workgroup is the tile kernel's (kvc_attention_chunk.h: the same LDS tile formats, the same MFMA products,
// the same fp8 stage), written out again here so that the tile kernels keep their text; what is new is the key range of
// a workgroup, the two forms of its loop, the partial epilogue and the combine kernel.
#pragma once
#include "kvc_attention_chunk.h"

#include <type_traits>

// experiment builds (build.sh, KVC_EXTRA_FLAGS) may try another rule; DESIGN.md 3.8 has what was tried
#ifndef KVC_SPLIT_PL_MIN
#define KVC_SPLIT_PL_MIN 1024
#endif
#ifndef KVC_SPLIT_MAX_WG
#define KVC_SPLIT_MAX_WG 32
#endif

namespace kvc {

// defined in kvc_attention_chunk_split_fp8.hip for the one entry in kvc_attention_chunk_split.hip; split_args is a
// SplitArgs (a type of the unnamed namespace cannot be in the signature)
int launch_split_fp8(const void* split_args, const kvc_attention_chunk_params* p, hipStream_t s);

namespace {

constexpr int SP_PL_MIN = KVC_SPLIT_PL_MIN;      // shortest key partition (a multiple of CH_KT)
constexpr int SP_MAX_WG = KVC_SPLIT_MAX_WG;      // (query tile, partition) pairs per (sequence, KV head, head group) at most
constexpr int SP_PL_MAX = 1 << 30;
static_assert(SP_PL_MIN % CH_KT == 0 && SP_PL_MIN > 0, "a partition is whole 32-key steps");

struct SplitArgs {
  ChunkArgs c;
  float* po;                       // partial O  [nparts][num_tokens][num_heads][hd], not normalised
  float* pml;                      // partial (m, l)  [nparts][num_tokens][num_heads][2]
  int32_t pl, nparts, qtiles, num_tokens;      // partition length, partitions of max_ctx, query tiles of max_q
};

// ---------------------------------------------------------------------------------- 1. output pass over one partition
template <typename T, int HD, int NT, int KVD>
__global__ __launch_bounds__(256) void chunk_split_out_kernel(SplitArgs x) {
  using M = Mma16<T>;
  using V8 = typename M::V8;
  constexpr int PP = HD / 8;                  // 16-byte pieces per K row
  constexpr int PP_LOG2 = HD == 128 ? 4 : 3;
  constexpr int KS = HD / 32;                 // MFMA k-steps of QK^T
  constexpr int DT = HD / 16;                 // 16-dim output tiles of P.V
  constexpr int KU = CH_KT + 1;               // K tile: units per piece row
  constexpr int VS = CH_KT + 8;               // V tile: elements per dim row
  constexpr int CPT = CH_KT * PP / 256;       // 16-byte chunks per thread and tile, of K and of V
  constexpr bool E5M2 = KVD == 2;
  constexpr int U = HD / 16;                  // fp8: 16-byte chunks per K row
  constexpr int U_LOG2 = HD == 128 ? 3 : 2;
  static_assert(HD == 64 || HD == 128, "chunk attention: head sizes 64 and 128");
  __shared__ __attribute__((aligned(16))) cu32x4 ktile[2][PP * KU];
  __shared__ __attribute__((aligned(16))) T vtile[2][HD * VS];

  const ChunkArgs& a = x.c;
  const int s = blockIdx.z;
  const int hk = blockIdx.y / a.head_groups, hg = blockIdx.y % a.head_groups;
  const HeadView hv(a, s, hk);
  // the query tile is the fastest index: the workgroups that read the same K/V bytes of a partition are neighbours
  const int part = blockIdx.x / x.qtiles, j0 = (blockIdx.x - part * x.qtiles) * CH_TQ;
  if (j0 >= hv.nq) return;                                       // (uniform: before any barrier)
  const int lim_max = hv.limit(min(hv.nq, j0 + CH_TQ) - 1);     // the tile's last token sees the most
  const int lim_min = hv.limit(j0);
  const int kbeg = part * x.pl;                                  // (<= max_ctx: no overflow)
  if (kbeg >= lim_max) return;                                   // the combine never looks at this partition of the tile
  const int kend = (int)min((int64_t)kbeg + x.pl, (int64_t)lim_max);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;
  const int nh = min(CH_HG, a.qpk - hg * CH_HG);                // query heads of this group
  const int h0 = hk * a.qpk + hg * CH_HG;
  const int tok = j0 + c;                                        // the lane's query token (MFMA column)
  const bool tok_ok = tok < hv.nq;
  const int lim = tok_ok ? hv.limit(tok) : 0;
  const T* kc = reinterpret_cast<const T*>(a.k_cache);
  const T* vc = reinterpret_cast<const T*>(a.v_cache);
  const int bs = a.bs, bsl = a.bs_log2;
  // fp8: at HD 128 one K and one V chunk per thread, at HD 64 waves 0, 1 take K and waves 2, 3 take V
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
  // global -> registers: keys k0 .. k0 + 31 of the head, in the tile kernel's chunk order.  below = true_type: every key
  // of the step is visible to every token of the tile -- no compare, no zeroing.  Otherwise a block is read if its first
  // key is visible (it exists then) and V elements of keys nobody sees are zeroed (0 * garbage could be NaN)
  auto fetch = [&](int k0, auto below) __attribute__((always_inline)) {
    constexpr bool ALL = decltype(below)::value;
    if constexpr (KVD != 0) {
      const int b = id8 >> (bsl + U_LOG2), r = id8 & ((U << bsl) - 1);       // block of the tile, chunk of the block
      const int kb = k0 + (b << bsl);
      kreg[0] = cu32x4{0u, 0u, 0u, 0u};
      vreg[0] = cu32x4{0u, 0u, 0u, 0u};
      if (k_mine && (ALL || kb < lim_max))
        kreg[0] = *reinterpret_cast<const cu32x4*>(kc8 + (int64_t)hv.bt[kb >> bsl] * a.kv_block_stride + 16 * r);
      if (v_mine && !a.slot_major) {                             // [hd][bs]: chunk r = 16 keys of dim r / (bs / 16)
        const int key = kb + 16 * (r & ((bs >> 4) - 1));
        if (ALL || key < lim_max) {
          cu32x4 v = *reinterpret_cast<const cu32x4*>(vc8 + (int64_t)hv.bt[kb >> bsl] * a.kv_block_stride + 16 * r);
          if (!ALL && key + 16 > lim_max) {                      // byte 0 is +0 in e4m3 and in e5m2
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
        if (ALL || key < lim_max)
          vreg[0] = *reinterpret_cast<const cu32x4*>(vc8 + (int64_t)hv.bt[key >> bsl] * a.kv_block_stride +
                                                     (int64_t)(key & (bs - 1)) * HD + 16 * u);
      }
    } else {
#pragma unroll
      for (int i = 0; i < CPT; ++i) {
        const int id = tid + 256 * i;
        const int b = id >> (bsl + PP_LOG2), r = id & ((PP << bsl) - 1);    // block of the tile, chunk of the block
        const int kb = k0 + (b << bsl);
        kreg[i] = cu32x4{0u, 0u, 0u, 0u};
        if (ALL || kb < lim_max)
          kreg[i] = *reinterpret_cast<const cu32x4*>(kc + (int64_t)hv.bt[kb >> bsl] * a.kv_block_stride + 8 * r);
        vreg[i] = cu32x4{0u, 0u, 0u, 0u};
        if (!a.slot_major) {                                     // [hd][bs]: chunk r = 8 keys of dim r / (bs / 8)
          const int key = kb + 8 * (r & ((bs >> 3) - 1));
          if (ALL || key < lim_max) {
            cu32x4 v = *reinterpret_cast<const cu32x4*>(vc + (int64_t)hv.bt[kb >> bsl] * a.kv_block_stride + 8 * r);
            if (!ALL && key + 8 > lim_max) {
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                if (key + 2 * e >= lim_max) v[e] = 0u;
                else if (key + 2 * e + 1 >= lim_max) v[e] &= 0xFFFFu;
              }
            }
            vreg[i] = v;
          }
        } else {                                                 // [bs][hd]: key fastest over the lanes (see park)
          const int key = k0 + (id & (CH_KT - 1)), p = id >> 5;
          if (ALL || key < lim_max)
            vreg[i] = *reinterpret_cast<const cu32x4*>(vc + (int64_t)hv.bt[key >> bsl] * a.kv_block_stride +
                                                       (int64_t)(key & (bs - 1)) * HD + 8 * p);
        }
      }
    }
  };
  // registers -> LDS: K unit (piece p, key) at p * 33 + key, V transposed in rows of 40 elements; fp8 bytes are
  // converted (exactly) once per workgroup on the way
  auto park = [&](int buf) __attribute__((always_inline)) {
    if constexpr (KVD != 0) {
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
    } else {
#pragma unroll
      for (int i = 0; i < CPT; ++i) {
        const int id = tid + 256 * i;
        const int b = id >> (bsl + PP_LOG2), r = id & ((PP << bsl) - 1);
        int p, kt;
        if (!a.slot_major) { p = r >> bsl; kt = (b << bsl) + (r & (bs - 1)); }     // K [hd/8][bs][8]
        else { p = r & (PP - 1); kt = (b << bsl) + (r >> PP_LOG2); }               // K [bs][hd]
        ktile[buf][p * KU + kt] = kreg[i];
        if (!a.slot_major) {
          const int d = r >> (bsl - 3), k8 = (b << bsl) + 8 * (r & ((bs >> 3) - 1));
          *reinterpret_cast<cu32x4*>(&vtile[buf][d * VS + k8]) = vreg[i];
        } else {
          const int vk = id & (CH_KT - 1), vp = id >> 5;
          const V8 v = __builtin_bit_cast(V8, vreg[i]);
#pragma unroll
          for (int e = 0; e < 8; ++e) vtile[buf][(8 * vp + e) * VS + vk] = v[e];
        }
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
  // one 32-key step of the wave's heads out of LDS buffer buf: S^T = K Q^T, online max / sum, P.V (P stays in registers)
  auto step = [&](int buf, int k0, bool masked) __attribute__((always_inline)) {
    V8 ak[2][KS], av[DT];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) ak[kt][ks] = __builtin_bit_cast(V8, ktile[buf][(4 * ks + g) * KU + 16 * kt + c]);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {                            // dim 16 dt + c, keys 4 g .. + 3 and 16 + 4 g .. + 3
      const T* row = &vtile[buf][(16 * dt + c) * VS + 4 * g];
      const cu32x2 lo = *reinterpret_cast<const cu32x2*>(row), hi = *reinterpret_cast<const cu32x2*>(row + 16);
      av[dt] = __builtin_bit_cast(V8, cu32x4{lo[0], lo[1], hi[0], hi[1]});
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      if (w + 4 * nt >= nh) continue;                            // (wave-uniform)
      cf32x4 sa[2] = {cf32x4{0.f, 0.f, 0.f, 0.f}, cf32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) sa[kt] = M::mma(ak[kt][ks], bq[nt][ks], sa[kt]);
      float tv[8], tmax = -INFINITY;
#pragma unroll
      for (int j = 0; j < 8; ++j) {                              // key k0 + 16 (j / 4) + 4 g + j % 4 of token c
        float t = sa[j >> 2][j & 3] * sc;
        if (masked && k0 + 16 * (j >> 2) + 4 * g + (j & 3) >= lim) t = -INFINITY;
        tv[j] = t;
        tmax = fmaxf(tmax, t);
      }
      tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
      const float mn = fmaxf(m[nt], tmax);
      const float ms = mn == -INFINITY ? 0.0f : mn;              // (a row that has seen nothing yet: every weight 0)
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
  };
  // the partition's steps, two LDS buffers, the next step's global reads in flight while this one computes, one barrier
  // per step.  below: the whole partition lies under the tile's smallest limit (most partitions of a long context do) --
  // that loop has neither the bound compares and the V zeroing of the fetch nor the causal mask
  auto walk = [&](auto below) __attribute__((always_inline)) {
    constexpr bool ALL = decltype(below)::value;
    fetch(kbeg, below);
    park(0);
    __syncthreads();
    for (int k0 = kbeg, buf = 0; k0 < kend; k0 += CH_KT, buf ^= 1) {
      const bool more = k0 + CH_KT < kend;
      if (more) fetch(k0 + CH_KT, below);
      if (w < nh) step(buf, k0, !ALL && k0 + CH_KT > lim_min);
      if (more) park(buf ^ 1);
      __syncthreads();
    }
  };
  if ((int64_t)kbeg + x.pl <= (int64_t)lim_min) walk(std::true_type{});       // (uniform over the workgroup)
  else walk(std::false_type{});

  // the partition's result as it stands: not normalised, no v_scale.  A row that saw nothing here holds (-inf, 0, 0)
  if (!tok_ok) return;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int hi = w + 4 * nt;
    if (hi >= nh) continue;
    const int64_t row = ((int64_t)part * x.num_tokens + hv.q0 + tok) * a.num_heads + h0 + hi;
    float* o = x.po + row * HD + 4 * g;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) *reinterpret_cast<cf32x4*>(o + 16 * dt) = O[nt][dt];
    if (g == 0) {
      x.pml[row * 2] = m[nt];
      x.pml[row * 2 + 1] = l[nt];
    }
  }
}

// ---------------------------------------------------------------------------------- 2. the partitions of a row -> out
// A thread owns 4 dims of one (token, query head) row and merges the row's ceil(limit / PL) partitions in ascending
// order -- exactly those the output pass wrote for it.  v_scale is 1 for caches in the query's dtype.
template <typename T, int HD>
__global__ __launch_bounds__(256) void chunk_split_combine_kernel(SplitArgs x) {
  constexpr int TPR = HD / 4, RPW = 256 / TPR;
  const ChunkArgs& a = x.c;
  const int s = blockIdx.z, hk = blockIdx.y;
  const HeadView hv(a, s, hk);
  const int r = blockIdx.x * RPW + threadIdx.x / TPR, d4 = threadIdx.x % TPR;      // row = token * qpk + query head
  if (hv.nq <= 0 || r >= hv.nq * a.qpk) return;
  const int tok = r / a.qpk, hq = r - tok * a.qpk;
  const int np = (int)(((int64_t)hv.limit(tok) + x.pl - 1) / x.pl);
  const int64_t first = (int64_t)(hv.q0 + tok) * a.num_heads + hk * a.qpk + hq;
  const int64_t pstep = (int64_t)x.num_tokens * a.num_heads;
  float mx = -INFINITY;
  for (int p = 0; p < np; ++p) mx = fmaxf(mx, x.pml[(first + p * pstep) * 2]);
  const float ms = mx == -INFINITY ? 0.0f : mx;
  float ls = 0.0f;
  cf32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int p = 0; p < np; ++p) {
    const int64_t at = first + p * pstep;
    const float f = __builtin_amdgcn_exp2f(x.pml[at * 2] - ms);
    ls += x.pml[at * 2 + 1] * f;
    acc += *reinterpret_cast<const cf32x4*>(x.po + at * HD + 4 * d4) * f;
  }
  const float inv = ls > 0.0f ? 1.0f / ls : 0.0f;
  const float fin = inv * a.v_scale;                             // (fp32, the last multiply)
  typedef T T4 __attribute__((ext_vector_type(4)));
  T4 t;
#pragma unroll
  for (int i = 0; i < 4; ++i) t[i] = (T)(acc[i] * fin);
  *reinterpret_cast<T4*>(reinterpret_cast<T*>(a.out) + (int64_t)(hv.q0 + tok) * a.o_stride + (int64_t)(hk * a.qpk + hq) * HD +
                         4 * d4) = t;
  if (d4 == 0) {                                                 // the tile kernel's convention: chunk_metric_kernel reads it
    float* st = a.stats + first * 2;
    st[0] = ls > 0.0f ? mx : 0.0f;
    st[1] = inv;
  }
}

template <typename T, int HD, int KVD>
int launch_split(const SplitArgs& x, int num_seqs, int use_l2, hipStream_t s) {
  const ChunkArgs& a = x.c;
  const int nh = a.qpk < CH_HG ? a.qpk : CH_HG;
  const dim3 grid(x.qtiles * x.nparts, a.num_kv_heads * a.head_groups, num_seqs);
  if (nh <= 4) hipLaunchKernelGGL((chunk_split_out_kernel<T, HD, 1, KVD>), grid, dim3(256), 0, s, x);
  else if (nh <= 8) hipLaunchKernelGGL((chunk_split_out_kernel<T, HD, 2, KVD>), grid, dim3(256), 0, s, x);
  else hipLaunchKernelGGL((chunk_split_out_kernel<T, HD, 4, KVD>), grid, dim3(256), 0, s, x);
  constexpr int RPW = 256 / (HD / 4);
  const dim3 cgrid((int)(((int64_t)a.max_q * a.qpk + RPW - 1) / RPW), a.num_kv_heads, num_seqs);
  hipLaunchKernelGGL((chunk_split_combine_kernel<T, HD>), cgrid, dim3(256), 0, s, x);
  if (a.metrics != nullptr) {
    const dim3 mgrid((a.max_ctx + CH_MP - 1) / CH_MP, a.num_kv_heads, num_seqs);
    if (use_l2) hipLaunchKernelGGL((chunk_metric_kernel<T, HD, true, KVD>), mgrid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((chunk_metric_kernel<T, HD, false, KVD>), mgrid, dim3(256), 0, s, a);
  }
  return check_launch("paged_attention_chunk_split");
}

template <int KVD>
int launch_split_any(const SplitArgs& x, const kvc_attention_chunk_params* p, hipStream_t s) {
  if (p->head_size == 128)
    return p->dtype == 0 ? launch_split<_Float16, 128, KVD>(x, p->num_seqs, p->use_l2, s)
                         : launch_split<__bf16, 128, KVD>(x, p->num_seqs, p->use_l2, s);
  return p->dtype == 0 ? launch_split<_Float16, 64, KVD>(x, p->num_seqs, p->use_l2, s)
                       : launch_split<__bf16, 64, KVD>(x, p->num_seqs, p->use_l2, s);
}

}  // namespace
}  // namespace kvc
