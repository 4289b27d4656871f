// The kernel of the "wide" schedule of the query-block attention: the short schedule's work split (keys over workgroups
// and waves, K/V read once per call in MFMA operand form; kvc_attention_chunk_short.h) for three and four 16-row tiles
// per KV head, 33 .. 64 rows.  The description is in kvc_attention_chunk_wide.hip; ShortArgs, the partial scratch, the
// combine kernel and the metric kernel are the short schedule's.
#pragma once
#include "kvc_attention_chunk_short.h"

namespace kvc {
namespace {

constexpr int CW_MAX_ROWS = 64;    // (token, query head) rows per KV head: four MFMA tiles

// TREE: the tree rule (kvc_attention_chunk.h) instead of the chain's limits; the rows' mask words sit in an LDS tile
// where the chain keeps slim, read on masked steps only
template <typename T, int HD, int NT, bool SM, bool TREE = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void chunk_wide_kernel(ShortArgsOf<TREE> x) {
  using M = Mma16<T>;
  using V8 = typename M::V8;
  constexpr int KS = HD / 32;                 // MFMA k-steps of QK^T
  constexpr int DT = HD / 16;                 // output tiles of P.V (= dims per lane of slot-major V)
  constexpr int NP = HD / 8;                  // 16-byte pieces of a Q row (= units of a slot-major K row)
  constexpr int NR = 16 * NT;
  constexpr int RB = HD * 2;                  // bytes per slot-major K row
  constexpr int STAGE = 16 * RB;              // bytes of a wave's K tile
  constexpr int QB = NP * NR * 16;            // bytes of the Q tile: 16 KiB at hd 128 / NT 4
  constexpr int KB = SM ? 4 * STAGE : 0;
  constexpr int HDP = HD + 4;                 // floats per row of the merged O tile
  constexpr int OB = NR * HDP * 4;
  constexpr int LB = QB + KB > OB ? QB + KB : OB;
  constexpr bool PF = HD == 64;               // the next step's K and V run ahead (hd 128: no registers left for them)
  static_assert(HD == 64 || HD == 128, "chunk attention: head sizes 64 and 128");
  static_assert(NT == 3 || NT == 4, "wide schedule: three or four row tiles");
  // the Q tile, then (slot-major) the waves' K tiles; after the key loop the merged O over both
  __shared__ __attribute__((aligned(16))) uint8_t lds[LB];
  __shared__ float sm[4][NR], sl[4][NR], rM[NR], rL[NR];
  __shared__ int slim[TREE ? 1 : NR];                            // the rows' causal limits: read on masked steps only
  __shared__ uint64_t stree[TREE ? NR : 1];                      // TREE: the rows' mask words instead

  const ChunkArgs& a = x.c;
  const int s = blockIdx.z, hk = blockIdx.y;
  const HeadView hv(a, s, hk);
  if (hv.nq <= 0) return;                                        // (uniform: before any barrier)
  const int base = hv.ctx - hv.nq;                               // TREE: the first new slot (signed)
  const int lim_max = TREE ? hv.ctx : hv.limit(hv.nq - 1), lim_min = TREE ? base : hv.limit(0);
  const int kp0 = blockIdx.x * x.pl;
  if (x.nparts > 1 && kp0 >= lim_max) return;                    // the combine never looks at this partition
  const int part_end = min(kp0 + x.pl, lim_max);
  const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, g = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nrows = hv.nq * a.qpk;                               // <= 16 NT
  const int bs = a.bs, bsl = a.bs_log2;
  const T* kc = reinterpret_cast<const T*>(a.k_cache);
  const T* vc = reinterpret_cast<const T*>(a.v_cache);
  const int64_t kvs = a.kv_block_stride;
  auto swz = [](int key) { return (key / (256 / RB)) % NP; };

  // ---- Q: the head's rows once into the LDS, shared by the four waves.  Unit (piece p = dims 8 p .., row r) sits at
  // p * NR + (r + 4 (p % 4)) % NR: the 16 lanes of a group (one piece, rows 16 nt + c) read 16 consecutive units
  // (256 bytes, every bank once), and the four groups of a k-step (pieces 4 ks + g) start 64 bytes apart, so that four
  // lanes of each group together hit every bank once as well.  Rows past nq * qpk are zero.
  for (int idx = tid; idx < NR * NP; idx += 256) {
    const int r = idx / NP, pc = idx % NP;
    cu32x4 raw = {0u, 0u, 0u, 0u};
    if (r < nrows) {
      const int tok = r / a.qpk, hq = r - tok * a.qpk;
      raw = *reinterpret_cast<const cu32x4*>(reinterpret_cast<const T*>(a.q) + (int64_t)(hv.q0 + tok) * a.q_stride +
                                             (int64_t)(hk * a.qpk + hq) * HD + 8 * pc);
    }
    int rr = r + 4 * (pc & 3);
    if (rr >= NR) rr -= NR;
    *reinterpret_cast<cu32x4*>(lds + (pc * NR + rr) * 16) = raw;
  }
  if constexpr (TREE) {
    if (tid < NR) stree[tid] = tid < nrows ? tree_word(x.tree, hv.q0 + tid / a.qpk, hv.nq) : 0ull;
  } else {
    if (tid < NR) slim[tid] = tid < nrows ? hv.limit(tid / a.qpk) : 0;
  }
  // byte offset of (piece g, row 16 nt + c) in the Q tile: only the last row tile can wrap
  const int qrow = c + 4 * g, qbase = (g * NR + qrow) * 16;
  auto qoff = [&](int nt) { return qbase + (nt == NT - 1 && qrow >= 16 ? 16 * nt - NR : 16 * nt) * 16; };
  // a lane's part of the K and V addresses of a step, in elements; the rest is wave-uniform
  const uint32_t kl = SM ? lane * 8 : ((g << bsl) + c) * 8;
  const uint32_t vl = SM ? 4 * g * HD + DT * c : (c << bsl) + 4 * g;
  __syncthreads();                                               // the only barrier in front of the epilogue

  // one 32-key step of a wave as it comes from global memory: 64 / 32 registers at hd 128 / 64
  struct Raw {
    cu32x4 k[2 * KS];              // reference: [half][ks] operands; slot-major: [half][unit 64 k + lane of the tile]
    cu32x2 v[2 * DT];              // reference: [dt][half]; slot-major: key j = 4 half + i, dwords (DT / 2) j ..
  };
  // keys k0 .. k0 + 31 (k0 wave-uniform, a multiple of 32), the short kernel's forms.  A block is read if its first key
  // is visible (it exists then).  V of keys nobody sees stays zero (0 * garbage could be NaN); K beyond needs no care
  // (masked logits).
  auto load = [&](Raw& r, int k0) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int kb = k0 + 16 * h;
      const bool live = kb < lim_max;
      const int ko = kb & (bs - 1);
      const T* kp = kc + (live ? (int64_t)hv.bt[kb >> bsl] * kvs : 0) + ko * (SM ? HD : 8);      // (wave-uniform)
      const T* vp = vc + (live ? (int64_t)hv.bt[kb >> bsl] * kvs : 0) + ko * (SM ? HD : 1);
      if constexpr (!SM) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          r.k[h * KS + ks] = cu32x4{0u, 0u, 0u, 0u};
          if (kb + c < lim_max)
            r.k[h * KS + ks] = *reinterpret_cast<const cu32x4*>(kp + ((32 * ks) << bsl) + kl);
        }
        const int key = kb + 4 * g;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          cu32x2 v = {0u, 0u};
          if (key < lim_max) {
            v = *reinterpret_cast<const cu32x2*>(vp + ((16 * dt) << bsl) + vl);
            if (key + 4 > lim_max) {
#pragma unroll
              for (int e = 0; e < 2; ++e) {
                if (key + 2 * e >= lim_max) v[e] = 0u;
                else if (key + 2 * e + 1 >= lim_max) v[e] &= 0xFFFFu;
              }
            }
          }
          r.v[2 * dt + h] = v;
        }
      } else {
#pragma unroll
        for (int k = 0; k < KS; ++k) {
          r.k[h * KS + k] = cu32x4{0u, 0u, 0u, 0u};
          if (live) r.k[h * KS + k] = *reinterpret_cast<const cu32x4*>(kp + 512 * k + kl);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int j = 4 * h + i;
          const bool ok = kb + 4 * g + i < lim_max;
          if constexpr (HD == 128) {
            cu32x4 v = {0u, 0u, 0u, 0u};
            if (ok) v = *reinterpret_cast<const cu32x4*>(vp + i * HD + vl);
            r.v[2 * j] = cu32x2{v[0], v[1]};
            r.v[2 * j + 1] = cu32x2{v[2], v[3]};
          } else {
            r.v[j] = cu32x2{0u, 0u};
            if (ok) r.v[j] = *reinterpret_cast<const cu32x2*>(vp + i * HD + vl);
          }
        }
      }
    }
  };

  float m[NT], l[NT];
  cf32x4 O[NT][DT];              // O^T of row c: reference dims 16 dt + 4 g + i, slot-major dims DT (4 g + i) + dt
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    m[nt] = -INFINITY; l[nt] = 0.0f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) O[nt][dt] = cf32x4{0.f, 0.f, 0.f, 0.f};
  }
  const float sc = a.scale * CH_LOG2E;

  auto compute = [&](const Raw& r, int k0) {
    // the K operands of both halves (32 keys) stay for all row tiles; a row tile's Q operands pass through 4 registers
    // each, one ds_read_b128 per two MFMAs
    V8 ak[2][KS];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if constexpr (!SM) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) ak[h][ks] = __builtin_bit_cast(V8, r.k[h * KS + ks]);
      } else {
        uint8_t* kst = lds + QB + w * STAGE;                     // wave-private: the LDS runs a wave's accesses in order
        // the tile's 2 KS addresses are made from the lane number on every step: kept across the key loop they
        // would cost 2 KS registers that O needs
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int c = ln & 15, g = ln >> 4;
#pragma unroll
        for (int k = 0; k < KS; ++k) {
          const int u = 64 * k + ln, key = u / NP, j = u % NP;
          *reinterpret_cast<cu32x4*>(kst + key * RB + ((j ^ swz(key)) << 4)) = r.k[h * KS + k];
        }
        wave_lds_sync();
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
          ak[h][ks] = __builtin_bit_cast(V8, *reinterpret_cast<const cu32x4*>(kst + c * RB + (((4 * ks + g) ^ swz(c)) << 4)));
        wave_lds_sync();
      }
    }
    // the V operands of the step, made once for all row tiles.  Slot-major: two keys' dwords (dims DT c + dt, dt + 1)
    // become the two operand dwords (keys 2 tp, 2 tp + 1 of dim dt / of dim dt + 1) -- two registers in, two out
    cu32x4 va[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      if constexpr (!SM) {
        va[dt] = cu32x4{r.v[2 * dt][0], r.v[2 * dt][1], r.v[2 * dt + 1][0], r.v[2 * dt + 1][1]};
      } else {
#pragma unroll
        for (int tp = 0; tp < 4; ++tp) {                         // keys 2 tp (low half), 2 tp + 1 (high half) of dim DT c + dt
          const int lo = (DT / 2) * (2 * tp) + dt / 2, hi = (DT / 2) * (2 * tp + 1) + dt / 2;
          va[dt][tp] = __builtin_amdgcn_perm(r.v[hi / 2][hi % 2], r.v[lo / 2][lo % 2], (dt & 1) ? 0x07060302u : 0x05040100u);
        }
      }
    }
    const bool masked = k0 + 32 > lim_min;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      if (16 * nt >= nrows) continue;                            // (uniform) a tile of padding rows only
      cf32x4 sa[2] = {cf32x4{0.f, 0.f, 0.f, 0.f}, cf32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const V8 bq = __builtin_bit_cast(V8, *reinterpret_cast<const cu32x4*>(lds + qoff(nt) + ks * (4 * NR * 16)));
        sa[0] = M::mma(ak[0][ks], bq, sa[0]);
        sa[1] = M::mma(ak[1][ks], bq, sa[1]);
      }
      float tv[8], tmax = -INFINITY;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        tv[j] = sa[j >> 2][j & 3] * sc;
      }
      if (masked) {                                              // (uniform: the last steps of a head only)
        if constexpr (TREE) {
          // weight j is the new slot e0 + 16 (j / 4) + j % 4 with e0 = k0 + 4 g - base (the prefix: below 0)
          const uint32_t win = tree_window(stree[16 * nt + c], k0 + 4 * g - base);
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (((win >> (16 * (j >> 2) + (j & 3))) & 1u) == 0u) tv[j] = -INFINITY;
        } else {
          const int left = slim[16 * nt + c] - k0 - 4 * g;       // key 16 (j / 4) + 4 g + j % 4 of the step is weight j
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (16 * (j >> 2) + (j & 3) >= left) tv[j] = -INFINITY;
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) tmax = fmaxf(tmax, tv[j]);
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
      l[nt] = l[nt] * alpha + psum;                              // the lane's 8 keys: the four groups meet after the loop
      m[nt] = mn;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        O[nt][dt] *= alpha;
        O[nt][dt] = M::mma(__builtin_bit_cast(V8, va[dt]), pb, O[nt][dt]);
      }
    }
  };

  // the wave's steps (wave w: steps w, w + 4, ...).  hd 128: O (up to 128 registers), a raw step (64) and the softmax
  // of one row tile fill the 256 registers of two waves per SIMD -- nothing runs ahead, the SIMD's other wave and the
  // CU's second workgroup cover the latency.  hd 64: half of everything, the next step is requested before this one
  // is computed.
  if constexpr (!PF) {
    Raw ra;
    for (int k0 = kp0 + 32 * w; k0 < part_end; k0 += 128) {
      load(ra, k0);
      compute(ra, k0);
    }
  } else {
    Raw ra, rb;
    int k0 = kp0 + 32 * w;
    if (k0 < part_end) load(ra, k0);
    while (k0 < part_end) {
      if (k0 + 128 < part_end) load(rb, k0 + 128);
      compute(ra, k0);
      k0 += 128;
      if (k0 >= part_end) break;
      if (k0 + 128 < part_end) load(ra, k0 + 128);
      compute(rb, k0);
      k0 += 128;
    }
  }

  // ---- the four waves' (m, l, O) -> one, in the order w = 0 .. 3 (the short kernel's convention).  A wave that saw
  // nothing holds (-inf, 0, 0): its factor is 2^(-inf) = 0, and a row nobody saw has ms = 0 instead of -inf
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    l[nt] += __shfl_xor(l[nt], 16, 64);
    l[nt] += __shfl_xor(l[nt], 32, 64);
    if (g == 0) { sm[w][16 * nt + c] = m[nt]; sl[w][16 * nt + c] = l[nt]; }
  }
  __syncthreads();                                               // (also: every wave is done with the Q and K tiles)
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int r = 16 * nt + c;
    float mx = -INFINITY;
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) mx = fmaxf(mx, sm[ww][r]);
    const float ms = mx == -INFINITY ? 0.0f : mx;
    float ls = 0.0f;
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) ls += sl[ww][r] * __builtin_amdgcn_exp2f(sm[ww][r] - ms);
    if (w == 0 && g == 0) { rM[r] = mx; rL[r] = ls; }
    const float f = __builtin_amdgcn_exp2f(m[nt] - ms);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) O[nt][dt] *= f;
  }
  float* ob = reinterpret_cast<float*>(lds);
  for (int ww = 0; ww < 4; ++ww) {
    if (w == ww) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        float* row = ob + (16 * nt + c) * HDP;
        if constexpr (!SM) {
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) {
            cf32x4* d = reinterpret_cast<cf32x4*>(row + 16 * dt + 4 * g);
            *d = ww == 0 ? O[nt][dt] : *d + O[nt][dt];
          }
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e4 = 0; e4 < DT / 4; ++e4) {
              cf32x4* d = reinterpret_cast<cf32x4*>(row + DT * (4 * g + i) + 4 * e4);
              const cf32x4 o = {O[nt][4 * e4][i], O[nt][4 * e4 + 1][i], O[nt][4 * e4 + 2][i], O[nt][4 * e4 + 3][i]};
              *d = ww == 0 ? o : *d + o;
            }
        }
      }
    }
    __syncthreads();
  }

  // ---- rows x dims over the 256 threads: out and the statistics (one partition), or the partial scratch
  const int64_t chunk = (((int64_t)s * x.nparts + blockIdx.x) * a.num_kv_heads + hk) * x.rows;
  for (int idx = tid; idx < nrows * (HD / 4); idx += 256) {
    const int r = idx / (HD / 4), d4 = idx % (HD / 4);
    const cf32x4 o = *reinterpret_cast<const cf32x4*>(ob + r * HDP + 4 * d4);
    const float mx = rM[r], ls = rL[r];
    if (x.nparts > 1) {
      *reinterpret_cast<cf32x4*>(x.po + (chunk + r) * HD + 4 * d4) = o;
      if (d4 == 0) { x.pml[(chunk + r) * 2] = mx; x.pml[(chunk + r) * 2 + 1] = ls; }
    } else {
      const int tok = r / a.qpk, hq = r - tok * a.qpk;
      const float inv = ls > 0.0f ? 1.0f / ls : 0.0f;
      typedef T T4 __attribute__((ext_vector_type(4)));
      T4 t;
#pragma unroll
      for (int i = 0; i < 4; ++i) t[i] = (T)(o[i] * inv);
      *reinterpret_cast<T4*>(reinterpret_cast<T*>(a.out) + (int64_t)(hv.q0 + tok) * a.o_stride +
                             (int64_t)(hk * a.qpk + hq) * HD + 4 * d4) = t;
      if (d4 == 0) {
        float* st = a.stats + ((int64_t)(hv.q0 + tok) * a.num_heads + hk * a.qpk + hq) * 2;
        st[0] = ls > 0.0f ? mx : 0.0f;
        st[1] = inv;
      }
    }
  }
}

template <typename T, int HD>
int launch_wide(const ShortArgs& x, int num_seqs, int use_l2, hipStream_t s) {
  const ChunkArgs& a = x.c;
  const dim3 grid(x.nparts, a.num_kv_heads, num_seqs);
  const bool four = x.rows > 48;
  if (a.slot_major) {
    if (four) hipLaunchKernelGGL((chunk_wide_kernel<T, HD, 4, true>), grid, dim3(256), 0, s, x);
    else hipLaunchKernelGGL((chunk_wide_kernel<T, HD, 3, true>), grid, dim3(256), 0, s, x);
  } else {
    if (four) hipLaunchKernelGGL((chunk_wide_kernel<T, HD, 4, false>), grid, dim3(256), 0, s, x);
    else hipLaunchKernelGGL((chunk_wide_kernel<T, HD, 3, false>), grid, dim3(256), 0, s, x);
  }
  if (x.nparts > 1) {
    constexpr int RPW = 256 / (HD / 4);
    const dim3 cgrid((x.rows + RPW - 1) / RPW, a.num_kv_heads, num_seqs);
    hipLaunchKernelGGL((chunk_short_combine_kernel<T, HD, false>), cgrid, dim3(256), 0, s, x);
  }
  if (a.metrics != nullptr) {
    const dim3 mgrid((a.max_ctx + CH_MP - 1) / CH_MP, a.num_kv_heads, num_seqs);
    if (use_l2) hipLaunchKernelGGL((chunk_metric_kernel<T, HD, true, 0>), mgrid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((chunk_metric_kernel<T, HD, false, 0>), mgrid, dim3(256), 0, s, a);
  }
  return check_launch("paged_attention_chunk_wide");
}

// rows <= CW_MAX_ROWS for a call whose heads divide (anything else is chunk_prepare's to refuse)
inline bool wide_rows_ok(int32_t num_heads, int32_t num_kv_heads, int32_t max_query_len) {
  if (num_heads < 1 || num_kv_heads < 1 || num_heads % num_kv_heads != 0) return false;
  return (int64_t)(max_query_len > 0 ? max_query_len : 0) * (num_heads / num_kv_heads) <= CW_MAX_ROWS;
}

}  // namespace
}  // namespace kvc
