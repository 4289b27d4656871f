// The kernels of the "short" schedule of the query-block attention, instantiated by two translation units:
// kvc_attention_chunk_short.hip (KVD = 0: caches in the query's dtype; the description of the schedule is there) and
// kvc_attention_chunk_short_fp8.hip (KVD = 1 / 2: e4m3 / e5m2 caches; the byte geometry of the fp8 step is there).
// The softmax, the merge of the four waves, the partial scratch and the combine kernel are one text for both; what
// depends on KVD is how a wave reads its 32-key step from global memory, which key sits in which MFMA row, how the
// Q operands are numbered, and the v_scale factor of the last multiply.
#pragma once
#include "kvc_attention_chunk.h"

#include <type_traits>

namespace kvc {
namespace {

constexpr int CS_MAX_ROWS = 32;    // (token, query head) rows per KV head: two MFMA tiles
constexpr int CS_PL_MIN = 512;     // shortest key partition
constexpr int CS_MAX_PARTS = 32;   // partitions a context is split into at most

struct ShortArgs {
  ChunkArgs c;
  float* po;                       // partial O  [num_seqs][nparts][num_kv_heads][rows][hd]
  float* pml;                      // partial (m, l)  [num_seqs][nparts][num_kv_heads][rows][2]
  int32_t pl, nparts, rows;        // partition length, partitions of max_ctx, max_q * qpk
};
// the TREE variants' arguments (kvc_attention_chunk_tree.hip): the chain kernels' argument block stays what it is
struct ShortTreeArgs : ShortArgs {
  const uint64_t* tree;            // [num_tokens]: bit e of token t = t sees the sequence's e-th new slot
};
template <bool TREE> using ShortArgsOf = std::conditional_t<TREE, ShortTreeArgs, ShortArgs>;

// TREE: the rows' visibility is the tree rule (kvc_attention_chunk.h) instead of the chain's limits -- every row sees
// the whole prefix, the mask runs on the steps that reach the last nq slots, and a lane keeps the 64-bit word of its
// row 16 nt + c where the chain keeps lim[nt]
template <typename T, int HD, int NT, bool SM, int KVD, bool TREE = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void chunk_short_kernel(ShortArgsOf<TREE> x) {
  using M = Mma16<T>;
  using V8 = typename M::V8;
  constexpr bool F8 = KVD != 0, E5M2 = KVD == 2;
  constexpr int KS = HD / 32;                 // MFMA k-steps of QK^T (= 16-byte units per lane of a slot-major K tile)
  constexpr int DT = HD / 16;                 // output tiles of P.V (= dims per lane of slot-major V)
  constexpr int KX = HD / 64;                 // fp8: 16-byte K reads per lane and 16 keys, each feeds two k-steps
  constexpr int RB = F8 ? HD : HD * 2;        // bytes per slot-major K row
  constexpr int U = RB / 16;                  // 16-byte units per row
  constexpr int STAGE = 16 * RB;              // bytes of a wave's K tile
  constexpr int HDP = HD + 4;                 // floats per row of the merged O tile
  constexpr int NR = 16 * NT;
  constexpr int OB = NR * HDP * 4;
  constexpr int LB = (SM && 4 * STAGE > OB) ? 4 * STAGE : OB;
  static_assert(HD == 64 || HD == 128, "chunk attention: head sizes 64 and 128");
  __shared__ __attribute__((aligned(16))) uint8_t lds[LB];      // the waves' K tiles (slot-major), then the merged O
  __shared__ float sm[4][NR], sl[4][NR], rM[NR], rL[NR];

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
  const uint8_t* kc8 = reinterpret_cast<const uint8_t*>(a.k_cache);
  const uint8_t* vc8 = reinterpret_cast<const uint8_t*>(a.v_cache);
  const int64_t kvs = a.kv_block_stride;
  auto swz = [](int key) { return (key / (256 / RB)) % U; };

  // Q operands of row 16 nt + c.  2-byte caches: dims 32 ks + 8 g ..  fp8: a lane's 16-byte K read (dims 16 (g + 4 x)
  // ..) feeds k-steps 2 x and 2 x + 1 with its two halves, so k-step ks contracts dims 16 (g + 4 (ks / 2)) + 8 (ks % 2) ..
  V8 bq[NT][KS];
  int lim[TREE ? 1 : NT];
  uint64_t word[TREE ? NT : 1];                                  // TREE: the row's mask word, 0 for padding rows
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int r = 16 * nt + c, tok = r / a.qpk, hq = r - tok * a.qpk;
    const bool ok = r < nrows;
    if constexpr (TREE) word[nt] = ok ? tree_word(x.tree, hv.q0 + tok, hv.nq) : 0ull;
    else lim[nt] = ok ? hv.limit(tok) : 0;
    const T* qp = reinterpret_cast<const T*>(a.q) + (int64_t)(hv.q0 + tok) * a.q_stride + (int64_t)(hk * a.qpk + hq) * HD +
                  (F8 ? 16 : 8) * g;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      cu32x4 raw = {0u, 0u, 0u, 0u};
      if (ok) raw = *reinterpret_cast<const cu32x4*>(qp + (F8 ? 64 * (ks >> 1) + 8 * (ks & 1) : 32 * ks));
      bq[nt][ks] = __builtin_bit_cast(V8, raw);
    }
  }

  // one 32-key step of a wave as it comes from global memory.  2-byte caches: 64 / 32 registers at hd 128 / 64;
  // fp8 caches: 32 / 16
  struct Raw {
    // 2-byte reference: [half][ks] operands; slot-major: [half][unit 64 k + lane of the tile].  fp8: [half][x]
    cu32x4 k[F8 ? 2 * KX : 2 * KS];
    // 2-byte reference: [dt][half]; slot-major: key j = 4 half + i, dwords (DT / 2) j ..
    // fp8 reference: [dt] = the lane's 8 keys of dim 16 dt + c; slot-major: key j, dwords (DT / 4) j ..
    cu32x2 v[F8 ? DT : 2 * DT];
  };
  // keys k0 .. k0 + 31 (k0 wave-uniform, a multiple of 32).  A block is read if its first key is visible (it exists
  // then).  V of keys nobody sees stays zero (0 * garbage could be NaN); K beyond needs no care (masked logits).
  auto load = [&](Raw& r, int k0, bool want_k, bool want_v) {
    if constexpr (F8 && !SM) {
      // reference blocks, K [hd/16][bs][16] and V [hd][bs] bytes.  A row c of half h is key 8 (c / 4) + 4 h + c % 4,
      // so that the 8 weights of lane (c, g) belong to the 8 CONSECUTIVE keys 8 g .. 8 g + 7: the P.V operand of dim
      // 16 dt + c is one 8-byte read (keys 8 g .. never straddle a block).  The keys of a half lie in two blocks
      // when bs = 16: the block is the lane's own.
#pragma unroll
      for (int h = 0; h < 2 && want_k; ++h) {
        const int key = k0 + 8 * (c >> 2) + 4 * h + (c & 3);
        const bool ok = key < lim_max;
        const uint8_t* kp = kc8 + (ok ? (int64_t)hv.bt[key >> bsl] * kvs : 0) + (int64_t)(((g << bsl) + (key & (bs - 1))) * 16);
#pragma unroll
        for (int xx = 0; xx < KX; ++xx) {
          r.k[h * KX + xx] = cu32x4{0u, 0u, 0u, 0u};
          if (ok) r.k[h * KX + xx] = *reinterpret_cast<const cu32x4*>(kp + (int64_t)((64 * xx) << bsl));
        }
      }
      if (want_v) {
        const int kv = k0 + 8 * g, nb = lim_max - kv;            // nb: the lane's bytes that belong to visible keys
        const uint8_t* vp = vc8 + (nb > 0 ? (int64_t)hv.bt[kv >> bsl] * kvs : 0) + (int64_t)((c << bsl) + (kv & (bs - 1)));
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          cu32x2 v = {0u, 0u};
          if (nb > 0) {
            v = *reinterpret_cast<const cu32x2*>(vp + (int64_t)((16 * dt) << bsl));
            if (nb < 8) {                                        // byte 0 is +0 in e4m3 and in e5m2
              if (nb <= 4) v[1] = 0u;
              if (nb < 4) v[0] &= (1u << (8 * nb)) - 1u;
              else if (nb > 4) v[1] &= (1u << (8 * (nb - 4))) - 1u;
            }
          }
          r.v[dt] = v;
        }
      }
      return;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int kb = k0 + 16 * h;
      const bool live = kb < lim_max;
      const int64_t blk = live ? (int64_t)hv.bt[kb >> bsl] * kvs : 0;
      const int ko = kb & (bs - 1);
      if constexpr (F8) {
        // slot-major blocks, K and V [bs][hd] bytes: rows are keys 16 h + c as over 2-byte caches.  The 16-key K tile
        // is 16 * hd contiguous bytes; V: hd / 16 bytes (dims (hd / 16) c ..) of each of the lane's 8 keys
#pragma unroll
        for (int xx = 0; xx < KX && want_k; ++xx) {
          r.k[h * KX + xx] = cu32x4{0u, 0u, 0u, 0u};
          if (live) r.k[h * KX + xx] = *reinterpret_cast<const cu32x4*>(kc8 + blk + (int64_t)(ko * HD + (64 * xx + lane) * 16));
        }
#pragma unroll
        for (int i = 0; i < 4 && want_v; ++i) {
          const int j = 4 * h + i;
          const bool ok = kb + 4 * g + i < lim_max;
          const uint8_t* vp = vc8 + blk + (int64_t)((ko + 4 * g + i) * HD + DT * c);
          if constexpr (HD == 128) {
            r.v[j] = cu32x2{0u, 0u};
            if (ok) r.v[j] = *reinterpret_cast<const cu32x2*>(vp);
          } else {
            r.v[j >> 1][j & 1] = 0u;
            if (ok) r.v[j >> 1][j & 1] = *reinterpret_cast<const uint32_t*>(vp);
          }
        }
      } else if constexpr (!SM) {
#pragma unroll
        for (int ks = 0; ks < KS && want_k; ++ks) {
          r.k[h * KS + ks] = cu32x4{0u, 0u, 0u, 0u};
          if (kb + c < lim_max)
            r.k[h * KS + ks] = *reinterpret_cast<const cu32x4*>(kc + blk + (int64_t)((((4 * ks + g) << bsl) + ko + c) * 8));
        }
        const int key = kb + 4 * g;
#pragma unroll
        for (int dt = 0; dt < DT && want_v; ++dt) {
          cu32x2 v = {0u, 0u};
          if (key < lim_max) {
            v = *reinterpret_cast<const cu32x2*>(vc + blk + (int64_t)(((16 * dt + c) << bsl) + ko + 4 * g));
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
        for (int k = 0; k < KS && want_k; ++k) {
          r.k[h * KS + k] = cu32x4{0u, 0u, 0u, 0u};
          if (live) r.k[h * KS + k] = *reinterpret_cast<const cu32x4*>(kc + blk + (int64_t)(ko * HD + (64 * k + lane) * 8));
        }
#pragma unroll
        for (int i = 0; i < 4 && want_v; ++i) {
          const int j = 4 * h + i;
          const bool ok = kb + 4 * g + i < lim_max;
          const T* vp = vc + blk + (int64_t)((ko + 4 * g + i) * HD + DT * c);
          if constexpr (HD == 128) {
            cu32x4 v = {0u, 0u, 0u, 0u};
            if (ok) v = *reinterpret_cast<const cu32x4*>(vp);
            r.v[2 * j] = cu32x2{v[0], v[1]};
            r.v[2 * j + 1] = cu32x2{v[2], v[3]};
          } else {
            r.v[j] = cu32x2{0u, 0u};
            if (ok) r.v[j] = *reinterpret_cast<const cu32x2*>(vp);
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
  // the key (within the step) of weight j of a lane: fp8 reference blocks number the rows of QK^T differently (load)
  auto key_of = [&](int j) { return (F8 && !SM) ? 8 * g + j : 16 * (j >> 2) + 4 * g + (j & 3); };
  // TREE, masked steps: bit key_of(j) - key_of(0) says whether row 16 nt + c sees the key of weight j
  auto step_window = [&](int nt, bool masked, int k0) -> uint32_t {
    if constexpr (TREE) {
      return masked ? tree_window(word[nt], k0 + key_of(0) - base) : 0u;
    } else {
      return 0u;
    }
  };
  // row 16 nt + c does not see the key of weight j (asked on masked steps only)
  auto hidden = [&](int nt, uint32_t win, int j, int k0) {
    if constexpr (TREE) return ((win >> (key_of(j) - key_of(0))) & 1u) == 0u;
    else return k0 + key_of(j) >= lim[nt];
  };

  auto compute = [&](const Raw& r, const Raw& rv, int k0) {
    // S^T, one half (16 keys) at a time: the K operands of a half are dead before the next half's are made
    cf32x4 sa[NT][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      V8 ak[KS];
      if constexpr (F8) {
        // 16 raw bytes of one key -> the operands of two k-steps.  Slot-major: the tile is parked as the BYTES it is
        // and converted after the read-back -- converting first would double the LDS bytes written and read (and the
        // tile) for the same number of conversions, every byte being read back exactly once by its wave
        cu32x4 kr[KX];
        if constexpr (!SM) {
#pragma unroll
          for (int xx = 0; xx < KX; ++xx) kr[xx] = r.k[h * KX + xx];
        } else {
          uint8_t* kst = lds + w * STAGE;                        // wave-private: the LDS runs a wave's accesses in order
#pragma unroll
          for (int xx = 0; xx < KX; ++xx) {
            const int u = 64 * xx + lane, key = u / U, j = u % U;
            *reinterpret_cast<cu32x4*>(kst + key * RB + ((j ^ swz(key)) << 4)) = r.k[h * KX + xx];
          }
          wave_lds_sync();
#pragma unroll
          for (int xx = 0; xx < KX; ++xx)
            kr[xx] = *reinterpret_cast<const cu32x4*>(kst + c * RB + (((g + 4 * xx) ^ swz(c)) << 4));
          wave_lds_sync();
        }
#pragma unroll
        for (int xx = 0; xx < KX; ++xx) {
          ak[2 * xx] = __builtin_bit_cast(V8, cvt8x8<T, E5M2>(kr[xx][0], kr[xx][1]));
          ak[2 * xx + 1] = __builtin_bit_cast(V8, cvt8x8<T, E5M2>(kr[xx][2], kr[xx][3]));
        }
      } else if constexpr (!SM) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) ak[ks] = __builtin_bit_cast(V8, r.k[h * KS + ks]);
      } else {
        uint8_t* kst = lds + w * STAGE;                          // wave-private: the LDS runs a wave's accesses in order
#pragma unroll
        for (int k = 0; k < KS; ++k) {
          const int u = 64 * k + lane, key = u / U, j = u % U;
          *reinterpret_cast<cu32x4*>(kst + key * RB + ((j ^ swz(key)) << 4)) = r.k[h * KS + k];
        }
        wave_lds_sync();
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
          ak[ks] = __builtin_bit_cast(V8, *reinterpret_cast<const cu32x4*>(kst + c * RB + (((4 * ks + g) ^ swz(c)) << 4)));
        wave_lds_sync();
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        sa[nt][h] = cf32x4{0.f, 0.f, 0.f, 0.f};
        if (16 * nt >= nrows) continue;                          // (uniform) a tile of padding rows only
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) sa[nt][h] = M::mma(ak[ks], bq[nt][ks], sa[nt][h]);
      }
    }
    const bool masked = k0 + 32 > lim_min;
    if constexpr (F8) {
      // the weights of every row tile first, then P.V with the dim tile outside: a V operand is converted once and
      // serves both row tiles, and only one is alive at a time
      V8 pb[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        if (16 * nt >= nrows) continue;
        float tv[8], tmax = -INFINITY;
        const uint32_t win = step_window(nt, masked, k0);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float t = sa[nt][j >> 2][j & 3] * sc;
          if (masked && hidden(nt, win, j, k0)) t = -INFINITY;
          tv[j] = t;
          tmax = fmaxf(tmax, t);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float mn = fmaxf(m[nt], tmax);
        const float ms = mn == -INFINITY ? 0.0f : mn;            // (a row that has seen nothing yet: every weight 0)
        const float alpha = __builtin_amdgcn_exp2f(m[nt] - ms);
        float psum = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float p = __builtin_amdgcn_exp2f(tv[j] - ms);
          psum += p;
          pb[nt][j] = (T)p;
        }
        psum += __shfl_xor(psum, 16, 64);
        psum += __shfl_xor(psum, 32, 64);
        l[nt] = l[nt] * alpha + psum;
        m[nt] = mn;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) O[nt][dt] *= alpha;
      }
      if constexpr (!SM) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const V8 av = __builtin_bit_cast(V8, cvt8x8<T, E5M2>(rv.v[dt][0], rv.v[dt][1]));
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            if (16 * nt < nrows) O[nt][dt] = M::mma(av, pb[nt], O[nt][dt]);
        }
      } else {
        // four dims (one dword of every key) at a time: convert first -- 8 keys x 2 packed converts leave (dim, dim + 1)
        // pairs per key, and one v_perm_b32 per operand dword pairs two keys of one dim, with the selectors of the
        // 2-byte kernel.  Gathering the bytes first costs the same (a 4 x 4 byte transpose is 8 v_perm_b32 for 4
        // dwords, then the same converts) and needs a second set of selectors.
#pragma unroll
        for (int q4 = 0; q4 < DT / 4; ++q4) {
          cu32x2 cw[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int f = (DT / 4) * j + q4;
            cw[j] = cvt8x4<T, E5M2>(rv.v[f >> 1][f & 1]);
          }
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            cu32x4 av;
#pragma unroll
            for (int tp = 0; tp < 4; ++tp)                       // keys 2 tp (low half), 2 tp + 1 (high half)
              av[tp] = __builtin_amdgcn_perm(cw[2 * tp + 1][d >> 1], cw[2 * tp][d >> 1], (d & 1) ? 0x07060302u : 0x05040100u);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
              if (16 * nt < nrows) O[nt][4 * q4 + d] = M::mma(__builtin_bit_cast(V8, av), pb[nt], O[nt][4 * q4 + d]);
          }
        }
      }
      return;
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      if (16 * nt >= nrows) continue;
      float tv[8], tmax = -INFINITY;
      const uint32_t win = step_window(nt, masked, k0);
#pragma unroll
      for (int j = 0; j < 8; ++j) {                              // key k0 + 16 (j / 4) + 4 g + j % 4 of row c
        float t = sa[nt][j >> 2][j & 3] * sc;
        if (masked && hidden(nt, win, j, k0)) t = -INFINITY;
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
        cu32x4 av;
        if constexpr (!SM) {
          av = cu32x4{rv.v[2 * dt][0], rv.v[2 * dt][1], rv.v[2 * dt + 1][0], rv.v[2 * dt + 1][1]};
        } else {
#pragma unroll
          for (int tp = 0; tp < 4; ++tp) {                       // keys 2 tp (low half), 2 tp + 1 (high half) of dim DT c + dt
            const int lo = (DT / 2) * (2 * tp) + dt / 2, hi = (DT / 2) * (2 * tp + 1) + dt / 2;
            av[tp] = __builtin_amdgcn_perm(rv.v[hi / 2][hi % 2], rv.v[lo / 2][lo % 2], (dt & 1) ? 0x07060302u : 0x05040100u);
          }
        }
        O[nt][dt] *= alpha;
        O[nt][dt] = M::mma(__builtin_bit_cast(V8, av), pb, O[nt][dt]);
      }
    }
  };

  // the wave's steps, the next one requested before the current one is computed.  2-byte caches: two row tiles at hd 128
  // leave no room for two steps of V next to O and Q at two waves per SIMD: there only K runs ahead, V is requested in
  // front of the step's QK^T -- and over slot-major blocks (whose K goes through a second set of registers on its way
  // to the LDS) nothing runs ahead: the second workgroup of the CU covers the latency.  fp8 caches: a raw step is half
  // the registers, K and V of the next step run ahead in every instantiation
  if constexpr (!F8 && SM && NT == 2 && HD == 128) {
    Raw ra;
    for (int k0 = kp0 + 32 * w; k0 < part_end; k0 += 128) {
      load(ra, k0, true, true);
      compute(ra, ra, k0);
    }
  } else {
    constexpr bool PFV = F8 || !(NT == 2 && HD == 128);
    Raw ra, rb;
    int k0 = kp0 + 32 * w;
    if (k0 < part_end) load(ra, k0, true, PFV);
    while (k0 < part_end) {
      if (k0 + 128 < part_end) load(rb, k0 + 128, true, PFV);
      if constexpr (!PFV) load(ra, k0, false, true);
      compute(ra, ra, k0);
      k0 += 128;
      if (k0 >= part_end) break;
      if (k0 + 128 < part_end) load(ra, k0 + 128, true, PFV);
      if constexpr (!PFV) load(ra, k0, false, true);
      compute(rb, PFV ? rb : ra, k0);
      k0 += 128;
    }
  }

  // ---- the four waves' (m, l, O) -> one, in the order w = 0 .. 3.  A wave that saw nothing holds (-inf, 0, 0):
  // its factor is 2^(-inf) = 0, and a row nobody saw has ms = 0 instead of -inf (no inf - inf)
  if (g == 0) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) { sm[w][16 * nt + c] = m[nt]; sl[w][16 * nt + c] = l[nt]; }
  }
  __syncthreads();                                               // (also: every wave is done with its K tile)
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
      float fin = inv;                                           // fp8: v_scale goes into the last multiply (fp32)
      if constexpr (F8) fin = inv * a.v_scale;
      typedef T T4 __attribute__((ext_vector_type(4)));
      T4 t;
#pragma unroll
      for (int i = 0; i < 4; ++i) t[i] = (T)(o[i] * fin);
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

// the partitions of one (sequence, KV head), ascending: a thread owns 4 dims of one row.  VS: an fp8 cache's v_scale
// goes into the last multiply (the statistics stay without it)
template <typename T, int HD, bool VS>
__global__ __launch_bounds__(256) void chunk_short_combine_kernel(ShortArgs x) {
  constexpr int TPR = HD / 4, RPW = 256 / TPR;
  const ChunkArgs& a = x.c;
  const int s = blockIdx.z, hk = blockIdx.y;
  const HeadView hv(a, s, hk);
  const int r = blockIdx.x * RPW + threadIdx.x / TPR, d4 = threadIdx.x % TPR;
  if (hv.nq <= 0 || r >= hv.nq * a.qpk) return;
  const int np = min(x.nparts, (hv.limit(hv.nq - 1) + x.pl - 1) / x.pl);
  const int64_t first = ((int64_t)s * x.nparts * a.num_kv_heads + hk) * x.rows + r;
  const int64_t step = (int64_t)a.num_kv_heads * x.rows;
  float mx = -INFINITY;
  for (int p = 0; p < np; ++p) mx = fmaxf(mx, x.pml[(first + p * step) * 2]);
  const float ms = mx == -INFINITY ? 0.0f : mx;
  float ls = 0.0f;
  cf32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int p = 0; p < np; ++p) {
    const int64_t at = first + p * step;
    const float f = __builtin_amdgcn_exp2f(x.pml[at * 2] - ms);
    ls += x.pml[at * 2 + 1] * f;
    acc += *reinterpret_cast<const cf32x4*>(x.po + at * HD + 4 * d4) * f;
  }
  const int tok = r / a.qpk, hq = r - tok * a.qpk;
  const float inv = ls > 0.0f ? 1.0f / ls : 0.0f;
  float fin = inv;
  if constexpr (VS) fin = inv * a.v_scale;
  typedef T T4 __attribute__((ext_vector_type(4)));
  T4 t;
#pragma unroll
  for (int i = 0; i < 4; ++i) t[i] = (T)(acc[i] * fin);
  *reinterpret_cast<T4*>(reinterpret_cast<T*>(a.out) + (int64_t)(hv.q0 + tok) * a.o_stride + (int64_t)(hk * a.qpk + hq) * HD +
                         4 * d4) = t;
  if (d4 == 0) {
    float* st = a.stats + ((int64_t)(hv.q0 + tok) * a.num_heads + hk * a.qpk + hq) * 2;
    st[0] = ls > 0.0f ? mx : 0.0f;
    st[1] = inv;
  }
}

template <typename T, int HD, int KVD>
int launch_short(const ShortArgs& x, int num_seqs, int use_l2, hipStream_t s) {
  const ChunkArgs& a = x.c;
  const dim3 grid(x.nparts, a.num_kv_heads, num_seqs);
  const bool two = x.rows > 16;
  if (a.slot_major) {
    if (two) hipLaunchKernelGGL((chunk_short_kernel<T, HD, 2, true, KVD>), grid, dim3(256), 0, s, x);
    else hipLaunchKernelGGL((chunk_short_kernel<T, HD, 1, true, KVD>), grid, dim3(256), 0, s, x);
  } else {
    if (two) hipLaunchKernelGGL((chunk_short_kernel<T, HD, 2, false, KVD>), grid, dim3(256), 0, s, x);
    else hipLaunchKernelGGL((chunk_short_kernel<T, HD, 1, false, KVD>), grid, dim3(256), 0, s, x);
  }
  if (x.nparts > 1) {
    constexpr int RPW = 256 / (HD / 4);
    const dim3 cgrid((x.rows + RPW - 1) / RPW, a.num_kv_heads, num_seqs);
    hipLaunchKernelGGL((chunk_short_combine_kernel<T, HD, KVD != 0>), cgrid, dim3(256), 0, s, x);
  }
  if (a.metrics != nullptr) {
    const dim3 mgrid((a.max_ctx + CH_MP - 1) / CH_MP, a.num_kv_heads, num_seqs);
    if (use_l2) hipLaunchKernelGGL((chunk_metric_kernel<T, HD, true, KVD>), mgrid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((chunk_metric_kernel<T, HD, false, KVD>), mgrid, dim3(256), 0, s, a);
  }
  return check_launch("paged_attention_chunk_short");
}

template <int KVD>
int launch_short_any(const ShortArgs& x, const kvc_attention_chunk_params* p, hipStream_t s) {
  if (p->head_size == 128)
    return p->dtype == 0 ? launch_short<_Float16, 128, KVD>(x, p->num_seqs, p->use_l2, s)
                         : launch_short<__bf16, 128, KVD>(x, p->num_seqs, p->use_l2, s);
  return p->dtype == 0 ? launch_short<_Float16, 64, KVD>(x, p->num_seqs, p->use_l2, s)
                       : launch_short<__bf16, 64, KVD>(x, p->num_seqs, p->use_l2, s);
}

// rows <= CS_MAX_ROWS for a call whose heads divide (anything else is chunk_prepare's to refuse)
inline bool short_rows_ok(int32_t num_heads, int32_t num_kv_heads, int32_t max_query_len) {
  if (num_heads < 1 || num_kv_heads < 1 || num_heads % num_kv_heads != 0) return false;
  return (int64_t)(max_query_len > 0 ? max_query_len : 0) * (num_heads / num_kv_heads) <= CS_MAX_ROWS;
}

// The refusals and arguments both short entries share, behind their own checks of the cache dtype: the row limit,
// chunk_prepare (stride_mult: see there) and the partial scratch.  false: nothing is to be launched, *rc is the result.
inline bool short_prepare(const kvc_attention_chunk_params* p, int64_t stride_mult, void* partial, size_t partial_bytes,
                          const char* who, ShortArgs& x, int* rc) {
  if (p->num_heads >= 1 && p->num_kv_heads >= 1 && p->num_heads % p->num_kv_heads == 0 &&
      !short_rows_ok(p->num_heads, p->num_kv_heads, p->max_query_len)) {
    *rc = fail_invalid(std::string(who) + ": max_query_len * (num_heads / num_kv_heads) = " +
                       std::to_string((int64_t)p->max_query_len * (p->num_heads / p->num_kv_heads)) +
                       " rows per KV head, the short schedule takes at most " + std::to_string(CS_MAX_ROWS));
    return false;
  }
  if (!chunk_prepare(p, stride_mult, x.c, rc)) return false;
  x.pl = kvc_paged_attention_chunk_short_partition(x.c.max_ctx);
  x.nparts = x.c.max_ctx > x.pl ? (x.c.max_ctx + x.pl - 1) / x.pl : 1;
  x.rows = x.c.max_q * x.c.qpk;
  x.po = x.pml = nullptr;
  if (x.nparts > 1) {
    const size_t need = kvc_paged_attention_chunk_short_workspace_bytes(p->num_seqs, p->num_heads, p->head_size,
                                                                        p->max_query_len, x.c.max_ctx);
    if (partial == nullptr || (reinterpret_cast<uintptr_t>(partial) & 15) || partial_bytes < need) {
      *rc = fail_invalid(std::string(who) + ": partial scratch too small (or not 16-byte aligned)");
      return false;
    }
    x.po = reinterpret_cast<float*>(partial);
    x.pml = x.po + (size_t)p->num_seqs * x.nparts * x.rows * x.c.num_kv_heads * p->head_size;
  }
  return true;
}

}  // namespace
}  // namespace kvc
