// The kernel of the "wide" schedule of the query-block attention over fp8 caches (KVD = 1 / 2: e4m3 / e5m2 bytes):
// the work split of the 2-byte wide kernel (kvc_attention_chunk_wide.h: three or four 16-row tiles per KV head, Q in
// the LDS, the four waves take the partition's 32-key steps in turn) with the byte geometry of the fp8 short kernel
// (kvc_attention_chunk_short.h, KVD != 0).  The description is in kvc_attention_chunk_wide_fp8.hip; ShortArgs, the
// partial scratch, the combine kernel and the metric kernel are the short schedule's.
#pragma once
#include "kvc_attention_chunk_short.h"

namespace kvc {
namespace {

constexpr int CWF_MAX_ROWS = 64;   // (token, query head) rows per KV head: four MFMA tiles

// What runs ahead: 2 -- K and V of the next step are requested before the current step is computed; 1 -- the next
// step's K is requested between the current step's two halves (behind QK^T and the softmax, in front of P.V), V of a
// step at the same point of its own step.  Chosen per instantiation from the resource report (2 waves per SIMD, no
// scratch): the table is in DESIGN.md 3.8.
template <int HD, int NT, bool SM>
constexpr int wide_fp8_ahead() { return HD == 128 && NT == 4 ? 1 : 2; }

// TREE: the tree rule (kvc_attention_chunk.h) instead of the chain's limits; the rows' mask words sit in an LDS tile
// where the chain keeps slim, read on masked steps only
template <typename T, int HD, int NT, bool SM, int KVD, bool TREE = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void chunk_wide_kernel(ShortArgsOf<TREE> x) {
  using M = Mma16<T>;
  using V8 = typename M::V8;
  constexpr bool E5M2 = KVD == 2;
  constexpr int KS = HD / 32;                 // MFMA k-steps of QK^T
  constexpr int DT = HD / 16;                 // output tiles of P.V (= bytes per lane and key of slot-major V)
  constexpr int KX = HD / 64;                 // 16-byte K reads per lane and 16 keys, each feeds two k-steps
  constexpr int NP = HD / 8;                  // 16-byte pieces of a Q row
  constexpr int NR = 16 * NT;
  constexpr int RB = HD;                      // bytes per slot-major K row
  constexpr int U = RB / 16;                  // 16-byte units per row
  constexpr int STAGE = 16 * RB;              // bytes of a wave's raw K tile
  constexpr int QB = NP * NR * 16;            // bytes of the Q tile: 16 KiB at hd 128 / NT 4
  constexpr int KB = SM ? 4 * STAGE : 0;
  constexpr int HDP = HD + 4;                 // floats per row of the merged O tile
  constexpr int OB = NR * HDP * 4;
  constexpr int LB = QB + KB > OB ? QB + KB : OB;
  constexpr int AHEAD = wide_fp8_ahead<HD, NT, SM>();
  static_assert(KVD == 1 || KVD == 2, "fp8 caches: e4m3 (1) or e5m2 (2)");
  static_assert(HD == 64 || HD == 128, "chunk attention: head sizes 64 and 128");
  static_assert(NT == 3 || NT == 4, "wide schedule: three or four row tiles");
  // the Q tile, then (slot-major) the waves' raw K tiles; after the key loop the merged O over both
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
  const uint8_t* kc8 = reinterpret_cast<const uint8_t*>(a.k_cache);
  const uint8_t* vc8 = reinterpret_cast<const uint8_t*>(a.v_cache);
  const int64_t kvs = a.kv_block_stride;
  auto swz = [](int key) { return (key / (256 / RB)) % U; };

  // ---- Q: the head's rows once into the LDS, shared by the four waves.  A lane's 16-byte K read (dims 16 (g + 4 x)
  // ..) feeds k-steps 2 x and 2 x + 1 with its two halves, so k-step ks of lane group g contracts dims
  // 16 (g + 4 (ks / 2)) + 8 (ks % 2) ..: the four groups of one ds_read_b128 read the pieces 2 g + 8 (ks / 2) + ks % 2,
  // two apart.  Unit (piece p = dims 8 p .., row r) sits at p * NR + (r + 4 ((p / 2) % 4)) % NR: the rotation is
  // 4 g for group g whatever ks.  The 16 lanes of a group (one piece, rows 16 nt + c) read 16 consecutive units (256
  // bytes, every bank once); piece rows are 16 NR bytes = a multiple of 256 apart, so the groups' bank offsets come
  // from the rotation alone: they start 64 bytes apart, and four lanes of each group together hit every bank once as
  // well.  (p % 4, the 2-byte kernel's rotation, would give groups 0 and 2 -- pieces 0 and 4 -- the same banks.)
  // Rows past nq * qpk are zero.
  for (int idx = tid; idx < NR * NP; idx += 256) {
    const int r = idx / NP, pc = idx % NP;
    cu32x4 raw = {0u, 0u, 0u, 0u};
    if (r < nrows) {
      const int tok = r / a.qpk, hq = r - tok * a.qpk;
      raw = *reinterpret_cast<const cu32x4*>(reinterpret_cast<const T*>(a.q) + (int64_t)(hv.q0 + tok) * a.q_stride +
                                             (int64_t)(hk * a.qpk + hq) * HD + 8 * pc);
    }
    int rr = r + 4 * ((pc >> 1) & 3);
    if (rr >= NR) rr -= NR;
    *reinterpret_cast<cu32x4*>(lds + (pc * NR + rr) * 16) = raw;
  }
  if constexpr (TREE) {
    if (tid < NR) stree[tid] = tid < nrows ? tree_word(x.tree, hv.q0 + tid / a.qpk, hv.nq) : 0ull;
  } else {
    if (tid < NR) slim[tid] = tid < nrows ? hv.limit(tid / a.qpk) : 0;
  }
  // byte offset of (piece 2 g, row 16 nt + c) in the Q tile: only the last row tile can wrap
  const int qrow = c + 4 * g, qbase = (2 * g * NR + qrow) * 16;
  auto qoff = [&](int nt) { return qbase + (nt == NT - 1 && qrow >= 16 ? 16 * nt - NR : 16 * nt) * 16; };
  __syncthreads();                                               // the only barrier in front of the epilogue

  // one 32-key step of a wave as it comes from global memory: 32 / 16 registers at hd 128 / 64
  struct Raw {
    cu32x4 k[2 * KX];              // [half][x]: reference piece g + 4 x of the lane's key; slot-major unit 64 x + lane
    cu32x2 v[DT];                  // reference: [dt] = the lane's 8 keys of dim 16 dt + c; slot-major: key j, dwords (DT / 4) j ..
  };
  // keys k0 .. k0 + 31 (k0 wave-uniform, a multiple of 32), the fp8 short kernel's forms.  A block is read if a key
  // of it is visible (it exists then).  V of keys nobody sees stays zero (0 * garbage could be NaN; byte 0 is +0 in
  // e4m3 and in e5m2); K beyond needs no care (masked logits).
  auto load = [&](Raw& r, int k0, bool want_k, bool want_v) {
    // the lane's parts of the addresses are made from the lane number on every step: hoisted out of the key loop
    // they would cost registers that O needs
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const int c = ln & 15, g = ln >> 4, lane = ln;
    if constexpr (!SM) {
      // reference blocks, K [hd/16][bs][16] and V [hd][bs] bytes.  Row c of half h is key 8 (c / 4) + 4 h + c % 4, so
      // that the 8 weights of lane (c, g) belong to the 8 CONSECUTIVE keys 8 g .. 8 g + 7: the P.V operand of dim
      // 16 dt + c is one 8-byte read (8 keys never straddle a block).  With bs 16 the keys of a half lie in two
      // blocks: the block table entry is the lane's own.
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
      const int kv = k0 + 8 * g, nb = lim_max - kv;              // nb: the lane's bytes that belong to visible keys
      const uint8_t* vp = vc8 + (nb > 0 ? (int64_t)hv.bt[kv >> bsl] * kvs : 0) + (int64_t)((c << bsl) + (kv & (bs - 1)));
#pragma unroll
      for (int dt = 0; dt < DT && want_v; ++dt) {
        cu32x2 v = {0u, 0u};
        if (nb > 0) {
          v = *reinterpret_cast<const cu32x2*>(vp + (int64_t)((16 * dt) << bsl));
          if (nb < 8) {
            if (nb <= 4) v[1] = 0u;
            if (nb < 4) v[0] &= (1u << (8 * nb)) - 1u;
            else if (nb > 4) v[1] &= (1u << (8 * (nb - 4))) - 1u;
          }
        }
        r.v[dt] = v;
      }
    } else {
      // slot-major blocks, K and V [bs][hd] bytes: rows are keys 16 h + c.  The 16-key K tile is 16 * hd contiguous
      // bytes; V: hd / 16 bytes (dims (hd / 16) c ..) of each of the lane's 8 keys 16 h + 4 g + i
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int kb = k0 + 16 * h;
        const bool live = kb < lim_max;
        const int64_t blk = live ? (int64_t)hv.bt[kb >> bsl] * kvs : 0;
        const int ko = kb & (bs - 1);
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
  const float sc = a.scale * CH_LOG2E;                           // (scale * k_scale: the entry folded it in)
  // the key (within the step) of weight j of a lane is (reference: 8, slot-major: 4) g + key_of(j): reference blocks
  // number the rows of QK^T differently (load).  Split so that the mask compares against constants
  auto key_of = [](int j) { return !SM ? j : 16 * (j >> 2) + (j & 3); };

  auto compute = [&](Raw& r, Raw& next, int k0) {
    // the converted K operands of both halves (32 keys) stay for all row tiles: 16 raw bytes of one key are the
    // operands of two k-steps.  Slot-major: the tile is parked as the BYTES it is and converted after the read-back
    V8 ak[2][KS];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      cu32x4 kr[KX];
      if constexpr (!SM) {
#pragma unroll
        for (int xx = 0; xx < KX; ++xx) kr[xx] = r.k[h * KX + xx];
      } else {
        uint8_t* kst = lds + QB + w * STAGE;                     // wave-private: the LDS runs a wave's accesses in order
        // the tile's addresses are made from the lane number on every step: kept across the key loop they would
        // cost registers that O needs
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int c = ln & 15, g = ln >> 4;
#pragma unroll
        for (int xx = 0; xx < KX; ++xx) {
          const int u = 64 * xx + ln, key = u / U, j = u % U;
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
        ak[h][2 * xx] = __builtin_bit_cast(V8, cvt8x8<T, E5M2>(kr[xx][0], kr[xx][1]));
        ak[h][2 * xx + 1] = __builtin_bit_cast(V8, cvt8x8<T, E5M2>(kr[xx][2], kr[xx][3]));
      }
    }
    // ---- first half of the step, row tile by row tile: QK^T (a row tile's Q operands pass through 4 registers each,
    // one ds_read_b128 per two MFMAs), softmax, the rescale of O; what stays of a row tile is its packed weights
    const bool masked = k0 + 32 > lim_min;
    V8 pb[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      if (16 * nt >= nrows) continue;                            // (uniform) a tile of padding rows only
      cf32x4 sa[2] = {cf32x4{0.f, 0.f, 0.f, 0.f}, cf32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const V8 bq = __builtin_bit_cast(
            V8, *reinterpret_cast<const cu32x4*>(lds + qoff(nt) + ((ks & 1) + 8 * (ks >> 1)) * (NR * 16)));
        sa[0] = M::mma(ak[0][ks], bq, sa[0]);
        sa[1] = M::mma(ak[1][ks], bq, sa[1]);
      }
      float tv[8], tmax = -INFINITY;
#pragma unroll
      for (int j = 0; j < 8; ++j) tv[j] = sa[j >> 2][j & 3] * sc;
      if (masked) {                                              // (uniform: the last steps of a head only)
        int ln = lane;
        asm volatile("" : "+v"(ln));                             // (not hoisted: see load)
        if constexpr (TREE) {
          // weight j is the new slot e0 + key_of(j) with e0 = k0 + (8 or 4) g - base (the prefix: below 0)
          const uint32_t win = tree_window(stree[16 * nt + (ln & 15)], k0 + (!SM ? 8 : 4) * (ln >> 4) - base);
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (((win >> key_of(j)) & 1u) == 0u) tv[j] = -INFINITY;
        } else {
          const int left = slim[16 * nt + (ln & 15)] - k0 - (!SM ? 8 : 4) * (ln >> 4);
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (key_of(j) >= left) tv[j] = -INFINITY;
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
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float p = __builtin_amdgcn_exp2f(tv[j] - ms);
        psum += p;
        pb[nt][j] = (T)p;
      }
      l[nt] = l[nt] * alpha + psum;                              // the lane's 8 keys: the four groups meet after the loop
      m[nt] = mn;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) O[nt][dt] *= alpha;
    }
    // ---- second half, dim tile outside and row tile inside: a V operand is converted once per step, serves every
    // row tile and is dead before the next one is made.  The K operands are dead here: AHEAD 1 requests this step's V
    // and the next step's K into the registers they leave (V first: P.V waits for it alone)
    if constexpr (AHEAD == 1) {
      __builtin_amdgcn_sched_barrier(0);                         // (or the scheduler hoists the requests over QK^T)
      load(r, k0, false, true);
      if (k0 + 128 < part_end) load(next, k0 + 128, true, false);
    }
    const Raw& rv = r;
    if constexpr (!SM) {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const V8 av = __builtin_bit_cast(V8, cvt8x8<T, E5M2>(rv.v[dt][0], rv.v[dt][1]));
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          if (16 * nt < nrows) O[nt][dt] = M::mma(av, pb[nt], O[nt][dt]);
      }
    } else {
      // four dims (one dword of every key) at a time: 8 keys x 2 packed converts leave (dim, dim + 1) pairs per key,
      // one v_perm_b32 per operand dword pairs two keys of one dim
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
          for (int tp = 0; tp < 4; ++tp)                         // keys 2 tp (low half), 2 tp + 1 (high half)
            av[tp] = __builtin_amdgcn_perm(cw[2 * tp + 1][d >> 1], cw[2 * tp][d >> 1], (d & 1) ? 0x07060302u : 0x05040100u);
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            if (16 * nt < nrows) O[nt][4 * q4 + d] = M::mma(__builtin_bit_cast(V8, av), pb[nt], O[nt][4 * q4 + d]);
        }
      }
    }
  };

  // the wave's steps (wave w: steps w, w + 4, ...).  AHEAD 2: K and V of the next step are requested before this one
  // is computed.  AHEAD 1 (hd 128 / NT 4, where O, the K operands and the weights leave no room for raw V during
  // QK^T, let alone for a second raw step): the next step's K is requested between this step's two halves, behind
  // this step's V (compute) -- K, which a step needs first, is a whole P.V ahead; the wait for V is covered by the
  // SIMD's other wave and the CU's second workgroup, as every wait of the 2-byte kernel at this shape
  {
    Raw ra, rb;
    int k0 = kp0 + 32 * w;
    if (k0 < part_end) load(ra, k0, true, AHEAD == 2);
    while (k0 < part_end) {
      if constexpr (AHEAD == 2) {
        if (k0 + 128 < part_end) load(rb, k0 + 128, true, true);
      }
      compute(ra, rb, k0);
      k0 += 128;
      if (k0 >= part_end) break;
      if constexpr (AHEAD == 2) {
        if (k0 + 128 < part_end) load(ra, k0 + 128, true, true);
      }
      compute(rb, ra, k0);
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

  // ---- rows x dims over the 256 threads: out and the statistics (one partition), or the partial scratch.  v_scale
  // goes into the last multiply (fp32); the statistics and the partials stay without it
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
      const float fin = inv * a.v_scale;
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

template <typename T, int HD, int KVD>
int launch_wide_fp8(const ShortArgs& x, int num_seqs, int use_l2, hipStream_t s) {
  const ChunkArgs& a = x.c;
  const dim3 grid(x.nparts, a.num_kv_heads, num_seqs);
  const bool four = x.rows > 48;
  if (a.slot_major) {
    if (four) hipLaunchKernelGGL((chunk_wide_kernel<T, HD, 4, true, KVD>), grid, dim3(256), 0, s, x);
    else hipLaunchKernelGGL((chunk_wide_kernel<T, HD, 3, true, KVD>), grid, dim3(256), 0, s, x);
  } else {
    if (four) hipLaunchKernelGGL((chunk_wide_kernel<T, HD, 4, false, KVD>), grid, dim3(256), 0, s, x);
    else hipLaunchKernelGGL((chunk_wide_kernel<T, HD, 3, false, KVD>), grid, dim3(256), 0, s, x);
  }
  if (x.nparts > 1) {
    constexpr int RPW = 256 / (HD / 4);
    const dim3 cgrid((x.rows + RPW - 1) / RPW, a.num_kv_heads, num_seqs);
    hipLaunchKernelGGL((chunk_short_combine_kernel<T, HD, true>), cgrid, dim3(256), 0, s, x);
  }
  if (a.metrics != nullptr) {
    const dim3 mgrid((a.max_ctx + CH_MP - 1) / CH_MP, a.num_kv_heads, num_seqs);
    if (use_l2) hipLaunchKernelGGL((chunk_metric_kernel<T, HD, true, KVD>), mgrid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((chunk_metric_kernel<T, HD, false, KVD>), mgrid, dim3(256), 0, s, a);
  }
  return check_launch("paged_attention_chunk_wide_fp8");
}

template <int KVD>
int launch_wide_fp8_any(const ShortArgs& x, const kvc_attention_chunk_params* p, hipStream_t s) {
  if (p->head_size == 128)
    return p->dtype == 0 ? launch_wide_fp8<_Float16, 128, KVD>(x, p->num_seqs, p->use_l2, s)
                         : launch_wide_fp8<__bf16, 128, KVD>(x, p->num_seqs, p->use_l2, s);
  return p->dtype == 0 ? launch_wide_fp8<_Float16, 64, KVD>(x, p->num_seqs, p->use_l2, s)
                       : launch_wide_fp8<__bf16, 64, KVD>(x, p->num_seqs, p->use_l2, s);
}

// rows <= CWF_MAX_ROWS for a call whose heads divide (anything else is chunk_prepare's to refuse)
inline bool wide_fp8_rows_ok(int32_t num_heads, int32_t num_kv_heads, int32_t max_query_len) {
  if (num_heads < 1 || num_kv_heads < 1 || num_heads % num_kv_heads != 0) return false;
  return (int64_t)(max_query_len > 0 ? max_query_len : 0) * (num_heads / num_kv_heads) <= CWF_MAX_ROWS;
}

}  // namespace
}  // namespace kvc
