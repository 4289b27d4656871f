// The "short" schedule of the query-block attention (F5): calls whose query block is so short -- verifying a few draft
// tokens, a short follow-up turn -- that ALL (token, query head) pairs of a KV head fit one or two 16-row MFMA tiles,
// R = max_query_len * (num_heads / num_kv_heads) <= 32.  The tile kernel (kvc_attention_chunk.h) gives such a call one
// workgroup per (sequence, KV head x head group) whose tiles are mostly zero rows and which walks the whole context
// alone; here the KEYS are what is split.
//
//  1. chunk_short_kernel<T, HD, NT, SM>, grid (key partition of PL slots, KV head, sequence), 256 threads.
//     The N dimension of both MFMA products is the row r = token * qpk + query head of the KV head (NT = 1 or 2 tiles of
//     16 rows); every row carries its own causal limit, rows past nq_s * qpk have a zero Q and limit 0.  The four waves
//     take the partition's 32-key steps in turn (wave w: steps w, w + 4, ...): no two waves need the same K/V bytes, so
//     there is no workgroup-wide staging and no barrier in the key loop.  A wave reads its step straight from global
//     memory in operand form, one step ahead of the one it computes:
//       reference blocks   K [hd/8][bs][8]: the QK^T A operand (key c, dims 32 ks + 8 g ..) IS one 16-byte piece;
//                          V [hd][bs]: the P.V A operand (dim 16 dt + c, keys 4 g .. + 3 and 16 + 4 g .. + 3) is two
//                          8-byte reads -- the 64 lanes of one read cover 16 dims x 16 keys;
//       slot-major blocks  K [bs][hd]: a 16-key tile is read as the contiguous 16 * hd * 2 bytes it is, parked in the
//                          wave's own LDS tile (16-byte units XOR-swizzled by the key) and taken back as operands;
//                          V [bs][hd]: lane (c, g) reads hd / 16 consecutive dims of its 8 keys and builds the operand
//                          of MFMA e in registers with v_perm_b32 (dim (hd / 16) c + e of 8 keys) -- the dims of the
//                          accumulators are merely numbered differently, which only the epilogue sees.
//     S^T = K Q^T on v_mfma_f32_16x16x32 as in the tile kernel: a lane ends with 8 keys of ONE row, its 8 weights rounded
//     to T are the B operand of P.V, P never touches the LDS.  V of keys past the head's largest limit is never loaded
//     (a zero operand), the per-row mask runs on every step past the head's smallest limit.
//     Epilogue: the waves' (m, l) meet in the LDS, every wave rescales its O to the common max and the four O are
//     summed into one LDS tile in the order w = 0 .. 3.  One partition (max_context_len <= PL): the workgroup writes
//     out and the two row statistics itself.  Otherwise the unnormalised fp32 O[R][hd] with m and l per row goes to
//     the partial scratch and
//  2. chunk_short_combine_kernel<T, HD>, grid (row group, KV head, sequence), merges the ceil(largest limit / PL)
//     partitions of a head in ascending order, writes out (rounded once) and the statistics in the tile kernel's
//     convention (log2-domain max or 0, 1 / sum or 0).  chunk_metric_kernel then runs unchanged behind either.
// PL is a function of max_context_len alone (512 slots, doubled until 32 partitions cover the context): the result of a
// call does not depend on the batch, and the same call gives the same bits.
#include "kvc_attention_chunk.h"

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

template <typename T, int HD, int NT, bool SM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void chunk_short_kernel(ShortArgs x) {
  using M = Mma16<T>;
  using V8 = typename M::V8;
  constexpr int KS = HD / 32;                 // MFMA k-steps of QK^T (= 16-byte units per lane of a slot-major K tile)
  constexpr int DT = HD / 16;                 // output tiles of P.V (= dims per lane of slot-major V)
  constexpr int RB = HD * 2;                  // bytes per slot-major K row
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
  const int lim_max = hv.limit(hv.nq - 1), lim_min = hv.limit(0);
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
  auto swz = [](int key) { return (key / (256 / RB)) % U; };

  V8 bq[NT][KS];                                                 // Q operands: row 16 nt + c, dims 32 ks + 8 g ..
  int lim[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int r = 16 * nt + c, tok = r / a.qpk, hq = r - tok * a.qpk;
    const bool ok = r < nrows;
    lim[nt] = ok ? hv.limit(tok) : 0;
    const T* qp = reinterpret_cast<const T*>(a.q) + (int64_t)(hv.q0 + tok) * a.q_stride + (int64_t)(hk * a.qpk + hq) * HD + 8 * g;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      cu32x4 raw = {0u, 0u, 0u, 0u};
      if (ok) raw = *reinterpret_cast<const cu32x4*>(qp + 32 * ks);
      bq[nt][ks] = __builtin_bit_cast(V8, raw);
    }
  }

  // one 32-key step of a wave as it comes from global memory (64 / 32 registers at hd 128 / 64)
  struct Raw {
    cu32x4 k[2 * KS];              // reference: [half][ks] operands; slot-major: [half][unit 64 k + lane of the tile]
    cu32x2 v[2 * DT];              // reference: [dt][half]; slot-major: key j = 4 half + i, dwords (DT / 2) j ..
  };
  // keys k0 .. k0 + 31 (k0 wave-uniform, a multiple of 32).  A block is read if its first key is visible (it exists
  // then).  V of keys nobody sees stays zero (0 * garbage could be NaN); K beyond needs no care (masked logits).
  auto load = [&](Raw& r, int k0, bool want_k, bool want_v) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int kb = k0 + 16 * h;
      const bool live = kb < lim_max;
      const int64_t blk = live ? (int64_t)hv.bt[kb >> bsl] * kvs : 0;
      const int ko = kb & (bs - 1);
      if constexpr (!SM) {
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

  auto compute = [&](const Raw& r, const Raw& rv, int k0) {
    // S^T, one half (16 keys) at a time: the K operands of a half are dead before the next half's are made
    cf32x4 sa[NT][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      V8 ak[KS];
      if constexpr (!SM) {
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
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      if (16 * nt >= nrows) continue;
      float tv[8], tmax = -INFINITY;
#pragma unroll
      for (int j = 0; j < 8; ++j) {                              // key k0 + 16 (j / 4) + 4 g + j % 4 of row c
        float t = sa[nt][j >> 2][j & 3] * sc;
        if (masked && k0 + 16 * (j >> 2) + 4 * g + (j & 3) >= lim[nt]) t = -INFINITY;
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

  // the wave's steps, the next one requested before the current one is computed.  Two row tiles at hd 128 leave no
  // room for two steps of V next to O and Q at two waves per SIMD: there only K runs ahead, V is requested in front of
  // the step's QK^T -- and over slot-major blocks (whose K goes through a second set of registers on its way to the
  // LDS) nothing runs ahead: the second workgroup of the CU covers the latency
  if constexpr (SM && NT == 2 && HD == 128) {
    Raw ra;
    for (int k0 = kp0 + 32 * w; k0 < part_end; k0 += 128) {
      load(ra, k0, true, true);
      compute(ra, ra, k0);
    }
  } else {
    constexpr bool PFV = !(NT == 2 && HD == 128);
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

// the partitions of one (sequence, KV head), ascending: a thread owns 4 dims of one row
template <typename T, int HD>
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
  typedef T T4 __attribute__((ext_vector_type(4)));
  T4 t;
#pragma unroll
  for (int i = 0; i < 4; ++i) t[i] = (T)(acc[i] * inv);
  *reinterpret_cast<T4*>(reinterpret_cast<T*>(a.out) + (int64_t)(hv.q0 + tok) * a.o_stride + (int64_t)(hk * a.qpk + hq) * HD +
                         4 * d4) = t;
  if (d4 == 0) {
    float* st = a.stats + ((int64_t)(hv.q0 + tok) * a.num_heads + hk * a.qpk + hq) * 2;
    st[0] = ls > 0.0f ? mx : 0.0f;
    st[1] = inv;
  }
}

template <typename T, int HD>
int launch_short(const ShortArgs& x, int num_seqs, int use_l2, hipStream_t s) {
  const ChunkArgs& a = x.c;
  const dim3 grid(x.nparts, a.num_kv_heads, num_seqs);
  const bool two = x.rows > 16;
  if (a.slot_major) {
    if (two) hipLaunchKernelGGL((chunk_short_kernel<T, HD, 2, true>), grid, dim3(256), 0, s, x);
    else hipLaunchKernelGGL((chunk_short_kernel<T, HD, 1, true>), grid, dim3(256), 0, s, x);
  } else {
    if (two) hipLaunchKernelGGL((chunk_short_kernel<T, HD, 2, false>), grid, dim3(256), 0, s, x);
    else hipLaunchKernelGGL((chunk_short_kernel<T, HD, 1, false>), grid, dim3(256), 0, s, x);
  }
  if (x.nparts > 1) {
    constexpr int RPW = 256 / (HD / 4);
    const dim3 cgrid((x.rows + RPW - 1) / RPW, a.num_kv_heads, num_seqs);
    hipLaunchKernelGGL((chunk_short_combine_kernel<T, HD>), cgrid, dim3(256), 0, s, x);
  }
  if (a.metrics != nullptr) {
    const dim3 mgrid((a.max_ctx + CH_MP - 1) / CH_MP, a.num_kv_heads, num_seqs);
    if (use_l2) hipLaunchKernelGGL((chunk_metric_kernel<T, HD, true, 0>), mgrid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((chunk_metric_kernel<T, HD, false, 0>), mgrid, dim3(256), 0, s, a);
  }
  return check_launch("paged_attention_chunk_short");
}

}  // namespace
}  // namespace kvc

extern "C" int32_t kvc_paged_attention_chunk_short_eligible(int32_t num_heads, int32_t num_kv_heads, int32_t max_query_len,
                                                            int32_t kv_cache_dtype) {
  if (kv_cache_dtype != 0 || num_heads < 1 || num_kv_heads < 1 || num_heads % num_kv_heads != 0) return 0;
  const int64_t rows = (int64_t)(max_query_len > 0 ? max_query_len : 0) * (num_heads / num_kv_heads);
  return rows <= kvc::CS_MAX_ROWS ? 1 : 0;
}

extern "C" int32_t kvc_paged_attention_chunk_short_partition(int32_t max_context_len) {
  int32_t pl = kvc::CS_PL_MIN;
  while ((int64_t)pl * kvc::CS_MAX_PARTS < (int64_t)max_context_len) pl *= 2;
  return pl;
}

extern "C" size_t kvc_paged_attention_chunk_short_workspace_bytes(int32_t num_seqs, int32_t num_heads, int32_t head_size,
                                                                  int32_t max_query_len, int32_t max_context_len) {
  if (num_seqs <= 0 || num_heads <= 0 || head_size <= 0 || max_query_len <= 0 || max_context_len <= 0) return 0;
  const int32_t pl = kvc_paged_attention_chunk_short_partition(max_context_len);
  const size_t nparts = ((size_t)max_context_len + pl - 1) / pl;
  if (nparts <= 1) return 0;                                     // one partition: the kernel writes out itself
  return (size_t)num_seqs * nparts * (size_t)max_query_len * (size_t)num_heads * ((size_t)head_size + 2) * sizeof(float);
}

extern "C" int kvc_paged_attention_chunk_short(const kvc_attention_chunk_params* p, void* partial, size_t partial_bytes,
                                               kvc_stream_t stream) {
  using namespace kvc;
  if (p == nullptr) return fail_invalid("paged_attention_chunk_short: null params");
  if (p->kv_cache_dtype != 0)
    return fail_invalid("paged_attention_chunk_short: fp8 caches are not supported (they take the tile schedule)");
  if (p->num_heads >= 1 && p->num_kv_heads >= 1 && p->num_heads % p->num_kv_heads == 0 &&
      !kvc_paged_attention_chunk_short_eligible(p->num_heads, p->num_kv_heads, p->max_query_len, 0))
    return fail_invalid("paged_attention_chunk_short: max_query_len * (num_heads / num_kv_heads) = " +
                        std::to_string((int64_t)p->max_query_len * (p->num_heads / p->num_kv_heads)) +
                        " rows per KV head, the short schedule takes at most " + std::to_string(CS_MAX_ROWS));
  ShortArgs x;
  int rc = KVC_OK;
  if (!chunk_prepare(p, 8, x.c, &rc)) return rc;
  x.pl = kvc_paged_attention_chunk_short_partition(x.c.max_ctx);
  x.nparts = x.c.max_ctx > x.pl ? (x.c.max_ctx + x.pl - 1) / x.pl : 1;
  x.rows = x.c.max_q * x.c.qpk;
  x.po = x.pml = nullptr;
  if (x.nparts > 1) {
    const size_t need = kvc_paged_attention_chunk_short_workspace_bytes(p->num_seqs, p->num_heads, p->head_size,
                                                                        p->max_query_len, x.c.max_ctx);
    if (partial == nullptr || (reinterpret_cast<uintptr_t>(partial) & 15) || partial_bytes < need)
      return fail_invalid("paged_attention_chunk_short: partial scratch too small (or not 16-byte aligned)");
    x.po = reinterpret_cast<float*>(partial);
    x.pml = x.po + (size_t)p->num_seqs * x.nparts * x.rows * x.c.num_kv_heads * p->head_size;
  }
  hipStream_t s = (hipStream_t)stream;
  if (p->head_size == 128)
    return p->dtype == 0 ? launch_short<_Float16, 128>(x, p->num_seqs, p->use_l2, s)
                         : launch_short<__bf16, 128>(x, p->num_seqs, p->use_l2, s);
  return p->dtype == 0 ? launch_short<_Float16, 64>(x, p->num_seqs, p->use_l2, s)
                       : launch_short<__bf16, 64>(x, p->num_seqs, p->use_l2, s);
}
