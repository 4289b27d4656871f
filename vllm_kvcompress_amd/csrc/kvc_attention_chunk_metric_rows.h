// The "row form" of the metric pass of the query-block attention, for calls with at most 64 (token, query head) rows
// per KV head.  Instantiated by two translation units: kvc_attention_chunk_metric_rows.hip (KVD = 0: caches in the
// query's dtype; the description of the kernel and the C entry are there) and kvc_attention_chunk_metric_rows_fp8.hip
// (KVD = 1 / 2: e4m3 / e5m2 caches).  The masks, the weight p, the reduction and the single add per slot are one text
// for both; what depends on KVD is how a wave reads its 32-key step and how the Q operands are numbered.
#pragma once
#include "kvc_attention_chunk.h"

#include <type_traits>

namespace kvc {

// the fp8 instantiations' side of kvc_paged_attention_chunk_metric_rows (kvc_attention_chunk_metric_rows_fp8.hip)
int chunk_metric_rows_fp8(const kvc_attention_chunk_params* p, float k_scale, hipStream_t s);

namespace {

constexpr int MR_MAX_ROWS = 64;    // (token, query head) rows per KV head: four MFMA tiles
constexpr int MR_PL_MIN = 256;     // shortest key partition: two steps per wave, so the read-ahead always runs
constexpr int MR_PL_MAX = 4096;
constexpr int MR_GRID = 1024;      // workgroups a longer partition must leave: four per CU

struct MetricRowsArgs {
  ChunkArgs c;
  int32_t mpl, use_l2;             // partition length (128 * 2^k slots), sum p^2 or sum p
};
// the TREE variant's arguments (kvc_attention_chunk_tree.hip): the chain kernel's argument block stays what it is
struct MetricRowsTreeArgs : MetricRowsArgs {
  const uint64_t* tree;            // [num_tokens]: bit e of token t = t sees the sequence's e-th new slot
};
template <bool TREE> using MetricRowsArgsOf = std::conditional_t<TREE, MetricRowsTreeArgs, MetricRowsArgs>;

// The partition length: the longest 128 * 2^k in [MR_PL_MIN, MR_PL_MAX] that still leaves MR_GRID workgroups.  Every
// slot's sum is formed inside ONE 32-key step of one wave, and the steps start at multiples of 32 whatever the
// partition, so the result does not depend on this choice (nor, through it, on the batch).
inline int metric_rows_partition(int64_t max_ctx, int64_t heads_x_seqs) {
  int mpl = MR_PL_MIN;
  while (mpl < MR_PL_MAX && (max_ctx + 2 * mpl - 1) / (2 * mpl) * heads_x_seqs >= MR_GRID) mpl *= 2;
  return mpl;
}

// TREE: "sees" is the tree rule (kvc_attention_chunk.h).  A lane keeps the mask word of its row where the chain keeps
// the row's limit (padding rows: a base that puts every key past the word), and the wave-uniform skip asks the OR of
// a tile's words -- "no row of the tile sees these 16 keys" -- where the chain asks the tile's largest limit.
template <typename T, int HD, int NT, bool SM, int KVD, bool TREE = false>
__global__ __launch_bounds__(256) void chunk_metric_rows_kernel(MetricRowsArgsOf<TREE> x) {
  using M = Mma16<T>;
  using V8 = typename M::V8;
  constexpr bool F8 = KVD != 0, E5M2 = KVD == 2;
  constexpr int KS = HD / 32;                 // MFMA k-steps of QK^T
  constexpr int NK = F8 ? HD / 64 : KS;       // 16-byte K reads per lane and 16 keys (an fp8 read feeds two k-steps)
  static_assert(HD == 64 || HD == 128, "chunk attention: head sizes 64 and 128");

  const ChunkArgs& a = x.c;
  const int s = blockIdx.z, hk = blockIdx.y;
  const HeadView hv(a, s, hk);
  if (hv.nq <= 0) return;
  const int base = hv.ctx - hv.nq;                               // TREE: the first new slot (signed)
  const int lim_max = TREE ? hv.ctx : hv.limit(hv.nq - 1);       // the last token sees the most (TREE: nobody sees more)
  const int kp0 = blockIdx.x * x.mpl;
  if (kp0 >= lim_max) return;
  const int part_end = min(kp0 + x.mpl, lim_max);
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nrows = hv.nq * a.qpk;                               // <= 16 NT
  const int bs = a.bs, bsl = a.bs_log2;
  const T* kc = reinterpret_cast<const T*>(a.k_cache);
  const uint8_t* kc8 = reinterpret_cast<const uint8_t*>(a.k_cache);
  const int64_t kvs = a.kv_block_stride;
  const bool l2 = x.use_l2 != 0;

  // Row 16 nt + c: its Q operands, statistics and the two bounds.  2-byte caches: k-step ks contracts dims 32 ks +
  // 8 g ..; fp8: a lane's 16-byte K read (dims 16 (g + 4 x) ..) feeds k-steps 2 x and 2 x + 1 with its two halves, so
  // k-step ks contracts dims 16 (g + 4 (ks / 2)) + 8 (ks % 2) ..  Padding rows: zero Q, limit 0.
  V8 bq[NT][KS];
  int vis[NT], win[NT], tile_lim[NT];
  int rbase[TREE ? NT : 1];                                      // TREE: instead of vis and tile_lim
  uint64_t word[TREE ? NT : 1], tile_or[TREE ? NT : 1];
  float rmax[NT], rinv[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int r = 16 * nt + c, tok = r / a.qpk, hq = r - tok * a.qpk;
    const bool ok = r < nrows;
    if constexpr (TREE) {
      // a padding row's base makes e = key - base >= 2^30 for every key: past the word, never below 0
      rbase[nt] = ok ? base : -(1 << 30);
      vis[nt] = 0;
      word[nt] = ok ? tree_word(x.tree, hv.q0 + tok, hv.nq) : 0ull;
      // (wave-uniform) the OR over the tokens of the tile's rows
      tile_or[nt] = 0ull;
      if (16 * nt < nrows)
        for (int tt = 16 * nt / a.qpk; tt <= (min(nrows, 16 * nt + 16) - 1) / a.qpk; ++tt)
          tile_or[nt] |= tree_word(x.tree, hv.q0 + tt, hv.nq);
    } else {
      vis[nt] = ok ? hv.limit(tok) : 0;
    }
    win[nt] = ok ? a.qpos[hv.q0 + tok] - a.buf_len[s] : (int)0x80000000;
    rmax[nt] = rinv[nt] = 0.0f;
    if (ok) {
      const float* st = a.stats + ((int64_t)(hv.q0 + tok) * a.num_heads + hk * a.qpk + hq) * 2;
      rmax[nt] = st[0]; rinv[nt] = st[1];
    }
    // (wave-uniform) the largest limit of the tile's rows: that of its last row's token
    tile_lim[nt] = 16 * nt < nrows ? hv.limit((min(nrows, 16 * nt + 16) - 1) / a.qpk) : 0;
    const T* qp = reinterpret_cast<const T*>(a.q) + (int64_t)(hv.q0 + tok) * a.q_stride + (int64_t)(hk * a.qpk + hq) * HD +
                  (F8 ? 16 : 8) * g;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      cu32x4 raw = {0u, 0u, 0u, 0u};
      if (ok) raw = *reinterpret_cast<const cu32x4*>(qp + (F8 ? 64 * (ks >> 1) + 8 * (ks & 1) : 32 * ks));
      bq[nt][ks] = __builtin_bit_cast(V8, raw);
    }
  }

  // one 32-key step of a wave as it comes from global memory: the K operands of MFMA row c of both 16-key halves, and
  // the positions of the 8 keys the lane gets results for (key j of the lane: k0 + 16 (j / 4) + 4 g + j % 4)
  struct Step {
    cu32x4 k[2 * NK];
    int pos[8];
  };
  // keys k0 .. k0 + 31 (k0 wave-uniform, a multiple of 32, below lim_max).  A block is read if its first key is
  // visible (it exists then); K of keys beyond the limit needs no care, their weights are selected away, not multiplied.
  // Every lane reads whole 16-byte pieces: reference blocks, 16 lanes read 256 consecutive bytes of one piece row;
  // slot-major blocks, the four lane groups read 64 consecutive bytes of a key's row and the NK reads of a half
  // consume every byte of the rows they touch.
  auto load = [&](Step& r, int k0) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int kb = k0 + 16 * h;
      const bool live = kb < lim_max;
      const int64_t blk = live ? (int64_t)hv.bt[kb >> bsl] * kvs : 0;
      const int ko = (kb & (bs - 1)) + c;
#pragma unroll
      for (int n = 0; n < NK; ++n) {
        cu32x4 v = {0u, 0u, 0u, 0u};
        if (live) {
          if constexpr (F8) {
            const int u = g + 4 * n;                             // 16-byte piece (16 dims) of the key
            v = *reinterpret_cast<const cu32x4*>(kc8 + blk + (int64_t)(SM ? ko * HD + 16 * u : ((u << bsl) + ko) * 16));
          } else {
            const int p = 4 * n + g;                             // 16-byte piece (8 dims) of the key
            v = *reinterpret_cast<const cu32x4*>(kc + blk + (int64_t)(SM ? ko * HD + 8 * p : ((p << bsl) + ko) * 8));
          }
        }
        r.k[h * NK + n] = v;
      }
      const int kr = kb + 4 * g;                                 // four keys of one block
      const int64_t at = kr < lim_max ? (int64_t)hv.bt[kr >> bsl] * bs + (kr & (bs - 1)) : 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) r.pos[4 * h + i] = kr + i < lim_max ? a.kv_position[at + i] : 0x7FFFFFFF;
    }
  };

  const float sc = a.scale * CH_LOG2E;
  auto compute = [&](const Step& r, int k0) {
    float acc[8];
    uint32_t touched = 0u;                                       // bit j: some row passed both masks at key j
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.0f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      V8 ak[KS];
      if constexpr (F8) {
#pragma unroll
        for (int n = 0; n < NK; ++n) {
          ak[2 * n] = __builtin_bit_cast(V8, cvt8x8<T, E5M2>(r.k[h * NK + n][0], r.k[h * NK + n][1]));
          ak[2 * n + 1] = __builtin_bit_cast(V8, cvt8x8<T, E5M2>(r.k[h * NK + n][2], r.k[h * NK + n][3]));
        }
      } else {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) ak[ks] = __builtin_bit_cast(V8, r.k[h * NK + ks]);
      }
      // row tiles ascending: the order of a slot's sum inside the lane
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        // (wave-uniform) no row of the tile sees these keys
        if constexpr (TREE) {
          const int e0 = k0 + 16 * h - base;                     // >= 0: the half lies in the new slots; e0 < nq <= 64 there
          if (16 * nt >= nrows || (e0 >= 0 && (e0 >= hv.nq || ((tile_or[nt] >> (e0 & 63)) & 0xFFFFull) == 0ull))) continue;
        } else {
          if (tile_lim[nt] <= k0 + 16 * h) continue;
        }
        cf32x4 sa = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) sa = M::mma(ak[ks], bq[nt][ks], sa);
        uint32_t seen = 0u;                                      // TREE: bit i = the row sees key k0 + 16 h + 4 g + i
        if constexpr (TREE) seen = tree_window(word[nt], k0 + 16 * h + 4 * g - rbase[nt]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int j = 4 * h + i;
          bool sees;
          if constexpr (TREE) sees = (seen >> i) & 1u;
          else sees = k0 + 16 * h + 4 * g + i < vis[nt];
          const bool pass = sees && r.pos[j] <= win[nt];
          const float p = pass ? __builtin_amdgcn_exp2f(sa[i] * sc - rmax[nt]) * rinv[nt] : 0.0f;
          acc[j] = __builtin_fmaf(p, l2 ? p : 1.0f, acc[j]);
          touched |= (pass ? 1u : 0u) << j;
        }
      }
    }
    // The 16 rows of the lane group, reduce-scatter: halve the values a lane carries at every exchange (4 + 2 + 1
    // shuffles), the last exchange leaves both lanes of a pair with the sum.  A fixed tree over the rows: lane c ends
    // with key j = c / 2 of its group.
    float u4[4], u2[2];
    const bool b3 = c & 8, b2 = c & 4, b1 = c & 2;
#pragma unroll
    for (int t = 0; t < 4; ++t) u4[t] = (b3 ? acc[4 + t] : acc[t]) + __shfl_xor(b3 ? acc[t] : acc[4 + t], 8, 64);
#pragma unroll
    for (int t = 0; t < 2; ++t) u2[t] = (b2 ? u4[2 + t] : u4[t]) + __shfl_xor(b2 ? u4[t] : u4[2 + t], 4, 64);
    float mine = (b1 ? u2[1] : u2[0]) + __shfl_xor(b1 ? u2[0] : u2[1], 2, 64);
    mine += __shfl_xor(mine, 1, 64);
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) touched |= (uint32_t)__shfl_xor((int)touched, d, 64);
    const int j = c >> 1;
    const int key = k0 + 16 * (j >> 2) + 4 * g + (j & 3);
    if (!(c & 1) && ((touched >> j) & 1u)) {                     // (touched: key < lim_max, the block exists)
      float* dst = a.metrics + (int64_t)hv.bt[key >> bsl] * bs + (key & (bs - 1));
      *dst = *dst + mine;
    }
  };

  // the wave's steps, the next one requested before the current one is computed
  Step cur, nxt;
  int k0 = kp0 + 32 * w;
  if (k0 < part_end) load(cur, k0);
  while (k0 < part_end) {
    const bool more = k0 + 128 < part_end;
    if (more) load(nxt, k0 + 128);
    compute(cur, k0);
    if (more) cur = nxt;
    k0 += 128;
  }
}

template <typename T, int HD, int KVD>
int launch_metric_rows(const MetricRowsArgs& x, int num_seqs, hipStream_t s) {
  const ChunkArgs& a = x.c;
  const dim3 grid((a.max_ctx + x.mpl - 1) / x.mpl, a.num_kv_heads, num_seqs);
  const bool two = a.max_q * a.qpk <= 32;
  if (a.slot_major) {
    if (two) hipLaunchKernelGGL((chunk_metric_rows_kernel<T, HD, 2, true, KVD>), grid, dim3(256), 0, s, x);
    else hipLaunchKernelGGL((chunk_metric_rows_kernel<T, HD, 4, true, KVD>), grid, dim3(256), 0, s, x);
  } else {
    if (two) hipLaunchKernelGGL((chunk_metric_rows_kernel<T, HD, 2, false, KVD>), grid, dim3(256), 0, s, x);
    else hipLaunchKernelGGL((chunk_metric_rows_kernel<T, HD, 4, false, KVD>), grid, dim3(256), 0, s, x);
  }
  return check_launch("paged_attention_chunk_metric_rows");
}

template <int KVD>
int launch_metric_rows_any(const MetricRowsArgs& x, const kvc_attention_chunk_params* p, hipStream_t s) {
  if (p->head_size == 128)
    return p->dtype == 0 ? launch_metric_rows<_Float16, 128, KVD>(x, p->num_seqs, s)
                         : launch_metric_rows<__bf16, 128, KVD>(x, p->num_seqs, s);
  return p->dtype == 0 ? launch_metric_rows<_Float16, 64, KVD>(x, p->num_seqs, s)
                       : launch_metric_rows<__bf16, 64, KVD>(x, p->num_seqs, s);
}

// The entry's refusals and arguments, for every cache type (its own checks first, then those of the output entries:
// chunk_prepare).  false: nothing is to be launched and *rc is the entry's result.
inline bool metric_rows_prepare(const kvc_attention_chunk_params* p, float k_scale, MetricRowsArgs& x, int* rc) {
  auto refuse = [&](const std::string& msg) { *rc = fail_invalid("paged_attention_chunk_metric_rows: " + msg); return false; };
  if (p->kv_cache_dtype < 0 || p->kv_cache_dtype > 2) {
    *rc = fail_invalid("Unsupported data type of kv cache: " + std::to_string(p->kv_cache_dtype));
    return false;
  }
  if (p->kv_cache_dtype == 0 && k_scale != 1.0f) return refuse("k_scale belongs to an fp8 cache (kv_cache_dtype 0: 1)");
  if (!(k_scale > 0.0f) || isinf(k_scale)) return refuse("k_scale must be finite and > 0");    // (NaN fails the first)
  if (p->metrics == nullptr) return refuse("metrics is NULL: there is nothing to add to");
  if (p->num_heads >= 1 && p->num_kv_heads >= 1 && p->num_heads % p->num_kv_heads == 0 &&
      (int64_t)(p->max_query_len > 0 ? p->max_query_len : 0) * (p->num_heads / p->num_kv_heads) > MR_MAX_ROWS)
    return refuse("max_query_len * (num_heads / num_kv_heads) = " +
                  std::to_string((int64_t)p->max_query_len * (p->num_heads / p->num_kv_heads)) +
                  " rows per KV head, the row form takes at most " + std::to_string(MR_MAX_ROWS));
  if (!chunk_prepare(p, p->kv_cache_dtype == 0 ? 8 : 16, x.c, rc)) return false;
  if (x.c.metrics == nullptr) { *rc = KVC_OK; return false; }    // nothing cached: nothing to add
  x.c.scale = p->scale * k_scale;                                // (the output entries' product, the statistics' domain)
  x.mpl = metric_rows_partition(x.c.max_ctx, (int64_t)x.c.num_kv_heads * p->num_seqs);
  x.use_l2 = p->use_l2 ? 1 : 0;
  return true;
}

}  // namespace
}  // namespace kvc
