// What the two translation units of the TREE variants share (kvc_attention_chunk_tree.hip: caches in the query's
// dtype, the description and the C entry are there; kvc_attention_chunk_tree_fp8.hip: e4m3 / e5m2 caches): the
// entry's refusals and arguments, and the launches that do not depend on which wide kernel a unit holds -- the short
// TREE kernel (R <= 32), the combine kernel and the TREE row-form metric kernel.  The wide kernels of the two cache
// families are two templates of one name (kvc_attention_chunk_wide.h / _wide_fp8.h), so each unit hands its own
// launch of them to launch_tree.
#pragma once
#include "kvc_attention_chunk_metric_rows.h"
#include "kvc_attention_chunk_short.h"

namespace kvc {

// the fp8 instantiations' side of kvc_paged_attention_chunk_tree (kvc_attention_chunk_tree_fp8.hip)
int chunk_tree_fp8(const kvc_attention_chunk_params* p, const uint64_t* tree_mask, float k_scale, float v_scale,
                   void* partial, size_t partial_bytes, hipStream_t s);

namespace {

// (token, query head) rows per KV head: the wide kernels' and the row form's four tiles -- and, a token having at least
// one row, at most 64 new tokens per sequence: the bits of a mask word
constexpr int CT_MAX_ROWS = 64;

// 1 <= rows <= CT_MAX_ROWS for a call whose heads divide
inline bool tree_rows_ok(int32_t num_heads, int32_t num_kv_heads, int32_t max_query_len) {
  if (num_heads < 1 || num_kv_heads < 1 || num_heads % num_kv_heads != 0 || max_query_len < 1) return false;
  return (int64_t)max_query_len * (num_heads / num_kv_heads) <= CT_MAX_ROWS;
}

// The entry's refusals and the arguments of its passes, for every cache type: its own checks, then chunk_prepare's.
// x: the output pass (its metrics pointer is not used: the metric runs in row form behind it); m: the metric pass,
// m.c.metrics == nullptr when there is none.  false: nothing is to be launched and *rc is the entry's result.
inline bool tree_prepare(const kvc_attention_chunk_params* p, const uint64_t* tree_mask, float k_scale, float v_scale,
                         void* partial, size_t partial_bytes, ShortTreeArgs& x, MetricRowsTreeArgs& m, int* rc) {
  auto refuse = [&](const std::string& msg) { *rc = fail_invalid("paged_attention_chunk_tree: " + msg); return false; };
  const int kvd = p->kv_cache_dtype;
  if (kvd < 0 || kvd > 2) {
    *rc = fail_invalid("Unsupported data type of kv cache: " + std::to_string(kvd));
    return false;
  }
  if (kvd == 0 && (k_scale != 1.0f || v_scale != 1.0f))
    return refuse("k_scale and v_scale belong to an fp8 cache (kv_cache_dtype 0: both 1)");
  if (kvd != 0 && (!(k_scale > 0.0f) || !(v_scale > 0.0f) || isinf(k_scale) || isinf(v_scale)))     // (NaN fails the first two)
    return refuse("k_scale and v_scale must be finite and > 0");
  if (tree_mask == nullptr || (reinterpret_cast<uintptr_t>(tree_mask) & 7))
    return refuse("tree_mask is NULL or not 8-byte aligned");
  if (p->num_heads >= 1 && p->num_kv_heads >= 1 && p->num_heads % p->num_kv_heads == 0) {
    const int64_t rows = (int64_t)(p->max_query_len > 0 ? p->max_query_len : 0) * (p->num_heads / p->num_kv_heads);
    if (rows > CT_MAX_ROWS)                                      // (so max_query_len <= 64: a word holds every new token)
      return refuse("max_query_len * (num_heads / num_kv_heads) = " + std::to_string(rows) +
                    " rows per KV head, the tree variants take at most " + std::to_string(CT_MAX_ROWS));
  }
  if (!chunk_prepare(p, kvd == 0 ? 8 : 16, x.c, rc)) return false;
  x.pl = kvc_paged_attention_chunk_short_partition(x.c.max_ctx);
  x.nparts = x.c.max_ctx > x.pl ? (x.c.max_ctx + x.pl - 1) / x.pl : 1;
  x.rows = x.c.max_q * x.c.qpk;
  x.po = x.pml = nullptr;
  x.tree = tree_mask;
  if (x.nparts > 1) {
    const size_t need = kvc_paged_attention_chunk_short_workspace_bytes(p->num_seqs, p->num_heads, p->head_size,
                                                                        p->max_query_len, x.c.max_ctx);
    if (partial == nullptr || (reinterpret_cast<uintptr_t>(partial) & 15) || partial_bytes < need)
      return refuse("partial scratch too small (or not 16-byte aligned)");
    x.po = reinterpret_cast<float*>(partial);
    x.pml = x.po + (size_t)p->num_seqs * x.nparts * x.rows * x.c.num_kv_heads * p->head_size;
  }
  if (kvd != 0) {
    x.c.scale = p->scale * k_scale;
    x.c.v_scale = v_scale;
  }
  m.c = x.c;                                                     // (metrics: NULL already when nothing is cached)
  m.mpl = metric_rows_partition(x.c.max_ctx, (int64_t)x.c.num_kv_heads * p->num_seqs);
  m.use_l2 = p->use_l2 ? 1 : 0;
  m.tree = tree_mask;
  x.c.metrics = nullptr;
  return true;
}

// The passes of one call on one stream: the output kernel (rows <= 32: the short TREE kernel; more: wide(grid), the
// unit's launch of its wide TREE kernel), the short schedule's combine kernel -- which already merges
// ceil(context_lens / PL) partitions for every row, and to which a partition a row saw nothing of is (-inf, 0, 0): a
// factor 2^(-inf) = 0 on a zero O -- and, with metrics, the TREE row-form metric kernel from the statistics they left.
template <typename T, int HD, int KVD, typename Wide>
int launch_tree(const ShortTreeArgs& x, const MetricRowsTreeArgs& m, int num_seqs, hipStream_t s, Wide wide) {
  const ChunkArgs& a = x.c;
  const dim3 grid(x.nparts, a.num_kv_heads, num_seqs);
  if (x.rows > CS_MAX_ROWS) {
    wide(grid);
  } else if (a.slot_major) {
    if (x.rows > 16) hipLaunchKernelGGL((chunk_short_kernel<T, HD, 2, true, KVD, true>), grid, dim3(256), 0, s, x);
    else hipLaunchKernelGGL((chunk_short_kernel<T, HD, 1, true, KVD, true>), grid, dim3(256), 0, s, x);
  } else {
    if (x.rows > 16) hipLaunchKernelGGL((chunk_short_kernel<T, HD, 2, false, KVD, true>), grid, dim3(256), 0, s, x);
    else hipLaunchKernelGGL((chunk_short_kernel<T, HD, 1, false, KVD, true>), grid, dim3(256), 0, s, x);
  }
  if (x.nparts > 1) {
    constexpr int RPW = 256 / (HD / 4);
    const dim3 cgrid((x.rows + RPW - 1) / RPW, a.num_kv_heads, num_seqs);
    hipLaunchKernelGGL((chunk_short_combine_kernel<T, HD, KVD != 0>), cgrid, dim3(256), 0, s, static_cast<const ShortArgs&>(x));
  }
  if (m.c.metrics != nullptr) {
    const dim3 mgrid((a.max_ctx + m.mpl - 1) / m.mpl, a.num_kv_heads, num_seqs);
    const bool two = x.rows <= 32;
    if (a.slot_major) {
      if (two) hipLaunchKernelGGL((chunk_metric_rows_kernel<T, HD, 2, true, KVD, true>), mgrid, dim3(256), 0, s, m);
      else hipLaunchKernelGGL((chunk_metric_rows_kernel<T, HD, 4, true, KVD, true>), mgrid, dim3(256), 0, s, m);
    } else {
      if (two) hipLaunchKernelGGL((chunk_metric_rows_kernel<T, HD, 2, false, KVD, true>), mgrid, dim3(256), 0, s, m);
      else hipLaunchKernelGGL((chunk_metric_rows_kernel<T, HD, 4, false, KVD, true>), mgrid, dim3(256), 0, s, m);
    }
  }
  return check_launch("paged_attention_chunk_tree");
}

}  // namespace
}  // namespace kvc
