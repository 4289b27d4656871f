// The "split" schedule of the query-block attention (F5): the tile kernel's data path with the KEYS of a head split
// over workgroups, for calls with more than 32 (token, query head) rows per KV head -- chunked prefill with a small
// chunk budget, follow-up turns of tens of tokens, long draft trees -- on a long kept cache.  The tile schedule
// (kvc_attention_chunk.h) gives such a call one workgroup per (16-token query tile, KV head x head group, sequence) that
// walks the head's whole context alone: 128 workgroups on 256 CUs at nq 16 / batch 16, and a call's time is the time
// of one walk whatever nq is.  The short schedule (kvc_attention_chunk_short.h) splits the keys but holds all rows of a
// KV head in one workgroup's registers, which ends at 32 rows.
//
//  1. chunk_split_out_kernel<T, HD, NT, KVD = 0>, grid ((query tile, key partition), KV head x head group, sequence) with
//     the query tile as the fastest index, 256 threads.  A workgroup is the tile kernel's -- 16 query tokens, up to 16
//     query heads, wave w takes heads w, w + 4, ... (NT = 1 / 2 / 4), K/V of a 32-key step fetched by all 256 threads in
//     16-byte pieces one step ahead, parked in the other of two LDS buffers (K unit (piece, key) at p * 33 + key, V
//     transposed in rows of 40 elements), one barrier per step, S^T = K Q^T and P.V on v_mfma_f32_16x16x32, P never in
//     the LDS -- but owns only the keys [p PL, min((p + 1) PL, the tile's largest limit)) of its head.  A workgroup whose
//     partition starts at or past that limit returns at once.  The loop comes in two forms, chosen once per workgroup:
//     a partition that lies wholly below the tile's SMALLEST limit (all but the last one or two of a long context) runs
//     without the bound compares and the V zeroing of the fetch and without the causal mask; the others run the tile
//     kernel's loop (mask on the steps that reach past the smallest limit).
//     Epilogue: nothing is normalised.  A lane writes its O^T accumulators as 16-byte fp32 stores to
//     partial[p][token][query head][hd], lane group 0 the row's m (scaled log2 domain) and l; a row that saw nothing of
//     the partition writes (-inf, 0, 0).
//  2. chunk_split_combine_kernel<T, HD>, grid (row group, KV head, sequence): 4 dims of one (token, query head) row per
//     thread (a wave holds 2 rows at hd 128, 4 at hd 64), 16-byte loads, no LDS.  It merges the row's ceil(limit / PL)
//     partitions -- exactly those some workgroup wrote for it, so what else the scratch holds never shows -- in
//     ascending order: common max, 2^(m_p - m) factors, fp32 sums; writes out (rounded once, v_scale of an fp8 cache in
//     the final 1 / l multiply) and the row statistics in the tile kernel's convention.  chunk_metric_kernel then runs
//     unchanged.
// Partition rule (host, below): PL = SP_PL_MIN slots, doubled until (partitions of max_context_len) x (query tiles of
// max_query_len) <= SP_MAX_WG -- a function of the call's two maxima alone, so a sequence's bits do not depend on who
// else is in the batch.  One partition: the entry hands the call to the tile schedule's entry and launches nothing else.
#include "kvc_attention_chunk_split.h"

extern "C" int32_t kvc_paged_attention_chunk_split_partition(int32_t max_context_len, int32_t max_query_len) {
  const int64_t ctx = max_context_len > 0 ? max_context_len : 0;
  const int64_t tiles = ((int64_t)(max_query_len > 0 ? max_query_len : 1) + kvc::CH_TQ - 1) / kvc::CH_TQ;
  int64_t pl = kvc::SP_PL_MIN;
  while (pl < ctx && pl < kvc::SP_PL_MAX && ((ctx + pl - 1) / pl) * tiles > kvc::SP_MAX_WG) pl *= 2;
  return (int32_t)pl;
}

extern "C" size_t kvc_paged_attention_chunk_split_workspace_bytes(int32_t num_tokens, int32_t num_heads, int32_t head_size,
                                                                  int32_t max_query_len, int32_t max_context_len) {
  if (num_tokens <= 0 || num_heads <= 0 || head_size <= 0 || max_query_len <= 0 || max_context_len <= 0) return 0;
  const int32_t pl = kvc_paged_attention_chunk_split_partition(max_context_len, max_query_len);
  const size_t nparts = ((size_t)max_context_len + pl - 1) / pl;
  if (nparts <= 1) return 0;                                     // one partition: the tile schedule, no partials
  return nparts * (size_t)num_tokens * (size_t)num_heads * ((size_t)head_size + 2) * sizeof(float);
}

extern "C" int kvc_paged_attention_chunk_split(const kvc_attention_chunk_params* p, float k_scale, float v_scale, void* partial,
                                               size_t partial_bytes, kvc_stream_t stream) {
  using namespace kvc;
  if (p == nullptr) return fail_invalid("paged_attention_chunk_split: null params");
  const int kvd = p->kv_cache_dtype;
  if (kvd < 0 || kvd > 2) return fail_invalid("Unsupported data type of kv cache: " + std::to_string(kvd));
  if (kvd == 0 && (k_scale != 1.0f || v_scale != 1.0f))
    return fail_invalid("paged_attention_chunk_split: k_scale and v_scale belong to an fp8 cache (kv_cache_dtype 0: both 1)");
  if (kvd != 0 && (!(k_scale > 0.0f) || !(v_scale > 0.0f) || isinf(k_scale) || isinf(v_scale)))     // (NaN fails the first two)
    return fail_invalid("paged_attention_chunk_split: k_scale and v_scale must be finite and > 0");
  SplitArgs x;
  int rc = KVC_OK;
  if (!chunk_prepare(p, kvd == 0 ? 8 : 16, x.c, &rc)) return rc;
  x.pl = kvc_paged_attention_chunk_split_partition(x.c.max_ctx, x.c.max_q);
  x.nparts = (int32_t)(((int64_t)x.c.max_ctx + x.pl - 1) / x.pl);
  if (x.nparts <= 1)                                             // the tile schedule itself: the same launches, the same bits
    return kvd == 0 ? kvc_paged_attention_chunk(p, stream) : kvc_paged_attention_chunk_fp8(p, k_scale, v_scale, stream);
  const size_t need = kvc_paged_attention_chunk_split_workspace_bytes(p->num_tokens, p->num_heads, p->head_size, x.c.max_q,
                                                                      x.c.max_ctx);
  if (partial == nullptr || (reinterpret_cast<uintptr_t>(partial) & 15) || partial_bytes < need)
    return fail_invalid("paged_attention_chunk_split: partial scratch too small (or not 16-byte aligned)");
  x.qtiles = (x.c.max_q + CH_TQ - 1) / CH_TQ;
  x.num_tokens = p->num_tokens;
  x.po = reinterpret_cast<float*>(partial);
  x.pml = x.po + (size_t)x.nparts * p->num_tokens * p->num_heads * p->head_size;
  if (kvd != 0) {
    x.c.scale = p->scale * k_scale;
    x.c.v_scale = v_scale;
    return launch_split_fp8(&x, p, (hipStream_t)stream);
  }
  return launch_split_any<0>(x, p, (hipStream_t)stream);
}
