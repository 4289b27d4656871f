// The "short" schedule of the query-block attention (F5): calls whose query block is so short -- verifying a few draft
// tokens, a short follow-up turn -- that ALL (token, query head) pairs of a KV head fit one or two 16-row MFMA tiles,
// R = max_query_len * (num_heads / num_kv_heads) <= 32.  The tile kernel (kvc_attention_chunk.h) gives such a call one
// workgroup per (sequence, KV head x head group) whose tiles are mostly zero rows and which walks the whole context
// alone; here the KEYS are what is split.
//
//  1. chunk_short_kernel<T, HD, NT, SM, KVD = 0>, grid (key partition of PL slots, KV head, sequence), 256 threads.
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
//  2. chunk_short_combine_kernel<T, HD, VS = false>, grid (row group, KV head, sequence), merges the ceil(largest limit / PL)
//     partitions of a head in ascending order, writes out (rounded once) and the statistics in the tile kernel's
//     convention (log2-domain max or 0, 1 / sum or 0).  chunk_metric_kernel then runs unchanged behind either.
// PL is a function of max_context_len alone (512 slots, doubled until 32 partitions cover the context): the result of a
// call does not depend on the batch, and the same call gives the same bits.
// The templates are in kvc_attention_chunk_short.h; this file instantiates them for caches in the query's dtype
// (KVD = 0), kvc_attention_chunk_short_fp8.hip for fp8 caches.
#include "kvc_attention_chunk_short.h"

extern "C" int32_t kvc_paged_attention_chunk_short_eligible(int32_t num_heads, int32_t num_kv_heads, int32_t max_query_len,
                                                            int32_t kv_cache_dtype) {
  return kv_cache_dtype == 0 && kvc::short_rows_ok(num_heads, num_kv_heads, max_query_len) ? 1 : 0;
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
    return fail_invalid("paged_attention_chunk_short: fp8 caches go to kvc_paged_attention_chunk_short_fp8");
  ShortArgs x;
  int rc = KVC_OK;
  if (!short_prepare(p, 8, partial, partial_bytes, "paged_attention_chunk_short", x, &rc)) return rc;
  return launch_short_any<0>(x, p, (hipStream_t)stream);
}
