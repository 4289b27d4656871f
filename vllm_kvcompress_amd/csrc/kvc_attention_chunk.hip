// Query-block ("chunk") paged attention over the per-head cache, with the KV-Compress metric.
// Not in the reference: its prefix-enabled prefill branch (vllm/attention/backends/flash_attn.py:1046-1063) hands ONE
// block table per sequence to flash_attn_varlen_func, which cannot read a cache that has a block table, a context
// length and a sparse set of positions per (sequence, KV head).  Here: nq_s >= 0 new tokens per sequence, already
// written to the cache as the last nq_s logical slots of every head; token j of its sequence sees slots
// i < max(0, context_lens[s, h] - (nq_s - 1 - j)) of head h.
//
// Two kernels (templates in kvc_attention_chunk.h, instantiated here for caches in the query's dtype, KVD = 0; the
// fp8 instantiations and what they change are in kvc_attention_chunk_fp8.hip).
//  1. chunk_out_kernel, grid (query tile, KV head x head group, sequence).  A workgroup owns CH_TQ = 16 query tokens of
//     one sequence and up to 16 query heads of one KV head: one 16-row MFMA tile per query head (row = token), wave w
//     takes heads w, w + 4, ... (NT of them).  It walks the head's visible slots once in tiles of CH_KT = 32 keys that
//     all four waves fetch together, coalesced, two tiles in flight (registers -> LDS, one barrier per tile):
//       K tile  16-byte unit (piece p of 8 dims, key) at p * 33 + key   -- the QK^T operand (M = keys, N = tokens,
//               K = 32 dims per v_mfma_f32_16x16x32) is one unit; 16 lanes read 16 consecutive units
//       V tile  transposed, element (dim d, key) at d * 40 + key        -- the P.V operand (M = dims, N = tokens,
//               K = 32 keys) is two 8-byte reads of one row
//     Reference blocks (K [hd/8][bs][8], V [hd][bs]) and slot-major blocks (K [bs][hd], V [bs][hd]) differ only in the
//     addresses of this copy (slot-major V is transposed on the way in, 2-byte LDS stores with the key as the fastest
//     lane index).  S^T = K Q^T leaves a lane with 8 keys of ONE token: the row statistics need two shuffles, and the
//     lane's 8 weights ARE the B operand of P.V (the contraction order over keys is free, the V read-out follows it) --
//     P never goes through the LDS.  Online max / sum per row in fp32, output rounded once.  The two row statistics
//     (max in the log2 domain, 1 / sum) go to the workspace for kernel 2.
//     K and V of a head are read from HBM once per query tile and head group.
//  2. chunk_metric_kernel (only with metrics), grid (256-slot key partition, KV head, sequence).  A wave keeps 64 keys
//     as QK^T operands in registers; the workgroup streams the query rows (16 tokens of one query head per tile, four
//     tiles per barrier) through the LDS, recomputes S, takes p = 2^(t - max) / sum from the stored statistics, masks
//     (causal + metric window) and accumulates p^2 (or p) per key over rows in a fixed order; one lane then makes the
//     single add per slot.  No atomics: the result is identical from run to run.  Slots no query reaches are not written.
#include "kvc_attention_chunk.h"

extern "C" size_t kvc_paged_attention_chunk_workspace_bytes(int32_t num_tokens, int32_t num_heads) {
  if (num_tokens <= 0 || num_heads <= 0) return 0;
  return (size_t)num_tokens * (size_t)num_heads * 2 * sizeof(float);
}

extern "C" int kvc_paged_attention_chunk(const kvc_attention_chunk_params* p, kvc_stream_t stream) {
  using namespace kvc;
  if (p == nullptr) return fail_invalid("paged_attention_chunk: null params");
  if (p->kv_cache_dtype != 0) return fail_invalid("paged_attention_chunk: fp8 caches are not supported");
  ChunkArgs a;
  int rc = KVC_OK;
  if (!chunk_prepare(p, 8, a, &rc)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (p->head_size == 128)
    return p->dtype == 0 ? launch_chunk<_Float16, 128, 0>(a, p->num_seqs, p->use_l2, s)
                         : launch_chunk<__bf16, 128, 0>(a, p->num_seqs, p->use_l2, s);
  return p->dtype == 0 ? launch_chunk<_Float16, 64, 0>(a, p->num_seqs, p->use_l2, s)
                       : launch_chunk<__bf16, 64, 0>(a, p->num_seqs, p->use_l2, s);
}
