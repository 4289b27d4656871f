// The "wide" schedule of the query-block attention (F5): the short schedule (kvc_attention_chunk_short.hip) for calls
// with 33 .. 64 (token, query head) rows per KV head -- verifying 5 .. 8 tokens at 8 query heads per KV head, 9 .. 16 at
// 4 --, which the short kernel cannot hold: its two row tiles at hd 128 already fill the registers of two waves per
// SIMD with O (64), Q (32) and two raw steps.
//
//  chunk_wide_kernel<T, HD, NT, SM>, NT = 3 or 4 row tiles, grid (key partition of PL slots, KV head, sequence), 256
//  threads; caches in the query's dtype.  What it keeps of the short kernel: the N dimension of both MFMA products is
//  the row r = token * qpk + query head, every row with its own causal limit (padding rows: zero Q, limit 0); the
//  four waves take the partition's 32-key steps in turn, so every K/V byte of a partition is requested by exactly one
//  wave of one workgroup -- once per call for ALL rows of the head --, with no workgroup-wide staging and no barrier
//  in the key loop; the operand forms of both block layouts (reference: K pieces and V 8-byte reads ARE operands;
//  slot-major: K through the wave's own XOR-swizzled LDS tile under wave barriers, V assembled with v_perm_b32);
//  S^T = K Q^T on v_mfma_f32_16x16x32, a lane's 8 weights rounded to T are the P.V B operand, P never in the LDS; V of
//  keys at or past the head's largest limit is a zero operand; the row mask runs on steps past the smallest limit.
//  What is its own is where things live:
//    Q    leaves the registers.  The workgroup loads the head's rows once into an LDS tile of 16-byte units (piece p =
//         dims 8 p .., row r) at p * NR + (r + 4 (p % 4)) % NR -- 16 KiB at hd 128 / NT 4 -- behind the only barrier in
//         front of the epilogue.  A row tile's operand of k-step ks is one ds_read_b128 that feeds two MFMAs (both
//         16-key halves): NT * KS reads per step against 2 NT KS + NT DT MFMAs.  The 16 lanes of a group read 256
//         consecutive bytes, the groups of one read start 64 bytes apart: no bank conflicts.
//    K    the operands of BOTH halves of the step stay in registers for all row tiles (2 KS x 4), so that
//    S    exists for one row tile at a time (8 registers): QK^T, softmax and P.V of row tile nt finish before nt + 1.
//    O    16 NT x hd fp32 = up to 128 registers per lane, accumulators of the MFMAs (free to live in AGPRs).
//    hd 128: nothing runs ahead -- two waves per SIMD, the other wave and the CU's second workgroup cover the latency,
//    as in the short kernel's slot-major / NT 2 form; hd 64: the next step's K and V are requested before this one is
//    computed.
//  Epilogue, partial scratch (ShortArgs' layout), chunk_short_combine_kernel and chunk_metric_kernel are the short
//  schedule's: the waves' (m, l) meet in the LDS, every wave rescales to the common max, the four O are summed in the
//  order w = 0 .. 3 into one LDS tile over the Q and K tiles; one partition writes out and the statistics itself.
// PL = kvc_paged_attention_chunk_short_partition(max_context_len): the bits of a sequence do not depend on the batch.
#include "kvc_attention_chunk_wide.h"

extern "C" int32_t kvc_paged_attention_chunk_wide_eligible(int32_t num_heads, int32_t num_kv_heads, int32_t max_query_len,
                                                           int32_t kv_cache_dtype) {
  return kv_cache_dtype == 0 && max_query_len >= 1 && kvc::wide_rows_ok(num_heads, num_kv_heads, max_query_len) ? 1 : 0;
}

extern "C" int kvc_paged_attention_chunk_wide(const kvc_attention_chunk_params* p, void* partial, size_t partial_bytes,
                                              kvc_stream_t stream) {
  using namespace kvc;
  if (p == nullptr) return fail_invalid("paged_attention_chunk_wide: null params");
  if (p->kv_cache_dtype != 0)
    return fail_invalid("paged_attention_chunk_wide: fp8 caches are not served by the wide schedule");
  const bool divide = p->num_heads >= 1 && p->num_kv_heads >= 1 && p->num_heads % p->num_kv_heads == 0;
  if (divide && short_rows_ok(p->num_heads, p->num_kv_heads, p->max_query_len))     // the short schedule itself: the same bits
    return kvc_paged_attention_chunk_short(p, partial, partial_bytes, stream);
  if (divide && !wide_rows_ok(p->num_heads, p->num_kv_heads, p->max_query_len))
    return fail_invalid("paged_attention_chunk_wide: max_query_len * (num_heads / num_kv_heads) = " +
                        std::to_string((int64_t)p->max_query_len * (p->num_heads / p->num_kv_heads)) +
                        " rows per KV head, the wide schedule takes at most " + std::to_string(CW_MAX_ROWS));
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
      return fail_invalid("paged_attention_chunk_wide: partial scratch too small (or not 16-byte aligned)");
    x.po = reinterpret_cast<float*>(partial);
    x.pml = x.po + (size_t)p->num_seqs * x.nparts * x.rows * x.c.num_kv_heads * p->head_size;
  }
  hipStream_t s = (hipStream_t)stream;
  if (p->head_size == 128)
    return p->dtype == 0 ? launch_wide<_Float16, 128>(x, p->num_seqs, p->use_l2, s)
                         : launch_wide<__bf16, 128>(x, p->num_seqs, p->use_l2, s);
  return p->dtype == 0 ? launch_wide<_Float16, 64>(x, p->num_seqs, p->use_l2, s)
                       : launch_wide<__bf16, 64>(x, p->num_seqs, p->use_l2, s);
}
