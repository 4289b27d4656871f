// The "wide" schedule of the query-block attention (kvc_attention_chunk_wide.hip: 33 .. 64 (token, query head) rows
// per KV head) over an fp8 per-head cache (OCP e4m3fn or e5m2 bytes), both block layouts.  Dequantisation rule of the
// other fp8 chunk paths (kvc_attention_chunk_fp8.hip): bytes convert EXACTLY to the query's dtype (cvt8x4 / cvt8x8),
// k_scale rides in sc = scale * k_scale * log2(e), v_scale in the final 1 / l multiply -- of the single-partition
// epilogue and of chunk_short_combine_kernel<.., true> --, and the statistics in the workspace and in the partial
// scratch stay in the scaled log2 domain without v_scale, so chunk_metric_kernel<.., KVD> runs unchanged behind it.
//
//  chunk_wide_kernel<T, HD, NT, SM, KVD>, NT = 3 or 4 row tiles, KVD = 1 / 2, grid (key partition of PL slots, KV
//  head, sequence), 256 threads.  The work split is the 2-byte wide kernel's: the N dimension of both MFMA products is
//  the row r = token * qpk + query head, every row with its own causal limit (padding rows: zero Q, limit 0); the
//  four waves take the partition's 32-key steps in turn, so every K/V byte of a partition is requested by exactly one
//  wave of one workgroup, with no workgroup-wide staging and no barrier in the key loop; Q sits in the LDS behind the
//  only barrier in front of the epilogue; the waves' (m, l) meet in the LDS and the four O are summed in the order
//  w = 0 .. 3.  The byte geometry is the fp8 short kernel's (kvc_attention_chunk_short_fp8.hip), lane (c, g) =
//  (lane & 15, lane >> 4):
//    K    reference [hd/16][bs][16]: a lane reads whole 16-byte pieces -- piece g + 4 x of its key -- and cvt8x8 makes
//         the operands of k-steps 2 x and 2 x + 1 of the two halves.  Slot-major [bs][hd]: the 16-key tile (16 * hd
//         bytes) is parked RAW in the wave's XOR-swizzled LDS tile (unit j of key row k at j ^ ((k / (256 / hd)) %
//         (hd / 16)): writes and read-backs of a 16-lane group cover every bank once), wave barriers only, and
//         converted after the read-back.  The converted operands of BOTH 16-key halves (2 KS x 4 registers) stay for
//         all row tiles.
//    Q    k-step ks of lane group g contracts dims 16 (g + 4 (ks / 2)) + 8 (ks % 2) ..: the four groups of one
//         ds_read_b128 read the 16-byte pieces 2 g + 8 (ks / 2) + ks % 2, two apart.  Unit (piece p, row r) sits at
//         p * NR + (r + 4 ((p / 2) % 4)) % NR.  Banks: the 16 lanes of a group read 256 consecutive bytes (every bank
//         once); piece rows are 16 NR bytes apart, a multiple of 256, so only the rotation 4 g separates the groups:
//         they start 64 bytes apart and four lanes of each group together cover every bank once as well.  The 2-byte
//         kernel's rotation 4 (p % 4) would put groups 0 and 2 (pieces 0 and 4) and groups 1 and 3 on the same banks.
//    V    reference [hd][bs]: row c of half h of QK^T is key 8 (c / 4) + 4 h + c % 4, so a lane ends with the weights
//         of the 8 consecutive keys 8 g .. 8 g + 7 and the P.V operand of dim 16 dt + c is ONE 8-byte read (bs 16: the
//         block table entry is the lane's own); the mask and the zeroing use the same numbering (key_of).  Slot-major:
//         hd / 16 bytes of each of the lane's 8 keys; two packed converts and one v_perm_b32 make an operand dword.
//         V bytes of keys at or past the head's largest limit are zero before the conversion.
//  Loop order.  The 2-byte kernel finishes QK^T, softmax and P.V of a row tile before the next, with all DT converted
//  V operands alive (32 registers at hd 128).  Here a step has two halves: row tile by row tile QK^T, softmax and the
//  rescale of O, keeping the packed weights (4 registers per tile); then dim tile by dim tile one V operand is
//  converted and feeds all row tiles.  16 raw V dwords and 16 weight registers replace 32 converted ones, the K
//  operands are dead in the second half, and every V byte is converted once per step, not once per row tile.
//  Prefetch.  A raw step is 32 dwords at hd 128 (the 2-byte kernel: 64), so the next step's K and V can be requested
//  before the current one is computed where the 2-byte kernel runs nothing ahead; the depth per instantiation
//  (wide_fp8_ahead) is what two waves per SIMD without scratch allow -- the table is in DESIGN.md 3.8.
// PL = kvc_paged_attention_chunk_short_partition(max_context_len): the bits of a sequence do not depend on the batch.
#include "kvc_attention_chunk_wide_fp8.h"

extern "C" int32_t kvc_paged_attention_chunk_wide_fp8_eligible(int32_t num_heads, int32_t num_kv_heads, int32_t max_query_len,
                                                               int32_t kv_cache_dtype) {
  return (kv_cache_dtype == 1 || kv_cache_dtype == 2) && max_query_len >= 1 &&
                 kvc::wide_fp8_rows_ok(num_heads, num_kv_heads, max_query_len)
             ? 1
             : 0;
}

extern "C" int kvc_paged_attention_chunk_wide_fp8(const kvc_attention_chunk_params* p, float k_scale, float v_scale,
                                                  void* partial, size_t partial_bytes, kvc_stream_t stream) {
  using namespace kvc;
  if (p == nullptr) return fail_invalid("paged_attention_chunk_wide_fp8: null params");
  if (p->kv_cache_dtype == 0)
    return fail_invalid("paged_attention_chunk_wide_fp8: kv_cache_dtype 0 (a cache in the query's dtype) goes to "
                        "kvc_paged_attention_chunk_wide");
  if (p->kv_cache_dtype != 1 && p->kv_cache_dtype != 2)
    return fail_invalid("Unsupported data type of kv cache: " + std::to_string(p->kv_cache_dtype));
  if (!(k_scale > 0.0f) || !(v_scale > 0.0f) || isinf(k_scale) || isinf(v_scale))        // (NaN fails the first two)
    return fail_invalid("paged_attention_chunk_wide_fp8: k_scale and v_scale must be finite and > 0");
  const bool divide = p->num_heads >= 1 && p->num_kv_heads >= 1 && p->num_heads % p->num_kv_heads == 0;
  if (divide && short_rows_ok(p->num_heads, p->num_kv_heads, p->max_query_len))     // the short schedule itself: the same bits
    return kvc_paged_attention_chunk_short_fp8(p, k_scale, v_scale, partial, partial_bytes, stream);
  if (divide && !wide_fp8_rows_ok(p->num_heads, p->num_kv_heads, p->max_query_len))
    return fail_invalid("paged_attention_chunk_wide_fp8: max_query_len * (num_heads / num_kv_heads) = " +
                        std::to_string((int64_t)p->max_query_len * (p->num_heads / p->num_kv_heads)) +
                        " rows per KV head, the wide schedule takes at most " + std::to_string(CWF_MAX_ROWS));
  ShortArgs x;
  int rc = KVC_OK;
  if (!chunk_prepare(p, 16, x.c, &rc)) return rc;
  x.pl = kvc_paged_attention_chunk_short_partition(x.c.max_ctx);
  x.nparts = x.c.max_ctx > x.pl ? (x.c.max_ctx + x.pl - 1) / x.pl : 1;
  x.rows = x.c.max_q * x.c.qpk;
  x.po = x.pml = nullptr;
  if (x.nparts > 1) {
    const size_t need = kvc_paged_attention_chunk_short_workspace_bytes(p->num_seqs, p->num_heads, p->head_size,
                                                                        p->max_query_len, x.c.max_ctx);
    if (partial == nullptr || (reinterpret_cast<uintptr_t>(partial) & 15) || partial_bytes < need)
      return fail_invalid("paged_attention_chunk_wide_fp8: partial scratch too small (or not 16-byte aligned)");
    x.po = reinterpret_cast<float*>(partial);
    x.pml = x.po + (size_t)p->num_seqs * x.nparts * x.rows * x.c.num_kv_heads * p->head_size;
  }
  x.c.scale = p->scale * k_scale;
  x.c.v_scale = v_scale;
  hipStream_t s = (hipStream_t)stream;
  return p->kv_cache_dtype == 1 ? launch_wide_fp8_any<1>(x, p, s) : launch_wide_fp8_any<2>(x, p, s);
}
