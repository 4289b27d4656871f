// The short schedule of the query-block attention (kvc_attention_chunk_short.hip) over an fp8 per-head cache (OCP
// e4m3fn or e5m2 bytes): the KVD = 1 / 2 instantiations of kvc_attention_chunk_short.h.  Schedule, softmax, the merge
// of the waves, the partial scratch and the combine kernel are those of the 2-byte kernel; the dequantisation rule is
// the fp8 tile path's (kvc_attention_chunk_fp8.hip): bytes convert EXACTLY to the query's dtype (cvt8x4 / cvt8x8, a
// literal 1.0 through v_cvt_scalef32_pk_*), k_scale rides in sc = scale * k_scale * log2(e), v_scale in the final
// 1 / l multiply -- of the single-partition epilogue and of the combine kernel -- and the statistics in the workspace
// and in the partial scratch stay in the scaled log2 domain without v_scale, so chunk_metric_kernel<.., KVD> behind
// it recomputes the same p.
//
// What an fp8 block changes is the geometry of a wave's 32-key step, which is read from global memory in operand
// form, one step ahead.  Lane (c, g) = (lane & 15, lane >> 4); an MFMA A operand is 8 elements of row c, k-index
// 8 g .. 8 g + 7.  Per lane and step at hd 128 (hd 64: half of everything):
//
//   reference K [hd/16][bs][16]   The order in which QK^T contracts the dims is free as long as Q matches, so a lane
//     reads whole 16-byte pieces -- piece g + 4 x of its key, x < hd / 64 -- and feeds the two halves to k-steps 2 x and
//     2 x + 1: k-step ks contracts dims 16 (g + 4 (ks / 2)) + 8 (ks % 2) .. of lane group g, and bq[][ks] is loaded
//     from exactly there.  2 x 2 global_load_dwordx4 instead of 2 x 4 dwordx2; 16 lanes cover 256 contiguous bytes.
//   reference V [hd][bs]          Which key sits in which A row of QK^T is free as well.  Row c of half h is key
//     8 (c / 4) + 4 h + c % 4, so lane (c, g) ends with the weights of the 8 CONSECUTIVE keys 8 g .. 8 g + 7 (j-th
//     weight = key 8 g + j) and the P.V operand of dim 16 dt + c is ONE 8-byte read, 8 per step, not 16 4-byte ones
//     (8 keys never straddle a block).  The price: with bs 16 the 16 rows of a half lie in two blocks, the block
//     table entry is the lane's own.  The causal mask and the zeroing use the same numbering (key_of).
//   slot-major K [bs][hd]         A 16-key tile is 16 * hd contiguous bytes: 2 (hd 64: 1) dwordx4 per lane, parked RAW
//     in the wave's LDS tile and converted after the read-back.  Converting first would double the LDS bytes written,
//     read and held for the same number of conversions (a wave reads every byte of its tile back exactly once).  The
//     read-back is the reference trick again: unit g + 4 x of row c, both halves used, the same bq numbering.
//     Swizzle: 16-byte unit j of key row k is stored at unit j ^ ((k / (256 / hd)) % (hd / 16)).  hd 128: rows of 8
//     units, two rows per 256 bytes, XOR with (k / 2) % 8; hd 64: rows of 4 units, four rows per 256 bytes, XOR with
//     (k / 4) % 4.  A ds_write_b128 group of 16 lanes writes 16 consecutive units of the tile (a permutation within
//     each row): 256 contiguous bytes, every bank once.  A ds_read_b128 group (c = 0 .. 15, one g, one x) reads unit
//     (g + 4 x) ^ swz(c) of row c: the 256 / hd rows that share a 256-byte line differ in c % (256 / hd) -- distinct
//     line parts --, the rows c / (256 / hd) = 0 .. hd / 16 - 1 get distinct XORs -- distinct units: every bank once.
//     Wave barriers only.
//   slot-major V [bs][hd]         Rows are keys 16 h + c as over 2-byte caches (keys 4 g + i and 16 + 4 g + i per lane).
//     Lane (c, g) reads the hd / 16 bytes (dims (hd / 16) c ..) of each of its 8 keys: 8 dwordx2 (hd 64: 8 dword).
//     Operands: convert first -- per dword of every key two packed converts leave the pairs (dim, dim + 1), then one
//     v_perm_b32 per operand dword joins two keys of one dim (the 2-byte kernel's selectors).  1 convert + 1 perm per
//     operand dword; gathering bytes first (4 x 4 byte transposes, 8 perms per 4 dwords) costs the same and needs more
//     selectors.
//   V bytes of keys at or past the head's largest limit are zero before the conversion (byte 0 is +0 in both
//   formats): never loaded, or masked in the one read that straddles the limit.  K needs no care.
//
// Registers.  A raw step is 16 K + 16 V dwords (hd 128), half the 2-byte kernel's, so K AND V of the next step run
// ahead in every instantiation -- also NT = 2 at hd 128, where the 2-byte kernel prefetches K only (reference) or
// nothing (slot-major).  P.V runs with the dim tile outside and the row tile inside: one converted V operand (4
// dwords) is alive at a time and serves both row tiles.  All 32 instantiations: 2 waves per SIMD, no scratch (the
// VGPR counts are in DESIGN.md 3.8).
#include "kvc_attention_chunk_short.h"

extern "C" int32_t kvc_paged_attention_chunk_short_fp8_eligible(int32_t num_heads, int32_t num_kv_heads, int32_t max_query_len,
                                                                int32_t kv_cache_dtype) {
  return (kv_cache_dtype == 1 || kv_cache_dtype == 2) && kvc::short_rows_ok(num_heads, num_kv_heads, max_query_len) ? 1 : 0;
}

extern "C" int kvc_paged_attention_chunk_short_fp8(const kvc_attention_chunk_params* p, float k_scale, float v_scale,
                                                   void* partial, size_t partial_bytes, kvc_stream_t stream) {
  using namespace kvc;
  if (p == nullptr) return fail_invalid("paged_attention_chunk_short_fp8: null params");
  if (p->kv_cache_dtype == 0)
    return fail_invalid("paged_attention_chunk_short_fp8: kv_cache_dtype 0 (a cache in the query's dtype) goes to "
                        "kvc_paged_attention_chunk_short");
  if (p->kv_cache_dtype != 1 && p->kv_cache_dtype != 2)
    return fail_invalid("Unsupported data type of kv cache: " + std::to_string(p->kv_cache_dtype));
  if (!(k_scale > 0.0f) || !(v_scale > 0.0f) || isinf(k_scale) || isinf(v_scale))        // (NaN fails the first two)
    return fail_invalid("paged_attention_chunk_short_fp8: k_scale and v_scale must be finite and > 0");
  ShortArgs x;
  int rc = KVC_OK;
  if (!short_prepare(p, 16, partial, partial_bytes, "paged_attention_chunk_short_fp8", x, &rc)) return rc;
  x.c.scale = p->scale * k_scale;
  x.c.v_scale = v_scale;
  hipStream_t s = (hipStream_t)stream;
  return p->kv_cache_dtype == 1 ? launch_short_any<1>(x, p, s) : launch_short_any<2>(x, p, s);
}
