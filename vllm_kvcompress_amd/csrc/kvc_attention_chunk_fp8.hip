// Query-block ("chunk") paged attention over an fp8 per-head cache (OCP e4m3fn or e5m2 bytes, the formats
// kvc_reshape_and_cache_fp8 writes and the decode op reads): the KVD = 1 / 2 instantiations of the two kernels of
// kvc_attention_chunk.h.  Visibility rule, softmax, metric rule and the fixed-order single add per slot are those
// of kvc_attention_chunk.hip; this file is about what an fp8 cache changes.
//
// Dequantisation rule.  Every fp8 value converts EXACTLY to fp16 and to bf16, so the tiles hold the unscaled values
// and the two scales are applied in fp32, where the kernels multiply anyway:
//     logits = (scale * k_scale) * (q . k8)              -- k_scale rides in the `sc` factor of both kernels
//     out    = v_scale * (sum p . v8) / sum p            -- v_scale rides in the final 1 / l multiply
// This is not the decode op's rule, which rounds T(float(fp8) * scale) per element on load (KvFrag<T, 1 / 2>): that
// rounding is one more error per element for scales that are not a power of two, and none of it is needed here.
// The row statistics in the workspace stay in the scaled log2 domain (max of sc * (q . k8), 1 / sum without
// v_scale), and the metric pass uses the same sc: its p = 2^(t - max) / sum is the output pass's.
//
// Output pass: a new global -> register -> LDS stage in front of the unchanged compute loop.
//   Blocks are bytes: reference K [hd/16][bs][16], V [hd][bs]; slot-major K [bs][hd], V [bs][hd]; kv_block_stride in
//   bytes.  A 32-key tile is 32 * hd bytes of K and as many of V -- HALF the HBM bytes of a 2-byte cache -- fetched
//   as 16-byte chunks in the block's own byte order (coalesced), two tiles in flight (registers hold the raw bytes
//   of tile t + 1 while tile t is computed on: 8 VGPRs instead of the 16 of the 2-byte stage).  hd 128: 256 K chunks
//   and 256 V chunks, one of each per thread.  hd 64: 128 + 128, waves 0, 1 take K and waves 2, 3 take V.
//   The bytes are converted ONCE per workgroup, on their way into the LDS (the decode kernel converts per wave and
//   per use), with v_cvt_scalef32_pk_{f16,bf16}_{fp8,bf8} and a literal 1.0 as the scale operand -- the instruction
//   takes only the exponent of that operand, so a scale must never be passed through it -- or, e5m2 -> fp16, with
//   the byte shift (e5m2 is the top byte of an fp16).  The LDS tiles are the T tiles the compute loop already reads,
//   so LDS use is that of the 2-byte kernel:
//     K chunk   16 dims 16 u .. 16 u + 15 of one key  -> units (2 u, key) and (2 u + 1, key) at p * 33 + key
//     V chunk   reference: 16 keys of one dim         -> two 16-byte stores into row d (d * 40 + key)
//               slot-major: 16 dims of one key        -> sixteen 2-byte stores, key fastest over the lanes
//   V bytes of keys at or past the tile's limit are zeroed BEFORE the conversion (byte 0 is +0 in both formats; 0 *
//   garbage could be NaN); K needs no such care (masked logits are overwritten, not multiplied).
// Metric pass: the wave's 64 keys are loaded as 8 bytes per (key, 8-dim piece p) and converted in registers --
//   reference: byte (((p >> 1) << bs_log2) + slot) * 16 + 8 * (p & 1) of the block, slot-major: slot * hd + 8 * p.
#include "kvc_attention_chunk.h"

namespace kvc {
namespace {

template <int KVD>
int launch_chunk_fp8(const ChunkArgs& a, const kvc_attention_chunk_params* p, hipStream_t s) {
  if (p->head_size == 128)
    return p->dtype == 0 ? launch_chunk<_Float16, 128, KVD>(a, p->num_seqs, p->use_l2, s)
                         : launch_chunk<__bf16, 128, KVD>(a, p->num_seqs, p->use_l2, s);
  return p->dtype == 0 ? launch_chunk<_Float16, 64, KVD>(a, p->num_seqs, p->use_l2, s)
                       : launch_chunk<__bf16, 64, KVD>(a, p->num_seqs, p->use_l2, s);
}

}  // namespace
}  // namespace kvc

extern "C" int kvc_paged_attention_chunk_fp8(const kvc_attention_chunk_params* p, float k_scale, float v_scale,
                                             kvc_stream_t stream) {
  using namespace kvc;
  if (p == nullptr) return fail_invalid("paged_attention_chunk_fp8: null params");
  if (p->kv_cache_dtype == 0)
    return fail_invalid("paged_attention_chunk_fp8: kv_cache_dtype 0 (a cache in the query's dtype) goes to "
                        "kvc_paged_attention_chunk");
  if (p->kv_cache_dtype != 1 && p->kv_cache_dtype != 2)
    return fail_invalid("Unsupported data type of kv cache: " + std::to_string(p->kv_cache_dtype));
  if (!(k_scale > 0.0f) || !(v_scale > 0.0f) || isinf(k_scale) || isinf(v_scale))        // (NaN fails the first two)
    return fail_invalid("paged_attention_chunk_fp8: k_scale and v_scale must be finite and > 0");
  ChunkArgs a;
  int rc = KVC_OK;
  if (!chunk_prepare(p, 16, a, &rc)) return rc;
  a.scale = p->scale * k_scale;
  a.v_scale = v_scale;
  hipStream_t s = (hipStream_t)stream;
  return p->kv_cache_dtype == 1 ? launch_chunk_fp8<1>(a, p, s) : launch_chunk_fp8<2>(a, p, s);
}
