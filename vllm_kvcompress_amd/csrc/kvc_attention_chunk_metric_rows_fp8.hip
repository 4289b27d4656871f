// The row-form metric pass (kvc_attention_chunk_metric_rows.hip) over an fp8 per-head cache (OCP e4m3fn or e5m2
// bytes), both block layouts: the KVD = 1 / 2 instantiations of chunk_metric_rows_kernel.  Dequantisation rule of the
// other fp8 chunk paths (kvc_attention_chunk_fp8.hip): the bytes convert EXACTLY to the query's dtype (cvt8x8), k_scale
// rides in sc = scale * k_scale * log2(e) -- the domain of the statistics in the workspace -- and v_scale has no part
// in the metric.
//  K    a lane reads whole 16-byte pieces, 16 dims of its key -- reference [hd/16][bs][16]: piece g + 4 x, 16 lanes read
//       256 consecutive bytes of a piece row; slot-major [bs][hd]: byte 16 (g + 4 x) of the key's row, the four lane
//       groups read 64 consecutive bytes -- and cvt8x8 makes the operands of k-steps 2 x and 2 x + 1 from its halves.
//       A raw step is half the registers of a 2-byte step (hd 128: 16 dwords).
//  Q    k-step ks of lane group g contracts dims 16 (g + 4 (ks / 2)) + 8 (ks % 2) .. (the fp8 short kernel's numbering).
//  MFMA row c of half h is key 16 h + c as over 2-byte caches: the fp8 output kernels number the rows so that a lane's
//  8 weights belong to 8 consecutive keys for the V read-out; there is no V here.
#include "kvc_attention_chunk_metric_rows.h"

int kvc::chunk_metric_rows_fp8(const kvc_attention_chunk_params* p, float k_scale, hipStream_t s) {
  MetricRowsArgs x;
  int rc = KVC_OK;
  if (!metric_rows_prepare(p, k_scale, x, &rc)) return rc;
  return p->kv_cache_dtype == 1 ? launch_metric_rows_any<1>(x, p, s) : launch_metric_rows_any<2>(x, p, s);
}
