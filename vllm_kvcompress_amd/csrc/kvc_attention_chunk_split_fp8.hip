// The split schedule of the query-block attention (kvc_attention_chunk_split.hip) over an fp8 per-head cache (OCP
// e4m3fn or e5m2 bytes): the KVD = 1 / 2 instantiations of kvc_attention_chunk_split.h, reached through the one entry
// kvc_paged_attention_chunk_split.  Schedule, partition rule, partial scratch and combine kernel are those of the 2-byte
// kernels; the stage in front of the compute loop and the dequantisation rule are the fp8 tile path's
// (kvc_attention_chunk_fp8.hip): raw bytes in 16-byte chunks in the block's own order, one K and one V chunk per thread
// at hd 128 (hd 64: waves 0, 1 take K, waves 2, 3 take V), converted EXACTLY to the query's dtype once per workgroup on
// the way into the LDS; k_scale rides in sc = scale * k_scale * log2(e), v_scale in the combine kernel's final 1 / l
// multiply, and the partials and the row statistics stay in the scaled log2 domain without v_scale, so
// chunk_metric_kernel<.., KVD> behind it recomputes the same p.  A partition below the tile's smallest limit skips the
// byte masks of the V fetch together with the compares.
#include "kvc_attention_chunk_split.h"

int kvc::launch_split_fp8(const void* split_args, const kvc_attention_chunk_params* p, hipStream_t s) {
  const SplitArgs& x = *static_cast<const SplitArgs*>(split_args);
  return p->kv_cache_dtype == 1 ? launch_split_any<1>(x, p, s) : launch_split_any<2>(x, p, s);
}
