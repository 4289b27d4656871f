// The TREE variants (kvc_attention_chunk_tree.hip: the rule, which steps mask, where the mask words live) over an fp8
// per-head cache (OCP e4m3fn or e5m2 bytes), both block layouts: the KVD = 1 / 2 instantiations of the short kernel,
// of the fp8 wide kernel and of the row-form metric kernel with TREE set.  Byte geometry, dequantisation rule and
// prefetch depths are those of the chain kernels (kvc_attention_chunk_short_fp8.hip, kvc_attention_chunk_wide_fp8.hip,
// kvc_attention_chunk_metric_rows_fp8.hip); the fp8 output kernels number the keys of a lane's weights by key_of, and
// the tree test runs on the same numbering: weight j is the new slot k0 + key_of(j) - base.
#include "kvc_attention_chunk_wide_fp8.h"
#include "kvc_attention_chunk_tree.h"

namespace kvc {
namespace {

template <typename T, int HD, int KVD>
int launch_tree_fp8(const ShortTreeArgs& x, const MetricRowsTreeArgs& m, int num_seqs, hipStream_t s) {
  return launch_tree<T, HD, KVD>(x, m, num_seqs, s, [&](const dim3& grid) {
    const bool four = x.rows > 48;
    if (x.c.slot_major) {
      if (four) hipLaunchKernelGGL((chunk_wide_kernel<T, HD, 4, true, KVD, true>), grid, dim3(256), 0, s, x);
      else hipLaunchKernelGGL((chunk_wide_kernel<T, HD, 3, true, KVD, true>), grid, dim3(256), 0, s, x);
    } else {
      if (four) hipLaunchKernelGGL((chunk_wide_kernel<T, HD, 4, false, KVD, true>), grid, dim3(256), 0, s, x);
      else hipLaunchKernelGGL((chunk_wide_kernel<T, HD, 3, false, KVD, true>), grid, dim3(256), 0, s, x);
    }
  });
}

template <int KVD>
int launch_tree_fp8_any(const ShortTreeArgs& x, const MetricRowsTreeArgs& m, const kvc_attention_chunk_params* p, hipStream_t s) {
  if (p->head_size == 128)
    return p->dtype == 0 ? launch_tree_fp8<_Float16, 128, KVD>(x, m, p->num_seqs, s)
                         : launch_tree_fp8<__bf16, 128, KVD>(x, m, p->num_seqs, s);
  return p->dtype == 0 ? launch_tree_fp8<_Float16, 64, KVD>(x, m, p->num_seqs, s)
                       : launch_tree_fp8<__bf16, 64, KVD>(x, m, p->num_seqs, s);
}

}  // namespace
}  // namespace kvc

int kvc::chunk_tree_fp8(const kvc_attention_chunk_params* p, const uint64_t* tree_mask, float k_scale, float v_scale,
                        void* partial, size_t partial_bytes, hipStream_t s) {
  ShortTreeArgs x;
  MetricRowsTreeArgs m;
  int rc = KVC_OK;
  if (!tree_prepare(p, tree_mask, k_scale, v_scale, partial, partial_bytes, x, m, &rc)) return rc;
  return p->kv_cache_dtype == 1 ? launch_tree_fp8_any<1>(x, m, p, s) : launch_tree_fp8_any<2>(x, m, p, s);
}
