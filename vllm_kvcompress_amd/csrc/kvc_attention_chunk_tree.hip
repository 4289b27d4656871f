// Draft-TREE verification on the key-split schedules of the query-block attention (F5): the TREE variants of the short
// and wide output kernels and of the row-form metric kernel.  The chain kernels hard-wire one visibility rule -- token
// j sees slots i < ctx - (nq - 1 - j) --, which serves a linear draft.  A token tree (Medusa, EAGLE, SpecInfer) verifies
// in one call new tokens that see the whole cached prefix but, among the new tokens, only their own ancestors; with
// the chain rule a caller runs one call per root-to-leaf path, and each re-reads the context the key-split schedules
// were built to read once.
//
// Rule.  tree_mask holds one 64-bit word per query token.  For (sequence s, KV head h) base = context_lens[s, h] - nq_s,
// signed; slot i < context_lens[s, h] has e = i - base; token t sees it iff e < 0, or bit e of tree_mask[t] is set.  No
// bit is implied (a token that sees itself has its own bit), bits from nq_s up are ignored, and the chain is the mask
// (1 << (j + 1)) - 1 of token j.  Everything else is F5's text: a row that sees nothing is 0, plain softmax in fp32,
// one rounding, the metric rule with "sees" read as above.
//
// What the variants change -- `bool TREE` of chunk_short_kernel, of both chunk_wide_kernel and of
// chunk_metric_rows_kernel, under if constexpr, with an argument block of their own (ShortTreeArgs /
// MetricRowsTreeArgs), so that the chain instantiations compile to what they compiled to before:
//   key loop  Every row sees the whole prefix and the rows differ on the last nq <= 64 slots only, so a 32-key step is
//             masked iff k0 + 32 > base: at most three steps per head, in its last one or two partitions; every step
//             in front of them runs without a compare.  The head's largest limit is context_lens itself: partition
//             skipping, part_end and the zeroing of V past it are the chain's.
//   words     short kernel: a lane keeps the word of its row 16 nt + c in two VGPRs per row tile, where the chain keeps
//             lim[nt]; padding rows hold 0.  Wide kernels: a uint64 tile in the LDS where the chain keeps slim[], read
//             on masked steps only.  A lane's 8 keys of a step lie within 20 slots: tree_window (kvc_attention_chunk.h)
//             makes the visibility of 32 consecutive slots from e0 = the lane's first key - base with one 64-bit shift
//             -- ones below e = 0, the word's bits (those from nq up cleared when loaded), zeros from 64 -- and the
//             test of weight j is a constant bit of it.  Shift amounts are masked behind the compares that bound them.
//   combine   unchanged: chunk_short_combine_kernel merges ceil(context_lens / PL) partitions for every row already,
//             and the partial of a partition a row saw nothing of is (m, l, O) = (-inf, 0, 0) -- its factor is
//             2^(-inf - ms) = 0 against a finite ms, and a row that saw nothing anywhere gets ms = 0, l = 0, out 0.
//             Within a partition a step a row sees nothing of leaves its (m, l, O) alone (alpha = 1, every p = 0).
//   metric    chunk_metric_rows_kernel<.., TREE>: the lane keeps base (padding rows: a base that puts every key past
//             the word) and the row's word where the chain keeps vis[nt]; the wave-uniform skip of a (row tile, 16-key
//             half) asks the OR of the tile's words where the chain asks the tile's largest limit.  pass = sees &&
//             window; `touched` follows from the same test, so a draft slot no row sees is not written.  The window
//             test uses the positions the caller passes: for a tree, depths.
// The entry runs the output pass without metrics and, when p->metrics is set, the TREE row-form metric kernel behind
// it on the same stream; the tile-form metric kernel has no tree variant.
// This file holds the instantiations over caches in the query's dtype; kvc_attention_chunk_tree_fp8.hip the fp8 ones.
#include "kvc_attention_chunk_wide.h"
#include "kvc_attention_chunk_tree.h"

namespace kvc {
namespace {

template <typename T, int HD>
int launch_tree_2b(const ShortTreeArgs& x, const MetricRowsTreeArgs& m, int num_seqs, hipStream_t s) {
  return launch_tree<T, HD, 0>(x, m, num_seqs, s, [&](const dim3& grid) {
    const bool four = x.rows > 48;
    if (x.c.slot_major) {
      if (four) hipLaunchKernelGGL((chunk_wide_kernel<T, HD, 4, true, true>), grid, dim3(256), 0, s, x);
      else hipLaunchKernelGGL((chunk_wide_kernel<T, HD, 3, true, true>), grid, dim3(256), 0, s, x);
    } else {
      if (four) hipLaunchKernelGGL((chunk_wide_kernel<T, HD, 4, false, true>), grid, dim3(256), 0, s, x);
      else hipLaunchKernelGGL((chunk_wide_kernel<T, HD, 3, false, true>), grid, dim3(256), 0, s, x);
    }
  });
}

}  // namespace
}  // namespace kvc

extern "C" int32_t kvc_paged_attention_chunk_tree_eligible(int32_t num_heads, int32_t num_kv_heads, int32_t max_query_len) {
  return kvc::tree_rows_ok(num_heads, num_kv_heads, max_query_len) ? 1 : 0;
}

extern "C" int kvc_paged_attention_chunk_tree(const kvc_attention_chunk_params* p, const uint64_t* tree_mask, float k_scale,
                                              float v_scale, void* partial, size_t partial_bytes, kvc_stream_t stream) {
  using namespace kvc;
  if (p == nullptr) return fail_invalid("paged_attention_chunk_tree: null params");
  hipStream_t s = (hipStream_t)stream;
  if (p->kv_cache_dtype == 1 || p->kv_cache_dtype == 2)
    return chunk_tree_fp8(p, tree_mask, k_scale, v_scale, partial, partial_bytes, s);
  ShortTreeArgs x;
  MetricRowsTreeArgs m;
  int rc = KVC_OK;
  if (!tree_prepare(p, tree_mask, k_scale, v_scale, partial, partial_bytes, x, m, &rc)) return rc;
  if (p->head_size == 128)
    return p->dtype == 0 ? launch_tree_2b<_Float16, 128>(x, m, p->num_seqs, s) : launch_tree_2b<__bf16, 128>(x, m, p->num_seqs, s);
  return p->dtype == 0 ? launch_tree_2b<_Float16, 64>(x, m, p->num_seqs, s) : launch_tree_2b<__bf16, 64>(x, m, p->num_seqs, s);
}
