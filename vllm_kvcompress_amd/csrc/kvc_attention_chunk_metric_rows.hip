// The metric pass of the query-block attention in "row form", for at most 64 (token, query head) rows per KV head:
// what chunk_metric_kernel (kvc_attention_chunk.hip) adds to the metric store, by a kernel whose MFMA tiles are full
// at the shapes the short and wide schedules serve.  chunk_metric_kernel's row tile is 16 tokens of ONE query head:
// verifying 4 draft tokens at 4 query heads per KV head it runs 4 tiles with 4 of 16 rows alive.  Here the N dimension
// of the MFMA is the row r = token * qpk + query head, as in the short and wide output kernels, so those 16 rows are
// one tile.  The rule is unchanged: p = 2^(sc (q . k) - m_r) / l_r from the row statistics every output pass leaves in
// the workspace, summed (p^2 or p) per slot over the rows that see the slot and whose metric window holds its
// position; one fp32 add per reached slot, no atomics, slots no row reaches are not written.
//
//  chunk_metric_rows_kernel<T, HD, NT, SM, KVD>, NT = 2 or 4 row tiles, grid (key partition of MPL slots, KV head,
//  sequence), 256 threads, no LDS, no barrier.
//  Work split.  The four waves take the partition's 32-key steps in turn; a wave reads the K of a step once for ALL
//  rows of the head, so every K byte is requested by exactly one wave of one workgroup per call.  S^T = K Q^T on
//  v_mfma_f32_16x16x32 (M = 16 keys, N = 16 rows, K = 32 dims), two 16-key halves per step: lane (c, g) = (lane & 15,
//  lane >> 4) holds, per row tile, keys 16 h + 4 g + i of row c.  A slot's sum is finished inside its step: the lane
//  adds its row tiles in ascending order, then the 16 lanes of a group (the 16 rows of the tiles) are reduced by a
//  fixed reduce-scatter -- 4 + 2 + 1 + 1 shuffles for the lane's 8 keys where a butterfly per value takes 32 -- and
//  lane c = 2 j of the group makes the single add for key j.  The order depends on the rows alone, not on the batch
//  and not on the partition length (steps start at multiples of 32 whatever MPL is).
//  Data movement.  Q (NT x HD / 32 operands), the statistics (m, 1 / l), the causal limit and the window bound
//  qpos - buflen of the lane's NT rows live in registers for the whole partition; padding rows have zero Q and limit
//  0.  K goes from global memory straight into the MFMA operand registers, as 16-byte pieces, in every layout --
//  reference K [hd/8][bs][8]: 16 lanes read 256 consecutive bytes of a piece row; slot-major [bs][hd]: the four lane
//  groups read 64 consecutive bytes of a key's row and the reads of a half consume every byte of the 16 rows -- and the
//  next step's K and the kv_position of its 8 result keys are requested before the current step is computed.
//  Skipping.  Steps at or past the head's largest limit, row tiles whose largest limit is at or below the half's first
//  key (wave-uniform; the tiles of padding rows always), sequences without new tokens.
// MPL = metric_rows_partition(max_context_len, KV heads x sequences): 256 .. 4096 slots, chosen to fill the device.
#include "kvc_attention_chunk_metric_rows.h"

extern "C" int kvc_paged_attention_chunk_metric_rows(const kvc_attention_chunk_params* p, float k_scale, kvc_stream_t stream) {
  using namespace kvc;
  if (p == nullptr) return fail_invalid("paged_attention_chunk_metric_rows: null params");
  hipStream_t s = (hipStream_t)stream;
  if (p->kv_cache_dtype == 1 || p->kv_cache_dtype == 2) return chunk_metric_rows_fp8(p, k_scale, s);
  MetricRowsArgs x;
  int rc = KVC_OK;
  if (!metric_rows_prepare(p, k_scale, x, &rc)) return rc;
  return launch_metric_rows_any<0>(x, p, s);
}
