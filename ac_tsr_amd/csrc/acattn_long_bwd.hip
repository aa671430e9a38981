// Launcher of the long-sequence backward (acattn_long_bwd.inc; one translation unit per head size:
// acattn_long_bwd_dh16.hip ... acattn_long_bwd_dh128.hip): what the form does not compute is refused here, by name.
#include "acattn_common.h"

int acattn_launch_long_bwd_dh16(const acattn_problem& p, const acattn_bwd_io& io, hipStream_t stream);
int acattn_launch_long_bwd_dh32(const acattn_problem& p, const acattn_bwd_io& io, hipStream_t stream);
int acattn_launch_long_bwd_dh64(const acattn_problem& p, const acattn_bwd_io& io, hipStream_t stream);
int acattn_launch_long_bwd_dh128(const acattn_problem& p, const acattn_bwd_io& io, hipStream_t stream);

// The hints of acattn_bwd_io (active_qblocks, read_rows, attack_only) are ignored: every output is written in full.
int acattn_launch_bwd_long(const acattn_problem& p, const acattn_bwd_io& io, hipStream_t stream) {
  if (!p.two_level) {
    acattn_set_error("long-sequence backward (L > 208 or ACATTN_BWD_LONG): two_level = 0 is not supported");
    return -1;
  }
  if (!io.workspace) {
    acattn_set_error("long-sequence backward (L > 208 or ACATTN_BWD_LONG): workspace must be non-NULL "
                     "(acattn_calibrated_attention_bwd_workspace_bytes)");
    return -1;
  }
  if (io.dgate_summed || io.dqa2 || io.dka2 || io.d_ctx_calibrated2 || io.d_penalty_part2) {
    acattn_set_error("long-sequence backward (L > 208 or ACATTN_BWD_LONG): dgate_summed and the second cotangent set "
                     "(dqa2, dka2) are not supported");
    return -1;
  }
  // A_c = softmax(P exp(1 - M) + mask) and A_w take a fixed shift (the row's mask maximum): their arguments reach
  // e / (1 - p_drop), and exp overflows fp32 from p_drop = 0.967 on (a kept P = 1 entry whose M entry is dropped)
  if (p.p_drop > 0.95f) {
    acattn_set_error("long-sequence backward (L > 208 or pinned): p_drop above 0.95 is not supported");
    return -1;
  }
  // one wave per (sequence, head, block of 16); grid and in-sequence offsets are 32-bit
  if ((int64_t)p.B * p.n_heads * ((p.L + 15) / 16) >= (1LL << 31) || (int64_t)(p.L + 16) * p.H * 4 >= (1LL << 31)) {
    acattn_set_error("long-sequence backward: problem too large for one launch");
    return -1;
  }
  switch (p.H / p.n_heads) {
    case 16: return acattn_launch_long_bwd_dh16(p, io, stream);
    case 32: return acattn_launch_long_bwd_dh32(p, io, stream);
    case 64: return acattn_launch_long_bwd_dh64(p, io, stream);
    case 128: return acattn_launch_long_bwd_dh128(p, io, stream);
  }
  return -1;
}
