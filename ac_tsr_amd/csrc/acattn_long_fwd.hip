// Launcher of the long-sequence forward (acattn_long_fwd.inc; one translation unit per head size:
// acattn_long_fwd_dh16.hip ... acattn_long_fwd_dh128.hip): what the form does not compute is refused here, by name.
#include "acattn_common.h"

int acattn_launch_long_fwd_dh16(const acattn_problem& p, const acattn_fwd_out& o, hipStream_t stream);
int acattn_launch_long_fwd_dh32(const acattn_problem& p, const acattn_fwd_out& o, hipStream_t stream);
int acattn_launch_long_fwd_dh64(const acattn_problem& p, const acattn_fwd_out& o, hipStream_t stream);
int acattn_launch_long_fwd_dh128(const acattn_problem& p, const acattn_fwd_out& o, hipStream_t stream);

int acattn_launch_fwd_long(const acattn_problem& p, const acattn_fwd_out& o, hipStream_t stream) {
  if (p.adversarial && !p.two_level) {
    acattn_set_error("long-sequence forward (L > 208 or ACATTN_FWD_LONG): two_level = 0 is not supported");
    return -1;
  }
  if (o.after_spatial || o.before_spatial || o.perturbed_attention || o.calibrated_attention) {
    acattn_set_error("long-sequence forward (L > 208 or ACATTN_FWD_LONG): the probability dumps (after_spatial, before_spatial, "
                     "perturbed_attention, calibrated_attention) are not supported");
    return -1;
  }
  // A_c = softmax(P exp(1 - M) + mask) and A_w take a fixed shift (the row's mask maximum): their arguments reach
  // e / (1 - p_drop), and exp overflows fp32 from p_drop = 0.967 on (a kept P = 1 entry whose M entry is dropped)
  if (p.p_drop > 0.95f) {
    acattn_set_error("long-sequence forward (L > 208 or pinned): p_drop above 0.95 is not supported");
    return -1;
  }
  // one wave per (sequence, head, query block); a sequence's rows are addressed with 32-bit byte offsets
  if ((int64_t)p.B * p.n_heads * ((p.L + 15) / 16) >= (1LL << 31) || (int64_t)(p.L + 16) * p.H * 4 >= (1LL << 31)) {
    acattn_set_error("long-sequence forward: problem too large for one launch");
    return -1;
  }
  switch (p.H / p.n_heads) {
    case 16: return acattn_launch_long_fwd_dh16(p, o, stream);
    case 32: return acattn_launch_long_fwd_dh32(p, o, stream);
    case 64: return acattn_launch_long_fwd_dh64(p, o, stream);
    case 128: return acattn_launch_long_fwd_dh128(p, o, stream);
  }
  return -1;
}
