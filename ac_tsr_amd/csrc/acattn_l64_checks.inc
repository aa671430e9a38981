// The host-side limits the two L <= 64 cores without re-normalisation share (include/acattn.h), each answering the first
// limit a call breaks as a string literal, or NULL.  The including file defines ACATTN_L64_WHAT, the name its messages
// start with, and runs its own conditions behind these.
#ifndef ACATTN_L64_WHAT
#error "define ACATTN_L64_WHAT before including acattn_l64_checks.inc"
#endif

namespace {

// the configuration ...
const char* l64_config(const acattn_problem& p) {
  if (p.B < 1 || p.L < 1 || p.H < 1 || p.n_heads < 1 || p.H % p.n_heads != 0) return ACATTN_L64_WHAT ": B, L, H, n_heads must be positive and H a multiple of n_heads";
  if (p.L > 64) return ACATTN_L64_WHAT ": sequence length L must be <= 64";
  if (p.H / p.n_heads != 16 && p.H / p.n_heads != 32 && p.H / p.n_heads != 64) return ACATTN_L64_WHAT ": head size must be 16, 32 or 64";
  if (!p.adversarial) return ACATTN_L64_WHAT ": needs the adversarial calibrator (adversarial = 1)";
  if (p.combine_option != ACATTN_COMBINE_GATE) return ACATTN_L64_WHAT ": combine_option must be gate (fixed / annealing are not built)";
  if (!p.two_level) return ACATTN_L64_WHAT ": two_level must be 1 (the one-level form is not built)";
  if (p.mask_mode != ACATTN_MASK_STRUCTURED) return ACATTN_L64_WHAT ": the mask must be structured (key_valid + causal); dense masks are not built";
  if (p.rng_mode != ACATTN_RNG_EXPLICIT && p.rng_mode != ACATTN_RNG_COUNTER) return ACATTN_L64_WHAT ": unknown rng_mode";
  if (!(p.p_drop >= 0.f && p.p_drop < 1.f)) return ACATTN_L64_WHAT ": p_drop must lie in [0, 1)";
  return nullptr;
}

// ... and the 32-bit element offsets of the kernels
const char* l64_sizes(const acattn_problem& p) {
  if ((int64_t)p.B * p.n_heads * p.L * p.L >= (1LL << 31) || (int64_t)p.B * p.L * p.H >= (1LL << 31)) return ACATTN_L64_WHAT ": tensors of 2^31 elements or more";
  return nullptr;
}

const char* l64_pointers(const acattn_problem& p) {
  if (!p.q || !p.k || !p.v || !p.qa || !p.ka) return ACATTN_L64_WHAT ": q, k, v, qa, ka must be non-NULL";
  if (!p.gate_logits) return ACATTN_L64_WHAT ": combine_option gate needs gate_logits";
  if (!p.key_valid) return ACATTN_L64_WHAT ": structured mask needs key_valid";
  if (!p.w_order || !p.b_order || !p.w_dist || !p.b_dist || !p.scalar) return ACATTN_L64_WHAT ": both spatial terms must be present (order and distance affines, scalar)";
  if (p.rng_mode == ACATTN_RNG_EXPLICIT) {
    if (!p.noise) return ACATTN_L64_WHAT ": explicit rng mode needs noise";
    if (p.p_drop > 0.f && (!p.keep_after || !p.keep_mask)) return ACATTN_L64_WHAT ": explicit dropout needs keep_after and keep_mask";
  }
  return nullptr;
}

const char* l64_fwd_out(const acattn_fwd_out& o) {
  if (!o.ctx_attacked || !o.ctx_calibrated || !o.attack_mask) return ACATTN_L64_WHAT " forward: ctx_attacked, ctx_calibrated and attack_mask must be non-NULL";
  if (o.after_spatial || o.before_spatial || o.perturbed_attention || o.calibrated_attention) return ACATTN_L64_WHAT " forward: the probability dumps are not built";
  return nullptr;
}

const char* l64_bwd_io(const acattn_problem& p, const acattn_bwd_io& io) {
  if (!io.row_stats || !io.attack_mask) return ACATTN_L64_WHAT " backward: needs the forward's attack_mask and row_stats";
  if (!io.dq || !io.dk || !io.dv || !io.dqa || !io.dka) return ACATTN_L64_WHAT " backward: dq, dk, dv, dqa, dka must be non-NULL";
  if (!io.dgate_logits) return ACATTN_L64_WHAT " backward: gate combine needs dgate_logits";
  if (!io.dw_order_part || !io.dw_dist_part || !io.dsmall_part) return ACATTN_L64_WHAT " backward: parameter partial buffers must be non-NULL";
  if (io.part_stride != 0 && io.part_stride < 2 * (p.H / p.n_heads)) return ACATTN_L64_WHAT " backward: part_stride is smaller than a partial row";
  if (io.dgate_summed) return ACATTN_L64_WHAT " backward: dgate_summed is not built (per-head partials only)";
  if (io.dqa2 || io.dka2 || io.d_ctx_calibrated2 || io.d_penalty_part2) return ACATTN_L64_WHAT " backward: the second cotangent set is not built";
  return nullptr;
}

}  // namespace
