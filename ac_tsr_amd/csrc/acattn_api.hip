// C-ABI entry points of libacattn.so (include/acattn.h): argument validation, dispatch, error text.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "acattn_common.h"

namespace {
thread_local char g_err[256] = "";
// 31 key tiles of 16: the long forms (acattn_long_fwd.inc, acattn_long_bwd.inc) loop over tiles at run time and would take
// more; the ceiling is this validation's alone
constexpr int ACATTN_MAX_L = 496;

int fail(const char* msg) {
  snprintf(g_err, sizeof(g_err), "%s", msg);
  return -1;
}

int check_problem(const acattn_problem* p) {
  if (!p) return fail("problem is NULL");
  if (p->B < 1 || p->L < 1 || p->H < 1 || p->n_heads < 1) return fail("B, L, H, n_heads must be positive");
  if (p->H % p->n_heads != 0)
    return fail("The hidden size is not a multiple of the number of attention heads");  // layers.py:618-622
  const int dh = p->H / p->n_heads;
  if (dh != 16 && dh != 32 && dh != 64 && dh != 128) return fail("unsupported head size: dh must be 16, 32, 64 or 128");
  if (p->L > ACATTN_MAX_L) return fail("unsupported sequence length: L must be <= 496 (acattn_max_sequence_length)");
  if (!p->q || !p->k || !p->v) return fail("q, k, v must be non-NULL");
  if (p->mask_mode == ACATTN_MASK_STRUCTURED) {
    if (!p->key_valid) return fail("structured mask needs key_valid");
  } else if (p->mask_mode == ACATTN_MASK_DENSE_LL || p->mask_mode == ACATTN_MASK_DENSE_L) {
    if (!p->mask) return fail("dense mask mode needs mask");
  } else {
    return fail("unknown mask_mode");
  }
  if (p->w_order && !p->b_order) return fail("w_order given without b_order");
  if (p->w_dist && (!p->b_dist || !p->scalar)) return fail("w_dist given without b_dist / scalar");
  if (p->p_drop < 0.f || p->p_drop >= 1.f) return fail("p_drop must lie in [0, 1)");
  if (p->rng_mode != ACATTN_RNG_EXPLICIT && p->rng_mode != ACATTN_RNG_COUNTER) return fail("unknown rng_mode");
  if (p->rng_mode == ACATTN_RNG_EXPLICIT && p->p_drop > 0.f) {
    if (!p->keep_after) return fail("explicit dropout needs keep_after");
    if (p->adversarial && !p->keep_mask) return fail("explicit dropout needs keep_mask");
    if (p->adversarial && !p->two_level && !p->keep_before) return fail("explicit dropout needs keep_before");
  }
  if (p->adversarial) {
    if (!p->qa || !p->ka) return fail("adversarial calibrator needs qa and ka");
    if (p->rng_mode == ACATTN_RNG_EXPLICIT && !p->noise) return fail("explicit rng mode needs noise");
    if (p->combine_option == ACATTN_COMBINE_GATE) {
      if (!p->gate_logits) return fail("combine_option gate needs gate_logits");
    } else if (p->combine_option != ACATTN_COMBINE_FIXED && p->combine_option != ACATTN_COMBINE_ANNEALING) {
      return fail("unknown combine_option");  // layers.py:894-895 raises KeyError
    }
    if (!p->two_level) {
      if (p->rich_combine != ACATTN_RICH_FIXED && p->rich_combine != ACATTN_RICH_TRAINABLE)
        return fail("unknown rich_calibrated_combine");  // layers.py:935-936 raises KeyError
      if (p->rich_combine == ACATTN_RICH_TRAINABLE && !p->rich_ratio) return fail("trainable rich combine needs rich_ratio");
    }
  }
  return 0;
}
}  // namespace

void acattn_set_error(const char* msg) { snprintf(g_err, sizeof(g_err), "%s", msg); }

int acattn_launch_bwd_attack(const acattn_problem& p, const acattn_bwd_io& io, hipStream_t stream, float* gate_zero);  // acattn_bwd_attack.hip

// acattn_unnorm.hip: the un-normalised core of ACSSEPT (validation included: they set the error text themselves)
int acattn_unnorm_supported(const acattn_problem& p);
int acattn_launch_unnorm_fwd(const acattn_problem& p, const acattn_fwd_out& o, hipStream_t stream);
int acattn_launch_unnorm_bwd(const acattn_problem& p, const acattn_bwd_io& io, hipStream_t stream);

// acattn_timeaware.hip: the time-interval core of ACTiSASRec (validation included, as above)
int acattn_timeaware_supported(const acattn_problem& p, const acattn_time_ext& t, const char** why);
int acattn_launch_timeaware_fwd(const acattn_problem& p, const acattn_time_ext& t, const acattn_fwd_out& o, hipStream_t stream);
int acattn_launch_timeaware_bwd(const acattn_problem& p, const acattn_time_ext& t, const acattn_bwd_io& io,
                                const acattn_time_grads& g, hipStream_t stream);
int acattn_launch_time_rng(int B, int L, int H, uint64_t seed, float p, uint8_t* keep_k, uint8_t* keep_v, hipStream_t stream);

extern "C" {

int acattn_abi_version(void) { return ACATTN_ABI_VERSION; }

int acattn_timeaware_attention_supported(const acattn_problem* p, const acattn_time_ext* t) {
  if (!p || !t) return 0;
  const char* why = nullptr;
  const int ok = acattn_timeaware_supported(*p, *t, &why);
  if (!ok) snprintf(g_err, sizeof(g_err), "%s", why);
  return ok;
}

int acattn_timeaware_attention_fwd(const acattn_problem* p, const acattn_time_ext* t, const acattn_fwd_out* out, void* stream) {
  if (!p || !t || !out) return fail("problem, time and out must be non-NULL");
  int rc = acattn_launch_timeaware_fwd(*p, *t, *out, (hipStream_t)stream);
  if (rc == 0 && out->penalty_part)
    rc = acattn_launch_penalty_rows(out->attack_mask, p->B, p->n_heads, p->L, out->penalty_part, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_timeaware_attention_bwd(const acattn_problem* p, const acattn_time_ext* t, const acattn_bwd_io* io,
                                   const acattn_time_grads* grads, void* stream) {
  if (!p || !t || !io || !grads) return fail("problem, time, io and grads must be non-NULL");
  const int rc = acattn_launch_timeaware_bwd(*p, *t, *io, *grads, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_time_rng_materialize(int32_t B, int32_t L, int32_t H, uint64_t seed, float p, uint8_t* keep_k, uint8_t* keep_v,
                                void* stream) {
  if (B < 1 || L < 1 || H < 1) return fail("B, L, H must be positive");
  if (!(p >= 0.f && p < 1.f)) return fail("p must lie in [0, 1)");
  if ((int64_t)B * L * L * 2 * ((H + 31) / 32) >= (1LL << 32)) return fail("B L L H / 16 must stay below 2^32 (the time dropout's counter)");
  const int rc = acattn_launch_time_rng(B, L, H, seed, p, keep_k, keep_v, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_unnorm_attention_supported(const acattn_problem* p) { return p ? acattn_unnorm_supported(*p) : 0; }

int acattn_unnorm_attention_fwd(const acattn_problem* p, const acattn_fwd_out* out, void* stream) {
  if (!p || !out) return fail("problem and out must be non-NULL");
  int rc = acattn_launch_unnorm_fwd(*p, *out, (hipStream_t)stream);
  if (rc == 0 && out->penalty_part)
    rc = acattn_launch_penalty_rows(out->attack_mask, p->B, p->n_heads, p->L, out->penalty_part, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_unnorm_attention_bwd(const acattn_problem* p, const acattn_bwd_io* io, void* stream) {
  if (!p || !io) return fail("problem and io must be non-NULL");
  const int rc = acattn_launch_unnorm_bwd(*p, *io, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_max_sequence_length(void) { return ACATTN_MAX_L; }

int acattn_select_forward_kernel(int which) { return acattn_fwd_kernel_choice(which); }

int acattn_select_backward_kernel(int which) { return acattn_bwd_kernel_choice(which); }

const char* acattn_last_error(void) { return g_err; }

int64_t acattn_fwd_algorithmic_bytes(const acattn_problem* p) {
  if (!p) return -1;
  const int64_t t_lh = 4LL * p->L * p->H, t_ll = 4LL * p->L * p->L;
  if (!p->adversarial) return (int64_t)p->B * 4 * t_lh;  // contract A': read q,k,v, write one context
  // contract A: read q,k,v,qa,ka (+ gate logits), write two contexts + M (noise generated in-kernel)
  int64_t per_seq = 7 * t_lh + (int64_t)p->n_heads * t_ll;
  if (p->combine_option == ACATTN_COMBINE_GATE) per_seq += t_ll;
  return (int64_t)p->B * per_seq;
}

int acattn_calibrated_attention_fwd(const acattn_problem* p, const acattn_fwd_out* out, void* stream) {
  if (int rc = check_problem(p)) return rc;
  if (!out) return fail("out is NULL");
  if (!out->ctx_calibrated) return fail("ctx_calibrated must be non-NULL");
  if (p->adversarial && (!out->ctx_attacked || !out->attack_mask))
    return fail("adversarial forward needs ctx_attacked and attack_mask outputs");
  acattn_penalty_written_set(false);
  int rc = acattn_launch_fwd(*p, *out, (hipStream_t)stream);
  // acattn_fwd_out.penalty_part: the streaming kernel (L > 64) has formed the sums itself; behind every other kernel,
  // the long form (L > 208) included, they are taken from the mask it wrote
  if (rc == 0 && p->adversarial && out->penalty_part && !acattn_penalty_written())
    rc = acattn_launch_penalty_rows(out->attack_mask, p->B, p->n_heads, p->L, out->penalty_part, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_spatial_affines(const acattn_problem* p, float* affine, void* stream) {
  if (!p || !affine) return fail("problem and affine must be non-NULL");
  if (p->B < 1 || p->L < 1 || p->H < 1 || p->n_heads < 1 || p->H % p->n_heads != 0 || (p->H / p->n_heads) % 4 != 0)
    return fail("spatial affines: bad shape");
  if (!p->q || !p->k || !p->w_order || !p->b_order || !p->w_dist || !p->b_dist)
    return fail("spatial affines need q, k and both affines' parameters");
  const int rc = acattn_launch_spatial_affines(*p, affine, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_calibrated_attention_bwd(const acattn_problem* p, const acattn_bwd_io* io, void* stream) {
  if (int rc = check_problem(p)) return rc;
  if (!io) return fail("io is NULL");
  if (!p->adversarial) return fail("backward is defined for the adversarial (full) operator only");
  if (!io->attack_mask || !io->row_stats) return fail("backward needs the forward's attack_mask and row_stats");
  if (!io->dq || !io->dk || !io->dv || !io->dqa || !io->dka) return fail("dq, dk, dv, dqa, dka must be non-NULL");
  if (p->combine_option == ACATTN_COMBINE_GATE && !io->dgate_logits) return fail("gate combine needs dgate_logits");
  if (!io->dw_order_part || !io->dw_dist_part || !io->dsmall_part) return fail("parameter partial buffers must be non-NULL");
  if (io->part_stride != 0 && io->part_stride < 2 * (p->H / p->n_heads)) return fail("part_stride is smaller than a partial row");
  const int rc = acattn_launch_bwd(*p, *io, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_calibrated_attention_bwd_attack_side(const acattn_problem* p, const acattn_bwd_io* io, void* stream) {
  if (int rc = check_problem(p)) return rc;
  if (!io) return fail("io is NULL");
  if (!p->adversarial) return fail("backward is defined for the adversarial (full) operator only");
  if (!io->attack_mask || !io->row_stats) return fail("backward needs the forward's attack_mask and row_stats");
  if (!io->dqa || !io->dka) return fail("dqa, dka must be non-NULL");
  const int rc = acattn_launch_bwd_attack(*p, *io, (hipStream_t)stream, nullptr);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  if (rc == -100) snprintf(g_err, sizeof(g_err), "the attack-side backward (acattn_bwd_attack.hip) does not cover this launch");
  return rc;
}

int acattn_calibrated_attention_bwd_gate_summed(const acattn_problem* p, const acattn_bwd_io* io) {
  if (!p || !io || p->B < 1 || p->L < 1 || p->H < 1 || p->n_heads < 1) return 0;
  return acattn_bwd_gate_summed(*p, *io) ? 1 : 0;
}

int acattn_calibrated_attention_bwd_pair_supported(const acattn_problem* p, const acattn_bwd_io* io) {
  if (!p || !io || p->B < 1 || p->L < 1 || p->H < 1 || p->n_heads < 1) return 0;
  return acattn_bwd_pair_supported(*p, *io) ? 1 : 0;
}

int64_t acattn_calibrated_attention_bwd_workspace_bytes(const acattn_problem* p) {
  if (!p || p->B < 1 || p->L < 1 || p->n_heads < 1) return -1;
  // the streaming pair keeps 8 floats per (sequence, head, row): unchanged wherever it runs.  The long form (L > 208, or
  // pinned by the calling thread at any L) keeps 16: its row scalars and the corrections of a fully masked row's normalisers
  const bool long_form = p->L > 208 || acattn_bwd_kernel_choice(-1) == ACATTN_BWD_LONG;
  return (long_form ? 2 : 1) * acattn_bwd_stream_ws_bytes(*p);
}

int acattn_spatial_attention_bwd(const acattn_problem* p, const acattn_spatial_bwd_io* io, void* stream) {
  if (int rc = check_problem(p)) return rc;
  if (!io) return fail("io is NULL");
  if (p->L > 208) return fail("the spatial-only backward is built for sequence length L <= 208 (the long form covers the forward and acattn_calibrated_attention_bwd)");
  if (p->adversarial) return fail("the spatial-only backward needs adversarial == 0 (use acattn_calibrated_attention_bwd)");
  if (!io->d_ctx) return fail("d_ctx must be non-NULL");
  if (!io->dq || !io->dk || !io->dv) return fail("dq, dk, dv must be non-NULL");
  if (!io->dw_order_part || !io->dw_dist_part || !io->dsmall_part) return fail("parameter partial buffers must be non-NULL");
  if (io->part_stride != 0 && io->part_stride < 2 * (p->H / p->n_heads)) return fail("part_stride is smaller than a partial row");
  if (!io->workspace) return fail("workspace must be non-NULL (acattn_spatial_attention_bwd_workspace_bytes)");
  if (io->read_rows && io->n_read_rows < 1) return fail("read_rows given with n_read_rows < 1");
  const int rc = acattn_launch_spatial_bwd(*p, *io, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int64_t acattn_spatial_attention_bwd_workspace_bytes(const acattn_problem* p) {
  if (!p || p->B < 1 || p->L < 1 || p->n_heads < 1) return -1;
  return acattn_spatial_bwd_ws_bytes(*p);
}

int acattn_rng_materialize(int32_t B, int32_t n_heads, int32_t L, uint64_t seed, float p_drop, float* noise,
                           uint8_t* keep_after, uint8_t* keep_mask, uint8_t* keep_before, void* stream) {
  if (B < 1 || n_heads < 1 || L < 1) return fail("B, n_heads, L must be positive");
  const int rc = acattn_launch_rng(B, n_heads, L, seed, p_drop, noise, keep_after, keep_mask, keep_before,
                                   (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

static int check_ce(const acattn_ce_problem* p) {
  if (!p) return fail("ce problem is NULL");
  if (p->B < 1 || p->N < 1) return fail("B and N must be positive");
  if (p->H != 64 && p->H != 128 && p->H != 256) return fail("unsupported hidden size for the fused cross-entropy: H must be 64, 128 or 256");
  if (!p->out || !p->table || !p->target) return fail("out, table, target must be non-NULL");
  return 0;
}

int64_t acattn_full_sort_ce_workspace_bytes(const acattn_ce_problem* p) {
  if (!p || (p->H != 64 && p->H != 128 && p->H != 256)) return -1;
  return acattn_ce_ws_bytes(*p);
}

int acattn_full_sort_ce_fwd(const acattn_ce_problem* p, void* workspace, float* lse, float* row_loss, void* stream) {
  if (int rc = check_ce(p)) return rc;
  if (!workspace || !lse || !row_loss) return fail("workspace, lse, row_loss must be non-NULL");
  const int rc = acattn_launch_ce_fwd(*p, workspace, lse, row_loss, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_full_sort_ce_fwd_dir(const acattn_ce_problem* p, void* workspace, float* lse, float* row_loss, float* dir,
                                void* stream) {
  if (int rc = check_ce(p)) return rc;
  if (!workspace || !lse || !row_loss || !dir) return fail("workspace, lse, row_loss, dir must be non-NULL");
  const int rc = acattn_launch_ce_fwd_dir(*p, workspace, lse, row_loss, dir, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_full_sort_ce_bwd(const acattn_ce_problem* p, const float* lse, const float* coef, void* workspace,
                            float* d_out, float* d_table, void* stream) {
  if (int rc = check_ce(p)) return rc;
  if (!workspace || !lse || !coef || !d_out) return fail("workspace, lse, coef, d_out must be non-NULL");
  const int rc = acattn_launch_ce_bwd(*p, lse, coef, workspace, d_out, d_table, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

static int check_ce_pair(const acattn_ce_problem* pa, const acattn_ce_problem* pc) {
  if (int rc = check_ce(pa)) return rc;
  if (int rc = check_ce(pc)) return rc;
  if (pa->N != pc->N || pa->H != pc->H) return fail("the two row sets must share the table: N and H differ");
  return 0;
}

int64_t acattn_full_sort_ce_fwd_pair_workspace_bytes(const acattn_ce_problem* pa, const acattn_ce_problem* pc) {
  if (check_ce_pair(pa, pc)) return -1;
  return acattn_ce_pair_ws_bytes(*pa, *pc);
}

int acattn_full_sort_ce_fwd_pair(const acattn_ce_problem* pa, const acattn_ce_problem* pc, void* workspace, float* lse_a,
                                 float* row_loss_a, float* dir_a, float* lse_c, float* row_loss_c, void* stream) {
  if (int rc = check_ce_pair(pa, pc)) return rc;
  if (!workspace || !lse_a || !row_loss_a || !dir_a || !lse_c || !row_loss_c)
    return fail("workspace, lse_a, row_loss_a, dir_a, lse_c, row_loss_c must be non-NULL");
  const int rc = acattn_launch_ce_fwd_pair(*pa, *pc, workspace, lse_a, row_loss_a, dir_a, lse_c, row_loss_c, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_full_sort_ce_products(int mode) { return acattn_ce_products_choice(mode); }

int acattn_full_sort_rank_supported(int32_t H) { return (H == 64 || H == 128 || H == 256) ? 1 : 0; }

static int check_rank(const acattn_ce_problem* p, int32_t first_item) {
  if (!p) return fail("rank problem is NULL");
  if (!acattn_full_sort_rank_supported(p->H)) return fail("unsupported hidden size for the full-sort rank: H must be 64, 128 or 256");
  if (p->B < 1 || p->N < 1) return fail("full-sort rank: B and N must be positive");
  if (p->N > (1 << 30)) return fail("full-sort rank: N must not exceed 2^30");
  if (!p->out || !p->table || !p->target) return fail("full-sort rank: out, table, target must be non-NULL");
  if (first_item < 0 || first_item >= p->N) return fail("full-sort rank: first_item must lie in [0, N)");
  return 0;
}

int64_t acattn_full_sort_rank_workspace_bytes(const acattn_ce_problem* p) {
  if (!p || !acattn_full_sort_rank_supported(p->H) || p->B < 1 || p->N < 1 || p->N > (1 << 30)) return -1;
  return acattn_rank_ws_bytes(*p);
}

int acattn_full_sort_rank(const acattn_ce_problem* p, int32_t first_item, void* workspace, int32_t* rank, float* target_score,
                          void* stream) {
  if (int rc = check_rank(p, first_item)) return rc;
  if (!workspace || !rank || !target_score) return fail("full-sort rank: workspace, rank, target_score must be non-NULL");
  const int rc = acattn_launch_rank(*p, first_item, workspace, rank, target_score, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_full_sort_rank_exclude(const acattn_ce_problem* p, int32_t first_item, const int64_t* pair_row,
                                  const int64_t* pair_item, int64_t n_pairs, const float* target_score, int32_t* rank,
                                  void* stream) {
  if (int rc = check_rank(p, first_item)) return rc;
  if (!rank || !target_score) return fail("full-sort rank: rank, target_score must be non-NULL");
  if (n_pairs < 0) return fail("full-sort rank: n_pairs must not be negative");
  if (n_pairs > 0 && (!pair_row || !pair_item)) return fail("full-sort rank: pair_row, pair_item must be non-NULL when n_pairs > 0");
  if (n_pairs == 0) return 0;
  const int rc = acattn_launch_rank_exclude(*p, first_item, pair_row, pair_item, n_pairs, target_score, rank, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_linear_products(int mode) { return acattn_linear_products_choice(mode); }

static int check_ln(const acattn_ln_problem* p) {
  if (!p) return fail("ln problem is NULL");
  if (p->rows < 1) return fail("rows must be positive");
  if (p->H != 64 && p->H != 128 && p->H != 256) return fail("unsupported hidden size for the fused LayerNorm: H must be 64, 128 or 256");
  if (p->residual_rows < 1 || p->rows % p->residual_rows != 0) return fail("residual_rows must divide rows");
  if (!p->z || !p->residual || !p->gamma || !p->beta) return fail("z, residual, gamma, beta must be non-NULL");
  if (p->p_drop < 0.f || p->p_drop >= 1.f) return fail("p_drop must lie in [0, 1)");
  return 0;
}

int acattn_dropout_add_layernorm_fwd(const acattn_ln_problem* p, float* y, float* stats, void* stream) {
  if (int rc = check_ln(p)) return rc;
  if (!y || !stats) return fail("y and stats must be non-NULL");
  const int rc = acattn_launch_ln_fwd(*p, y, stats, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_dropout_add_layernorm_bwd(const acattn_ln_problem* p, const float* dy, const float* stats, float* dz,
                                     float* dres, float* dgb_part, void* stream) {
  if (int rc = check_ln(p)) return rc;
  if (!dy || !stats) return fail("dy and stats must be non-NULL");
  const int rc = acattn_launch_ln_bwd(*p, dy, stats, dz, dres, dgb_part, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

static int check_proj(const acattn_proj_problem* p) {
  if (!p) return fail("problem must be non-NULL");
  if (p->rows < 1) return fail("rows must be positive");
  if (!acattn_proj_supported(p->H, p->G)) return fail("projections: hidden_size must be 64, 128 or 256 and the gate at most 256 wide");
  if (!p->x || !p->wq || !p->bq || !p->wk || !p->bk || !p->wv || !p->bv || !p->waq || !p->baq || !p->wak || !p->bak)
    return fail("projections: input and parameters must be non-NULL");
  if ((p->wg != nullptr) != (p->bg != nullptr) || (p->wg != nullptr) != (p->G > 0))
    return fail("projections: gate weight, bias and width go together");
  if (((uintptr_t)p->split_planes & 15) != 0) return fail("projections: split_planes must be 16-byte aligned");
  return 0;
}

int acattn_projections_supported(int32_t H, int32_t G) { return acattn_proj_supported(H, G) ? 1 : 0; }

int64_t acattn_projections_bwd_workspace_bytes(const acattn_proj_problem* p) {
  if (!p || !acattn_proj_supported(p->H, p->G)) return -1;
  return acattn_proj_bwd_ws_bytes(*p);
}

int acattn_projections_fwd(const acattn_proj_problem* p, const acattn_proj_out* out, void* stream) {
  if (int rc = check_proj(p)) return rc;
  if (!out || !out->mq || !out->mk || !out->mv || !out->qa || !out->ka) return fail("projections: outputs must be non-NULL");
  if ((p->wg != nullptr) != (out->gate != nullptr)) return fail("projections: gate output goes with the gate parameters");
  if (out->affine) {
    if (!p->w_order || !p->b_order || !p->w_dist || !p->b_dist) return fail("projections: affine planes need the spatial calibrator's parameters");
    if (p->n_heads < 1 || p->H % p->n_heads != 0 || (p->H / p->n_heads) % 16 != 0) return fail("projections: affine planes need a head size that is a multiple of 16");
    if (p->L < 1 || p->rows % p->L != 0) return fail("projections: affine planes need rows = B * L");
  }
  const int rc = acattn_launch_proj_fwd(*p, *out, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_projections_qkv_supported(int32_t H) { return acattn_proj_qkv_supported(H) ? 1 : 0; }

int acattn_projections_qkv_fwd(const acattn_proj_problem* p, const acattn_proj_out* out, void* stream) {
  if (!p) return fail("problem must be non-NULL");
  if (p->rows < 1) return fail("rows must be positive");
  if (!acattn_proj_qkv_supported(p->H)) return fail("projections (q, k, v only): hidden_size must be 64 with the split products on");
  if (!p->x || !p->wq || !p->bq || !p->wk || !p->bk || !p->wv || !p->bv) return fail("projections: input and parameters must be non-NULL");
  if (!out || !out->mq || !out->mk || !out->mv) return fail("projections: outputs must be non-NULL");
  if (out->qa || out->ka || out->gate) return fail("projections (q, k, v only): qa, ka and gate outputs must be NULL");
  if (out->affine) {
    if (!p->w_order || !p->b_order || !p->w_dist || !p->b_dist) return fail("projections: affine planes need the spatial calibrator's parameters");
    if (p->n_heads < 1 || p->H % p->n_heads != 0 || (p->H / p->n_heads) % 16 != 0) return fail("projections: affine planes need a head size that is a multiple of 16");
    if (p->L < 1 || p->rows % p->L != 0) return fail("projections: affine planes need rows = B * L");
  }
  const int rc = acattn_launch_proj_qkv_fwd(*p, *out, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_projections_bwd(const acattn_proj_problem* p, const acattn_proj_bwd_io* io, void* stream) {
  if (int rc = check_proj(p)) return rc;
  if (!io) return fail("io must be non-NULL");
  if (!io->dmq_total && !io->dmk_total && !io->dx) return fail("projections backward: nothing to compute");
  const int rc = acattn_launch_proj_bwd(*p, *io, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

static int check_tail(const acattn_tail_problem* p, const acattn_tail_saved* s) {
  if (!p || !s) return fail("problem and saved must be non-NULL");
  if (p->rows < 1) return fail("rows must be positive");
  if (!acattn_tail_supported(p->H, p->I)) return fail("layer tail: (hidden_size, inner_size) must be (64, 256), (64, 128), (128, 512), (128, 256), (128, 64) or (256, 1024)");
  if (!p->ctx || !p->x || !p->wd || !p->bd || !p->g1 || !p->b1 || !p->w1 || !p->bb1 || !p->w2 || !p->bb2 || !p->g2 || !p->b2)
    return fail("layer tail: inputs and parameters must be non-NULL");
  if (!(p->p1 >= 0.f && p->p1 < 1.f) || !(p->p2 >= 0.f && p->p2 < 1.f)) return fail("dropout probabilities must be in [0, 1)");
  if (!s->h1 || !s->st1 || !s->a || !s->h3 || !s->st2) return fail("layer tail: saved tensors must be non-NULL");
  if (p->src_index && (p->src_R < 1 || p->src_L < 1)) return fail("layer tail: src_index needs src_R, src_L >= 1");
  if (p->split_planes && p->H != 64) return fail("layer tail: split_planes is for hidden 64 only");
  if (((uintptr_t)p->split_planes & 15) != 0) return fail("layer tail: split_planes must be 16-byte aligned");
  return 0;
}

int acattn_layer_tail_supported(int32_t H, int32_t I) { return acattn_tail_supported(H, I) ? 1 : 0; }

int32_t acattn_layer_tail_bwd_partial_rows(int32_t rows) { return acattn_tail_bwd_partial_rows(rows); }
int32_t acattn_layer_tail_bwd_partial_rows_for(int32_t rows, int32_t H) { return acattn_tail_bwd_partial_rows_h(rows, H); }
int64_t acattn_layer_tail_bwd_workspace_bytes(int32_t H, int32_t I) {
  return acattn_tail_supported(H, I) ? acattn_tail_bwd_ws_bytes(H, I) : -1;
}

int64_t acattn_layer_tail_split_bytes(int32_t H, int32_t I, int32_t rows) {
  return acattn_tail_supported(H, I) && rows > 0 ? acattn_tail_split_bytes(H, I, rows) : 0;
}

int acattn_layer_tail_split_weights(const acattn_tail_problem* p, void* planes, void* stream) {
  if (!p || !planes || !p->wd || !p->w1 || !p->w2) return fail("layer tail split planes: problem, weights and planes must be non-NULL");
  if (p->H != 64 || (p->I != 256 && p->I != 128)) return fail("layer tail split planes: hidden 64, inner 256 or 128 only");
  if (((uintptr_t)planes & 15) != 0) return fail("layer tail split planes: planes must be 16-byte aligned");
  const int rc = acattn_launch_tail_split(*p, planes, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int64_t acattn_projections_split_bytes(int32_t H, int32_t G) { return acattn_proj_split_bytes(H, G); }

int acattn_split_weights_many(const acattn_split_layer* layers, int32_t n_layers, void* stream) {
  if (!layers || n_layers < 1 || n_layers > ACATTN_SPLIT_MAX_LAYERS) return fail("split planes: 1 .. ACATTN_SPLIT_MAX_LAYERS layers");
  for (int k = 0; k < n_layers; ++k) {
    const acattn_split_layer& l = layers[k];
    if (l.tail_planes) {
      if (!l.wd || !l.w1 || !l.w2) return fail("split planes: tail planes need wd, w1 and w2");
      if (l.I != 256 && l.I != 128) return fail("split planes: tail planes are for hidden 64, inner 256 or 128");
    }
    if (l.proj_planes) {
      if (!l.wq || !l.wk || !l.wv || !l.waq || !l.wak) return fail("split planes: projection planes need the five square weights");
      if ((l.wg != nullptr) != (l.G > 0) || l.G < 0 || l.G > 64) return fail("split planes: gate weight and width go together, at most 64 outputs");
    }
    if ((((uintptr_t)l.tail_planes | (uintptr_t)l.proj_planes) & 15) != 0) return fail("split planes: planes must be 16-byte aligned");
  }
  const int rc = acattn_launch_split_many(layers, n_layers, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_select_layer_tail_blocks(int nb) {
  if (nb < 0 || nb > 2) return fail("rows per wave: 0 (automatic), 1 or 2 blocks of 16");
  return acattn_select_tail_nb(nb);
}

int acattn_layer_tail_fwd(const acattn_tail_problem* p, const acattn_tail_saved* saved, void* stream) {
  if (int rc = check_tail(p, saved)) return rc;
  if (!saved->act || !saved->out) return fail("layer tail forward: act and out must be non-NULL");
  const int rc = acattn_launch_tail_fwd(*p, *saved, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_layer_tail_fwd_pair(const acattn_tail_problem* p_a, const acattn_tail_saved* saved_a, const acattn_tail_problem* p_b,
                               const acattn_tail_saved* saved_b, void* stream) {
  if (int rc = check_tail(p_a, saved_a)) return rc;
  if (int rc = check_tail(p_b, saved_b)) return rc;
  if (!saved_a->act || !saved_a->out || !saved_b->act || !saved_b->out) return fail("layer tail forward: act and out must be non-NULL");
  const int rc = acattn_launch_tail_fwd_pair(*p_a, *saved_a, *p_b, *saved_b, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_layer_tail_bwd(const acattn_tail_problem* p, const acattn_tail_saved* saved, const acattn_tail_bwd_io* io,
                          void* stream) {
  if (int rc = check_tail(p, saved)) return rc;
  if (!io || !io->d_out) return fail("layer tail backward: d_out must be non-NULL");
  const int rc = acattn_launch_tail_bwd(*p, *saved, *io, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_dense_ce_fwd(const float* logits, int64_t rows, int64_t N, const int64_t* target, float* lse, float* row_loss,
                        void* stream) {
  if (!logits || !target || !lse || !row_loss) return fail("dense CE: logits, target, lse, row_loss must be non-NULL");
  if (rows < 1 || N < 1) return fail("dense CE: rows and N must be positive");
  const int rc = acattn_launch_dense_ce_fwd(logits, rows, N, target, lse, row_loss, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}
int acattn_dense_ce_bwd(const float* logits, const float* lse, const int64_t* target, const float* coef, int64_t rows, int64_t N,
                        float* d_logits, void* stream) {
  if (!logits || !lse || !target || !coef || !d_logits) return fail("dense CE backward: every pointer must be non-NULL");
  if (rows < 1 || N < 1) return fail("dense CE: rows and N must be positive");
  const int rc = acattn_launch_dense_ce_bwd(logits, lse, target, coef, rows, N, d_logits, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_step_inputs(const void* const* src, void* const* dst, const int64_t* bytes, int32_t n_copies, int64_t* counter,
                       const int64_t* item_length, int64_t* last_row, int32_t n_rows, void* stream) {
  if (n_copies < 0 || n_copies > ACATTN_MAX_COPIES) return fail("step inputs: 0 .. ACATTN_MAX_COPIES copies");
  if (n_copies > 0 && (!src || !dst || !bytes)) return fail("step inputs: src, dst, bytes must be non-NULL");
  for (int k = 0; k < n_copies; ++k)
    if (bytes[k] > 0 && (!src[k] || !dst[k])) return fail("step inputs: NULL copy operand");
  if ((item_length == nullptr) != (last_row == nullptr)) return fail("step inputs: item_length and last_row come together");
  if (last_row && n_rows < 1) return fail("step inputs: n_rows must be positive");
  const int rc = acattn_launch_step_inputs(src, dst, bytes, n_copies, counter, item_length, last_row, n_rows, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_sum_rows(const float* x, float* out, int32_t batch, int32_t R, int32_t C, void* stream) {
  if (!x || !out) return fail("x and out must be non-NULL");
  if (batch < 1 || R < 1 || C < 1) return fail("batch, R, C must be positive");
  const int rc = acattn_launch_sum_rows(x, out, batch, R, C, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_sum_rows_pair(const float* x1, float* out1, int32_t batch1, int32_t R1, int32_t C1, const float* x2, float* out2,
                         int32_t batch2, int32_t R2, int32_t C2, void* stream) {
  if (!x1 || !out1 || !x2 || !out2) return fail("x and out must be non-NULL");
  if (batch1 < 1 || R1 < 1 || C1 < 1 || batch2 < 1 || R2 < 1 || C2 < 1) return fail("batch, R, C must be positive");
  const int rc = acattn_launch_sum_rows_pair(x1, out1, batch1, R1, C1, x2, out2, batch2, R2, C2, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

static int check_embed(const acattn_embed_problem* p) {
  if (!p) return fail("embed problem is NULL");
  if (p->rows < 1 || p->L < 1 || p->rows % p->L != 0) return fail("rows must be a positive multiple of L");
  if (p->H != 64 && p->H != 128 && p->H != 256) return fail("unsupported hidden size for the fused embedding front end: H must be 64, 128 or 256");
  if (p->n_table_rows < 1) return fail("n_table_rows must be positive");
  if (!p->idx || !p->table || !p->gamma || !p->beta) return fail("idx, table, gamma, beta must be non-NULL");
  if (p->p_drop < 0.f || p->p_drop >= 1.f) return fail("p_drop must lie in [0, 1)");
  return 0;
}

int acattn_embed_layernorm_fwd(const acattn_embed_problem* p, float* y, float* stats, void* stream) {
  if (const int rc = check_embed(p)) return rc;
  if (!y || !stats) return fail("y and stats must be non-NULL");
  const int rc = acattn_launch_embed_fwd(*p, y, stats, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_embed_layernorm_bwd(const acattn_embed_problem* p, const float* dy, const float* stats, int64_t padding_idx,
                               float* d_table, float* d_pos_part, float* dgb_part, void* stream) {
  if (const int rc = check_embed(p)) return rc;
  if (!dy || !stats) return fail("dy and stats must be non-NULL");
  const int rc = acattn_launch_embed_bwd(*p, dy, stats, padding_idx, d_table, d_pos_part, dgb_part, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_embed_user_supported(int32_t H, int32_t Di) {
  if (H != 64 && H != 128 && H != 256) return 0;
  return Di > 0 && Di < H && Di % 4 == 0 && (H - Di) % 4 == 0;
}

static int check_embed_user(const acattn_embed_user_problem* p) {
  if (!p) return fail("embed_user problem is NULL");
  if (!acattn_embed_user_supported(p->H, p->Di))
    return fail("unsupported (H, Di) for the personalised front end: H must be 64, 128 or 256, Di and H - Di positive multiples of 4");
  if (p->rows < 1 || p->L < 1 || p->rows % p->L != 0) return fail("rows must be a positive multiple of L");
  if (p->n_table_rows < 1 || p->n_user_rows < 1) return fail("n_table_rows and n_user_rows must be positive");
  if (!p->idx) return fail("idx must be non-NULL");
  if (!p->user) return fail("user must be non-NULL");
  if (!p->table || !p->user_table) return fail("table and user_table must be non-NULL");
  if (!p->gamma || !p->beta) return fail("gamma and beta must be non-NULL");
  if (p->p_drop < 0.f || p->p_drop >= 1.f) return fail("p_drop must lie in [0, 1)");
  return 0;
}

int acattn_embed_user_layernorm_fwd(const acattn_embed_user_problem* p, float* y, float* stats, void* stream) {
  if (const int rc = check_embed_user(p)) return rc;
  if (!y) return fail("y must be non-NULL");
  if (!stats) return fail("stats must be non-NULL");
  const int rc = acattn_launch_embed_user_fwd(*p, y, stats, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_embed_user_layernorm_bwd(const acattn_embed_user_problem* p, const float* dy, const float* stats,
                                    int64_t item_padding_idx, int64_t user_padding_idx, float* d_item, float* d_user,
                                    float* user_rows_ws, float* d_pos_part, float* dgb_part, void* stream) {
  if (const int rc = check_embed_user(p)) return rc;
  if (!dy || !stats) return fail("dy and stats must be non-NULL");
  const int rc = acattn_launch_embed_user_bwd(*p, dy, stats, item_padding_idx, user_padding_idx, d_item, d_user, user_rows_ws,
                                              d_pos_part, dgb_part, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_mask_penalty_fwd(const float* m, int64_t n, float* workspace, float* norm, void* stream) {
  if (!m || !workspace || !norm) return fail("m, workspace and norm must be non-NULL");
  if (n < 1) return fail("n must be positive");
  if (((uintptr_t)m & 15) != 0) return fail("m must be 16-byte aligned");
  const int rc = acattn_launch_penalty_fwd(m, n, workspace, norm, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_mask_penalty_bwd(const float* m, const float* norm, const float* d_norm, int64_t n, float* d_m, void* stream) {
  if (!m || !norm || !d_norm || !d_m) return fail("m, norm, d_norm and d_m must be non-NULL");
  if (n < 1) return fail("n must be positive");
  if ((((uintptr_t)m | (uintptr_t)d_m) & 15) != 0) return fail("m and d_m must be 16-byte aligned");
  const int rc = acattn_launch_penalty_bwd(m, norm, d_norm, n, d_m, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_mask_penalty_partial(const float* m, int64_t n, float* part, void* stream) {
  if (!m || !part) return fail("m and part must be non-NULL");
  if (n < 1) return fail("n must be positive");
  if (((uintptr_t)m & 15) != 0) return fail("m must be 16-byte aligned");
  const int rc = acattn_launch_penalty_partial(m, n, part, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_attacked_loss_finish(const float* row_loss, int32_t B, const float* part, int32_t n_masks, int64_t mask_numel,
                                float weight, float* out, float* scale_buf, int32_t n_scale, void* stream) {
  if (!row_loss || !part || !out) return fail("row_loss, part and out must be non-NULL");
  if (B < 1 || n_masks < 1 || mask_numel < 1) return fail("B, n_masks and mask_numel must be positive");
  if (n_scale < 0 || (n_scale > 0 && !scale_buf)) return fail("scale_buf must be given with n_scale > 0");
  const int rc = acattn_launch_attacked_loss_finish(row_loss, B, part, n_masks, mask_numel, weight, out, scale_buf, n_scale,
                                                    (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_mask_penalty_rows(const float* m, int32_t B, int32_t n_heads, int32_t L, float* pen, void* stream) {
  if (!m || !pen) return fail("m and pen must be non-NULL");
  if (B < 1 || n_heads < 1 || L < 1) return fail("B, n_heads and L must be positive");
  const int rc = acattn_launch_penalty_rows(m, B, n_heads, L, pen, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_attacked_loss_finish_rows(const float* row_loss, int32_t B, const float* const* pen, int32_t n_masks, int32_t count,
                                     float weight, float* out, float* scale_buf, int32_t n_scale, void* stream) {
  if (!row_loss || !pen || !out) return fail("row_loss, pen and out must be non-NULL");
  if (B < 1 || count < 1 || n_masks < 1 || n_masks > ACATTN_MAX_MASKS) return fail("B, count positive, 1 <= n_masks <= ACATTN_MAX_MASKS");
  for (int l = 0; l < n_masks; ++l)
    if (!pen[l]) return fail("every pen vector must be non-NULL");
  if (n_scale < 0 || (n_scale > 0 && !scale_buf)) return fail("scale_buf must be given with n_scale > 0");
  const int rc = acattn_launch_attacked_loss_finish_rows(row_loss, B, pen, n_masks, count, weight, out, scale_buf, n_scale,
                                                         (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_attacked_loss_finish_rows_pair(const float* row_loss, int32_t B, const float* const* pen, int32_t n_masks,
                                          int32_t count, float weight, float* out, float* scale_buf, int32_t n_scale,
                                          const float* row_loss_c, int32_t B_c, float* mean_c, void* stream) {
  if (!row_loss || !pen || !out) return fail("row_loss, pen and out must be non-NULL");
  if (!row_loss_c || !mean_c || B_c < 1) return fail("row_loss_c and mean_c must be non-NULL, B_c positive");
  if (B < 1 || count < 1 || n_masks < 1 || n_masks > ACATTN_MAX_MASKS) return fail("B, count positive, 1 <= n_masks <= ACATTN_MAX_MASKS");
  for (int l = 0; l < n_masks; ++l)
    if (!pen[l]) return fail("every pen vector must be non-NULL");
  if (n_scale < 0 || (n_scale > 0 && !scale_buf)) return fail("scale_buf must be given with n_scale > 0");
  const int rc = acattn_launch_attacked_loss_finish_rows(row_loss, B, pen, n_masks, count, weight, out, scale_buf, n_scale,
                                                         (hipStream_t)stream, row_loss_c, B_c, mean_c);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_mask_penalty_drows(const float* norms, const float* d_loss, float scale, int32_t count, float* const* d_pen,
                              int32_t n_masks, void* stream) {
  if (!norms || !d_loss || !d_pen) return fail("norms, d_loss and d_pen must be non-NULL");
  if (count < 1 || n_masks < 1 || n_masks > ACATTN_MAX_MASKS) return fail("count positive, 1 <= n_masks <= ACATTN_MAX_MASKS");
  for (int l = 0; l < n_masks; ++l)
    if (!d_pen[l]) return fail("every d_pen vector must be non-NULL");
  const int rc = acattn_launch_penalty_drows(norms, d_loss, scale, count, d_pen, n_masks, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_mask_penalty_drows_dir(const float* norms, const float* d_loss, float scale, int32_t count, float* const* d_pen,
                                  int32_t n_masks, const float* direction, float* d_out, int32_t n_dir, void* stream) {
  if (!norms || !d_loss || !d_pen || !direction || !d_out) return fail("norms, d_loss, d_pen, direction and d_out must be non-NULL");
  if (count < 1 || n_dir < 1 || n_masks < 1 || n_masks > ACATTN_MAX_MASKS) return fail("count, n_dir positive, 1 <= n_masks <= ACATTN_MAX_MASKS");
  for (int l = 0; l < n_masks; ++l)
    if (!d_pen[l]) return fail("every d_pen vector must be non-NULL");
  const int rc = acattn_launch_penalty_drows(norms, d_loss, scale, count, d_pen, n_masks, (hipStream_t)stream, direction, d_out, n_dir);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_mask_penalty_bwd_scaled(const float* m, const float* norm, const float* d_loss, float scale, int64_t n, float* d_m,
                                   void* stream) {
  if (!m || !norm || !d_loss || !d_m) return fail("m, norm, d_loss and d_m must be non-NULL");
  if (n < 1) return fail("n must be positive");
  if ((((uintptr_t)m | (uintptr_t)d_m) & 15) != 0) return fail("m and d_m must be 16-byte aligned");
  const int rc = acattn_launch_penalty_bwd_scaled(m, norm, d_loss, scale, n, d_m, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_mask_penalty_partial_multi(const float* const* m, int32_t n_masks, int64_t n, float* part, void* stream) {
  if (!m || !part) return fail("m and part must be non-NULL");
  if (n < 1 || n_masks < 1 || n_masks > ACATTN_MAX_MASKS) return fail("n must be positive, 1 <= n_masks <= ACATTN_MAX_MASKS");
  for (int l = 0; l < n_masks; ++l)
    if (!m[l] || ((uintptr_t)m[l] & 15) != 0) return fail("every mask must be non-NULL and 16-byte aligned");
  const int rc = acattn_launch_penalty_partial_multi(m, n_masks, n, part, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_mask_penalty_bwd_scaled_multi(const float* const* m, const float* norms, const float* d_loss, float scale, int64_t n,
                                         float* const* d_m, int32_t n_masks, void* stream) {
  if (!m || !norms || !d_loss || !d_m) return fail("m, norms, d_loss and d_m must be non-NULL");
  if (n < 1 || n_masks < 1 || n_masks > ACATTN_MAX_MASKS) return fail("n must be positive, 1 <= n_masks <= ACATTN_MAX_MASKS");
  for (int l = 0; l < n_masks; ++l)
    if (!m[l] || !d_m[l] || (((uintptr_t)m[l] | (uintptr_t)d_m[l]) & 15) != 0)
      return fail("every m and d_m must be non-NULL and 16-byte aligned");
  const int rc = acattn_launch_penalty_bwd_scaled_multi(m, norms, d_loss, scale, n, d_m, n_masks, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_adam_step(const acattn_adam_group* g, double lr, double beta1, double beta2, double eps, double weight_decay,
                     int32_t* done, void* stream) {
  if (!g || !done) return fail("group and done must be non-NULL");
  if (g->n_tensors < 1 || g->n_tensors > ACATTN_ADAM_MAX_TENSORS) return fail("1 <= n_tensors <= ACATTN_ADAM_MAX_TENSORS");
  int64_t blocks = 0;
  for (int t = 0; t < g->n_tensors; ++t) {
    if (!g->param[t] || !g->grad[t] || !g->exp_avg[t] || !g->exp_avg_sq[t] || !g->step[t])
      return fail("param, grad, exp_avg, exp_avg_sq and step of every tensor must be non-NULL");
    if (g->numel[t] < 1) return fail("numel must be positive");
    blocks += (g->numel[t] + 4095) / 4096;
  }
  if (blocks >= (1ll << 31)) return fail("too many elements for one launch");
  if (!(beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1)) return fail("betas must lie in [0, 1)");
  const int rc = acattn_launch_adam_step(*g, lr, beta1, beta2, eps, weight_decay, done, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_adam_step_cached(const acattn_adam_group* g, double lr, double beta1, double beta2, double eps, double weight_decay,
                            int32_t* done, void* cache, void* stream) {
  if (!g || !done || !cache) return fail("group, done and cache must be non-NULL");
  if (((uintptr_t)cache & 15) != 0) return fail("cache must be 16-byte aligned");
  if (g->n_tensors < 1 || g->n_tensors > ACATTN_ADAM_MAX_TENSORS) return fail("1 <= n_tensors <= ACATTN_ADAM_MAX_TENSORS");
  int64_t trips = 0;
  for (int t = 0; t < g->n_tensors; ++t) {
    if (!g->param[t] || !g->grad[t] || !g->exp_avg[t] || !g->exp_avg_sq[t] || !g->step[t])
      return fail("param, grad, exp_avg, exp_avg_sq and step of every tensor must be non-NULL");
    if (g->numel[t] < 1) return fail("numel must be positive");
    trips += (g->numel[t] + 1023) / 1024;
  }
  if (trips >= (1ll << 30)) return fail("too many elements for one launch");
  if (!(beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1)) return fail("betas must lie in [0, 1)");
  const int rc = acattn_launch_adam_step_cached(*g, lr, beta1, beta2, eps, weight_decay, done, cache, (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_select_adam_grid(int workgroups) {
  if (workgroups < 0 || workgroups > (1 << 20)) return fail("workgroups: 0 (by the device's compute units) or a positive count");
  return acattn_select_adam_grid_choice(workgroups);
}

int64_t acattn_linear_wgrad_workspace_bytes(int64_t M, int32_t K, int32_t N) {
  if (M < 1 || K < 1 || N < 1) return fail("M, K, N must be positive");
  return acattn_linear_wgrad_ws_bytes(M, K, N);
}

int acattn_linear_wgrad_grouped(const float* const* x, const float* const* dy, const int32_t* K, const int32_t* N,
                                float* const* dw, float* const* db, int32_t n_items, int64_t M, void* workspace,
                                void* stream) {
  if (!x || !dy || !K || !N || !dw || !db || !workspace) return fail("x, dy, K, N, dw, db and workspace must be non-NULL");
  if (n_items < 1 || n_items > ACATTN_WGRAD_MAX_GROUP) return fail("n_items must lie in [1, ACATTN_WGRAD_MAX_GROUP]");
  if (M < 1) return fail("M must be positive");
  for (int i = 0; i < n_items; ++i) {
    if (!x[i] || !dy[i] || !dw[i]) return fail("every item needs x, dy and dw");
    if (K[i] < 1 || N[i] < 1) return fail("K and N must be positive");
    if (M * (int64_t)std::max(K[i], N[i]) >= (1LL << 40)) return fail("matrix too large");
  }
  const int rc = acattn_launch_linear_wgrad(x, dy, (const int*)K, (const int*)N, dw, db, n_items, M, workspace,
                                            (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_linear_wgrad_grouped_partial(const float* const* x, const float* const* dy, const int32_t* K, const int32_t* N,
                                        const int32_t* want_bias, int32_t n_items, int64_t M, void* workspace, int32_t* n_partials,
                                        int64_t* w_offset, int64_t* b_offset, void* stream) {
  if (!x || !dy || !K || !N || !want_bias || !workspace || !n_partials || !w_offset || !b_offset)
    return fail("x, dy, K, N, want_bias, workspace, n_partials, w_offset and b_offset must be non-NULL");
  if (n_items < 1 || n_items > ACATTN_WGRAD_MAX_GROUP) return fail("n_items must lie in [1, ACATTN_WGRAD_MAX_GROUP]");
  if (M < 1) return fail("M must be positive");
  float* dw[ACATTN_WGRAD_MAX_GROUP];
  float* db[ACATTN_WGRAD_MAX_GROUP];
  for (int i = 0; i < n_items; ++i) {
    if (!x[i] || !dy[i]) return fail("every item needs x and dy");
    if (K[i] < 1 || N[i] < 1) return fail("K and N must be positive");
    if (M * (int64_t)std::max(K[i], N[i]) >= (1LL << 40)) return fail("matrix too large");
    dw[i] = nullptr;                                   // (stage 1 writes partials only; db != NULL = "bias partials wanted")
    db[i] = want_bias[i] ? (float*)workspace : nullptr;
  }
  int P = 0;
  long long wo[ACATTN_WGRAD_MAX_GROUP], bo[ACATTN_WGRAD_MAX_GROUP];
  const int rc = acattn_launch_linear_wgrad(x, dy, (const int*)K, (const int*)N, dw, db, n_items, M, workspace,
                                            (hipStream_t)stream, &P, wo, bo);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  *n_partials = P;
  for (int i = 0; i < n_items; ++i) {
    w_offset[i] = wo[i];
    b_offset[i] = bo[i];
  }
  return rc;
}

int acattn_linear_wgrad_reduce_many(const float* const* part_w, const float* const* part_b, const int32_t* K, const int32_t* N,
                                    const int32_t* n_partials, float* const* dw, float* const* db, int32_t n_items,
                                    const float* const* sum_x, float* const* sum_out, const int32_t* sum_R, const int32_t* sum_C,
                                    int32_t n_sums, void* stream) {
  if (n_items < 0 || n_items > ACATTN_WGRAD_MAX_REDUCE) return fail("n_items must lie in [0, ACATTN_WGRAD_MAX_REDUCE]");
  if (n_sums < 0 || n_sums > ACATTN_SUMROWS_MAX_DEFER) return fail("n_sums must lie in [0, ACATTN_SUMROWS_MAX_DEFER]");
  if (n_items + n_sums < 1) return fail("nothing to reduce");
  if (n_items > 0 && (!part_w || !part_b || !K || !N || !n_partials || !dw || !db)) return fail("every weight-gradient array must be non-NULL");
  if (n_sums > 0 && (!sum_x || !sum_out || !sum_R || !sum_C)) return fail("every row-sum array must be non-NULL");
  for (int i = 0; i < n_sums; ++i)
    if (!sum_x[i] || !sum_out[i] || sum_R[i] < 1 || sum_C[i] < 1) return fail("every row sum needs x, out and positive sizes");
  for (int i = 0; i < n_items; ++i) {
    if (!part_w[i] || !dw[i]) return fail("every item needs its partials and dw");
    if (db[i] && !part_b[i]) return fail("db given without bias partials");
    if (K[i] < 1 || N[i] < 1 || n_partials[i] < 1) return fail("K, N and n_partials must be positive");
  }
  const int rc = acattn_launch_linear_wgrad_reduce_many(part_w, part_b, (const int*)K, (const int*)N, (const int*)n_partials, dw, db,
                                                        n_items, sum_x, sum_out, (const int*)sum_R, (const int*)sum_C, n_sums,
                                                        (hipStream_t)stream);
  if (rc > 0) snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString((hipError_t)rc));
  return rc;
}

int acattn_linear_wgrad(const float* x, const float* dy, int64_t M, int32_t K, int32_t N, void* workspace, float* dw,
                        float* db, void* stream) {
  return acattn_linear_wgrad_grouped(&x, &dy, &K, &N, &dw, &db, 1, M, workspace, stream);
}

}  // extern "C"
