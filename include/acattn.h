/*
 * acattn.h -- C ABI of the MI355X-native calibrated multi-head self-attention core of AC-TSR.
 *
 * The reference (AIM-SE/AC-TSR, a RecBole fork) has no native / FFI boundary: its hot path is a
 * chain of ATen ops dispatched from Python.  This header defines the boundary
 * a maintainer would bind instead: plain pointers + sizes, no torch types.  Every entry point names
 * the reference code it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - all tensors fp32, contiguous, row-major, resident in device (HBM) memory of the current HIP
 *     device; ids / validity flags uint8;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls only enqueue work,
 *     never synchronise, never allocate (hipGraph-capturable);
 *   - inputs are borrowed for the duration of the enqueued work and never written;
 *     outputs are caller-allocated;
 *   - return value 0 = ok; negative = argument error (nothing enqueued), see acattn_last_error();
 *     positive = hipError_t from the launch.
 *
 * Shapes: B batch, L sequence length, H hidden size, nh heads, dh = H / nh.
 * Supported: dh in {16, 32, 64, 128}, 1 <= L <= 496 (acattn_max_sequence_length()).  L <= 208 runs the kernels that hold a
 * query block's row of 13 key tiles in registers; 208 < L <= 496 runs the long forms (ACATTN_FWD_LONG / ACATTN_BWD_LONG:
 * key tiles in a run-time loop), which refuse, with an error text that names the option: two_level == 0, the four
 * optional probability dumps of acattn_fwd_out, and in the backward dgate_summed, the second cotangent set (dqa2 ...) and a
 * NULL workspace, and p_drop > 0.95 (their calibrated soft-max takes a fixed shift: its arguments reach e / (1 - p_drop), and
 * exp overflows fp32 from p_drop = 0.967 on).  acattn_spatial_attention_bwd stays at L <= 208.
 */
#ifndef ACATTN_H_
#define ACATTN_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACATTN_ABI_VERSION 34

/* attention-mask encodings (recbole/model/abstract_recommender.py:136-143 builds the dense form) */
enum {
  ACATTN_MASK_STRUCTURED = 0, /* key_valid[B,L] (item_seq != 0) + `causal` flag; 0 / -10000 derived in-kernel */
  ACATTN_MASK_DENSE_LL = 1,   /* additive mask[B,L,L]  (the reference's [B,1,L,L]) */
  ACATTN_MASK_DENSE_L = 2     /* additive mask[B,L]    (the reference's [B,1,1,L], AcBERT4Rec acbert4rec.py:173) */
};

/* combine_option of AttackRTransformerLayer.combine_attention (recbole/model/layers.py:883-896) */
enum { ACATTN_COMBINE_FIXED = 0, ACATTN_COMBINE_GATE = 1, ACATTN_COMBINE_ANNEALING = 2 };

/* rich_calibrated_combine, used only when two_level == 0 (recbole/model/layers.py:929-936) */
enum { ACATTN_RICH_NONE = 0, ACATTN_RICH_FIXED = 1, ACATTN_RICH_TRAINABLE = 2 };

/* source of the layer's randomness (recbole/model/layers.py:672,736,917) */
enum {
  ACATTN_RNG_EXPLICIT = 0, /* noise / keep masks are read from the tensors below (parity mode) */
  ACATTN_RNG_COUNTER = 1   /* generated in-kernel from (seed, element index); reproducible, see acattn_rng_materialize */
};

#define ACATTN_NSTAT 8 /* floats per (b, head, query row) in `row_stats` */

typedef struct acattn_problem {
  int32_t B, L, H, n_heads;
  /* projected activations, [B,L,H] each */
  const float* q;  /* mixed_query_layer  = query(x)                      layers.py:687 */
  const float* k;  /* mixed_key_layer    = key(x)                        layers.py:688 */
  const float* v;  /* mixed_value_layer  = value(x)                      layers.py:689 */
  const float* qa; /* attack_query_transform(mixed_query)  (NULL if !adversarial)   layers.py:658 */
  const float* ka; /* attack_key_transform(mixed_key)      (NULL if !adversarial)   layers.py:659 */
  const float* gate_logits; /* gate(mixed_query) BEFORE the sigmoid, [B,L,L]; combine GATE only   layers.py:887 */
  /* attention mask */
  int32_t mask_mode;        /* ACATTN_MASK_* */
  int32_t causal;           /* STRUCTURED only: 1 = tril (SASRec), 0 = bidirectional */
  const uint8_t* key_valid; /* STRUCTURED: [B,L] */
  const float* mask;        /* DENSE_*: additive mask */
  /* spatial calibrator parameters (device pointers; NULL weight = term disabled)  layers.py:636-640 */
  const float* w_order; /* order_affine.weight    [2*dh] */
  const float* b_order; /* order_affine.bias      [1]    */
  const float* w_dist;  /* distance_affine.weight [2*dh] */
  const float* b_dist;  /* distance_affine.bias   [1]    */
  const float* scalar;  /* scalar                 [1]    */
  /* adversarial calibrator options */
  int32_t adversarial; /* 0 = spatial calibrator only: ctx_calibrated = after_spatial . V, nothing else written */
  int32_t combine_option; /* ACATTN_COMBINE_* */
  float anneal_rate;      /* ANNEALING: exp(-step/1e5), computed by the caller (layers.py:890) */
  int32_t two_level;      /* layers.py:911-914 */
  int32_t rich_combine;   /* ACATTN_RICH_* (two_level == 0 only) */
  const float* rich_ratio; /* TRAINABLE: rich_calibrated_combine_ratio [1] */
  /* randomness */
  int32_t rng_mode; /* ACATTN_RNG_* */
  float p_drop;     /* attn_dropout_prob; 0 = no dropout (eval mode) */
  const float* noise;         /* EXPLICIT: [B,nh,L,L] standard normal draws          layers.py:917 */
  const uint8_t* keep_after;  /* EXPLICIT: [B,nh,L,L] 0/1 keep mask or NULL           layers.py:736 (after_spatial) */
  const uint8_t* keep_before; /* EXPLICIT: [B,nh,L,L] or NULL                        layers.py:736 (before_spatial) */
  const uint8_t* keep_mask;   /* EXPLICIT: [B,nh,L,L] or NULL                        layers.py:672 */
  uint64_t seed;              /* COUNTER */
  const uint64_t* seed_device; /* COUNTER, optional: *seed_device (device memory) is added to `seed` when the kernel
                                  starts -- lets a captured hipGraph draw fresh randomness on every replay */
  /* ---- optional per-row products of the PRODUCER of q / k / gate (ABI 26) ------------------------------------------
   * Both are O(L H) work that belongs with the projections; the core re-derives them 2-4 times per sequence when they
   * are absent (once per head for the gate, once per query block for the key halves).  acattn_projections_fwd writes
   * both; acattn_spatial_affines() computes `affine` from q, k and the calibrator parameters for any other producer. */
  const float* affine;  /* NULL, or [B,nh,4,LP] with LP = 16*ceil(L/16): the rank-1 halves of the two spatial affines
                           of layers.py:705-708, affine(q_i || k_j) = q_i.w[:dh] + k_j.w[dh:] + b:
                             plane 0 [i] = -log2(e) * (q_i . w_order[:dh] + b_order)     (sigmoid(o) = 1/(1+exp2(p0+p2)))
                             plane 1 [i] =             q_i . w_dist[:dh]  + b_dist
                             plane 2 [j] = -log2(e) *  k_j . w_order[dh:]
                             plane 3 [j] =             k_j . w_dist[dh:]
                           entries L..LP-1 must be finite (zeros). */
  int32_t gate_is_prob; /* non-zero: `gate_logits` holds sigmoid(gate(mixed_query)) (layers.py:887: one sigmoid per
                           (b, i, j), shared by the heads) instead of the logits; d gate_logits of the backward is
                           still the gradient of the LOGITS */
} acattn_problem;

/* Non-finite inputs: a NaN in a valid row of q, k, v, qa, ka or the gate comes out as NaN in the context rows (and, for qa /
 * ka, the attack-mask rows) that row feeds, in every forward kernel -- the streaming kernel's translation units are built with
 * -fno-honor-nans (no canonicalising v_max in front of the row maxima), which does not change that
 * (tests/test_hip_onehop.py::test_a_nan_in_the_inputs_reaches_the_outputs_of_the_streaming_forward).  Rows of PADDED positions
 * (key_valid == 0) are never read by a masked soft-max in the kernels for L <= 208, whereas the reference's additive -10000
 * would propagate a NaN sitting there.  The long forms (ACATTN_FWD_LONG / ACATTN_BWD_LONG, every L > 208) ADD the mask as
 * the reference does: they read K, Ka and V of padded keys inside the key tiles they visit and give them a weight of zero, so
 * a NaN or Inf at a padded position reaches the outputs of the query blocks that visit its tile, as in the reference. */
typedef struct acattn_fwd_out {
  float* ctx_attacked;   /* [B,L,H] head-merged perturbed_attention . V        layers.py:677-680 via :938 */
  float* ctx_calibrated; /* [B,L,H] head-merged combined attention . V         layers.py:677-680 via :942 */
  float* attack_mask;    /* [B,nh,L,L] M as returned by the layer (after dropout)  layers.py:915,951 */
  float* row_stats;      /* [B,nh,L,ACATTN_NSTAT] log-normalisers for the backward, or NULL */
  /* optional probability dumps, [B,nh,L,L] each, NULL = skip (return_all_attention_prob, layers.py:899-927) */
  float* after_spatial;
  float* before_spatial;
  float* perturbed_attention;
  float* calibrated_attention;
  /* ABI 26, optional (adversarial form only): [B, nh, ceil(L/16)] -- acattn_mask_penalty_rows of attack_mask, i.e.
   * sum (1 - M)^2 over each query block's rows and all L keys.  The streaming forward (L > 64; L <= 64 at p_drop = 0.5) sums the
   * M block it stages for its store; for every other kernel the entry point runs acattn_mask_penalty_rows behind the
   * launch.  Always filled when given; the two ways differ in the order of the sum only. */
  float* penalty_part;
} acattn_fwd_out;

typedef struct acattn_bwd_io {
  /* forward results the backward re-uses */
  const float* attack_mask; /* [B,nh,L,L] as written by the forward */
  const float* row_stats;   /* [B,nh,L,ACATTN_NSTAT] */
  /* cotangents (NULL = zero) */
  const float* d_ctx_attacked;   /* [B,L,H] */
  const float* d_ctx_calibrated; /* [B,L,H] */
  const float* d_attack_mask;    /* [B,nh,L,L] */
  /* gradients, caller-allocated, fully overwritten */
  float* dq;  /* [B,L,H] */
  float* dk;  /* [B,L,H] */
  float* dv;  /* [B,L,H] */
  float* dqa; /* [B,L,H] */
  float* dka; /* [B,L,H] */
  float* dgate_logits; /* [B,nh,L,L] per-head partials of d gate_logits (combine GATE; the caller sums over heads) or NULL */
  /* per-(b,head) partial sums of the small parameters; the caller reduces over (B, nh) */
  float* dw_order_part; /* [B,nh,2*dh] */
  float* dw_dist_part;  /* [B,nh,2*dh] */
  float* dsmall_part;   /* [B,nh,4]: d b_order, d b_dist, d scalar, d rich_ratio */
  int32_t part_stride;  /* row stride (floats) of the three partial buffers; 0 = dense (2*dh, 2*dh, 4).  With a
                           common stride the three may be column ranges of ONE [B*nh, stride] buffer, which the
                           caller then reduces in a single pass */
  const uint32_t* active_qblocks; /* optional hint [B]: bit q set = some query row in [16q, 16q+16) of that sequence
                           has a non-zero cotangent (d_ctx_*); blocks with a clear bit are skipped and their dq, dqa,
                           gate partials written as zeros.  With d_attack_mask given no block is skipped, but one with a
                           clear bit only owes the soft-max of the mask scores (dqa, dka).  NULL = all active.
                           A hint, not a mask: a kernel may ignore it (the skipped work multiplies zeros anyway). */
  int32_t attack_only;  /* non-zero: the caller will read ONLY dqa and dka (pass 2 of the two-pass trainer through a
                           layer with no attack transform upstream, recbole/trainer/trainer.py:678-684); every other
                           output buffer must still be valid memory but may be left unwritten.  A hint like the above. */
  void* workspace;      /* device scratch of acattn_calibrated_attention_bwd_workspace_bytes(p) bytes (contents irrelevant;
                           8 floats per (b, head, query row) for the streaming pair, 16 where the long form runs: L > 208,
                           or ACATTN_BWD_LONG pinned by the thread that asks).  Optional for L <= 208: with it, L > 64
                           takes the streaming two-kernel backward (acattn_bwd_stream.hip), NULL = the row-resident
                           kernels only.  REQUIRED by the long form: NULL there is an error. */
  const int64_t* read_rows; /* the same hint as active_qblocks in its raw form: [B, n_read_rows] positions whose context
                           cotangents are the only non-zero ones (item_seq_len - 1 of abstract_recommender.py:130-134).
                           Consulted when active_qblocks is NULL; NULL = all active.  PRECONDITION: 0 <= position < L
                           (the reference's gather raises an index error otherwise); the kernels clamp a position
                           outside that range into it rather than touch another sequence's memory. */
  int32_t n_read_rows;
  const float* d_penalty_part; /* ABI 26, optional: [B, nh, ceil(L/16)] cotangent of acattn_mask_penalty_rows' sums.  The
                           kernels then add d M = 2 * d_penalty_part[b, head, query block] * (M - 1) to the mask cotangent
                           from the M tile they rebuild -- the mask penalty's gradient (acsasrec.py:131-137) without a
                           dense [B,nh,L,L] cotangent.  Like d_attack_mask it keeps every query block active. */
  int32_t dgate_summed; /* ABI 27, request: `dgate_logits` is [B,L,L] and receives the gate-logit gradient SUMMED over the heads
                           (the gate is shared by them, layers.py:887 unsqueeze(1)) instead of [B,nh,L,L] per-head partials.
                           Honoured by the one-row form of the backward only (one read position per sequence,
                           acattn_bwd_io.read_rows with n_read_rows == 1: of each sequence's L x L gate gradient ONE row is
                           non-zero, and writing nh dense partials of it -- 164 MB of zeros at B = 512, L = 200, 2 heads --
                           plus summing them was most of that launch): ask acattn_calibrated_attention_bwd_gate_summed()
                           first; a launch that cannot honour the request fails instead of misreading the buffer. */
  /* ABI 27, optional: a SECOND cotangent set evaluated in the same launch (the single-pass combined backward of the two-pass
   * protocol, recbole/trainer/trainer.py:672-686: the calibrated loss's cotangents above, the attacked loss's here).  The
   * backward is linear in its cotangents and both sets need the same rebuilt probability tiles; the second set is taken in
   * the form the attacked loss has in a layer with no attack transform upstream: d ctx_calibrated2 [B,L,H] and / or
   * d_penalty_part2 [B,nh,ceil(L/16)], no attacked-context and no dense mask cotangent, and of its gradients dqa2, dka2
   * ([B,L,H], fully overwritten) alone.  Honoured by the streaming kernels (needs `workspace`) when the FIRST set has no
   * d_ctx_attacked either and no block hints are given: ask acattn_calibrated_attention_bwd_pair_supported() first; a launch
   * that cannot honour a non-NULL dqa2 fails. */
  const float* d_ctx_calibrated2;
  const float* d_penalty_part2;
  float* dqa2;
  float* dka2;
} acattn_bwd_io;

/* Full-catalogue cross-entropy: ACSASRec._cal_loss for loss_type 'CE',
 * recbole/model/sequential_recommender/acsasrec.py:117-120, without materialising the [B, N] logits. */
typedef struct acattn_ce_problem {
  int32_t B, N, H;       /* rows (sequences), catalogue size, hidden size (64, 128 or 256) */
  const float* out;      /* [B,H] sequence representations (attacked_output / calibrated_output)  acsasrec.py:101-103 */
  const float* table;    /* [N,H] item_embedding.weight                                           acsasrec.py:117 */
  const int64_t* target; /* [B]   pos_items                                                      acsasrec.py:108 */
  /* backward only: how `coef` (d loss / d row_loss) is read.  coef_is_scalar: coef[0] holds for every row (the
   * cotangent of a mean, nn.CrossEntropyLoss's default reduction: acsasrec.py:119); coef_scale multiplies it
   * (1 / B of that mean), 0 = 1. */
  int32_t coef_is_scalar;
  float coef_scale;
} acattn_ce_problem;

/* Bytes of scratch both CE entry points need (caller-allocated device memory, contents irrelevant). */
int64_t acattn_full_sort_ce_workspace_bytes(const acattn_ce_problem* p);

/* lse[b] = logsumexp_n(out_b . table_n);  row_loss[b] = lse[b] - out_b . table_target(b).
 * mean(row_loss) == CrossEntropyLoss(out @ table^T, target)   (acsasrec.py:118-120). */
int acattn_full_sort_ce_fwd(const acattn_ce_problem* p, void* workspace, float* lse, float* row_loss, void* stream);

/* The forward plus dir[b] = softmax_b . table - table_target(b) = d row_loss[b] / d out_b in ONE sweep of the table
 * (flash-attention with K = V = the item table): for a loss whose table gradient is never taken -- the attacked loss
 * of the two-pass trainer (recbole/trainer/trainer.py:678-684) -- the backward is then d_out = coef[:, None] * dir, an
 * elementwise product, and the second sweep of acattn_full_sort_ce_bwd disappears.  Returns -100 (no error text)
 * when B is too large for its per-workgroup slabs (~96 MB); use _fwd and _bwd then. */
int acattn_full_sort_ce_fwd_dir(const acattn_ce_problem* p, void* workspace, float* lse, float* row_loss, float* dir,
                                void* stream);

/* [ABI 34] The forward of two row sets over ONE sweep of the table: set a (`pa`) gets what acattn_full_sort_ce_fwd_dir
 * gives (bit for bit), set c (`pc`) what acattn_full_sort_ce_fwd gives (its partial sums are grouped per workgroup instead
 * of per wave pair).  The attacked and the calibrated loss of a training step (acsasrec.py:123-138) are such a pair: same
 * table, same targets, different rows.  pa and pc must share table, N and H; B and target may differ.  Four launches
 * (row split, sweep, finish; the caller's acattn_attacked_loss_finish_rows_pair) replace eight.
 * Both return -100 (no error text) when the paired form does not apply -- hidden size other than 64, the exact-fp32
 * products or a catalogue the split sweeps do not take, set a's slabs beyond their budget, different tables -- and
 * the caller falls back to the two separate calls.  `workspace`: acattn_full_sort_ce_fwd_pair_workspace_bytes bytes. */
int64_t acattn_full_sort_ce_fwd_pair_workspace_bytes(const acattn_ce_problem* pa, const acattn_ce_problem* pc);
int acattn_full_sort_ce_fwd_pair(const acattn_ce_problem* pa, const acattn_ce_problem* pc, void* workspace, float* lse_a,
                                 float* row_loss_a, float* dir_a, float* lse_c, float* row_loss_c, void* stream);

/* Gradients of sum_b coef[b] * row_loss[b]: d_out [B,H] always; d_table [N,H] (fully overwritten) unless NULL. */
int acattn_full_sort_ce_bwd(const acattn_ce_problem* p, const float* lse, const float* coef, void* workspace,
                            float* d_out, float* d_table, void* stream);

/* [ABI 28] How the three products of the full-catalogue cross-entropy are evaluated at hidden 64 (acattn_ce_bf16.hip).
 * gfx950's fp32 matrix instruction runs at 1/16 of the bf16 one, so the default splits every fp32 operand exactly
 * into three bf16 numbers and evaluates a product as the six bf16 MFMAs whose dropped remainder is below 2^-23 of
 * |a||b| -- one fp32 rounding; results are as close to fp64 as the exact-fp32 kernels' (tests/test_hip_ce.py).
 *   ACATTN_CE_PRODUCTS_FP32 (0)    exact fp32 MFMA everywhere (round 3's kernels; also ACATTN_CE_PRODUCTS=fp32)
 *   ACATTN_CE_PRODUCTS_DEFAULT (1) the split sweeps for catalogues of more than 65,536 items (waves of six item tiles: one
 *                                  round of workgroups up to 98,304 items, one round + leftover tiles up to 102,400 --
 *                                  the benchmark's 100,000 --, several rounds beyond), the fp32 kernels below
 *   ACATTN_CE_PRODUCTS_ALL (2)     the split sweeps for every catalogue size (tests)
 * Process-wide; returns the previous mode; any other value only queries.  Non-finite inputs: an infinite operand splits
 * into inf + nan, so an infinite logit becomes NaN instead of inf (the loss is non-finite either way). */
#define ACATTN_CE_PRODUCTS_FP32 0
#define ACATTN_CE_PRODUCTS_DEFAULT 1
#define ACATTN_CE_PRODUCTS_ALL 2
int acattn_full_sort_ce_products(int mode);

/* Full-sort evaluation for leave-one-out data (one positive per row) without the [B, N] scores (acattn_rank.hip):
 *   rank[b] = 1 + #{ j in [first_item, N), j != target[b] : out_b . table_j ahead of out_b . table_target(b) }
 * Replaces, per evaluation batch, the dense scores of _full_sort_batch_eval and their masking
 * (recbole/trainer/trainer.py:926-945: full_sort_predict, scores[:, 0] = -inf, scores[history_index] = -inf) and the
 * top-K selection and gather of the collector (recbole/evaluator/collector.py:141-153): Hit / Recall / MRR / NDCG /
 * Precision of a row with one positive are functions of that rank alone.
 * `p` is read as for the cross-entropy: out [B,H], table [>= N,H], target [B]; N = the table rows that take part (a
 * model whose table carries a mask token behind the items passes n_items).  first_item = 1 leaves the padding item out
 * (trainer.py:942), 0 ranks every row of the table.
 * "Ahead" is !(s_j <= s_t) on exact-fp32 scores that have the same bits wherever they are formed: an item whose table
 * row equals the target's bit for bit is not ahead, a NaN item score is (torch.topk's order).  rank[b] = 0 marks an
 * invalid row: a target outside [first_item, N) (never read out of bounds) or a NaN target score; target_score[b] is NaN
 * for the former.  No float atomics; every output element has one writer; results do not depend on launch order.
 * `workspace`: acattn_full_sort_rank_workspace_bytes bytes (-1 for an unsupported problem), contents irrelevant.
 * Validation (before any HIP call, -1 and acattn_last_error): H not in {64, 128, 256}, B or N < 1, NULL pointers,
 * first_item outside [0, N). */
int64_t acattn_full_sort_rank_workspace_bytes(const acattn_ce_problem* p);
int acattn_full_sort_rank(const acattn_ce_problem* p, int32_t first_item, void* workspace, int32_t* rank, float* target_score,
                          void* stream);

/* History exclusion behind acattn_full_sort_rank (trainer.py:943-944, scores[history_index] = -inf): n_pairs UNIQUE
 * (pair_row[i], pair_item[i]) pairs become inadmissible -- each pair's score is formed by the routine that formed the
 * targets' and, where the sweep counted it as ahead, takes 1 off rank[row] (integer atomics: deterministic).  Ignored:
 * rows outside [0, B), items outside [first_item, N), the target itself, rows with rank 0.  target_score and rank are
 * acattn_full_sort_rank's outputs for the same `p` and first_item.  n_pairs = 0 launches nothing. */
int acattn_full_sort_rank_exclude(const acattn_ce_problem* p, int32_t first_item, const int64_t* pair_row,
                                  const int64_t* pair_item, int64_t n_pairs, const float* target_score, int32_t* rank,
                                  void* stream);

/* 1 for the hidden sizes acattn_full_sort_rank takes (64, 128, 256), else 0. */
int acattn_full_sort_rank_supported(int32_t H);

/* y = LayerNorm(dropout(z) + residual) * gamma + beta   (the tail of both sub-blocks
 * of a layer -- recbole/model/layers.py:681-683 and :794-796).  Rows of H in {64, 128, 256} floats. */
#define ACATTN_LN_BWD_GRID 512 /* workgroups of the backward == rows of its dgamma/dbeta partial buffer */
typedef struct acattn_ln_problem {
  int32_t rows, H;
  int32_t residual_rows;  /* == rows, or a divisor of it when the residual is broadcast over a leading dimension */
  const float* z;         /* [rows,H] output of the dense layer (bias included) */
  const float* residual;  /* [residual_rows,H] */
  const float* gamma;     /* [H] LayerNorm.weight */
  const float* beta;      /* [H] LayerNorm.bias */
  float eps;              /* layer_norm_eps */
  float p_drop;           /* hidden_dropout_prob in training, 0 in eval */
  const uint8_t* keep;    /* optional explicit keep mask [rows,H]; NULL = counter RNG from (seed, seed_device) */
  uint64_t seed;
  const uint64_t* seed_device;
} acattn_ln_problem;

/* stats[rows,2] receives (mean, 1/std) per row for the backward. */
int acattn_dropout_add_layernorm_fwd(const acattn_ln_problem* p, float* y, float* stats, void* stream);

/* dz [rows,H] and dres [rows,H] may each be NULL; dgb_part is [ACATTN_LN_BWD_GRID, 2, H] partial sums of
 * (dgamma, dbeta), or NULL; the caller adds the partials (and folds dres when the residual was broadcast). */
int acattn_dropout_add_layernorm_bwd(const acattn_ln_problem* p, const float* dy, const float* stats, float* dz,
                                     float* dres, float* dgb_part, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * y = dropout(LayerNorm(item_embedding[idx] + position_embedding[position])): the front end of both models
 * (recbole/model/sequential_recommender/acsasrec.py:87-95, acbert4rec.py:163-171).  Rows of H in {64, 128, 256}. */
#define ACATTN_EMBED_BWD_CHUNKS 8 /* the backward runs L x 8 workgroups: leading dimension of its partial buffers */
typedef struct acattn_embed_problem {
  int32_t rows, L, H;     /* rows = B*L; row r sits at position r % L */
  int64_t n_table_rows;   /* rows of `table` (ids outside [0, n) are clamped, never dereferenced out of bounds) */
  const int64_t* idx;     /* [rows] item ids (item_seq, row-major [B,L]) */
  const float* table;     /* [n_table_rows,H] item_embedding.weight */
  const float* pos;       /* [>=L,H] position_embedding.weight, or NULL (use_position_embedding: False) */
  const float* gamma;     /* [H] LayerNorm.weight */
  const float* beta;      /* [H] LayerNorm.bias */
  float eps;              /* layer_norm_eps */
  float p_drop;           /* hidden_dropout_prob in training, 0 in eval (the dropout FOLLOWS the norm here) */
  const uint8_t* keep;    /* optional explicit keep mask [rows,H]; NULL = counter RNG from (seed, seed_device) */
  uint64_t seed;
  const uint64_t* seed_device;
  uint8_t* nonzero_out;   /* optional [rows]: receives idx != 0, the key-validity bytes of the structured mask
                             (abstract_recommender.py:137: attention_mask = item_seq != 0); forward only */
  int64_t hot_id_plus1;   /* ABI 27, backward only, 0 = none: id + 1 of ONE table row that a large share of the lookups hit
                             (AcBERT4Rec's mask token, acbert4rec.py:105-150: 20 % of all positions).  Its gradient rows are
                             summed inside each workgroup first and added with one atomic per column and workgroup: 20,480
                             float atomics per address on one row were 1.1 ms at B = 512, L = 200, H = 256. */
} acattn_embed_problem;

/* stats[rows,2] receives (mean, 1/std) per row for the backward. */
int acattn_embed_layernorm_fwd(const acattn_embed_problem* p, float* y, float* stats, void* stream);

/* d_table [n_table_rows,H] must be ZERO-INITIALISED by the caller: rows are accumulated with float atomics and rows
 * whose id == padding_idx are skipped (nn.Embedding(padding_idx=0): acsasrec.py:33); pass padding_idx = -1 for none.
 * d_pos_part [ACATTN_EMBED_BWD_CHUNKS, L, H] (or NULL) and dgb_part [ACATTN_EMBED_BWD_CHUNKS * L, 2, H] (or NULL)
 * receive partial sums of the position-embedding and (dgamma, dbeta) gradients; the caller adds the partials. */
int acattn_embed_layernorm_bwd(const acattn_embed_problem* p, const float* dy, const float* stats, int64_t padding_idx,
                               float* d_table, float* d_pos_part, float* dgb_part, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Within ABI 34 (additions only): the personalised front end of ACSSEPT,
 * y = dropout(LayerNorm(cat(item_embedding[idx], user_embedding[user] over L) + position_embedding[position]))
 * (recbole/model/sequential_recommender/acssept.py:120-131).  Columns [0, Di) of row r = b*L + l come from
 * table[idx[r]], columns [Di, H) from user_table[user[b]].  H in {64, 128, 256}; Di and H - Di positive multiples of 4
 * (a 16-byte lane never straddles the seam). */
typedef struct acattn_embed_user_problem {
  int32_t rows, L, H;     /* rows = B*L; row r sits at position r % L of sequence r / L */
  int32_t Di;             /* item_hidden_size: width of `table`; user_hidden_size = H - Di is the width of `user_table` */
  int64_t n_table_rows;   /* rows of `table` (ids outside [0, n) are clamped, never dereferenced out of bounds) */
  int64_t n_user_rows;    /* rows of `user_table` (clamped likewise) */
  const int64_t* idx;     /* [rows] item ids (item_seq, row-major [B,L]) */
  const int64_t* user;    /* [rows / L] user ids, one per sequence */
  const float* table;     /* [n_table_rows,Di] item_embedding.weight */
  const float* user_table;/* [n_user_rows,H-Di] user_embedding.weight */
  const float* pos;       /* [>=L,H] position_embedding.weight, or NULL (use_position_embedding: False) */
  const float* gamma;     /* [H] LayerNorm.weight */
  const float* beta;      /* [H] LayerNorm.bias */
  float eps;              /* layer_norm_eps */
  float p_drop;           /* hidden_dropout_prob in training, 0 in eval (the dropout FOLLOWS the norm) */
  const uint8_t* keep;    /* optional explicit keep mask [rows,H]; NULL = counter RNG from (seed, seed_device) */
  uint64_t seed;
  const uint64_t* seed_device;
  uint8_t* nonzero_out;   /* optional [rows]: receives idx != 0 (abstract_recommender.py:137); forward only */
} acattn_embed_user_problem;

/* 1 if the front end above takes hidden size H split at column Di, else 0 (acssept.py:33-35: H = item + user width). */
int acattn_embed_user_supported(int32_t H, int32_t Di);

/* acssept.py:120-131 in one launch.  stats[rows,2] receives (mean, 1/std) per row for the backward. */
int acattn_embed_user_layernorm_fwd(const acattn_embed_user_problem* p, float* y, float* stats, void* stream);

/* The backward of acssept.py:120-131.  d_item [n_table_rows,Di] and d_user [n_user_rows,H-Di] (each may be NULL) must be
 * ZERO-INITIALISED by the caller: rows are accumulated with float atomics; item rows whose id == item_padding_idx and
 * user rows whose id == user_padding_idx are skipped (nn.Embedding(padding_idx=0): acssept.py:57-59); pass -1 for none.
 * A user may occur in any number of sequences.  user_rows_ws: [rows,H-Di] floats of scratch, or NULL.  Given, the user
 * half of every row's gradient is stored there and a second small launch sums each sequence over its L positions before it
 * touches d_user (one atomic per sequence and column); NULL scatters per row like the item half (L atomics per address).
 * d_pos_part and dgb_part as in acattn_embed_layernorm_bwd ([ACATTN_EMBED_BWD_CHUNKS, L, H] and
 * [ACATTN_EMBED_BWD_CHUNKS * L, 2, H], or NULL). */
int acattn_embed_user_layernorm_bwd(const acattn_embed_user_problem* p, const float* dy, const float* stats,
                                    int64_t item_padding_idx, int64_t user_padding_idx, float* d_item, float* d_user,
                                    float* user_rows_ws, float* d_pos_part, float* dgb_part, void* stream);

/* out[bt, c] = sum_r x[bt, r, c]  (x is [batch, R, C] contiguous).  The reductions of the training step's backward:
 * bias gradients (sum over B*L rows), split-K slabs, per-(b,head) parameter partials, per-head gate gradients. */
int acattn_sum_rows(const float* x, float* out, int32_t batch, int32_t R, int32_t C, void* stream);
/* Two such reductions in one launch (independent shapes): the attention backward's parameter partials and its per-head
 * gate gradient (layers.py:887: the gate is shared by the heads) are summed together. */
int acattn_sum_rows_pair(const float* x1, float* out1, int32_t batch1, int32_t R1, int32_t C1, const float* x2, float* out2,
                         int32_t batch2, int32_t R2, int32_t C2, void* stream);

/* ABI 27: cross-entropy over MATERIALISED logits [rows, N] (the masked-slot loss of AcBERT4Rec, acbert4rec.py:201-209, at the
 * widths where the catalogue product is a library GEMM): `CrossEntropyLoss(reduction='none')` without the [rows, N]
 * log-probabilities torch writes in the forward and the zero-filled [rows, N] tensor its backward starts from.
 *   fwd: lse[r] = logsumexp_n logits[r, n]; row_loss[r] = lse[r] - logits[r, target[r]]  (NaN for a target outside [0, N))
 *   bwd: d_logits[r, n] = coef[r] * (exp(logits[r, n] - lse[r]) - [n == target[r]])       (one read, one write of [rows, N])
 * logits and d_logits contiguous fp32, target int64 [rows], lse / row_loss / coef fp32 [rows]. */
int acattn_dense_ce_fwd(const float* logits, int64_t rows, int64_t N, const int64_t* target, float* lse, float* row_loss,
                        void* stream);
int acattn_dense_ce_bwd(const float* logits, const float* lse, const int64_t* target, const float* coef, int64_t rows, int64_t N,
                        float* d_logits, void* stream);

/* ABI 27: the start of a (replayed) training step in ONE launch: up to ACATTN_MAX_COPIES device-to-device copies of the
 * batch tensors into the static buffers a captured hipGraph reads (recbole/trainer/trainer.py:661 interaction.to(device)
 * ends in such buffers here), `*counter += 1` when counter != NULL (the replay counter the in-kernel RNG adds to its
 * seeds), and last_row[b] = item_length[b] - 1 when both are given (the position the models read,
 * abstract_recommender.py:130-134; `item_length` is read from its SOURCE, so it may be one of the tensors being copied).
 * Sizes in bytes, any alignment; src[i] == dst[i] is skipped. */
#define ACATTN_MAX_COPIES 6
int acattn_step_inputs(const void* const* src, void* const* dst, const int64_t* bytes, int32_t n_copies, int64_t* counter,
                       const int64_t* item_length, int64_t* last_row, int32_t n_rows, void* stream);

/* The mask penalty || 1 - M ||_2 over a whole attack-mask tensor (torch.norm(1 - attack_mask, p=2):
 * recbole/model/sequential_recommender/acsasrec.py:131-137, acbert4rec.py:229-232) and its gradient
 * d_m = d_norm * (m - 1) / norm.  m has n floats (16-byte aligned); `workspace` holds
 * ACATTN_PENALTY_WS_FLOATS floats; norm, d_norm are device scalars. */
#define ACATTN_PENALTY_WS_FLOATS 1024
int acattn_mask_penalty_fwd(const float* m, int64_t n, float* workspace, float* norm, void* stream);
int acattn_mask_penalty_bwd(const float* m, const float* norm, const float* d_norm, int64_t n, float* d_m, void* stream);

/* The attacked loss of the two-pass protocol assembled in one launch (acsasrec.py:129-137):
 *     loss = -mean_b row_loss_b + weight * mean_l || 1 - M_l ||_2
 * acattn_mask_penalty_partial: partial sums of (1 - m)^2 over one mask into `part` (ACATTN_PENALTY_WS_FLOATS floats).
 * acattn_attacked_loss_finish: row_loss [B] from acattn_full_sort_ce_fwd[_dir]; part [n_masks, ACATTN_PENALTY_WS_FLOATS],
 *   every mask of mask_numel elements; out [2 + n_masks] = (loss, mean row loss, norm_0, ...).  scale_buf (or NULL,
 *   n_scale floats, at most a few 100k: one workgroup walks it) is multiplied by -1/B in place: pass the CE direction
 *   so that d loss / d out = scale_buf * d_loss.
 * acattn_mask_penalty_bwd_scaled: d_m = d_loss * scale * (m - 1) / norm, scale = weight / n_masks. */
int acattn_mask_penalty_partial(const float* m, int64_t n, float* part, void* stream);
int acattn_attacked_loss_finish(const float* row_loss, int32_t B, const float* part, int32_t n_masks, int64_t mask_numel,
                                float weight, float* out, float* scale_buf, int32_t n_scale, void* stream);
int acattn_mask_penalty_bwd_scaled(const float* m, const float* norm, const float* d_loss, float scale, int64_t n, float* d_m,
                                   void* stream);
/* The penalty through the attention node instead of through M [round 3]:
 * acattn_mask_penalty_rows: pen[b, head, qb] = sum over the rows of query block qb (16 rows) and all L keys of (1 - M)^2,
 *   M [B,nh,L,L] -> pen [B, nh, ceil(L/16)].  The sum of pen is || 1 - M ||_2 ^ 2.
 * acattn_attacked_loss_finish_rows: acattn_attacked_loss_finish with one pen vector (count floats) per mask in place of the
 *   partial-sum workspace.
 * acattn_mask_penalty_drows: d_pen[l][:] = d_loss * scale / (2 * norm_l) for every mask l (count floats each), i.e. the
 *   cotangent of pen under loss = ... + scale * sum_l sqrt(sum pen_l): feed it to acattn_bwd_io.d_penalty_part. */
int acattn_mask_penalty_rows(const float* m, int32_t B, int32_t n_heads, int32_t L, float* pen, void* stream);
int acattn_attacked_loss_finish_rows(const float* row_loss, int32_t B, const float* const* pen, int32_t n_masks, int32_t count,
                                     float weight, float* out, float* scale_buf, int32_t n_scale, void* stream);
/* [ABI 34] acattn_attacked_loss_finish_rows + mean_c[0] = mean(row_loss_c[0 .. B_c)) in the same launch, summed in a fixed
 * order (the calibrated loss behind acattn_full_sort_ce_fwd_pair, without a reduction launch of its own). */
int acattn_attacked_loss_finish_rows_pair(const float* row_loss, int32_t B, const float* const* pen, int32_t n_masks,
                                          int32_t count, float weight, float* out, float* scale_buf, int32_t n_scale,
                                          const float* row_loss_c, int32_t B_c, float* mean_c, void* stream);
int acattn_mask_penalty_drows(const float* norms, const float* d_loss, float scale, int32_t count, float* const* d_pen,
                              int32_t n_masks, void* stream);
/* [ABI 29] acattn_mask_penalty_drows + d_out[:] = direction[:] * d_loss[0] (n_dir floats; the attacked loss's output
 * cotangent from the direction acattn_full_sort_ce_fwd_dir saved, acsasrec.py:129-137) in the same launch. */
int acattn_mask_penalty_drows_dir(const float* norms, const float* d_loss, float scale, int32_t count, float* const* d_pen,
                                  int32_t n_masks, const float* direction, float* d_out, int32_t n_dir, void* stream);
/* The same two for all masks of a model (one per layer, each of n elements, at most ACATTN_MAX_MASKS) in ONE launch each:
 * part [n_masks, ACATTN_PENALTY_WS_FLOATS]; norms [n_masks] (the out + 2 of acattn_attacked_loss_finish). */
#define ACATTN_MAX_MASKS 8
int acattn_mask_penalty_partial_multi(const float* const* m, int32_t n_masks, int64_t n, float* part, void* stream);
int acattn_mask_penalty_bwd_scaled_multi(const float* const* m, const float* norms, const float* d_loss, float scale, int64_t n,
                                         float* const* d_m, int32_t n_masks, void* stream);

/* Parameter gradients of y = x W^T + b (torch.nn.functional.linear as called for query/key/value, the attack
 * transforms, dense, the gate and the feed-forward pair: recbole/model/layers.py:687-690, 660-661, 681, 792-794, 863):
 *   dw[N,K] = sum_m dy[m,n] x[m,k]      db[N] = sum_m dy[m,n]  (db may be NULL)
 * x [M,K] and dy [M,N] contiguous fp32, M = B*L rows; one pass over both, fp32 MFMA, deterministic two-stage
 * reduction.  `workspace` is caller-owned scratch of acattn_linear_wgrad_workspace_bytes(M, K, N) bytes. */
int64_t acattn_linear_wgrad_workspace_bytes(int64_t M, int32_t K, int32_t N);
int acattn_linear_wgrad(const float* x, const float* dy, int64_t M, int32_t K, int32_t N, void* workspace, float* dw,
                        float* db, void* stream);

/* The same for up to ACATTN_WGRAD_MAX_GROUP layers in ONE launch pair (the six projections of an encoder layer, or
 * dense + the feed-forward pair of a layer's tail, are differentiated together).  Item i has operands x[i] [M,K[i]],
 * dy[i] [M,N[i]] and results dw[i] [N[i],K[i]], db[i] [N[i]] (db[i] may be NULL); all items share M.  The arrays are
 * host arrays (of device pointers / sizes), read during the call.
 * `workspace`: sum_i acattn_linear_wgrad_workspace_bytes(M, K[i], N[i]) bytes. */
#define ACATTN_WGRAD_MAX_GROUP 8
int acattn_linear_wgrad_grouped(const float* const* x, const float* const* dy, const int32_t* K, const int32_t* N,
                                float* const* dw, float* const* db, int32_t n_items, int64_t M, void* workspace,
                                void* stream);

/* [ABI 29] The two stages of acattn_linear_wgrad_grouped separately.  A training step has one stage-2 launch per layer and
 * walk -- six 6-us launches at the benchmark shape for results that only the optimizer reads.  A trainer can launch stage 1
 * where the gradient is due (`_partial`: the items' partial sums go to `workspace`; `n_partials` and, per item, the offsets
 * in floats of its weight / bias partials inside `workspace` come back; want_bias[i] != 0 = bias partials wanted) and ONE
 * stage 2 for all of them when the backward walk is over (`_reduce_many`: up to ACATTN_WGRAD_MAX_REDUCE items, each with its
 * own partial pointers, sizes and partial count; db[i] may be NULL) -- which also takes up to ACATTN_SUMROWS_MAX_DEFER plain
 * row sums sum_out[i][c] = sum_r sum_x[i][r, c] (sum_x[i] contiguous [sum_R[i], sum_C[i]]: the LayerNorm / calibrator
 * parameter partials of the same walk, acattn_sum_rows with batch 1) as further slices of the same launch; either list may
 * be empty.  The workspaces must stay untouched in between. */
#define ACATTN_WGRAD_MAX_REDUCE 32
#define ACATTN_SUMROWS_MAX_DEFER 8
int acattn_linear_wgrad_grouped_partial(const float* const* x, const float* const* dy, const int32_t* K, const int32_t* N,
                                        const int32_t* want_bias, int32_t n_items, int64_t M, void* workspace, int32_t* n_partials,
                                        int64_t* w_offset, int64_t* b_offset, void* stream);
int acattn_linear_wgrad_reduce_many(const float* const* part_w, const float* const* part_b, const int32_t* K, const int32_t* N,
                                    const int32_t* n_partials, float* const* dw, float* const* db, int32_t n_items,
                                    const float* const* sum_x, float* const* sum_out, const int32_t* sum_R, const int32_t* sum_C,
                                    int32_t n_sums, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * The position-wise tail of one branch of an encoder layer in one launch (forward) / one launch (input gradients):
 *     a   = LayerNorm(dropout(dense(ctx)) + x)                  recbole/model/layers.py:681-683 (cal_adjusted_outputs)
 *     out = LayerNorm(dropout(dense_2(gelu(dense_1(a)))) + a)   recbole/model/layers.py:790-798 (FeedForward, erf-GELU)
 * Replaces 3 GEMM + 2 dropout/add/LayerNorm + 1 GELU launches.  (H, I) in {(64, 256), (64, 128), (128, 512), (128, 256),
 * (128, 64), (256, 1024)} (acattn_layer_tail_supported); weights are the
 * row-major nn.Linear parameters ([out, in]).  Dropout decisions are those of acattn_dropout_add_layernorm_* for
 * the same (seed, row, column). */
typedef struct acattn_tail_problem {
  int32_t rows, H, I;      /* rows = positions (B*L or the selected ones); H hidden_size; I inner_size */
  const float* ctx;        /* [rows,H] merged-head context (attention output before the dense) */
  const float* x;          /* [rows,H] the layer's input (residual of the first LayerNorm) */
  const float* wd;         /* [H,H] attack_attention.dense.weight */
  const float* bd;         /* [H] */
  const float* g1;         /* [H] attack_attention.LayerNorm.weight */
  const float* b1;         /* [H] */
  const float* w1;         /* [I,H] feed_forward.dense_1.weight */
  const float* bb1;        /* [I] */
  const float* w2;         /* [H,I] feed_forward.dense_2.weight */
  const float* bb2;        /* [H] */
  const float* g2;         /* [H] feed_forward.LayerNorm.weight */
  const float* b2;         /* [H] */
  float eps1, eps2;        /* layer_norm_eps of the two norms */
  float p1, p2;            /* hidden_dropout_prob of out_dropout / feed_forward.dropout in training, 0 in eval */
  const uint8_t* keep1;    /* optional explicit keep masks [rows,H]; NULL = counter RNG from (seed, seed_device) */
  const uint8_t* keep2;
  uint64_t seed1, seed2;
  const uint64_t* seed_device;
  /* Optional row selection: tail row r reads ctx / x at row (r / src_R) * src_L + src_index[r] (ctx, x are
   * [*, src_L, H]; src_index [rows] positions, e.g. item_seq_len - 1 of abstract_recommender.py:130-134 with
   * src_R = 1), and the backward ADDS the d_ctx / d_x rows there (a position may be picked twice): the caller
   * zero-fills those two.  NULL = identity. */
  const int64_t* src_index;
  int32_t src_R, src_L;
  /* ABI 31, optional: hidden 64 only, the weight planes acattn_layer_tail_split_weights wrote from THESE wd / w1 / w2
   * (acattn_layer_tail_split_bytes(H, I, rows) bytes, 16-byte aligned).  Given, the products run on bf16 matrix
   * instructions with exactly split operands (per element closer to fp64 than fp32, with a small negative mean error
   * that adds up in sums over many rows: DESIGN.md 4.7); NULL = the exact-fp32 kernels.  The
   * planes are a copy of the weights: after any change of wd / w1 / w2 they must be written again before use. */
  const void* split_planes;
} acattn_tail_problem;

/* Tensors the forward writes and the backward reads (all required in both directions, `act` forward only). */
typedef struct acattn_tail_saved {
  float* h1;   /* [rows,H] dense(ctx) + bias */
  float* st1;  /* [rows,2] (mean, 1/std) of the first norm */
  float* a;    /* [rows,H] output of the first norm */
  float* act;  /* [rows,I] gelu(dense_1(a)): operand of dense_2's weight gradient */
  float* h3;   /* [rows,H] dense_2(act) + bias */
  float* st2;  /* [rows,2] */
  float* out;  /* [rows,H] the branch's output */
  /* ABI 26, optional (NULL = off), hidden 128 only: [rows,I] gelu'(dense_1(a)).  When the forward is given it, the
   * backward given the same pointer reads it instead of rebuilding dense_1(a) (a fourth of its matrix work at that
   * width).  Ignored at hidden 64 (the rebuild is cheaper than the traffic there). */
  float* gelu_grad;
} acattn_tail_saved;

typedef struct acattn_tail_bwd_io {
  const float* d_out;  /* [rows,H] */
  float* d_ctx;        /* [rows,H] or NULL */
  float* d_x;          /* [rows,H] or NULL */
  float* d_h1;         /* [rows,H], d_h2 [rows,I], d_h3 [rows,H]: cotangents of the three dense outputs, i.e. the */
  float* d_h2;         /*   operands of acattn_linear_wgrad_grouped with (ctx, a, act); each may be NULL */
  float* d_h3;
  float* dgb_part;     /* [acattn_layer_tail_bwd_partial_rows(rows), 4, H] partial sums of (dgamma1, dbeta1, dgamma2,
                          dbeta2), to be summed over the leading dimension by the caller; or NULL.  Hidden 128 / 256:
                          acattn_layer_tail_bwd_partial_rows_for(rows, H) rows */
  void* workspace;     /* ABI 26: device scratch of acattn_layer_tail_bwd_workspace_bytes(H, I) bytes: transposed weight
                          copies live in it during the launch (every width but hidden 64 at <= 4096 rows needs it) */
} acattn_tail_bwd_io;

int acattn_layer_tail_supported(int32_t H, int32_t I);
int acattn_layer_tail_fwd(const acattn_tail_problem* p, const acattn_tail_saved* saved, void* stream);
/* [added within ABI 34: a new entry point, nothing existing changes] acattn_layer_tail_fwd(p_a, saved_a) and
 * acattn_layer_tail_fwd(p_b, saved_b) as ONE launch of twice the workgroups: the attacked and the calibrated tail of a
 * layer -- the same weights and planes, each with its own ctx, outputs, saved tensors and dropout seeds.  Every output is
 * bit for bit what the two single launches write.  Returns -100 (no error text) where the pair form does not apply --
 * hidden size other than 64, different inner sizes or row counts, no split planes, a row count that does not take the
 * four-wave form -- and the caller makes the two calls. */
int acattn_layer_tail_fwd_pair(const acattn_tail_problem* p_a, const acattn_tail_saved* saved_a, const acattn_tail_problem* p_b,
                               const acattn_tail_saved* saved_b, void* stream);
int acattn_layer_tail_bwd(const acattn_tail_problem* p, const acattn_tail_saved* saved, const acattn_tail_bwd_io* io,
                          void* stream);
int32_t acattn_layer_tail_bwd_partial_rows(int32_t rows);               /* hidden 64 */
int32_t acattn_layer_tail_bwd_partial_rows_for(int32_t rows, int32_t H); /* any supported hidden size */
int64_t acattn_layer_tail_bwd_workspace_bytes(int32_t H, int32_t I);
/* Measurement hook: rows per wave of the forward = 16 * nb (0 = chosen by size).  Returns the previous setting. */
int acattn_select_layer_tail_blocks(int nb);
/* ABI 31: bytes of the split weight planes of acattn_tail_problem.split_planes for a tail of `rows` rows, or 0 where the
 * exact-fp32 kernels run: hidden other than 64, rows of the staged form, acattn_linear_products(ACATTN_LINEAR_PRODUCTS_FP32)
 * or the environment variable ACATTN_TAIL_PRODUCTS=fp32 (the tails alone).  The answer may change with those settings:
 * ask before each forward. */
int64_t acattn_layer_tail_split_bytes(int32_t H, int32_t I, int32_t rows);
/* ABI 31: writes the planes of p->wd, p->w1, p->w2 (hidden 64) into `planes` (one launch on `stream`). */
int acattn_layer_tail_split_weights(const acattn_tail_problem* p, void* planes, void* stream);

/* ABI 33: the split planes of SEVERAL layers in ONE launch -- what an encoder forward needs of them, written once at its
 * head instead of once per autograd node (tails) and once per workgroup of every launch (projections).  Per layer either
 * half may be left out (its planes pointer NULL):
 *   tail_planes  acattn_tail_problem.split_planes of wd / w1 / w2 ([64,64], [I,64], [64,I], I = 256 or 128), bytewise what
 *                acattn_layer_tail_split_weights writes;
 *   proj_planes  acattn_proj_problem.split_planes of wq, wk, wv, waq, wak ([64,64]) and wg ([G,64], G <= 64, or NULL without
 *                the gate: its two slots are then left unwritten).  16-byte fragments [matrix][tile][K-block][plane][lane];
 *                forward image (A[m][k] = W[m][k]) in the order Wq, Waq, Wg, Wk, Wak, Wv, then the backward image
 *                (A[m][k] = W[k][m]) in the order Waq, Wg, Wq, Wak, Wk, Wv; gate rows / columns past G are zeros.
 * All planes pointers 16-byte aligned.  `layers` is a host array read during the call; at most ACATTN_SPLIT_MAX_LAYERS
 * entries per call. */
#define ACATTN_SPLIT_MAX_LAYERS 8
typedef struct acattn_split_layer {
  const float *wd, *w1, *w2;
  int32_t I;
  void* tail_planes;
  const float *wq, *wk, *wv, *waq, *wak, *wg;
  int32_t G;
  void* proj_planes;
} acattn_split_layer;
int acattn_split_weights_many(const acattn_split_layer* layers, int32_t n_layers, void* stream);
/* ABI 33: bytes of acattn_proj_problem.split_planes, or 0 where the projections do not run on split products: hidden other
 * than 64, a gate wider than 64, acattn_linear_products(ACATTN_LINEAR_PRODUCTS_FP32).  The answer may change with that
 * setting: ask before each forward. */
int64_t acattn_projections_split_bytes(int32_t H, int32_t G);

/* ------------------------------------------------------------------------------------------------------------------
 * The six projections in front of the attention core in one launch (forward) / one launch (input gradients):
 *     mq, mk, mv = query(x), key(x), value(x)                               recbole/model/layers.py:687-689
 *     qa, ka     = attack_query_transform(mq), attack_key_transform(mk)     recbole/model/layers.py:658-659
 *     gate       = gate(mq)  [rows, G], G = seq_length                      recbole/model/layers.py:887
 * hidden_size 64, 128 or 256, G <= 256; weights are the row-major nn.Linear parameters ([out, in]). */
typedef struct acattn_proj_problem {
  int32_t rows, H, G;        /* G = 0 and wg = bg = NULL without the gate (combine_option != 'gate') */
  const float* x;            /* [rows,H] the layer's input */
  const float *wq, *bq;      /* attack_attention.query */
  const float *wk, *bk;      /* attack_attention.key */
  const float *wv, *bv;      /* attack_attention.value */
  const float *waq, *baq;    /* attack_attention.attack_query_transform */
  const float *wak, *bak;    /* attack_attention.attack_key_transform */
  const float *wg, *bg;      /* gate [G,H], [G]; or NULL */
  /* ABI 26, only read when acattn_proj_out.affine is set: the spatial calibrator's parameters (layers.py:636-640), the
   * head count and the sequence length (rows = B * L, row r sits at position r % L of sequence r / L) */
  const float *w_order, *b_order, *w_dist, *b_dist; /* [2*dh], [1], [2*dh], [1] */
  int32_t n_heads, L;
  /* ABI 33, optional: hidden 64 with a gate of at most 64 outputs only, the weight planes acattn_split_weights_many wrote
   * from THESE six weights (acattn_projections_split_bytes(H, G) bytes, 16-byte aligned: the forward image, then the
   * transposed image of the backward).  Given, acattn_projections_fwd / _bwd read their weight fragments from the planes
   * (proj_planes_fwd_kernel / proj_planes_bwd_kernel: one wave per workgroup, no LDS image, no split of the weights inside
   * the launch); the products and every tensor written are bitwise those of the NULL form, which splits the weights
   * inside every workgroup.  The planes are a copy of the weights: after any change of a weight they must be written again
   * before use.  Planes given where these kernels do not run (acattn_linear_products(0) since they were made) are not read:
   * the launch takes the kernels it would take without them.  acattn_projections_qkv_fwd does not read the field. */
  const void* split_planes;
} acattn_proj_problem;

typedef struct acattn_proj_out {
  float *mq, *mk, *mv, *qa, *ka; /* [rows,H] each */
  float* gate;                   /* [rows,G] or NULL */
  /* ABI 26: what the attention core would otherwise re-derive per head / per query block (acattn_problem.affine,
   * .gate_is_prob) */
  float* affine;      /* NULL, or [B,nh,4,LP], LP = 16*ceil(L/16): entries [0, L) of every plane are written, the
                         padding entries are left alone (allocate the buffer zeroed once; they must be finite) */
  int32_t gate_prob;  /* non-zero: `gate` receives sigmoid(logits) instead of the logits */
} acattn_proj_out;

/* Cotangents in (each may be NULL = zero), gradients out (each may be NULL = not wanted):
 *   dmq_total = dmq + dqa . Waq + dgate . Wg     (cotangent operand of query's weight gradient; may alias dmq)
 *   dmk_total = dmk + dka . Wak                  (the same for key; may alias dmk)
 *   dx        = dmq_total . Wq + dmk_total . Wk + dmv . Wv */
typedef struct acattn_proj_bwd_io {
  const float *dmq, *dmk, *dmv, *dqa, *dka; /* [rows,H] */
  const float* dgate;                       /* [rows,G] */
  float *dmq_total, *dmk_total, *dx;        /* [rows,H] */
  /* [rows,H] or NULL: dx starts from it.  x also feeds the layer tails as the residual (layers.py:683): their d_x is
   * handed in here instead of being added to dx by a separate elementwise launch. */
  const float* dx_init;
  /* ABI 26: device scratch of acattn_projections_bwd_workspace_bytes(p) bytes (0 at hidden 64: may be NULL there); hidden
   * 128 / 256 keep transposed copies of the layer's weights in it for the duration of the launch */
  void* workspace;
} acattn_proj_bwd_io;

int acattn_projections_supported(int32_t H, int32_t G);
int64_t acattn_projections_bwd_workspace_bytes(const acattn_proj_problem* p);
int acattn_projections_fwd(const acattn_proj_problem* p, const acattn_proj_out* out, void* stream);
int acattn_projections_bwd(const acattn_proj_problem* p, const acattn_proj_bwd_io* io, void* stream);
/* [ABI 32] mq, mk, mv alone -- what a layer WITHOUT the adversarial calibrator needs: no attack transform and no gate is
 * evaluated.  Reads x, wq / bq, wk / bk, wv / bv (and, for out->affine, the spatial fields) of *p; writes out->mq, mk, mv
 * (and affine); out->qa, ka, gate must be NULL.  Served where acattn_projections_qkv_supported(H) answers 1: hidden 64 on
 * the split bf16 products (acattn_linear_products: the answer may change with that setting).  The input gradient is
 * acattn_projections_bwd with dqa = dka = dgate = NULL. */
int acattn_projections_qkv_supported(int32_t H);
int acattn_projections_qkv_fwd(const acattn_proj_problem* p, const acattn_proj_out* out, void* stream);

/* ABI 30: arithmetic of the hidden-64 projection products (acattn_projections_fwd / _bwd).  ACATTN_LINEAR_PRODUCTS_FP32:
 * the exact-fp32 matrix instruction; ACATTN_LINEAR_PRODUCTS_DEFAULT: bf16 matrix instructions on operands split exactly
 * into three bf16 planes (six products per pair, as accurate as fp32: DESIGN.md 4.6) wherever the gate has at most 64
 * outputs.  ABI 31: the same mode chooses the products of the hidden-64 layer tails (acattn_layer_tail_split_bytes
 * answers 0 in mode ACATTN_LINEAR_PRODUCTS_FP32).  Hidden 128 / 256 always use fp32.  The environment variable ACATTN_LINEAR_PRODUCTS=fp32 sets the initial mode.
 * Process-wide; returns the previous mode; any other value only queries. */
#define ACATTN_LINEAR_PRODUCTS_FP32 0
#define ACATTN_LINEAR_PRODUCTS_DEFAULT 1
int acattn_linear_products(int mode);

/*
 * torch.optim.Adam's update (the reference's optimizer: recbole/trainer/trainer.py:590-615, `learner: adam`) for up to
 * ACATTN_ADAM_MAX_TENSORS parameters in one launch: amsgrad = False, maximize = False, weight decay as in Adam (added to
 * the gradient).  Per tensor: fp32 param / grad / exp_avg / exp_avg_sq of `numel` elements and the step counter as a
 * device float (torch's `capturable` state layout).  The counters hold the number of updates done BEFORE the call and
 * are incremented by the launch.  `done`: a device int32 that is zero before the first call (the launch leaves it zero).
 * The arithmetic reproduces ATen's fused kernel operation by operation (csrc/acattn_adam.hip).
 */
#define ACATTN_ADAM_MAX_TENSORS 64
typedef struct acattn_adam_group {
  int32_t n_tensors;
  float* param[ACATTN_ADAM_MAX_TENSORS];
  const float* grad[ACATTN_ADAM_MAX_TENSORS];
  float* exp_avg[ACATTN_ADAM_MAX_TENSORS];
  float* exp_avg_sq[ACATTN_ADAM_MAX_TENSORS];
  float* step[ACATTN_ADAM_MAX_TENSORS];
  int64_t numel[ACATTN_ADAM_MAX_TENSORS];
} acattn_adam_group;
int acattn_adam_step(const acattn_adam_group* g, double lr, double beta1, double beta2, double eps, double weight_decay,
                     int32_t* done, void* stream);
/* [added within ABI 34: new entry points only, nothing existing changes, and tests/test_ce_pair_cpu.py pins the number]
 * The same update, bit for bit, by a persistent kernel: a fixed grid sized from the device's compute units walks
 * all tensors' 1,024-element chunks grid-stride with the next chunk's loads in flight under the current one's arithmetic,
 * and the two bias corrections (1 - beta1^step, sqrt(1 - beta2^step)) are read from `cache` instead of being recomputed by
 * every wave.  `cache`: ACATTN_ADAM_CACHE_BYTES of device memory, 16-byte aligned, zero before the first call, owned by one
 * optimizer (launches that share it are ordered by the stream).  The last workgroup to finish writes, per tensor slot, the
 * corrections of the NEXT step together with the step and the betas they belong to; an entry is used only when all three
 * equal the launch's (a zero entry never does: the corrected step is >= 1), otherwise the wave computes the corrections
 * itself -- a changed counter, beta or tensor list costs time, never a wrong value. */
#define ACATTN_ADAM_CACHE_BYTES (32 * ACATTN_ADAM_MAX_TENSORS)
int acattn_adam_step_cached(const acattn_adam_group* g, double lr, double beta1, double beta2, double eps, double weight_decay,
                            int32_t* done, void* cache, void* stream);
/* [added within ABI 34] Measurement / test hook: workgroups of acattn_adam_step_cached's grid (0 = from the device's compute units; the
 * environment variable ACATTN_ADAM_GRID sets the initial value).  Returns the previous setting. */
int acattn_select_adam_grid(int workgroups);

/* ABI 27: 1 when acattn_calibrated_attention_bwd(p, io) with io->dgate_summed = 1 will write the head-summed [B,L,L] gate
 * gradient (see acattn_bwd_io.dgate_summed), 0 when the launch needs the per-head [B,nh,L,L] buffer.  Validates nothing
 * else; every other field of `io` as for the launch itself (pointers are only tested for NULL). */
int acattn_calibrated_attention_bwd_gate_summed(const acattn_problem* p, const acattn_bwd_io* io);
/* ABI 27: 1 when the launch will evaluate the second cotangent set of `io` (see acattn_bwd_io.dqa2), else 0. */
int acattn_calibrated_attention_bwd_pair_supported(const acattn_problem* p, const acattn_bwd_io* io);

/* ABI version of the loaded library (== ACATTN_ABI_VERSION of the header it was built from). */
int acattn_abi_version(void);

/* Thread-local description of the last negative return value. */
const char* acattn_last_error(void);

/* Bytes of algorithmic HBM traffic of one forward call (DESIGN.md "Contract A"/"A'"): what bench.py prices. */
int64_t acattn_fwd_algorithmic_bytes(const acattn_problem* p);

/*
 * Fused calibrated attention, forward.  Replaces, for all heads of all sequences in one launch:
 *   raw scores + spatial calibrator + two softmaxes   recbole/model/layers.py:695-740
 *   attack-mask scores + softmax                       recbole/model/layers.py:661-672
 *   noise, perturbed / calibrated / combined probs     recbole/model/layers.py:917-936
 *   the two P.V products and head merge                recbole/model/layers.py:677-680
 */
int acattn_calibrated_attention_fwd(const acattn_problem* p, const acattn_fwd_out* out, void* stream);

/* The affine planes of acattn_problem.affine ([B,nh,4,16*ceil(L/16)], padding written as zeros) from p->q, p->k and the
 * spatial calibrator's parameters (recbole/model/layers.py:705-708 in rank-1 form), for a producer of q / k other than
 * acattn_projections_fwd.  Reads only B, L, H, n_heads, q, k, w_order, b_order, w_dist, b_dist of *p. */
int acattn_spatial_affines(const acattn_problem* p, float* affine, void* stream);

/* Backward of the above (what autograd derives for the same op chain in the reference). May be
 * called any number of times for one forward (the trainer walks the graph twice:
 * recbole/trainer/trainer.py:677,684). */
int acattn_calibrated_attention_bwd(const acattn_problem* p, const acattn_bwd_io* io, void* stream);

/* Bytes of `acattn_bwd_io.workspace` for this problem (5 row scalars of the chained soft-max backward per query row). */
int64_t acattn_calibrated_attention_bwd_workspace_bytes(const acattn_problem* p);

/* [ABI 32] Backward of the SPATIAL-ONLY operator (acattn_problem.adversarial == 0):
 *     ctx = dropout(softmax((q k^T + e_order + e_distance) / sqrt(dh) + mask)) . V     recbole/model/layers.py:695-740, 677-680
 * The spatial-only forward saves nothing, so the backward rebuilds the probabilities from the forward's acattn_problem
 * (q, k, v, the mask in any of the three modes, either or both spatial terms, p_drop and the same randomness: the counter
 * seed / seed_device, or the explicit keep_after) and forms the row normalisers itself (csrc/acattn_bwd_spatial.hip: a row
 * kernel and a key kernel, no float atomics on dq / dk / dv).  May be called any number of times for one forward. */
typedef struct acattn_spatial_bwd_io {
  const float* d_ctx; /* [B,L,H] cotangent of ctx_calibrated */
  /* gradients, caller-allocated, fully overwritten */
  float* dq; /* [B,L,H] */
  float* dk; /* [B,L,H] */
  float* dv; /* [B,L,H] */
  /* per-(b,head) partial sums of the calibrator parameters in the layout of acattn_bwd_io; the caller reduces over
   * (B, nh).  Fully written: the columns of a disabled term (NULL weight) and the spare fourth small column are zeros. */
  float* dw_order_part; /* [B,nh,2*dh] */
  float* dw_dist_part;  /* [B,nh,2*dh] */
  float* dsmall_part;   /* [B,nh,4]: d b_order, d b_dist, d scalar, 0 */
  int32_t part_stride;  /* as acattn_bwd_io.part_stride */
  int32_t n_read_rows;
  const int64_t* read_rows; /* optional [B, n_read_rows], as acattn_bwd_io.read_rows: the caller promises that d_ctx is zero
                               outside those positions; query blocks without one are skipped (their dq rows are zeros).
                               NULL = every row may carry a cotangent. */
  void* workspace;          /* device scratch of acattn_spatial_attention_bwd_workspace_bytes(p) bytes (contents
                               irrelevant): four floats per (b, head, query row) */
} acattn_spatial_bwd_io;
int acattn_spatial_attention_bwd(const acattn_problem* p, const acattn_spatial_bwd_io* io, void* stream);
int64_t acattn_spatial_attention_bwd_workspace_bytes(const acattn_problem* p);

/* Materialise the COUNTER-mode randomness for (seed, shape) so a run can be replayed in EXPLICIT mode. */
int acattn_rng_materialize(int32_t B, int32_t n_heads, int32_t L, uint64_t seed, float p_drop, float* noise,
                           uint8_t* keep_after, uint8_t* keep_mask, uint8_t* keep_before, void* stream);

/* Diagnostics / measurement: pin the forward kernel acattn_calibrated_attention_fwd dispatches to (process-wide).
 * Every kernel computes the same function; one that does not cover the problem (options, L, rng mode) is skipped
 * and the automatic choice applies.  Returns the previous setting.  The setting is PER HOST THREAD (thread_local): it
 * affects the launches the calling thread issues afterwards and nobody else's. */
enum {
  ACATTN_FWD_AUTO = 0,    /* L <= 208: streaming kernel where it applies (training configuration), else general;
                             L > 208: the long form */
  ACATTN_FWD_STREAM = 1,  /* acattn_fwd_stream.hip: one wave per 16-row query block, no LDS staging (L <= 208) */
  ACATTN_FWD_STAGED = 2,  /* acattn_fwd_dma.hip / acattn_fwd_fast.hip: K, Ka, V, gate logits staged in LDS (L <= 64) */
  ACATTN_FWD_GENERAL = 3, /* acattn_fwd.hip: every option, explicit randomness, probability dumps (L <= 208) */
  ACATTN_FWD_LONG = 4     /* acattn_long_fwd.inc: key tiles in a run-time loop, three sweeps; any L up to
                             acattn_max_sequence_length(), every option but two_level = 0 and the probability dumps.
                             The automatic choice for L > 208; any other pinned kernel fails there. */
};
int acattn_select_forward_kernel(int which);

/* [added within ABI 34] The largest sequence length L the attention core accepts (496: 31 key tiles of 16). */
int acattn_max_sequence_length(void);

/* The same for acattn_calibrated_attention_bwd. */
enum {
  ACATTN_BWD_AUTO = 0,    /* training configuration: row-resident for L <= 64, streaming (io.workspace given) up to 208;
                             L > 208: the long form (io.workspace required).  Only here: the one-row form
                             (acattn_bwd_stream.hip) and, for L <= 64, acattn_bwd_attack.hip: an attack-only launch
                             without d_ctx_attacked, read rows or a block bitmap.  Its cotangents are the attack mask's
                             (dqa, dka from the soft-max of the mask scores alone; also the mask launch in front of the
                             one-row form), d_ctx_calibrated (layer 0 of the attacked-loss walk), or both.
                             ACATTN_BWD_ATTACK=0 in the environment leaves those launches on the row-resident kernel,
                             ACATTN_BWD_ATTACK_CTX=0 the ones with d_ctx_calibrated alone. */
  ACATTN_BWD_STREAM = 1,  /* acattn_bwd_stream.hip: row kernel + key kernel, tiles rebuilt from the saved normalisers */
  ACATTN_BWD_ROW = 2,     /* acattn_bwd_fast.hip / acattn_bwd.hip: a query block's whole row in registers */
  ACATTN_BWD_LONG = 3     /* acattn_long_bwd.inc: row kernel + key kernel with run-time tile loops; any L up to
                             acattn_max_sequence_length(), every option but two_level = 0, the second cotangent set and
                             dgate_summed; needs io.workspace.  The automatic choice for L > 208; any other pinned kernel
                             fails there. */
};
int acattn_select_backward_kernel(int which);

/* [added within ABI 34] acattn_calibrated_attention_bwd's arguments, issued on acattn_bwd_attack.hip or not at all: 0 when
   the attack-side kernel took the launch, -100 when the launch is outside its domain (nothing was launched).  Neither the
   calling thread's acattn_select_backward_kernel setting nor ACATTN_BWD_ATTACK is consulted; for tests and measurements
   that must know which kernel ran. */
int acattn_calibrated_attention_bwd_attack_side(const acattn_problem* p, const acattn_bwd_io* io, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * [added within ABI 34: new entry points only, the structs are unchanged] The UN-NORMALISED attention core of ACSSEPT
 * (acssept.py:17 builds its encoder from recbole/model/transformer_layers.py:873-1006, not from recbole/model/layers.py).  That
 * encoder shares every parameter and state-dict key with the one above, but transformer_layers.py:920-928 has none of the
 * three softmax(. + attention_mask) re-normalisations of layers.py:919, 921, 925: per head, with P = after_spatial
 * (transformer_layers.py:823-867), M the attack mask (:785-802), N ~ randn and g = sigmoid(gate(query)) (:901),
 *     A_att = P M + N (1 - M)                      transformer_layers.py:921-922
 *     A_w   = g P + (1 - g) P exp(1 - M)           transformer_layers.py:924, :901-902
 *     ctx_attacked = A_att . V,  ctx_calibrated = A_w . V      transformer_layers.py:805
 * A kernel pair of its own (csrc/acattn_unnorm.hip); never a fallback to or from acattn_calibrated_attention_*.
 *
 * Supported (acattn_unnorm_attention_supported answers 1 / 0 from the configuration alone, without a launch): adversarial = 1,
 * combine_option GATE, two_level = 1, mask_mode STRUCTURED (causal or not), 1 <= L <= 64, head size 16, 32 or 64, rng_mode
 * EXPLICIT (noise, keep_after, keep_mask; p_drop = 0 = no dropout, keep_before is not read) or COUNTER (seed, seed_device; the
 * draws of acattn_rng_materialize), gate_is_prob 0 or 1; both spatial terms must be present; `affine` is ignored.  Anything
 * else: -1 and a text that names the limit.
 *
 * Consequences of the missing re-normalisation, all as in the reference: where M = 0 (padded keys, future keys under the
 * causal mask) A_att = N, so ctx_attacked sums over ALL L keys -- V of padded and future positions included: a NaN or Inf
 * there reaches ctx_attacked.  A query row without an allowed key (left padding under the causal mask) gets the soft-max
 * over all L keys, the mask's common -10000 dropped; the reference's fp32 rounding of `score - 10000` is NOT reproduced
 * (its float64 value is).  ctx_attacked is O(sqrt(L) |V|).
 *
 * Forward: writes ctx_attacked, ctx_calibrated, attack_mask (all required), row_stats when given and penalty_part when
 * given (acattn_mask_penalty_rows behind the launch).  row_stats [B,nh,L,ACATTN_NSTAT]: slot 0 = the log-normaliser of P's
 * row, slot 1 = that of M's row, both in LOG2 units of the scaled, masked scores (P before dropout = exp2(log2(e) x - slot 0));
 * slots 2..7 are written as zeros.  A non-NULL probability dump (after_spatial ...) is an error.
 * Backward: rebuilds P and M (before dropout) from q, k, qa, ka, the calibrator parameters and row_stats, replays the keep
 * bits and the noise; every combination of d_ctx_attacked, d_ctx_calibrated, d_attack_mask, d_penalty_part (NULL = zero);
 * writes dq, dk, dv, dqa, dka, dgate_logits ([B,nh,L,L] per-head partials) and the three parameter partials (part_stride
 * honoured) in full.  active_qblocks, read_rows and attack_only are ignored (every output is written); workspace is unused;
 * dgate_summed and the second cotangent set (dqa2 ...) are errors.  No float atomics: two launches give the same bits. */
int acattn_unnorm_attention_supported(const acattn_problem* p);
int acattn_unnorm_attention_fwd(const acattn_problem* p, const acattn_fwd_out* out, void* stream);
int acattn_unnorm_attention_bwd(const acattn_problem* p, const acattn_bwd_io* io, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * [added within ABI 34: new entry points and two new structs only, every existing struct is unchanged] The TIME-INTERVAL
 * attention core of ACTiSASRec (actisasrec.py:59 builds its encoder from
 * recbole/model/transformer_layers.py:1010-1422).  The un-normalised core above (same mixtures, :1297-1303, no soft-max over
 * them) with a per-key absolute-position term and a per-PAIR time-interval term in the scores and in the value sum.  Per head,
 * with pk_j, pv_j the head's slices of the (already dropped) position rows, t_ij = time_index[b, i, j] and
 * TK_ij = dropout(time_k[t_ij]), TV_ij = dropout(time_v[t_ij]) (head slices; actisasrec.py:113-114, :123-124):
 *     S_ij = q_i.(k_j + pk_j) + q_i.TK_ij + e_order(q_i, k_j) + e_distance(q_i, k_j)      transformer_layers.py:1125-1166
 *     P = dropout(softmax(S / sqrt(dh) + mask)),  M = dropout(softmax(qa.ka^T / sqrt(dh) + mask))      :1168-1176, :1065-1082
 *     ctx_x[i] = sum_j A_x[i, j] (v_j + pv_j + TV_ij),   x in {attacked, calibrated}                   :1084-1090
 * The reference gathers TK and TV as two [B,L,L,H] tensors per forward; here the kernels (csrc/acattn_timeaware.hip) gather
 * the table rows where they need them and replay the dropout bits, so nothing of that size exists.  A kernel family of its
 * own: never a fallback to or from acattn_unnorm_attention_* or acattn_calibrated_attention_*.
 *
 * Supported (acattn_timeaware_attention_supported: 1 / 0 from the configuration alone, no launch): everything
 * acattn_unnorm_attention_supported requires (adversarial, GATE, two_level, STRUCTURED mask, both spatial terms, 1 <= L <= 64,
 * head size 16 / 32 / 64, EXPLICIT or COUNTER randomness of the layer's own draws), and 1 <= time_span with
 * 8 (time_span + 1) dh <= 160 KiB (the two gradient tables of one head in one workgroup's LDS: time_span <= 319 at head size
 * 64, so the reference's default 256 fits every head size), 0 <= p_time < 1.  Anything else: -1 and a text naming the limit.
 *
 * time_index values are CLAMPED into [0, time_span] by every kernel before a table is addressed (get_time_matrix,
 * actisasrec.py:148-157, already clips: a bad batch gives a wrong number, never an out-of-bounds access).  Nothing is read
 * for a key j >= L of the tile padding: no index, and TK, TV, pk, pv count as zero there.  Every key j < L enters the value
 * sums, padded and future ones included (A_attacked = N where M = 0); a zero weight of the CALIBRATED mixture skips its TV
 * row, so a non-finite table row reached only through masked keys shows in ctx_attacked alone.
 *
 * Time dropout: keep_time_k / keep_time_v given = those bits; both NULL with p_time > 0 = the counter stream of
 * (time_seed + *time_seed_device), the bits acattn_time_rng_materialize writes -- a stream disjoint from
 * acattn_rng_materialize's, and a seed of its own because all layers of one forward share the dropped tensors
 * (actisasrec.py:123-124 runs once per forward).  p_time = 0: no dropout. */
typedef struct acattn_time_ext {
  const float* pos_k;         /* [B,L,H] dropout(absolute_pos_K_embedding(position_ids))   actisasrec.py:110, :121 */
  const float* pos_v;         /* [B,L,H] dropout(absolute_pos_V_embedding(position_ids))   actisasrec.py:111, :122 */
  const int32_t* time_index;  /* [B,L,L] get_time_matrix(time_seq)                          actisasrec.py:148-157 */
  const float* time_k;        /* [time_span + 1, H] time_matrix_emb_K_embedding.weight      actisasrec.py:56 */
  const float* time_v;        /* [time_span + 1, H] time_matrix_emb_V_embedding.weight      actisasrec.py:57 */
  int32_t time_span;
  float p_time;               /* hidden_dropout_prob of actisasrec.py:123-124; 0 = none */
  const uint8_t* keep_time_k; /* [B,L,L,H] 0/1 or NULL */
  const uint8_t* keep_time_v; /* [B,L,L,H] 0/1 or NULL */
  uint64_t time_seed;
  const uint64_t* time_seed_device; /* optional, added to time_seed when a kernel starts */
} acattn_time_ext;

/* What the backward writes beyond acattn_bwd_io (all required, fully overwritten).  d pos_v = dv and is not written again.
 * d_time_k / d_time_v are the TRUE derivatives, row 0 included (nn.Embedding(padding_idx=0) zeroes that row: the caller's
 * business).  They come from a second launch (timeaware_table_grad_kernel) that sums in LDS and flushes with float atomics:
 * these two outputs alone may differ in the last bits between two launches; every other output keeps the un-normalised
 * core's property (no atomic, same bits). */
typedef struct acattn_time_grads {
  float* d_pos_k;  /* [B,L,H]: sum_i dS_ij q_i, the product share of dk (the spatial affines' share goes to dk alone) */
  float* d_time_k; /* [time_span + 1, H] */
  float* d_time_v; /* [time_span + 1, H] */
  void* workspace; /* 3 * B * n_heads * L * L floats (contents irrelevant): dS, A_attacked, A_calibrated for the second launch */
} acattn_time_grads;

int acattn_timeaware_attention_supported(const acattn_problem* p, const acattn_time_ext* t);
/* Replaces transformer_layers.py:1107-1180 (cal_origin_qkv after the projections), :1065-1082, :1296-1303 and the three
 * matmuls of :1087-1090.  Outputs as acattn_unnorm_attention_fwd (row_stats slots 0-1, penalty_part). */
int acattn_timeaware_attention_fwd(const acattn_problem* p, const acattn_time_ext* t, const acattn_fwd_out* out, void* stream);
/* The backward of the above: acattn_unnorm_attention_bwd's contract for `io`, with dq carrying the pk and TK terms and
 * dA_x[i,j] = d_ctx_x[i].(v_j + pv_j + TV_ij), plus `grads`. */
int acattn_timeaware_attention_bwd(const acattn_problem* p, const acattn_time_ext* t, const acattn_bwd_io* io,
                                   const acattn_time_grads* grads, void* stream);
/* The counter-mode keep bits of the two time dropouts for (seed, shape): uint8 [B,L,L,H] each (either may be NULL). */
int acattn_time_rng_materialize(int32_t B, int32_t L, int32_t H, uint64_t seed, float p, uint8_t* keep_k, uint8_t* keep_v,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ACATTN_H_ */
