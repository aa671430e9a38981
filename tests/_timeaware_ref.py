"""CPU restatement of ACTiSASRec and of its TIME-INTERVAL attention core, for tests and tools only.

ACTiSASRec (recbole/model/sequential_recommender/actisasrec.py) builds its encoder from
recbole/model/transformer_layers.py:1010-1422: the un-normalised layer of tests/_unnorm_ref.py (same parameters, same draw
order, the mixtures of :1297-1303 without a soft-max over them) whose scores and value sums carry two more terms, a per-key
absolute-position row and a per-pair time-interval row:
    S_ij     = q_i.(k_j + pk_j) + q_i.TK_ij + e_order(q_i, k_j) + e_distance(q_i, k_j)          :1125-1166
    ctx_x[i] = sum_j A_x[i,j] (v_j + pv_j + TV_ij)                                              :1084-1090
with TK_ij = dropout(time_K[t_ij]), TV_ij = dropout(time_V[t_ij]) and pk, pv the dropped position rows (actisasrec.py:110-124).
Composed from oracle/ac_tsr_ref.py's functions (imported, never changed) and tests/_unnorm_ref.mixtures; works in float32 and
float64 (tests/_attention_fp64.default_dtype sets the dtype of the oracle's constants).  tools/gen_tisasrec_golden.py pins it
to the genuine reference.
"""
import math
from dataclasses import dataclass
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from oracle import ac_tsr_ref as O
from tests._unnorm_ref import mixtures

Tensor = torch.Tensor


@dataclass
class TimeInputs:
    """What actisasrec.py:110-124 hands the encoder, before the [B,L,L,H] gathers: pos_k / pos_v [B,L,H] already dropped,
    the index matrix [B,L,L], the two [time_span + 1, H] tables and the keep masks of the two time dropouts ([B,L,L,H], 0/1
    floats, None = no dropout) at rate p."""
    pos_k: Tensor
    pos_v: Tensor
    index: Tensor
    time_k: Tensor
    time_v: Tensor
    keep_k: Optional[Tensor] = None
    keep_v: Optional[Tensor] = None
    p: float = 0.0

    def gathered(self, n_heads: int):
        """(TK, TV) as transformer_layers.py:1119-1122 arranges them: [B,h,L,L,dh]."""
        idx = self.index.long()
        tk = O._drop(F.embedding(idx, self.time_k), self.keep_k, self.p)
        tv = O._drop(F.embedding(idx, self.time_v), self.keep_v, self.p)
        B, L = idx.shape[:2]
        split = lambda t: t.view(B, L, L, n_heads, -1).permute(0, 3, 1, 2, 4)
        return split(tk), split(tv)


def get_time_matrix(time_seq: Tensor, time_span: int) -> Tensor:
    """ACTiSASRec.get_time_matrix (actisasrec.py:148-157): |t_i - t_j| clipped at time_span, int32 [B,L,L]."""
    L = time_seq.shape[1]
    ti = time_seq.unsqueeze(-1).expand([-1, L, L])
    tj = time_seq.unsqueeze(1).expand([-1, L, L])
    m = torch.abs(ti - tj)
    return torch.where(m > time_span, torch.ones_like(m) * time_span, m).int()


def time_context(prob: Tensor, v: Tensor, pos_v: Tensor, tv: Tensor) -> Tensor:
    """The three matmuls and the head merge of cal_adjusted_outputs (:1087-1094) -> [B,L,H]."""
    ctx = torch.matmul(prob, v) + torch.matmul(prob, pos_v) + torch.matmul(prob.unsqueeze(-2), tv).squeeze(-2)
    ctx = ctx.permute(0, 2, 1, 3).contiguous()
    return ctx.view(ctx.shape[0], ctx.shape[1], -1)


def time_scores(q: Tensor, k: Tensor, pos_k: Tensor, tk: Tensor) -> Tensor:
    """attention_scores + attention_scores_pos + attention_scores_time (:1125-1130); q, k, pos_k [B,h,L,dh]."""
    return (torch.matmul(q, k.transpose(-1, -2)) + torch.matmul(q, pos_k.transpose(-1, -2))
            + torch.matmul(tk, q.unsqueeze(-1)).squeeze(-1))


def core_from_projected_time(mq: Tensor, mk: Tensor, mv: Tensor, qa: Tensor, ka: Tensor, gate_logits: Tensor, mask: Tensor,
                             w_order, b_order, w_dist, b_dist, scalar, cfg: O.EncoderCfg, noise: Tensor, ti: TimeInputs,
                             keep_after=None, keep_mask=None, materialize: bool = False):
    """Everything between the projections and the output dense of ACTimeAwareTransformerLayer ('gate', two-level).
    Returns dict(ctx_attacked, ctx_calibrated [B,L,H]; M, after, attacked, combined [B,h,L,L]; lse_p, lse_m [B,h,L]: the
    log-normalisers of P's and M's rows, natural-log units of the scaled masked scores)."""
    h = cfg.n_heads
    heads = lambda t: O._heads(t, h).permute(0, 2, 1, 3)
    q, k, v = heads(mq), heads(mk), heads(mv)
    dh = q.shape[-1]
    p = {"attack_attention.order_affine.weight": w_order, "attack_attention.order_affine.bias": b_order,
         "attack_attention.distance_affine.weight": w_dist, "attack_attention.distance_affine.bias": b_dist,
         "attack_attention.scalar": scalar}
    tk, tv = ti.gathered(h)
    e_o, e_d = O.spatial_errors(q, k, p, cfg, materialize=materialize)  # the plain k (:1142-1145)
    pa = cfg.attn_dropout_prob
    s_p = (time_scores(q, k, heads(ti.pos_k), tk) + e_o + e_d) / math.sqrt(dh) + mask
    s_m = torch.matmul(heads(qa), heads(ka).transpose(-1, -2)) / math.sqrt(dh) + mask
    after = O._drop(torch.softmax(s_p, dim=-1), keep_after, pa)
    M = O._drop(torch.softmax(s_m, dim=-1), keep_mask, pa)
    attacked, combined = mixtures(after, M, noise, torch.sigmoid(gate_logits))
    pv = heads(ti.pos_v)
    return dict(ctx_attacked=time_context(attacked, v, pv, tv), ctx_calibrated=time_context(combined, v, pv, tv), M=M,
                after=after, attacked=attacked, combined=combined, lse_p=torch.logsumexp(s_p, dim=-1),
                lse_m=torch.logsumexp(s_m, dim=-1))


def _outputs(ctx: Tensor, x: Tensor, p: Dict[str, Tensor], cfg: O.EncoderCfg, keep) -> Tensor:
    """dense, dropout, LayerNorm(+ residual) of cal_adjusted_outputs (:1095-1097)."""
    hid = O._drop(O._lin(ctx, p, "attack_attention.dense"), keep, cfg.hidden_dropout_prob)
    return F.layer_norm(hid + x, (x.shape[-1],), p["attack_attention.LayerNorm.weight"], p["attack_attention.LayerNorm.bias"],
                        cfg.layer_norm_eps)


def layer_forward_time(x: Tensor, mask: Tensor, p: Dict[str, Tensor], cfg: O.EncoderCfg, rnd: O.LayerRandomness,
                       ti: TimeInputs, materialize: bool = True):
    """ACTimeAwareTransformerLayer.forward ('gate', two-level, :1285-1327) -> (attacked_out, calibrated_out, M, dbg)."""
    assert cfg.combine_option == "gate" and cfg.two_level
    mq = O._lin(x, p, "attack_attention.query")
    mk = O._lin(x, p, "attack_attention.key")
    mv = O._lin(x, p, "attack_attention.value")
    r = core_from_projected_time(
        mq, mk, mv, O._lin(mq, p, "attack_attention.attack_query_transform"),
        O._lin(mk, p, "attack_attention.attack_key_transform"), O._lin(mq, p, "gate"), mask,
        p["attack_attention.order_affine.weight"], p["attack_attention.order_affine.bias"],
        p["attack_attention.distance_affine.weight"], p["attack_attention.distance_affine.bias"], p["attack_attention.scalar"],
        cfg, rnd.noise, ti, keep_after=rnd.keep_after, keep_mask=rnd.keep_mask, materialize=materialize)
    att = O.feed_forward(_outputs(r["ctx_attacked"], x, p, cfg, rnd.keep_out_att), p, cfg, rnd.keep_ffn_att)
    cal = O.feed_forward(_outputs(r["ctx_calibrated"], x, p, cfg, rnd.keep_out_cal), p, cfg, rnd.keep_ffn_cal)
    dbg = dict(mixed_query=mq, mixed_key=mk, mixed_value=mv, ctx_attacked=r["ctx_attacked"], ctx_calibrated=r["ctx_calibrated"])
    return att, cal, r["M"], dbg


@dataclass
class ModelRandomness:
    """The draws of one ACTiSASRec.forward in the reference's order (actisasrec.py:119-124, then the layers'): 0/1 keep masks,
    None = eval mode."""
    keep_emb: Optional[Tensor] = None     # [B,L,H]
    keep_pos_k: Optional[Tensor] = None   # [B,L,H]
    keep_pos_v: Optional[Tensor] = None   # [B,L,H]
    keep_time_k: Optional[Tensor] = None  # [B,L,L,H]
    keep_time_v: Optional[Tensor] = None  # [B,L,L,H]


def time_inputs(item_seq: Tensor, time_matrix: Tensor, P: Dict[str, Tensor], cfg: O.ModelCfg, mr: ModelRandomness) -> TimeInputs:
    B, L = item_seq.shape
    ph = cfg.enc.hidden_dropout_prob
    pos = torch.arange(L, dtype=torch.long).unsqueeze(0).expand(B, L)
    return TimeInputs(pos_k=O._drop(F.embedding(pos, P["absolute_pos_K_embedding.weight"]), mr.keep_pos_k, ph),
                      pos_v=O._drop(F.embedding(pos, P["absolute_pos_V_embedding.weight"]), mr.keep_pos_v, ph),
                      index=time_matrix, time_k=P["time_matrix_emb_K_embedding.weight"],
                      time_v=P["time_matrix_emb_V_embedding.weight"], keep_k=mr.keep_time_k, keep_v=mr.keep_time_v, p=ph)


def model_forward(item_seq: Tensor, item_seq_len: Tensor, time_matrix: Tensor, P: Dict[str, Tensor], cfg: O.ModelCfg, rnds,
                  mr: Optional[ModelRandomness] = None, materialize: bool = True):
    """ACTiSASRec.forward (actisasrec.py:106-141) -> (attacked [B,H], calibrated [B,H], list[M], list[dbg])."""
    mr = mr or ModelRandomness()
    ti = time_inputs(item_seq, time_matrix, P, cfg, mr)
    emb = F.embedding(item_seq, P["item_embedding.weight"], padding_idx=0)  # (the catalogue product still reaches row 0)
    emb = F.layer_norm(emb, (emb.shape[-1],), P["LayerNorm.weight"], P["LayerNorm.bias"], cfg.enc.layer_norm_eps)
    emb = O._drop(emb, mr.keep_emb, cfg.enc.hidden_dropout_prob)
    mask = O.attention_mask(item_seq)
    hidden, masks, dbgs = emb, [], []
    att = cal = None
    for i in range(cfg.enc.n_layers):
        att, cal, M, dbg = layer_forward_time(hidden, mask, O.layer_params(P, f"ti_trm_encoder.layer.{i}."), cfg.enc, rnds[i],
                                              ti, materialize)
        hidden = cal
        masks.append(M)
        dbgs.append(dbg)
    return O.gather_indexes(att, item_seq_len - 1), O.gather_indexes(cal, item_seq_len - 1), masks, dbgs


def _time_matrix(batch, time_span: int, time_field: str = "timestamp_list"):
    return get_time_matrix(batch[time_field], time_span)


def calculate_loss(batch: Dict[str, Tensor], P: Dict[str, Tensor], cfg: O.ModelCfg, time_span: int, rnds, mr=None,
                   materialize: bool = True):
    """ACTiSASRec.calculate_loss (actisasrec.py:175-195), loss 'CE' -> (final_attacked_loss, calibrated_loss)."""
    att, cal, masks, _ = model_forward(batch["item_id_list"], batch["item_length"], _time_matrix(batch, time_span), P, cfg, rnds,
                                       mr, materialize)
    E, pos = P["item_embedding.weight"], batch["item_id"]
    attacked_loss = -F.cross_entropy(att @ E.t(), pos)
    penalty = torch.stack([torch.norm(1 - M, p=2) for M in masks]).mean()
    w = P["mask_loss_weight"][0] if cfg.trainable_mask_loss_weight else cfg.mask_loss_weight
    return attacked_loss + penalty * w, F.cross_entropy(cal @ E.t(), pos)


def full_sort_predict(batch: Dict[str, Tensor], P: Dict[str, Tensor], cfg: O.ModelCfg, time_span: int, rnds):
    """ACTiSASRec.full_sort_predict (actisasrec.py:212-224) -> (attacked_scores, scores), [B, n_items] each."""
    att, cal, _, _ = model_forward(batch["item_id_list"], batch["item_length"], _time_matrix(batch, time_span), P, cfg, rnds)
    E = P["item_embedding.weight"]
    return att @ E.t(), cal @ E.t()


# the four tables that are read through nn.Embedding(padding_idx=0) lookups ONLY: their row 0 is never trained
PADDED_TABLES = ("absolute_pos_K_embedding.weight", "absolute_pos_V_embedding.weight", "time_matrix_emb_K_embedding.weight",
                 "time_matrix_emb_V_embedding.weight")


def two_pass_grads(batch, P: Dict[str, Tensor], cfg: O.ModelCfg, time_span: int, rnds, mr=None, materialize: bool = True,
                   zero_padding_rows: bool = True):
    """oracle.ac_tsr_ref.two_pass_grads for ACTiSASRec (recbole/trainer/trainer.py:672-686).  nn.Embedding(padding_idx=0)
    gives row 0 of the four position / time tables no gradient; `zero_padding_rows=False` returns the un-masked derivative."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in P.items() if v.is_floating_point()}
    att_loss, cal_loss = calculate_loss(batch, leaves, cfg, time_span, rnds, mr, materialize)
    names = list(leaves)
    g_cal = torch.autograd.grad(cal_loss, [leaves[n] for n in names], retain_graph=True, allow_unused=True)
    g_att = torch.autograd.grad(att_loss, [leaves[n] for n in names], allow_unused=True)
    grads = {}
    for n, gc, ga in zip(names, g_cal, g_att):
        g = ga if O.is_attack_param(n) else gc
        g = torch.zeros_like(P[n]) if g is None else g.clone()
        if zero_padding_rows and n in PADDED_TABLES:
            g[0] = 0
        grads[n] = g
    return att_loss.detach(), cal_loss.detach(), grads
