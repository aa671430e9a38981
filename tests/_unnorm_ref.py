"""CPU restatement of ACSSEPT and of its UN-NORMALISED attention core, for tests and tools only.

ACSSEPT (recbole/model/sequential_recommender/acssept.py) builds its encoder from recbole/model/transformer_layers.py:873-1006.
That layer has the parameters and the draw order of recbole/model/layers.py's (oracle.ac_tsr_ref.LayerRandomness) and differs in
one thing: transformer_layers.py:920-928 feeds the attacked mixture P M + N (1 - M) and the gated mixture
g P + (1 - g) P exp(1 - M) into the value product as they are, without the three softmax(. + attention_mask) of
layers.py:919, 921, 925.  Everything here is composed from oracle/ac_tsr_ref.py's functions (imported, never changed) and
works in float32 and float64 (tests/_attention_fp64.default_dtype sets the dtype of the oracle's constants).
tools/gen_ssept_golden.py pins it to the genuine reference.
"""
import math
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from oracle import ac_tsr_ref as O

Tensor = torch.Tensor


def mixtures(P: Tensor, M: Tensor, noise: Tensor, gate: Tensor):
    """(attacked, combined) attention of transformer_layers.py:921-924, :901-902 from P (after_spatial, after dropout), the
    attack mask M (after dropout), the noise and g = sigmoid(gate(query)) [B,L,L].  No soft-max."""
    g = gate.unsqueeze(1)
    return P * M + noise * (1 - M), g * P + (1 - g) * (P * torch.exp(1 - M))


def core_from_projected_unnorm(mq: Tensor, mk: Tensor, mv: Tensor, qa: Tensor, ka: Tensor, gate_logits: Tensor, mask: Tensor,
                               w_order, b_order, w_dist, b_dist, scalar, cfg: O.EncoderCfg, noise: Tensor, keep_after=None,
                               keep_mask=None, materialize: bool = False):
    """oracle.ac_tsr_ref.core_from_projected for the un-normalised layer ('gate', two-level): everything between the
    projections and the output dense.  mq/mk/mv/qa/ka [B,L,H], gate_logits [B,L,L] before the sigmoid, mask additive.
    Returns dict(ctx_attacked, ctx_calibrated [B,L,H]; M, after, attacked, combined [B,h,L,L])."""
    h = cfg.n_heads
    q = O._heads(mq, h).permute(0, 2, 1, 3)
    k = O._heads(mk, h).permute(0, 2, 1, 3)
    v = O._heads(mv, h).permute(0, 2, 1, 3)
    dh = q.shape[-1]
    p = {"attack_attention.order_affine.weight": w_order, "attack_attention.order_affine.bias": b_order,
         "attack_attention.distance_affine.weight": w_dist, "attack_attention.distance_affine.bias": b_dist,
         "attack_attention.scalar": scalar}
    raw = torch.matmul(q, k.transpose(-1, -2))
    e_o, e_d = O.spatial_errors(q, k, p, cfg, materialize=materialize)
    pa = cfg.attn_dropout_prob
    after = O._drop(torch.softmax((raw + e_o + e_d) / math.sqrt(dh) + mask, dim=-1), keep_after, pa)
    qah = O._heads(qa, h).permute(0, 2, 1, 3)
    kah = O._heads(ka, h).permute(0, 2, 3, 1)
    M = O._drop(torch.softmax(torch.matmul(qah, kah) / math.sqrt(dh) + mask, dim=-1), keep_mask, pa)
    attacked, combined = mixtures(after, M, noise, torch.sigmoid(gate_logits))
    return dict(ctx_attacked=O.context_only(attacked, v), ctx_calibrated=O.context_only(combined, v), M=M, after=after,
                attacked=attacked, combined=combined)


def layer_forward_unnorm(x: Tensor, mask: Tensor, p: Dict[str, Tensor], cfg: O.EncoderCfg, rnd: O.LayerRandomness,
                         materialize: bool = True):
    """transformer_layers.AttackRTransformerLayer.forward ('gate', two-level) -> (attacked_out, calibrated_out, M, dbg)."""
    assert cfg.combine_option == "gate" and cfg.two_level
    mq, mk, v, after, _ = O.origin_qkv(x, mask, p, cfg, rnd.keep_after, rnd.keep_before, materialize)
    M = O.attack_mask(mq, mk, mask, p, cfg, rnd.keep_mask)
    attacked, combined = mixtures(after, M, rnd.noise, torch.sigmoid(O._lin(mq, p, "gate")))
    att = O.feed_forward(O.adjusted_outputs(attacked, x, v, p, cfg, rnd.keep_out_att), p, cfg, rnd.keep_ffn_att)
    cal = O.feed_forward(O.adjusted_outputs(combined, x, v, p, cfg, rnd.keep_out_cal), p, cfg, rnd.keep_ffn_cal)
    dbg = dict(mixed_query=mq, mixed_key=mk, value=v, after_spatial=after, ctx_attacked=O.context_only(attacked, v),
               ctx_calibrated=O.context_only(combined, v))
    return att, cal, M, dbg


def model_forward(item_seq: Tensor, item_seq_len: Tensor, user_id: Tensor, P: Dict[str, Tensor], cfg: O.ModelCfg, rnds,
                  keep_emb: Optional[Tensor] = None, materialize: bool = True):
    """ACSSEPT.forward (acssept.py:120-140) -> (attacked [B,H], calibrated [B,H], list[M], list[dbg])."""
    item = F.embedding(item_seq, P["item_embedding.weight"])
    user = F.embedding(user_id, P["user_embedding.weight"]).unsqueeze(1).expand(-1, item.shape[1], -1)
    emb = torch.cat([item, user], dim=-1)
    if cfg.use_position_embedding:
        pos = torch.arange(item_seq.size(1), dtype=torch.long)
        emb = emb + F.embedding(pos, P["position_embedding.weight"]).unsqueeze(0)
    emb = F.layer_norm(emb, (emb.shape[-1],), P["LayerNorm.weight"], P["LayerNorm.bias"], cfg.enc.layer_norm_eps)
    emb = O._drop(emb, keep_emb, cfg.enc.hidden_dropout_prob)
    mask = O.attention_mask(item_seq)
    hidden, masks, dbgs = emb, [], []
    att = cal = None
    for i in range(cfg.enc.n_layers):
        att, cal, M, dbg = layer_forward_unnorm(hidden, mask, O.layer_params(P, f"trm_encoder.layer.{i}."), cfg.enc, rnds[i],
                                                materialize)
        hidden = cal
        masks.append(M)
        dbgs.append(dbg)
    return O.gather_indexes(att, item_seq_len - 1), O.gather_indexes(cal, item_seq_len - 1), masks, dbgs


def logits(out: Tensor, user_id: Tensor, P: Dict[str, Tensor], user_table: str) -> Tensor:
    """out . cat(item_embedding, user row)^T over the catalogue (acssept.py:163-169 with `user_embedding`, :213-225 with
    `user_test_embedding`) -> [B, n_items]."""
    E = P["item_embedding.weight"]
    Di = E.shape[1]
    return out[:, :Di] @ E.t() + (out[:, Di:] * F.embedding(user_id, P[user_table])).sum(-1, keepdim=True)


def calculate_loss(batch: Dict[str, Tensor], P: Dict[str, Tensor], cfg: O.ModelCfg, rnds, keep_emb=None,
                   materialize: bool = True):
    """ACSSEPT.calculate_loss (acssept.py:175-191), loss 'CE' -> (final_attacked_loss, calibrated_loss)."""
    att, cal, masks, _ = model_forward(batch["item_id_list"], batch["item_length"], batch["user_id"], P, cfg, rnds, keep_emb,
                                       materialize)
    pos = batch["item_id"]
    attacked_loss = -F.cross_entropy(logits(att, batch["user_id"], P, "user_embedding.weight"), pos)
    penalty = torch.stack([torch.norm(1 - M, p=2) for M in masks]).mean()
    w = P["mask_loss_weight"][0] if cfg.trainable_mask_loss_weight else cfg.mask_loss_weight
    return attacked_loss + penalty * w, F.cross_entropy(logits(cal, batch["user_id"], P, "user_embedding.weight"), pos)


def full_sort_predict(batch: Dict[str, Tensor], P: Dict[str, Tensor], cfg: O.ModelCfg, rnds):
    """ACSSEPT.full_sort_predict (acssept.py:209-228) -> (attacked_scores, scores), [B, n_items] each."""
    att, cal, _, _ = model_forward(batch["item_id_list"], batch["item_length"], batch["user_id"], P, cfg, rnds)
    return (logits(att, batch["user_id"], P, "user_test_embedding.weight"),
            logits(cal, batch["user_id"], P, "user_test_embedding.weight"))


def two_pass_grads(batch, P: Dict[str, Tensor], cfg: O.ModelCfg, rnds, keep_emb=None, materialize: bool = True):
    """oracle.ac_tsr_ref.two_pass_grads for ACSSEPT (recbole/trainer/trainer.py:672-686)."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in P.items() if v.is_floating_point()}
    att_loss, cal_loss = calculate_loss(batch, leaves, cfg, rnds, keep_emb, materialize)
    names = list(leaves)
    g_cal = torch.autograd.grad(cal_loss, [leaves[n] for n in names], retain_graph=True, allow_unused=True)
    g_att = torch.autograd.grad(att_loss, [leaves[n] for n in names], allow_unused=True)
    grads = {}
    for n, gc, ga in zip(names, g_cal, g_att):
        g = ga if O.is_attack_param(n) else gc
        grads[n] = torch.zeros_like(P[n]) if g is None else g
    return att_loss.detach(), cal_loss.detach(), grads
