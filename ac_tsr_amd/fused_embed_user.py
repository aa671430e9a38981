"""dropout(LayerNorm(cat(item_embedding[item_seq], user_embedding[user_id] over L) + position_embedding)) as one HIP
launch forward and one (plus a small row sum for the user table) backward (include/acattn.h:
acattn_embed_user_layernorm_*): the front end of ACSSEPT.forward (recbole/model/sequential_recommender/acssept.py:120-131).
model.ACSSEPT calls it; the encoder behind it is the un-normalised attention core.

The backward adds both table gradients with float atomics into zero-initialised buffers, skipping the `padding_idx` rows
like nn.Embedding; the item half joins the hand-over of fused_embed (the loss node's published [n_items, Di] gradient is
scattered into, StepState.table_grad); the user half is summed over each sequence's positions first (USER_SUM_FIRST).
Position and LayerNorm gradients come back as per-workgroup partials that are summed here.  Seeds and the explicit `keep`
mask as in fused_embed.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib, attn_launch, ops
from .state import state_of
from .ops import _need_cuda, _ptr, _stream

# The user-table gradient: True = a [rows, Du] scratch and a row sum over each sequence's positions, one atomic per (sequence,
# column); False = one atomic per (row, column) like the item half (include/acattn.h: user_rows_ws).  Same gradients; the
# times are in profiles/ssept_front_end.txt.
USER_SUM_FIRST = True


def _problem(idx, user, table, user_table, pos, gamma, beta, eps, p_drop, keep, seed, seed_tensor) -> _lib.EmbedUserProblem:
    p = _lib.EmbedUserProblem()
    p.rows, p.L, p.Di = idx.numel(), idx.shape[-1], table.shape[1]
    p.H = table.shape[1] + user_table.shape[1]
    p.n_table_rows, p.n_user_rows = table.shape[0], user_table.shape[0]
    p.idx, p.user, p.table, p.user_table = _ptr(idx), _ptr(user), _ptr(table), _ptr(user_table)
    p.pos, p.gamma, p.beta = _ptr(pos), _ptr(gamma), _ptr(beta)
    p.eps, p.p_drop = float(eps), float(p_drop)
    p.keep = _ptr(keep)
    p.seed = seed & 0xFFFFFFFFFFFFFFFF
    p.seed_device = _ptr(seed_tensor)
    return p


class _EmbedUserLayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, idx, user, table, user_table, pos, gamma, beta, eps, p_drop, keep, seed, seed_tensor, item_padding_idx,
                user_padding_idx, state):
        ctx.state = state
        _need_cuda("item_seq", idx, torch.int64)
        _need_cuda("user_id", user, torch.int64)
        for name, t in (("item_embedding.weight", table), ("user_embedding.weight", user_table), ("LayerNorm.weight", gamma),
                        ("LayerNorm.bias", beta)):
            _need_cuda(name, t)
        H = table.shape[1] + user_table.shape[1]
        if idx.dim() != 2 or user.shape != idx.shape[:1]:
            raise ValueError(f"item_seq must be [B, L] and user_id [B], got {tuple(idx.shape)} and {tuple(user.shape)}")
        if gamma.numel() != H or beta.numel() != H:
            raise ValueError(f"LayerNorm is {gamma.numel()} wide, the item and user tables together {H}")
        if pos is not None:
            _need_cuda("position_embedding.weight", pos)
            if pos.shape[1] != H:
                raise ValueError(f"position_embedding is {pos.shape[1]} wide, the item and user tables together {H}")
            if idx.shape[-1] > pos.shape[0]:
                raise IndexError("index out of range in self")  # nn.Embedding's error for position ids >= rows
        if keep is not None:
            keep = keep.to(torch.uint8).contiguous()
            assert keep.shape == (*idx.shape, H)
        lib = _lib.load()
        p = _problem(idx, user, table, user_table, pos, gamma, beta, eps, p_drop, keep, seed, seed_tensor)
        new = attn_launch.allocator(table, attn_launch.POISON)
        y = new(*idx.shape, H)
        stats = new(p.rows, 2)
        nonzero = torch.empty(idx.shape, device=table.device, dtype=torch.uint8)  # idx != 0: the mask's validity bytes
        p.nonzero_out = _ptr(nonzero)
        _lib.check(lib.acattn_embed_user_layernorm_fwd(C.byref(p), _ptr(y), _ptr(stats), _stream()), "embed_user_layernorm_fwd")
        empty = torch.empty(0)
        ctx.save_for_backward(idx, user, table, user_table, pos if pos is not None else empty, gamma, beta, stats,
                              keep if keep is not None else empty, seed_tensor if seed_tensor is not None else empty)
        ctx.args = (eps, p_drop, pos is not None, keep is not None, seed, seed_tensor is not None, item_padding_idx,
                    user_padding_idx)
        ctx.tick = state.next_tick()
        ctx.mark_non_differentiable(nonzero)
        ctx.set_materialize_grads(False)  # no zero-filled "gradient" of the validity bytes (one launch per backward)
        return y, nonzero

    @staticmethod
    def backward(ctx, dy, _d_nonzero=None):
        idx, user, table, user_table, pos, gamma, beta, stats, keep, seed_tensor = ctx.saved_tensors
        eps, p_drop, has_pos, has_keep, seed, has_seed_t, item_padding_idx, user_padding_idx = ctx.args
        if ctx.state.attack_pass_only or dy is None:  # none of these parameters is an attack transform (trainer.py:678-684)
            return (None,) * 15
        lib = _lib.load()
        p = _problem(idx, user, table, user_table, pos if has_pos else None, gamma, beta, eps, p_drop,
                     keep if has_keep else None, seed, seed_tensor if has_seed_t else None)
        L, H, chunks = p.L, p.H, _lib.EMBED_BWD_CHUNKS
        # the loss node's dense item-table gradient, if one was published in this walk: the rows are scattered into it and the
        # table gets no second gradient from here (fused_embed._EmbedLayerNorm.backward); else a zero-filled buffer of our own
        handed = ctx.state.take_table_grad(ctx.tick, table) if ctx.needs_input_grad[2] else None
        d_item = handed if handed is not None else (torch.zeros_like(table) if ctx.needs_input_grad[2] else None)
        d_user = torch.zeros_like(user_table) if ctx.needs_input_grad[3] else None
        new = attn_launch.allocator(table, attn_launch.POISON)
        want_pos = has_pos and ctx.needs_input_grad[4]
        pos_part = new(chunks, L, H) if want_pos else None
        want_gb = ctx.needs_input_grad[5] or ctx.needs_input_grad[6]
        gb_part = new(chunks * L, 2, H) if want_gb else None
        # the user half of every row's gradient, summed over each sequence's positions before it touches d_user
        user_rows = new(p.rows, H - p.Di) if (d_user is not None and USER_SUM_FIRST) else None
        _lib.check(lib.acattn_embed_user_layernorm_bwd(C.byref(p), _ptr(dy.contiguous()), _ptr(stats),
                                                       -1 if item_padding_idx is None else int(item_padding_idx),
                                                       -1 if user_padding_idx is None else int(user_padding_idx),
                                                       _ptr(d_item), _ptr(d_user), _ptr(user_rows), _ptr(pos_part),
                                                       _ptr(gb_part), _stream()),
                   "embed_user_layernorm_bwd")
        d_pos = None
        if want_pos:
            d_pos = torch.zeros_like(pos)
            d_pos[:L] = ops.sum_rows(pos_part, 0)
        dgamma = dbeta = None
        if want_gb:
            st = getattr(ctx, "state", None)
            gb = ops.sum_rows0(gb_part, st)
            dgamma, dbeta = gb[0], gb[1]
            if st is not None:
                st.watch(gb, dgamma if ctx.needs_input_grad[5] else None, dbeta if ctx.needs_input_grad[6] else None)
        return (None, None, (None if handed is not None else d_item), d_user, d_pos, dgamma, dbeta) + (None,) * 8


def embed_user_layer_norm(item_seq: torch.Tensor, user_id: torch.Tensor, item_embedding: torch.nn.Embedding,
                          user_embedding: torch.nn.Embedding, position_embedding: Optional[torch.nn.Embedding],
                          norm: torch.nn.LayerNorm, p_drop: float, training: bool, keep: Optional[torch.Tensor] = None,
                          return_nonzero: bool = False):
    """dropout(norm(cat(item_embedding(item_seq), user_embedding(user_id) expanded over L) + position_embedding(arange(L))),
    p_drop, training) -> [B, L, H] with H = item width + user width (acssept.py:120-131); with `return_nonzero` also
    `item_seq != 0` as bytes [B, L], written by the same launch."""
    if not supported(norm.normalized_shape[-1], item_embedding.weight.shape[1]):
        raise _lib.AcattnError(f"the personalised front end does not take hidden size {norm.normalized_shape[-1]} split at "
                               f"column {item_embedding.weight.shape[1]} (acattn_embed_user_supported)")
    p = p_drop if (training or keep is not None) else 0.0
    state = state_of(norm)
    seed = state.draw_seed() if (p > 0 and keep is None) else 0
    y, nonzero = _EmbedUserLayerNorm.apply(item_seq.contiguous(), user_id.contiguous(), item_embedding.weight,
                                           user_embedding.weight,
                                           None if position_embedding is None else position_embedding.weight, norm.weight,
                                           norm.bias, norm.eps, p, keep, seed, state.seed_tensor if keep is None else None,
                                           item_embedding.padding_idx, user_embedding.padding_idx, state)
    return (y, nonzero) if return_nonzero else y


def supported(hidden_size: int, item_hidden_size: int) -> bool:
    return bool(_lib.load().acattn_embed_user_supported(int(hidden_size), int(item_hidden_size)))
