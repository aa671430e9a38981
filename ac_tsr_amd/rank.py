"""Full-sort evaluation without the [B, N] scores (include/acattn.h: acattn_full_sort_rank*).

For leave-one-out evaluation every row has one positive, and the reference's default metrics (Recall, MRR, NDCG, Hit,
Precision) are functions of one integer per row: the rank of the target among the admissible items,

    rank[b] = 1 + #{ j in [first_item, N), j != target[b], (b, j) not in history : s_bj ahead of s_b,target }.

`full_sort_ranks` counts it in one sweep of the item table on the matrix cores instead of writing the scores
(recbole/trainer/trainer.py:926-945) and selecting the top K of every row (recbole/evaluator/collector.py:141-153).
`dense_ranks` counts the same thing from materialised scores, for the hidden sizes and devices the kernels do not take.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _lib, attn_launch
from .ops import _need_cuda, _ptr, _stream


class Ranks(NamedTuple):
    """rank: int32 [B], 1 = best, 0 = invalid row (target outside the admissible items, or a NaN target score);
    target_score: float32 [B]."""
    rank: torch.Tensor
    target_score: torch.Tensor


def supported(hidden_size: int) -> bool:
    return hidden_size in (64, 128, 256)


def unique_pairs(history_index, n_items: int):
    """The reference's history_index, a (rows, items) tuple, as two int64 vectors without repeated pairs."""
    rows, items = history_index
    rows, items = torch.as_tensor(rows).reshape(-1).long(), torch.as_tensor(items).reshape(-1).long()
    if rows.shape != items.shape:
        raise ValueError(f"history_index: {rows.numel()} rows for {items.numel()} items")
    inside = (items >= 0) & (items < n_items) & (rows >= 0)  # (pairs outside the table are inadmissible already)
    key = torch.unique(rows[inside] * n_items + items[inside])
    return (key // n_items).contiguous(), (key % n_items).contiguous()


@torch.no_grad()
def full_sort_ranks(output: torch.Tensor, table: torch.Tensor, target: torch.Tensor, n_items: Optional[int] = None,
                    first_item: int = 1, history_index=None) -> Ranks:
    """Ranks of `target` [B] (int64) under the scores output [B, H] @ table[:n_items].T, items below `first_item` (the
    padding item) and the pairs of `history_index` left out.  HIP kernels only: CUDA tensors, H in {64, 128, 256}."""
    output, table = output.detach(), table.detach()
    for name, t in (("output", output), ("item table", table)):
        _need_cuda(name, t)
    _need_cuda("target", target, torch.int64)
    if output.dim() != 2 or table.dim() != 2 or output.shape[1] != table.shape[1] or target.shape != (output.shape[0],):
        raise ValueError(f"full_sort_ranks: output {tuple(output.shape)}, table {tuple(table.shape)}, target {tuple(target.shape)}")
    n = table.shape[0] if n_items is None else int(n_items)
    if not 1 <= n <= table.shape[0]:
        raise ValueError(f"full_sort_ranks: n_items = {n} outside [1, {table.shape[0]}]")
    lib = _lib.load()
    p = _lib.CeProblem()
    p.B, p.N, p.H = output.shape[0], n, output.shape[1]
    p.out, p.table, p.target = _ptr(output), _ptr(table), _ptr(target)
    nbytes = lib.acattn_full_sort_rank_workspace_bytes(C.byref(p))
    if nbytes < 0:
        raise _lib.AcattnError(f"full-sort rank supports hidden sizes 64, 128 and 256 and at least one row and item, got "
                               f"H = {p.H}, B = {p.B}, N = {p.N}")
    new = attn_launch.allocator(output, attn_launch.POISON)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=output.device)
    rank = new(p.B).view(torch.int32)  # (the poison's bits, 0x7FC00000, are no rank a catalogue can produce)
    target_score = new(p.B)
    _lib.check(lib.acattn_full_sort_rank(C.byref(p), int(first_item), _ptr(ws), _ptr(rank), _ptr(target_score), _stream()),
               "full_sort_rank")
    if history_index is not None:
        rows, items = unique_pairs(history_index, n)
        rows, items = rows.to(output.device), items.to(output.device)
        _lib.check(lib.acattn_full_sort_rank_exclude(C.byref(p), int(first_item), _ptr(rows), _ptr(items), rows.numel(),
                                                     _ptr(target_score), _ptr(rank), _stream()), "full_sort_rank_exclude")
    return Ranks(rank, target_score)


@torch.no_grad()
def dense_ranks(scores: torch.Tensor, target: torch.Tensor, first_item: int = 1, history_index=None) -> Ranks:
    """The same ranks counted from materialised scores [B, N] (any device): the path of the hidden sizes the kernels do not
    take.  Same order rule: ahead is !(s_j <= s_t), a NaN item score is ahead, a NaN target score or a target outside
    [first_item, N) gives rank 0."""
    B, N = scores.shape
    target = target.to(scores.device).long()
    ok = (target >= first_item) & (target < N)
    idx = torch.where(ok, target, torch.zeros_like(target))
    s_t = scores.gather(1, idx.unsqueeze(1)).squeeze(1)
    s_t = torch.where(ok, s_t, torch.full_like(s_t, float("nan")))
    ahead = ~(scores <= s_t.unsqueeze(1))
    ahead[:, :first_item] = False
    ahead[torch.arange(B, device=scores.device), idx] = False
    if history_index is not None:
        rows, items = unique_pairs(history_index, N)
        keep = rows < B
        ahead[rows[keep].to(scores.device), items[keep].to(scores.device)] = False
    rank = 1 + ahead.sum(dim=1)
    rank = torch.where(torch.isnan(s_t), torch.zeros_like(rank), rank).to(torch.int32)
    return Ranks(rank, s_t.float())
