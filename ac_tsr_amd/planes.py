"""The split weight planes of an encoder forward, made ONCE at its head.

At hidden 64 the projections and the layer tails run their products on bf16 matrix instructions with exactly split
operands.  The split of a WEIGHT depends on the weight alone, yet every workgroup of every projections launch and every
tail node used to redo it.  `make(...)` writes, in one launch (acattn_split_weights_many), the planes of every layer of
the encoder into one buffer and returns one `LayerPlanes` holder per layer; the encoder hands it to the layer, the layer
to `linear.projections` and `tail.layer_tail`, and each autograd node keeps the holder for its own backward.  The planes
are made from the weights of THIS call and die with this call's graph: an in-place update (Adam) between two forwards
cannot leave them stale, and no trainer step boundary is involved.

A holder is a plain Python object, never a tensor argument of a Function (combined.py counts graph edges per tensor
argument).  A layer or operator called without one behaves as before: the tail splits per node, the projections split
inside every workgroup.  `SHARED_PLANES = False` (or ACATTN_SHARED_PLANES=0 in the environment) restores that behaviour
for the encoder as well.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib

SHARED_PLANES = os.environ.get("ACATTN_SHARED_PLANES", "1") != "0"


class LayerPlanes:
    """`tail`: acattn_tail_problem.split_planes of the layer's dense / feed-forward weights, `proj`:
    acattn_proj_problem.split_planes of its six projections; either may be None (not made: the consumer splits itself)."""
    __slots__ = ("tail", "proj")

    def __init__(self, tail=None, proj=None):
        self.tail, self.proj = tail, proj


def _plain(*tensors) -> bool:
    return all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in tensors)


def make(layers, hidden_states, last_rows=None):
    """One holder (or None) per layer of `layers` (AttackRTransformerLayer modules) for a forward on `hidden_states`
    ([B, L, H]); `last_rows` as AttackRTransformerEncoder.forward's `_last_rows` (the last layer's tail then runs on
    those rows only, and the library may choose another form for that row count)."""
    n = len(layers)
    if not SHARED_PLANES or n == 0 or not hidden_states.is_cuda or hidden_states.dtype != torch.float32:
        return [None] * n
    from . import linear, tail as tail_mod
    from .ops import _ptr, _stream
    lib = _lib.load()
    H = hidden_states.shape[-1]
    rows_all = hidden_states.numel() // H
    jobs, sizes = [], []
    for k, layer in enumerate(layers):
        att, ffn = layer.attack_attention, layer.feed_forward
        rows = last_rows.numel() if (last_rows is not None and k == n - 1) else rows_all
        job = _lib.SplitLayer()
        keep = []
        t_bytes = p_bytes = 0
        if (tail_mod.supported(att, ffn) and tail_mod.fused_supported(att, ffn)
                and _plain(att.dense.weight, ffn.dense_1.weight, ffn.dense_2.weight)):
            t_bytes = int(lib.acattn_layer_tail_split_bytes(H, ffn.dense_1.out_features, rows))
            if t_bytes > 0:
                job.wd, job.w1, job.w2 = (_ptr(w) for w in (att.dense.weight, ffn.dense_1.weight, ffn.dense_2.weight))
                job.I = ffn.dense_1.out_features
        gate = layer.gate if layer.combine_option == 'gate' else None
        mods = (att.query, att.key, att.value, att.attack_query_transform, att.attack_key_transform)
        # (the conditions under which linear.projections takes the single-launch node: planes nobody reads are not made)
        every = mods + ((gate,) if gate is not None else ())
        if (layer.adversarial and linear.FUSED_PROJECTIONS and all(m.bias is not None for m in every)
                and _plain(*(m.weight for m in every))
                and lib.acattn_projections_supported(H, gate.out_features if gate is not None else 0)):
            p_bytes = int(lib.acattn_projections_split_bytes(H, gate.out_features if gate is not None else 0))
            if p_bytes > 0:
                job.wq, job.wk, job.wv, job.waq, job.wak = (_ptr(m.weight) for m in mods)
                if gate is not None:
                    job.wg, job.G = _ptr(gate.weight), gate.out_features
        jobs.append(job)
        sizes.append((t_bytes, p_bytes))
    total = sum(t + p for t, p in sizes)
    if total == 0:
        return [None] * n
    buf = torch.empty(total // 4, device=hidden_states.device, dtype=torch.float32)  # (every size is a multiple of 16)
    holders, off = [], 0
    for job, (t_bytes, p_bytes) in zip(jobs, sizes):
        h = LayerPlanes()
        if t_bytes:
            h.tail = buf[off // 4:(off + t_bytes) // 4]
            job.tail_planes = _ptr(h.tail)
            off += t_bytes
        if p_bytes:
            h.proj = buf[off // 4:(off + p_bytes) // 4]
            job.proj_planes = _ptr(h.proj)
            off += p_bytes
        holders.append(h if (t_bytes or p_bytes) else None)
    live = [j for j, s in zip(jobs, sizes) if s[0] or s[1]]
    for a in range(0, len(live), _lib.SPLIT_MAX_LAYERS):
        chunk = live[a:a + _lib.SPLIT_MAX_LAYERS]
        arr = (_lib.SplitLayer * len(chunk))(*chunk)
        _lib.check(lib.acattn_split_weights_many(arr, len(chunk), _stream()), "split_weights_many")
    return holders
