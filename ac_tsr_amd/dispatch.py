"""The fused core as torch dispatcher operators: `torch.ops.acattn.calibrated_attention_fwd / _bwd`.

SURVEY.md section 8(b) asks for the native side to sit behind a torch custom op.  The library itself stays a plain C ABI
(include/acattn.h: no torch types in it, any host can bind it); this module registers that ABI's two attention entry
points with the dispatcher (`torch.library`), in the form the training step uses -- structured mask, counter RNG, `gate`
combine, two_level -- so that

  * the launches are visible to the dispatcher (profiler op names, `torch.library.opcheck`, FakeTensor / meta tracing: each
    op has a Meta implementation that only computes shapes),
  * `calibrated_attention_fwd` carries an autograd formula of its own (`register_autograd`: a caller of the raw op gets
    gradients without ops._CalibratedAttention), and
  * ops._CalibratedAttention routes its launches through them when the call has that form (`ops.USE_DISPATCHER`), so the
    operators tested here are the operators that train.

The options outside that form (dense masks, explicit randomness for parity tests, 'fixed' / 'annealing', one-level,
probability dumps) keep the direct C-ABI call in ops.py.  Reference semantics: recbole/model/layers.py:657-742, 883-936,
677-680 (see ops.py).
"""
from __future__ import annotations

import torch

from . import _lib, attn_launch

_LIB = torch.library.Library("acattn", "DEF")
_LIB.define(
    "calibrated_attention_fwd(Tensor q, Tensor k, Tensor v, Tensor? qa, Tensor? ka, Tensor? gate, Tensor key_valid, "
    "bool causal, Tensor w_order, Tensor b_order, Tensor w_dist, Tensor b_dist, Tensor scalar, int n_heads, "
    "float p_drop, int seed, Tensor? seed_tensor, bool gate_is_prob, Tensor? affine, bool adversarial, "
    "bool want_penalty=True) -> (Tensor, Tensor, Tensor, Tensor, Tensor)")
_LIB.define(
    "calibrated_attention_bwd(Tensor q, Tensor k, Tensor v, Tensor qa, Tensor ka, Tensor gate, Tensor key_valid, "
    "bool causal, Tensor w_order, Tensor b_order, Tensor w_dist, Tensor b_dist, Tensor scalar, int n_heads, "
    "float p_drop, int seed, Tensor? seed_tensor, bool gate_is_prob, Tensor attack_mask, Tensor row_stats, "
    "Tensor? d_ctx_attacked, Tensor? d_ctx_calibrated, Tensor? d_attack_mask, Tensor? read_rows, Tensor? active_qblocks, "
    "bool attack_only, Tensor? d_penalty_part=None) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
# Backward of the spatial-only operator (adversarial == False of the forward above).  ONE output shape whatever the
# arguments: (dq, dk, dv [B,L,H], parameter partials [B * n_heads, 4 * dh + 4] in the layout of acattn_bwd_io).
_LIB.define(
    "spatial_attention_bwd(Tensor q, Tensor k, Tensor v, Tensor key_valid, bool causal, Tensor w_order, Tensor b_order, "
    "Tensor w_dist, Tensor b_dist, Tensor scalar, int n_heads, float p_drop, int seed, Tensor? seed_tensor, Tensor d_ctx, "
    "Tensor? read_rows=None) -> (Tensor, Tensor, Tensor, Tensor)")


def _problem(q, k, v, qa, ka, gate, key_valid, causal, w_order, b_order, w_dist, b_dist, scalar, n_heads, p_drop, seed,
             seed_tensor, gate_is_prob, affine, adversarial) -> _lib.Problem:
    return attn_launch.fill_problem(q, k, v, qa, ka, gate, w_order, b_order, w_dist, b_dist, scalar, n_heads, p_drop, seed,
                                    seed_tensor, key_valid=key_valid, causal=causal, adversarial=adversarial,
                                    gate_is_prob=gate_is_prob, affine=affine)


def _check(name, t, shape, dtype, device, optional=False):
    """The operators hand raw device pointers to the C ABI, which reads them as contiguous fp32 / uint8 / int of exactly the
    documented shape (include/acattn.h): anything else -- an autocast bf16 tensor, an int64 validity mask, a gate of
    another sequence length, a tensor on another GPU -- would be reinterpreted and read out of bounds.  TypeError /
    ValueError here instead."""
    if t is None:
        if optional:
            return
        raise TypeError(f"acattn: `{name}` is required")
    if not t.is_cuda:
        raise _lib.AcattnError(f"acattn operators run only as HIP kernels on an MI355X (`{name}` is on {t.device}): no CPU fallback")
    if t.device != device:
        raise ValueError(f"acattn: `{name}` is on {t.device}, the other tensors on {device}")
    if t.dtype != dtype:
        raise TypeError(f"acattn: `{name}` must be {dtype} (got {t.dtype}): the kernels compute in fp32, outside autocast")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"acattn: `{name}` must have shape {tuple(shape)} (got {tuple(t.shape)})")
    if not t.is_contiguous():
        raise ValueError(f"acattn: `{name}` must be contiguous")


def _check_problem(q, k, v, qa, ka, gate, key_valid, w_order, b_order, w_dist, b_dist, scalar, n_heads, seed_tensor, affine,
                   adversarial):
    if q.dim() != 3:
        raise ValueError(f"acattn: `q` must be [B, L, H] (got {tuple(q.shape)})")
    B, L, H = q.shape
    if n_heads <= 0 or H % n_heads:
        raise ValueError(f"The hidden size ({H}) is not a multiple of the number of attention heads ({n_heads})")  # layers.py:618-622
    dh, dev, f32 = H // n_heads, q.device, torch.float32
    _check("q", q, (B, L, H), f32, dev)
    _check("k", k, (B, L, H), f32, dev)
    _check("v", v, (B, L, H), f32, dev)
    if adversarial:
        _check("qa", qa, (B, L, H), f32, dev)
        _check("ka", ka, (B, L, H), f32, dev)
        _check("gate", gate, (B, L, L), f32, dev)
    _check("key_valid", key_valid, (B, L), torch.uint8, dev)
    for name, t, n in (("w_order", w_order, 2 * dh), ("w_dist", w_dist, 2 * dh), ("b_order", b_order, 1), ("b_dist", b_dist, 1),
                       ("scalar", scalar, 1)):
        _check(name, t, None, f32, dev)
        if t.numel() != n:
            raise ValueError(f"acattn: `{name}` must hold {n} value(s) (got shape {tuple(t.shape)})")
    _check("seed_tensor", seed_tensor, (1,), torch.int64, dev, optional=True)
    _check("affine", affine, (B, n_heads, 4, 16 * ((L + 15) // 16)), f32, dev, optional=True)
    return B, L, H, dh


def _fwd_cuda(q, k, v, qa, ka, gate, key_valid, causal, w_order, b_order, w_dist, b_dist, scalar, n_heads, p_drop, seed,
              seed_tensor, gate_is_prob, affine, adversarial, want_penalty=True):
    B, L, H, _ = _check_problem(q, k, v, qa, ka, gate, key_valid, w_order, b_order, w_dist, b_dist, scalar, n_heads, seed_tensor,
                                affine, adversarial)
    prob = _problem(q, k, v, qa, ka, gate, key_valid, causal, w_order, b_order, w_dist, b_dist, scalar, n_heads, p_drop,
                    seed, seed_tensor, gate_is_prob, affine, adversarial)
    # the penalty row sums only when a gradient can flow (evaluation / no_grad: for L <= 64 it is one more launch behind the
    # kernel); what this form does not write is returned as an empty tensor
    ctx_att, ctx_cal, M, stats, _, pen = attn_launch.attention_fwd_launch(
        _lib.load(), prob, q, n_heads, adversarial=adversarial, want_penalty=want_penalty)
    ctx_att, M, stats, pen = (q.new_empty(0) if t is None else t for t in (ctx_att, M, stats, pen))
    return ctx_att, ctx_cal, M, stats, pen


def _fwd_meta(q, k, v, qa, ka, gate, key_valid, causal, w_order, b_order, w_dist, b_dist, scalar, n_heads, p_drop, seed,
              seed_tensor, gate_is_prob, affine, adversarial, want_penalty=True):
    B, L, H = q.shape
    if adversarial:
        return (torch.empty_like(q), torch.empty_like(q), q.new_empty(B, n_heads, L, L), q.new_empty(B, n_heads, L, _lib.NSTAT),
                q.new_empty(B, n_heads, (L + 15) // 16) if want_penalty else q.new_empty(0))
    return q.new_empty(0), torch.empty_like(q), q.new_empty(0), q.new_empty(0), q.new_empty(0)


def _bwd_cuda(q, k, v, qa, ka, gate, key_valid, causal, w_order, b_order, w_dist, b_dist, scalar, n_heads, p_drop, seed,
              seed_tensor, gate_is_prob, attack_mask, row_stats, d_ctx_attacked, d_ctx_calibrated, d_attack_mask, read_rows,
              active_qblocks, attack_only, d_penalty_part=None):
    B, L, H, dh = _check_problem(q, k, v, qa, ka, gate, key_valid, w_order, b_order, w_dist, b_dist, scalar, n_heads, seed_tensor,
                                 None, True)
    dev, f32 = q.device, torch.float32
    _check("attack_mask", attack_mask, (B, n_heads, L, L), f32, dev)
    _check("row_stats", row_stats, (B, n_heads, L, _lib.NSTAT), f32, dev)
    _check("d_ctx_attacked", d_ctx_attacked, (B, L, H), f32, dev, optional=True)
    _check("d_ctx_calibrated", d_ctx_calibrated, (B, L, H), f32, dev, optional=True)
    _check("d_attack_mask", d_attack_mask, (B, n_heads, L, L), f32, dev, optional=True)
    _check("d_penalty_part", d_penalty_part, (B, n_heads, (L + 15) // 16), f32, dev, optional=True)
    _check("active_qblocks", active_qblocks, (B,), torch.int32, dev, optional=True)
    if read_rows is not None:
        if read_rows.dim() != 2 or read_rows.shape[0] != B:
            raise ValueError(f"acattn: `read_rows` must be [B, n] (got {tuple(read_rows.shape)})")
        _check("read_rows", read_rows, None, torch.int64, dev)
    prob = _problem(q, k, v, qa, ka, gate, key_valid, causal, w_order, b_order, w_dist, b_dist, scalar, n_heads, p_drop,
                    seed, seed_tensor, gate_is_prob, None, True)
    # one read position per sequence: ONE row of each sequence's gate gradient is non-zero, and the one-row form of the
    # backward adds it straight into the head-summed [B,L,L] tensor (acattn_bwd_io.dgate_summed); returned as [B,1,L,L]
    return attn_launch.attention_bwd_launch(
        _lib.load(), prob, q, n_heads, attack_mask, row_stats, d_att=d_ctx_attacked, d_cal=d_ctx_calibrated, d_M=d_attack_mask,
        d_pen=d_penalty_part, read_rows=read_rows, active_qblocks=active_qblocks, attack_only=attack_only)


def _bwd_meta(q, k, v, qa, ka, gate, key_valid, causal, w_order, b_order, w_dist, b_dist, scalar, n_heads, p_drop, seed,
              seed_tensor, gate_is_prob, attack_mask, row_stats, d_ctx_attacked, d_ctx_calibrated, d_attack_mask, read_rows,
              active_qblocks, attack_only, d_penalty_part=None):
    B, L, H = q.shape
    e = lambda: torch.empty_like(q)
    one = attn_launch.gate_summed_rule(B, L, H, n_heads, 0 if read_rows is None else read_rows.shape[1],
                                       active_qblocks is not None, d_attack_mask is not None or d_penalty_part is not None,
                                       attack_only)
    return (e(), e(), e(), e(), e(), q.new_empty(B, 1 if one else n_heads, L, L),
            q.new_empty(B * n_heads, 4 * (H // n_heads) + 4))


def _spatial_bwd_cuda(q, k, v, key_valid, causal, w_order, b_order, w_dist, b_dist, scalar, n_heads, p_drop, seed, seed_tensor,
                      d_ctx, read_rows=None):
    B, L, H, dh = _check_problem(q, k, v, None, None, None, key_valid, w_order, b_order, w_dist, b_dist, scalar, n_heads,
                                 seed_tensor, None, False)
    _check("d_ctx", d_ctx, (B, L, H), torch.float32, q.device)
    if read_rows is not None:
        if read_rows.dim() != 2 or read_rows.shape[0] != B or read_rows.shape[1] < 1:
            raise ValueError(f"acattn: `read_rows` must be [B, n] (got {tuple(read_rows.shape)})")
        _check("read_rows", read_rows, None, torch.int64, q.device)
    prob = _problem(q, k, v, None, None, None, key_valid, causal, w_order, b_order, w_dist, b_dist, scalar, n_heads, p_drop,
                    seed, seed_tensor, False, None, False)
    return attn_launch.spatial_attention_bwd_launch(_lib.load(), prob, q, d_ctx, n_heads, read_rows)


def _spatial_bwd_meta(q, k, v, key_valid, causal, w_order, b_order, w_dist, b_dist, scalar, n_heads, p_drop, seed, seed_tensor,
                      d_ctx, read_rows=None):
    B, L, H = q.shape
    return torch.empty_like(q), torch.empty_like(q), torch.empty_like(q), q.new_empty(B * n_heads, 4 * (H // n_heads) + 4)


_LIB.impl("spatial_attention_bwd", _spatial_bwd_cuda, "CUDA")
_LIB.impl("spatial_attention_bwd", _spatial_bwd_meta, "Meta")
_LIB.impl("calibrated_attention_fwd", _fwd_cuda, "CUDA")
_LIB.impl("calibrated_attention_fwd", _fwd_meta, "Meta")
_LIB.impl("calibrated_attention_bwd", _bwd_cuda, "CUDA")
_LIB.impl("calibrated_attention_bwd", _bwd_meta, "Meta")


# ---- autograd formula of the raw forward op (a caller that bypasses ops._CalibratedAttention) ---------------------------------
def _setup_context(ctx, inputs, output):
    (q, k, v, qa, ka, gate, key_valid, causal, w_order, b_order, w_dist, b_dist, scalar, n_heads, p_drop, seed, seed_tensor,
     gate_is_prob, affine, adversarial) = inputs[:20]
    ctx.adversarial, ctx.has_seed_tensor = adversarial, seed_tensor is not None
    ctx.set_materialize_grads(False)
    ctx.bwd_kernel = attn_launch.backward_kernel_choice(_lib.load())  # this thread's pin, for the backward's (attn_launch.py)
    seed_t = seed_tensor if seed_tensor is not None else q.new_empty(0)
    if adversarial:
        ctx.args = (causal, n_heads, p_drop, seed, gate_is_prob)
        ctx.save_for_backward(q, k, v, qa, ka, gate, key_valid, w_order, b_order, w_dist, b_dist, scalar, seed_t, output[2],
                              output[3])
    else:
        ctx.args = (causal, n_heads, p_drop, seed)
        ctx.save_for_backward(q, k, v, key_valid, w_order, b_order, w_dist, b_dist, scalar, seed_t)


def _spatial_backward(ctx, d_cal):
    if d_cal is None:
        return (None,) * 21
    q, k, v, key_valid, w_order, b_order, w_dist, b_dist, scalar, seed_t = ctx.saved_tensors
    causal, n_heads, p_drop, seed = ctx.args
    dq, dk, dv, part = torch.ops.acattn.spatial_attention_bwd(
        q, k, v, key_valid, causal, w_order, b_order, w_dist, b_dist, scalar, n_heads, p_drop, seed,
        seed_t if ctx.has_seed_tensor else None, d_cal.contiguous(), None)
    grads = attn_launch.unpack_partials(part.sum(0), q.shape[-1] // n_heads, w_order, b_order, w_dist, b_dist, scalar)
    return (dq, dk, dv, None, None, None, None, None) + grads[:5] + (None,) * 8


def _backward(ctx, d_att, d_cal, d_M, _d_stats, d_pen=None):
    if not ctx.adversarial:
        return _spatial_backward(ctx, d_cal)
    q, k, v, qa, ka, gate, key_valid, w_order, b_order, w_dist, b_dist, scalar, seed_t, M, stats = ctx.saved_tensors
    causal, n_heads, p_drop, seed, gate_is_prob = ctx.args
    con = lambda t: None if t is None else t.contiguous()
    with attn_launch.backward_kernel(_lib.load(), ctx.bwd_kernel):
        dq, dk, dv, dqa, dka, dgate_part, part = torch.ops.acattn.calibrated_attention_bwd(
            q, k, v, qa, ka, gate, key_valid, causal, w_order, b_order, w_dist, b_dist, scalar, n_heads, p_drop, seed,
            seed_t if ctx.has_seed_tensor else None, gate_is_prob, M, stats, con(d_att), con(d_cal), con(d_M), None, None, False,
            con(d_pen))
    grads = attn_launch.unpack_partials(part.sum(0), q.shape[-1] // n_heads, w_order, b_order, w_dist, b_dist, scalar)
    dgate = dgate_part[:, 0] if dgate_part.shape[1] == 1 else dgate_part.sum(1)
    return (dq, dk, dv, dqa, dka, dgate, None, None) + grads[:5] + (None,) * 8


torch.library.register_autograd("acattn::calibrated_attention_fwd", _backward, setup_context=_setup_context, lib=_LIB)
