"""The one Python launch path of the attention core: struct filling, output allocation and the C-ABI calls.

ops.py (the autograd node, any configuration, validated with ops._need_cuda) and dispatch.py (the torch.ops.acattn
operators, the training form, validated with dispatch._check_problem) both end here: each entry point of
include/acattn.h's attention core is called from exactly one function below.  Nothing here validates tensors -- the callers
did -- and nothing imports ops or dispatch.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from typing import Optional

import torch

from . import _lib

# ACATTN_POISON_OUTPUTS=1 (tests): every output buffer of a launch starts as NaN instead of uninitialised memory, so an
# output element a kernel forgets to write shows up instead of reading what an earlier launch left in a reused buffer
# (round 4 found the one-row backward at head size 128 writing half of dq's columns that way).  A test switches it on after
# import by patching this name, or per call with the launch helpers' `poison` argument.
POISON = os.environ.get("ACATTN_POISON_OUTPUTS") == "1"


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def allocator(like: torch.Tensor, poison: bool):
    """new(*shape): an fp32 output buffer on `like`'s device -- NaN-filled when poisoning, torch.empty otherwise (the step
    is captured into a hipGraph: a fill would be one more node)."""
    dev = like.device
    if poison:
        return lambda *shape: torch.full(shape, float("nan"), device=dev, dtype=torch.float32)
    return lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)


def check_sequence_length(L: int) -> None:
    """One early, readable error for a sequence the attention core does not take (acattn_max_sequence_length(): 496)."""
    top = _lib.load().acattn_max_sequence_length()
    if L > top:
        raise ValueError(f"sequence length {L} is beyond the attention core's limit of {top} "
                         "(MAX_ITEM_LIST_LENGTH <= acattn_max_sequence_length())")


def fill_problem(q, k, v, qa, ka, gate, w_order, b_order, w_dist, b_dist, scalar, n_heads, p_drop, seed, seed_tensor, *,
                 key_valid=None, causal=True, mask=None, mask_mode=_lib.MASK_STRUCTURED, adversarial=True, combine="gate",
                 gate_is_prob=False, affine=None, two_level=True, rich="none", rich_ratio=None, anneal_rate=0.0,
                 rnd=None) -> _lib.Problem:
    """acattn_problem from checked tensors.  The defaults are the operator form (structured mask, counter RNG, `gate`,
    two_level).  `rnd` = (noise, keep_after, keep_mask, keep_before), fp32 / uint8 tensors or None, selects explicit
    randomness; the caller keeps those tensors alive until the launch has returned."""
    B, L, H = q.shape
    check_sequence_length(L)
    p = _lib.Problem()
    p.B, p.L, p.H, p.n_heads = B, L, H, n_heads
    p.q, p.k, p.v = _ptr(q), _ptr(k), _ptr(v)
    p.adversarial = int(adversarial)
    p.combine_option = _lib.COMBINE[combine]
    if adversarial:
        p.qa, p.ka = _ptr(qa), _ptr(ka)
        if combine == "gate":
            p.gate_logits, p.gate_is_prob = _ptr(gate), int(bool(gate_is_prob))
    p.affine = _ptr(affine)
    p.mask_mode = mask_mode
    if mask_mode == _lib.MASK_STRUCTURED:
        p.causal, p.key_valid = int(causal), _ptr(key_valid)
    else:
        p.mask = _ptr(mask)
    if w_order is not None:
        p.w_order, p.b_order = _ptr(w_order), _ptr(b_order)
    if w_dist is not None:
        p.w_dist, p.b_dist, p.scalar = _ptr(w_dist), _ptr(b_dist), _ptr(scalar)
    p.anneal_rate, p.two_level = anneal_rate, int(two_level)
    if not two_level:
        p.rich_combine, p.rich_ratio = _lib.RICH[rich], _ptr(rich_ratio)
    p.p_drop = float(p_drop)
    if rnd is not None:
        p.rng_mode = _lib.RNG_EXPLICIT
        p.noise, p.keep_after, p.keep_mask, p.keep_before = (_ptr(t) for t in rnd)
        if rnd[1] is None:
            p.p_drop = 0.0  # keep masks None = no dropout
    else:
        p.rng_mode, p.seed, p.seed_device = _lib.RNG_COUNTER, seed & 0xFFFFFFFFFFFFFFFF, _ptr(seed_tensor)
    return p


def partials(io, q, n_heads: int, new) -> torch.Tensor:
    """The three per-(b, head) parameter-partial sums of a backward share ONE [B * n_heads, 4 * dh + 4] buffer (dw_order |
    dw_dist | db_order, db_dist, dscalar, drich_ratio), reduced over its rows in a single pass by the caller."""
    dh = q.shape[2] // n_heads
    width = 4 * dh + 4
    part = new(q.shape[0] * n_heads, width)
    base = part.data_ptr()
    io.dw_order_part, io.dw_dist_part, io.dsmall_part = base, base + 4 * 2 * dh, base + 4 * 4 * dh
    io.part_stride = width
    return part


def unpack_partials(tot, dh: int, w_order, b_order, w_dist, b_dist, scalar, rich_ratio=None):
    """(g_w_order, g_b_order, g_w_dist, g_b_dist, g_scalar, g_rich_ratio) as views of the row-summed partials `tot`."""
    small = tot[4 * dh:]
    return (tot[:2 * dh].view_as(w_order) if w_order is not None else None,
            small[0:1].view_as(b_order) if w_order is not None else None,
            tot[2 * dh:4 * dh].view_as(w_dist) if w_dist is not None else None,
            small[1:2].view_as(b_dist) if w_dist is not None else None,
            small[2:3].view_as(scalar) if w_dist is not None else None,
            small[3:4].view_as(rich_ratio) if rich_ratio is not None else None)


def workspace(n_bytes: int, device) -> torch.Tensor:
    """A launch's scratch (row scalars of the streaming and the long backward); `n_bytes` is the library's `*_workspace_bytes` answer."""
    return torch.empty(max(int(n_bytes), 4) // 4, device=device, dtype=torch.float32)


def gate_summed_rule(B: int, L: int, H: int, n_heads: int, n_read_rows: int, block_bitmap: bool, mask_cotangent: bool,
                     attack_only: bool) -> bool:
    """gate_summed() below without a library or pointers, for shape functions (Meta / fake tensors): the operator form
    under the default environment and ACATTN_BWD_AUTO.  One read position per sequence, no block bitmap, not attack-only:
    the one-row backward, alone or (mask cotangent, L <= 64, dh <= 64) behind the mask-only launch of the split
    (csrc/acattn_bwd.hip: acattn_bwd_gate_summed; tests/test_hip_onehop.py compares the two).  A pinned backward kernel
    (backward_kernel below) is not known here: a read-row launch under a pin writes [B,nh,L,L] where this rule says
    [B,1,L,L], so fake-tensor tracing of the backward is only right under ACATTN_BWD_AUTO; the pin is for measurements."""
    dh = H // n_heads
    if n_read_rows != 1 or block_bitmap or attack_only or L > 208 or dh not in (16, 32, 64, 128):
        return False
    if B * n_heads * L * L >= 1 << 30 or B * L * H >= 1 << 30:
        return False
    return not mask_cotangent or (L <= 64 and dh <= 64)


def backward_kernel_choice(lib) -> int:
    """The calling thread's acattn_select_backward_kernel setting (an out-of-range argument changes nothing)."""
    return lib.acattn_select_backward_kernel(-1)


@contextlib.contextmanager
def backward_kernel(lib, which: int):
    """acattn_select_backward_kernel is per host thread, and autograd runs the backward of a node with HIP tensors on a
    worker thread of its own, where a kernel pinned by the thread that built the graph is not in force.  The forward records
    its thread's setting (backward_kernel_choice) and the backward issues its launches under it, on whichever thread it
    runs (tests/test_hip_attention_bwd_fp64.py asserts that a pinned kernel is the one that ran)."""
    prev = lib.acattn_select_backward_kernel(which)
    try:
        yield
    finally:
        lib.acattn_select_backward_kernel(prev)


def gate_summed(lib, prob, io) -> bool:
    """Will this launch write the gate gradient already summed over the heads ([B,1,L,L], acattn_bwd_io.dgate_summed)?
    `io.dgate_logits` must be non-NULL (any pointer: it is only tested)."""
    return bool(lib.acattn_calibrated_attention_bwd_gate_summed(C.byref(prob), C.byref(io)))


def attention_fwd_launch(lib, prob, q, n_heads: int, *, adversarial: bool, want_probs: bool = False, want_penalty: bool,
                         poison: bool = False):
    """One acattn_calibrated_attention_fwd call for a filled `prob`.  Returns (ctx_attacked, ctx_calibrated, M, row_stats,
    probs, penalty_part); what the configuration does not produce is None (probs: {} unless `want_probs`)."""
    B, L, H = q.shape
    new = allocator(q, poison or POISON)
    out = _lib.FwdOut()
    ctx_cal = new(B, L, H)
    out.ctx_calibrated = _ptr(ctx_cal)
    ctx_att = M = stats = pen = None
    probs = {}
    if adversarial:
        ctx_att, M = new(B, L, H), new(B, n_heads, L, L)
        stats = torch.empty(B, n_heads, L, _lib.NSTAT, device=q.device, dtype=torch.float32)  # (3 of its 8 columns are spare)
        out.ctx_attacked, out.attack_mask, out.row_stats = _ptr(ctx_att), _ptr(M), _ptr(stats)
        if want_probs:
            for name in ("after_spatial", "before_spatial", "perturbed_attention", "calibrated_attention"):
                probs[name] = new(B, n_heads, L, L)
                setattr(out, name, _ptr(probs[name]))
        # sum (1 - M)^2 per (sequence, head, query block): the mask penalty without another pass over M (include/acattn.h);
        # filled by the launch itself or by acattn_mask_penalty_rows behind it (L <= 64: one more launch)
        if want_penalty:
            pen = new(B, n_heads, (L + 15) // 16)
            out.penalty_part = _ptr(pen)
    _lib.check(lib.acattn_calibrated_attention_fwd(C.byref(prob), C.byref(out), _stream()), "calibrated_attention_fwd")
    return ctx_att, ctx_cal, M, stats, probs, pen


def attention_bwd_launch(lib, prob, q, n_heads: int, M, stats, *, d_att=None, d_cal=None, d_M=None, d_pen=None,
                         read_rows=None, active_qblocks=None, attack_only: bool = False, gate: bool = True, second=None,
                         poison: bool = False):
    """One acattn_calibrated_attention_bwd call for a filled `prob`: allocates the gradients, the parameter partials and the
    workspace.  Returns (dq, dk, dv, dqa, dka, dgate_part, part).

    `read_rows` / `active_qblocks`: the context cotangents are zero outside those positions / query blocks (the caller's
    promise; with a mask cotangent every block stays active, but those without a read position only owe the mask path).
    `attack_only`: only dqa and dka are wanted (and written).  `gate` False ('fixed' / 'annealing'): no gate gradient,
    dgate_part is None; otherwise it is [B,1,L,L] when the launch sums over the heads itself (gate_summed) and
    [B,n_heads,L,L] when not.  `second` = (d_ctx_calibrated2, d_penalty_part2): the second cotangent set of the combined
    backward (acattn_bwd_io.dqa2); the result is None when the library cannot evaluate it in this launch, else it ends in
    (..., dqa2, dka2)."""
    B, L, H = q.shape
    new = allocator(q, poison or POISON)
    rest = allocator(q, False) if attack_only else new  # an attack-only launch leaves everything but dqa, dka unwritten
    io = _lib.BwdIO()
    io.attack_mask, io.row_stats = _ptr(M), _ptr(stats)
    io.d_ctx_attacked, io.d_ctx_calibrated, io.d_attack_mask = _ptr(d_att), _ptr(d_cal), _ptr(d_M)
    io.d_penalty_part = _ptr(d_pen)  # [B, n_heads, ceil(L/16)]: include/acattn.h
    dq, dk, dv, dqa, dka = rest(B, L, H), rest(B, L, H), rest(B, L, H), new(B, L, H), new(B, L, H)
    io.dq, io.dk, io.dv, io.dqa, io.dka = _ptr(dq), _ptr(dk), _ptr(dv), _ptr(dqa), _ptr(dka)
    extra = ()
    if second is not None:
        extra = (new(B, L, H), new(B, L, H))
        io.d_ctx_calibrated2, io.d_penalty_part2 = _ptr(second[0]), _ptr(second[1])
        io.dqa2, io.dka2 = _ptr(extra[0]), _ptr(extra[1])
    part = partials(io, q, n_heads, rest)
    ws = workspace(lib.acattn_calibrated_attention_bwd_workspace_bytes(C.byref(prob)), q.device)
    io.workspace = _ptr(ws)
    io.active_qblocks = _ptr(active_qblocks)
    if read_rows is not None:
        io.read_rows, io.n_read_rows = _ptr(read_rows), read_rows.shape[1]
    io.attack_only = int(attack_only)
    dgate_part = None
    if gate:
        io.dgate_logits = _ptr(q)  # (placeholder for the query: only tested for NULL)
        # (the pair launch is L > 64 without read rows, where the one-row form does not apply: not asked)
        summed = second is None and gate_summed(lib, prob, io)
        dgate_part = rest(B, 1 if summed else n_heads, L, L)
        io.dgate_logits, io.dgate_summed = _ptr(dgate_part), int(summed)
    if second is not None and not lib.acattn_calibrated_attention_bwd_pair_supported(C.byref(prob), C.byref(io)):
        return None  # (L <= 64: the row-resident kernel; L > 208: the long form; head size 128; a pinned kernel)
    _lib.check(lib.acattn_calibrated_attention_bwd(C.byref(prob), C.byref(io), _stream()), "calibrated_attention_bwd")
    return (dq, dk, dv, dqa, dka, dgate_part, part) + extra


def spatial_attention_bwd_launch(lib, prob, q, d_ctx, n_heads: int, read_rows=None, poison: bool = False):
    """One acattn_spatial_attention_bwd call for a filled `prob` (adversarial == 0): allocates the outputs, the parameter
    partials and the workspace.  Returns (dq, dk, dv, part)."""
    B, L, H = q.shape
    new = allocator(q, poison or POISON)
    io = _lib.SpatialBwdIO()
    io.d_ctx = _ptr(d_ctx)
    dq, dk, dv = new(B, L, H), new(B, L, H), new(B, L, H)
    io.dq, io.dk, io.dv = _ptr(dq), _ptr(dk), _ptr(dv)
    part = partials(io, q, n_heads, new)
    if read_rows is not None:
        io.read_rows, io.n_read_rows = _ptr(read_rows), read_rows.shape[1]
    ws = workspace(lib.acattn_spatial_attention_bwd_workspace_bytes(C.byref(prob)), q.device)
    io.workspace = _ptr(ws)
    _lib.check(lib.acattn_spatial_attention_bwd(C.byref(prob), C.byref(io), _stream()), "spatial_attention_bwd")
    return dq, dk, dv, part


def _l64_fwd_out(q, n_heads: int, want_penalty: bool, poison: bool):
    """The forward outputs of the two L <= 64 cores without re-normalisation: (FwdOut, (ctx_attacked, ctx_calibrated, M,
    row_stats, penalty_part or None))."""
    B, L, H = q.shape
    new = allocator(q, poison or POISON)
    out = _lib.FwdOut()
    ctx_att, ctx_cal, M, stats = new(B, L, H), new(B, L, H), new(B, n_heads, L, L), new(B, n_heads, L, _lib.NSTAT)
    out.ctx_attacked, out.ctx_calibrated, out.attack_mask, out.row_stats = _ptr(ctx_att), _ptr(ctx_cal), _ptr(M), _ptr(stats)
    pen = None
    if want_penalty:
        pen = new(B, n_heads, (L + 15) // 16)
        out.penalty_part = _ptr(pen)
    return out, (ctx_att, ctx_cal, M, stats, pen)


def _l64_bwd_io(new, q, n_heads: int, M, stats, d_att, d_cal, d_M, d_pen):
    """The backward's BwdIO of the same two cores with the gradients, the parameter partials and the per-head gate partials
    allocated by `new`: (BwdIO, (dq, dk, dv, dqa, dka, dgate_part [B,n_heads,L,L], part))."""
    B, L, H = q.shape
    io = _lib.BwdIO()
    io.attack_mask, io.row_stats = _ptr(M), _ptr(stats)
    io.d_ctx_attacked, io.d_ctx_calibrated, io.d_attack_mask = _ptr(d_att), _ptr(d_cal), _ptr(d_M)
    io.d_penalty_part = _ptr(d_pen)
    dq, dk, dv, dqa, dka = (new(B, L, H) for _ in range(5))
    io.dq, io.dk, io.dv, io.dqa, io.dka = _ptr(dq), _ptr(dk), _ptr(dv), _ptr(dqa), _ptr(dka)
    part = partials(io, q, n_heads, new)
    dgate_part = new(B, n_heads, L, L)
    io.dgate_logits = _ptr(dgate_part)
    return io, (dq, dk, dv, dqa, dka, dgate_part, part)


def unnorm_attention_supported(lib, prob) -> bool:
    """acattn_unnorm_attention_supported: does the un-normalised pair (csrc/acattn_unnorm.hip) cover this configuration?"""
    return bool(lib.acattn_unnorm_attention_supported(C.byref(prob)))


def unnorm_attention_fwd_launch(lib, prob, q, n_heads: int, *, want_penalty: bool, poison: bool = False):
    """One acattn_unnorm_attention_fwd call for a filled `prob` (ACSSEPT's core: no re-normalisation of the mixtures).
    Returns (ctx_attacked, ctx_calibrated, M, row_stats, penalty_part or None)."""
    out, res = _l64_fwd_out(q, n_heads, want_penalty, poison)
    _lib.check(lib.acattn_unnorm_attention_fwd(C.byref(prob), C.byref(out), _stream()), "unnorm_attention_fwd")
    return res


def unnorm_attention_bwd_launch(lib, prob, q, n_heads: int, M, stats, *, d_att=None, d_cal=None, d_M=None, d_pen=None,
                                read_rows=None, attack_only: bool = False, poison: bool = False):
    """One acattn_unnorm_attention_bwd call: allocates the gradients and the parameter partials.  Returns (dq, dk, dv, dqa,
    dka, dgate_part [B,n_heads,L,L], part) -- attention_bwd_launch's tuple.  `read_rows` / `attack_only` travel as the hints
    they are; the kernel writes every output whatever they say."""
    io, res = _l64_bwd_io(allocator(q, poison or POISON), q, n_heads, M, stats, d_att, d_cal, d_M, d_pen)
    if read_rows is not None:
        io.read_rows, io.n_read_rows = _ptr(read_rows), read_rows.shape[1]
    io.attack_only = int(attack_only)
    _lib.check(lib.acattn_unnorm_attention_bwd(C.byref(prob), C.byref(io), _stream()), "unnorm_attention_bwd")
    return res


def fill_time_ext(pos_k, pos_v, time_index, time_k, time_v, p_time: float, *, keep_k=None, keep_v=None, seed: int = 0,
                  seed_tensor=None) -> _lib.TimeExt:
    """acattn_time_ext from checked tensors (pos_k / pos_v [B,L,H] already dropped, time_index int32 [B,L,L], the two
    [time_span + 1, H] tables).  keep_k / keep_v (uint8 [B,L,L,H]) select explicit time-dropout bits; without them and with
    p_time > 0 the kernels draw the counter stream of `seed` (+ *seed_tensor).  The caller keeps the tensors alive."""
    t = _lib.TimeExt()
    t.pos_k, t.pos_v, t.time_index, t.time_k, t.time_v = _ptr(pos_k), _ptr(pos_v), _ptr(time_index), _ptr(time_k), _ptr(time_v)
    t.time_span, t.p_time = time_k.shape[0] - 1, float(p_time)
    t.keep_time_k, t.keep_time_v = _ptr(keep_k), _ptr(keep_v)
    t.time_seed, t.time_seed_device = seed & 0xFFFFFFFFFFFFFFFF, _ptr(seed_tensor)
    return t


def timeaware_attention_supported(lib, prob, text) -> bool:
    """acattn_timeaware_attention_supported: does csrc/acattn_timeaware.hip cover this configuration?  (acattn_last_error
    names the limit when not.)"""
    return bool(lib.acattn_timeaware_attention_supported(C.byref(prob), C.byref(text)))


def timeaware_attention_fwd_launch(lib, prob, text, q, n_heads: int, *, want_penalty: bool, poison: bool = False):
    """One acattn_timeaware_attention_fwd call (ACTiSASRec's core).  Returns (ctx_attacked, ctx_calibrated, M, row_stats,
    penalty_part or None)."""
    out, res = _l64_fwd_out(q, n_heads, want_penalty, poison)
    _lib.check(lib.acattn_timeaware_attention_fwd(C.byref(prob), C.byref(text), C.byref(out), _stream()),
               "timeaware_attention_fwd")
    return res


def timeaware_attention_bwd_launch(lib, prob, text, q, n_heads: int, M, stats, n_table_rows: int, *, d_att=None, d_cal=None,
                                   d_M=None, d_pen=None, poison: bool = False):
    """One acattn_timeaware_attention_bwd call: allocates the gradients, the parameter partials and the second launch's
    workspace.  Returns (dq, dk, dv, dqa, dka, dgate_part [B,n_heads,L,L], part, d_pos_k, d_time_k, d_time_v); d pos_v is dv.
    The table gradients are the kernel's true derivatives, row 0 included."""
    B, L, H = q.shape
    new = allocator(q, poison or POISON)
    io, res = _l64_bwd_io(new, q, n_heads, M, stats, d_att, d_cal, d_M, d_pen)
    g = _lib.TimeGrads()
    d_pos_k, d_time_k, d_time_v = new(B, L, H), new(n_table_rows, H), new(n_table_rows, H)
    ws = new(3, B, n_heads, L, L)
    g.d_pos_k, g.d_time_k, g.d_time_v, g.workspace = _ptr(d_pos_k), _ptr(d_time_k), _ptr(d_time_v), _ptr(ws)
    _lib.check(lib.acattn_timeaware_attention_bwd(C.byref(prob), C.byref(text), C.byref(io), C.byref(g), _stream()),
               "timeaware_attention_bwd")
    return res + (d_pos_k, d_time_k, d_time_v)
