"""Case table of the time-interval attention core (csrc/acattn_timeaware.hip) and its oracle, shared by
tests/test_timeaware_cases_cpu.py (conditioning of every case, on the CPU) and tests/test_hip_timeaware_attention.py (the
kernels).  Nothing here touches a GPU.

A case is a tests/_attention_fp64 case (inputs, mask, cotangents from _attention_fp64.problem, draws from torch_draws) plus the
time side: time_span, the time dropout's rate, which outputs carry a cotangent, and how the timestamps are drawn.  Every
kernel-level case has B <= 6 and 2 heads.  Shapes: L on, one short of and one past a tile edge (15, 16, 17, 63, 64), a single
key (1), mid-tile (33, 50), one to four key tiles, head sizes 16, 32, 64, time_span 1, 7 and 256.

Rows without an allowed key (left padding under the causal mask): the reference adds -10000 to every score of such a row, and
its fp32 rounding of `score - 10000` is 0.5-1.6e-4 of scale.  The soft-max does not see a common shift, so the restatement is
handed those rows' mask with the shift removed (`mask_for_oracle`): in float64 nothing changes beyond 1e-12
(tests/test_timeaware_cases_cpu.py asserts it), and the float32 restatement stays a usable yardstick on EVERY row -- no row,
no tensor and no case is left out of a comparison.
"""
from collections import namedtuple

import torch

from oracle import ac_tsr_ref as O
from tests import _attention_fp64 as F
from tests import _timeaware_ref as T

OUTPUTS = ("ctx_attacked", "ctx_calibrated", "M")
COMPARED_OUTPUTS = OUTPUTS + ("pen", "lse_p", "lse_m")  # penalty rows and row_stats slots 0, 1 (log2 units)
TIME_LEAVES = ("pos_k", "pos_v", "time_k", "time_v")
SUBSETS = tuple(tuple(n for n, bit in zip(OUTPUTS, (1, 2, 4)) if mask & bit) for mask in range(1, 8))
LOG2E = 1.4426950408889634

TCase = namedtuple("TCase", "id base span p_time cots stamps")


def _case(shape, span, tag="", p_drop=0.5, p_time=0.5, cots=OUTPUTS, stamps="mixed", **kw):
    name = "B{}_L{}_H{}_span{}".format(shape[0], shape[1], shape[2], span) + (f"-{tag}" if tag else "")
    return TCase(name, F._case(name, "timeaware", tuple(shape) + (2,), p_drop=p_drop, **kw), span, p_time, tuple(cots), stamps)


def _table():
    cases = [
        _case((2, 1, 32), 1), _case((3, 15, 32), 7), _case((2, 16, 64), 256), _case((3, 17, 32), 7), _case((2, 33, 64), 1),
        _case((3, 50, 128), 256), _case((2, 63, 64), 7), _case((2, 64, 128), 256), _case((2, 64, 32), 1),
    ]
    for shape, span in (((3, 17, 32), 7), ((3, 50, 128), 256)):
        cases += [
            _case(shape, span, "attn_p0", p_drop=0.0), _case(shape, span, "time_p0", p_time=0.0),
            _case(shape, span, "no_dropout", p_drop=0.0, p_time=0.0), _case(shape, span, "left_pad", left_pad=True),
            _case(shape, span, "bidirectional", causal=False),
            _case(shape, span, "bidirectional_left_pad", causal=False, left_pad=True),
        ]
    # every combination of present / NULL cotangents (`all` is above; the empty one is a test of its own)
    cases += [_case((3, 17, 32), 7, "cot_" + "+".join(s), cots=s) for s in SUBSETS[:-1]]
    cases += [_case((3, 37, 64), 256, "cot_" + "+".join(s), cots=s) for s in (("ctx_calibrated",), ("ctx_attacked", "M"))]
    # hot rows: every pair on row 0, every off-diagonal pair on row time_span
    cases += [_case((6, 50, 128), 256, "equal_stamps", stamps="equal"), _case((6, 50, 128), 256, "far_stamps", stamps="far"),
              _case((6, 17, 32), 7, "equal_stamps", stamps="equal"), _case((6, 17, 32), 7, "far_stamps", stamps="far")]
    assert len({c.id for c in cases}) == len(cases)
    return cases


CASES = _table()


def forward_key(c: TCase):
    """What the forward depends on: everything but the cotangents."""
    return c._replace(id="", cots=(), base=c.base._replace(id=""))


def leaf_names(c: TCase):
    return F.leaf_names(c.base) + list(TIME_LEAVES)


def timestamps(c: TCase, g) -> torch.Tensor:
    """int64 [B, L]: `mixed` = gaps of 0 (equal stamps: index 0 off the diagonal), small gaps and gaps past time_span (clipped),
    about a third each; `equal` = one stamp; `far` = gaps of time_span + 3."""
    B, L, span = c.base.B, c.base.L, c.span
    if c.stamps == "equal":
        return torch.full((B, L), 1000, dtype=torch.int64)
    if c.stamps == "far":
        return (torch.arange(L, dtype=torch.int64) * (span + 3) + 17).unsqueeze(0).repeat(B, 1)
    kind = torch.randint(0, 3, (B, L), generator=g)
    small = torch.randint(1, max(2, span // 4 + 1), (B, L), generator=g)
    gaps = torch.where(kind == 0, torch.zeros_like(small), torch.where(kind == 1, small, torch.full_like(small, span + 5)))
    return gaps.cumsum(1) + 5


Problem = namedtuple("Problem", "pr t index keep_k keep_v mask_for_oracle cot cot_dead")


def problem(c: TCase, seed=707) -> Problem:
    """The attention-side problem of tests/_attention_fp64.problem plus the time side, all float32 / int32 on the CPU.  The
    position rows and the tables are 0.5 N(0, 1): with the time dropout's 1 / (1 - p) the three score terms are of one size."""
    pr = F.problem(c.base)
    B, L, H = c.base.B, c.base.L, c.base.H
    g = torch.Generator().manual_seed(seed)
    t = dict(pr.t)
    t["pos_k"] = 0.5 * torch.randn(B, L, H, generator=g)
    t["pos_v"] = 0.5 * torch.randn(B, L, H, generator=g)
    t["time_k"] = 0.5 * torch.randn(c.span + 1, H, generator=g)
    t["time_v"] = 0.5 * torch.randn(c.span + 1, H, generator=g)
    index = T.get_time_matrix(timestamps(c, g), c.span)
    keep_k = keep_v = None
    if c.p_time > 0:
        keep_k = torch.empty(B, L, L, H).bernoulli_(1.0 - c.p_time, generator=g)
        keep_v = torch.empty(B, L, L, H).bernoulli_(1.0 - c.p_time, generator=g)
    mask = pr.mask_dense.expand(B, 1, L, pr.mask_dense.shape[-1]).clone()
    mask[pr.dead[:, None, :, None].expand_as(mask)] = 0.0  # the common -10000 of a row without an allowed key
    cot = {k: v + pr.cot_dead[k] for k, v in pr.cot.items() if k in c.cots}  # every row carries a cotangent, dead ones too
    cot_dead = {k: v for k, v in pr.cot_dead.items() if k in c.cots}
    return Problem(pr, t, index, keep_k, keep_v, mask, cot, cot_dead)


def oracle(c: TCase, p: Problem, draws, cot, dtype, index=None, keeps=None, tables=None):
    """({leaf: gradient}, {output: value}) of the time-interval core in `dtype` on the CPU; the loss is sum_k (out_k * cot_k)
    over the outputs in `cot`.  A leaf the loss does not reach gets zeros.  `index` / `keeps` = (keep_k, keep_v) / `tables` =
    {time_k, time_v} replace the problem's.  The table gradients are the plain derivatives, row 0 included."""
    names = leaf_names(c)
    b = c.base
    keep_k, keep_v = (p.keep_k, p.keep_v) if keeps is None else keeps
    with F.default_dtype(dtype):
        src = dict(p.t, **(tables or {}))
        x = {k: src[k].to(dtype).clone().requires_grad_(True) for k in names}
        cfg = O.EncoderCfg(n_layers=1, n_heads=b.nh, hidden_size=b.H, inner_size=4 * b.H, combine_option="gate", seq_length=b.L,
                           attn_dropout_prob=b.p_drop)
        cast = lambda v: None if v is None else v.to(dtype)
        ti = T.TimeInputs(x["pos_k"], x["pos_v"], p.index if index is None else index, x["time_k"], x["time_v"], cast(keep_k),
                          cast(keep_v), c.p_time)
        ref = T.core_from_projected_time(x["q"], x["k"], x["v"], x["qa"], x["ka"], x["gl"], p.mask_for_oracle.to(dtype),
                                         x["w_order"], x["b_order"], x["w_dist"], x["b_dist"], x["scalar"], cfg,
                                         cast(draws["noise"]), ti, keep_after=cast(draws["keep_after"]),
                                         keep_mask=cast(draws["keep_mask"]))
        grads = [None] * len(names)
        if cot:
            loss = sum((ref[k] * cot[k].to(dtype)).sum() for k in cot)
            grads = torch.autograd.grad(loss, [x[n] for n in names], allow_unused=True)
    outs = {k: ref[k].detach() for k in OUTPUTS}
    pen = torch.nn.functional.pad((1 - outs["M"]) ** 2, (0, 0, 0, (-b.L) % 16)).sum(-1)
    outs["pen"] = pen.view(b.B, b.nh, -1, 16).sum(-1)
    outs["lse_p"], outs["lse_m"] = ref["lse_p"].detach() * LOG2E, ref["lse_m"].detach() * LOG2E
    return {n: torch.zeros_like(x[n]).detach() if g is None else g for n, g in zip(names, grads)}, outs
