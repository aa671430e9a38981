"""Case table of the un-normalised attention core (csrc/acattn_unnorm.hip) and its oracle, shared by
tests/test_unnorm_cases_cpu.py (conditioning of every case, on the CPU) and tests/test_hip_unnorm_attention.py (the kernels).

Inputs and cotangents come from tests/_attention_fp64.problem (calibrator weights at calibrator_scale), draws from
tests/_attention_fp64.torch_draws, the reference from tests/_unnorm_ref.core_from_projected_unnorm differentiated by torch
autograd in a chosen dtype.  Nothing here touches a GPU.

Shapes (B, L, H, heads): L on, one past and one short of a tile edge (16, 17, 49, 50, 64) and mid-tile (37), one to four key
tiles, head sizes 16, 32 and 64.  (3, 50, 128, 4) with `all` at p_drop 0 sits at e32 = 2.4e-5, past the precondition, and
is deliberately not in the table.
"""
import torch

from oracle import ac_tsr_ref as O
from tests import _attention_fp64 as F
from tests import _unnorm_ref as U

SHAPES = ((3, 17, 32, 2), (2, 16, 32, 2), (3, 37, 64, 2), (2, 49, 64, 2), (3, 50, 128, 2), (2, 64, 128, 2))
PATTERNS = ("all", "attacked_read_row_plus_mask", "calibrated_read_row")
OUTPUTS = ("ctx_attacked", "ctx_calibrated", "M")


def _table():
    cases = []

    def add(shape, pattern, tag="", **kw):
        name = "B{}_L{}_H{}_h{}".format(*shape) + f"-{pattern}" + (f"-{tag}" if tag else "")
        cases.append(F._case(name, "unnorm", shape, pattern=pattern, **kw))

    for shape in SHAPES:
        for pattern in PATTERNS:
            add(shape, pattern)
        add(shape, "all", "p0", p_drop=0.0)
        add(shape, "all", "left_pad", left_pad=True)
        add(shape, "all", "bidirectional", causal=False)
    for pattern in PATTERNS:
        add((3, 50, 128, 4), pattern)
    assert len({c.id for c in cases}) == len(cases)
    return cases


CASES = _table()


def forward_key(c):
    """What the forward depends on: everything but the cotangent pattern."""
    return c._replace(id="", pattern="")


def oracle(c, pr, draws, cot, dtype):
    """({leaf: gradient}, {output: value}) of the un-normalised core in `dtype` on the CPU; the loss is sum_k (out_k * cot_k)
    over the outputs in `cot`.  A leaf the loss does not reach gets zeros."""
    names = F.leaf_names(c)
    with F.default_dtype(dtype):
        x = {k: pr.t[k].to(dtype).clone().requires_grad_(True) for k in names}
        cfg = O.EncoderCfg(n_layers=1, n_heads=c.nh, hidden_size=c.H, inner_size=4 * c.H, combine_option="gate", seq_length=c.L,
                           attn_dropout_prob=c.p_drop)
        cast = lambda v: None if v is None else v.to(dtype)
        ref = U.core_from_projected_unnorm(x["q"], x["k"], x["v"], x["qa"], x["ka"], x["gl"], pr.mask_dense.to(dtype),
                                           x["w_order"], x["b_order"], x["w_dist"], x["b_dist"], x["scalar"], cfg,
                                           cast(draws["noise"]), keep_after=cast(draws["keep_after"]),
                                           keep_mask=cast(draws["keep_mask"]))
        grads = [None] * len(names)
        if cot:
            loss = sum((ref[k] * cot[k].to(dtype)).sum() for k in cot)
            grads = torch.autograd.grad(loss, [x[n] for n in names], allow_unused=True)
    outs = {k: ref[k].detach() for k in OUTPUTS}
    return {n: torch.zeros_like(x[n]).detach() if g is None else g for n, g in zip(names, grads)}, outs


def live_rows(pr, name, t):
    """`t` with the rows that have no allowed key zeroed (M: [B,h,L,L]; contexts: [B,L,H])."""
    live = ~pr.dead
    return t * (live[:, None, :, None] if name == "M" else live[:, :, None]).to(t.dtype)
