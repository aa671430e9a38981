"""CPU check of the case table of the time-interval attention core (tests/_timeaware_cases.py).  Every case must satisfy the
project's precondition -- the float32 restatement within E32_PRECONDITION = 2e-5 of the float64 one, relative to the tensor's
maximum, on EVERY compared output and EVERY tensor gradient, all rows included (1e-4 for the three single numbers) -- so that tensor_bound(e32) = max(1e-4, 2 e32) in
tests/test_hip_timeaware_attention.py is the 1e-4 floor and a badly conditioned input cannot loosen it.  Every compared tensor
must also have a scale: a gradient the loss reaches is not allowed to be (nearly) zero.  Share of tensors, rows or cases
excluded from a comparison: 0.
"""
import pytest
import torch

from tests import _attention_fp64 as F
from tests import _timeaware_cases as TC

MIN_SCALE = 1e-4
# The three single-number gradients (b_order, b_dist, scalar) are sums of B h L L signed terms: their float32 value carries the
# cancellation, up to 6e-5 of the result in this table.  They are held to 1e-4, so their bound max(1e-4, 2 e32) stays <= 2e-4.
SCALAR_E32 = 1e-4


def test_the_table_is_the_one_the_kernels_are_held_to():
    shapes = {(c.base.L, c.base.H // c.base.nh, c.span) for c in TC.CASES}
    assert {s[0] for s in shapes} >= {1, 15, 16, 17, 33, 50, 63, 64}
    assert {s[1] for s in shapes} == {16, 32, 64}
    assert {s[2] for s in shapes} == {1, 7, 256}
    assert all(c.base.B <= 6 and c.base.nh == 2 for c in TC.CASES)
    assert {(c.base.causal, c.base.left_pad) for c in TC.CASES} == {(True, False), (True, True), (False, False), (False, True)}
    assert {(c.base.p_drop, c.p_time) for c in TC.CASES} == {(0.5, 0.5), (0.0, 0.5), (0.5, 0.0), (0.0, 0.0)}
    assert {c.cots for c in TC.CASES} == set(TC.SUBSETS)  # every non-empty combination of cotangents
    assert {c.stamps for c in TC.CASES} == {"mixed", "equal", "far"}
    assert max(c.base.B for c in TC.CASES if c.stamps != "mixed") == 6


@pytest.mark.parametrize("case", [c for c in TC.CASES if c.stamps == "mixed"], ids=lambda c: c.id)
def test_the_mixed_timestamps_reach_row_0_off_the_diagonal_and_the_clip(case):
    c = case
    if c.base.L == 1:
        return
    p = TC.problem(c)
    off = ~torch.eye(c.base.L, dtype=torch.bool).expand_as(p.index)
    assert (p.index[off] == 0).any() and (p.index == c.span).any()
    assert p.index.min() == 0 and p.index.max() == c.span and p.index.dtype == torch.int32


def test_the_hot_row_cases_put_every_pair_on_one_row():
    for c in TC.CASES:
        p = TC.problem(c)
        off = ~torch.eye(c.base.L, dtype=torch.bool).expand_as(p.index)
        if c.stamps == "equal":
            assert (p.index == 0).all()
        if c.stamps == "far":
            assert (p.index[off] == c.span).all()


@pytest.mark.parametrize("case", TC.CASES, ids=lambda c: c.id)
def test_fp32_restatement_is_a_usable_yardstick_on_every_tensor(case):
    c = case
    p, draws = TC.problem(c), F.torch_draws(c.base)
    g32, o32 = TC.oracle(c, p, draws, p.cot, torch.float32)
    g64, o64 = TC.oracle(c, p, draws, p.cot, torch.float64)
    worst, scales = {}, {}
    for k in TC.COMPARED_OUTPUTS:
        worst["out " + k], scales["out " + k] = F.err(o32[k], o64[k]), o64[k].abs().max().item()
    reached = set(TC.leaf_names(c))
    if "ctx_attacked" not in c.cots and "ctx_calibrated" not in c.cots:  # the mask's cotangent reaches qa and ka alone
        reached = {"qa", "ka"}
    if "ctx_calibrated" not in c.cots:  # the gate enters the calibrated mixture alone
        reached -= {"gl"}
    if c.base.L == 1:  # a soft-max over one key is the constant 1: nothing reaches the scores
        reached &= {"v", "gl", "pos_v", "time_v"}
    for n in TC.leaf_names(c):
        if n in reached:
            worst["d" + n], scales["d" + n] = F.err(g32[n], g64[n]), g64[n].abs().max().item()
        else:
            assert g64[n].abs().max() == 0, n
    print(f"timeaware_conditioning case={c.id} " + " ".join(f"{k}={v:.1e}/{scales[k]:.1e}" for k, v in worst.items()))
    limit = lambda k: SCALAR_E32 if k[1:] in F.SCALAR_GRADS else F.E32_PRECONDITION
    bad = {k: v for k, v in worst.items() if not v <= limit(k)}
    assert not bad, f"{c.id}: e32 beyond {F.E32_PRECONDITION:.0e} ({SCALAR_E32:.0e} for the single numbers): {bad}"
    flat = {k: v for k, v in scales.items() if not v >= MIN_SCALE}
    assert not flat, f"{c.id}: compared tensors without a scale: {flat}"


@pytest.mark.parametrize("case", [c for c in TC.CASES if c.base.left_pad and c.base.causal], ids=lambda c: c.id)
def test_dropping_the_common_shift_of_a_dead_row_changes_nothing_in_float64(case):
    """The restatement on the reference's own mask (-10000 on every key of a row without an allowed key) against the one
    the tests use (that row's mask zeroed): the soft-max does not see a common shift."""
    c = case
    p, draws = TC.problem(c), F.torch_draws(c.base)
    assert p.pr.dead.any()
    g_used, o_used = TC.oracle(c, p, draws, p.pr.cot_dead, torch.float64)
    literal = p._replace(mask_for_oracle=p.pr.mask_dense)
    g_lit, o_lit = TC.oracle(c, literal, draws, p.pr.cot_dead, torch.float64)
    for k in TC.OUTPUTS + ("pen",):
        assert F.err(o_used[k], o_lit[k]) <= 1e-11, k
    for n in TC.leaf_names(c):
        assert F.err(g_used[n], g_lit[n]) <= 1e-10, n
