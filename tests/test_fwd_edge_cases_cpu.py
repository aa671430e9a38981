"""CPU suite: the case table of the forward tile-edge tests (tests/_fwd_edge_cases.py; tests/test_hip_fwd_edges.py runs it).

(a) the table is what it claims: unique ids, the form column agrees with expected_form() (written from the conditions of
    acattn_fwd.hip::acattn_launch_fwd and the launch_* functions, cited there), the tail-block predicate marks exactly the
    lengths 1 <= L % 16 <= 4 of the 4-tile streaming form with the producer extras, every form runs at every length the
    table lists for it (LENGTHS), and every (form, head size) and every (HALF, PRE, flavour) the dispatch can produce appears -- the
    streaming instantiations each at an on-edge and at a one-past length.
(b) the yardstick is sound: with torch-drawn noise and keep masks standing in for the counter draws, the float32 oracle is
    within a QUARTER of each bound of the GPU test from the float64 oracle on live rows, so what the GPU test measures
    against float64 is the kernel's error and not the conditioning of the inputs.  A case that misses the quarter gets
    other inputs (its `seed`), never another bound.
(c) the dead-row sets (query rows without an allowed key) are what the layout says."""
import itertools

import pytest
import torch

from tests import _attention_fp64 as F
from tests import _attention_fwd_ref as R
from tests import _fwd_edge_cases as E


def test_ids_are_unique_and_the_batch_is_four_sequences_of_two_heads():
    assert len({c.id for c in E.CASES}) == len(E.CASES)
    assert all(c.B == 4 and c.nh == 2 for c in E.CASES)


@pytest.mark.parametrize("case", E.CASES, ids=lambda c: c.id)
def test_the_form_column_is_what_the_dispatch_conditions_give(case):
    assert E.expected_form(case) == case.form
    assert case.L in E.LENGTHS[case.form] or case.H // case.nh != 32 or case.fpin == "auto"


def test_the_tail_block_predicate_marks_the_tail_lengths():
    tail = [c for c in E.CASES if E.tail_block(c)]
    assert all(c.form == "stream4" and c.extras and c.L % 16 in (1, 2, 3, 4) for c in tail)
    assert all(E.tail_block(c) for c in E.CASES if c.form == "stream4" and c.extras and c.L in (1, 2, 17, 20, 33, 36, 49, 51, 52))
    assert not any(E.tail_block(c) for c in E.CASES if c.L % 16 in (0, 5, 15) or not c.extras or c.form != "stream4")
    # one, two, three and four rows; one, two, three and four query blocks; both masks; every (ADV, HALF)
    assert {c.L % 16 for c in tail} == {1, 2, 3, 4} and {(c.L + 15) // 16 for c in tail} == {1, 2, 3, 4}
    assert {(c.adversarial, c.p_drop == 0.5, c.causal) for c in tail} == set(itertools.product((True, False), repeat=3))
    # the re-ordered grid (causal, at least two blocks), and the same lengths on the ordinary path: without the extras,
    # under either mask
    assert {(c.L + 15) // 16 for c in tail if E.reordered_grid(c)} == {2, 3, 4}
    for L in sorted({c.L for c in tail}):
        plain = {c.causal for c in E.CASES if c.form == "stream4" and c.L == L and not c.extras and c.adversarial}
        assert plain == {True, False}, L


def test_every_form_runs_at_every_listed_length_and_in_every_instantiation():
    for form, lengths in E.LENGTHS.items():
        at32 = {c.L for c in E.CASES if c.form == form and c.H // c.nh == 32}
        assert set(lengths) <= at32, (form, sorted(set(lengths) - at32))
    sizes = {(c.form, c.H // c.nh) for c in E.CASES}
    want = {(f, dh) for f in E.FORMS for dh in (16, 32, 64, 128)} - {("dma", 128), ("fast", 128)}
    assert sizes == want, sizes ^ want
    for form in ("stream4", "stream13"):
        combos = {(c.p_drop == 0.5, c.extras, c.adversarial) for c in E.CASES if c.form == form}
        assert combos == set(itertools.product((True, False), repeat=3)), form
        # every instantiation at a multiple of 16 and one past a multiple of 16
        for dh, adv, half, pre in itertools.product((16, 32, 64, 128), (True, False), (True, False), (True, False)):
            ls = {c.L % 16 for c in E.CASES if E.instantiation(c) == (form, dh, adv, half, pre)}
            assert {0, 1} <= ls, (form, dh, adv, half, pre, ls)
    for form in ("dma", "fast"):
        for dh, adv in itertools.product(E.STAGED_HEAD_SIZES, (True, False)):
            ls = {c.L % 16 for c in E.CASES if E.instantiation(c) == (form, dh, adv)}
            assert {0, 1} <= ls, (form, dh, adv, ls)
    assert {c.p_drop for c in E.CASES} == {0.5, 0.1, 0.0}
    # the instantiation of the streaming kernel that keeps registers in scratch: head size 64, L > 64, in-kernel affines
    assert {c.L for c in E.CASES if c.form == "stream13" and c.H // c.nh == 64 and not c.extras and c.adversarial} >= {65, 208}
    # the general kernel's options at a one-past length of either tile count
    for L in (17, 65):
        opts = [c for c in E.CASES if c.form == "general" and c.L == L and c.kind == "general"]
        assert {c.combine for c in opts} == {"gate", "fixed", "annealing"} and {c.mask for c in opts} == {"structured", "dense_LL", "dense_L"}
        assert {(c.two_level, c.rich) for c in opts} >= {(False, "fixed"), (False, "trainable")}
        assert {c.terms for c in opts} == {("order", "distance"), ("order",), ("distance",)}
    # only the streaming and the long forms read the affine planes; explicit randomness is the general kernel's alone
    assert all(c.form == "general" for c in E.CASES if c.kind == "general")
    assert all(c.two_level for c in E.CASES if c.form == "long")


@pytest.mark.parametrize("L,causal", [(L, causal) for L in sorted({c.L for c in E.CASES}) for causal in (True, False)])
def test_dead_rows_are_what_the_layout_says(L, causal):
    c = next((c for c in E.CASES if c.L == L and c.causal == causal and c.H == 64), None)
    if c is None:
        c = next(c for c in E.CASES if c.L == L and c.H == 64)._replace(causal=causal, mask="structured")
    pr = R.edge_problem(c)
    assert torch.equal(pr.dead, R.edge_dead_rows(L, causal))
    assert pr.kv[0].all() and not pr.kv[3].any() and pr.kv[1].sum() == max(1, L // 2) and pr.kv[1][0] == 1
    assert pr.dead[3].all() and not pr.dead[0].any() and not pr.dead[1].any()
    if L >= 2:
        assert pr.kv[2][-1] == 1 and pr.kv[2][0] == 0 and bool(pr.dead[2].any()) == causal and not pr.dead[2].all()


_KEYS = {}
for _c in E.CASES:
    _KEYS.setdefault(E.problem_key(_c), _c)


@pytest.mark.parametrize("case", list(_KEYS.values()), ids=lambda c: c.id)
def test_the_fp32_oracle_is_within_a_quarter_of_each_bound_on_live_rows(case):
    c = case
    pr = R.edge_problem(c, seed=c.seed)
    draws = F.torch_draws(c)
    ref32, ref64 = R.oracle_forward(c, pr, draws, torch.float32), R.oracle_forward(c, pr, draws, torch.float64)
    got = {"M": ref32["M"], "ctx_attacked": ref32["ctx_attacked"], "ctx_calibrated": ref32["ctx_calibrated"],
           "ctx_spatial": ref32["ctx_spatial"], "row_stats": ref32["stats"]}
    for k in ("lse_f", "lse_b"):
        if ref64[k] is not None:
            got[k] = ref32[k]
    bounds = {"M": R.M_BOUND, "ctx_attacked": R.CTX_BOUND, "ctx_calibrated": R.CTX_BOUND, "ctx_spatial": R.CTX_BOUND,
              "row_stats": R.STAT_BOUND, "lse_f": R.STAT_BOUND, "lse_b": R.STAT_BOUND}
    errs = R.edge_errors(pr, got, ref32, ref64)
    print(f"fwd_edges_conditioning case={c.id} " + " ".join(f"{k}={v[0]:.3e}" for k, v in errs.items()))
    for k, (e_live, _, _) in errs.items():
        assert torch.isfinite(got[k]).all(), k
        assert e_live <= bounds[k] / 4, f"{c.id}: the fp32 oracle's {k} is {e_live:.3e} from the fp64 one (> {bounds[k] / 4:.2e})"
