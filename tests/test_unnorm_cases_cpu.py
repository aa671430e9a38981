"""CPU check of the case table of the un-normalised attention core (tests/_unnorm_cases.py): every case must satisfy the
project's precondition -- the float32 oracle within E32_PRECONDITION = 2e-5 of the float64 oracle on every output and every
gradient -- so that a badly conditioned input cannot loosen tensor_bound(e32) in tests/test_hip_unnorm_attention.py.  Rows
without an allowed key are excluded from the forward outputs here: there the fp32 oracle carries the reference's rounding
of `score - 10000` (0.5-1.6e-4 of scale) and float64 is the yardstick on its own.
"""
import pytest
import torch

from tests import _attention_fp64 as F
from tests import _unnorm_cases as UC


def test_the_table_is_the_one_the_kernels_are_held_to():
    assert len(UC.CASES) == 6 * 6 + 3
    assert {(c.B, c.L, c.H, c.nh) for c in UC.CASES} == set(UC.SHAPES) | {(3, 50, 128, 4)}
    assert {c.L % 16 for c in UC.CASES} >= {0, 1, 2, 5}  # on, one past, two past (50) a tile edge, mid-tile (37)
    assert {c.H // c.nh for c in UC.CASES} == {16, 32, 64}
    assert {(c.L + 15) // 16 for c in UC.CASES} == {1, 2, 3, 4}
    assert not any((c.B, c.L, c.H, c.nh, c.p_drop) == (3, 50, 128, 4, 0.0) for c in UC.CASES)


@pytest.mark.parametrize("case", UC.CASES, ids=lambda c: c.id)
def test_fp32_oracle_is_a_usable_yardstick(case):
    c = case
    pr, draws = F.problem(c), F.torch_draws(c)
    g32, o32 = UC.oracle(c, pr, draws, pr.cot, torch.float32)
    g64, o64 = UC.oracle(c, pr, draws, pr.cot, torch.float64)
    worst = {}
    for k in UC.OUTPUTS:
        worst["out " + k] = F.err(UC.live_rows(pr, k, o32[k]), UC.live_rows(pr, k, o64[k]))
    for n in F.leaf_names(c):
        if n in F.TENSOR_GRADS and g64[n].abs().max() > 0:
            worst["d" + n] = F.err(g32[n], g64[n])
    print(f"unnorm_conditioning case={c.id} " + " ".join(f"{k}={v:.1e}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= F.E32_PRECONDITION}
    assert not bad, f"{c.id}: e32 beyond {F.E32_PRECONDITION:.0e}: {bad}"
