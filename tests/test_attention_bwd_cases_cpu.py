"""CPU suite: the case table of tests/test_hip_attention_bwd_fp64.py is well conditioned.

That test bounds a kernel's gradient error by max(1e-4, 2 * e32), where e32 is the error of the float32 oracle against the
float64 one on the same inputs.  A badly conditioned input (an order affine whose argument reaches the range where fp32
`1 - sigmoid(x)` rounds to 0, x > 16.6) makes the float32 oracle itself wrong and would loosen that bound without anybody
noticing.  Here every case of the table (tests/_attention_fp64.py::CASES; cases that differ only in the pinned backward
kernel share their inputs and are run once) runs oracle/ac_tsr_ref.py::core_from_projected(..., materialize=False) under
torch autograd in float64 and in float32, with torch-drawn noise and keep masks standing in for the kernels' counter draws,
and the precondition of the GPU test is asserted: e32 <= 2e-5 on every tensor-valued gradient.
"""
import pytest
import torch

from tests import _attention_fp64 as F


def _unique_problems():
    seen, out = set(), []
    for c in F.CASES:
        if F.problem_key(c) not in seen:
            seen.add(F.problem_key(c))
            out.append(c)
    return out


def test_the_table_holds_the_cases_it_is_meant_to():
    train = [c for c in F.CASES if c.kind == "train"]
    general = [c for c in F.CASES if c.kind == "general"]
    assert len(train) == 40 and len(general) == 14
    assert {(c.B, c.L, c.H, c.nh) for c in train} == {(64, 50, 64, 2), (512, 50, 64, 2), (12, 50, 64, 4), (6, 37, 64, 2), (8, 64, 128, 2),
                                                     (5, 77, 64, 4), (8, 200, 128, 4), (2, 130, 256, 4), (3, 200, 256, 2), (5, 50, 256, 2)}
    assert all(c.pattern == "all" for c in general)
    assert F.calibrator_scale(64, 2) == 0.3 and abs(F.calibrator_scale(128, 2) - 0.2121) < 1e-4 and F.calibrator_scale(256, 2) == 0.15


@pytest.mark.parametrize("case", _unique_problems(), ids=lambda c: c.id)
def test_fp32_oracle_is_a_usable_yardstick_on_every_case(case):
    pr = F.problem(case)
    draws = F.torch_draws(case)
    ref64 = F.oracle_grads(case, pr, draws, pr.cot, torch.float64)
    ref32 = F.oracle_grads(case, pr, draws, pr.cot, torch.float32)
    bad = []
    for n in F.leaf_names(case):
        e32 = F.err(ref32[n], ref64[n]) if ref64[n].abs().max() > 0 else ref32[n].abs().max().item()
        print(f"attention_bwd_conditioning case={case.id} grad=d{n} e32={e32:.3e}")
        assert torch.isfinite(ref64[n]).all() and torch.isfinite(ref32[n]).all(), n
        if n in F.TENSOR_GRADS and not e32 <= F.E32_PRECONDITION:
            bad.append(f"d{n}: e32 = {e32:.3e}")
    assert not bad, f"{case.id}: the fp32 oracle is off by more than {F.E32_PRECONDITION:.0e}: " + "; ".join(bad)
    # a gradient the loss does not reach is identically zero on both sides (the gate's without a calibrated cotangent)
    if case.pattern == "attacked_read_row_plus_mask":
        assert ref64["gl"].abs().max() == 0 and ref32["gl"].abs().max() == 0
