"""CPU suite: the case table of tests/test_hip_bwd_attack_ctx.py is well conditioned.

That test bounds the kernel's dqa and dka by tensor_bound(e32), e32 being the float32 oracle's own error against the float64
one.  For every case and cotangent form of the table (tests/_bwd_attack_ctx_cases.py), with torch-drawn noise and keep masks
standing in for the kernels' counter draws, the precondition of the GPU test is asserted here: e32 <= E32_PRECONDITION on
both gradients -- a failure on the GPU can then not be blamed on an ill-conditioned case.
"""
import pytest
import torch

from tests import _attention_fp64 as F
from tests import _bwd_attack_ctx_cases as T

CASES = [(c, False) for c in T.SHAPES] + [(T.LEFT_PAD, True)]


def test_the_table_holds_the_cases_it_is_meant_to():
    assert [(c.B, c.L, c.H, c.nh) for c in T.SHAPES] == [(3, 50, 64, 2), (8, 37, 64, 2), (8, 16, 64, 4), (8, 17, 64, 4), (8, 64, 128, 2),
                                                        (8, 50, 64, 2)]
    assert not T.SHAPES[-1].causal and T.SHAPES[-1].p_drop == 0.0 and all(c.causal and c.p_drop == 0.5 for c in T.SHAPES[:-1])
    assert (T.LEFT_PAD.B, T.LEFT_PAD.L) == (8, 50) and (T.REPLAY.B, T.REPLAY.L) == (8, 50)
    assert T.FORMS == ("cal", "cal_dpen", "cal_dM")
    pr = T.problem(T.LEFT_PAD, True)
    assert pr.dead[3, :20].all() and not pr.dead[3, 20:].any() and pr.kv[3, 20:].all() and not pr.kv[3, :20].any()


@pytest.mark.parametrize("case,left_pad", CASES, ids=[c.id for c, _ in CASES])
def test_fp32_oracle_is_a_usable_yardstick_on_every_case_and_form(case, left_pad):
    pr = T.problem(case, left_pad)
    draws = F.torch_draws(case)
    cots = T.cotangents(case, pr)
    bad = []
    for form in T.FORMS:
        cot = T.form_cotangents(cots, form)
        ref64 = T.oracle(case, pr, draws, *cot, torch.float64)
        ref32 = T.oracle(case, pr, draws, *cot, torch.float32)
        for n in ("qa", "ka"):
            assert torch.isfinite(ref64[n]).all() and torch.isfinite(ref32[n]).all() and ref64[n].abs().max() > 0, n
            e32 = F.err(ref32[n], ref64[n])
            print(f"bwd_attack_ctx_conditioning case={case.id} form={form} grad=d{n} e32={e32:.3e}")
            if not e32 <= F.E32_PRECONDITION:
                bad.append(f"{form} d{n}: e32 = {e32:.3e}")
    assert not bad, f"{case.id}: the fp32 oracle is off by more than {F.E32_PRECONDITION:.0e}: " + "; ".join(bad)
