"""CPU suite of the long-sequence attention (208 < L <= 496): the conditioning of its case table, the validation paths that
return before any HIP call, and the register / scratch figures of the long kernels' code objects.

(a) as tests/test_attention_bwd_cases_cpu.py for tests/_long_cases.py::CASES: the float32 oracle must be within 2e-5 of the
float64 one on every tensor-valued gradient, or the bound max(1e-4, 2 * e32) of the GPU test would be loosened by the input.
(b) the ceiling and the refusals of include/acattn.h's "Supported:" paragraph.  (c) no long kernel spills."""
import ctypes as C
import glob
import os
import shutil

import pytest
import torch

from ac_tsr_amd import _lib
from tests import _attention_fp64 as F
from tests import _long_cases as LC


def test_the_table_holds_the_cases_it_is_meant_to():
    assert all(208 < c.L <= 496 for c in LC.CASES)
    assert {c.L for c in LC.CASES} == {209, 224, 257, 272, 300, 496}
    assert {c.H // c.nh for c in LC.CASES} == {16, 32, 64, 128}
    assert {c.combine for c in LC.CASES} == {"gate", "fixed", "annealing"} and {c.mask for c in LC.CASES} == {"structured", "dense_LL", "dense_L"}
    assert {c.pattern for c in LC.CASES} == {"all", "calibrated_read_row", "attacked_read_row_plus_mask", "calibrated_dense_plus_mask"}
    assert any(c.left_pad for c in LC.CASES) and any(not c.causal for c in LC.CASES) and any(c.p_drop == 0 for c in LC.CASES)
    assert all(c.two_level for c in LC.CASES)  # two_level = 0 is refused above 208 keys


@pytest.mark.parametrize("case", LC.CASES, ids=lambda c: c.id)
def test_fp32_oracle_is_a_usable_yardstick_on_every_long_case(case):
    pr = F.problem(case)
    draws = F.torch_draws(case)
    ref64 = F.oracle_grads(case, pr, draws, pr.cot, torch.float64)
    ref32 = F.oracle_grads(case, pr, draws, pr.cot, torch.float32)
    bad = []
    for n in F.leaf_names(case):
        e32 = F.err(ref32[n], ref64[n]) if ref64[n].abs().max() > 0 else ref32[n].abs().max().item()
        print(f"long_sequences_conditioning case={case.id} grad=d{n} e32={e32:.3e}")
        assert torch.isfinite(ref64[n]).all() and torch.isfinite(ref32[n]).all(), n
        if n in F.TENSOR_GRADS and not e32 <= F.E32_PRECONDITION:
            bad.append(f"d{n}: e32 = {e32:.3e}")
    assert not bad, f"{case.id}: the fp32 oracle is off by more than {F.E32_PRECONDITION:.0e}: " + "; ".join(bad)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _fake_problem(L, two_level=1):
    """A problem whose pointers are never dereferenced: every call below returns before the first HIP call."""
    p = _lib.Problem()
    p.B, p.L, p.H, p.n_heads = 2, L, 64, 2
    fake = C.c_void_p(0x1000)
    p.q = p.k = p.v = p.qa = p.ka = p.gate_logits = p.key_valid = fake
    p.w_order = p.b_order = p.w_dist = p.b_dist = p.scalar = fake
    p.mask_mode, p.causal, p.adversarial, p.combine_option = _lib.MASK_STRUCTURED, 1, 1, _lib.COMBINE["gate"]
    p.two_level, p.rng_mode, p.p_drop = two_level, _lib.RNG_COUNTER, 0.5
    if not two_level:
        p.rich_combine = _lib.RICH["fixed"]
    return p


def test_the_ceiling_and_the_refusals_need_no_gpu(lib):
    assert lib.acattn_max_sequence_length() == 496
    err = lambda: lib.acattn_last_error().decode()
    p, o = _lib.Problem(), _lib.FwdOut()
    p.B, p.L, p.H, p.n_heads = 2, 496, 64, 2
    assert lib.acattn_calibrated_attention_fwd(C.byref(p), C.byref(o), None) < 0 and "non-NULL" in err()  # past the length check
    p.L = 497
    assert lib.acattn_calibrated_attention_fwd(C.byref(p), C.byref(o), None) < 0 and "sequence length" in err() and "496" in err()
    fake = C.c_void_p(0x1000)
    o.ctx_calibrated = o.ctx_attacked = o.attack_mask = fake
    assert lib.acattn_calibrated_attention_fwd(C.byref(_fake_problem(209, two_level=0)), C.byref(o), None) < 0 and "two_level" in err()
    o.after_spatial = fake
    assert lib.acattn_calibrated_attention_fwd(C.byref(_fake_problem(209)), C.byref(o), None) < 0 and "probability dumps" in err()
    o.after_spatial = None
    hot = _fake_problem(209)
    hot.p_drop = 0.96  # the calibrated soft-max's fixed shift would overflow from 0.967 on
    assert lib.acattn_calibrated_attention_fwd(C.byref(hot), C.byref(o), None) < 0 and "p_drop above 0.95" in err()
    # a kernel that holds a whole row, pinned at L > 208
    assert lib.acattn_select_forward_kernel(_lib.FWD_STREAM) == _lib.FWD_AUTO
    try:
        assert lib.acattn_calibrated_attention_fwd(C.byref(_fake_problem(209)), C.byref(o), None) < 0 and "ACATTN_FWD_LONG" in err()
    finally:
        assert lib.acattn_select_forward_kernel(_lib.FWD_AUTO) == _lib.FWD_STREAM
    assert lib.acattn_select_forward_kernel(_lib.FWD_LONG) == _lib.FWD_AUTO and lib.acattn_select_forward_kernel(_lib.FWD_AUTO) == _lib.FWD_LONG
    assert lib.acattn_select_backward_kernel(_lib.BWD_LONG) == _lib.BWD_AUTO and lib.acattn_select_backward_kernel(_lib.BWD_AUTO) == _lib.BWD_LONG
    # backward: NULL workspace, a second cotangent set, dgate_summed
    io = _lib.BwdIO()
    for f in ("attack_mask", "row_stats", "dq", "dk", "dv", "dqa", "dka", "dgate_logits", "dw_order_part", "dw_dist_part", "dsmall_part"):
        setattr(io, f, fake)
    pb = _fake_problem(209)
    assert lib.acattn_calibrated_attention_bwd(C.byref(pb), C.byref(io), None) < 0 and "workspace" in err()
    io.workspace = fake
    io.dqa2 = io.dka2 = io.d_ctx_calibrated2 = fake
    assert lib.acattn_calibrated_attention_bwd_pair_supported(C.byref(pb), C.byref(io)) == 0
    assert lib.acattn_calibrated_attention_bwd(C.byref(pb), C.byref(io), None) < 0 and "second cotangent set" in err()
    io.dqa2 = io.dka2 = io.d_ctx_calibrated2 = None
    io.dgate_summed = 1
    assert lib.acattn_calibrated_attention_bwd_gate_summed(C.byref(pb), C.byref(io)) == 0
    assert lib.acattn_calibrated_attention_bwd(C.byref(pb), C.byref(io), None) < 0 and "dgate_summed" in err()
    assert lib.acattn_calibrated_attention_bwd_workspace_bytes(C.byref(pb)) == 2 * 2 * 209 * 16 * 4  # 16 floats per (sequence, head, row)
    # ... and 8 wherever the streaming pair runs: nothing moves at L <= 208 unless the long form is pinned
    p208 = _fake_problem(208)
    assert lib.acattn_calibrated_attention_bwd_workspace_bytes(C.byref(p208)) == 2 * 2 * 208 * 8 * 4
    lib.acattn_select_backward_kernel(_lib.BWD_LONG)
    try:
        assert lib.acattn_calibrated_attention_bwd_workspace_bytes(C.byref(p208)) == 2 * 2 * 208 * 16 * 4
    finally:
        lib.acattn_select_backward_kernel(_lib.BWD_AUTO)
    # the spatial-only backward stays at L <= 208, with a text of its own
    ps, sio = _fake_problem(209), _lib.SpatialBwdIO()
    ps.adversarial = 0
    assert lib.acattn_spatial_attention_bwd(C.byref(ps), C.byref(sio), None) < 0 and "spatial-only backward" in err() and "208" in err()


def test_python_refuses_a_sequence_beyond_the_ceiling_early():
    from ac_tsr_amd import attn_launch
    attn_launch.check_sequence_length(496)
    with pytest.raises(ValueError, match="496"):
        attn_launch.check_sequence_length(497)


def test_long_kernels_keep_nothing_in_scratch():
    """Spilling builds of the attention kernels have produced wrong tiles before (tests/test_abi_cpu.py): every kernel of the
    long family must have zero spilled registers and zero private segment, from the code objects' own metadata."""
    from tools import kernel_resources as KR
    if not (shutil.which("objcopy") and os.path.exists(os.path.join(KR.LLVM, "clang-offload-bundler"))
            and os.path.exists(os.path.join(KR.LLVM, "llvm-readelf"))):
        pytest.skip("no binutils / ROCm LLVM tools here")
    objs = sorted(glob.glob(os.path.join(KR.ROOT, "ac_tsr_amd", "csrc", "acattn_long_*_dh*.o")))
    if not objs:
        pytest.skip("objects not built in-tree (library built elsewhere)")
    n, bad = 0, []
    for o in objs:
        for k in KR.code_object_kernels(o):
            n += 1
            if k.get("vgpr_spill_count", 0) or k.get("sgpr_spill_count", 0) or k.get("private_segment_fixed_size", 0):
                bad.append((os.path.basename(o), k["name"], k.get("vgpr_spill_count", 0), k.get("sgpr_spill_count", 0),
                            k.get("private_segment_fixed_size", 0)))
    assert n == 16, n  # 4 head sizes x (forward with / without the adversarial calibrator, backward row + key kernel)
    assert not bad, bad
