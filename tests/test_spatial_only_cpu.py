"""CPU suite of the spatial-only backward and the trainable spatial-only model (no GPU needed): the new C-ABI entry
points are declared, exported, bound and laid out as in C; they validate their arguments before any HIP call; the
dispatcher operator has a Meta kernel with one fixed output shape; the modules construct without the adversarial
calibrator and keep the state-dict keys; the new kernels use no scratch and spill nothing."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

from ac_tsr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("acattn_spatial_attention_bwd", "acattn_spatial_attention_bwd_workspace_bytes",
               "acattn_projections_qkv_fwd", "acattn_projections_qkv_supported")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_new_symbols_are_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    declared = set(re.findall(r"\b(acattn_[a-z_]+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert name in declared, f"include/acattn.h does not declare {name}"
        assert hasattr(lib, name), f"libacattn.so does not export {name}"
        assert name in _lib.SYMBOLS, f"ctypes binding lacks {name}"
    assert "typedef struct acattn_spatial_bwd_io" in text
    assert _lib.ABI_VERSION >= 32 and lib.acattn_abi_version() == _lib.ABI_VERSION


def test_spatial_bwd_io_layout_matches_c(tmp_path):
    """sizeof / offsetof of acattn_spatial_bwd_io from gcc against the ctypes mirror (the method of
    tests/test_abi_cpu.py::test_ctypes_layout_matches_c)."""
    cls, cname = _lib.SpatialBwdIO, "acattn_spatial_bwd_io"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "acattn.h"', 'int main(void){',
             f'printf("{cname} %zu\\n", sizeof({cname}));']
    for fname, _ in cls._fields_:
        lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    assert int(got[cname]) == C.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, fname
    # the C struct has no field the mirror lacks: the last field ends where the struct does (up to tail padding)
    last = cls._fields_[-1][0]
    assert getattr(cls, last).offset + getattr(cls, last).size > C.sizeof(cls) - 8


def _valid_problem():
    """A problem that passes validation without any device memory: the pointers are only tested for NULL."""
    p = _lib.Problem()
    p.B, p.L, p.H, p.n_heads = 2, 50, 64, 2
    p.q = p.k = p.v = p.key_valid = C.c_void_p(64)
    p.mask_mode, p.causal = _lib.MASK_STRUCTURED, 1
    p.w_order = p.b_order = p.w_dist = p.b_dist = p.scalar = C.c_void_p(64)
    p.rng_mode, p.p_drop, p.adversarial = _lib.RNG_COUNTER, 0.5, 0
    return p


def test_validation_without_a_device(lib):
    p, io = _valid_problem(), _lib.SpatialBwdIO()
    io.d_ctx = C.c_void_p(64)
    assert lib.acattn_spatial_attention_bwd(C.byref(p), C.byref(io), None) < 0  # dq, dk, dv are NULL
    assert b"non-NULL" in lib.acattn_last_error()
    assert lib.acattn_spatial_attention_bwd(C.byref(p), None, None) < 0
    p.adversarial = 1
    p.qa = p.ka = p.gate_logits = C.c_void_p(64)
    p.combine_option, p.two_level = _lib.COMBINE["gate"], 1
    assert lib.acattn_spatial_attention_bwd(C.byref(p), C.byref(io), None) < 0
    assert b"adversarial == 0" in lib.acattn_last_error()
    p = _valid_problem()
    p.L = 500
    assert lib.acattn_spatial_attention_bwd(C.byref(p), C.byref(io), None) < 0
    assert b"sequence length" in lib.acattn_last_error()
    p = _valid_problem()
    assert lib.acattn_spatial_attention_bwd_workspace_bytes(C.byref(p)) == 2 * 2 * 50 * 4 * 4  # four floats per (b, head, row)
    assert lib.acattn_spatial_attention_bwd_workspace_bytes(None) < 0
    # all outputs given but no workspace: still refused before any launch
    io.dq = io.dk = io.dv = io.dw_order_part = io.dw_dist_part = io.dsmall_part = C.c_void_p(64)
    assert lib.acattn_spatial_attention_bwd(C.byref(p), C.byref(io), None) < 0 and b"workspace" in lib.acattn_last_error()
    io.workspace, io.part_stride = C.c_void_p(64), 8
    assert lib.acattn_spatial_attention_bwd(C.byref(p), C.byref(io), None) < 0 and b"part_stride" in lib.acattn_last_error()
    # the adversarial entry point still refuses the spatial-only problem
    assert lib.acattn_calibrated_attention_bwd(C.byref(p), C.byref(_lib.BwdIO()), None) < 0
    assert b"adversarial (full) operator only" in lib.acattn_last_error()


def test_three_projection_entry_point_validates_without_a_device(lib):
    assert lib.acattn_projections_qkv_supported(128) == 0 and lib.acattn_projections_qkv_supported(96) == 0
    old = lib.acattn_linear_products(-1)
    try:
        lib.acattn_linear_products(1)
        assert lib.acattn_projections_qkv_supported(64) == 1
        pp, po = _lib.ProjProblem(), _lib.ProjOut()
        pp.rows, pp.H = 16, 64
        assert lib.acattn_projections_qkv_fwd(C.byref(pp), C.byref(po), None) < 0 and b"non-NULL" in lib.acattn_last_error()
        pp.x = pp.wq = pp.bq = pp.wk = pp.bk = pp.wv = pp.bv = C.c_void_p(64)
        po.mq = po.mk = po.mv = po.qa = C.c_void_p(64)
        assert lib.acattn_projections_qkv_fwd(C.byref(pp), C.byref(po), None) < 0 and b"must be NULL" in lib.acattn_last_error()
        lib.acattn_linear_products(0)  # exact-fp32 mode: the caller runs three plain linear layers
        assert lib.acattn_projections_qkv_supported(64) == 0
    finally:
        lib.acattn_linear_products(old)


def test_dispatcher_operator_is_registered_with_one_output_shape():
    from ac_tsr_amd import dispatch  # noqa: F401
    B, L, H, nh = 3, 50, 64, 2
    q = torch.empty(B, L, H, device="meta")
    kv = torch.empty(B, L, dtype=torch.uint8, device="meta")
    w, b1 = torch.empty(2 * H // nh, device="meta"), torch.empty(1, device="meta")
    want = [(B, L, H)] * 3 + [(B * nh, 4 * (H // nh) + 4)]
    outs = torch.ops.acattn.spatial_attention_bwd(q, q, q, kv, True, w, b1, w, b1, b1, nh, 0.5, 1, None, q, None)
    assert [tuple(t.shape) for t in outs] == want
    rows = torch.empty(B, 1, dtype=torch.int64, device="meta")  # the read-row hint changes no shape
    outs = torch.ops.acattn.spatial_attention_bwd(q, q, q, kv, False, w, b1, w, b1, b1, nh, 0.0, 1, None, q, rows)
    assert [tuple(t.shape) for t in outs] == want
    cpu = torch.zeros(B, L, H)
    with pytest.raises(Exception):  # no CPU kernel is registered: the dispatcher refuses
        torch.ops.acattn.spatial_attention_bwd(cpu, cpu, cpu, torch.ones(B, L, dtype=torch.uint8), True, torch.zeros(64),
                                               torch.zeros(1), torch.zeros(64), torch.zeros(1), torch.zeros(1), nh, 0.5, 1,
                                               None, cpu, None)


def _model_config(**extra):
    import ac_tsr_amd as A
    return A.DictConfig(n_layers=2, n_heads=2, hidden_size=64, inner_size=256, hidden_dropout_prob=0.5,
                        attn_dropout_prob=0.5, hidden_act='gelu', layer_norm_eps=1e-12, initializer_range=0.02,
                        loss_type='CE', combine_option='gate', two_level=True, use_order=True, use_distance=True,
                        rich_calibrated_combine='none', mask_loss_weight=0.03, use_position_embedding=True, **extra)


def test_modules_construct_without_the_adversarial_calibrator_and_keep_their_keys():
    import ac_tsr_amd as A
    from ac_tsr_amd.layers import AttackRTransformerEncoder, AttackRTransformerLayer
    kw = dict(n_layers=2, n_heads=2, hidden_size=64, inner_size=256, combine_option='gate', seq_length=50)
    full, spatial = AttackRTransformerEncoder(**kw), AttackRTransformerEncoder(**kw, adversarial=False)
    assert set(spatial.state_dict()) == set(full.state_dict())
    assert any("attack_query_transform" in k for k in spatial.state_dict()) and any(".gate." in k for k in spatial.state_dict())
    assert all(not l.adversarial for l in spatial.layer) and all(l.adversarial for l in full.layer)
    full.load_state_dict(spatial.state_dict(), strict=True)
    spatial.load_state_dict(full.state_dict(), strict=True)
    # the keyword comes AFTER the reference's positional arguments
    layer = AttackRTransformerLayer(2, 64, 256, 0.5, 0.5, 'gelu', 1e-12, 'gate', True, True, True, 'fixed', 50)
    assert layer.adversarial is True
    assert AttackRTransformerLayer(2, 64, 256, 0.5, 0.5, 'gelu', 1e-12, 'gate', adversarial=False)._config().adversarial is False

    m_full = A.ACSASRec(_model_config(), A.ItemCount(100))
    m_spat = A.ACSASRec(_model_config(adversarial_calibrator=False), A.ItemCount(100))
    assert m_full.adversarial_calibrator is True and m_spat.adversarial_calibrator is False
    assert set(m_spat.state_dict()) == set(m_full.state_dict())
    m_spat.load_state_dict(m_full.state_dict(), strict=True)
    # the probability dumps belong to the adversarial core
    x = torch.zeros(1, 50, 64)
    with pytest.raises(ValueError, match="probability"):
        spatial.layer[0](x, torch.zeros(1, 1, 50, 50), return_all_attention_prob=True)
    with pytest.raises(ValueError, match="probability"):
        spatial(x, torch.zeros(1, 1, 50, 50), return_attention_prob=True)


def test_out_of_scope_combinations_are_refused_with_a_message():
    import ac_tsr_amd as A
    with pytest.raises(NotImplementedError, match="ACSASRec only"):
        A.AcBERT4Rec(_model_config(adversarial_calibrator=False, mask_ratio=0.2), A.ItemCount(100))
    m = A.ACSASRec(_model_config(adversarial_calibrator=False), A.ItemCount(100))
    with pytest.raises(ValueError, match="combined_backward"):
        A.AttackSASRecTrainer(None, m, combined_backward=True)


def _spatial_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    if not (shutil.which("objcopy") and os.path.exists(os.path.join(KR.LLVM, "clang-offload-bundler"))):
        pytest.skip("no binutils / ROCm LLVM tools here")
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    ks = KR.code_object_kernels(_lib.LIB_PATH)
    names = KR.demangle([k["name"] for k in ks])
    return [(names[k["name"]].replace("(anonymous namespace)::", "").split("(")[0], k) for k in ks
            if "acattn_spatial_bwd" in k["name"]]


def test_spatial_backward_kernels_use_no_scratch_and_spill_nothing():
    """Every instantiation of the two kernels (four head sizes x training / general form), read from the built library's
    code-object metadata: 0 spilled vector registers, 0 spilled scalar registers, 0 bytes of scratch."""
    ks = _spatial_kernels()
    assert len(ks) == 16, [n for n, _ in ks]
    for dh in (16, 32, 64, 128):
        for kind in ("row", "key"):
            assert sum(1 for n, _ in ks if f"acattn_spatial_bwd_{kind}_kernel<{dh}," in n) == 2, (dh, kind)
    for name, k in ks:
        assert k.get("vgpr_spill_count", 0) == 0, name
        assert k.get("sgpr_spill_count", 0) == 0, name
        assert k.get("private_segment_fixed_size", 0) == 0, name


def test_committed_resource_table_is_the_built_kernels():
    """profiles/spatial_bwd_kernel_resources.txt lists every instantiation, with zero spills and zero scratch."""
    path = os.path.join(ROOT, "profiles", "spatial_bwd_kernel_resources.txt")
    rows = [l.split(None, 6) for l in open(path) if "acattn_spatial_bwd" in l]
    assert len(rows) == 16
    assert {r[6].strip().replace("void ", "") for r in rows} == {n.replace("void ", "") for n, _ in _spatial_kernels()}
    for r in rows:
        assert (int(r[2]), int(r[3]), int(r[4])) == (0, 0, 0), r
