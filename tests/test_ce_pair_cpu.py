"""CPU suite: the paired cross-entropy forward's C ABI (acattn_full_sort_ce_fwd_pair*, acattn_attacked_loss_finish_rows_pair)
is declared, exported and bound, refuses bad arguments before any HIP call, and ce.PAIRED_FORWARD follows its environment
variable.  Nothing is launched."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from ac_tsr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("acattn_full_sort_ce_fwd_pair_workspace_bytes", "acattn_full_sort_ce_fwd_pair", "acattn_attacked_loss_finish_rows_pair")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_new_symbols_are_declared_exported_and_bound(lib):
    header = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", header), f"include/acattn.h does not declare {name}"
        assert hasattr(lib, name), f"libacattn.so does not export {name}"
        assert name in _lib.SYMBOLS, f"ctypes binding lacks {name}"


def test_abi_version_is_34_on_both_sides(lib):
    assert _lib.ABI_VERSION == 34 and lib.acattn_abi_version() == 34
    assert re.search(r"#define\s+ACATTN_ABI_VERSION\s+34\b", open(_lib.HEADER_PATH).read())


def _problem(B, N, H, out=0x1000, table=0x2000, target=0x3000):
    p = _lib.CeProblem()
    p.B, p.N, p.H, p.out, p.table, p.target = B, N, H, out, table, target
    return p


def test_bad_arguments_are_refused_before_any_hip_call(lib):
    """The addresses below are not device memory: every call must return on its argument checks."""
    pa, pc = _problem(8, 100000, 64), _problem(12, 100000, 64)
    ptr = 0x4000
    # NULL problems / pointers
    assert lib.acattn_full_sort_ce_fwd_pair_workspace_bytes(None, C.byref(pc)) < 0
    assert lib.acattn_full_sort_ce_fwd_pair_workspace_bytes(C.byref(pa), None) < 0
    assert lib.acattn_full_sort_ce_fwd_pair(None, C.byref(pc), ptr, ptr, ptr, ptr, ptr, ptr, None) < 0
    assert lib.acattn_full_sort_ce_fwd_pair(C.byref(pa), None, ptr, ptr, ptr, ptr, ptr, ptr, None) < 0
    for k in range(6):
        args = [ptr] * 6
        args[k] = None
        assert lib.acattn_full_sort_ce_fwd_pair(C.byref(pa), C.byref(pc), *args, None) == -1
        assert b"non-NULL" in lib.acattn_last_error()
    no_out = _problem(8, 100000, 64, out=None)
    assert lib.acattn_full_sort_ce_fwd_pair(C.byref(no_out), C.byref(pc), ptr, ptr, ptr, ptr, ptr, ptr, None) == -1
    assert lib.acattn_full_sort_ce_fwd_pair(C.byref(pa), C.byref(_problem(0, 100000, 64)), ptr, ptr, ptr, ptr, ptr, ptr, None) == -1
    # the two sets must share the table: sizes are a caller's mistake, another table of the same size means "not paired"
    other_n = _problem(12, 99999, 64)
    assert lib.acattn_full_sort_ce_fwd_pair(C.byref(pa), C.byref(other_n), ptr, ptr, ptr, ptr, ptr, ptr, None) == -1
    assert lib.acattn_full_sort_ce_fwd_pair_workspace_bytes(C.byref(pa), C.byref(other_n)) == -1
    other_table = _problem(12, 100000, 64, table=0x5000)
    assert lib.acattn_full_sort_ce_fwd_pair(C.byref(pa), C.byref(other_table), ptr, ptr, ptr, ptr, ptr, ptr, None) == -100
    assert lib.acattn_full_sort_ce_fwd_pair_workspace_bytes(C.byref(pa), C.byref(other_table)) == -100
    # hidden sizes other than 64 are never paired
    pa128, pc128 = _problem(8, 100000, 128), _problem(12, 100000, 128)
    assert lib.acattn_full_sort_ce_fwd_pair(C.byref(pa128), C.byref(pc128), ptr, ptr, ptr, ptr, ptr, ptr, None) == -100
    assert lib.acattn_full_sort_ce_fwd_pair_workspace_bytes(C.byref(pa128), C.byref(pc128)) == -100
    # the finishing launch with the second mean
    pens = (C.c_void_p * 2)(ptr, ptr)
    f = lib.acattn_attacked_loss_finish_rows_pair
    assert f(None, 4, pens, 2, 16, 0.03, ptr, None, 0, ptr, 4, ptr, None) < 0
    assert f(ptr, 4, pens, 2, 16, 0.03, ptr, None, 0, None, 4, ptr, None) < 0
    assert f(ptr, 4, pens, 2, 16, 0.03, ptr, None, 0, ptr, 4, None, None) < 0
    assert f(ptr, 4, pens, 2, 16, 0.03, ptr, None, 0, ptr, 0, ptr, None) < 0
    assert f(ptr, 4, pens, 2, 16, 0.03, ptr, None, 8, ptr, 4, ptr, None) < 0  # n_scale without scale_buf


@pytest.mark.parametrize("value,expect", [(None, True), ("1", True), ("0", False)])
def test_paired_forward_switch_follows_the_environment(value, expect):
    env = {k: v for k, v in os.environ.items() if k != "ACATTN_CE_PAIRED"}
    if value is not None:
        env["ACATTN_CE_PAIRED"] = value
    out = subprocess.run([sys.executable, "-c", "from ac_tsr_amd import ce; print(ce.PAIRED_FORWARD)"], cwd=ROOT, env=env,
                         capture_output=True, text=True, check=True).stdout.strip()
    assert out == str(expect)
