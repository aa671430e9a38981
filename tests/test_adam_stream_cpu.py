"""CPU suite: the persistent Adam launch's C ABI (acattn_adam_step_cached, acattn_select_adam_grid) is declared, exported
and bound, refuses bad arguments before any HIP call, the binding's cache size is the header's, and optim.STREAM_KERNEL
follows its environment variable.  Nothing is launched."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from ac_tsr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_new_symbols_are_declared_exported_and_bound(lib):
    header = open(_lib.HEADER_PATH).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("acattn_adam_step_cached", "acattn_select_adam_grid"):
        assert re.search(r"\b" + name + r"\s*\(", code) and hasattr(lib, name) and name in _lib.SYMBOLS, name
    assert lib.acattn_abi_version() == _lib.ABI_VERSION
    m = re.search(r"#define\s+ACATTN_ADAM_CACHE_BYTES\s+\((\d+)\s*\*\s*ACATTN_ADAM_MAX_TENSORS\)", header)
    assert m and int(m.group(1)) * _lib.ADAM_MAX_TENSORS == _lib.ADAM_CACHE_BYTES


def test_bad_arguments_are_refused_before_any_hip_call(lib):
    """The addresses below are not device memory: every call must return on its argument checks."""
    ptr = 0x4000
    g = _lib.AdamGroup()
    g.n_tensors = 1
    g.param[0] = g.grad[0] = g.exp_avg[0] = g.exp_avg_sq[0] = g.step[0] = ptr
    g.numel[0] = 10
    f = lib.acattn_adam_step_cached
    assert f(None, 1e-3, 0.9, 0.999, 1e-8, 0.0, ptr, ptr, None) < 0
    assert f(C.byref(g), 1e-3, 0.9, 0.999, 1e-8, 0.0, None, ptr, None) < 0
    assert f(C.byref(g), 1e-3, 0.9, 0.999, 1e-8, 0.0, ptr, None, None) < 0 and b"non-NULL" in lib.acattn_last_error()
    assert f(C.byref(g), 1e-3, 0.9, 0.999, 1e-8, 0.0, ptr, ptr + 8, None) < 0 and b"aligned" in lib.acattn_last_error()
    assert f(C.byref(g), 1e-3, 1.0, 0.999, 1e-8, 0.0, ptr, ptr, None) < 0 and b"betas" in lib.acattn_last_error()
    g.numel[0] = 0
    assert f(C.byref(g), 1e-3, 0.9, 0.999, 1e-8, 0.0, ptr, ptr, None) < 0
    g.numel[0], g.step[0] = 10, None
    assert f(C.byref(g), 1e-3, 0.9, 0.999, 1e-8, 0.0, ptr, ptr, None) < 0
    g.n_tensors = _lib.ADAM_MAX_TENSORS + 1
    assert f(C.byref(g), 1e-3, 0.9, 0.999, 1e-8, 0.0, ptr, ptr, None) < 0
    # the grid hook: returns the previous setting, refuses a negative count
    old = lib.acattn_select_adam_grid(3)
    assert lib.acattn_select_adam_grid(old) == 3
    assert lib.acattn_select_adam_grid(-1) < 0 and lib.acattn_select_adam_grid(old) == old


@pytest.mark.parametrize("value,expect", [(None, True), ("stream", True), ("chunk", False)])
def test_kernel_switch_follows_the_environment(value, expect):
    env = {k: v for k, v in os.environ.items() if k != "ACATTN_ADAM_KERNEL"}
    if value is not None:
        env["ACATTN_ADAM_KERNEL"] = value
    out = subprocess.run([sys.executable, "-c", "from ac_tsr_amd import optim; print(optim.STREAM_KERNEL)"], cwd=ROOT, env=env,
                         capture_output=True, text=True, check=True).stdout.strip()
    assert out == str(expect)
