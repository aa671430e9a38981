"""CPU suite: the C ABI of the personalised front end (acattn_embed_user_*, the front end of ACSSEPT: acssept.py:120-131) --
its symbols are declared, exported and bound, the ctypes mirror of its struct matches the C layout, and every argument error
returns before any HIP call.  Nothing is launched (there is no GPU here)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from ac_tsr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("acattn_embed_user_supported", "acattn_embed_user_layernorm_fwd", "acattn_embed_user_layernorm_bwd")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_new_symbols_are_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    declared = set(re.findall(r"\b(acattn_[a-z_]+)\s*\(", text))
    for n in NEW:
        assert n in declared, f"include/acattn.h does not declare {n}"
        assert hasattr(lib, n), f"libacattn.so does not export {n}"
        assert n in _lib.SYMBOLS, f"ctypes binding lacks {n}"
    assert "typedef struct acattn_embed_user_problem" in text
    assert lib.acattn_abi_version() == 34  # additions within ABI 34


def test_embed_user_struct_layout_matches_c(tmp_path):
    """sizeof / offsetof of acattn_embed_user_problem from a tiny C program against include/acattn.h, compared with ctypes
    (the method of tests/test_abi_cpu.py::test_ctypes_layout_matches_c)."""
    cname, cls = "acattn_embed_user_problem", _lib.EmbedUserProblem
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "acattn.h"', 'int main(void){',
             f'printf("{cname} %zu\\n", sizeof({cname}));']
    for fname, _ in cls._fields_:
        lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = dict(l.split() for l in out.strip().splitlines())
    assert int(got[cname]) == C.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, fname
    # the fields of acattn_embed_problem without hot_id_plus1, plus Di, n_user_rows, user, user_table
    old = [f for f, _ in _lib.EmbedProblem._fields_ if f != "hot_id_plus1"]
    assert sorted(f for f, _ in cls._fields_) == sorted(old + ["Di", "n_user_rows", "user", "user_table"])


def test_supported_shapes(lib):
    for H, Di in ((64, 32), (128, 64), (128, 96), (64, 16), (256, 128), (256, 4)):
        assert lib.acattn_embed_user_supported(H, Di) == 1, (H, Di)
    for H, Di in ((128, 66), (96, 32), (64, 0), (64, 64), (64, 68), (64, -4), (128, 2)):
        assert lib.acattn_embed_user_supported(H, Di) == 0, (H, Di)


def _valid_problem():
    """Every pointer non-NULL (the address of a host array: nothing is dereferenced before the checks are through)."""
    buf = (C.c_char * 64)()
    a = C.addressof(buf)
    p = _lib.EmbedUserProblem()
    p.rows, p.L, p.H, p.Di = 100, 50, 128, 64
    p.n_table_rows, p.n_user_rows = 10, 5
    p.idx = p.user = p.table = p.user_table = p.gamma = p.beta = a
    return p, buf


def test_validation_errors_without_gpu(lib):
    fwd = lambda p, y=None, stats=None: lib.acattn_embed_user_layernorm_fwd(C.byref(p), y, stats, None)
    bwd = lambda p, dy=None, stats=None: lib.acattn_embed_user_layernorm_bwd(C.byref(p), dy, stats, 0, 0, None, None, None, None,
                                                                             None, None)
    err = lambda: lib.acattn_last_error()
    assert lib.acattn_embed_user_layernorm_fwd(None, None, None, None) < 0 and b"NULL" in err()
    for H, Di in ((96, 32), (128, 66), (128, 128)):
        p, keep = _valid_problem()
        p.H, p.Di = H, Di
        assert fwd(p) < 0 and b"unsupported (H, Di)" in err()
        assert bwd(p) < 0 and b"unsupported (H, Di)" in err()
    p, keep = _valid_problem()
    p.rows = 101
    assert fwd(p) < 0 and b"multiple of L" in err()
    assert bwd(p) < 0 and b"multiple of L" in err()
    for field, text in (("idx", b"idx must be non-NULL"), ("user", b"user must be non-NULL"),
                        ("table", b"table and user_table must be non-NULL"),
                        ("user_table", b"table and user_table must be non-NULL"), ("gamma", b"gamma and beta"),
                        ("beta", b"gamma and beta")):
        p, keep = _valid_problem()
        setattr(p, field, None)
        assert fwd(p) < 0 and text in err(), field
        assert bwd(p) < 0 and text in err(), field
    p, keep = _valid_problem()
    p.n_user_rows = 0
    assert fwd(p) < 0 and b"n_user_rows" in err()
    p, keep = _valid_problem()
    p.p_drop = 1.0
    assert fwd(p) < 0 and b"p_drop" in err()
    p, keep = _valid_problem()
    assert fwd(p, None, C.addressof(keep)) < 0 and b"y must be non-NULL" in err()
    assert fwd(p, C.addressof(keep), None) < 0 and b"stats must be non-NULL" in err()
    assert bwd(p, None, C.addressof(keep)) < 0 and b"dy and stats" in err()


def test_wrapper_refuses_cpu_tensors_and_unsupported_splits(lib):
    import torch

    from ac_tsr_amd import fused_embed_user
    item, user, norm = torch.nn.Embedding(10, 32, padding_idx=0), torch.nn.Embedding(4, 32, padding_idx=0), torch.nn.LayerNorm(64)
    seq, uid = torch.ones(2, 5, dtype=torch.long), torch.ones(2, dtype=torch.long)
    with pytest.raises(_lib.AcattnError):  # no CPU fallback
        fused_embed_user.embed_user_layer_norm(seq, uid, item, user, None, norm, 0.0, False)
    with pytest.raises(_lib.AcattnError):  # 30 + 34: a lane would straddle the seam
        fused_embed_user.embed_user_layer_norm(seq, uid, torch.nn.Embedding(10, 30), torch.nn.Embedding(4, 34), None, norm, 0.0, False)
    assert fused_embed_user.supported(128, 64) and not fused_embed_user.supported(96, 32)
