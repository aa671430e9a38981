"""CPU suite for the full-sort rank: the C ABI's validation (which returns before any HIP call) and the conditioning of the
GPU case table tests/_rank_cases.py -- the intervals the GPU tests hold the kernels to must contain torch's own fp32 ranks
and must (almost) all be single points, otherwise those tests would pin nothing."""
import ctypes as C

import pytest
import torch

from ac_tsr_amd import _lib
from ac_tsr_amd import rank as R
from tests import _rank_cases as RC


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _problem(B=4, N=100, H=64):
    p = _lib.CeProblem()
    p.B, p.N, p.H = B, N, H
    p.out = p.table = p.target = 0x1000  # never dereferenced: validation comes first, and every call below fails it
    return p


def test_abi_stays_34_and_supported_widths(lib):
    assert lib.acattn_abi_version() == 34 == _lib.ABI_VERSION
    for H in (64, 128, 256):
        assert lib.acattn_full_sort_rank_supported(H) == 1 and R.supported(H)
    for H in (0, 16, 32, 96, 192, 512):
        assert lib.acattn_full_sort_rank_supported(H) == 0 and not R.supported(H)


def test_validation_errors_without_gpu(lib):
    fake = C.c_void_p(0x1000)
    err = lambda: lib.acattn_last_error().decode()
    p = _problem(H=96)
    assert lib.acattn_full_sort_rank(C.byref(p), 1, fake, fake, fake, None) < 0 and "H must be 64, 128 or 256" in err()
    assert lib.acattn_full_sort_rank_workspace_bytes(C.byref(p)) < 0
    p = _problem()
    assert lib.acattn_full_sort_rank(C.byref(p), 1, fake, None, fake, None) < 0 and "rank, target_score must be non-NULL" in err()
    assert lib.acattn_full_sort_rank(C.byref(p), 1, fake, fake, None, None) < 0 and "non-NULL" in err()
    assert lib.acattn_full_sort_rank(C.byref(p), 1, None, fake, fake, None) < 0 and "workspace" in err()
    assert lib.acattn_full_sort_rank(C.byref(p), p.N, fake, fake, fake, None) < 0 and "first_item must lie in [0, N)" in err()
    assert lib.acattn_full_sort_rank(C.byref(p), -1, fake, fake, fake, None) < 0 and "first_item" in err()
    assert lib.acattn_full_sort_rank_exclude(C.byref(p), 1, None, None, 3, fake, fake, None) < 0
    assert "pair_row, pair_item must be non-NULL when n_pairs > 0" in err()
    assert lib.acattn_full_sort_rank_exclude(C.byref(p), 1, fake, fake, -1, fake, fake, None) < 0 and "n_pairs" in err()
    assert lib.acattn_full_sort_rank_exclude(C.byref(p), p.N, fake, fake, 3, fake, fake, None) < 0 and "first_item" in err()
    assert lib.acattn_full_sort_rank_exclude(C.byref(p), 1, fake, fake, 3, None, fake, None) < 0 and "non-NULL" in err()
    assert lib.acattn_full_sort_rank_exclude(C.byref(p), 1, None, None, 0, fake, fake, None) == 0  # nothing to launch
    for bad in (dict(B=0), dict(N=0)):
        q = _problem(**bad)
        assert lib.acattn_full_sort_rank(C.byref(q), 0, fake, fake, fake, None) < 0 and "B and N must be positive" in err()
        assert lib.acattn_full_sort_rank_workspace_bytes(C.byref(q)) < 0
    q = _problem()
    q.out = None
    assert lib.acattn_full_sort_rank(C.byref(q), 1, fake, fake, fake, None) < 0 and "out, table, target" in err()
    assert lib.acattn_full_sort_rank(None, 1, fake, fake, fake, None) < 0 and "NULL" in err()


def test_workspace_is_one_int_per_wave_and_row(lib):
    # the query touches no device when the CU count is already known; here it falls back to the MI355X's 256 CUs
    for H, N, B in ((64, 100000, 4096), (64, 3000, 17), (128, 100000, 33), (256, 65, 1)):
        p = _problem(B=B, N=N, H=H)
        got = lib.acattn_full_sort_rank_workspace_bytes(C.byref(p))
        assert got == (4 * B + 255) // 256 * 256 + 4 * B * RC.n_waves(H, N)
    p = _problem(B=4096, N=100000, H=64)
    assert lib.acattn_full_sort_rank_workspace_bytes(C.byref(p)) < 4 * 4096 * 100000 // 100  # 14.7 MB against 1.6 GB of scores


def test_cpu_tensors_fail_loudly():
    with pytest.raises(_lib.AcattnError):
        R.full_sort_ranks(torch.zeros(4, 64), torch.zeros(10, 64), torch.ones(4, dtype=torch.int64))


def test_unique_pairs():
    rows, items = R.unique_pairs((torch.tensor([3, 0, 3, 1]), torch.tensor([5, 2, 5, 99])), 10)
    assert rows.tolist() == [0, 3] and items.tolist() == [2, 5]  # the repeat and the item outside the table are gone


def test_case_table_covers_what_the_issue_asks_for():
    ids = set(RC.CASE_IDS)
    assert len(ids) == len(RC.CASES)
    for H in (64, 128, 256):
        for B in (1, 15, 16, 17, 33):
            assert any(c["H"] == H and c["B"] == B for c in RC.CASES)
        for N in (2, 16, 17, 63, 64, 65):
            assert any(c["H"] == H and c["N"] == N and c["first_item"] == f for c in RC.CASES for f in (0, 1))
        assert RC.pick_tiles(H, 64) == 1 and RC.wave_span(H, 64) * RC.NW == 64
    assert any(c["B"] == 4096 and c["N"] == 3000 for c in RC.CASES)
    assert {RC.pick_tiles(c["H"], c["N"]) for c in RC.CASES if c["H"] == 64} == {1, 2, 4, 6, 7}
    assert {RC.pick_tiles(c["H"], c["N"]) for c in RC.CASES if c["H"] == 128} == {1, 2, 3}
    kinds = set()
    for cid in RC.CASE_IDS:
        if "_B33_" in cid or "_B17_" in cid:
            kinds |= set(RC.build(cid)["kinds"])
    assert kinds >= {"first_item", "last_item", "span_first", "span_last", "ragged_tile", "argmax", "argmin", "random"}


@pytest.mark.parametrize("case_id", RC.CASE_IDS)
def test_case_is_conditioned(case_id):
    d = RC.build(case_id)
    c = d["case"]
    B, N, first = c["B"], c["N"], c["first_item"]
    tgt, lo, hi = d["target"], d["lo"], d["hi"]
    assert bool(((tgt >= first) & (tgt < N)).all())
    # torch's own fp32 product lies in every row's interval
    r32 = RC.torch_fp32_ranks(d["out"], d["table"], tgt, first)
    assert bool(((r32 >= lo) & (r32 <= hi)).all()), (r32 - lo).abs().max()
    open_rows = int((hi > lo).sum())
    assert open_rows <= 0.05 * B, f"{open_rows} of {B} rows have a non-degenerate interval"
    for b, kind in enumerate(d["kinds"]):
        if kind == "argmax":
            assert int(lo[b]) == 1 == int(hi[b])
        if kind == "argmin":
            assert int(lo[b]) == N - first == int(hi[b])
