"""GPU suite (-m gpu): acattn_full_sort_rank / acattn_full_sort_rank_exclude through the C ABI against float64.

A rank is a count of fp32 comparisons, so it is held to the float64 INTERVAL of tests/_rank_cases.py (the ranks every
correct fp32 evaluation can give; tests/test_rank_cases_cpu.py shows the intervals of the case table are single points but
for at most 5 % of a case's rows) and the target's score to its bound delta_bt = 2 (H + 4) 2^-24 sum_k |x_bk w_tk|.
Outputs lie between guards and start as poison, the workspace between guards and starts as garbage, inputs are followed
by NaN / out-of-range guards (tests/_guarded.py); every launch sequence runs twice and must give the same bits.  int32
ranks live in an fp32 guarded buffer viewed as int32: no rank's bit pattern is a NaN, the poison's is.
"""
import ctypes as C

import pytest
import torch

from ac_tsr_amd import _lib
from ac_tsr_amd import rank as R
from tests import _rank_cases as RC
from tests._guarded import check_all, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, I64 = torch.float32, torch.int64


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _launch(out, table, target, first_item, pairs=None, nan_score_rows=()):
    """acattn_full_sort_rank (+ _exclude for `pairs` = (rows, items) int64) twice on fresh guarded buffers.
    Returns (rank int64 [B], target_score fp32 [B]) on the CPU."""
    lib = _lib.load()
    B, H = out.shape
    N = table.shape[0]
    results = []
    for _ in range(2):
        inp = {"out": guarded((B, H), F32, DEV, H, out), "table": guarded((N, H), F32, DEV, H, table),
               "target": guarded((B,), I64, DEV, 1, target)}
        if pairs is not None and pairs[0].numel():
            inp["pair_row"] = guarded(tuple(pairs[0].shape), I64, DEV, 1, pairs[0])
            inp["pair_item"] = guarded(tuple(pairs[1].shape), I64, DEV, 1, pairs[1])
        P = _lib.CeProblem()
        P.B, P.N, P.H = B, N, H
        P.out, P.table, P.target = inp["out"].ptr(), inp["table"].ptr(), inp["target"].ptr()
        nbytes = lib.acattn_full_sort_rank_workspace_bytes(C.byref(P))
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert nbytes == (4 * B + 255) // 256 * 256 + 4 * B * RC.n_waves(H, N, cus)
        outs = {"rank": guarded((B,), F32, DEV, 1, "poison"), "target_score": guarded((B,), F32, DEV, 1, "poison"),
                "workspace": guarded((nbytes,), torch.uint8, DEV, 4 * B, "scratch")}
        outs["workspace"].t.fill_(0xA5)  # starts as garbage: nothing in it may be read before it is written
        rc = lib.acattn_full_sort_rank(C.byref(P), first_item, outs["workspace"].ptr(), outs["rank"].ptr(),
                                       outs["target_score"].ptr(), _stream())
        assert rc == 0, lib.acattn_last_error().decode()
        if pairs is not None:
            n_pairs = pairs[0].numel()
            rc = lib.acattn_full_sort_rank_exclude(C.byref(P), first_item, inp["pair_row"].ptr() if n_pairs else None,
                                                   inp["pair_item"].ptr() if n_pairs else None, n_pairs,
                                                   outs["target_score"].ptr(), outs["rank"].ptr(), _stream())
            assert rc == 0, lib.acattn_last_error().decode()
        torch.cuda.synchronize()
        unwritten = None
        if len(nan_score_rows):  # the documented NaN target scores: the single exemption from "no NaN left in an output"
            m = torch.zeros(B, dtype=torch.bool)
            m[list(nan_score_rows)] = True
            unwritten = {"target_score": m}
        check_all({**inp, **outs}, unwritten)
        results.append((outs["rank"].t.view(torch.int32).cpu().clone(), outs["target_score"].t.cpu().clone()))
    (r1, s1), (r2, s2) = results
    assert torch.equal(r1, r2) and torch.equal(s1.view(torch.int32), s2.view(torch.int32)), "two launches, different bits"
    return r1.long(), s1


def _in_interval(rank, lo, hi, what=""):
    bad = (rank < lo) | (rank > hi)
    assert not bool(bad.any()), f"{what}: rows {torch.nonzero(bad).reshape(-1).tolist()[:8]}: rank {rank[bad][:8].tolist()} " \
                                f"outside [{lo[bad][:8].tolist()}, {hi[bad][:8].tolist()}]"


def _score_ok(score, s64, delta):
    err = (score.double() - s64).abs()
    print(f"target_score: max error {err.max().item():.3e}, smallest bound {delta.min().item():.3e}")
    assert bool((err <= delta).all()), f"target_score off by {(err - delta).max().item():.3e} beyond its bound"


@pytest.mark.parametrize("case_id", RC.CASE_IDS)
def test_rank_and_score_against_float64(case_id):
    d = RC.build(case_id)
    rank, score = _launch(d["out"], d["table"], d["target"], d["case"]["first_item"])
    print(f"{case_id}: ranks {rank.min().item()} .. {rank.max().item()}, open intervals {(d['hi'] > d['lo']).sum().item()}")
    _in_interval(rank, d["lo"], d["hi"], case_id)
    _score_ok(score, d["s_t"], d["delta_t"])


def _base(H, N=200, B=33, seed=5):
    g = torch.Generator().manual_seed(seed + H + N)
    out, table = torch.randn(B, H, generator=g), torch.randn(N, H, generator=g)
    target = torch.randint(1, N, (B,), generator=g)
    return out, table, target


def _surely_behind(out_row, n):
    """n table rows whose scores against out_row lie far below every score of a N(0, 1) table."""
    return (-8.0 * out_row / out_row.norm()).repeat(n, 1)


@pytest.mark.parametrize("H,N", [(64, 200), (128, 200), (256, 200), (64, 20001), (128, 20001)])
def test_exact_ties_are_not_counted(H, N):
    """The target's table row copied bit for bit into an item of a main tile and into an item of the ragged last tile: those
    copies score what the target scores -- formed by the pair launch -- to the last bit wherever the sweep forms them, so
    the rank is the rank with those two items out of the race."""
    out, table, target = _base(H, N, B=17)
    main_item, ragged_item = 16 * RC.pick_tiles(H, N) * 5 + 3, N - 1  # a middle tile of wave 5; the last, ragged tile
    assert (N - 1) // 16 * 16 + 15 >= N  # the last tile is ragged
    for b0 in (0, 9, 16):
        t = int(target[b0])
        assert t not in (main_item, ragged_item)
        without = table.clone()
        without[[main_item, ragged_item]] = _surely_behind(out[b0], 2)
        with_copies = table.clone()
        with_copies[[main_item, ragged_item]] = table[t]
        r0, s0 = _launch(out, without, target, 1)
        r1, s1 = _launch(out, with_copies, target, 1)
        assert int(r1[b0]) == int(r0[b0]), f"row {b0}: rank {int(r1[b0])} with the copies, {int(r0[b0])} without"
        assert torch.equal(s0.view(torch.int32)[b0], s1.view(torch.int32)[b0])
        # ... and the copies, as targets themselves, score the same bits and rank the same
        tgt2 = target.clone()
        tgt2[b0] = ragged_item
        r2, s2 = _launch(out, with_copies, tgt2, 1)
        assert int(r2[b0]) == int(r1[b0]) and torch.equal(s2.view(torch.int32)[b0], s1.view(torch.int32)[b0])


@pytest.mark.parametrize("H", [64, 128, 256])
def test_nan_table_row_is_ahead_of_everything(H):
    out, table, target = _base(H)
    B, N = out.shape[0], table.shape[0]
    j_nan, b_nan = 77, 5
    target[b_nan] = j_nan
    target[target == j_nan] = j_nan + 1
    target[b_nan] = j_nan
    s, delta = RC.scores64(out, table)
    gone = torch.zeros(B, N, dtype=torch.bool)
    gone[:, j_nan] = True
    lo, hi = RC.intervals(s, delta, torch.where(target == j_nan, torch.ones_like(target), target), 1, gone)
    poisoned = table.clone()
    poisoned[j_nan] = float("nan")
    rank, score = _launch(out, poisoned, target, 1, nan_score_rows=[b_nan])
    others = torch.arange(B) != b_nan
    _in_interval(rank[others], lo[others] + 1, hi[others] + 1, "NaN item")  # exactly one more than without the item
    assert int(rank[b_nan]) == 0 and bool(torch.isnan(score[b_nan]))
    assert not bool(torch.isnan(score[others]).any())


@pytest.mark.parametrize("H", [64, 128, 256])
@pytest.mark.parametrize("first_item", [0, 1])
def test_target_outside_the_admissible_items_gives_rank_zero(H, first_item):
    out, table, target = _base(H, N=65, B=17)
    N = table.shape[0]
    bad = {0: -1, 3: N, 4: N + 5, 8: 2 ** 40, 15: -2 ** 40, 16: 2 ** 31}
    if first_item == 1:
        bad[1] = 0
    ok_target = target.clone()
    for b, t in bad.items():
        target[b] = t
        ok_target[b] = 1
    s, delta = RC.scores64(out, table)
    lo, hi = RC.intervals(s, delta, ok_target, first_item)
    rank, score = _launch(out, table, target, first_item, nan_score_rows=list(bad))  # (guards checked inside)
    good = torch.ones(17, dtype=torch.bool)
    good[list(bad)] = False
    assert rank[~good].tolist() == [0] * len(bad) and bool(torch.isnan(score[~good]).all())
    _in_interval(rank[good], lo[good], hi[good], "valid rows")


@pytest.mark.parametrize("H", [64, 128, 256])
def test_history_exclusion(H):
    out, table, target = _base(H, N=200, B=33)
    B, N = out.shape[0], table.shape[0]
    s, delta = RC.scores64(out, table)
    g = torch.Generator().manual_seed(3 + H)
    key = torch.randperm(B * N, generator=g)[:150]  # unique pairs, more than two waves of the pair launch
    rows, items = key // N, key % N
    # the best items of some rows: pairs that were certainly counted as ahead
    top = torch.topk(s[:, 1:], 3, dim=1).indices + 1
    rows = torch.cat([rows, torch.arange(0, B, 4).repeat_interleave(3)])
    items = torch.cat([items, top[0:B:4].reshape(-1)])
    key = torch.unique(rows * N + items)
    rows, items = key // N, key % N
    gone = torch.zeros(B, N, dtype=torch.bool)
    gone[rows, items] = True
    gone[torch.arange(B), target] = False  # a pair naming the target is ignored
    lo, hi = RC.intervals(s, delta, target, 1, gone)
    lo0, hi0 = RC.intervals(s, delta, target, 1)
    assert int((lo0 - lo).sum()) >= 20  # the exclusion moves ranks
    rank, score = _launch(out, table, target, 1, pairs=(rows, items))
    _in_interval(rank, lo, hi, "history")
    _score_ok(score, s[torch.arange(B), target], delta[torch.arange(B), target])
    # pairs that change nothing: the target itself, the padding item, rows and items outside the problem
    rank0, _ = _launch(out, table, target, 1, pairs=(torch.zeros(0, dtype=I64), torch.zeros(0, dtype=I64)))
    _in_interval(rank0, lo0, hi0, "no pairs")
    nothing = (torch.tensor([0, 1, 2, B, -1, 3, 4]), torch.tensor([int(target[0]), 0, 0, 5, 5, N, -7]))
    rank1, _ = _launch(out, table, target, 1, pairs=nothing)
    assert torch.equal(rank1, rank0)
    # a duplicated pair goes through the Python wrapper, which makes the pairs unique
    dup = (torch.cat([rows, rows[:40]]), torch.cat([items, items[:40]]))
    got = R.full_sort_ranks(out.to(DEV), table.to(DEV), target.to(DEV), first_item=1, history_index=dup)
    assert got.rank.dtype == torch.int32 and torch.equal(got.rank.cpu().long(), rank)
    assert torch.equal(got.target_score.cpu().view(torch.int32), score.view(torch.int32))


def test_python_wrapper_n_items_and_poisoned_outputs(monkeypatch):
    """n_items < table rows (a mask-token row behind the items never takes part), outputs allocated through
    attn_launch.allocator (NaN-filled under ACATTN_POISON_OUTPUTS=1), first_item = 0."""
    from ac_tsr_amd import attn_launch
    monkeypatch.setattr(attn_launch, "POISON", True)
    out, table, target = _base(64, N=130, B=33)
    big = torch.cat([table, 50.0 * torch.ones(3, 64) * out[0].sign()])  # rows that would be ahead for row 0
    s, delta = RC.scores64(out, table)
    for first in (0, 1):
        lo, hi = RC.intervals(s, delta, target, first)
        got = R.full_sort_ranks(out.to(DEV), big.to(DEV), target.to(DEV), n_items=130, first_item=first)
        _in_interval(got.rank.cpu().long(), lo, hi, f"first_item {first}")
        assert not bool(torch.isnan(got.target_score).any())
    with pytest.raises(_lib.AcattnError):
        R.full_sort_ranks(torch.zeros(4, 96, device=DEV), torch.zeros(9, 96, device=DEV), torch.ones(4, dtype=I64, device=DEV))
