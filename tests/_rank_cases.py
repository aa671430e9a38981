"""Case table of the full-sort rank tests and its float64 conditioning (plain torch on the CPU; shared by
tests/test_rank_cases_cpu.py and tests/test_hip_full_sort_rank.py).

A rank is a count of comparisons between fp32 scores, so a test can only pin it where the comparisons are decided beyond the
rounding of ANY correct fp32 evaluation.  For every case the scores are formed in float64 and every pair (row b, item j) gets
the bound

    delta_bj = 2 (H + 4) 2^-24 sum_k |x_bk w_jk|

-- the fp32 dot-product bound for any summation order, (H + 4) u sum|x w| up to second order, doubled; derived, not measured.
Item j is SURELY AHEAD of the target t if s64_j - s64_t > delta_bj + delta_bt, SURELY BEHIND if the difference is below the
negative of that, AMBIGUOUS otherwise; the row's admissible ranks are [1 + #sure, 1 + #sure + #ambiguous].

The inputs are conditioned so that (almost) every interval is degenerate -- at most 5 % of a case's rows may not be, which
for the small batches means none: out ~ N(0, 1), table ~ N(0, 1); targets at the positions a kernel can get wrong (first
admissible item, last item, first / last item of a wave's span, an item of the ragged last tile) have their table row moved
along the row's direction into the sparse upper tail of the row's scores, the row's arg-max and arg-min are tails by
themselves, and every other target is drawn at random among the admissible items until its interval is degenerate (the row's
best item if none is found: at 100,000 items hardly any mid-rank target is).  All of this uses float64 only.
"""
from __future__ import annotations

import functools

import torch

N_CUS = 256  # MI355X: the launcher's tile count depends on it (acattn_rank.hip: pick_tiles)
NW = 4       # waves per workgroup


def pick_tiles(H: int, N: int, n_cus: int = N_CUS) -> int:
    """16-item tiles per wave as acattn_rank.hip picks them."""
    per_tile = n_cus * NW * 16
    need = (N + per_tile - 1) // per_tile
    if H == 64:
        return 1 if need <= 1 else 2 if need <= 2 else 4 if need <= 4 else 6 if need <= 6 else 7
    if H == 128:
        return 1 if need <= 1 else 2 if need <= 2 else 3
    return 1


def wave_span(H: int, N: int) -> int:
    return 16 * pick_tiles(H, N)


def n_waves(H: int, N: int, n_cus: int = N_CUS) -> int:
    wg = NW * 16 * pick_tiles(H, N, n_cus)
    return (N + wg - 1) // wg * NW


def delta_scale(H: int) -> float:
    return 2.0 * (H + 4) * 2.0 ** -24


def scores64(out: torch.Tensor, table: torch.Tensor):
    """(s64 [B, N], delta [B, N]) of fp32 inputs."""
    s = out.double() @ table.double().T
    a = out.double().abs() @ table.double().abs().T
    return s, a * delta_scale(out.shape[1])


def intervals(s: torch.Tensor, delta: torch.Tensor, target: torch.Tensor, first_item: int, inadmissible=None):
    """(lo, hi) int64 [B]: the admissible ranks of `target` given float64 scores `s` and bounds `delta`; `inadmissible`:
    optional bool [B, N], pairs left out (history).  Targets must lie in [first_item, N)."""
    B, N = s.shape
    rows = torch.arange(B)
    s_t, d_t = s[rows, target], delta[rows, target]
    diff = s - s_t[:, None]
    thr = delta + d_t[:, None]
    live = torch.ones(B, N, dtype=torch.bool)
    live[:, :first_item] = False
    live[rows, target] = False
    if inadmissible is not None:
        live &= ~inadmissible
    sure = ((diff > thr) & live).sum(1)
    amb = ((diff.abs() <= thr) & live).sum(1)
    return 1 + sure, 1 + sure + amb


def _cases():
    cases = []
    small_n = (2, 16, 17, 63, 64, 65, 200, 3000)  # 63 / 64 / 65: below, at, above a workgroup's span at one tile per wave
    k = 0
    for H in (64, 128, 256):
        for B in (1, 15, 16, 17, 33):
            for N in small_n:
                cases.append(dict(H=H, B=B, N=N, first_item=k % 2, seed=1000 + k))
                k += 1
    cases.append(dict(H=64, B=4096, N=3000, first_item=1, seed=77))  # many row blocks
    # more than one tile per wave (2, 4, 6, 7 at hidden 64; 2, 3 at 128), >= 3 workgroups, a ragged last tile
    for H, N in ((64, 20001), (64, 40010), (64, 70003), (64, 100000), (128, 20001), (128, 100000), (256, 20001)):
        cases.append(dict(H=H, B=17, N=N, first_item=1, seed=2000 + N % 97 + H))
    for c in cases:
        c["id"] = f"H{c['H']}_B{c['B']}_N{c['N']}_f{c['first_item']}"
    return cases


CASES = _cases()
CASE_IDS = [c["id"] for c in CASES]


def special_items(H: int, N: int, first_item: int):
    """Target positions a sweep can get wrong, as (name, item); duplicates and inadmissible ones dropped."""
    span = wave_span(H, N)
    last_wave0 = (N - 1) // span * span          # first item of the last (possibly ragged) wave
    want = [("first_item", first_item), ("last_item", N - 1), ("span_first", span if span < N else last_wave0),
            ("span_last", span - 1 if span - 1 < N else N - 1), ("ragged_tile", (N - 1) // 16 * 16),
            ("span_first_last_wave", last_wave0)]
    seen, out = set(), []
    for name, j in want:
        if first_item <= j < N and j not in seen:
            seen.add(j)
            out.append((name, j))
    return out


@functools.lru_cache(maxsize=None)
def build(case_id: str):
    """The case's inputs and float64 facts, built once per process and never changed by the tests."""
    c = CASES[CASE_IDS.index(case_id)]
    H, B, N, first = c["H"], c["B"], c["N"], c["first_item"]
    gen = torch.Generator().manual_seed(c["seed"])
    out = torch.randn(B, H, generator=gen)
    table = torch.randn(N, H, generator=gen)
    target = torch.full((B,), -1, dtype=torch.int64)
    kinds = [""] * B
    specials = special_items(H, N, first)
    offset = c["seed"] % 7
    # rows 0 .. : the special positions (rotated by case so that a one-row case does not always get the same one), each with
    # its table row moved into the upper tail of ITS row's scores: table_j += (z |x| - x . table_j) x / |x|^2
    b = 0
    for q in range(len(specials)):
        if b >= B or N - first < 4:
            break
        name, j = specials[(q + offset) % len(specials)]
        x = out[b].double()
        z = 3.5 + 0.25 * q
        w = table[j].double()
        table[j] = (w + (z * x.norm() - x @ w) * x / (x @ x)).float()
        target[b], kinds[b] = j, name
        b += 1
    s, delta = scores64(out, table)
    adm = s.clone()
    adm[:, :first] = float("nan")
    for name, pick in (("argmax", lambda r: torch.nan_to_num(adm[r], nan=-float("inf")).argmax()),
                       ("argmin", lambda r: torch.nan_to_num(adm[r], nan=float("inf")).argmin())):
        if b < B:
            target[b], kinds[b] = int(pick(b)), name
            b += 1
    # the rest: random admissible targets, redrawn while the interval is not degenerate
    rest = torch.nonzero(target < 0).reshape(-1)
    if rest.numel():
        best = torch.nan_to_num(adm[rest], nan=-float("inf")).argmax(1)
        chosen = torch.full_like(best, -1)
        for _ in range(12):
            todo = torch.nonzero(chosen < 0).reshape(-1)
            if not todo.numel():
                break
            cand = torch.randint(first, N, (todo.numel(),), generator=gen)
            lo, hi = intervals(s[rest[todo]], delta[rest[todo]], cand, first)
            good = lo == hi
            chosen[todo[good]] = cand[good]
        chosen = torch.where(chosen < 0, best, chosen)
        target[rest] = chosen
        for r in rest.tolist():
            kinds[r] = "random"
    lo, hi = intervals(s, delta, target, first)
    rows = torch.arange(B)
    return dict(case=c, out=out, table=table, target=target, kinds=kinds, s64=s, delta=delta, lo=lo, hi=hi,
                s_t=s[rows, target], delta_t=delta[rows, target])


def torch_fp32_ranks(out, table, target, first_item):
    """Ranks counted from torch's own fp32 matmul on the CPU, with the library's order rule."""
    sc = out @ table.T
    s_t = sc[torch.arange(out.shape[0]), target]
    ahead = ~(sc <= s_t[:, None])
    ahead[:, :first_item] = False
    ahead[torch.arange(out.shape[0]), target] = False
    return 1 + ahead.sum(1)
