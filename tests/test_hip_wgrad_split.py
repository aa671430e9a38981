"""GPU suite (-m gpu): stage 1 of the weight gradients on split bf16 products (wgrad_split_partial_kernel,
csrc/acattn_linear.hip) against an fp64 product of the same operands and against the exact-fp32 kernel it
replaces by default.  acattn_linear_products(0) (or ACATTN_LINEAR_PRODUCTS=fp32) brings the fp32 kernel back.

The kernel works on 32-row slabs, four waves per workgroup, and loads 16 bytes per row: the row counts below end inside
a slab, on its edge, one past it, below the partial count and in a second workgroup; the widths are whole 64-blocks, a
ragged last block with dword-aligned rows on either side (50) and a 16-byte-aligned ragged one (200, 72).

Launches of fewer than 4096 rows stay on the fp32 kernel (use_split_wgrad: they measured slower on the split one), so
the small row counts check that path and the same slab edges are repeated above 4096 rows for the split kernel; launches
of more than 8 slabs per wave go back to the fp32 kernel as well, and one case pins each of the two borders."""
import functools

import pytest
import torch

from ac_tsr_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPLIT_MIN_ROWS = 4096  # kSplitMinRows of acattn_linear.hip
ROWS = (1, 31, 32, 33, 63, 65, 100, 1000) + tuple(SPLIT_MIN_ROWS + m for m in (0, 1, 31, 32, 33, 63, 65, 100, 1000))
WIDTHS = ((64, 64), (64, 50), (50, 64), (64, 256), (256, 64), (200, 72))


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@functools.lru_cache(maxsize=None)
def _case(M, K, N):
    """(x, dy, fp64 dW, fp64 db), made once per shape and shared (nobody writes to them)"""
    g = torch.Generator().manual_seed(M + K + N)
    x = torch.randn(M, K, generator=g)
    dy = torch.randn(M, N, generator=g)
    return x, dy, dy.double().t() @ x.double(), dy.double().sum(0)


def _within_fp64_tolerance(M, got, ref):
    # the tolerance formula of test_hip_linear.py::test_linear_wgrad_matches_fp64
    tol = 4e-6 * (M ** 0.5) + 1e-5
    err = (got.cpu().double() - ref).abs().max().item()
    bound = tol * max(1.0, ref.abs().max().item() / (M ** 0.5))
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("K,N", WIDTHS)
@pytest.mark.parametrize("bias", [True, False])
def test_split_wgrad_matches_fp64(lib, M, K, N, bias):
    assert lib.acattn_linear_products(-1) == 1
    x, dy, ref_w, ref_b = _case(M, K, N)
    dw, db = ops.linear_wgrad(x.to(DEV), dy.to(DEV), bias)
    assert dw.shape == (N, K)
    _within_fp64_tolerance(M, dw, ref_w)
    if bias:
        _within_fp64_tolerance(M, db, ref_b)
    else:
        assert db is None


@pytest.mark.parametrize("K,N", [(64, 64), (64, 50)])
def test_split_wgrad_is_as_accurate_as_the_fp32_kernel(lib, K, N):
    """M = 4096: enough rows that neither form's accumulated error is all zeros.  The rule of
    test_hip_ce.py::test_split_products_are_as_accurate_as_fp32_products: within twice the fp32 form's error plus one
    fp32 rounding (2e-7) of the largest reference element."""
    M = 4096
    x, dy, ref_w, ref_b = _case(M, K, N)
    xd, gd = x.to(DEV), dy.to(DEV)
    split_w, split_b = ops.linear_wgrad(xd, gd, True)
    old = lib.acattn_linear_products(0)
    try:
        fp32_w, fp32_b = ops.linear_wgrad(xd, gd, True)
    finally:
        lib.acattn_linear_products(old)
    for name, s, f, ref in (("dW", split_w, fp32_w, ref_w), ("db", split_b, fp32_b, ref_b)):
        e_split = (s.cpu().double() - ref).abs().max().item()
        e_fp32 = (f.cpu().double() - ref).abs().max().item()
        print(f"{name} K={K} N={N}: split {e_split:.3e} fp32 {e_fp32:.3e} max|ref| {ref.abs().max().item():.3e}")
        assert e_split <= 2.0 * e_fp32 + 2e-7 * ref.abs().max().item(), (name, e_split, e_fp32)
    # the switch really changes the arithmetic
    assert not torch.equal(split_w, fp32_w)


@pytest.mark.parametrize("M", [33, SPLIT_MIN_ROWS + 33])
@pytest.mark.parametrize("K,N", [(64, 64), (64, 50), (200, 72)])
def test_rows_past_the_end_contribute_nothing(M, K, N):
    """M rows (whole slabs and one row of the next) against the same rows followed by 31 zero rows.  33 and 64 rows both
    take one partial; 4129 and 4160 rows both take 32 (64 rows per workgroup would allow 64 and 65, one workgroup per CU
    asks for 32 or more, 128 rows per workgroup allow 32): the same sums in the same order on either kernel."""
    x, dy, ref_w, ref_b = _case(M, K, N)
    xp, gp = torch.zeros(M + 31, K), torch.zeros(M + 31, N)
    xp[:M], gp[:M] = x, dy
    dw, db = ops.linear_wgrad(x.to(DEV), dy.to(DEV), True)
    dwp, dbp = ops.linear_wgrad(xp.to(DEV), gp.to(DEV), True)
    for got in (dw, dwp):
        _within_fp64_tolerance(M, got, ref_w)
    for got in (db, dbp):
        _within_fp64_tolerance(M, got, ref_b)
    assert torch.equal(dw, dwp) and torch.equal(db, dbp)


@pytest.mark.parametrize("M,K,N,split", [(SPLIT_MIN_ROWS - 1, 64, 64, False), (SPLIT_MIN_ROWS, 64, 64, True),
                                         (16384, 256, 256, True), (16416, 256, 256, False), (25600, 256, 256, False)])
def test_short_and_long_launches_stay_on_the_fp32_kernel(lib, M, K, N, split):
    """The split kernel takes launches of at least 4096 rows and at most 8 slabs per wave over 1024 SIMDs (blocks x
    slabs <= 8192; 256 x 256 is 16 blocks: 512 slabs = 16384 rows).  Outside that range the default mode gives what
    acattn_linear_products(0) gives, bit for bit (the same kernel and partial count); inside it does not.  Both hold the
    fp64 bound."""
    x, dy, ref_w, ref_b = _case(M, K, N)
    xd, gd = x.to(DEV), dy.to(DEV)
    dw, db = ops.linear_wgrad(xd, gd, True)
    old = lib.acattn_linear_products(0)
    try:
        fw, fb = ops.linear_wgrad(xd, gd, True)
    finally:
        lib.acattn_linear_products(old)
    _within_fp64_tolerance(M, dw, ref_w)
    _within_fp64_tolerance(M, db, ref_b)
    assert torch.equal(dw, fw) == (not split)


def test_grouped_split_wgrad_equals_individual_calls():
    """One launch: three items on one x tensor, one on its own x, a 64 -> 256 item and a 64 -> 50 item; M ends inside a
    slab and spans several workgroups.  Tolerance of test_hip_linear.py::test_grouped_wgrad_equals_individual_calls."""
    g = torch.Generator().manual_seed(21)
    M = 4099
    r = lambda n: torch.randn(M, n, generator=g).to(DEV)
    x, y = r(64), r(64)
    items = [(x, r(64), True), (x, r(64), False), (x, r(64), True), (y, r(64), True), (y, r(256), True), (x, r(50), True)]
    got = ops.linear_wgrad_grouped(items)
    again = ops.linear_wgrad_grouped(items)
    assert len(got) == len(items)
    for (xi, gi, wb), (dw, db), (dw2, db2) in zip(items, got, again):
        rw, rb = ops.linear_wgrad(xi, gi, wb)
        # (the number of partials follows the group: same sums, different association)
        assert (dw - rw).abs().max() <= 2e-5 * rw.abs().max()
        assert (db is None) == (not wb) and (db is None or (db - rb).abs().max() <= 2e-5 * rb.abs().max())
        assert torch.equal(dw, dw2) and (db is None or torch.equal(db, db2))


@pytest.mark.parametrize("M,K,N", [(1000, 64, 64), (1000, 64, 50), (100, 200, 72)])
def test_fp32_mode_runs_the_fp32_kernel(lib, M, K, N):
    """acattn_linear_products(0): two calls are equal bit for bit and hold the fp64 bound; the mode is restored."""
    x, dy, ref_w, ref_b = _case(M, K, N)
    xd, gd = x.to(DEV), dy.to(DEV)
    old = lib.acattn_linear_products(0)
    try:
        assert lib.acattn_linear_products(-1) == 0
        a = ops.linear_wgrad(xd, gd, True)
        b = ops.linear_wgrad(xd, gd, True)
    finally:
        lib.acattn_linear_products(old)
    assert lib.acattn_linear_products(-1) == old
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    _within_fp64_tolerance(M, a[0], ref_w)
    _within_fp64_tolerance(M, a[1], ref_b)
