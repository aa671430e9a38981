"""GPU suite (-m gpu): acattn_linear_wgrad / acattn_linear_wgrad_grouped at their row-slab edges, dw and db between guards
and poisoned (tests/_guarded.py), the workspace between guards, x and dy behind a NaN back guard (a row read past the end
that reaches a sum turns it into NaN), every value against an fp64 product of the same operands.

Slabs, as tests/test_hip_wgrad_split.py names them (acattn_linear.hip): stage 1 works on 64 x 64 blocks of dw; the fp32
kernel walks 64-row slabs, the split (bf16 MFMA) kernel 32-row slabs with four waves per workgroup; launches below
kSplitMinRows = 4,096 rows stay on the fp32 kernel.  Hence M in {1, 63, 64, 65, 127, 128, 129} (fp32 kernel in either mode) and
4,096 + {0, 1, 31, 32, 33, 63, 65} (the split kernel in the default mode, the fp32 kernel under acattn_linear_products(0)).
(K, N): whole 64-blocks, a ragged last block with dword-aligned dy rows (50), a 16-byte-aligned ragged pair (200, 72), four
blocks along K (256).

Tolerance: the formula of tests/test_hip_linear.py::test_linear_wgrad_matches_fp64, which tests/test_hip_wgrad_split.py
applies to both kernels: |err| <= (4e-6 sqrt(M) + 1e-5) * max(1, max|ref| / sqrt(M)).
"""
import ctypes as C
import functools

import pytest
import torch

from ac_tsr_amd import _lib
from tests._guarded import check_all, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
SPLIT_MIN_ROWS = 4096
ROWS = (1, 63, 64, 65, 127, 128, 129) + tuple(SPLIT_MIN_ROWS + m for m in (0, 1, 31, 32, 33, 63, 65))
WIDTHS = ((64, 64), (64, 50), (200, 72), (256, 64))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture
def lib():
    lib = _lib.load()
    products = lib.acattn_linear_products(-1)
    yield lib
    lib.acattn_linear_products(products)


@functools.lru_cache(maxsize=None)
def _case(M, K, N):
    """(x, dy, fp64 dW, fp64 db), made once per shape and shared (nobody writes to them)."""
    g = torch.Generator().manual_seed(M + 7 * K + 13 * N)
    x, dy = torch.randn(M, K, generator=g), torch.randn(M, N, generator=g)
    return x, dy, dy.double().t() @ x.double(), dy.double().sum(0)


def _within(name, M, got, ref):
    tol = 4e-6 * (M ** 0.5) + 1e-5
    err = (got.cpu().double() - ref).abs().max().item()
    bound = tol * max(1.0, ref.abs().max().item() / (M ** 0.5))
    print(f"{name}: max error {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{name}: max error {err:.3e} > {bound:.3e}"


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("K,N", WIDTHS)
@pytest.mark.parametrize("mode", [1, 0], ids=["split", "fp32"])
def test_linear_wgrad(lib, M, K, N, mode):
    lib.acattn_linear_products(mode)
    x, dy, ref_w, ref_b = _case(M, K, N)
    for bias in (True, False):
        inp = {"x": guarded((M, K), F32, DEV, K, x), "dy": guarded((M, N), F32, DEV, N, dy)}
        out = {"dw": guarded((N, K), F32, DEV, K, "poison"), "db": guarded((N,), F32, DEV, 1, "poison") if bias else None,
               "workspace": guarded((int(lib.acattn_linear_wgrad_workspace_bytes(M, K, N)) // 4,), F32, DEV, 64, "scratch")}
        _lib.check(lib.acattn_linear_wgrad(inp["x"].ptr(), inp["dy"].ptr(), M, K, N, out["workspace"].ptr(), out["dw"].ptr(),
                                           out["db"].ptr() if bias else None, _stream()), "linear_wgrad")
        torch.cuda.synchronize()
        check_all(out)
        check_all(inp)
        _within("dw", M, out["dw"].t, ref_w)
        if bias:
            _within("db", M, out["db"].t, ref_b)


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("mode", [1, 0], ids=["split", "fp32"])
def test_linear_wgrad_grouped(lib, M, mode):
    """The four widths as ONE group (the two K = 64 items on one x tensor; one item without a bias gradient)."""
    lib.acattn_linear_products(mode)
    cases = [_case(M, K, N) for K, N in WIDTHS]
    n = len(WIDTHS)
    xs = [guarded(c[0].shape, F32, DEV, c[0].shape[1], c[0]) for c in cases]
    xs[1] = xs[0]  # (64, 64) and (64, 50) read the same x, like the projections of a layer
    shared_x = cases[0][0]
    dys = [guarded(c[1].shape, F32, DEV, c[1].shape[1], c[1]) for c in cases]
    dws = [guarded((N, K), F32, DEV, K, "poison") for K, N in WIDTHS]
    dbs = [guarded((N,), F32, DEV, 1, "poison") if i != 2 else None for i, (K, N) in enumerate(WIDTHS)]
    ws = guarded((sum(int(lib.acattn_linear_wgrad_workspace_bytes(M, K, N)) for K, N in WIDTHS) // 4,), F32, DEV, 64, "scratch")
    arr = lambda bufs: (C.c_void_p * n)(*(None if b is None else b.t.data_ptr() for b in bufs))
    Ks, Ns = (C.c_int32 * n)(*(K for K, _ in WIDTHS)), (C.c_int32 * n)(*(N for _, N in WIDTHS))
    _lib.check(lib.acattn_linear_wgrad_grouped(arr(xs), arr(dys), Ks, Ns, arr(dws), arr(dbs), n, M, ws.ptr(), _stream()),
               "linear_wgrad_grouped")
    torch.cuda.synchronize()
    ws.check("workspace")
    for i, (K, N) in enumerate(WIDTHS):
        for name, b in ((f"x[{i}]", xs[i]), (f"dy[{i}]", dys[i]), (f"dw[{i}]", dws[i]), (f"db[{i}]", dbs[i])):
            if b is not None:
                b.check(name)
        ref_w = cases[i][2] if i != 1 else cases[1][1].double().t() @ shared_x.double()
        _within(f"dw[{i}]", M, dws[i].t, ref_w)
        if dbs[i] is not None:
            _within(f"db[{i}]", M, dbs[i].t, cases[i][3])
