"""GPU suite (-m gpu): the full-catalogue cross-entropy (acattn_full_sort_ce_fwd / _fwd_dir / _fwd_pair / _bwd) at its
row-block and item-tile edges, every output between guards and poisoned (tests/_guarded.py), the workspace between guards,
the rows and targets behind NaN / out-of-range back guards, every value against materialised logits in fp64.

Edges (acattn_ce.hip, acattn_ce_bf16.hip): rows are taken in blocks of 32 (B in {1, 31, 32, 33}: a ragged only block, a full
one, one row into a second); the catalogue is swept in tiles of 64 items (N in {64, 257, 449}: one whole tile, a last tile of
one item, a ragged last tile of seven tiles -- more than the six a split-product wave takes).  Products modes
ACATTN_CE_PRODUCTS_FP32 (0) and ACATTN_CE_PRODUCTS_ALL (2: the split sweeps at every catalogue size); the paired forward
exists on the split sweeps only (-100 under mode 0, which the test asserts).

d_table is poisoned: include/acattn.h, acattn_full_sort_ce_bwd: "d_table [N,H] (fully overwritten) unless NULL".

Tolerances are those of tests/test_hip_ce.py: lse and row losses 1e-5 * max(1, |.|), gradients (dir, d_out, d_table) 1e-4 of
the tensor's largest magnitude + 1e-9.
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
H = 64


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture
def lib():
    lib = _lib.load()
    products = lib.acattn_full_sort_ce_products(-1)
    yield lib
    lib.acattn_full_sort_ce_products(products)


@functools.lru_cache(maxsize=None)
def _case(B, N, seed=0):
    """Rows, table, targets (the last item is one), row weights, and the fp64 reference of everything the launches write."""
    g = torch.Generator().manual_seed(B + 1000 * N + seed)
    out, table = torch.randn(B, H, generator=g), torch.randn(N, H, generator=g)
    target = torch.randint(0, N, (B,), generator=g)
    target[-1] = N - 1
    coef = torch.randn(B, generator=g)
    od, td = out.double(), table.double()
    logits = od @ td.t()
    lse = torch.logsumexp(logits, 1)
    row_loss = lse - logits.gather(1, target[:, None])[:, 0]
    p = torch.exp(logits - lse[:, None])
    p[torch.arange(B), target] -= 1.0           # d row_loss / d logits
    direction = p @ td                          # d row_loss / d out
    ref = {"lse": lse, "row_loss": row_loss, "dir": direction, "d_out": coef.double()[:, None] * direction,
           "d_table": (coef.double()[:, None] * p).t() @ od}
    return {"B": B, "N": N, "out": out, "table": table, "target": target, "coef": coef}, ref


def _inputs(c):
    return {"out": guarded((c["B"], H), F32, DEV, H, c["out"]), "target": guarded((c["B"],), torch.int64, DEV, 1, c["target"]),
            "coef": guarded((c["B"],), F32, DEV, 1, c["coef"])}


def _problem(c, inp, table):
    P = _lib.CeProblem()
    P.B, P.N, P.H = c["B"], c["N"], H
    P.out, P.table, P.target = inp["out"].ptr(), table.data_ptr(), inp["target"].ptr()
    return P


def _close(name, got, want, tol_abs, tol_rel=0.0):
    err = (got.detach().cpu().double() - want).abs().max().item()
    bound = tol_abs + tol_rel * want.abs().max().item()
    print(f"{name}: max error {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{name}: max error {err:.3e} > {bound:.3e}"


def _check_values(out, ref):
    for k, g in out.items():
        if k in ("lse", "row_loss"):
            _close(k, g.t, ref[k], 1e-5 * max(1.0, ref[k].abs().max().item()))
        elif k in ("dir", "d_out", "d_table"):
            _close(k, g.t, ref[k], 1e-9, 1e-4)


def _workspace(nbytes):
    assert nbytes >= 0
    return guarded((max(int(nbytes), 16),), torch.uint8, DEV, 64, "scratch")


@pytest.mark.parametrize("B", [1, 31, 32, 33])
@pytest.mark.parametrize("N", [64, 257, 449])
@pytest.mark.parametrize("mode", [0, 2], ids=["fp32", "split"])
def test_full_sort_ce(lib, B, N, mode):
    lib.acattn_full_sort_ce_products(mode)
    c, ref = _case(B, N)
    inp, table = _inputs(c), c["table"].to(DEV)
    P = _problem(c, inp, table)
    nbytes = lib.acattn_full_sort_ce_workspace_bytes(C.byref(P))
    # forward
    out = {"lse": guarded((B,), F32, DEV, 1, "poison"), "row_loss": guarded((B,), F32, DEV, 1, "poison"), "workspace": _workspace(nbytes)}
    _lib.check(lib.acattn_full_sort_ce_fwd(C.byref(P), out["workspace"].ptr(), out["lse"].ptr(), out["row_loss"].ptr(), _stream()),
               "full_sort_ce_fwd")
    torch.cuda.synchronize()
    check_all(out)
    check_all(inp)
    _check_values(out, ref)
    # forward with the direction
    out = {"lse": guarded((B,), F32, DEV, 1, "poison"), "row_loss": guarded((B,), F32, DEV, 1, "poison"),
           "dir": guarded((B, H), F32, DEV, H, "poison"), "workspace": _workspace(nbytes)}
    _lib.check(lib.acattn_full_sort_ce_fwd_dir(C.byref(P), out["workspace"].ptr(), out["lse"].ptr(), out["row_loss"].ptr(),
                                               out["dir"].ptr(), _stream()), "full_sort_ce_fwd_dir")
    torch.cuda.synchronize()
    check_all(out)
    check_all(inp)
    _check_values(out, ref)
    # backward: with the table gradient, and without it (d_table == NULL)
    inp["lse"] = guarded((B,), F32, DEV, 1, ref["lse"].float())
    for with_table in (True, False):
        out = {"d_out": guarded((B, H), F32, DEV, H, "poison"), "d_table": guarded((N, H), F32, DEV, H, "poison") if with_table else None,
               "workspace": _workspace(nbytes)}
        _lib.check(lib.acattn_full_sort_ce_bwd(C.byref(P), inp["lse"].ptr(), inp["coef"].ptr(), out["workspace"].ptr(), out["d_out"].ptr(),
                                               out["d_table"].ptr() if with_table else None, _stream()), "full_sort_ce_bwd")
        torch.cuda.synchronize()
        check_all(out)
        check_all(inp)
        _check_values({k: v for k, v in out.items() if v is not None}, ref)


@pytest.mark.parametrize("B,N", [(33, 257), (1, 64)])
@pytest.mark.parametrize("mode", [0, 2], ids=["fp32", "split"])
def test_full_sort_ce_bwd_scalar_coef(lib, B, N, mode):
    """coef_is_scalar: coef[0] * coef_scale holds for every row (the cotangent of a mean)."""
    lib.acattn_full_sort_ce_products(mode)
    c, ref = _case(B, N)
    inp, table = _inputs(c), c["table"].to(DEV)
    inp["lse"] = guarded((B,), F32, DEV, 1, ref["lse"].float())
    inp["coef"] = guarded((1,), F32, DEV, 1, c["coef"][:1].clone())
    P = _problem(c, inp, table)
    P.coef_is_scalar, P.coef_scale = 1, 1.0 / B
    out = {"d_out": guarded((B, H), F32, DEV, H, "poison"), "d_table": guarded((N, H), F32, DEV, H, "poison"),
           "workspace": _workspace(lib.acattn_full_sort_ce_workspace_bytes(C.byref(P)))}
    _lib.check(lib.acattn_full_sort_ce_bwd(C.byref(P), inp["lse"].ptr(), inp["coef"].ptr(), out["workspace"].ptr(), out["d_out"].ptr(),
                                           out["d_table"].ptr(), _stream()), "full_sort_ce_bwd")
    torch.cuda.synchronize()
    check_all(out)
    check_all(inp)
    k = c["coef"][0].double() / B
    od, td = c["out"].double(), c["table"].double()
    p = torch.softmax(od @ td.t(), 1)
    p[torch.arange(B), c["target"]] -= 1.0
    _close("d_out", out["d_out"].t, k * ref["dir"], 1e-9, 1e-4)
    _close("d_table", out["d_table"].t, k * (p.t() @ od), 1e-9, 1e-4)


@pytest.mark.parametrize("B_a,B_c", [(1, 1), (31, 33), (32, 32), (33, 1)])
@pytest.mark.parametrize("N", [64, 257, 449])
def test_full_sort_ce_fwd_pair(lib, B_a, B_c, N):
    """Two row sets over one sweep of the table: set a gets lse, row loss and direction, set c lse and row loss."""
    (ca, ra), (cc, _) = _case(B_a, N), _case(B_c, N, seed=5)
    table = ca["table"].to(DEV)
    od = cc["out"].double()
    logits = od @ ca["table"].double().t()   # set c against set a's table
    lse_c = torch.logsumexp(logits, 1)
    ref_c = {"lse": lse_c, "row_loss": lse_c - logits.gather(1, cc["target"][:, None])[:, 0]}
    ia, ic = _inputs(ca), _inputs(cc)
    Pa, Pc = _problem(ca, ia, table), _problem(cc, ic, table)
    lib.acattn_full_sort_ce_products(0)
    assert lib.acattn_full_sort_ce_fwd_pair_workspace_bytes(C.byref(Pa), C.byref(Pc)) == -100  # exact-fp32 products: not served
    lib.acattn_full_sort_ce_products(2)
    nbytes = lib.acattn_full_sort_ce_fwd_pair_workspace_bytes(C.byref(Pa), C.byref(Pc))
    assert nbytes >= 0, nbytes
    out = {"lse_a": guarded((B_a,), F32, DEV, 1, "poison"), "row_loss_a": guarded((B_a,), F32, DEV, 1, "poison"),
           "dir_a": guarded((B_a, H), F32, DEV, H, "poison"), "lse_c": guarded((B_c,), F32, DEV, 1, "poison"),
           "row_loss_c": guarded((B_c,), F32, DEV, 1, "poison"), "workspace": _workspace(nbytes)}
    _lib.check(lib.acattn_full_sort_ce_fwd_pair(C.byref(Pa), C.byref(Pc), out["workspace"].ptr(), out["lse_a"].ptr(), out["row_loss_a"].ptr(),
                                                out["dir_a"].ptr(), out["lse_c"].ptr(), out["row_loss_c"].ptr(), _stream()),
               "full_sort_ce_fwd_pair")
    torch.cuda.synchronize()
    check_all(out)
    check_all(ia)
    check_all(ic)
    _check_values({"lse": out["lse_a"], "row_loss": out["row_loss_a"], "dir": out["dir_a"]}, ra)
    _check_values({"lse": out["lse_c"], "row_loss": out["row_loss_c"]}, ref_c)
