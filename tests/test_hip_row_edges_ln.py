"""GPU suite (-m gpu): acattn_dropout_add_layernorm_fwd / _bwd at their row-block edges, every output between guards and
poisoned (tests/_guarded.py), every input behind a NaN back guard, every value against fp64 torch ops on the CPU.

Form thresholds, read from acattn_ln.hip (launch_fwd, launch_bwd):

    H     lanes/row  RPB = rows per workgroup pass   forward: one pass up to 2048 * RPB   backward: 512 workgroups cover
    64       16            16                                 32,768 rows                         8,192 rows per pass
    128      32             8                                 16,384 rows                         4,096
    256      64             4                                  8,192 rows                         2,048

  * forward grid = min(ceil(rows / RPB), 2048): above 2048 * RPB rows the grid-stride loop makes a second pass, the one in
    which `row` stops being blockIdx.x * RPB + rsub -- rows 2 * 2048 * RPB + 3 end inside a THIRD pass's first workgroup;
  * backward grid = ACATTN_LN_BWD_GRID = 512 whatever the size: below 512 * RPB rows there are workgroups with no row, which
    still owe their [2, H] row of dgb_part (zeros), and the partials must sum to the fp64 dgamma / dbeta;
  * hence rows 1, RPB - 1, RPB, RPB + 1, 512 * RPB -+ 1, 2048 * RPB - 1, 2048 * RPB, 2048 * RPB + 1, 2 * 2048 * RPB + 3.

Tolerances are those of tests/test_hip_ln.py: y <= 2e-5; each gradient <= 1e-4 * max|g| + 1e-6.  `stats` has no test of its
own there; its bound is worked out from the arithmetic: the mean is a tree sum of H <= 256 fp32 terms of size |s| <~ 6 (depth
8: <= 8 * 2^-24 * mean|s| ~ 5e-7), held to 2e-6; 1/std is one hardware rsq (1 ulp) of a variance summed the same way
(relative error ~ 5e-7, halved by the root), held to 2e-6 relative -- tighter than what y's 2e-5 at |y| <~ 6 implies (3e-6).
"""
import ctypes as C

import pytest
import torch

from ac_tsr_amd import _lib
from tests import _row_edge_refs as R
from tests._guarded import check_all, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(g):
    return None if g is None else g.ptr()


def _inputs(c):
    """Guarded device copies of the row-indexed inputs (NaN / 0x5A back guards); gamma and beta need none."""
    H = c["H"]
    b = {"z": guarded(c["z"].shape, torch.float32, DEV, H, c["z"]),
         "residual": guarded(c["residual"].shape, torch.float32, DEV, H, c["residual"]),
         "dy": guarded(c["dy"].shape, torch.float32, DEV, H, c["dy"])}
    if c["keep"] is not None:
        b["keep"] = guarded(c["keep"].shape, torch.uint8, DEV, H, c["keep"])
    return b


def _problem(c, inp, gamma, beta, p, seed=0):
    P = _lib.LnProblem()
    P.rows, P.H, P.residual_rows = c["rows"], c["H"], c["residual_rows"]
    P.z, P.residual, P.gamma, P.beta = inp["z"].ptr(), inp["residual"].ptr(), gamma.data_ptr(), beta.data_ptr()
    P.eps, P.p_drop = 1e-12, float(p)
    P.keep = inp["keep"].ptr() if "keep" in inp else None
    P.seed = seed
    P.seed_device = None
    return P


def _close(name, got, want, tol_abs, tol_rel=0.0):
    err = (got.detach().cpu().double() - want).abs().max().item()
    bound = tol_abs + tol_rel * want.abs().max().item()
    print(f"{name}: max error {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{name}: max error {err:.3e} > {bound:.3e}"


def _run(c, want_dz=True, want_dres=True, want_gb=True, ref=None, seed=0):
    """One forward and one backward launch on guarded buffers; returns the output buffers after their guard / poison check."""
    H, rows = c["H"], c["rows"]
    lib = _lib.load()
    inp = _inputs(c)
    gamma, beta = c["gamma"].to(DEV), c["beta"].to(DEV)
    P = _problem(c, inp, gamma, beta, c["p"], seed)
    out = {"y": guarded((rows, H), torch.float32, DEV, H, "poison"), "stats": guarded((rows, 2), torch.float32, DEV, 2, "poison")}
    _lib.check(lib.acattn_dropout_add_layernorm_fwd(C.byref(P), out["y"].ptr(), out["stats"].ptr(), _stream()), "ln fwd")
    torch.cuda.synchronize()
    check_all(out)
    check_all(inp)
    # the backward reads stats as an input: the reference's (fp32-rounded) when there is one, else the forward's own
    stats_in = ref["stats"].float() if ref is not None else out["stats"].t.clone()
    inp["stats"] = guarded((rows, 2), torch.float32, DEV, 2, stats_in.to(DEV))
    bwd = {"dz": guarded((rows, H), torch.float32, DEV, H, "poison") if want_dz else None,
           "dres": guarded((rows, H), torch.float32, DEV, H, "poison") if want_dres else None,
           "dgb_part": guarded((R.LN_BWD_GRID, 2, H), torch.float32, DEV, 2 * H, "poison") if want_gb else None}
    _lib.check(lib.acattn_dropout_add_layernorm_bwd(C.byref(P), inp["dy"].ptr(), inp["stats"].ptr(), _ptr(bwd["dz"]),
                                                    _ptr(bwd["dres"]), _ptr(bwd["dgb_part"]), _stream()), "ln bwd")
    torch.cuda.synchronize()
    check_all(bwd)
    check_all(inp)
    out.update(bwd)
    return out


def _compare(out, ref):
    _close("y", out["y"].t, ref["y"], 2e-5)
    _close("stats.mean", out["stats"].t[:, 0], ref["stats"][:, 0], 2e-6)
    rel = ((out["stats"].t[:, 1].cpu().double() - ref["stats"][:, 1]) / ref["stats"][:, 1]).abs().max().item()
    print(f"stats.rstd: max relative error {rel:.3e} (bound 2e-6)")
    assert rel <= 2e-6, f"stats.rstd: max relative error {rel:.3e} > 2e-6"
    if out["dz"] is not None:
        _close("dz", out["dz"].t, ref["dz"], 1e-6, 1e-4)
    if out["dres"] is not None:
        _close("dres", out["dres"].t, ref["dres"], 1e-6, 1e-4)
    if out["dgb_part"] is not None:
        gb = out["dgb_part"].t.cpu().double().sum(0)
        _close("sum dgb_part[:, 0] (dgamma)", gb[0], ref["dgamma"], 1e-6, 1e-4)
        _close("sum dgb_part[:, 1] (dbeta)", gb[1], ref["dbeta"], 1e-6, 1e-4)


CASES = [(H, rows) for H in (64, 128, 256) for rows in R.ln_rows(H)]


@pytest.mark.parametrize("H,rows", CASES)
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_ln_row_edges(H, rows, p):
    c = R.ln_case(H, rows, rows, p)
    ref = R.ln_ref(c)
    _compare(_run(c, ref=ref), ref)


@pytest.mark.parametrize("H", [64, 128, 256])
def test_ln_broadcast_residual(H):
    """residual_rows a proper divisor of rows: row r reads residual row r % residual_rows, across row blocks."""
    rr = R.rpb(H) + 1
    c = R.ln_case(H, 3 * rr, rr, 0.5)
    ref = R.ln_ref(c)
    _compare(_run(c, ref=ref), ref)


@pytest.mark.parametrize("H", [64, 128, 256])
@pytest.mark.parametrize("absent", ["dz", "dres", "dgb_part"])
def test_ln_bwd_optional_outputs(H, absent):
    """dz / dres / dgb_part NULL in turn (header: "may each be NULL"): the other two are written in full."""
    rows = R.rpb(H) + 1
    c = R.ln_case(H, rows, rows, 0.5)
    ref = R.ln_ref(c)
    _compare(_run(c, want_dz=absent != "dz", want_dres=absent != "dres", want_gb=absent != "dgb_part", ref=ref), ref)


@pytest.mark.parametrize("H", [64, 128, 256])
def test_ln_counter_rng_writes_everything(H):
    """Dropout from the counter RNG (keep == NULL, p = 0.5): guards and poison only."""
    rows = 2048 * R.rpb(H) + 1
    c = R.ln_case(H, rows, rows, 0.0)
    c["p"] = 0.5
    _run(c, seed=0x1234567)
