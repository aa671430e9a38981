"""GPU suite (-m gpu): the two embedding front ends (acattn_embed_layernorm_*, acattn_embed_user_layernorm_*) at their
row-block edges: every output between guards (tests/_guarded.py), fully written ones poisoned, accumulated ones zero-filled,
every row-indexed input behind a NaN / out-of-range-id back guard, every value against fp64 torch ops on the CPU.

Form thresholds, read from launch_fwd / launch_bwd of acattn_embed.hip and acattn_embed_user.hip:

    H     RPB = rows per workgroup pass    forward: one pass up to 2048 * RPB rows (grid = min(ceil(rows / RPB), 2048))
    64        16                                    32,768
    128        8                                    16,384
    256        4                                     8,192

  * above that the forward's grid-stride loop makes a second pass (`row` stops being blockIdx.x * RPB + rsub); row r sits at
    position r % L of sequence r / L, so L = 1 puts every row in its own sequence and L = 50 crosses the limit inside one;
  * the backward runs L x ACATTN_EMBED_BWD_CHUNKS = L x 8 workgroups; workgroup (l, chunk) walks ceil(B / 8) sequences at
    position l, RPB at a time: B < 8 leaves whole workgroups without a row, which still owe their rows of d_pos_part
    [8, L, H] and dgb_part [8 * L, 2, H]; the partials must sum to the fp64 gradients;
  * embed_user: lanes left of column Di read the item row, lanes right of it the user row; Di in {4, H / 2, H - 4} puts the
    seam behind the first lane, in the middle, and in front of the last lane.

d_table / d_item / d_user start as zeros (header: "must be ZERO-INITIALISED by the caller: rows are accumulated with float
atomics"); their last row is hit, ids -1 and n are clamped (header: "ids outside [0, n) are clamped, never dereferenced out of
bounds"), so the guards around the tables' gradients must stay intact.

Tolerances are those of tests/test_hip_embed.py and tests/test_hip_embed_user.py: y <= 3e-5, each gradient <= 1e-4 * max|g| +
1e-6; nonzero_out exact.  `stats` as in tests/test_hip_row_edges_ln.py (the same arithmetic): mean <= 2e-6, 1/std <= 2e-6
relative.  user_rows_ws holds the user half of every row's input gradient: held like a gradient.
"""
import ctypes as C

import pytest
import torch

from ac_tsr_amd import _lib
from tests import _row_edge_refs as R
from tests._guarded import check_all, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHUNKS = R.EMBED_BWD_CHUNKS


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(g):
    return None if g is None else g.ptr()


def _close(name, got, want, tol_abs, tol_rel=0.0):
    err = (got.detach().cpu().double() - want).abs().max().item()
    bound = tol_abs + tol_rel * want.abs().max().item()
    print(f"{name}: max error {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{name}: max error {err:.3e} > {bound:.3e}"


def _inputs(c):
    H, rows = c["H"], c["B"] * c["L"]
    b = {"idx": guarded((rows,), torch.int64, DEV, 1, c["idx"].reshape(-1)),
         "dy": guarded((rows, H), torch.float32, DEV, H, c["dy"])}
    if c["keep"] is not None:
        b["keep"] = guarded((rows, H), torch.uint8, DEV, H, c["keep"])
    if "user" in c:
        b["user"] = guarded((c["B"],), torch.int64, DEV, 1, c["user"])
    return b


def _check_forward(out, ref):
    _close("y", out["y"].t, ref["y"], 3e-5)
    _close("stats.mean", out["stats"].t[:, 0], ref["stats"][:, 0], 2e-6)
    rel = ((out["stats"].t[:, 1].cpu().double() - ref["stats"][:, 1]) / ref["stats"][:, 1]).abs().max().item()
    print(f"stats.rstd: max relative error {rel:.3e} (bound 2e-6)")
    assert rel <= 2e-6, f"stats.rstd: max relative error {rel:.3e} > 2e-6"
    assert torch.equal(out["nonzero_out"].t.cpu(), ref["nonzero"]), "nonzero_out"


def _check_partials(bwd, ref):
    _close("sum d_pos_part", bwd["d_pos_part"].t.cpu().double().sum(0), ref["d_pos"], 1e-6, 1e-4)
    gb = bwd["dgb_part"].t.cpu().double().sum(0)
    _close("sum dgb_part[:, 0] (dgamma)", gb[0], ref["dgamma"], 1e-6, 1e-4)
    _close("sum dgb_part[:, 1] (dbeta)", gb[1], ref["dbeta"], 1e-6, 1e-4)


# ---------------------------------------------------------------------------------------------------------------------------
def _run_embed(c, ref=None, padding_idx=0, hot_id=None, seed=0):
    H, B, L, N = c["H"], c["B"], c["L"], c["N"]
    rows = B * L
    lib = _lib.load()
    inp = _inputs(c)
    dev = {k: c[k].to(DEV) for k in ("table", "gamma", "beta")}
    pos = c["pos"].to(DEV) if c["pos"] is not None else None
    out = {"y": guarded((rows, H), torch.float32, DEV, H, "poison"), "stats": guarded((rows, 2), torch.float32, DEV, 2, "poison"),
           "nonzero_out": guarded((rows,), torch.uint8, DEV, 1, "poison")}
    P = _lib.EmbedProblem()
    P.rows, P.L, P.H, P.n_table_rows = rows, L, H, N
    P.idx, P.table, P.pos = inp["idx"].ptr(), dev["table"].data_ptr(), None if pos is None else pos.data_ptr()
    P.gamma, P.beta, P.eps, P.p_drop = dev["gamma"].data_ptr(), dev["beta"].data_ptr(), 1e-12, float(c["p"])
    P.keep = inp["keep"].ptr() if "keep" in inp else None
    P.seed, P.seed_device = seed, None
    P.nonzero_out = out["nonzero_out"].ptr()
    _lib.check(lib.acattn_embed_layernorm_fwd(C.byref(P), out["y"].ptr(), out["stats"].ptr(), _stream()), "embed fwd")
    torch.cuda.synchronize()
    check_all(out)
    check_all(inp)
    stats_in = ref["stats"].float() if ref is not None else out["stats"].t.clone()
    inp["stats"] = guarded((rows, 2), torch.float32, DEV, 2, stats_in.to(DEV))
    bwd = {"d_table": guarded((N, H), torch.float32, DEV, H, "zero"),
           "d_pos_part": guarded((CHUNKS, L, H), torch.float32, DEV, H, "poison"),
           "dgb_part": guarded((CHUNKS * L, 2, H), torch.float32, DEV, 2 * H, "poison")}
    P.nonzero_out = None  # forward only
    if hot_id is not None:
        P.hot_id_plus1 = hot_id + 1
    _lib.check(lib.acattn_embed_layernorm_bwd(C.byref(P), inp["dy"].ptr(), inp["stats"].ptr(), padding_idx, bwd["d_table"].ptr(),
                                              bwd["d_pos_part"].ptr(), bwd["dgb_part"].ptr(), _stream()), "embed bwd")
    torch.cuda.synchronize()
    check_all(bwd)
    check_all(inp)
    out.update(bwd)
    return out


EMBED_CASES = [(H, B, L) for H in (64, 128, 256) for (B, L) in R.embed_shapes(H)]


@pytest.mark.parametrize("H,B,L", EMBED_CASES)
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_embed_row_edges(H, B, L, p):
    c = R.embed_case(H, B, L, 301, p)
    ref = R.embed_ref(c)
    out = _run_embed(c, ref=ref)
    _check_forward(out, ref)
    _close("d_table", out["d_table"].t, ref["d_table"], 1e-6, 1e-4)
    _check_partials(out, ref)


@pytest.mark.parametrize("H", [64, 128, 256])
def test_embed_hot_id_no_padding_no_pos(H):
    """hot_id_plus1 set (the hot row is summed in the workgroup first), padding_idx = -1 (no row skipped), pos == NULL."""
    B, L = R.rpb(H) + 1, 7
    c = R.embed_case(H, B, L, 5, 0.5, with_pos=False)
    c["idx"].view(-1)[::3] = 4          # a third of the lookups hit the last table row, which is the hot one
    ref = R.embed_ref(c, padding_idx=-1)
    out = _run_embed(c, ref=ref, padding_idx=-1, hot_id=4)
    _check_forward(out, ref)
    _close("d_table", out["d_table"].t, ref["d_table"], 1e-6, 1e-4)
    _check_partials(out, ref)


@pytest.mark.parametrize("H", [64, 128, 256])
def test_embed_counter_rng_writes_everything(H):
    """Dropout from the counter RNG (keep == NULL, p = 0.5): guards and poison only."""
    c = R.embed_case(H, 2048 * R.rpb(H) + 1, 1, 301, 0.0)
    c["p"] = 0.5
    _run_embed(c, seed=0x1234567)


# ---------------------------------------------------------------------------------------------------------------------------
def _run_embed_user(c, ref=None, with_ws=True, seed=0):
    H, Di, B, L, N, U = c["H"], c["Di"], c["B"], c["L"], c["N"], c["U"]
    rows, Du = B * L, H - Di
    lib = _lib.load()
    assert lib.acattn_embed_user_supported(H, Di) == 1
    inp = _inputs(c)
    dev = {k: c[k].to(DEV) for k in ("table", "user_table", "gamma", "beta")}
    pos = c["pos"].to(DEV) if c["pos"] is not None else None
    out = {"y": guarded((rows, H), torch.float32, DEV, H, "poison"), "stats": guarded((rows, 2), torch.float32, DEV, 2, "poison"),
           "nonzero_out": guarded((rows,), torch.uint8, DEV, 1, "poison")}
    P = _lib.EmbedUserProblem()
    P.rows, P.L, P.H, P.Di, P.n_table_rows, P.n_user_rows = rows, L, H, Di, N, U
    P.idx, P.user = inp["idx"].ptr(), inp["user"].ptr()
    P.table, P.user_table, P.pos = dev["table"].data_ptr(), dev["user_table"].data_ptr(), None if pos is None else pos.data_ptr()
    P.gamma, P.beta, P.eps, P.p_drop = dev["gamma"].data_ptr(), dev["beta"].data_ptr(), 1e-12, float(c["p"])
    P.keep = inp["keep"].ptr() if "keep" in inp else None
    P.seed, P.seed_device = seed, None
    P.nonzero_out = out["nonzero_out"].ptr()
    _lib.check(lib.acattn_embed_user_layernorm_fwd(C.byref(P), out["y"].ptr(), out["stats"].ptr(), _stream()), "embed_user fwd")
    torch.cuda.synchronize()
    check_all(out)
    check_all(inp)
    stats_in = ref["stats"].float() if ref is not None else out["stats"].t.clone()
    inp["stats"] = guarded((rows, 2), torch.float32, DEV, 2, stats_in.to(DEV))
    bwd = {"d_item": guarded((N, Di), torch.float32, DEV, Di, "zero"),
           "d_user": guarded((U, Du), torch.float32, DEV, Du, "zero"),
           "user_rows_ws": guarded((rows, Du), torch.float32, DEV, Du, "poison") if with_ws else None,
           "d_pos_part": guarded((CHUNKS, L, H), torch.float32, DEV, H, "poison"),
           "dgb_part": guarded((CHUNKS * L, 2, H), torch.float32, DEV, 2 * H, "poison")}
    P.nonzero_out = None  # forward only
    _lib.check(lib.acattn_embed_user_layernorm_bwd(C.byref(P), inp["dy"].ptr(), inp["stats"].ptr(), 0, 0, bwd["d_item"].ptr(),
                                                   bwd["d_user"].ptr(), _ptr(bwd["user_rows_ws"]), bwd["d_pos_part"].ptr(),
                                                   bwd["dgb_part"].ptr(), _stream()), "embed_user bwd")
    torch.cuda.synchronize()
    check_all(bwd)
    check_all(inp)
    out.update(bwd)
    return out


def _embed_user_cases():
    cases = []
    for H in (64, 128, 256):
        r = R.rpb(H)
        cap = R.FWD_GRID_CAP * r
        for Di in (4, H // 2, H - 4):
            # every seam at the small edges; the single-pass limit and the second pass once per seam, the full list of
            # tests/_row_edge_refs.embed_shapes at the middle seam
            shapes = R.embed_shapes(H) if Di == H // 2 else [(1, 1), (r + 1, 1), (1, 50), (cap + 1, 1), (cap // 50 + 1, 50)]
            cases += [(H, Di, B, L) for (B, L) in shapes]
    return cases


@pytest.mark.parametrize("H,Di,B,L", _embed_user_cases())
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_embed_user_row_edges(H, Di, B, L, p):
    c = R.embed_user_case(H, Di, B, L, 301, 23, p)
    ref = R.embed_user_ref(c)
    out = _run_embed_user(c, ref=ref)
    _check_forward(out, ref)
    _close("d_item", out["d_item"].t, ref["d_item"], 1e-6, 1e-4)
    _close("d_user", out["d_user"].t, ref["d_user"], 1e-6, 1e-4)
    _close("user_rows_ws", out["user_rows_ws"].t, ref["user_rows"], 1e-6, 1e-4)
    _check_partials(out, ref)


@pytest.mark.parametrize("H", [64, 128, 256])
def test_embed_user_scatter_without_workspace(H):
    """user_rows_ws == NULL: the user half is scattered per row like the item half."""
    c = R.embed_user_case(H, H // 2, R.rpb(H) + 1, 7, 11, 5, 0.5)
    ref = R.embed_user_ref(c)
    out = _run_embed_user(c, ref=ref, with_ws=False)
    _check_forward(out, ref)
    _close("d_item", out["d_item"].t, ref["d_item"], 1e-6, 1e-4)
    _close("d_user", out["d_user"].t, ref["d_user"], 1e-6, 1e-4)
    _check_partials(out, ref)


@pytest.mark.parametrize("H", [64, 128, 256])
def test_embed_user_counter_rng_writes_everything(H):
    """Dropout from the counter RNG (keep == NULL, p = 0.5): guards and poison only."""
    c = R.embed_user_case(H, H // 2, 2048 * R.rpb(H) + 1, 1, 301, 23, 0.0)
    c["p"] = 0.5
    _run_embed_user(c, seed=0x1234567)
