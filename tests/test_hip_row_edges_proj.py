"""GPU suite (-m gpu): acattn_projections_fwd / _qkv_fwd / _bwd at their row-block edges, every output between guards and
poisoned (tests/_guarded.py), x and every cotangent behind a NaN back guard, every value against six nn.Linear in fp64.

Launch forms, read from acattn_launch_proj_fwd / _bwd, launch_wide_fwd / launch_wide_bwd of acattn_proj.hip (a row block is
16 rows; loads are clamped to the last row, stores masked):

    hidden 64    rows < 16,384   one wave per workgroup, one row block (16 rows) per wave
                 rows >= 16,384  one wave per workgroup, two row blocks (32 rows) per wave       (rows_per_wave)
                 split bf16 products for G <= 64 (weights split in the workgroup, or read from split_planes), exact-fp32
                 kernels for a wider gate
    hidden 128   staged: workgroups of 4 waves x 2 row blocks = 128 rows at every size
    hidden 256   staged: workgroups of 4 waves x 1 row block  =  64 rows at every size

  * hence rows 1, 15, 16, 17, 31, 32, 33, 63, 64, 65 (wave and workgroup edges, waves wholly past the end) and 16,384 + {0, 1,
    17} (where hidden 64 doubles its rows per wave; at 128 / 256 a large ragged count);
  * G in {0, 37, 50, 200}: no gate, a gate that ends inside a 16-column tile, and one wider than the hidden size;
  * backward MODE 1 (every cotangent given, dx / dmq_total / dmk_total wanted), MODE 2 (dqa, dka alone), MODE 0 (anything
    else) as BWD_CASES of tests/test_hip_proj_planes.py; hidden 128 / 256 refuse dx without dmq_total ("it is read back as a
    source of dx"), so the q/k/v-only case asks for it there.

`affine` [B, nh, 4, LP]: the one use of `unwritten=` in this module -- include/acattn.h, acattn_proj_out.affine: "entries [0,
L) of every plane are written, the padding entries are left alone (allocate the buffer zeroed once; they must be finite)".

Tolerances are those of tests/test_hip_proj.py: outputs <= 2e-5 absolute, gradients <= 2e-4 of the tensor's largest
magnitude + 1e-6.  The affine planes and the gate probabilities are O(1) outputs of the same products: 2e-5.
"""
import ctypes as C

import pytest
import torch

from ac_tsr_amd import _lib
from tests import _row_edge_refs as R
from tests._guarded import check_all, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
ROWS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 16384, 16384 + 1, 16384 + 17]
COTS = ("dmq", "dmk", "dmv", "dqa", "dka", "dgate")
BWD_CASES = {
    "mode1": (("dmq", "dmk", "dmv", "dqa", "dka", "dgate"), ("dmq_total", "dmk_total", "dx")),
    "mode2": (("dqa", "dka"), ("dmq_total", "dmk_total", "dx")),
    "mode0_attack_only": (("dqa", "dka"), ("dmq_total", "dmk_total")),
    "mode0_no_dmv": (("dmq", "dmk", "dqa", "dka", "dgate"), ("dmq_total", "dmk_total", "dx")),
    "mode0_qkv": (("dmq", "dmk", "dmv"), ("dx",)),
}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(g):
    return None if g is None else g.ptr()


@pytest.fixture
def lib():
    lib = _lib.load()
    products = lib.acattn_linear_products(-1)
    yield lib
    lib.acattn_linear_products(products)


def _close(name, got, want, tol_abs, tol_rel=0.0):
    err = (got.detach().cpu().double() - want).abs().max().item()
    bound = tol_abs + tol_rel * want.abs().max().item()
    print(f"{name}: max error {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{name}: max error {err:.3e} > {bound:.3e}"


def _device(c):
    names = [p + n for n in R.PROJ_MATS + (("g",) if c["G"] else ()) for p in ("w", "b")]
    return {k: c[k].to(DEV) for k in names + ["w_order", "b_order", "w_dist", "b_dist"]}


def _inputs(c):
    H, rows = c["H"], c["rows"]
    inp = {k: guarded((rows, H), F32, DEV, H, c[k]) for k in ("x", "dmq", "dmk", "dmv", "dqa", "dka", "dx_init")}
    if c["G"]:
        inp["dgate"] = guarded((rows, c["G"]), F32, DEV, c["G"], c["dgate"])
    return inp


def _problem(c, inp, dev, planes=None):
    P = _lib.ProjProblem()
    P.rows, P.H, P.G, P.x = c["rows"], c["H"], c["G"], inp["x"].ptr()
    for k, t in dev.items():
        setattr(P, k, t.data_ptr())
    P.n_heads, P.L = c["n_heads"], c["L"]
    P.split_planes = _ptr(planes)
    return P


def _proj_planes(lib, c, dev):
    """The split weight planes of hidden 64 (guards only: a copy of the weights in another format), or None."""
    nbytes = int(lib.acattn_projections_split_bytes(c["H"], c["G"]))
    if nbytes == 0:
        return None
    planes = guarded((nbytes // 4,), F32, DEV, 64, "scratch")
    job = _lib.SplitLayer()
    for n in R.PROJ_MATS:
        setattr(job, "w" + n, dev["w" + n].data_ptr())
    if c["G"]:
        job.wg, job.G = dev["wg"].data_ptr(), c["G"]
    job.proj_planes = planes.ptr()
    _lib.check(lib.acattn_split_weights_many(C.byref(job), 1, _stream()), "split_weights_many")
    torch.cuda.synchronize()
    planes.check("split_planes")
    return planes


def _forward(lib, c, inp, P, ref, gate_prob, with_affine, qkv=False):
    H, G, rows, nh, L = c["H"], c["G"], c["rows"], c["n_heads"], c["L"]
    out = {k: guarded((rows, H), F32, DEV, H, "poison") for k in (("mq", "mk", "mv") if qkv else ("mq", "mk", "mv", "qa", "ka"))}
    if G and not qkv:
        out["gate"] = guarded((rows, G), F32, DEV, G, "poison")
    LP = 16 * ((L + 15) // 16)
    if with_affine:
        out["affine"] = guarded((rows // L, nh, 4, LP), F32, DEV, LP, "poison")
    O = _lib.ProjOut()
    for k, g in out.items():
        setattr(O, k, g.ptr())
    O.gate_prob = int(gate_prob)
    fn = lib.acattn_projections_qkv_fwd if qkv else lib.acattn_projections_fwd
    _lib.check(fn(C.byref(P), C.byref(O), _stream()), "projections fwd")
    torch.cuda.synchronize()
    # include/acattn.h, acattn_proj_out.affine: "entries [0, L) of every plane are written, the padding entries are left alone"
    padding = torch.zeros(rows // L, nh, 4, LP, dtype=torch.bool)
    padding[..., L:] = True
    check_all(out, unwritten={"affine": padding} if LP > L else None)
    check_all(inp)
    for k, g in out.items():
        if k == "affine":
            _close(k, g.t[..., :L], ref[k][..., :L], 2e-5)
        else:
            _close(k, g.t, ref["gate_prob" if (k == "gate" and gate_prob) else k], 2e-5)


def _backward(lib, c, inp, P, case, dx_init):
    H, rows = c["H"], c["rows"]
    given, wanted = BWD_CASES[case]
    if H > 64 and "dx" in wanted and "dmq_total" not in wanted:
        wanted = ("dmq_total",) + wanted  # hidden 128 / 256: "dx needs dmq_total (it is read back as a source of dx)"
    given = tuple(k for k in given if k != "dgate" or c["G"])
    io = _lib.ProjBwdIO()
    for k in given:
        setattr(io, k, inp[k].ptr())
    out = {k: guarded((rows, H), F32, DEV, H, "poison") for k in wanted}
    for k, g in out.items():
        setattr(io, k, g.ptr())
    if dx_init and "dx" in wanted:
        io.dx_init = inp["dx_init"].ptr()
    ws_bytes = int(lib.acattn_projections_bwd_workspace_bytes(C.byref(P)))
    if ws_bytes:
        out["workspace"] = guarded((ws_bytes // 4,), F32, DEV, H, "scratch")
        io.workspace = out["workspace"].ptr()
    _lib.check(lib.acattn_projections_bwd(C.byref(P), C.byref(io), _stream()), "projections bwd")
    torch.cuda.synchronize()
    check_all(out)
    check_all(inp)
    ref = R.proj_bwd_ref(c, given, dx_init)
    for k in wanted:
        _close(f"{case}{' +dx_init' if dx_init else ''}: {k}", out[k].t, ref[k], 1e-6, 2e-4)


def _run(lib, H, G, rows, use_planes=False):
    c = R.proj_case(H, G, rows)
    ref = R.proj_fwd_ref(c)
    dev, inp = _device(c), _inputs(c)
    planes = _proj_planes(lib, c, dev) if use_planes else None
    P = _problem(c, inp, dev, planes)
    _forward(lib, c, inp, P, ref, gate_prob=False, with_affine=True)
    _forward(lib, c, inp, P, ref, gate_prob=True, with_affine=False)
    for case in BWD_CASES:
        for dx_init in (False, True):
            if dx_init and "dx" not in BWD_CASES[case][1]:
                continue
            _backward(lib, c, inp, P, case, dx_init)
    if planes is not None:
        planes.check("split_planes")


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("G", [0, 37, 50, 200])
@pytest.mark.parametrize("H", [128, 256])
def test_proj_wide_row_edges(lib, H, G, rows):
    _run(lib, H, G, rows)


@pytest.mark.parametrize("rows", [1, 15, 16, 17])
@pytest.mark.parametrize("G,form", [(0, "split"), (37, "split"), (50, "split"), (50, "planes"), (0, "planes"), (200, "fp32"),
                                    (50, "fp32")])
def test_proj64_row_edges(lib, G, form, rows):
    """Hidden 64: the split products with the weights split in the workgroup or read from planes, and the exact-fp32 kernels
    (a gate wider than 64, or acattn_linear_products(0))."""
    if form == "fp32" and G <= 64:
        lib.acattn_linear_products(0)
    _run(lib, 64, G, rows, use_planes=form == "planes")


@pytest.mark.parametrize("rows", [1, 15, 16, 17, 16384 + 17])
def test_proj64_qkv_forward(lib, rows):
    """acattn_projections_qkv_fwd: mq, mk, mv (and the affine planes) alone; qa, ka, gate NULL."""
    assert lib.acattn_projections_qkv_supported(64) == 1
    c = R.proj_case(64, 0, rows)
    ref = R.proj_fwd_ref(c)
    dev, inp = _device(c), _inputs(c)
    P = _problem(c, inp, dev)
    _forward(lib, c, inp, P, ref, gate_prob=False, with_affine=True, qkv=True)
    _forward(lib, c, inp, P, ref, gate_prob=False, with_affine=False, qkv=True)
