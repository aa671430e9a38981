"""GPU suite (-m gpu): acattn_layer_tail_fwd / _fwd_pair / _bwd at the row-block edges of every launch form, every output
between guards and poisoned (tests/_guarded.py; d_ctx / d_x zero-filled under a row selection, as the header asks), every
row-indexed input and saved tensor behind a NaN back guard, every value against the chain in fp64 on the CPU.

Launch forms, read from launch_fwd / launch_bwd / launch_wide_fwd / launch_wide_bwd of acattn_tail.hip (a row block is 16
rows; loads are clamped to row R - 1 and stores masked by ok[] in wave_rows; the staged / chunked kernels skip the dgb_part
row of a wave whose rows all lie past the end through write_part):

    hidden 64   rows <= 4,096        four waves share one row block            dgb_part rows = ceil(rows / 16)
                4,097 .. 16,383      one wave, one row block  (nb = 1)                          ceil(rows / 16)
                16,384 .. 32,767     one wave, two row blocks (nb = 2)                          ceil(rows / 32)
                >= 32,768            staged: workgroups of four waves = 64 rows                 ceil(rows / 16)
                acattn_select_layer_tail_blocks(1 / 2) forces the nb = 1 / nb = 2 form at any size (and switches the
                four-wave and the staged form off); with nb = 2, rows 33 .. 48 leave the second block of the last wave
                wholly past the end.  With split planes the same row blocks run on bf16 products (the four-wave backward
                and the staged form stay on fp32; acattn_layer_tail_split_bytes says 0 for the latter).
    hidden 128  rows <= 8,192        wide: four waves (two at inner 64) share one row block     ceil(rows / 16)
                >= 8,193             staged: workgroups of four waves = 64 rows                 ceil(rows / 16)
    hidden 256  every size           chunked: workgroups of four waves = 64 rows                ceil(rows / 16)

gelu_grad is written by the hidden-128 / 256 forward and by the staged hidden-64 forward when given, and read by the matching
backward; the other hidden-64 forms ignore it (header), so it is only passed where the form takes it.

Tolerances are those of tests/test_hip_tail.py: forward tensors <= 3e-5 absolute, gradients <= 2e-4 of the tensor's largest
magnitude + 1e-6 -- with ONE exception, h3.  The existing bound rests on "LayerNorm outputs are O(1)"; h1 and act (sums of H
= 64 .. 256 products, |.| <= 15, one fp32 ulp <= 9.5e-7) still have 30 ulps of room in it, but dense_2's output h3 is a sum
of I = 128 .. 1,024 fp32 products that reaches |h3| = 25 .. 46 with these inputs, where one ulp is 3.8e-6: 3e-5 absolute is 8
ulps after a 1,024-term sum (random-walk estimate of the rounding alone: sqrt(I) * 2^-24 * |h3| = 7.7e-5; the kernels measure
1.5e-5 .. 5.1e-5, every form and width alike).  No existing test bounds h3; it is held to 3e-5 OF ITS SCALE, 3e-5 * max(1,
max|ref|): a wrong row, a dropped column or a stale value is off by the scale itself.
st1 / st2 (mean, 1/std) are held to 3e-5 (1/std relative): a = (s - mean) / std * g + b is held to 3e-5 at |a| up to 10, which
a relative error of 1/std above 3e-6 would already break -- the bound on the statistics asks no more than the bounds on a
and out imply.
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


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(g):
    return None if g is None else g.ptr()


@pytest.fixture
def lib():
    """The library with its process-wide switches restored afterwards."""
    lib = _lib.load()
    nb = lib.acattn_select_layer_tail_blocks(0)
    products = lib.acattn_linear_products(-1)
    yield lib
    lib.acattn_select_layer_tail_blocks(nb)
    lib.acattn_linear_products(products)


def _close(name, got, want, tol_abs, tol_rel=0.0):
    err = (got.detach().cpu().double() - want).abs().max().item()
    bound = tol_abs + tol_rel * want.abs().max().item()
    print(f"{name}: max error {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{name}: max error {err:.3e} > {bound:.3e}"


def _problem(c, inp, dev, planes, seeds=(0, 0)):
    P = _lib.TailProblem()
    P.rows, P.H, P.I = c["rows"], c["H"], c["I"]
    P.ctx, P.x = inp["ctx"].ptr(), inp["x"].ptr()
    for k in R.TAIL_PARAMS:
        setattr(P, k, dev[k].data_ptr())
    P.eps1 = P.eps2 = 1e-12
    P.p1 = P.p2 = float(c["p"])
    P.keep1 = inp["keep1"].ptr() if "keep1" in inp else None
    P.keep2 = inp["keep2"].ptr() if "keep2" in inp else None
    P.seed1, P.seed2 = seeds
    P.seed_device = None
    if c["src_index"] is not None:
        P.src_index, P.src_R, P.src_L = inp["src_index"].ptr(), c["src_R"], c["src_L"]
    P.split_planes = _ptr(planes)
    return P


def _inputs(c):
    H, rows = c["H"], c["rows"]
    inp = {"ctx": guarded(c["ctx"].shape, F32, DEV, H, c["ctx"]), "x": guarded(c["x"].shape, F32, DEV, H, c["x"]),
           "d_out": guarded((rows, H), F32, DEV, H, c["d_out"])}
    for k in ("keep1", "keep2"):
        if c[k] is not None:
            inp[k] = guarded((rows, H), torch.uint8, DEV, H, c[k])
    if c["src_index"] is not None:
        inp["src_index"] = guarded((rows,), torch.int64, DEV, 1, c["src_index"])
    return inp


def _planes(lib, c, inp, dev, split):
    """The split weight planes (guards only: a copy of the weights in another format) or None for the exact-fp32 products."""
    nbytes = int(lib.acattn_layer_tail_split_bytes(c["H"], c["I"], c["rows"])) if split else 0
    if nbytes == 0:
        return None
    planes = guarded((nbytes // 4,), F32, DEV, 64, "scratch")
    P = _problem(c, inp, dev, None)
    _lib.check(lib.acattn_layer_tail_split_weights(C.byref(P), planes.ptr(), _stream()), "tail split weights")
    torch.cuda.synchronize()
    planes.check("split_planes")
    return planes


def _saved_outputs(c, with_gelu_grad):
    H, I, rows = c["H"], c["I"], c["rows"]
    out = {k: guarded((rows, H), F32, DEV, H, "poison") for k in ("h1", "a", "h3", "out")}
    out.update({k: guarded((rows, 2), F32, DEV, 2, "poison") for k in ("st1", "st2")})
    out["act"] = guarded((rows, I), F32, DEV, I, "poison")
    out["gelu_grad"] = guarded((rows, I), F32, DEV, I, "poison") if with_gelu_grad else None
    return out


def _saved_struct(bufs):
    S = _lib.TailSaved()
    for k in ("h1", "st1", "a", "act", "h3", "st2", "out", "gelu_grad"):
        setattr(S, k, _ptr(bufs.get(k)))
    return S


def _check_forward(out, ref):
    for k in ("h1", "a", "act", "out"):  # the bound of tests/test_hip_tail.py as it stands
        _close(k, out[k].t, ref[k], 3e-5)
    _close("h3", out["h3"].t, ref["h3"], 3e-5 * max(1.0, ref["h3"].abs().max().item()))  # 3e-5 of its scale, see above
    if out["gelu_grad"] is not None:
        _close("gelu_grad", out["gelu_grad"].t, ref["gelu_grad"], 3e-5)
    for k in ("st1", "st2"):
        _close(k + ".mean", out[k].t[:, 0], ref[k][:, 0], 3e-5)
        rel = ((out[k].t[:, 1].cpu().double() - ref[k][:, 1]) / ref[k][:, 1]).abs().max().item()
        print(f"{k}.rstd: max relative error {rel:.3e} (bound 3e-5)")
        assert rel <= 3e-5, f"{k}.rstd: max relative error {rel:.3e} > 3e-5"


def _forward(lib, c, inp, dev, planes, with_gelu_grad, seeds=(0, 0)):
    P = _problem(c, inp, dev, planes, seeds)
    out = _saved_outputs(c, with_gelu_grad)
    S = _saved_struct(out)
    _lib.check(lib.acattn_layer_tail_fwd(C.byref(P), C.byref(S), _stream()), "tail fwd")
    torch.cuda.synchronize()
    check_all(out)
    check_all(inp)
    return out


def _backward(lib, c, inp, dev, planes, saved_values, with_gelu_grad, with_params, seeds=(0, 0)):
    """One backward launch: the saved tensors are guarded inputs holding `saved_values` (name -> fp32 CPU tensor)."""
    H, I, rows = c["H"], c["I"], c["rows"]
    names = ("h1", "st1", "a", "act", "h3", "st2", "out") + (("gelu_grad",) if with_gelu_grad else ())
    width = {"st1": 2, "st2": 2, "act": I, "gelu_grad": I}
    sv = {k: guarded(saved_values[k].shape, F32, DEV, width.get(k, H), saved_values[k]) for k in names}
    P = _problem(c, inp, dev, planes, seeds)
    S = _saved_struct(sv)
    picked = c["src_index"] is not None
    # header: under a row selection "the backward ADDS the d_ctx / d_x rows there ...: the caller zero-fills those two"
    fill = "zero" if picked else "poison"
    out = {"d_ctx": guarded((c["src_rows"], H), F32, DEV, H, fill), "d_x": guarded((c["src_rows"], H), F32, DEV, H, fill)}
    if with_params:
        out["d_h1"] = guarded((rows, H), F32, DEV, H, "poison")
        out["d_h2"] = guarded((rows, I), F32, DEV, I, "poison")
        out["d_h3"] = guarded((rows, H), F32, DEV, H, "poison")
        out["dgb_part"] = guarded((int(lib.acattn_layer_tail_bwd_partial_rows_for(rows, H)), 4, H), F32, DEV, 4 * H, "poison")
    ws_bytes = int(lib.acattn_layer_tail_bwd_workspace_bytes(H, I))
    out["workspace"] = guarded((ws_bytes // 4,), F32, DEV, H, "scratch")
    io = _lib.TailBwdIO()
    io.d_out = inp["d_out"].ptr()
    for k in ("d_ctx", "d_x", "d_h1", "d_h2", "d_h3", "dgb_part", "workspace"):
        setattr(io, k, _ptr(out.get(k)))
    _lib.check(lib.acattn_layer_tail_bwd(C.byref(P), C.byref(S), C.byref(io), _stream()), "tail bwd")
    torch.cuda.synchronize()
    check_all(out)
    check_all(sv)
    check_all(inp)
    return out


def _check_backward(out, ref):
    for k in ("d_ctx", "d_x", "d_h1", "d_h2", "d_h3"):
        if k in out:
            _close(k, out[k].t, ref[k], 1e-6, 2e-4)
    if "dgb_part" in out:
        gb = out["dgb_part"].t.cpu().double().sum(0)
        for i, k in enumerate(("dgamma1", "dbeta1", "dgamma2", "dbeta2")):
            _close(f"sum dgb_part[:, {i}] ({k})", gb[i], ref["dgb"][i], 1e-6, 2e-4)


def _takes_gelu_grad(lib, H, rows):
    """Forms that write / read acattn_tail_saved.gelu_grad: hidden 128 / 256, and the staged form of hidden 64."""
    return H > 64 or rows >= 32768


def _run(lib, H, I, rows, p, split, pick=False, nb=0):
    lib.acattn_select_layer_tail_blocks(nb)
    c = R.tail_case(H, I, rows, p, pick)
    ref = R.tail_ref(c)
    inp = _inputs(c)
    dev = {k: c[k].to(DEV) for k in R.TAIL_PARAMS}
    planes = _planes(lib, c, inp, dev, split)
    gg = _takes_gelu_grad(lib, H, rows) and nb == 0
    _check_forward(_forward(lib, c, inp, dev, planes, gg), ref)
    saved = {k: ref[k].float() for k in ("h1", "st1", "a", "act", "h3", "st2", "out", "gelu_grad")}
    # with and without gelu_grad where the form takes both; with the parameter-side outputs given and NULL (the attack pass)
    for with_gg in ((True, False) if gg else (False,)):
        for with_params in (True, False):
            print(f"backward: gelu_grad {'given' if with_gg else 'NULL'}, d_h* / dgb_part {'given' if with_params else 'NULL'}")
            _check_backward(_backward(lib, c, inp, dev, planes, saved, with_gg, with_params), ref)
    if planes is not None:
        planes.check("split_planes")


# hidden 64: (rows, nb hook); nb = 0 leaves the choice to the size
H64_SMALL = [(r, 0) for r in (1, 15, 16, 17, 33)] + [(r, 1) for r in (1, 16, 17)] + [(r, 2) for r in (1, 16, 17, 32, 33, 48, 49)]


@pytest.mark.parametrize("rows,nb", H64_SMALL)
@pytest.mark.parametrize("I", [256, 128])
@pytest.mark.parametrize("split", [False, True], ids=["fp32", "split"])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_tail64_small_forms(lib, rows, nb, I, split, p):
    _run(lib, 64, I, rows, p, split, nb=nb)


@pytest.mark.parametrize("rows", [4096, 4097])
@pytest.mark.parametrize("I", [256, 128])
@pytest.mark.parametrize("split", [False, True], ids=["fp32", "split"])
def test_tail64_form_border(lib, rows, I, split):
    _run(lib, 64, I, rows, 0.5, split)


@pytest.mark.parametrize("rows", [32768, 32768 + 1, 32768 + 17, 32768 + 63])
@pytest.mark.parametrize("I", [256, 128])
def test_tail64_staged(lib, rows, I):
    assert lib.acattn_layer_tail_split_bytes(64, I, rows) == 0  # the staged form reads no planes
    _run(lib, 64, I, rows, 0.5, False)


@pytest.mark.parametrize("rows", [1, 15, 16, 17, 8192, 8193, 8193 + 16, 8193 + 63])
@pytest.mark.parametrize("I", [512, 256, 64])
def test_tail128(lib, rows, I):
    _run(lib, 128, I, rows, 0.5, False)


@pytest.mark.parametrize("I", [512, 256, 64])
def test_tail128_without_dropout(lib, I):
    _run(lib, 128, I, 17, 0.0, False)


@pytest.mark.parametrize("rows", [1, 16, 17, 63, 64, 65])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_tail256_chunked(lib, rows, p):
    _run(lib, 256, 1024, rows, p, False)


# one row selection per form: duplicate picks, positions -1 and L (clamped), d_ctx / d_x zero-filled
@pytest.mark.parametrize("H,I,rows,nb,split", [
    (64, 256, 33, 0, True), (64, 128, 33, 0, False), (64, 256, 33, 1, True), (64, 256, 48, 2, True), (64, 128, 48, 2, False),
    (64, 256, 4098, 0, True), (64, 256, 32768 + 19, 0, False), (128, 512, 33, 0, False), (128, 64, 8193 + 18, 0, False),
    (256, 1024, 66, 0, False)])
def test_tail_row_selection(lib, H, I, rows, nb, split):
    _run(lib, H, I, rows, 0.5, split, pick=True, nb=nb)


@pytest.mark.parametrize("H,I,rows,nb", [(64, 256, 17, 0), (64, 256, 49, 2), (64, 128, 4097, 0), (64, 256, 32768 + 17, 0),
                                         (128, 512, 17, 0), (128, 256, 8193 + 16, 0), (256, 1024, 65, 0)])
def test_tail_counter_rng_writes_everything(lib, H, I, rows, nb):
    """Dropout from the counter RNG (keep1 == keep2 == NULL, p = 0.5): guards and poison only; the backward reads what the
    forward saved."""
    lib.acattn_select_layer_tail_blocks(nb)
    c = R.tail_case(H, I, rows, 0.0)
    c["p"] = 0.5
    inp = _inputs(c)
    dev = {k: c[k].to(DEV) for k in R.TAIL_PARAMS}
    planes = _planes(lib, c, inp, dev, True)
    gg = _takes_gelu_grad(lib, H, rows) and nb == 0
    seeds = (0x1234567, 0x89ABCDE)
    out = _forward(lib, c, inp, dev, planes, gg, seeds)
    saved = {k: v.t.cpu() for k, v in out.items() if v is not None}
    _backward(lib, c, inp, dev, planes, saved, gg, True, seeds)


@pytest.mark.parametrize("rows", [1, 15, 16, 17, 33])
@pytest.mark.parametrize("I", [256, 128])
def test_tail64_pair_forward(lib, rows, I):
    """acattn_layer_tail_fwd_pair: two problems (own ctx, keep masks, outputs; shared x, weights, planes) in one launch of twice
    the workgroups -- both sides' outputs guarded, poisoned and held to fp64."""
    ca, cb = R.tail_case(64, I, rows, 0.5), R.tail_case(64, I, rows, 0.5, pick=False)
    g = torch.Generator().manual_seed(rows + I)
    cb["ctx"] = torch.randn(rows, 64, generator=g)
    cb["keep1"] = torch.empty(rows, 64).bernoulli_(0.5, generator=g).to(torch.uint8)
    cb["keep2"] = torch.empty(rows, 64).bernoulli_(0.5, generator=g).to(torch.uint8)
    refs = [R.tail_ref(ca), R.tail_ref(cb)]
    dev = {k: ca[k].to(DEV) for k in R.TAIL_PARAMS}
    inps = [_inputs(ca), _inputs(cb)]
    planes = _planes(lib, ca, inps[0], dev, True)
    assert planes is not None
    outs = [_saved_outputs(ca, False), _saved_outputs(cb, False)]
    Ps = [_problem(c, inp, dev, planes) for c, inp in zip((ca, cb), inps)]
    Ss = [_saved_struct(o) for o in outs]
    _lib.check(lib.acattn_layer_tail_fwd_pair(C.byref(Ps[0]), C.byref(Ss[0]), C.byref(Ps[1]), C.byref(Ss[1]), _stream()),
               "tail fwd pair")
    torch.cuda.synchronize()
    for out, inp, ref in zip(outs, inps, refs):
        check_all(out)
        check_all(inp)
        _check_forward(out, ref)
    planes.check("split_planes")
