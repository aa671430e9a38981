"""GPU suite (-m gpu): the small reductions and loss finishers of acattn_util.hip at the edges of their loops, every output
between guards and poisoned (tests/_guarded.py), every input behind a NaN back guard, every value against fp64 on the CPU.

Loop shapes, read from acattn_util.hip / acattn_sumrows.h:

  acattn_sum_rows(_pair)    a workgroup of 256 threads = CT column threads (4 columns each) x RL = 256 / CT row lanes; CT is
                            the smallest power of two >= ceil(C / 4), halved while fewer than 32 workgroups share the work
                            and R >= 4 * RL (pick_ct, restated below); rows are read four at a time per lane (r, r + RL, r +
                            2 RL, r + 3 RL), then one at a time: R in {1, 3, 4 RL - 1, 4 RL + 1}; C % 4 != 0 takes the scalar
                            path and ends inside a column thread: C in {1, 3, 4, 5, 50, 1023, 1024, 1025}
  acattn_mask_penalty_rows  one wave per (b, head, query block of 16 rows): 16-byte loads when the block's address is 16-byte
                            aligned (then a tail of n % 4), dword loads otherwise: odd L puts the blocks of odd (b, head) at
                            odd offsets
  acattn_mask_penalty_fwd / _bwd / _partial_multi / _bwd_scaled_multi
                            16-byte grid-stride loop over n / 4, a tail of n % 4 by workgroup 0; at most 1,024 workgroups
                            forward: n = 1023 * 4 + 1 ends one short of that
  acattn_attacked_loss_finish_rows(_pair)
                            one workgroup sums B row losses and `count` floats per mask, four 16-byte loads per thread per
                            trip (1,024 f4 = 4,096 floats), then single f4, then a scalar tail; up to 64 more workgroups scale
                            scale_buf (n_scale / 4 f4 + a tail of n_scale % 4 by workgroup 1)
  acattn_mask_penalty_drows(_dir)
                            up to 64 workgroups per mask fill d_pen; one more slice writes d_out = dir * d_loss (n_dir)
  acattn_dense_ce_fwd / _bwd  forward: a workgroup per row, 1,024 columns per trip (256 threads x 4); backward: 1,024 columns
                            per workgroup: N in {1, 255, 256, 257, 1023, 1024, 1025}

Tolerances are those of the existing tests of each kernel: sum_rows 1e-4 * max(1, |sum|) (tests/test_hip_ln.py); dense
cross-entropy lse / loss 1e-5 * max(1, |.|), d_logits 2e-6 * max(1, |.|) (tests/test_hip_ce.py); penalty rows (terms + 3) *
2^-24 * value (tests/test_hip_fwd_penalty_fused.py); the norm 2e-6 * norm + 1e-6 and its gradient 1e-6 * max|g| + 1e-9
(tests/test_hip_ln.py); means 1e-6 relative, the loss 1e-5 * max(1, |loss|) (tests/test_hip_ce_pair.py, tests/test_hip_ce.py).
Products of two or three fp32 numbers (scale_buf, d_pen, d_out) are held to one rounding per operation: 2^-23 per factor.
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
ULP = 2.0 ** -23


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptrs(bufs):
    return (C.c_void_p * len(bufs))(*(b.t.data_ptr() for b in bufs))


def _gen(*key):
    return torch.Generator().manual_seed(sum(int(k) * m for k, m in zip(key, (1, 7919, 104729, 1299709))))


def _close(name, got, want, tol_abs, tol_rel=0.0):
    err = (got.detach().cpu().double() - want).abs().max().item()
    bound = tol_abs + tol_rel * want.abs().max().item()
    print(f"{name}: max error {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{name}: max error {err:.3e} > {bound:.3e}"


# ---------------------------------------------------------------------------------------------------------------------------
def _pick_ct(batch, rows, cols):
    """pick_ct of acattn_sumrows.h."""
    c4 = (cols + 3) // 4
    ct = 256
    while ct > 1 and ct // 2 >= c4:
        ct //= 2
    while ct > 1 and batch * ((c4 + ct - 1) // ct) < 32 and rows >= 4 * (256 // ct):
        ct //= 2
    return ct


def _sum_rows_R(batch, cols):
    """1, 3 and 4 RL -+ 1 for the row lanes the launch will pick at that R."""
    out = {1, 3}
    for guess in (1, 2, 4, 8, 16, 32, 64, 128, 256):
        for r in (4 * guess - 1, 4 * guess + 1):
            if 256 // _pick_ct(batch, r, cols) == guess:
                out.add(r)
    return sorted(out)


SUM_CASES = [(batch, r, cols) for batch in (1, 33) for cols in (1, 3, 4, 5, 50, 1023, 1024, 1025) for r in _sum_rows_R(batch, cols)]


def _sum_case(batch, rows, cols):
    x = torch.randn(batch, rows, cols, generator=_gen(batch, rows, cols))
    return x, guarded(x.shape, F32, DEV, cols, x), guarded((batch, cols), F32, DEV, cols, "poison")


@pytest.mark.parametrize("batch,rows,cols", SUM_CASES)
def test_sum_rows(batch, rows, cols):
    x, gx, out = _sum_case(batch, rows, cols)
    _lib.check(_lib.load().acattn_sum_rows(gx.ptr(), out.ptr(), batch, rows, cols, _stream()), "sum_rows")
    torch.cuda.synchronize()
    out.check("out")
    gx.check("x")
    want = R.sum_rows_ref(x)
    _close("out", out.t, want, 1e-4 * max(1.0, want.abs().max().item()))


@pytest.mark.parametrize("first,second", [((1, 1, 1), (33, 5, 1025)), ((33, 3, 5), (1, 127, 3)), ((1, 17, 1024), (33, 1, 50)),
                                          ((1, 1025, 4), (1, 33, 1023))])
def test_sum_rows_pair(first, second):
    (x1, g1, o1), (x2, g2, o2) = _sum_case(*first), _sum_case(*second)
    _lib.check(_lib.load().acattn_sum_rows_pair(g1.ptr(), o1.ptr(), *first, g2.ptr(), o2.ptr(), *second, _stream()), "sum_rows_pair")
    torch.cuda.synchronize()
    check_all({"out1": o1, "out2": o2, "x1": g1, "x2": g2})
    for name, o, x in (("out1", o1, x1), ("out2", o2, x2)):
        want = R.sum_rows_ref(x)
        _close(name, o.t, want, 1e-4 * max(1.0, want.abs().max().item()))


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 15, 16, 17, 50])
@pytest.mark.parametrize("B,nh", [(1, 1), (3, 2)])
def test_mask_penalty_rows(B, nh, L):
    m = torch.rand(B, nh, L, L, generator=_gen(B, nh, L))
    nqb = (L + 15) // 16
    gm = guarded(m.shape, F32, DEV, L, m)
    pen = guarded((B, nh, nqb), F32, DEV, nqb, "poison")
    _lib.check(_lib.load().acattn_mask_penalty_rows(gm.ptr(), B, nh, L, pen.ptr(), _stream()), "mask_penalty_rows")
    torch.cuda.synchronize()
    pen.check("pen")
    gm.check("m")
    want = R.penalty_rows_ref(m)
    terms = torch.tensor([min(16, L - 16 * qb) * L for qb in range(nqb)], dtype=torch.float64)
    err = (pen.t.cpu().double() - want).abs()
    bound = (terms + 3.0) * 2.0 ** -24 * want
    print(f"pen: max err / bound = {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023 * 4 + 1])
def test_mask_penalty_norm_and_gradient(n):
    lib = _lib.load()
    g = _gen(n, 5)
    m = torch.rand(n, generator=g)
    d_norm = torch.randn(1, generator=g)
    gm = guarded((n,), F32, DEV, 1, m)
    ws = guarded((_lib.PENALTY_WS_FLOATS,), F32, DEV, 1, "scratch")
    norm = guarded((1,), F32, DEV, 1, "poison")
    _lib.check(lib.acattn_mask_penalty_fwd(gm.ptr(), n, ws.ptr(), norm.ptr(), _stream()), "mask_penalty_fwd")
    torch.cuda.synchronize()
    check_all({"norm": norm, "workspace": ws, "m": gm})
    want = torch.linalg.vector_norm(1 - m.double()).reshape(1)
    _close("norm", norm.t, want, 1e-6, 2e-6)
    norm_in = guarded((1,), F32, DEV, 1, want.float())
    gd = guarded((1,), F32, DEV, 1, d_norm)
    d_m = guarded((n,), F32, DEV, 1, "poison")
    _lib.check(lib.acattn_mask_penalty_bwd(gm.ptr(), norm_in.ptr(), gd.ptr(), n, d_m.ptr(), _stream()), "mask_penalty_bwd")
    torch.cuda.synchronize()
    check_all({"d_m": d_m, "m": gm, "norm": norm_in, "d_norm": gd})
    _close("d_m", d_m.t, d_norm.double() * (m.double() - 1) / want, 1e-9, 1e-6)
    # d_m = d_loss * scale * (m - 1) / norm
    d_s = guarded((n,), F32, DEV, 1, "poison")
    _lib.check(lib.acattn_mask_penalty_bwd_scaled(gm.ptr(), norm_in.ptr(), gd.ptr(), 0.37, n, d_s.ptr(), _stream()),
               "mask_penalty_bwd_scaled")
    torch.cuda.synchronize()
    check_all({"d_m (scaled)": d_s, "m": gm})
    _close("d_m (scaled)", d_s.t, 0.37 * d_norm.double() * (m.double() - 1) / want, 1e-9, 1e-6)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023 * 4 + 1])
@pytest.mark.parametrize("n_masks", [1, 3])
def test_mask_penalty_multi(n, n_masks):
    """acattn_mask_penalty_partial_multi: part [n_masks, 1024], of which each mask's first min(ceil(n / 1024), 1024) entries
    are its partial sums (the finisher reads that many) -- scratch beyond them, so guards only and the SUM of a zeroed row is
    compared; acattn_mask_penalty_bwd_scaled_multi: every d_m written in full."""
    lib = _lib.load()
    g = _gen(n, n_masks, 7)
    ms = [torch.rand(n, generator=g) for _ in range(n_masks)]
    d_loss = torch.randn(1, generator=g)
    gms = [guarded((n,), F32, DEV, 1, m) for m in ms]
    part = guarded((n_masks, _lib.PENALTY_WS_FLOATS), F32, DEV, _lib.PENALTY_WS_FLOATS, "scratch")
    _lib.check(lib.acattn_mask_penalty_partial_multi(_ptrs(gms), n_masks, n, part.ptr(), _stream()), "mask_penalty_partial_multi")
    torch.cuda.synchronize()
    check_all({"part": part, **{f"m[{i}]": b for i, b in enumerate(gms)}})
    sq = torch.stack([((1 - m.double()) ** 2).sum() for m in ms])
    _close("sum part", part.t.cpu().double().sum(1), sq, 0.0, 4e-6)  # the square of a norm held to 2e-6 relative
    norms = sq.sqrt()
    gn = guarded((n_masks,), F32, DEV, 1, norms.float())
    gd = guarded((1,), F32, DEV, 1, d_loss)
    d_ms = [guarded((n,), F32, DEV, 1, "poison") for _ in range(n_masks)]
    _lib.check(lib.acattn_mask_penalty_bwd_scaled_multi(_ptrs(gms), gn.ptr(), gd.ptr(), 0.01, n, _ptrs(d_ms), n_masks, _stream()),
               "mask_penalty_bwd_scaled_multi")
    torch.cuda.synchronize()
    check_all({"norms": gn, "d_loss": gd, **{f"d_m[{i}]": b for i, b in enumerate(d_ms)}, **{f"m[{i}]": b for i, b in enumerate(gms)}})
    for i in range(n_masks):
        _close(f"d_m[{i}]", d_ms[i].t, 0.01 * d_loss.double() * (ms[i].double() - 1) / norms[i], 1e-9, 1e-6)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 3, 1024, 1025, 4099])
@pytest.mark.parametrize("n_scale", [0, 1, 3, 4, 5, 4 * 256 * 64 + 3])
@pytest.mark.parametrize("pair", [False, True], ids=["rows", "rows_pair"])
def test_attacked_loss_finish_rows(count, n_scale, pair):
    """out [2 + n_masks] = (weight * mean_l norm_l - mean row_loss, mean row_loss, norm_0, ...); scale_buf *= -1 / B in place;
    the pair form adds mean_c = mean(row_loss_c)."""
    lib = _lib.load()
    n_masks, weight = 2, 0.03
    B = count  # the row losses share the summing loop with the pen vectors: the same edge counts
    B_c = max(1, count - 2)
    g = _gen(count, n_scale, int(pair))
    row_loss = 3 * torch.rand(B, generator=g) + 0.5
    pens = [torch.rand(count, generator=g) for _ in range(n_masks)]
    scale = torch.randn(max(n_scale, 1), generator=g)[:n_scale]
    row_loss_c = 3 * torch.rand(B_c, generator=g) + 0.5
    bufs = {"row_loss": guarded((B,), F32, DEV, 1, row_loss), "out": guarded((2 + n_masks,), F32, DEV, 1, "poison")}
    gp = [guarded((count,), F32, DEV, 1, p) for p in pens]
    bufs.update({f"pen[{i}]": b for i, b in enumerate(gp)})
    gs = None
    if n_scale:
        # read and written in place: its own check follows the comparison (neither poison nor an input)
        gs = guarded((n_scale,), F32, DEV, 1, "scratch")
        gs.t.copy_(scale)
        bufs["scale_buf"] = gs
    sp = None if gs is None else gs.ptr()
    if pair:
        bufs["row_loss_c"] = guarded((B_c,), F32, DEV, 1, row_loss_c)
        bufs["mean_c"] = guarded((1,), F32, DEV, 1, "poison")
        rc = lib.acattn_attacked_loss_finish_rows_pair(bufs["row_loss"].ptr(), B, _ptrs(gp), n_masks, count, weight, bufs["out"].ptr(),
                                                       sp, n_scale, bufs["row_loss_c"].ptr(), B_c, bufs["mean_c"].ptr(), _stream())
    else:
        rc = lib.acattn_attacked_loss_finish_rows(bufs["row_loss"].ptr(), B, _ptrs(gp), n_masks, count, weight, bufs["out"].ptr(), sp,
                                                  n_scale, _stream())
    _lib.check(rc, "attacked_loss_finish_rows")
    torch.cuda.synchronize()
    check_all(bufs)
    norms = torch.stack([p.double().sum().sqrt() for p in pens])
    ce = row_loss.double().mean()
    out = bufs["out"].t.cpu().double()
    assert abs(out[1].item() - ce.item()) <= 1e-6 * abs(ce.item()), ("mean row loss", out[1].item(), ce.item())
    _close("norms", out[2:], norms, 1e-6, 2e-6)
    loss = weight * norms.mean() - ce
    assert abs(out[0].item() - loss.item()) <= 1e-5 * max(1.0, abs(loss.item())), ("loss", out[0].item(), loss.item())
    if n_scale:
        want = scale.double() * (-1.0 / B)
        err = (gs.t.cpu().double() - want).abs()
        assert bool((err <= 2 * ULP * want.abs()).all()), f"scale_buf: first bad offset {int(torch.nonzero(err > 2 * ULP * want.abs())[0, 0])}"
    if pair:
        want = row_loss_c.double().mean().item()
        assert abs(bufs["mean_c"].t.item() - want) <= 1e-6 * abs(want), ("mean_c", bufs["mean_c"].t.item(), want)


@pytest.mark.parametrize("count", [1, 3, 1024, 1025, 4099])
@pytest.mark.parametrize("n_dir", [None, 0, 1, 3, 4, 5, 4 * 256 * 64 + 3])
def test_mask_penalty_drows(count, n_dir):
    """d_pen[l][:] = d_loss * scale / (2 norm_l), and (the _dir form) d_out = direction * d_loss.  n_dir == 0 is refused by the
    _dir entry point ("count, n_dir positive"): that case asserts the refusal and that nothing was written."""
    lib = _lib.load()
    n_masks, scale = 3, 0.015
    g = _gen(count, -1 if n_dir is None else n_dir, 11)
    norms = torch.rand(n_masks, generator=g) + 0.5
    d_loss = torch.randn(1, generator=g)
    bufs = {"norms": guarded((n_masks,), F32, DEV, 1, norms), "d_loss": guarded((1,), F32, DEV, 1, d_loss)}
    refused = n_dir == 0  # the _dir entry point takes n_dir >= 1 (an argument error otherwise: nothing may be enqueued)
    d_pen = [guarded((count,), F32, DEV, 1, torch.zeros(count) if refused else "poison") for _ in range(n_masks)]
    bufs.update({f"d_pen[{i}]": b for i, b in enumerate(d_pen)})
    if n_dir is None:
        rc = lib.acattn_mask_penalty_drows(bufs["norms"].ptr(), bufs["d_loss"].ptr(), scale, count, _ptrs(d_pen), n_masks, _stream())
    else:
        # (n_dir == 0: both pointers must still be valid; one float each that the launch may neither read nor write)
        direction = torch.randn(max(n_dir, 1), generator=g)
        bufs["direction"] = guarded((max(n_dir, 1),), F32, DEV, 1, direction)
        bufs["d_out"] = guarded((max(n_dir, 1),), F32, DEV, 1, "poison" if n_dir else direction)
        rc = lib.acattn_mask_penalty_drows_dir(bufs["norms"].ptr(), bufs["d_loss"].ptr(), scale, count, _ptrs(d_pen), n_masks,
                                               bufs["direction"].ptr(), bufs["d_out"].ptr(), n_dir, _stream())
    torch.cuda.synchronize()
    if refused:
        assert rc < 0 and b"n_dir" in lib.acattn_last_error(), (rc, lib.acattn_last_error())
        check_all(bufs)  # every buffer (held as an input here) keeps its bits, every guard stands
        return
    _lib.check(rc, "mask_penalty_drows")
    check_all(bufs)
    for i in range(n_masks):
        want = (d_loss.double() * scale / (2 * norms[i].double())).expand(count)
        err = (d_pen[i].t.cpu().double() - want).abs().max().item()
        assert err <= 4 * ULP * want.abs().max().item(), (f"d_pen[{i}]", err)
    if n_dir:
        want = direction.double() * d_loss.double()
        err = (bufs["d_out"].t.cpu().double() - want).abs()
        assert bool((err <= 2 * ULP * want.abs()).all()), f"d_out: first bad offset {int(torch.nonzero(err > 2 * ULP * want.abs())[0, 0])}"


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 255, 256, 257, 1023, 1024, 1025])
@pytest.mark.parametrize("rows", [1, 3])
def test_dense_cross_entropy(rows, N):
    lib = _lib.load()
    c = R.dense_ce_case(rows, N)
    ref = R.dense_ce_ref(c)
    inp = {"logits": guarded((rows, N), F32, DEV, N, c["logits"]), "target": guarded((rows,), torch.int64, DEV, 1, c["target"]),
           "coef": guarded((rows,), F32, DEV, 1, c["coef"])}
    out = {"lse": guarded((rows,), F32, DEV, 1, "poison"), "row_loss": guarded((rows,), F32, DEV, 1, "poison")}
    _lib.check(lib.acattn_dense_ce_fwd(inp["logits"].ptr(), rows, N, inp["target"].ptr(), out["lse"].ptr(), out["row_loss"].ptr(),
                                       _stream()), "dense_ce_fwd")
    torch.cuda.synchronize()
    check_all(out)
    check_all(inp)
    for k in ("lse", "row_loss"):
        _close(k, out[k].t, ref[k], 1e-5 * max(1.0, ref[k].abs().max().item()))
    inp["lse"] = guarded((rows,), F32, DEV, 1, ref["lse"].float())
    d = guarded((rows, N), F32, DEV, N, "poison")
    _lib.check(lib.acattn_dense_ce_bwd(inp["logits"].ptr(), inp["lse"].ptr(), inp["target"].ptr(), inp["coef"].ptr(), rows, N, d.ptr(),
                                       _stream()), "dense_ce_bwd")
    torch.cuda.synchronize()
    d.check("d_logits")
    check_all(inp)
    _close("d_logits", d.t, ref["d_logits"], 2e-6 * max(1.0, ref["d_logits"].abs().max().item()))
