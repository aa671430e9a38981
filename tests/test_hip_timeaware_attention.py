"""GPU suite (-m gpu): the time-interval attention core of ACTiSASRec (csrc/acattn_timeaware.hip) through the C ABI
(acattn_timeaware_attention_fwd / _bwd, acattn_time_rng_materialize) and through ops.timeaware_attention.

Reference: tests/_timeaware_ref.py::core_from_projected_time in FLOAT64 on the CPU (tests/_timeaware_cases.py), fed the very
draws and keep bits the kernels use.  Bound, for EVERY forward output (ctx_attacked, ctx_calibrated, M, the penalty rows,
row_stats slots 0-1) and EVERY gradient (dq, dk, dv, dqa, dka, the gate logits, the five calibrator parameters, d pos_k,
d pos_v = dv, d time_k, d time_v -- the kernels' plain derivatives, row 0 of the tables included): with e32 the float32
restatement's own error against float64, max(1e-4, 2 e32) of the float64 tensor's maximum (capped at 2e-3, floor 1e-7
absolute).  tests/test_timeaware_cases_cpu.py holds e32 to 2e-5 (1e-4 for the three single numbers), so the bound is the 1e-4
floor for every tensor.  All rows are compared, those without an allowed key included.
"""
import ctypes as C

import pytest
import torch

import ac_tsr_amd as A
from ac_tsr_amd import _lib, attn_launch
from tests import _attention_fp64 as F
from tests import _timeaware_cases as TC

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED, TIME_SEED = 4242, 977
_PROBLEMS, _ORACLES = {}, {}


def _problem(c):
    key = TC.forward_key(c)._replace(cots=c.cots)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = (TC.problem(c), F.torch_draws(c.base))
    return _PROBLEMS[key]


def _oracle(c, p, draws, dtype):
    """The restatement of the case's own problem, computed once per (case, dtype) and left unchanged."""
    key = (TC.forward_key(c)._replace(cots=c.cots), dtype)
    if key not in _ORACLES:
        _ORACLES[key] = TC.oracle(c, p, draws, p.cot, dtype)
    return _ORACLES[key]


def _dev(p):
    return {k: v.to(DEV).contiguous() for k, v in p.t.items()}


_u8 = lambda t: None if t is None else t.to(torch.uint8).to(DEV).contiguous()


def _fill(c, p, x, draws=None, seed=None, noise=None, index=None, keeps="explicit", time_seed=TIME_SEED):
    """(acattn_problem, acattn_time_ext, tensors to keep alive) for case `c`.  `draws` = explicit layer randomness (else the
    counter stream of `seed`); `keeps` = "explicit" (the problem's bits), "counter" (time_seed) or a (keep_k, keep_v) pair of
    device tensors; `index` replaces the problem's index matrix (a device int32 tensor)."""
    b = c.base
    hold = [p.pr.kv.to(DEV).contiguous()]
    rnd = None
    if draws is not None:
        rnd = (draws["noise"].to(DEV).contiguous() if noise is None else noise, _u8(draws["keep_after"]), _u8(draws["keep_mask"]),
               None)
        hold += [t for t in rnd if t is not None]
    flat = [x[k].reshape(-1) if k.startswith("w_") else x[k] for k in ("w_order", "b_order", "w_dist", "b_dist", "scalar")]
    prob = attn_launch.fill_problem(x["q"], x["k"], x["v"], x["qa"], x["ka"], x["gl"], *flat, b.nh, b.p_drop, seed or 0, None,
                                    key_valid=hold[0], causal=b.causal, rnd=rnd)
    idx = p.index.to(DEV).contiguous() if index is None else index
    kk = kv = None
    if keeps == "explicit":
        kk, kv = _u8(p.keep_k), _u8(p.keep_v)
    elif keeps != "counter":
        kk, kv = keeps
    text = attn_launch.fill_time_ext(x["pos_k"], x["pos_v"], idx, x["time_k"], x["time_v"], c.p_time, keep_k=kk, keep_v=kv,
                                     seed=time_seed)
    return prob, text, hold + flat + [idx, kk, kv]


def _forward(c, p, x, poison=False, **kw):
    prob, text, hold = _fill(c, p, x, **kw)
    ctx_a, ctx_c, M, stats, pen = attn_launch.timeaware_attention_fwd_launch(_lib.load(), prob, text, x["q"], c.base.nh,
                                                                             want_penalty=True, poison=poison)
    torch.cuda.synchronize()
    return {"ctx_attacked": ctx_a, "ctx_calibrated": ctx_c, "M": M, "stats": stats, "pen": pen}


def _backward(c, p, x, fwd, cot, poison=False, d_pen=None, **kw):
    """({leaf: gradient} on the CPU, raw device outputs) of sum_k out_k cot_k through acattn_timeaware_attention_bwd; an output
    without a cotangent is passed as NULL."""
    prob, text, hold = _fill(c, p, x, **kw)
    dc = {k: v.to(DEV).contiguous() for k, v in cot.items()}
    res = attn_launch.timeaware_attention_bwd_launch(
        _lib.load(), prob, text, x["q"], c.base.nh, fwd["M"], fwd["stats"], c.span + 1, d_att=dc.get("ctx_attacked"),
        d_cal=dc.get("ctx_calibrated"), d_M=dc.get("M"), d_pen=d_pen, poison=poison)
    torch.cuda.synchronize()
    dq, dk, dv, dqa, dka, dgate, part, d_pos_k, d_time_k, d_time_v = res
    dh = c.base.H // c.base.nh
    tot = part.sum(0)
    g_wo, g_bo, g_wd, g_bd, g_sc, _ = attn_launch.unpack_partials(tot, dh, p.t["w_order"], p.t["b_order"], p.t["w_dist"],
                                                                  p.t["b_dist"], p.t["scalar"])
    out = dict(q=dq, k=dk, v=dv, qa=dqa, ka=dka, gl=dgate.sum(1), w_order=g_wo, b_order=g_bo, w_dist=g_wd, b_dist=g_bd, scalar=g_sc,
               pos_k=d_pos_k, pos_v=dv, time_k=d_time_k, time_v=d_time_v)
    raw = dict(dq=dq, dk=dk, dv=dv, dqa=dqa, dka=dka, dgate=dgate, part=part, d_pos_k=d_pos_k, d_time_k=d_time_k, d_time_v=d_time_v)
    return {k: v.detach().cpu() for k, v in out.items()}, raw


def _outs(fwd):
    o = {k: fwd[k].detach().cpu() for k in TC.OUTPUTS + ("pen",)}
    o["lse_p"], o["lse_m"] = fwd["stats"][..., 0].cpu(), fwd["stats"][..., 1].cpu()
    return o


def _failures(tag, got, ref64, ref32, names):
    bad = []
    for n in names:
        abs_e, scale = F.abs_err_and_scale(got[n], ref64[n])
        abs_e32, _ = F.abs_err_and_scale(ref32[n], ref64[n])
        e, e32 = (abs_e / scale, abs_e32 / scale) if scale > 0 else (abs_e, abs_e32)
        bound = F.tensor_bound(e32)
        print(f"timeaware_accuracy {tag} {n} e={e:.3e} e32={e32:.3e} bound={bound:.1e} scale={scale:.3e}")
        if not abs_e <= bound * scale + F.ABS_FLOOR:
            bad.append(f"{n}: e = {e:.3e} > {bound:.3e} (e32 = {e32:.3e}, scale {scale:.3e})")
    return bad


_FWD_CASES = list({TC.forward_key(c): c for c in reversed(TC.CASES)}.values())[::-1]  # one case per forward problem


@pytest.mark.parametrize("case", _FWD_CASES, ids=lambda c: c.id)
def test_forward_matches_the_fp64_restatement_on_every_row(case):
    c = case
    p, draws = _problem(c)
    got = _forward(c, p, _dev(p), draws=draws, poison=True)
    _, ref64 = _oracle(c, p, draws, torch.float64)
    _, ref32 = _oracle(c, p, draws, torch.float32)
    bad = _failures(f"case={c.id} fwd", _outs(got), ref64, ref32, TC.COMPARED_OUTPUTS)
    assert not bad, f"{c.id}: " + "; ".join(bad)
    assert (got["stats"][..., 2:] == 0).all()


@pytest.mark.parametrize("case", TC.CASES, ids=lambda c: c.id)
def test_backward_matches_the_fp64_restatement(case):
    """Explicit bits; the cotangents the case names, NULL for the rest; every row carries one, dead rows included."""
    c = case
    p, draws = _problem(c)
    x = _dev(p)
    fwd = _forward(c, p, x, draws=draws)
    got, _ = _backward(c, p, x, fwd, p.cot, draws=draws, poison=True)
    ref64, _ = _oracle(c, p, draws, torch.float64)
    ref32, _ = _oracle(c, p, draws, torch.float32)
    bad = _failures(f"case={c.id} bwd", got, ref64, ref32, TC.leaf_names(c))
    assert not bad, f"{c.id}: " + "; ".join(bad)
    if c.base.L > 1 and {"ctx_attacked", "ctx_calibrated"} & set(c.cots):
        # row 0 of both tables is the padding row of nn.Embedding: the kernel returns its true derivative, which is not zero
        for n in ("time_k", "time_v"):
            assert ref64[n][0].abs().max() > 0 and got[n][0].abs().max() > 0, n


def test_no_cotangent_at_all_gives_zero_gradients():
    c = TC._case((3, 17, 32), 7)
    p, draws = _problem(c)
    x = _dev(p)
    fwd = _forward(c, p, x, draws=draws)
    got, _ = _backward(c, p, x, fwd, {}, draws=draws, poison=True)
    for n, g in got.items():
        assert torch.isfinite(g).all() and g.abs().max() == 0, n


_COUNTER_CASES = [c for c in TC.CASES if c.cots == TC.OUTPUTS and c.stamps == "mixed" and not c.base.left_pad and c.base.causal
                  and (c.base.L, c.base.H) in ((17, 32), (50, 128), (64, 32))]


@pytest.mark.parametrize("case", _COUNTER_CASES, ids=lambda c: c.id)
def test_counter_bits_are_the_materialised_ones(case):
    """Counter randomness on both sides (the layer's draws and the time dropouts): the launch against the float64 restatement
    on the bits acattn_rng_materialize / acattn_time_rng_materialize return, and an EXPLICIT launch on those bits."""
    c = case
    b = c.base
    p, _ = _problem(c)
    x = _dev(p)
    rnd = A.materialize_randomness(b.B, b.nh, b.L, SEED, b.p_drop, DEV)
    draws = {"noise": rnd.noise.cpu(), "keep_after": None, "keep_mask": None, "keep_before": None}
    if b.p_drop > 0:
        draws.update(keep_after=rnd.keep_after.cpu().float(), keep_mask=rnd.keep_mask.cpu().float())
    keeps = None, None
    if c.p_time > 0:
        keeps = A.materialize_time_randomness(b.B, b.L, b.H, TIME_SEED, c.p_time, DEV)
        other = A.materialize_time_randomness(b.B, b.L, b.H, TIME_SEED + 1, c.p_time, DEV)
        for t in keeps:
            assert abs(t.float().mean().item() - (1 - c.p_time)) < 0.02
        assert (keeps[0] != keeps[1]).float().mean() > 0.3 and (keeps[0] != other[0]).float().mean() > 0.3
    fwd = _forward(c, p, x, seed=SEED, keeps="counter")
    got, _ = _backward(c, p, x, fwd, p.cot, seed=SEED, keeps="counter")
    cpu_keeps = tuple(None if t is None else t.cpu().float() for t in keeps)
    ref64g, ref64 = TC.oracle(c, p, draws, p.cot, torch.float64, keeps=cpu_keeps)
    ref32g, ref32 = TC.oracle(c, p, draws, p.cot, torch.float32, keeps=cpu_keeps)
    bad = _failures(f"case={c.id} counter fwd", _outs(fwd), ref64, ref32, TC.COMPARED_OUTPUTS)
    bad += _failures(f"case={c.id} counter bwd", got, ref64g, ref32g, TC.leaf_names(c))
    assert not bad, f"{c.id}: " + "; ".join(bad)
    fwd_e = _forward(c, p, x, draws=draws, keeps=keeps if c.p_time > 0 else "explicit")
    got_e, _ = _backward(c, p, x, fwd_e, p.cot, draws=draws, keeps=keeps if c.p_time > 0 else "explicit")
    for k in TC.OUTPUTS:
        assert F.err(fwd_e[k], fwd[k]) <= 1e-6, k
    for n in TC.leaf_names(c):
        assert F.err(got_e[n], got[n]) <= 1e-6, n


def test_a_general_dropout_rate_draws_its_own_counter_bits():
    """p_time = 0.3 takes the per-column branch of the counter stream: the materialised bits keep 70 % and are the kernel's."""
    c = TC._case((3, 17, 32), 7, p_time=0.3)
    p, draws = TC.problem(c), F.torch_draws(c.base)
    x = _dev(p)
    keeps = A.materialize_time_randomness(c.base.B, c.base.L, c.base.H, TIME_SEED, 0.3, DEV)
    for t in keeps:
        assert abs(t.float().mean().item() - 0.7) < 0.02
    a = _forward(c, p, x, draws=draws, keeps="counter")
    b = _forward(c, p, x, draws=draws, keeps=keeps)
    ga, _ = _backward(c, p, x, a, p.cot, draws=draws, keeps="counter")
    gb, _ = _backward(c, p, x, b, p.cot, draws=draws, keeps=keeps)
    for k in TC.OUTPUTS:
        assert torch.equal(a[k], b[k]), k
    for n in ga:
        assert F.err(gb[n], ga[n]) <= 1e-6, n


def test_a_nan_behind_masked_keys_reaches_the_attacked_context_alone():
    """A_att = N where M = 0: a NaN in time_v at an index used only at padded or future keys reaches ctx_attacked, and not
    ctx_calibrated (P = 0 there: the weight skips the row)."""
    c = TC._case((3, 37, 64), 256, p_drop=0.0, p_time=0.0)
    p, draws = TC.problem(c), F.torch_draws(c.base)
    L, span = c.base.L, c.span
    allowed = (p.pr.mask_dense.expand(c.base.B, 1, L, L)[:, 0] == 0)  # [B, L, L]
    index = p.index.clone()
    index[allowed & (index == span)] = span - 1  # keep row `span` for masked pairs only
    index[~allowed] = span
    assert (~allowed).any() and not (index[allowed] == span).any()
    x = _dev(p)
    base = _forward(c, p, x, draws=draws, index=index.to(DEV))
    x2 = dict(x)
    x2["time_v"] = x["time_v"].clone()
    x2["time_v"][span, :] = float("nan")
    got = _forward(c, p, x2, draws=draws, index=index.to(DEV))
    assert torch.isnan(got["ctx_attacked"]).any()
    assert torch.equal(got["ctx_calibrated"], base["ctx_calibrated"]) and torch.equal(got["M"], base["M"])
    # and with finite values there the masked keys do enter ctx_attacked (no (i, j) below L is skipped on the value side)
    x3 = dict(x)
    x3["time_v"] = x["time_v"].clone()
    x3["time_v"][span, :] += 1.0
    moved = _forward(c, p, x3, draws=draws, index=index.to(DEV))
    assert (moved["ctx_attacked"] - base["ctx_attacked"]).abs().max() > 1e-2
    assert torch.equal(moved["ctx_calibrated"], base["ctx_calibrated"])


@pytest.mark.parametrize("L", (17, 49))
def test_tile_padding_columns_contribute_nothing_and_every_element_is_written(L):
    """time_index, the two tables and pos_k / pos_v are cut from larger buffers whose neighbouring memory holds out-of-range
    indices and 1e30; outputs are NaN-prefilled.  Bitwise the results from clean buffers (the table gradients, the one pair of
    outputs with atomics, to 1e-6)."""
    c = TC._case((2, L, 64), 7)
    p, draws = TC.problem(c), F.torch_draws(c.base)
    x = _dev(p)

    def cut(t, fill):
        big = torch.full((t.numel() + 8192,), fill, device=DEV, dtype=t.dtype)
        view = big[4096:4096 + t.numel()].view(t.shape)
        view.copy_(t)
        return view

    x2 = dict(x)
    for k in ("pos_k", "pos_v", "time_k", "time_v"):
        x2[k] = cut(x[k], 1e30)
    index = cut(p.index.to(DEV), 1 << 20)
    a = _forward(c, p, x, draws=draws)
    b = _forward(c, p, x2, draws=draws, index=index, poison=True)
    for k in ("ctx_attacked", "ctx_calibrated", "M", "stats", "pen"):
        assert torch.isfinite(b[k]).all(), k
        assert torch.equal(a[k], b[k]), k
    assert a["ctx_attacked"].abs().max() < 1e4
    _, ra = _backward(c, p, x, a, p.cot, draws=draws)
    _, rb = _backward(c, p, x2, b, p.cot, draws=draws, index=index, poison=True)
    for k in ra:
        assert torch.isfinite(rb[k]).all(), k
        if k in ("d_time_k", "d_time_v"):
            assert F.err(rb[k], ra[k]) <= 1e-6, k
        else:
            assert torch.equal(ra[k], rb[k]), k


def test_indices_are_clamped_into_the_table():
    """time_span + 5 gives the result of time_span, -3 that of 0, forward and backward."""
    c = TC._case((3, 17, 32), 7)
    p, draws = TC.problem(c), F.torch_draws(c.base)
    x = _dev(p)
    clean = p.index.to(DEV)
    wild = clean.clone()
    wild[clean == c.span] = c.span + 5
    wild[clean == 0] = -3
    assert (wild > c.span).any() and (wild < 0).any()
    a = _forward(c, p, x, draws=draws)
    b = _forward(c, p, x, draws=draws, index=wild)
    for k in ("ctx_attacked", "ctx_calibrated", "M", "stats"):
        assert torch.equal(a[k], b[k]), k
    _, ra = _backward(c, p, x, a, p.cot, draws=draws)
    _, rb = _backward(c, p, x, b, p.cot, draws=draws, index=wild)
    for k in ra:
        if k in ("d_time_k", "d_time_v"):
            assert F.err(rb[k], ra[k]) <= 1e-6, k
        else:
            assert torch.equal(ra[k], rb[k]), k


def test_two_backward_launches_give_the_same_bits_outside_the_table_gradients():
    c = TC._case((3, 50, 128), 256)
    p, draws = _problem(c)
    x = _dev(p)
    fwd = _forward(c, p, x, draws=draws)
    again = _forward(c, p, x, draws=draws)
    for k in fwd:
        assert torch.equal(fwd[k], again[k]), k
    _, one = _backward(c, p, x, fwd, p.cot, draws=draws)
    _, two = _backward(c, p, x, fwd, p.cot, draws=draws)
    for k in one:
        if k in ("d_time_k", "d_time_v"):  # summed with float atomics: equal to rounding, not to the bit
            assert F.err(two[k], one[k]) <= 1e-6, k
        else:
            assert torch.equal(one[k], two[k]), k


def test_penalty_cotangent_equals_the_dense_mask_cotangent_it_stands_for():
    c = TC._case((3, 50, 128), 256)
    p, draws = _problem(c)
    x = _dev(p)
    fwd = _forward(c, p, x, draws=draws)
    d_pen = torch.rand(c.base.B, c.base.nh, (c.base.L + 15) // 16, device=DEV) + 0.5
    rows = d_pen.repeat_interleave(16, dim=2)[:, :, :c.base.L]
    dense = 2 * rows[..., None] * (fwd["M"] - 1)
    via_pen, _ = _backward(c, p, x, fwd, {}, draws=draws, d_pen=d_pen)
    via_mask, _ = _backward(c, p, x, fwd, {"M": dense}, draws=draws)
    for n in ("qa", "ka"):
        assert via_mask[n].abs().max() > 0
        assert F.err(via_pen[n], via_mask[n]) <= 1e-5, n
    for n in ("q", "k", "v", "gl", "pos_k", "time_k", "time_v"):
        assert via_pen[n].abs().max() <= F.ABS_FLOOR and via_mask[n].abs().max() <= F.ABS_FLOOR, n


def _operator(c, p, draws, x, keeps=True):
    u8 = lambda t: None if t is None else t.to(torch.uint8).to(DEV)
    rnd = A.ExplicitRandomness(noise=draws["noise"].to(DEV), keep_after=u8(draws["keep_after"]), keep_mask=u8(draws["keep_mask"]))
    index = p.index.to(DEV)
    tk = A.TimeIntervals(x["time_k"], index, c.p_time, u8(p.keep_k))
    tv = A.TimeIntervals(x["time_v"], index, c.p_time, u8(p.keep_v))
    cfg = A.AttentionConfig(n_heads=c.base.nh)
    return A.timeaware_attention(
        x["q"], x["k"], x["v"], x["qa"], x["ka"], x["gl"], A.StructuredMask(p.pr.kv.to(DEV), causal=c.base.causal), cfg,
        p_drop=c.base.p_drop, rnd=rnd, pos_k=x["pos_k"], pos_v=x["pos_v"], time_k=tk, time_v=tv,
        **{k: x[k] for k in ("w_order", "b_order", "w_dist", "b_dist", "scalar")})


def test_the_operator_zeroes_row_0_of_the_table_gradients_and_can_be_walked_twice(monkeypatch):
    """ops.timeaware_attention: gradients by autograd against the float64 restatement with row 0 of the two table gradients
    zeroed (nn.Embedding(padding_idx=0)) -- the restatement's own row 0 is not zero --, two walks of one graph (the trainer's
    retain_graph=True), the penalty rows attached, and no launch of another attention kernel."""
    def other(*a, **k):
        raise AssertionError("another attention kernel was launched")

    for name in ("attention_fwd_launch", "attention_bwd_launch", "unnorm_attention_fwd_launch", "unnorm_attention_bwd_launch"):
        monkeypatch.setattr(attn_launch, name, other)
    c = TC._case((3, 50, 128), 256)
    p, draws = _problem(c)
    names = TC.leaf_names(c)
    x = {k: p.t[k].to(DEV).requires_grad_(True) for k in names}
    ctx_a, ctx_c, M, probs = _operator(c, p, draws, x)
    assert probs == {} and M._acattn_pen.shape == (c.base.B, c.base.nh, 4)
    outs = {"ctx_attacked": ctx_a, "ctx_calibrated": ctx_c, "M": M}
    loss = sum((outs[k] * p.cot[k].to(DEV)).sum() for k in p.cot)
    leaves = [x[n] for n in names]
    first = torch.autograd.grad(loss, leaves, retain_graph=True)
    second = torch.autograd.grad(loss, leaves)
    for n, a, b in zip(names, first, second):
        if n in ("time_k", "time_v"):
            assert F.err(b, a) <= 1e-6, n
        else:
            assert torch.equal(a, b), n
    got = {n: g.detach().cpu().reshape(p.t[n].shape) for n, g in zip(names, first)}
    ref64, _ = _oracle(c, p, draws, torch.float64)
    ref32, _ = _oracle(c, p, draws, torch.float32)
    ref64, ref32 = dict(ref64), dict(ref32)
    for n in ("time_k", "time_v"):
        assert ref64[n][0].abs().max() > 1e-3 * ref64[n].abs().max()  # the rule has something to zero
        assert got[n][0].abs().max() == 0
        for r in (ref64, ref32):
            r[n] = r[n].clone()
            r[n][0] = 0
    bad = _failures("ops", got, ref64, ref32, names)
    assert not bad, "; ".join(bad)


def test_the_operator_and_the_c_abi_name_the_limit_they_refuse():
    c = TC._case((2, 16, 32), 7)
    p, draws = TC.problem(c), F.torch_draws(c.base)
    x = _dev(p)
    mask = A.StructuredMask(p.pr.kv.to(DEV), causal=True)
    index = p.index.to(DEV)
    kw = {k: x[k] for k in ("w_order", "b_order", "w_dist", "b_dist", "scalar", "pos_k", "pos_v")}
    handles = lambda idx=index, tab=x: dict(time_k=A.TimeIntervals(tab["time_k"], idx), time_v=A.TimeIntervals(tab["time_v"], idx))
    args = lambda t=x: (t["q"], t["k"], t["v"], t["qa"], t["ka"], t["gl"])

    def refused(match, *a, **k):
        with pytest.raises(ValueError, match=match):
            A.timeaware_attention(*a, **k)

    refused("dense masks", *args(), p.pr.mask_dense.to(DEV).contiguous(), A.AttentionConfig(n_heads=2), **kw, **handles())
    for combine in ("fixed", "annealing"):
        refused("gate", *args(), mask, A.AttentionConfig(n_heads=2, combine_option=combine), **kw, **handles())
    refused("two_level", *args(), mask, A.AttentionConfig(n_heads=2, two_level=False), **kw, **handles())
    refused("int32", *args(), mask, A.AttentionConfig(n_heads=2), **kw, **handles(idx=index.long()))
    wide = {"time_k": torch.zeros(2000, 32, device=DEV), "time_v": torch.zeros(2000, 32, device=DEV)}
    refused("time_span", *args(), mask, A.AttentionConfig(n_heads=2), **kw, **handles(tab=wide))
    long = {k: torch.zeros(2, 65, 32, device=DEV) for k in ("q", "k", "v", "qa", "ka")}
    long["gl"] = torch.zeros(2, 65, 65, device=DEV)
    refused("L <= 64", *args(long), A.StructuredMask(torch.ones(2, 65, dtype=torch.uint8, device=DEV)),
            A.AttentionConfig(n_heads=2), **dict(kw, pos_k=long["q"], pos_v=long["q"]),
            **handles(idx=torch.zeros(2, 65, 65, dtype=torch.int32, device=DEV)))
    # and the C ABI: -1 with a text, never another kernel
    lib = _lib.load()
    prob, text, hold = _fill(c, p, x, draws=draws)
    out = _lib.FwdOut()
    prob.two_level = 0
    assert lib.acattn_timeaware_attention_fwd(C.byref(prob), C.byref(text), C.byref(out), None) == -1
    assert b"two_level" in lib.acattn_last_error()
    prob.two_level = 1
    text.time_span = 0
    assert lib.acattn_timeaware_attention_fwd(C.byref(prob), C.byref(text), C.byref(out), None) == -1
    assert b"time_span" in lib.acattn_last_error()
