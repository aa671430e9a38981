"""GPU suite (-m gpu): the un-normalised attention core of ACSSEPT (csrc/acattn_unnorm.hip) through the C ABI
(acattn_unnorm_attention_fwd / _bwd) and through ops.calibrated_attention(renormalise=False).

Reference: tests/_unnorm_ref.py::core_from_projected_unnorm in FLOAT64 on the CPU (tests/_unnorm_cases.py), fed the very
draws the kernels use.  Bounds are the project's (tests/_attention_fp64.py): with e = max|got - ref64| / max|ref64| and e32
the same figure of the float32 oracle, a tensor is held to min(max(1e-4, 2 e32), 2e-3) of its own maximum (ctx_attacked is
O(sqrt(L) |V|): every tolerance is relative), the single-number gradients to 2e-3, each with the absolute floor 1e-7.  ALL
rows of the forward are compared, the rows without an allowed key (left padding under the causal mask) included: for them
the float64 oracle is the yardstick, the kernel drops the mask's common -10000 and does not reproduce the reference's fp32
rounding of `score - 10000` (the fp32 oracle itself is 0.5-1.6e-4 of scale off its float64 self there).
"""
import ctypes as C

import pytest
import torch

import ac_tsr_amd as A
from ac_tsr_amd import _lib, attn_launch
from tests import _attention_fp64 as F
from tests import _unnorm_cases as UC

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 4242
_PROBLEMS, _FORWARD, _BACKWARD = {}, {}, {}


def _problem(c):
    key = UC.forward_key(c)._replace(pattern=c.pattern)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = (F.problem(c), F.torch_draws(c))
    return _PROBLEMS[key]


def _dev(pr):
    return {k: v.to(DEV).contiguous() for k, v in pr.t.items()}


def _fill(c, pr, x, draws=None, seed=None, seed_tensor=None, noise=None):
    """acattn_problem for case `c`; explicit draws (`draws`: CPU dict, `noise` overrides its noise tensor) or the counter
    RNG.  Returns (problem, tensors to keep alive)."""
    keep = [pr.kv.to(DEV).contiguous()]
    rnd = None
    if draws is not None:
        u8 = lambda t: None if t is None else t.to(torch.uint8).to(DEV).contiguous()
        rnd = (draws["noise"].to(DEV).contiguous() if noise is None else noise, u8(draws["keep_after"]), u8(draws["keep_mask"]), None)
        keep += [t for t in rnd if t is not None]
    flat = [x[k].reshape(-1) if k.startswith("w_") else x[k] for k in ("w_order", "b_order", "w_dist", "b_dist", "scalar")]
    prob = attn_launch.fill_problem(x["q"], x["k"], x["v"], x["qa"], x["ka"], x["gl"], *flat, c.nh, c.p_drop, seed or 0,
                                    seed_tensor, key_valid=keep[0], causal=c.causal, rnd=rnd)
    return prob, keep + flat


def _forward(c, pr, x, poison=False, **kw):
    prob, keep = _fill(c, pr, x, **kw)
    ctx_a, ctx_c, M, stats, pen = attn_launch.unnorm_attention_fwd_launch(_lib.load(), prob, x["q"], c.nh, want_penalty=True,
                                                                          poison=poison)
    torch.cuda.synchronize()
    return {"ctx_attacked": ctx_a, "ctx_calibrated": ctx_c, "M": M, "stats": stats, "pen": pen}


def _backward(c, pr, x, fwd, cot, poison=False, d_pen=None, hints=False, **kw):
    """{leaf: gradient} (CPU) of sum_k out_k cot_k through acattn_unnorm_attention_bwd; an output without a cotangent is
    passed as NULL."""
    prob, keep = _fill(c, pr, x, **kw)
    dc = {k: v.to(DEV).contiguous() for k, v in cot.items()}
    res = attn_launch.unnorm_attention_bwd_launch(
        _lib.load(), prob, x["q"], c.nh, fwd["M"], fwd["stats"], d_att=dc.get("ctx_attacked"), d_cal=dc.get("ctx_calibrated"),
        d_M=dc.get("M"), d_pen=d_pen, read_rows=pr.rows.to(DEV).contiguous() if hints else None,
        attack_only=hints and "ctx_calibrated" not in cot, poison=poison)
    torch.cuda.synchronize()
    dq, dk, dv, dqa, dka, dgate, part = res
    dh = c.H // c.nh
    tot = part.sum(0)
    g_wo, g_bo, g_wd, g_bd, g_sc, _ = attn_launch.unpack_partials(tot, dh, pr.t["w_order"], pr.t["b_order"], pr.t["w_dist"],
                                                                  pr.t["b_dist"], pr.t["scalar"])
    out = dict(q=dq, k=dk, v=dv, qa=dqa, ka=dka, gl=dgate.sum(1), w_order=g_wo, b_order=g_bo, w_dist=g_wd, b_dist=g_bd, scalar=g_sc)
    raw = dict(dq=dq, dk=dk, dv=dv, dqa=dqa, dka=dka, dgate=dgate, part=part)
    return {k: v.detach().cpu() for k, v in out.items()}, raw


def _failures(tag, got, ref64, ref32, names, scalar=()):
    bad = []
    for n in names:
        abs_e, scale = F.abs_err_and_scale(got[n], ref64[n])
        abs_e32, _ = F.abs_err_and_scale(ref32[n], ref64[n])
        e, e32 = (abs_e / scale, abs_e32 / scale) if scale > 0 else (abs_e, abs_e32)
        bound = F.SCALAR_BOUND if n in scalar else F.tensor_bound(e32)
        print(f"unnorm_accuracy {tag} {n} e={e:.3e} e32={e32:.3e} bound={bound:.1e} scale={scale:.3e}")
        if not abs_e <= bound * scale + F.ABS_FLOOR:
            bad.append(f"{n}: e = {e:.3e} > {bound:.3e} (e32 = {e32:.3e}, scale {scale:.3e})")
    return bad


def _cpu(outs):
    return {k: outs[k].detach().cpu() for k in UC.OUTPUTS}


_FWD_CASES = list({UC.forward_key(c): c for c in reversed(UC.CASES)}.values())[::-1]  # one case per forward problem


@pytest.mark.parametrize("case", _FWD_CASES, ids=lambda c: c.id)
def test_forward_matches_the_fp64_oracle_on_every_row(case):
    c = case
    pr, draws = _problem(c)
    got = _forward(c, pr, _dev(pr), draws=draws)
    _, ref64 = UC.oracle(c, pr, draws, {}, torch.float64)
    _, ref32 = UC.oracle(c, pr, draws, {}, torch.float32)
    bad = _failures(f"case={c.id} fwd", _cpu(got), ref64, ref32, UC.OUTPUTS)
    assert not bad, f"{c.id}: " + "; ".join(bad)
    # the penalty rows are the sums of (1 - M)^2 the attacked loss needs
    pen = ((1 - ref64["M"]) ** 2).sum(-1)
    pad = (-c.L) % 16
    pen = torch.nn.functional.pad(pen, (0, pad)).view(c.B, c.nh, -1, 16).sum(-1)
    assert F.err(got["pen"].cpu(), pen) <= 1e-5


@pytest.mark.parametrize("case", UC.CASES, ids=lambda c: c.id)
def test_backward_matches_the_fp64_oracle(case):
    c = case
    pr, draws = _problem(c)
    x = _dev(pr)
    fwd = _forward(c, pr, x, draws=draws)
    got, _ = _backward(c, pr, x, fwd, pr.cot, draws=draws, hints=c.pattern in F.READ_ROW_PATTERNS)
    ref64, _ = UC.oracle(c, pr, draws, pr.cot, torch.float64)
    ref32, _ = UC.oracle(c, pr, draws, pr.cot, torch.float32)
    bad = _failures(f"case={c.id} bwd", got, ref64, ref32, F.leaf_names(c), scalar=F.SCALAR_GRADS)
    assert not bad, f"{c.id}: " + "; ".join(bad)


@pytest.mark.parametrize("case", [c for c in UC.CASES if c.left_pad], ids=lambda c: c.id)
def test_backward_of_rows_without_an_allowed_key(case):
    """The cotangents of the left-padded sequence's dead rows alone, against the float64 oracle (which takes their soft-max
    over all L keys, as the kernel does)."""
    c = case
    pr, draws = _problem(c)
    assert pr.dead.any()
    x = _dev(pr)
    fwd = _forward(c, pr, x, draws=draws)
    got, _ = _backward(c, pr, x, fwd, pr.cot_dead, draws=draws)
    ref64, _ = UC.oracle(c, pr, draws, pr.cot_dead, torch.float64)
    ref32, _ = UC.oracle(c, pr, draws, pr.cot_dead, torch.float32)
    bad = _failures(f"case={c.id} bwd_dead_rows", got, ref64, ref32, F.leaf_names(c), scalar=F.SCALAR_GRADS)
    assert not bad, f"{c.id}: " + "; ".join(bad)


_COUNTER_CASES = [c for c in UC.CASES if c.pattern == "all" and not c.left_pad and c.causal]


@pytest.mark.parametrize("case", _COUNTER_CASES, ids=lambda c: c.id)
def test_counter_rng_uses_the_materialised_draws(case):
    c = case
    pr, _ = _problem(c)
    x = _dev(pr)
    counter = torch.tensor([3], dtype=torch.int64, device=DEV)
    for seed, seed_tensor, effective in ((SEED, None, SEED), (SEED, counter, SEED + 3)):
        rnd = A.materialize_randomness(c.B, c.nh, c.L, effective, c.p_drop, DEV)
        draws = {"noise": rnd.noise.cpu(), "keep_after": None, "keep_mask": None, "keep_before": None}
        if c.p_drop > 0:
            draws.update(keep_after=rnd.keep_after.cpu().float(), keep_mask=rnd.keep_mask.cpu().float())
        fwd = _forward(c, pr, x, seed=seed, seed_tensor=seed_tensor)
        got, _ = _backward(c, pr, x, fwd, pr.cot, seed=seed, seed_tensor=seed_tensor)
        ref64g, ref64 = UC.oracle(c, pr, draws, pr.cot, torch.float64)
        ref32g, ref32 = UC.oracle(c, pr, draws, pr.cot, torch.float32)
        tag = f"case={c.id} counter seed_device={seed_tensor is not None}"
        bad = _failures(tag + " fwd", _cpu(fwd), ref64, ref32, UC.OUTPUTS)
        bad += _failures(tag + " bwd", got, ref64g, ref32g, F.leaf_names(c), scalar=F.SCALAR_GRADS)
        assert not bad, f"{c.id}: " + "; ".join(bad)
        # an EXPLICIT launch on the materialised draws is the COUNTER launch
        fwd_e = _forward(c, pr, x, draws=draws)
        got_e, _ = _backward(c, pr, x, fwd_e, pr.cot, draws=draws)
        for k in UC.OUTPUTS:
            assert F.err(fwd_e[k], fwd[k]) <= 1e-6, k
        for n in F.leaf_names(c):
            assert F.err(got_e[n], got[n]) <= 1e-6, n


def _case(shape, **kw):
    kw.setdefault("pattern", "all")
    return F._case("adhoc", "unnorm", shape, **kw)


def test_noise_reaches_masked_and_padded_keys():
    """A_att = N where M = 0: V at a PADDED position of a right-padded sequence moves ctx_attacked of an earlier valid row by
    N_ij times the change, and ctx_calibrated (P = 0 there) not at all.  The normalised core would not move either."""
    c = _case((3, 37, 64, 2), p_drop=0.0)
    pr, draws = _problem(c)
    b = int(torch.argmin(pr.lens))
    j, i = int(pr.lens[b]), 0  # the first padded position, the first row
    assert j < c.L and pr.kv[b, i] == 1 and pr.kv[b, j] == 0
    x = _dev(pr)
    base = _forward(c, pr, x, draws=draws)
    x2 = dict(x)
    x2["v"] = x["v"].clone()
    x2["v"][b, j, :] += 1.0
    moved = _forward(c, pr, x2, draws=draws)
    delta = (moved["ctx_attacked"] - base["ctx_attacked"])[b, i].cpu().view(c.nh, -1)
    expect = draws["noise"][b, :, i, j].view(c.nh, 1).expand_as(delta)  # M_ij = 0: the weight of key j is N_ij
    assert (delta - expect).abs().max() <= 1e-5 * max(1.0, base["ctx_attacked"].abs().max().item())
    assert expect.abs().min() > 1e-3  # (the draws at that place are not tiny: the shift is visible)
    assert torch.equal(moved["ctx_calibrated"], base["ctx_calibrated"])
    assert torch.equal(moved["M"], base["M"])


@pytest.mark.parametrize("L", (17, 49))
def test_tile_padding_columns_contribute_nothing_and_every_element_is_written(L):
    """The noise rows are cut from a larger buffer whose neighbouring memory holds 1e30: nothing past a row's L floats is
    read into a result (bitwise), forward and backward.  And with NaN-prefilled outputs every element is written."""
    c = _case((2, L, 64, 2))
    pr, draws = _problem(c)
    x = _dev(pr)
    big = torch.full((c.B * c.nh * L * L + 4096,), 1e30, device=DEV)
    cut = big[2048:2048 + c.B * c.nh * L * L].view(c.B, c.nh, L, L)
    cut.copy_(draws["noise"])
    a = _forward(c, pr, x, draws=draws)
    b = _forward(c, pr, x, draws=draws, noise=cut, poison=True)
    for k in ("ctx_attacked", "ctx_calibrated", "M", "stats", "pen"):
        assert torch.isfinite(b[k]).all(), k
        assert torch.equal(a[k], b[k]), k
    assert a["ctx_attacked"].abs().max() < 1e4
    _, ra = _backward(c, pr, x, a, pr.cot, draws=draws)
    _, rb = _backward(c, pr, x, b, pr.cot, draws=draws, noise=cut, poison=True)
    for k in ra:
        assert torch.isfinite(rb[k]).all(), k
        assert torch.equal(ra[k], rb[k]), k


def test_penalty_cotangent_equals_the_dense_mask_cotangent_it_stands_for():
    c = _case((3, 50, 128, 2))
    pr, draws = _problem(c)
    x = _dev(pr)
    fwd = _forward(c, pr, x, draws=draws)
    d_pen = torch.rand(c.B, c.nh, (c.L + 15) // 16, device=DEV) + 0.5
    rows = d_pen.repeat_interleave(16, dim=2)[:, :, :c.L]
    dense = 2 * rows[..., None] * (fwd["M"] - 1)
    via_pen, _ = _backward(c, pr, x, fwd, {}, draws=draws, d_pen=d_pen)
    via_mask, _ = _backward(c, pr, x, fwd, {"M": dense}, draws=draws)
    for n in ("qa", "ka"):
        assert via_mask[n].abs().max() > 0
        assert F.err(via_pen[n], via_mask[n]) <= 1e-5, n
    for n in ("q", "k", "v", "gl"):
        assert via_pen[n].abs().max() <= F.ABS_FLOOR and via_mask[n].abs().max() <= F.ABS_FLOOR, n


@pytest.mark.parametrize("pattern", F.READ_ROW_PATTERNS)
def test_hints_do_not_change_what_they_promise(pattern):
    c = _case((3, 50, 128, 2), pattern=pattern)
    pr, draws = _problem(c)
    x = _dev(pr)
    fwd = _forward(c, pr, x, draws=draws)
    _, plain = _backward(c, pr, x, fwd, pr.cot, draws=draws)
    _, hinted = _backward(c, pr, x, fwd, pr.cot, draws=draws, hints=True)
    attack_only = "ctx_calibrated" not in pr.cot
    for k in (("dqa", "dka") if attack_only else tuple(plain)):
        assert torch.equal(plain[k], hinted[k]), k


def test_two_backward_launches_give_the_same_bits():
    c = _case((3, 50, 128, 2))
    pr, draws = _problem(c)
    x = _dev(pr)
    fwd = _forward(c, pr, x, draws=draws)
    _, one = _backward(c, pr, x, fwd, pr.cot, draws=draws)
    _, two = _backward(c, pr, x, fwd, pr.cot, draws=draws)
    for k in one:
        assert torch.equal(one[k], two[k]), k


def test_the_operator_routes_to_the_new_pair_and_can_be_walked_twice(monkeypatch):
    """ops.calibrated_attention(renormalise=False): gradients by autograd against the float64 oracle, two walks of one graph
    (the trainer's retain_graph=True) with equal bits, the penalty rows attached, and no launch of the normalised kernels."""
    def normalised(*a, **k):
        raise AssertionError("a normalised attention kernel was launched")

    monkeypatch.setattr(attn_launch, "attention_fwd_launch", normalised)
    monkeypatch.setattr(attn_launch, "attention_bwd_launch", normalised)
    c = _case((3, 50, 128, 2))
    pr, draws = _problem(c)
    names = F.leaf_names(c)
    x = {k: pr.t[k].to(DEV).requires_grad_(True) for k in names}
    u8 = lambda t: t.to(torch.uint8).to(DEV)
    rnd = A.ExplicitRandomness(noise=draws["noise"].to(DEV), keep_after=u8(draws["keep_after"]), keep_mask=u8(draws["keep_mask"]))
    cfg = A.AttentionConfig(n_heads=c.nh, renormalise=False)
    ctx_a, ctx_c, M, probs = A.calibrated_attention(
        x["q"], x["k"], x["v"], x["qa"], x["ka"], x["gl"], A.StructuredMask(pr.kv.to(DEV), causal=True), cfg, p_drop=c.p_drop,
        rnd=rnd, **{k: x[k] for k in names[6:]})
    assert probs == {} and M._acattn_pen.shape == (c.B, c.nh, 4)
    outs = {"ctx_attacked": ctx_a, "ctx_calibrated": ctx_c, "M": M}
    loss = sum((outs[k] * pr.cot[k].to(DEV)).sum() for k in pr.cot)
    leaves = [x[n] for n in names]
    first = torch.autograd.grad(loss, leaves, retain_graph=True)
    second = torch.autograd.grad(loss, leaves)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    got = {n: g.detach().cpu().reshape(pr.t[n].shape) for n, g in zip(names, first)}
    ref64, _ = UC.oracle(c, pr, draws, pr.cot, torch.float64)
    ref32, _ = UC.oracle(c, pr, draws, pr.cot, torch.float32)
    bad = _failures("ops", got, ref64, ref32, names, scalar=F.SCALAR_GRADS)
    assert not bad, "; ".join(bad)


def test_the_operator_names_the_limit_it_refuses():
    c = _case((2, 16, 32, 2))
    pr, _ = _problem(c)
    x = _dev(pr)
    mask = A.StructuredMask(pr.kv.to(DEV), causal=True)
    kw = {k: x[k] for k in ("w_order", "b_order", "w_dist", "b_dist", "scalar")}
    args = lambda t=x: (t["q"], t["k"], t["v"], t["qa"], t["ka"], t["gl"])

    def refused(match, *a, **k):
        with pytest.raises(ValueError, match=match):
            A.calibrated_attention(*a, **k)

    refused("dense masks", *args(), pr.mask_dense.to(DEV).contiguous(), A.AttentionConfig(n_heads=2, renormalise=False), **kw)
    refused("probability dumps", *args(), mask, A.AttentionConfig(n_heads=2, renormalise=False), want_probs=True, **kw)
    for combine in ("fixed", "annealing"):
        refused("gate", *args(), mask, A.AttentionConfig(n_heads=2, renormalise=False, combine_option=combine), **kw)
    refused("two_level", *args(), mask, A.AttentionConfig(n_heads=2, renormalise=False, two_level=False), **kw)
    refused("GPU", *args({k: v.cpu() for k, v in x.items()}), mask, A.AttentionConfig(n_heads=2, renormalise=False), **kw)
    long = {k: torch.zeros(2, 65, 32, device=DEV) for k in ("q", "k", "v", "qa", "ka")}
    long["gl"] = torch.zeros(2, 65, 65, device=DEV)
    refused("L <= 64", *args(long), A.StructuredMask(torch.ones(2, 65, dtype=torch.uint8, device=DEV)),
            A.AttentionConfig(n_heads=2, renormalise=False), **kw)
    # and the C ABI: -1 with a text, never another kernel
    lib = _lib.load()
    prob, keep = _fill(c, pr, x, seed=1)
    prob.two_level = 0
    out = _lib.FwdOut()
    assert lib.acattn_unnorm_attention_fwd(C.byref(prob), C.byref(out), None) == -1
    assert b"two_level" in lib.acattn_last_error()


def test_layer_0_of_the_reference_fixture_through_the_c_abi():
    """ssept_train (tensors of the genuine reference at the shipped shape: 64 + 64, 2 heads, L = 50, training mode): the
    projected tensors of its first layer, as tests/_unnorm_ref.py forms them, through acattn_unnorm_attention_fwd with the
    fixture's draws; contexts and M against the restatement the generator pinned to the reference."""
    from oracle import ac_tsr_ref as O
    from tests import _unnorm_ref as U
    from tests._ssept_golden import SseptCase

    c = SseptCase("ssept_train")
    P, cfg, rnds, b = c.params(), c.model_cfg(), c.layer_randomness(), c.batch()
    with torch.no_grad():
        _, _, masks, dbgs = U.model_forward(b["item_id_list"], b["item_length"], b["user_id"], P, cfg, rnds, c.keep_emb())
    d, p0 = dbgs[0], O.layer_params(P, "trm_encoder.layer.0.")
    mq, mk = d["mixed_query"], d["mixed_key"]
    B, L, H = mq.shape
    x = {"q": mq, "k": mk, "v": d["value"].permute(0, 2, 1, 3).reshape(B, L, H),
         "qa": O._lin(mq, p0, "attack_attention.attack_query_transform"), "ka": O._lin(mk, p0, "attack_attention.attack_key_transform"),
         "gl": O._lin(mq, p0, "gate"), "w_order": p0["attack_attention.order_affine.weight"],
         "b_order": p0["attack_attention.order_affine.bias"], "w_dist": p0["attack_attention.distance_affine.weight"],
         "b_dist": p0["attack_attention.distance_affine.bias"], "scalar": p0["attack_attention.scalar"]}
    case = F._case("ssept_train_layer0", "unnorm", (B, L, H, c.n_heads))
    pr = F.Problem(x, (b["item_id_list"] != 0).to(torch.uint8), b["item_length"], None, None, None, None, None)
    draws = {"noise": rnds[0].noise, "keep_after": rnds[0].keep_after, "keep_mask": rnds[0].keep_mask}
    got = _forward(case, pr, {k: v.to(DEV).contiguous() for k, v in x.items()}, draws=draws)
    for k, ref in (("ctx_attacked", d["ctx_attacked"]), ("ctx_calibrated", d["ctx_calibrated"]), ("M", masks[0])):
        e = F.err(got[k].cpu(), ref)
        print(f"unnorm_accuracy ssept_train layer0 {k} e={e:.3e} scale={ref.abs().max().item():.3e}")
        assert e <= F.TENSOR_FLOOR, k
