"""GPU suite (-m gpu): the backward of the SPATIAL-ONLY attention operator (acattn_spatial_attention_bwd,
csrc/acattn_bwd_spatial.hip) against the oracle differentiated by torch autograd in FLOAT64.

Reference: O.spatial_errors(q, k, p, cfg, materialize=False) -> softmax(z / sqrt(dh) + mask) -> O._drop with the kernel's
own keep bits (A.materialize_randomness(...).keep_after) -> O.context_only, loss = sum(ctx * G) with a seeded random G
(recbole/model/layers.py:695-740, 677-680).  Compared: dq, dk, dv, dw_order, db_order, dw_dist, db_dist, dscalar, each as
e = max|got - ref64| / max|ref64|.  Inputs as tests/test_hip_onehop.py::_problem draws them, seed 404.

Bounds.  Tensor-valued gradients (dq, dk, dv, dw_order, dw_dist): e <= max(1e-4, 2 * e32) and in any case e <= 2e-3, where
e32 is the error of the same oracle run in float32 on the CPU against the float64 one on the same inputs (1e-4 of scale
against fp64: VERDICT.md next-round item 6; 2 * e32: the margin tests/test_hip_ce.py grants a kernel over the fp32
restatement of its arithmetic; 2e-3: the cap of every gradient test, tests/test_hip_backward.py).  The three
single-number gradients (db_order, db_dist, dscalar) are cancelling sums over B * h * L^2 terms whose "scale" is the value
itself: e <= 2e-3 only.

Fully masked query rows (the left-padded sequence under the causal mask) follow the reference's fp32 `+ (-10000)`
quantisation, which a float64 oracle does not reproduce: those rows get a zero cotangent in the fp64 comparison and are
checked on their own against the float32 oracle at the 2e-3 cap.  The measured figures are printed per case and gradient
(profiles/spatial_bwd_accuracy.txt holds a run).
"""
import math

import pytest
import torch

import ac_tsr_amd as A
from ac_tsr_amd import attn_launch, dispatch, ops  # noqa: F401  (dispatch: registers torch.ops.acattn.*)
from oracle import ac_tsr_ref as O
from tests._attention_fp64 import default_dtype as _default_dtype, err as _err  # shared with test_hip_attention_bwd_fp64.py

pytestmark = pytest.mark.gpu
DEV = "cuda"
TENSOR_GRADS = ("q", "k", "v", "w_order", "w_dist")
SCALAR_GRADS = ("b_order", "b_dist", "scalar")


def _problem(B, L, H, nh, seed, causal=True, scale=0.3, left_pad=False):
    """tests/test_hip_onehop.py::_problem, draw for draw (qa / ka / the gate are drawn and not used)."""
    g = torch.Generator().manual_seed(seed)
    t = {k: torch.randn(B, L, H, generator=g) for k in ("q", "k", "v", "qa", "ka")}
    t["gl"] = torch.randn(B, L, L, generator=g)
    dh = H // nh
    for k, shp in (("w_order", (1, 2 * dh)), ("b_order", (1,)), ("w_dist", (1, 2 * dh)), ("b_dist", (1,)), ("scalar", (1,))):
        t[k] = scale * torch.randn(*shp, generator=g)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0] = L
    kv = (torch.arange(L)[None, :] < lens[:, None]).to(torch.uint8)
    if left_pad:
        kv[1] = 1 - kv[1]
    return t, kv, lens, g


def _leaf_names(terms):
    return ["q", "k", "v"] + (["w_order", "b_order"] if "order" in terms else []) + \
        (["w_dist", "b_dist", "scalar"] if "distance" in terms else [])


def _oracle_grads(t, mask, keep, p_drop, nh, terms, G, dtype):
    """Gradients of sum(ctx * G) by torch autograd over the oracle's own functions, in `dtype`, on the CPU."""
    names = _leaf_names(terms)
    with _default_dtype(dtype):
        x = {k: t[k].to(dtype).clone().requires_grad_(True) for k in names}
        B, L, H = t["q"].shape
        cfg = O.EncoderCfg(n_layers=1, n_heads=nh, hidden_size=H, inner_size=4 * H, use_order="order" in terms,
                           use_distance="distance" in terms, attn_dropout_prob=p_drop, seq_length=L)
        p = {}
        if "order" in terms:
            p.update({"attack_attention.order_affine.weight": x["w_order"], "attack_attention.order_affine.bias": x["b_order"]})
        if "distance" in terms:
            p.update({"attack_attention.distance_affine.weight": x["w_dist"], "attack_attention.distance_affine.bias": x["b_dist"],
                      "attack_attention.scalar": x["scalar"]})
        q = O._heads(x["q"], nh).permute(0, 2, 1, 3)
        k = O._heads(x["k"], nh).permute(0, 2, 1, 3)
        v = O._heads(x["v"], nh).permute(0, 2, 1, 3)
        e_order, e_dist = O.spatial_errors(q, k, p, cfg, materialize=False)
        z = torch.matmul(q, k.transpose(-1, -2)) + e_order + e_dist
        prob = torch.softmax(z / math.sqrt(H // nh) + mask.to(dtype), dim=-1)
        prob = O._drop(prob, None if keep is None else keep.to(dtype), p_drop)
        ctx = O.context_only(prob, v)
        grads = torch.autograd.grad((ctx * G.to(dtype)).sum(), [x[n] for n in names])
    return dict(zip(names, grads))


def _kernel_grads(t, mask_dev, nh, terms, p_drop, G, seed=None, rnd=None, read_rows=None, twice=False):
    names = _leaf_names(terms)
    x = {k: t[k].to(DEV).requires_grad_(True) for k in names}
    cal = {}
    if "order" in terms:
        cal.update(w_order=x["w_order"], b_order=x["b_order"])
    if "distance" in terms:
        cal.update(w_dist=x["w_dist"], b_dist=x["b_dist"], scalar=x["scalar"])
    cfg = A.AttentionConfig(n_heads=nh, combine_option="gate", adversarial=False)
    att, ctx, M, _ = A.calibrated_attention(x["q"], x["k"], x["v"], None, None, None, mask_dev, cfg, p_drop=p_drop, seed=seed,
                                            rnd=rnd, read_rows=read_rows, **cal)
    assert att is None and M is None
    loss = (ctx * G.to(DEV)).sum()
    leaves = [x[n] for n in names]
    first = torch.autograd.grad(loss, leaves, retain_graph=twice)
    out = {n: g.detach().cpu() for n, g in zip(names, first)}
    if twice:
        second = torch.autograd.grad(loss, leaves)
        return out, {n: g.detach().cpu() for n, g in zip(names, second)}
    return out


def _setup(B, L, H, nh, mask_kind, causal, left_pad, p_drop, scale, rng):
    t, kv, lens, g = _problem(B, L, H, nh, seed=404, causal=causal, scale=scale, left_pad=left_pad)
    dense = O.attention_mask(kv.to(torch.int64), bidirectional=not causal)  # [B,1,L,L] causal / [B,1,1,L] bidirectional
    if mask_kind == "structured":
        mask_dev = A.StructuredMask(kv.to(DEV), causal=causal)
    else:
        assert dense.shape == ((B, 1, L, L) if mask_kind == "dense_LL" else (B, 1, 1, L))
        mask_dev = dense.to(DEV).contiguous()
    seed, keep, rnd = 4040, None, None
    if p_drop > 0:
        keep_dev = A.materialize_randomness(B, nh, L, seed, p_drop, DEV).keep_after  # the kernel's own counter draws
        keep = keep_dev.cpu().float()
        if rng == "explicit":
            rnd = A.ExplicitRandomness(keep_after=keep_dev)
    G = torch.randn(B, L, H, generator=g)
    # query rows without any allowed key: every entry of their mask row is the fill value
    dead = (dense.expand(B, 1, L, L) == 0).sum(-1).squeeze(1) == 0  # [B, L]
    return t, kv, lens, dense, mask_dev, seed, keep, rnd, G, dead


CASES = [
    # id, B, L, H, heads, mask, causal, left_pad, p_drop, scale, rng, terms
    ("bench_shape_p05", 512, 50, 64, 2, "structured", True, True, 0.5, 0.3, "counter", ("order", "distance")),
    ("bench_shape_p0", 512, 50, 64, 2, "structured", True, True, 0.0, 0.3, "counter", ("order", "distance")),
    ("bidirectional", 64, 50, 64, 2, "structured", False, False, 0.5, 0.3, "counter", ("order", "distance")),
    ("cfg4_shape", 16, 200, 128, 4, "structured", True, False, 0.5, 0.3, "counter", ("order", "distance")),
    ("dh128_dense_L_bidirectional", 8, 200, 256, 2, "dense_L", False, False, 0.0, 0.1, "counter", ("order", "distance")),
    ("dh16_dense_LL_L37_explicit_keep", 8, 37, 64, 4, "dense_LL", True, False, 0.5, 0.3, "explicit", ("order", "distance")),
    ("order_only", 8, 50, 64, 2, "structured", True, False, 0.0, 0.3, "counter", ("order",)),
    ("distance_only", 8, 50, 64, 2, "structured", True, False, 0.0, 0.3, "counter", ("distance",)),
]


@pytest.mark.parametrize("B,L,H,nh,mask_kind,causal,left_pad,p_drop,scale,rng,terms", [c[1:] for c in CASES],
                         ids=[c[0] for c in CASES])
def test_gradients_match_the_fp64_oracle(B, L, H, nh, mask_kind, causal, left_pad, p_drop, scale, rng, terms, request):
    t, kv, lens, dense, mask_dev, seed, keep, rnd, G, dead = _setup(B, L, H, nh, mask_kind, causal, left_pad, p_drop, scale, rng)
    live = (~dead).unsqueeze(-1).to(G.dtype)
    G_live = G * live  # fully masked rows: zero cotangent here, checked below
    got, again = _kernel_grads(t, mask_dev, nh, terms, p_drop, G_live, seed=None if rnd is not None else seed, rnd=rnd, twice=True)
    ref64 = _oracle_grads(t, dense, keep, p_drop, nh, terms, G_live, torch.float64)
    ref32 = _oracle_grads(t, dense, keep, p_drop, nh, terms, G_live, torch.float32)
    case = request.node.callspec.id
    failures = []
    for n in _leaf_names(terms):
        e, e32 = _err(got[n], ref64[n]), _err(ref32[n], ref64[n])
        print(f"spatial_bwd_accuracy case={case} grad=d{n} e={e:.3e} e32={e32:.3e}")
        bound = min(max(1e-4, 2 * e32), 2e-3) if n in TENSOR_GRADS else 2e-3
        if not e <= bound:
            failures.append(f"d{n}: e = {e:.3e} > {bound:.3e} (e32 = {e32:.3e})")
    assert not failures, f"{case}: " + "; ".join(failures)
    # re-entrancy and no float atomics on the activations' gradients: a second walk gives the same bits
    for n in ("q", "k", "v"):
        assert torch.equal(got[n], again[n]), f"d{n} differs between two walks of the same graph"
    assert dead.any() == (left_pad and causal)
    if dead.any():
        # the fully masked rows alone, against the float32 oracle (it quantises them like the reference)
        G_dead = G * dead.unsqueeze(-1).to(G.dtype)
        got_d = _kernel_grads(t, mask_dev, nh, terms, p_drop, G_dead, seed=None if rnd is not None else seed, rnd=rnd)
        ref_d = _oracle_grads(t, dense, keep, p_drop, nh, terms, G_dead, torch.float32)
        bad = []
        for n in _leaf_names(terms):
            e = _err(got_d[n], ref_d[n])
            print(f"spatial_bwd_accuracy case={case} fully_masked_rows grad=d{n} e_vs_fp32={e:.3e}")
            if not e <= 2e-3:
                bad.append(f"d{n}: {e:.3e}")
        assert not bad, f"{case}, fully masked rows against the fp32 oracle (cap 2e-3): " + "; ".join(bad)


def test_read_rows_changes_nothing_when_the_cotangent_is_zero_elsewhere():
    B, L, H, nh = 64, 200, 128, 4
    t, kv, lens, dense, mask_dev, seed, keep, rnd, G, dead = _setup(B, L, H, nh, "structured", True, False, 0.5, 0.3, "counter")
    rows = (lens - 1).view(-1, 1)
    G_rows = torch.zeros(B, L, H).scatter_(1, rows.unsqueeze(-1).expand(-1, -1, H), G[:, :1])
    terms = ("order", "distance")
    full = _kernel_grads(t, mask_dev, nh, terms, 0.5, G_rows, seed=seed)
    hinted = _kernel_grads(t, mask_dev, nh, terms, 0.5, G_rows, seed=seed, read_rows=rows.to(DEV))
    for n in _leaf_names(terms):
        assert _err(hinted[n], full[n]) <= 1e-6, n
    ref64 = _oracle_grads(t, dense, keep, 0.5, nh, terms, G_rows, torch.float64)
    for n in TENSOR_GRADS:
        assert _err(hinted[n], ref64[n]) <= 2e-3, n


@pytest.mark.parametrize("terms", [("order", "distance"), ("order",), ("distance",)], ids=["both", "order_only", "distance_only"])
def test_poisoned_outputs_are_fully_written(terms, monkeypatch):
    """ACATTN_POISON_OUTPUTS=1: every output buffer starts as NaN; a disabled term's partial columns, the spare column and
    the dq rows of skipped query blocks must have been written (as zeros)."""
    monkeypatch.setenv("ACATTN_POISON_OUTPUTS", "1")
    monkeypatch.setattr(attn_launch, "POISON", True)
    B, L, H, nh = 8, 50, 64, 2
    t, kv, lens, dense, mask_dev, seed, keep, rnd, G, dead = _setup(B, L, H, nh, "structured", True, True, 0.5, 0.3, "counter")
    rows = (lens - 1).view(-1, 1)
    G_rows = torch.zeros(B, L, H).scatter_(1, rows.unsqueeze(-1).expand(-1, -1, H), G[:, :1])
    for G_use, rr in ((G, None), (G_rows, rows.to(DEV))):
        got = _kernel_grads(t, mask_dev, nh, terms, 0.5, G_use, seed=seed, read_rows=rr)
        for n, g in got.items():
            assert torch.isfinite(g).all(), f"d{n} holds unwritten (NaN) elements"
    # the raw partial buffer of the C ABI, spare column included
    import ctypes as C
    from ac_tsr_amd import _lib
    dev = {k: v.to(DEV) for k, v in t.items()}
    wo = dev["w_order"].reshape(-1) if "order" in terms else None
    wd = dev["w_dist"].reshape(-1) if "distance" in terms else None
    prob = ops._fill_problem(dev["q"], dev["k"], dev["v"], None, None, None, mask_dev, wo, dev["b_order"] if wo is not None else None,
                             wd, dev["b_dist"] if wd is not None else None, dev["scalar"] if wd is not None else None, None,
                             A.AttentionConfig(n_heads=nh, adversarial=False), 0.5, None, seed, [])
    dq, dk, dv, part = ops.spatial_attention_bwd_launch(_lib.load(), prob, dev["q"], G.to(DEV), nh, None, poison=True)
    torch.cuda.synchronize()
    assert all(torch.isfinite(x).all() for x in (dq, dk, dv, part))
    dh = H // nh
    assert (part[:, 4 * dh + 3] == 0).all()
    if "order" not in terms:
        assert (part[:, :2 * dh] == 0).all() and (part[:, 4 * dh] == 0).all()
    if "distance" not in terms:
        assert (part[:, 2 * dh:4 * dh] == 0).all() and (part[:, 4 * dh + 1:4 * dh + 3] == 0).all()


def test_dispatcher_form_and_direct_c_abi_form_agree(monkeypatch):
    B, L, H, nh = 32, 50, 64, 2
    t, kv, lens, dense, mask_dev, seed, keep, rnd, G, dead = _setup(B, L, H, nh, "structured", True, True, 0.5, 0.3, "counter")
    terms = ("order", "distance")
    monkeypatch.setattr(ops, "USE_DISPATCHER", True)
    via_op = _kernel_grads(t, mask_dev, nh, terms, 0.5, G, seed=seed)
    monkeypatch.setattr(ops, "USE_DISPATCHER", False)
    direct = _kernel_grads(t, mask_dev, nh, terms, 0.5, G, seed=seed)
    for n in ("q", "k", "v"):
        assert torch.equal(via_op[n], direct[n]), n  # the same kernels on the same inputs: the same bits
    for n in ("w_order", "b_order", "w_dist", "b_dist", "scalar"):  # (partials are summed with float atomics)
        assert _err(via_op[n], direct[n]) <= 1e-5, n


def test_raw_dispatcher_operator_carries_an_autograd_formula():
    """torch.ops.acattn.calibrated_attention_fwd(adversarial=False) differentiates through acattn::spatial_attention_bwd."""
    B, L, H, nh = 16, 50, 64, 2
    t, kv, lens, dense, mask_dev, seed, keep, rnd, G, dead = _setup(B, L, H, nh, "structured", True, False, 0.5, 0.3, "counter")
    names = _leaf_names(("order", "distance"))
    x = {k: t[k].to(DEV).requires_grad_(True) for k in names}
    outs = torch.ops.acattn.calibrated_attention_fwd(
        x["q"], x["k"], x["v"], None, None, None, kv.to(DEV), True, x["w_order"].reshape(-1), x["b_order"],
        x["w_dist"].reshape(-1), x["b_dist"], x["scalar"], nh, 0.5, seed, None, False, None, False)
    grads = torch.autograd.grad((outs[1] * G.to(DEV)).sum(), [x[n] for n in names])
    ref = _kernel_grads(t, mask_dev, nh, ("order", "distance"), 0.5, G, seed=seed)
    for n, g in zip(names, grads):
        assert _err(g.cpu().reshape(ref[n].shape), ref[n]) <= 1e-5, n


def test_the_adversarial_entry_point_still_refuses_the_spatial_only_problem():
    import ctypes as C
    from ac_tsr_amd import _lib
    lib = _lib.load()
    p = _lib.Problem()
    p.B, p.L, p.H, p.n_heads = 2, 50, 64, 2
    x = torch.zeros(2, 50, 64, device=DEV)
    kvd = torch.ones(2, 50, dtype=torch.uint8, device=DEV)
    p.q = p.k = p.v = C.c_void_p(x.data_ptr())
    p.key_valid, p.mask_mode, p.rng_mode = C.c_void_p(kvd.data_ptr()), _lib.MASK_STRUCTURED, _lib.RNG_COUNTER
    assert lib.acattn_calibrated_attention_bwd(C.byref(p), C.byref(_lib.BwdIO()), None) < 0
    assert b"adversarial (full) operator only" in lib.acattn_last_error()
