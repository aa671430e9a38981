"""The forward oracle of the calibrated attention core and the comparison of a launch with it, shared by
tests/test_hip_long_sequences.py, tests/test_hip_fwd_edges.py and the CPU check of the latter's case table
(tests/test_fwd_edge_cases_cpu.py).  Nothing here touches a GPU or imports the HIP package.

  oracle_forward   oracle/ac_tsr_ref.py::core_from_projected in a chosen dtype on the CPU, plus the natural-log normalisers
                   of its soft-maxes (what acattn_fwd_out.row_stats holds) and the spatial-only context (adversarial = 0:
                   one soft-max, one context, O.context_only).
  check_forward    the long-sequence module's comparison of live and fully masked rows (its bounds, unchanged).
  edge_problem     tests/_attention_fp64.problem's inputs with the four-sequence batch of the tile-edge cases: full length,
                   right-padded, left-padded, and one sequence with no valid key at all.
  edge_errors      the figures the tile-edge tests bound: live rows against the float64 oracle, fully masked rows against
                   the float32 one.
"""
import math

import torch

from oracle import ac_tsr_ref as O
from tests import _attention_fp64 as F

M_BOUND, CTX_BOUND, STAT_BOUND, DEAD_CAP = 5e-6, 1e-4, 1e-4, 2e-3
# a fully masked row's normalisers carry the -10000 of the mask: two fp32 roundings at that magnitude (ulp(1e4) = 2^-10)
DEAD_STAT_BOUND = 2 * 2.0 ** -10


def ocfg(c):
    return O.EncoderCfg(n_layers=1, n_heads=c.nh, hidden_size=c.H, inner_size=4 * c.H, combine_option=c.combine,
                        use_order="order" in c.terms, use_distance="distance" in c.terms, two_level=c.two_level,
                        rich_calibrated_combine=c.rich, seq_length=c.L, attn_dropout_prob=c.p_drop)


def oracle_forward(c, pr, draws, dtype):
    """core_from_projected in `dtype` plus the log-normalisers of its soft-maxes ([B, nh, L] each).

    `stats` [..., 0:5]: the spatial soft-max, the attack mask's, the attacked, the calibrated and the combined one; `lse_f`
    the inner, un-masked soft-max of combine `fixed` (else None); `lse_b` the plain soft-max that two_level = False
    builds on (else None); `ctx_spatial` the context of the spatial-only operator (adversarial = 0)."""
    with F.default_dtype(dtype), torch.no_grad():
        t = {k: v.to(dtype) for k, v in pr.t.items()}
        cast = lambda v: None if v is None else v.to(dtype)
        mask = pr.mask_dense.to(dtype)
        cfg = ocfg(c)
        kw = {k: t[k] if (("order" in k and cfg.use_order) or (k in ("w_dist", "b_dist", "scalar") and cfg.use_distance)) else None
              for k in ("w_order", "b_order", "w_dist", "b_dist", "scalar")}
        ref = O.core_from_projected(t["q"], t["k"], t["v"], t["qa"], t["ka"], t["gl"] if c.combine == "gate" else None, mask,
                                    kw["w_order"], kw["b_order"], kw["w_dist"], kw["b_dist"], kw["scalar"], cfg,
                                    cast(draws["noise"]), keep_after=cast(draws["keep_after"]), keep_mask=cast(draws["keep_mask"]),
                                    keep_before=cast(draws.get("keep_before")), anneal_rate=c.anneal_rate,
                                    rich_ratio=t["rich_ratio"] if not c.two_level and c.rich == "trainable" else None,
                                    materialize=False)
        heads = lambda x: O._heads(x, c.nh).permute(0, 2, 1, 3)
        q, k = heads(t["q"]), heads(t["k"])
        dh = c.H // c.nh
        p = {"attack_attention.order_affine.weight": kw["w_order"], "attack_attention.order_affine.bias": kw["b_order"],
             "attack_attention.distance_affine.weight": kw["w_dist"], "attack_attention.distance_affine.bias": kw["b_dist"],
             "attack_attention.scalar": kw["scalar"]}
        e_o, e_d = O.spatial_errors(q, k, p, cfg, materialize=False)
        lse = lambda x: torch.logsumexp(x, dim=-1)
        P, M = (ref["after"] if c.two_level else ref["before"]), ref["M"]
        raw = q @ k.transpose(-1, -2)
        stats = [lse((raw + e_o + e_d) / math.sqrt(dh) + mask),
                 lse(heads(t["qa"]) @ heads(t["ka"]).transpose(-1, -2) / math.sqrt(dh) + mask),
                 lse(P * M + cast(draws["noise"]) * (1 - M) + mask)]
        v_arg = P * torch.exp(1 - M) + mask
        stats.append(lse(v_arg))
        Ac = torch.softmax(v_arg, dim=-1)
        if c.combine == "fixed":
            inner = P + 0.5 * Ac
            comb, lse_f = torch.softmax(inner, dim=-1), lse(inner)
        else:
            g = torch.sigmoid(t["gl"]).unsqueeze(1) if c.combine == "gate" else c.anneal_rate
            comb, lse_f = g * P + (1 - g) * Ac, None
        stats.append(lse(comb + mask))
        ref["stats"], ref["lse_f"] = torch.stack(stats, dim=-1), lse_f
        ref["lse_b"] = None if c.two_level else lse(raw / math.sqrt(dh) + mask)
        ref["ctx_spatial"] = O.context_only(ref["after"], heads(t["v"]))
    return ref


def check_forward(c, pr, got, ref32, ref64, tag=""):
    """`got` = (ctx_attacked, ctx_calibrated, M, row_stats) as CPU tensors."""
    ctx_a, ctx_c, M, stats = got
    for name, t in (("ctx_attacked", ctx_a), ("ctx_calibrated", ctx_c), ("M", M), ("row_stats", stats[..., :5])):
        assert torch.isfinite(t).all(), f"{c.id}{tag}: {name} holds an element no kernel wrote (or a non-finite value)"
    live, dead = ~pr.dead, pr.dead  # [B, L]
    figures = {}
    for name, t, bound in (("M", M, M_BOUND), ("ctx_attacked", ctx_a, CTX_BOUND), ("ctx_calibrated", ctx_c, CTX_BOUND)):
        row = live[:, None, :, None] if name == "M" else live[:, :, None]
        e = ((t - ref32[name]).abs() * row).max().item()
        figures[name] = e
        assert e <= bound, f"{c.id}{tag}: {name} differs from the fp32 oracle by {e:.3e} > {bound:.0e}"
        if dead.any():
            drow = ~row
            scale = (ref32[name].abs() * drow).max().item()
            ed = ((t - ref32[name]).abs() * drow).max().item()
            figures[name + "_dead"] = ed
            assert ed <= DEAD_CAP * scale + F.ABS_FLOOR, f"{c.id}{tag}: fully masked rows of {name}: {ed:.3e} of {scale:.3e}"
    es = ((stats[..., :5].double() - ref64["stats"]).abs() * live[:, None, :, None]).max().item()
    figures["row_stats"] = es
    assert es <= STAT_BOUND, f"{c.id}{tag}: row_stats differ from the fp64 normalisers by {es:.3e}"
    if dead.any():
        ed = ((stats[..., :5].double() - ref64["stats"]).abs() * dead[:, None, :, None]).max().item()
        assert ed <= 2 * 2.0 ** -10 + STAT_BOUND, f"{c.id}{tag}: row_stats of fully masked rows: {ed:.3e}"
    if ref64["lse_f"] is not None:
        ef = (stats[..., 5].double() - ref64["lse_f"]).abs().max().item()
        assert ef <= STAT_BOUND, f"{c.id}{tag}: the inner soft-max's normaliser (combine fixed): {ef:.3e}"
    # what the fp32 oracle itself is from the fp64 one on these rows: the yardstick's own error next to the kernel's
    e32 = {n: ((ref32[n].double() - ref64[n]).abs() * (live[:, None, :, None] if n == "M" else live[:, :, None])).max().item()
           for n in ("M", "ctx_attacked", "ctx_calibrated")}
    print(f"long_sequences_accuracy case={c.id}{tag} " + " ".join(f"{k}={v:.3e}" for k, v in figures.items()) +
          " oracle32_vs_64: " + " ".join(f"{k}={v:.3e}" for k, v in e32.items()))


# ---- the tile-edge cases ------------------------------------------------------------------------------------------------------
def edge_key_valid(L):
    """[4, L] uint8: sequence 0 full length; 1 right-padded to about L / 2; 2 left-padded to about L / 3 (under the causal
    mask its first rows have no allowed key; a single position cannot be left-padded, so at L = 1 it is full); 3 without
    any valid key."""
    pos = torch.arange(L)
    n_right, n_left = max(1, L // 2), max(1, L // 3)
    left = pos >= L - n_left if L >= 2 else torch.ones(L, dtype=torch.bool)
    return torch.stack([torch.ones(L, dtype=torch.bool), pos < n_right, left, torch.zeros(L, dtype=torch.bool)]).to(torch.uint8)


def edge_dead_rows(L, causal):
    """[4, L] bool, from the layout alone (the CPU test holds the mask's own count against it): the rows in front of the
    left-padded sequence's first valid key under the causal mask, and every row of the sequence without a valid key."""
    dead = torch.zeros(4, L, dtype=torch.bool)
    dead[3] = True
    if causal and L >= 2:
        dead[2, :L - max(1, L // 3)] = True
    return dead


# The order affine's weights of the tile-edge cases (the distance term keeps its full scale), as a fraction of tests._attention_fp64.calibrator_scale.  At the full scale
# the order affine's argument has a standard deviation of 2.4 and reaches 12 somewhere in 4 x 2 x L x L draws, where fp32
# `1 - sigmoid(x)` keeps two digits: the float32 oracle's spatial soft-max was then up to 1.5e-4 from the float64 one
# (seed 606, L = 48), more than the bound the kernels are held to.  At half the scale it is within a quarter of every bound
# at every case (tests/test_fwd_edge_cases_cpu.py).
EDGE_CALIBRATOR_FRACTION = 0.5


def edge_problem(c, seed=606):
    """tests/_attention_fp64.problem's inputs (same generator, same order; the order affine at EDGE_CALIBRATOR_FRACTION)
    under edge_key_valid's four sequences."""
    assert c.B == 4
    base = F.problem(c._replace(left_pad=False), seed=seed)  # (its own `dead.any()` assertion holds: nothing is dead there)
    for name in ("w_order", "b_order"):
        base.t[name] = base.t[name] * EDGE_CALIBRATOR_FRACTION
    kv = edge_key_valid(c.L)
    mask_dense = O.attention_mask(kv.to(torch.int64), bidirectional=not c.causal).float()
    dead = (mask_dense.expand(c.B, 1, c.L, mask_dense.shape[-1]) == 0).sum(-1).squeeze(1) == 0  # [B, L]
    lens = kv.sum(-1).to(torch.int64)
    return base._replace(kv=kv, lens=lens, rows=(lens - 1).clamp_min(0).view(-1, 1), mask_dense=mask_dense, dead=dead,
                         cot=None, cot_dead=None)


def _rows(name, rows_bl):
    if name == "M":
        return rows_bl[:, None, :, None]
    if name in ("row_stats", "lse_f", "lse_b"):
        return rows_bl[:, None, :] if name != "row_stats" else rows_bl[:, None, :, None]
    return rows_bl[:, :, None]


def edge_errors(pr, got, ref32, ref64):
    """{name: (live error against ref64, dead error against ref32 -- against ref64 for the normalisers --, dead scale)} for
    the tensors in `got` (CPU tensors by name: M, ctx_attacked, ctx_calibrated, row_stats [.., :5], lse_f, lse_b)."""
    out = {}
    for name, t in got.items():
        key = "stats" if name == "row_stats" else name
        live, dead = _rows(name, ~pr.dead), _rows(name, pr.dead)
        e_live = ((t.double() - ref64[key]).abs() * live).max().item()
        dref = ref64[key] if name in ("row_stats", "lse_f", "lse_b") else ref32[key].double()
        e_dead = ((t.double() - dref).abs() * dead).max().item()
        out[name] = (e_live, e_dead, (dref.abs() * dead).max().item())
    return out
