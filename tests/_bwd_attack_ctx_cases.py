"""Shared by tests/test_hip_bwd_attack_ctx.py (GPU) and tests/test_bwd_attack_ctx_cases_cpu.py: the case table of the
attack-side backward's CTX form (csrc/acattn_bwd_attack.hip: an attack-only launch that carries a cotangent of the
calibrated context), its inputs, cotangents and the oracle's autograd.  Nothing here touches a GPU or imports the HIP package.

Inputs are tests/_attention_fp64.py's (problem(); the lengths as tests/test_hip_bwd_attack.py sets them: every batch holds a
sequence of length 1, one of length L and one whose length is a multiple of 16).  Cotangent forms:
  "cal"       d_ctx_calibrated alone, dense, at unit scale (problem()'s `calibrated_dense` patterns);
  "cal_dpen"  ... + d_pen per (sequence, head, query block): the training step's form;
  "cal_dM"    ... + a dense cotangent of M.
The mask-side cotangents are drawn at 1e-2 (problem()'s `calibrated_dense_plus_mask` scale), so that what they add to dqa
and dka next to the context's part stays well above the 1e-4 floor of tensor_bound: a mask path that went wrong in the
presence of the context cotangent would not hide below the bound.
"""
import torch

from oracle import ac_tsr_ref as O
from tests import _attention_fp64 as F

SHAPES = [
    F._case("B3_L50", "train", (3, 50, 64, 2)),          # decode_block's second branch; a two-row tail block
    F._case("L37", "train", (8, 37, 64, 2)),             # odd L, a partial 16-byte segment, three blocks
    F._case("dh16_L16", "train", (8, 16, 64, 4)),        # head size 16; one block
    F._case("dh16_L17", "train", (8, 17, 64, 4)),        # ... and a one-row second block
    F._case("dh64_L64", "train", (8, 64, 128, 2)),       # head size 64, four full blocks
    F._case("bidirectional_p0", "train", (8, 50, 64, 2), causal=False, p_drop=0.0),
]
LEFT_PAD = F._case("left_pad_L50", "train", (8, 50, 64, 2))
REPLAY = F._case("replay_B8_L50", "train", (8, 50, 64, 2))
FORMS = ("cal", "cal_dpen", "cal_dM")


def problem(c, left_pad=False):
    """F.problem's inputs with the lengths this suite wants: L, 1, a multiple of 16 in every batch; `left_pad`: sequence 3
    keeps only its last 30 keys (valid from key 20 on: query blocks 0 and 1 have rows that see no key)."""
    pr = F.problem(c)
    lens = pr.lens.clone()
    lens[0], lens[1], lens[2] = c.L, 1, 16 * max(1, (c.L - 1) // 16)
    kv = (torch.arange(c.L)[None, :] < lens[:, None]).to(torch.uint8)
    if left_pad:
        kv[3] = (torch.arange(c.L) >= 20).to(torch.uint8)
    mask_dense = O.attention_mask(kv.to(torch.int64), bidirectional=not c.causal).float()
    dead = (mask_dense.expand(c.B, 1, c.L, mask_dense.shape[-1]) == 0).sum(-1).squeeze(1) == 0  # [B, L]
    assert bool(dead.any()) == left_pad
    n_keys = kv.sum(1)
    assert (n_keys == 1).any() and (n_keys == c.L).any() and ((n_keys % 16 == 0) & (n_keys > 0)).any()
    return pr._replace(kv=kv, lens=lens, mask_dense=mask_dense, dead=dead, rows=(lens - 1).view(-1, 1))


def cotangents(c, pr):
    """{"cal", "dM", "dpen"} zeroed on the fully masked rows, and {"cal_dead", "dM_dead"}: those rows' cotangents alone."""
    g = torch.Generator().manual_seed(4343)
    live_h = (~pr.dead)[:, :, None].float()
    live_m = (~pr.dead)[:, None, :, None].float()
    d_cal = torch.randn(c.B, c.L, c.H, generator=g)
    d_M = torch.randn(c.B, c.nh, c.L, c.L, generator=g) * 1e-2
    d_pen = torch.randn(c.B, c.nh, (c.L + 15) // 16, generator=g) * 1e-2
    return {"cal": d_cal * live_h, "cal_dead": d_cal * (1 - live_h), "dM": d_M * live_m, "dM_dead": d_M * (1 - live_m), "dpen": d_pen}


def form_cotangents(cots, form, dead=False):
    """(d_cal, d_M, d_pen) of a form; `dead`: the fully masked rows' cotangents alone ("cal", "cal_dM")."""
    assert form in FORMS and not (dead and form == "cal_dpen")
    sfx = "_dead" if dead else ""
    return cots["cal" + sfx], cots["dM" + sfx] if form == "cal_dM" else None, cots["dpen"] if form == "cal_dpen" else None


def oracle(c, pr, draws, d_cal, d_M, d_pen, dtype):
    """{qa, ka: gradient} of sum ctx_calibrated . d_cal (+ sum M . d_M) (+ sum d_pen[b,h,qb] * sum_{rows of qb} (1 - M)^2)
    over the oracle's own outputs, in `dtype` on the CPU."""
    with F.default_dtype(dtype):
        x = {k: pr.t[k].to(dtype).clone().requires_grad_(k in ("qa", "ka")) for k in F.leaf_names(c)}
        cfg = O.EncoderCfg(n_layers=1, n_heads=c.nh, hidden_size=c.H, inner_size=4 * c.H, combine_option="gate", use_order=True,
                           use_distance=True, two_level=True, rich_calibrated_combine=c.rich, seq_length=c.L, attn_dropout_prob=c.p_drop)
        cast = lambda v: None if v is None else v.to(dtype)
        ref = O.core_from_projected(x["q"], x["k"], x["v"], x["qa"], x["ka"], x["gl"], pr.mask_dense.to(dtype), x["w_order"],
                                    x["b_order"], x["w_dist"], x["b_dist"], x["scalar"], cfg, cast(draws["noise"]),
                                    keep_after=cast(draws["keep_after"]), keep_mask=cast(draws["keep_mask"]), keep_before=None,
                                    anneal_rate=c.anneal_rate, rich_ratio=None, materialize=False)
        M = ref["M"]
        loss = (ref["ctx_calibrated"] * d_cal.to(dtype)).sum()
        if d_M is not None:
            loss = loss + (M * d_M.to(dtype)).sum()
        if d_pen is not None:
            nT = (c.L + 15) // 16
            rows = torch.nn.functional.pad(((1 - M) ** 2).sum(-1), (0, 16 * nT - c.L))  # [B, nh, 16 nT]
            loss = loss + (rows.view(c.B, c.nh, nT, 16).sum(-1) * d_pen.to(dtype)).sum()
        gqa, gka = torch.autograd.grad(loss, [x["qa"], x["ka"]])
    return {"qa": gqa, "ka": gka}
