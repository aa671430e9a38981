"""Shared by the float64 gradient tests of the attention operators (tests/test_hip_spatial_bwd.py,
tests/test_hip_attention_bwd_fp64.py) and by the CPU check of the latter's case table (tests/test_attention_bwd_cases_cpu.py).

Nothing here touches a GPU or imports the HIP package: the case table of the adversarial operator's backward, its inputs
and cotangents, and the oracle's autograd over oracle/ac_tsr_ref.py::core_from_projected(..., materialize=False) in a
chosen dtype on the CPU.
"""
import contextlib
import math
from collections import namedtuple

import torch

from oracle import ac_tsr_ref as O

TENSOR_GRADS = ("q", "k", "v", "qa", "ka", "gl", "w_order", "w_dist")
SCALAR_GRADS = ("b_order", "b_dist", "scalar", "rich_ratio")
PATTERNS = ("all", "calibrated_read_row", "attacked_read_row_plus_mask", "calibrated_dense_only", "calibrated_dense_plus_mask")
# the outputs that are part of the loss; the others get NO cotangent (None, not zeros): the kernels specialise on it
USED_OUTPUTS = {"all": ("ctx_attacked", "ctx_calibrated", "M"), "calibrated_read_row": ("ctx_calibrated",),
                "attacked_read_row_plus_mask": ("ctx_attacked", "M"), "calibrated_dense_only": ("ctx_calibrated",),
                "calibrated_dense_plus_mask": ("ctx_calibrated", "M")}
READ_ROW_PATTERNS = ("calibrated_read_row", "attacked_read_row_plus_mask")

# Bounds (see tests/test_hip_attention_bwd_fp64.py): e = max|got - ref64| / max|ref64|, e32 the same for the fp32 oracle
TENSOR_FLOOR, TENSOR_CAP, SCALAR_BOUND, ABS_FLOOR, E32_PRECONDITION = 1e-4, 2e-3, 2e-3, 1e-7, 2e-5


@contextlib.contextmanager
def default_dtype(dtype):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)  # the oracle creates its constants (zeros, the distance table) in the default dtype
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def err(got, ref):
    return ((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-300)).item()


def abs_err_and_scale(got, ref):
    return (got.double() - ref.double()).abs().max().item(), ref.double().abs().max().item()


def tensor_bound(e32):
    return min(max(TENSOR_FLOOR, 2 * e32), TENSOR_CAP)


# ---- the case table -------------------------------------------------------------------------------------------------------
# kind "train": structured mask, counter RNG, `gate`, two-level, both spatial terms (the tuned kernels; `pin` = the backward
# kernel, "auto" | "stream" | "row").  kind "general": explicit randomness (torch-drawn noise and keeps) -> the general kernel.
Case = namedtuple("Case", "id kind B L H nh causal left_pad p_drop pattern pin combine anneal_rate two_level rich mask terms")


def _case(id, kind, shape, pattern="all", pin="auto", causal=True, left_pad=False, p_drop=0.5, combine="gate", anneal_rate=1.0,
          two_level=True, rich="fixed", mask="structured", terms=("order", "distance")):
    return Case(id, kind, *shape, causal, left_pad, p_drop, pattern, pin, combine, anneal_rate, two_level, rich, mask, terms)


def _table():
    cases = []

    def train(tag, shape, patterns, pins, **kw):
        for pin in pins:
            for pattern in patterns:
                cases.append(_case(f"{tag}-{pattern}-{pin}", "train", shape, pattern=pattern, pin=pin, **kw))

    train("B64_L50", (64, 50, 64, 2), PATTERNS, ("auto",))
    train("B64_L50", (64, 50, 64, 2), ("all",), ("stream", "row"))
    train("bench_shape", (512, 50, 64, 2), ("all",), ("auto",))
    train("bidirectional_p0", (64, 50, 64, 2), ("all",), ("auto",), causal=False, p_drop=0.0)
    train("bidirectional_p05", (64, 50, 64, 2), ("all",), ("auto",), causal=False, p_drop=0.5)
    train("dh16_L50", (12, 50, 64, 4), PATTERNS[:3], ("auto", "stream"))
    train("L37", (6, 37, 64, 2), ("all", "attacked_read_row_plus_mask"), ("auto", "stream"))
    train("dh64_L64", (8, 64, 128, 2), PATTERNS[:3], ("row", "stream"))
    train("dh16_L77", (5, 77, 64, 4), ("all",), ("auto",))
    train("cfg4_shape", (8, 200, 128, 4), PATTERNS, ("auto",))
    train("dh64_L130", (2, 130, 256, 4), ("all", "calibrated_dense_only"), ("auto",))
    train("dh128_L200", (3, 200, 256, 2), ("all", "calibrated_read_row"), ("auto",))
    train("dh128_L50", (5, 50, 256, 2), ("all", "calibrated_read_row"), ("auto",))
    # (with the streaming pair pinned: its key kernel's two defects under left padding, tests/test_hip_attention_bwd_fp64.py)
    train("left_pad", (64, 50, 64, 2), ("all",), ("auto", "stream"), left_pad=True)
    for tag, shape in (("B64_L50", (64, 50, 64, 2)), ("dh16_L50", (12, 50, 64, 4)), ("dh64_L64", (8, 64, 128, 2)),
                       ("cfg4_L200", (2, 200, 128, 4)), ("dh128_L200", (3, 200, 256, 2))):
        cases.append(_case(f"general-{tag}", "general", shape))
    opt = (16, 50, 64, 2)
    cases += [
        _case("general-fixed", "general", opt, combine="fixed"),
        _case("general-annealing_037", "general", opt, combine="annealing", anneal_rate=0.37),
        _case("general-one_level_fixed", "general", opt, two_level=False, rich="fixed"),
        _case("general-one_level_trainable", "general", opt, two_level=False, rich="trainable"),
        _case("general-dense_LL", "general", opt, mask="dense_LL"),
        _case("general-dense_L", "general", opt, mask="dense_L", causal=False),
        _case("general-order_only", "general", opt, terms=("order",)),
        _case("general-distance_only", "general", opt, terms=("distance",)),
        _case("general-p0", "general", opt, p_drop=0.0),
    ]
    assert len({c.id for c in cases}) == len(cases)
    return cases


CASES = _table()


def problem_key(c: Case):
    """What the inputs, cotangents and the reference depend on: everything but the pinned kernel."""
    return c._replace(id="", pin="")


def leaf_names(c: Case):
    names = ["q", "k", "v", "qa", "ka"] + (["gl"] if c.combine == "gate" else [])
    names += ["w_order", "b_order"] if "order" in c.terms else []
    names += ["w_dist", "b_dist", "scalar"] if "distance" in c.terms else []
    return names + (["rich_ratio"] if not c.two_level and c.rich == "trainable" else [])


def calibrator_scale(H, nh):
    """0.3 as tests/test_hip_onehop.py, shrunk for head sizes above 32 so that the order affine's argument stays below the
    range where fp32 `1 - sigmoid(x)` rounds to 0 (x > 16.6) and the fp32 oracle stops being a usable yardstick."""
    dh = H // nh
    return 0.3 * math.sqrt(32 / dh) if dh > 32 else 0.3


Problem = namedtuple("Problem", "t kv lens rows mask_dense dead cot cot_dead")


def problem(c: Case, seed=606) -> Problem:
    """Inputs as tests/test_hip_onehop.py::_problem draws them (calibrator weights at calibrator_scale), cotangents as its
    tuned-backward test forms them, all float32 on the CPU.  `dead`: query rows without an allowed key (the left-padded
    sequence under the causal mask); `cot` is zero there and `cot_dead` holds those rows' cotangents alone."""
    B, L, H, nh = c.B, c.L, c.H, c.nh
    g = torch.Generator().manual_seed(seed)
    t = {k: torch.randn(B, L, H, generator=g) for k in ("q", "k", "v", "qa", "ka")}
    t["gl"] = torch.randn(B, L, L, generator=g)
    dh = H // nh
    scale = calibrator_scale(H, nh)
    for k, shp in (("w_order", (1, 2 * dh)), ("b_order", (1,)), ("w_dist", (1, 2 * dh)), ("b_dist", (1,)), ("scalar", (1,))):
        t[k] = scale * torch.randn(*shp, generator=g)
    t["rich_ratio"] = torch.tensor([0.3])
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0] = L
    kv = (torch.arange(L)[None, :] < lens[:, None]).to(torch.uint8)
    if c.left_pad:
        kv[1] = 1 - kv[1]
    rows = (lens - 1).view(-1, 1)
    mask_dense = O.attention_mask(kv.to(torch.int64), bidirectional=not c.causal).float()
    dead = (mask_dense.expand(B, 1, L, mask_dense.shape[-1]) == 0).sum(-1).squeeze(1) == 0  # [B, L]
    assert bool(dead.any()) == (c.left_pad and c.causal)
    cot = {"ctx_attacked": torch.zeros(B, L, H), "ctx_calibrated": torch.zeros(B, L, H), "M": torch.zeros(B, nh, L, L)}
    row_cot = torch.randn(B, 1, H, generator=g)
    idx = rows.unsqueeze(-1).expand(-1, -1, H)
    if c.pattern == "all":
        cot = {k: torch.randn(v.shape, generator=g) for k, v in cot.items()}
    elif c.pattern.startswith("calibrated_dense"):
        cot["ctx_calibrated"] = torch.randn(B, L, H, generator=g)
        if c.pattern.endswith("plus_mask"):
            cot["M"] = torch.randn(B, nh, L, L, generator=g) * 1e-2
    elif c.pattern == "calibrated_read_row":
        cot["ctx_calibrated"].scatter_(1, idx, row_cot)
    else:
        cot["ctx_attacked"].scatter_(1, idx, row_cot)
        cot["M"] = torch.randn(B, nh, L, L, generator=g) * 1e-3  # the penalty's cotangent is small and dense
    cot = {k: cot[k] for k in USED_OUTPUTS[c.pattern]}
    row_of = lambda k, rows_bl: rows_bl[:, None, :, None] if k == "M" else rows_bl[:, :, None]
    cot_dead = {k: v * row_of(k, dead).to(v.dtype) for k, v in cot.items()}
    cot = {k: v * row_of(k, ~dead).to(v.dtype) for k, v in cot.items()}
    return Problem(t, kv, lens, rows, mask_dense, dead, cot, cot_dead)


def torch_draws(c: Case, seed=6060):
    """Noise and 0/1 keep masks from torch's generator: the explicit randomness of the general-kernel cases (handed to both
    sides) and, in the CPU test of the case table, the stand-in for the kernels' counter draws."""
    g = torch.Generator().manual_seed(seed)
    shape = (c.B, c.nh, c.L, c.L)
    d = {"noise": torch.randn(shape, generator=g), "keep_after": None, "keep_mask": None, "keep_before": None}
    if c.p_drop > 0:
        for k in ("keep_after", "keep_mask") + (() if c.two_level else ("keep_before",)):
            d[k] = torch.empty(shape).bernoulli_(1.0 - c.p_drop, generator=g)
    return d


def oracle_grads(c: Case, pr: Problem, draws, cot, dtype):
    """{leaf: gradient} of sum_k (out_k * cot_k) over the outputs in `cot`, by torch autograd over
    core_from_projected(..., materialize=False) in `dtype` on the CPU.  A leaf the loss does not reach gets zeros."""
    names = leaf_names(c)
    with default_dtype(dtype):
        x = {k: pr.t[k].to(dtype).clone().requires_grad_(True) for k in names}
        cfg = O.EncoderCfg(n_layers=1, n_heads=c.nh, hidden_size=c.H, inner_size=4 * c.H, combine_option=c.combine,
                           use_order="order" in c.terms, use_distance="distance" in c.terms, two_level=c.two_level,
                           rich_calibrated_combine=c.rich, seq_length=c.L, attn_dropout_prob=c.p_drop)
        cast = lambda v: None if v is None else v.to(dtype)
        ref = O.core_from_projected(x["q"], x["k"], x["v"], x["qa"], x["ka"], x.get("gl"), pr.mask_dense.to(dtype),
                                    x.get("w_order"), x.get("b_order"), x.get("w_dist"), x.get("b_dist"), x.get("scalar"), cfg,
                                    cast(draws["noise"]), keep_after=cast(draws["keep_after"]), keep_mask=cast(draws["keep_mask"]),
                                    keep_before=cast(draws["keep_before"]), anneal_rate=c.anneal_rate,
                                    rich_ratio=x.get("rich_ratio"), materialize=False)
        loss = sum((ref[k] * cot[k].to(dtype)).sum() for k in cot)
        grads = torch.autograd.grad(loss, [x[n] for n in names], allow_unused=True)
    return {n: torch.zeros_like(x[n]).detach() if g is None else g for n, g in zip(names, grads)}
