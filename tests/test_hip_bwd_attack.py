"""GPU suite (-m gpu): the attack-side backward (csrc/acattn_bwd_attack.hip) -- dqa and dka of an attack-only launch whose
only cotangent is the attack mask's -- against the oracle differentiated by torch autograd in FLOAT64.

Inputs, oracle and bounds are tests/_attention_fp64.py's: core_from_projected(..., materialize=False) on the CPU fed the
kernels' own counter draws (A.materialize_randomness), e = max|got - ref64| / max|ref64| <= tensor_bound(e32) with the
precondition e32 <= E32_PRECONDITION and the absolute floor ABS_FLOOR.  The launches are issued directly
(attn_launch.attention_bwd_launch(..., attack_only=True, poison=True)) with
  (i)  a dense cotangent of M at the 1e-3 scale problem() uses for the penalty's, or
  (ii) d_pen per (sequence, head, query block): the oracle's loss is sum d_pen[b,h,qb] * sum_{rows of qb} (1 - M)^2 of its own M.
Every batch holds a sequence of length 1, one of length L and one whose length is a multiple of 16.  Each case also asserts
that no NaN is left in the poisoned outputs, that a second launch gives the same bits, and that the row-resident kernel
(ACATTN_BWD_ROW pinned, which never takes the new launcher) passes the same bound on the same inputs.

The left-padded sequence (fully masked rows under the causal mask; its first blocks see no key and spread over every key
tile, so the workgroup's tiles do not fit the slots and its waves take turns) is checked as
tests/test_hip_attention_bwd_fp64.py checks such rows: the live rows against the float64 oracle, the dead rows' cotangents
alone against the float32 oracle at the 2e-3 cap.

The split (the mask launch in front of the one-row launch, which now also writes the zeros of the head-summed gate
gradient): `attacked_read_row_plus_mask` through A.calibrated_attention under the automatic choice.
"""
import pytest
import torch

import ac_tsr_amd as A
from ac_tsr_amd import _lib, attn_launch, ops
from oracle import ac_tsr_ref as O
from tests import _attention_fp64 as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 777

SHAPES = [
    F._case("B3_L50", "train", (3, 50, 64, 2)),          # decode_block's second branch; a two-row tail block
    F._case("L37", "train", (8, 37, 64, 2)),             # odd L, a partial 16-byte segment, three blocks
    F._case("dh16_L16", "train", (8, 16, 64, 4)),        # head size 16; one block
    F._case("dh16_L17", "train", (8, 17, 64, 4)),        # ... and a one-row second block
    F._case("dh64_L64", "train", (8, 64, 128, 2)),       # head size 64, four full blocks
    F._case("bidirectional_p0", "train", (8, 50, 64, 2), causal=False, p_drop=0.0),
]
LEFT_PAD = F._case("left_pad_L50", "train", (8, 50, 64, 2))
_CACHE = {}


def _problem(c, left_pad=False):
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


def _cotangents(c, pr):
    g = torch.Generator().manual_seed(4242)
    live = (~pr.dead)[:, None, :, None].float()
    d_M = torch.randn(c.B, c.nh, c.L, c.L, generator=g) * 1e-3
    d_pen = torch.randn(c.B, c.nh, (c.L + 15) // 16, generator=g) * 1e-3
    return {"dM": d_M * live, "dM_dead": d_M * (1 - live), "dpen": d_pen}


def _oracle(c, pr, draws, form, cot, dtype):
    """{qa, ka: gradient} of the form's loss over the oracle's own M."""
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
        if form == "dpen":
            nT = (c.L + 15) // 16
            rows = torch.nn.functional.pad(((1 - M) ** 2).sum(-1), (0, 16 * nT - c.L))  # [B, nh, 16 nT]
            loss = (rows.view(c.B, c.nh, nT, 16).sum(-1) * cot.to(dtype)).sum()
        else:
            loss = (M * cot.to(dtype)).sum()
        gqa, gka = torch.autograd.grad(loss, [x["qa"], x["ka"]])
    return {"qa": gqa, "ka": gka}


def _setup(c, left_pad=False):
    key = (c.id, left_pad)
    if key not in _CACHE:
        pr = _problem(c, left_pad)
        rnd = A.materialize_randomness(c.B, c.nh, c.L, SEED, c.p_drop, DEV)
        draws = {"noise": rnd.noise.cpu(), "keep_after": None, "keep_mask": None}
        if c.p_drop > 0:
            draws.update(keep_after=rnd.keep_after.cpu().float(), keep_mask=rnd.keep_mask.cpu().float())
        _CACHE[key] = (pr, draws, _cotangents(c, pr), {})
    return _CACHE[key]


def _references(c, left_pad, form, cot_name, dtypes):
    pr, draws, cots, refs = _setup(c, left_pad)
    for dt in dtypes:
        if (cot_name, dt) not in refs:
            refs[(cot_name, dt)] = _oracle(c, pr, draws, form, cots[cot_name], dt)
    return [refs[(cot_name, dt)] for dt in dtypes]


def _launch(c, pr, d_M=None, d_pen=None, pin=_lib.BWD_AUTO):
    """(dqa, dka) of one attack-only launch into NaN-filled buffers, as CPU tensors."""
    lib = _lib.load()
    x = {k: v.to(DEV) for k, v in pr.t.items()}
    cfg = A.AttentionConfig(n_heads=c.nh, combine_option="gate", two_level=True)
    mask = A.StructuredMask(pr.kv.to(DEV), causal=c.causal)
    keep = [x, mask]
    flat = lambda t: t.reshape(-1).contiguous()
    prob = ops._fill_problem(x["q"], x["k"], x["v"], x["qa"], x["ka"], x["gl"], mask, flat(x["w_order"]), x["b_order"],
                             flat(x["w_dist"]), x["b_dist"], x["scalar"], None, cfg, c.p_drop, None, SEED, keep)
    _, _, M, stats, _, _ = attn_launch.attention_fwd_launch(lib, prob, x["q"], c.nh, adversarial=True, want_penalty=False)
    dev = lambda t: None if t is None else t.to(DEV).contiguous()
    old = lib.acattn_select_backward_kernel(pin)
    try:
        res = attn_launch.attention_bwd_launch(lib, prob, x["q"], c.nh, M, stats, d_M=dev(d_M), d_pen=dev(d_pen), attack_only=True,
                                               poison=True)
    finally:
        lib.acattn_select_backward_kernel(old)
    torch.cuda.synchronize()
    return {"qa": res[3].cpu(), "ka": res[4].cpu()}


def _failures(tag, got, ref64, ref32):
    out = []
    for n in ("qa", "ka"):
        abs_e, scale = F.abs_err_and_scale(got[n], ref64[n])
        abs_e32, _ = F.abs_err_and_scale(ref32[n], ref64[n])
        e, e32 = abs_e / scale, abs_e32 / scale
        print(f"bwd_attack_accuracy case={tag} grad=d{n} e={e:.3e} e32={e32:.3e}")
        if not e32 <= F.E32_PRECONDITION:
            out.append(f"d{n}: precondition e32 = {e32:.3e} > {F.E32_PRECONDITION:.0e}")
        if not abs_e <= F.tensor_bound(e32) * scale + F.ABS_FLOOR:
            out.append(f"d{n}: e = {e:.3e} > {F.tensor_bound(e32):.3e} (e32 = {e32:.3e}, scale {scale:.3e})")
    return out


def _check_case(c, left_pad, form):
    pr, draws, cots, _ = _setup(c, left_pad)
    ref64, ref32 = _references(c, left_pad, form, form, (torch.float64, torch.float32))
    kw = {"d_pen": cots["dpen"]} if form == "dpen" else {"d_M": cots["dM"]}
    got = _launch(c, pr, **kw)
    for n in ("qa", "ka"):
        assert not torch.isnan(got[n]).any(), f"d{n}: an element below L was not written"
    again = _launch(c, pr, **kw)
    for n in ("qa", "ka"):
        assert torch.equal(got[n], again[n]), f"d{n} differs between two launches"
    failures = _failures(f"{c.id}-{form}-auto", got, ref64, ref32)
    row = _launch(c, pr, pin=_lib.BWD_ROW, **kw)
    failures += [f"(row-resident) {f}" for f in _failures(f"{c.id}-{form}-row", row, ref64, ref32)]
    assert not failures, f"{c.id}-{form}: " + "; ".join(failures)


@pytest.mark.parametrize("form", ["dM", "dpen"])
@pytest.mark.parametrize("case", SHAPES, ids=lambda c: c.id)
def test_dqa_dka_match_the_fp64_oracle(case, form):
    _check_case(case, False, form)


def test_left_padded_live_rows_match_the_fp64_oracle():
    """Dense d M on the live rows (the fully masked rows' cotangents zeroed, as in tests/test_hip_attention_bwd_fp64.py)."""
    _check_case(LEFT_PAD, True, "dM")


def test_left_padded_dead_rows_match_the_fp32_oracle():
    """The fully masked rows' cotangents alone against the FLOAT32 oracle at the 2e-3 cap
    (test_fully_masked_rows_match_the_fp32_oracle's check)."""
    c = LEFT_PAD
    pr, draws, cots, _ = _setup(c, True)
    assert pr.dead.any()
    (ref32,) = _references(c, True, "dM", "dM_dead", (torch.float32,))
    got = _launch(c, pr, d_M=cots["dM_dead"])
    for n in ("qa", "ka"):
        assert not torch.isnan(got[n]).any()
        abs_e, scale = F.abs_err_and_scale(got[n], ref32[n])
        print(f"bwd_attack_accuracy case={c.id} fully_masked_rows grad=d{n} e_vs_fp32={abs_e / scale:.3e}")
        assert scale > 0 and abs_e <= 2e-3 * scale + F.ABS_FLOOR, f"d{n}: {abs_e:.3e} of {scale:.3e}"


# ---- the split: mask launch (which writes the gate gradient's zeros) + one-row launch -----------------------------------------
def test_split_gate_gradient_is_zero_outside_the_read_row_and_replays(monkeypatch):
    c = F._case("split_B8_L50", "train", (8, 50, 64, 2), pattern="attacked_read_row_plus_mask")
    pr = F.problem(c)
    rnd = A.materialize_randomness(c.B, c.nh, c.L, SEED, c.p_drop, DEV)
    draws = {"noise": rnd.noise.cpu(), "keep_after": rnd.keep_after.cpu().float(), "keep_mask": rnd.keep_mask.cpu().float(),
             "keep_before": None}
    ref64 = F.oracle_grads(c, pr, draws, pr.cot, torch.float64)
    ref32 = F.oracle_grads(c, pr, draws, pr.cot, torch.float32)
    names = F.leaf_names(c)
    x = {k: pr.t[k].to(DEV).requires_grad_(True) for k in names}
    cfg = A.AttentionConfig(n_heads=c.nh, combine_option="gate", two_level=True)
    mask = A.StructuredMask(pr.kv.to(DEV), causal=True)
    rows = pr.rows.to(DEV)
    cot = {k: v.to(DEV) for k, v in pr.cot.items()}
    kw = {k: x[k] for k in names[5:] if k != "gl"}
    gates = []
    real = attn_launch.attention_bwd_launch

    def recording(*a, **k):
        res = real(*a, **k)
        gates.append(res[5])
        return res

    monkeypatch.setattr(attn_launch, "attention_bwd_launch", recording)
    monkeypatch.setattr(attn_launch, "POISON", True)

    def walk():
        ctx_a, _, M, _ = A.calibrated_attention(x["q"], x["k"], x["v"], x["qa"], x["ka"], x["gl"], mask, cfg, p_drop=c.p_drop, seed=SEED,
                                                read_rows=rows, **kw)
        loss = (ctx_a * cot["ctx_attacked"]).sum() + (M * cot["M"]).sum()
        return [loss] + list(torch.autograd.grad(loss, [x[n] for n in names], allow_unused=True))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [None if t is None else t.detach().clone() for t in walk()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert len(gates) == 1 and gates[0].shape == (c.B, 1, c.L, c.L)  # the one-row form behind the mask launch
    gate = gates[0].cpu()
    off_row = torch.ones(c.B, c.L, dtype=torch.bool)
    off_row[torch.arange(c.B), pr.rows.view(-1)] = False
    assert (gate[:, 0][off_row] == 0.0).all(), "the gate gradient outside the read row is not exactly zero"
    dgl = eager[1 + names.index("gl")].cpu()
    abs_e, scale = F.abs_err_and_scale(dgl, ref64["gl"])
    abs_e32, _ = F.abs_err_and_scale(ref32["gl"], ref64["gl"])
    # the gate only reaches the calibrated context, which carries no cotangent here: the float64 reference is identically
    # zero and the read row must be within the absolute floor (tests/test_hip_attention_bwd_fp64.py: `ref64=0`)
    print(f"bwd_attack_accuracy case={c.id} grad=dgl abs_e={abs_e:.3e} abs_e32={abs_e32:.3e} scale={scale:.3e}")
    assert scale == 0 and abs_e32 <= F.E32_PRECONDITION
    assert abs_e <= F.ABS_FLOOR
    for n in ("qa", "ka"):
        g = eager[1 + names.index(n)].cpu()
        abs_e, scale = F.abs_err_and_scale(g, ref64[n])
        abs_e32, _ = F.abs_err_and_scale(ref32[n], ref64[n])
        print(f"bwd_attack_accuracy case={c.id} grad=d{n} e={abs_e / scale:.3e} e32={abs_e32 / scale:.3e}")
        assert abs_e <= F.tensor_bound(abs_e32 / scale) * scale + F.ABS_FLOOR, n

    monkeypatch.setattr(attn_launch, "POISON", False)  # (a NaN fill would be one more captured node per buffer)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = walk()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for name, a, b in zip(["loss"] + names, got, eager):
        if b is None:
            assert a is None, name
            continue
        assert torch.equal(a, b), f"{name}: eager and replayed graph differ by {(a - b).abs().max().item():.3e}"
