"""GPU suite (-m gpu): the backward of the ADVERSARIAL attention operator -- the row-resident kernel, the streaming row / key
pair, the one-row and mask-only forms (csrc/acattn_bwd_fast.hip, acattn_bwd_stream.hip) and the general kernel behind them
(acattn_bwd_general.inc) -- against the oracle differentiated by torch autograd in FLOAT64.

Reference: oracle/ac_tsr_ref.py::core_from_projected(..., materialize=False) in float64 on the CPU, fed the kernels' own
draws: A.materialize_randomness for the counter RNG, torch-drawn noise and keep masks handed to both sides for the general
kernel (ExplicitRandomness).  Loss: sum_k (out_k * cot_k) over the outputs the cotangent pattern uses (an unused output gets
NO cotangent, as in the trainer's walks).  Inputs as tests/test_hip_onehop.py::_problem draws them, with the calibrator
weights at 0.3 * sqrt(32 / dh) for head sizes above 32: at 0.3 the order affine's argument reaches the range where fp32
`1 - sigmoid(x)` rounds to 0 and the float32 oracle is itself off by up to 7e-3 (tests/test_attention_bwd_cases_cpu.py checks
the whole table for that on the CPU).  Cases, inputs and the oracle's autograd: tests/_attention_fp64.py.

Bounds, with e = max|got - ref64| / max|ref64| and e32 the same figure for the oracle run in float32 on the same inputs and
draws.  Tensor-valued gradients (dq, dk, dv, dqa, dka, dgl, dw_order, dw_dist): e <= max(1e-4, 2 * e32) and never above 2e-3
(1e-4 of scale against fp64: VERDICT.md next-round item 6 and tests/test_hip_spatial_bwd.py; 2 * e32: the margin
tests/test_hip_ce.py and tests/test_hip_tail_split.py grant a kernel over the fp32 restatement of its arithmetic; 2e-3: the
cap of every gradient test here).  Precondition, asserted: e32 <= 2e-5 on every tensor-valued gradient, so that a badly
conditioned input cannot loosen the bound.  Single-number gradients (db_order, db_dist, dscalar, drich_ratio) are cancelling
sums over B * h * L^2 terms whose scale is the value itself: e <= 2e-3 only.  Every bound carries an absolute floor of 1e-7
(tests/test_hip_onehop.py's own); a gradient whose float64 reference is identically zero (the gate's when the calibrated
context has no cotangent) must be within that floor.

Fully masked query rows (the left-padded sequence under the causal mask) follow the reference's fp32 `+ (-10000)`
quantisation, which float64 does not reproduce: their rows of both contexts and of M get a zero cotangent in the float64
comparison and are then checked alone against the float32 oracle at the 2e-3 cap
(test_fully_masked_rows_match_the_fp32_oracle: one gradient each, dscalar a strict xfail with its figures and cause).

Which form ran is asserted as far as the library can say (_check_form): a case pinned to the streaming pair or the
row-resident kernel must not have taken the one-row form the automatic choice would take, and a general-kernel case must
have reached the launch with explicit draws.  That is all the library can say: for the dense patterns (`all`,
`calibrated_dense_*`) the streaming pair and the row-resident kernel both write the gate gradient per head, so NOTHING here
asserts which of the two a `-stream`, `-row` or `-auto` case ran; that those pins took effect shows only in the printed
figures and second-walk bits, which differ between them.  The pin is per host thread and autograd runs the backward on a thread of its
own; the autograd node carries the pin of the thread that ran its forward (ac_tsr_amd/attn_launch.py: backward_kernel) --
before it did, the pinned read-row cases here ran the one-row form and failed this check.

A second walk of the same graph: tests/test_hip_backward.py asserts `equal bits or within 1e-5` of the general kernel and
nothing of the tuned kernels; the same is asserted here of the general kernel's dq, dk, dv, and whether the bits were equal
is printed for every case.

One line per (case, gradient) is printed; profiles/attention_bwd_accuracy.txt holds one run's lines.
"""
import pytest
import torch

import ac_tsr_amd as A
from ac_tsr_amd import _lib, attn_launch
from tests import _attention_fp64 as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
PINS = {"auto": _lib.BWD_AUTO, "stream": _lib.BWD_STREAM, "row": _lib.BWD_ROW}
SEED = 777
_REFERENCES = {}  # problem_key -> (Problem, draws, ref64, ref32): cases that differ only in the pinned kernel share one


@pytest.fixture
def backward_kernel():
    """Pins the backward kernel (acattn_select_backward_kernel) for one test and restores the automatic choice."""
    lib = _lib.load()
    yield lambda which: lib.acattn_select_backward_kernel(which)
    lib.acattn_select_backward_kernel(_lib.BWD_AUTO)


@pytest.fixture
def launches(monkeypatch):
    """Records every attention-backward launch of the test (ops.py and dispatch.py both end in
    attn_launch.attention_bwd_launch): what the library was asked and the shape of the gate gradient it wrote."""
    seen = []
    real = attn_launch.attention_bwd_launch

    def recording(lib, prob, q, n_heads, M, stats, **kw):
        res = real(lib, prob, q, n_heads, M, stats, **kw)
        seen.append(dict(rng_mode=prob.rng_mode, mask_mode=prob.mask_mode, read_rows=kw.get("read_rows"),
                         gate_heads=None if res[5] is None else res[5].shape[1]))
        return res

    monkeypatch.setattr(attn_launch, "attention_bwd_launch", recording)
    return seen


def _draws(c, dev_rnd):
    """The draws both sides use, as float32 CPU tensors for the oracle."""
    if c.kind == "general":
        return F.torch_draws(c)
    d = {"noise": dev_rnd.noise.cpu(), "keep_after": None, "keep_mask": None, "keep_before": None}
    if c.p_drop > 0:
        d.update(keep_after=dev_rnd.keep_after.cpu().float(), keep_mask=dev_rnd.keep_mask.cpu().float())
    return d


def _reference(c):
    key = F.problem_key(c)
    if key not in _REFERENCES:
        pr = F.problem(c)
        draws = _draws(c, A.materialize_randomness(c.B, c.nh, c.L, SEED, c.p_drop, DEV) if c.kind == "train" else None)
        _REFERENCES[key] = (pr, draws, F.oracle_grads(c, pr, draws, pr.cot, torch.float64),
                            F.oracle_grads(c, pr, draws, pr.cot, torch.float32))
    return _REFERENCES[key]


def _kernel_grads(c, pr, draws, cot, twice=False):
    """{leaf: gradient} from A.calibrated_attention and torch autograd over the HIP backward, as CPU tensors."""
    names = F.leaf_names(c)
    x = {k: pr.t[k].to(DEV).requires_grad_(True) for k in names}
    cfg = A.AttentionConfig(n_heads=c.nh, combine_option=c.combine, two_level=c.two_level, rich_calibrated_combine=c.rich,
                            anneal_rate=c.anneal_rate)
    mask = A.StructuredMask(pr.kv.to(DEV), causal=c.causal) if c.mask == "structured" else pr.mask_dense.to(DEV).contiguous()
    if c.mask != "structured":
        assert mask.shape == ((c.B, 1, c.L, c.L) if c.mask == "dense_LL" else (c.B, 1, 1, c.L))
    rnd = None
    if c.kind == "general":
        u8 = lambda t: None if t is None else t.to(torch.uint8).to(DEV)
        rnd = A.ExplicitRandomness(noise=draws["noise"].to(DEV), keep_after=u8(draws["keep_after"]), keep_mask=u8(draws["keep_mask"]),
                                   keep_before=u8(draws["keep_before"]))
    read_rows = pr.rows.to(DEV) if c.pattern in F.READ_ROW_PATTERNS else None
    kw = {k: x[k] for k in names[5:] if k != "gl"}
    ctx_a, ctx_c, M, _ = A.calibrated_attention(x["q"], x["k"], x["v"], x["qa"], x["ka"], x.get("gl"), mask, cfg, p_drop=c.p_drop,
                                                rnd=rnd, seed=None if rnd is not None else SEED, read_rows=read_rows, **kw)
    outs = {"ctx_attacked": ctx_a, "ctx_calibrated": ctx_c, "M": M}
    loss = sum((outs[k] * cot[k].to(DEV)).sum() for k in cot)
    leaves = [x[n] for n in names]
    cpu = lambda gs: {n: torch.zeros_like(pr.t[n]) if g is None else g.detach().cpu().reshape(pr.t[n].shape) for n, g in zip(names, gs)}
    first = cpu(torch.autograd.grad(loss, leaves, retain_graph=twice, allow_unused=True))
    if twice:
        return first, cpu(torch.autograd.grad(loss, leaves, allow_unused=True))
    return first


def _check_form(c, seen):
    """What the library can say about the form that ran: explicit draws or a dense mask reach only the general kernel (every
    tuned launcher refuses them: acattn_launch_bwd_fast / _stream / _onerow); under the automatic choice a read-row pattern
    takes the one-row form, alone or behind the mask-only launch of the split, exactly when the launch writes the gate
    gradient summed over the heads (acattn_calibrated_attention_bwd_gate_summed); a pinned kernel never does.  A pin is
    thereby verified for the read-row patterns only: with a dense pattern the streaming pair and the row-resident kernel
    are not told apart."""
    assert len(seen) >= 1
    for s in seen:
        assert s["rng_mode"] == (_lib.RNG_EXPLICIT if c.kind == "general" else _lib.RNG_COUNTER)
        assert (s["mask_mode"] == _lib.MASK_STRUCTURED) == (c.mask == "structured")
        assert (s["read_rows"] is not None) == (c.pattern in F.READ_ROW_PATTERNS)
        if c.combine != "gate":
            assert s["gate_heads"] is None
            continue
        one_row = (c.kind == "train" and c.pin == "auto" and c.pattern in F.READ_ROW_PATTERNS and
                   attn_launch.gate_summed_rule(c.B, c.L, c.H, c.nh, 1, False, "M" in F.USED_OUTPUTS[c.pattern], False))
        if c.pattern == "calibrated_read_row" and c.kind == "train" and c.pin == "auto":
            assert one_row  # every shape of the table is inside the one-row kernel's domain
        assert s["gate_heads"] == (1 if one_row else c.nh), (c.id, s["gate_heads"])


def _compare(c, tag, got, ref64, ref32):
    failures = []
    for n in F.leaf_names(c):
        abs_e, scale = F.abs_err_and_scale(got[n], ref64[n])
        abs_e32, _ = F.abs_err_and_scale(ref32[n], ref64[n])
        e, e32 = (abs_e / scale, abs_e32 / scale) if scale > 0 else (abs_e, abs_e32)  # (a zero reference: absolute figures)
        print(f"attention_bwd_accuracy case={c.id}{tag} grad=d{n} e={e:.3e} e32={e32:.3e}" + ("" if scale > 0 else " ref64=0"))
        if n in F.TENSOR_GRADS:
            if not e32 <= F.E32_PRECONDITION:
                failures.append(f"d{n}: precondition e32 = {e32:.3e} > {F.E32_PRECONDITION:.0e}")
            bound = F.tensor_bound(e32)
        else:
            bound = F.SCALAR_BOUND
        if not abs_e <= bound * scale + F.ABS_FLOOR:
            failures.append(f"d{n}: e = {e:.3e} > {bound:.3e} (e32 = {e32:.3e}, scale {scale:.3e})")
    return failures


@pytest.mark.parametrize("case", F.CASES, ids=lambda c: c.id)
def test_gradients_match_the_fp64_oracle(case, backward_kernel, launches):
    c = case
    pr, draws, ref64, ref32 = _reference(c)
    assert backward_kernel(PINS[c.pin]) == _lib.BWD_AUTO  # (returns the previous choice: nothing was left pinned)
    got, again = _kernel_grads(c, pr, draws, pr.cot, twice=True)
    assert backward_kernel(_lib.BWD_AUTO) == PINS[c.pin]
    _check_form(c, launches)
    failures = _compare(c, "", got, ref64, ref32)
    assert not failures, f"{c.id}: " + "; ".join(failures)
    same_bits = all(torch.equal(got[n], again[n]) for n in ("q", "k", "v"))
    print(f"attention_bwd_accuracy case={c.id} second_walk_equal_bits_dq_dk_dv={same_bits}")
    if c.kind == "general":
        for n in ("q", "k", "v"):
            assert torch.equal(again[n], got[n]) or F.err(again[n], got[n]) <= 1e-5, f"d{n} differs between two walks"


_LEFT_PAD = [c for c in F.CASES if c.left_pad]  # the row-resident kernel (automatic at L = 50) and the streaming pair
_DEAD_ROWS = {}
# The one (case, gradient) pair left failing, strictly (figures of profiles/attention_bwd_accuracy.txt).
_DSCALAR_REASON = (
    "left_pad-all-auto, dscalar of the fully masked rows alone: e = 4.667e-3 against the fp32 oracle (cap 2e-3), 6.682e-3 "
    "against the fp64 oracle, e32 = 2.006e-3 (fp32 against fp64 oracle: the size of the -10000 quantisation itself in this "
    "sum).  Narrowed by elimination to the row-resident kernel's fully masked rows (csrc/acattn_bwd_fast.hip): on the same "
    "inputs and draws the general kernel is at 6.1e-4 and the streaming pair at 7.9e-4 of the fp32 oracle, and the live rows "
    "of the same case at 3.7e-6 of the fp64 one.  The term is only SUPPOSED, not shown: the kernel rebuilds such a row's "
    "probabilities as ex2(u * log2e + (mask4(t) - lse)), the fill added in log2 units (s_km = -10000 * log2e) to an "
    "un-quantised argument, where the forward (deadq, acattn_fwd_body.inc) adds -10000 in natural units, rounds in fp32 and "
    "takes it out again before it saves the normalisers (DESIGN 4.1b, VERDICT weak 2).  The streaming pair does not quantise "
    "either and stays inside the cap, so this alone does not explain the factor 6 between the two; dscalar is a cancelling "
    "sum and the one gradient past the cap")


def _dead_rows(c):
    if c.id not in _DEAD_ROWS:
        pr, draws, _, _ = _reference(c)
        if not pr.dead.any():  # (no AssertionError here: the strict xfail below expects one from the comparison alone)
            raise RuntimeError(f"{c.id}: no fully masked row")
        lib = _lib.load()
        lib.acattn_select_backward_kernel(PINS[c.pin])
        try:
            got = _kernel_grads(c, pr, draws, pr.cot_dead)
        finally:
            lib.acattn_select_backward_kernel(_lib.BWD_AUTO)
        _DEAD_ROWS[c.id] = dict(got=got, ref32=F.oracle_grads(c, pr, draws, pr.cot_dead, torch.float32),
                                ref64=F.oracle_grads(c, pr, draws, pr.cot_dead, torch.float64))
    return _DEAD_ROWS[c.id]


def _dead_row_params():
    for c in _LEFT_PAD:
        for n in F.leaf_names(c):
            marks = [pytest.mark.xfail(strict=True, raises=AssertionError, reason=_DSCALAR_REASON)] if (c.pin, n) == ("auto", "scalar") else []
            yield pytest.param(c, n, marks=marks, id=f"{c.id}-d{n}")


@pytest.mark.parametrize("case,grad", list(_dead_row_params()))
def test_fully_masked_rows_match_the_fp32_oracle(case, grad):
    """The fully masked rows of the left-padded sequence alone (their cotangents only), against the FLOAT32 oracle, which
    quantises them as the reference's fp32 `+ (-10000)` does, at the 2e-3 cap of every gradient test; the figure against the
    float64 oracle, which does not quantise, and e32 between the two oracles are printed next to it.  With the streaming
    pair pinned this is the case that showed two defects of its key kernel under left padding: it left out the key tiles
    behind a query block with a fully masked row, and the rows past L of the last query block borrowed a fully masked
    row 0's shifted normaliser, against which their mask fill cancelled (dk, dv, dka, dw_order, dw_dist were 0.75 to 1.03
    of their scale off).  One pair misses the cap and is left as a strict xfail: _DSCALAR_REASON."""
    d = _dead_rows(case)
    abs_e, scale = F.abs_err_and_scale(d["got"][grad], d["ref32"][grad])
    abs_e64, scale64 = F.abs_err_and_scale(d["got"][grad], d["ref64"][grad])
    print(f"attention_bwd_accuracy case={case.id} fully_masked_rows grad=d{grad} e_vs_fp32={abs_e / scale:.3e} "
          f"e_vs_fp64={abs_e64 / scale64:.3e} e32={F.err(d['ref32'][grad], d['ref64'][grad]):.3e}")
    assert abs_e <= 2e-3 * scale + F.ABS_FLOOR, f"d{grad}: {abs_e:.3e} of {scale:.3e}"
