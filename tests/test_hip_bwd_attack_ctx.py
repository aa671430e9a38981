"""GPU suite (-m gpu): the CTX form of the attack-side backward (csrc/acattn_bwd_attack.hip) -- dqa and dka of an
attack-only launch that carries a dense cotangent of the calibrated context and no cotangent of the attacked one (layer 0 of
the attacked-loss walk) -- against the oracle differentiated by torch autograd in FLOAT64.

Cases, inputs, cotangent forms and the oracle are tests/_bwd_attack_ctx_cases.py's (tests/test_bwd_attack_ctx_cases_cpu.py
asserts the table's conditioning without a GPU); the bounds are tests/_attention_fp64.py's: e = max|got - ref64| / max|ref64|
<= tensor_bound(e32) with the precondition e32 <= E32_PRECONDITION and the absolute floor ABS_FLOOR.  The oracle is fed the
kernels' own counter draws (A.materialize_randomness).  The launches are issued directly
(attn_launch.attention_bwd_launch(..., d_cal=..., d_pen=... / d_M=..., attack_only=True, poison=True)).  Each case asserts
that no NaN is left in the poisoned outputs, that a second launch gives the same bits, that the automatic choice passes the
bound and that the row-resident kernel (ACATTN_BWD_ROW pinned, which never takes the attack-side launcher) passes the same
bound on the same inputs.

Which kernel served the automatic launch: acattn_calibrated_attention_bwd_attack_side issues the same arguments on
acattn_bwd_attack.hip or not at all (0 / -100).  Each case expects 0 from it and the bits of the automatic launch (the
kernel is bit-stable from launch to launch; the row-resident kernel sums dka in another order and through LDS atomics).

The left-padded sequence (valid from key 20 on, L = 50: blocks 0 and 1 see no key and spread over every tile, so the
workgroup's 15 tiles do not fit the 10 slots and its waves take turns) is checked as tests/test_hip_bwd_attack.py checks it:
the live rows against the float64 oracle, the dead rows' cotangents alone against the float32 oracle at the 2e-3 cap.
"""
import pytest
import torch

import ac_tsr_amd as A
from ac_tsr_amd import _lib, attn_launch, ops
from tests import _attention_fp64 as F
from tests import _bwd_attack_ctx_cases as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 777
_CACHE = {}


def _setup(c, left_pad=False):
    key = (c.id, left_pad)
    if key not in _CACHE:
        pr = T.problem(c, left_pad)
        rnd = A.materialize_randomness(c.B, c.nh, c.L, SEED, c.p_drop, DEV)
        draws = {"noise": rnd.noise.cpu(), "keep_after": None, "keep_mask": None}
        if c.p_drop > 0:
            draws.update(keep_after=rnd.keep_after.cpu().float(), keep_mask=rnd.keep_mask.cpu().float())
        _CACHE[key] = (pr, draws, T.cotangents(c, pr), {})
    return _CACHE[key]


def _references(c, left_pad, form, dead, dtypes):
    pr, draws, cots, refs = _setup(c, left_pad)
    for dt in dtypes:
        if (form, dead, dt) not in refs:
            refs[(form, dead, dt)] = T.oracle(c, pr, draws, *T.form_cotangents(cots, form, dead), dt)
    return [refs[(form, dead, dt)] for dt in dtypes]


class _AttackSideOnly:
    """The library with acattn_calibrated_attention_bwd replaced by the entry that launches acattn_bwd_attack.hip or nothing."""

    def __init__(self, lib):
        self._lib = lib
        self.acattn_calibrated_attention_bwd = lib.acattn_calibrated_attention_bwd_attack_side

    def __getattr__(self, name):
        return getattr(self._lib, name)


def _forward(c, pr):
    """(prob, x, M, stats, keep-alive) of one forward launch on the case's inputs."""
    lib = _lib.load()
    x = {k: v.to(DEV) for k, v in pr.t.items()}
    cfg = A.AttentionConfig(n_heads=c.nh, combine_option="gate", two_level=True)
    mask = A.StructuredMask(pr.kv.to(DEV), causal=c.causal)
    keep = [x, mask]
    flat = lambda t: t.reshape(-1).contiguous()
    prob = ops._fill_problem(x["q"], x["k"], x["v"], x["qa"], x["ka"], x["gl"], mask, flat(x["w_order"]), x["b_order"],
                             flat(x["w_dist"]), x["b_dist"], x["scalar"], None, cfg, c.p_drop, None, SEED, keep)
    _, _, M, stats, _, _ = attn_launch.attention_fwd_launch(lib, prob, x["q"], c.nh, adversarial=True, want_penalty=False)
    return prob, x, M, stats, keep


def _backward(c, fwd, cot, pin=_lib.BWD_AUTO, direct=False, poison=True, d_att=None):
    """(dqa, dka) on the device of one attack-only launch; `cot` = (d_cal, d_M, d_pen) on the device."""
    lib = _lib.load()
    prob, x, M, stats, _ = fwd
    old = lib.acattn_select_backward_kernel(pin)
    try:
        res = attn_launch.attention_bwd_launch(_AttackSideOnly(lib) if direct else lib, prob, x["q"], c.nh, M, stats, d_att=d_att,
                                               d_cal=cot[0], d_M=cot[1], d_pen=cot[2], attack_only=True, poison=poison)
    finally:
        lib.acattn_select_backward_kernel(old)
    return res[3], res[4]


def _dev(cot):
    return tuple(None if t is None else t.to(DEV).contiguous() for t in cot)


def _launch(c, pr, cot, **kw):
    got = _backward(c, _forward(c, pr), _dev(cot), **kw)
    torch.cuda.synchronize()
    return {"qa": got[0].cpu(), "ka": got[1].cpu()}


def _failures(tag, got, ref64, ref32):
    out = []
    for n in ("qa", "ka"):
        abs_e, scale = F.abs_err_and_scale(got[n], ref64[n])
        abs_e32, _ = F.abs_err_and_scale(ref32[n], ref64[n])
        e, e32 = abs_e / scale, abs_e32 / scale
        print(f"bwd_attack_ctx_accuracy case={tag} grad=d{n} e={e:.3e} e32={e32:.3e}")
        if not e32 <= F.E32_PRECONDITION:
            out.append(f"d{n}: precondition e32 = {e32:.3e} > {F.E32_PRECONDITION:.0e}")
        if not abs_e <= F.tensor_bound(e32) * scale + F.ABS_FLOOR:
            out.append(f"d{n}: e = {e:.3e} > {F.tensor_bound(e32):.3e} (e32 = {e32:.3e}, scale {scale:.3e})")
    return out


def _check_case(c, left_pad, form):
    pr, draws, cots, _ = _setup(c, left_pad)
    ref64, ref32 = _references(c, left_pad, form, False, (torch.float64, torch.float32))
    cot = T.form_cotangents(cots, form)
    got = _launch(c, pr, cot)
    for n in ("qa", "ka"):
        assert not torch.isnan(got[n]).any(), f"d{n}: an element below L was not written"
    again = _launch(c, pr, cot)
    for n in ("qa", "ka"):
        assert torch.equal(got[n], again[n]), f"d{n} differs between two launches"
    side = _launch(c, pr, cot, direct=True)  # (raises where the attack-side launcher answers -100)
    for n in ("qa", "ka"):
        assert torch.equal(got[n], side[n]), f"d{n}: the automatic launch did not run the attack-side kernel"
    failures = _failures(f"{c.id}-{form}-auto", got, ref64, ref32)
    row = _launch(c, pr, cot, pin=_lib.BWD_ROW)
    failures += [f"(row-resident) {f}" for f in _failures(f"{c.id}-{form}-row", row, ref64, ref32)]
    assert not failures, f"{c.id}-{form}: " + "; ".join(failures)


@pytest.mark.parametrize("form", T.FORMS)
@pytest.mark.parametrize("case", T.SHAPES, ids=lambda c: c.id)
def test_dqa_dka_match_the_fp64_oracle(case, form):
    _check_case(case, False, form)


def test_left_padded_live_rows_match_the_fp64_oracle():
    """The context cotangent and a dense d M on the live rows (the fully masked rows' cotangents zeroed)."""
    _check_case(T.LEFT_PAD, True, "cal_dM")


def test_left_padded_dead_rows_match_the_fp32_oracle():
    """The fully masked rows' cotangents alone against the FLOAT32 oracle at the 2e-3 cap
    (tests/test_hip_attention_bwd_fp64.py::test_fully_masked_rows_match_the_fp32_oracle's check)."""
    c = T.LEFT_PAD
    pr, draws, cots, _ = _setup(c, True)
    assert pr.dead.any()
    for form in ("cal", "cal_dM"):
        (ref32,) = _references(c, True, form, True, (torch.float32,))
        got = _launch(c, pr, T.form_cotangents(cots, form, dead=True))
        for n in ("qa", "ka"):
            assert not torch.isnan(got[n]).any()
            abs_e, scale = F.abs_err_and_scale(got[n], ref32[n])
            print(f"bwd_attack_ctx_accuracy case={c.id}-{form} fully_masked_rows grad=d{n} e_vs_fp32={abs_e / scale:.3e}")
            assert scale > 0 and abs_e <= 2e-3 * scale + F.ABS_FLOOR, f"{form} d{n}: {abs_e:.3e} of {scale:.3e}"


def test_a_cotangent_of_the_attacked_context_stays_on_the_row_resident_kernel():
    c = T.SHAPES[0]
    pr, draws, cots, _ = _setup(c)
    cot = _dev(T.form_cotangents(cots, "cal_dpen"))
    with pytest.raises(_lib.AcattnError, match="rc=-100"):
        _backward(c, _forward(c, pr), cot, direct=True, d_att=cot[0])
    torch.cuda.synchronize()


def test_graph_replay_gives_the_eager_bits():
    c = T.REPLAY
    pr, draws, cots, _ = _setup(c)
    cot = _dev(T.form_cotangents(cots, "cal_dpen"))
    fwd = _forward(c, pr)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [t.clone() for t in _backward(c, fwd, cot)]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert not any(torch.isnan(t).any() for t in eager)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = _backward(c, fwd, cot, poison=False)  # (a NaN fill would be one more captured node per buffer)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for n, a, b in zip(("qa", "ka"), got, eager):
        assert torch.equal(a, b), f"d{n}: eager and replayed graph differ by {(a - b).abs().max().item():.3e}"
