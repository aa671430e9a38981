"""GPU suite (-m gpu): every form of the calibrated attention forward against the float64 oracle at tile-edge lengths.

Cases: tests/_fwd_edge_cases.py (tests/test_fwd_edge_cases_cpu.py checks the table, its form column and its conditioning
without a GPU).  Each case goes through the C ABI (acattn_calibrated_attention_fwd) with the kernel pinned by
acattn_select_forward_kernel:

  * every output pointer (ctx_attacked, ctx_calibrated, attack_mask, row_stats, penalty_part) lies inside a guarded,
    poisoned buffer (tests/_guarded.py) and every input inside a guarded input buffer: a store in front of or behind an
    output, an element left unwritten, a NaN read from behind an input, or a written input fails check_all;
  * row_stats: include/acattn.h promises "log-normalisers for the backward" and names no slot, so what is held to the
    oracle is what the backward kernels read -- slots 0..4 (the five soft-maxes), slot 5 under combine `fixed` (the inner,
    un-masked soft-max) and slot 6 under two_level = 0 (the plain soft-max); the remaining slots may be left unwritten;
  * counter-RNG cases feed the oracle the kernel's own draws (acattn_rng_materialize), explicit cases hand
    tests/_attention_fp64.torch_draws to both sides;
  * every case launches twice, into fresh poison, and the outputs must be bit-identical.

Bounds (the project's own: tests/test_hip_onehop.py, tests/test_hip_long_sequences.py, now against float64):
  live rows (at least one allowed key)   |M - ref64| <= 5e-6, both contexts <= 1e-4, the normalisers <= 1e-4
  fully masked rows                      M and the contexts within 2e-3 of the float32 oracle's scale there (it quantises
                                         them as the reference's fp32 `+ (-10000)` does); their normalisers carry the
                                         -10000: two fp32 roundings at that magnitude on top of the live bound
  penalty_part                           (n_t + 3) 2^-24 of the fp64 sum over the launch's own M
                                         (derived in tests/test_hip_fwd_penalty_fused.py)
Fully masked rows and the rows of padded positions feed nothing the losses read.

A HIP error ends the module: the cases after it fail without touching the GPU."""
import ctypes as C
import math

import pytest
import torch

import ac_tsr_amd as A
from ac_tsr_amd import _lib, attn_launch
from tests import _attention_fp64 as F
from tests import _attention_fwd_ref as R
from tests import _fwd_edge_cases as E
from tests._guarded import check_all, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 4321
PINS = {"auto": _lib.FWD_AUTO, "stream": _lib.FWD_STREAM, "staged": _lib.FWD_STAGED, "general": _lib.FWD_GENERAL,
        "long": _lib.FWD_LONG}
_BROKEN = []


@pytest.fixture
def pin():
    """Pins the forward kernel for one test and restores the automatic choice."""
    lib = _lib.load()

    def select(name):
        lib.acattn_select_forward_kernel(PINS[name])
        return lib
    yield select
    lib.acattn_select_forward_kernel(_lib.FWD_AUTO)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _affine_planes(t, nh):
    """The producer's affine planes in fp64 on the host (tests/test_hip_onehop.py::_affine_planes)."""
    B, L, H = t["q"].shape
    dh = H // nh
    LP = 16 * ((L + 15) // 16)
    q = t["q"].double().view(B, L, nh, dh).permute(0, 2, 1, 3)
    k = t["k"].double().view(B, L, nh, dh).permute(0, 2, 1, 3)
    wo, wd = t["w_order"].double().reshape(-1), t["w_dist"].double().reshape(-1)
    l2e = 1.0 / math.log(2.0)
    planes = torch.zeros(B, nh, 4, LP, dtype=torch.float64)
    planes[:, :, 0, :L] = -l2e * (q @ wo[:dh] + t["b_order"].double())
    planes[:, :, 1, :L] = q @ wd[:dh] + t["b_dist"].double()
    planes[:, :, 2, :L] = -l2e * (k @ wo[dh:])
    planes[:, :, 3, :L] = k @ wd[dh:]
    return planes.float()


def _inputs(c, pr, draws):
    """(acattn_problem, {name: guarded input buffer}).  Every tensor the problem points to lies between guards."""
    B, L, H, nh = c.B, c.L, c.H, c.nh
    dh = H // nh
    g = {}

    def put(name, t, width):
        g[name] = guarded(tuple(t.shape), t.dtype, DEV, width, t.contiguous().to(DEV))
        return g[name].t

    x = {k: put(k, pr.t[k], H) for k in ("q", "k", "v", "qa", "ka")}
    gate = None
    if c.adversarial and c.combine == "gate":
        # the producer's probabilities: one sigmoid per (b, i, j), in fp64 here
        gate = put("gate", torch.sigmoid(pr.t["gl"].double()).float() if c.extras else pr.t["gl"], L)
    par = {k: put(k, pr.t[k].reshape(-1), 2 * dh) for k in ("w_order", "b_order", "w_dist", "b_dist", "scalar")}
    kw = {}
    if c.mask == "structured":
        kw.update(key_valid=put("key_valid", pr.kv, L), causal=c.causal)
    else:
        kw.update(mask=put("mask", pr.mask_dense, L), mask_mode=_lib.MASK_DENSE_LL if c.mask == "dense_LL" else _lib.MASK_DENSE_L)
    if not c.two_level:
        kw.update(two_level=False, rich=c.rich, rich_ratio=put("rich_ratio", pr.t["rich_ratio"], 1) if c.rich == "trainable" else None)
    rnd = None
    if c.kind == "general":
        u8 = lambda name: None if draws[name] is None else put(name, draws[name].to(torch.uint8), L)
        rnd = (put("noise", draws["noise"], L), u8("keep_after"), u8("keep_mask"), u8("keep_before"))
    if c.extras:
        kw.update(affine=put("affine", _affine_planes(pr.t, nh), 16 * ((L + 15) // 16)), gate_is_prob=c.adversarial)
    prob = attn_launch.fill_problem(x["q"], x["k"], x["v"], x["qa"], x["ka"], gate,
                                    par["w_order"] if "order" in c.terms else None, par["b_order"],
                                    par["w_dist"] if "distance" in c.terms else None, par["b_dist"], par["scalar"], nh, c.p_drop,
                                    SEED, None, adversarial=c.adversarial, combine=c.combine, anneal_rate=c.anneal_rate, rnd=rnd, **kw)
    return prob, g


def _checked_slots(c):
    return [0, 1, 2, 3, 4] + ([5] if c.combine == "fixed" else []) + ([] if c.two_level else [6])


def _launch(c, lib, prob, inputs):
    """One launch into fresh guarded, poisoned outputs; check_all over outputs and inputs; the outputs by name."""
    B, L, H, nh = c.B, c.L, c.H, c.nh
    nT = (L + 15) // 16
    out = {"ctx_calibrated": guarded((B, L, H), torch.float32, DEV, H, "poison")}
    if c.adversarial:
        out.update(ctx_attacked=guarded((B, L, H), torch.float32, DEV, H, "poison"),
                   attack_mask=guarded((B, nh, L, L), torch.float32, DEV, L, "poison"),
                   row_stats=guarded((B, nh, L, _lib.NSTAT), torch.float32, DEV, _lib.NSTAT, "poison"),
                   penalty_part=guarded((B, nh, nT), torch.float32, DEV, nT, "poison"))
    o = _lib.FwdOut()
    for name, buf in out.items():
        setattr(o, name, buf.t.data_ptr())
    _lib.check(lib.acattn_calibrated_attention_fwd(C.byref(prob), C.byref(o), _stream()), "calibrated_attention_fwd")
    torch.cuda.synchronize()
    unwritten = None
    if c.adversarial:
        free = torch.ones(_lib.NSTAT, dtype=torch.bool)
        free[_checked_slots(c)] = False
        unwritten = {"row_stats": free.expand(B, nh, L, _lib.NSTAT).contiguous()}
    check_all(out, unwritten)
    check_all(inputs)
    return {name: buf.t for name, buf in out.items()}


def _draws(c):
    if c.kind == "general":
        return F.torch_draws(c)
    rnd = A.materialize_randomness(c.B, c.nh, c.L, SEED, c.p_drop, DEV)
    keep = lambda t: t.cpu().float() if c.p_drop > 0 else None
    return {"noise": rnd.noise.cpu(), "keep_after": keep(rnd.keep_after), "keep_mask": keep(rnd.keep_mask),
            "keep_before": keep(rnd.keep_before)}


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("case", E.CASES, ids=lambda c: c.id)
def test_forward_matches_the_fp64_oracle_inside_guards(case, pin):
    c = case
    if _BROKEN:
        pytest.fail(f"not run: an earlier case ended in a HIP error ({_BROKEN[0]})")
    lib = pin(c.fpin)
    pr = R.edge_problem(c, seed=c.seed)
    try:
        draws = _draws(c)
        prob, inputs = _inputs(c, pr, draws)
        first = _launch(c, lib, prob, inputs)
        second = _launch(c, lib, prob, inputs)
        dev_out = first
        first = {k: v.cpu() for k, v in first.items()}
        identical = {k: torch.equal(_bits(dev_out[k]), _bits(second[k])) for k in dev_out}
    except RuntimeError as e:  # torch's HIP errors; _lib.AcattnError is one too
        if not isinstance(e, _lib.AcattnError) or "HIP launch failed" in str(e):  # (a refusal of the entry point is an ordinary failure)
            _BROKEN.append(f"{c.id}: {e}")
        raise
    assert all(identical.values()), f"{c.id}: two launches differ in {[k for k, v in identical.items() if not v]}"

    ref32, ref64 = R.oracle_forward(c, pr, draws, torch.float32), R.oracle_forward(c, pr, draws, torch.float64)
    if c.adversarial:
        stats = first["row_stats"]
        got = {"M": first["attack_mask"], "ctx_attacked": first["ctx_attacked"], "ctx_calibrated": first["ctx_calibrated"],
               "row_stats": stats[..., :5]}
        if c.combine == "fixed":
            got["lse_f"] = stats[..., 5]
        if not c.two_level:
            got["lse_b"] = stats[..., 6]
    else:
        got = {"ctx_spatial": first["ctx_calibrated"]}
    bounds = {"M": R.M_BOUND, "ctx_attacked": R.CTX_BOUND, "ctx_calibrated": R.CTX_BOUND, "ctx_spatial": R.CTX_BOUND,
              "row_stats": R.STAT_BOUND, "lse_f": R.STAT_BOUND, "lse_b": R.STAT_BOUND}
    errs = R.edge_errors(pr, got, ref32, ref64)
    line = f"fwd_edges_accuracy case={c.id} " + " ".join(f"{k}={v[0]:.3e} {k}_dead={v[1]:.3e}/{v[2]:.3e}" for k, v in errs.items())

    pen_fail = None
    if c.adversarial:
        # penalty_part against the fp64 sums over the M of the same launch
        M = first["attack_mask"].double()
        nT = (c.L + 15) // 16
        row = torch.nn.functional.pad(((1.0 - M) ** 2).sum(-1), (0, 16 * nT - c.L)).view(c.B, c.nh, nT, 16).sum(-1)
        terms = torch.tensor([min(16, c.L - 16 * qb) * c.L for qb in range(nT)], dtype=torch.float64)
        pen_err = (first["penalty_part"].double() - row).abs()
        ratio = (pen_err / ((terms + 3.0) * 2.0 ** -24 * row).clamp_min(1e-300)).max().item()
        line += f" penalty_part_err_over_bound={ratio:.3f}"
        if ratio > 1.0:
            pen_fail = f"penalty_part: max err / bound = {ratio:.3f}"
    print(line)

    failures = [] if pen_fail is None else [pen_fail]
    for k, (e_live, e_dead, scale) in errs.items():
        if not e_live <= bounds[k]:
            failures.append(f"{k}: {e_live:.3e} from the fp64 oracle on live rows (> {bounds[k]:.0e})")
        dead_bound = R.DEAD_STAT_BOUND + R.STAT_BOUND if k in ("row_stats", "lse_f", "lse_b") else R.DEAD_CAP * scale + F.ABS_FLOOR
        if not e_dead <= dead_bound:
            failures.append(f"{k}: fully masked rows {e_dead:.3e} of {scale:.3e} (> {dead_bound:.3e})")
    assert not failures, f"{c.id}: " + "; ".join(failures)
