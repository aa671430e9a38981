"""GPU suite: the penalty row sums of the streaming forward at L <= 64 (acattn_fwd_out.penalty_part).

The 4-tile form of acattn_fwd_stream_kernel sums (1 - M)^2 over the block of M it staged in LDS (p_drop = 0.5; every other
instantiation leaves the sums to acattn_mask_penalty_rows behind the launch).  Whichever way they come about, every
entry [b, head, query block] must be written, must equal the fp64 sum over the M of the SAME launch within the rounding
of an fp32 sum of that many terms, and asking for the sums must not change anything else the launch writes.

The bound is derived, not tuned: a block has n_t <= 16 L <= 1,024 terms, each (1 - M)^2 carries at most three roundings
(the difference, the square, its entry into a sum), and an fp32 sum of n_t non-negative terms in any order is within
(n_t - 1) 2^-24 of the exact sum, relatively: |pen - sum64| <= (n_t + 3) 2^-24 sum64."""
import ctypes as C
import itertools

import pytest
import torch

from ac_tsr_amd import _lib, attn_launch

pytestmark = pytest.mark.gpu

B, NH = 4, 2
LENGTHS = (1, 15, 16, 17, 33, 48, 50, 64)
CASES = ([(L, dh, p, causal, True) for L, dh, p, causal in itertools.product(LENGTHS, (16, 32, 64), (0.5, 0.1), (True, False))]
         + [(L, 32, 0.5, causal, False) for L, causal in itertools.product(LENGTHS, (True, False))])


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _key_valid(L, dev):
    """Sequence 0 right-padded, 1 left-padded (the first rows of its first query block see no valid key under the causal
    mask: from L = 17 on that is the whole block), 2 full length, 3 without any valid key (under either mask)."""
    pos = torch.arange(L)
    n_right = max(1, L // 2)
    n_left = max(1, L // 3) if L > 1 else 0
    kv = torch.stack([pos < n_right, pos >= L - n_left if L > 16 else pos >= min(L - 1, 1), torch.ones(L, dtype=torch.bool),
                      torch.zeros(L, dtype=torch.bool)])
    return kv.to(torch.uint8).to(dev)


def _inputs(L, dh, p_drop, causal, pre, dev):
    H = NH * dh
    gen = torch.Generator().manual_seed(1000 * L + dh)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev)
    q, k, v, qa, ka = (rnd(B, L, H) for _ in range(5))
    gate = rnd(B, L, L)
    w_order, b_order, w_dist, b_dist = (0.1 * rnd(2 * dh), 0.1 * rnd(1), 0.1 * rnd(2 * dh), 0.1 * rnd(1))
    scalar = rnd(1)
    kv = _key_valid(L, dev)
    keep = [q, k, v, qa, ka, gate, w_order, b_order, w_dist, b_dist, scalar, kv]
    prob = attn_launch.fill_problem(q, k, v, qa, ka, gate, w_order, b_order, w_dist, b_dist, scalar, NH, p_drop, 4321, None,
                                    key_valid=kv, causal=causal)
    if pre:  # the producer's extras, as the training step hands them over: affine planes and gate probabilities
        lib = _lib.load()
        affine = torch.zeros(B, NH, 4, 16 * ((L + 15) // 16), device=dev)
        _lib.check(lib.acattn_spatial_affines(C.byref(prob), affine.data_ptr(), _stream()), "spatial_affines")
        gate_p = torch.sigmoid(gate)
        prob.affine, prob.gate_logits, prob.gate_is_prob = affine.data_ptr(), gate_p.data_ptr(), 1
        keep += [affine, gate_p]
    return prob, q, keep


def _launch(prob, q, with_pen):
    lib = _lib.load()
    Bq, L, H = q.shape
    nan = float("nan")
    ctx_a, ctx_c = torch.full_like(q, nan), torch.full_like(q, nan)
    M = torch.full((Bq, NH, L, L), nan, device=q.device)
    stats = torch.full((Bq, NH, L, _lib.NSTAT), nan, device=q.device)
    pen = torch.full((Bq, NH, (L + 15) // 16), nan, device=q.device) if with_pen else None
    out = _lib.FwdOut()
    out.ctx_attacked, out.ctx_calibrated, out.attack_mask, out.row_stats = (t.data_ptr() for t in (ctx_a, ctx_c, M, stats))
    if with_pen:
        out.penalty_part = pen.data_ptr()
    _lib.check(lib.acattn_calibrated_attention_fwd(C.byref(prob), C.byref(out), _stream()), "calibrated_attention_fwd")
    return ctx_a, ctx_c, M, stats, pen


def _reference(M):
    """fp64 sums of (1 - M)^2 per (b, head, query block), the number of terms of each block."""
    Bq, nh, L, _ = M.shape
    nT = (L + 15) // 16
    d2 = (1.0 - M.double()) ** 2
    row = d2.sum(-1)  # [B, nh, L]
    row = torch.nn.functional.pad(row, (0, 16 * nT - L)).view(Bq, nh, nT, 16).sum(-1)
    terms = torch.tensor([min(16, L - 16 * qb) * L for qb in range(nT)], device=M.device, dtype=torch.float64)
    return row, terms


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("L,dh,p_drop,causal,pre", CASES)
def test_penalty_sums_of_the_4_tile_forward(L, dh, p_drop, causal, pre):
    dev = torch.device("cuda:0")
    prob, q, keep = _inputs(L, dh, p_drop, causal, pre, dev)
    ctx_a, ctx_c, M, stats, pen = _launch(prob, q, True)
    ctx_a0, ctx_c0, M0, stats0, _ = _launch(prob, q, False)
    assert bool(torch.isfinite(pen).all()), "an entry of penalty_part was not written"
    assert bool(torch.isfinite(M).all())
    ref, terms = _reference(M)
    bound = (terms + 3.0) * 2.0 ** -24 * ref
    err = (pen.double() - ref).abs()
    assert bool((err <= bound).all()), f"launch: max err / bound = {(err / bound.clamp_min(1e-300)).max().item():.3f}"
    # the path it replaces meets the same bound on the same mask
    pen_rows = torch.full_like(pen, float("nan"))
    lib = _lib.load()
    _lib.check(lib.acattn_mask_penalty_rows(M.data_ptr(), B, NH, L, pen_rows.data_ptr(), _stream()), "mask_penalty_rows")
    err_rows = (pen_rows.double() - ref).abs()
    assert bool((err_rows <= bound).all()), f"penalty_rows: max err / bound = {(err_rows / bound.clamp_min(1e-300)).max().item():.3f}"
    # asking for the sums changes nothing else
    for name, a, b in (("ctx_attacked", ctx_a, ctx_a0), ("ctx_calibrated", ctx_c, ctx_c0), ("attack_mask", M, M0),
                       ("row_stats", stats, stats0)):
        assert torch.equal(_bits(a), _bits(b)), f"{name} differs between a launch with and one without penalty_part"
