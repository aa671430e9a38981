"""GPU suite (-m gpu): the fused layer tail at hidden 128 / inner 64, the shape of three of the four shipped dataset
configurations (yelp, amazon-sports-outdoors, amazon-toys-games).

The inputs, the fp64 chain and the tolerances are those of tests/test_hip_tail.py (the project's for hidden 128; the inner
sums here are shorter): output 3e-5 absolute, gradients 2e-4 of the tensor's largest magnitude + 1e-6.  Row counts: 37 (a
ragged last row block), 512 (several waves per row block: two in the forward, four in the backward), 8192 and 8213 (both
sides of the boundary between that form and the staged one).  Every figure is printed before it is asserted (pytest -s shows them)."""
import ctypes as C

import pytest
import torch

from ac_tsr_amd import _lib, tail
from ac_tsr_amd.ops import _ptr, _stream
from ac_tsr_amd.state import StepState
from tests.test_hip_tail import NAMES, _apply, _inputs, _reference

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, I = 128, 64
EPS = 1e-12


@pytest.mark.parametrize("rows", [37, 512, 8192, 8213])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_fused_tail_128_64_matches_fp64_chain(rows, p):
    t, g = _inputs(rows, H, I, seed=rows + I)
    keep1 = torch.empty(rows, H).bernoulli_(1 - p, generator=g) if p > 0 else None
    keep2 = torch.empty(rows, H).bernoulli_(1 - p, generator=g) if p > 0 else None
    cot = torch.randn(rows, H, generator=g)
    d, ref = _reference(t, keep1, keep2, p, EPS)
    want = torch.autograd.grad((ref * cot.double()).sum(), [d[k] for k in NAMES])
    dev = {k: v.to(DEV).requires_grad_(True) for k, v in t.items()}
    to = lambda k: None if k is None else k.to(DEV)
    out = _apply(tail._FusedLayerTail, dev, EPS, p, to(keep1), to(keep2), 0, 0, StepState())
    err = (out.detach().cpu() - ref.detach().float()).abs().max().item()
    print(f"rows {rows} p {p}: out {err:.3e}")
    assert err <= 3e-5
    got = torch.autograd.grad((out * cot.to(DEV)).sum(), [dev[k] for k in NAMES], retain_graph=True)
    for k, gv, wv in zip(NAMES, got, want):
        err, scale = (gv.cpu() - wv.float()).abs().max().item(), wv.abs().max().item()
        print(f"rows {rows} p {p}: d{k} {err:.3e} of {scale:.3e}")
        assert err <= 2e-4 * scale + 1e-6, (k, err)
    # the attack pass skips the parameter gradients and returns the same input gradients
    st = StepState()
    out2 = _apply(tail._FusedLayerTail, dev, EPS, p, to(keep1), to(keep2), 0, 0, st)
    with st.attack_pass():
        gc, gx = torch.autograd.grad((out2 * cot.to(DEV)).sum(), [dev["c"], dev["x"]])
    assert torch.equal(gc, got[0]) and torch.equal(gx, got[1])


@pytest.mark.parametrize("rows", [512, 8213])
def test_fused_tail_128_64_counter_dropout_equals_unfused_node(rows):
    """In-kernel dropout: same seeds, same keep decisions as the unfused node; another seed differs; a repeat is bit-equal."""
    p = 0.5
    t, g = _inputs(rows, H, I, seed=7)
    cot = torch.randn(rows, H, generator=g).to(DEV)
    dev = {k: v.to(DEV).requires_grad_(True) for k, v in t.items()}
    outs, grads = [], []
    for node in (tail._FusedLayerTail, tail._LayerTail):
        out = _apply(node, dev, EPS, p, None, None, 1234, 99, StepState())
        outs.append(out)
        grads.append(torch.autograd.grad((out * cot).sum(), [dev[k] for k in NAMES]))
    err = (outs[0] - outs[1]).abs().max().item()
    print(f"rows {rows}: fused - unfused out {err:.3e}")
    assert err <= 3e-5
    for k, a, b in zip(NAMES, *grads):
        assert (a - b).abs().max() <= 2e-4 * b.abs().max() + 1e-6, k
    other = _apply(tail._FusedLayerTail, dev, EPS, p, None, None, 1235, 99, StepState())
    assert (other - outs[0]).abs().max() > 0.1
    again = _apply(tail._FusedLayerTail, dev, EPS, p, None, None, 1234, 99, StepState())
    assert torch.equal(again, outs[0])


def test_fused_tail_128_64_row_selection_equals_gather_then_tail():
    B, L, R, p = 37, 50, 3, 0.5
    t, g = _inputs(B * L, H, I, seed=11)
    pick = torch.randint(0, L, (B, R), generator=g)
    cot = torch.randn(B, R, H, generator=g).to(DEV)
    dev = {k: v.to(DEV).requires_grad_(True) for k, v in t.items()}
    c3, x3 = dev["c"].view(B, L, H), dev["x"].view(B, L, H)
    idx = pick.to(DEV)
    args = [dev[k] for k in NAMES[2:]]
    out_a = tail._FusedLayerTail.apply(c3, x3, *args, EPS, EPS, p, p, None, None, 5, 6, None, StepState(), idx)
    index = idx.unsqueeze(-1).expand(-1, -1, H)
    out_b = tail._FusedLayerTail.apply(c3.gather(1, index), x3.gather(1, index), *args, EPS, EPS, p, p, None, None, 5, 6,
                                       None, StepState())
    assert out_a.shape == (B, R, H) and torch.equal(out_a, out_b)
    leaves = [dev[k] for k in NAMES]
    ga = torch.autograd.grad((out_a * cot).sum(), leaves)
    gb = torch.autograd.grad((out_b * cot).sum(), leaves)
    for k, a, b in zip(NAMES, ga, gb):
        assert (a - b).abs().max() <= 1e-6 * b.abs().max() + 1e-9, k


@pytest.mark.parametrize("rows", [512, 8213], ids=["wide", "staged"])
def test_backward_without_saved_gelu_grad_equals_the_saved_one(rows):
    """acattn_tail_saved.gelu_grad = NULL makes the backward rebuild gelu'(dense_1(a)) from `a`.  The Python node always
    saves it at hidden 128, so these instantiations are reached through the C ABI only: d_ctx, d_x and d_h1..3 within 1e-5
    of the tensor's scale of the run that reads the saved values.  Every buffer the launches write starts as NaN, the
    transposed-weight workspace included."""
    lib = _lib.load()
    t, g = _inputs(rows, H, I, seed=rows)
    dev = {k: v.to(DEV).contiguous() for k, v in t.items()}
    d_out = torch.randn(rows, H, generator=g).to(DEV)
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV, dtype=torch.float32)
    p = tail._tail_problem(*(dev[k] for k in NAMES), EPS, EPS, 0.5, 0.5, None, None, 1234, 99, None)
    h1, a, h3, out = (nan(rows, H) for _ in range(4))
    st1, st2, act, dgelu = nan(rows, 2), nan(rows, 2), nan(rows, I), nan(rows, I)
    sv = _lib.TailSaved()
    sv.h1, sv.st1, sv.a, sv.act, sv.h3, sv.st2, sv.out = (_ptr(x) for x in (h1, st1, a, act, h3, st2, out))
    sv.gelu_grad = _ptr(dgelu)
    _lib.check(lib.acattn_layer_tail_fwd(C.byref(p), C.byref(sv), _stream()), "layer_tail_fwd")
    assert torch.isfinite(dgelu).all() and torch.isfinite(out).all()
    assert lib.acattn_layer_tail_bwd_workspace_bytes(H, I) == 131072
    runs = []
    for saved in (True, False):
        sv.gelu_grad = _ptr(dgelu) if saved else None
        bufs = dict(d_ctx=nan(rows, H), d_x=nan(rows, H), d_h1=nan(rows, H), d_h2=nan(rows, I), d_h3=nan(rows, H))
        part = nan(int(lib.acattn_layer_tail_bwd_partial_rows_for(rows, H)), 4 * H)
        ws = nan(131072 // 4)
        io = _lib.TailBwdIO()
        io.d_out, io.dgb_part, io.workspace = _ptr(d_out), _ptr(part), _ptr(ws)
        io.d_ctx, io.d_x, io.d_h1, io.d_h2, io.d_h3 = (_ptr(bufs[k]) for k in ("d_ctx", "d_x", "d_h1", "d_h2", "d_h3"))
        _lib.check(lib.acattn_layer_tail_bwd(C.byref(p), C.byref(sv), C.byref(io), _stream()), "layer_tail_bwd")
        assert torch.isfinite(ws).all() and torch.isfinite(part).all()
        runs.append(bufs)
    for k in ("d_ctx", "d_x", "d_h1", "d_h2", "d_h3"):
        err, scale = (runs[1][k] - runs[0][k]).abs().max().item(), runs[0][k].abs().max().item()
        print(f"rows {rows}: {k} rebuilt - saved {err:.3e} of {scale:.3e}")
        assert err <= 1e-5 * scale, (k, err, scale)
