"""The hidden-64 layer tails on split bf16 products (csrc/acattn_tail.hip, tail_split_*) against the
exact-fp32 kernels they replace: both are measured against the same chain in fp64 on the CPU, and the split kernels may
miss by at most twice what the fp32 kernels miss by, plus 2e-7 of the tensor's magnitude, in the output and every
gradient (the yardstick of test_hip_linear_split.py).  acattn_linear_products(0) (or ACATTN_LINEAR_PRODUCTS=fp32) brings
the fp32 tails back together with the fp32 projections.

The size queries are CPU-only; everything else needs the GPU (-m gpu)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ac_tsr_amd import _lib, tail
from ac_tsr_amd.state import StepState

DEV = "cuda"
NAMES = ("c", "x", "wd", "bd", "g1", "b1", "w1", "bb1", "w2", "bb2", "g2", "b2")
EPS = 1e-12


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _plane_bytes(I):
    return (2 * 64 * 64 + 4 * I * 64) * 3 * 2  # six matrices, three bf16 planes each


def test_split_plane_size_query_needs_no_gpu(lib):
    assert lib.acattn_layer_tail_split_bytes(64, 256, 25600) == _plane_bytes(256)
    assert lib.acattn_layer_tail_split_bytes(64, 128, 100) == _plane_bytes(128)
    assert lib.acattn_layer_tail_split_bytes(64, 256, 102400) == 0  # the staged form stays on fp32
    assert lib.acattn_layer_tail_split_bytes(128, 512, 512) == 0
    assert lib.acattn_layer_tail_split_bytes(64, 100, 512) == 0
    old = lib.acattn_linear_products(0)
    try:
        assert lib.acattn_layer_tail_split_bytes(64, 256, 25600) == 0
    finally:
        lib.acattn_linear_products(old)


def _inputs(rows, I, seed, scale=0.3):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    t = dict(c=r(rows, 64), x=r(rows, 64), wd=scale * r(64, 64), bd=0.1 * r(64), g1=1 + 0.3 * r(64), b1=0.3 * r(64),
             w1=scale * r(I, 64), bb1=0.1 * r(I), w2=scale * r(64, I), bb2=0.1 * r(64), g2=1 + 0.3 * r(64), b2=0.3 * r(64))
    return t, g


def _reference(t, pick, keep1, keep2, p, cot):
    """output and every gradient of the chain in fp64; with `pick` ([B, R]) on those positions of c, x viewed [B, L, 64]"""
    d = {k: v.double().requires_grad_(True) for k, v in t.items()}
    c, x = d["c"], d["x"]
    if pick is not None:
        B = pick.shape[0]
        index = pick.unsqueeze(-1).expand(-1, -1, 64)
        c, x = c.view(B, -1, 64).gather(1, index).reshape(-1, 64), x.view(B, -1, 64).gather(1, index).reshape(-1, 64)
    drop = lambda z, k: z if k is None else z * (k.double() / (1 - p))
    a = F.layer_norm(drop(F.linear(c, d["wd"], d["bd"]), keep1) + x, (64,), d["g1"], d["b1"], EPS)
    h3 = F.linear(F.gelu(F.linear(a, d["w1"], d["bb1"])), d["w2"], d["bb2"])
    out = F.layer_norm(drop(h3, keep2) + a, (64,), d["g2"], d["b2"], EPS)
    grads = torch.autograd.grad((out * cot.double()).sum(), [d[k] for k in NAMES])
    return out.detach(), dict(zip(NAMES, grads))


def _run(lib, mode, t, pick, keep1, keep2, p, cot, state=None):
    old = lib.acattn_linear_products(mode)
    try:
        dev = {k: v.to(DEV).requires_grad_(True) for k, v in t.items()}
        to = lambda k: None if k is None else k.to(DEV)
        c, x = dev["c"], dev["x"]
        extra = ()
        if pick is not None:
            B = pick.shape[0]
            c, x, extra = c.view(B, -1, 64), x.view(B, -1, 64), (pick.to(DEV),)
        out = tail._FusedLayerTail.apply(c, x, *(dev[k] for k in NAMES[2:]), EPS, EPS, p, p, to(keep1), to(keep2), 0, 0,
                                         None, state or StepState(), *extra)
        out = out.reshape(-1, 64)
        grads = torch.autograd.grad((out * cot.to(DEV)).sum(), [dev[k] for k in NAMES])
        torch.cuda.synchronize()
        return out.detach().cpu(), {k: v.cpu() for k, v in zip(NAMES, grads)}
    finally:
        lib.acattn_linear_products(old)


def _check(ref, ref_grad, r32, r6):
    """Output and input gradients: at most twice the fp32 kernels' error + 2e-7 of the magnitude.  The parameter gradients
    are sums over every row, and the bf16 MFMA's sums carry a negative mean error (acattn_tail.hip) that
    adds up there: measured up to 4.1 times the fp32 kernels' error at 25,600 rows, so those are held to 4.5 times."""
    (out32, grad32), (out6, grad6) = r32, r6
    for got32, got6, want, name in [(out32, out6, ref, "out")] + [(grad32[k], grad6[k], ref_grad[k], k) for k in NAMES]:
        e32 = (got32.double() - want).abs().max().item()
        e6 = (got6.double() - want).abs().max().item()
        factor = 2 if name in ("out", "c", "x") else 4.5
        assert e6 <= factor * e32 + 2e-7 * max(1.0, want.abs().max().item()), (name, e6, e32)
    assert not torch.equal(out32, out6)  # the switch really changes the arithmetic


# the bench shape (25,600 rows: two row blocks per wave), a ragged count with two row blocks per wave, one row block
# per wave (4,097 - 16,383 rows), the last layer's 512 positions and a ragged 37 (four waves per row block); inner 128
@pytest.mark.gpu
@pytest.mark.parametrize("rows,I", [(25600, 256), (16384 + 21, 256), (8192 + 21, 256), (512, 256), (37, 256), (100, 128),
                                    (8192 + 21, 128)])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_split_tail_is_as_accurate_as_fp32(lib, rows, I, p):
    t, g = _inputs(rows, I, seed=rows + I)
    keep1 = torch.empty(rows, 64).bernoulli_(1 - p, generator=g) if p > 0 else None
    keep2 = torch.empty(rows, 64).bernoulli_(1 - p, generator=g) if p > 0 else None
    cot = torch.randn(rows, 64, generator=g)
    ref, ref_grad = _reference(t, None, keep1, keep2, p, cot)
    _check(ref, ref_grad, _run(lib, 0, t, None, keep1, keep2, p, cot), _run(lib, 1, t, None, keep1, keep2, p, cot))


# row selection: the last layer's one position of 512 sequences of 50, and three positions of 37
@pytest.mark.gpu
@pytest.mark.parametrize("B,L,R", [(512, 50, 1), (37, 50, 3)])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_split_tail_with_row_selection_is_as_accurate_as_fp32(lib, B, L, R, p):
    t, g = _inputs(B * L, 256, seed=B + R)
    pick = torch.randint(0, L, (B, R), generator=g)
    keep1 = torch.empty(B * R, 64).bernoulli_(1 - p, generator=g) if p > 0 else None
    keep2 = torch.empty(B * R, 64).bernoulli_(1 - p, generator=g) if p > 0 else None
    cot = torch.randn(B * R, 64, generator=g)
    ref, ref_grad = _reference(t, pick, keep1, keep2, p, cot)
    _check(ref, ref_grad, _run(lib, 0, t, pick, keep1, keep2, p, cot), _run(lib, 1, t, pick, keep1, keep2, p, cot))


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [25600, 512])
def test_split_tail_reruns_are_bit_identical(lib, rows):
    t, g = _inputs(rows, 256, seed=3)
    keep = torch.empty(rows, 64).bernoulli_(0.5, generator=g)
    cot = torch.randn(rows, 64, generator=g)
    a_out, a_grad = _run(lib, 1, t, None, keep, keep, 0.5, cot)
    b_out, b_grad = _run(lib, 1, t, None, keep, keep, 0.5, cot)
    assert torch.equal(a_out, b_out)
    for k in NAMES:
        assert torch.equal(a_grad[k], b_grad[k]), k


def _kperm(s, g, j):
    return 32 * s + 16 * (j >> 2) + 4 * g + (j & 3)


def _unpack(planes, M, K):
    """the fp64 sum of the three planes of an A-form matrix [M][K] laid out [mt][s][plane][lane][j]"""
    KS = K // 32
    v = planes.reshape(M // 16, KS, 3, 64, 8).double().sum(2)  # [mt, s, lane, j]
    mt, s, lane, j = np.meshgrid(np.arange(M // 16), np.arange(KS), np.arange(64), np.arange(8), indexing="ij")
    m, k = 16 * mt + (lane & 15), _kperm(s, lane >> 4, j)
    out = torch.zeros(M, K, dtype=torch.float64)
    out[torch.from_numpy(m.ravel()), torch.from_numpy(k.ravel())] = v.reshape(-1)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("I", [256, 128])
def test_split_planes_sum_back_to_the_weights(lib, I):
    t, _ = _inputs(64, I, seed=5)
    dev = {k: v.to(DEV) for k, v in t.items()}
    # weights far from the usual range, values that round up in bf16, zeros (residuals stay normal numbers: the planes
    # are exact for every weight above 2^-100 in magnitude)
    dev["w1"][0, :8] = torch.tensor([1e-20, -3e-25, 1e30, 1.0 + 2 ** -9, -(1.0 + 2 ** -8 + 2 ** -20), 0.0, -0.0, 7.0], device=DEV)
    p = tail._tail_problem(dev["c"], dev["x"], *(dev[k] for k in NAMES[2:]), EPS, EPS, 0.0, 0.0, None, None, 0, 0, None)
    nbytes = int(lib.acattn_layer_tail_split_bytes(64, I, 64))
    assert nbytes == _plane_bytes(I)
    planes = torch.empty(nbytes // 2, device=DEV, dtype=torch.bfloat16)
    _lib.check(lib.acattn_layer_tail_split_weights(C.byref(p), C.c_void_p(planes.data_ptr()),
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)), "split_weights")
    torch.cuda.synchronize()
    planes = planes.cpu().float()
    wd, w1, w2 = (dev[k].cpu().double() for k in ("wd", "w1", "w2"))
    SQ, RECT = 64 * 64 * 3, I * 64 * 3
    offs, mats = 0, []
    for size, M, K, want in ((SQ, 64, 64, wd), (RECT, I, 64, w1), (RECT, 64, I, w2),
                             (SQ, 64, 64, wd.t()), (RECT, 64, I, w1.t()), (RECT, I, 64, w2.t())):
        got = _unpack(planes[offs:offs + size], M, K)
        assert torch.equal(got, want.contiguous()), (M, K)
        offs += size
    assert offs * 2 == nbytes


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [25600, 512])
def test_weights_changed_in_place_between_steps_change_the_output(lib, rows):
    """Adam updates the weights in place: a second forward of one StepState after an in-place update must compute with
    the NEW weights, i.e. no weight planes may be reused from the first one (a guard for any future caching)."""
    t, g = _inputs(rows, 256, seed=9)
    cot = torch.randn(rows, 64, generator=g)
    t2 = dict(t)
    for k in ("wd", "w1", "w2"):
        t2[k] = t[k] * 1.25 + 0.01
    want = _run(lib, 1, t2, None, None, None, 0.0, cot)[0]  # fresh tensors, fresh state
    state = StepState()
    dev = {k: v.to(DEV).requires_grad_(True) for k, v in t.items()}
    run = lambda: tail._FusedLayerTail.apply(*(dev[k] for k in NAMES), EPS, EPS, 0.0, 0.0, None, None, 0, 0, None, state)
    first = run().detach().cpu()
    with torch.no_grad():
        for k in ("wd", "w1", "w2"):
            dev[k].mul_(1.25).add_(0.01)
    second = run().detach().cpu()
    assert (second - first).abs().max() > 0.01
    assert torch.equal(second, want)
