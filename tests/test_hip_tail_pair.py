"""GPU suite: both tails of a layer in one forward launch (acattn_layer_tail_fwd_pair, tail.layer_tail_pair).

The pair launch is the four-wave split forward kernel over two problems: everything it writes -- outputs and every saved
tensor of both branches -- must be bit for bit what two acattn_layer_tail_fwd launches write, and the two autograd nodes
behind tail.layer_tail_pair, walked separately with one cotangent each, must give exactly the gradients of two unpaired
nodes.  Rows 1, 15, 16, 17 (around one 16-row block) and 512 (the benchmark's), picked out of [B, L, 64]; explicit keep
masks and counter dropout; different seeds per branch."""
import ctypes as C

import pytest
import torch

from ac_tsr_amd import _lib, layers, planes, tail
from ac_tsr_amd.state import StepState

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-12
# rows -> (B, R picked positions per sequence, L)
SHAPES = {1: (1, 1, 7), 15: (3, 5, 9), 16: (4, 4, 50), 17: (1, 17, 20), 512: (4, 128, 128)}
SAVED = ("h1", "st1", "a", "act", "h3", "st2", "out")


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _weights(I, gen):
    r = lambda *s: torch.randn(*s, generator=gen)
    return [t.to(DEV) for t in (0.3 * r(64, 64), 0.1 * r(64), 1 + 0.3 * r(64), 0.3 * r(64), 0.3 * r(I, 64), 0.1 * r(I),
                                0.3 * r(64, I), 0.1 * r(64), 1 + 0.3 * r(64), 0.3 * r(64))]


def _pick(B, R, L, gen):
    return torch.stack([torch.randperm(L, generator=gen)[:R] for _ in range(B)]).to(DEV)


def _split_planes(lib, params, I, rows):
    nbytes = int(lib.acattn_layer_tail_split_bytes(64, I, rows))
    assert nbytes > 0
    buf = torch.empty(nbytes // 4, device=DEV)
    p = _lib.TailProblem()
    p.H, p.I, p.rows = 64, I, rows
    p.wd, p.w1, p.w2 = params[0].data_ptr(), params[4].data_ptr(), params[6].data_ptr()
    _lib.check(lib.acattn_layer_tail_split_weights(C.byref(p), _ptr(buf), None), "layer_tail_split_weights")
    return buf


def _saved(rows, I, shape):
    nan = float("nan")
    t = dict(h1=torch.full((*shape, 64), nan, device=DEV), st1=torch.full((rows, 2), nan, device=DEV),
             a=torch.full((*shape, 64), nan, device=DEV), act=torch.full((rows, I), nan, device=DEV),
             h3=torch.full((*shape, 64), nan, device=DEV), st2=torch.full((rows, 2), nan, device=DEV),
             out=torch.full((*shape, 64), nan, device=DEV))
    sv = _lib.TailSaved()
    for k in SAVED:
        setattr(sv, k, t[k].data_ptr())
    return sv, t


@pytest.mark.parametrize("explicit", [False, True])
@pytest.mark.parametrize("I", [256, 128])
@pytest.mark.parametrize("rows", sorted(SHAPES))
def test_pair_launch_writes_what_two_launches_write(rows, I, explicit):
    lib = _lib.load()
    B, R, L = SHAPES[rows]
    gen = torch.Generator().manual_seed(100 * rows + I)
    params = _weights(I, gen)
    buf = _split_planes(lib, params, I, rows)
    x = torch.randn(B, L, 64, generator=gen).to(DEV)
    pick = _pick(B, R, L, gen)
    seed_t = torch.tensor([5], dtype=torch.int64, device=DEV)
    probs, keep_alive = [], []
    for branch in range(2):  # its own ctx, keep masks / seeds
        c = torch.randn(B, L, 64, generator=gen).to(DEV)
        k1 = k2 = None
        if explicit:
            k1, k2 = ((torch.rand(B, R, 64, generator=gen) < 0.5).to(torch.uint8).to(DEV) for _ in range(2))
        p = tail._tail_problem(c, x, *params, EPS, EPS, 0.5, 0.5, k1, k2, 0 if explicit else 1000 + branch,
                               0 if explicit else 2000 + branch, None if explicit else seed_t, pick)
        p.split_planes = buf.data_ptr()
        probs.append(p)
        keep_alive += [c, k1, k2]
    single, paired = [], []
    for p in probs:
        sv, t = _saved(rows, I, (B, R))
        _lib.check(lib.acattn_layer_tail_fwd(C.byref(p), C.byref(sv), None), "layer_tail_fwd")
        single.append(t)
    svs = []
    for p in probs:
        sv, t = _saved(rows, I, (B, R))
        svs.append(sv)
        paired.append(t)
    rc = lib.acattn_layer_tail_fwd_pair(C.byref(probs[0]), C.byref(svs[0]), C.byref(probs[1]), C.byref(svs[1]), None)
    assert rc == 0, (rc, lib.acattn_last_error())
    torch.cuda.synchronize()
    for branch in range(2):
        for k in SAVED:
            assert not torch.isnan(paired[branch][k]).any(), (branch, k)
            assert torch.equal(_bits(paired[branch][k]), _bits(single[branch][k])), (branch, k)
    assert not torch.equal(paired[0]["out"], paired[1]["out"])  # (two problems, not one twice)


def test_where_the_pair_form_does_not_apply():
    """Row counts of the per-wave forms, different row counts, no planes: -100 and nothing written."""
    lib = _lib.load()
    gen = torch.Generator().manual_seed(3)
    params = _weights(256, gen)
    buf = _split_planes(lib, params, 256, 16)

    def problem(rows, with_planes=True):
        c, x = torch.randn(rows, 64, generator=gen).to(DEV), torch.randn(rows, 64, generator=gen).to(DEV)
        p = tail._tail_problem(c, x, *params, EPS, EPS, 0.0, 0.0, None, None, 0, 0, None)
        p.split_planes = buf.data_ptr() if with_planes else None
        sv, t = _saved(rows, 256, (rows,))
        return p, sv, t, (c, x)

    for (ra, rb, planes_b) in ((8192, 8192, True), (16, 32, True), (16, 16, False)):
        pa, sa, ta, ka = problem(ra)
        pb, sb, tb, kb = problem(rb, planes_b)
        assert lib.acattn_layer_tail_fwd_pair(C.byref(pa), C.byref(sa), C.byref(pb), C.byref(sb), None) == -100
        torch.cuda.synchronize()
        assert torch.isnan(ta["out"]).all() and torch.isnan(tb["out"]).all()


def _modules(I):
    torch.manual_seed(0)
    att = layers.AttackRMultiHeadAttention(2, 64, 0.5, 0.5, EPS, True, True).to(DEV).train()
    ffn = layers.FeedForward(64, I, 0.5, 'gelu', EPS).to(DEV).train()
    state = StepState()
    state.attach(att)
    state.attach(ffn)
    return att, ffn


@pytest.mark.parametrize("explicit", [False, True])
@pytest.mark.parametrize("rows", sorted(SHAPES))
def test_paired_nodes_give_the_gradients_of_unpaired_nodes(rows, explicit, monkeypatch):
    lib = _lib.load()
    I = 256
    B, R, L = SHAPES[rows]
    att, ffn = _modules(I)
    params = [att.dense.weight, att.dense.bias, att.LayerNorm.weight, att.LayerNorm.bias, ffn.dense_1.weight, ffn.dense_1.bias,
              ffn.dense_2.weight, ffn.dense_2.bias, ffn.LayerNorm.weight, ffn.LayerNorm.bias]
    holder = planes.LayerPlanes(tail=_split_planes(lib, [p.detach() for p in params], I, rows))
    gen = torch.Generator().manual_seed(rows)
    base = [torch.randn(B, L, 64, generator=gen).to(DEV) for _ in range(3)]
    pick = _pick(B, R, L, gen)
    cots = [torch.randn(B, R, 64, generator=gen).to(DEV) for _ in range(2)]
    keeps = [(None, None), (None, None)]
    if explicit:
        keeps = [tuple((torch.rand(B, R, 64, generator=gen) < 0.5).to(DEV) for _ in range(2)) for _ in range(2)]
    launched = []
    real = tail._pair_forward
    monkeypatch.setattr(tail, "_pair_forward", lambda *a, **k: launched.append(real(*a, **k)) or launched[-1])

    def run(paired):
        monkeypatch.setattr(tail, "PAIRED_FORWARD", paired)
        torch.manual_seed(11)  # the nodes' dropout seeds come from torch's CPU generator
        ca, cb, x = (t.clone().requires_grad_(True) for t in base)
        outs = tail.layer_tail_pair(ca, cb, x, att, ffn, keeps[0], keeps[1], pick=pick, planes=holder)
        saved = [[t.clone() for t in o.grad_fn.saved_tensors] for o in outs]
        grads = [torch.autograd.grad(outs[0], [ca, x] + params, cots[0], retain_graph=True),
                 torch.autograd.grad(outs[1], [cb, x] + params, cots[1])]
        torch.cuda.synchronize()
        return [o.detach() for o in outs], saved, grads

    out_p, saved_p, grads_p = run(True)
    assert len(launched) == 1 and launched[0] is not None, "the pair launch did not run"
    out_u, saved_u, grads_u = run(False)
    assert len(launched) == 1
    for branch in range(2):
        assert torch.equal(_bits(out_p[branch]), _bits(out_u[branch])), branch
        assert len(saved_p[branch]) == len(saved_u[branch])
        for k, (a, b) in enumerate(zip(saved_p[branch], saved_u[branch])):
            assert a.shape == b.shape and a.dtype == b.dtype, (branch, k)
            if a.dtype == torch.float32:
                assert torch.equal(_bits(a), _bits(b)), (branch, k)
            else:
                assert torch.equal(a, b), (branch, k)
        for k, (a, b) in enumerate(zip(grads_p[branch], grads_u[branch])):
            assert torch.isfinite(a).all() and torch.equal(_bits(a), _bits(b)), (branch, k, (a - b).abs().max().item())
    assert not torch.equal(out_p[0], out_p[1])
