"""The hidden-64 projections on split bf16 products (csrc/acattn_proj.hip, proj_split_*) against the
exact-fp32 kernels they replace: both are measured against the same six nn.Linear in fp64 on the CPU, and the split
kernels may miss by at most twice what the fp32 kernels miss by, plus 2e-7 of the tensor's magnitude, in every output
and every gradient.  acattn_linear_products(0) (or ACATTN_LINEAR_PRODUCTS=fp32) brings the fp32 kernels back.

The mode query is CPU-only; everything else needs the GPU (-m gpu)."""
import pytest
import torch
import torch.nn.functional as F

from ac_tsr_amd import _lib, linear
from ac_tsr_amd.state import StepState

DEV = "cuda"
W = ("wq", "bq", "wk", "bk", "wv", "bv", "waq", "baq", "wak", "bak", "wg", "bg")
OUT = ("mq", "mk", "mv", "qa", "ka", "gate")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_linear_products_mode_query_needs_no_gpu(lib):
    old = lib.acattn_linear_products(-1)
    assert old in (0, 1)
    assert lib.acattn_linear_products(0) == old
    assert lib.acattn_linear_products(5) == 0  # out of range: query only
    assert lib.acattn_linear_products(old) == 0


def _inputs(rows, G, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    t = dict(x=r(rows, 64))
    for n in ("q", "k", "v", "aq", "ak"):
        t["w" + n], t["b" + n] = 0.2 * r(64, 64), 0.1 * r(64)
    if G:
        t["wg"], t["bg"] = 0.2 * r(G, 64), 0.1 * r(G)
    cot = {k: r(rows, G if k == "gate" else 64) for k in OUT if (k != "gate" or G)}
    return t, cot


def _reference(t, cot, G):
    d = {k: v.double().requires_grad_(True) for k, v in t.items()}
    mq, mk, mv = F.linear(d["x"], d["wq"], d["bq"]), F.linear(d["x"], d["wk"], d["bk"]), F.linear(d["x"], d["wv"], d["bv"])
    out = dict(mq=mq, mk=mk, mv=mv, qa=F.linear(mq, d["waq"], d["baq"]), ka=F.linear(mk, d["wak"], d["bak"]))
    if G:
        out["gate"] = F.linear(mq, d["wg"], d["bg"])
    loss = sum((out[k] * cot[k].double()).sum() for k in cot)
    names = ["x"] + [n for n in W if n in t]
    grads = dict(zip(names, torch.autograd.grad(loss, [d[n] for n in names])))
    return {k: v.detach() for k, v in out.items()}, grads


def _run(lib, mode, t, cot):
    """outputs and every gradient (no pass restriction) of the fused projections in product mode `mode`"""
    old = lib.acattn_linear_products(mode)
    try:
        dev = {k: v.to(DEV).requires_grad_(True) for k, v in t.items()}
        outs = linear._FusedProjections.apply(dev["x"], *[dev.get(n) for n in W], True, StepState())
        got = dict(zip(OUT, outs))
        loss = sum((got[k] * cot[k].to(DEV)).sum() for k in cot)
        names = ["x"] + [n for n in W if n in t]
        grads = dict(zip(names, torch.autograd.grad(loss, [dev[n] for n in names])))
        torch.cuda.synchronize()
        return {k: got[k].detach().cpu() for k in cot}, {k: v.cpu() for k, v in grads.items()}
    finally:
        lib.acattn_linear_products(old)


# the bench shape (B = 512, L = 50: two row blocks per wave), ragged row counts that end inside a wave's second block and
# inside a workgroup, a gate that ends inside its first tile, a 64-wide gate, no gate
@pytest.mark.gpu
@pytest.mark.parametrize("rows,G", [(25600, 50), (16384 + 21, 50), (1000 + 17, 50), (37, 50), (48, 37), (64, 64), (100, 0)])
def test_split_projections_are_as_accurate_as_fp32(lib, rows, G):
    t, cot = _inputs(rows, G, seed=rows + G)
    ref_out, ref_grad = _reference(t, cot, G)
    out32, grad32 = _run(lib, 0, t, cot)
    out6, grad6 = _run(lib, 1, t, cot)
    for got32, got6, ref in ((out32, out6, ref_out), (grad32, grad6, ref_grad)):
        for k, want in ref.items():
            e32 = (got32[k].double() - want).abs().max().item()
            e6 = (got6[k].double() - want).abs().max().item()
            assert e6 <= 2 * e32 + 2e-7 * max(1.0, want.abs().max().item()), (k, e6, e32)
    # the switch really changes the arithmetic (the split results are not the fp32 kernels' bit for bit)
    assert any(not torch.equal(out32[k], out6[k]) for k in out32)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_projections_are_deterministic_in_both_modes(lib, mode):
    t, cot = _inputs(25600, 50, seed=7)
    a_out, a_grad = _run(lib, mode, t, cot)
    b_out, b_grad = _run(lib, mode, t, cot)
    for k in a_out:
        assert torch.equal(a_out[k], b_out[k]), k
    for k in a_grad:
        assert torch.equal(a_grad[k], b_grad[k]), k
