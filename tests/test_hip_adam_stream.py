"""GPU suite (-m gpu): the persistent Adam launch (acattn_adam_step_cached, csrc/acattn_adam.hip: grid-stride stream with
the next trip's loads in flight, bias corrections from the per-optimizer cache) against the one-workgroup-per-chunk launch
it replaces (acattn_adam_step) -- equality, not a tolerance: the per-element arithmetic is the same code and the cached
corrections come from the same evaluation as the computed ones -- and against torch.optim.Adam(fused=True,
capturable=True) within the bounds of tests/test_hip_adam.py.  The grid forced to 3 workgroups makes every workgroup take
many trips and cross tensor boundaries mid-walk."""
import functools

import pytest
import torch

from ac_tsr_amd import _lib, optim
from ac_tsr_amd.optim import Adam

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (4099,): whole trips + a ragged tail; (1,), (3, 7): tails only; (16384, 5), (2000, 64): many trips; "view": 300 x 64
# starting one element into its storage, so that the parameter's pointer is not 16-byte aligned (checked scalar path)
SHAPES = [(4099,), (1,), (3, 7), (50, 64), (16384, 5), "view", (2000, 64)]
STEPS = 6


def _shape(s):
    return (300, 64) if s == "view" else s


@functools.lru_cache(maxsize=None)
def _data():
    g = torch.Generator().manual_seed(5)
    init = [torch.randn(*_shape(s), generator=g) * 0.1 for s in SHAPES]
    grads = [[torch.randn(*_shape(s), generator=g) * (0.01 if i % 2 else 1.0) for s in SHAPES] for i in range(STEPS)]
    return init, grads


def _params(init):
    ps = []
    for s, t in zip(SHAPES, init):
        if s == "view":
            store = torch.zeros(t.numel() + 1, device=DEV)
            view = store[1:].view(t.shape)
            view.copy_(t)
            assert view.data_ptr() % 16 == 4 and view.is_contiguous()
            ps.append(torch.nn.Parameter(view))
        else:
            ps.append(torch.nn.Parameter(t.clone().to(DEV)))
    return ps


def _run(cls, weight_decay, stream_kernel=True, grid=0):
    """STEPS steps over SHAPES; returns [(param, exp_avg, exp_avg_sq, step)] as CPU tensors."""
    init, grads = _data()
    lib = _lib.load()
    old_switch, old_grid = optim.STREAM_KERNEL, lib.acattn_select_adam_grid(grid)
    optim.STREAM_KERNEL = stream_kernel
    try:
        ps = _params(init)
        opt = cls(ps, lr=1e-3, weight_decay=weight_decay, capturable=True, fused=True)
        for step_grads in grads:
            for p, gr in zip(ps, step_grads):
                p.grad = gr.to(DEV).clone()
            opt.step()
        torch.cuda.synchronize()
        return [tuple(x.detach().cpu().clone() for x in (p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], opt.state[p]["step"]))
                for p in ps]
    finally:
        optim.STREAM_KERNEL = old_switch
        lib.acattn_select_adam_grid(old_grid)


@functools.lru_cache(maxsize=None)
def _chunk_kernel(weight_decay):
    return _run(Adam, weight_decay, stream_kernel=False)


@functools.lru_cache(maxsize=None)
def _torch_fused(weight_decay):
    return _run(torch.optim.Adam, weight_decay)


def _close(got, ref, what):
    """The bounds of tests/test_hip_adam.py."""
    for name, a, b, floor in zip(("param", "exp_avg", "exp_avg_sq", "step"), got, ref, (1e-9, 1e-12, 1e-12, 1e-12)):
        assert torch.isfinite(a).all()
        diff = (a - b).abs().max().item()
        assert diff <= 2e-7 * b.abs().max().item() + floor, (what, name, diff)


@pytest.mark.parametrize("grid", [0, 3])
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
def test_persistent_kernel_is_bitwise_the_chunk_kernel(weight_decay, grid):
    ref = _chunk_kernel(weight_decay)
    got = _run(Adam, weight_decay, stream_kernel=True, grid=grid)
    for s, a, b in zip(SHAPES, got, ref):
        for name, x, y in zip(("param", "exp_avg", "exp_avg_sq", "step"), a, b):
            assert torch.equal(x, y), (s, name, (x - y).abs().max().item())
    assert float(got[0][3]) == STEPS


@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
def test_persistent_kernel_equals_torch_fused_adam(weight_decay):
    ref = _torch_fused(weight_decay)
    got = _run(Adam, weight_decay, stream_kernel=True, grid=3)
    for s, a, b in zip(SHAPES, got, ref):
        _close(a, b, s)


def test_cache_never_serves_a_stale_correction():
    """Counters that diverge inside one launch (a parameter without a gradient on steps 2 and 4), a counter overwritten on
    the device after step 3, and a state_dict round trip into a fresh optimizer (fresh zero cache) after step 5."""
    g = torch.Generator().manual_seed(11)
    init = [torch.randn(70, 64, generator=g) * 0.1, torch.randn(1500, generator=g) * 0.1]
    grads = [[torch.randn(*t.shape, generator=g) for t in init] for _ in range(6)]

    def make(cls):
        ps = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
        return ps, cls(ps, lr=1e-3, capturable=True, fused=True)

    assert optim.STREAM_KERNEL
    (ps, opt), (rps, ropt) = make(Adam), make(torch.optim.Adam)
    for i in range(6):
        for params in (ps, rps):
            params[0].grad = grads[i][0].to(DEV).clone()
            params[1].grad = None if i in (1, 3) else grads[i][1].to(DEV).clone()
        opt.step()
        ropt.step()
        for k, (a, b) in enumerate(zip(ps, rps)):
            _close((a.detach(), opt.state[a]["exp_avg"], opt.state[a]["exp_avg_sq"], opt.state[a]["step"]),
                   (b.detach(), ropt.state[b]["exp_avg"], ropt.state[b]["exp_avg_sq"], ropt.state[b]["step"]), (i, k))
        if i == 2:
            opt.state[ps[0]]["step"].fill_(10.0)
            ropt.state[rps[0]]["step"].fill_(10.0)
        if i == 4:
            sd = opt.state_dict()
            opt = Adam(ps, lr=1e-3, capturable=True, fused=True)
            opt.load_state_dict(sd)
            assert "_acattn_corrections" not in opt.__dict__
    # param 0: 3 steps, counter set to 10, 3 more; param 1: 6 steps less the two it skipped
    assert float(opt.state[ps[0]]["step"]) == 13.0 and float(opt.state[ps[1]]["step"]) == 4.0
    assert float(ropt.state[rps[0]]["step"]) == 13.0 and float(ropt.state[rps[1]]["step"]) == 4.0
    assert not opt.__dict__["_acattn_corrections"].eq(0).all()


def test_more_tensors_than_one_launch_takes_share_the_cache():
    n = _lib.ADAM_MAX_TENSORS + 6
    g = torch.Generator().manual_seed(13)
    init = [torch.randn(64, generator=g) * 0.1 for _ in range(n)]
    grads = [[torch.randn(64, generator=g) for _ in range(n)] for _ in range(4)]

    def run(cls):
        ps = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
        opt = cls(ps, lr=1e-3, weight_decay=0.01, capturable=True, fused=True)
        for step_grads in grads:
            for p, gr in zip(ps, step_grads):
                p.grad = gr.to(DEV).clone()
            opt.step()
        return ps, opt

    assert optim.STREAM_KERNEL
    (ps, opt), (rps, ropt) = run(Adam), run(torch.optim.Adam)
    for k, (a, b) in enumerate(zip(ps, rps)):
        _close((a.detach(), opt.state[a]["exp_avg"], opt.state[a]["exp_avg_sq"], opt.state[a]["step"]),
               (b.detach(), ropt.state[b]["exp_avg"], ropt.state[b]["exp_avg_sq"], ropt.state[b]["step"]), k)
        assert float(opt.state[a]["step"]) == 4.0


def test_captured_step_replays_with_advancing_cache_and_counters():
    """One torch step (creates the state), one eager library step, then one captured step replayed 4 times: the 5 library
    steps equal 5 eager steps of the chunk kernel bit for bit (the gradients stay what they are, as under the trainer's
    graph)."""
    g = torch.Generator().manual_seed(17)
    init = [torch.randn(3000, 64, generator=g) * 0.1, torch.randn(777, generator=g) * 0.1]
    grads = [torch.randn(*t.shape, generator=g) for t in init]

    def start(stream_kernel):
        ps = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
        opt = Adam(ps, lr=1e-3, weight_decay=0.01, capturable=True, fused=True)
        for p, gr in zip(ps, grads):
            p.grad = gr.to(DEV).clone()
        opt.step()  # torch's implementation: creates the state
        return ps, opt

    old = optim.STREAM_KERNEL
    try:
        optim.STREAM_KERNEL = False
        rps, ropt = start(False)
        for _ in range(5):
            ropt.step()
        optim.STREAM_KERNEL = True
        ps, opt = start(True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            opt.step()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            opt.step()
        for _ in range(4):
            graph.replay()
        torch.cuda.synchronize()
    finally:
        optim.STREAM_KERNEL = old
    for a, b in zip(ps, rps):
        assert torch.equal(a, b)
        for key in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(opt.state[a][key], ropt.state[b][key]), key
        assert float(opt.state[a]["step"]) == 6.0
    # a cache slot: double beta1, beta2; float step, bc1, bc2s, pad -- the entries now hold the corrections of step 7
    slots = opt.__dict__["_acattn_corrections"].view(torch.float32).view(-1, 8).cpu()
    assert slots[0, 4].item() == 7.0 and slots[1, 4].item() == 7.0 and slots[2, 4].item() == 0.0
    assert abs(slots[0, 5].item() - (1 - 0.9 ** 7)) < 1e-6 and abs(slots[0, 6].item() - (1 - 0.999 ** 7) ** 0.5) < 1e-6
