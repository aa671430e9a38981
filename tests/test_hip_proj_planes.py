"""The split weight planes made once per encoder forward (acattn_split_weights_many, ac_tsr_amd/planes.py) and the
projection kernels that read them (proj_planes_fwd_kernel / proj_planes_bwd_kernel, csrc/acattn_proj.hip).

The planes kernels keep the MFMA order of the kernels that split the weights inside every workgroup, so through the C ABI
every tensor they write must equal that form's BITWISE; against six fp64 nn.Linear they stay within the bound of
tests/test_hip_linear_split.py (twice the exact-fp32 kernels' error + 2e-7 of the magnitude).  Every output buffer starts
as NaN, so an element a kernel failed to write shows."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import ac_tsr_amd as A
from ac_tsr_amd import _lib, attn_launch, planes

pytestmark = pytest.mark.gpu
DEV = "cuda"
MATS = ("wq", "wk", "wv", "waq", "wak")
FWD_ORDER = ("wq", "waq", "wg", "wk", "wak", "wv")
BWD_ORDER = ("waq", "wg", "wq", "wak", "wk", "wv")
ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
nans = lambda *shape: torch.full(shape, float("nan"), device=DEV)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _weights(G, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    w = {}
    for n in ("q", "k", "v", "aq", "ak"):
        w["w" + n], w["b" + n] = 0.2 * r(64, 64), 0.1 * r(64)
    if G:
        w["wg"], w["bg"] = 0.2 * r(G, 64), 0.1 * r(G)
    w["w_order"], w["b_order"], w["w_dist"], w["b_dist"] = 0.3 * r(64), 0.1 * r(1), 0.3 * r(64), 0.1 * r(1)
    return {k: v.to(DEV) for k, v in w.items()}


def _proj_planes(lib, w, G):
    nbytes = int(lib.acattn_projections_split_bytes(64, G))
    assert nbytes == 2 * 6 * 4 * 2 * 3 * 64 * 16
    buf = torch.zeros(nbytes // 4, device=DEV)  # (zeros: the gate's slots stay unwritten without a gate)
    job = _lib.SplitLayer()
    job.wq, job.wk, job.wv, job.waq, job.wak = (ptr(w[n]) for n in MATS)
    if G:
        job.wg, job.G = ptr(w["wg"]), G
    job.proj_planes = ptr(buf)
    _lib.check(lib.acattn_split_weights_many(C.byref(job), 1, stream()), "split_weights_many")
    return buf


def _problem(rows, w, G, x, planes_buf):
    p = _lib.ProjProblem()
    p.rows, p.H, p.G, p.x = rows, 64, G, ptr(x)
    for n in ("q", "k", "v", "aq", "ak") + (("g",) if G else ()):
        setattr(p, "w" + n, ptr(w["w" + n]))
        setattr(p, "b" + n, ptr(w["b" + n]))
    p.split_planes = ptr(planes_buf)
    return p


def _forward(lib, rows, w, G, x, planes_buf, extras):
    p = _problem(rows, w, G, x, planes_buf)
    out = {k: nans(rows, 64) for k in ("mq", "mk", "mv", "qa", "ka")}
    if G:
        out["gate"] = nans(rows, G)
    o = _lib.ProjOut()
    for k, t in out.items():
        setattr(o, k, ptr(t))
    if extras:  # affine planes (one sequence of `rows` positions, two heads) and the gate as probabilities
        p.w_order, p.b_order, p.w_dist, p.b_dist = (ptr(w[k]) for k in ("w_order", "b_order", "w_dist", "b_dist"))
        p.n_heads, p.L = 2, rows
        out["affine"] = nans(1, 2, 4, 16 * ((rows + 15) // 16))
        o.affine, o.gate_prob = ptr(out["affine"]), 1
    _lib.check(lib.acattn_projections_fwd(C.byref(p), C.byref(o), stream()), "projections_fwd")
    if extras:
        out["affine"] = out["affine"][..., :rows]  # (the padding entries are the caller's)
    return out


# cotangents given / gradients wanted; with dx, dmq_total and dmk_total all wanted the launch picks MODE 1 (everything
# given) or MODE 2 (the attack transforms' alone), otherwise MODE 0
BWD_CASES = {
    "mode1": (("dmq", "dmk", "dmv", "dqa", "dka", "dgate"), ("dmq_total", "dmk_total", "dx")),
    "mode2": (("dqa", "dka"), ("dmq_total", "dmk_total", "dx")),
    "mode0_attack_only": (("dqa", "dka"), ("dmq_total", "dmk_total")),
    "mode0_no_dmv": (("dmq", "dmk", "dqa", "dka", "dgate"), ("dmq_total", "dmk_total", "dx")),
    "mode0_qkv": (("dmq", "dmk", "dmv"), ("dx",)),
}


def _backward(lib, rows, w, G, x, planes_buf, cot, case, dx_init):
    given, wanted = BWD_CASES[case]
    p = _problem(rows, w, G, x, planes_buf)
    io = _lib.ProjBwdIO()
    for k in given:
        if k != "dgate" or G:
            setattr(io, k, ptr(cot[k]))
    out = {k: nans(rows, 64) for k in wanted}
    for k, t in out.items():
        setattr(io, k, ptr(t))
    if dx_init is not None and "dx" in wanted:
        io.dx_init = ptr(dx_init)
    _lib.check(lib.acattn_projections_bwd(C.byref(p), C.byref(io), stream()), "projections_bwd")
    return out


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert not torch.isnan(a[k]).any(), (what, k, "an element was not written")
        assert torch.equal(a[k], b[k]), (what, k, (a[k] - b[k]).abs().max().item())


# ---- planes content --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [64, 50, 37, 0])
def test_projection_planes_hold_the_exact_split_of_every_weight(lib, G):
    w = _weights(G, seed=100 + G)
    buf = _proj_planes(lib, w, G)
    torch.cuda.synchronize()
    # [direction][matrix][tile][K-block][plane][lane][j] bf16; the three planes summed in fp32 (exact: 16 + 8 bits)
    frag = buf.view(torch.bfloat16).view(2, 6, 4, 2, 3, 64, 8).float()
    total = (frag[:, :, :, :, 0] + frag[:, :, :, :, 1]) + frag[:, :, :, :, 2]  # [2, 6, 4, 2, 64, 8]
    lane, j = torch.arange(64, device=DEV).view(1, 1, 64, 1), torch.arange(8, device=DEV).view(1, 1, 1, 8)
    nt, s = torch.arange(4, device=DEV).view(4, 1, 1, 1), torch.arange(2, device=DEV).view(1, 2, 1, 1)
    m = (16 * nt + (lane & 15)).expand(4, 2, 64, 8)
    k = (32 * s + 16 * (j >> 2) + 4 * (lane >> 4) + (j & 3)).expand(4, 2, 64, 8)
    for d, order in enumerate((FWD_ORDER, BWD_ORDER)):
        for mi, name in enumerate(order):
            if name == "wg" and not G:
                continue
            full = torch.zeros(64, 64, device=DEV)
            full[:w[name].shape[0]] = w[name]  # gate rows past G: zeros
            want = full[m, k] if d == 0 else full[k, m]  # forward A[m][k] = W[m][k], backward A[m][k] = W[k][m]
            assert torch.equal(total[d, mi], want), (d, name)
            if name == "wg" and G < 64:
                past = (m >= G) if d == 0 else (k >= G)
                assert (frag[d, mi].permute(0, 1, 3, 4, 2)[past] == 0).all(), (d, name)


@pytest.mark.parametrize("I", [256, 128])
def test_tail_planes_of_the_many_launch_are_those_of_the_single_launch(lib, I):
    g = torch.Generator().manual_seed(I)
    wd, w1, w2 = (torch.randn(*s, generator=g).to(DEV) for s in ((64, 64), (I, 64), (64, I)))
    nbytes = int(lib.acattn_layer_tail_split_bytes(64, I, 25600))
    assert nbytes > 0
    one, many = (torch.zeros(nbytes // 4, dtype=torch.int32, device=DEV) for _ in range(2))
    tp = _lib.TailProblem()
    tp.rows, tp.H, tp.I, tp.wd, tp.w1, tp.w2 = 25600, 64, I, ptr(wd), ptr(w1), ptr(w2)
    _lib.check(lib.acattn_layer_tail_split_weights(C.byref(tp), ptr(one), stream()), "layer_tail_split_weights")
    jobs = (_lib.SplitLayer * 2)()  # two layers in one launch, the second one's tail only
    jobs[1].wd, jobs[1].w1, jobs[1].w2, jobs[1].I, jobs[1].tail_planes = ptr(wd), ptr(w1), ptr(w2), I, ptr(many)
    w = _weights(50, seed=3)
    proj = torch.zeros(int(lib.acattn_projections_split_bytes(64, 50)) // 4, device=DEV)
    jobs[0].wq, jobs[0].wk, jobs[0].wv, jobs[0].waq, jobs[0].wak = (ptr(w[n]) for n in MATS)
    jobs[0].wg, jobs[0].G, jobs[0].proj_planes = ptr(w["wg"]), 50, ptr(proj)
    _lib.check(lib.acattn_split_weights_many(jobs, 2, stream()), "split_weights_many")
    assert torch.equal(one, many)
    assert torch.equal(proj, _proj_planes(lib, w, 50))


def test_size_query_follows_the_product_mode(lib):
    assert lib.acattn_projections_split_bytes(64, 65) == 0 and lib.acattn_projections_split_bytes(128, 50) == 0
    old = lib.acattn_linear_products(0)
    try:
        assert lib.acattn_projections_split_bytes(64, 50) == 0
    finally:
        lib.acattn_linear_products(old)
    assert lib.acattn_projections_split_bytes(64, 0) == lib.acattn_projections_split_bytes(64, 50) > 0


# ---- the kernels through the C ABI: planes form against the in-kernel-split form ------------------------------------------
# 1 .. 129: wave, row-block and (old) workgroup edges, a last partial block; 520: several workgroups; 16,405: two row blocks
# per wave (the regime of tests/test_hip_linear_split.py)
@pytest.mark.parametrize("rows", [1, 15, 16, 17, 33, 127, 128, 129, 520, 16405])
def test_planes_kernels_equal_the_in_kernel_split_bitwise(lib, rows):
    for G in (64, 50, 37, 0):
        w = _weights(G, seed=rows + G)
        buf = _proj_planes(lib, w, G)
        g = torch.Generator().manual_seed(rows * 7 + G)
        x = torch.randn(rows, 64, generator=g).to(DEV)
        cot = {k: torch.randn(rows, 64, generator=g).to(DEV) for k in ("dmq", "dmk", "dmv", "dqa", "dka")}
        cot["dgate"] = torch.randn(rows, max(G, 1), generator=g).to(DEV)
        dx_init = torch.randn(rows, 64, generator=g).to(DEV)
        for extras in (False, True):
            _same(_forward(lib, rows, w, G, x, buf, extras), _forward(lib, rows, w, G, x, None, extras), ("fwd", G, extras))
        for case in BWD_CASES:
            for init in (None, dx_init):
                _same(_backward(lib, rows, w, G, x, buf, cot, case, init), _backward(lib, rows, w, G, x, None, cot, case, init),
                      ("bwd", G, case, init is not None))


@pytest.mark.parametrize("rows", [129, 16405])
def test_planes_kernels_are_deterministic(lib, rows):
    w = _weights(50, seed=5)
    buf = _proj_planes(lib, w, 50)
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, 64, generator=g).to(DEV)
    cot = {k: torch.randn(rows, 50 if k == "dgate" else 64, generator=g).to(DEV) for k in BWD_CASES["mode1"][0]}
    _same(_forward(lib, rows, w, 50, x, buf, True), _forward(lib, rows, w, 50, x, buf, True), "fwd")
    _same(_backward(lib, rows, w, 50, x, buf, cot, "mode1", x), _backward(lib, rows, w, 50, x, buf, cot, "mode1", x), "bwd")


@pytest.mark.parametrize("rows,G", [(129, 50), (520, 37), (16405, 50), (33, 0)])
def test_planes_kernels_are_as_accurate_as_fp32(lib, rows, G):
    """against fp64 nn.Linear: at most twice the exact-fp32 kernels' error + 2e-7 of the magnitude (test_hip_linear_split)"""
    w = _weights(G, seed=rows)
    buf = _proj_planes(lib, w, G)
    g = torch.Generator().manual_seed(rows + 1)
    x = torch.randn(rows, 64, generator=g).to(DEV)
    cot = {k: torch.randn(rows, 64, generator=g).to(DEV) for k in ("dmq", "dmk", "dmv", "dqa", "dka")}
    cot["dgate"] = torch.randn(rows, max(G, 1), generator=g).to(DEV)
    d = {k: v.double().cpu() for k, v in w.items()}
    xd = x.double().cpu().requires_grad_(True)
    mq, mk, mv = F.linear(xd, d["wq"], d["bq"]), F.linear(xd, d["wk"], d["bk"]), F.linear(xd, d["wv"], d["bv"])
    mq.retain_grad(), mk.retain_grad()
    ref = dict(mq=mq, mk=mk, mv=mv, qa=F.linear(mq, d["waq"], d["baq"]), ka=F.linear(mk, d["wak"], d["bak"]))
    if G:
        ref["gate"] = F.linear(mq, d["wg"], d["bg"])
    pairs = (("mq", "dmq"), ("mk", "dmk"), ("mv", "dmv"), ("qa", "dqa"), ("ka", "dka")) + ((("gate", "dgate"),) if G else ())
    sum((ref[a] * cot[b].double().cpu()).sum() for a, b in pairs).backward()
    ref.update(dmq_total=mq.grad, dmk_total=mk.grad, dx=xd.grad)
    got6 = {**_forward(lib, rows, w, G, x, buf, False), **_backward(lib, rows, w, G, x, buf, cot, "mode1", None)}
    old = lib.acattn_linear_products(0)
    try:
        got32 = {**_forward(lib, rows, w, G, x, None, False), **_backward(lib, rows, w, G, x, None, cot, "mode1", None)}
    finally:
        lib.acattn_linear_products(old)
    for k, v in got6.items():
        want = ref[k].detach()
        e6 = (v.double().cpu() - want).abs().max().item()
        e32 = (got32[k].double().cpu() - want).abs().max().item()
        print(f"rows {rows} G {G} {k}: planes {e6:.3e} fp32 {e32:.3e}")
        assert e6 <= 2 * e32 + 2e-7 * max(1.0, want.abs().max().item()), (k, e6, e32)


def test_planes_are_ignored_once_the_product_mode_is_fp32(lib):
    """planes made, then acattn_linear_products(0) (say between a forward and its backward): the launches take the exact-fp32
    kernels, as they do without planes"""
    w = _weights(50, seed=1)
    buf = _proj_planes(lib, w, 50)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(40, 64, generator=g).to(DEV)
    cot = {k: torch.randn(40, 50 if k == "dgate" else 64, generator=g).to(DEV) for k in BWD_CASES["mode1"][0]}
    old = lib.acattn_linear_products(0)
    try:
        _same(_forward(lib, 40, w, 50, x, buf, False), _forward(lib, 40, w, 50, x, None, False), "fwd")
        _same(_backward(lib, 40, w, 50, x, buf, cot, "mode1", None), _backward(lib, 40, w, 50, x, None, cot, "mode1", None), "bwd")
    finally:
        lib.acattn_linear_products(old)


# ---- ownership: per encoder forward -------------------------------------------------------------------------------------
CFG = dict(n_layers=2, n_heads=2, hidden_size=64, inner_size=256, hidden_dropout_prob=0.5, attn_dropout_prob=0.5,
           hidden_act='gelu', layer_norm_eps=1e-12, initializer_range=0.02, loss_type='CE', combine_option='gate',
           two_level=True, use_order=True, use_distance=True, mask_loss_weight=0.03)


def _batch(B=48, L=50, N=700, seed=1):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    ids = torch.randint(1, N, (B, L), generator=g) * (torch.arange(L)[None] < lens[:, None])
    return {"item_id_list": ids.to(DEV), "item_length": lens.to(DEV), "item_id": torch.randint(1, N, (B,), generator=g).to(DEV)}


def _model(**over):
    torch.manual_seed(0)
    return A.ACSASRec(A.DictConfig(dict(CFG, **over)), A.ItemCount(700)).to(DEV)


@pytest.fixture
def shared_switch(monkeypatch):
    return lambda on: monkeypatch.setattr(planes, "SHARED_PLANES", on)


def test_nothing_stale_survives_a_forward(shared_switch, monkeypatch):
    """forward, change a projection weight and a tail weight in place, forward again: the second call sees the new weights
    exactly as a run without shared planes does (eval / no_grad: the planes serve that forward too), with poisoned buffers"""
    monkeypatch.setattr(attn_launch, "POISON", True)
    model = _model().eval()
    batch = _batch()
    enc = model.trm_encoder
    made = []
    real = planes.make
    monkeypatch.setattr(planes, "make", lambda *a, **k: made.append(real(*a, **k)) or made[-1])
    # what the launches were handed: the planes pointers of every projections / tail forward
    lib, seen = _lib.load(), {"proj": [], "tail": []}
    for name, key in (("acattn_projections_fwd", "proj"), ("acattn_layer_tail_fwd", "tail")):
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda p, *rest, _fn=fn, _key=key: seen[_key].append(p._obj.split_planes) or _fn(p, *rest))
    with torch.no_grad():
        shared_switch(True)
        _, before, _ = model.forward(batch["item_id_list"], batch["item_length"])
        assert all(h is not None and h.proj is not None and h.tail is not None for h in made[-1])
        # the kernels consumed them: layer k's projections and tails ran on layer k's slices
        assert seen["proj"] == [h.proj.data_ptr() for h in made[-1]]
        assert seen["tail"] == [made[-1][0].tail.data_ptr()] + [made[-1][1].tail.data_ptr()] * 2
        enc.layer[0].attack_attention.query.weight.mul_(1.5)
        enc.layer[1].feed_forward.dense_1.weight.add_(0.01)
        _, after, _ = model.forward(batch["item_id_list"], batch["item_length"])
        shared_switch(False)
        seen["proj"].clear()
        _, want, _ = model.forward(batch["item_id_list"], batch["item_length"])
        assert made[-1] == [None, None] and seen["proj"] == [None, None]
    assert torch.isfinite(after).all() and not torch.equal(before, after)
    # the two forms run the same products: no more than the 2e-7 of the magnitude that the bound above grants on top of the
    # fp32 kernels' error
    assert (after - want).abs().max().item() <= 2e-7 * max(1.0, want.abs().max().item())


def test_a_layer_called_alone_splits_for_itself(shared_switch):
    model = _model().eval()
    layer = model.trm_encoder.layer[0]
    x = torch.randn(6, 50, 64, generator=torch.Generator().manual_seed(2)).to(DEV)
    mask = A.StructuredMask(key_valid=torch.ones(6, 50, dtype=torch.uint8, device=DEV), causal=True)
    with torch.no_grad():
        shared_switch(True)
        torch.manual_seed(3)
        alone = layer(x, mask)[1]
        torch.manual_seed(3)
        layers, _ = model.trm_encoder(x, mask, output_all_encoded_layers=True)
    assert torch.isfinite(alone).all()
    assert (alone - layers[0][1]).abs().max().item() <= 2e-7 * max(1.0, alone.abs().max().item())
    xg = x.clone().requires_grad_(True)  # and with a graph: the nodes of a lone layer keep no holder
    layer(xg, mask)[1].sum().backward()
    assert torch.isfinite(xg.grad).all()


@pytest.mark.parametrize("learner,lr,n_off", [("sgd", 0.05, 2), ("adam", 1e-3, 4)])
def test_captured_training_losses_do_not_depend_on_the_switch(shared_switch, learner, lr, n_off):
    """three captured steps with the planes shared against runs without: the losses differ from a run without by no more
    than the runs without differ among themselves (float atomics in the step: bitwise equality is not expected).
    Plain SGD carries the gradients' noise into the weights at its own size.  Adam's first updates are
    lr * g / (|g| + eps): a weight whose gradient is a cancelling sum (the attack key transform's bias, 1e-10) moves by a
    good part of lr in a direction the order of the float atomics decides; with two runs without the switch that agreed to
    the last bit, the first replayed calibrated loss once came out 2 ulp apart with it (6.4966784 / 6.4966774), everything
    else equal -- so the Adam case takes its level from four runs without the switch."""
    def run(on):
        shared_switch(on)
        torch.manual_seed(0)
        model = _model().train()
        trainer = A.AttackSASRecTrainer(A.DictConfig(learner=learner, learning_rate=lr), model)
        batch = _batch()
        trainer.enable_graph(batch, warmup=1)
        out = []
        for _ in range(3):
            att, cal = trainer.train_step(batch)
            out += [att.item(), cal.item()]
        return torch.tensor(out, dtype=torch.float64)

    off = [run(False) for _ in range(n_off)]
    on = run(True)
    rel = lambda a, b: ((a - b).abs() / b.abs()).max().item()
    level = max(rel(a, b) for i, a in enumerate(off) for b in off[:i])
    diff = rel(on, off[0])
    print(f"{learner}: losses off {[o.tolist() for o in off]} on {on.tolist()}: run-to-run {level:.3e}, switch {diff:.3e}")
    assert torch.isfinite(on).all()
    assert (on[0::2] != on[0]).any() or (on[1::2] != on[1]).any()  # the steps are different steps
    assert diff <= level
