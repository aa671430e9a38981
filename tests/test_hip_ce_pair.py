"""GPU suite (-m gpu): the paired cross-entropy forward (acattn_full_sort_ce_fwd_pair: the attacked rows' loss and
direction and the calibrated rows' loss from ONE sweep of the catalogue) against the two separate entry points, the fp64
reference, and the model / trainer with ce.PAIRED_FORWARD off."""
import ctypes as C

import pytest
import torch

import ac_tsr_amd as A
from ac_tsr_amd import _lib, ce

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


@pytest.fixture
def products():
    """Sets the CE products mode for one test and restores what was there."""
    lib = _lib.load()
    old = lib.acattn_full_sort_ce_products(-1)
    yield lambda mode: lib.acattn_full_sort_ce_products(mode)
    lib.acattn_full_sort_ce_products(old)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _problem(out, table, target):
    p = _lib.CeProblem()
    p.B, p.N, p.H = out.shape[0], table.shape[0], out.shape[1]
    p.out, p.table, p.target = out.data_ptr(), table.data_ptr(), target.data_ptr()
    return p


def _inputs(B_a, B_c, N, scale, seed):
    g = torch.Generator().manual_seed(seed)
    out_a = scale * torch.randn(B_a, 64, generator=g)
    out_c = scale * torch.randn(B_c, 64, generator=g)
    table = scale * torch.randn(N, 64, generator=g)
    tgts = []
    for B in (B_a, B_c):
        t = torch.randint(0, N, (B,), generator=g)
        t[: B // 4] = N - 1 - torch.arange(B // 4) % min(N, 1500)  # (targets among the last items: the leftover tiles)
        tgts.append(t)
    return out_a, out_c, table, tgts[0], tgts[1]


def _pair_call(out_a, out_c, table, tgt_a, tgt_c):
    """(rc, lse_a, row_loss_a, dir_a, lse_c, row_loss_c) of the paired entry point; every output starts as NaN."""
    lib = _lib.load()
    pa, pc = _problem(out_a, table, tgt_a), _problem(out_c, table, tgt_c)
    nbytes = lib.acattn_full_sort_ce_fwd_pair_workspace_bytes(C.byref(pa), C.byref(pc))
    if nbytes < 0:
        return (int(nbytes),) + (None,) * 5
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    B_a, B_c = out_a.shape[0], out_c.shape[0]
    lse_a, rl_a, dir_a = (torch.full(s, NAN, device=DEV) for s in ((B_a,), (B_a,), (B_a, 64)))
    lse_c, rl_c = (torch.full((B_c,), NAN, device=DEV) for _ in range(2))
    rc = lib.acattn_full_sort_ce_fwd_pair(C.byref(pa), C.byref(pc), _ptr(ws), _ptr(lse_a), _ptr(rl_a), _ptr(dir_a), _ptr(lse_c),
                                          _ptr(rl_c), None)
    torch.cuda.synchronize()
    return rc, lse_a, rl_a, dir_a, lse_c, rl_c


def _dir_call(out, table, tgt):
    lib = _lib.load()
    p = _problem(out, table, tgt)
    ws = torch.empty(lib.acattn_full_sort_ce_workspace_bytes(C.byref(p)), dtype=torch.uint8, device=DEV)
    B = out.shape[0]
    lse, rl, d = (torch.full(s, NAN, device=DEV) for s in ((B,), (B,), (B, 64)))
    assert lib.acattn_full_sort_ce_fwd_dir(C.byref(p), _ptr(ws), _ptr(lse), _ptr(rl), _ptr(d), None) == 0
    torch.cuda.synchronize()
    return lse, rl, d


# (B_a, B_c, N, products mode): both sets end inside a super-block of 32 rows, different super-block counts, ragged last wave,
# no leftover tiles; a single partial super-block and fewer items than one workgroup; set c with more super-blocks than set
# a; [default mode] one leftover tile, itself ragged; the shape of SPLIT in tests/test_hip_ce.py
SHAPES = [(33, 40, 1000, 2), (1, 5, 449, 2), (16, 70, 257, 2), (40, 33, 98305, 1), (33, 48, 99990, 1)]


@pytest.mark.parametrize("B_a,B_c,N,mode", SHAPES)
@pytest.mark.parametrize("scale", [0.02, 1.0])
def test_paired_call_matches_the_separate_calls(B_a, B_c, N, mode, scale, products):
    """Set a: bitwise what acattn_full_sort_ce_fwd_dir gives (same code path, same summation order).  Set c: the bounds
    tests/test_hip_ce.py states for acattn_full_sort_ce_fwd against fp64 on the CPU -- row losses within
    1e-5 max(1, |ref|), their mean within 1e-5 relative (its partials are grouped per workgroup, not per wave pair, so it
    need not be bitwise equal to that entry point)."""
    products(mode)
    out_a, out_c, table, tgt_a, tgt_c = _inputs(B_a, B_c, N, scale, B_a + B_c + N)
    ref_c = torch.nn.functional.cross_entropy(out_c.double() @ table.double().t(), tgt_c, reduction="none")
    dev = [t.to(DEV) for t in (out_a, out_c, table, tgt_a, tgt_c)]
    rc, lse_a, rl_a, dir_a, lse_c, rl_c = _pair_call(*dev)
    assert rc == 0
    want = _dir_call(dev[0], dev[2], dev[3])
    for name, got, exp in zip(("lse_a", "row_loss_a", "dir_a"), (lse_a, rl_a, dir_a), want):
        assert not torch.isnan(got).any(), name
        assert torch.equal(got, exp), (name, (got - exp).abs().max().item())
    err = (rl_c.cpu().double() - ref_c).abs().max().item()
    mean_err = abs(rl_c.cpu().double().mean().item() - ref_c.mean().item()) / abs(ref_c.mean().item())
    lse_ref = torch.logsumexp(out_c.double() @ table.double().t(), dim=1)
    lse_err = (lse_c.cpu().double() - lse_ref).abs().max().item()
    print(f"set c: row loss err {err:.3e} (bound {1e-5 * max(1.0, ref_c.abs().max().item()):.3e}), mean rel err {mean_err:.3e}, "
          f"lse err {lse_err:.3e}")
    assert not torch.isnan(rl_c).any() and not torch.isnan(lse_c).any()
    assert err <= 1e-5 * max(1.0, ref_c.abs().max().item())
    assert mean_err <= 1e-5
    assert lse_err <= 1e-5 * max(1.0, lse_ref.abs().max().item())


def test_mean_output_of_the_finishing_launch(products):
    """acattn_attacked_loss_finish_rows_pair: mean_c against row_loss_c.mean() within 1e-6 relative (the bound of
    test_mean_node_scalar_cotangent_matches_rows_node between two forms of the same mean); the attacked outputs are those
    of acattn_attacked_loss_finish_rows."""
    products(2)
    lib = _lib.load()
    B, N = 64, 3001
    out_a, out_c, table, tgt_a, tgt_c = (t.to(DEV) for t in _inputs(B, B, N, 0.5, 3))
    rc, lse_a, rl_a, dir_a, lse_c, rl_c = _pair_call(out_a, out_c, table, tgt_a, tgt_c)
    assert rc == 0
    g = torch.Generator().manual_seed(4)
    pens = [torch.rand(B, 2, 4, generator=g).to(DEV) for _ in range(2)]
    ptrs = (C.c_void_p * 2)(*(t.data_ptr() for t in pens))
    res, res_ref = torch.full((4,), NAN, device=DEV), torch.full((4,), NAN, device=DEV)
    mean_c = torch.full((), NAN, device=DEV)
    d1, d2 = dir_a.clone(), dir_a.clone()
    assert lib.acattn_attacked_loss_finish_rows_pair(_ptr(rl_a), B, ptrs, 2, pens[0].numel(), 0.03, _ptr(res), _ptr(d1), d1.numel(),
                                                     _ptr(rl_c), B, _ptr(mean_c), None) == 0
    assert lib.acattn_attacked_loss_finish_rows(_ptr(rl_a), B, ptrs, 2, pens[0].numel(), 0.03, _ptr(res_ref), _ptr(d2), d2.numel(),
                                                None) == 0
    torch.cuda.synchronize()
    want = rl_c.mean().item()
    assert abs(mean_c.item() - want) <= 1e-6 * abs(want), (mean_c.item(), want)
    assert torch.equal(res, res_ref) and torch.equal(d1, d2)


def _tiny_model(N, seed=0):
    torch.manual_seed(seed)
    cfgd = dict(n_layers=2, n_heads=2, hidden_size=64, inner_size=256, hidden_dropout_prob=0.2, attn_dropout_prob=0.2,
                hidden_act='gelu', layer_norm_eps=1e-12, initializer_range=0.02, loss_type='CE', combine_option='gate',
                two_level=True, use_order=True, use_distance=True, mask_loss_weight=0.03)
    return A.ACSASRec(A.DictConfig(cfgd), A.ItemCount(N)).to(DEV).train()


def _tiny_batch(B, N, L=50):
    g = torch.Generator().manual_seed(1)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    ids = torch.randint(1, N, (B, L), generator=g) * (torch.arange(L)[None] < lens[:, None])
    return {"item_id_list": ids.to(DEV), "item_length": lens.to(DEV), "item_id": ids[torch.arange(B), lens - 1].to(DEV)}


@pytest.fixture
def paired_switch():
    old = ce.PAIRED_FORWARD
    yield lambda on: setattr(ce, "PAIRED_FORWARD", bool(on))
    ce.PAIRED_FORWARD = old


def _losses(model, batch, seed=7):
    torch.manual_seed(seed)  # the kernels' dropout / noise seeds are drawn from torch's CPU generator
    att, cal = model.calculate_loss(batch)
    torch.cuda.synchronize()
    return att.detach().clone(), cal.detach().clone()


@pytest.mark.parametrize("mode,N", [(1, 3001), (0, 100000)])
def test_where_the_paired_form_does_not_apply(mode, N, products, paired_switch):
    """A small catalogue in the default mode and the exact-fp32 products at any size: -100 from the argument checks (nothing
    is launched behind the refusal), and the model's losses with PAIRED_FORWARD on are exactly those with it off."""
    products(mode)
    out_a, out_c, table, tgt_a, tgt_c = (t.to(DEV) for t in _inputs(8, 8, N, 0.5, 11))
    lib = _lib.load()
    pa, pc = _problem(out_a, table, tgt_a), _problem(out_c, table, tgt_c)
    assert lib.acattn_full_sort_ce_fwd_pair_workspace_bytes(C.byref(pa), C.byref(pc)) == -100
    junk = torch.full((8, 64), NAN, device=DEV)
    assert lib.acattn_full_sort_ce_fwd_pair(C.byref(pa), C.byref(pc), _ptr(junk), _ptr(junk), _ptr(junk), _ptr(junk), _ptr(junk),
                                            _ptr(junk), None) == -100
    torch.cuda.synchronize()
    assert torch.isnan(junk).all()
    assert ce.paired_forward(out_a, out_c, table, tgt_a) is None
    model, batch = _tiny_model(N), _tiny_batch(8, N)
    paired_switch(True)
    on = _losses(model, batch)
    paired_switch(False)
    off = _losses(model, batch)
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])


def test_invalid_targets_give_nan_losses_and_no_out_of_bounds_access(products):
    """Targets -1 and N in both sets: those rows' losses are NaN, every other row (and all of lse and the direction's
    soft-max part) is what it is without them -- the finish clamps the address, it does not read a table row for them
    (the pattern of test_invalid_target_gives_nan_loss_and_no_out_of_bounds_access)."""
    products(2)
    B, N = 16, 257
    out_a, out_c, table, tgt_a, tgt_c = (t.to(DEV) for t in _inputs(B, B, N, 1.0, 5))
    good = _pair_call(out_a, out_c, table, tgt_a, tgt_c)
    bad_a, bad_c = tgt_a.clone(), tgt_c.clone()
    bad_a[3], bad_a[9], bad_c[2], bad_c[11] = -1, N, N, -1
    rc, lse_a, rl_a, dir_a, lse_c, rl_c = _pair_call(out_a, out_c, table, bad_a, bad_c)
    assert rc == 0 and good[0] == 0
    ok_a, ok_c = torch.ones(B, dtype=torch.bool, device=DEV), torch.ones(B, dtype=torch.bool, device=DEV)
    ok_a[[3, 9]] = False
    ok_c[[2, 11]] = False
    assert torch.isnan(rl_a[~ok_a]).all() and torch.isnan(rl_c[~ok_c]).all()
    assert torch.equal(rl_a[ok_a], good[2][ok_a]) and torch.equal(rl_c[ok_c], good[5][ok_c])
    assert torch.equal(lse_a, good[1]) and torch.equal(lse_c, good[4])
    assert torch.equal(dir_a[ok_a], good[3][ok_a]) and torch.isfinite(dir_a).all()


def _grads(N, batch, seed=7):
    model = _tiny_model(N)
    trainer = A.AttackSASRecTrainer(A.DictConfig(learner='adam', learning_rate=1e-3), model)
    torch.manual_seed(seed)
    att, cal = trainer._pass_one(batch)
    trainer._pass_two(att)
    torch.cuda.synchronize()
    return att.detach().clone(), cal.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()
                                                       if p.grad is not None}


def test_model_losses_and_gradients_with_the_switch_on_against_off(products, paired_switch):
    """A small ACSASRec (B = 8, L = 50, hidden 64, 2 heads, 2 layers, 300 items; split products for every size, train mode,
    the same torch seed and therefore the same kernel seeds): the attacked loss is bitwise what it is without the paired
    forward, the calibrated loss within 1e-6 relative, every gradient of the two-pass step within
    1e-6 max|g| + 1e-9 per tensor."""
    products(2)
    N = 300
    model, batch = _tiny_model(N), _tiny_batch(8, N)
    paired_switch(True)
    assert ce.paired_forward(torch.zeros(8, 64, device=DEV), torch.zeros(8, 64, device=DEV), model.item_embedding.weight,
                             batch["item_id"]) is not None  # (the paired path is the one taken here)
    att_on, cal_on, g_on = _grads(N, batch)
    paired_switch(False)
    att_off, cal_off, g_off = _grads(N, batch)
    print(f"attacked {att_on.item()!r} / {att_off.item()!r}, calibrated {cal_on.item()!r} / {cal_off.item()!r}")
    assert torch.equal(att_on, att_off)
    assert abs(cal_on.item() - cal_off.item()) <= 1e-6 * abs(cal_off.item())
    assert set(g_on) == set(g_off) and any("attack_query_transform" in n for n in g_on) and "item_embedding.weight" in g_on
    worst = []
    for n in g_off:
        scale = g_off[n].abs().max().item()
        diff = (g_on[n] - g_off[n]).abs().max().item()
        print(f"{n}: max|on - off| = {diff:.3e}, max|g| = {scale:.3e}")
        if diff > 1e-6 * scale + 1e-9:
            worst.append((n, diff, scale))
    assert not worst, worst


def _train(N, graph, combined=False, steps=1):
    """Parameters and losses after one warm-up step and `steps` further steps.  The captured step draws its host seeds at the
    capture and adds a device counter that every replay advances (trainer.enable_graph); the eager trainer is given the
    same counter (StepState.seed_tensor, advanced by _pass_one), so that both see the same dropout / noise draws."""
    model, batch = _tiny_model(N, seed=3), _tiny_batch(8, N)
    trainer = A.AttackSASRecTrainer(A.DictConfig(learner='adam', learning_rate=1e-3), model, combined_backward=combined)
    torch.manual_seed(5)
    if graph:
        trainer.enable_graph(batch, warmup=1)  # (>= 1: Adam's state must exist before the capture)
    else:
        trainer._seed_t = torch.zeros(1, dtype=torch.int64, device=DEV)
        trainer.state.seed_tensor = trainer._seed_t
        att, cal = (t.detach().clone() for t in trainer.train_step(batch))
    for _ in range(steps):
        att, cal = (t.detach().clone() for t in trainer.train_step(batch))
    torch.cuda.synchronize()
    return att, cal, {k: v.detach().clone() for k, v in model.state_dict().items()}


def test_trainer_step_eager_graph_and_one_walk_with_the_paired_forward(products, paired_switch):
    """AttackSASRecTrainer.train_step through the paired forward: captured (enable_graph) against eager -- the same losses
    and the same updated parameters within 1e-6 max(1, max|x|).  No existing test compares a captured trainer with an eager
    one number for number; the bound is the tightest trainer-against-trainer bound of tests/test_hip_backward.py, the one
    test_data_parallel_code_path_matches_plain_trainer holds the synchronizer's trainer to against the plain one (each
    under graph and under eager).  Same kernels, same inputs, same seeds on both sides here: what may differ is the
    arrival order of the float atomics (one-hot rows of d_table).  The eager side is given the captured side's seed
    counter through the trainer's own fields (_seed_t / StepState.seed_tensor, what enable_graph sets): the trainer has
    no public hook for it.  And the one-walk mode (combined_backward=True) still runs and gives the same losses."""
    products(2)
    paired_switch(True)
    N = 300
    att_e, cal_e, st_e = _train(N, graph=False)
    att_g, cal_g, st_g = _train(N, graph=True)
    print(f"eager {att_e.item()!r} {cal_e.item()!r}   graph {att_g.item()!r} {cal_g.item()!r}")
    for a, b in ((att_g, att_e), (cal_g, cal_e)):
        assert torch.isfinite(a) and abs(a.item() - b.item()) <= 1e-6 * max(1.0, abs(b.item())), (a.item(), b.item())
    for k in st_e:
        diff = (st_e[k] - st_g[k]).abs().max().item()
        if diff > 0:
            print(f"{k}: max|eager - graph| = {diff:.3e}")
        assert diff <= 1e-6 * max(1.0, st_e[k].abs().max().item()), k
    att_1, cal_1, _ = _train(N, graph=False, combined=True, steps=0)  # (first step: the losses of the same forward)
    att_2, cal_2, _ = _train(N, graph=False, combined=False, steps=0)
    assert torch.isfinite(att_1) and torch.isfinite(cal_1)
    assert att_1.item() == att_2.item() and cal_1.item() == cal_2.item()
