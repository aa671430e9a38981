"""GPU suite (-m gpu): the long form of the calibrated attention core (csrc/acattn_long_fwd.inc, acattn_long_bwd.inc),
208 < L <= 496 -- and at L <= 208 with the long form pinned -- through the operator, the encoder, both models and the trainer.

Cases: tests/_long_cases.py (its conditioning is checked on the CPU by tests/test_long_sequence_cases_cpu.py).  The forward
oracle and the comparison of live and fully masked rows live in tests/_attention_fwd_ref.py (shared with
tests/test_hip_fwd_edges.py).

Forward bounds, on query rows the mask lets see a key: |M - ref| <= 5e-6 and both contexts <= 1e-4 against
oracle/ac_tsr_ref.py::core_from_projected in float32 (the project's figures: tests/test_hip_onehop.py).  row_stats are the
natural-log normalisers of the five soft-maxes (six with combine `fixed`), compared with a float64 evaluation of the same
chain on the same draws: <= 1e-4, the contexts' bound (a normaliser's error is the relative error of a row sum).  Fully
masked rows (left padding under the causal mask) follow the reference's fp32 `+ (-10000)` quantisation: they are compared
against the float32 oracle at the 2e-3 cap of every gradient test, the way
tests/test_hip_attention_bwd_fp64.py::test_fully_masked_rows_match_the_fp32_oracle treats them; their normalisers carry the
-10000 and are held to two fp32 roundings at that magnitude (2 * 2^-10).

Backward bounds: tests/test_hip_attention_bwd_fp64.py's (its helpers are imported): tensor gradients within
max(1e-4, 2 * e32) of the float64 oracle (never above 2e-3), single-number gradients within 2e-3, absolute floor 1e-7.
Model bounds: 2e-3 * max|g| against the float32 oracle's two-pass gradients (tests/test_hip_backward.py), logits 1e-4.

Every output buffer of every launch here starts as NaN (attn_launch.POISON is switched on for the module): an element a
long kernel does not write fails the comparison it takes part in, or the finiteness assertions.
"""
import math
import types

import pytest
import torch

import ac_tsr_amd as A
from ac_tsr_amd import _lib, attn_launch, ops
from oracle import ac_tsr_ref as O
from tests import _attention_fp64 as F
from tests._attention_fwd_ref import (CTX_BOUND, DEAD_CAP, M_BOUND, STAT_BOUND, check_forward as _check_forward,  # noqa: F401
                                      ocfg as _ocfg, oracle_forward as _oracle_forward)
from tests import _long_cases as LC
from tests import test_hip_attention_bwd_fp64 as T64

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 777


@pytest.fixture(autouse=True, scope="module")
def _poisoned_outputs():
    old = attn_launch.POISON
    attn_launch.POISON = True
    yield
    attn_launch.POISON = old


@pytest.fixture
def pins():
    """Pins the forward / backward kernel for one test and restores the automatic choice."""
    lib = _lib.load()
    yield lib
    lib.acattn_select_forward_kernel(_lib.FWD_AUTO)
    lib.acattn_select_backward_kernel(_lib.BWD_AUTO)


def _device_problem(c, pr, draws, explicit=True, seed=SEED):
    """(lib, acattn_problem, the device tensors it points to) through ops._fill_problem, the operator's own checks."""
    lib = _lib.load()
    x = {k: v.to(DEV) for k, v in pr.t.items()}
    cfg = A.AttentionConfig(n_heads=c.nh, combine_option=c.combine, two_level=True, anneal_rate=c.anneal_rate)
    mask = A.StructuredMask(pr.kv.to(DEV), causal=c.causal) if c.mask == "structured" else pr.mask_dense.to(DEV).contiguous()
    rnd = None
    if explicit:
        u8 = lambda t: None if t is None else t.to(torch.uint8).to(DEV)
        rnd = A.ExplicitRandomness(noise=draws["noise"].to(DEV), keep_after=u8(draws["keep_after"]), keep_mask=u8(draws["keep_mask"]))
    keep = [x, mask, rnd]
    flat = lambda t: t.reshape(-1).contiguous()
    prob = ops._fill_problem(x["q"], x["k"], x["v"], x["qa"], x["ka"], x["gl"] if c.combine == "gate" else None, mask,
                             flat(x["w_order"]) if "order" in c.terms else None, x["b_order"],
                             flat(x["w_dist"]) if "distance" in c.terms else None, x["b_dist"], x["scalar"], None, cfg, c.p_drop,
                             rnd, seed, keep)
    return lib, prob, x, keep


# ---- 1. forward, explicit randomness --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LC.CASES, ids=lambda c: c.id)
def test_forward_matches_the_oracle_with_explicit_randomness(case):
    c = case
    pr, draws = F.problem(c), F.torch_draws(c)
    lib, prob, x, keep = _device_problem(c, pr, draws)
    ctx_a, ctx_c, M, stats, _, pen = attn_launch.attention_fwd_launch(lib, prob, x["q"], c.nh, adversarial=True, want_penalty=True)
    got = tuple(t.cpu() for t in (ctx_a, ctx_c, M, stats))
    _check_forward(c, pr, got, _oracle_forward(c, pr, draws, torch.float32), _oracle_forward(c, pr, draws, torch.float64))
    # acattn_fwd_out.penalty_part: sum (1 - M)^2 over each query block's rows and all keys
    B, nh, L = c.B, c.nh, c.L
    rows = torch.nn.functional.pad((1 - got[2].double()) ** 2, (0, 0, 0, 16 * ((L + 15) // 16) - L)).sum(-1)
    want = rows.view(B, nh, -1, 16).sum(-1)
    assert torch.isfinite(pen).all() and (pen.cpu().double() - want).abs().max().item() <= 1e-5 * want.max().item()


def test_spatial_only_forward_runs_at_long_sequences():
    """adversarial = 0: one soft-max, one context (the spatial-only backward stays at L <= 208: the CPU suite)."""
    c = LC.CASES[0]
    pr = F.problem(c)
    x = {k: v.to(DEV) for k, v in pr.t.items()}
    cfg = A.AttentionConfig(n_heads=c.nh, combine_option="gate", adversarial=False)
    kw = {k: x[k] for k in ("w_order", "b_order", "w_dist", "b_dist", "scalar")}
    with torch.no_grad():
        _, ctx, _, _ = A.calibrated_attention(x["q"], x["k"], x["v"], None, None, None, A.StructuredMask(pr.kv.to(DEV), causal=True), cfg,
                                              p_drop=0.0, seed=SEED, **kw)
        ocfg = _ocfg(c._replace(p_drop=0.0))
        ref = O.core_from_projected(pr.t["q"], pr.t["k"], pr.t["v"], pr.t["qa"], pr.t["ka"], pr.t["gl"], pr.mask_dense, pr.t["w_order"],
                                    pr.t["b_order"], pr.t["w_dist"], pr.t["b_dist"], pr.t["scalar"], ocfg, torch.zeros(c.B, c.nh, c.L, c.L),
                                    materialize=False)
    want = O.context_only(ref["after"], O._heads(pr.t["v"], c.nh).permute(0, 2, 1, 3))
    assert torch.isfinite(ctx).all() and (ctx.cpu() - want).abs().max().item() <= CTX_BOUND


# ---- 2. forward, counter randomness ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 257, 64, 2), (1, 496, 64, 2)], ids=lambda s: "B%d_L%d_H%d_h%d" % s)
def test_forward_matches_the_oracle_with_counter_randomness(shape):
    c = F._case("counter", "train", shape)
    pr = F.problem(c)
    rnd = A.materialize_randomness(c.B, c.nh, c.L, SEED, c.p_drop, DEV)
    draws = {"noise": rnd.noise.cpu(), "keep_after": rnd.keep_after.cpu().float(), "keep_mask": rnd.keep_mask.cpu().float(),
             "keep_before": None}
    lib, prob, x, keep = _device_problem(c, pr, draws, explicit=False)
    run = lambda p: tuple(t.cpu() for t in attn_launch.attention_fwd_launch(lib, p, x["q"], c.nh, adversarial=True, want_penalty=False)[:4])
    got = run(prob)
    _check_forward(c, pr, got, _oracle_forward(c, pr, draws, torch.float32), _oracle_forward(c, pr, draws, torch.float64), tag="-counter")
    again = run(prob)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), "two launches with one seed differ"
    # seed_device is added to the seed inside the kernel: the draws of seed + 5
    step = torch.tensor([5], dtype=torch.int64, device=DEV)
    _, prob5, x5, keep5 = _device_problem(c, pr, draws, explicit=False)
    prob5.seed_device = step.data_ptr()
    shifted = tuple(t.cpu() for t in attn_launch.attention_fwd_launch(lib, prob5, x5["q"], c.nh, adversarial=True, want_penalty=False)[:4])
    _, prob_plain, x6, keep6 = _device_problem(c, pr, draws, explicit=False, seed=SEED + 5)
    plain = tuple(t.cpu() for t in attn_launch.attention_fwd_launch(lib, prob_plain, x6["q"], c.nh, adversarial=True, want_penalty=False)[:4])
    assert all(torch.equal(a, b) for a, b in zip(shifted, plain))
    assert not torch.equal((shifted[2] == 0), (got[2] == 0)), "seed_device did not shift the dropout draws"


# ---- 3. the long form pinned where the other kernels also run -------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 208, 64, 2), (3, 50, 64, 2), (6, 37, 64, 2)], ids=lambda s: "B%d_L%d_H%d_h%d" % s)
def test_pinned_long_forward_equals_the_automatic_choice(shape, pins):
    c = F._case("pinned", "train", shape)
    pr = F.problem(c)
    lib, prob, x, keep = _device_problem(c, pr, None, explicit=False)
    run = lambda: tuple(t.cpu() for t in attn_launch.attention_fwd_launch(lib, prob, x["q"], c.nh, adversarial=True, want_penalty=False)[:4])
    auto = run()
    assert pins.acattn_select_forward_kernel(_lib.FWD_LONG) == _lib.FWD_AUTO
    long_ = run()
    assert pins.acattn_select_forward_kernel(_lib.FWD_AUTO) == _lib.FWD_LONG
    assert torch.equal(auto[2] == 0, long_[2] == 0), "the dropped entries of M differ: not the same counter draws"
    for name, a, b, bound in (("ctx_attacked", auto[0], long_[0], CTX_BOUND), ("ctx_calibrated", auto[1], long_[1], CTX_BOUND),
                              ("M", auto[2], long_[2], M_BOUND), ("row_stats", auto[3][..., :5], long_[3][..., :5], STAT_BOUND)):
        e = (a - b).abs().max().item()
        print(f"long_sequences_accuracy pinned_forward B{c.B}_L{c.L} {name} long_vs_auto={e:.3e}")
        assert torch.isfinite(b).all() and e <= bound, (name, e)


def _backward_case(c, lib, pin):
    pr = F.problem(c)
    draws = T64._draws(c, A.materialize_randomness(c.B, c.nh, c.L, T64.SEED, c.p_drop, DEV) if c.kind == "train" else None)
    ref64 = F.oracle_grads(c, pr, draws, pr.cot, torch.float64)
    ref32 = F.oracle_grads(c, pr, draws, pr.cot, torch.float32)
    lib.acattn_select_backward_kernel(pin)
    try:
        got = T64._kernel_grads(c, pr, draws, pr.cot)
    finally:
        lib.acattn_select_backward_kernel(_lib.BWD_AUTO)
    for n, g in got.items():
        assert torch.isfinite(g).all(), f"{c.id}: d{n} holds an element no kernel wrote (or a non-finite value)"
    failures = T64._compare(c, "-long", got, ref64, ref32)
    assert not failures, f"{c.id}: " + "; ".join(failures)
    return pr, draws, got, ref64


@pytest.mark.parametrize("case", [next(c for c in F.CASES if c.id == "L37-all-auto"), F._case("cfg4_shape_B2-all-long", "train", (2, 200, 128, 4))],
                         ids=lambda c: c.id)
def test_pinned_long_backward_matches_the_fp64_oracle(case, pins):
    _backward_case(case, pins, _lib.BWD_LONG)


# ---- 4. backward against the float64 oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LC.CASES, ids=lambda c: c.id)
def test_gradients_match_the_fp64_oracle(case, pins):
    c = case
    pr, draws, got, ref64 = _backward_case(c, pins, _lib.BWD_AUTO)
    # gradients the loss does not reach are exactly zero
    if c.pattern == "attacked_read_row_plus_mask":
        assert ref64["gl"].abs().max() == 0 and got["gl"].abs().max() == 0


_LEFT_PAD = next(c for c in LC.CASES if c.left_pad)
_DEAD = {}


def _dead_rows():
    if not _DEAD:
        c = _LEFT_PAD
        pr = F.problem(c)
        draws = T64._draws(c, A.materialize_randomness(c.B, c.nh, c.L, T64.SEED, c.p_drop, DEV))
        _DEAD.update(got=T64._kernel_grads(c, pr, draws, pr.cot_dead), ref32=F.oracle_grads(c, pr, draws, pr.cot_dead, torch.float32),
                     ref64=F.oracle_grads(c, pr, draws, pr.cot_dead, torch.float64))
    return _DEAD


@pytest.mark.parametrize("grad", F.leaf_names(_LEFT_PAD))
def test_fully_masked_rows_match_the_fp32_oracle(grad):
    """The fully masked rows of the left-padded sequence alone (their cotangents only), against the FLOAT32 oracle, which
    quantises them as the reference's fp32 `+ (-10000)` does, at the 2e-3 cap of every gradient test -- or, where the float32
    oracle is itself further than half of that from the float64 one on these rows, at twice that distance (the margin this
    project grants a kernel over the fp32 restatement of its arithmetic).
    The backward renormalises such rows (csrc/acattn_long_bwd.inc: their stored normalisers carry the -10000 and are rounded
    to 2^-10, which scaled a row's whole contribution by 1 +- 5e-4): without that db_order, a sum over rows that cancels to
    1e-2 of its terms, was 1.3e-2 of its value off; with it every gradient here is within 6e-5 (db_order 4.1e-6)."""
    d = _dead_rows()
    abs_e, scale = F.abs_err_and_scale(d["got"][grad], d["ref32"][grad])
    e32 = F.abs_err_and_scale(d["ref32"][grad], d["ref64"][grad])[0] / max(scale, 1e-300)
    bound = max(DEAD_CAP, 2 * e32)
    print(f"long_sequences_accuracy case={_LEFT_PAD.id} fully_masked_rows grad=d{grad} e_vs_fp32={abs_e / max(scale, 1e-300):.3e} "
          f"oracle32_vs_64={e32:.3e} bound={bound:.3e}")
    assert torch.isfinite(d["got"][grad]).all()
    assert abs_e <= bound * scale + F.ABS_FLOOR, f"d{grad}: {abs_e:.3e} of {scale:.3e} (bound {bound:.3e})"


# ---- 5. models ------------------------------------------------------------------------------------------------------------------
L_MODEL, N_ITEMS = 224, 500
CFGD = dict(n_layers=2, n_heads=2, hidden_size=64, inner_size=128, hidden_dropout_prob=0.5, attn_dropout_prob=0.5, hidden_act='gelu',
            layer_norm_eps=1e-12, initializer_range=0.02, loss_type='CE', combine_option='gate', two_level=True, use_order=True,
            use_distance=True, mask_loss_weight=0.03, MAX_ITEM_LIST_LENGTH=L_MODEL, gate_seq_length=L_MODEL)


def _mcfg(bidirectional=False, **over):
    d = dict(CFGD, **over)
    enc = O.EncoderCfg(n_layers=d["n_layers"], n_heads=d["n_heads"], hidden_size=d["hidden_size"], inner_size=d["inner_size"],
                       hidden_dropout_prob=d["hidden_dropout_prob"], attn_dropout_prob=d["attn_dropout_prob"], combine_option="gate",
                       seq_length=L_MODEL)
    return O.ModelCfg(enc=enc, n_items=N_ITEMS, max_seq_length=L_MODEL, mask_loss_weight=d["mask_loss_weight"], bidirectional=bidirectional)


def _batch(B=4, seed=1):
    g = torch.Generator().manual_seed(seed)
    lens = torch.tensor([L_MODEL, 17, 130, 209][:B]) if B <= 4 else torch.randint(1, L_MODEL + 1, (B,), generator=g)
    ids = torch.randint(1, N_ITEMS, (B, L_MODEL), generator=g) * (torch.arange(L_MODEL)[None] < lens[:, None])
    return {"item_id_list": ids, "item_length": lens, "item_id": torch.randint(1, N_ITEMS, (B,), generator=g)}


def _sasrec(**over):
    torch.manual_seed(0)
    return A.ACSASRec(A.DictConfig(dict(CFGD, **over)), A.ItemCount(N_ITEMS)).to(DEV)


def _device_rnds(rnds):
    out = []
    for r in rnds:
        ns = types.SimpleNamespace()
        for f in ("noise", "keep_after", "keep_before", "keep_mask", "keep_out_att", "keep_out_cal", "keep_ffn_att", "keep_ffn_cal"):
            t = getattr(r, f)
            setattr(ns, f, None if t is None else (t.to(DEV) if f == "noise" else t.to(torch.uint8).to(DEV)))
        out.append(ns)
    return out


def _two_pass(model, att, cal):
    for n, p in model.named_parameters():
        p.requires_grad = not A.is_attack_param(n)
    cal.backward(retain_graph=True)
    for n, p in model.named_parameters():
        p.requires_grad = A.is_attack_param(n)
    att.backward()
    for n, p in model.named_parameters():
        p.requires_grad = True


def _model_reference(model, batch, train):
    cfg = _mcfg()
    P = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    torch.manual_seed(11)
    B = batch["item_id_list"].shape[0]
    rnds = [O.draw_layer_randomness((B, 2, L_MODEL, L_MODEL), (B, L_MODEL, 64), cfg.enc, train) for _ in range(2)]
    keep_emb = torch.empty(B, L_MODEL, 64).bernoulli_(0.5) if train else None
    return cfg, P, rnds, keep_emb


def _losses_fp64(batch, P, cfg, rnds, keep_emb):
    import copy
    with F.default_dtype(torch.float64), torch.no_grad():
        r64 = []
        for r in rnds:
            rr = copy.copy(r)
            for f, t in vars(r).items():
                setattr(rr, f, None if t is None else t.double())
            r64.append(rr)
        att, cal = O.calculate_loss(batch, {k: v.double() for k, v in P.items()}, cfg, True, r64, keep_emb.double(), materialize=False)
    return att.item(), cal.item()


@pytest.mark.parametrize("combined", [False, True], ids=["two_walks", "combined_backward"])
def test_acsasrec_losses_and_two_pass_gradients_match_the_oracle(combined):
    model = _sasrec().train()
    batch = _batch()
    cfg, P, rnds, keep_emb = _model_reference(model, batch, True)
    ref_att, ref_cal, ref = O.two_pass_grads(batch, P, cfg, True, rnds, keep_emb, materialize=False)
    dev_batch = {k: v.to(DEV) for k, v in batch.items()}
    trainer = A.AttackSASRecTrainer(A.DictConfig(learner='adam', learning_rate=1e-4), model, combined_backward=combined)
    model.zero_grad()
    att, cal = model.calculate_loss(dev_batch, _rnds=_device_rnds(rnds), _keep_emb=keep_emb.to(DEV))
    # Losses: within the absolute 1e-4 of the L = 50 tests (tests/test_hip_backward.py), of the oracle in FLOAT64.  The
    # attacked loss is mostly its penalty term here, 0.03 * || 1 - M || over 4 x 2 x 224 x 224 elements, and the float32
    # oracle's own sum of those 4e5 terms is 1.98e-4 from the float64 one (printed): not a yardstick at 1e-4.
    att64, cal64 = _losses_fp64(batch, P, cfg, rnds, keep_emb)
    print(f"long_sequences_accuracy model losses att={att.item():.7f} ref64={att64:.7f} ref32={ref_att.item():.7f} "
          f"cal={cal.item():.7f} ref64={cal64:.7f} ref32={ref_cal.item():.7f}")
    assert abs(att.item() - att64) <= 1e-4 and abs(cal.item() - cal64) <= 1e-4
    if combined:
        trainer.combined_backward_walk(att, cal)
        # above 208 keys the library has no paired (two-cotangent) launch: the walk takes its one-launch-per-set path
        assert trainer.last_walk_stats["pair_nodes"] == 0, trainer.last_walk_stats
    else:
        _two_pass(model, att, cal)
    for n, p in model.named_parameters():
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        assert torch.isfinite(g).all(), n
        err = (g.cpu() - ref[n]).abs().max().item()
        assert err <= 2e-3 * ref[n].abs().max().item() + 2e-8, (n, err, ref[n].abs().max().item())


def test_acsasrec_full_sort_logits_match_the_oracle():
    model = _sasrec().eval()
    batch = _batch()
    cfg, P, rnds, _ = _model_reference(model, batch, False)
    with torch.no_grad():
        _, scores = model.full_sort_predict({k: v.to(DEV) for k, v in batch.items()})
        want = O.full_sort_predict(batch, P, cfg, rnds)
    assert torch.isfinite(scores).all() and (scores.cpu() - want).abs().max().item() <= 1e-4


def _train(graph, steps=1):
    """Parameters and losses after one warm-up step and `steps` further steps (tests/test_hip_ce_pair.py::_train at
    L = 224): Adam at 1e-3, both dropouts on.  The captured step draws its host seeds at the capture and adds a device
    counter that every replay advances (trainer.enable_graph); the eager trainer is given the same counter
    (StepState.seed_tensor), so both sides see the same dropout / noise draws -- through acattn_problem.seed_device in the
    long forward AND the long backward."""
    model = _sasrec(hidden_dropout_prob=0.1, attn_dropout_prob=0.5).train()
    batch = {k: v.to(DEV) for k, v in _batch(B=8, seed=3).items()}
    trainer = A.AttackSASRecTrainer(A.DictConfig(learner='adam', learning_rate=1e-3), model)
    torch.manual_seed(5)
    if graph:
        trainer.enable_graph(batch, warmup=1)  # (>= 1: Adam's state must exist before the capture)
    else:
        trainer._seed_t = torch.zeros(1, dtype=torch.int64, device=DEV)
        trainer.state.seed_tensor = trainer._seed_t
        trainer.train_step(batch)
    for _ in range(steps):
        att, cal = (t.detach().clone() for t in trainer.train_step(batch))
    torch.cuda.synchronize()
    return att, cal, {k: v.detach().clone() for k, v in model.state_dict().items()}


def test_trainer_step_eager_and_captured_give_the_same_losses_and_parameters():
    """AttackSASRecTrainer.train_step at L = 224: captured (enable_graph) against eager, the same losses and the same updated
    parameters within 1e-6 max(1, max|x|) -- the bound and the form of
    tests/test_hip_ce_pair.py::test_trainer_step_eager_graph_and_one_walk_with_the_paired_forward.  Same kernels, inputs and
    seeds on both sides; what may differ is the arrival order of float atomics (parameter partials, d_table)."""
    att_e, cal_e, st_e = _train(graph=False)
    att_g, cal_g, st_g = _train(graph=True)
    print(f"eager {att_e.item()!r} {cal_e.item()!r}   graph {att_g.item()!r} {cal_g.item()!r}")
    for a, b in ((att_g, att_e), (cal_g, cal_e)):
        assert torch.isfinite(a) and abs(a.item() - b.item()) <= 1e-6 * max(1.0, abs(b.item())), (a.item(), b.item())
    moved = 0.0
    first = _sasrec(hidden_dropout_prob=0.1, attn_dropout_prob=0.5).state_dict()
    for k in st_e:
        diff = (st_e[k] - st_g[k]).abs().max().item()
        if diff > 0:
            print(f"{k}: max|eager - graph| = {diff:.3e}")
        assert torch.isfinite(st_g[k]).all() and diff <= 1e-6 * max(1.0, st_e[k].abs().max().item()), k
        moved = max(moved, (st_e[k] - first[k]).abs().max().item())
    assert moved >= 1e-3  # (two Adam steps at 1e-3: the parameters that are compared did move)


def test_trainer_step_is_the_same_eager_and_from_a_captured_graph():
    """As tests/test_hip_model_surface.py::test_train_epoch_sums_are_the_same_with_and_without_a_graph: frozen weights and no
    dropout leave the attack noise as the only randomness, which enters the attacked loss alone."""
    batch = {k: v.to(DEV) for k, v in _batch(B=8, seed=3).items()}
    losses, states = [], []
    for graph in (False, True):
        model = _sasrec(hidden_dropout_prob=0.0, attn_dropout_prob=0.0).train()
        trainer = A.AttackSASRecTrainer(A.DictConfig(learner='sgd', learning_rate=1e-30), model)
        if graph:
            trainer.enable_graph(batch, warmup=1)  # (one eager step: Adam-free here, but the capture needs the buffers)
        else:
            trainer.train_step(batch)
        att, cal = trainer.train_step(batch)
        torch.cuda.synchronize()
        losses.append((float(att.detach()), float(cal.detach())))
        states.append({k: v.detach().clone() for k, v in model.state_dict().items()})
    assert all(math.isfinite(v) for pair in losses for v in pair)
    assert abs(losses[0][1] - losses[1][1]) <= 1e-4 * abs(losses[0][1])  # calibrated loss: deterministic
    assert abs(losses[0][0] - losses[1][0]) <= 0.05 * abs(losses[0][0])  # attacked losses differ by their noise draws only
    for k in states[0]:  # two steps of 1e-30 * gradient each way: nothing above one such step apart
        assert (states[0][k] - states[1][k]).abs().max().item() <= 1e-29, k


def test_acbert4rec_trains_and_its_encoder_matches_the_oracle():
    torch.manual_seed(0)
    conf = dict(CFGD, mask_ratio=0.2, use_position_embedding=False, hidden_dropout_prob=0.0, attn_dropout_prob=0.0)
    model = A.AcBERT4Rec(A.DictConfig(conf), A.ItemCount(N_ITEMS)).to(DEV)
    batch = _batch()
    ids = batch["item_id_list"].to(DEV)
    model.train()
    torch.manual_seed(4)
    import random
    random.seed(4)
    model.zero_grad()
    att, cal = model.calculate_loss({"item_id_list": ids})
    assert torch.isfinite(att) and torch.isfinite(cal)
    _two_pass(model, att, cal)
    for n, p in model.named_parameters():
        if n in ("mask_loss_weight",):
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        if n.endswith("weight"):
            assert p.grad.abs().max() > 0, n
    # the encoder's calibrated output at every position (it does not depend on the attack noise)
    model.eval()
    with torch.no_grad():
        _, cal_out, _ = model.forward(ids)
        P = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        cfg = _mcfg(bidirectional=True, hidden_dropout_prob=0.0, attn_dropout_prob=0.0)
        B = ids.shape[0]
        rnds = [O.LayerRandomness(noise=torch.zeros(B, 2, L_MODEL, L_MODEL)) for _ in range(2)]
        _, want, _ = O.bert_forward(batch["item_id_list"], P, cfg, False, rnds, materialize=False)
    assert cal_out.shape == want.shape and (cal_out.cpu() - want).abs().max().item() <= 1e-4


def test_meta_functions_report_the_shapes_the_launches_return_at_long_sequences():
    """torch.ops.acattn.calibrated_attention_fwd / _bwd on meta tensors at L = 257 with one read position per sequence,
    against the shapes the HIP implementation returns: above 208 keys there is no one-row form, so the gate gradient is the
    per-head [B, nh, L, L] (dispatch._bwd_meta's hand-written rule)."""
    from ac_tsr_amd import dispatch  # noqa: F401  (registers torch.ops.acattn.*)
    c = F._case("meta", "train", (2, 257, 64, 2))
    pr = F.problem(c)
    x = {k: v.to(DEV) for k, v in pr.t.items()}
    B, L, H, nh = c.B, c.L, c.H, c.nh
    flat = lambda t: t.reshape(-1).contiguous()
    fwd_args = [x["q"], x["k"], x["v"], x["qa"], x["ka"], x["gl"], pr.kv.to(DEV), True, flat(x["w_order"]), x["b_order"],
                flat(x["w_dist"]), x["b_dist"], x["scalar"], nh, 0.5, SEED, None, False, None, True, True]
    meta = lambda args: [a.to("meta") if isinstance(a, torch.Tensor) else a for a in args]
    real = torch.ops.acattn.calibrated_attention_fwd(*fwd_args)
    fake = torch.ops.acattn.calibrated_attention_fwd(*meta(fwd_args))
    assert [tuple(t.shape) for t in fake] == [tuple(t.shape) for t in real]
    assert tuple(real[2].shape) == (B, nh, L, L) and tuple(real[4].shape) == (B, nh, (L + 15) // 16)
    d_cal = torch.zeros(B, L, H, device=DEV)
    rows = pr.rows.to(DEV)
    d_cal.scatter_(1, rows.unsqueeze(-1).expand(-1, -1, H), torch.randn(B, 1, H, device=DEV))
    bwd_args = fwd_args[:18] + [real[2], real[3], None, d_cal, None, rows, None, False, None]
    real_b = torch.ops.acattn.calibrated_attention_bwd(*bwd_args)
    fake_b = torch.ops.acattn.calibrated_attention_bwd(*meta(bwd_args))
    assert [tuple(t.shape) for t in fake_b] == [tuple(t.shape) for t in real_b]
    assert tuple(real_b[5].shape) == (B, nh, L, L) and all(torch.isfinite(t).all() for t in real_b)
    assert not attn_launch.gate_summed_rule(B, L, H, nh, 1, False, False, False)
    assert attn_launch.gate_summed_rule(B, 208, H, nh, 1, False, False, False)
