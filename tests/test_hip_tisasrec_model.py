"""GPU suite (-m gpu): the ACTiSASRec model (ac_tsr_amd.model.ACTiSASRec over the time-interval attention core) against
tensors the genuine reference produced (tests/golden/tisasrec_*.partNN.npz, tools/gen_tisasrec_golden.py), and its eager
training step.  In every test here the other attention kernels are unreachable: a model that ran them would load the same
checkpoint and compute something else."""
import types

import pytest
import torch

import ac_tsr_amd as A
from ac_tsr_amd import attn_launch, ops
from tests._tisasrec_golden import KEEPS, TisasrecCase

pytestmark = pytest.mark.gpu
DEV = "cuda"
PADDED = ("absolute_pos_K_embedding.weight", "absolute_pos_V_embedding.weight", "time_matrix_emb_K_embedding.weight",
          "time_matrix_emb_V_embedding.weight")


@pytest.fixture(autouse=True)
def no_other_attention_kernels(monkeypatch):
    def unreachable(*args, **kwargs):
        raise AssertionError("another attention kernel was asked for by ACTiSASRec")

    for name in ("attention_fwd_launch", "attention_bwd_launch", "unnorm_attention_fwd_launch", "unnorm_attention_bwd_launch"):
        monkeypatch.setattr(attn_launch, name, unreachable)
    monkeypatch.setattr(ops._CalibratedAttention, "apply", unreachable)
    monkeypatch.setattr(ops._UnnormalisedAttention, "apply", unreachable)


def _model(c):
    model = A.ACTiSASRec(A.DictConfig(c.config()), A.ItemCount(c.n_items)).to(DEV)
    model.load_state_dict({k: v.to(DEV) for k, v in c.params().items()}, strict=True)  # the reference's keys, all of them
    return model


def _rnds(c, noise_key="noise"):
    out = []
    for r in c.layer_randomness(noise_key):
        ns = types.SimpleNamespace(noise=r.noise.to(DEV))
        for f in KEEPS:
            t = getattr(r, f)
            setattr(ns, f, None if t is None else t.to(torch.uint8).to(DEV))
        out.append(ns)
    return out


def test_full_sort_scores_of_both_branches():
    c = TisasrecCase("tisasrec_eval")
    model = _model(c).eval()
    batch = {k: v.to(DEV) for k, v in c.batch().items()}
    with torch.no_grad():
        att, cal = model.full_sort_predict(batch, _rnds=_rnds(c, "score_noise"))
    for got, key in ((att, "out.attacked_scores"), (cal, "out.scores")):
        ref = c.t(key)
        err = (got.cpu() - ref).abs().max().item()
        print(f"tisasrec_eval {key} err={err:.3e} max={ref.abs().max().item():.3e}")
        assert err <= 1e-4 * max(1.0, ref.abs().max().item()), key


@pytest.mark.parametrize("prune", [True, False], ids=["pruned_schedule", "reference_schedule"])
def test_two_pass_losses_and_gradients(prune):
    c = TisasrecCase("tisasrec_train")
    model = _model(c)
    model.step_state.prune_dead_work = prune
    model.train(c.train)
    batch = {k: v.to(DEV) for k, v in c.batch().items()}
    mr = c.model_randomness()
    dev = lambda t: t.to(torch.uint8).to(DEV)
    model.zero_grad()
    att, cal = model.calculate_loss(batch, _rnds=_rnds(c), _keep_emb=dev(mr.keep_emb), _keep_pos=(dev(mr.keep_pos_k), dev(mr.keep_pos_v)),
                                    _keep_time=(dev(mr.keep_time_k), dev(mr.keep_time_v)))
    for got, key in ((att, "out.att_loss"), (cal, "out.cal_loss")):
        ref = float(c.raw[key])
        print(f"tisasrec_train {key} got={got.item():.6f} ref={ref:.6f}")
        assert abs(got.item() - ref) <= 1e-4 * max(1.0, abs(ref)), key
    for n, p in model.named_parameters():
        p.requires_grad = not A.is_attack_param(n)
    cal.backward(retain_graph=True)
    for n, p in model.named_parameters():
        p.requires_grad = A.is_attack_param(n)
    att.backward()
    for n, p in model.named_parameters():
        p.requires_grad = True
    ref = c.grads()
    for n, p in model.named_parameters():
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        err = (g.cpu() - ref[n]).abs().max().item()
        print(f"tisasrec_train grad {n} err={err:.3e} max={ref[n].abs().max().item():.3e}")
        assert err <= 2e-3 * ref[n].abs().max().item() + 2e-8, (n, err, ref[n].abs().max().item())
    for n in PADDED:  # nn.Embedding(padding_idx=0): the rows the forward reads and the training never moves
        g = dict(model.named_parameters())[n].grad
        assert g[0].abs().max().item() == 0 and g[1:].abs().max().item() > 0, n


def _toy(n_items=300, B=32, L=50, drop=0.5, seed=5, span=256):
    torch.manual_seed(seed)
    cfg = dict(n_layers=2, n_heads=2, hidden_size=64, inner_size=256, hidden_dropout_prob=drop, attn_dropout_prob=drop,
               hidden_act="gelu", layer_norm_eps=1e-12, initializer_range=0.02, loss_type="CE", combine_option="gate",
               two_level=True, use_order=True, use_distance=True, mask_loss_weight=0.03, time_span=span, TIME_FIELD="timestamp")
    model = A.ACTiSASRec(A.DictConfig(cfg), A.ItemCount(n_items)).to(DEV)
    g = torch.Generator().manual_seed(seed + 1)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    live = torch.arange(L)[None] < lens[:, None]
    ids = torch.randint(1, n_items, (B, L), generator=g) * live
    stamps = (1000 + torch.randint(0, span // 2, (B, L), generator=g).cumsum(1)) * live
    batch = {"item_id_list": ids, "item_length": lens, "item_id": ids[torch.arange(B), lens - 1], "timestamp_list": stamps}
    return model, {k: v.to(DEV) for k, v in batch.items()}


def test_training_step_eager():
    model, batch = _toy()
    trainer = A.AttackSASRecTrainer(A.DictConfig(learner="adam", learning_rate=1e-3), model)
    model.train()
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    first = None
    for _ in range(10):
        att, cal = trainer.train_step(batch)
        assert torch.isfinite(att) and torch.isfinite(cal)
        first = cal.item() if first is None else first
    assert cal.item() < first  # (the toy target is the sequence's last item: ten steps already lower the loss)
    for n, p in model.named_parameters():  # every parameter moves ...
        assert not torch.equal(p, before[n]), n
    for n in PADDED:  # ... the four time / position tables included, their rows 0 excluded
        p = dict(model.named_parameters())[n]
        assert torch.equal(p[0], before[n][0]), n
        used = slice(1, 50) if "absolute_pos" in n else slice(1, None)
        assert (p[used] != before[n][used]).any(dim=1).float().mean() > 0.5, n


def test_the_calibrated_loss_follows_the_timestamps():
    """No dropout: the calibrated loss is a function of the batch alone, so it must follow the time stamps and come back, to
    the bit, when they do."""
    model, batch = _toy(drop=0.0)
    model.train()
    other = dict(batch)
    other["timestamp_list"] = batch["timestamp_list"] * 3
    with torch.no_grad():
        (_, first), (_, second), (_, third) = (model.calculate_loss(b) for b in (batch, other, batch))
    assert first.item() == third.item()
    assert abs(first.item() - second.item()) > 1e-6 * abs(first.item())


def test_graph_capture_and_the_one_walk_backward_are_refused():
    model, batch = _toy()
    trainer = A.AttackSASRecTrainer(A.DictConfig(learner="adam"), model)
    with pytest.raises(ValueError, match="ACTiSASRec.*eagerly only"):
        trainer.enable_graph(batch, warmup=1)
    with pytest.raises(ValueError, match="combined_backward.*ACTiSASRec"):
        A.AttackSASRecTrainer(A.DictConfig(learner="adam"), model, combined_backward=True)


def test_the_layer_refuses_what_the_core_does_not_have():
    B, L, H = 2, 50, 64
    x = torch.randn(B, L, H, device=DEV)
    mask = A.StructuredMask(torch.ones(B, L, dtype=torch.uint8, device=DEV))
    index = torch.zeros(B, L, L, dtype=torch.int32, device=DEV)
    table = torch.randn(9, H, device=DEV)
    args = lambda n=L, idx=index: (torch.randn(B, n, H, device=DEV), torch.randn(B, n, H, device=DEV),
                                   A.TimeIntervals(table, idx), A.TimeIntervals(table, idx))
    layer = lambda **kw: A.ACTimeAwareTransformerLayer(2, H, 256, 0.5, 0.5, "gelu", 1e-12, **kw).to(DEV).eval()
    with pytest.raises(ValueError, match="gate"):
        layer()(x, mask, *args())  # the reference's default combine_option, 'fixed'
    with pytest.raises(ValueError, match="two_level"):
        layer(combine_option="gate", two_level=False)(x, mask, *args())
    with pytest.raises(ValueError, match="probability dumps"):
        layer(combine_option="gate")(x, mask, *args(), return_attention_prob=True)
    long = layer(combine_option="gate", seq_length=65)
    with pytest.raises(ValueError, match="L <= 64"):
        long(torch.randn(B, 65, H, device=DEV), A.StructuredMask(torch.ones(B, 65, dtype=torch.uint8, device=DEV)),
             *args(65, torch.zeros(B, 65, 65, dtype=torch.int32, device=DEV)))
    att, cal, M = layer(combine_option="gate")(x, mask, *args())  # and what it has, it runs
    assert att.shape == cal.shape == (B, L, H) and M.shape == (B, 2, L, L) and torch.isfinite(cal).all()
