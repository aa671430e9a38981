"""GPU suite (-m gpu): the ACSSEPT model (ac_tsr_amd.model.ACSSEPT over the un-normalised attention core) against tensors
the genuine reference produced (tests/golden/ssept_*.partNN.npz, tools/gen_ssept_golden.py), and its eager training step.  In every test here the normalised attention kernels are unreachable: a model that ran them would
load the same checkpoint and compute something else."""
import types

import pytest
import torch

import ac_tsr_amd as A
from ac_tsr_amd import attn_launch, ops
from tests._ssept_golden import KEEPS, SseptCase

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def no_normalised_kernels(monkeypatch):
    def unreachable(*args, **kwargs):
        raise AssertionError("a normalised attention kernel was asked for by ACSSEPT")

    monkeypatch.setattr(attn_launch, "attention_fwd_launch", unreachable)
    monkeypatch.setattr(attn_launch, "attention_bwd_launch", unreachable)
    monkeypatch.setattr(ops._CalibratedAttention, "apply", unreachable)  # (the torch.ops.acattn.* call site is inside it)


def _model(c):
    model = A.ACSSEPT(A.DictConfig(c.config()), A.Counts(c.n_items, c.n_users)).to(DEV)
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


def test_state_dict_keys_are_the_references():
    c = SseptCase("ssept_train")
    model = _model(c)
    assert set(model.state_dict()) == set(c.params())
    back = A.ACSSEPT(A.DictConfig(c.config()), A.Counts(c.n_items, c.n_users))
    back.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()}, strict=True)
    for k, v in c.params().items():
        assert torch.equal(back.state_dict()[k], v), k


def test_full_sort_scores_of_both_branches():
    c = SseptCase("ssept_eval")
    model = _model(c).eval()
    batch = {k: v.to(DEV) for k, v in c.batch().items()}
    with torch.no_grad():
        att, cal = model.full_sort_predict(batch, _rnds=_rnds(c, "score_noise"))
    for got, key in ((att, "out.attacked_scores"), (cal, "out.scores")):
        ref = c.t(key)
        err = (got.cpu() - ref).abs().max().item()
        print(f"ssept_eval {key} err={err:.3e} max={ref.abs().max().item():.3e}")
        assert err <= 1e-4 * max(1.0, ref.abs().max().item()), key


@pytest.mark.parametrize("prune", [True, False], ids=["pruned_schedule", "reference_schedule"])
def test_two_pass_losses_and_gradients(prune):
    c = SseptCase("ssept_train")
    model = _model(c)
    model.step_state.prune_dead_work = prune
    model.train(c.train)
    batch = {k: v.to(DEV) for k, v in c.batch().items()}
    model.zero_grad()
    att, cal = model.calculate_loss(batch, _rnds=_rnds(c), _keep_emb=c.t("in.keep_emb").to(DEV))
    for got, key in ((att, "out.att_loss"), (cal, "out.cal_loss")):
        ref = float(c.raw[key])
        print(f"ssept_train {key} got={got.item():.6f} ref={ref:.6f}")
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
        assert err <= 2e-3 * ref[n].abs().max().item() + 2e-8, (n, err, ref[n].abs().max().item())
    # the test-time user table takes no part in training; a user who occurs twice collects both sequences' gradients
    g_test = model.user_test_embedding.weight.grad
    assert g_test is None or g_test.abs().max().item() == 0
    users = c.t("in.user_id")
    twice = [int(u) for u in users.unique() if int((users == u).sum()) > 1]
    assert twice
    g_user = model.user_embedding.weight.grad.cpu()
    assert g_user[twice[0]].abs().max() > 0
    assert sorted(int(u) for u in g_user.abs().sum(1).nonzero().view(-1)) == sorted(int(u) for u in users.unique())


def _toy(n_items=300, n_users=50, B=32, L=50, drop=0.5, seed=5):
    torch.manual_seed(seed)
    cfg = dict(n_layers=2, n_heads=2, user_hidden_size=64, item_hidden_size=64, inner_size=256, hidden_dropout_prob=drop,
               attn_dropout_prob=drop, hidden_act="gelu", layer_norm_eps=1e-12, initializer_range=0.02, loss_type="CE",
               combine_option="gate", two_level=True, use_order=True, use_distance=True, mask_loss_weight=0.03)
    model = A.ACSSEPT(A.DictConfig(cfg), A.Counts(n_items, n_users)).to(DEV)
    g = torch.Generator().manual_seed(seed + 1)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    ids = torch.randint(1, n_items, (B, L), generator=g) * (torch.arange(L)[None] < lens[:, None])
    batch = {"item_id_list": ids, "item_length": lens, "item_id": ids[torch.arange(B), lens - 1],
             "user_id": torch.randint(1, n_users, (B,), generator=g)}
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
    moved = [n for n, p in model.named_parameters() if not torch.equal(p, before[n])]
    for n in ("item_embedding.weight", "user_embedding.weight", "trm_encoder.layer.0.attack_attention.attack_query_transform.weight",
              "trm_encoder.layer.1.gate.weight", "trm_encoder.layer.0.attack_attention.scalar"):
        assert n in moved, n
    assert "user_test_embedding.weight" not in moved


def test_the_calibrated_loss_follows_the_user_ids():
    """No dropout: the calibrated loss is a function of the batch alone (the noise reaches the attacked branch only), so it
    must follow user_id and come back, to the bit, when user_id does; the attacked loss draws new noise every time."""
    model, batch = _toy(drop=0.0)
    model.train()
    other = dict(batch)
    other["user_id"] = batch["user_id"].roll(1) % 49 + 1
    assert not torch.equal(other["user_id"], batch["user_id"])
    with torch.no_grad():
        (att1, first), (_, second), (att3, third) = (model.calculate_loss(b) for b in (batch, other, batch))
    assert first.item() == third.item()
    assert abs(first.item() - second.item()) > 1e-6 * abs(first.item())
    assert att1.item() != att3.item()


def test_graph_capture_is_refused_by_name():
    model, batch = _toy()
    trainer = A.AttackSASRecTrainer(A.DictConfig(learner="adam"), model)
    with pytest.raises(ValueError, match="eagerly only"):
        trainer.enable_graph(batch, warmup=1)


def test_the_one_walk_backward_is_refused():
    model, _ = _toy()
    with pytest.raises(ValueError, match="combined_backward"):
        A.AttackSASRecTrainer(A.DictConfig(learner="adam"), model, combined_backward=True)


def test_the_layer_refuses_what_the_core_does_not_have():
    with pytest.raises(ValueError, match="adversarial"):
        A.AttackRTransformerLayer(2, 64, 256, 0.5, 0.5, "gelu", 1e-12, combine_option="gate", adversarial=False, renormalise=False)
    layer = A.AttackRTransformerLayer(2, 64, 256, 0.5, 0.5, "gelu", 1e-12, combine_option="gate", renormalise=False).to(DEV)
    x = torch.randn(2, 50, 64, device=DEV)
    mask = A.StructuredMask(torch.ones(2, 50, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="probability dumps"):
        layer(x, mask, return_attention_prob=True)
