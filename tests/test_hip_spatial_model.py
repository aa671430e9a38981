"""GPU suite (-m gpu): the modules, the model and the trainer WITHOUT the adversarial calibrator
(AttackRTransformerLayer / AttackRTransformerEncoder(adversarial=False), ACSASRec(adversarial_calibrator=False)).

(i)   a 2-layer spatial-only encoder, eval and train mode with explicit keeps, against the oracle composed here from
      O.origin_qkv -> O.adjusted_outputs(after_spatial, x, value) -> O.feed_forward (float32): outputs <= 1e-4, input
      and parameter gradients of sum(out * G) <= 2e-3 * max|g| + 2e-8; attack transforms and gate have no gradient;
(ii)  one layer against tensors the GENUINE reference produced (tests/golden/spatial_layer.npz, tools/gen_spatial_golden.py);
(iii) ACSASRec(adversarial_calibrator=False) at 100k items, B = 512, L = 50: losses, training, untouched attack
      transforms / gate, graph replay, full-sort logits against the oracle, predict, loading a reference checkpoint.
"""
import os
import types

import numpy as np
import pytest
import torch

import ac_tsr_amd as A
from ac_tsr_amd.layers import AttackRTransformerEncoder, AttackRTransformerLayer
from oracle import ac_tsr_ref as O
from tests._golden import GOLDEN_DIR, Case

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _unused(name):
    return A.is_attack_param(name) or ".gate." in name or name.startswith("gate.")


def _item_seq(B, L, gen, left_pad_row=None, n_items=1000):
    lens = torch.randint(1, L + 1, (B,), generator=gen)
    lens[0] = L
    seq = torch.zeros(B, L, dtype=torch.long)
    for b in range(B):
        n = int(lens[b])
        ids = torch.randint(1, n_items, (n,), generator=gen)
        if b == left_pad_row:
            seq[b, L - n:] = ids
        else:
            seq[b, :n] = ids
    return seq, lens


def _oracle_spatial_encoder(x, mask, P, cfg, rnds):
    """The reference's own three calls per layer with the spatial-only probabilities (layers.py:686-742, 676-684, 790-798)."""
    hidden = x
    for i in range(cfg.n_layers):
        p = O.layer_params(P, f"layer.{i}.")
        r = rnds[i] if rnds is not None else O.LayerRandomness()
        _, _, v, after_spatial, _ = O.origin_qkv(hidden, mask, p, cfg, keep_after=r.keep_after, keep_before=None, materialize=False)
        a = O.adjusted_outputs(after_spatial, hidden, v, p, cfg, keep=r.keep_out_cal)
        hidden = O.feed_forward(a, p, cfg, keep=r.keep_ffn_cal)
    return hidden


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train_explicit_keeps"])
def test_spatial_only_encoder_matches_the_oracle(train):
    B, L, H, nh, inner, n_layers = 8, 50, 64, 2, 256, 2
    gen = torch.Generator().manual_seed(77)
    torch.manual_seed(77)
    enc = AttackRTransformerEncoder(n_layers=n_layers, n_heads=nh, hidden_size=H, inner_size=inner, hidden_dropout_prob=0.5,
                                    attn_dropout_prob=0.5, combine_option='gate', seq_length=L, adversarial=False)
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if n.endswith("LayerNorm.weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=gen))
            elif "affine" in n or n.endswith("scalar"):
                p.copy_(0.3 * torch.randn(p.shape, generator=gen))
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=gen))
    P = {n: p.detach().clone().requires_grad_(True) for n, p in enc.named_parameters()}
    enc = enc.to(DEV).train(train)
    seq, lens = _item_seq(B, L, gen, left_pad_row=1)
    mask = O.attention_mask(seq, bidirectional=False)
    x = torch.randn(B, L, H, generator=gen)
    G = torch.randn(B, L, H, generator=gen)
    cfg = O.EncoderCfg(n_layers=n_layers, n_heads=nh, hidden_size=H, inner_size=inner, combine_option="gate", seq_length=L)
    rnds_cpu = rnds_dev = None
    if train:
        bern = lambda *s: torch.empty(*s).bernoulli_(0.5, generator=gen)
        rnds_cpu = [O.LayerRandomness(keep_after=bern(B, nh, L, L), keep_out_cal=bern(B, L, H), keep_ffn_cal=bern(B, L, H))
                    for _ in range(n_layers)]
        rnds_dev = [types.SimpleNamespace(noise=None, keep_after=r.keep_after.to(torch.uint8).to(DEV),
                                          keep_out_cal=r.keep_out_cal.to(torch.uint8).to(DEV),
                                          keep_ffn_cal=r.keep_ffn_cal.to(torch.uint8).to(DEV)) for r in rnds_cpu]
    x_ref = x.clone().requires_grad_(True)
    ref = _oracle_spatial_encoder(x_ref, mask, P, cfg, rnds_cpu)
    used = [n for n in P if not _unused(n)]
    ref_grads = torch.autograd.grad((ref * G).sum(), [x_ref] + [P[n] for n in used])

    for mask_dev in (A.StructuredMask((seq != 0).to(torch.uint8).to(DEV), causal=True), mask.to(DEV)):
        enc.zero_grad()
        x_dev = x.to(DEV).requires_grad_(True)
        layers_out, all_masks = enc(x_dev, mask_dev, output_all_encoded_layers=True, _rnds=rnds_dev)
        assert all_masks == [None] * n_layers
        assert all(att is None for att, _ in layers_out)
        out = layers_out[-1][1]
        assert (out.detach().cpu() - ref.detach()).abs().max().item() <= 1e-4
        (out * G.to(DEV)).sum().backward()
        got = {"x": x_dev.grad.cpu()}
        got.update({n: p.grad.cpu() for n, p in enc.named_parameters() if p.grad is not None})
        for n, g in zip(["x"] + used, ref_grads):
            err = (got[n] - g).abs().max().item()
            assert err <= 2e-3 * g.abs().max().item() + 2e-8, (n, err, g.abs().max().item())
        for n, p in enc.named_parameters():
            assert (p.grad is None) == _unused(n), n


def test_spatial_only_layer_matches_the_genuine_reference():
    z = np.load(os.path.join(GOLDEN_DIR, "spatial_layer.npz"), allow_pickle=False)
    t = lambda k: torch.from_numpy(z[k])
    B, L, H = z["x"].shape
    layer = AttackRTransformerLayer(2, H, 256, 0.5, 0.5, 'gelu', 1e-12, 'gate', True, True, True, 'fixed', L, adversarial=False)
    layer.load_state_dict({k[len("param."):]: t(k) for k in z.files if k.startswith("param.")}, strict=True)
    layer = layer.to(DEV).eval()
    item_seq = t("item_seq")
    assert (item_seq[2, 0] == 0) and (item_seq[2, -1] != 0)  # the left-padded sequence
    for mask_dev in (A.StructuredMask((item_seq != 0).to(torch.uint8).to(DEV), causal=True),
                     O.attention_mask(item_seq, bidirectional=False).to(DEV)):
        layer.zero_grad()
        x = t("x").to(DEV).requires_grad_(True)
        att, out, M, prob = layer(x, mask_dev)
        assert att is None and M is None and prob is None
        assert (out.detach().cpu() - t("out")).abs().max().item() <= 1e-4
        (out * t("G").to(DEV)).sum().backward()
        got = {"x": x.grad.cpu()}
        got.update({n: p.grad.cpu() for n, p in layer.named_parameters() if p.grad is not None})
        ref = {k[len("grad."):]: t(k) for k in z.files if k.startswith("grad.")}
        assert set(got) == set(ref)  # the attack transforms and the gate take no part on either side
        for n, g in ref.items():
            err = (got[n] - g).abs().max().item()
            assert err <= 2e-3 * g.abs().max().item() + 2e-8, (n, err, g.abs().max().item())


CFG = dict(n_layers=2, n_heads=2, hidden_size=64, inner_size=256, hidden_dropout_prob=0.5, attn_dropout_prob=0.5,
           hidden_act='gelu', layer_norm_eps=1e-12, initializer_range=0.02, loss_type='CE', combine_option='gate',
           two_level=True, use_order=True, use_distance=True, mask_loss_weight=0.03, adversarial_calibrator=False)


def _model(N, **over):
    torch.manual_seed(0)
    return A.ACSASRec(A.DictConfig(dict(CFG, **over)), A.ItemCount(N)).to(DEV)


def _batch(B, L, N, seed=1):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    ids = torch.randint(1, N, (B, L), generator=g) * (torch.arange(L)[None] < lens[:, None])
    target = ids[torch.arange(B), lens - 1]  # learnable toy target: the last item of the sequence
    return {"item_id_list": ids.to(DEV), "item_length": lens.to(DEV), "item_id": target.to(DEV)}


def test_spatial_only_model_trains_and_leaves_the_unused_parameters_alone():
    N, B, L = 100_000, 512, 50
    model = _model(N).train()
    batch = _batch(B, L, N)
    att, cal = model.calculate_loss(batch)
    assert att is None and torch.isfinite(cal)
    a_out, c_out, masks = model.forward(batch["item_id_list"], batch["item_length"])
    assert a_out is None and c_out.shape == (B, 64) and masks == [None, None]
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    trainer = A.AttackSASRecTrainer(A.DictConfig(learner='adam', learning_rate=1e-3), model)
    first = last = None
    for _ in range(30):
        att, cal = trainer.train_step(batch)
        assert att is None and torch.isfinite(cal)
        first = cal.item() if first is None else first
        last = cal.item()
    assert last < first, (first, last)
    for n, p in model.named_parameters():
        if _unused(n):
            assert p.grad is None and torch.equal(p.detach(), before[n]), n  # bit for bit
        else:
            assert not torch.equal(p.detach(), before[n]), f"{n} has not moved"
            assert torch.isfinite(p).all(), n


def test_spatial_only_epoch_sums_are_the_same_with_and_without_a_graph():
    """As tests/test_hip_model_surface.py::test_train_epoch_sums_are_the_same_with_and_without_a_graph demands of the
    calibrated sums; the attacked sum of a model without an attacked loss is 0."""
    N = 700
    batches = [_batch(48, 50, N, seed=s) for s in (1, 2, 3)] + [_batch(20, 50, N, seed=4)]
    sums = []
    for graph in (False, True):
        torch.manual_seed(0)
        model = _model(N, hidden_dropout_prob=0.0, attn_dropout_prob=0.0).train()
        trainer = A.AttackSASRecTrainer(A.DictConfig(learner='sgd', learning_rate=1e-30), model)
        if graph:
            trainer.enable_graph(batches[0], warmup=1)
        sums.append(trainer._train_epoch(batches))
    assert sums[0][0] == 0 and sums[1][0] == 0
    assert abs(sums[0][1] - sums[1][1]) <= 1e-4 * abs(sums[0][1])
    assert 5.0 < sums[0][1] / len(batches) < 8.0


def test_spatial_only_graph_training_learns():
    N, B, L = 5000, 512, 50
    model = _model(N).train()
    batch = _batch(B, L, N)
    trainer = A.AttackSASRecTrainer(A.DictConfig(learner='adam', learning_rate=1e-3), model)
    trainer.enable_graph(batch, warmup=2)
    first = last = None
    for _ in range(30):
        att, cal = trainer.train_step(batch)
        assert att is None
        first = cal.item() if first is None else first
        last = cal.item()
    assert last < first - 0.5, (first, last)
    for n, p in model.named_parameters():
        assert torch.isfinite(p).all(), n


def test_spatial_only_predictions_match_the_oracle_and_a_reference_checkpoint_loads():
    c = Case("model_eval")
    cfg = c.model_cfg()
    model = A.ACSASRec(A.DictConfig(dict(CFG, n_layers=cfg.enc.n_layers, n_heads=cfg.enc.n_heads, hidden_size=cfg.enc.hidden_size,
                                         inner_size=cfg.enc.inner_size, rich_calibrated_combine='none',
                                         mask_loss_weight=cfg.mask_loss_weight, MAX_ITEM_LIST_LENGTH=cfg.max_seq_length)),
                       A.ItemCount(cfg.n_items))
    P = c.params()
    model.load_state_dict(P, strict=True)  # the reference's own state dict, strict
    model = model.to(DEV).eval()
    batch = c.batch()
    dev_batch = {k: v.to(DEV) for k, v in batch.items()}
    with torch.no_grad():
        none, scores = model.full_sort_predict(dev_batch)
        att_s, s = model.predict(dev_batch)
        # the oracle's spatial-only logits: the model's front end, the three reference calls per layer, the read position
        item_seq, item_len = batch["item_id_list"], batch["item_length"]
        emb = torch.nn.functional.embedding(item_seq, P["item_embedding.weight"])
        if "position_embedding.weight" in P and model.use_position_embedding:
            emb = emb + P["position_embedding.weight"][:item_seq.size(1)].unsqueeze(0)
        emb = torch.nn.functional.layer_norm(emb, (emb.shape[-1],), P["LayerNorm.weight"], P["LayerNorm.bias"], cfg.enc.layer_norm_eps)
        enc_P = {k[len("trm_encoder."):]: v for k, v in P.items() if k.startswith("trm_encoder.")}
        hidden = _oracle_spatial_encoder(emb, O.attention_mask(item_seq), enc_P, cfg.enc, None)
        ref = O.gather_indexes(hidden, item_len - 1) @ P["item_embedding.weight"].t()
    assert none is None and att_s is None
    assert (scores.cpu() - ref).abs().max().item() <= 1e-4
    picked = scores.gather(1, dev_batch["item_id"].view(-1, 1)).squeeze(1)
    assert (s - picked).abs().max().item() <= 1e-5
    # ... and back: the spatial-only model's state dict loads into the adversarial twin
    twin = A.ACSASRec(A.DictConfig(dict(CFG, adversarial_calibrator=True, n_layers=cfg.enc.n_layers, n_heads=cfg.enc.n_heads,
                                        hidden_size=cfg.enc.hidden_size, inner_size=cfg.enc.inner_size,
                                        rich_calibrated_combine='none', MAX_ITEM_LIST_LENGTH=cfg.max_seq_length)),
                      A.ItemCount(cfg.n_items))
    twin.load_state_dict(model.state_dict(), strict=True)


def test_three_projection_launch_equals_the_linear_layers():
    """linear.projections_qkv at hidden 64 (one launch on the split bf16 products) against torch's fp64 linear layers,
    forward and input / parameter gradients; hidden 128 takes the three-call path and must agree as well."""
    from ac_tsr_amd import linear
    for H in (64, 128):
        g = torch.Generator().manual_seed(5)
        q, k, v = (torch.nn.Linear(H, H) for _ in range(3))
        for m in (q, k, v):
            m.to(DEV)
        x = torch.randn(6, 50, H, generator=g).to(DEV).requires_grad_(True)
        G = [torch.randn(6, 50, H, generator=g).to(DEV) for _ in range(3)]
        mq, mk, mv, x_res, extras = linear.projections_qkv(x, q, k, v)
        (sum((o * gg).sum() for o, gg in zip((mq, mk, mv), G)) + x_res.sum()).backward()
        got = [x.grad.clone()] + [p.grad.clone() for m in (q, k, v) for p in (m.weight, m.bias)]
        x64 = x.detach().double().requires_grad_(True)
        ws = []
        outs = []
        for m in (q, k, v):
            w = m.weight.detach().double().requires_grad_(True)
            b = m.bias.detach().double().requires_grad_(True)
            ws += [w, b]
            outs.append(torch.nn.functional.linear(x64, w, b))
        ref = torch.autograd.grad(sum((o * gg.double()).sum() for o, gg in zip(outs, G)) + x64.sum(), [x64] + ws)
        for o, r in zip((mq, mk, mv), outs):
            assert (o.double() - r).abs().max().item() <= 1e-5 * max(1.0, r.abs().max().item())
        for a, r in zip(got, ref):
            assert (a.double() - r).abs().max().item() <= 2e-5 * r.abs().max().item() + 1e-8
