#!/usr/bin/env python3
"""Generate the fixtures `tisasrec_train` and `tisasrec_eval` under tests/golden/ by RUNNING THE GENUINE REFERENCE's ACTiSASRec
(recbole/model/sequential_recommender/actisasrec.py over recbole/model/transformer_layers.py:1010-1422) on the CPU: in training
mode through the two-pass protocol of oracle/gen_golden.py (recbole/trainer/trainer.py:662-686), in eval mode through
full_sort_predict (and the two-pass protocol as well).

While generating, the randomness is drawn again in the reference's order -- input dropout, posK, posV, timeK, timeV
(actisasrec.py:119-124), then the layers' (oracle.ac_tsr_ref.draw_layer_randomness) -- and the CPU restatement
tests/_timeaware_ref.py evaluated on it; the run ABORTS unless restatement and reference agree within gen_golden's own limits:
2e-5 on losses and scores, 2e-3 of a gradient's maximum on every gradient.

TEST INFRASTRUCTURE ONLY; copies nothing from the reference, only tensors are written, in parts under 1 MiB
(tools/gen_shipped_golden.py: write_parts; tests put them together again).  Keep masks are packed with np.packbits.

Usage:  ACTSR_REFERENCE=<checkout of the reference> python tools/gen_tisasrec_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {
    # the shipped shape: hidden 64, 2 heads, L = 50, time_span 256, gate, two-level
    "tisasrec_train": dict(B=4, L=50, H=64, h=2, inner=256, n_layers=2, n_items=400, span=256, sigma=0.05, seed=41, train=True),
    "tisasrec_eval": dict(B=4, L=50, H=32, h=2, inner=128, n_layers=2, n_items=400, span=16, sigma=0.05, seed=42, train=False),
}
LAYER_KEEPS = ("keep_after", "keep_before", "keep_mask", "keep_out_att", "keep_out_cal", "keep_ffn_att", "keep_ffn_cal")
MODEL_KEEPS = ("keep_emb", "keep_pos_k", "keep_pos_v", "keep_time_k", "keep_time_v")


def make_stamps(B, L, lens, span, gen):
    """Right-padded time stamps (0 at padded positions, as RecBole pads): runs of equal stamps (index 0 off the diagonal),
    gaps well inside time_span and gaps past it (clipped)."""
    stamps = torch.zeros(B, L, dtype=torch.long)
    for b, n in enumerate(lens):
        kind = torch.randint(0, 3, (n,), generator=gen)
        small = torch.randint(1, max(2, span // 8), (n,), generator=gen)
        gaps = torch.where(kind == 0, torch.zeros_like(small), torch.where(kind == 1, small, torch.full_like(small, 2 * span)))
        stamps[b, :n] = 1000 + gaps.cumsum(0)
    return stamps


def pack(t):
    return np.packbits(t.to(torch.uint8).numpy().reshape(-1))


def tisasrec_case(G, O, T, RefModel, name, *, B, L, H, h, inner, n_layers, n_items, span, sigma, seed, train,
                  mask_loss_weight=0.03):
    print(f"[tisasrec] {name} train={train}")
    gen = torch.Generator().manual_seed(seed)
    cfg = G.Cfg(n_layers=n_layers, n_heads=h, hidden_size=H, inner_size=inner, hidden_dropout_prob=0.5, attn_dropout_prob=0.5,
                hidden_act="gelu", layer_norm_eps=1e-12, initializer_range=0.02, loss_type="CE", combine_option="gate",
                rich_calibrated_combine="none", two_level=True, use_position_embedding=False, use_order=True,
                use_distance=True, trainable_mask_loss_weight=True, mask_loss_weight=mask_loss_weight, time_span=span,
                TIME_FIELD="timestamp", USER_ID_FIELD="user_id", ITEM_ID_FIELD="item_id", LIST_SUFFIX="_list",
                ITEM_LIST_LENGTH_FIELD="item_length", NEG_PREFIX="neg_", MAX_ITEM_LIST_LENGTH=L, device="cpu")
    torch.manual_seed(seed)
    model = RefModel(cfg, G.FakeDataset(n_items))
    G.reinit(model, sigma, gen)  # (row 0 of the five padded tables included, as the reference's own _init_weights does)
    lens = [int(v) for v in torch.randint(2, L + 1, (B,), generator=gen)]
    lens[0], lens[1] = 1, L
    item_seq = G.make_item_seq(B, L, n_items, lens, gen)
    stamps = make_stamps(B, L, lens, span, gen)
    batch = {"item_id_list": item_seq, "item_length": torch.tensor(lens, dtype=torch.long),
             "item_id": torch.randint(1, n_items, (B,), generator=gen), "timestamp_list": stamps}
    tm = T.get_time_matrix(stamps, span)
    assert torch.equal(tm, model.get_time_matrix(stamps))
    off = ~torch.eye(L, dtype=torch.bool).expand_as(tm)
    assert (tm[off] == 0).any() and (tm == span).any() and 0 < int(((tm > 0) & (tm < span)).sum())
    ecfg = O.EncoderCfg(n_layers=n_layers, n_heads=h, hidden_size=H, inner_size=inner, combine_option="gate",
                        rich_calibrated_combine="none", seq_length=50)
    mcfg = O.ModelCfg(enc=ecfg, n_items=n_items, max_seq_length=L, mask_loss_weight=mask_loss_weight,
                      trainable_mask_loss_weight=True)
    P = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.train(train)
    arr = {"in.item_id_list": item_seq, "in.item_length": batch["item_length"], "in.item_id": batch["item_id"],
           "in.timestamp_list": stamps, "meta.cfg": np.array([n_layers, h, H, inner, L, n_items, span, B]), "meta.combine": "gate",
           "meta.train": int(train), "meta.mask_loss_weight": mask_loss_weight}
    for k, v in P.items():
        arr["p." + k] = v
    shapes = ((B, h, L, L), (B, L, H))

    def draw_model_randomness():
        if not train:
            return T.ModelRandomness()
        bern = lambda *shape: torch.empty(*shape).bernoulli_(0.5)
        return T.ModelRandomness(keep_emb=bern(B, L, H), keep_pos_k=bern(B, L, H), keep_pos_v=bern(B, L, H),
                                 keep_time_k=bern(B, L, L, H), keep_time_v=bern(B, L, L, H))

    if not train:  # full-sort scores of both branches (actisasrec.py:212-224)
        torch.manual_seed(seed + 7)
        with torch.no_grad():
            att_scores, scores = model.full_sort_predict(batch)
        torch.manual_seed(seed + 7)
        rnds = [O.draw_layer_randomness(*shapes, ecfg, False) for _ in range(n_layers)]
        with torch.no_grad():
            o_att, o_cal = T.full_sort_predict(batch, P, mcfg, span, rnds)
        print(f"  scores: max abs diff {G.check(name + '.attacked_scores', o_att, att_scores, 2e-5):.3g}, "
              f"{G.check(name + '.scores', o_cal, scores, 2e-5):.3g}")
        arr["out.attacked_scores"], arr["out.scores"] = att_scores, scores
        for i, r in enumerate(rnds):
            arr[f"in.score_noise.{i}"] = r.noise

    # the two-pass trainer protocol (recbole/trainer/trainer.py:662-686), as oracle/gen_golden.py runs it
    model.zero_grad()
    torch.manual_seed(seed + 11)
    att_loss, cal_loss = model.calculate_loss(batch)
    for n, prm in model.named_parameters():
        prm.requires_grad = not O.is_attack_param(n)
    cal_loss.backward(retain_graph=True)
    for n, prm in model.named_parameters():
        prm.requires_grad = O.is_attack_param(n)
    att_loss.backward()
    for n, prm in model.named_parameters():
        prm.requires_grad = True
    ref_grads = {n: (prm.grad.detach().clone() if prm.grad is not None else torch.zeros_like(prm))
                 for n, prm in model.named_parameters()}
    # the same draws again, in the reference's order
    torch.manual_seed(seed + 11)
    mr = draw_model_randomness()
    rnds = [O.draw_layer_randomness(*shapes, ecfg, train) for _ in range(n_layers)]
    o_att, o_cal, o_grads = T.two_pass_grads(batch, P, mcfg, span, rnds, mr)
    print(f"  losses: ref ({att_loss.item():.6f}, {cal_loss.item():.6f})  restated ({o_att.item():.6f}, {o_cal.item():.6f})")
    G.check(name + ".att_loss", o_att, att_loss.detach(), 2e-5)
    G.check(name + ".cal_loss", o_cal, cal_loss.detach(), 2e-5)
    worst = 0.0
    for n, g in ref_grads.items():
        scale = max(g.abs().max().item(), 1e-6)
        worst = max(worst, G.check(name + ".grad." + n, o_grads[n] / scale, g / scale, 2e-3))
    print(f"  grads: worst relative-to-max diff {worst:.3g}")
    for n in T.PADDED_TABLES:  # nn.Embedding(padding_idx=0)
        assert ref_grads[n][0].abs().max() == 0, n
    arr["out.att_loss"], arr["out.cal_loss"] = att_loss.detach(), cal_loss.detach()
    for n, g in ref_grads.items():
        arr["grad." + n] = g
    if train:
        for f in MODEL_KEEPS:
            arr["bits." + f] = pack(getattr(mr, f))
    for i, r in enumerate(rnds):
        arr[f"in.noise.{i}"] = r.noise
        if train:
            for f in LAYER_KEEPS:
                arr[f"bits.{f}.{i}"] = pack(getattr(r, f))
    return {k: (v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arr.items()}


def main():
    ref = os.environ.get("ACTSR_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
    if not ref or not os.path.isdir(os.path.join(ref, "recbole")):
        raise SystemExit("usage: ACTSR_REFERENCE=<checkout of the reference> python tools/gen_tisasrec_golden.py  (or pass the path)")
    os.environ["ACTSR_REFERENCE"] = ref
    from oracle import gen_golden as G  # imports the reference behind its logging stand-ins
    from oracle import ac_tsr_ref as O
    from recbole.model.sequential_recommender.actisasrec import ACTiSASRec as RefModel  # the reference
    from tests import _timeaware_ref as T
    from tools.gen_shipped_golden import write_parts
    for name, args in CASES.items():
        write_parts(name, tisasrec_case(G, O, T, RefModel, name, **args))


if __name__ == "__main__":
    main()
