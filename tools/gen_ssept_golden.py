#!/usr/bin/env python3
"""Generate the fixtures `ssept_train` and `ssept_eval` under tests/golden/ by RUNNING THE GENUINE REFERENCE's ACSSEPT
(recbole/model/sequential_recommender/acssept.py over recbole/model/transformer_layers.py) through the two-pass protocol of
oracle/gen_golden.py (recbole/trainer/trainer.py:662-686) and, in eval mode, through full_sort_predict.

While generating, the randomness is drawn again in the reference's order (oracle.ac_tsr_ref.draw_layer_randomness) and the
CPU restatement tests/_unnorm_ref.py evaluated on it; the run ABORTS unless restatement and reference agree within
gen_golden's own limits: 2e-5 on losses and scores, 2e-3 of a gradient's maximum on every gradient.

TEST INFRASTRUCTURE ONLY; copies nothing from the reference, only tensors are written, in parts under 1 MiB
(tools/gen_shipped_golden.py: write_parts; tests put them together again).

Usage:  ACTSR_REFERENCE=<checkout of the reference> python tools/gen_ssept_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {
    # the shipped shape: hidden 64 + 64, 2 heads (head size 64), L = 50, gate, two-level
    "ssept_train": dict(B=6, L=50, Di=64, Du=64, h=2, inner=256, n_layers=2, n_items=400, n_users=40, sigma=0.05, seed=31,
                        train=True),
    "ssept_eval": dict(B=6, L=50, Di=32, Du=32, h=2, inner=128, n_layers=2, n_items=400, n_users=40, sigma=0.05, seed=32,
                       train=False),
}


class Dataset:
    def __init__(self, n_items, n_users):
        self.n_items, self.n_users = n_items, n_users

    def num(self, field):
        return self.n_users if field == "user_id" else self.n_items


def ssept_case(G, O, U, RefACSSEPT, name, *, B, L, Di, Du, h, inner, n_layers, n_items, n_users, sigma, seed, train,
               mask_loss_weight=0.03):
    print(f"[ssept] {name} train={train}")
    H = Di + Du
    gen = torch.Generator().manual_seed(seed)
    cfg = G.Cfg(n_layers=n_layers, n_heads=h, user_hidden_size=Du, item_hidden_size=Di, inner_size=inner,
                hidden_dropout_prob=0.5, attn_dropout_prob=0.5, hidden_act="gelu", layer_norm_eps=1e-12, initializer_range=0.02,
                loss_type="CE", combine_option="gate", rich_calibrated_combine="none", two_level=True,
                use_position_embedding=False, use_order=True, use_distance=True, trainable_mask_loss_weight=True,
                mask_loss_weight=mask_loss_weight, USER_ID_FIELD="user_id", ITEM_ID_FIELD="item_id", LIST_SUFFIX="_list",
                ITEM_LIST_LENGTH_FIELD="item_length", NEG_PREFIX="neg_", MAX_ITEM_LIST_LENGTH=L, device="cpu")
    torch.manual_seed(seed)
    model = RefACSSEPT(cfg, Dataset(n_items, n_users))
    G.reinit(model, sigma, gen)
    lens = [int(v) for v in torch.randint(1, L + 1, (B,), generator=gen)]
    lens[0], lens[1] = 1, L
    item_seq = G.make_item_seq(B, L, n_items, lens, gen)  # right padding, as RecBole's loader pads
    users = torch.randint(1, n_users, (B,), generator=gen)
    users[-1] = users[2]  # one user twice: its embedding row accumulates two sequences' gradients
    batch = {"item_id_list": item_seq, "item_length": torch.tensor(lens, dtype=torch.long),
             "item_id": torch.randint(1, n_items, (B,), generator=gen), "user_id": users}
    ecfg = O.EncoderCfg(n_layers=n_layers, n_heads=h, hidden_size=H, inner_size=inner, combine_option="gate",
                        rich_calibrated_combine="none", seq_length=50)
    mcfg = O.ModelCfg(enc=ecfg, n_items=n_items, max_seq_length=L, mask_loss_weight=mask_loss_weight,
                      trainable_mask_loss_weight=True)
    P = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.train(train)
    arr = {"in.item_id_list": item_seq, "in.item_length": batch["item_length"], "in.item_id": batch["item_id"],
           "in.user_id": users, "meta.cfg": np.array([n_layers, h, Di, Du, inner, L, n_items, n_users]), "meta.combine": "gate",
           "meta.train": int(train), "meta.mask_loss_weight": mask_loss_weight}
    for k, v in P.items():
        arr["p." + k] = v
    shapes = ((B, h, L, L), (B, L, H))

    if not train:  # full-sort scores of both branches (acssept.py:209-228)
        torch.manual_seed(seed + 7)
        with torch.no_grad():
            att_scores, scores = model.full_sort_predict(batch)
        torch.manual_seed(seed + 7)
        rnds = [O.draw_layer_randomness(*shapes, ecfg, False) for _ in range(n_layers)]
        with torch.no_grad():
            o_att, o_cal = U.full_sort_predict(batch, P, mcfg, rnds)
        print(f"  scores: max abs diff {G.check(name + '.attacked_scores', o_att, att_scores, 2e-5):.3g}, "
              f"{G.check(name + '.scores', o_cal, scores, 2e-5):.3g}")
        arr["out.attacked_scores"], arr["out.scores"] = att_scores, scores
        for i, r in enumerate(rnds):
            arr[f"in.score_noise.{i}"] = r.noise

    # the two-pass trainer protocol (recbole/trainer/trainer.py:662-686), as oracle/gen_golden.py:210-223 runs it
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
    keep_emb = torch.empty(B, L, H).bernoulli_(0.5) if train else None
    rnds = [O.draw_layer_randomness(*shapes, ecfg, train) for _ in range(n_layers)]
    o_att, o_cal, o_grads = U.two_pass_grads(batch, P, mcfg, rnds, keep_emb)
    print(f"  losses: ref ({att_loss.item():.6f}, {cal_loss.item():.6f})  restated ({o_att.item():.6f}, {o_cal.item():.6f})")
    G.check(name + ".att_loss", o_att, att_loss.detach(), 2e-5)
    G.check(name + ".cal_loss", o_cal, cal_loss.detach(), 2e-5)
    worst = 0.0
    for n, g in ref_grads.items():
        scale = max(g.abs().max().item(), 1e-6)
        worst = max(worst, G.check(name + ".grad." + n, o_grads[n] / scale, g / scale, 2e-3))
    print(f"  grads: worst relative-to-max diff {worst:.3g}")
    assert ref_grads["user_test_embedding.weight"].abs().max() == 0
    arr["out.att_loss"], arr["out.cal_loss"] = att_loss.detach(), cal_loss.detach()
    for n, g in ref_grads.items():
        arr["grad." + n] = g
    if train:
        arr["in.keep_emb"] = keep_emb.to(torch.uint8)
    for i, r in enumerate(rnds):
        arr[f"in.noise.{i}"] = r.noise
        if train:
            for f in ("keep_after", "keep_before", "keep_mask", "keep_out_att", "keep_out_cal", "keep_ffn_att", "keep_ffn_cal"):
                arr[f"in.{f}.{i}"] = getattr(r, f).to(torch.uint8)
    return {k: (v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arr.items()}


def main():
    ref = os.environ.get("ACTSR_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
    if not ref or not os.path.isdir(os.path.join(ref, "recbole")):
        raise SystemExit("usage: ACTSR_REFERENCE=<checkout of the reference> python tools/gen_ssept_golden.py  (or pass the path)")
    os.environ["ACTSR_REFERENCE"] = ref
    from oracle import gen_golden as G  # imports the reference behind its logging stand-ins
    from oracle import ac_tsr_ref as O
    from recbole.model.sequential_recommender.acssept import ACSSEPT as RefACSSEPT  # the reference
    from tests import _unnorm_ref as U
    from tools.gen_shipped_golden import write_parts
    for name, args in CASES.items():
        write_parts(name, ssept_case(G, O, U, RefACSSEPT, name, **args))


if __name__ == "__main__":
    main()
