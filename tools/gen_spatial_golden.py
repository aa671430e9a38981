#!/usr/bin/env python3
"""Generate tests/golden/spatial_layer.npz by RUNNING THE GENUINE REFERENCE: one AttackRTransformerLayer used the way
the paper's ablation uses it, the spatial calibrator without the adversarial one --

    _, _, value, after_spatial, _ = layer.attack_attention.cal_origin_qkv(x, mask)      recbole/model/layers.py:686-742
    a   = layer.attack_attention.cal_adjusted_outputs(after_spatial, x, value)           layers.py:676-684
    out = layer.feed_forward(a)                                                          layers.py:790-798

in eval mode, plus the gradients of sum(out * G) with respect to the input and every parameter that takes part.

TEST INFRASTRUCTURE ONLY.  Imports the reference from its checkout (environment variable ACTSR_REFERENCE) the way
oracle/gen_golden.py does -- three logging-only modules registered as empty stand-ins -- and copies nothing from it: only
tensors are written (inputs, parameters by state-dict key, the output, the gradients).  While generating, the case is also
evaluated with the CPU restatement (oracle/ac_tsr_ref.py) and the script aborts if the two disagree.

Usage:  ACTSR_REFERENCE=<checkout of the reference> python tools/gen_spatial_golden.py
"""
import os
import sys
import types

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
REF = os.environ.get("ACTSR_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
if not REF or not os.path.isdir(os.path.join(REF, "recbole")):
    raise SystemExit("usage: ACTSR_REFERENCE=<checkout of the reference> python tools/gen_spatial_golden.py  (or pass the path)")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)

import numpy as np
import torch

for _name in ("colorlog", "colorama"):
    _m = types.ModuleType(_name)
    _m.init = lambda *a, **k: None
    sys.modules.setdefault(_name, _m)
_tb = types.ModuleType("torch.utils.tensorboard")
_tb.SummaryWriter = object
sys.modules.setdefault("torch.utils.tensorboard", _tb)

from recbole.model.layers import AttackRTransformerLayer  # noqa: E402  (the reference)

from oracle import ac_tsr_ref as O  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "spatial_layer.npz")
B, L, H, NH, INNER = 8, 50, 64, 2, 256


def main():
    torch.set_num_threads(4)
    gen = torch.Generator().manual_seed(1404)
    torch.manual_seed(1404)
    layer = AttackRTransformerLayer(NH, H, INNER, 0.5, 0.5, "gelu", 1e-12, "gate", True, True, True, "fixed", L)
    with torch.no_grad():  # parameters at a scale where every term matters (the reference's init is N(0, 0.02^2))
        for name, prm in layer.named_parameters():
            if name.endswith("LayerNorm.weight"):
                prm.copy_(1.0 + 0.1 * torch.randn(prm.shape, generator=gen))
            elif "affine" in name or name.endswith("scalar"):
                prm.copy_(0.3 * torch.randn(prm.shape, generator=gen))
            else:
                prm.copy_(0.1 * torch.randn(prm.shape, generator=gen))
    layer.eval()
    lens = [L, 23, 31, 1, 50, 7, 44, 12]
    item_seq = torch.zeros(B, L, dtype=torch.long)
    for b, n in enumerate(lens):
        ids = torch.randint(1, 1000, (n,), generator=gen)
        if b == 2:  # one LEFT-padded sequence: fully masked causal rows
            item_seq[b, L - n:] = ids
        else:       # right-padded, as RecBole's loader produces them
            item_seq[b, :n] = ids
    mask = O.attention_mask(item_seq, bidirectional=False)  # the tensor of abstract_recommender.py:136-143
    x = torch.randn(B, L, H, generator=gen).requires_grad_(True)
    G = torch.randn(B, L, H, generator=gen)

    att = layer.attack_attention
    _, _, value, after_spatial, _ = att.cal_origin_qkv(x, mask)
    out = layer.feed_forward(att.cal_adjusted_outputs(after_spatial, x, value))
    named = [(n, p) for n, p in layer.named_parameters()]
    grads = torch.autograd.grad((out * G).sum(), [x] + [p for _, p in named], allow_unused=True)

    # the CPU restatement must agree on this vector
    P = {n: p.detach() for n, p in layer.named_parameters()}
    cfg = O.EncoderCfg(n_layers=1, n_heads=NH, hidden_size=H, inner_size=INNER, combine_option="gate", seq_length=L)
    with torch.no_grad():
        _, _, v, prob, _ = O.origin_qkv(x.detach(), mask, P, cfg)
        ref = O.feed_forward(O.adjusted_outputs(prob, x.detach(), v, P, cfg), P, cfg)
    err = (ref - out.detach()).abs().max().item()
    if err > 2e-5:
        raise SystemExit(f"restatement and reference disagree: {err:.3e}")

    blob = {"item_seq": item_seq.numpy(), "x": x.detach().numpy(), "G": G.numpy(), "out": out.detach().numpy(),
            "grad.x": grads[0].numpy()}
    for (n, p), g in zip(named, grads[1:]):
        blob["param." + n] = p.detach().numpy()
        if g is not None:  # the attack transforms and the gate take no part: no gradient is stored for them
            blob["grad." + n] = g.numpy()
    np.savez_compressed(OUT, **blob)
    unused = [n for (n, _), g in zip(named, grads[1:]) if g is None]
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes); restatement error {err:.2e}; parameters without a gradient: {unused}")


if __name__ == "__main__":
    main()
