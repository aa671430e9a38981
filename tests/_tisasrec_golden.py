"""Loader of the ACTiSASRec fixtures tests/golden/tisasrec_{train,eval}.partNN.npz (tools/gen_tisasrec_golden.py: tensors the
genuine reference produced, on which tests/_timeaware_ref.py agreed with it when they were written).  Keep masks are stored
packed (np.packbits) under `bits.*`."""
import glob
import os

import numpy as np
import torch

from oracle import ac_tsr_ref as O
from tests import _golden
from tests import _timeaware_ref as T

KEEPS = ("keep_after", "keep_before", "keep_mask", "keep_out_att", "keep_out_cal", "keep_ffn_att", "keep_ffn_cal")


class TisasrecCase:
    def __init__(self, name):
        parts = sorted(glob.glob(os.path.join(_golden.GOLDEN_DIR, name + ".part*.npz")))
        assert parts, name
        self.name, self.raw = name, {}
        for path in parts:
            z = np.load(path, allow_pickle=False)
            assert not set(z.files) & set(self.raw), path
            self.raw.update({k: z[k] for k in z.files})
        (self.n_layers, self.n_heads, self.H, self.inner, self.L, self.n_items, self.span,
         self.B) = (int(v) for v in self.raw["meta.cfg"])
        self.train = bool(int(self.raw["meta.train"]))

    def t(self, key):
        return torch.from_numpy(self.raw[key])

    def bits(self, key, shape):
        n = int(np.prod(shape))
        return torch.from_numpy(np.unpackbits(self.raw["bits." + key])[:n].reshape(shape).copy()).float()

    def params(self):
        return {k[2:]: torch.from_numpy(v) for k, v in self.raw.items() if k.startswith("p.")}

    def grads(self):
        return {k[5:]: torch.from_numpy(v) for k, v in self.raw.items() if k.startswith("grad.")}

    def batch(self):
        return {k: self.t("in." + k) for k in ("item_id_list", "item_length", "item_id", "timestamp_list")}

    def model_cfg(self):
        enc = O.EncoderCfg(n_layers=self.n_layers, n_heads=self.n_heads, hidden_size=self.H, inner_size=self.inner,
                           combine_option="gate", rich_calibrated_combine="none", seq_length=50)
        return O.ModelCfg(enc=enc, n_items=self.n_items, max_seq_length=self.L,
                          mask_loss_weight=float(self.raw["meta.mask_loss_weight"]), trainable_mask_loss_weight=True)

    def config(self):
        """The config mapping of ac_tsr_amd.ACTiSASRec (and of the reference's) for this fixture."""
        return dict(n_layers=self.n_layers, n_heads=self.n_heads, hidden_size=self.H, inner_size=self.inner,
                    hidden_dropout_prob=0.5, attn_dropout_prob=0.5, hidden_act="gelu", layer_norm_eps=1e-12,
                    initializer_range=0.02, loss_type="CE", combine_option="gate", rich_calibrated_combine="none",
                    two_level=True, use_position_embedding=False, use_order=True, use_distance=True,
                    trainable_mask_loss_weight=True, mask_loss_weight=float(self.raw["meta.mask_loss_weight"]),
                    time_span=self.span, TIME_FIELD="timestamp", MAX_ITEM_LIST_LENGTH=self.L)

    def layer_randomness(self, noise_key="noise"):
        """The draws of the two-pass run (`noise_key` "score_noise": of the full_sort_predict run, noise only)."""
        B, L, H, h = self.B, self.L, self.H, self.n_heads
        out = []
        for i in range(self.n_layers):
            r = O.LayerRandomness(noise=self.t(f"in.{noise_key}.{i}"))
            if self.train and noise_key == "noise":
                for f in KEEPS:
                    setattr(r, f, self.bits(f"{f}.{i}", (B, h, L, L) if f in KEEPS[:3] else (B, L, H)))
            out.append(r)
        return out

    def model_randomness(self):
        if not self.train:
            return T.ModelRandomness()
        B, L, H = self.B, self.L, self.H
        return T.ModelRandomness(keep_emb=self.bits("keep_emb", (B, L, H)), keep_pos_k=self.bits("keep_pos_k", (B, L, H)),
                                 keep_pos_v=self.bits("keep_pos_v", (B, L, H)), keep_time_k=self.bits("keep_time_k", (B, L, L, H)),
                                 keep_time_v=self.bits("keep_time_v", (B, L, L, H)))
