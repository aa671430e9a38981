#!/usr/bin/env python3
"""Generate tests/golden/eval_metrics.npz by RUNNING THE GENUINE REFERENCE's evaluation pieces on the CPU: the collector's
top-K selection and hit gather (recbole/evaluator/collector.py:141-153, Collector.eval_batch_collect) and the five default
metric classes Recall, MRR, NDCG, Hit, Precision (recbole/evaluator/metrics.py) through recbole/evaluator/evaluator.py, on a
random [64, 300] score matrix with one positive per row and the padding column at -inf (recbole/trainer/trainer.py:941-942),
at topk [1, 5, 10, 20].

TEST INFRASTRUCTURE ONLY; copies nothing from the reference.  Only data is written: the scores, the targets, the reference's
`rec.topk` structure and its metric dict (as two parallel arrays, keys and values).  The reference's logging-only imports are
registered as empty stand-ins (as oracle/gen_golden.py does) and `np.float`, which its metrics still use, is set here.

Usage:  ACTSR_REFERENCE=<checkout of the reference> python tools/gen_eval_golden.py
"""
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("ACTSR_REFERENCE", "/root/reference")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)

if not hasattr(np, "float"):
    np.float = float  # removed from numpy 1.24; recbole/evaluator/metrics.py:90 still names it
for _name in ("colorlog", "colorama"):
    _m = types.ModuleType(_name)
    _m.init = lambda *a, **k: None
    sys.modules.setdefault(_name, _m)
_tb = types.ModuleType("torch.utils.tensorboard")
_tb.SummaryWriter = object
sys.modules.setdefault("torch.utils.tensorboard", _tb)

from recbole.evaluator.collector import Collector  # noqa: E402  (the reference)
from recbole.evaluator.evaluator import Evaluator  # noqa: E402

B, N, TOPK, SEED = 64, 300, [1, 5, 10, 20], 20240607
METRICS = ["Recall", "MRR", "NDCG", "Hit", "Precision"]


class Cfg(dict):
    """recbole Config look-alike: missing keys read as None."""

    def __getitem__(self, k):
        return self.get(k, None)


def main():
    gen = torch.Generator().manual_seed(SEED)
    scores = torch.randn(B, N, generator=gen)
    target = torch.randint(1, N, (B,), generator=gen)
    # ranks of every kind: a few rows whose target is the best item, a few where it is far down
    scores[torch.arange(0, 8), target[:8]] += 6.0
    scores[torch.arange(8, 12), target[8:12]] -= 6.0
    scores[:, 0] = -np.inf  # trainer.py:942
    cfg = Cfg(eval_args={"mode": "full"}, topk=TOPK, device="cpu", metrics=METRICS, metric_decimal_place=4,
              eval_type=None)
    collector = Collector(cfg)
    collector.eval_batch_collect(scores.clone(), None, torch.arange(B), target)
    struct = collector.get_data_struct()
    result = Evaluator(cfg).evaluate(struct)
    rec_topk = struct.get("rec.topk").numpy()
    keys = np.array(list(result.keys()))
    values = np.array([float(v) for v in result.values()], dtype=np.float64)
    out = os.path.join(ROOT, "tests", "golden", "eval_metrics.npz")
    np.savez_compressed(out, scores=scores.numpy(), target=target.numpy(), topk=np.array(TOPK), metrics=np.array(METRICS),
                        rec_topk=rec_topk, keys=keys, values=values)
    print(f"wrote {out} ({os.path.getsize(out)} bytes)")
    for k, v in result.items():
        print(f"  {k} = {v}")


if __name__ == "__main__":
    main()
