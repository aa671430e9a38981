"""Top-K metrics of leave-one-out evaluation from the targets' ranks (ac_tsr_amd/rank.py): host arithmetic on [B] integers.

With one positive per row, what recbole/evaluator/metrics.py computes from the [B, K] hit matrix of the collector
(recbole/evaluator/collector.py:141-153) has closed forms in the rank r of the positive:

    Hit@K = Recall@K = [r <= K]     MRR@K = [r <= K] / r     NDCG@K = [r <= K] / log2(r + 1)     Precision@K = [r <= K] / K

Keys ('mrr@10') and rounding follow recbole/evaluator/base_metric.py:65-80 and evaluator.py:28-42.  Metrics that need the
recommended item lists (ItemCoverage, ...) or several positives per row are not derivable from a rank: use
AttackSASRecTrainer.evaluate_scores and the reference's evaluator for those.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import torch

DEFAULT_METRICS = ('Recall', 'MRR', 'NDCG', 'Hit', 'Precision')
_SUPPORTED = ('recall', 'mrr', 'ndcg', 'hit', 'precision')


def _ranks(rank) -> np.ndarray:
    r = rank.detach().cpu().numpy() if isinstance(rank, torch.Tensor) else np.asarray(rank)
    r = r.reshape(-1).astype(np.int64)
    if r.size == 0:
        raise ValueError("no ranks to evaluate")
    if (r <= 0).any():
        raise ValueError(f"{int((r <= 0).sum())} of {r.size} ranks are 0 (invalid rows: a target outside the admissible items, "
                         "or a NaN score -- a model that produces NaN reports no metrics)")
    return r


def check_metric_names(metrics) -> list:
    names = [str(m).lower() for m in metrics]
    for m in names:
        if m not in _SUPPORTED:
            raise NotImplementedError(f"metric {m!r} is not a function of the target's rank (supported: "
                                      f"{', '.join(DEFAULT_METRICS)}); take the dense scores from "
                                      "AttackSASRecTrainer.evaluate_scores for it")
    return names


def topk_metrics(rank, topk=(10,), metrics=DEFAULT_METRICS, decimal_place: int = 4) -> OrderedDict:
    """{'recall@10': ..., 'mrr@10': ...}: every metric of `metrics` (in that order) at every K of `topk`, averaged over the
    rows and rounded to `decimal_place`."""
    names = check_metric_names(metrics)
    r = _ranks(rank)
    rf = r.astype(np.float64)
    result = OrderedDict()
    for m in names:
        for k in topk:
            hit = r <= int(k)
            if m in ('hit', 'recall'):
                value = hit.astype(np.float64)
            elif m == 'mrr':
                value = np.where(hit, 1.0 / rf, 0.0)
            elif m == 'ndcg':
                value = np.where(hit, 1.0 / np.log2(rf + 1.0), 0.0)
            else:
                value = hit.astype(np.float64) / float(k)
            result[f'{m}@{k}'] = round(value.mean(), decimal_place)
    return result


def rec_topk(rank, K: int) -> torch.Tensor:
    """The reference's `rec.topk` structure for these rows, int [B, K + 1]: the one-hot hit row of the top K followed by
    pos_len = 1 (collector.py:147-153), as a reference Evaluator consumes it."""
    r = torch.from_numpy(_ranks(rank))
    out = torch.zeros(r.numel(), int(K) + 1, dtype=torch.int)
    inside = r <= int(K)
    out[torch.nonzero(inside).reshape(-1), r[inside] - 1] = 1
    out[:, int(K)] = 1
    return out
