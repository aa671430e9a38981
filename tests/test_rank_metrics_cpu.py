"""CPU suite: ac_tsr_amd.metrics against the genuine reference's evaluator.

tests/golden/eval_metrics.npz (tools/gen_eval_golden.py) holds a random [64, 300] score matrix with one positive per row, the
reference collector's `rec.topk` structure for it (recbole/evaluator/collector.py:141-153) and what the reference's Recall,
MRR, NDCG, Hit and Precision classes make of that at topk [1, 5, 10, 20] (recbole/evaluator/metrics.py).  The library gets
there from the targets' ranks alone."""
import os

import numpy as np
import pytest
import torch

from ac_tsr_amd import metrics as M
from ac_tsr_amd import rank as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_metrics.npz")


@pytest.fixture(scope="module")
def fixture():
    z = np.load(GOLDEN)
    scores, target = torch.from_numpy(z["scores"]), torch.from_numpy(z["target"])
    ranks = R.dense_ranks(scores, target, first_item=1)
    return z, scores, target, ranks


def test_dense_ranks_are_the_positions_in_torch_topk(fixture):
    z, scores, target, ranks = fixture
    order = torch.argsort(scores, dim=1, descending=True, stable=True)
    pos = (order == target[:, None]).nonzero()[:, 1] + 1
    assert ranks.rank.dtype == torch.int32 and torch.equal(ranks.rank.long(), pos)  # (continuous scores: no ties)
    assert torch.equal(ranks.target_score, scores[torch.arange(64), target])
    assert int(ranks.rank.min()) == 1 and int(ranks.rank.max()) > 20  # hits and misses at every K of the fixture


def test_topk_metrics_equal_the_reference_evaluator(fixture):
    z, _, _, ranks = fixture
    got = M.topk_metrics(ranks.rank, topk=[int(k) for k in z["topk"]], metrics=[str(m) for m in z["metrics"]], decimal_place=4)
    assert list(got.keys()) == [str(k) for k in z["keys"]]  # the reference's keys in the reference's order
    for k, v in zip(z["keys"], z["values"]):
        assert got[str(k)] == pytest.approx(float(v), abs=1e-12), k
    # numpy ranks and the default arguments
    d = M.topk_metrics(ranks.rank.numpy())
    assert list(d.keys()) == ["recall@10", "mrr@10", "ndcg@10", "hit@10", "precision@10"]
    assert d["mrr@10"] == got["mrr@10"]


def test_rec_topk_is_the_reference_collectors_structure(fixture):
    z, _, _, ranks = fixture
    K = int(max(z["topk"]))
    got = M.rec_topk(ranks.rank, K)
    assert got.shape == (64, K + 1) and got.dtype == torch.int
    assert torch.equal(got, torch.from_numpy(z["rec_topk"]).to(torch.int))


def test_closed_forms():
    r = torch.tensor([1, 2, 3, 11], dtype=torch.int32)
    d = M.topk_metrics(r, topk=(1, 10), decimal_place=6)
    assert d["hit@1"] == 0.25 and d["recall@10"] == 0.75 and d["precision@10"] == 0.075
    assert d["mrr@10"] == round((1 + 1 / 2 + 1 / 3) / 4, 6)
    assert d["ndcg@10"] == round((1 + 1 / np.log2(3) + 1 / 2) / 4, 6)


def test_invalid_rows_and_unknown_metrics_raise():
    with pytest.raises(ValueError, match="ranks are 0"):
        M.topk_metrics(torch.tensor([3, 0, 1]))
    with pytest.raises(ValueError, match="ranks are 0"):
        M.rec_topk(torch.tensor([0]), 10)
    with pytest.raises(NotImplementedError, match="evaluate_scores"):
        M.topk_metrics(torch.tensor([3, 1]), metrics=("MRR", "ItemCoverage"))


def test_dense_ranks_rules():
    s = torch.tensor([[9.0, 1.0, 3.0, 3.0, float("nan")],
                      [9.0, float("nan"), 3.0, 2.0, 1.0],
                      [9.0, 1.0, 2.0, 3.0, 4.0]])
    # row 0: target 2 ties with item 3 (not ahead), the NaN item is ahead, the padding column never counts;
    # row 1: a NaN target score is invalid; row 2: a target outside [first_item, N) is invalid
    got = R.dense_ranks(s, torch.tensor([2, 1, 7]), first_item=1)
    assert got.rank.tolist() == [2, 0, 0]
    assert float(got.target_score[0]) == 3.0 and torch.isnan(got.target_score[1:]).all()
    # history: unique pairs, the target itself and the padding item change nothing
    hist = (torch.tensor([0, 0, 0, 0]), torch.tensor([4, 4, 2, 0]))
    assert R.dense_ranks(s, torch.tensor([2, 1, 7]), 1, hist).rank.tolist() == [1, 0, 0]
