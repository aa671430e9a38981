"""GPU suite (-m gpu): full_sort_rank of the four models and AttackSASRecTrainer.evaluate / _valid_epoch.

A model's full_sort_rank must give the ranks counted from the same model's own full_sort_predict scores, on every row whose
rank is decided beyond fp32 rounding: the float64 interval of tests/_rank_cases.py, computed from the model's returned
representation and its item table, is a single point there.  The attacked branch draws its noise from torch's seeded CPU
generator, so every forward of a comparison starts from the same seed.  Tiny configurations of the existing model tests.
"""
import pytest
import torch

import ac_tsr_amd as A
from ac_tsr_amd import metrics as M
from ac_tsr_amd import rank as R
from tests import _rank_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_ITEMS, B, L = 300, 48, 50

BASE = dict(n_layers=2, n_heads=2, inner_size=256, hidden_dropout_prob=0.5, attn_dropout_prob=0.5, hidden_act='gelu',
            layer_norm_eps=1e-12, initializer_range=0.02, loss_type='CE', combine_option='gate', two_level=True, use_order=True,
            use_distance=True, mask_loss_weight=0.03)


def _batch(seed=1, rows=B, max_len=L):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(5, max_len + 1, (rows,), generator=g)
    live = torch.arange(L)[None] < lens[:, None]
    ids = torch.randint(1, N_ITEMS, (rows, L), generator=g) * live
    stamps = (1000 + torch.randint(0, 128, (rows, L), generator=g).cumsum(1)) * live
    b = {"item_id_list": ids, "item_length": lens, "item_id": torch.randint(1, N_ITEMS, (rows,), generator=g),
         "user_id": torch.randint(1, 50, (rows,), generator=g), "timestamp_list": stamps}
    return {k: v.to(DEV) for k, v in b.items()}


def _sasrec(hidden=64):
    torch.manual_seed(0)
    return A.ACSASRec(A.DictConfig(dict(BASE, hidden_size=hidden)), A.ItemCount(N_ITEMS)).to(DEV).eval()


def _ssept():
    torch.manual_seed(0)
    return A.ACSSEPT(A.DictConfig(dict(BASE, user_hidden_size=64, item_hidden_size=64)), A.Counts(N_ITEMS, 50)).to(DEV).eval()


def _tisasrec():
    torch.manual_seed(0)
    cfg = dict(BASE, hidden_size=64, time_span=256, TIME_FIELD="timestamp")
    return A.ACTiSASRec(A.DictConfig(cfg), A.ItemCount(N_ITEMS)).to(DEV).eval()


def _bert():
    torch.manual_seed(0)
    # evaluation runs on L + 1 columns: combine_option 'fixed' and no position table, as the golden case bert_fixed_scores
    # (the gate and the position table are L wide: tests/test_hip_bert4rec.py::test_evaluation_keeps_the_reference_failure_modes)
    cfg = dict(BASE, hidden_size=64, combine_option='fixed', use_position_embedding=False, mask_ratio=0.2, cloze_on_device=True,
               device=DEV)
    return A.AcBERT4Rec(A.DictConfig(cfg), A.ItemCount(N_ITEMS)).to(DEV).eval()


def _representations(kind, m, b):
    """(attacked or None, calibrated) [B, H'] and the table rows full_sort_predict scores against."""
    if kind == "sasrec":
        _, cal, _ = m.forward(b["item_id_list"], b["item_length"])
        return None, cal, m.item_embedding.weight
    if kind == "ssept":
        att, cal, _ = m.forward(b["item_id_list"], b["item_length"], b["user_id"])
        Di = m.item_hidden_size
        return att[:, :Di], cal[:, :Di], m.item_embedding.weight
    if kind == "tisasrec":
        att, cal, _ = m._outputs(b)
        return att, cal, m.item_embedding.weight
    seq = m.reconstruct_test_data(b["item_id_list"], b["item_length"])
    att, cal, _ = m.forward(seq, _rows=b["item_length"].view(-1, 1))
    return att.squeeze(1), cal.squeeze(1), m.item_embedding.weight[:m.n_items]


def _decided(rep, table, target):
    """(lo, hi, s_t64, delta_t) of the float64 intervals for a representation."""
    s, delta = RC.scores64(rep.detach().cpu(), table.detach().cpu())
    lo, hi = RC.intervals(s, delta, target.cpu(), 1)
    rows = torch.arange(rep.shape[0])
    return lo, hi, s[rows, target.cpu()], delta[rows, target.cpu()]


MODELS = {"sasrec": _sasrec, "ssept": _ssept, "tisasrec": _tisasrec, "bert": _bert}


@pytest.mark.parametrize("kind", list(MODELS))
def test_full_sort_rank_equals_ranks_counted_from_full_sort_predict(kind):
    m = MODELS[kind]()
    b = _batch(max_len=L - 1 if kind == "bert" else L)  # (AcBERT4Rec appends the mask token to the sequence)
    target = b["item_id"]
    with torch.no_grad():
        torch.manual_seed(3)
        att_s, cal_s = m.full_sort_predict(b)
        torch.manual_seed(3)
        att_r, cal_r = m.full_sort_rank(b)
        torch.manual_seed(3)
        att_rep, cal_rep, table = _representations(kind, m, b)
    assert (att_s is None) == (att_r is None) == (att_rep is None)
    for name, scores, got, rep in (("attacked", att_s, att_r, att_rep), ("calibrated", cal_s, cal_r, cal_rep)):
        if scores is None:
            continue
        assert isinstance(got, R.Ranks) and got.rank.dtype == torch.int32 and got.rank.shape == (B,)
        want = R.dense_ranks(scores.view(B, N_ITEMS), target, 1)
        lo, hi, s_t, delta_t = _decided(rep, table, target)
        sure = (lo == hi)
        print(f"{kind} {name}: {int(sure.sum())} of {B} rows decided, ranks {int(got.rank.min())} .. {int(got.rank.max())}")
        assert int(sure.sum()) >= B // 2
        assert torch.equal(got.rank.cpu()[sure], want.rank.cpu()[sure])
        assert torch.equal(got.rank.cpu().long()[sure], lo[sure])
        assert bool(((got.rank.cpu() >= lo) & (got.rank.cpu() <= hi)).all())
        if kind != "ssept":
            assert bool(((got.target_score.cpu().double() - s_t).abs() <= delta_t).all())


def test_ssept_target_score_includes_the_user_term():
    m, b = _ssept(), _batch()
    target = b["item_id"]
    with torch.no_grad():
        torch.manual_seed(3)
        _, cal_s = m.full_sort_predict(b)
        torch.manual_seed(3)
        _, cal_r = m.full_sort_rank(b)
        _, cal, _ = m.forward(b["item_id_list"], b["item_length"], b["user_id"])
        term = m._user_test_term(cal, b["user_id"])
    picked = cal_s.gather(1, target.view(-1, 1)).squeeze(1)
    # both sides are fp32 sums of the same two fp32 terms, each within its dot-product bound: 1e-5 of the scores' scale is
    # far above that and far below the term itself
    scale = picked.abs().max().item()
    assert (cal_r.target_score - picked).abs().max().item() <= 1e-5 * max(scale, 1.0)
    assert term.abs().max().item() > 1e-3 * max(scale, 1.0)  # dropping the term would be seen
    assert (cal_r.target_score - term - picked).abs().max().item() > 1e-4 * max(scale, 1.0)


def test_bert4rec_never_counts_the_mask_token_row():
    m, b = _bert(), _batch(max_len=L - 1)
    assert m.item_embedding.weight.shape[0] == N_ITEMS + 1
    with torch.no_grad():
        m.item_embedding.weight[N_ITEMS] *= 40.0  # a row that scores far above or below everything
        torch.manual_seed(3)
        _, cal_s = m.full_sort_predict(b)
        torch.manual_seed(3)
        _, cal_r = m.full_sort_rank(b)
        _, cal_rep, table = _representations("bert", m, b)
        mask_row_score = cal_rep.double() @ m.item_embedding.weight[N_ITEMS].double()
    lo, hi, s_t, _ = _decided(cal_rep, table, b["item_id"])
    assert int((mask_row_score.cpu() > s_t).sum()) >= 1  # counting it would raise these rows' ranks
    sure = lo == hi
    assert torch.equal(cal_r.rank.cpu().long()[sure], lo[sure])
    assert torch.equal(cal_r.rank.cpu()[sure], R.dense_ranks(cal_s, b["item_id"], 1).rank.cpu()[sure])


def test_unsupported_hidden_size_takes_the_dense_path_and_agrees():
    m, b = _sasrec(hidden=32), _batch()
    assert not R.supported(32)
    with torch.no_grad():
        _, scores = m.full_sort_predict(b)
        none, got = m.full_sort_rank(b)
    assert none is None
    want = R.dense_ranks(scores, b["item_id"], 1)
    assert torch.equal(got.rank, want.rank) and got.rank.dtype == torch.int32
    assert (got.target_score - want.target_score).abs().max().item() <= 1e-6


def _loader(seeds=(1, 2)):
    out = []
    for s in seeds:
        b = _batch(seed=s)
        inter = {k: v.cpu() for k, v in b.items() if k != "item_id"}  # the reference's loader: "interaction without item ids"
        out.append((inter, None, torch.arange(B), b["item_id"].cpu()))
    return out


def test_trainer_evaluate_and_valid_epoch():
    m = _sasrec()
    trainer = A.AttackSASRecTrainer(A.DictConfig(learner='adam', learning_rate=1e-3, metric_decimal_place=10), m)
    loader = _loader()
    m.train()
    result = trainer.evaluate(loader)
    assert not m.training
    assert list(result) == ["recall@10", "mrr@10", "ndcg@10", "hit@10", "precision@10"]
    topk = [5, 20, 100]
    result = trainer.evaluate(loader, topk=topk)
    # == topk_metrics of the concatenated ranks
    ranks, open_rows, dense = [], 0, []
    for inter, _, _, pos_i in loader:
        dev = {k: v.to(DEV) for k, v in inter.items()}
        _, r = m.full_sort_rank(dev, target=pos_i.to(DEV))
        ranks.append(r.rank)
        with torch.no_grad():
            _, cal, _ = m.forward(dev["item_id_list"], dev["item_length"])
        lo, hi, _, _ = _decided(cal, m.item_embedding.weight, pos_i)
        open_rows += int((hi > lo).sum())
        # what the reference does: dense scores with the padding column at -inf, top-K, position of the positive
        scores = trainer.evaluate_scores(dev)
        idx = torch.topk(scores, max(topk), dim=-1).indices.cpu()
        hit = idx == pos_i[:, None]
        dense.append(torch.where(hit.any(1), hit.float().argmax(1) + 1, torch.full((B,), N_ITEMS)))
    assert result == M.topk_metrics(torch.cat(ranks), topk, M.DEFAULT_METRICS, 10)
    want = M.topk_metrics(torch.cat(dense), topk, M.DEFAULT_METRICS, 10)
    assert result["hit@100"] > 0
    for k in want:
        assert abs(result[k] - want[k]) <= open_rows / (2 * B) + 1e-9, (k, result[k], want[k], open_rows)
    score, res = trainer._valid_epoch(loader)
    assert list(res) == ["recall@10", "mrr@10", "ndcg@10", "hit@10", "precision@10"] and score == res["mrr@10"]
    trainer.config["valid_metric"] = "NDCG@10"
    assert trainer._valid_epoch(loader)[0] == res["ndcg@10"]


def test_trainer_evaluate_refuses_what_a_rank_cannot_express():
    m = _sasrec()
    trainer = A.AttackSASRecTrainer(A.DictConfig(learner='adam', learning_rate=1e-3), m)
    inter, _, pos_u, pos_i = _loader()[0]
    with pytest.raises(NotImplementedError, match="evaluate_scores"):
        trainer.evaluate([(inter, None, torch.cat([pos_u[:-1], pos_u[-2:-1]]), pos_i)])  # two positives in one row
    with pytest.raises(NotImplementedError, match="evaluate_scores"):
        trainer.evaluate([(inter, None, pos_u, pos_i)], metrics=["MRR", "GAUC"])
    # history pairs reach the kernel: with every row's best items taken out, no rank gets worse and some improve
    dev = {k: v.to(DEV) for k, v in inter.items()}
    scores = trainer.evaluate_scores(dev)
    best = torch.topk(scores, 5, dim=-1).indices.cpu()
    hist = (torch.arange(B).repeat_interleave(5), best.reshape(-1))
    r0 = trainer.evaluate([(inter, None, pos_u, pos_i)], topk=[100], metrics=["MRR"])
    r1 = trainer.evaluate([(inter, hist, pos_u, pos_i)], topk=[100], metrics=["MRR"])
    assert r1["mrr@100"] > r0["mrr@100"]
