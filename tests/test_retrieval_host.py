"""CPU: multi-answer retrieval (literalkg_amd/retrieval.py) -- the two numpy references of retrieval_cases.py against each
other and against lists written out by hand, the metric formulas, the argument checks (all of them before any device
work), the empty result and the exports."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import retrieval_cases as RC
from literalkg_amd import ops, retrieval
from literalkg_amd.retrieval import AnswerRanks, evaluate_retrieval, rank_answers

NAN, INF = float("nan"), float("inf")


def both(keys, ids, answers, known=()):
    a = RC.places(keys, ids, answers, known)
    b = RC.places_brute(keys, ids, answers, known)
    assert a == b
    return a


# ----------------------------------------------------------------------------- the references
def test_ties_go_to_the_smaller_id():
    ids = [10, 11, 12, 13, 14]
    keys = [2.0, 2.0, 2.0, 1.0, 3.0]
    # the answer 11 ties with a smaller id (10, ahead of it) and a larger one (12, behind it)
    assert both(keys, ids, [11]) == {11: (2, 3)}                # list: 13, 10, 11, 12, 14
    assert both(keys, ids, [10]) == {10: (1, 2)}
    assert both(keys, ids, [12]) == {12: (3, 4)}


def test_two_tied_answers_and_answers_ahead():
    ids = [5, 6, 7, 8, 9]
    keys = [1.0, 1.0, 0.5, 1.0, 2.0]
    # list: 7, 5, 6, 8, 9; the answers 5 and 8 tie, 6 (not an answer) sits between them
    assert both(keys, ids, [5, 8]) == {5: (1, 2), 8: (2, 4)}
    assert both(keys, ids, [5, 6, 8]) == {5: (1, 2), 6: (1, 3), 8: (1, 4)}
    assert both(keys, ids, ids) == {5: (0, 2), 6: (0, 3), 7: (0, 1), 8: (0, 4), 9: (0, 5)}


def test_signed_zeros_tie():
    ids = [3, 2, 1, 0]
    keys = np.array([0.0, -0.0, 1e-45, -1.0], dtype=np.float32)
    # list: 0 (-1), then the zeros by id: 2 (-0.0), 3 (+0.0), then the subnormal 1
    assert both(keys, ids, [3]) == {3: (2, 3)}
    assert both(keys, ids, [2]) == {2: (1, 2)}
    assert both(keys, ids, [2, 3, 1]) == {2: (1, 2), 3: (1, 3), 1: (1, 4)}


def test_nan_answers_nan_candidates_and_infinities():
    ids = [0, 1, 2, 3, 4, 5]
    keys = [NAN, 1.0, NAN, INF, -INF, 2.0]
    got = both(keys, ids, [0, 5, 3])
    assert got == {0: (-1, -1), 5: (2, 3), 3: (2, 4)}           # list: 4, 1, 5, 3; the NaN candidate 2 is nowhere
    assert both(keys, ids, [2]) == {2: (-1, -1)}


def test_known_candidates_leave_the_list_but_answers_stay():
    ids = [4, 9, 2, 7, 1]
    keys = [1.0, 2.0, 3.0, 4.0, 5.0]
    assert both(keys, ids, [7], known=[4, 9, 9, 100]) == {7: (1, 2)}
    # an answer that is known is still listed: known may or may not hold the evaluated triples
    assert both(keys, ids, [9, 7], known=[4, 9, 7]) == both(keys, ids, [9, 7], known=[4]) == {9: (0, 1), 7: (1, 3)}
    with pytest.raises(AssertionError, match="not among the candidates"):
        RC.places(keys, ids, [8])


@pytest.mark.parametrize("seed", range(6))
def test_references_agree_on_random_integer_rows(seed):
    rng = np.random.default_rng(seed)
    n = 60
    ids = rng.permutation(200)[:n]
    keys = rng.integers(-3, 4, n).astype(np.float32)
    keys[rng.random(n) < 0.1] = NAN
    keys[rng.random(n) < 0.05] = -0.0
    answers = rng.choice(ids, rng.integers(1, 40), replace=False)
    known = rng.choice(ids, rng.integers(0, 25)).tolist() + [999]
    got = both(keys, ids, answers, known)
    listed = sorted(p for _, p in got.values() if p > 0)
    assert len(set(listed)) == len(listed)                      # one place each
    for a, (before, position) in got.items():
        assert (position == -1) == (before == -1) == bool(np.isnan(keys[list(ids).index(a)]))


def test_metric_formulas():
    ks = (1, 3, 10)
    q = RC.query_metrics([2, 1, 7, -1], ks)                     # m = 4, one NaN answer
    assert q["hits"] == [1, 2, 3] and q["m"] == 4
    assert q["precision"] == [1.0, 2 / 3, 0.3] and q["recall"] == [0.25, 0.5, 0.75] and q["hit"] == [1.0, 1.0, 1.0]
    d = lambda p: 1.0 / math.log2(1.0 + p)                       # noqa: E731
    assert q["ndcg"][0] == 1.0                                   # ideal at k = 1 is one term
    assert q["ndcg"][1] == pytest.approx((d(1) + d(2)) / (d(1) + d(2) + d(3)), rel=1e-15)
    # m > k: the ideal DCG stops at k; m < k: at m
    assert q["ndcg"][2] == pytest.approx((d(1) + d(2) + d(7)) / (d(1) + d(2) + d(3) + d(4)), rel=1e-15)
    assert q["ap"] == pytest.approx((1 / 1 + 2 / 2 + 3 / 7) / 4, rel=1e-15) and q["rr"] == 1.0
    miss = RC.query_metrics([-1, -1], ks)
    assert miss["hits"] == [0, 0, 0] and miss["ndcg"] == [0.0] * 3 and miss["ap"] == 0.0 and miss["rr"] == 0.0
    far = RC.query_metrics([500], ks)
    assert far["hits"] == [0, 0, 0] and far["ap"] == 1 / 500 and far["rr"] == 1 / 500
    agg = RC.aggregate([q, miss, far], ks)
    assert agg["n_queries"] == 3 and agg["n_answers"] == 7
    assert agg["hit@1"] == pytest.approx(1 / 3) and agg["mrr"] == pytest.approx((1.0 + 0.0 + 1 / 500) / 3)
    assert RC.aggregate([], ks)["map"] == 0.0


def test_discount_tables():
    disc, icum = ops.retrieval_tables(5, torch.device("cpu"))
    assert disc.dtype == icum.dtype == torch.float64 and disc.numel() == icum.numel() == 6
    assert disc[0] == 0.0 and disc[1] == 1.0 and float(disc[3]) == 0.5
    assert float(icum[5]) == pytest.approx(sum(1 / math.log2(1 + p) for p in range(1, 6)), rel=1e-15)


# ----------------------------------------------------------------------------- the front end
def stand_in(scoring="transe", n=40, c=8, n_rel=3, trans=False):
    gen = torch.Generator().manual_seed(5)
    table = torch.randn(n, c, generator=gen)

    def no_table():
        raise AssertionError("the inference table was asked for")
    return SimpleNamespace(entity_embed=SimpleNamespace(weight=table),
                           relation_embed=SimpleNamespace(weight=torch.randn(n_rel, c, generator=gen)),
                           gat_trans_M=torch.randn(n_rel, c, c, generator=gen) if trans else None,
                           n_entities=n, n_relations=n_rel, relation_dim=c, scoring=scoring, training=False,
                           eval=lambda: None, train=lambda mode=True: None, _table_for_inference=no_table)


def test_argument_errors_come_before_any_device_work():
    """everything here runs on CPU tensors: a check that reached the device code would raise RuntimeError instead"""
    m = stand_in()
    h, r, t = torch.tensor([0, 1, 2]), torch.tensor([0, 1, 2]), torch.tensor([3, 4, 5])
    for call in (lambda *a, **kw: rank_answers(m, *a, **kw), lambda *a, **kw: evaluate_retrieval(m, *a, **kw)):
        with pytest.raises(ValueError, match="rank_pairs_mlp"):
            call(h, r, t, scoring="mlp")
        with pytest.raises(ValueError, match="scoring"):
            call(h, r, t, scoring="distmult")
        with pytest.raises(ValueError, match="1-D"):
            call(h.float(), r, t)
        with pytest.raises(ValueError, match="1-D"):
            call(h, r, t[None])
        with pytest.raises(ValueError, match="1-D"):
            call(h, r == 0, t)
        with pytest.raises(ValueError, match="different lengths"):
            call(h, r[:2], t)
        with pytest.raises(ValueError, match="different lengths"):
            call(h, None, t[:2], scoring="dot")
        with pytest.raises(ValueError, match="needs the relations"):
            call(h, None, t)
        with pytest.raises(ValueError, match="1-D"):
            call(h, r, t, candidates=torch.tensor([0.5]))
        with pytest.raises(ValueError, match="unique"):
            call(h, r, t, candidates=torch.tensor([4, 2, 4]))
        with pytest.raises(ValueError, match="batch_size"):
            call(h, r, t, batch_size=0)
        with pytest.raises(ValueError, match="gat_trans_M"):
            call(h, r, t, scoring="transr")
        with pytest.raises(ValueError, match="41 entities"):
            call(h, r, t, known=SimpleNamespace(n_entities=41, device=torch.device("cpu")))
        with pytest.raises(ValueError, match="known triples live on"):
            call(h, r, t, known=SimpleNamespace(n_entities=40, device=torch.device("meta")))
        for ks in ((0,), (1.5,), (True,), (3, -1)):
            with pytest.raises(ValueError, match="positive integers"):
                call(h, r, t, ks=ks)
    with pytest.raises(ValueError, match="one side at a time"):
        rank_answers(m, h, r, t, side="both")
    with pytest.raises(ValueError, match="side"):
        evaluate_retrieval(m, h, r, t, side="left")
    # past the checks the device code refuses CPU tensors: there is no fallback
    with pytest.raises(RuntimeError, match="MI355X"):
        rank_answers(m, h, r, t)
    with pytest.raises(RuntimeError, match="MI355X"):
        evaluate_retrieval(m, h, r, t, side="both")


def test_empty_triples():
    e = torch.zeros(0, dtype=torch.int64)
    for scoring, trans in (("transe", False), ("transr", True), ("dot", False)):
        m = stand_in(scoring, trans=trans)
        res = rank_answers(m, e, e, e, side="head", ks=(1, 5))
        assert isinstance(res, AnswerRanks) and res.side == "head" and res.ks == (1, 5)
        for name in ("query", "before", "position", "q_ids", "q_rel", "n_answers", "a_query", "a_ids", "a_before",
                     "a_position"):
            x = getattr(res, name)
            assert x.shape == (0,) and x.dtype == torch.int64, name
        assert res.nan.shape == (0,) and res.nan.dtype == torch.bool
        assert res.hits.shape == (0, 2) and res.hits.dtype == torch.int64
        assert res.ndcg.shape == (0, 2) and res.ndcg.dtype == res.ap.dtype == res.rr.dtype == torch.float64
        assert rank_answers(m, e, e, e).hits is None
        for side in ("tail", "head", "both"):
            out = evaluate_retrieval(m, e, e, e, ks=(1, 5), side=side)
            assert out["n_queries"] == out["n_answers"] == out["nan"] == 0 and out["map"] == out["mrr"] == 0.0
            assert out["precision@1"] == out["recall@5"] == out["hit@5"] == out["ndcg@1"] == 0.0
            assert out["per_answer"] == {"n": 0, "mr": 0.0, "mrr": 0.0, "hits@1": 0.0, "hits@5": 0.0}
            assert ("tail" in out and "head" in out) == (side == "both")
    assert rank_answers(stand_in("dot"), e, None, e).query.numel() == 0


def test_exports():
    import literalkg_amd as L
    for name in ("rank_answers", "evaluate_retrieval", "AnswerRanks"):
        assert name in L.__all__ and getattr(L, name) is getattr(retrieval, name)
    assert callable(L.LiteralKG.rank_answers) and callable(L.LiteralKG.evaluate_retrieval)
    assert ops.RETRIEVAL_SLICE == 32
