"""No GPU: the numpy references of tests/relation_cases.py against a brute-force double loop on hand-made matrices (ties,
NaNs, duplicates in the known list, a known truth), and the argument checks of score_relations / rank_relations /
predict_relations / evaluate_relation_prediction (literalkg_amd/relations.py), which precede any device work; the empty
inputs; the exports."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import relation_cases as RC
from literalkg_amd import ops, relations
from literalkg_amd.relations import (RelationTopK, evaluate_relation_prediction, predict_relations, rank_relations,
                                     score_relations)

NAN = float("nan")
INF = float("inf")


# ----------------------------------------------------------------------------- the references, by hand
def hand_case():
    #            r: 0     1     2     3     4     5
    s = [[2.0, 1.0, 2.0, NAN, 0.5, 2.0],       # ties with the truth (2), a NaN, one better
         [NAN, 3.0, 1.0, 1.0, 4.0, -INF],      # a NaN truth
         [0.0, -0.0, 1.0, 1.0, 1.0, INF],      # signed zeros tie; +inf is an ordinary score
         [NAN, NAN, NAN, NAN, NAN, NAN],       # nothing to select
         [5.0, 4.0, 3.0, 2.0, 1.0, 0.0]]
    truth = [2, 0, 1, 3, 0]
    h, t = [7, 7, 8, 9, 3], [1, 2, 1, 1, 3]
    # known triples: duplicates, a known truth (7, 2, 1), every relation of (3, ., 3), a pair nobody asks about
    kh = [7, 7, 7, 7, 8, 8, 3, 3, 3, 3, 3, 3, 3, 1]
    kr = [2, 4, 4, 0, 2, 2, 0, 1, 2, 3, 4, 5, 5, 0]
    kt = [1, 1, 1, 1, 1, 1, 3, 3, 3, 3, 3, 3, 3, 1]
    return np.array(s, dtype=np.float32), truth, RC.known_sets(h, t, kh, kr, kt)


def test_known_sets_by_hand():
    _, _, known = hand_case()
    assert known == [{0, 2, 4}, set(), {2}, set(), {0, 1, 2, 3, 4, 5}]


def test_counts_by_hand_and_by_brute_force():
    s, truth, known = hand_case()
    better, equal = RC.counts(s, truth)
    assert better.tolist() == [2, 0, 0, 0, 5] and equal.tolist() == [2, 0, 1, 0, 0]
    better, equal = RC.counts(s, truth, known)
    #   row 0: relations 0 and 4 are dropped (the truth 2 is known too and stays): better {1}, equal {5}
    #   row 4: everything but the truth is dropped
    assert better.tolist() == [1, 0, 0, 0, 0] and equal.tolist() == [1, 0, 1, 0, 0]
    for kn in (None, known):
        b, e = RC.counts(s, truth, kn)
        bb, ee = RC.counts_brute(s.tolist(), truth, kn)
        assert b.tolist() == bb and e.tolist() == ee
    rng = np.random.default_rng(3)
    for n_rel in (1, 2, 7):
        s = rng.integers(0, 3, (40, n_rel)).astype(np.float32)
        s[rng.random(s.shape) < 0.2] = np.nan
        truth = rng.integers(0, n_rel, 40).tolist()
        kn = [set(rng.integers(0, n_rel, rng.integers(0, 4)).tolist()) for _ in range(40)]
        b, e = RC.counts(s, truth, kn)
        bb, ee = RC.counts_brute(s.tolist(), truth, kn)
        assert b.tolist() == bb and e.tolist() == ee


def as_lists(ids, sc):
    return ids.tolist(), [[None if math.isnan(x) else x for x in row] for row in sc.tolist()]


def test_topk_by_hand_and_by_brute_force():
    s, _, known = hand_case()
    ids, sc = RC.topk(s, 3)
    assert ids.tolist() == [[4, 1, 0], [5, 2, 3], [0, 1, 2], [-1, -1, -1], [5, 4, 3]]
    assert as_lists(ids, sc)[1][0] == [0.5, 1.0, 2.0] and as_lists(ids, sc)[1][3] == [None] * 3
    ids, sc = RC.topk(s, 4, known)
    #   row 0: 0, 2, 4 dropped, 3 is NaN: 1, 5 remain;   row 2: 2 dropped;   row 4: all dropped
    assert ids.tolist() == [[1, 5, -1, -1], [5, 2, 3, 1], [0, 1, 3, 4], [-1] * 4, [-1] * 4]
    for kn in (None, known):
        for k in (1, 3, 6, 9):
            assert as_lists(*RC.topk(s, k, kn)) == RC.topk_brute(s.tolist(), k, kn)
    rng = np.random.default_rng(4)
    s = rng.integers(0, 3, (30, 5)).astype(np.float32)
    s[rng.random(s.shape) < 0.2] = np.nan
    kn = [set(rng.integers(0, 5, rng.integers(0, 3)).tolist()) for _ in range(30)]
    for k in (1, 2, 5, 8):
        assert as_lists(*RC.topk(s, k, kn)) == RC.topk_brute(s.tolist(), k, kn)


def test_metrics_by_hand():
    better, equal, truth = [0, 1, 0, 4, 2], [0, 1, 2, 0, 0], [0, 0, 2, 2, 3]
    m = RC.metrics(better, equal, truth, 5, ks=(1, 3))
    #   ranks 1, 2.5, 2, 5, 3
    assert m["n"] == 5 and m["mr"] == 13.5 / 5 and m["hits@1"] == 1 / 5 and m["hits@3"] == 4 / 5
    assert m["mrr"] == (1 + 0.4 + 0.5 + 0.2 + 1 / 3) / 5
    per = m["per_relation"]
    assert per["n"].tolist() == [2, 0, 2, 1, 0]
    assert per["mr"][[0, 2, 3]].tolist() == [1.75, 3.5, 3.0] and np.isnan(per["mr"][[1, 4]]).all()
    assert per["hits@1"][[0, 2, 3]].tolist() == [0.5, 0.0, 0.0]
    got = relations.relation_metrics(torch.tensor(better), torch.tensor(equal), torch.tensor(truth), 5, ks=(1, 3))
    RC.same_metrics(got, m)
    assert got["per_relation"]["n"].dtype == torch.int64 and got["per_relation"]["mr"].dtype == torch.float64
    e = torch.zeros(0, dtype=torch.int64)
    got = relations.relation_metrics(e, e, e, 3)
    RC.same_metrics(got, RC.metrics([], [], [], 3))
    assert got["n"] == 0 and got["mr"] == 0.0 and bool(torch.isnan(got["per_relation"]["mrr"]).all())


# ----------------------------------------------------------------------------- the entry points without a library
def stand_in(scoring="transe", n=40, c=8, n_rel=3, trans=False, modes=None):
    gen = torch.Generator().manual_seed(5)
    table = torch.randn(n, c, generator=gen)
    modes = modes if modes is not None else []
    return SimpleNamespace(entity_embed=SimpleNamespace(weight=table),
                           relation_embed=SimpleNamespace(weight=torch.randn(n_rel, c, generator=gen)),
                           gat_trans_M=torch.randn(n_rel, c, c, generator=gen) if trans else None,
                           n_entities=n, n_relations=n_rel, relation_dim=c, scoring=scoring, training=False,
                           _table_for_inference=lambda: table, eval=lambda: modes.append("eval"),
                           train=lambda mode: modes.append(mode))


def entry_points(m):
    return (lambda a, b, c, **kw: score_relations(m, a, c, **kw),
            lambda a, b, c, **kw: rank_relations(m, a, b, c, **kw),
            lambda a, b, c, **kw: predict_relations(m, a, c, **kw),
            lambda a, b, c, **kw: evaluate_relation_prediction(m, a, b, c, **kw))


def test_argument_errors_come_before_any_device_work():
    """everything here runs on CPU tensors: a check that reached the device code would raise RuntimeError instead"""
    modes = []
    m = stand_in(modes=modes)
    h, r, t = torch.tensor([0, 1, 2]), torch.tensor([0, 2, 2]), torch.tensor([5, 6, 7])
    for i, call in enumerate(entry_points(m)):
        with pytest.raises(ValueError, match="h must"):
            call(h.float(), r, t)
        with pytest.raises(ValueError, match="t must"):
            call(h, r, t.reshape(3, 1))
        with pytest.raises(ValueError, match="lengths"):
            call(h, r, t[:2])
        if i in (1, 3):                                    # the entry points that take the true relations
            with pytest.raises(ValueError, match="r must"):
                call(h, [0, 2, 2], t)
            with pytest.raises(ValueError, match="lengths"):
                call(h, r[:2], t)
        for bs in (0, -3, 2.5, True):
            with pytest.raises(ValueError, match="batch_size"):
                call(h, r, t, batch_size=bs)
        with pytest.raises(ValueError, match="does not depend on the relation"):
            call(h, r, t, scoring="dot")
        with pytest.raises(ValueError, match="score_pairs_mlp"):
            call(h, r, t, scoring="mlp")
        with pytest.raises(ValueError, match="scoring must"):
            call(h, r, t, scoring="cosine")
        with pytest.raises(ValueError, match="gat_trans_M"):
            call(h, r, t, scoring="transr")
        if i != 3:
            for side in ("both", "left", None):
                with pytest.raises(ValueError, match="side"):
                    call(h, r, t, side=side)
            for chunk in (0, -1, 1.5, True):
                with pytest.raises(ValueError, match="relation_chunk"):
                    call(h, r, t, relation_chunk=chunk)
        if i != 0:                                         # the entry points that take a filter
            other = SimpleNamespace(n_entities=40, n_relations=4, device=torch.device("cpu"))
            with pytest.raises(ValueError, match="4 relations, the model has 3"):
                call(h, r, t, known=other)
            other = SimpleNamespace(n_entities=41, n_relations=3, device=torch.device("cpu"))
            with pytest.raises(ValueError, match="41 entities"):
                call(h, r, t, known=other)
    for name in ("dot", "mlp"):                            # ... also as the model's own scoring
        for call in entry_points(stand_in(scoring=name)):
            with pytest.raises(ValueError, match="relation|score_pairs_mlp"):
                call(h, r, t)
    for k in (0, -1, ops.TOPK_MAX + 1, 2.0, True, None):
        with pytest.raises(ValueError, match="k must"):
            predict_relations(m, h, t, k=k)
    for ks in ((0,), (1, -2), (1.5,), (True,)):
        with pytest.raises(ValueError, match="Hits@k"):
            evaluate_relation_prediction(m, h, r, t, ks=ks)
    big = stand_in(n_rel=ops.RELATION_MAX + 1)
    for call in entry_points(big):
        with pytest.raises(ValueError, match="LDS"):
            call(h, r, t)
    assert ops.RELATION_MAX == 4096
    assert modes == []                                    # no check of the arguments touched the model's mode
    # with valid arguments the first device op is reached -- and refuses CPU tensors: there is no fallback
    for i, call in enumerate(entry_points(m)):
        with pytest.raises(RuntimeError, match="no CPU"):
            call(h, r, t)
        assert modes == (["eval", False] if i == 3 else [])     # eval mode for the evaluation alone, restored after the error
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.relation_scores(torch.zeros(9, 8), torch.zeros(9), h, t, torch.zeros(3, 8))
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.relation_order(torch.zeros(3, 3), truth=r)


def test_empty_inputs():
    e = torch.zeros(0, dtype=torch.int64)
    for scoring in ("transe", "transr"):
        modes = []
        m = stand_in(scoring, trans=scoring == "transr", modes=modes)
        s = score_relations(m, e, e)
        assert s.shape == (0, 3) and s.dtype == torch.float32
        res = rank_relations(m, e, e, e)
        assert res.better.shape == (0,) == res.equal.shape == res.rank.shape and res.better.dtype == torch.int64
        assert res.rank.dtype == torch.float64 and res.side == "tail"
        top = predict_relations(m, e, e, k=4, side="head")
        assert isinstance(top, RelationTopK) and top.side == "head"
        assert top.ids.shape == (0, 4) == top.scores.shape and top.ids.dtype == torch.int64
        assert top.scores.dtype == torch.float32
        got = evaluate_relation_prediction(m, e, e, e, ks=(1, 2))
        RC.same_metrics(got, RC.metrics([], [], [], 3, ks=(1, 2)))
        assert modes == ["eval", False]


def test_exports():
    import literalkg_amd as L
    for name in ("score_relations", "rank_relations", "predict_relations", "evaluate_relation_prediction",
                 "RelationTopK"):
        assert getattr(L, name) is getattr(relations, name) and name in L.__all__
    for name in ("score_relations", "rank_relations", "predict_relations", "evaluate_relation_prediction"):
        assert callable(getattr(L.LiteralKG, name))
