"""No GPU: the numpy references of tests/triple_cases.py against hand-worked cases, and the argument checks of
score_triples / fit_triple_thresholds / evaluate_triple_classification (literalkg_amd/triples.py), which precede any
device work; the empty inputs; the exports."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import triple_cases as TC
from literalkg_amd import triples
from literalkg_amd.triples import (TripleThresholds, evaluate_triple_classification, fit_triple_thresholds,
                                   score_triples)

INF = np.float32(np.inf)
NAN = np.float32(np.nan)


# ----------------------------------------------------------------------------- the references, by hand
def test_decisions_by_hand():
    #          rel 0: 1.0+  2.0-  2.0+  3.0-   rel 1: nan+  -0.0+  0.0-   rel 2: (none)   rel 3: 5.0-
    s = np.array([1.0, 2.0, 2.0, 3.0, np.nan, -0.0, 0.0, 5.0], dtype=np.float32)
    r = np.array([0, 0, 0, 0, 1, 1, 1, 3])
    y = np.array([1, 0, 1, 0, 1, 1, 0, 0])
    thr = np.array([2.0, 0.0, 7.0, -np.inf], dtype=np.float32)
    got = TC.decisions(s, r, y, thr, True, 4)
    #   rel 0: <= 2: 1.0+ tp, 2.0- fp, 2.0+ tp, 3.0- tn      rel 1: nan; -0.0 <= 0.0 tp; 0.0 <= 0.0 fp      rel 3: tn
    assert got.tolist() == [[2, 1, 1, 0, 0], [1, 1, 0, 0, 1], [0, 0, 0, 0, 0], [0, 0, 1, 0, 0]]
    # higher is better, one threshold everywhere: >= 2.0
    got = TC.decisions(s, r, y, np.float32(2.0), False, 4)
    #   rel 0: 1.0+ fn, 2.0- fp, 2.0+ tp, 3.0- fp      rel 1: nan; -0.0+ fn; 0.0- tn      rel 3: 5.0- fp
    assert got.tolist() == [[1, 2, 0, 1, 0], [0, 0, 1, 1, 1], [0, 0, 0, 0, 0], [0, 1, 0, 0, 0]]
    # the sentinels: nothing is positive
    assert TC.decisions(s, r, y, -INF, True, 4)[:, [0, 1]].sum() == 0
    assert TC.decisions(s, r, y, INF, False, 4)[:, [0, 1]].sum() == 0


def test_fit_by_hand():
    # rel 0: ties across the cut.  ascending groups 1.0 {+}, 2.0 {-, +, +}, 3.0 {-}; n_neg = 2
    #        correct: cut 0 -> 2, after 1.0 -> 3, after 2.0 -> 4, after 3.0 -> 3       => thr 2.0, correct 4
    # rel 1: only positives 4.0, 5.0 -> cut after the last: thr 5.0, correct 2
    # rel 2: only negatives -> the sentinel, correct 2
    # rel 3: empty -> the pooled threshold
    # rel 4: nan+, -0.0 +, 0.0 -  : one group {+, -}: correct(0) = 1 = correct(1) -> the sentinel (the smaller g), correct 1
    # rel 5: 1.0 -, 2.0 +, 3.0 +  : correct 1, 0, 1, 2 -> thr 3.0, correct 2
    # rel 6: 1.0 +, 2.0 -, 3.0 +  : correct 1, 2, 1, 2 -> the smallest maximiser: thr 1.0, correct 2
    s = np.array([1, 2, 2, 2, 3, 4, 5, 7, 8, np.nan, -0.0, 0.0, 1, 2, 3, 1, 2, 3], dtype=np.float32)
    r = np.array([0, 0, 0, 0, 0, 1, 1, 2, 2, 4, 4, 4, 5, 5, 5, 6, 6, 6])
    y = np.array([1, 0, 1, 1, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1, 1, 1, 0, 1])
    fit = TC.fit_by_definition(s, r, y, 7, True)
    assert fit["n"].tolist() == [5, 2, 2, 0, 3, 3, 3]
    assert fit["correct"].tolist() == [4, 2, 2, 0, 1, 2, 2]
    assert fit["fitted"].tolist() == [2.0, 5.0, -math.inf, -math.inf, -math.inf, 3.0, 1.0]
    # pooled, ascending: -0 {+,-} 1 {+,-,+} 2 {-,+,+,+,-} 3 {-,+,+} 4 {+} 5 {+} 7 {-} 8 {-}; n_neg = 7, n_pos = 10 (+ the nan)
    #   TP - FP after each group: 0, 1, 2, 3, 4, 5, 4, 3 -> after 5.0: correct = 7 + 5 = 12
    assert fit["global_threshold"] == np.float32(5.0) and fit["global_correct"] == 12
    assert fit["thresholds"].tolist() == [2.0, 5.0, -math.inf, 5.0, -math.inf, 3.0, 1.0]
    # what the fit calls correct is what decisions() counts at that threshold (NaN: wrong)
    d = TC.decisions(s, r, y, fit["thresholds"], True, 7)
    assert (d[:, 0] + d[:, 2]).tolist() == fit["correct"].tolist()
    # higher is better: the mirror image (negate the scores) gives the negated thresholds and the same integers
    neg = TC.fit_by_definition(-s, r, y, 7, False)
    assert neg["correct"].tolist() == fit["correct"].tolist() and neg["global_correct"] == 12
    assert neg["fitted"].tolist() == [-2.0, -5.0, math.inf, math.inf, math.inf, -3.0, -1.0]
    # a zero threshold is +0.0:  -0.0 +, 1.0 -
    z = TC.fit_by_definition(np.array([-0.0, 1.0], dtype=np.float32), [0, 0], [1, 0], 1, True)
    assert z["correct"].tolist() == [2] and z["thresholds"].view(np.uint32).tolist() == [0]


def test_metrics_by_hand():
    counts = np.array([[2, 1, 1, 0, 0], [1, 1, 0, 0, 1], [0, 0, 0, 0, 0], [0, 0, 1, 0, 0]])
    y = np.array([1, 0, 1, 0, 1, 1, 0, 0])
    m = TC.metrics(counts, y, (4, 4, 0, 5, 20, 0.75))
    assert (m["tp"], m["fp"], m["tn"], m["fn"], m["nan"], m["n"], m["n_pos"], m["n_neg"]) == (3, 2, 2, 0, 1, 8, 4, 4)
    assert m["accuracy"] == 5 / 8 and m["precision"] == 3 / 5 and m["recall"] == 1.0
    assert m["f1"] == (2.0 * (3 / 5) * 1.0) / ((3 / 5) + 1.0)
    assert m["macro_accuracy"] == (3 / 4 + 1 / 3 + 1.0) / 3                  # the empty relation is left out
    assert m["roc_auc"] == 20 / 32 and m["average_precision"] == 0.75
    assert m["per_relation"]["nan"].tolist() == [0, 1, 0, 0]
    e = TC.metrics(np.zeros((3, 5), dtype=np.int64), np.zeros(0))
    assert e["n"] == 0 and e["accuracy"] == 0.0 and e["macro_accuracy"] == 0.0 and math.isnan(e["roc_auc"])
    TC.same_metrics(triples.triple_metrics(torch.from_numpy(counts), 4, 4, (4, 4, 0, 5, 20, 0.75)), m, 5)
    TC.same_metrics(triples.triple_metrics(torch.zeros((3, 5), dtype=torch.int64), 0, 0), e)


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


def test_argument_errors_come_before_any_device_work():
    """everything here runs on CPU tensors: a check that reached the device code would raise RuntimeError instead"""
    modes = []
    m = stand_in(modes=modes)
    h, r, t = torch.tensor([0, 1, 2]), torch.tensor([0, 2, 2]), torch.tensor([5, 6, 7])
    y = torch.tensor([0, 1, 1], dtype=torch.uint8)
    calls = (lambda a, b, c, **kw: score_triples(m, a, b, c, **kw),
             lambda a, b, c, **kw: fit_triple_thresholds(m, a, b, c, y, **kw),
             lambda a, b, c, **kw: evaluate_triple_classification(m, a, b, c, y, 1.0, **kw))
    for call in calls:
        with pytest.raises(ValueError, match="h must"):
            call(h.float(), r, t)
        with pytest.raises(ValueError, match="r must"):
            call(h, [0, 2, 2], t)
        with pytest.raises(ValueError, match="t must"):
            call(h, r, t.reshape(3, 1))
        with pytest.raises(ValueError, match="lengths"):
            call(h, r[:2], t)
        for bs in (0, -3, 2.5, True):
            with pytest.raises(ValueError, match="batch_size"):
                call(h, r, t, batch_size=bs)
        with pytest.raises(ValueError, match="score_pairs_mlp"):
            call(h, r, t, scoring="mlp")
        with pytest.raises(ValueError, match="scoring must"):
            call(h, r, t, scoring="cosine")
        with pytest.raises(ValueError, match="gat_trans_M"):
            call(h, r, t, scoring="transr")
    for side in ("both", "left", None):
        with pytest.raises(ValueError, match="side"):
            score_triples(m, h, r, t, side=side)
    for bad in (y[:2], y.long(), y.float(), y.reshape(1, 3), [0, 1, 1]):
        with pytest.raises(ValueError, match="labels"):
            fit_triple_thresholds(m, h, r, t, bad)
        with pytest.raises(ValueError, match="labels"):
            evaluate_triple_classification(m, h, r, t, bad, 1.0)
    for bad in (math.nan, torch.tensor([1.0, math.nan, 2.0]), torch.zeros(2), torch.zeros(3, dtype=torch.float64),
                torch.zeros(1, 3), "0.5", None, True,
                TripleThresholds(torch.zeros(3), 0.0, "dot", torch.zeros(3), torch.zeros(3))):
        with pytest.raises(ValueError, match="threshold"):
            evaluate_triple_classification(m, h, r, t, y, bad)
    assert modes == []                                    # no check of the arguments touched the model's mode
    # with valid arguments the first device op is reached -- and refuses CPU tensors: there is no fallback
    with pytest.raises(RuntimeError, match="no CPU"):
        score_triples(m, h, r, t, side="head", batch_size=2, kernel_scores=True)
    assert modes == []                                    # score_triples leaves the mode alone
    for labels in (y, y.bool()):
        with pytest.raises(RuntimeError, match="no CPU"):
            fit_triple_thresholds(m, h, r, t, labels, per_relation=False)
        for thr in (0.5, -math.inf, torch.zeros(3), TripleThresholds(torch.zeros(3), 0.0, "transe", None, None)):
            with pytest.raises(RuntimeError, match="no CPU"):
                evaluate_triple_classification(m, h, r, t, labels, thr)
    assert modes == ["eval", False] * 10                  # eval mode for the work, the previous mode restored after the error
    from literalkg_amd import ops
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.triple_scores(torch.zeros(3, 8), h, t)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.threshold_fit(torch.zeros(3), y, r, 3, True)


def test_empty_inputs():
    e = torch.zeros(0, dtype=torch.int64)
    y = torch.zeros(0, dtype=torch.uint8)
    for scoring, s_ in (("transe", -math.inf), ("dot", math.inf), ("transr", -math.inf)):
        modes = []
        m = stand_in(scoring, trans=scoring == "transr", modes=modes)
        out = score_triples(m, e, e, e)
        assert out.shape == (0,) and out.dtype == torch.float32
        fit = fit_triple_thresholds(m, e, e, e, y)
        assert fit.scoring == scoring and fit.global_threshold == s_ == triples.sentinel(scoring)
        assert fit.thresholds.tolist() == [s_] * 3 and fit.thresholds.dtype == torch.float32
        assert fit.n.tolist() == [0, 0, 0] == fit.correct.tolist() and fit.n.dtype == torch.int64
        got = evaluate_triple_classification(m, e, e, e, y, fit)
        TC.same_metrics(got, TC.metrics(np.zeros((3, 5), dtype=np.int64), np.zeros(0)))
        assert math.isnan(got["roc_auc"]) and math.isnan(got["average_precision"]) and got["n"] == 0
        assert modes == []


def test_exports():
    import literalkg_amd as L
    for name in ("score_triples", "fit_triple_thresholds", "evaluate_triple_classification", "TripleThresholds"):
        assert getattr(L, name) is getattr(triples, name) and name in L.__all__
    for name in ("score_triples", "fit_triple_thresholds", "evaluate_triple_classification"):
        assert callable(getattr(L.LiteralKG, name))
