"""No GPU: the argument checks of score_pairs_mlp / evaluate_mlp_classification (literalkg_amd/pairmlp.py), which precede
any device work, the empty case, the exports -- and the numpy references of tests/pair_cases.py themselves: they accept
a correct restatement of the definitions and reject five planted faults."""
import math
import struct
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pair_cases as PC
from literalkg_amd import pairmlp
from literalkg_amd.pairmlp import evaluate_mlp_classification, score_pairs_mlp

from test_pairmlp_host import stand_in


def with_modes(m, modes):
    model = SimpleNamespace(eval=lambda: modes.append("eval"), train=lambda mode: modes.append(mode), **vars(m))
    return model


def test_argument_errors_come_before_any_device_work():
    """everything here runs on CPU tensors: a check that reached the device code would raise RuntimeError instead"""
    m, table, gen = stand_in()
    modes = []
    me = with_modes(m, modes)
    h, t, y = torch.tensor([0, 1, 2]), torch.tensor([5, 6, 7]), torch.tensor([0, 1, 1])
    for call in (lambda a, b, **kw: score_pairs_mlp(m, a, b, **kw),
                 lambda a, b, **kw: evaluate_mlp_classification(me, a, b, y, **kw)):
        with pytest.raises(ValueError, match="h must"):
            call(h.float(), t)
        with pytest.raises(ValueError, match="t must"):
            call(h, t.reshape(3, 1))
        with pytest.raises(ValueError, match="h must"):
            call([0, 1, 2], t)
        with pytest.raises(ValueError, match="lengths"):
            call(h[:2], t)
        for bs in (0, -3, 2.5, True):
            with pytest.raises(ValueError, match="batch_size"):
                call(h, t, batch_size=bs)
    with pytest.raises(ValueError, match="lengths"):
        evaluate_mlp_classification(me, h, t, y[:2])
    for bad in (torch.tensor([0, 1, 2]), torch.tensor([0.0, 0.5, 1.0]), torch.tensor([0.0, math.nan, 1.0]),
                torch.tensor([[0, 1, 1]]), [0, 1, 1], torch.tensor([0, -1, 1])):
        with pytest.raises(ValueError, match="labels"):
            evaluate_mlp_classification(me, h, t, bad)
    for thr in (0, 1, 1.5, -0.2, math.nan):
        with pytest.raises(ValueError, match="threshold"):
            evaluate_mlp_classification(me, h, t, y, threshold=thr)
    with pytest.raises(ValueError, match="logit_threshold"):
        evaluate_mlp_classification(me, h, t, y, logit_threshold=math.nan)
    assert modes == []                                    # no check of the arguments touched the model's mode
    # a model without a head
    bare = SimpleNamespace(entity_embed=m.entity_embed, n_entities=m.n_entities, n_relations=3, scoring="dot",
                           training=False, _table_for_inference=m._table_for_inference, eval=lambda: None,
                           train=lambda mode: None)
    with pytest.raises(AttributeError, match="initialize_MLP"):
        score_pairs_mlp(bare, h, t)
    with pytest.raises(AttributeError, match="initialize_MLP"):
        evaluate_mlp_classification(bare, h, t, y)
    # with valid arguments the first device op is reached -- and refuses CPU tensors: there is no fallback
    with pytest.raises(RuntimeError, match="no CPU"):
        score_pairs_mlp(m, h, t)
    for labels in (y, y.bool(), y.to(torch.int32), y.float()):
        with pytest.raises(RuntimeError, match="no CPU"):
            evaluate_mlp_classification(me, h, t, labels, threshold=0.3, batch_size=2)
    with pytest.raises(RuntimeError, match="no CPU"):
        evaluate_mlp_classification(me, h, t, y, threshold=7, logit_threshold=-math.inf)      # the override wins
    assert modes == ["eval", False] * 5                   # eval mode for the work, the previous mode restored after the error
    from literalkg_amd import ops
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.binary_curve(torch.zeros(3), torch.zeros(3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.pair_mlp_pairs(torch.zeros(3, 128), torch.zeros(3, 128), torch.zeros(64, 128), torch.zeros(64),
                           torch.zeros(64), torch.zeros(1))


def test_threshold_is_applied_on_the_logit():
    assert pairmlp.logit_of_probability(0.5) == 0.0 and math.copysign(1.0, pairmlp.logit_of_probability(0.5)) == 1.0
    for p in (0.3, 0.9, 1e-9, 1 - 1e-12):
        want = struct.unpack("f", struct.pack("f", math.log(p / (1.0 - p))))[0]      # float64, rounded once to float32
        assert pairmlp.logit_of_probability(p) == want


def test_empty_input_needs_no_device():
    m, table, gen = stand_in()
    e = torch.zeros(0, dtype=torch.int64)
    for kw in (dict(), dict(logits=True, batch_size=5)):
        z = score_pairs_mlp(m, e, e, **kw)
        assert z.shape == (0,) and z.dtype == torch.float32
    modes = []
    model = with_modes(m, modes)
    model.training = True
    out = evaluate_mlp_classification(model, e, e, torch.zeros(0, dtype=torch.bool), batch_size=3)
    assert modes == ["eval", True]                       # switched to eval, previous mode restored
    assert set(out) == {"accuracy", "precision", "recall", "f1", "tp", "fp", "tn", "fn", "nan", "n", "n_pos", "n_neg",
                        "roc_auc", "average_precision"}
    for k in ("accuracy", "precision", "recall", "f1", "tp", "fp", "tn", "fn", "nan", "n", "n_pos", "n_neg"):
        assert out[k] == 0, k
    assert math.isnan(out["roc_auc"]) and math.isnan(out["average_precision"])


def test_exports_and_abi_names():
    import inspect

    import literalkg_amd
    from literalkg_amd import _native, ops
    assert literalkg_amd.score_pairs_mlp is pairmlp.score_pairs_mlp
    assert literalkg_amd.evaluate_mlp_classification is pairmlp.evaluate_mlp_classification
    assert "score_pairs_mlp" in literalkg_amd.__all__ and "evaluate_mlp_classification" in literalkg_amd.__all__
    assert list(inspect.signature(score_pairs_mlp).parameters) == ["model", "h", "t", "logits", "batch_size"]
    assert list(inspect.signature(literalkg_amd.LiteralKG.score_pairs).parameters)[1:] == \
        list(inspect.signature(score_pairs_mlp).parameters)[1:]
    assert list(inspect.signature(evaluate_mlp_classification).parameters) == [
        "model", "h", "t", "labels", "threshold", "logit_threshold", "batch_size"]
    sig = inspect.signature(evaluate_mlp_classification).parameters
    assert sig["threshold"].default == 0.5 and sig["logit_threshold"].default is None
    assert list(inspect.signature(ops.pair_mlp_pairs).parameters)[:11] == [
        "u", "v", "w2", "b2", "w3", "b3", "u_idx", "v_idx", "labels", "thr", "want_logits"]
    assert list(inspect.signature(ops.binary_curve).parameters) == ["scores", "labels"]
    for name in ("lkg_pair_mlp_pairs_f32", "lkg_binary_curve_f32", "lkg_binary_curve_workspace"):
        assert name in _native.PROTOTYPES


def test_metrics_follow_the_reference_conventions():
    """classification_metrics against hand-worked numbers: accuracy over all pairs (NaN is wrong), zero conventions"""
    d = pairmlp.classification_metrics(3, 1, 4, 2, 1, 6, 5, (5, 5, 1, 7, 30, 0.625))
    assert d["n"] == 11 and d["accuracy"] == 7 / 11 and d["precision"] == 3 / 4 and d["recall"] == 3 / 5
    assert d["f1"] == (2.0 * (3 / 4) * (3 / 5)) / ((3 / 4) + (3 / 5)) and d["roc_auc"] == 30 / 50
    assert d["average_precision"] == 0.625 and d["n_pos"] == 6 and d["n_neg"] == 5
    d = pairmlp.classification_metrics(0, 0, 4, 2, 0, 2, 4, (2, 4, 0, 3, 9, 0.4))
    assert d["precision"] == 0 and d["recall"] == 0 and d["f1"] == 0 and d["accuracy"] == 4 / 6
    d = pairmlp.classification_metrics(0, 3, 2, 0, 0, 0, 5, (0, 5, 0, 2, 0, 0.0))          # an empty class
    assert math.isnan(d["roc_auc"]) and math.isnan(d["average_precision"]) and d["accuracy"] == 2 / 5


# ----------------------------------------------------------------------------- the references, and planted faults
def restated(scores, labels, thr, fault=None):
    """The definitions once more, element by element in plain Python -- with a switch for each planted fault.
    Returns (tp, fp, tn, fn, nan), (n_pos, n_neg, n_nan, n_groups, auc2, ap)."""
    s32 = np.asarray(scores, dtype=np.float32)
    items = [(float(s), int(y)) for s, y in zip(s32.tolist(), labels)]
    thr = float(np.float32(thr))
    conf = [0, 0, 0, 0, 0]
    for s, y in items:
        if math.isnan(s):
            if fault == "nan_is_negative":
                conf[3 if y else 2] += 1
            else:
                conf[4] += 1
            continue
        pos = s >= thr if fault == "ge_threshold" else s > thr
        conf[(0 if y else 1) if pos else (3 if y else 2)] += 1
    if fault == "nan_is_negative":
        live = [(-math.inf if math.isnan(s) else s, y) for s, y in items]
    else:
        live = [(s, y) for s, y in items if not math.isnan(s)]

    def key(s):                       # the order of the scores; the fault orders -0.0 strictly below +0.0
        if fault == "signed_zero" and s == 0.0:
            return (0.0, math.copysign(1.0, s))
        return (s, 0.0)
    n_pos = sum(y for _, y in live)
    n_neg = len(live) - n_pos
    auc2 = 0
    for si, yi in live:
        if yi:
            for sj, yj in live:
                if not yj:
                    if key(sj) < key(si):
                        auc2 += 2
                    elif key(sj) == key(si):
                        auc2 += 2 if fault == "ties_win" else 1
    ordered = sorted(live, key=lambda it: key(it[0]), reverse=True)
    ap, tp, prev = Fraction(0), 0, 0
    n_groups = 0
    for k, (s, y) in enumerate(ordered):
        tp += y
        last = k == len(ordered) - 1 or key(ordered[k + 1][0]) != key(s)
        n_groups += last
        if last or fault == "ap_every_element":
            if n_pos:
                ap += Fraction(tp - prev, n_pos) * Fraction(tp, k + 1)
            prev = tp
    return tuple(conf), (n_pos, n_neg, len(items) - len(live), n_groups, auc2, ap)


def fault_cases():
    rng = np.random.default_rng(11)
    inf, nan = math.inf, math.nan
    yield [0.5, -0.0, 0.0, 0.0, -0.0, 1.5, -2.0], [1, 1, 0, 1, 0, 0, 1], 0.0
    yield [0.25, 0.25, 0.25, nan, 0.25, -1.0, nan, 3.0], [1, 0, 1, 1, 0, 1, 0, 0], 0.25
    yield [inf, -inf, 0.0, inf, -inf, 1e-45, -1e-45], [1, 0, 1, 0, 1, 0, 1], -inf
    for n in (1, 2, 40, 200):
        s = rng.integers(-3, 4, n).astype(np.float32) / 2
        s[rng.random(n) < 0.1] = nan
        s[rng.random(n) < 0.1] = -0.0
        yield s.tolist(), rng.integers(0, 2, n).tolist(), float(s[0]) if not math.isnan(s[0]) else 0.5
    yield rng.standard_normal(300).astype(np.float32).tolist(), rng.integers(0, 2, 300).tolist(), 0.1
    yield [1.0, 2.0, 3.0], [1, 1, 1], 2.0
    yield [1.0, 1.0, 3.0], [0, 0, 0], 1.0
    yield [], [], 0.0


def test_references_accept_a_correct_restatement():
    for s, y, thr in fault_cases():
        conf, curve = restated(s, y, thr)
        assert PC.confusion_counts(s, y, thr) == conf, (s, y, thr)
        assert PC.curve_reference(s, y) == curve, (s, y)
        assert PC.curve_reference(s, y, small=0)[4] == curve[4], (s, y)              # the sorting form of auc2 too
        if len(s):
            assert PC.auc2_by_definition(s, y) == PC.auc2_by_sorting(s, y) == curve[4]


@pytest.mark.parametrize("fault,part", [("ties_win", "auc2"), ("signed_zero", "curve"), ("nan_is_negative", "both"),
                                        ("ge_threshold", "counts"), ("ap_every_element", "ap")])
def test_references_reject_a_planted_fault(fault, part):
    hit = {"counts": 0, "auc2": 0, "ap": 0, "groups": 0}
    for s, y, thr in fault_cases():
        conf, curve = restated(s, y, thr, fault)
        want = PC.curve_reference(s, y)
        hit["counts"] += PC.confusion_counts(s, y, thr) != conf
        hit["auc2"] += want[4] != curve[4]
        hit["ap"] += want[5] != curve[5]
        hit["groups"] += want[3] != curve[3]
    if part == "auc2":
        assert hit["auc2"] and not hit["counts"]
    elif part == "curve":
        assert hit["auc2"] and hit["ap"] and hit["groups"] and not hit["counts"]
    elif part == "both":
        assert hit["counts"] and hit["auc2"] and hit["ap"]
    elif part == "counts":
        assert hit["counts"] and not (hit["auc2"] or hit["ap"] or hit["groups"])
    else:
        assert hit["ap"] and not (hit["counts"] or hit["auc2"] or hit["groups"])
