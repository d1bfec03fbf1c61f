"""Plain numpy / Python references for the pair-head classification metrics, written from the definitions (not from the
code under test):

    confusion counts   positive iff float32(z) > float32(thr); a NaN logit is 'nan' and nothing else
    ties               by float equality (-0.0 == +0.0); NaN scores take part in nothing but n_nan
    auc2               sum over positives i of (2 #{negatives j: s_j < s_i} + #{negatives j: s_j == s_i})
    ap                 sum over the distinct scores, descending, of (TP_g - TP_(g-1)) / n_pos * TP_g / (TP_g + FP_g) with the
                       cumulative counts taken at the END of each tie group; exact, as a fractions.Fraction
"""
from fractions import Fraction

import numpy as np


def confusion_counts(z, labels, thr):
    """(tp, fp, tn, fn, nan) of float32 logits against 0 / 1 labels"""
    z = np.asarray(z, dtype=np.float32)
    y = np.asarray(labels).astype(bool)
    nan = np.isnan(z)
    with np.errstate(invalid="ignore"):
        pos = z > np.float32(thr)
    ok = ~nan
    return (int((ok & pos & y).sum()), int((ok & pos & ~y).sum()), int((ok & ~pos & ~y).sum()),
            int((ok & ~pos & y).sum()), int(nan.sum()))


def _split(scores, labels):
    s = np.asarray(scores, dtype=np.float32)
    y = np.asarray(labels).astype(bool)
    keep = ~np.isnan(s)
    return s[keep].astype(np.float64), y[keep], int((~keep).sum())       # float64 holds every float32; -0.0 == 0.0 stays


def auc2_by_definition(scores, labels):
    """O(P N): every (positive, negative) pair looked at"""
    s, y, _ = _split(scores, labels)
    pos, neg = s[y], s[~y]
    total = 0
    for sp in pos.tolist():
        total += 2 * int((neg < sp).sum()) + int((neg == sp).sum())
    return total


def auc2_by_sorting(scores, labels):
    s, y, _ = _split(scores, labels)
    neg = np.sort(s[~y])
    pos = s[y]
    below = np.searchsorted(neg, pos, side="left").astype(np.int64)
    upto = np.searchsorted(neg, pos, side="right").astype(np.int64)
    return int((2 * below + (upto - below)).sum())


def groups(scores, labels):
    """[(TP_g, FP_g)] cumulative at the end of each tie group, scores descending"""
    s, y, _ = _split(scores, labels)
    order = np.argsort(-s, kind="stable")
    s, y = s[order], y[order]
    out, tp, fp = [], 0, 0
    for k in range(len(s)):
        tp += int(y[k])
        fp += int(not y[k])
        if k == len(s) - 1 or s[k + 1] != s[k]:
            out.append((tp, fp))
    return out


def ap_exact(scores, labels):
    """the average precision as an exact Fraction (0 without positives)"""
    g = groups(scores, labels)
    n_pos = g[-1][0] if g else 0
    if n_pos == 0:
        return Fraction(0)
    terms, prev = [], 0
    for tp, fp in g:
        if tp != prev:
            terms.append(Fraction(tp - prev, n_pos) * Fraction(tp, tp + fp))
        prev = tp
    while len(terms) > 1:                 # exact in any order; pairwise keeps the denominators small for longer
        terms = [sum(terms[i:i + 2], Fraction(0)) for i in range(0, len(terms), 2)]
    return terms[0]


def curve_reference(scores, labels, small=400):
    """(n_pos, n_neg, n_nan, n_groups, auc2, ap Fraction)"""
    s, y, n_nan = _split(scores, labels)
    auc2 = auc2_by_definition(scores, labels) if len(s) <= small else auc2_by_sorting(scores, labels)
    return int(y.sum()), int((~y).sum()), n_nan, len(np.unique(s)), auc2, ap_exact(scores, labels)


def metrics_reference(z, labels, thr, curve=None):
    """the dict evaluate_mlp_classification must return for the logits z: integers from the references above, ratios as
    the reference's utils/metric_utils.py forms them (curve: curve_reference(z, labels), where the caller has it)"""
    tp, fp, tn, fn, nan = confusion_counts(z, labels, thr)
    y = np.asarray(labels).astype(bool)
    n = len(y)
    c_pos, c_neg, _, _, auc2, ap = curve if curve is not None else curve_reference(z, labels)
    precision = tp / (tp + fp) if tp + fp != 0 else 0
    recall = tp / (tp + fn) if tp + fn != 0 else 0
    f1 = (2.0 * precision * recall) / (precision + recall) if precision + recall > 0 else 0.
    both = c_pos > 0 and c_neg > 0
    return {"accuracy": (tp + tn) / n, "precision": precision, "recall": recall, "f1": f1, "tp": tp, "fp": fp, "tn": tn,
            "fn": fn, "nan": nan, "n": n, "n_pos": int(y.sum()), "n_neg": int((~y).sum()),
            "roc_auc": auc2 / (2 * c_pos * c_neg) if both else float("nan"),
            "average_precision": ap if both else float("nan")}
