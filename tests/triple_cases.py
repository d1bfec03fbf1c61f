"""Plain numpy references for triple classification (literalkg_amd/triples.py), written from the definitions: decisions
on a float32 score against a per-relation threshold, the exact tie-aware threshold fit by brute force over every cut, and
the metrics dict.  No device, no library."""
import math

import numpy as np


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def sentinel(lower_is_better):
    return np.float32(-np.inf if lower_is_better else np.inf)


def decisions(scores, r, labels, thr, lower_is_better, n_rel=None):
    """int64[n_rel, 5]: tp, fp, tn, fn, nan per relation.  thr: one float32 per relation (or a scalar for all).  A triple
    is positive iff score <= thr[r] (lower_is_better) / score >= thr[r]: one float32 compare; a NaN score counts in nan
    alone."""
    s, r, y = _f32(scores), np.asarray(r, dtype=np.int64), np.asarray(labels).astype(bool)
    n_rel = int(n_rel if n_rel is not None else (r.max() + 1 if r.size else 0))
    thr = np.broadcast_to(_f32(thr), (n_rel,)) if np.ndim(thr) == 0 else _f32(thr)
    out = np.zeros((n_rel, 5), dtype=np.int64)
    for i in range(s.size):
        rho = r[i]
        if np.isnan(s[i]):
            out[rho, 4] += 1
            continue
        pos = bool(s[i] <= thr[rho]) if lower_is_better else bool(s[i] >= thr[rho])
        out[rho, (0 if y[i] else 1) if pos else (3 if y[i] else 2)] += 1
    return out


def _fit_one(s, y, lower_is_better):
    """(threshold float32, correct int) over the (score, label) pairs of one relation, by the definition: every distinct
    non-NaN score is a candidate cut, correct(cut) counts by brute force; the best-first smallest maximiser wins, the cut
    before every score (the sentinel) winning a tie with any of them."""
    ok = ~np.isnan(s)
    s, y = s[ok], y[ok]
    best_thr, best = sentinel(lower_is_better), int((~y).sum())          # correct(0) = n_neg
    cuts = np.unique(s)                                                   # ascending; -0.0 and +0.0 are one value
    if not lower_is_better:
        cuts = cuts[::-1]
    for c in cuts:                                                        # best first
        pred = (s <= c) if lower_is_better else (s >= c)
        correct = int((pred == y).sum())
        if correct > best:
            best, best_thr = correct, np.float32(c) + np.float32(0.0)     # (a zero threshold is +0.0)
    return best_thr, best


def fit_by_definition(scores, r, labels, n_rel, lower_is_better):
    """{'thresholds' float32[n_rel], 'n' int64[n_rel], 'correct' int64[n_rel], 'global_threshold', 'global_correct',
    'fitted' float32[n_rel]}: O(P G) brute force.  'fitted' is every relation's own fit (the sentinel without scores);
    'thresholds' replaces it by the pooled threshold where the relation has no triple.  NaN scores count in n and are
    never correct."""
    s, r, y = _f32(scores), np.asarray(r, dtype=np.int64), np.asarray(labels).astype(bool)
    g_thr, g_correct = _fit_one(s, y, lower_is_better)
    fitted = np.empty(n_rel, dtype=np.float32)
    n = np.zeros(n_rel, dtype=np.int64)
    correct = np.zeros(n_rel, dtype=np.int64)
    for rho in range(n_rel):
        m = r == rho
        n[rho] = int(m.sum())
        fitted[rho], correct[rho] = _fit_one(s[m], y[m], lower_is_better)
    thr = np.where(n > 0, fitted, g_thr).astype(np.float32)
    return {"thresholds": thr, "n": n, "correct": correct, "global_threshold": g_thr, "global_correct": g_correct,
            "fitted": fitted}


def metrics(counts, labels, curve=None):
    """The dict evaluate_triple_classification must return from the per-relation counts of decisions() and, for the two
    curve metrics, (n_pos, n_neg, n_nan, n_groups, auc2, ap) of pair_cases.curve_reference on the plausibility."""
    counts = np.asarray(counts, dtype=np.int64)
    y = np.asarray(labels).astype(bool)
    tp, fp, tn, fn, nan = (int(x) for x in counts.sum(0))
    n = tp + fp + tn + fn + nan
    precision = tp / (tp + fp) if tp + fp != 0 else 0.0
    recall = tp / (tp + fn) if tp + fn != 0 else 0.0
    f1 = (2.0 * precision * recall) / (precision + recall) if precision + recall > 0 else 0.0
    per_n = counts.sum(1)
    accs = [(counts[i, 0] + counts[i, 2]) / per_n[i] for i in range(counts.shape[0]) if per_n[i] > 0]
    roc_auc = ap = float("nan")
    if curve is not None and curve[0] > 0 and curve[1] > 0:
        roc_auc, ap = curve[4] / (2 * curve[0] * curve[1]), curve[5]
    return {"accuracy": (tp + tn) / n if n else 0.0, "macro_accuracy": float(np.mean(accs)) if accs else 0.0,
            "precision": precision, "recall": recall, "f1": f1, "tp": tp, "fp": fp, "tn": tn, "fn": fn, "nan": nan,
            "n": n, "n_pos": int(y.sum()), "n_neg": int((~y).sum()), "roc_auc": roc_auc, "average_precision": ap,
            "per_relation": {k: counts[:, j].copy() for j, k in enumerate(("tp", "fp", "tn", "fn", "nan"))}}


COUNT_KEYS = ("tp", "fp", "tn", "fn", "nan", "n", "n_pos", "n_neg")


def same_metrics(got, want, n_groups=0):
    """got (the library's dict) against want (metrics()): integers and ratios exactly, average precision within the
    (n_groups + 4) 2^-53 relative bound of the curve kernel's float64 sum (want's may be a Fraction), NaN as NaN."""
    from fractions import Fraction
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k, w in want.items():
        g = got[k]
        if k == "per_relation":
            assert set(g) == set(w)
            for kk in w:
                assert np.array_equal(np.asarray(g[kk]), w[kk]), (kk, g[kk], w[kk])
        elif isinstance(w, float) and math.isnan(w):
            assert isinstance(g, float) and math.isnan(g), (k, g)
        elif k == "average_precision":
            assert abs(Fraction(g) - Fraction(w)) <= (n_groups + 4) * Fraction(1, 2 ** 53) * Fraction(w), (g, float(w))
        elif k == "macro_accuracy":
            assert abs(g - w) <= 4 * 2.0 ** -53 * len(want["per_relation"]["tp"]), (k, g, w)
        else:
            assert g == w and (k not in COUNT_KEYS or isinstance(g, int)), (k, g, w)
