"""Numpy references of relation prediction (literalkg_amd/relations.py), by definition: from a P x R matrix of float32
scores and the known relations of every pair as Python sets, the filtered better / equal counts of a true relation, the
filtered top-k, and the metrics overall and per relation.  Lower is better; ties by float equality (-0.0 == +0.0), to the
smaller relation id in the top-k; a NaN score counts nowhere and is never listed; a NaN truth compares false everywhere."""
import numpy as np


def known_sets(h, t, kh, kr, kt):
    """Per pair (h_i, t_i) the set of relations r' with (h_i, r', t_i) among the known triples (duplicates merge)."""
    by_pair = {}
    for a, b, c in zip(np.asarray(kh).tolist(), np.asarray(kr).tolist(), np.asarray(kt).tolist()):
        by_pair.setdefault((a, c), set()).add(b)
    return [by_pair.get((a, b), set()) for a, b in zip(np.asarray(h).tolist(), np.asarray(t).tolist())]


def counts(scores, truth, known=None):
    """(better, equal) int64[P]: the relations r' != truth[i], not in known[i], with score < / == the truth's."""
    scores = np.asarray(scores, dtype=np.float32)
    p, n_rel = scores.shape
    better, equal = np.zeros(p, dtype=np.int64), np.zeros(p, dtype=np.int64)
    idx = np.arange(n_rel)
    for i in range(p):
        keep = idx != truth[i]
        if known is not None and known[i]:
            keep &= ~np.isin(idx, list(known[i]))
        ts = scores[i, truth[i]]
        with np.errstate(invalid="ignore"):
            better[i] = int((scores[i, keep] < ts).sum())
            equal[i] = int((scores[i, keep] == ts).sum())
    return better, equal


def topk(scores, k, known=None):
    """(ids int64[P, k], scores float32[P, k]): the k smallest (score, id) among the relations not in known[i] whose score
    is not NaN, padded with -1 / NaN."""
    scores = np.asarray(scores, dtype=np.float32)
    p, n_rel = scores.shape
    ids = np.full((p, k), -1, dtype=np.int64)
    out = np.full((p, k), np.nan, dtype=np.float32)
    for i in range(p):
        ok = ~np.isnan(scores[i])
        if known is not None and known[i]:
            ok &= ~np.isin(np.arange(n_rel), list(known[i]))
        cand = np.nonzero(ok)[0]
        order = cand[np.argsort(scores[i, cand], kind="stable")]       # stable over ascending ids: ties to the smaller id
        order = order[:k]
        ids[i, :order.size] = order
        out[i, :order.size] = scores[i, order]
    return ids, out


def counts_brute(scores, truth, known=None):
    """counts() as a double loop of Python floats."""
    p, n_rel = len(scores), len(scores[0])
    better, equal = [0] * p, [0] * p
    for i in range(p):
        ts = float(scores[i][truth[i]])
        for j in range(n_rel):
            if j == truth[i] or (known is not None and j in known[i]):
                continue
            x = float(scores[i][j])
            better[i] += 1 if x < ts else 0
            equal[i] += 1 if x == ts else 0
    return better, equal


def topk_brute(scores, k, known=None):
    """topk() by k rounds of picking the minimum (score, id); ids and Python floats (None: padding)."""
    p, n_rel = len(scores), len(scores[0])
    ids, out = [], []
    for i in range(p):
        left = [j for j in range(n_rel) if not (known is not None and j in known[i]) and scores[i][j] == scores[i][j]]
        row_i, row_s = [], []
        for _ in range(k):
            if not left:
                row_i.append(-1)
                row_s.append(None)
                continue
            best = left[0]
            for j in left[1:]:
                if float(scores[i][j]) < float(scores[i][best]):       # strict: an equal score keeps the smaller id
                    best = j
            left.remove(best)
            row_i.append(best)
            row_s.append(float(scores[i][best]))
        ids.append(row_i)
        out.append(row_s)
    return ids, out


def metrics(better, equal, truth, n_rel, ks=(1, 3, 10)):
    """The dict of evaluate_relation_prediction: float64 of the same integers."""
    better, equal, truth = (np.asarray(x).reshape(-1).astype(np.int64) for x in (better, equal, truth))
    rank = 1.0 + better.astype(np.float64) + 0.5 * equal.astype(np.float64)
    n = rank.size
    out = {"n": n}
    per = {"n": np.bincount(truth, minlength=n_rel).astype(np.int64)}
    names = ["mr", "mrr"] + [f"hits@{k}" for k in ks]
    values = [rank, 1.0 / rank] + [(rank <= k).astype(np.float64) for k in ks]
    for name, v in zip(names, values):
        out[name] = float(v.mean()) if n else 0.0
        col = np.full(n_rel, np.nan, dtype=np.float64)
        for rho in range(n_rel):
            if per["n"][rho]:
                col[rho] = v[truth == rho].sum() / float(per["n"][rho])
        per[name] = col
    out["per_relation"] = per
    return out


def same_metrics(got, want, rel=1e-12):
    """Integers exactly; ratios as float64 of the same integers (sums of at most a few thousand terms: the order of the
    additions moves the last bits only, hence rel)."""
    assert got["n"] == want["n"]
    assert got["per_relation"]["n"].tolist() == want["per_relation"]["n"].tolist()
    for name, w in want.items():
        if name in ("n", "per_relation"):
            continue
        assert abs(got[name] - w) <= rel * max(abs(w), 1.0), (name, got[name], w)
        g = np.asarray(got["per_relation"][name], dtype=np.float64)
        wp = want["per_relation"][name]
        assert g.dtype == np.float64 and np.array_equal(np.isnan(g), np.isnan(wp)), name
        ok = ~np.isnan(wp)
        assert np.all(np.abs(g[ok] - wp[ok]) <= rel * np.maximum(np.abs(wp[ok]), 1.0)), (name, g, wp)
