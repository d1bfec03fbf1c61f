"""Numpy references for multi-answer retrieval (literalkg_amd/retrieval.py); no library code.

A query is a dense row of candidates: ``keys`` the kernel scores (float32), ``ids`` their entity ids, ``answers`` the
query's answers (ids) and ``known`` the ids the filter drops.  The list holds every candidate whose key is not NaN and
that is an answer or not known, ordered by ascending key under float comparison (-0.0 == +0.0), then ascending id.  An
answer's ``position`` is its 1-based place in the list and ``before`` the number of non-answers ahead of it; an answer
with a NaN key has (-1, -1)."""
import math

import numpy as np


def places(keys, ids, answers, known=()):
    """{answer: (before, position)} by sorting the row: lexsort((ids, keys + 0.0))."""
    keys, ids = np.asarray(keys, dtype=np.float32), np.asarray(ids, dtype=np.int64)
    ans = np.fromiter(set(int(a) for a in answers), dtype=np.int64)
    kn = np.fromiter(set(int(x) for x in known), dtype=np.int64)
    is_ans = np.isin(ids, ans)
    assert int(is_ans.sum()) == ans.size, "an answer is not among the candidates"
    listed = ~np.isnan(keys) & (is_ans | ~np.isin(ids, kn))
    sel = np.flatnonzero(listed)
    order = sel[np.lexsort((ids[sel], keys[sel] + np.float32(0.0)))]      # (-0.0 + 0.0 = +0.0: the zeros share a key)
    ahead = np.cumsum(is_ans[order]) - is_ans[order]                       # answers strictly ahead
    out = {int(a): (-1, -1) for a in ans}
    for place, c in enumerate(order):
        if is_ans[c]:
            out[int(ids[c])] = (int(place - ahead[place]), int(place + 1))
    return out


def places_brute(keys, ids, answers, known=()):
    """The same by the definition alone: every answer against one candidate at a time."""
    keys = [float(x) for x in np.asarray(keys, dtype=np.float32)]
    ids = [int(x) for x in np.asarray(ids)]
    ans, kn = set(int(a) for a in answers), set(int(x) for x in known)
    at = {cid: c for c, cid in enumerate(ids)}
    out = {}
    for a in ans:
        ka = keys[at[a]]
        if ka != ka:
            out[a] = (-1, -1)
            continue
        before = ahead = 0
        for c, cid in enumerate(ids):
            k = keys[c]
            if k != k or cid == a or not (k < ka or (k == ka and cid < a)):
                continue
            if cid in ans:
                ahead += 1
            elif cid not in kn:
                before += 1
        out[a] = (before, 1 + before + ahead)
    return out


def query_metrics(positions, ks):
    """The per-query values in float64 from the positions of ALL the query's answers (-1: a NaN answer).  The sums are
    math.fsum: correctly rounded, so the reference's own error is one rounding per value."""
    m = len(positions)
    ps = sorted(p for p in positions if p > 0)
    out = {"m": m, "hits": [], "precision": [], "recall": [], "hit": [], "ndcg": []}
    for k in ks:
        hits = sum(1 for p in ps if p <= k)
        dcg = math.fsum(1.0 / math.log2(1.0 + p) for p in ps if p <= k)
        ideal = math.fsum(1.0 / math.log2(1.0 + i) for i in range(1, min(m, k) + 1))
        out["hits"].append(hits)
        out["precision"].append(hits / k)
        out["recall"].append(hits / m)
        out["hit"].append(1.0 if hits > 0 else 0.0)
        out["ndcg"].append(dcg / ideal if ideal > 0 else 0.0)
    out["ap"] = math.fsum((i + 1) / p for i, p in enumerate(ps)) / m
    out["rr"] = 1.0 / ps[0] if ps else 0.0
    return out


def aggregate(per_query, ks):
    """The means over the queries (math.fsum / Q) under evaluate_retrieval's names."""
    n = len(per_query)
    mean = lambda xs: math.fsum(xs) / n if n else 0.0                     # noqa: E731
    out = {}
    for j, k in enumerate(ks):
        for name in ("precision", "recall", "hit", "ndcg"):
            out[f"{name}@{k}"] = mean([q[name][j] for q in per_query])
    out["map"], out["mrr"] = mean([q["ap"] for q in per_query]), mean([q["rr"] for q in per_query])
    out["n_queries"], out["n_answers"] = n, sum(q["m"] for q in per_query)
    return out
