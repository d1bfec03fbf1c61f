"""Numpy references for threshold retrieval (literalkg_amd/accepted.py); no library code.

A row is a dense list of candidates: ``values`` the reported scores (float32), ``keys`` the kernel scores the lists are
ordered by (float32), ``ids`` the entity ids.  Candidate c is accepted iff values[c] is not NaN, values[c] <= thr
(lower_is_better) or values[c] >= thr in float32, and ids[c] is not known for the row.  The list is ordered by ascending
key under float comparison (-0.0 == +0.0), then ascending id."""
import numpy as np


def _rows(x, dtype):
    x = np.asarray(x, dtype=dtype)
    return x[None, :] if x.ndim == 1 else x


def accepted_lists(values, keys, ids, thr, lower_is_better, known_sets=None):
    """Per row the ordered (ids int64, values float32, keys float32) of the accepted candidates.  values / keys: [N] or
    [B, N]; ids: [N]; thr: a scalar or one per row; known_sets: per row an iterable of known ids (duplicates allowed)."""
    values, keys = _rows(values, np.float32), _rows(keys, np.float32)
    ids = np.asarray(ids, dtype=np.int64)
    thr = np.broadcast_to(np.asarray(thr, dtype=np.float32), (values.shape[0],))
    out = []
    for i in range(values.shape[0]):
        v, k = values[i], keys[i]
        with np.errstate(invalid="ignore"):
            ok = ~np.isnan(v) & ((v <= thr[i]) if lower_is_better else (v >= thr[i]))
        if known_sets is not None and len(known_sets[i]):
            ok &= ~np.isin(ids, np.fromiter(set(known_sets[i]), dtype=np.int64))
        sel = np.flatnonzero(ok)
        order = np.lexsort((ids[sel], k[sel] + np.float32(0.0)))          # (-0.0 + 0.0 = +0.0: the zeros share a key)
        sel = sel[order]
        out.append((ids[sel], v[sel], k[sel]))
    return out


def accepted_lists_brute(values, keys, ids, thr, lower_is_better, known_sets=None):
    """The same lists by the definition alone: one candidate at a time, inserted where it belongs."""
    values, keys = _rows(values, np.float32), _rows(keys, np.float32)
    ids = [int(x) for x in np.asarray(ids)]
    thr = np.broadcast_to(np.asarray(thr, dtype=np.float32), (values.shape[0],))
    out = []
    for i in range(values.shape[0]):
        t = float(thr[i])
        known = set(int(x) for x in known_sets[i]) if known_sets is not None else set()
        got = []                                                          # (key, id, position), kept sorted
        for c, cid in enumerate(ids):
            v, k = float(values[i, c]), float(keys[i, c])
            if v != v:
                continue
            if not (v <= t if lower_is_better else v >= t):
                continue
            if cid in known:
                continue
            at = 0
            while at < len(got) and (got[at][0] < k or (got[at][0] == k and got[at][1] < cid)):
                at += 1
            got.insert(at, (k, cid, c))
        pos = np.array([g[2] for g in got], dtype=np.int64)
        out.append((np.array([g[1] for g in got], dtype=np.int64), values[i, pos], keys[i, pos]))
    return out


def same_lists(a, b):
    """Two results equal: ids exactly, values and keys by their bits."""
    if len(a) != len(b):
        return False
    for (ia, va, ka), (ib, vb, kb) in zip(a, b):
        if not (np.array_equal(ia, ib) and np.array_equal(va.view(np.uint32), vb.view(np.uint32))
                and np.array_equal(ka.view(np.uint32), kb.view(np.uint32))):
            return False
    return True


def flatten(lists):
    """(rowptr int64[B + 1], ids, values, keys) of per-row lists."""
    rowptr = np.zeros(len(lists) + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum([len(x[0]) for x in lists])
    cat = lambda j, dt: np.concatenate([x[j] for x in lists]).astype(dt) if lists else np.zeros(0, dt)
    return rowptr, cat(0, np.int64), cat(1, np.float32), cat(2, np.float32)
