"""References for threshold retrieval under the MLP pair head (literalkg_amd/pairmlp.py: predict_accepted_mlp,
count_accepted_mlp), written in numpy and Python, independent of the library; test_pair_accepted_host.py holds them to
planted faults, test_pair_accepted_gpu.py holds the device to them.

The object: for every query i the candidates c with z(i, c) > thr_i (one float32 compare, strict; a NaN never passes) that
are eligible (not known with the query), ordered by descending logit -- float comparison, -0.0 == +0.0 -- then ascending
entity id; in CSR form."""
from types import SimpleNamespace

import numpy as np
import torch


def accepted_lists(z, thr, cand_ids, eligible=None):
    """The reference lists.  z: B x N float32 logits (row i, column j = query i against candidate cand_ids[j]); thr: a
    float or B floats; cand_ids: N entity ids; eligible: B x N bool (None: all).  Returns rowptr int64[B + 1], counts
    int64[B], ids int64[M], logits float32[M]."""
    z = np.asarray(z)
    assert z.dtype == np.float32 and z.ndim == 2
    b, n = z.shape
    cand_ids = np.asarray(cand_ids, dtype=np.int64).reshape(-1)
    assert cand_ids.shape == (n,) and np.unique(cand_ids).size == n
    thr = np.broadcast_to(np.asarray(thr, dtype=np.float32), (b,))
    ids, logits, counts = [], [], []
    for i in range(b):
        with np.errstate(invalid="ignore"):
            keep = z[i] > thr[i]                                  # (NaN > x and x > NaN are False)
        if eligible is not None:
            keep &= np.asarray(eligible[i], dtype=bool)
        j = np.flatnonzero(keep)
        j = j[np.lexsort((cand_ids[j], -z[i, j]))]                # by -z (so -0.0 == +0.0 tie), then by id
        ids.append(cand_ids[j])
        logits.append(z[i, j])
        counts.append(j.size)
    counts = np.asarray(counts, dtype=np.int64)
    rowptr = np.zeros(b + 1, dtype=np.int64)
    np.cumsum(counts, out=rowptr[1:])
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    return SimpleNamespace(rowptr=rowptr, counts=counts, ids=cat(ids, np.int64), logits=cat(logits, np.float32))


def eligibility(queries, cand_ids, side, triples, r=None):
    """B x N bool from a Python set of known (h, r, t): side 'tail' asks about (query, r_i, c), side 'head' about
    (c, r_i, query); r None: known under ANY relation."""
    pairs = {(h, t) for h, _, t in triples}
    out = np.ones((len(queries), len(cand_ids)), dtype=bool)
    for i, q in enumerate(queries):
        for j, c in enumerate(cand_ids):
            h, t = (q, c) if side == "tail" else (c, q)
            out[i, j] = ((h, t) not in pairs) if r is None else ((h, r[i], t) not in triples)
    return out


def int_logits(uq, v, w2, b2, w3, b3):
    """n_q x n_c int64: the folded head on small-integer operands, exactly -- x1 = relu(u + v), x2 = relu(W2 x1 + b2),
    z = w3 . x2 + b3 -- in integer arithmetic."""
    uq, v, w2, b2, w3, b3 = (np.asarray(t).astype(np.int64) for t in (uq, v, w2, b2, w3, b3))
    x1 = np.maximum(uq[:, None, :] + v[None, :, :], 0)
    x2 = np.maximum(x1 @ w2.T + b2, 0)
    return x2 @ w3 + b3.reshape(-1)[0]


def _bits(x):
    x = x.detach().cpu().contiguous() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    assert x.dtype == torch.float32, x.dtype
    return x.view(torch.int32).numpy()


def reference_probabilities(logits, device="cpu"):
    """float32: the float64 sigmoid of the float32 logits, rounded once (evaluated on `device`)."""
    z = torch.from_numpy(np.ascontiguousarray(logits)).to(device)
    return torch.sigmoid(z.double()).float().cpu().numpy()


def check_lists(res, ref, what=""):
    """AssertionError unless the result (rowptr, counts, ids int64; kernel_scores = logits, scores = probabilities,
    float32) IS the reference: the same segments, the same ids in the same order, the logits and the probabilities to the
    bit."""
    head = f"{what}: " if what else ""
    for name in ("rowptr", "counts", "ids"):
        got = getattr(res, name)
        assert got.dtype == torch.int64, f"{head}{name} is {got.dtype}"
        got = got.detach().cpu().numpy()
        want = getattr(ref, name)
        assert got.shape == want.shape, f"{head}{name} has shape {got.shape}, the reference {want.shape}"
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{head}{name} differs at {bad[:5].tolist()}: {got[bad[:5]].tolist()} != {want[bad[:5]].tolist()}"
    assert res.kernel_scores.dtype == torch.float32 and res.scores.dtype == torch.float32, head + "score dtypes"
    assert tuple(res.kernel_scores.shape) == ref.logits.shape == tuple(res.scores.shape), head + "score shapes"
    bad = np.flatnonzero(_bits(res.kernel_scores) != _bits(ref.logits))
    assert bad.size == 0, f"{head}kernel_scores differ in bits at {bad[:5].tolist()}"
    probs = reference_probabilities(ref.logits, res.scores.device)
    bad = np.flatnonzero(_bits(res.scores) != _bits(probs))
    assert bad.size == 0, f"{head}scores differ in bits at {bad[:5].tolist()}"
    return True


def as_result(ref, device="cpu", side="tail", query_ids=None, r=None):
    """The reference as an object of the result's shape (tensors on `device`)."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return SimpleNamespace(rowptr=t(ref.rowptr), counts=t(ref.counts), ids=t(ref.ids), kernel_scores=t(ref.logits),
                           scores=t(reference_probabilities(ref.logits, device)), side=side, query_ids=query_ids, r=r)
