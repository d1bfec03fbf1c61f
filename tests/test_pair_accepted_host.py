"""CPU tier of threshold retrieval under the MLP pair head (literalkg_amd/pairmlp.py: predict_accepted_mlp,
count_accepted_mlp; include/literalkg_hip.h; the device tier is test_pair_accepted_gpu.py): the checker of
pair_accept_cases.py rejects every planted fault, every argument error is raised before any device work, and the
entry points are declared, bound and exported."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pair_accept_cases as PA
from test_pairmlp_gpu import StandIn, random_head

NAMES = ["lkg_pair_mlp_accept_append_f32", "lkg_pair_mlp_accept_count_f32", "lkg_pair_mlp_accept_emit_f32"]


# ----------------------------------------------------------------------------- the entry points and the package
def test_the_entry_points_are_declared_and_bound_and_the_package_exports_the_api():
    import __graft_entry__ as ge
    ge.build()
    from literalkg_amd import _native, build
    from wide_cases import prototypes
    assert "lkg_pairmlp.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "lkg_pairmlp.hip"))
    assert set(NAMES) <= set(_native.PROTOTYPES) and set(NAMES) <= set(prototypes())
    import literalkg_amd as L
    from literalkg_amd import pairmlp
    for name in ("predict_accepted_mlp", "count_accepted_mlp"):
        assert name in L.__all__ and getattr(L, name) is getattr(pairmlp, name)
    assert callable(L.LiteralKG.predict_accepted_pairs) and callable(L.LiteralKG.count_accepted_pairs)
    assert callable(L.AcceptedResult.pairs)


# ----------------------------------------------------------------------------- the checker and its planted faults
B, N, THR = 6, 40, np.float32(1.5)
CAND = np.arange(100, 100 + 3 * N, 3)[::-1].copy()                            # descending ids with gaps
QUERIES = [7, 8, 9, 10, 11, 12]
KNOWN = {(8, 0, int(CAND[5])), (8, 1, int(CAND[6])), (9, 0, int(CAND[0]))}


def logits():
    gen = np.random.default_rng(3)
    z = gen.integers(-4, 6, size=(B, N)).astype(np.float32) / 2                # many ties, many values equal to 1.5
    z[1, 5] = 4.0                                                              # known with query 8: would pass
    z[1, 6] = 4.5
    z[2, 3] = np.nan
    z[3, 0], z[3, 1] = 0.0, -0.0
    return z


def reference():
    z = logits()
    assert (z[0] == THR).any() and (z > THR).sum() > B
    return PA.accepted_lists(z, THR, CAND, PA.eligibility(QUERIES, CAND.tolist(), "tail", KNOWN))


def test_the_reference_is_what_it_says():
    z, ref = logits(), reference()
    assert ref.rowptr[-1] == ref.ids.size == ref.logits.size == ref.counts.sum() > 0
    assert int(CAND[5]) not in ref.ids[ref.rowptr[1]:ref.rowptr[2]].tolist()
    assert int(CAND[6]) not in ref.ids[ref.rowptr[1]:ref.rowptr[2]].tolist()
    assert not np.isnan(ref.logits).any() and (ref.logits > THR).all()
    for i in range(B):
        zz, ii = ref.logits[ref.rowptr[i]:ref.rowptr[i + 1]], ref.ids[ref.rowptr[i]:ref.rowptr[i + 1]]
        assert all(zz[j] > zz[j + 1] or (zz[j] == zz[j + 1] and ii[j] < ii[j + 1]) for j in range(len(zz) - 1))
    # zeros of either sign tie and fall back on the id
    zero = PA.accepted_lists(z[3:4, :2], -1.0, CAND[:2])
    assert zero.ids.tolist() == sorted(CAND[:2].tolist())
    assert PA.check_lists(PA.as_result(ref), ref)
    # an exact head
    gen = np.random.default_rng(5)
    uq, v = gen.integers(-3, 4, (3, 128)), gen.integers(-3, 4, (5, 128))
    w2, b2, w3, b3 = gen.integers(-2, 3, (64, 128)), gen.integers(-60, -20, 64), gen.integers(-2, 3, 64), np.array([2])
    want = PA.int_logits(uq, v, w2, b2, w3, b3)
    x1 = np.maximum(uq[1] + v[4], 0)
    assert want.shape == (3, 5) and want[1, 4] == int(np.maximum(w2 @ x1 + b2, 0) @ w3 + 2)


def _insert(ref, row, at, cid, z):
    """the reference with one more entry (cid, z) at place `at` of row `row`"""
    o = int(ref.rowptr[row]) + at
    rowptr = ref.rowptr.copy()
    rowptr[row + 1:] += 1
    counts = ref.counts.copy()
    counts[row] += 1
    return SimpleNamespace(rowptr=rowptr, counts=counts, ids=np.insert(ref.ids, o, cid),
                           logits=np.insert(ref.logits, o, np.float32(z)))


def _place(ref, row, z, cid):
    zz, ii = ref.logits[ref.rowptr[row]:ref.rowptr[row + 1]], ref.ids[ref.rowptr[row]:ref.rowptr[row + 1]]
    return sum(1 for a, b in zip(zz, ii) if a > z or (a == z and b < cid))


def planted_faults():
    z, ref = logits(), reference()
    out = {}
    # an entry dropped
    o = int(ref.rowptr[2])
    rowptr, counts = ref.rowptr.copy(), ref.counts.copy()
    rowptr[3:] -= 1
    counts[2] -= 1
    out["an entry dropped"] = SimpleNamespace(rowptr=rowptr, counts=counts, ids=np.delete(ref.ids, o),
                                              logits=np.delete(ref.logits, o))
    # two neighbours swapped (inside row 0)
    ids, lg = ref.ids.copy(), ref.logits.copy()
    assert ref.counts[0] >= 2
    ids[[0, 1]], lg[[0, 1]] = ids[[1, 0]], lg[[1, 0]]
    out["two neighbours swapped"] = SimpleNamespace(rowptr=ref.rowptr, counts=ref.counts, ids=ids, logits=lg)
    # a known candidate listed, at the place the order gives it
    out["a known candidate listed"] = _insert(ref, 1, _place(ref, 1, 4.0, int(CAND[5])), int(CAND[5]), 4.0)
    # a logit equal to the threshold listed (z >= thr instead of z > thr), at the end of its row
    j = int(np.flatnonzero(z[0] == THR)[0])
    out["a logit equal to the threshold listed"] = _insert(ref, 0, _place(ref, 0, THR, int(CAND[j])), int(CAND[j]), THR)
    # a NaN logit listed, at the head and at the end of its row
    out["a NaN logit listed first"] = _insert(ref, 2, 0, int(CAND[3]), np.nan)
    out["a NaN logit listed last"] = _insert(ref, 2, int(ref.counts[2]), int(CAND[3]), np.nan)
    return ref, out


def test_the_checker_rejects_every_planted_fault():
    ref, faults = planted_faults()
    assert len(faults) == 6
    for what, bad in faults.items():
        with pytest.raises(AssertionError):
            PA.check_lists(PA.as_result(bad), ref, what)
    # a probability off by one ulp, either way; the logits intact
    for step in (1, -1):
        res = PA.as_result(ref)
        res.scores = res.scores.clone()
        res.scores.view(torch.int32)[4] += step
        with pytest.raises(AssertionError, match="scores differ"):
            PA.check_lists(res, ref)
    # a logit off by one ulp; -0.0 for +0.0
    res = PA.as_result(ref)
    res.kernel_scores = res.kernel_scores.clone()
    res.kernel_scores.view(torch.int32)[0] += 1
    with pytest.raises(AssertionError, match="kernel_scores differ"):
        PA.check_lists(res, ref)
    for name, dt in (("ids", torch.int32), ("counts", torch.int32)):
        res = PA.as_result(ref)
        setattr(res, name, getattr(res, name).to(dt))
        with pytest.raises(AssertionError):
            PA.check_lists(res, ref)


# ----------------------------------------------------------------------------- argument errors, before any device work
class DeviceWork(Exception):
    pass


@pytest.fixture()
def cpu_model(monkeypatch):
    """a CPU stand-in with a head, on which any step past the argument checks raises DeviceWork"""
    import __graft_entry__ as ge
    ge.build()
    from literalkg_amd import _native, ops
    gen = torch.Generator().manual_seed(1)
    model = StandIn(torch.randn(50, 8, generator=gen), random_head(gen, 8, "cpu"))

    def refuse(*a, **k):
        raise DeviceWork()
    monkeypatch.setattr(_native, "call", refuse)
    monkeypatch.setattr(ops, "checked_ids", refuse)
    monkeypatch.setattr(ops, "gather_rows", refuse)
    model._table_for_inference = refuse
    return model


def test_argument_errors_come_before_any_device_work(cpu_model):
    import literalkg_amd as L
    m = cpu_model
    ids, r = torch.tensor([1, 2, 3]), torch.tensor([0, 1, 2])
    cpu = torch.device("cpu")
    for fn in (L.predict_accepted_mlp, L.count_accepted_mlp):
        with pytest.raises(DeviceWork):                                    # good arguments get as far as the device
            fn(m, ids, r)
        with pytest.raises(DeviceWork):
            fn(m, ids, None, logit_threshold=torch.zeros(3), side="head", candidates=torch.tensor([4, 5]),
               known=SimpleNamespace(n_entities=50, device=cpu), batch_size=2, splits=64)
        bad = [
            (dict(ids=ids.float()), ValueError), (dict(ids=ids.reshape(3, 1)), ValueError),           # lengths and ids
            (dict(r=r[:2]), ValueError), (dict(r=r.float()), ValueError),
            (dict(candidates=torch.tensor([[1, 2]])), ValueError), (dict(candidates=torch.tensor([1.0])), ValueError),
            (dict(side="both"), ValueError), (dict(side="left"), ValueError),
            (dict(batch_size=0), ValueError), (dict(splits=65), ValueError), (dict(splits=-1), ValueError),
            (dict(candidates=torch.tensor([4, 5, 4])), ValueError),                                   # not unique
            (dict(known=SimpleNamespace(n_entities=51, device=cpu)), ValueError),
            (dict(known=SimpleNamespace(n_entities=50, device=torch.device("cuda", 0))), ValueError),
            (dict(threshold=0.0), ValueError), (dict(threshold=1.0), ValueError), (dict(threshold=-0.2), ValueError),
            (dict(threshold=1.5), ValueError), (dict(threshold=float("nan")), ValueError),
            (dict(logit_threshold=float("nan")), ValueError),
            (dict(logit_threshold=torch.zeros(2)), ValueError), (dict(logit_threshold=torch.zeros(4)), ValueError),
            (dict(logit_threshold=torch.zeros(3, dtype=torch.float64)), ValueError),
            (dict(logit_threshold=torch.zeros(3, 1)), ValueError),
        ]
        for kw, exc in bad:
            args = dict(ids=ids, r=r)
            args.update(kw)
            with pytest.raises(exc):
                fn(m, args.pop("ids"), args.pop("r"), **args)
    for kw in (dict(buffer=-1), dict(buffer=1.5), dict(buffer=True), dict(buffer=None), dict(max_total=-1),
               dict(max_total=2.0), dict(max_total=False)):
        with pytest.raises(ValueError, match="non-negative integer"):
            L.predict_accepted_mlp(m, ids, r, **kw)
    # an in-range probability is not refused, and a logit threshold overrides a bad probability's check
    with pytest.raises(DeviceWork):
        L.predict_accepted_mlp(m, ids, r, threshold=0.999)
    with pytest.raises(DeviceWork):
        L.predict_accepted_mlp(m, ids, r, threshold=7.0, logit_threshold=float("-inf"))
    # no head: AttributeError, as fold_mlp_head raises
    bare = StandIn(m.T, {})
    for fn in (L.predict_accepted_mlp, L.count_accepted_mlp):
        with pytest.raises(AttributeError, match="no MLP head"):
            fn(bare, ids, r)
    # the order of predict_topk: the side before the lists, the head before the thresholds
    with pytest.raises(ValueError, match="side must be"):
        L.predict_accepted_mlp(m, ids.float(), r, side="both")
    with pytest.raises(AttributeError):
        L.predict_accepted_mlp(bare, ids, r, threshold=2.0)
    # empty queries need no device either
    res = L.predict_accepted_mlp(m, ids[:0], None)
    assert res.rowptr.tolist() == [0] and res.ids.numel() == 0 and res.counts.numel() == 0
    assert L.count_accepted_mlp(m, ids[:0], None).numel() == 0


def test_the_embedding_scorings_keep_refusing_the_head(cpu_model):
    import literalkg_amd as L
    with pytest.raises(ValueError, match="predict_topk"):
        L.predict_accepted(cpu_model, torch.tensor([1]), None, 0.0, scoring="mlp")
    with pytest.raises(ValueError, match="predict_topk"):
        L.count_accepted(cpu_model, torch.tensor([1]), None, 0.0, scoring="mlp")


def test_pairs_and_triples_of_a_result():
    from literalkg_amd.accepted import AcceptedResult
    i64 = lambda *x: torch.tensor(x, dtype=torch.int64)
    z = torch.zeros(4)
    for side in ("tail", "head"):
        res = AcceptedResult(i64(0, 2, 2, 4), i64(30, 31, 40, 41), z, z, i64(2, 0, 2), side, i64(5, 6, 7), None)
        h, t = res.pairs()
        q, c = (h, t) if side == "tail" else (t, h)
        assert q.tolist() == [5, 5, 7, 7] and c.tolist() == [30, 31, 40, 41]
        with pytest.raises(ValueError):
            res.triples()
        res.r = i64(1, 0, 2)
        hh, rr, tt = res.triples()
        assert torch.equal(hh, h) and torch.equal(tt, t) and rr.tolist() == [1, 1, 2, 2]
