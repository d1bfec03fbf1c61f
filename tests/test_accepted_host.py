"""CPU: threshold retrieval (literalkg_amd/accepted.py) -- the two numpy references of accepted_cases.py against each
other and against lists written out by hand, the argument checks (all of them before any device work), the empty
result, the host side of the defensive emit, and the exports."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import accepted_cases as AC
from literalkg_amd import accepted, ops
from literalkg_amd.accepted import AcceptedResult, count_accepted, predict_accepted
from literalkg_amd.triples import TripleThresholds

NAN, INF = float("nan"), float("inf")


def both(values, keys, ids, thr, lower, known=None):
    a = AC.accepted_lists(values, keys, ids, thr, lower, known)
    b = AC.accepted_lists_brute(values, keys, ids, thr, lower, known)
    assert AC.same_lists(a, b)
    return a


# ----------------------------------------------------------------------------- the references
def test_ties_at_the_threshold_nan_and_infinities():
    ids = [10, 11, 12, 13, 14, 15, 16]
    v = [1.0, 2.0, 2.0, NAN, 3.0, -INF, INF]
    (got,) = both(v, v, ids, 2.0, True)
    assert got[0].tolist() == [15, 10, 11, 12]                 # -inf first; both scores AT the threshold, by id
    assert got[1].tolist() == [-INF, 1.0, 2.0, 2.0]
    # the dot product: higher is better, the key is -2 v
    k = [-2.0 * x for x in v]
    (got,) = both(v, k, ids, 2.0, False)
    assert got[0].tolist() == [16, 14, 11, 12]
    assert got[1].tolist() == [INF, 3.0, 2.0, 2.0]


def test_signed_zeros_straddle_a_zero_threshold():
    ids = [3, 2, 1, 0]
    v = np.array([0.0, -0.0, 1e-45, -1.0], dtype=np.float32)
    for thr in (0.0, -0.0):
        (got,) = both(v, v, ids, thr, True)
        assert got[0].tolist() == [0, 2, 3]                    # the zeros tie: by id; the smallest subnormal is out
        assert np.signbit(got[1]).tolist() == [True, True, False]        # each keeps its own bits
    (got,) = both(v, -2.0 * v, ids, -0.0, False)
    assert got[0].tolist() == [1, 2, 3]


def test_sentinels():
    ids = list(range(6))
    v = [5.0, NAN, 0.0, INF, 7.0, 1.0]
    (none,) = both(v, v, ids, -INF, True)
    assert none[0].size == 0 and none[1].dtype == np.float32
    (every,) = both(v, v, ids, INF, True)
    assert every[0].tolist() == [2, 5, 0, 4, 3]                # every candidate that is not NaN, +inf included
    k = [-2.0 * x for x in v]
    (none,) = both([5.0, NAN, 0.0, 7.0], k[:3] + [-14.0], ids[:4], INF, False)
    assert none[0].size == 0
    (every,) = both(v, k, ids, -INF, False)
    assert every[0].tolist() == [3, 4, 0, 5, 2]


def test_known_rows_and_duplicates_in_the_known_list():
    ids = [4, 9, 2, 7]
    v = [[1.0, 2.0, 3.0, 4.0], [1.0, 2.0, 3.0, 4.0], [4.0, 3.0, 2.0, 1.0]]
    known = [[4, 9, 2, 7, 9, 9], [], [7, 7, 2, 100]]           # row 0: everything known; duplicates change nothing
    got = both(v, v, ids, [10.0, 2.5, 3.5], True, known)
    assert got[0][0].size == 0
    assert got[1][0].tolist() == [4, 9]
    assert got[2][0].tolist() == [9]
    assert AC.same_lists(got, both(v, v, ids, [10.0, 2.5, 3.5], True, [set(k) for k in known]))
    rowptr, fi, fv, fk = AC.flatten(got)
    assert rowptr.tolist() == [0, 0, 2, 3] and fi.tolist() == [4, 9, 9] and fv.tolist() == [1.0, 2.0, 3.0]


@pytest.mark.parametrize("seed", range(6))
def test_references_agree_on_random_integer_rows(seed):
    rng = np.random.default_rng(seed)
    b, n = 5, 40
    ids = rng.permutation(200)[:n]
    v = rng.integers(-3, 4, (b, n)).astype(np.float32)
    v[rng.random((b, n)) < 0.1] = NAN
    v[rng.random((b, n)) < 0.05] = -0.0
    lower = bool(seed % 2)
    k = v if lower else -2.0 * v
    thr = rng.integers(-2, 3, b).astype(np.float32)
    known = [rng.choice(ids, rng.integers(0, 15)).tolist() for _ in range(b)]        # (with repeats)
    got = both(v, k, ids, thr, lower, known)
    for i, (gi, gv, gk) in enumerate(got):
        assert len(set(gi.tolist())) == gi.size and not set(gi.tolist()) & set(known[i])
        assert bool(np.all(gv <= thr[i])) if lower else bool(np.all(gv >= thr[i]))
        assert bool(np.all(np.diff(gk) >= 0))
    assert sum(g[0].size for g in got) > 0


# ----------------------------------------------------------------------------- the front end
def stand_in(scoring="transe", n=40, c=8, n_rel=3, trans=False):
    gen = torch.Generator().manual_seed(5)
    table = torch.randn(n, c, generator=gen)

    def no_table():
        raise AssertionError("the inference table was asked for")
    return SimpleNamespace(entity_embed=SimpleNamespace(weight=table),
                           relation_embed=SimpleNamespace(weight=torch.randn(n_rel, c, generator=gen)),
                           gat_trans_M=torch.randn(n_rel, c, c, generator=gen) if trans else None,
                           n_entities=n, n_relations=n_rel, relation_dim=c, scoring=scoring, training=False,
                           _table_for_inference=no_table)


def test_argument_errors_come_before_any_device_work():
    """everything here runs on CPU tensors: a check that reached the device code would raise RuntimeError instead"""
    m = stand_in()
    ids, r = torch.tensor([0, 1, 2]), torch.tensor([0, 1, 2])
    for call in (lambda *a, **kw: predict_accepted(m, *a, **kw), lambda *a, **kw: count_accepted(m, *a, **kw)):
        with pytest.raises(ValueError, match="side"):
            call(ids, r, 1.0, side="both")
        with pytest.raises(ValueError, match="predict_topk\\(scoring='mlp'\\)"):
            call(ids, r, 1.0, scoring="mlp")
        with pytest.raises(ValueError, match="scoring"):
            call(ids, r, 1.0, scoring="distmult")
        with pytest.raises(ValueError, match="1-D"):
            call(ids.float(), r, 1.0)
        with pytest.raises(ValueError, match="1-D"):
            call(ids[None], r, 1.0)
        with pytest.raises(ValueError, match="1-D"):
            call(ids, r == 0, 1.0)
        with pytest.raises(ValueError, match="different lengths"):
            call(ids, r[:2], 1.0)
        with pytest.raises(ValueError, match="needs the relations"):
            call(ids, None, 1.0)
        with pytest.raises(ValueError, match="1-D"):
            call(ids, r, 1.0, candidates=torch.tensor([0.5]))
        with pytest.raises(ValueError, match="unique"):
            call(ids, r, 1.0, candidates=torch.tensor([4, 2, 4]))
        with pytest.raises(ValueError, match="batch_size"):
            call(ids, r, 1.0, batch_size=0)
        for splits in (-1, 65, 1.5):
            with pytest.raises(ValueError, match="splits"):
                call(ids, r, 1.0, splits=splits)
        with pytest.raises(ValueError, match="gat_trans_M"):
            call(ids, r, 1.0, scoring="transr")
        with pytest.raises(ValueError, match="41 entities"):
            call(ids, r, 1.0, known=SimpleNamespace(n_entities=41, device=torch.device("cpu")))
        with pytest.raises(ValueError, match="known triples live on"):
            call(ids, r, 1.0, known=SimpleNamespace(n_entities=40, device=torch.device("meta")))
        # the thresholds, through triples.threshold_list
        with pytest.raises(ValueError, match="NaN"):
            call(ids, r, NAN)
        with pytest.raises(ValueError, match="NaN"):
            call(ids, r, torch.tensor([1.0, NAN, 2.0]))
        with pytest.raises(ValueError, match="3 elements"):
            call(ids, r, torch.tensor([1.0, 2.0]))
        with pytest.raises(ValueError, match="float32"):
            call(ids, r, torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64))
        with pytest.raises(ValueError, match="thresholds must be"):
            call(ids, r, "high")
        with pytest.raises(ValueError, match="thresholds must be"):
            call(ids, r, True)
        fitted = TripleThresholds(torch.zeros(3), 0.0, "dot", torch.zeros(3, dtype=torch.int64),
                                  torch.zeros(3, dtype=torch.int64))
        with pytest.raises(ValueError, match="fitted on scoring='dot'"):
            call(ids, r, fitted)
        # 'dot' without relations: one float only
        with pytest.raises(ValueError, match="one float"):
            call(ids, None, torch.zeros(3), scoring="dot")
        with pytest.raises(ValueError, match="one float"):
            call(ids, None, fitted, scoring="dot")
    for bad in (-1, 1.5, True, None):
        with pytest.raises(ValueError, match="max_total"):
            predict_accepted(m, ids, r, 1.0, max_total=bad)
    # past the checks the device code refuses CPU tensors: there is no fallback
    with pytest.raises(RuntimeError, match="MI355X"):
        predict_accepted(m, ids, r, 1.0)


def test_empty_queries():
    e = torch.zeros(0, dtype=torch.int64)
    for scoring, trans in (("transe", False), ("transr", True), ("dot", False)):
        m = stand_in(scoring, trans=trans)
        res = predict_accepted(m, e, e, 1.0)
        assert isinstance(res, AcceptedResult) and res.side == "tail"
        assert res.rowptr.tolist() == [0] and res.rowptr.dtype == torch.int64
        assert res.ids.shape == (0,) and res.ids.dtype == torch.int64
        assert res.scores.shape == (0,) and res.scores.dtype == torch.float32
        assert res.kernel_scores.shape == (0,) and res.kernel_scores.dtype == torch.float32
        assert res.counts.shape == (0,) and res.counts.dtype == torch.int64
        h, r, t = res.triples()
        assert h.numel() == r.numel() == t.numel() == 0
        n = count_accepted(m, e, e, 1.0, side="head")
        assert n.shape == (0,) and n.dtype == torch.int64
    res = predict_accepted(stand_in("dot"), e, None, 0.5)
    assert res.rowptr.tolist() == [0]
    with pytest.raises(ValueError, match="r=None"):
        res.triples()


def test_triples_of_a_result():
    """AcceptedResult.triples() repeats every query over its list, on the side it was asked from."""
    mk = lambda side: AcceptedResult(torch.tensor([0, 2, 2, 3]), torch.tensor([7, 8, 9]), torch.zeros(3), torch.zeros(3),
                                     torch.tensor([2, 0, 1]), side, torch.tensor([1, 2, 3]), torch.tensor([0, 1, 0]))
    h, r, t = mk("tail").triples()
    assert (h.tolist(), r.tolist(), t.tolist()) == ([1, 1, 3], [0, 0, 0], [7, 8, 9])
    h, r, t = mk("head").triples()
    assert (h.tolist(), r.tolist(), t.tolist()) == ([7, 8, 9], [0, 0, 0], [1, 1, 3])


def test_a_raised_emit_flag_is_an_error():
    """The emit kernel never stores outside a row's counted range; it raises a flag instead, which the wrapper turns
    into an error (the flag is fed in directly: nothing on the device is made to disagree)."""
    ops.accept_check_flag(torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="count pass had not counted"):
        ops.accept_check_flag(torch.ones(1, dtype=torch.int32))


def test_exports():
    import literalkg_amd as L
    for name in ("predict_accepted", "count_accepted", "AcceptedResult"):
        assert name in L.__all__ and getattr(L, name) is getattr(accepted, name)
    assert callable(L.LiteralKG.predict_accepted) and callable(L.LiteralKG.count_accepted)
