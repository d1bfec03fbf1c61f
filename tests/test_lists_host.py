"""CPU tier of ranking against per-query candidate lists (literalkg_amd/lists.py: score_lists, rank_in_lists,
evaluate_list_ranking; include/literalkg_hip.h; the device tier is test_lists_gpu.py): the entry points are declared,
bound and exported; the reference of list_cases.py is what it says on a hand-written
case and its comparator rejects every planted fault; every argument error is raised before any device work."""
import os
from types import SimpleNamespace

import pytest
import torch

import list_cases as LC
from test_topk_gpu import StandIn

NAMES = ["lkg_list_count_f32", "lkg_list_scores_f32"]
NAN = float("nan")


# ----------------------------------------------------------------------------- the entry points and the package
def test_the_entry_points_are_declared_and_bound_and_the_package_exports_the_api():
    import __graft_entry__ as ge
    ge.build()
    from literalkg_amd import _native, build
    from wide_cases import prototypes
    assert "lkg_lists.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "lkg_lists.hip"))
    assert set(NAMES) <= set(_native.PROTOTYPES) and set(NAMES) <= set(prototypes())
    import literalkg_amd as L
    from literalkg_amd import lists
    for name in ("ListRanks", "score_lists", "rank_in_lists", "evaluate_list_ranking"):
        assert name in L.__all__ and getattr(L, name) is getattr(lists, name)
    for name in ("score_lists", "rank_in_lists", "evaluate_list_ranking"):
        assert callable(getattr(L.LiteralKG, name))


# ----------------------------------------------------------------------------- the reference on a hand-written case
# query 0: the truth inside its own list, a duplicate id (both better), an empty slot, a tie
# query 1: a NaN slot, a slot known under r[1] (dropped), a slot known under another relation only (kept), a tie, an empty slot
# query 2: a NaN truth
H_, R_, T_ = torch.tensor([1, 2, 3]), torch.tensor([0, 1, 0]), torch.tensor([4, 5, 9])
LISTS = torch.tensor([[4, 7, 7, -1, 9],
                      [3, 6, 8, 0, -1],
                      [1, 2, 3, 4, 5]])
SCORES = torch.tensor([[2.0, 1.0, 1.0, 0.0, 2.0],          # (the empty slots hold a finite, BETTER score here: a reference
                       [NAN, 0.5, 3.0, 1.5, 0.0],          #  that counted them would show it)
                       [1.0, 2.0, 3.0, 4.0, 5.0]])
TRUTH_SCORES = torch.tensor([2.0, 1.5, NAN])
KNOWN = {(2, 1, 6), (2, 0, 8), (7, 0, 1)}                  # (the last: known on the head side only)
WANT = (torch.tensor([2, 0, 0]), torch.tensor([1, 1, 0]), torch.tensor([3, 3, 5]))


def as_result(ref):
    better, equal, kept = (x.clone() for x in ref)
    return SimpleNamespace(better=better, equal=equal, kept=kept, rank=1.0 + better.double() + 0.5 * equal.double())


def test_the_reference_is_what_it_says():
    keep = LC.keep_mask(LISTS, T_, H_, R_, KNOWN, "tail")
    assert keep.tolist() == [[False, True, True, False, True], [True, False, True, True, False], [True] * 5]
    got = LC.counts(SCORES, TRUTH_SCORES, keep)
    assert all(torch.equal(g, w) for g, w in zip(got, WANT))
    # no filter: the known slot of query 1 is better than its truth
    free = LC.counts(SCORES, TRUTH_SCORES, LC.keep_mask(LISTS, T_))
    assert free[0].tolist() == [2, 1, 0] and free[2].tolist() == [3, 4, 5]
    # any relation: (2, 0, 8) drops slot 2 of query 1 as well
    anyrel = LC.keep_mask(LISTS, T_, H_, None, KNOWN, "tail")
    assert anyrel[1].tolist() == [True, False, False, True, False]
    # the head side reads the triples the other way round: (7, 0, 1) makes 7 a known head of query entity 1
    head = LC.keep_mask(LISTS, T_, H_, R_, KNOWN, "head")
    assert head[0].tolist() == [False, False, False, False, True] and head[1].tolist() == [True, True, True, True, False]
    # higher is better: the compare turns round, ties and NaN stay
    hi = LC.counts(SCORES, TRUTH_SCORES, keep, higher=True)
    assert hi[0].tolist() == [0, 1, 0] and hi[1].tolist() == [1, 1, 0]
    assert LC.check_ranks(as_result(WANT), WANT)
    m = LC.metrics({"tail": WANT[:2]}, ks=(1, 3))
    assert m["n"] == 3 and m["tail"]["n"] == 3 and m["mr"] == pytest.approx((3.5 + 1.5 + 1.0) / 3)
    assert m["hits@1"] == pytest.approx(1 / 3) and m["hits@3"] == pytest.approx(2 / 3)
    both = LC.metrics({"tail": WANT[:2], "head": WANT[:2]}, ks=(1,))
    assert both["n"] == 6 and both["head"] == both["tail"]


def planted_faults():
    keep = LC.keep_mask(LISTS, T_, H_, R_, KNOWN, "tail")
    full, s, t = LISTS >= 0, SCORES, TRUTH_SCORES[:, None]
    out = {}
    out["truth counted against itself"] = LC.counts(s, TRUTH_SCORES, keep | (full & (LISTS == T_[:, None])))
    out["empty slot counted"] = LC.counts(s, TRUTH_SCORES, keep | ~full)
    out["known slot kept"] = LC.counts(s, TRUTH_SCORES, LC.keep_mask(LISTS, T_))
    out["tie counted as better"] = (((s <= t) & keep).sum(1), WANT[1], WANT[2])
    out["NaN counted"] = ((~(s >= t) & keep & ~torch.isnan(t)).sum(1), WANT[1], WANT[2])
    kept = WANT[2].clone()
    kept[2] -= 1
    out["kept off by one"] = (WANT[0], WANT[1], kept)
    return out


def test_the_comparator_rejects_every_planted_fault():
    faults = planted_faults()
    assert len(faults) == 6
    for what, bad in faults.items():
        assert any(not torch.equal(b, w) for b, w in zip(bad, WANT)), what        # the fault shows in a count at all
        with pytest.raises(AssertionError):
            LC.check_ranks(as_result(bad), WANT, what)
        assert LC.check_ranks(as_result(WANT), WANT, what)                        # ... and its correct twin passes
    res = as_result(WANT)
    res.rank = res.rank + 0.5
    with pytest.raises(AssertionError, match="rank"):
        LC.check_ranks(res, WANT)
    res = as_result(WANT)
    res.kept = res.kept.to(torch.int32)
    with pytest.raises(AssertionError, match="int32"):
        LC.check_ranks(res, WANT)


# ----------------------------------------------------------------------------- argument errors, before any device work
class DeviceWork(Exception):
    pass


@pytest.fixture()
def cpu_model(monkeypatch):
    """a CPU stand-in on which any step past the argument checks raises DeviceWork"""
    import __graft_entry__ as ge
    ge.build()
    from literalkg_amd import _native, ops
    gen = torch.Generator().manual_seed(1)
    model = StandIn(torch.randn(50, 8, generator=gen), torch.randn(3, 8, generator=gen),
                    torch.randn(3, 8, 8, generator=gen), "transr")

    def refuse(*a, **k):
        raise DeviceWork()
    monkeypatch.setattr(_native, "call", refuse)
    for name in ("checked_ids", "checked_list_ids", "gather_rows", "rank_sqnorm", "rank_queries", "list_scores",
                 "list_count"):
        monkeypatch.setattr(ops, name, refuse)
    model._table_for_inference = refuse
    model.eval = lambda: model
    model.train = lambda mode=True: model
    return model


def test_argument_errors_come_before_any_device_work(cpu_model):
    import literalkg_amd as L
    m = cpu_model
    cpu = torch.device("cpu")
    ids, r, t = torch.tensor([1, 2, 3]), torch.tensor([0, 1, 2]), torch.tensor([4, 5, 6])
    lists = torch.tensor([[1, 2], [3, -1], [-1, -1]])
    good_known = SimpleNamespace(n_entities=50, device=cpu)
    bad_lists = [torch.tensor([1, 2, 3]), lists.float(), lists.int(), lists[:2], lists[:, :0], [[1, 2], [3, 4], [5, 6]], None]
    shared = [
        (dict(lists=x), ValueError) for x in bad_lists] + [
        (dict(side="both"), ValueError), (dict(side="left"), ValueError),
        (dict(scoring="nope"), ValueError), (dict(batch_size=0), ValueError), (dict(batch_size=1.5), ValueError),
        (dict(r=r[:2]), ValueError), (dict(r=r.float()), ValueError), (dict(r=None), ValueError),   # transr needs r
        (dict(r=None, scoring="transe"), ValueError),
    ]
    calls = {
        "score": (lambda a: L.score_lists(m, a.pop("ids"), a.pop("r"), a.pop("lists"), **a),
                  [(dict(ids=ids.float()), ValueError), (dict(ids=ids.reshape(3, 1)), ValueError),
                   (dict(ids=ids[:2]), ValueError)]),
        "rank": (lambda a: L.rank_in_lists(m, a.pop("ids"), a.pop("r"), t, a.pop("lists"), **a),
                 [(dict(ids=ids.float()), ValueError), (dict(ids=ids[:2]), ValueError),
                  (dict(known=SimpleNamespace(n_entities=51, device=cpu)), ValueError),
                  (dict(known=SimpleNamespace(n_entities=50, device=torch.device("cuda", 0))), ValueError)]),
    }
    for what, (fn, own) in calls.items():
        with pytest.raises(DeviceWork):                                    # good arguments get as far as the device
            fn(dict(ids=ids, r=r, lists=lists))
        with pytest.raises(DeviceWork):
            fn(dict(ids=ids, r=None, lists=lists, scoring="dot", side="head", batch_size=2))
        with pytest.raises(ValueError, match="score_pairs_mlp"):           # the pair head is refused, by name
            fn(dict(ids=ids, r=r, lists=lists, scoring="mlp"))
        for kw, exc in shared + own:
            args = dict(ids=ids, r=r, lists=lists)
            args.update(kw)
            with pytest.raises(exc):
                fn(args)
    with pytest.raises(DeviceWork):
        L.rank_in_lists(m, ids, r, t, lists, known=good_known)
    with pytest.raises(ValueError):
        L.rank_in_lists(m, ids, r, t[:2], lists)
    # score_triples' order: the scoring before the side, the side before the lists
    with pytest.raises(ValueError, match="score_pairs_mlp"):
        L.score_lists(m, ids.float(), r, lists, side="both", scoring="mlp")
    with pytest.raises(ValueError, match="side must be"):
        L.score_lists(m, ids.float(), r, lists, side="both")
    # a model without gat_trans_M has no 'transr' lists
    bare = StandIn(m.T, m.relation_embed.weight, None, "transe")
    with pytest.raises(ValueError, match="gat_trans_M"):
        L.score_lists(bare, ids, r, lists, scoring="transr")
    # the evaluation: a side at least, the ks, each list by its name, then the device
    with pytest.raises(ValueError, match="tail_lists, head_lists or both"):
        L.evaluate_list_ranking(m, ids, r, t)
    with pytest.raises(ValueError, match="Hits@k"):
        L.evaluate_list_ranking(m, ids, r, t, tail_lists=lists, ks=(0,))
    with pytest.raises(ValueError, match="head_lists"):
        L.evaluate_list_ranking(m, ids, r, t, tail_lists=lists, head_lists=lists[:2])
    with pytest.raises(ValueError, match="score_pairs_mlp"):
        L.evaluate_list_ranking(m, ids, r, t, tail_lists=lists, scoring="mlp")
    with pytest.raises(DeviceWork):
        L.evaluate_list_ranking(m, ids, r, t, tail_lists=lists, head_lists=lists, known=good_known)
    # the methods hand their arguments on
    for name in ("score_lists", "rank_in_lists", "evaluate_list_ranking"):
        assert getattr(L.LiteralKG, name).__code__.co_varnames[0] == "self"
    # empty queries need no device
    e = ids[:0]
    empty = torch.empty((0, 4), dtype=torch.int64)
    s = L.score_lists(m, e, e, empty)
    assert s.shape == (0, 4) and s.dtype == torch.float32
    res = L.rank_in_lists(m, e, e, e, empty, known=good_known)
    assert res.better.numel() == res.equal.numel() == res.kept.numel() == res.rank.numel() == 0
    assert res.better.dtype == res.kept.dtype == torch.int64 and res.rank.dtype == torch.float64 and res.side == "tail"
    out = L.evaluate_list_ranking(m, e, e, e, head_lists=empty)
    assert out["n"] == 0 and out["head"]["n"] == 0 and "tail" not in out
