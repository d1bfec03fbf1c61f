"""No GPU: the ORDER of the argument checks of the inference entry points, and the checks of the shared front end
(literalkg_amd/_queries.py) that have a contract of their own.

The other host tests inject one fault at a time.  Here every call starts with every argument wrong at once; a step names
the error that must be raised now and the repair that removes it, down to the device code's refusal of CPU tensors (there
is no fallback) and the empty return.  A message is matched by the words only its own check uses, so a check that moved in
front of another one fails its step."""
from types import SimpleNamespace

import pytest
import torch

from literalkg_amd import _queries as Q
from literalkg_amd import ops
from literalkg_amd.accepted import count_accepted, predict_accepted
from literalkg_amd.ranking import rank_triples
from literalkg_amd.relations import rank_relations
from literalkg_amd.retrieval import evaluate_retrieval, rank_answers
from literalkg_amd.topk import predict_topk
from literalkg_amd.triples import score_triples

NAN = float("nan")
DEVICE = "MI355X|no CPU"
CPU, META = torch.device("cpu"), torch.device("meta")


def stand_in(scoring="transe", n=40, c=8, n_rel=3):
    """a model without gat_trans_M whose inference table must not be asked for"""
    gen = torch.Generator().manual_seed(5)
    table = torch.randn(n, c, generator=gen)

    def no_table():
        raise AssertionError("the inference table was asked for")
    return SimpleNamespace(entity_embed=SimpleNamespace(weight=table),
                           relation_embed=SimpleNamespace(weight=torch.randn(n_rel, c, generator=gen)),
                           gat_trans_M=None, n_entities=n, n_relations=n_rel, relation_dim=c, scoring=scoring,
                           training=False, eval=lambda: None, train=lambda mode=True: None,
                           _table_for_inference=no_table)


def known(n_entities=40, n_relations=3, device=CPU):
    return SimpleNamespace(n_entities=n_entities, n_relations=n_relations, device=device)


def walk(call, state, steps):
    """Raise every step's error in turn, repairing as it goes; the state with every step repaired."""
    state = dict(state)
    for match, repair in steps:
        with pytest.raises(ValueError, match=match):
            call(**state)
        state.update(repair)
    return state


M = stand_in()
IDS, R, T = torch.tensor([0, 1, 2]), torch.tensor([0, 1, 2]), torch.tensor([3, 4, 5])
EMPTY = torch.zeros(0, dtype=torch.int64)
DUP = torch.tensor([4, 2, 4])

SCORING_STEPS = [("scoring must be one of", dict(scoring="transr"))]
IDS_R_STEPS = [("ids must be a 1-D", dict(ids=IDS)),
               ("needs the relations r", dict(r=R == 0)),
               ("r must be a 1-D", dict(r=R[:2])),
               ("ids and r have different lengths", dict(r=R))]
HRT_STEPS = [("h must be a 1-D tensor of integer ids", dict(h=IDS)),
             ("r must be a 1-D tensor of integer ids", dict(r=R)),
             ("t must be a 1-D tensor of integer ids", dict(t=T[:2])),
             ("h, r, t have different lengths", dict(t=T))]
CANDIDATE_STEPS = [("candidates must be a 1-D", dict(candidates=DUP))]
TRANSR_STEPS = [("needs a model with gat_trans_M", dict(scoring="transe"))]


def topk_like_state(**more):
    return dict(ids=IDS.float(), r=None, side="both", known=known(41, device=META), scoring="distmult",
                candidates=torch.tensor([0.5]), batch_size=0, splits=65, **more)


def test_predict_topk():
    call = lambda **kw: predict_topk(M, **kw)                                       # noqa: E731
    state = walk(call, topk_like_state(k=0),
                 [("top-k ranks one side at a time", dict(side="head"))] + SCORING_STEPS
                 + [("k must be an integer", dict(k=3))] + IDS_R_STEPS + CANDIDATE_STEPS
                 + [("batch_size must", dict(batch_size=2)), ("splits must", dict(splits=2))] + TRANSR_STEPS
                 + [("41 entities", dict(known=known(device=META))),
                    ("known triples live on", dict(known=known()))])
    # the moved candidates are checked for repeats after the ids have gone to the device: the empty return comes first
    assert state["candidates"] is DUP
    res = call(**dict(state, ids=EMPTY, r=EMPTY))
    assert res.ids.shape == (0, 3) and res.side == "head"
    with pytest.raises(RuntimeError, match=DEVICE):
        call(**state)


def test_predict_topk_with_the_pair_head():
    """scoring='mlp' takes the same checks up to the filter, then the repeats, then folds the head"""
    call = lambda **kw: predict_topk(M, **kw)                                       # noqa: E731
    state = dict(topk_like_state(k=0), scoring="mlp", r=R == 0)
    state = walk(call, state,
                 [("top-k ranks one side at a time", dict(side="tail")), ("k must be an integer", dict(k=3)),
                  ("ids must be a 1-D", dict(ids=IDS)), ("r must be a 1-D", dict(r=R[:2])),
                  ("ids and r have different lengths", dict(r=None))] + CANDIDATE_STEPS
                 + [("batch_size must", dict(batch_size=2)), ("splits must", dict(splits=2)),
                    ("41 entities", dict(known=known(device=META))),
                    ("candidates must be unique", dict(candidates=None))])
    with pytest.raises(AttributeError):                      # no head on the stand-in; the filter's device comes after
        call(**state)


@pytest.mark.parametrize("entry", [predict_accepted, count_accepted])
def test_accepted(entry):
    call = lambda **kw: entry(M, **kw)                                              # noqa: E731
    state = dict(topk_like_state(thresholds=NAN), scoring="mlp")
    steps = [("top-k ranks one side at a time", dict(side="head")),
             ("predict_topk\\(scoring='mlp'\\)", dict(scoring="distmult"))] + SCORING_STEPS + IDS_R_STEPS \
        + CANDIDATE_STEPS + [("batch_size must", dict(batch_size=2)), ("splits must", dict(splits=2))] + TRANSR_STEPS \
        + [("a threshold is NaN", dict(thresholds=1.0)), ("41 entities", dict(known=known(device=META))),
           ("candidates must be unique", dict(candidates=torch.tensor([4, 2]))),
           ("known triples live on", dict(known=known()))]
    if entry is predict_accepted:
        state["max_total"] = -1
        steps.insert(0, ("max_total must", dict(max_total=5)))
    state = walk(call, state, steps)
    res = call(**dict(state, ids=EMPTY, r=EMPTY))
    assert (res.numel() if entry is count_accepted else res.ids.numel()) == 0
    with pytest.raises(RuntimeError, match=DEVICE):
        call(**state)


@pytest.mark.parametrize("entry", [rank_answers, evaluate_retrieval])
def test_retrieval(entry):
    call = lambda **kw: entry(M, **kw)                                              # noqa: E731
    state = dict(h=IDS.float(), r=None, t=T[None], side="left", known=known(41, device=META), scoring="mlp",
                 candidates=torch.tensor([0.5]), batch_size=0, ks=(0,))
    side_words = "top-k ranks one side at a time" if entry is rank_answers else "'tail', 'head', 'both'"
    state = walk(call, state,
                 [("Hits@k needs positive integers", dict(ks=(1, 5))), (side_words, dict(side="head")),
                  ("from rank_pairs_mlp", dict(scoring="distmult"))] + SCORING_STEPS
                 + [("needs the relations r", dict(r=R == 0))] + HRT_STEPS + CANDIDATE_STEPS
                 + [("batch_size must", dict(batch_size=2))] + TRANSR_STEPS
                 + [("41 entities", dict(known=known(device=META))),
                    ("candidates must be unique", dict(candidates=torch.tensor([4, 2]))),
                    ("known triples live on", dict(known=known()))])
    res = call(**dict(state, h=EMPTY, r=EMPTY, t=EMPTY))
    assert (res["n_queries"] if entry is evaluate_retrieval else res.query.numel()) == 0
    with pytest.raises(RuntimeError, match=DEVICE):
        call(**state)


def test_retrieval_without_relations():
    """'dot' with r=None: the two id lists and their lengths stand where the triple lists stand"""
    call = lambda **kw: rank_answers(M, **kw)                                       # noqa: E731
    state = dict(h=IDS.float(), r=None, t=T[None], scoring="dot", candidates=torch.tensor([0.5]))
    state = walk(call, state, [("h must be a 1-D", dict(h=IDS)), ("t must be a 1-D", dict(t=None)),
                               ("t must be a 1-D", dict(t=T[:2])),
                               ("h and t have different lengths", dict(t=T))] + CANDIDATE_STEPS
                 + [("candidates must be unique", dict(candidates=None))])
    with pytest.raises(RuntimeError, match=DEVICE):
        call(**state)


def test_rank_triples():
    call = lambda **kw: rank_triples(M, **kw)                                       # noqa: E731
    state = dict(h=IDS[None], r=[0, 1, 2], t=T[None], side="left", known=known(41), scoring="distmult", batch_size=0)
    state = walk(call, state,
                 [("'tail', 'head', 'both'", dict(side="both"))] + SCORING_STEPS
                 + [("h must be a 1-D tensor of ids", dict(h=IDS)), ("r must be a 1-D tensor of ids", dict(r=R)),
                    ("t must be a 1-D tensor of ids", dict(t=T[:2])), ("h, r, t have different lengths", dict(t=T)),
                    ("batch_size must", dict(batch_size=2))] + TRANSR_STEPS + [("41 entities", dict(known=known()))])
    res = call(**dict(state, h=EMPTY, r=EMPTY, t=EMPTY))
    assert res.better.shape == (2, 0) and res.side == "both"
    with pytest.raises(RuntimeError, match=DEVICE):
        call(**state)


def test_score_triples():
    call = lambda **kw: score_triples(M, **kw)                                      # noqa: E731
    state = dict(h=IDS.float(), r=R == 0, t=T[None], side="both", scoring="mlp", batch_size=0)
    state = walk(call, state,
                 [("score_pairs_mlp", dict(scoring="distmult"))] + SCORING_STEPS + TRANSR_STEPS
                 + [("a triple is scored from one side at a time", dict(side="head"))] + HRT_STEPS
                 + [("batch_size must", dict(batch_size=2))])
    assert call(**dict(state, h=EMPTY, r=EMPTY, t=EMPTY)).shape == (0,)
    with pytest.raises(RuntimeError, match=DEVICE):
        call(**state)


def test_rank_relations():
    big = stand_in(n_rel=ops.RELATION_MAX + 1)
    call = lambda model, **kw: rank_relations(model, **kw)                          # noqa: E731
    state = dict(model=big, h=IDS.float(), r=R == 0, t=T[None], side="both", known=known(41, 4, META), scoring="dot",
                 batch_size=0, relation_chunk=0)
    state = walk(call, state,
                 [("does not depend on the relation", dict(scoring="mlp")),
                  ("score_pairs_mlp", dict(scoring="distmult"))] + SCORING_STEPS + TRANSR_STEPS
                 + [("a triple is scored from one side at a time", dict(side="head")),
                    ("h must be a 1-D", dict(h=IDS)), ("r must be a 1-D", dict(r=R)),
                    ("t must be a 1-D", dict(t=T[:2])), ("h, r, t have different lengths", dict(t=T)),
                    ("batch_size must", dict(batch_size=2)), ("relation_chunk must", dict(relation_chunk=1)),
                    ("in LDS", dict(model=M)), ("4 relations, the model has 3", dict(known=known(41, 3, META))),
                    ("41 entities", dict(known=known(device=META)))])
    res = call(**dict(state, h=EMPTY, r=EMPTY, t=EMPTY))           # the empty return comes before the filter's device
    assert res.better.shape == (0,) and res.side == "head"
    state = walk(call, state, [("known triples live on", dict(known=known()))])
    with pytest.raises(RuntimeError, match=DEVICE):
        call(**state)


# ----------------------------------------------------------------------------- the shared checks on their own
def test_check_one_side_carries_the_callers_words():
    for why in ("top-k ranks one side at a time", "a triple is scored from one side at a time"):
        assert Q.check_one_side("tail", why) == "tail" and Q.check_one_side("head", why) == "head"
        for bad in ("both", "left", None):
            with pytest.raises(ValueError) as err:
                Q.check_one_side(bad, why)
            assert str(err.value) == f"side must be one of ('tail', 'head') ({why}), got {bad!r}"


def test_check_splits():
    for good in (0, 1, ops.TOPK_MAX_SPLITS, 2.0):
        Q.check_splits(good)
    assert ops.TOPK_MAX_SPLITS == 64
    for bad in (-1, 65, 1.5, True):
        with pytest.raises(ValueError, match=f"splits must be an integer in \\[0, 64\\], got {bad!r}"):
            Q.check_splits(bad)


def test_resolve_scoring():
    assert Q.resolve_scoring(M, None) == "transe" and Q.resolve_scoring(M, "dot", "no pair head here") == "dot"
    with pytest.raises(ValueError, match="no pair head here"):
        Q.resolve_scoring(stand_in("mlp"), None, "no pair head here")
    with pytest.raises(ValueError, match="scoring must be one of"):
        Q.resolve_scoring(M, "mlp")


def test_rows_to_project(monkeypatch):
    """the whole table with the ids as they are, or the distinct rows with the ids renumbered into them"""
    monkeypatch.setattr(ops, "gather_rows", lambda table, ids: table[ids])         # (the device gather, in plain torch)
    table = torch.arange(12.0).reshape(6, 2)
    rowmax = table.abs().amax(1)
    qi, ci = torch.tensor([4, 1, 4]), torch.tensor([1, 5, 5])
    for project in (None, "distinct"):
        rows, rm, qj, cj = Q.rows_to_project(table, rowmax, qi, ci, project)
        assert rows.shape == (3, 2) and torch.equal(rows, table[torch.tensor([1, 4, 5])]) and torch.equal(rm, rowmax[[1, 4, 5]])
        assert torch.equal(rows[qj], table[qi]) and torch.equal(rows[cj], table[ci])
    rows, rm, qj, cj = Q.rows_to_project(table, rowmax, qi, ci, "full")
    assert rows is table and rm is rowmax and qj is qi and cj is ci
    every = torch.tensor([0, 1, 2, 3, 4, 5])                      # the distinct rows are not fewer than the table's
    rows, rm, qj, cj = Q.rows_to_project(table, rowmax, every, every.flip(0), None)
    assert rows is table and rm is rowmax and qj is every
    rows, rm, qj, cj = Q.rows_to_project(table, rowmax, every, every.flip(0), "distinct")
    assert rows is not table and torch.equal(rows, table) and torch.equal(qj, every) and torch.equal(cj, every.flip(0))
