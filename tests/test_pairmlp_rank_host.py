"""No GPU: the argument checks of rank_pairs_mlp / evaluate_mlp_ranking (literalkg_amd/pairmlp.py), which precede any
device work, the empty case and the exports."""
from types import SimpleNamespace

import pytest
import torch

from literalkg_amd import pairmlp, ranking
from literalkg_amd.pairmlp import evaluate_mlp_ranking, rank_pairs_mlp

from test_pairmlp_host import stand_in


def test_argument_errors_come_before_any_device_work():
    """everything here runs on CPU tensors: a check that reached the device code would raise RuntimeError instead"""
    m, table, gen = stand_in()
    h, t, r = torch.tensor([0, 1, 2]), torch.tensor([5, 6, 7]), torch.tensor([0, 1, 2])
    with pytest.raises(ValueError, match="side"):
        rank_pairs_mlp(m, h, t, side="left")
    with pytest.raises(ValueError, match="h must"):
        rank_pairs_mlp(m, h.float(), t)
    with pytest.raises(ValueError, match="t must"):
        rank_pairs_mlp(m, h, t.reshape(3, 1))
    with pytest.raises(ValueError, match="h must"):
        rank_pairs_mlp(m, [0, 1, 2], t)
    with pytest.raises(ValueError, match="r must"):
        rank_pairs_mlp(m, h, t, r.bool())
    with pytest.raises(ValueError, match="lengths"):
        rank_pairs_mlp(m, h, t[:2])
    with pytest.raises(ValueError, match="lengths"):
        rank_pairs_mlp(m, h, t, r[:2])
    for bs in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="batch_size"):
            rank_pairs_mlp(m, h, t, batch_size=bs)
    with pytest.raises(ValueError, match="known"):
        rank_pairs_mlp(m, h, t, known=SimpleNamespace(n_entities=m.n_entities + 1, device=torch.device("cpu")))
    with pytest.raises(ValueError, match="known triples live on"):
        rank_pairs_mlp(m, h, t, known=SimpleNamespace(n_entities=m.n_entities, device=torch.device("meta")))
    # candidate sets
    with pytest.raises(ValueError, match="candidates"):
        rank_pairs_mlp(m, h, t, candidates=torch.tensor([0.5]))
    with pytest.raises(ValueError, match="unique"):
        rank_pairs_mlp(m, h, t, candidates=torch.tensor([5, 6, 7, 5]))
    with pytest.raises(ValueError, match="2 of the 3 true tails are not among"):
        rank_pairs_mlp(m, h, t, candidates=torch.tensor([6, 9, 11]))
    with pytest.raises(ValueError, match="1 of the 3 true heads are not among"):
        rank_pairs_mlp(m, h, t, side="head", candidates=torch.tensor([0, 2, 30]))
    with pytest.raises(ValueError, match="candidates go with side"):
        rank_pairs_mlp(m, h, t, side="both", candidates=torch.tensor([5, 6, 7]))
    with pytest.raises(ValueError, match="candidates go with side"):
        evaluate_mlp_ranking(SimpleNamespace(eval=lambda: None, train=lambda mode: None, **vars(m)), h, t,
                             candidates=torch.tensor([5, 6, 7]))
    # a model without a head
    bare = SimpleNamespace(entity_embed=m.entity_embed, n_entities=m.n_entities, n_relations=3, scoring="dot",
                           training=False, _table_for_inference=m._table_for_inference)
    with pytest.raises(AttributeError, match="initialize_MLP"):
        rank_pairs_mlp(bare, h, t)
    # evaluate_mlp_ranking checks ks and side before it touches the model's mode
    for ks in ((0,), (1.5,), (True,)):
        with pytest.raises(ValueError, match="Hits@k"):
            evaluate_mlp_ranking(m, h, t, ks=ks)
    with pytest.raises(ValueError, match="side"):
        evaluate_mlp_ranking(m, h, t, side="left")
    # with valid arguments the first device op is reached -- and refuses CPU tensors: there is no fallback
    with pytest.raises(RuntimeError, match="no CPU"):
        rank_pairs_mlp(m, h, t)
    # rank_triples keeps rejecting the pair head: it has entry points of its own
    with pytest.raises(ValueError, match="scoring must be one of"):
        ranking.rank_triples(m, h, r, t, scoring="mlp")


def test_empty_input_needs_no_device():
    m, table, gen = stand_in()
    e = torch.zeros(0, dtype=torch.int64)
    for side, shape in (("tail", (0,)), ("head", (0,)), ("both", (2, 0))):
        res = rank_pairs_mlp(m, e, e, side=side)
        assert isinstance(res, ranking.RankResult) and res.side == side
        assert res.better.shape == shape == res.equal.shape == res.rank.shape
        assert res.better.dtype == torch.int64 and res.equal.dtype == torch.int64 and res.rank.dtype == torch.float64
    res = rank_pairs_mlp(m, e, e, r=e, side="tail", candidates=torch.tensor([3, 4]), batch_size=5)
    assert res.better.shape == (0,)
    modes = []
    model = SimpleNamespace(eval=lambda: modes.append("eval"), train=lambda mode: modes.append(mode), **vars(m))
    model.training = True
    out = evaluate_mlp_ranking(model, e, e, ks=(1, 10))
    assert out["n"] == 0 and out["mr"] == 0.0 and out["hits@10"] == 0.0 and out["tail"]["n"] == 0 == out["head"]["n"]
    assert modes == ["eval", True]                       # switched to eval, previous mode restored
    out = evaluate_mlp_ranking(model, e, e, side="head")
    assert set(out) == {"n", "mr", "mrr", "hits@1", "hits@3", "hits@10", "head"}


def test_exports_and_abi_names():
    import inspect

    import literalkg_amd
    from literalkg_amd import _native, ops
    assert literalkg_amd.rank_pairs_mlp is pairmlp.rank_pairs_mlp
    assert literalkg_amd.evaluate_mlp_ranking is pairmlp.evaluate_mlp_ranking
    assert "rank_pairs_mlp" in literalkg_amd.__all__ and "evaluate_mlp_ranking" in literalkg_amd.__all__
    assert hasattr(literalkg_amd.LiteralKG, "rank_pairs")
    assert list(inspect.signature(rank_pairs_mlp).parameters) == ["model", "h", "t", "r", "side", "known", "candidates",
                                                                  "batch_size"]
    assert list(inspect.signature(literalkg_amd.LiteralKG.rank_pairs).parameters)[1:] == \
        list(inspect.signature(rank_pairs_mlp).parameters)[1:]
    assert list(inspect.signature(ops.pair_mlp_rank_count).parameters)[:11] == [
        "uq", "v", "w2", "b2", "w3", "b3", "truth_rows", "filt", "filter_row", "filter_rel", "cand_ids"]
    for name in ("lkg_pair_mlp_prepare_f32", "lkg_pair_mlp_count_f32"):
        assert name in _native.PROTOTYPES
    assert ranking.SCORINGS == ("transr", "transe", "dot")
