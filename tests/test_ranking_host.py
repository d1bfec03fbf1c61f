"""CPU: the ranking metrics from (better, equal) counts against hand-computed values, and the argument checks of the
ranking surface that need no device (literalkg_amd/ranking.py)."""
import math
from types import SimpleNamespace

import pytest
import torch

from conftest import golden_cfg, load_golden


@pytest.fixture(scope="module")
def R():
    from literalkg_amd import ranking
    return ranking


def test_metrics_hand_computed(R):
    # ranks 1 + better + equal / 2: 1, 2.5, 4, 11, 1.5
    better = torch.tensor([0, 1, 3, 10, 0])
    equal = torch.tensor([0, 1, 0, 0, 1])
    m = R.metrics_from_counts(better, equal, (1, 3, 10, 1000))
    ranks = [1.0, 2.5, 4.0, 11.0, 1.5]
    assert m["n"] == 5
    assert m["mr"] == pytest.approx(sum(ranks) / 5, abs=0, rel=1e-15)
    assert m["mrr"] == pytest.approx(sum(1 / x for x in ranks) / 5, rel=1e-15)
    assert m["hits@1"] == pytest.approx(1 / 5)          # a tie (rank 1.5) is not a hit at 1
    assert m["hits@3"] == pytest.approx(3 / 5)
    assert m["hits@10"] == pytest.approx(4 / 5)
    assert m["hits@1000"] == 1.0                        # k larger than any rank (and than N)


def test_metrics_ties_and_empty(R):
    r = R.realistic_rank(torch.tensor([2]), torch.tensor([3]))
    assert float(r[0]) == 4.5                           # optimistic 3, pessimistic 6
    m = R.metrics_from_counts(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))
    assert m["n"] == 0 and not any(math.isnan(v) for v in m.values())
    all_tied = R.metrics_from_counts(torch.tensor([0, 0]), torch.tensor([4, 0]), (1, 3))
    assert all_tied["mr"] == 2.0 and all_tied["hits@1"] == 0.5 and all_tied["hits@3"] == 1.0


@pytest.mark.parametrize("ks", [(0,), (1, -3), (2.5,), (True,)])
def test_bad_ks(R, ks):
    with pytest.raises(ValueError):
        R.metrics_from_counts(torch.tensor([0]), torch.tensor([0]), ks)


def _cpu_model():
    import literalkg_amd as L
    gd = load_golden("encoder_gcn_l2_gatenum")
    cfg = golden_cfg(gd)
    cfg.use_num_lit = False
    return L.LiteralKG(cfg, int(gd["n"]), int(gd["n_rel"]))


def test_argument_checks_without_device(R):
    import literalkg_amd as L
    m = _cpu_model()
    ids = torch.tensor([0, 1])
    with pytest.raises(ValueError, match="side"):
        m.rank_triples(ids, ids, ids, side="middle")
    with pytest.raises(ValueError, match="scoring"):
        m.rank_triples(ids, ids, ids, scoring="distmult")
    with pytest.raises(ValueError, match="side"):
        L.evaluate_ranking(m, ids, ids, ids, side="sideways")
    with pytest.raises(ValueError, match="positive"):
        L.evaluate_ranking(m, ids, ids, ids, ks=(1, 0))
    with pytest.raises(ValueError, match="scoring"):
        L.evaluate_ranking(m, ids, ids, ids, scoring="rotate")
    with pytest.raises(ValueError, match="lengths"):
        m.rank_triples(ids, ids[:1], ids)
    with pytest.raises(ValueError, match="batch_size"):
        m.rank_triples(ids, ids, ids, batch_size=0)
    with pytest.raises(ValueError, match="batch_size"):
        m.rank_triples(ids, ids, ids, batch_size=True)      # a bool is no batch size (as for its siblings)
    assert m.training                                   # a rejected call leaves the mode alone
