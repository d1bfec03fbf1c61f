"""CPU: the argument checks of the top-k surface (literalkg_amd/topk.py) that need no device."""
import pytest
import torch

from conftest import golden_cfg, load_golden


def _cpu_model():
    import literalkg_amd as L
    gd = load_golden("encoder_gcn_l2_gatenum")
    cfg = golden_cfg(gd)
    cfg.use_num_lit = False
    return L.LiteralKG(cfg, int(gd["n"]), int(gd["n_rel"]))


def test_exports():
    import literalkg_amd as L
    assert "predict_topk" in L.__all__ and "TopKResult" in L.__all__
    assert callable(L.LiteralKG.predict_topk)


@pytest.mark.parametrize("k", [0, 129, -1, 2.5, True, "10"])
def test_bad_k(k):
    m = _cpu_model()
    ids = torch.tensor([0, 1])
    with pytest.raises(ValueError, match="k must"):
        m.predict_topk(ids, ids, k=k)


def test_argument_checks_without_device():
    import literalkg_amd as L
    m = _cpu_model()
    ids = torch.tensor([0, 1])
    with pytest.raises(ValueError, match="side"):
        m.predict_topk(ids, ids, side="both")
    with pytest.raises(ValueError, match="side"):
        L.predict_topk(m, ids, ids, side="middle")
    with pytest.raises(ValueError, match="scoring"):
        m.predict_topk(ids, ids, scoring="distmult")
    with pytest.raises(ValueError, match="needs the relations"):
        m.predict_topk(ids, None, scoring="transr")
    with pytest.raises(ValueError, match="needs the relations"):
        m.predict_topk(ids, None, scoring="transe")
    with pytest.raises(ValueError, match="lengths"):
        m.predict_topk(ids, ids[:1])
    with pytest.raises(ValueError, match="1-D"):
        m.predict_topk(ids.view(1, 2), ids.view(1, 2))
    with pytest.raises(ValueError, match="1-D"):
        m.predict_topk(ids.float(), ids)
    with pytest.raises(ValueError, match="1-D"):
        m.predict_topk(ids, ids, candidates=torch.tensor([[0, 1]]))
    with pytest.raises(ValueError, match="batch_size"):
        m.predict_topk(ids, ids, batch_size=0)
    with pytest.raises(ValueError, match="splits"):
        m.predict_topk(ids, ids, splits=65)
    with pytest.raises(ValueError, match="splits"):
        m.predict_topk(ids, ids, splits=-1)
    assert m.training                                   # a rejected call leaves the mode alone


def test_known_over_other_entities_is_rejected():
    from types import SimpleNamespace
    m = _cpu_model()
    ids = torch.tensor([0, 1])
    other = SimpleNamespace(n_entities=m.n_entities + 1, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="entities"):
        m.predict_topk(ids, ids, known=other)


def test_empty_query_set_without_device():
    m = _cpu_model()
    e = torch.zeros(0, dtype=torch.int64)
    res = m.predict_topk(e, e, k=7)
    assert res.ids.shape == (0, 7) and res.scores.shape == (0, 7) and res.side == "tail"
    assert res.ids.dtype == torch.int64 and res.scores.dtype == torch.float32
