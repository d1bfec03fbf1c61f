"""No GPU: folding the MLP pair head (literalkg_amd/pairmlp.py) and the argument checks that precede any device work."""
from types import SimpleNamespace

import pytest
import torch

import oracle.literalkg_oracle as O
from literalkg_amd import pairmlp, ranking
from literalkg_amd.pairmlp import fold_mlp_head, fold_mlp_head_f64, mlp_scores
from literalkg_amd.topk import predict_topk


def make_head(seed, c, h1=128, h2=64):
    """random parameters with non-trivial affine terms and running statistics"""
    gen = torch.Generator().manual_seed(seed)
    m = SimpleNamespace(fc1=torch.nn.Linear(2 * c, h1), norm1=torch.nn.BatchNorm1d(h1), fc2=torch.nn.Linear(h1, h2),
                        norm2=torch.nn.BatchNorm1d(h2), fc3=torch.nn.Linear(h2, 1))
    with torch.no_grad():
        for fc in (m.fc1, m.fc2, m.fc3):
            torch.nn.init.xavier_uniform_(fc.weight, generator=gen)
            fc.bias.copy_(0.2 * torch.randn(fc.bias.shape, generator=gen))
        for bn in (m.norm1, m.norm2):
            d = bn.num_features
            bn.weight.copy_(0.5 + torch.rand(d, generator=gen))
            bn.bias.copy_(0.3 * torch.randn(d, generator=gen))
            bn.running_mean.copy_(0.2 + 0.2 * torch.randn(d, generator=gen))
            bn.running_var.copy_(0.3 + 1.5 * torch.rand(d, generator=gen))
    return m, gen


def stand_in(seed=3, n=50, c=12):
    m, gen = make_head(seed, c)
    table = torch.nn.functional.normalize(torch.randn(n, c, generator=gen), dim=1)
    m.entity_embed = SimpleNamespace(weight=table)
    m.n_entities, m.n_relations, m.scoring, m.training = n, 3, "dot", False
    m._table_for_inference = lambda: table
    return m, table, gen


@pytest.mark.parametrize("c", [12, 37])
def test_fold_is_the_rounded_float64_fold_and_reproduces_the_head(c):
    m, gen = make_head(c, c)
    d = lambda t: t.detach().double()
    w1, w2, w3 = d(m.fc1.weight), d(m.fc2.weight), d(m.fc3.weight).reshape(-1)
    a1 = d(m.norm1.weight) / torch.sqrt(d(m.norm1.running_var) + m.norm1.eps)
    c1 = d(m.norm1.bias) - d(m.norm1.running_mean) * a1
    a2 = d(m.norm2.weight) / torch.sqrt(d(m.norm2.running_var) + m.norm2.eps)
    c2 = d(m.norm2.bias) - d(m.norm2.running_mean) * a2
    want = dict(w1h=w1[:, :c], w1t=w1[:, c:], b1=d(m.fc1.bias), w2=w2 * a1[None, :],
                b2=(w2 * c1[None, :]).sum(dim=1) + d(m.fc2.bias), w3=w3 * a2,
                b3=((w3 * c2).sum() + d(m.fc3.bias).reshape(())).reshape(1))
    got = fold_mlp_head(m)
    for name, w in want.items():
        g = getattr(got, name)
        assert g.dtype == torch.float32 and g.is_contiguous() and g.shape == w.shape, name
        assert torch.equal(g, w.to(torch.float32)), name                 # the float64 value, rounded once
    assert float((got.w2.double() - d(m.fc2.weight)).abs().max()) > 1e-3       # (the fold is not the identity)
    # the float64 fold reproduces the unfolded head in float64
    n = 200
    gat = torch.nn.functional.normalize(torch.randn(n, c, generator=gen), dim=1).double()
    h, t = (torch.randint(0, n, (500,), generator=gen) for _ in range(2))
    p = {f"{k}.{q}": d(v) for k in ("fc1", "fc2", "fc3", "norm1", "norm2")
         for q, v in list(getattr(m, k).named_parameters()) + list(getattr(m, k).named_buffers()) if v.is_floating_point()}
    prob = O.mlp_head(p, gat, h, t, training=False).reshape(-1)
    f = fold_mlp_head_f64(m)
    x1 = (gat[h] @ f[0].T + f[2] + gat[t] @ f[1].T).clamp_min(0)
    z = (x1 @ f[3].T + f[4]).clamp_min(0) @ f[5] + f[6]
    assert float(z.abs().max()) < 20 and float(z.abs().max()) > 0.1
    assert float((torch.sigmoid(z) - prob).abs().max()) < 1e-12
    mid = z.abs() < 5                       # where the oracle's probability still determines the logit to ~1e-14
    assert int(mid.sum()) > 400 and float((z - torch.logit(prob))[mid].abs().max()) < 1e-12


def test_fold_errors():
    m, _ = make_head(1, 8)
    del m.fc2
    with pytest.raises(AttributeError, match="initialize_MLP"):
        fold_mlp_head(m)
    m, _ = make_head(1, 8)
    m.norm1 = torch.nn.BatchNorm1d(128, track_running_stats=False)
    with pytest.raises(ValueError, match="running statistics"):
        fold_mlp_head(m)
    for h1, h2 in ((64, 64), (128, 32)):
        m, _ = make_head(1, 8, h1, h2)
        with pytest.raises(ValueError, match="128"):
            fold_mlp_head(m)
    m, _ = make_head(1, 8)
    m.fc3 = torch.nn.Linear(64, 2)
    with pytest.raises(ValueError):
        fold_mlp_head(m)


def test_argument_errors_come_before_any_device_work():
    """everything here runs on CPU tensors: a check that reached the device code would raise RuntimeError instead"""
    m, table, gen = stand_in()
    ids, r = torch.tensor([0, 1, 2]), torch.tensor([0, 1, 2])
    kw = dict(scoring="mlp")
    with pytest.raises(ValueError, match="side"):
        predict_topk(m, ids, r, side="both", **kw)
    for k in (0, 129, 2.0, True):
        with pytest.raises(ValueError, match="k must"):
            predict_topk(m, ids, r, k=k, **kw)
    with pytest.raises(ValueError, match="ids"):
        predict_topk(m, ids.float(), r, **kw)
    with pytest.raises(ValueError, match="ids"):
        predict_topk(m, ids.reshape(3, 1), r, **kw)
    with pytest.raises(ValueError, match="lengths"):
        predict_topk(m, ids, r[:2], **kw)
    with pytest.raises(ValueError, match="candidates"):
        predict_topk(m, ids, r, candidates=torch.tensor([0.5]), **kw)
    with pytest.raises(ValueError, match="unique"):
        predict_topk(m, ids, None, candidates=torch.tensor([4, 2, 4]), **kw)
    with pytest.raises(ValueError, match="batch_size"):
        predict_topk(m, ids, r, batch_size=0, **kw)
    with pytest.raises(ValueError, match="splits"):
        predict_topk(m, ids, r, splits=65, **kw)
    with pytest.raises(ValueError, match="known"):
        predict_topk(m, ids, r, known=SimpleNamespace(n_entities=m.n_entities + 1, device=torch.device("cpu")), **kw)
    with pytest.raises(ValueError, match="scoring"):
        predict_topk(m, ids, r, scoring="distmult")
    with pytest.raises(ValueError, match="needs the relations"):
        predict_topk(m, ids, None, scoring="transe")
    bare = SimpleNamespace(entity_embed=m.entity_embed, n_entities=m.n_entities, n_relations=3, scoring="dot",
                           training=False, _table_for_inference=m._table_for_inference)
    with pytest.raises(AttributeError, match="initialize_MLP"):
        predict_topk(bare, ids, None, **kw)
    with pytest.raises(AttributeError, match="initialize_MLP"):
        mlp_scores(bare, ids, ids)
    with pytest.raises(ValueError, match="head_ids"):
        mlp_scores(m, ids.float(), ids)
    with pytest.raises(ValueError, match="tail_ids"):
        mlp_scores(m, ids, ids.reshape(1, 3))
    # the counting kernels keep rejecting the pair head
    with pytest.raises(ValueError, match="scoring must be one of"):
        ranking.rank_triples(m, ids, r, ids, scoring="mlp")
    with pytest.raises(ValueError, match="scoring must be one of"):
        ranking.evaluate_ranking(m, ids, r, ids, scoring="mlp")
    assert ranking.SCORINGS == ("transr", "transe", "dot")
    # an empty query list needs no device either
    res = predict_topk(m, ids[:0], None, k=4, **kw)
    assert res.ids.shape == (0, 4)


def test_exports_and_abi_names():
    import literalkg_amd
    from literalkg_amd import _native
    assert literalkg_amd.mlp_scores is pairmlp.mlp_scores and literalkg_amd.fold_mlp_head is pairmlp.fold_mlp_head
    assert hasattr(literalkg_amd.LiteralKG, "mlp_scores")
    for name in ("lkg_pair_mlp_scores_f32", "lkg_pair_mlp_splits", "lkg_pair_mlp_select_f32"):
        assert name in _native.PROTOTYPES
