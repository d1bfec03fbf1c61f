"""GPU, model level: LiteralKG.calc_relation_loss (literalkg_amd/relation_loss.py) -- every parameter's gradient against a
dense float64 torch head written here (the library's encoder, then einsum, squared norm and masked cross_entropy in
float64) within 1e-4 of the parameter's largest entry, for 'transr' and 'transe', with and without ``known`` and with
prune_to_batch on and off; the reductions and the empty batch; the refusals; twenty Adam steps, over which the loss falls
and evaluate_relation_prediction's MRR on the trained pairs does not."""
import math

import pytest
import torch

import relation_loss_cases as RC

pytestmark = pytest.mark.gpu

N_ENT, N_REL = 600, 5


@pytest.fixture(scope="module")
def L(gpu_device):
    import __graft_entry__ as ge
    ge.build()
    import literalkg_amd
    return literalkg_amd


def _synthetic_model(L, dev, scoring, dim=8, seed=0):
    from oracle import literalkg_oracle as O
    from literalkg_amd import io
    from literalkg_amd.synth import make_kg
    h, t, r = make_kg(N_ENT, 4000, seed=seed + 1)
    r = r % N_REL
    cfg = O.default_cfg(embed_dim=dim, relation_dim=2 * dim if scoring != "transr" else 12, conv_dim=dim, n_conv_layers=1,
                        device=dev)
    torch.manual_seed(seed)
    m = L.LiteralKG(cfg, N_ENT, N_REL, io.initial_a_in(N_ENT, h, t, r), scoring=scoring)
    return m.to(dev), tuple(torch.from_numpy(x).to(dev) for x in (h, r, t))


def _dense_head(model, scoring, h, r, t, mask, scale):
    """float64[P]: the library's encoder, the head in dense float64 torch ops"""
    table = model.gat_embeddings().double()
    e = model.relation_embed.weight.double()
    d = table[h] - table[t]
    u3 = d[:, None, :] if scoring == "transe" else torch.einsum("pc,rcd->prd", d, model.gat_trans_M.double())
    z = -scale * ((u3 + e[None]) ** 2).sum(2)
    if mask is not None:
        z = z.masked_fill(mask, -math.inf)
    return torch.nn.functional.cross_entropy(z, r, reduction="none")


def _grads(model):
    return {k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None}


def _assert_same_gradients(got, want):
    assert set(got) == set(want) and "entity_embed.weight" in got and "relation_embed.weight" in got
    for name, w in want.items():
        w = w.to_dense() if w.is_sparse else w
        gq = got[name].to_dense() if got[name].is_sparse else got[name]
        tol = 1e-4 * float(w.abs().max())
        assert float((gq - w).abs().max()) <= tol, (name, float((gq - w).abs().max()), tol)


@pytest.mark.parametrize("prune", [False, True])
@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("scoring", ["transe", "transr"])
def test_model_parameter_gradients_against_a_dense_float64_head(L, gpu_device, scoring, filtered, prune):
    model, (kh, kr, kt) = _synthetic_model(L, gpu_device, scoring)
    model.train()
    model.prune_max_fraction = 1.0                     # a tiny graph: keep the compact path whatever the frontier covers
    model.prune_to_batch = prune
    # the batch: 80 triples of the graph, and 20 pairs that are known under ANOTHER relation than the one trained
    h, t = torch.cat((kh[:80], kh[80:100])), torch.cat((kt[:80], kt[80:100]))
    r = torch.cat((kr[:80], (kr[80:100] + 1) % N_REL))
    known = L.KnownTriples(kh, kr, kt, N_ENT, N_REL) if filtered else None
    mask = RC.dropped_mask(kh.cpu(), kr.cpu(), kt.cpu(), h.cpu(), r.cpu(), t.cpu(), N_REL).to(gpu_device) if filtered else None
    if filtered:
        assert int(mask.sum()) >= 20
    scale = 0.5
    model.zero_grad()
    loss = model.calc_relation_loss(h, r, t, known=known, scale=scale)
    loss.backward()
    got = _grads(model)
    if prune:
        assert model.gat_rows is not None and model.gat_rows.numel() < N_ENT     # the pruned path did run
    model.prune_to_batch = False
    model.zero_grad()
    want_rows = _dense_head(model, scoring, h, r, t, mask, scale)
    want_rows.mean().backward()
    want = _grads(model)
    want_loss = float(want_rows.mean().detach())
    assert abs(float(loss.detach()) - want_loss) <= 1e-4 * max(1.0, abs(want_loss))
    _assert_same_gradients(got, want)
    assert ("gat_trans_M" in got) == (scoring == "transr")
    model.prune_to_batch = prune
    with torch.no_grad():                              # the reductions: one set of per-pair values behind all three
        rows = model.calc_relation_loss(h, r, t, known=known, scale=scale, reduction="none")
        assert rows.shape == (100,) and rows.dtype == torch.float32
        assert float((rows.double() - want_rows).abs().max()) <= 1e-4 * max(1.0, float(want_rows.abs().max()))
        assert torch.equal(model.calc_relation_loss(h, r, t, known=known, scale=scale, reduction="sum"), rows.sum())
        assert torch.equal(model.calc_relation_loss(h, r, t, known=known, scale=scale, reduction="mean"), rows.mean())
        flip = torch.arange(99, -1, -1, device=gpu_device)                       # the pairs in another order: the same values
        assert torch.equal(model.calc_relation_loss(h[flip], r[flip], t[flip], known=known, scale=scale, reduction="none"),
                           rows[flip])
        assert torch.equal(L.relation_loss(model, h.cpu(), r.cpu(), t.cpu(), known=known, scale=scale, reduction="none"), rows)
        if filtered:                                   # a filter without the trained triples: the truth is exempt anyway
            other = L.KnownTriples(kh[100:], kr[100:], kt[100:], N_ENT, N_REL)
            keep = ~RC.dropped_mask(kh[:100].cpu(), kr[:100].cpu(), kt[:100].cpu(), h.cpu(), r.cpu(), t.cpu(), N_REL).any(1)
            a = model.calc_relation_loss(h, r, t, known=other, scale=scale, reduction="none")
            assert bool(keep.any()) and torch.equal(a[keep.to(gpu_device)], rows[keep.to(gpu_device)])


def test_the_empty_batch_and_the_refusals(L, gpu_device):
    model, (h, r, t) = _synthetic_model(L, gpu_device, "transe")
    model.eval()
    empty = model.calc_relation_loss(h[:0], r[:0], t[:0], reduction="none")
    assert empty.shape == (0,) and empty.dtype == torch.float32 and empty.device.type == "cuda"
    for reduction in ("mean", "sum"):
        zero = model.calc_relation_loss(h[:0], r[:0], t[:0], reduction=reduction)
        assert zero.shape == () and float(zero) == 0.0
    with pytest.raises(ValueError, match="scoring='dot' has no relation prediction"):
        model.calc_relation_loss(h[:4], r[:4], t[:4], scoring="dot")
    with pytest.raises(ValueError, match="scoring='mlp' has no triple score"):
        model.calc_relation_loss(h[:4], r[:4], t[:4], scoring="mlp")
    with pytest.raises(ValueError, match="needs a model with gat_trans_M"):
        model.calc_relation_loss(h[:4], r[:4], t[:4], scoring="transr")
    with pytest.raises(ValueError, match="known triples over 4 relations"):
        model.calc_relation_loss(h[:4], r[:4], t[:4], known=L.KnownTriples(h, r % 4, t, N_ENT, 4))
    with pytest.raises(ValueError, match="known triples live on"):
        cpu_known = L.KnownTriples(h, r, t, N_ENT, N_REL)
        cpu_known.device = torch.device("cpu")
        model.calc_relation_loss(h[:4], r[:4], t[:4], known=cpu_known)
    from literalkg_amd.distributed import ShardedLiteralKG
    with pytest.raises(NotImplementedError, match="row-sharded"):
        ShardedLiteralKG.calc_relation_loss(None, h[:4], r[:4], t[:4])
    with pytest.raises(IndexError, match="outside"):
        model.calc_relation_loss(h[:4], r[:4] + N_REL, t[:4])
        L.ops.check_deferred_errors()
    with pytest.raises(IndexError, match="outside"):
        model.calc_relation_loss(h[:4] + N_ENT, r[:4], t[:4])
        L.ops.check_deferred_errors()


@pytest.mark.parametrize("scoring", ["transe", "transr"])
def test_twenty_adam_steps_lower_the_loss_and_do_not_lower_the_relation_mrr(L, gpu_device, scoring):
    model, (h, r, t) = _synthetic_model(L, gpu_device, scoring, seed=4)
    known = L.KnownTriples(h, r, t, N_ENT, N_REL)
    h, r, t = h[:256], r[:256], t[:256]
    before = L.evaluate_relation_prediction(model, h, r, t, known=known)["mrr"]
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = model.calc_relation_loss(h, r, t, known=known)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    after = L.evaluate_relation_prediction(model, h, r, t, known=known)["mrr"]
    print(f"{scoring}: loss {losses[0]:.4f} -> {losses[-1]:.4f}, filtered relation MRR {before:.4f} -> {after:.4f}")
    assert math.isfinite(losses[-1]) and losses[-1] < losses[0], losses
    assert after >= before, (before, after)
