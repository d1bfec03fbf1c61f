"""GPU, model level: LiteralKG.calc_self_adversarial_loss (literalkg_amd/self_adversarial.py) -- every parameter's gradient
against a dense float32 torch head written here (the library's encoder, the head in torch ops) within 1e-4 of the
parameter's largest entry, for 'transr', 'transe' and 'dot', both sides, with a relation that is absent from the batch; the
reductions; group_sampled_batch on a real KGBatchSampler batch; prune_to_batch against the full table; twenty Adam steps."""
import math

import pytest
import torch

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
    m = L.LiteralKG(cfg, N_ENT, N_REL, io.initial_a_in(N_ENT, h, t, r), scoring="transr" if scoring == "transr" else "transe")
    return m.to(dev), tuple(torch.from_numpy(x).to(dev) for x in (h, r, t))


def _batch(h, r, t, g, kn, seed, absent=3):
    """g triples none of which has relation `absent`, and kn random negatives each"""
    keep = (r != absent).nonzero()[:, 0][:g]
    neg = torch.randint(0, N_ENT, (g, kn), generator=torch.Generator().manual_seed(seed)).to(h.device)
    return h[keep], r[keep], t[keep], neg


def _dense_head(model, scoring, side, h, r, t, neg, margin, scale, temperature):
    """float32[G]: the library's encoder, the head in dense torch ops (the weights detached)"""
    table = model.gat_embeddings()
    e = model.relation_embed.weight
    sign = 1.0 if side == "tail" else -1.0
    anchor, pos = (h, t) if side == "tail" else (t, h)

    def group_loss(q, p, n):                       # q, p [G, k], n [G, K, k]
        if scoring == "dot":
            zp, zn = scale * (margin + (q * p).sum(1)), scale * (margin + (q[:, None] * n).sum(2))
        else:
            zp, zn = scale * (margin - ((q - p) ** 2).sum(1)), scale * (margin - ((q[:, None] - n) ** 2).sum(2))
        w = torch.softmax(temperature * zn, dim=1).detach()
        sp = torch.nn.functional.softplus
        return sp(-zp) + (w * sp(zn)).sum(1)
    if scoring == "dot":
        return group_loss(table[anchor], table[pos], table[neg])
    if scoring == "transe":
        return group_loss(table[anchor] + sign * e[r], table[pos], table[neg])
    loss = torch.zeros(h.numel(), device=h.device)
    for rr in r.unique().tolist():
        at = (r == rr).nonzero()[:, 0]
        p_r = table @ model.gat_trans_M[rr]
        loss = loss.index_put((at,), group_loss(p_r[anchor[at]] + sign * e[rr], p_r[pos[at]], p_r[neg[at]]))
    return loss


def _assert_same_gradients(got, want):
    assert set(got) == set(want) and "entity_embed.weight" in got
    for name, w in want.items():
        w = w.to_dense() if w.is_sparse else w
        gq = got[name].to_dense() if got[name].is_sparse else got[name]
        tol = 1e-4 * float(w.abs().max())
        assert float((gq - w).abs().max()) <= tol, (name, float((gq - w).abs().max()), tol)


def _grads(model):
    return {k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None}


@pytest.mark.parametrize("scoring,side", [("transe", "tail"), ("transe", "head"), ("transr", "tail"), ("transr", "head"),
                                          ("dot", "tail"), ("dot", "head")])
def test_model_parameter_gradients_against_a_dense_torch_head(L, gpu_device, scoring, side):
    model, (h, r, t) = _synthetic_model(L, gpu_device, scoring)
    model.train()
    h, r, t, neg = _batch(h, r, t, 80, 5, seed=2)
    assert len(r.unique()) >= 2 and 3 not in r.tolist()                          # several relations, one of them absent
    margin, scale, temperature = 6.0, 0.5, 0.7
    kw = dict(side=side, margin=margin, scale=scale, temperature=temperature, scoring=scoring)
    model.zero_grad()
    loss = model.calc_self_adversarial_loss(h, r, t, neg, **kw)
    loss.backward()
    got = _grads(model)
    model.zero_grad()
    want_rows = _dense_head(model, scoring, side, h, r, t, neg, margin, scale, temperature)
    want_rows.mean().backward()
    want = _grads(model)
    want_loss = float(want_rows.mean().detach())
    assert abs(float(loss.detach()) - want_loss) <= 1e-4 * max(1.0, abs(want_loss))
    _assert_same_gradients(got, want)
    if scoring != "dot":
        assert "relation_embed.weight" in got and float(got["relation_embed.weight"][3].abs().max()) == 0.0
    if scoring == "transr":
        assert float(got["gat_trans_M"][3].abs().max()) == 0.0                   # the absent relation: no gradient at all
    # the reductions: one set of per-group values behind all three, in the caller's order
    with torch.no_grad():
        rows = model.calc_self_adversarial_loss(h, r, t, neg, reduction="none", **kw)
        assert rows.shape == (80,) and float((rows - want_rows).abs().max()) <= 1e-4 * max(1.0, float(want_rows.abs().max()))
        assert torch.equal(model.calc_self_adversarial_loss(h, r, t, neg, reduction="sum", **kw), rows.sum())
        assert torch.equal(model.calc_self_adversarial_loss(h, r, t, neg, reduction="mean", **kw), rows.mean())
        flip = torch.arange(79, -1, -1, device=gpu_device)                       # the groups in another order: the same values
        again = model.calc_self_adversarial_loss(h[flip], r[flip], t[flip], neg[flip], reduction="none", **kw)
        assert torch.equal(again, rows[flip])


def test_group_sampled_batch_gives_the_result_of_the_two_dimensional_call(L, gpu_device):
    from literalkg_amd.sampler import KGBatchSampler
    model, (h, r, t) = _synthetic_model(L, gpu_device, "transe")
    model.eval()
    kn = 4
    graph = L.KGStructure.from_triples(N_ENT, h.cpu().numpy(), t.cpu().numpy(), r.cpu().numpy(), device=gpu_device)
    torch.manual_seed(3)
    bh, br, bp, bn = KGBatchSampler(graph, kn).sample(kn * 50, seed=9)
    gh, gr, gt, gneg = L.group_sampled_batch(bh, br, bp, bn, kn)
    assert gh.shape == (50,) and gneg.shape == (50, kn)
    assert torch.equal(gh, bh[::kn]) and torch.equal(gr, br[::kn]) and torch.equal(gt, bp[::kn])
    assert torch.equal(gneg.reshape(-1), bn)
    with torch.no_grad():
        a = model.calc_self_adversarial_loss(gh, gr, gt, gneg, margin=6.0, reduction="none")
        b = model.calc_self_adversarial_loss(bh[::kn], br[::kn], bp[::kn], bn.view(-1, kn), margin=6.0, reduction="none")
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    with pytest.raises(ValueError, match="not whole groups of 5"):
        L.group_sampled_batch(bh, br, bp, bn, 5)                                 # 200 rows in fives: groups of another size
    with pytest.raises(ValueError, match="not whole groups of 3"):
        L.group_sampled_batch(bh, br, bp, bn, 3)
    with pytest.raises(IndexError, match="outside"):
        model.calc_self_adversarial_loss(gh, gr, gt, gneg + N_ENT)
        L.ops.check_deferred_errors()


@pytest.mark.parametrize("scoring", ["transe", "transr"])
def test_prune_to_batch_against_the_full_table(L, gpu_device, scoring):
    model, (h, r, t) = _synthetic_model(L, gpu_device, scoring)
    model.train()
    model.prune_max_fraction = 1.0                     # a tiny graph: keep the compact path whatever the frontier covers
    h, r, t, neg = _batch(h, r, t, 40, 3, seed=5)
    out = {}
    for prune in (False, True):
        model.prune_to_batch = prune
        model.zero_grad()
        loss = model.calc_self_adversarial_loss(h, r, t, neg, margin=6.0, scale=0.5, temperature=0.7)
        loss.backward()
        out[prune] = (float(loss.detach()), _grads(model))
        if prune:
            assert model.gat_rows is not None and model.gat_rows.numel() < N_ENT     # the pruned path did run
    assert abs(out[True][0] - out[False][0]) <= 1e-4 * max(1.0, abs(out[False][0]))
    _assert_same_gradients(out[True][1], out[False][1])


def test_twenty_adam_steps_lower_the_loss(L, gpu_device):
    model, (h, r, t) = _synthetic_model(L, gpu_device, "transe", seed=4)
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    neg = torch.randint(0, N_ENT, (256, 8), generator=torch.Generator().manual_seed(0)).to(gpu_device)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = model.calc_self_adversarial_loss(h[:256], r[:256], t[:256], neg, margin=6.0)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert math.isfinite(losses[-1]) and losses[-1] < losses[0], losses
