"""GPU: explicit triples under the model's own score (literalkg_amd/triples.py, lkg_triples.hip, lkg_threshold_fit_f32).

1. score_triples has the BITS predict_topk reports for the same (query, candidate), both sides, reported and kernel
   scores, for any batch size, order and projection route;  2. it lies within the float64 margin of DESIGN.md section
   3.6a (test_topk_gpu.oracle);  3. the confusion counts are those of triple_cases.decisions on the device's own float32
   scores, every integer exact;  4. the fitted thresholds are those of triple_cases.fit_by_definition, by bits;  5. the
   curve metrics and ratios follow the references;  6. the same on the golden models;  7. 64-bit addressing."""
import math

import numpy as np
import pytest
import torch

import pair_cases as PC
import triple_cases as TC
from test_topk_gpu import StandIn, U, _golden_model, oracle, random_model

pytestmark = pytest.mark.gpu

SHAPES = [("transr", 120, 37, 32), ("transr", 500, 300, 300), ("transe", 128, 33, 33), ("dot", 100, 64, 64)]
GRID_TRIPLES = 4096 * 64                     # lkg_triples.hip: TS_GRID workgroups of TS_TRIPLES triples per trip
# ... and the smallest P that gives workgroup 0 a second trip with a full wave, a partly filled one and two past the end
PS = [1, 15, 16, 17, 63, 64, 65, 255, 257, 4099, GRID_TRIPLES + 17]
P_MAX = PS[-1]
P_MID = 4099
N_CAND = 128
N_HEADS = 40


@pytest.fixture(scope="module")
def L(gpu_device):
    import __graft_entry__ as ge
    ge.build()
    import literalkg_amd
    return literalkg_amd


@pytest.fixture(scope="module")
def T(L):
    from literalkg_amd import triples
    return triples


@pytest.fixture(scope="module")
def ops(L):
    from literalkg_amd import ops
    return ops


class Model(StandIn):
    """StandIn with the two mode switches the evaluate / fit entry points use."""

    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        self.training = mode
        return self


def bits(x):
    return x.contiguous().view(torch.int32)


def rel_choices(n_rel):
    return [0] if n_rel == 1 else [0, 1, 2, 4]           # (n_rel = 5: relation 3 stays unused)


_CASES = {}


def case(scoring, n, k, c, n_rel, dev):
    """One model and P_MAX triples per shape, shared by the tests (never changed): heads from N_HEADS entities, tails from
    at most N_CAND unique candidates, so that one predict_topk over the distinct (query, relation) pairs holds every
    triple's score."""
    key = (scoring, n, k, c, n_rel)
    if key not in _CASES:
        gen = torch.Generator().manual_seed(1000 * len(scoring) + n + k + c + n_rel)
        m = random_model(gen, scoring, n, k, c, n_rel, dev)
        model = Model(m.T, m.relation_embed.weight, m.gat_trans_M, scoring)
        cand = torch.randperm(n, generator=gen)[:min(n, N_CAND)].sort().values
        heads = torch.randperm(n, generator=gen)[:N_HEADS]
        rels = torch.tensor(rel_choices(n_rel))
        h = heads[torch.randint(0, N_HEADS, (P_MAX,), generator=gen)].to(dev)
        t = cand[torch.randint(0, cand.numel(), (P_MAX,), generator=gen)].to(dev)
        r = rels[torch.randint(0, rels.numel(), (P_MAX,), generator=gen)].to(dev)
        y = torch.randint(0, 2, (P_MAX,), generator=gen).to(torch.uint8).to(dev)
        _CASES[key] = dict(model=model, cand=cand.to(dev), h=h, r=r, t=t, y=y, gen=gen, topk={})
    return _CASES[key]


def topk_lookup(L, cs, side):
    """(reported, kernel) float32[P_MAX]: what predict_topk reports for every triple of the case on that side, the roles
    swapped on the head side (the queries are the tails -- candidates of the tail side -- and the candidate set is made
    of the heads)."""
    if side in cs["topk"]:
        return cs["topk"][side]
    model, dev = cs["model"], cs["h"].device
    n, n_rel = model.n_entities, model.n_relations
    qid, cid = (cs["h"], cs["t"]) if side == "tail" else (cs["t"], cs["h"])
    cand = cs["cand"] if side == "tail" else torch.unique(cs["h"])
    assert cand.numel() <= 128
    uq, inv = torch.unique(qid * n_rel + cs["r"], return_inverse=True)
    res = L.predict_topk(model, uq // n_rel, uq % n_rel, side=side, k=cand.numel(), candidates=cand)
    assert bool((res.ids >= 0).all())                      # no filter, no NaN: every candidate is listed
    slot = torch.full((n,), -1, dtype=torch.int64, device=dev)
    slot[cand] = torch.arange(cand.numel(), device=dev)
    by_slot = [torch.empty_like(x).scatter_(1, slot[res.ids], x) for x in (res.scores, res.kernel_scores)]
    cs["topk"][side] = tuple(x[inv, slot[cid]] for x in by_slot)
    return cs["topk"][side]


# ----------------------------------------------------------------------------- 1. the bits of top-k
@pytest.mark.parametrize("n_rel", [1, 5])
@pytest.mark.parametrize("scoring,n,k,c", SHAPES)
def test_bits_of_topk(L, T, gpu_device, monkeypatch, scoring, n, k, c, n_rel):
    cs = case(scoring, n, k, c, n_rel, gpu_device)
    model, h, r, t = cs["model"], cs["h"], cs["r"], cs["t"]
    for side in ("tail", "head"):
        want, want_k = topk_lookup(L, cs, side)
        for p in PS:
            got = L.score_triples(model, h[:p], r[:p], t[:p], side=side)
            got_k = L.score_triples(model, h[:p], r[:p], t[:p], side=side, kernel_scores=True)
            assert got.shape == (p,) and got.dtype == torch.float32
            assert torch.equal(bits(got), bits(want[:p])), (side, p)
            assert torch.equal(bits(got_k), bits(want_k[:p])), (side, p)
        # any order, any batch size, either projection route
        p = 257
        perm = torch.randperm(p, generator=cs["gen"]).to(gpu_device)
        got = L.score_triples(model, h[:p][perm], r[:p][perm], t[:p][perm], side=side)
        assert torch.equal(bits(got), bits(want[:p][perm])), side
        for bs in (1, 7, p):
            got = L.score_triples(model, h[:p], r[:p], t[:p], side=side, batch_size=bs)
            assert torch.equal(bits(got), bits(want[:p])), (side, bs)
        if scoring == "transr":
            for route in ("distinct", "full"):
                monkeypatch.setattr(T, "PROJECT", route)
                for kern, w in ((False, want), (True, want_k)):
                    got = L.score_triples(model, h[:P_MID], r[:P_MID], t[:P_MID], side=side, kernel_scores=kern)
                    assert torch.equal(bits(got), bits(w[:P_MID])), (side, route, kern)
            monkeypatch.setattr(T, "PROJECT", None)


# ----------------------------------------------------------------------------- 2. float64
@pytest.mark.parametrize("scoring,n,k,c", SHAPES)
def test_scores_within_the_float64_margin(L, gpu_device, scoring, n, k, c):
    cs = case(scoring, n, k, c, 5, gpu_device)
    model, dev = cs["model"], gpu_device
    n_rel = model.n_relations
    p = P_MID
    h, r, t = cs["h"][:p], cs["r"][:p], cs["t"][:p]
    for side in ("tail", "head"):
        qid, cid = (h, t) if side == "tail" else (t, h)
        cand = torch.unique(cid)
        uq, inv = torch.unique(qid * n_rel + r, return_inverse=True)
        chunks = oracle(model.T, model.relation_embed.weight, model.gat_trans_M, scoring, side, uq // n_rel, uq % n_rel,
                        cand=cand)
        d64 = torch.empty((uq.numel(), cand.numel()), dtype=torch.float64, device=dev)
        e64 = torch.empty_like(d64)
        for i in range(uq.numel()):
            (cid_, d, e, _), = list(chunks(i))
            d64[i], e64[i] = d, e
        slot = torch.full((n,), -1, dtype=torch.int64, device=dev)
        slot[cand] = torch.arange(cand.numel(), device=dev)
        d, e = d64[inv, slot[cid]], e64[inv, slot[cid]]
        got = L.score_triples(model, h, r, t, side=side).double()
        if scoring == "dot":                               # the oracle's d is -2 q.p
            err, bound = (got - (-0.5 * d)).abs(), 0.5 * e + 1e-30
        else:
            err, bound = (got - d).abs(), e + 4 * U * d.abs() + 1e-30
        print(f"[{scoring} k={k} {side}] worst error / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), (side, float((err / bound).max()))


# ----------------------------------------------------------------------------- 3. + 5. counts, curve and ratios
def sick_copy(cs, row):
    """The case's model with one table row set to NaN (its own table: the shared one stays as it is)."""
    m = cs["model"]
    table = m.T.clone()
    table[row] = float("nan")
    return Model(table, m.relation_embed.weight, m.gat_trans_M, m.scoring)


def thresholds_for(s, r, n_rel, lower, kind):
    """float32[n_rel]: an observed score of every relation (a tie at the cut), the sentinel, or a value between scores"""
    thr = np.full(n_rel, TC.sentinel(lower), dtype=np.float32)
    if kind == "sentinel":
        return thr
    for rho in range(n_rel):
        v = np.sort(s[(r == rho) & ~np.isnan(s)])
        if v.size == 0:
            thr[rho] = np.float32(0.25)
        elif kind == "observed":
            thr[rho] = v[v.size // 2]
        else:
            a, b = v[v.size // 3], v[min(v.size // 3 + 1, v.size - 1)]
            thr[rho] = np.float32((np.float64(a) + np.float64(b)) / 2)
    return thr


@pytest.mark.parametrize("n_rel", [1, 5])
@pytest.mark.parametrize("scoring,n,k,c", SHAPES)
def test_counts_curve_and_ratios(L, gpu_device, scoring, n, k, c, n_rel):
    cs = case(scoring, n, k, c, n_rel, gpu_device)
    lower = scoring != "dot"
    for name, model in (("clean", cs["model"]), ("nan", sick_copy(cs, int(cs["t"][0])))):
        for p in (P_MID, 65):
            h, r, t, y = cs["h"][:p], cs["r"][:p], cs["t"][:p], cs["y"][:p]
            s = L.score_triples(model, h, r, t)
            sn, rn, yn = s.cpu().numpy(), r.cpu().numpy(), y.cpu().numpy()
            assert (np.isnan(sn).sum() > 0) == (name == "nan")
            curve = PC.curve_reference(-sn if lower else sn, yn)
            for kind in ("observed", "sentinel", "between"):
                thr = thresholds_for(sn, rn, n_rel, lower, kind)
                want = TC.metrics(TC.decisions(sn, rn, yn, thr, lower, n_rel), yn, curve)
                assert want["nan"] == int(np.isnan(sn).sum())
                for bs in ((None, 1000) if p == P_MID else (None, 1, 7)):
                    got = L.evaluate_triple_classification(model, h, r, t, y, torch.from_numpy(thr).to(gpu_device),
                                                           batch_size=bs)
                    TC.same_metrics(got, want, curve[3])
                    assert got["accuracy"] == (got["tp"] + got["tn"]) / p      # a NaN score is wrong
            # one float everywhere, and bool labels
            one = float(thresholds_for(sn, np.zeros_like(rn), 1, lower, "observed")[0])
            want = TC.metrics(TC.decisions(sn, rn, yn, np.float32(one), lower, n_rel), yn, curve)
            TC.same_metrics(L.evaluate_triple_classification(model, h, r, t, y.bool(), one), want, curve[3])
    # an empty class: the curve metrics are NaN, the rest stays defined
    h, r, t = cs["h"][:65], cs["r"][:65], cs["t"][:65]
    for fill in (0, 1):
        y1 = torch.full((65,), fill, dtype=torch.uint8, device=gpu_device)
        got = L.evaluate_triple_classification(cs["model"], h, r, t, y1, 0.5)
        assert math.isnan(got["roc_auc"]) and math.isnan(got["average_precision"]) and got["n"] == 65
        assert got["n_pos"] == 65 * fill and got["tp"] + got["fn"] == 65 * fill


def test_counts_accumulate_in_a_given_counter(ops, gpu_device):
    cs = case("transe", 128, 33, 33, 5, gpu_device)
    model, p = cs["model"], 257
    h, r, t, y = cs["h"][:p], cs["r"][:p], cs["t"][:p], cs["y"][:p]
    pn = ops.rank_sqnorm(model.T)
    e = model.relation_embed.weight
    s, c1 = ops.triple_scores(model.T, h, t, pn, e, r, labels=y, thr=60.0)
    counts = torch.zeros(5, dtype=torch.int64, device=gpu_device)
    for lo in range(0, p, 100):
        _, c2 = ops.triple_scores(model.T, h[lo:lo + 100], t[lo:lo + 100], pn, e, r[lo:lo + 100], labels=y[lo:lo + 100],
                                  thr=60.0, want_scores=False, counts=counts)
        assert c2 is counts
    want = TC.decisions(s.cpu().numpy(), np.zeros(p, dtype=np.int64), y.cpu().numpy(), np.float32(60.0), True, 1)[0]
    assert c1.tolist() == want.tolist() == counts.tolist() and 0 < want[0] + want[1] < p


# ----------------------------------------------------------------------------- 4. the fit
def same_fit(fit, want, per_relation=True):
    thr = fit.thresholds.cpu().numpy()
    w = want["thresholds"] if per_relation else np.full_like(want["thresholds"], want["global_threshold"])
    assert thr.dtype == np.float32 and np.array_equal(thr.view(np.uint32), w.view(np.uint32)), (thr, w)
    assert np.float32(fit.global_threshold).view(np.uint32) == np.float32(want["global_threshold"]).view(np.uint32)
    assert fit.n.dtype == torch.int64 and fit.n.cpu().tolist() == want["n"].tolist()
    if per_relation:
        assert fit.correct.cpu().tolist() == want["correct"].tolist()


@pytest.mark.parametrize("n_rel", [1, 5])
@pytest.mark.parametrize("scoring,n,k,c", SHAPES)
def test_fit_is_the_fit_by_definition(L, gpu_device, scoring, n, k, c, n_rel):
    cs = case(scoring, n, k, c, n_rel, gpu_device)
    lower = scoring != "dot"
    model, gen = cs["model"], cs["gen"]
    p = 1500
    h, r, t, y = (cs[x][:p].clone() for x in ("h", "r", "t", "y"))
    if n_rel > 1:
        r[r == 2] = 1                                      # relation 2: exactly one triple; 3 stays unused
        r[17] = 2
    sn = L.score_triples(model, h, r, t).cpu().numpy()
    rn = r.cpu().numpy()
    labelings = {"random": y.cpu().numpy()}
    sep = np.zeros(p, dtype=np.uint8)                      # labels a threshold separates perfectly
    for rho in np.unique(rn):
        m = rn == rho
        sep[m] = (sn[m] <= np.median(sn[m])) if lower else (sn[m] >= np.median(sn[m]))
    labelings["separable"] = sep
    one_class = y.cpu().numpy().copy()                     # relation 0: only positives; the last one: only negatives
    one_class[rn == 0] = 1
    one_class[rn == rn.max()] = 0 if n_rel > 1 else 1
    labelings["one class"] = one_class
    labelings["all negative"] = np.zeros(p, dtype=np.uint8)
    for name, yn in labelings.items():
        want = TC.fit_by_definition(sn, rn, yn, n_rel, lower)
        yt = torch.from_numpy(yn).to(gpu_device)
        fit = L.fit_triple_thresholds(model, h, r, t, yt)
        same_fit(fit, want)
        assert fit.scoring == scoring
        if name == "separable":
            assert fit.correct.cpu().tolist() == want["n"].tolist()
        if name == "all negative":
            assert bool((fit.thresholds == TC.sentinel(lower)).all())
        if n_rel > 1:                                      # the unused relation takes the pooled threshold
            assert float(fit.thresholds[3]) == fit.global_threshold and int(fit.n[3]) == 0
        # the fit is what the evaluation then counts
        got = L.evaluate_triple_classification(model, h, r, t, yt, fit)
        assert (got["per_relation"]["tp"] + got["per_relation"]["tn"]).tolist() == want["correct"].tolist()
        # any order, any batch size
        perm = torch.randperm(p, generator=gen).to(gpu_device)
        same_fit(L.fit_triple_thresholds(model, h[perm], r[perm], t[perm], yt[perm], batch_size=700), want)
        # one pooled threshold everywhere
        pooled = L.fit_triple_thresholds(model, h, r, t, yt, per_relation=False)
        same_fit(pooled, want, per_relation=False)
        d = TC.decisions(sn, rn, yn, want["global_threshold"], lower, n_rel)
        assert pooled.correct.cpu().tolist() == (d[:, 0] + d[:, 2]).tolist()
        assert int(pooled.correct.sum()) == want["global_correct"]
    # all scores equal: the same triple, over and over, under mixed labels
    for n_pos in (3, 5, 7):
        hh, rr, tt = h[:1].repeat(10), r[:1].repeat(10), t[:1].repeat(10)
        yn = (np.arange(10) < n_pos).astype(np.uint8)
        s1 = L.score_triples(model, hh, rr, tt).cpu().numpy()
        assert np.unique(s1.view(np.uint32)).size == 1
        fit = L.fit_triple_thresholds(model, hh, rr, tt, torch.from_numpy(yn).to(gpu_device))
        same_fit(fit, TC.fit_by_definition(s1, rr.cpu().numpy(), yn, n_rel, lower))
        assert int(fit.correct.sum()) == max(n_pos, 10 - n_pos)
        assert (fit.global_threshold == TC.sentinel(lower)) == (n_pos <= 5)       # a tie goes to the smaller cut
    # NaN scores present
    sick = sick_copy(cs, int(t[0]))
    sn = L.score_triples(sick, h, r, t).cpu().numpy()
    assert 0 < np.isnan(sn).sum() < p
    yt = y
    same_fit(L.fit_triple_thresholds(sick, h, r, t, yt), TC.fit_by_definition(sn, rn, yt.cpu().numpy(), n_rel, lower))


def fit_draws(rng, n, n_rel):
    r = rng.integers(0, n_rel, n)
    if n_rel > 2:
        r[r == 1] = 0                                      # an unused relation
    y = rng.integers(0, 2, n).astype(np.uint8)
    coarse = (rng.integers(-20, 20, n) / 4).astype(np.float32)        # heavy ties, +0.0 among them
    coarse[rng.random(n) < 0.05] = -0.0
    yield "coarse", coarse, r, y
    fine = rng.standard_normal(n).astype(np.float32).round(2)
    yield "fine", fine, r, y
    special = coarse.copy()
    special[rng.random(n) < 0.1] = np.nan
    special[rng.random(n) < 0.05] = np.inf
    special[rng.random(n) < 0.05] = -np.inf
    yield "nan and inf", special, r, y
    yield "informative", (coarse + 3 * y).astype(np.float32), r, y


@pytest.mark.parametrize("n_rel", [1, 5, 300])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4097, 20_001])
def test_threshold_fit_kernel(ops, gpu_device, n, n_rel):
    """lkg_threshold_fit_f32 alone, on scores with heavy ties: n around the 256-key workgroups of the segmented arg-max,
    relations that span several workgroups (n_rel 1, 5) and several relations inside one (300)."""
    rng = np.random.default_rng(100 * n + n_rel)
    for name, s, r, y in fit_draws(rng, n, n_rel):
        for lower in (True, False):
            want = TC.fit_by_definition(s, r, y, n_rel, lower)
            st, rt, yt = (torch.from_numpy(x).to(gpu_device) for x in (s, r, y))
            thr, stats = ops.threshold_fit(st, yt, rt, n_rel, lower)
            what = (name, n, n_rel, lower)
            assert np.array_equal(thr.cpu().numpy().view(np.uint32), want["fitted"].view(np.uint32)), what
            stats = stats.cpu().numpy()
            assert stats[:, 0].tolist() == want["n"].tolist() and stats[:, 2].tolist() == want["correct"].tolist(), what
            nan = np.isnan(s)
            assert stats[:, 3].tolist() == np.bincount(r[nan], minlength=n_rel).tolist(), what
            assert stats[:, 1].tolist() == np.bincount(r[~nan & (y != 0)], minlength=n_rel).tolist(), what
            thr_g, stats_g = ops.threshold_fit(st, yt, None, 1, lower)
            assert np.float32(thr_g.item()).view(np.uint32) == np.float32(want["global_threshold"]).view(np.uint32), what
            assert stats_g.cpu().tolist() == [[n, int((~nan & (y != 0)).sum()), want["global_correct"], int(nan.sum())]]
            perm = torch.from_numpy(rng.permutation(n)).to(gpu_device)
            thr2, stats2 = ops.threshold_fit(st[perm], yt[perm], rt[perm], n_rel, lower)
            assert torch.equal(bits(thr2), bits(thr)) and torch.equal(stats2.cpu(), torch.from_numpy(stats)), what
    # nothing to fit
    e = torch.zeros(0, device=gpu_device)
    thr, stats = ops.threshold_fit(e, e.to(torch.uint8), e.long(), n_rel, True)
    assert thr.tolist() == [-math.inf] * n_rel and int(stats.abs().sum()) == 0


# ----------------------------------------------------------------------------- 6. model level
@pytest.mark.parametrize("name,scoring", [("encoder_gcn_l2_gatenum", "transr"), ("transe_gcn_l1", "transe")])
def test_golden_model(L, gpu_device, name, scoring):
    model, gd = _golden_model(L, name, gpu_device, scoring)
    gen = torch.Generator().manual_seed(11)
    h, r, t = (torch.from_numpy(gd[x]).to(gpu_device) for x in ("h", "r", "t"))
    cand = torch.unique(t)[:128]
    keep = torch.isin(t, cand) & torch.isin(h, torch.unique(h)[:128])
    h, r, t = h[keep][:300], r[keep][:300], t[keep][:300]
    p = h.numel()
    assert p >= 200
    # negatives: every second triple gets a random tail among the candidates
    y = (torch.arange(p) % 2 == 0).to(torch.uint8).to(gpu_device)
    t = torch.where(y.bool(), t, cand[torch.randint(0, cand.numel(), (p,), generator=gen).to(gpu_device)])
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    n_rel = model.n_relations
    model.eval()
    topk = {}
    for side, qid, cid, cc in (("tail", h, t, cand), ("head", t, h, torch.unique(h))):
        uq, inv = torch.unique(qid * n_rel + r, return_inverse=True)
        res = model.predict_topk(uq // n_rel, uq % n_rel, side=side, k=cc.numel(), candidates=cc)
        slot = torch.full((model.n_entities,), -1, dtype=torch.int64, device=gpu_device)
        slot[cc] = torch.arange(cc.numel(), device=gpu_device)
        topk[side] = tuple(torch.empty_like(x).scatter_(1, slot[res.ids], x)[inv, slot[cid]]
                           for x in (res.scores, res.kernel_scores))
    cache = model._eval_cache
    assert cache is not None
    for side in ("tail", "head"):
        for kern in (False, True):
            got = model.score_triples(h, r, t, side=side, kernel_scores=kern, batch_size=64)
            assert torch.equal(bits(got), bits(topk[side][int(kern)])), (side, kern)
    s = model.score_triples(h, r, t)
    sn, rn, yn = s.cpu().numpy(), r.cpu().numpy(), y.cpu().numpy()
    fit = model.fit_triple_thresholds(h, r, t, y)
    want_fit = TC.fit_by_definition(sn, rn, yn, n_rel, True)
    same_fit(fit, want_fit)
    curve = PC.curve_reference(-sn, yn)
    for thr in (fit, fit.thresholds, float(np.median(sn))):
        thr_np = want_fit["thresholds"] if not isinstance(thr, float) else np.float32(thr)
        got = model.evaluate_triple_classification(h, r, t, y, thr, batch_size=100)
        TC.same_metrics(got, TC.metrics(TC.decisions(sn, rn, yn, thr_np, True, n_rel), yn, curve), curve[3])
    assert not model.training and model._eval_cache is cache       # the mode and the kept table are left as found
    model.train()                                          # from training mode: evaluated in eval mode, the mode restored
    same_fit(model.fit_triple_thresholds(h, r, t, y), want_fit)
    assert model.training
    got = model.evaluate_triple_classification(h, r, t, y, fit)
    TC.same_metrics(got, TC.metrics(TC.decisions(sn, rn, yn, want_fit["thresholds"], True, n_rel), yn, curve), curve[3])
    assert model.training
    for k_, v in model.state_dict().items():
        v0 = params[k_]
        if v.is_sparse:
            v, v0 = v.coalesce().values(), v0.coalesce().values()
        assert torch.equal(v, v0), k_


# ----------------------------------------------------------------------------- 7. scale guard
def test_two_million_rows(L, gpu_device):
    """Row indices whose byte offset lies past 2^31 (the rows of a 2 M x 16 table kept 304 floats apart), and the same
    table packed: float64 margin on both, bit equality between the two (the stride does not enter the arithmetic)."""
    gen = torch.Generator(device=gpu_device).manual_seed(77)
    n, kd, ld, n_rel, p = 2_000_000, 16, 304, 3, 3000
    store = torch.empty((n, ld), dtype=torch.float32, device=gpu_device)
    wide = store[:, :kd]
    wide.copy_(torch.randn(n, kd, generator=gen, device=gpu_device))
    relemb = torch.randn(n_rel, kd, generator=gen, device=gpu_device) * 0.3
    h = torch.randint(0, n, (p,), generator=gen, device=gpu_device)
    t = torch.randint(n - 200_000, n, (p,), generator=gen, device=gpu_device)
    h[:64] = torch.arange(n - 64, n, device=gpu_device)
    r = torch.randint(0, n_rel, (p,), generator=gen, device=gpu_device)
    assert int(t.min()) * ld * 4 > 2 ** 31
    packed = wide.contiguous()
    out = {}
    for name, table in (("strided", wide), ("packed", packed)):
        model = Model(table, relemb, None, "transe")
        for side in ("tail", "head"):
            out[name, side] = L.score_triples(model, h, r, t, side=side)
            q = packed[h if side == "tail" else t].double() + (1.0 if side == "tail" else -1.0) * relemb[r].double()
            x = packed[t if side == "tail" else h].double()
            d = ((x - q) ** 2).sum(1)
            dq = U * q.norm(dim=1)
            e = (kd + 2) * U * (x.norm(dim=1) + q.norm(dim=1)) ** 2 + 2.0 * d.sqrt() * dq + dq * dq
            assert bool(((out[name, side].double() - d).abs() <= e + 4 * U * d + 1e-30).all()), (name, side)
    for side in ("tail", "head"):
        assert torch.equal(bits(out["strided", side]), bits(out["packed", side])), side
    y = torch.randint(0, 2, (p,), generator=gen, device=gpu_device).to(torch.uint8)
    model = Model(wide, relemb, None, "transe")
    fit = L.fit_triple_thresholds(model, h, r, t, y)
    sn = out["strided", "tail"].cpu().numpy()
    same_fit(fit, TC.fit_by_definition(sn, r.cpu().numpy(), y.cpu().numpy(), n_rel, True))
