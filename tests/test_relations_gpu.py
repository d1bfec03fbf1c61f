"""GPU: relation prediction (literalkg_amd/relations.py, lkg_relations.hip).

1. score_relations has the BITS of score_triples, column by column, on both sides, for any number of pairs, any order,
   batch size, relation chunk and projection route (so the float64 margin of test_triples_gpu.py is inherited);
2. on tables of small integers every score is exact, and the ranks and lists equal tests/relation_cases.py with natural
   ties, with and without a filter;  3. lkg_relation_order_f32 alone on synthetic matrices with heavy ties, NaNs and
   awkward filters;  4. two relations built to tie bitwise;  5. a NaN relation embedding;  6. the golden models;
   7. the LiteralKG methods and the empty input."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import relation_cases as RC
from test_topk_gpu import StandIn, _golden_model, random_model

pytestmark = pytest.mark.gpu

SMALL = [("transr", 120, 37, 32), ("transe", 128, 33, 33)]
WIDE = [("transr", 300, 300, 300), ("transe", 200, 300, 300)]
BIT_CASES = [(*s, n_rel) for s in SMALL for n_rel in (1, 2, 5, 17, 70)] + [(*s, n_rel) for s in WIDE for n_rel in (1, 2, 5)]
PS = [1, 15, 16, 17, 63, 64, 65, 257, 4099]
P_MAX = PS[-1]
GRID_PAIRS = 4096 * 64                       # lkg_relations.hip: RS_GRID workgroups of RS_PAIRS pairs per trip
N_POOL = 40


@pytest.fixture(scope="module")
def L(gpu_device):
    import __graft_entry__ as ge
    ge.build()
    import literalkg_amd
    return literalkg_amd


@pytest.fixture(scope="module")
def REL(L):
    from literalkg_amd import relations
    return relations


@pytest.fixture(scope="module")
def ops(L):
    from literalkg_amd import ops
    return ops


class Model(StandIn):
    """StandIn with the two mode switches evaluate_relation_prediction uses."""

    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        self.training = mode
        return self


def bits(x):
    return x.contiguous().view(torch.int32)


def pairs(gen, n, p, dev):
    """p pairs whose heads and tails come from N_POOL entities (rows repeat), every seventh with h == t"""
    pool = torch.randperm(n, generator=gen)[:N_POOL]
    h = pool[torch.randint(0, N_POOL, (p,), generator=gen)]
    t = pool[torch.randint(0, N_POOL, (p,), generator=gen)]
    t[::7] = h[::7]
    return h.to(dev), t.to(dev)


def columns_of_score_triples(L, model, h, t, side):
    """float32[P, n_rel]: column j is score_triples(model, h, full(j), t, side=side)"""
    cols = [L.score_triples(model, h, torch.full_like(h, j), t, side=side) for j in range(model.n_relations)]
    return torch.stack(cols, dim=1)


# ----------------------------------------------------------------------------- 1. the bits of score_triples
@pytest.mark.parametrize("scoring,n,k,c,n_rel", BIT_CASES)
def test_bits_of_score_triples(L, REL, gpu_device, monkeypatch, scoring, n, k, c, n_rel):
    gen = torch.Generator().manual_seed(7 * n + k + 1000 * n_rel)
    m = random_model(gen, scoring, n, k, c, n_rel, gpu_device)
    model = Model(m.T, m.relation_embed.weight, m.gat_trans_M, scoring)
    h, t = pairs(gen, n, P_MAX, gpu_device)
    assert bool((h == t).any()) and bool((h != t).any())
    for side in ("tail", "head"):
        want = columns_of_score_triples(L, model, h, t, side)             # once per side; never changed
        assert not bool(torch.isnan(want).any())
        for p in PS:
            got = L.score_relations(model, h[:p], t[:p], side=side)
            assert got.shape == (p, n_rel) and got.dtype == torch.float32
            assert torch.equal(bits(got), bits(want[:p])), (side, p)
        p = 257
        perm = torch.randperm(p, generator=gen).to(gpu_device)
        got = L.score_relations(model, h[:p][perm], t[:p][perm], side=side)
        assert torch.equal(bits(got), bits(want[:p][perm])), side
        p = 65
        for bs in (1, 7, p):
            got = L.score_relations(model, h[:p], t[:p], side=side, batch_size=bs)
            assert torch.equal(bits(got), bits(want[:p])), (side, bs)
        for chunk in (1, 3, n_rel):
            got = L.score_relations(model, h[:p], t[:p], side=side, relation_chunk=chunk, batch_size=33)
            assert torch.equal(bits(got), bits(want[:p])), (side, chunk)
        if scoring == "transr":
            for route in ("distinct", "full"):
                monkeypatch.setattr(REL, "PROJECT", route)
                got = L.score_relations(model, h, t, side=side, relation_chunk=2)
                assert torch.equal(bits(got), bits(want)), (side, route)
            monkeypatch.setattr(REL, "PROJECT", None)
    assert bool((bits(L.score_relations(model, h[:65], t[:65], side="tail")) !=
                 bits(L.score_relations(model, h[:65], t[:65], side="head"))).any())     # the sides are different numbers


@pytest.mark.parametrize("scoring,n,k,c", SMALL)
def test_a_workgroup_takes_a_second_trip(L, gpu_device, scoring, n, k, c):
    """the smallest P at which workgroup 0 comes round again: one pair in its first wave, the other waves past the end"""
    gen = torch.Generator().manual_seed(31 + n)
    m = random_model(gen, scoring, n, k, c, 2, gpu_device)
    model = Model(m.T, m.relation_embed.weight, m.gat_trans_M, scoring)
    p = GRID_PAIRS + 1
    h, t = pairs(gen, n, p, gpu_device)
    for side in ("tail", "head"):
        want = columns_of_score_triples(L, model, h, t, side)
        got = L.score_relations(model, h, t, side=side)
        assert torch.equal(bits(got), bits(want)), side


# ----------------------------------------------------------------------------- 2. exact integer tables
def integer_model(gen, scoring, n, c, k, n_rel, dev):
    """Table, W_r and e_r of entries in {-1, 0, 1}, c = k = 8.  |x W| <= 8, |q| <= 9, every product at most 81 and every
    partial sum at most 8 * 17^2 = 2312 < 2^24: float32 is exact throughout.  The scores are small integers, so relations
    tie often."""
    table = torch.randint(-1, 2, (n, c), generator=gen).float()
    e = torch.randint(-1, 2, (n_rel, k), generator=gen).float()
    w = torch.randint(-1, 2, (n_rel, c, k), generator=gen).float() if scoring == "transr" else None
    return Model(table.to(dev), e.to(dev), None if w is None else w.to(dev), scoring), table, e, w


def integer_scores(table, e, w, h, t):
    """int64[P, n_rel]: ||x_h W_r + e_r - x_t W_r||^2 (W_r the identity without w)"""
    x, ee = table.numpy().astype(np.int64), e.numpy().astype(np.int64)
    h, t = h.cpu().numpy(), t.cpu().numpy()
    out = np.empty((h.size, ee.shape[0]), dtype=np.int64)
    for j in range(ee.shape[0]):
        pr = x if w is None else x @ w[j].numpy().astype(np.int64)
        d = pr[h] + ee[j] - pr[t]
        out[:, j] = (d * d).sum(1)
    return out


def some_known(gen, h, r, t, n_rel, n_extra):
    """Known triples about the pairs themselves: the truths of every third pair, n_extra random relations of random pairs,
    and the first 50 of them once more (duplicates)."""
    p = h.numel()
    pick = torch.randint(0, p, (n_extra,), generator=gen).to(h.device)
    kh = torch.cat((h[::3], h[pick]))
    kt = torch.cat((t[::3], t[pick]))
    kr = torch.cat((r[::3], torch.randint(0, n_rel, (n_extra,), generator=gen).to(h.device)))
    return torch.cat((kh, kh[:50])), torch.cat((kr, kr[:50])), torch.cat((kt, kt[:50]))


def check_against_references(L, model, h, r, t, scores_np, known_triples, side="tail"):
    """rank_relations and predict_relations against relation_cases on the given score matrix, without and with a filter"""
    n_rel = model.n_relations
    kh, kr, kt = known_triples
    known = L.KnownTriples(kh, kr, kt, model.n_entities, n_rel)
    sets = RC.known_sets(h.cpu().numpy(), t.cpu().numpy(), kh.cpu().numpy(), kr.cpu().numpy(), kt.cpu().numpy())
    truth = r.cpu().numpy()
    out = {}
    for name, kn, kn_sets in (("raw", None, None), ("filtered", known, sets)):
        res = L.rank_relations(model, h, r, t, known=kn, side=side)
        wb, we = RC.counts(scores_np, truth, kn_sets)
        assert res.better.dtype == torch.int64 and res.side == side
        assert res.better.cpu().tolist() == wb.tolist() and res.equal.cpu().tolist() == we.tolist(), name
        assert torch.equal(res.rank.cpu(), torch.from_numpy(1.0 + wb + 0.5 * we)), name
        for k in (1, 3, min(n_rel + 2, 128)):
            top = L.predict_relations(model, h, t, k=k, known=kn, side=side)
            wi, ws = RC.topk(scores_np, k, kn_sets)
            assert top.ids.dtype == torch.int64 and top.ids.cpu().tolist() == wi.tolist(), (name, k)
            assert np.array_equal(top.scores.cpu().numpy().view(np.uint32), ws.view(np.uint32)), (name, k)
        out[name] = (wb, we)
    return out


@pytest.mark.parametrize("scoring", ["transr", "transe"])
def test_exact_integer_tables(L, gpu_device, scoring):
    gen = torch.Generator().manual_seed(17)
    n, c, n_rel, p = 50, 8, 6, 300
    model, table, e, w = integer_model(gen, scoring, n, c, c, n_rel, gpu_device)
    h, t = pairs(gen, n, p, gpu_device)
    r = torch.randint(0, n_rel, (p,), generator=gen).to(gpu_device)
    want = integer_scores(table, e, w, h, t)
    assert want.max() < 2 ** 24
    got = L.score_relations(model, h, t)
    assert np.array_equal(got.cpu().numpy().astype(np.float64), want.astype(np.float64))          # every score exact
    got_head = L.score_relations(model, h, t, side="head")             # ||x_t W - e - x_h W||^2: the same integer
    assert np.array_equal(got_head.cpu().numpy().astype(np.float64), want.astype(np.float64))
    both = check_against_references(L, model, h, r, t, want.astype(np.float32), some_known(gen, h, r, t, n_rel, 400))
    assert both["raw"][1].sum() > 0                                    # natural ties are present ...
    assert (both["raw"][0] != both["filtered"][0]).any()               # ... and the filter bites


# ----------------------------------------------------------------------------- 3. the order kernel alone
N_ENT = 50


def order_case(rng, n, n_rel):
    """Scores from a few distinct values (ties everywhere) with NaNs and an all-NaN row; pairs over N_ENT entities; raw
    known edges with duplicates, a known truth, every relation of pair 0 known, and pairs absent from the structure
    (the edges drawn for rows 40 .. 49 are moved to other rows; many (row, col) of the other rows have none either)."""
    s = rng.choice(np.array([-1.5, -0.0, 0.0, 0.25, 0.25, 3.0, np.inf], dtype=np.float32), (n, n_rel))
    s[rng.random((n, n_rel)) < 0.1] = np.nan
    s[n // 2] = np.nan
    truth = rng.integers(0, n_rel, n)
    fr, fc = rng.integers(0, N_ENT, n), rng.integers(0, N_ENT, n)
    n_edges = 4 * n + 10
    pick = rng.integers(0, n, n_edges)
    kh, kt, kr = fr[pick], fc[pick], rng.integers(0, n_rel, n_edges)
    kh[kh >= 40] -= 10                                                 # (those pairs stay unknown)
    kh = np.concatenate((kh, kh[:20], fr[:1].repeat(n_rel), fr[-1:]))  # duplicates; all of pair 0; the last pair's truth
    kt = np.concatenate((kt, kt[:20], fc[:1].repeat(n_rel), fc[-1:]))
    kr = np.concatenate((kr, kr[:20], np.arange(n_rel), truth[-1:]))
    return s, truth, fr, fc, kh, kr, kt


@pytest.mark.parametrize("n_rel", [1, 2, 63, 64, 65, 300, 4096])
def test_order_kernel_on_synthetic_matrices(ops, gpu_device, n_rel):
    rng = np.random.default_rng(n_rel)
    dev = gpu_device
    for n in (1, 2, 63, 64, 65, 1025):
        s, truth, fr, fc, kh, kr, kt = order_case(rng, n, n_rel)
        sets = RC.known_sets(fr, fc, kh, kr, kt)
        assert len(sets[0]) == n_rel and truth[-1] in sets[-1]
        st, tt, frt, fct = (torch.from_numpy(x).to(dev) for x in (s, truth, fr, fc))
        filt = ops.csr_build_device(N_ENT, *(torch.from_numpy(x).to(dev) for x in (kh, kt, kr)))
        for name, f, kn in (("raw", None, None), ("filtered", filt, sets)):
            better, equal, ids, top = ops.relation_order(st, truth=tt, filt=f, filter_row=frt, filter_col=fct)
            assert ids is None and top is None and better.dtype == torch.int32
            wb, we = RC.counts(s, truth, kn)
            assert better.cpu().tolist() == wb.tolist() and equal.cpu().tolist() == we.tolist(), (name, n)
            for top_k in (1, 3, 128):                                  # 128 > n_rel for the small ones: padding
                b2, e2, ids, top = ops.relation_order(st, truth=tt if top_k == 3 else None, filt=f, filter_row=frt,
                                                      filter_col=fct, top_k=top_k)
                wi, ws = RC.topk(s, top_k, kn)
                assert ids.dtype == torch.int64 and ids.cpu().tolist() == wi.tolist(), (name, n, top_k)
                assert np.array_equal(top.cpu().numpy().view(np.uint32), ws.view(np.uint32)), (name, n, top_k)
                if top_k == 3:                                         # counts and lists from one launch
                    assert b2.cpu().tolist() == wb.tolist() and e2.cpu().tolist() == we.tolist(), (name, n)
                else:
                    assert b2 is None and e2 is None
        if n > 1:                                                      # a column block of a wider matrix (lds > n_rel)
            wide = torch.full((n, n_rel + 3), -9.0, device=dev)
            wide[:, 1:n_rel + 1] = st
            better, equal, ids, _ = ops.relation_order(wide[:, 1:n_rel + 1], truth=tt, top_k=1)
            wb, we = RC.counts(s, truth)
            assert better.cpu().tolist() == wb.tolist() and equal.cpu().tolist() == we.tolist()
            assert ids.cpu().tolist() == RC.topk(s, 1)[0].tolist()


def test_order_kernel_refuses_what_it_cannot_take(ops, gpu_device):
    s = torch.zeros((2, ops.RELATION_MAX + 1), device=gpu_device)
    with pytest.raises(ValueError, match="LDS"):
        ops.relation_order(s, top_k=1)
    with pytest.raises(ValueError, match="top_k"):
        ops.relation_order(s[:, :5], top_k=ops.TOPK_MAX + 1)
    with pytest.raises(ValueError, match="nothing to compute"):
        ops.relation_order(s[:, :5])
    with pytest.raises(ValueError, match="truths"):
        ops.relation_order(s[:, :5], truth=torch.zeros(3, dtype=torch.int64, device=gpu_device))


# ----------------------------------------------------------------------------- 4. constructed ties
@pytest.mark.parametrize("scoring,n,k,c", SMALL)
def test_twin_relations_tie_bitwise(L, gpu_device, scoring, n, k, c):
    gen = torch.Generator().manual_seed(41)
    n_rel, a, b, p = 5, 1, 3, 200
    m = random_model(gen, scoring, n, k, c, n_rel, gpu_device)
    e = m.relation_embed.weight.clone()
    e[b] = e[a]
    w = m.gat_trans_M
    if w is not None:
        w = w.clone()
        w[b] = w[a]
    model = Model(m.T, e, w, scoring)
    h, t = pairs(gen, n, p, gpu_device)
    for side in ("tail", "head"):
        s = L.score_relations(model, h, t, side=side)
        assert torch.equal(bits(s[:, a]), bits(s[:, b]))
        sn = s.cpu().numpy()
        for truth, twin in ((a, b), (b, a)):
            r = torch.full_like(h, truth)
            res = L.rank_relations(model, h, r, t, side=side)
            wb, we = RC.counts(sn, r.cpu().numpy())
            assert res.better.cpu().tolist() == wb.tolist() and res.equal.cpu().tolist() == we.tolist()
            assert bool((res.equal >= 1).all())                        # the twin counts as a tie ...
            known = L.KnownTriples(h, torch.full_like(h, twin), t, n, n_rel)
            res_f = L.rank_relations(model, h, r, t, known=known, side=side)
            assert torch.equal(res_f.equal, res.equal - 1) and torch.equal(res_f.better, res.better)   # ... until filtered
        top = L.predict_relations(model, h, t, k=n_rel, side=side)
        ids = top.ids.cpu().numpy()
        assert ids.tolist() == RC.topk(sn, n_rel)[0].tolist()
        pos_a, pos_b = np.nonzero(ids == a)[1], np.nonzero(ids == b)[1]
        assert np.array_equal(pos_b, pos_a + 1)                        # the smaller id first, the twin right behind it
        known = L.KnownTriples(h, torch.full_like(h, a), t, n, n_rel)
        top = L.predict_relations(model, h, t, k=n_rel, known=known, side=side)
        ids_f = top.ids.cpu().numpy()
        assert not (ids_f == a).any() and (ids_f[:, -1] == -1).all() and (ids_f == b).sum() == p
        assert bool(torch.isnan(top.scores[:, -1]).all())


# ----------------------------------------------------------------------------- 5. NaN
@pytest.mark.parametrize("scoring,n,k,c", SMALL)
def test_a_nan_relation_counts_nowhere(L, gpu_device, scoring, n, k, c):
    gen = torch.Generator().manual_seed(43)
    n_rel, sick, p = 5, 2, 130
    m = random_model(gen, scoring, n, k, c, n_rel, gpu_device)
    e = m.relation_embed.weight.clone()
    e[sick, k // 2] = float("nan")
    model = Model(m.T, e, m.gat_trans_M, scoring)
    h, t = pairs(gen, n, p, gpu_device)
    r = torch.randint(0, n_rel, (p,), generator=gen).to(gpu_device)
    s = L.score_relations(model, h, t)
    assert bool(torch.isnan(s[:, sick]).all()) and int(torch.isnan(s).sum()) == p
    sn, rn = s.cpu().numpy(), r.cpu().numpy()
    res = L.rank_relations(model, h, r, t)
    wb, we = RC.counts(sn, rn)
    assert res.better.cpu().tolist() == wb.tolist() and res.equal.cpu().tolist() == we.tolist()
    as_truth = rn == sick
    assert as_truth.any() and not res.better.cpu().numpy()[as_truth].any() and not res.equal.cpu().numpy()[as_truth].any()
    assert int(res.better.max()) <= n_rel - 2                          # never counted against a healthy truth either
    top = L.predict_relations(model, h, t, k=n_rel)
    assert not bool((top.ids == sick).any()) and bool((top.ids[:, -1] == -1).all())
    assert top.ids.cpu().tolist() == RC.topk(sn, n_rel)[0].tolist()
    assert bool(torch.isnan(top.scores[:, -1]).all()) and not bool(torch.isnan(top.scores[:, :-1]).any())


# ----------------------------------------------------------------------------- 6. + 7. model level
@pytest.mark.parametrize("name,scoring", [("encoder_gcn_l2_gatenum", "transr"), ("transe_gcn_l1", "transe")])
def test_golden_model(L, gpu_device, name, scoring):
    model, gd = _golden_model(L, name, gpu_device, scoring)
    model.eval()
    n_rel = model.n_relations
    kh, kr, kt = (torch.from_numpy(gd[x]).to(gpu_device) for x in ("h", "r", "t"))
    known = L.KnownTriples(kh, kr, kt, model.n_entities, n_rel)
    h, r, t = kh[:300], kr[:300], kt[:300]
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    sets = RC.known_sets(h.cpu().numpy(), t.cpu().numpy(), kh.cpu().numpy(), kr.cpu().numpy(), kt.cpu().numpy())
    rn = r.cpu().numpy()
    assert all(int(x) in s_ for x, s_ in zip(rn, sets))                # every truth is known: it must not drop itself
    for side in ("tail", "head"):
        cols = columns_of_score_triples(L, model, h, t, side)
        s = model.score_relations(h, t, side=side, batch_size=64)
        assert torch.equal(bits(s), bits(cols)), side
        assert torch.equal(bits(s), bits(L.score_relations(model, h, t, side=side)))
        wb, we = RC.counts(cols.cpu().numpy(), rn, sets)
        res = model.rank_relations(h, r, t, known=known, side=side, relation_chunk=2)
        assert res.better.cpu().tolist() == wb.tolist() and res.equal.cpu().tolist() == we.tolist(), side
        res2 = L.rank_relations(model, h, r, t, known=known, side=side)
        assert torch.equal(res.better, res2.better) and torch.equal(res.equal, res2.equal) and res.side == side
        top = model.predict_relations(h, t, k=3, known=known, side=side)
        wi, ws = RC.topk(cols.cpu().numpy(), 3, sets)
        assert top.ids.cpu().tolist() == wi.tolist() and top.side == side
        assert np.array_equal(top.scores.cpu().numpy().view(np.uint32), ws.view(np.uint32))
        top2 = L.predict_relations(model, h, t, k=3, known=known, side=side)
        assert torch.equal(top.ids, top2.ids) and torch.equal(bits(top.scores), bits(top2.scores))
    cols = columns_of_score_triples(L, model, h, t, "tail").cpu().numpy()
    for kn, kn_sets in ((known, sets), (None, None)):
        wb, we = RC.counts(cols, rn, kn_sets)
        want = RC.metrics(wb, we, rn, n_rel, ks=(1, 2, 10))
        got = model.evaluate_relation_prediction(h, r, t, known=kn, ks=(1, 2, 10), batch_size=100)
        RC.same_metrics(got, want)
        RC.same_metrics(L.evaluate_relation_prediction(model, h, r, t, known=kn, ks=(1, 2, 10)), want)
    assert not model.training
    model.train()                                          # from training mode: evaluated in eval mode, the mode restored
    RC.same_metrics(model.evaluate_relation_prediction(h, r, t, ks=(1, 2, 10)), want)
    assert model.training
    model.predict_relations(h[:5], t[:5], k=2)
    assert model.training                                  # (the other entry points leave the mode alone)
    for k_, v in model.state_dict().items():
        v0 = params[k_]
        if v.is_sparse:
            v, v0 = v.coalesce().values(), v0.coalesce().values()
        assert torch.equal(v, v0), k_


def test_empty_input_and_device_checks(L, gpu_device):
    gen = torch.Generator().manual_seed(3)
    m = random_model(gen, "transe", 30, 16, 16, 4, gpu_device)
    model = Model(m.T, m.relation_embed.weight, None, "transe")
    e = torch.zeros(0, dtype=torch.int64, device=gpu_device)
    s = L.score_relations(model, e, e)
    assert s.shape == (0, 4) and s.dtype == torch.float32 and s.device == m.T.device
    res = L.rank_relations(model, e, e, e)
    assert res.better.shape == (0,) and res.better.dtype == torch.int64 and res.rank.shape == (0,)
    top = L.predict_relations(model, e, e, k=3)
    assert top.ids.shape == (0, 3) and top.scores.shape == (0, 3) and top.ids.device == m.T.device
    got = L.evaluate_relation_prediction(model, e, e, e)
    assert got["n"] == 0 and got["per_relation"]["n"].tolist() == [0] * 4
    h = torch.tensor([1, 2, 3])                             # ids from the host are taken to the device; a bad one raises
    assert L.score_relations(model, h, h).shape == (3, 4)
    with pytest.raises(IndexError):
        L.score_relations(model, torch.tensor([1, 30]), torch.tensor([0, 0]))
    with pytest.raises(IndexError):
        L.rank_relations(model, h, torch.tensor([0, 4, 0]), h)
    known = SimpleNamespace(n_entities=30, n_relations=4, device=torch.device("cpu"))      # a filter that lives elsewhere
    with pytest.raises(ValueError, match="known triples live on"):
        L.rank_relations(model, h, torch.tensor([0, 1, 2]), h, known=known)
