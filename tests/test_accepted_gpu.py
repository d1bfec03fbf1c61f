"""GPU: threshold retrieval (literalkg_amd/accepted.py, lkg_accept.hip, lkg_accept_order) -- exact, no tolerance.

The accepted list of a query is defined by the reported score of every (query, candidate), one float32 compare, the
known-triple filter and the order (kernel score, id); accepted_cases.py restates that in numpy.  The dense scores come
from an int64 computation (integer tables: every f32 step is exact) or from score_triples over all B x N explicit triples,
whose bits the lists must carry.  Shapes sit on the tile edges: B in {1, 70} (64 query rows per workgroup), N in
{1, 257, 700} (256-candidate tiles), widths 5, 30, 64 and 300 (16-element chunks, 4-element vectors)."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import accepted_cases as AC
from conftest import golden_cfg, golden_params, load_golden

pytestmark = pytest.mark.gpu

INF = float("inf")


@pytest.fixture(scope="module")
def L(gpu_device):
    import __graft_entry__ as ge
    ge.build()
    import literalkg_amd
    return literalkg_amd


@pytest.fixture(scope="module")
def R(L):
    from literalkg_amd import ranking
    return ranking


class StandIn:
    """What predict_accepted reads of a LiteralKG, over a given table."""

    def __init__(self, table, relemb, trans_m=None, scoring="transr"):
        self.T = table
        self.entity_embed = SimpleNamespace(weight=table)
        self.relation_embed = SimpleNamespace(weight=relemb)
        self.gat_trans_M = trans_m
        self.n_entities, self.n_relations = table.shape[0], relemb.shape[0]
        self.relation_dim = relemb.shape[1]
        self.scoring = scoring
        self.training = False

    def _table_for_inference(self):
        return self.T


def random_model(gen, scoring, n, k, c, n_rel, dev):
    table = torch.randn(n, c, generator=gen).to(dev)
    relemb = torch.randn(n_rel, k, generator=gen).to(dev) * 0.3
    trans_m = (torch.randn(n_rel, c, k, generator=gen) / math.sqrt(c)).to(dev) if scoring == "transr" else None
    return StandIn(table, relemb, trans_m, scoring)


def bits(x):
    return x.detach().cpu().contiguous().numpy().view(np.uint32)


def rows_of(res):
    """The result as per-row (ids, values, keys) numpy lists; the CSR invariants on the way."""
    rp = res.rowptr.cpu().numpy()
    assert res.rowptr.dtype == torch.int64 and res.counts.dtype == torch.int64 and res.ids.dtype == torch.int64
    assert res.scores.dtype == torch.float32 and res.kernel_scores.dtype == torch.float32
    assert rp[0] == 0 and rp[-1] == res.ids.numel() == res.scores.numel() == res.kernel_scores.numel()
    assert np.array_equal(np.diff(rp), res.counts.cpu().numpy())
    ids, v, k = res.ids.cpu().numpy(), res.scores.cpu().numpy(), res.kernel_scores.cpu().numpy()
    return [(ids[a:b], v[a:b], k[a:b]) for a, b in zip(rp[:-1], rp[1:])]


def assert_lists(res, want, what=""):
    got = rows_of(res)
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[0].tolist() == w[0].tolist(), (what, i, g[0][:8], w[0][:8])
        assert np.array_equal(g[1].view(np.uint32), w[1].view(np.uint32)), (what, i, "scores")
        assert np.array_equal(g[2].view(np.uint32), w[2].view(np.uint32)), (what, i, "kernel scores")


def same_result(a, b):
    return all(torch.equal(getattr(a, f), getattr(b, f)) for f in ("rowptr", "ids", "scores", "kernel_scores", "counts"))


def known_sets(known, ids, r, side):
    """Per query the candidate ids known for it: under its relation, or (r None) under any."""
    kh, kr, kt = (x.cpu().numpy() for x in known)
    mine, other = (kh, kt) if side == "tail" else (kt, kh)
    ids = ids.cpu().tolist()
    rr = r.cpu().tolist() if r is not None else None
    return [set(other[(mine == q) & ((kr == rr[i]) if rr is not None else True)].tolist()) for i, q in enumerate(ids)]


def draw_known(gen, n, n_rel, ids, r, m):
    """triples around the queries (both directions) and random ones, some of them repeated"""
    dev = ids.device
    pick = torch.randint(0, ids.numel(), (m,), generator=gen).to(dev)
    other = torch.randint(0, n, (m,), generator=gen).to(dev)
    kh = torch.cat([ids[pick], other, torch.randint(0, n, (m,), generator=gen).to(dev), ids[pick][:5]])
    kt = torch.cat([other, ids[pick], torch.randint(0, n, (m,), generator=gen).to(dev), other[:5]])
    kr = torch.cat([r[pick], r[pick], torch.randint(0, n_rel, (m,), generator=gen).to(dev), r[pick][:5]])
    return kh, kr, kt


def observed_thresholds(values, r, n_rel, lower, rank=20):
    """One threshold per relation, each an OBSERVED score: the rank-th best of the first row with that relation (ties at
    the threshold are then certain); a relation without a row takes the last one found."""
    thr, last = [], None
    rr = r.cpu().tolist()
    for rho in range(n_rel):
        if rho in rr:
            row = values[rr.index(rho)]
            row = np.sort(row[~np.isnan(row)])
            row = row if lower else row[::-1]
            last = float(row[min(rank, row.size) - 1])
        thr.append(last)
    fill = next(x for x in thr if x is not None)
    return torch.tensor([fill if x is None else x for x in thr], dtype=torch.float32)


def dense_scores(L, model, ids, r, side, scoring, cand=None):
    """values, keys float32[B, N]: score_triples over all B x N explicit triples (reported and kernel scores)."""
    dev = ids.device
    c = torch.arange(model.n_entities, device=dev) if cand is None else cand
    b, n = ids.numel(), c.numel()
    q, cc = ids.repeat_interleave(n), c.repeat(b)
    rr = (r if r is not None else torch.zeros_like(ids)).repeat_interleave(n)
    h, t = (q, cc) if side == "tail" else (cc, q)
    v = L.score_triples(model, h, rr, t, scoring=scoring, side=side)
    k = L.score_triples(model, h, rr, t, scoring=scoring, side=side, kernel_scores=True)
    return v.view(b, n).cpu().numpy(), k.view(b, n).cpu().numpy()


# ----------------------------------------------------------------------------- 1. exact case
@pytest.mark.parametrize("scoring", ["transe", "dot"])
@pytest.mark.parametrize("side", ["tail", "head"])
@pytest.mark.parametrize("b,n,kd", [(70, 700, 5), (1, 257, 30), (70, 257, 64), (3, 1, 300)])
def test_exact_integer_tables(L, R, gpu_device, scoring, side, b, n, kd):
    """Small integers: every f32 product, sum and the final fma are exact, so the lists equal an int64 computation."""
    gen = torch.Generator().manual_seed(11 + len(scoring) + len(side) + n + kd)
    n_rel = 3
    table = torch.randint(-2, 3, (n, kd), generator=gen)
    relemb = torch.randint(-1, 2, (n_rel, kd), generator=gen)
    ids = torch.randint(0, n, (b,), generator=gen)
    r = torch.randint(0, n_rel, (b,), generator=gen)
    q = table[ids] + (0 if scoring == "dot" else (1 if side == "tail" else -1)) * relemb[r]
    dots = q @ table.T                                                 # int64 throughout
    if scoring == "dot":
        keys = (-2 * dots).numpy().astype(np.float32)                  # (exact: small integers)
        values = np.float32(-0.5) * keys                               # the report is -s / 2: a zero dot product is -0.0
    else:
        keys = ((table * table).sum(1)[None, :] - 2 * dots).numpy().astype(np.float32)
        values = ((q * q).sum(1, keepdim=True) + (table * table).sum(1)[None, :] - 2 * dots).numpy().astype(np.float32)
    lower = scoring != "dot"
    thr = observed_thresholds(values, r, n_rel, lower, rank=10)
    model = StandIn(table.float().to(gpu_device), relemb.float().to(gpu_device), None, scoring)
    ids_d, r_d = ids.to(gpu_device), r.to(gpu_device)
    known = draw_known(gen, n, n_rel, ids_d, r_d, 2 * b + 3)
    kt_ = R.KnownTriples(*known, n, n_rel)
    want = AC.accepted_lists(values, keys, np.arange(n), thr.numpy()[r.numpy()], lower,
                             known_sets(known, ids, r, side))
    res = L.predict_accepted(model, ids_d, r_d, thr.to(gpu_device), side=side, known=kt_, scoring=scoring)
    assert_lists(res, want, f"{scoring} {side}")
    assert res.side == side and (n == 1 or int(res.counts.sum()) > 0)
    assert torch.equal(L.count_accepted(model, ids_d, r_d, thr.to(gpu_device), side=side, known=kt_, scoring=scoring),
                       res.counts)


# ----------------------------------------------------------------------------- 2, 3. score_triples and top-k
SHAPES = {"big": (70, 700), "small": (1, 257)}
WIDTHS = {("transr", "big"): (37, 32), ("transr", "small"): (30, 32), ("transe", "big"): (300, 300),
          ("transe", "small"): (30, 30), ("dot", "big"): (64, 64), ("dot", "small"): (5, 5)}


@functools.lru_cache(maxsize=None)
def scored_case(L, R, dev, scoring, side, shape):
    """One random case, scored densely once and shared by the tests below (nothing in it is changed afterwards)."""
    b, n = SHAPES[shape]
    kd, c = WIDTHS[scoring, shape]
    gen = torch.Generator().manual_seed(900 + 7 * len(scoring) + len(side) + n)
    n_rel = 4
    model = random_model(gen, scoring, n, kd, c, n_rel, dev)
    model.T[n - 5:n - 2] = model.T[2:5]                                 # bit-identical rows: ties between candidates
    ids = torch.randint(0, n, (b,), generator=gen).to(dev)
    r = torch.randint(0, n_rel, (b,), generator=gen).to(dev)
    values, keys = dense_scores(L, model, ids, r, side, scoring)
    lower = scoring != "dot"
    thr = observed_thresholds(values, r, n_rel, lower)
    kh, kr, kt = draw_known(gen, n, n_rel, ids, r, 3 * b)
    best = torch.from_numpy(np.argsort(values if lower else -values, axis=1)[:, :3].copy()).to(dev)   # known among the best
    q3, r3 = ids[:, None].expand(-1, 3).reshape(-1), r[:, None].expand(-1, 3).reshape(-1)
    kh = torch.cat([kh, q3 if side == "tail" else best.reshape(-1)])
    kt = torch.cat([kt, best.reshape(-1) if side == "tail" else q3])
    kr = torch.cat([kr, r3])
    known = R.KnownTriples(kh, kr, kt, n, n_rel)
    want = AC.accepted_lists(values, keys, np.arange(n), thr.numpy()[r.cpu().numpy()], lower,
                             known_sets((kh, kr, kt), ids, r, side))
    res = L.predict_accepted(model, ids, r, thr.to(dev), side=side, known=known, scoring=scoring)
    return SimpleNamespace(model=model, ids=ids, r=r, thr=thr.to(dev), known=known, want=want, res=res, lower=lower)


CASES = [(s, side, shape) for s in ("transr", "transe", "dot") for side in ("tail", "head") for shape in SHAPES]


@pytest.mark.parametrize("scoring,side,shape", CASES)
def test_equals_score_triples_over_all_pairs(L, R, gpu_device, scoring, side, shape):
    c = scored_case(L, R, gpu_device, scoring, side, shape)
    assert_lists(c.res, c.want, f"{scoring} {side} {shape}")
    lens = [w[0].size for w in c.want]
    assert sum(lens) > 0 and (len(lens) == 1 or len(set(lens)) > 1)     # lists of mixed, non-zero length
    n = L.count_accepted(c.model, c.ids, c.r, c.thr, side=side, known=c.known, scoring=scoring)
    assert n.dtype == torch.int64 and torch.equal(n, c.res.counts)
    # the same thresholds as a TripleThresholds object
    from literalkg_amd.triples import TripleThresholds
    z = torch.zeros(4, dtype=torch.int64)
    fitted = TripleThresholds(c.thr, 0.0, scoring, z, z)
    assert same_result(L.predict_accepted(c.model, c.ids, c.r, fitted, side=side, known=c.known, scoring=scoring), c.res)


@pytest.mark.parametrize("scoring,side,shape", CASES)
def test_prefix_of_topk(L, R, gpu_device, scoring, side, shape):
    c = scored_case(L, R, gpu_device, scoring, side, shape)
    top = L.predict_topk(c.model, c.ids, c.r, side=side, k=128, known=c.known, scoring=scoring)
    thr_q = c.thr[c.r].cpu().numpy()
    for i, (gi, gv, gk) in enumerate(rows_of(c.res)):
        m = min(128, gi.size)
        assert top.ids[i, :m].cpu().tolist() == gi[:m].tolist(), i
        assert np.array_equal(bits(top.scores[i, :m]), gv[:m].view(np.uint32)), i
        assert np.array_equal(bits(top.kernel_scores[i, :m]), gk[:m].view(np.uint32)), i
        if gi.size < 128 and int(top.ids[i, gi.size]) != -1:             # the next best fails the threshold
            nxt = np.float32(top.scores[i, gi.size].item())
            assert not (nxt <= thr_q[i] if c.lower else nxt >= thr_q[i]), (i, nxt, thr_q[i])


# ----------------------------------------------------------------------------- 4. sentinels and saturation
@pytest.mark.parametrize("scoring", ["transe", "dot"])
def test_sentinels_saturation_and_max_total(L, R, gpu_device, scoring):
    gen = torch.Generator().manual_seed(41 + len(scoring))
    n, kd, n_rel, b = 700, 30, 3, 70
    model = random_model(gen, scoring, n, kd, kd, n_rel, gpu_device)
    model.T[7] = float("nan")                                           # a NaN candidate: never accepted
    ids = (8 + torch.randint(0, n - 8, (b,), generator=gen)).to(gpu_device)
    r = torch.randint(0, n_rel, (b,), generator=gen).to(gpu_device)
    known = draw_known(gen, n, n_rel, ids, r, 4 * b)
    kt_ = R.KnownTriples(*known, n, n_rel)
    nothing, everything = (-INF, INF) if scoring != "dot" else (INF, -INF)
    for side in ("tail", "head"):
        res = L.predict_accepted(model, ids, r, nothing, side=side, known=kt_, scoring=scoring)
        assert res.ids.numel() == 0 and not bool(res.counts.any()) and res.rowptr.tolist() == [0] * (b + 1)
        res = L.predict_accepted(model, ids, r, everything, side=side, known=kt_, scoring=scoring)
        sets = known_sets(known, ids, r, side)
        want_n = [n - 1 - len(s - {7}) for s in sets]                   # N minus NaN minus known
        assert res.counts.cpu().tolist() == want_n
        assert torch.equal(L.count_accepted(model, ids, r, everything, side=side, known=kt_, scoring=scoring), res.counts)
        top = L.predict_topk(model, ids, r, side=side, k=128, known=kt_, scoring=scoring)
        for i, (gi, gv, gk) in enumerate(rows_of(res)):
            assert 7 not in gi and not set(gi.tolist()) & sets[i] and len(set(gi.tolist())) == gi.size
            assert bool(np.all((gk[1:] > gk[:-1]) | ((gk[1:] == gk[:-1]) & (gi[1:] > gi[:-1])))), i
            assert top.ids[i].cpu().tolist() == gi[:128].tolist() and np.array_equal(bits(top.scores[i]),
                                                                                      gv[:128].view(np.uint32))
    total = int(res.counts.sum())
    for bs in (None, 7):
        with pytest.raises(ValueError, match="max_total"):
            L.predict_accepted(model, ids, r, everything, side="head", known=kt_, scoring=scoring, max_total=total - 1,
                               batch_size=bs)
        ok = L.predict_accepted(model, ids, r, everything, side="head", known=kt_, scoring=scoring, max_total=total,
                                batch_size=bs)
        assert same_result(ok, res)


# ----------------------------------------------------------------------------- 5. invariance
@pytest.mark.parametrize("scoring", ["transr", "dot"])
def test_invariance(L, R, gpu_device, scoring):
    c = scored_case(L, R, gpu_device, scoring, "tail", "big")
    kw = dict(side="tail", known=c.known, scoring=scoring)
    for bs in (1, 7, None):
        for splits in (0, 1, 3):
            got = L.predict_accepted(c.model, c.ids, c.r, c.thr, batch_size=bs, splits=splits, **kw)
            assert same_result(got, c.res), (bs, splits)
    gen = torch.Generator().manual_seed(5)
    perm = torch.randperm(c.ids.numel(), generator=gen).to(gpu_device)
    got = L.predict_accepted(c.model, c.ids[perm], c.r[perm], c.thr, **kw)
    assert torch.equal(got.counts, c.res.counts[perm])
    mine, base = rows_of(got), rows_of(c.res)
    assert AC.same_lists(mine, [base[j] for j in perm.cpu().tolist()])
    n = c.model.n_entities
    everyone = L.predict_accepted(c.model, c.ids, c.r, c.thr, candidates=torch.arange(n, device=gpu_device), **kw)
    shuffled = L.predict_accepted(c.model, c.ids, c.r, c.thr,
                                  candidates=torch.randperm(n, generator=gen).to(gpu_device), **kw)
    assert same_result(everyone, c.res) and same_result(shuffled, c.res)


# ----------------------------------------------------------------------------- 6. candidates and the any-relation filter
@pytest.mark.parametrize("scoring", ["transr", "transe", "dot"])
def test_candidate_subset(L, R, gpu_device, scoring):
    c = scored_case(L, R, gpu_device, scoring, "head", "big")
    gen = torch.Generator().manual_seed(21)
    cand = torch.randperm(c.model.n_entities, generator=gen)[:200].to(gpu_device)          # unsorted entity ids
    res = L.predict_accepted(c.model, c.ids, c.r, c.thr, side="head", known=c.known, scoring=scoring, candidates=cand)
    inside = set(cand.cpu().tolist())
    want = []
    for wi, wv, wk in c.want:                                           # the full lists, restricted: the order is kept
        keep = np.array([x in inside for x in wi.tolist()], dtype=bool)
        want.append((wi[keep], wv[keep], wk[keep]))
    assert_lists(res, want, f"candidates {scoring}")
    assert 0 < res.ids.numel() < c.res.ids.numel()


def test_any_relation_filter(L, R, gpu_device):
    gen = torch.Generator().manual_seed(9)
    n, kd, n_rel, b = 700, 64, 3, 70
    model = random_model(gen, "dot", n, kd, kd, n_rel, gpu_device)
    ids = torch.randint(0, n, (b,), generator=gen).to(gpu_device)
    r = torch.randint(0, n_rel, (b,), generator=gen).to(gpu_device)
    values, keys = dense_scores(L, model, ids, None, "tail", "dot")
    thr = float(np.sort(values[0])[-30])
    best = torch.from_numpy(np.argsort(-values, axis=1)[:, :4].copy()).to(gpu_device)
    kh = ids[:, None].expand(-1, 4).reshape(-1)
    kr = ((r[:, None] + torch.arange(4, device=gpu_device)[None, :]) % n_rel).reshape(-1)     # under several relations
    known = (kh, kr, best.reshape(-1))
    kt_ = R.KnownTriples(*known, n, n_rel)
    res = L.predict_accepted(model, ids, None, thr, known=kt_, scoring="dot")
    assert_lists(res, AC.accepted_lists(values, keys, np.arange(n), thr, False, known_sets(known, ids, None, "tail")))
    with pytest.raises(ValueError, match="r=None"):
        res.triples()
    # with r only (query, r, c) drops
    res_r = L.predict_accepted(model, ids, r, thr, known=kt_, scoring="dot")
    assert_lists(res_r, AC.accepted_lists(values, keys, np.arange(n), thr, False, known_sets(known, ids, r, "tail")))
    assert res_r.ids.numel() > res.ids.numel() > 0


# ----------------------------------------------------------------------------- 7. golden models
def _golden_model(L, name, dev, scoring):
    gd = load_golden(name)
    cfg = golden_cfg(gd)
    n, n_rel = int(gd["n"]), int(gd["n_rel"])
    a_in = torch.sparse_coo_tensor(torch.from_numpy(gd["a_indices"]), torch.from_numpy(gd["a_values"]), (n, n)).coalesce()
    num = torch.from_numpy(gd["num"]) if "num" in gd else None
    txt = torch.from_numpy(gd["txt"]) if "txt" in gd else None
    m = L.LiteralKG(cfg, n, n_rel, a_in, num, txt, scoring=scoring)
    own = set(m.state_dict().keys())
    m.load_state_dict({k: v for k, v in golden_params(gd).items() if k in own}, strict=False)
    return m.to(dev), gd


@pytest.mark.parametrize("name,scoring", [("encoder_gcn_l2_gatenum", "transr"), ("transe_gcn_l1", "transe")])
def test_golden_model(L, R, gpu_device, name, scoring):
    model, gd = _golden_model(L, name, gpu_device, scoring)
    model.eval()
    h, r, t = (torch.from_numpy(gd[x]).to(gpu_device) for x in ("h", "r", "t"))
    n = model.n_entities
    gen = torch.Generator().manual_seed(1)
    nv = min(300, h.numel() // 2)
    vh, vr, vt = h[:nv], r[:nv], t[:nv]
    corrupt = torch.randint(0, n, (nv,), generator=gen).to(gpu_device)
    fitted = model.fit_triple_thresholds(torch.cat([vh, vh]), torch.cat([vr, vr]), torch.cat([vt, corrupt]),
                                         torch.cat([torch.ones(nv), torch.zeros(nv)]).to(torch.uint8).to(gpu_device))
    known = R.KnownTriples(h[nv:], r[nv:], t[nv:], n, model.n_relations)
    median = float(model.score_triples(vh, vr, vt).median())
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    total = 0
    for thr, kn in ((fitted, known), (median, None)):
        res = model.predict_accepted(vh[:60], vr[:60], thr, known=kn)
        assert not model.training
        ph, pr, pt = res.triples()
        assert ph.numel() == res.ids.numel() and torch.equal(pt, res.ids)
        assert np.array_equal(bits(model.score_triples(ph, pr, pt)), bits(res.scores))
        assert np.array_equal(bits(model.score_triples(ph, pr, pt, kernel_scores=True)), bits(res.kernel_scores))
        if ph.numel():
            ev = model.evaluate_triple_classification(ph, pr, pt, torch.ones(ph.numel(), dtype=torch.uint8,
                                                                             device=gpu_device), thr)
            assert ev["fn"] == 0 and ev["tp"] == ph.numel()
        assert torch.equal(model.count_accepted(vh[:60], vr[:60], thr, known=kn), res.counts)
        total += ph.numel()
        heads = model.predict_accepted(vt[:20], vr[:20], thr, side="head", known=kn)
        ph, pr, pt = heads.triples()
        assert torch.equal(ph, heads.ids)
        assert np.array_equal(bits(model.score_triples(ph, pr, pt, side="head")), bits(heads.scores))
    assert total > 0                                                    # (the median accepts half of the true tails)
    for k_, v in model.state_dict().items():
        v0 = params[k_]
        if v.is_sparse:
            v, v0 = v.coalesce().values(), v0.coalesce().values()
        assert torch.equal(v, v0), k_
    model.train()
    model.predict_accepted(vh[:5], vr[:5], median)
    assert model.training


# ----------------------------------------------------------------------------- 8. large
def test_two_million_candidates(L, R, gpu_device):
    gen = torch.Generator(device=gpu_device).manual_seed(2026)
    n, kd, n_rel = 2_000_000, 300, 2
    table = torch.randn(n, kd, generator=gen, device=gpu_device)
    relemb = torch.randn(n_rel, kd, generator=gen, device=gpu_device) * 0.3
    model = StandIn(table, relemb, None, "transe")
    ids = torch.tensor([0, 5, 1_999_990, 123_456, 1_500_000, 77], device=gpu_device)
    r = torch.tensor([0, 1, 0, 1, 0, 1], device=gpu_device)
    # near neighbours in the last rows: byte offsets past 2^31.  Their squared distance is about 300 * 0.05^2 = 0.75;
    # a query's own row lies at |e_r|^2 ~ 27 and the bulk at ~ 300 * 2.09 ~ 630: a threshold of 8 separates them
    near = torch.arange(n - 6, n, device=gpu_device)
    table[near] = table[ids] + relemb[r] + 0.05 * torch.randn(6, kd, generator=gen, device=gpu_device)
    known = (ids[:2], r[:2], near[:2])
    kt_ = R.KnownTriples(*known, n, n_rel)
    res = L.predict_accepted(model, ids, r, 8.0, known=kt_, scoring="transe")
    assert res.counts.tolist() == [0, 0, 1, 1, 1, 1] and res.ids.tolist() == [n - 4, n - 3, n - 2, n - 1]
    h, rr, t = res.triples()
    assert np.array_equal(bits(L.score_triples(model, h, rr, t, scoring="transe")), bits(res.scores))
    assert bool((res.scores < 2.0).all())
    assert torch.equal(L.count_accepted(model, ids, r, 8.0, known=kt_, scoring="transe"), res.counts)
    assert L.count_accepted(model, ids, r, 8.0, scoring="transe").tolist() == [1] * 6         # unless known


# ----------------------------------------------------------------------------- 9. errors
def test_errors_on_the_device_path(L, R, gpu_device):
    gen = torch.Generator().manual_seed(3)
    model = random_model(gen, "transe", 300, 16, 16, 3, gpu_device)
    ids = torch.tensor([0, 1, 2], device=gpu_device)
    r = torch.tensor([0, 1, 2], device=gpu_device)
    for call in (L.predict_accepted, L.count_accepted):
        with pytest.raises(IndexError):
            call(model, torch.tensor([0, 300, 1], device=gpu_device), r, 1.0, scoring="transe")
        with pytest.raises(IndexError):
            call(model, ids, torch.tensor([0, 3, 1], device=gpu_device), 1.0, scoring="transe")
        with pytest.raises(IndexError):
            call(model, ids, r, 1.0, scoring="transe", candidates=torch.tensor([1, 300], device=gpu_device))
        with pytest.raises(IndexError):
            call(model, ids, r, 1.0, scoring="transe", candidates=torch.tensor([-1, 2], device=gpu_device))
        with pytest.raises(ValueError, match="known triples live on"):
            call(model, ids, r, 1.0, scoring="transe", known=SimpleNamespace(n_entities=300, device=torch.device("cpu")))
        with pytest.raises(ValueError, match="301 entities"):
            call(model, ids, r, 1.0, scoring="transe", known=R.KnownTriples(ids, r, ids, 301, 3))
    # nothing left pending: a valid call works
    ok = L.predict_accepted(model, ids, r, INF, scoring="transe")
    assert ok.counts.tolist() == [300] * 3 and ok.ids.numel() == 900
    assert L.count_accepted(model, ids, r, INF, scoring="transe").tolist() == [300] * 3
