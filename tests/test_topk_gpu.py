"""GPU: filtered top-k link prediction (literalkg_amd/topk.py, lkg_topk.hip) against a float64 oracle restated here.

The oracle computes every distance d64(q, x) in float64 from the f32 inputs and the margin of DESIGN.md section 3.6a,
    E(q, x) = (k + 2) u (|p_x| + |q|)^2  +  2 sqrt(d(q, x)) (dq + dp_x)  +  (dq + dp_x)^2,      u = 2^-24,
that bounds the device's rounding (dp_x: the TransR projection's error, dq: the query's).  A correct top-k list then
satisfies, for every returned c and every eligible x that was not returned, d64(c) <= d64(x) + E(q, c) + E(q, x); the
reported score lies within E (plus the rounding of |q|^2 + s) of d64; and the number of returned ids is
min(k, #eligible) exactly.  Integer-valued tables make every f32 step exact: there the lists must equal the oracle's."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import golden_cfg, golden_params, load_golden

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


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
    """What predict_topk reads of a LiteralKG, over a given table."""

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


# ----------------------------------------------------------------------------- float64 oracle
def oracle(table, relemb, trans_m, scoring, side, ids, r, known=None, cand=None, chunk=1 << 17):
    """Per query row (input order) a generator over candidate chunks of (cand ids, d64, E, eligible), plus q-level data.
    Returns a function chunks(i_rows) -> iterator; d64 is the distance (dot: -2 q.p), E its margin."""
    dev = table.device
    n, c_dim = table.shape
    n_rel = relemb.shape[0]
    b = ids.numel()
    cand_all = torch.arange(n, device=dev) if cand is None else cand.to(dev).long()
    kkeys = None
    if known is not None:
        kh, kr, kt = (x.long() for x in known)
        kkeys = torch.unique((kh * n_rel + kr) * n + kt)
        pkeys = torch.unique(kh * n + kt)
    rel_list = [None] if r is None else torch.unique(r).tolist()
    qs, dqs, ws = torch.zeros(b, relemb.shape[1] if scoring != "dot" else c_dim, dtype=torch.float64, device=dev), \
        torch.zeros(b, dtype=torch.float64, device=dev), {}
    eps_p = 2.0 * (c_dim + 4) * U
    for rr in rel_list:
        idx = torch.arange(b, device=dev) if rr is None else torch.nonzero(r == rr, as_tuple=True)[0]
        x = table[ids[idx]].double()
        if scoring == "transr":
            w = trans_m[rr].double()
            pq, dpq = x @ w, eps_p * (x.abs() @ w.abs()).norm(dim=1)
        else:
            pq, dpq = x, torch.zeros(idx.numel(), dtype=torch.float64, device=dev)
        if scoring == "dot":
            q, dq = pq, dpq
        else:
            q = pq + (1.0 if side == "tail" else -1.0) * relemb[rr].double()
            dq = dpq + U * q.norm(dim=1)
        qs[idx], dqs[idx] = q, dq

    def rows(rr, lo, hi):
        x = table[cand_all[lo:hi]].double()
        if scoring == "transr":
            w = trans_m[rr].double()
            return x @ w, eps_p * (x.abs() @ w.abs()).norm(dim=1)
        return x, torch.zeros(hi - lo, dtype=torch.float64, device=dev)

    def chunks(i):
        """(cand ids, d64, E, eligible) over the candidates, in chunks, for query row i (a 0-d index)."""
        rr = None if r is None else int(r[i])
        q, dq = qs[i], dqs[i]
        kd = q.numel()
        for lo in range(0, cand_all.numel(), chunk):
            hi = min(cand_all.numel(), lo + chunk)
            p, dp = rows(rr, lo, hi)
            cid = cand_all[lo:hi]
            if scoring == "dot":
                d = -2.0 * (p @ q)
            else:
                d = ((p - q[None, :]) ** 2).sum(1)
            dd = dq + dp
            e = (kd + 2) * U * (p.norm(dim=1) + q.norm()) ** 2 + 2.0 * d.clamp_min(0).sqrt() * dd + dd * dd
            elig = ~torch.isnan(d)
            if kkeys is not None:
                qid = int(ids[i])
                if rr is None:
                    keys = qid * n + cid if side == "tail" else cid * n + qid
                    elig &= ~torch.isin(keys, pkeys)
                else:
                    keys = (qid * n_rel + rr) * n + cid if side == "tail" else (cid * n_rel + rr) * n + qid
                    elig &= ~torch.isin(keys, kkeys)
            yield cid, d, e, elig
    return chunks


def check_topk(res, chunks, k, scoring, what=""):
    ids, sc, ks = res.ids.cpu(), res.scores.cpu(), res.kernel_scores.cpu()
    assert ids.shape[1] == k and sc.shape == ids.shape and ks.shape == ids.shape
    for i in range(ids.shape[0]):
        row = ids[i]
        m = int((row >= 0).sum())
        assert bool((row[:m] >= 0).all()) and bool((row[m:] == -1).all()), (what, i, row)
        assert bool(torch.isnan(sc[i, m:]).all()) and bool(torch.isnan(ks[i, m:]).all()), (what, i)
        got = row[:m].tolist()
        assert len(set(got)) == m, (what, i, got)
        # sorted by (kernel score, id)
        for a in range(m - 1):
            assert ks[i, a] < ks[i, a + 1] or (ks[i, a] == ks[i, a + 1] and got[a] < got[a + 1]), (what, i, a)
        if scoring == "dot":
            assert bool((sc[i, :m][1:] <= sc[i, :m][:-1]).all()), (what, i)
        else:
            assert bool((sc[i, :m][1:] >= sc[i, :m][:-1]).all()), (what, i)
        n_elig, worst_in, best_out = 0, -math.inf, math.inf
        got_t = torch.tensor(got, dtype=torch.int64)
        for cid, d, e, elig in chunks(i):
            cid, d, e, elig = cid.cpu(), d.cpu(), e.cpu(), elig.cpu()
            n_elig += int(elig.sum())
            inside = torch.isin(cid, got_t)
            assert bool(elig[inside].all()), (what, i, "a returned id is not eligible")
            if inside.any():
                worst_in = max(worst_in, float((d[inside] - e[inside]).max()))
                # the reported score against d64 (dot: q.p = -d / 2)
                pos = {int(c): j for j, c in enumerate(got)}
                for c_, d_, e_ in zip(cid[inside].tolist(), d[inside].tolist(), e[inside].tolist()):
                    v = float(sc[i, pos[c_]])
                    if scoring == "dot":
                        assert abs(v - (-0.5 * d_)) <= 0.5 * e_ + 1e-30, (what, i, c_, v, d_, e_)
                    else:
                        assert abs(v - d_) <= e_ + 4 * U * abs(d_) + 1e-30, (what, i, c_, v, d_, e_)
            out = elig & ~inside
            if out.any():
                best_out = min(best_out, float((d[out] + e[out]).min()))
        assert m == min(k, n_elig), (what, i, m, n_elig)
        assert worst_in <= best_out, (what, i, worst_in, best_out)


def draw_known(gen, n, n_rel, ids, r, m):
    """triples around the queries (both directions) and random ones"""
    dev = ids.device
    pick = torch.randint(0, ids.numel(), (m,), generator=gen).to(dev)
    other = torch.randint(0, n, (m,), generator=gen).to(dev)
    kh = torch.cat([ids[pick], other[: m // 2], torch.randint(0, n, (m,), generator=gen).to(dev)])
    kt = torch.cat([other, ids[pick][: m // 2], torch.randint(0, n, (m,), generator=gen).to(dev)])
    kr = torch.cat([r[pick], r[pick][: m // 2], torch.randint(0, n_rel, (m,), generator=gen).to(dev)])
    return kh, kr, kt


# ----------------------------------------------------------------------------- 1. exact case
@pytest.mark.parametrize("scoring", ["transe", "dot"])
@pytest.mark.parametrize("side", ["tail", "head"])
def test_exact_integer_tables(L, R, gpu_device, scoring, side):
    """Small integers: every f32 product, sum and the final fma are exact, so ids, scores, tie order and padding must
    equal the float64 oracle's sorted list exactly."""
    gen = torch.Generator().manual_seed(11 + len(scoring) + len(side))
    n, kd, n_rel, k = 300, 8, 3, 20
    table = torch.randint(-2, 3, (n, kd), generator=gen).float().to(gpu_device)
    relemb = torch.randint(-1, 2, (n_rel, kd), generator=gen).float().to(gpu_device)
    model = StandIn(table, relemb, None, scoring)
    b = 50
    ids = torch.randint(0, n, (b,), generator=gen).to(gpu_device)
    r = torch.randint(0, n_rel, (b,), generator=gen).to(gpu_device)
    # rows 0..9: known with almost every candidate -> fewer than k eligible, padded
    heavy = torch.arange(n, device=gpu_device)[torch.randperm(n, generator=gen)[: n - 7].to(gpu_device)]
    kh, kr, kt = draw_known(gen, n, n_rel, ids, r, 400)
    ext = [ids[i].repeat(heavy.numel()) for i in range(10)]
    ext_r = [r[i].repeat(heavy.numel()) for i in range(10)]
    if side == "tail":
        kh, kt = torch.cat([kh] + ext), torch.cat([kt] + [heavy] * 10)
    else:
        kh, kt = torch.cat([kh] + [heavy] * 10), torch.cat([kt] + ext)
    kr = torch.cat([kr] + ext_r)
    known = R.KnownTriples(kh, kr, kt, n, n_rel)
    res = L.predict_topk(model, ids, r, side=side, k=k, known=known, scoring=scoring)
    ch = oracle(table, relemb, None, scoring, side, ids, r, (kh, kr, kt))
    for i in range(b):
        cid, d, _, elig = next(ch(i))
        cid, d, elig = cid[elig].cpu(), d[elig].cpu(), None
        order = sorted(range(cid.numel()), key=lambda j: (float(d[j]), int(cid[j])))[:k]
        want_ids = [int(cid[j]) for j in order] + [-1] * (k - len(order))
        assert res.ids[i].cpu().tolist() == want_ids, (i, res.ids[i].tolist(), want_ids)
        want_sc = [(-0.5 * float(d[j]) if scoring == "dot" else float(d[j])) for j in order]
        got_sc = res.scores[i].cpu().double().tolist()
        assert got_sc[:len(order)] == want_sc, i
        assert all(math.isnan(x) for x in got_sc[len(order):]), i
    assert int((res.ids[:10] == -1).sum()) > 0               # the heavy rows are padded
    assert res.side == side


# ----------------------------------------------------------------------------- 2. random tables
CASES = [("transr", 700, 37, 32, 10), ("transr", 3000, 64, 48, 100), ("transe", 1000, 33, 33, 10),
         ("transe", 513, 64, 64, 128), ("dot", 1000, 32, 32, 10), ("dot", 2000, 300, 300, 17)]


@pytest.mark.parametrize("scoring,n,kd,c,k", CASES)
@pytest.mark.parametrize("side", ["tail", "head"])
def test_random_tables_against_margin(L, R, gpu_device, scoring, n, kd, c, k, side):
    gen = torch.Generator().manual_seed(n + kd + k + len(scoring) + len(side))
    n_rel = 5
    model = random_model(gen, scoring, n, kd, c, n_rel, gpu_device)
    b = 90
    ids = torch.randint(0, n, (b,), generator=gen).to(gpu_device)
    r = torch.randint(0, n_rel, (b,), generator=gen).to(gpu_device)
    known = draw_known(gen, n, n_rel, ids, r, 3 * b)
    kt_ = R.KnownTriples(*known, n, n_rel)
    res = model_res = L.predict_topk(model, ids, r, side=side, k=k, known=kt_, scoring=scoring)
    check_topk(model_res, oracle(model.T, model.relation_embed.weight, model.gat_trans_M, scoring, side, ids, r, known),
               k, scoring, f"{scoring} {side}")
    # no returned (query, r, c) is known
    keys = set(zip(*(x.cpu().tolist() for x in known)))
    for i in range(b):
        for c_ in res.ids[i].cpu().tolist():
            if c_ >= 0:
                trip = (int(ids[i]), int(r[i]), c_) if side == "tail" else (c_, int(r[i]), int(ids[i]))
                assert trip not in keys


# ----------------------------------------------------------------------------- 3. agreement with ranking
@pytest.mark.parametrize("scoring", ["transr", "transe", "dot"])
@pytest.mark.parametrize("side", ["tail", "head"])
def test_agrees_with_rank_triples_bit_for_bit(L, R, gpu_device, scoring, side):
    gen = torch.Generator().manual_seed(400 + len(scoring) + len(side))
    n, kd, c, n_rel, k = 600, 40, 40, 4, 128
    model = random_model(gen, scoring, n, kd, c, n_rel, gpu_device)
    # a few bit-identical rows, so that ties occur
    model.T[500:510] = model.T[100:110]
    m_all = 4000
    h = torch.randint(0, n, (m_all,), generator=gen).to(gpu_device)
    t = torch.randint(0, n, (m_all,), generator=gen).to(gpu_device)
    rr = torch.randint(0, n_rel, (m_all,), generator=gen).to(gpu_device)
    h[:10], t[:10] = torch.arange(100, 110, device=gpu_device), torch.arange(100, 110, device=gpu_device)
    test = torch.arange(0, 400, device=gpu_device)
    train = torch.arange(400, m_all, device=gpu_device)
    keys_test = set(zip(h[test].tolist(), rr[test].tolist(), t[test].tolist()))
    keep = torch.tensor([(a, b_, c_) not in keys_test for a, b_, c_ in
                         zip(h[train].tolist(), rr[train].tolist(), t[train].tolist())], device=gpu_device)
    train = train[keep]
    known = R.KnownTriples(h[train], rr[train], t[train], n, n_rel)
    th, tr_, tt = h[test], rr[test], t[test]
    rk = R.rank_triples(model, th, tr_, tt, side=side, known=known, scoring=scoring)
    q_ids, truth = (th, tt) if side == "tail" else (tt, th)
    res = L.predict_topk(model, q_ids, tr_, side=side, k=k, known=known, scoring=scoring)
    ids, ks = res.ids.cpu(), res.kernel_scores.cpu()
    better, equal, truth = rk.better.cpu(), rk.equal.cpu(), truth.cpu()
    n_checked = 0
    for i in range(th.numel()):
        bt, eq = int(better[i]), int(equal[i])
        if bt + eq >= k:
            continue
        n_checked += 1
        row = ids[i].tolist()
        assert int(truth[i]) in row, (i, bt, eq)
        pos = row.index(int(truth[i]))
        assert bt <= pos <= bt + eq, (i, pos, bt, eq)
        assert int((ks[i] == ks[i, pos]).sum()) == eq + 1, (i, eq)
    assert n_checked >= 20, n_checked


# ----------------------------------------------------------------------------- 4. filter
def test_filter_any_relation_and_padding(L, R, gpu_device):
    gen = torch.Generator().manual_seed(9)
    n, kd, n_rel, k = 400, 16, 3, 30
    model = random_model(gen, "dot", n, kd, kd, n_rel, gpu_device)
    ids = torch.arange(0, 40, device=gpu_device)
    r = torch.randint(0, n_rel, (40,), generator=gen).to(gpu_device)
    kh, kr, kt = draw_known(gen, n, n_rel, ids, r, 300)
    # query 0 knows all but 5 candidates, under relations other than its own
    rest = torch.arange(5, n, device=gpu_device)
    kh = torch.cat([kh, torch.zeros_like(rest)])
    kt = torch.cat([kt, rest])
    kr = torch.cat([kr, (r[0] + 1 + rest % (n_rel - 1)) % n_rel])
    known = R.KnownTriples(kh, kr, kt, n, n_rel)
    res = L.predict_topk(model, ids, None, side="tail", k=k, known=known, scoring="dot")
    check_topk(res, oracle(model.T, model.relation_embed.weight, None, "dot", "tail", ids, None, (kh, kr, kt)), k,
               "dot", "r=None")
    pairs = set(zip(kh.tolist(), kt.tolist()))
    for i in range(40):
        for c_ in res.ids[i].tolist():
            if c_ >= 0:
                assert (i, c_) not in pairs
    got0 = [x for x in res.ids[0].tolist() if x >= 0]
    assert set(got0) <= {0, 1, 2, 3, 4} and res.ids[0].tolist()[len(got0):] == [-1] * (k - len(got0))
    # with r, only (0, r0, c) drops: query 0 has its full list
    res_r = L.predict_topk(model, ids, r, side="tail", k=k, known=known, scoring="dot")
    assert int((res_r.ids[0] >= 0).sum()) == k


# ----------------------------------------------------------------------------- 5. candidates
@pytest.mark.parametrize("scoring", ["transr", "transe", "dot"])
def test_candidate_subset(L, R, gpu_device, scoring):
    gen = torch.Generator().manual_seed(21 + len(scoring))
    n, kd, c, n_rel, k = 2000, 24, 24, 3, 12
    model = random_model(gen, scoring, n, kd, c, n_rel, gpu_device)
    cand = torch.randperm(n, generator=gen)[:333].to(gpu_device)           # unsorted entity ids
    ids = torch.randint(0, n, (70,), generator=gen).to(gpu_device)
    r = torch.randint(0, n_rel, (70,), generator=gen).to(gpu_device)
    known = draw_known(gen, n, n_rel, ids, r, 500)
    kt_ = R.KnownTriples(*known, n, n_rel)
    for side in ("tail", "head"):
        res = L.predict_topk(model, ids, r, side=side, k=k, known=kt_, scoring=scoring, candidates=cand)
        assert bool(torch.isin(res.ids[res.ids >= 0], cand).all())
        check_topk(res, oracle(model.T, model.relation_embed.weight, model.gat_trans_M, scoring, side, ids, r, known,
                               cand), k, scoring, f"cand {scoring} {side}")


# ----------------------------------------------------------------------------- 6. invariance and shapes
def test_invariance_splits_and_batches(L, R, gpu_device):
    gen = torch.Generator().manual_seed(66)
    n, kd, n_rel = 9000, 32, 3
    for scoring, k in (("transr", 10), ("transe", 100), ("dot", 128)):
        model = random_model(gen, scoring, n, kd, kd, n_rel, gpu_device)
        ids = torch.randint(0, n, (150,), generator=gen).to(gpu_device)
        r = torch.randint(0, n_rel, (150,), generator=gen).to(gpu_device)
        kt_ = R.KnownTriples(*draw_known(gen, n, n_rel, ids, r, 400), n, n_rel)
        base = L.predict_topk(model, ids, r, k=k, known=kt_, scoring=scoring)
        for splits in (0, 1, 3, 17):
            for bs in (None, 7, 1000):
                got = L.predict_topk(model, ids, r, k=k, known=kt_, scoring=scoring, splits=splits, batch_size=bs)
                assert torch.equal(got.ids, base.ids), (scoring, splits, bs)
                assert torch.equal(got.scores.nan_to_num(7.0), base.scores.nan_to_num(7.0)), (scoring, splits, bs)
                assert torch.equal(got.kernel_scores.nan_to_num(7.0), base.kernel_scores.nan_to_num(7.0))
        # the kernel entry point directly, with its own split counts
        from literalkg_amd import ops
        q = torch.randn(77, kd, generator=gen).to(gpu_device)
        pn = ops.rank_sqnorm(model.T)
        ref = ops.topk_select(q, model.T, pn, k)
        for splits in (1, 3, 17, 64):
            got = ops.topk_select(q, model.T, pn, k, splits=splits)
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), splits


@pytest.mark.parametrize("scoring", ["transe", "dot", "transr"])
def test_odd_shapes(L, R, gpu_device, scoring):
    gen = torch.Generator().manual_seed(77 + len(scoring))
    n_rel = 2
    # N not a multiple of 256, odd k_dim on a row stride that is not a multiple of 4 (the non-vector path)
    kd = 37
    base = torch.randn(1001, kd + 1, generator=gen).to(gpu_device)
    table = base[:, :kd]
    model = random_model(gen, scoring, 1001, kd, kd, n_rel, gpu_device)
    model.T = table
    model.entity_embed.weight = table
    ids = torch.randint(0, 1001, (65,), generator=gen).to(gpu_device)
    r = torch.randint(0, n_rel, (65,), generator=gen).to(gpu_device)
    for side in ("tail", "head"):
        res = L.predict_topk(model, ids, r, side=side, k=13, scoring=scoring)
        check_topk(res, oracle(table, model.relation_embed.weight, model.gat_trans_M, scoring, side, ids, r), 13,
                   scoring, f"odd {scoring} {side}")
    # N < k: every candidate, then padding
    small = random_model(gen, scoring, 6, 8, 8, n_rel, gpu_device)
    ids = torch.tensor([0, 5, 3], device=gpu_device)
    r = torch.tensor([0, 1, 1], device=gpu_device)
    res = L.predict_topk(small, ids, r, k=10, scoring=scoring)
    assert bool((res.ids[:, :6] >= 0).all()) and bool((res.ids[:, 6:] == -1).all())
    assert sorted(res.ids[0, :6].tolist()) == list(range(6))
    check_topk(res, oracle(small.T, small.relation_embed.weight, small.gat_trans_M, scoring, "tail", ids, r), 10, scoring)
    # B = 0
    e = torch.zeros(0, dtype=torch.int64, device=gpu_device)
    res = L.predict_topk(small, e, e, k=4, scoring=scoring)
    assert res.ids.shape == (0, 4) and res.scores.shape == (0, 4)


# ----------------------------------------------------------------------------- 7. golden model
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
    known = R.KnownTriples(h, r, t, model.n_entities, model.n_relations)
    th, tr_, tt = h[:200], r[:200], t[:200]
    rank_before = model.rank_triples(th, tr_, tt, side="both", known=known)
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for side, qid in (("tail", th), ("head", tt)):
        res = model.predict_topk(qid, tr_, side=side, k=10, known=known)
        assert not model.training                              # the mode is left as it was
        with torch.no_grad():
            table = model._table_for_inference().detach()
        tm = model.gat_trans_M.detach() if scoring == "transr" else None
        check_topk(res, oracle(table, model.relation_embed.weight.detach(), tm, scoring, side, qid, tr_, (h, r, t)), 10,
                   scoring, f"{name} {side}")
    for k_, v in model.state_dict().items():
        v0 = params[k_]
        if v.is_sparse:
            v, v0 = v.coalesce().values(), v0.coalesce().values()
        assert torch.equal(v, v0), k_
    rank_after = model.rank_triples(th, tr_, tt, side="both", known=known)
    model.train()
    model.predict_topk(th[:5], tr_[:5], k=3, known=known)
    assert model.training
    assert torch.equal(rank_before.better, rank_after.better) and torch.equal(rank_before.equal, rank_after.equal)
    assert model(th[:4], tt[:4], device=gpu_device, mode="no_such_mode") is None


# ----------------------------------------------------------------------------- 8. large
def test_two_million_candidates(L, R, gpu_device):
    gen = torch.Generator(device=gpu_device).manual_seed(2026)
    n, kd, n_rel, k = 2_000_000, 300, 2, 10
    table = torch.randn(n, kd, generator=gen, device=gpu_device)
    relemb = torch.randn(n_rel, kd, generator=gen, device=gpu_device) * 0.3
    model = StandIn(table, relemb, None, "transe")
    ids = torch.tensor([0, 5, 1_999_990, 123_456, 1_500_000, 77], device=gpu_device)
    r = torch.tensor([0, 1, 0, 1, 0, 1], device=gpu_device)
    # plant near neighbours past 2^31 / 4 / k rows
    near = torch.arange(n - 6, n, device=gpu_device)
    table[near] = table[ids] + relemb[r] + 0.05 * torch.randn(6, kd, generator=gen, device=gpu_device)
    known = (ids[:2], r[:2], near[:2])
    kt_ = R.KnownTriples(*known, n, n_rel)
    res = L.predict_topk(model, ids, r, k=k, known=kt_, scoring="transe")
    check_topk(res, oracle(table, relemb, None, "transe", "tail", ids, r, known, chunk=1 << 19), k, "transe", "2M")
    ids_l = res.ids.cpu().tolist()
    assert all(ids_l[i][0] == n - 6 + i for i in range(2, 6))     # the planted tails come first
    assert all(n - 6 + i not in ids_l[i] for i in range(2))        # unless known


# ----------------------------------------------------------------------------- 9. errors
def test_errors(L, R, gpu_device):
    gen = torch.Generator().manual_seed(3)
    model = random_model(gen, "transe", 300, 16, 16, 3, gpu_device)
    ids = torch.tensor([0, 1, 2], device=gpu_device)
    r = torch.tensor([0, 1, 2], device=gpu_device)
    for k in (0, 129):
        with pytest.raises(ValueError):
            L.predict_topk(model, ids, r, k=k, scoring="transe")
    with pytest.raises(ValueError):
        L.predict_topk(model, ids, r, side="both", scoring="transe")
    with pytest.raises(ValueError):
        L.predict_topk(model, ids, r, scoring="distmult")
    with pytest.raises(ValueError):
        L.predict_topk(model, ids, None, scoring="transe")          # r needed
    with pytest.raises(IndexError):
        L.predict_topk(model, torch.tensor([0, 300, 1], device=gpu_device), r, scoring="transe")
    with pytest.raises(IndexError):
        L.predict_topk(model, ids, torch.tensor([0, 3, 1], device=gpu_device), scoring="transe")
    with pytest.raises(IndexError):
        L.predict_topk(model, ids, r, scoring="transe", candidates=torch.tensor([1, 300], device=gpu_device))
    with pytest.raises(IndexError):
        L.predict_topk(model, ids, r, scoring="transe", candidates=torch.tensor([-1, 2], device=gpu_device))
    with pytest.raises(ValueError):
        L.predict_topk(model, ids, r, scoring="transe", candidates=torch.tensor([4, 2, 4], device=gpu_device))
    other = R.KnownTriples(ids, r, ids, 301, 3)
    with pytest.raises(ValueError):
        L.predict_topk(model, ids, r, scoring="transe", known=other)
    cpu_known = SimpleNamespace(n_entities=300, device=torch.device("cpu"))
    with pytest.raises(ValueError):
        L.predict_topk(model, ids, r, scoring="transe", known=cpu_known)
    with pytest.raises(ValueError):
        L.predict_topk(model, ids, r, scoring="transr")                # no gat_trans_M
    # nothing left pending: a valid call works
    ok = L.predict_topk(model, ids, r, k=5, scoring="transe")
    assert ok.ids.shape == (3, 5) and bool((ok.ids >= 0).all())
    # a NaN candidate row is never selected
    saved = model.T[7].clone()
    model.T[7] = float("nan")
    res = L.predict_topk(model, ids, r, k=128, scoring="transe")
    model.T[7] = saved
    assert not bool((res.ids == 7).any()) and bool((res.ids >= 0).all())
