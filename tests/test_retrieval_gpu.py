"""GPU: multi-answer retrieval (literalkg_amd/retrieval.py, lkg_retrieval.hip) -- positions and counts exact, the float64
metrics to a bound worked out from their number of summands.

The place of an answer is defined by the kernel score of every (query, candidate), the known-triple filter with the
query's answers exempt, and the order (kernel score, id); retrieval_cases.py restates that in numpy.  The dense scores
come from an int64 computation (integer tables: every f32 step is exact) or from score_triples(kernel_scores=True) over
all Q x N explicit triples.  Shapes sit on the tile edges: N in {1, 257, 700, 1500} (256-candidate tiles), more than 64
rows per launch, widths 5, 30, 64 and 300, and queries with 1, T, T + 1 and 3 T + 2 answers (T = ops.RETRIEVAL_SLICE keys
per row) next to a query whose answers are all the candidates."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import retrieval_cases as RC
from conftest import golden_cfg, golden_params, load_golden

pytestmark = pytest.mark.gpu

KS = (1, 3, 10, 100, 1000)
EPS = 2.0 ** -52


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
    """What rank_answers reads of a LiteralKG, over a given table."""

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

    def eval(self):
        self.training = False

    def train(self, mode=True):
        self.training = mode


def random_model(gen, scoring, n, k, c, n_rel, dev):
    table = torch.randn(n, c, generator=gen).to(dev)
    relemb = torch.randn(n_rel, k, generator=gen).to(dev) * 0.3
    trans_m = (torch.randn(n_rel, c, k, generator=gen) / math.sqrt(c)).to(dev) if scoring == "transr" else None
    return StandIn(table, relemb, trans_m, scoring)


def draw_triples(gen, n, n_rel, b, sizes, side):
    """b random triples and, per entry of sizes, one query with that many distinct answers (at most n); shuffled."""
    ent = [torch.randint(0, n, (b,), generator=gen)]
    rel = [torch.randint(0, n_rel, (b,), generator=gen)]
    ans = [torch.randint(0, n, (b,), generator=gen)]
    for j, size in enumerate(sizes):
        m = min(size, n)
        ent.append(torch.randint(0, n, (1,), generator=gen).expand(m))
        rel.append(torch.full((m,), j % n_rel))
        ans.append(torch.randperm(n, generator=gen)[:m])
    ent, rel, ans = torch.cat(ent), torch.cat(rel), torch.cat(ans)
    perm = torch.randperm(ent.numel(), generator=gen)
    ent, rel, ans = ent[perm], rel[perm], ans[perm]
    return (ent, rel, ans) if side == "tail" else (ans, rel, ent)


def draw_known(gen, n, n_rel, h, r, t, m):
    """triples around the evaluated ones (both directions), random ones, and some of the evaluated triples themselves"""
    pick = torch.randint(0, h.numel(), (m,), generator=gen)
    other = torch.randint(0, n, (m,), generator=gen)
    kh = torch.cat([h[pick], other, torch.randint(0, n, (m,), generator=gen), h[:10]])
    kt = torch.cat([other, t[pick], torch.randint(0, n, (m,), generator=gen), t[:10]])
    kr = torch.cat([r[pick], r[pick], torch.randint(0, n_rel, (m,), generator=gen), r[:10]])
    return kh, kr, kt


def without(known, h, r, t):
    """known minus the evaluated triples"""
    ev = set(zip(h.tolist(), r.tolist(), t.tolist()))
    keep = torch.tensor([x not in ev for x in zip(*(k.tolist() for k in known))], dtype=torch.bool)
    return tuple(k[keep] for k in known)


def plus(known, h, r, t):
    return torch.cat([known[0], h]), torch.cat([known[1], r]), torch.cat([known[2], t])


def queries_of(h, r, t, side, n):
    """(q_ent, q_rel, query, ans) in numpy: the distinct queries ordered by (relation, entity) and every triple's query."""
    h, t = h.cpu().numpy(), t.cpu().numpy()
    ent, ans = (h, t) if side == "tail" else (t, h)
    rel = r.cpu().numpy() if r is not None else np.zeros_like(ent)
    uq, query = np.unique(rel * n + ent, return_inverse=True)
    return uq % n, (uq // n if r is not None else np.full_like(uq, -1)), query.reshape(-1), ans


def expected(h, r, t, side, n, dense, cand_ids, known, ks=KS):
    """The reference result: dense float32[Q, len(cand_ids)] holds the kernel scores of the distinct queries."""
    q_ent, q_rel, query, ans = queries_of(h, r, t, side, n)
    before, position = np.zeros_like(query), np.zeros_like(query)
    per_query, n_answers = [], []
    if known is not None:
        kh, kr, kt = (x.cpu().numpy() for x in known)
        mine, other = (kh, kt) if side == "tail" else (kt, kh)
    for u in range(q_ent.size):
        sel = np.flatnonzero(query == u)
        kn = ()
        if known is not None:
            kn = other[(mine == q_ent[u]) & ((kr == q_rel[u]) if r is not None else True)]
        pl = RC.places(dense[u], cand_ids, ans[sel], kn)
        for i in sel:
            before[i], position[i] = pl[int(ans[i])]
        per_query.append(RC.query_metrics([p for _, p in pl.values()], ks))
        n_answers.append(len(pl))
    return SimpleNamespace(q_ent=q_ent, q_rel=q_rel, query=query, ans=ans, before=before, position=position,
                           n_answers=np.array(n_answers), per_query=per_query, ks=ks)


def check(res, exp, what=""):
    """integers exactly; each per-query float within (terms + 8) * 2^-52 of the float64 reference (terms: its summands,
    each at most 1 and carrying a few roundings)"""
    for name in ("query", "before", "position", "q_ids", "q_rel", "n_answers", "a_query", "a_ids", "a_before", "a_position"):
        assert getattr(res, name).dtype == torch.int64, name
    assert res.query.cpu().tolist() == exp.query.tolist(), what
    assert res.q_ids.cpu().tolist() == exp.q_ent.tolist() and res.q_rel.cpu().tolist() == exp.q_rel.tolist(), what
    assert res.n_answers.cpu().tolist() == exp.n_answers.tolist(), what
    got_b, got_p = res.before.cpu().numpy(), res.position.cpu().numpy()
    bad = np.flatnonzero((got_b != exp.before) | (got_p != exp.position))
    assert bad.size == 0, (what, bad[:8], got_b[bad[:8]], exp.before[bad[:8]], got_p[bad[:8]], exp.position[bad[:8]])
    assert res.nan.dtype == torch.bool and res.nan.cpu().tolist() == (exp.position < 0).tolist(), what
    # the per-answer view: query u owns n_answers[u] consecutive entries, ascending by id
    aq, ai = res.a_query.cpu().numpy(), res.a_ids.cpu().numpy()
    assert aq.tolist() == np.repeat(np.arange(exp.q_ent.size), exp.n_answers).tolist(), what
    assert bool(np.all((np.diff(aq) > 0) | (np.diff(ai) > 0))), what
    if res.ks is None:
        return
    assert res.ks == exp.ks and res.hits.dtype == torch.int64 and res.ndcg.dtype == torch.float64
    hits, ndcg, ap, rr = (x.cpu().numpy() for x in (res.hits, res.ndcg, res.ap, res.rr))
    for u, q in enumerate(exp.per_query):
        assert hits[u].tolist() == q["hits"], (what, u)
        for j, k in enumerate(exp.ks):
            assert abs(ndcg[u, j] - q["ndcg"][j]) <= (min(k, q["m"]) + 8) * EPS, (what, u, k, ndcg[u, j], q["ndcg"][j])
        assert abs(ap[u] - q["ap"]) <= (q["m"] + 8) * EPS, (what, u, ap[u], q["ap"])
        assert abs(rr[u] - q["rr"]) <= 9 * EPS, (what, u)


def check_aggregates(out, exp, what=""):
    """the means get a further (Q + 2) * 2^-53 relative over the per-query bound"""
    ref = RC.aggregate(exp.per_query, exp.ks)
    n_q = len(exp.per_query)
    assert out["n_queries"] == ref["n_queries"] and out["n_answers"] == ref["n_answers"], what
    _, first = np.unique(np.stack([exp.query, exp.ans]), axis=1, return_index=True)          # the distinct answers
    assert out["nan"] == int((exp.position[first] < 0).sum()), what
    terms = max(max(q["m"] for q in exp.per_query), 1)
    for name, want in ref.items():
        if name in ("n_queries", "n_answers"):
            continue
        exact = name.split("@")[0] in ("precision", "recall", "hit")
        tol = (0.0 if exact else (terms + 8) * EPS) + (n_q + 2) * 2.0 ** -53 * abs(want)
        assert abs(out[name] - want) <= tol, (what, name, out[name], want)
    ranks = 1.0 + exp.before[first][exp.position[first] > 0]
    pa = out["per_answer"]
    assert pa["n"] == ranks.size
    if ranks.size:
        assert pa["mr"] == pytest.approx(float(ranks.mean()), rel=1e-12)
        assert pa["mrr"] == pytest.approx(float((1.0 / ranks).mean()), rel=1e-12)
        for k in exp.ks:
            assert pa[f"hits@{k}"] == pytest.approx(float((ranks <= k).mean()), rel=1e-12)


def same_ranks(a, b):
    for name in ("query", "before", "position", "nan", "q_ids", "q_rel", "n_answers", "a_query", "a_ids", "a_before",
                 "a_position", "hits", "ndcg", "ap", "rr"):
        x, y = getattr(a, name), getattr(b, name)
        if (x is None) != (y is None) or (x is not None and not torch.equal(x, y)):
            return False
    return True


def dense_scores(L, model, q_ent, q_rel, side, scoring, cand=None):
    """float32[Q, N]: score_triples(kernel_scores=True) over all Q x N explicit triples."""
    dev = model.T.device if hasattr(model, "T") else model.entity_embed.weight.device
    ids = torch.from_numpy(np.asarray(q_ent)).to(dev)
    rel = torch.from_numpy(np.maximum(np.asarray(q_rel), 0)).to(dev)
    c = torch.arange(model.n_entities, device=dev) if cand is None else cand
    b, n = ids.numel(), c.numel()
    q, cc, rr = ids.repeat_interleave(n), c.repeat(b), rel.repeat_interleave(n)
    h, t = (q, cc) if side == "tail" else (cc, q)
    k = L.score_triples(model, h, rr, t, scoring=scoring, side=side, kernel_scores=True)
    return k.view(b, n).cpu().numpy()


def sizes_for(L):
    tee = L.ops.RETRIEVAL_SLICE
    return (1, tee, tee + 1, 3 * tee + 2, 10 ** 9)                      # the last: every candidate is an answer


# ----------------------------------------------------------------------------- 1. exact integer tables
@pytest.mark.parametrize("scoring", ["transe", "dot"])
@pytest.mark.parametrize("side", ["tail", "head"])
@pytest.mark.parametrize("b,n,kd", [(70, 700, 5), (1, 257, 30), (70, 257, 64), (3, 1, 300)])
def test_exact_integer_tables(L, R, gpu_device, scoring, side, b, n, kd):
    """Small integers: every f32 product, sum and the final fma are exact, so the keys equal an int64 computation; ties
    are plentiful.  b random triples next to queries with 1, T, T + 1, 3 T + 2 and N answers."""
    gen = torch.Generator().manual_seed(17 + len(scoring) + len(side) + n + kd)
    n_rel = 3
    table = torch.randint(-2, 3, (n, kd), generator=gen)
    relemb = torch.randint(-1, 2, (n_rel, kd), generator=gen)
    h, r, t = draw_triples(gen, n, n_rel, b, sizes_for(L), side)
    q_ent, q_rel, _, _ = queries_of(h, r, t, side, n)
    q = table[torch.from_numpy(q_ent)] + (0 if scoring == "dot" else (1 if side == "tail" else -1)) * \
        relemb[torch.from_numpy(q_rel)]
    dots = q @ table.T                                                  # int64 throughout
    keys = (-2 * dots if scoring == "dot" else (table * table).sum(1)[None, :] - 2 * dots).numpy().astype(np.float32)
    known = draw_known(gen, n, n_rel, h, r, t, 2 * b + 3)
    exp = expected(h, r, t, side, n, keys, np.arange(n), known)
    model = StandIn(table.float().to(gpu_device), relemb.float().to(gpu_device), None, scoring)
    kt_ = R.KnownTriples(*(x.to(gpu_device) for x in known), n, n_rel)
    dev = lambda *xs: tuple(x.to(gpu_device) for x in xs)               # noqa: E731
    res = L.rank_answers(model, *dev(h, r, t), side=side, known=kt_, scoring=scoring, ks=KS)
    check(res, exp, f"{scoring} {side}")
    assert res.side == side and int(res.n_answers.max()) == n
    if n > 1:
        assert len(set(res.position.cpu().tolist())) > 10               # (the answers are spread over the list)
    # against rank_triples with the evaluated triples known: ties make it an interval
    rk = R.rank_triples(model, *dev(h, r, t), side=side, scoring=scoring,
                        known=R.KnownTriples(*dev(*plus(known, h, r, t)), n, n_rel))
    assert bool((rk.better <= res.before).all()) and bool((res.before <= rk.better + rk.equal).all())
    assert n == 1 or int(rk.equal.sum()) > 0


@pytest.mark.parametrize("scoring,side", [("transe", "tail"), ("dot", "head")])
def test_one_answer_per_query(L, R, gpu_device, scoring, side):
    """Every row holds one key: the kernel's reduction for workgroups without a bucket search (130 rows: three of them)."""
    gen = torch.Generator().manual_seed(23 + len(scoring))
    n, kd, n_rel, b = 700, 30, 3, 130
    table = torch.randint(-2, 3, (n, kd), generator=gen)
    relemb = torch.randint(-1, 2, (n_rel, kd), generator=gen)
    ent, rel = torch.randperm(n, generator=gen)[:b], torch.randint(0, n_rel, (b,), generator=gen)
    ans = torch.randint(0, n, (b,), generator=gen)
    h, r, t = (ent, rel, ans) if side == "tail" else (ans, rel, ent)
    q_ent, q_rel, _, _ = queries_of(h, r, t, side, n)
    q = table[torch.from_numpy(q_ent)] + (0 if scoring == "dot" else (1 if side == "tail" else -1)) * \
        relemb[torch.from_numpy(q_rel)]
    dots = q @ table.T
    keys = (-2 * dots if scoring == "dot" else (table * table).sum(1)[None, :] - 2 * dots).numpy().astype(np.float32)
    known = draw_known(gen, n, n_rel, h, r, t, 2 * b)
    exp = expected(h, r, t, side, n, keys, np.arange(n), known)
    model = StandIn(table.float().to(gpu_device), relemb.float().to(gpu_device), None, scoring)
    kt_ = R.KnownTriples(*(x.to(gpu_device) for x in known), n, n_rel)
    res = L.rank_answers(model, *(x.to(gpu_device) for x in (h, r, t)), side=side, known=kt_, scoring=scoring, ks=KS)
    check(res, exp, f"{scoring} {side}")
    assert int(res.n_answers.max()) == 1 and res.q_ids.numel() == b and int(res.position.max()) > 100


# ----------------------------------------------------------------------------- 2 - 4, 6, 7, 10: one scored case each
WIDTHS = {"transr": (37, 32), "transe": (300, 300), "dot": (64, 64)}


@functools.lru_cache(maxsize=None)
def scored_case(L, R, dev, scoring, side):
    """One random-float case, scored densely once and shared by the tests below (nothing in it is changed afterwards):
    70 random triples and the structured queries over N = 700."""
    b, n, n_rel = 70, 700, 4
    kd, c = WIDTHS[scoring]
    gen = torch.Generator().manual_seed(1200 + 7 * len(scoring) + len(side))
    model = random_model(gen, scoring, n, kd, c, n_rel, dev)
    h, r, t = draw_triples(gen, n, n_rel, b, sizes_for(L), side)
    q_ent, q_rel, _, _ = queries_of(h, r, t, side, n)
    dense = dense_scores(L, model, q_ent, q_rel, side, scoring)
    known = draw_known(gen, n, n_rel, h, r, t, 3 * b)
    best = torch.from_numpy(np.argsort(dense, axis=1)[:, :3].copy())     # known among the best of every query
    q3 = torch.from_numpy(q_ent)[:, None].expand(-1, 3).reshape(-1)
    r3 = torch.from_numpy(q_rel)[:, None].expand(-1, 3).reshape(-1)
    known = plus(known, *((q3, r3, best.reshape(-1)) if side == "tail" else (best.reshape(-1), r3, q3)))
    k_without, k_with = without(known, h, r, t), plus(known, h, r, t)
    to = lambda xs: tuple(x.to(dev) for x in xs)                        # noqa: E731
    kt_without, kt_with = R.KnownTriples(*to(k_without), n, n_rel), R.KnownTriples(*to(k_with), n, n_rel)
    h, r, t = to((h, r, t))
    exp = expected(h, r, t, side, n, dense, np.arange(n), k_without)
    res = L.rank_answers(model, h, r, t, side=side, known=kt_without, scoring=scoring, ks=KS)
    return SimpleNamespace(model=model, h=h, r=r, t=t, n=n, n_rel=n_rel, dense=dense, known=k_without, exp=exp, res=res,
                           kt_without=kt_without, kt_with=kt_with)


CASES = [(s, side) for s in ("transr", "transe", "dot") for side in ("tail", "head")]


@pytest.mark.parametrize("scoring,side", CASES)
def test_equals_score_triples_over_all_pairs(L, R, gpu_device, scoring, side):
    c = scored_case(L, R, gpu_device, scoring, side)
    check(c.res, c.exp, f"{scoring} {side}")
    # known with the evaluated triples in it: the answers are exempt, nothing changes
    held = L.rank_answers(c.model, c.h, c.r, c.t, side=side, known=c.kt_with, scoring=scoring, ks=KS)
    assert same_ranks(held, c.res)
    # without a filter
    free = L.rank_answers(c.model, c.h, c.r, c.t, side=side, scoring=scoring, ks=KS)
    check(free, expected(c.h, c.r, c.t, side, c.n, c.dense, np.arange(c.n), None), f"{scoring} {side} unfiltered")
    assert not torch.equal(free.before, c.res.before)                    # (the filter matters in this case)
    plain = L.rank_answers(c.model, c.h, c.r, c.t, side=side, known=c.kt_without, scoring=scoring)
    assert plain.ks is None and plain.hits is None and torch.equal(plain.position, c.res.position)


@pytest.mark.parametrize("scoring,side", CASES)
def test_agrees_with_predict_topk(L, R, gpu_device, scoring, side):
    """known is disjoint from the evaluated triples here, so predict_topk lists the answers too: an answer is at position
    p <= 128 iff the p-th entry of its query's top-k is that answer, and no other answer appears."""
    c = scored_case(L, R, gpu_device, scoring, side)
    top = L.predict_topk(c.model, c.res.q_ids, c.res.q_rel, side=side, k=128, known=c.kt_without, scoring=scoring)
    ids = top.ids.cpu().numpy()
    aq, ai, ap = (x.cpu().numpy() for x in (c.res.a_query, c.res.a_ids, c.res.a_position))
    seen = 0
    for u in range(ids.shape[0]):
        mine = aq == u
        shallow = mine & (ap > 0) & (ap <= 128)
        assert ids[u, ap[shallow] - 1].tolist() == ai[shallow].tolist(), u
        assert set(ids[u].tolist()) & set(ai[mine].tolist()) == set(ai[shallow].tolist()), u
        seen += int(shallow.sum())
    assert seen > 0 and int((ap > 128).sum()) > 0


@pytest.mark.parametrize("scoring,side", CASES)
def test_agrees_with_rank_triples(L, R, gpu_device, scoring, side):
    c = scored_case(L, R, gpu_device, scoring, side)
    rk = R.rank_triples(c.model, c.h, c.r, c.t, side=side, known=c.kt_with, scoring=scoring)
    assert int(rk.equal.sum()) == 0                                      # (a seed with a tie would weaken the check)
    assert torch.equal(c.res.before, rk.better)


@pytest.mark.parametrize("scoring", ["transr", "dot"])
def test_metrics_and_aggregates(L, R, gpu_device, scoring):
    c = scored_case(L, R, gpu_device, scoring, "tail")
    out = L.evaluate_retrieval(c.model, c.h, c.r, c.t, known=c.kt_without, ks=KS, scoring=scoring)
    check_aggregates(out, c.exp, scoring)
    assert "tail" not in out and 0.0 < out["map"] < 1.0 and 0.0 < out["recall@100"] < 1.0
    both = L.evaluate_retrieval(c.model, c.h, c.r, c.t, known=c.kt_without, ks=KS, scoring=scoring, side="both")
    assert both["tail"] == out
    head = L.evaluate_retrieval(c.model, c.h, c.r, c.t, known=c.kt_without, ks=KS, scoring=scoring, side="head")
    assert both["head"] == head and both["n_queries"] == out["n_queries"] + head["n_queries"]
    w = out["n_queries"] / both["n_queries"]
    assert both["map"] == pytest.approx(w * out["map"] + (1 - w) * head["map"], rel=1e-12)
    assert both["per_answer"]["n"] == out["per_answer"]["n"] + head["per_answer"]["n"]


# ----------------------------------------------------------------------------- 5. a hub on the head side
def test_head_side_hub(L, R, gpu_device):
    """one (?, r, t) with 1000 heads among 1500 entities -- 32 rows of one query vector -- next to ordinary queries"""
    gen = torch.Generator().manual_seed(77)
    n, kd, n_rel = 1500, 30, 3
    model = random_model(gen, "transe", n, kd, kd, n_rel, gpu_device)
    h, r, t = draw_triples(gen, n, n_rel, 40, (1000, 5), "head")
    known = draw_known(gen, n, n_rel, h, r, t, 200)
    q_ent, q_rel, _, _ = queries_of(h, r, t, "head", n)
    dense = dense_scores(L, model, q_ent, q_rel, "head", "transe")
    exp = expected(h, r, t, "head", n, dense, np.arange(n), known, ks=(10, 1000, 5000))
    to = lambda xs: tuple(x.to(gpu_device) for x in xs)                 # noqa: E731
    res = L.rank_answers(model, *to((h, r, t)), side="head", known=R.KnownTriples(*to(known), n, n_rel),
                         scoring="transe", ks=(10, 1000, 5000))
    check(res, exp, "hub")
    assert int(res.n_answers.max()) == 1000 and int(res.position.max()) > 1400


# ----------------------------------------------------------------------------- 6. invariance
@pytest.mark.parametrize("scoring", ["transr", "dot"])
def test_invariance(L, R, gpu_device, scoring):
    c = scored_case(L, R, gpu_device, scoring, "tail")
    kw = dict(side="tail", known=c.kt_without, scoring=scoring, ks=KS)
    for bs in (1, 7, None):
        assert same_ranks(L.rank_answers(c.model, c.h, c.r, c.t, batch_size=bs, **kw), c.res), bs
    gen = torch.Generator().manual_seed(5)
    perm = torch.randperm(c.h.numel(), generator=gen).to(gpu_device)
    got = L.rank_answers(c.model, c.h[perm], c.r[perm], c.t[perm], **kw)
    for name in ("query", "before", "position", "nan"):
        assert torch.equal(getattr(got, name), getattr(c.res, name)[perm]), name
    for name in ("q_ids", "q_rel", "n_answers", "a_query", "a_ids", "a_before", "a_position", "hits", "ndcg", "ap", "rr"):
        assert torch.equal(getattr(got, name), getattr(c.res, name)), name
    twice = L.rank_answers(c.model, torch.cat([c.h, c.h[:9]]), torch.cat([c.r, c.r[:9]]), torch.cat([c.t, c.t[:9]]), **kw)
    m = c.h.numel()
    assert torch.equal(twice.position[:m], c.res.position) and torch.equal(twice.position[m:], c.res.position[:9])
    assert torch.equal(twice.before[m:], c.res.before[:9]) and torch.equal(twice.query[m:], c.res.query[:9])
    for name in ("n_answers", "a_ids", "a_position", "hits", "ndcg", "ap", "rr"):
        assert torch.equal(getattr(twice, name), getattr(c.res, name)), name
    everyone = L.rank_answers(c.model, c.h, c.r, c.t, candidates=torch.arange(c.n, device=gpu_device), **kw)
    shuffled = L.rank_answers(c.model, c.h, c.r, c.t, candidates=torch.randperm(c.n, generator=gen).to(gpu_device), **kw)
    assert same_ranks(everyone, c.res) and same_ranks(shuffled, c.res)
    ev = dict(known=c.kt_without, scoring=scoring, ks=KS)
    base = L.evaluate_retrieval(c.model, c.h, c.r, c.t, **ev)
    assert L.evaluate_retrieval(c.model, c.h[perm], c.r[perm], c.t[perm], batch_size=7, **ev) == base
    assert L.evaluate_retrieval(c.model, torch.cat([c.h, c.h[:9]]), torch.cat([c.r, c.r[:9]]), torch.cat([c.t, c.t[:9]]),
                                candidates=torch.randperm(c.n, generator=gen).to(gpu_device), **ev) == base


# ----------------------------------------------------------------------------- 7. a subset of the candidates
@pytest.mark.parametrize("scoring", ["transr", "transe", "dot"])
def test_candidate_subset(L, R, gpu_device, scoring):
    c = scored_case(L, R, gpu_device, scoring, "head")
    gen = torch.Generator().manual_seed(21)
    few = c.exp.n_answers < 100                                          # (leave the all-candidates query out)
    keep = torch.from_numpy(few[c.exp.query]).to(gpu_device)
    h, r, t = c.h[keep], c.r[keep], c.t[keep]
    extra = torch.randperm(c.n, generator=gen)[:200].to(gpu_device)
    cand = torch.unique(torch.cat([h, extra]))
    cand = cand[torch.randperm(cand.numel(), generator=gen).to(gpu_device)]                # unsorted entity ids
    res = L.rank_answers(c.model, h, r, t, side="head", known=c.kt_without, scoring=scoring, candidates=cand, ks=KS)
    cols = cand.cpu().numpy()
    exp = expected(h, r, t, "head", c.n, c.dense[few][:, cols], cols, c.known)
    check(res, exp, f"candidates {scoring}")
    assert 0 < cand.numel() < c.n and int(res.position.max()) <= cand.numel()
    missing = cand[cand != h[0]]
    with pytest.raises(ValueError, match="must contain every answer"):
        L.rank_answers(c.model, h, r, t, side="head", known=c.kt_without, scoring=scoring, candidates=missing)


# ----------------------------------------------------------------------------- 8. any relation
def test_any_relation(L, R, gpu_device):
    gen = torch.Generator().manual_seed(9)
    n, kd, n_rel = 700, 64, 3
    model = random_model(gen, "dot", n, kd, kd, n_rel, gpu_device)
    h, r, t = draw_triples(gen, n, n_rel, 70, (1, 40), "tail")
    q_ent, q_rel, _, _ = queries_of(h, None, t, "tail", n)
    dense = dense_scores(L, model, q_ent, np.zeros_like(q_ent), "tail", "dot")
    best = torch.from_numpy(np.argsort(dense, axis=1)[:, :4].copy())
    kh = torch.from_numpy(q_ent)[:, None].expand(-1, 4).reshape(-1)
    kr = (torch.arange(q_ent.size)[:, None] + torch.arange(4)[None, :]).reshape(-1) % n_rel      # under several relations
    known = plus((kh, kr, best.reshape(-1)), h[:10], r[:10], t[:10])
    to = lambda xs: tuple(x.to(gpu_device) for x in xs)                 # noqa: E731
    kt_ = R.KnownTriples(*to(known), n, n_rel)
    hd, rd, td = to((h, r, t))
    res = L.rank_answers(model, hd, None, td, known=kt_, scoring="dot", ks=KS)
    check(res, expected(h, None, t, "tail", n, dense, np.arange(n), known), "any relation")
    assert bool((res.q_rel == -1).all())
    # with r only (query, r, c) drops, and the queries split by relation
    qe, qr, _, _ = queries_of(h, r, t, "tail", n)
    res_r = L.rank_answers(model, hd, rd, td, known=kt_, scoring="dot", ks=KS)
    check(res_r, expected(h, r, t, "tail", n, dense_scores(L, model, qe, qr, "tail", "dot"), np.arange(n), known), "dot r")
    assert res_r.q_ids.numel() > res.q_ids.numel()
    out = L.evaluate_retrieval(model, hd, None, td, known=kt_, scoring="dot", ks=KS)
    check_aggregates(out, expected(h, None, t, "tail", n, dense, np.arange(n), known), "any relation")
    # a filter that knows one triple elsewhere: every query of another head walks an empty row
    lone = (torch.tensor([n - 1]), torch.tensor([0]), torch.tensor([n - 1]))
    assert int((h != n - 1).sum()) > 0
    res_l = L.rank_answers(model, hd, None, td, known=R.KnownTriples(*to(lone), n, n_rel), scoring="dot", ks=KS)
    check(res_l, expected(h, None, t, "tail", n, dense, np.arange(n), lone), "a filter elsewhere")


# ----------------------------------------------------------------------------- 9. NaN
@pytest.mark.parametrize("scoring", ["transe", "dot"])
def test_nan_rows(L, R, gpu_device, scoring):
    gen = torch.Generator().manual_seed(41 + len(scoring))
    n, kd, n_rel = 700, 30, 3
    model = random_model(gen, scoring, n, kd, kd, n_rel, gpu_device)
    model.T[7] = float("nan")                                           # an answer of some queries, a non-answer of the rest
    model.T[300] = float("nan")                                         # never an answer
    h, r, t = draw_triples(gen, n, n_rel, 40, (40,), "tail")
    bad = (h == 7) | (h == 300) | (t == 300) | (h == 650)
    h, r, t = h[~bad], r[~bad], t[~bad]
    h = torch.cat([h, h[:6], torch.tensor([650])])                      # six queries with the NaN answer among theirs ...
    r = torch.cat([r, r[:6], torch.tensor([1])])
    t = torch.cat([t, torch.full((6,), 7), torch.tensor([7])])          # ... and one whose only answer is NaN
    known = draw_known(gen, n, n_rel, h, r, t, 100)
    q_ent, q_rel, _, _ = queries_of(h, r, t, "tail", n)
    dense = dense_scores(L, model, q_ent, q_rel, "tail", scoring)
    assert np.isnan(dense[:, 7]).all() and int(np.isnan(dense).sum()) == 2 * q_ent.size
    exp = expected(h, r, t, "tail", n, dense, np.arange(n), known)
    to = lambda xs: tuple(x.to(gpu_device) for x in xs)                 # noqa: E731
    kt_ = R.KnownTriples(*to(known), n, n_rel)
    res = L.rank_answers(model, *to((h, r, t)), known=kt_, scoring=scoring, ks=KS)
    check(res, exp, f"nan {scoring}")
    assert int(res.nan.sum()) >= 7 and bool((res.before[res.nan] == -1).all())
    assert int(res.position.max()) <= n - 2                              # the NaN candidates are in no list
    out = L.evaluate_retrieval(model, *to((h, r, t)), known=kt_, scoring=scoring, ks=KS)
    check_aggregates(out, exp, f"nan {scoring}")
    assert out["nan"] >= 2


# ----------------------------------------------------------------------------- 11. golden models
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
    nv = min(300, h.numel() // 2)
    vh, vr, vt = h[:nv], r[:nv], t[:nv]
    known = (h[nv:], r[nv:], t[nv:])
    kt_ = R.KnownTriples(*known, n, model.n_relations)
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for side in ("tail", "head"):
        q_ent, q_rel, _, _ = queries_of(vh, vr, vt, side, n)
        dense = dense_scores(L, model, q_ent, q_rel, side, scoring)
        exp = expected(vh, vr, vt, side, n, dense, np.arange(n), known)
        res = model.rank_answers(vh, vr, vt, side=side, known=kt_, ks=KS)
        check(res, exp, f"{name} {side}")
        assert not model.training
        check_aggregates(model.evaluate_retrieval(vh, vr, vt, known=kt_, ks=KS, side=side), exp, f"{name} {side}")
    for k_, v in model.state_dict().items():
        v0 = params[k_]
        if v.is_sparse:
            v, v0 = v.coalesce().values(), v0.coalesce().values()
        assert torch.equal(v, v0), k_
    model.train()
    model.evaluate_retrieval(vh[:5], vr[:5], vt[:5])
    assert model.training
