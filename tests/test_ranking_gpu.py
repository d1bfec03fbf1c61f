"""GPU: filtered link-prediction ranking (literalkg_amd/ranking.py, lkg_rank.hip) against a float64 oracle restated here.

The oracle computes every distance in float64 from the f32 inputs (dense for small N, in candidate chunks for the big case)
and a per-pair margin that bounds the device's rounding ("Filtered ranking"):
    E(q, x) = (k + 2) u (|p_x| + |q|)^2  +  2 sqrt(d(q, x)) (dq + dp_x)  +  (dq + dp_x)^2,      u = 2^-24,
with dp_x = 2 (C + 4) u | |T_x| |W_r| | the error of the tall GEMM's projection (TransR only; 0 otherwise) and
dq = dp_query + u |q| that of the query (projected row plus relation vector).  A candidate c is clear of the truth t when
|d(q, c) - d(q, t)| > E(q, c) + E(q, t).  Where every kept candidate is clear, better / equal equal the oracle's counts;
elsewhere the rank may differ by at most the number of candidates that are not clear.
LKG_RANK_FUZZ_CASES (default 24) / LKG_RANK_FUZZ_SEED (default 5000) set the drawn configurations of the last test."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import golden_cfg, golden_params, load_golden

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
N_FUZZ = int(os.environ.get("LKG_RANK_FUZZ_CASES", "24"))
FUZZ_SEED0 = int(os.environ.get("LKG_RANK_FUZZ_SEED", "5000"))


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
    """What rank_triples reads of a LiteralKG, over a given table (random-table tests)."""

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
        return self

    def train(self, mode=True):
        self.training = mode
        return self


# ----------------------------------------------------------------------------- float64 oracle
def oracle(table, relemb, trans_m, scoring, side, h, r, t, known=None, chunk=1 << 18):
    """(better, equal, sure_better, unclear) int64[B] in input order; known = (kh, kr, kt) device tensors or None."""
    dev = table.device
    n, c_dim = table.shape
    n_rel = relemb.shape[0]
    b = h.numel()
    out = [torch.zeros(b, dtype=torch.int64, device=dev) for _ in range(4)]
    if known is not None:
        kh, kr, kt = (x.long() for x in known)
        kkeys = torch.unique((kh * n_rel + kr) * n + kt)
    e64 = relemb.double()
    for rr in torch.unique(r).tolist():
        idx = torch.nonzero(r == rr, as_tuple=True)[0]
        qid, truth = (h[idx], t[idx]) if side == "tail" else (t[idx], h[idx])
        if scoring == "transr":
            w = trans_m[rr].double()
            eps_p = 2.0 * (c_dim + 4) * U

            def rows(lo, hi):
                x = table[lo:hi].double()
                return x @ w, eps_p * (x.abs() @ w.abs()).norm(dim=1)

            def rows_at(ids):
                x = table[ids].double()
                return x @ w, eps_p * (x.abs() @ w.abs()).norm(dim=1)
        else:
            def rows(lo, hi):
                x = table[lo:hi].double()
                return x, torch.zeros(hi - lo, dtype=torch.float64, device=dev)

            def rows_at(ids):
                x = table[ids].double()
                return x, torch.zeros(ids.numel(), dtype=torch.float64, device=dev)
        pq, dpq = rows_at(qid)
        if scoring == "dot":
            q, dq = pq, dpq
        else:
            q = pq + (1.0 if side == "tail" else -1.0) * e64[rr]
            dq = dpq + U * q.norm(dim=1)
        k = q.shape[1]
        qn = q.norm(dim=1)

        def dist(p):
            if scoring == "dot":
                return -2.0 * (q @ p.t())
            return (q * q).sum(1, keepdim=True) - 2.0 * (q @ p.t()) + (p * p).sum(1)[None, :]

        def err(p, dp, d):
            s = (p.norm(dim=1)[None, :] + qn[:, None]) ** 2
            dd = dq[:, None] + dp[None, :]
            return (k + 2) * U * s + 2.0 * d.clamp_min(0).sqrt() * dd + dd * dd

        pt, dpt = rows_at(truth)
        # the truth's distance and error, row by row (pt[i] against q[i])
        if scoring == "dot":
            d_t = -2.0 * (q * pt).sum(1)
        else:
            d_t = ((q - pt) ** 2).sum(1)
        dd_t = dq + dpt
        e_t = (k + 2) * U * (pt.norm(dim=1) + qn) ** 2 + 2.0 * d_t.clamp_min(0).sqrt() * dd_t + dd_t * dd_t
        if scoring != "dot":      # the same quantity through the expansion the candidates use (identical up to f64 noise)
            d_t = (q * q).sum(1) - 2.0 * (q * pt).sum(1) + (pt * pt).sum(1)
        acc = [torch.zeros(idx.numel(), dtype=torch.int64, device=dev) for _ in range(4)]
        for lo in range(0, n, chunk):
            hi = min(n, lo + chunk)
            p, dp = rows(lo, hi)
            d = dist(p)
            m = err(p, dp, d) + e_t[:, None]
            diff = d - d_t[:, None]
            # equal rows give equal f64 distances up to the f64 GEMM's own rounding: call those exact ties
            diff = torch.where(diff.abs() <= 1e-12 * (p.norm(dim=1)[None, :] + qn[:, None]) ** 2, torch.zeros_like(diff), diff)
            cand = torch.arange(lo, hi, device=dev)
            kept = (cand[None, :] != truth[:, None]) & ~torch.isnan(diff)
            if known is not None:
                if side == "tail":
                    keys = ((qid * n_rel + rr) * n)[:, None] + cand[None, :]
                else:
                    keys = (cand * (n_rel * n))[None, :] + (rr * n + qid)[:, None]
                kept &= ~torch.isin(keys, kkeys)
            acc[0] += ((diff < 0) & kept).sum(1)
            acc[1] += ((diff == 0) & kept).sum(1)
            acc[2] += ((diff < -m) & kept).sum(1)
            acc[3] += ((diff.abs() <= m) & kept).sum(1)
        for o, a in zip(out, acc):
            o[idx] = a
    return out


def check(got_better, got_equal, ora, min_clear=0.0, what="", min_exact=0.75):
    """The rigorous part: exact counts where every kept candidate is clear, the rank within the unclear ones elsewhere;
    min_clear: the share of queries that have to be clear.  The margin is a worst case (linear in k, the rounding of the
    projection included); the device's actual error is far smaller, so at least min_exact of the queries -- clear or
    not -- must also reproduce the oracle's counts exactly."""
    b_o, e_o, sure, unclear = (x.cpu() for x in ora)
    gb, ge = got_better.cpu(), got_equal.cpu()
    clear = unclear == 0
    assert torch.equal(gb[clear], b_o[clear]), (what, torch.nonzero(gb[clear] != b_o[clear])[:5])
    assert torch.equal(ge[clear], e_o[clear]), what
    assert bool((gb >= sure).all()) and bool((gb + ge <= sure + unclear).all()), what
    r_got = 1.0 + gb.double() + 0.5 * ge.double()
    r_o = 1.0 + b_o.double() + 0.5 * e_o.double()
    assert bool(((r_got - r_o).abs() <= unclear.double()).all()), what
    assert clear.double().mean() >= min_clear, (what, float(clear.double().mean()))
    exact = (gb == b_o) & (ge == e_o)
    assert exact.double().mean() >= min_exact, (what, float(exact.double().mean()))


# ----------------------------------------------------------------------------- inputs
def draw_queries(gen, n, n_rel, max_per_rel=300, dev="cuda"):
    """1..7 relations (at most n_rel) with 1..max_per_rel queries each, uneven; truths at ids 0 and n-1; duplicates."""
    rels = torch.randperm(n_rel, generator=gen)[:int(torch.randint(1, min(7, n_rel) + 1, (1,), generator=gen))]
    hs, rs, ts = [], [], []
    for rr in rels.tolist():
        m = int(torch.randint(1, max_per_rel + 1, (1,), generator=gen))
        hs.append(torch.randint(0, n, (m,), generator=gen))
        ts.append(torch.randint(0, n, (m,), generator=gen))
        rs.append(torch.full((m,), rr, dtype=torch.int64))
    h, r, t = torch.cat(hs), torch.cat(rs), torch.cat(ts)
    perm = torch.randperm(h.numel(), generator=gen)         # relations interleaved in input order
    h, r, t = h[perm], r[perm], t[perm]
    t[0], h[-1] = 0, n - 1
    if h.numel() > 3:
        t[1] = n - 1
        h[2], r[2], t[2] = h[0], r[0], t[0]                  # a duplicate test triple
    return h.to(dev), r.to(dev), t.to(dev)


def draw_known(gen, n, n_rel, h, r, t, extra):
    """the test triples themselves (the filter holds every truth) + neighbours sharing (h, r) or (r, t) + random ones"""
    b = h.numel()
    m = max(extra, 1)
    pick = torch.randint(0, b, (m,), generator=gen).to(h.device)
    nh = torch.randint(0, n, (m,), generator=gen).to(h.device)
    nt = torch.randint(0, n, (m,), generator=gen).to(h.device)
    rh = torch.randint(0, n, (m,), generator=gen).to(h.device)
    rt = torch.randint(0, n, (m,), generator=gen).to(h.device)
    rr = torch.randint(0, n_rel, (m,), generator=gen).to(h.device)
    kh = torch.cat([h, h[pick], nh, rh, h[:5]])
    kr = torch.cat([r, r[pick], r[pick], rr, r[:5]])
    kt = torch.cat([t, nt, t[pick], rt, t[:5]])                # (h[:5] ...: duplicates inside the filter)
    return kh, kr, kt


def random_model(gen, scoring, n, k, c, n_rel, dev, scale=1.0):
    table = (torch.randn(n, c, generator=gen) * scale).to(dev)
    relemb = torch.randn(n_rel, k, generator=gen).to(dev) * 0.3
    trans_m = (torch.randn(n_rel, c, k, generator=gen) / math.sqrt(c)).to(dev) if scoring == "transr" else None
    return StandIn(table, relemb, trans_m, scoring)


def run_and_check(R, model, scoring, h, r, t, known=None, batch_size=None, min_clear=0.0, what=""):
    kt_ = R.KnownTriples(*known, model.n_entities, model.n_relations) if known is not None else None
    res = R.rank_triples(model, h, r, t, side="both", known=kt_, scoring=scoring, batch_size=batch_size)
    assert res.better.shape == (2, h.numel()) and res.better.dtype == torch.int64
    for j, side in enumerate(("tail", "head")):
        ora = oracle(model.T, model.relation_embed.weight, model.gat_trans_M, scoring, side, h, r, t, known)
        check(res.better[j], res.equal[j], ora, min_clear, f"{what} {side}")
    torch.testing.assert_close(res.rank, 1.0 + res.better.double() + 0.5 * res.equal.double())
    return res, kt_


# ----------------------------------------------------------------------------- 1. random-table parity
PARITY = [("transr", 257, 37, 32), ("transr", 5000, 300, 300), ("transr", 1, 1, 32), ("transr", 5000, 64, 32),
          ("transr", 257, 300, 32), ("transe", 257, 32, 32), ("transe", 5000, 300, 300), ("transe", 1, 32, 32),
          ("transe", 257, 37, 37), ("dot", 257, 300, 300), ("dot", 5000, 32, 32), ("dot", 1, 32, 32), ("dot", 257, 1, 1)]


@pytest.mark.parametrize("scoring,n,k,c", PARITY)
def test_random_table_parity(R, gpu_device, scoring, n, k, c):
    gen = torch.Generator().manual_seed(n * 1000 + k * 10 + c + len(scoring))
    n_rel = 9
    model = random_model(gen, scoring, n, k, c, n_rel, gpu_device)
    h, r, t = draw_queries(gen, n, n_rel)
    run_and_check(R, model, scoring, h, r, t, what=f"{scoring} raw")
    known = draw_known(gen, n, n_rel, h, r, t, extra=4 * h.numel())
    res, kt_ = run_and_check(R, model, scoring, h, r, t, known, what=f"{scoring} filtered")
    # one side alone, and in small launches, gives the same counts
    one = R.rank_triples(model, h, r, t, side="head", known=kt_, scoring=scoring, batch_size=7)
    assert torch.equal(one.better, res.better[1]) and torch.equal(one.equal, res.equal[1])


def test_tiny_filter_reaches_every_branch_of_the_row_walk(R, gpu_device):
    """5 entities, 6 known triples, the pair (0, 1) under both relations, entity 4 in none.  On either side the queries
    meet an empty filter row, a row with one entry under the wanted relation and one under the other only, and a row
    whose entry under the wanted relation is the truth itself."""
    model = random_model(torch.Generator().manual_seed(5), "transe", 5, 8, 8, 2, gpu_device)
    known = tuple(torch.tensor(x, device=gpu_device) for x in ([0, 0, 0, 2, 2, 3], [0, 1, 0, 1, 0, 1], [1, 1, 3, 3, 0, 2]))
    h, r, t = (torch.tensor(x, device=gpu_device) for x in ([4, 0, 2, 3, 0], [0, 1, 0, 0, 0], [0, 4, 0, 4, 3]))
    run_and_check(R, model, "transe", h, r, t, known, what="tiny")


# ----------------------------------------------------------------------------- 2. trained-like geometry
@pytest.mark.parametrize("scoring", ["transe", "transr"])
def test_trained_like_geometry(R, gpu_device, scoring):
    """Large rows around a common offset, the truth close to the query: pn - 2 q.p cancels most of its bits."""
    gen = torch.Generator().manual_seed(77 if scoring == "transe" else 78)
    n, k, n_rel = 4000, 64, 3
    c = k
    model = random_model(gen, scoring, n, k, c, n_rel, gpu_device)
    base = torch.randn(1, c, generator=gen) * (60.0 / math.sqrt(c))                  # |base| ~ 60
    table = base + torch.randn(n, c, generator=gen) * (3.0 / math.sqrt(c))          # rows 3 apart, norm ~ 60
    h, r, t = draw_queries(gen, n, n_rel, max_per_rel=100, dev="cpu")
    if scoring == "transe":
        rel = model.relation_embed.weight.cpu()
        table[t] = table[h] + rel[r] + torch.randn(h.numel(), c, generator=gen) * 0.05     # truth at distance ~0.05
    model.T = table.to(gpu_device)
    model.entity_embed.weight = model.T
    h, r, t = h.to(gpu_device), r.to(gpu_device), t.to(gpu_device)
    res = R.rank_triples(model, h, r, t, side="both", scoring=scoring)
    for j, side in enumerate(("tail", "head")):
        ora = oracle(model.T, model.relation_embed.weight, model.gat_trans_M, scoring, side, h, r, t)
        check(res.better[j], res.equal[j], ora, 0.5 if scoring == "transe" else 0.0, f"{scoring} {side}")
    if scoring == "transe":
        assert float((res.rank[0] <= 3).double().mean()) > 0.5        # the planted truths do rank near the top


# ----------------------------------------------------------------------------- 3. exact ties
@pytest.mark.parametrize("scoring", ["transr", "transe", "dot"])
def test_bit_identical_rows_tie_exactly(R, gpu_device, scoring):
    """Candidates whose rows are bit copies of the truth's count in `equal` -- the truth's score and the candidates' come
    from the same arithmetic -- and leave it when the filter drops them."""
    gen = torch.Generator().manual_seed(31 + len(scoring))
    n, k, c, n_rel = 3000, 300, 300, 4
    model = random_model(gen, scoring, n, k, c, n_rel, gpu_device)
    b = 40
    h = torch.randperm(n // 2, generator=gen)[:b]          # distinct heads
    t = torch.arange(n // 2, n // 2 + b)                  # distinct truths
    r = torch.randint(0, n_rel, (b,), generator=gen)
    copies = torch.arange(n - 3 * b, n).view(b, 3)       # three copies of each truth's row (tail side) ...
    hcopies = torch.arange(n - 6 * b, n - 3 * b).view(b, 3)      # ... and of each head's row (head side)
    table = model.T.clone()
    table[copies.reshape(-1).to(gpu_device)] = table[t.repeat_interleave(3).to(gpu_device)]
    table[hcopies.reshape(-1).to(gpu_device)] = table[h.repeat_interleave(3).to(gpu_device)]
    model.T = table
    model.entity_embed.weight = table
    h, r, t = h.to(gpu_device), r.to(gpu_device), t.to(gpu_device)
    res = R.rank_triples(model, h, r, t, side="both", scoring=scoring)
    assert bool((res.equal[0] >= 3).all()), res.equal[0]
    assert bool((res.equal[1] >= 3).all()), res.equal[1]
    for j, side in enumerate(("tail", "head")):
        ora = oracle(model.T, model.relation_embed.weight, model.gat_trans_M, scoring, side, h, r, t)
        assert torch.equal(res.equal[j].cpu(), ora[1].cpu()), side     # exactly the copies (f64 ties)
        check(res.better[j], res.equal[j], ora, 0.0, side)
    # filtered: (h, r, copy) and (hcopy, r, t) are known -> the copies are dropped
    cp, hc = copies.to(gpu_device), hcopies.to(gpu_device)
    kh = torch.cat([h.repeat_interleave(3), hc.reshape(-1)])
    kr = torch.cat([r.repeat_interleave(3), r.repeat_interleave(3)])
    kt = torch.cat([cp.reshape(-1), t.repeat_interleave(3)])
    known = R.KnownTriples(kh, kr, kt, n, n_rel)
    res_f = R.rank_triples(model, h, r, t, side="both", known=known, scoring=scoring)
    assert torch.equal(res_f.equal, res.equal - 3)
    assert torch.equal(res_f.better, res.better)


# ----------------------------------------------------------------------------- 4. model level
def _golden_model(L, name, dev, scoring):
    gd = load_golden(name)
    cfg = golden_cfg(gd)
    n, n_rel = int(gd["n"]), int(gd["n_rel"])
    a_in = torch.sparse_coo_tensor(torch.from_numpy(gd["a_indices"]), torch.from_numpy(gd["a_values"]), (n, n)).coalesce()
    num = torch.from_numpy(gd["num"]) if "num" in gd else None
    txt = torch.from_numpy(gd["txt"]) if "txt" in gd else None
    m = L.LiteralKG(cfg, n, n_rel, a_in, num, txt, scoring=scoring)
    params = golden_params(gd)
    own = set(m.state_dict().keys())
    m.load_state_dict({k: v for k, v in params.items() if k in own}, strict=False)
    return m.to(dev), gd


@pytest.mark.parametrize("name,form,scoring", [("encoder_gcn_l2_gatenum", "transr", "transr"),
                                               ("encoder_gcn_l2_scale", "transr", "transr"),
                                               ("transe_gcn_l1", "transe", "transe"),
                                               ("encoder_gcn_l2_gatenum", "transr", "dot")])
def test_model_level_against_oracle(L, R, gpu_device, name, form, scoring):
    model, gd = _golden_model(L, name, gpu_device, form)
    model.eval()
    h, r, t = (torch.from_numpy(gd[k]).to(gpu_device) for k in ("h", "r", "t"))
    known = R.KnownTriples(h, r, t, model.n_entities, model.n_relations)
    th, tr_, tt = h[:300], r[:300], t[:300]
    res = model.rank_triples(th, tr_, tt, side="both", known=known, scoring=scoring)
    with torch.no_grad():
        table = model.gat_embeddings()
    tm = model.gat_trans_M.detach() if scoring == "transr" else None
    got_ranks = []
    for j, side in enumerate(("tail", "head")):
        ora = oracle(table, model.relation_embed.weight.detach(), tm, scoring, side, th, tr_, tt, (h, r, t))
        check(res.better[j], res.equal[j], ora, 0.5, f"{name} {scoring} {side}")
        got_ranks.append((res.better[j], res.equal[j]))
    metrics = L.evaluate_ranking(model, th, tr_, tt, known=known, ks=(1, 3, 10, 100000), scoring=scoring)
    want = R.metrics_from_counts(res.better.cpu(), res.equal.cpu(), (1, 3, 10, 100000))
    for key in ("mr", "mrr", "hits@1", "hits@3", "hits@10", "hits@100000"):
        assert metrics[key] == want[key], key
        assert all(math.isfinite(metrics[s][key]) for s in ("tail", "head"))
    assert metrics["hits@100000"] == 1.0 and metrics["n"] == 600
    assert metrics["tail"] == R.metrics_from_counts(res.better[0].cpu(), res.equal[0].cpu(), (1, 3, 10, 100000))


# ----------------------------------------------------------------------------- 5. no side effects
def test_no_side_effects(L, R, gpu_device):
    a, gd = _golden_model(L, "encoder_gcn_l2_gatenum", gpu_device, "transr")
    b, _ = _golden_model(L, "encoder_gcn_l2_gatenum", gpu_device, "transr")
    c, _ = _golden_model(L, "encoder_gcn_l2_gatenum", gpu_device, "transr")      # a second model that never ranks
    h, r, t = (torch.from_numpy(gd[k]).to(gpu_device) for k in ("h", "r", "t"))
    # eval mode: the kept inference table is reused, not dropped or rebuilt
    a.eval()
    with torch.no_grad():
        s_before = a(h[:50], t[:50], device=gpu_device, mode="predict")
    kept = a.__dict__.get("_eval_cache")
    L.evaluate_ranking(a, h[:100], r[:100], t[:100])
    assert not a.training and a.__dict__.get("_eval_cache") is kept
    # training mode is restored
    a.train()
    b.train()
    c.train()
    L.evaluate_ranking(a, h[:100], r[:100], t[:100], known=R.KnownTriples(h, r, t, a.n_entities, a.n_relations))
    assert a.training
    for name, p in a.named_parameters():
        q = dict(b.named_parameters())[name]
        if p.is_sparse:
            p, q = p.data.coalesce(), q.data.coalesce()
            assert torch.equal(p.indices().cpu(), q.indices().cpu()), name
            p, q = p.values(), q.values()
        assert torch.equal(p.data.cpu(), q.data.cpu()), name
    batch = [torch.from_numpy(gd[k]).to(gpu_device) for k in ("bh", "br", "bp", "bn")]
    losses = []
    for m in (a, b, c):
        loss = m(*batch, device=gpu_device, mode="pre_training")
        loss.backward()
        losses.append(loss.detach().cpu())
    assert torch.equal(losses[0], losses[1]) and torch.equal(losses[1], losses[2])
    # bit-identical gradients -- as far as the step itself is: some reductions of its backward are f32 atomics, whose
    # order may differ between two runs of the same step (b against c shows it); where they do, the ranked model's
    # gradient is held to the suite's gradient tolerance (1e-4 of the parameter's largest entry)
    for (name, pa), pb, pc in zip(a.named_parameters(), b.parameters(), c.parameters()):
        if pa.grad is None and pb.grad is None:
            continue
        ga, gb, gc = pa.grad.cpu(), pb.grad.cpu(), pc.grad.cpu()
        if torch.equal(gb, gc):
            assert torch.equal(ga, gb), name
        else:
            assert float((ga - gb).abs().max()) <= 1e-4 * float(gb.abs().max()), name
    a.eval()
    b.eval()
    with torch.no_grad():
        assert torch.equal(a(h[:50], t[:50], device=gpu_device, mode="predict").cpu(),
                           b(h[:50], t[:50], device=gpu_device, mode="predict").cpu())
        assert torch.equal(s_before.cpu(), b(h[:50], t[:50], device=gpu_device, mode="predict").cpu())


# ----------------------------------------------------------------------------- 6. scale
def test_scale_two_million_candidates(R, gpu_device):
    """N = 2 M, k = 300: N k 4 bytes > 2^31 (64-bit addressing), 512 queries over 4 relations, filtered."""
    gen = torch.Generator(device=gpu_device).manual_seed(2024)
    n, k, n_rel = 2_000_000, 300, 4
    table = torch.randn(n, k, generator=gen, device=gpu_device)
    relemb = torch.randn(n_rel, k, generator=gen, device=gpu_device) * 0.3
    model = StandIn(table, relemb, None, "transe")
    b = 512
    h = torch.randint(0, n, (b,), generator=gen, device=gpu_device)
    t = torch.randint(0, n, (b,), generator=gen, device=gpu_device)
    r = torch.arange(b, device=gpu_device) % n_rel
    t[0], h[1], t[2] = n - 1, n - 1, 0
    # plant truths near the queries so that ranks are small and non-trivial; rows past 2^31 / 4 / k as truths too
    t[:64] = torch.arange(n - 64, n, device=gpu_device)
    table[t[:64]] = table[h[:64]] + relemb[r[:64]] + 0.3 * torch.randn(64, k, generator=gen, device=gpu_device)
    known = (torch.cat([h, h[:32]]), torch.cat([r, r[:32]]), torch.cat([t, torch.randint(0, n, (32,), device=gpu_device)]))
    kt_ = R.KnownTriples(*known, n, n_rel)
    res = R.rank_triples(model, h, r, t, side="tail", known=kt_, scoring="transe")
    ora = oracle(table, relemb, None, "transe", "tail", h, r, t, known, chunk=1 << 17)
    check(res.better, res.equal, ora, 0.1, "scale", min_exact=0.1)
    assert float((res.better[:64] < 1000).double().mean()) > 0.9      # the planted truths rank near the top


# ----------------------------------------------------------------------------- 7. errors and edges
def test_errors_and_edges(L, R, gpu_device):
    gen = torch.Generator().manual_seed(5)
    model = random_model(gen, "transe", 300, 32, 32, 3, gpu_device)
    h = torch.tensor([0, 1, 2], device=gpu_device)
    r = torch.tensor([0, 1, 2], device=gpu_device)
    t = torch.tensor([3, 4, 5], device=gpu_device)
    with pytest.raises(IndexError):
        R.rank_triples(model, h, r, torch.tensor([3, 300, 5], device=gpu_device), scoring="transe")
    with pytest.raises(IndexError):
        R.rank_triples(model, torch.tensor([-1, 1, 2], device=gpu_device), r, t, scoring="transe")
    with pytest.raises(IndexError):
        R.rank_triples(model, h, torch.tensor([0, 3, 1], device=gpu_device), t, scoring="transe")
    with pytest.raises(IndexError):
        R.KnownTriples(h, torch.tensor([0, 7, 1], device=gpu_device), t, 300, 3)
    with pytest.raises(ValueError):
        R.rank_triples(model, h, r[:2], t, scoring="transe")
    with pytest.raises(ValueError):
        R.rank_triples(model, h, r, t, scoring="transr")           # no gat_trans_M
    wide = random_model(gen, "transe", 300, 16, 32, 3, gpu_device)
    with pytest.raises(ValueError):
        R.rank_triples(wide, h, r, t, scoring="transe")             # width 32 != relation_dim 16
    # one filter row and one filter relation per query: a short list is refused, not read past
    from literalkg_amd import ops
    filt = R.KnownTriples(h, r, t, 300, 3).by_head
    for frow, frel in ((h[:2], r), (h, r[:2]), (h[:2], r[:2])):
        said = f"{frow.numel()} filter rows and {frel.numel()} filter relations for 3 queries"
        with pytest.raises(ValueError, match=said):
            ops.rank_count(model.T[:3], model.T, None, t, filt, frow, frel)
    # the calls above leave nothing pending: a valid call works
    ok = R.rank_triples(model, h, r, t, side="both", scoring="transe")
    assert ok.better.shape == (2, 3)
    # empty query set
    e = torch.zeros(0, dtype=torch.int64, device=gpu_device)
    res = R.rank_triples(model, e, e, e, side="both", scoring="transe")
    assert res.better.shape == (2, 0) and res.rank.numel() == 0
    met = R.evaluate_ranking(model, e, e, e, scoring="transe")
    assert met["n"] == 0 and all(not math.isnan(v) for v in (met["mr"], met["mrr"], met["hits@10"]))
    # a NaN row among the candidates: the other ranks are unchanged, the NaN candidate counts nowhere
    for scoring in ("transe", "dot"):
        hh = torch.randint(0, 250, (64,), generator=gen).to(gpu_device)
        rr = torch.randint(0, 3, (64,), generator=gen).to(gpu_device)
        tt = torch.randint(0, 250, (64,), generator=gen).to(gpu_device)
        # the NaN candidate counts nowhere: the ranks equal those with row 299 filtered out
        drop = R.KnownTriples(torch.cat([hh, torch.full_like(tt, 299)]), torch.cat([rr, rr]),
                              torch.cat([torch.full_like(hh, 299), tt]), 300, 3)
        before = R.rank_triples(model, hh, rr, tt, side="both", known=drop, scoring=scoring)
        saved = model.T[299].clone()
        model.T[299] = float("nan")
        after = R.rank_triples(model, hh, rr, tt, side="both", scoring=scoring)
        model.T[299] = saved
        assert torch.equal(before.better, after.better) and torch.equal(before.equal, after.equal), scoring
        # a NaN truth / query: nothing counts, nothing faults
        saved = model.T[298].clone()
        model.T[298] = float("nan")
        nan_t = R.rank_triples(model, hh[:1], rr[:1], torch.full((1,), 298, device=gpu_device), scoring=scoring)
        model.T[298] = saved
        assert int(nan_t.better[0]) == 0 and int(nan_t.equal[0]) == 0


# ----------------------------------------------------------------------------- 8. drawn configurations
def draw(seed):
    rng = np.random.default_rng(seed)
    pick = lambda xs: xs[int(rng.integers(len(xs)))]
    scoring = pick(["transr", "transe", "dot"])
    n = pick([1, 2, 17, 64, 255, 256, 257, 1000, 3001])
    c = pick([1, 3, 16, 32, 33, 64, 100, 256, 300])
    k = c if scoring != "transr" else pick([1, 5, 16, 37, 64, 128, 300])
    n_rel = int(rng.integers(1, 12))
    return dict(scoring=scoring, n=n, c=c, k=k, n_rel=n_rel, filtered=bool(rng.random() < 0.6),
                batch=pick([None, None, 1, 5, 64, 100]), per_rel=pick([1, 3, 40, 300]))


@pytest.mark.parametrize("seed", [FUZZ_SEED0 + i for i in range(N_FUZZ)])
def test_drawn_configurations(R, gpu_device, seed):
    cfg = draw(seed)
    gen = torch.Generator().manual_seed(seed)
    model = random_model(gen, cfg["scoring"], cfg["n"], cfg["k"], cfg["c"], cfg["n_rel"], gpu_device)
    h, r, t = draw_queries(gen, cfg["n"], cfg["n_rel"], cfg["per_rel"])
    known = draw_known(gen, cfg["n"], cfg["n_rel"], h, r, t, 3 * h.numel()) if cfg["filtered"] else None
    run_and_check(R, model, cfg["scoring"], h, r, t, known, cfg["batch"], what=f"seed {seed} {cfg}")
