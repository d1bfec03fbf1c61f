"""GPU: filtered ranking under the MLP pair head (rank_pairs_mlp / evaluate_mlp_ranking of literalkg_amd/pairmlp.py,
ops.pair_mlp_rank_count, the prepare and count kernels of lkg_pairmlp.hip).

The contract is exactness: a pair's logit in the counting path has the bits ``mlp_scores(..., logits=True)`` stores for
it, so ``better`` / ``equal`` are the counts one gets by comparing the stored logits -- for every query, with any filter,
candidate set, batch size or order.  Tests 1 and 2 hold the kernels to that without a tolerance (1 on small-integer data
where every f32 step is exact and the expected counts come from integer arithmetic in Python; 2 on random models against
the stored logits).  Test 3 is independent of the device's logits: float64 logits Z with the per-pair error bound E of
tests/test_pairmlp_gpu.py (its module docstring derives it).  A candidate whose float64 logit beats the truth's by more
than E_c + E_t must be counted ``better``; one within E_c + E_t may fall either way; so

    sure <= better    and    better + equal <= sure + band        for every query,

with sure = #{kept c : Z_c - Z_t > E_c + E_t}, band = #{kept c != t : |Z_c - Z_t| <= E_c + E_t}.  The bound is a worst
case; that the band stays narrow (mean at most 5 % of N per shape: 0.64 % / 1.07 % / 3.3 % on the three shapes when
computed on the CPU) is asserted from the float64 reference alone.
"""
import pytest
import torch

from test_pairmlp_gpu import SHAPES, StandIn, _golden_mlp_model, int_head, int_logits, random_head, random_model, ref64

pytestmark = pytest.mark.gpu

N_QUERIES = 256


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


@pytest.fixture(scope="module")
def ops(L):
    from literalkg_amd import ops
    return ops


# ----------------------------------------------------------------------------- counting in torch from stored logits
def counts_from(d, tpos, kept):
    """(better, equal) int64 per row of the logits d (B x M) against the entry at column tpos[i]; kept: B x M bool, the
    candidates that take part (the truth's own column never does)"""
    rows = torch.arange(d.shape[0], device=d.device)
    kept = kept.clone()
    kept[rows, tpos] = False
    zt = d[rows, tpos][:, None]
    return ((d > zt) & kept).sum(1), ((d == zt) & kept).sum(1)


def eligibility(n, n_rel, side, q, r, cand, known):
    """B x len(cand) bool: (q_i, r_i, c) resp. (c, r_i, q_i) is not a known triple (r None: under no relation)"""
    kh, kr, kt = known
    a, b_ = (kh, kt) if side == "tail" else (kt, kh)              # a: the query's end, b_: the candidate's
    if r is None:
        keys = q[:, None] * n + cand[None, :]
        return ~torch.isin(keys, a * n + b_)
    keys = (q * n_rel + r)[:, None] * n + cand[None, :]
    return ~torch.isin(keys, (a * n_rel + kr) * n + b_)


# ----------------------------------------------------------------------------- 1. exact integer op
@pytest.mark.parametrize("n_q,n_c", [(50, 300), (1, 777), (65, 64), (130, 1000), (3, 5), (600, 300)])
def test_exact_integer_op(R, ops, gpu_device, n_q, n_c):
    gen = torch.Generator().manual_seed(n_q * 1000 + n_c)
    dev = gpu_device
    uq = torch.randint(-3, 4, (n_q, 128), generator=gen).float().to(dev)
    v = torch.randint(-3, 4, (n_c, 128), generator=gen).float().to(dev)
    head = int_head(gen, dev)
    want = int_logits(uq, v, *head)                                        # int64, on the CPU
    assert int(want.abs().max()) < 2 ** 16
    if want.numel() > 1000:
        assert want.unique().numel() < want.numel() // 4                   # ties are frequent
    stored = ops.pair_mlp_scores(uq, v, *head)
    truth = torch.randint(0, n_c, (n_q,), generator=gen)
    rows = torch.arange(n_q)

    def check(res, kept, what):
        better, equal, thr = res
        assert better.dtype == torch.int32 and equal.dtype == torch.int32 and thr.dtype == torch.float32, what
        assert better.shape == (n_q,) == equal.shape == thr.shape, what
        wb, we = counts_from(want, truth, kept)
        assert torch.equal(better.cpu().long(), wb), what
        assert torch.equal(equal.cpu().long(), we), what
        assert torch.equal(thr.view(torch.int32), stored[rows.to(dev), truth.to(dev)].view(torch.int32)), what

    everyone = torch.ones((n_q, n_c), dtype=torch.bool)
    check(ops.pair_mlp_rank_count(uq, v, *head, truth.to(dev)), everyone, "no filter")
    assert int(counts_from(want, truth, everyone)[1].sum()) > 0 or want.numel() < 10000     # (ties with the truth do occur)

    # entity ids: a permutation with gaps of a larger id space; known triples over entity ids that include every truth,
    # ids outside the candidate set, and duplicates; query 0 is known with all but 4 candidates under relation 1
    n_ent, n_rel = 2 * n_c + 11, 3
    cand = torch.randperm(n_ent, generator=gen)[:n_c]
    frow = torch.randint(0, n_ent, (n_q,), generator=gen)
    m = 40 * n_q
    kh = frow[torch.randint(0, n_q, (m,), generator=gen)]
    kt = torch.where(torch.rand(m, generator=gen) < 0.8, cand[torch.randint(0, n_c, (m,), generator=gen)],
                     torch.randint(0, n_ent, (m,), generator=gen))
    kr = torch.randint(0, n_rel, (m,), generator=gen)
    kh, kt, kr = (torch.cat([x, y]) for x, y in ((kh, frow), (kt, cand[truth]), (kr, torch.randint(0, n_rel, (n_q,), generator=gen))))
    if n_c > 8:
        rest = torch.tensor([j for j in range(n_c) if j != int(truth[0])][: n_c - 5])       # all but the truth and 4 others
        kh = torch.cat([kh, frow[0].repeat(rest.numel())])
        kt = torch.cat([kt, cand[rest]])
        kr = torch.cat([kr, torch.ones(rest.numel(), dtype=torch.int64)])
    dup = torch.randint(0, kh.numel(), (kh.numel() // 3,), generator=gen)
    kh, kt, kr = (torch.cat([x, x[dup]]) for x in (kh, kt, kr))
    known = R.KnownTriples(kh.to(dev), kr.to(dev), kt.to(dev), n_ent, n_rel)
    slot = {c: j for j, c in enumerate(cand.tolist())}
    by_row = {}
    for i, f in enumerate(frow.tolist()):
        by_row.setdefault(f, []).append(i)

    def kept_under(frel_l):
        kept = torch.ones((n_q, n_c), dtype=torch.bool)
        for a, rel, c in zip(kh.tolist(), kr.tolist(), kt.tolist()):
            if c in slot:
                for i in by_row.get(a, ()):
                    if frel_l[i] < 0 or frel_l[i] == rel:
                        kept[i, slot[c]] = False
        return kept

    for name, frel in (("any", torch.full((n_q,), -1, dtype=torch.int64)), ("fixed", torch.ones(n_q, dtype=torch.int64)),
                       ("random", torch.randint(0, n_rel, (n_q,), generator=gen))):
        kept = kept_under(frel.tolist())
        assert int((~kept).sum()) >= n_q                                   # the filter bites
        res = ops.pair_mlp_rank_count(uq, v, *head, truth.to(dev), known.by_head, frow.to(dev), frel.to(dev),
                                      cand.to(dev))
        check(res, kept, f"candidate set, filter_rel {name}")
        if n_c > 8 and name in ("any", "fixed"):                           # query 0: at most 4 candidates are left
            assert int(res[0][0]) + int(res[1][0]) <= 4
    # the filter over the candidates' own numbering (no candidate ids)
    k2 = R.KnownTriples(torch.randint(0, n_c, (m,), generator=gen).to(dev), torch.randint(0, n_rel, (m,), generator=gen).to(dev),
                        torch.randint(0, n_c, (m,), generator=gen).to(dev), n_c, n_rel)
    frow2 = torch.randint(0, n_c, (n_q,), generator=gen)
    rowptr, col = (x.cpu().tolist() for x in k2.by_head[:2])
    kept = torch.ones((n_q, n_c), dtype=torch.bool)
    for i, f in enumerate(frow2.tolist()):
        kept[i, col[rowptr[f]:rowptr[f + 1]]] = False
    check(ops.pair_mlp_rank_count(uq, v, *head, truth.to(dev), k2.by_head, frow2.to(dev),
                                  torch.full((n_q,), -1, dtype=torch.int64, device=dev)), kept, "identity slots")
    with pytest.raises(ValueError):
        ops.pair_mlp_rank_count(uq, v, *head, truth[:-1].to(dev) if n_q > 1 else truth.repeat(2).to(dev))
    with pytest.raises(ValueError):
        ops.pair_mlp_rank_count(uq[:, :100], v, *head, truth.to(dev))
    with pytest.raises(ValueError):                                         # a filter over other rows needs candidate ids
        ops.pair_mlp_rank_count(uq, v, *head, truth.to(dev), known.by_head, frow.to(dev), frow.to(dev))


# ----------------------------------------------------------------------------- random models: stored logits, float64
@pytest.fixture(scope="module")
def cases(L, R, gpu_device):
    """per shape: the model, 256 pairs (h, t) with relations, known triples that bite on both sides, a candidate subset
    that holds every truth, and per side the device's stored logits D and float64's (Z, E), 256 x n: row i, column c =
    the pair (h_i, c) (tail side) resp. (c, t_i) (head side)"""
    from types import SimpleNamespace
    made = {}

    def get(n, c):
        if (n, c) in made:
            return made[(n, c)]
        dev = gpu_device
        model, gen = random_model(100 + n + c, n, c, dev)
        n_rel = model.n_relations
        h, t = (torch.randint(0, n, (N_QUERIES,), generator=gen).to(dev) for _ in range(2))
        r = torch.randint(0, n_rel, (N_QUERIES,), generator=gen).to(dev)
        every = torch.arange(n, device=dev)
        D = dict(tail=L.mlp_scores(model, h, every, logits=True),
                 head=L.mlp_scores(model, every, t, logits=True).T.contiguous())
        zt, et = ref64(model, h, every)
        zh, eh = ref64(model, every, t, chunk=512)
        # known: some of each query's best candidates (own relation or another), random triples, the pairs themselves, twice
        kh, kr, kt = [h, h], [r, r], [t, t]
        for side, q in (("tail", h), ("head", t)):
            top = torch.topk(D[side], 12, dim=1).indices
            pick = torch.rand(top.shape, generator=gen).to(dev) < 0.4
            qq, cc, rr = q[:, None].expand_as(top)[pick], top[pick], r[:, None].expand_as(top)[pick]
            rr = torch.where(torch.rand(rr.shape, generator=gen).to(dev) < 0.3, (rr + 1) % n_rel, rr)
            kh.append(qq if side == "tail" else cc)
            kt.append(cc if side == "tail" else qq)
            kr.append(rr)
        kh.append(torch.randint(0, n, (2000,), generator=gen).to(dev))
        kt.append(torch.randint(0, n, (2000,), generator=gen).to(dev))
        kr.append(torch.randint(0, n_rel, (2000,), generator=gen).to(dev))
        known = tuple(torch.cat(x) for x in (kh, kr, kt))
        sub = {}
        for side, truth in (("tail", t), ("head", h)):
            s_ = torch.randperm(n, generator=gen)[: (2 * n) // 3].to(dev)
            s_ = torch.cat([s_, truth.unique()[~torch.isin(truth.unique(), s_)]])
            sub[side] = s_[torch.randperm(s_.numel(), generator=gen).to(dev)]      # unsorted entity ids
        made[(n, c)] = SimpleNamespace(model=model, gen=gen, n=n, n_rel=n_rel, h=h, t=t, r=r, every=every, D=D,
                                       Z=dict(tail=zt, head=zh.T.contiguous()), E=dict(tail=et, head=eh.T.contiguous()),
                                       known=known, kt=R.KnownTriples(*known, n, n_rel), sub=sub)
        return made[(n, c)]
    return get


def variants(cs, side):
    """(what, r, known triples or None, candidate ids or None) -- with and without a filter (r given and r=None), with
    and without a candidate set"""
    for kn in (None, "any", "rel"):
        for cand in (None, cs.sub[side]):
            yield (f"{side} known={kn} candidates={'subset' if cand is not None else 'all'}",
                   cs.r if kn == "rel" else None, cs.known if kn else None, cand)


def kept_and_truth(cs, side, r, known, cand):
    q, truth = (cs.h, cs.t) if side == "tail" else (cs.t, cs.h)
    cc = cs.every if cand is None else cand
    kept = torch.ones((q.numel(), cc.numel()), dtype=torch.bool, device=q.device) if known is None else \
        eligibility(cs.n, cs.n_rel, side, q, r, cc, known)
    pos_of = torch.full((cs.n,), -1, dtype=torch.int64, device=q.device)
    pos_of[cc] = torch.arange(cc.numel(), device=q.device)
    tpos = pos_of[truth]
    assert bool((tpos >= 0).all())
    return cc, kept, tpos


# ----------------------------------------------------------------------------- 2. the bits of mlp_scores
@pytest.mark.parametrize("n,c", SHAPES)
@pytest.mark.parametrize("side", ["tail", "head"])
def test_same_counts_as_the_stored_logits(L, cases, n, c, side):
    cs = cases(n, c)
    for what, r, known, cand in variants(cs, side):
        cc, kept, tpos = kept_and_truth(cs, side, r, known, cand)
        wb, we = counts_from(cs.D[side][:, cc], tpos, kept)
        res = L.rank_pairs_mlp(cs.model, cs.h, cs.t, r, side=side, known=cs.kt if known is not None else None,
                               candidates=cand)
        assert res.side == side and res.better.dtype == torch.int64 and res.rank.dtype == torch.float64
        assert torch.equal(res.better, wb), (n, c, what)                   # every query, exactly
        assert torch.equal(res.equal, we), (n, c, what)
        assert torch.equal(res.rank, 1.0 + wb.double() + 0.5 * we.double()), (n, c, what)
        if known is not None:
            rows = torch.arange(N_QUERIES, device=tpos.device)
            assert int((~kept).sum()) > N_QUERIES and bool((~kept[rows, tpos]).all())    # the filter bites and names the truths
            free, _ = counts_from(cs.D[side][:, cc], tpos, torch.ones_like(kept))
            assert int((free - wb).sum()) > 0                              # ... and changes the counts
    both = L.rank_pairs_mlp(cs.model, cs.h, cs.t, cs.r, side="both", known=cs.kt)
    one = L.rank_pairs_mlp(cs.model, cs.h, cs.t, cs.r, side=side, known=cs.kt)
    j = 0 if side == "tail" else 1
    assert both.better.shape == (2, N_QUERIES) and torch.equal(both.better[j], one.better) and \
        torch.equal(both.equal[j], one.equal) and torch.equal(both.rank[j], one.rank)


# ----------------------------------------------------------------------------- 3. against float64
@pytest.mark.parametrize("n,c", SHAPES)
@pytest.mark.parametrize("side", ["tail", "head"])
def test_counts_against_float64(L, cases, n, c, side):
    cs = cases(n, c)
    rows = torch.arange(N_QUERIES, device=cs.h.device)
    for what, r, known, cand in variants(cs, side):
        cc, kept, tpos = kept_and_truth(cs, side, r, known, cand)
        z, e = cs.Z[side][:, cc], cs.E[side][:, cc]
        zt, et = z[rows, tpos][:, None], e[rows, tpos][:, None]
        others = kept.clone()
        others[rows, tpos] = False
        sure = ((z - zt > e + et) & others).sum(1)
        band = (((z - zt).abs() <= e + et) & others).sum(1)
        share = float(band.double().mean()) / cc.numel()
        res = L.rank_pairs_mlp(cs.model, cs.h, cs.t, r, side=side, known=cs.kt if known is not None else None,
                               candidates=cand)
        b64, e64 = counts_from(z, tpos, kept)
        exact = float(((res.better == b64) & (res.equal == e64)).double().mean())
        print(f"\n[{n} x {c} {what}] mean band {100 * share:.2f} % of {cc.numel()} candidates; "
              f"queries with float64's counts exactly: {100 * exact:.1f} %")
        assert share <= 0.05, (n, c, what, share)                          # from float64 alone: the check is not vacuous
        assert bool((sure <= res.better).all()), (n, c, what)
        assert bool((res.better + res.equal <= sure + band).all()), (n, c, what)


# ----------------------------------------------------------------------------- 4. agreement with the top-k path
def in_list(ids, zs, truth, better, equal, k):
    """every query with better + equal < k finds its truth in the list at a position in [better, better + equal], and
    exactly equal + 1 list entries carry its logit; returns how many queries that was"""
    ids, zs, truth, better, equal = (x.cpu() for x in (ids, zs, truth, better, equal))
    n_checked = 0
    for i in range(truth.numel()):
        bt, eq = int(better[i]), int(equal[i])
        if bt + eq >= k:
            continue
        n_checked += 1
        row = ids[i].tolist()
        assert int(truth[i]) in row, (i, bt, eq)
        pos = row.index(int(truth[i]))
        assert bt <= pos <= bt + eq, (i, pos, bt, eq)
        assert int((zs[i] == zs[i, pos]).sum()) == eq + 1, (i, eq)
    return n_checked


def test_agrees_with_topk_at_the_ops_level(R, ops, gpu_device):
    gen = torch.Generator().manual_seed(77)
    dev = gpu_device
    n_q, n_c, n_rel, k = 200, 500, 3, 64
    uq = torch.randint(-3, 4, (n_q, 128), generator=gen).float().to(dev)
    v = torch.randint(-3, 4, (n_c, 128), generator=gen).float().to(dev)
    head = int_head(gen, dev)
    truth = torch.randint(0, n_c, (n_q,), generator=gen)
    n_ent = 3 * n_c
    cand = torch.randperm(n_ent, generator=gen)[:n_c]
    frow = torch.randperm(n_ent, generator=gen)[:n_q]                       # distinct rows: a query's pair is its own
    m = 30 * n_q
    kh, kt = frow[torch.randint(0, n_q, (m,), generator=gen)], cand[torch.randint(0, n_c, (m,), generator=gen)]
    kr = torch.randint(0, n_rel, (m,), generator=gen)
    pairs = set(zip(frow.tolist(), cand[truth].tolist()))
    keep = torch.tensor([(a, b_) not in pairs for a, b_ in zip(kh.tolist(), kt.tolist())])
    known = R.KnownTriples(kh[keep].to(dev), kr[keep].to(dev), kt[keep].to(dev), n_ent, n_rel)
    for frel in (torch.full((n_q,), -1, dtype=torch.int64), torch.randint(0, n_rel, (n_q,), generator=gen)):
        args = (known.by_head, frow.to(dev), frel.to(dev), cand.to(dev))
        better, equal, thr = ops.pair_mlp_rank_count(uq, v, *head, truth.to(dev), *args)
        ids, zs = ops.pair_mlp_topk(uq, v, *head, k, *args)
        n_checked = in_list(ids, zs, cand[truth], better, equal, k)
        assert n_checked >= 20, n_checked
        assert int(equal.sum()) > n_q // 4                                 # ties are frequent here


@pytest.mark.parametrize("side", ["tail", "head"])
def test_agrees_with_predict_topk(L, R, gpu_device, side):
    n, c, n_rel, k = 600, 40, 4, 128
    model, gen = random_model(400 + len(side), n, c, gpu_device)
    model.n_relations = n_rel
    model.T[500:510] = model.T[100:110]                                    # a few bit-identical rows, so that ties occur
    m_all = 4000
    h, t = (torch.randint(0, n, (m_all,), generator=gen).to(gpu_device) for _ in range(2))
    rr = torch.randint(0, n_rel, (m_all,), generator=gen).to(gpu_device)
    h[:10], t[:10] = torch.arange(100, 110, device=gpu_device), torch.arange(100, 110, device=gpu_device)
    test, train = torch.arange(0, 400, device=gpu_device), torch.arange(400, m_all, device=gpu_device)
    keys_test = set(zip(h[test].tolist(), rr[test].tolist(), t[test].tolist()))
    keep = torch.tensor([(a, b_, c_) not in keys_test for a, b_, c_ in
                         zip(h[train].tolist(), rr[train].tolist(), t[train].tolist())], device=gpu_device)
    train = train[keep]
    known = R.KnownTriples(h[train], rr[train], t[train], n, n_rel)
    th, tr_, tt = h[test], rr[test], t[test]
    rk = L.rank_pairs_mlp(model, th, tt, tr_, side=side, known=known)
    q_ids, truth = (th, tt) if side == "tail" else (tt, th)
    res = L.predict_topk(model, q_ids, tr_, side=side, k=k, known=known, scoring="mlp")
    assert in_list(res.ids, res.kernel_scores, truth, rk.better, rk.equal, k) >= 20
    assert bool((rk.equal[:10] >= 1).all())                                # rows 500.. tie with the truths 100..


# ----------------------------------------------------------------------------- 5. invariance
def test_invariance(L, cases, gpu_device):
    cs = cases(3000, 48)
    h, t, r = cs.h[:100], cs.t[:100], cs.r[:100]
    for side in ("tail", "head", "both"):
        kw = dict(side=side, known=cs.kt)
        base = L.rank_pairs_mlp(cs.model, h, t, r, **kw)
        for bs in (1, 7, 64):
            res = L.rank_pairs_mlp(cs.model, h, t, r, batch_size=bs, **kw)
            assert torch.equal(res.better, base.better) and torch.equal(res.equal, base.equal), (side, bs)
        perm = torch.randperm(100, generator=cs.gen).to(gpu_device)
        res = L.rank_pairs_mlp(cs.model, h[perm], t[perm], r[perm], **kw)
        assert torch.equal(res.better, base.better[..., perm]) and torch.equal(res.equal, base.equal[..., perm]), side
        if side == "both":
            continue
        for cand in (cs.every, torch.randperm(cs.n, generator=cs.gen).to(gpu_device)):      # all entities, in any order
            res = L.rank_pairs_mlp(cs.model, h, t, r, candidates=cand, **kw)
            assert torch.equal(res.better, base.better) and torch.equal(res.equal, base.equal), side
        sub = cs.sub[side]
        a = L.rank_pairs_mlp(cs.model, h, t, r, candidates=sub, **kw)
        b_ = L.rank_pairs_mlp(cs.model, h, t, r, candidates=sub[torch.randperm(sub.numel(), generator=cs.gen).to(gpu_device)],
                              batch_size=7, **kw)
        assert torch.equal(a.better, b_.better) and torch.equal(a.equal, b_.equal), side
        assert bool((a.better <= base.better).all()) and int((base.better - a.better).sum()) > 0


def test_duplicated_rows_tie(L, gpu_device):
    n, c = 700, 24
    model, gen = random_model(31, n, c, gpu_device)
    model.T[600:620] = model.T[50:70]
    model.T[650:660] = model.T[50:60]
    h = torch.randint(0, n, (20,), generator=gen).to(gpu_device)
    t = torch.arange(50, 70, device=gpu_device)
    res = L.rank_pairs_mlp(model, h, t, side="both")
    assert bool((res.equal[0, :10] >= 2).all()) and bool((res.equal[0, 10:] >= 1).all())
    d = L.mlp_scores(model, h, torch.arange(n, device=gpu_device), logits=True)
    wb, we = counts_from(d, t, torch.ones_like(d, dtype=torch.bool))
    assert torch.equal(res.better[0], wb) and torch.equal(res.equal[0], we)
    # head side: the heads 50.. as truths, with their copies among the candidates
    res = L.rank_pairs_mlp(model, t, h, side="head")
    assert bool((res.equal[:10] >= 2).all()) and bool((res.equal[10:] >= 1).all())
    # a known triple takes a copy out again; one under another relation does not
    known = L.KnownTriples(h[:1], torch.zeros(1, dtype=torch.int64, device=gpu_device),
                           torch.tensor([600], device=gpu_device), n, model.n_relations)
    zero, one = (torch.full((1,), x, dtype=torch.int64, device=gpu_device) for x in (0, 1))
    full = L.rank_pairs_mlp(model, h[:1], t[:1])
    assert int(L.rank_pairs_mlp(model, h[:1], t[:1], known=known).equal[0]) == int(full.equal[0]) - 1
    assert int(L.rank_pairs_mlp(model, h[:1], t[:1], zero, known=known).equal[0]) == int(full.equal[0]) - 1
    assert int(L.rank_pairs_mlp(model, h[:1], t[:1], one, known=known).equal[0]) == int(full.equal[0])
    # a query that is the head of no known triple walks an empty filter row: the unfiltered counts
    q = (h[:1] + 1) % n
    lone, free = L.rank_pairs_mlp(model, q, t[:1], zero, known=known), L.rank_pairs_mlp(model, q, t[:1])
    assert torch.equal(lone.better, free.better) and torch.equal(lone.equal, free.equal)


def test_errors_on_the_device(L, R, gpu_device):
    n = 300
    model, gen = random_model(9, n, 24, gpu_device)
    h, t = torch.tensor([5, 17, 100], device=gpu_device), torch.tensor([9, 299, 0], device=gpu_device)
    with pytest.raises(IndexError):
        L.rank_pairs_mlp(model, torch.tensor([0, n], device=gpu_device), t[:2])
    with pytest.raises(IndexError):
        L.rank_pairs_mlp(model, h, t, torch.tensor([0, 1, model.n_relations], device=gpu_device))
    with pytest.raises(ValueError, match="1 of the 3 true tails"):
        L.rank_pairs_mlp(model, h, t, candidates=torch.tensor([9, 0, 4, 5], device=gpu_device))
    with pytest.raises(ValueError, match="known"):
        L.rank_pairs_mlp(model, h, t, known=R.KnownTriples(h, torch.zeros_like(h), t, n + 1, 3))
    ok = L.rank_pairs_mlp(model, h, t.cpu(), candidates=torch.tensor([9, 0, 299, 5]))     # ids may come from the host
    assert ok.better.shape == (3,) and bool((ok.better + ok.equal <= 3).all())            # nothing left pending
    nan = StandIn(model.T.clone(), {k: getattr(model, k) for k in ("fc1", "norm1", "fc2", "norm2", "fc3")})
    nan.T[7] = float("nan")
    res = L.rank_pairs_mlp(nan, torch.tensor([5, 5], device=gpu_device), torch.tensor([9, 7], device=gpu_device))
    ref = L.rank_pairs_mlp(model, h[:1], t[:1])
    assert int(res.better[1]) == 0 == int(res.equal[1])                    # a NaN truth: 0 / 0
    assert int(ref.better[0]) - 1 <= int(res.better[0]) <= int(ref.better[0])     # a NaN candidate counts nowhere
    assert int(res.better[0]) + int(res.equal[0]) <= n - 2


# ----------------------------------------------------------------------------- 6. the whole model
@pytest.mark.parametrize("name", ["mlp_model_gcn_l1_scale", "mlp_bce_gcn_l2_scale"])
def test_whole_model_on_the_reference_fixtures(L, R, gpu_device, name):
    m, gd = _golden_mlp_model(L, name, gpu_device)
    heads, tails = (torch.from_numpy(gd[k]).to(gpu_device) for k in ("heads", "tails"))
    n = m.n_entities
    every = torch.arange(n, device=gpu_device)
    rel = torch.zeros_like(heads)
    trip = (torch.cat([heads, tails]), torch.cat([rel, rel]), torch.cat([tails, heads]))
    known = R.KnownTriples(*trip, n, m.n_relations)
    d = dict(tail=m.mlp_scores(heads, every, logits=True), head=m.mlp_scores(every, tails, logits=True).T.contiguous())
    want = {}
    for side, q, truth in (("tail", heads, tails), ("head", tails, heads)):
        kept = eligibility(n, m.n_relations, side, q, None, every, trip)
        want[side] = counts_from(d[side], truth, kept)
        res = m.rank_pairs(heads, tails, side=side, known=known)
        assert torch.equal(res.better, want[side][0]) and torch.equal(res.equal, want[side][1]), side
    both = m.rank_pairs(heads, tails, side="both", known=known, batch_size=40)
    assert torch.equal(both.better, torch.stack([want["tail"][0], want["head"][0]]))
    assert torch.equal(both.equal, torch.stack([want["tail"][1], want["head"][1]]))
    ks = (1, 5, 20)
    got = L.evaluate_mlp_ranking(m, heads, tails, known=known, ks=ks)
    exp = R.metrics_from_counts(both.better.cpu(), both.equal.cpu(), ks)
    exp["tail"] = R.metrics_from_counts(both.better[0].cpu(), both.equal[0].cpu(), ks)
    exp["head"] = R.metrics_from_counts(both.better[1].cpu(), both.equal[1].cpu(), ks)
    assert got == exp and got["n"] == 2 * heads.numel() and 1.0 <= got["mr"] <= n
    one = L.evaluate_mlp_ranking(m, heads, tails, known=known, ks=ks, side="tail", candidates=torch.unique(tails))
    assert set(one) == {"n", "mr", "mrr", "hits@1", "hits@5", "hits@20", "tail"} and one["n"] == heads.numel()
    sub = m.rank_pairs(heads, tails, known=known, candidates=torch.unique(tails))
    assert one["tail"] == R.metrics_from_counts(sub.better.cpu(), sub.equal.cpu(), ks)
    assert bool((sub.better <= want["tail"][0]).all())


@pytest.mark.parametrize("training", [False, True])
def test_model_state_untouched(L, R, gpu_device, training):
    m, gd = _golden_mlp_model(L, "mlp_model_gcn_l1_scale", gpu_device)
    heads, tails = (torch.from_numpy(gd[k]).to(gpu_device) for k in ("heads", "tails"))
    with torch.no_grad():
        m._table_for_inference()
    m.train(training)
    cache = m.__dict__.get("_eval_cache")
    assert (cache is None) == training
    before = {k: (v, v._version, v.detach().clone()) for k, v in list(m.named_parameters()) + list(m.named_buffers())
              if not v.is_sparse}
    assert "norm1.num_batches_tracked" in before and "norm2.running_var" in before
    known = R.KnownTriples(heads, torch.zeros_like(heads), tails, m.n_entities, m.n_relations)
    res = m.rank_pairs(heads, tails, side="both", known=known)
    res_c = L.rank_pairs_mlp(m, heads, tails, torch.zeros_like(heads), side="head", known=known,
                             candidates=torch.unique(heads))
    assert m.training == training
    for mod in (m.norm1, m.norm2, m.fc1):
        assert mod.training == training
    assert m.__dict__.get("_eval_cache") is cache
    out = L.evaluate_mlp_ranking(m, heads, tails, known=known)
    assert m.training == training
    for mod in (m.norm1, m.norm2, m.fc1):
        assert mod.training == training
    if not training:
        assert m.__dict__.get("_eval_cache") is cache
        assert out == {**R.metrics_from_counts(res.better.cpu(), res.equal.cpu()),
                       "tail": R.metrics_from_counts(res.better[0].cpu(), res.equal[0].cpu()),
                       "head": R.metrics_from_counts(res.better[1].cpu(), res.equal[1].cpu())}
    after = dict(list(m.named_parameters()) + list(m.named_buffers()))
    for k, (v, ver, val) in before.items():
        assert after[k] is v and v._version == ver and torch.equal(v.detach(), val), k
    assert res.better.shape == (2, heads.numel()) and res_c.better.shape == (heads.numel(),) and out["n"] == 2 * heads.numel()


# ----------------------------------------------------------------------------- 7. large shape, once
def test_two_million_candidates(L, R, gpu_device):
    n, c = 1 << 21, 32
    gen = torch.Generator().manual_seed(2027)
    dgen = torch.Generator(device=gpu_device).manual_seed(2027)
    table = torch.nn.functional.normalize(torch.randn(n, c, generator=dgen, device=gpu_device), dim=1)
    model = StandIn(table, random_head(gen, c, gpu_device))
    h = torch.cat([torch.tensor([0, n - 1, 1 << 20]), torch.randint(0, n, (9,), generator=gen)]).to(gpu_device)
    t = torch.cat([torch.tensor([n - 1, 0, n - 3]), torch.randint(0, n, (9,), generator=gen)]).to(gpu_device)
    table[n - 64:n - 52] = table[t]                     # copies of the truths' rows past 2^31 / 128 / 4: ties up there
    every = torch.arange(n, device=gpu_device)
    kh = torch.cat([h.repeat_interleave(50), h])
    kt = torch.cat([torch.randint(n - 4096, n - 64, (kh.numel() - h.numel(),), generator=gen).to(gpu_device), t])
    known = R.KnownTriples(kh, torch.zeros_like(kh), kt, n, model.n_relations)
    res = L.rank_pairs_mlp(model, h, t, side="both", known=known)
    for j, (side, q, truth) in enumerate((("tail", h, t), ("head", t, h))):
        better = torch.zeros(q.numel(), dtype=torch.int64, device=gpu_device)
        equal = torch.zeros_like(better)
        zt = (L.mlp_scores(model, q, truth, logits=True) if side == "tail" else
              L.mlp_scores(model, truth, q, logits=True).T).diagonal()[:, None]
        for lo in range(0, n, 1 << 19):                  # the stored logits, a chunk of candidates at a time
            cols = every[lo:lo + (1 << 19)]
            d = L.mlp_scores(model, q, cols, logits=True) if side == "tail" else L.mlp_scores(model, cols, q, logits=True).T
            kept = eligibility(n, model.n_relations, side, q, None, cols, (kh, torch.zeros_like(kh), kt))
            kept &= cols[None, :] != truth[:, None]
            better += ((d > zt) & kept).sum(1)
            equal += ((d == zt) & kept).sum(1)
        assert torch.equal(res.better[j], better) and torch.equal(res.equal[j], equal), side
    assert bool((res.equal[0] >= 1).all())              # tail side: the copies at n - 64 .. tie with their truths
