"""GPU: threshold retrieval under the MLP pair head (literalkg_amd/pairmlp.py: predict_accepted_mlp, count_accepted_mlp;
lkg_pairmlp.hip: pair_mlp_accept_kernel; include/literalkg_hip.h) against the references of
pair_accept_cases.py -- without tolerance: the object is unique.

The op tier runs on small-integer operands, where every logit is an exact integer in float32 and the int64 reference is
the truth; the model tier takes its logit matrix from mlp_scores(..., logits=True), whose bits the lists must carry, and
builds the lists from it in numpy.  Shapes cross the kernel's edges: 64 query rows per workgroup (16 / 32 for small
batches), 64 candidates per tile, 16 per wave, 4 speaking lanes per row group."""
import math

import numpy as np
import pytest
import torch

import invariance as V
import pair_accept_cases as PA
import test_pairmlp_gpu as PG

pytestmark = pytest.mark.gpu

MAX_SPLITS = 64
SPLITS = (0, 1, 3, MAX_SPLITS)


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
    assert ops.TOPK_MAX_SPLITS == MAX_SPLITS
    return ops


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


# ----------------------------------------------------------------------------- 1. the three entry points, exactly
def sorted_entries(rows, ids, z):
    """the appended entries grouped by row and ordered inside it, as numpy (rows, ids, z)"""
    rows, ids, z = rows.cpu().numpy().astype(np.int64), ids.cpu().numpy().astype(np.int64), z.cpu().numpy()
    o = np.lexsort((ids, -z, rows))
    return rows[o], ids[o], z[o]


@pytest.mark.parametrize("n_c", [1, 3, 17, 64, 65, 257, 1000])
@pytest.mark.parametrize("n_q", [1, 63, 65, 130])
def test_exact_integer_op(L, R, ops, gpu_device, n_q, n_c):
    dev = gpu_device
    gen = torch.Generator().manual_seed(n_q * 10007 + n_c)
    uq = torch.randint(-3, 4, (n_q, 128), generator=gen).float()
    v = torch.randint(-3, 4, (n_c, 128), generator=gen).float()
    head = PG.int_head(gen, dev)
    want = PA.int_logits(uq.numpy(), v.numpy(), *(t.cpu().numpy() for t in head))
    assert int(np.abs(want).max()) < 2 ** 16                                  # exact in f32 with room
    z = want.astype(np.float32)
    uq, v = uq.to(dev), v.to(dev)
    # a threshold that EQUALS an observed logit of its row (the row's upper quartile): that pair is out, and the next
    # float below the threshold brings it in
    thr = np.array([np.sort(z[i])[(3 * n_c) // 4] for i in range(n_q)], dtype=np.float32)
    below = np.nextafter(thr, np.float32(-np.inf))
    assert (z == thr[:, None]).any(1).all()
    # entity ids through cand_ids (a permutation with gaps) and known triples that hit what would pass
    n_ent, n_rel = 2 * n_c + 11, 3
    cand = torch.randperm(n_ent, generator=gen)[:n_c]
    cand_l = cand.tolist()
    frow = torch.randint(0, n_ent, (n_q,), generator=gen)
    frow_l = frow.tolist()
    kh, kr, kt = [], [], []
    for i in range(n_q):
        passing = np.flatnonzero(z[i] >= thr[i])
        for j in passing[:: max(1, passing.size // 3)][:3]:
            kh.append(frow_l[i]), kr.append(int(torch.randint(0, n_rel, (1,), generator=gen))), kt.append(cand_l[j])
    m_extra = 10 * n_q
    kh += frow[torch.randint(0, n_q, (m_extra,), generator=gen)].tolist()
    kt += cand[torch.randint(0, n_c, (m_extra,), generator=gen)].tolist()
    kr += torch.randint(0, n_rel, (m_extra,), generator=gen).tolist()
    trip = set(zip(kh, kr, kt))
    t64 = lambda x: torch.tensor(x, dtype=torch.int64, device=dev)
    known = R.KnownTriples(t64(kh), t64(kr), t64(kt), n_ent, n_rel)
    frel_any = [-1] * n_q
    frel_own = torch.randint(0, n_rel, (n_q,), generator=gen).tolist()
    configs = [("plain", {}, np.arange(n_c), None)]
    for name, frel in (("any relation", frel_any), ("own relation", frel_own)):
        elig = PA.eligibility(frow_l, cand_l, "tail", trip, None if frel is frel_any else frel)
        kw = dict(filt=known.by_head, filter_row=frow.to(dev), filter_rel=t64(frel), cand_ids=cand.to(dev))
        configs.append((name, kw, np.array(cand_l), elig))
    assert not configs[1][3].all()                                            # the filter bites
    for name, kw, ids_of, elig in configs:
        for t_name, t in (("thr", thr), ("below", below)):
            ref = PA.accepted_lists(z, t, ids_of, elig)
            m = int(ref.rowptr[-1])
            ref_rows = np.repeat(np.arange(n_q), ref.counts)
            tt = torch.from_numpy(t).to(dev)
            for splits in SPLITS:
                what = f"{n_q} x {n_c} {name} {t_name} splits={splits}"
                cnt = ops.pair_mlp_accept_count(uq, v, *head, tt, splits=splits, **kw)
                assert cnt.dtype == torch.int32 and cnt.cpu().tolist() == ref.counts.tolist(), what
                # one pass, the buffer exactly large enough
                c2, rows, ii, zz, n_w = ops.pair_mlp_accept_append(uq, v, *head, tt, splits=splits, capacity=m, **kw)
                assert torch.equal(c2, cnt) and n_w == m and rows.numel() == m, what
                rr, ii, zz = sorted_entries(rows, ii, zz)
                assert (rr == ref_rows).all() and (ii == ref.ids).all(), what
                assert (zz.view(np.int32) == ref.logits.view(np.int32)).all(), what
                # one entry short: the counts stay exact, nothing is written past the capacity
                if m > 0:
                    c3, rows, ii, zz, n_w = ops.pair_mlp_accept_append(uq, v, *head, tt, splits=splits, capacity=m - 1,
                                                                       **kw)
                    assert torch.equal(c3, cnt) and n_w == m - 1 and rows.numel() == m - 1, what
                    got = set(zip(rows.cpu().tolist(), ii.cpu().tolist(), zz.cpu().tolist()))
                    assert len(got) == m - 1 and got <= set(zip(ref_rows.tolist(), ref.ids.tolist(), ref.logits.tolist())), what
                # two passes: emit into the counted segments, then the order
                rowptr, ii, ss, zz = ops.pair_mlp_accept_emit(uq, v, *head, tt, splits=splits, counts=cnt, **kw)
                assert rowptr.cpu().tolist() == ref.rowptr.tolist() and ii.dtype == torch.int64, what
                assert torch.equal(ss, -2 * zz), what
                ii, ss, zz = ops.accept_order(rowptr, ii, ss, zz, n_ent)
                assert ii.cpu().tolist() == ref.ids.tolist() and (bits(zz) == ref.logits.view(np.int32)).all(), what
                assert torch.equal(ss, -2 * zz), what
        if elig is None:                                                      # the equal pairs: out at thr, in just below
            at, under = PA.accepted_lists(z, thr, ids_of), PA.accepted_lists(z, below, ids_of)
            assert (under.counts > at.counts).all() and not (at.logits == np.repeat(thr, at.counts)).any()
            assert (under.logits == np.repeat(thr, under.counts)).sum() == (under.counts - at.counts).sum()
    # argument errors of the op layer
    tt = torch.from_numpy(thr).to(dev)
    with pytest.raises(ValueError):
        ops.pair_mlp_accept_count(uq, v, *head, tt.double())
    with pytest.raises(ValueError):
        ops.pair_mlp_accept_count(uq, v, *head, torch.zeros(n_q + 1, device=dev))
    with pytest.raises(ValueError):
        ops.pair_mlp_accept_count(uq, v, *head, tt, splits=MAX_SPLITS + 1)
    with pytest.raises(ValueError):
        ops.pair_mlp_accept_append(uq, v, *head, tt, capacity=-1)
    with pytest.raises(ValueError):
        ops.pair_mlp_accept_emit(uq, v, *head, tt, counts=torch.zeros(n_q, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        ops.pair_mlp_accept_emit(uq, v, *head, tt)


# ----------------------------------------------------------------------------- 2. the model tier
N_ENT, WIDTH, N_REL, N_QUERIES = 1000, 24, 5, 130


@pytest.fixture(scope="module")
def world(L, R, gpu_device):
    """One model, 130 queries, a candidate subset, known triples that hit the best candidates of either side, and the
    logit matrices of mlp_scores for both sides (row i, column c = query i against ENTITY c): computed once."""
    dev = gpu_device
    model, gen = PG.random_model(77, N_ENT, WIDTH, dev)
    model.n_relations = N_REL
    q = torch.randint(0, N_ENT, (N_QUERIES,), generator=gen)
    q[100:110] = q[:10]                                                       # some queries twice
    r = torch.randint(0, N_REL, (N_QUERIES,), generator=gen)
    r[100:110] = r[:10]
    subset = torch.randperm(N_ENT, generator=gen)[:601]                       # unsorted entity ids
    every = torch.arange(N_ENT, device=dev)
    qd = q.to(dev)
    Z = {"tail": L.mlp_scores(model, qd, every, logits=True).cpu().numpy(),
         "head": L.mlp_scores(model, every, qd, logits=True).T.contiguous().cpu().numpy()}
    kh, kr, kt = [], [], []
    q_l, r_l = q.tolist(), r.tolist()
    for side in ("tail", "head"):
        top = np.argsort(-Z[side], axis=1)[:, :40]
        for i in range(N_QUERIES):
            for j in top[i][torch.randperm(40, generator=gen)[:6].numpy()]:
                rel = r_l[i] if float(torch.rand(1, generator=gen)) < 0.6 else (r_l[i] + 1) % N_REL
                h, t = (q_l[i], int(j)) if side == "tail" else (int(j), q_l[i])
                kh.append(h), kr.append(rel), kt.append(t)
    extra = 3000
    kh += torch.randint(0, N_ENT, (extra,), generator=gen).tolist()
    kt += torch.randint(0, N_ENT, (extra,), generator=gen).tolist()
    kr += torch.randint(0, N_REL, (extra,), generator=gen).tolist()
    t64 = lambda x: torch.tensor(x, dtype=torch.int64, device=dev)
    known = R.KnownTriples(t64(kh), t64(kr), t64(kt), N_ENT, N_REL)
    from types import SimpleNamespace
    return SimpleNamespace(model=model, gen=gen, q=qd, r=r.to(dev), q_l=q_l, r_l=r_l, subset=subset.to(dev),
                           subset_l=subset.tolist(), Z=Z, triples=set(zip(kh, kr, kt)), kh=t64(kh), kr=t64(kr),
                           kt=t64(kt), known=known, elig={})


def case_reference(w, side, with_r, with_cand, thr=None):
    """(reference lists, threshold, logits of the case, eligibility) -- the threshold defaults to the median of the case's
    own reference logits, so about half the pairs pass"""
    cols = np.array(w.subset_l) if with_cand else np.arange(N_ENT)
    z = np.ascontiguousarray(w.Z[side][:, cols])
    key = (side, with_r, with_cand)
    if key not in w.elig:
        w.elig[key] = PA.eligibility(w.q_l, cols.tolist(), side, w.triples, w.r_l if with_r else None)
    if thr is None:
        thr = float(np.float32(np.median(z)))
    return PA.accepted_lists(z, thr, cols, w.elig[key]), thr, z, w.elig[key]


@pytest.mark.parametrize("with_cand", [False, True])
@pytest.mark.parametrize("with_r", [False, True])
@pytest.mark.parametrize("side", ["tail", "head"])
def test_lists_are_the_reference(L, world, side, with_r, with_cand):
    w = world
    ref, thr, z, elig = case_reference(w, side, with_r, with_cand)
    m = int(ref.rowptr[-1])
    with np.errstate(invalid="ignore"):
        passing = z > np.float32(thr)
    assert 0 < m < z.size and (ref.counts > 0).any() and (passing & ~elig).any()      # no case is vacuous
    kw = dict(r=w.r if with_r else None, logit_threshold=thr, side=side, known=w.known,
              candidates=w.subset if with_cand else None)
    res = L.predict_accepted_mlp(w.model, w.q, **kw)
    assert isinstance(res, L.AcceptedResult) and res.side == side and torch.equal(res.query_ids, w.q)
    PA.check_lists(res, ref, f"{side} r={with_r} candidates={with_cand}")
    n = L.count_accepted_mlp(w.model, w.q, **kw)
    assert n.dtype == torch.int64 and torch.equal(n, res.counts)
    # the methods are the functions
    PA.check_lists(L.LiteralKG.predict_accepted_pairs(w.model, w.q, **kw), ref)
    assert torch.equal(L.LiteralKG.count_accepted_pairs(w.model, w.q, **kw), n)
    # pairs() / triples(): the listed pairs in list order
    rows = np.repeat(np.arange(N_QUERIES), ref.counts)
    qq = np.array(w.q_l)[rows]
    h, t = res.pairs()
    hq, tc = (h, t) if side == "tail" else (t, h)
    assert hq.cpu().tolist() == qq.tolist() and tc.cpu().tolist() == ref.ids.tolist()
    if with_r:
        hh, rr, tt = res.triples()
        assert torch.equal(hh, h) and torch.equal(tt, t) and rr.cpu().tolist() == np.array(w.r_l)[rows].tolist()
    else:
        with pytest.raises(ValueError):
            res.triples()


@pytest.mark.parametrize("side", ["tail", "head"])
def test_every_list_is_a_prefix_of_the_topk_list(L, world, side):
    w = world
    depth = [0, 1, 5, 127, 128, 129, 500]
    desc = -np.sort(-w.Z[side], axis=1)
    thr = np.array([desc[i, depth[i % len(depth)]] for i in range(N_QUERIES)], dtype=np.float32)
    kw = dict(side=side, known=w.known)
    res = L.predict_accepted_mlp(w.model, w.q, w.r, logit_threshold=torch.from_numpy(thr).to(w.q.device), **kw)
    top = L.predict_topk(w.model, w.q, w.r, k=128, scoring="mlp", **kw)
    counts, rowptr = res.counts.cpu().tolist(), res.rowptr.cpu().tolist()
    assert min(counts) == 0 and any(0 < c < 128 for c in counts) and max(counts) > 128
    ids, ks, sc = res.ids.cpu(), res.kernel_scores.cpu(), res.scores.cpu()
    t_ids, t_ks, t_sc = top.ids.cpu(), top.kernel_scores.cpu(), top.scores.cpu()
    for i, c in enumerate(counts):
        m, lo = min(c, 128), rowptr[i]
        assert ids[lo:lo + m].tolist() == t_ids[i, :m].tolist(), i
        assert torch.equal(ks[lo:lo + m].view(torch.int32), t_ks[i, :m].view(torch.int32)), i
        assert torch.equal(sc[lo:lo + m].view(torch.int32), t_sc[i, :m].view(torch.int32)), i
        if c < 128:                                                           # the next top-k entry did not pass
            assert int(t_ids[i, c]) == -1 or float(t_ks[i, c]) <= float(thr[i]), i


def test_sentinels_and_special_values(L, world):
    w = world
    dev = w.q.device
    q, r = w.q[:40], w.r[:40]
    for side in ("tail", "head"):
        kw = dict(side=side, known=w.known)
        none = L.predict_accepted_mlp(w.model, q, r, logit_threshold=math.inf, **kw)
        assert none.ids.numel() == 0 and none.rowptr.tolist() == [0] * 41 and int(none.counts.sum()) == 0
        assert int(L.count_accepted_mlp(w.model, q, r, logit_threshold=math.inf, **kw).sum()) == 0
        # a NaN row: never listed as a candidate, an empty list as a query; -inf lists every eligible non-NaN candidate
        bad = int(q[3])
        table = w.model.T.clone()
        table[bad] = float("nan")
        model2 = PG.StandIn(table, {k: getattr(w.model, k) for k in ("fc1", "norm1", "fc2", "norm2", "fc3")}, N_REL)
        every = torch.arange(N_ENT, device=dev)
        z2 = (L.mlp_scores(model2, q, every, logits=True) if side == "tail"
              else L.mlp_scores(model2, every, q, logits=True).T.contiguous()).cpu().numpy()
        assert np.isnan(z2[:, bad]).all() and np.isnan(z2[3]).all() and not np.isnan(np.delete(z2[0], bad)).any()
        elig = PA.eligibility(w.q_l[:40], list(range(N_ENT)), side, w.triples, w.r_l[:40])
        ref = PA.accepted_lists(z2, -math.inf, np.arange(N_ENT), elig)
        res = L.predict_accepted_mlp(model2, q, r, logit_threshold=-math.inf, **kw)
        PA.check_lists(res, ref, f"-inf {side}")
        assert int(res.counts[3]) == 0 and bad not in res.ids.cpu().tolist()
        assert ref.counts[0] == elig[0].sum() - int(elig[0, bad]) > N_ENT // 2
        # threshold=0.5 is logit_threshold=0.0
        half, zero = (L.predict_accepted_mlp(w.model, q, r, **kw, **t) for t in (dict(threshold=0.5),
                                                                                 dict(logit_threshold=0.0)))
        default = L.predict_accepted_mlp(w.model, q, r, **kw)
        for a in (half, default):
            for name in ("rowptr", "ids", "scores", "kernel_scores", "counts"):
                V.same_bits(getattr(a, name), getattr(zero, name), name)
        assert 0 < zero.ids.numel() and bool((zero.kernel_scores > 0).all()) and bool((zero.scores >= 0.5).all())
        # another probability: float32(log(p / (1 - p))) formed in float64
        p7 = L.predict_accepted_mlp(w.model, q, r, threshold=0.7, **kw)
        PA.check_lists(p7, PA.accepted_lists(w.Z[side][:40], np.float32(math.log(0.7 / 0.3)), np.arange(N_ENT), elig))
        # per-query tensor thresholds are the per-query float calls
        thr = torch.linspace(-1.0, 2.0, 40)
        thr[5], thr[6], thr[7] = math.inf, -math.inf, float("nan")
        many = L.predict_accepted_mlp(w.model, q, r, logit_threshold=thr.to(dev), **kw)
        assert int(many.counts[5]) == 0 and int(many.counts[7]) == 0 and int(many.counts[6]) == int(elig[6].sum())
        for i in (0, 6, 17, 39):
            one = L.predict_accepted_mlp(w.model, q[i:i + 1], r[i:i + 1], logit_threshold=float(thr[i]), **kw)
            lo, hi = int(many.rowptr[i]), int(many.rowptr[i + 1])
            assert hi - lo == int(one.counts[0])
            V.same_bits(many.ids[lo:hi], one.ids)
            V.same_bits(many.kernel_scores[lo:hi], one.kernel_scores)
            V.same_bits(many.scores[lo:hi], one.scores)


# ----------------------------------------------------------------------------- 3. invariance, all by bits
def same_result(a, b, what):
    for name in ("rowptr", "counts", "ids", "kernel_scores", "scores"):
        V.same_bits(getattr(a, name), getattr(b, name), f"{what}: {name}")


def rows_of(res):
    rp = res.rowptr.cpu().tolist()
    ids, ks, sc = res.ids.cpu(), bits(res.kernel_scores), bits(res.scores)
    return [(ids[rp[i]:rp[i + 1]].tolist(), ks[rp[i]:rp[i + 1]].tolist(), sc[rp[i]:rp[i + 1]].tolist())
            for i in range(len(rp) - 1)]


@pytest.mark.parametrize("side", ["tail", "head"])
def test_invariance(L, R, world, side):
    w = world
    ref, thr, _, _ = case_reference(w, side, True, False)
    m = int(ref.rowptr[-1])
    kw = dict(logit_threshold=thr, side=side, known=w.known)
    base = L.predict_accepted_mlp(w.model, w.q, w.r, **kw)
    PA.check_lists(base, ref)
    variants = [dict(batch_size=1), dict(batch_size=7), dict(batch_size=None)] + [dict(splits=s) for s in SPLITS] + \
        [dict(buffer=x) for x in (0, 1, m, m - 1, 1 << 22)] + \
        [dict(batch_size=7, buffer=x, splits=3) for x in (0, 1, int(ref.counts[:7].sum()), int(ref.counts[:7].sum()) - 1)] + \
        [dict()] * 3
    for extra in variants:
        same_result(L.predict_accepted_mlp(w.model, w.q, w.r, **kw, **extra), base, f"{side} {extra}")
    assert torch.equal(L.count_accepted_mlp(w.model, w.q, w.r, batch_size=7, splits=3, **kw), base.counts)
    # queries permuted and duplicated
    rows = rows_of(base)
    assert rows[100:110] == rows[:10]                                          # duplicate queries get equal lists
    perm = torch.randperm(N_QUERIES, generator=w.gen).to(w.q.device)
    again = torch.cat([perm, perm[:9]])
    res = L.predict_accepted_mlp(w.model, w.q[again], w.r[again], **kw)
    assert rows_of(res) == [rows[i] for i in again.cpu().tolist()]
    # candidates permuted: all of them, in another order
    shuffled = torch.randperm(N_ENT, generator=w.gen).to(w.q.device)
    same_result(L.predict_accepted_mlp(w.model, w.q, w.r, candidates=shuffled, **kw), base, "candidates permuted")
    sub = case_reference(w, side, True, True, thr)[0]
    for cand in (w.subset, w.subset.flip(0), w.subset.sort().values):
        PA.check_lists(L.predict_accepted_mlp(w.model, w.q, w.r, candidates=cand, **kw), sub, "subset reordered")
    # known rebuilt with duplicate triples, in another order
    o = torch.randperm(w.kh.numel(), generator=w.gen).to(w.q.device)
    twice = R.KnownTriples(torch.cat([w.kh[o], w.kh[:500]]), torch.cat([w.kr[o], w.kr[:500]]),
                           torch.cat([w.kt[o], w.kt[:500]]), N_ENT, N_REL)
    same_result(L.predict_accepted_mlp(w.model, w.q, w.r, **dict(kw, known=twice)), base, "known with duplicates")
    # poisoned scratch and a side stream, on the one-pass route, the overflow route and the two-pass route
    for extra in (dict(), dict(buffer=m - 1), dict(buffer=0, batch_size=50)):
        for byte in (0xFF, 0x7F):
            with V.poisoned(byte):
                same_result(L.predict_accepted_mlp(w.model, w.q, w.r, **kw, **extra), base, f"poisoned {byte:#x} {extra}")
        with V.side_stream(), V.poisoned(0xFF):
            res = L.predict_accepted_mlp(w.model, w.q, w.r, **kw, **extra)
            n = L.count_accepted_mlp(w.model, w.q, w.r, **kw)
        same_result(res, base, f"side stream {extra}")
        assert torch.equal(n, base.counts)


# ----------------------------------------------------------------------------- 4. counts alone; the cap
def test_count_allocates_nothing_of_the_size_of_the_lists(L, gpu_device):
    n, b = 20000, 512
    model, gen = PG.random_model(5, n, WIDTH, gpu_device)
    q = torch.randint(0, n, (b,), generator=gen).to(gpu_device)
    L.count_accepted_mlp(model, q[:4], logit_threshold=0.0)                    # (workspaces the library keeps)

    def peak(thr):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        cnt = L.count_accepted_mlp(model, q, logit_threshold=thr)
        torch.cuda.synchronize()
        return cnt, torch.cuda.max_memory_allocated() - before

    none, p_none = peak(math.inf)
    every, p_every = peak(-math.inf)
    m = int(every.sum())
    assert int(none.sum()) == 0 and m == b * n and every.dtype == torch.int64
    print(f"\ncount_accepted_mlp: peak {p_none} bytes with M = 0, {p_every} bytes with M = {m} ({16 * m} bytes of lists)")
    assert p_every <= p_none + (1 << 20)                                       # the same, whatever M
    assert p_every < 4 * m                                                     # and below ONE float per listed entry


def test_max_total(L, world):
    w = world
    ref, thr, _, _ = case_reference(w, "tail", True, False)
    m = int(ref.rowptr[-1])
    kw = dict(logit_threshold=thr, known=w.known)
    for extra in (dict(), dict(batch_size=7), dict(buffer=0), dict(buffer=10, batch_size=40)):
        PA.check_lists(L.predict_accepted_mlp(w.model, w.q, w.r, max_total=m, **kw, **extra), ref, f"max_total = M {extra}")
        with pytest.raises(ValueError, match="max_total"):
            L.predict_accepted_mlp(w.model, w.q, w.r, max_total=m - 1, **kw, **extra)
    with pytest.raises(ValueError, match="max_total"):
        L.predict_accepted_mlp(w.model, w.q, w.r, max_total=0, **kw)
    assert L.predict_accepted_mlp(w.model, w.q, w.r, max_total=0, logit_threshold=math.inf).ids.numel() == 0
    assert torch.equal(L.count_accepted_mlp(w.model, w.q, w.r, **kw).cpu(), torch.from_numpy(ref.counts))   # no cap there


# ----------------------------------------------------------------------------- 5. the model's state is untouched
@pytest.mark.parametrize("training", [False, True])
def test_model_state_untouched(L, R, gpu_device, training):
    m, gd = PG._golden_mlp_model(L, "mlp_model_gcn_l1_scale", gpu_device)
    heads, tails = (torch.from_numpy(gd[k]).to(gpu_device) for k in ("heads", "tails"))
    with torch.no_grad():
        m._table_for_inference()
    every = torch.arange(m.n_entities, device=gpu_device)
    thr = float(m.mlp_scores(heads, every, logits=True).median())              # about half the pairs pass
    m.train(training)
    cache = m.__dict__.get("_eval_cache")
    assert (cache is None) == training
    before = {k: (v, v._version, v.detach().clone()) for k, v in list(m.named_parameters()) + list(m.named_buffers())
              if not v.is_sparse}
    assert "norm1.num_batches_tracked" in before and "norm2.running_var" in before
    known = R.KnownTriples(heads, torch.zeros_like(heads), tails, m.n_entities, m.n_relations)
    res = m.predict_accepted_pairs(heads, None, logit_threshold=thr, known=known)
    res_h = m.predict_accepted_pairs(tails, torch.zeros_like(tails), logit_threshold=thr, side="head", known=known, buffer=0)
    cnt = m.count_accepted_pairs(heads, None, logit_threshold=thr, known=known)
    assert m.training == training
    for mod in (m.norm1, m.norm2, m.fc1):
        assert mod.training == training
    assert m.__dict__.get("_eval_cache") is cache
    after = dict(list(m.named_parameters()) + list(m.named_buffers()))
    for k, (v, ver, val) in before.items():
        assert after[k] is v and v._version == ver and torch.equal(v.detach(), val), k
    assert res.counts.shape == cnt.shape == res_h.counts.shape == heads.shape
    # BatchNorm enters in inference form whatever the mode: over one fixed table, the lists taken with the head's modules
    # in this mode are those of the eval-mode logits
    with torch.no_grad():
        table = m._table_for_inference().detach().clone()
    sm = PG.StandIn(table, {k: getattr(m, k) for k in ("fc1", "norm1", "fc2", "norm2", "fc3")}, m.n_relations)
    sm.training = training
    got = L.predict_accepted_mlp(sm, heads, None, logit_threshold=thr, known=known)
    got_n = L.count_accepted_mlp(sm, heads, None, logit_threshold=thr, known=known)
    assert m.norm1.training == training
    m.eval()
    z = L.mlp_scores(sm, heads, every, logits=True).cpu().numpy()
    trip = set(zip(heads.cpu().tolist(), [0] * heads.numel(), tails.cpu().tolist()))
    elig = PA.eligibility(heads.cpu().tolist(), list(range(m.n_entities)), "tail", trip)
    ref = PA.accepted_lists(z, thr, np.arange(m.n_entities), elig)
    assert 0 < ref.rowptr[-1] < z.size
    PA.check_lists(got, ref, f"training={training}")
    assert torch.equal(got_n, got.counts)
