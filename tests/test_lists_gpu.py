"""GPU: scores and filtered ranks against per-query candidate lists (literalkg_amd/lists.py, lkg_lists.hip).

1. score_lists has the BITS of score_triples for every non-empty slot, NaN in the empty ones: both sides, reported and
   kernel scores, every B x M of the tile edges;  2. on small-integer tables the scores and the counts equal an int64
   computation;  3. rank_in_lists equals list_cases.counts on the device's own kernel scores, with and without a filter,
   'dot' under any relation, a NaN candidate and a NaN truth;  4. with lists = arange(N) the counts are rank_triples';
   5. nothing depends on the batch size, the order of queries or slots, the projection route, the scratch or the stream;
   6. evaluate_list_ranking on the golden models;  7. 64-bit addressing of the table's rows.

Everything is exact: no tolerance appears.  The launch does not cap its grid (one workgroup per query and slice of 256
slots), so no workgroup makes a second trip over queries; M = 500 gives a workgroup four trips over its slice, the last
one partly filled."""
import pytest
import torch

import invariance as V
import list_cases as LC
from test_topk_gpu import StandIn, _golden_model, random_model
from test_triples_gpu import SHAPES, Model, bits, rel_choices

pytestmark = pytest.mark.gpu

BS = [1, 2, 5, 64, 65, 257]
MS = [1, 15, 16, 17, 64, 65, 500]
B_MAX, M_MAX = BS[-1], MS[-1]
ROW_EMPTY, ROW_SAME = 3, 4                    # one all-empty row, one row whose every slot is the same id
SIDES = ("tail", "head")


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


def ends(side, h, t):
    """(query entities, truths) of a side"""
    return (h, t) if side == "tail" else (t, h)


def flat_scores(L, model, side, q, r, lists, kernel):
    """float32[B, M]: score_triples on the flattened non-empty slots, NaN elsewhere (r None: 'dot', any relation id)"""
    full = lists >= 0
    i = torch.nonzero(full)[:, 0]
    qq, cc = q[i], lists[full]
    rr = r[i] if r is not None else torch.zeros_like(qq)
    hh, tt = (qq, cc) if side == "tail" else (cc, qq)
    out = torch.full(lists.shape, float("nan"), dtype=torch.float32, device=lists.device)
    out[full] = L.score_triples(model, hh, rr, tt, side=side, kernel_scores=kernel)
    return out


_CASES = {}


def case(L, scoring, n, k, c, n_rel, dev):
    """One model, B_MAX triples and their B_MAX x M_MAX lists per shape, shared by the tests and never changed: about a
    tenth of the slots empty, the truth of some queries inside their own list, rows ROW_EMPTY and ROW_SAME."""
    key = (scoring, n, k, c, n_rel)
    if key not in _CASES:
        gen = torch.Generator().manual_seed(77 + 1000 * len(scoring) + n + k + c + n_rel)
        m = random_model(gen, scoring, n, k, c, n_rel, dev)
        model = Model(m.T, m.relation_embed.weight, m.gat_trans_M, scoring)
        rels = torch.tensor(rel_choices(n_rel))
        h = torch.randint(0, n, (B_MAX,), generator=gen)
        t = torch.randint(0, n, (B_MAX,), generator=gen)
        r = rels[torch.randint(0, rels.numel(), (B_MAX,), generator=gen)]
        lists = torch.randint(0, n, (B_MAX, M_MAX), generator=gen)
        lists[torch.rand(B_MAX, M_MAX, generator=gen) < 0.1] = -1
        rows = torch.arange(B_MAX)
        lists[rows % 7 == 0, 0] = t[rows % 7 == 0]               # the truth of either side inside its own list
        lists[rows % 7 == 1, 1] = h[rows % 7 == 1]
        lists[rows % 7 == 2, 20] = t[rows % 7 == 2]
        lists[ROW_EMPTY] = -1
        lists[ROW_SAME] = int(lists[ROW_SAME + 1, 2].clamp(min=0))
        _CASES[key] = dict(model=model, h=h.to(dev), r=r.to(dev), t=t.to(dev), lists=lists.to(dev), gen=gen, ref={}, known={})
    return _CASES[key]


def reference(L, cs, side, kernel):
    """float32[B_MAX, M_MAX] of flat_scores, made once per (side, kernel)"""
    if (side, kernel) not in cs["ref"]:
        q, _ = ends(side, cs["h"], cs["t"])
        cs["ref"][side, kernel] = flat_scores(L, cs["model"], side, q, cs["r"], cs["lists"], kernel)
    return cs["ref"][side, kernel]


def known_for(L, cs, side):
    """(KnownTriples, the same triples as a Python set) that hit listed slots of every third query, the truth itself, a
    slot under another relation only, and hold duplicates"""
    if side not in cs["known"]:
        model, lists = cs["model"], cs["lists"].cpu()
        q, tru = (x.cpu() for x in ends(side, cs["h"], cs["t"]))
        r = cs["r"].cpu()
        n_rel = model.n_relations
        trip = []
        for i in range(0, B_MAX, 3):
            for j in (0, 1, 5, 16, 63, 64, 255, 256, 499):
                c = int(lists[i, j])
                if c >= 0:
                    trip.append((int(q[i]), int(r[i]), c))
            c = int(lists[i, 7])
            if c >= 0:
                trip.append((int(q[i]), (int(r[i]) + 1) % n_rel, c))          # under another relation (n_rel 1: the same)
            trip.append((int(q[i]), int(r[i]), int(tru[i])))                  # the truth itself: never compared anyway
        trip += trip[:40]                                                     # duplicates
        a, rr, b = (torch.tensor(x, device=cs["lists"].device) for x in zip(*trip))
        hh, tt = (a, b) if side == "tail" else (b, a)
        known = L.KnownTriples(hh, rr, tt, model.n_entities, n_rel)
        cs["known"][side] = (known, set(zip(hh.tolist(), rr.tolist(), tt.tolist())))
    return cs["known"][side]


# ----------------------------------------------------------------------------- 1. the bits of score_triples
@pytest.mark.parametrize("n_rel", [1, 5])
@pytest.mark.parametrize("scoring,n,k,c", SHAPES)
def test_bits_of_score_triples(L, gpu_device, scoring, n, k, c, n_rel):
    cs = case(L, scoring, n, k, c, n_rel, gpu_device)
    model, r, lists = cs["model"], cs["r"], cs["lists"]
    for side in SIDES:
        q, _ = ends(side, cs["h"], cs["t"])
        for kernel in (False, True):
            want = reference(L, cs, side, kernel)
            for b in BS:
                for m in MS:
                    got = L.score_lists(model, q[:b], r[:b], lists[:b, :m], side=side, kernel_scores=kernel)
                    assert got.shape == (b, m) and got.dtype == torch.float32
                    full = lists[:b, :m] >= 0
                    assert torch.equal(bits(got)[full], bits(want[:b, :m])[full]), (side, kernel, b, m)
                    assert bool(torch.isnan(got[~full]).all()), (side, kernel, b, m)
    assert bool(torch.isnan(got[ROW_EMPTY]).all()) and int(torch.unique(bits(got[ROW_SAME])).numel()) == 1
    assert not bool(torch.isnan(want[lists >= 0]).any())
    if scoring == "dot":                                                      # r may be None, as elsewhere
        got = L.score_lists(model, q, None, lists, side=side)
        assert torch.equal(bits(got)[lists >= 0], bits(reference(L, cs, side, False))[lists >= 0])


# ----------------------------------------------------------------------------- 2. exact int64
@pytest.mark.parametrize("k", [37, 300])
@pytest.mark.parametrize("scoring", ["transe", "dot"])
def test_exact_integer_tables(L, gpu_device, scoring, k):
    """Entries in [-3, 3]: every product, partial sum, squared norm and the final fma stay below 2^24 in magnitude and are
    exact in float32, so the scores and the counts have one right value, computed in int64."""
    gen = torch.Generator().manual_seed(5 + k + len(scoring))
    n, n_rel, b, m = 200, 3, 65, 130
    table = torch.randint(-3, 4, (n, k), generator=gen)
    relemb = torch.randint(-3, 4, (n_rel, k), generator=gen)
    table[1] = table[0]                                                       # equal rows: ties by construction ...
    table[n // 2:] = table[n // 2:] // 3                                      # ... and many more among rows of -1, 0, 1
    h, t = torch.randint(0, n, (b,), generator=gen), torch.randint(0, n, (b,), generator=gen)
    r = torch.randint(0, n_rel, (b,), generator=gen)
    lists = torch.randint(0, n, (b, m), generator=gen)
    lists[torch.rand(b, m, generator=gen) < 0.1] = -1
    lists[:, 0] = t
    lists[:, 1], lists[:, 2] = 0, 1
    t[::4], h[1::4] = 0, 0                                                    # a truth in row 0 ties with the listed row 1
    model = StandIn(table.float().to(gpu_device), relemb.float().to(gpu_device), None, scoring)
    for side in SIDES:
        qid, tru = ends(side, h, t)
        q = table[qid] + (0 if scoring == "dot" else (1 if side == "tail" else -1) * relemb[r])      # int64
        qn, pn = (q * q).sum(1), (table * table).sum(1)
        dots = (q[:, None, :] * table[lists.clamp(min=0)]).sum(2)
        assert int(qn.max()) + int(pn.max()) + 2 * int((q.abs().sum(1).max()) * 3) < 2 ** 24         # the bound, on the CPU
        if scoring == "dot":
            kern, rep = -2 * dots, dots
            kern_t = -2 * (q * table[tru]).sum(1)
        else:
            kern = pn[lists.clamp(min=0)] - 2 * dots
            rep = qn[:, None] + kern
            kern_t = pn[tru] - 2 * (q * table[tru]).sum(1)
        dev = [x.to(gpu_device) for x in (qid, r, lists, h, t)]
        full = lists >= 0
        for kernel, want in ((False, rep), (True, kern)):
            got = L.score_lists(model, dev[0], dev[1], dev[2], side=side, kernel_scores=kernel).cpu()
            assert torch.equal(got[full].double(), want[full].double()), (side, kernel)
            assert bool(torch.isnan(got[~full]).all())
        keep = LC.keep_mask(lists, tru)
        ref = LC.counts(kern, kern_t, keep)
        assert int(ref[1].sum()) >= b // 4 and int(ref[0].sum()) > 0                                  # ties are plentiful
        res = L.rank_in_lists(model, dev[3], dev[1], dev[4], dev[2], side=side)
        LC.check_ranks(res, ref, f"{scoring} k {k} {side}")
        assert res.side == side


# ----------------------------------------------------------------------------- 3. counts on the device's own scores
@pytest.mark.parametrize("n_rel", [1, 5])
@pytest.mark.parametrize("scoring,n,k,c", SHAPES)
def test_counts_on_the_devices_own_scores(L, gpu_device, scoring, n, k, c, n_rel):
    cs = case(L, scoring, n, k, c, n_rel, gpu_device)
    model, h, r, t, lists = cs["model"], cs["h"], cs["r"], cs["t"], cs["lists"]
    for side in SIDES:
        q, tru = ends(side, h, t)
        scores = L.score_lists(model, q, r, lists, side=side, kernel_scores=True)
        assert torch.equal(bits(scores)[lists >= 0], bits(reference(L, cs, side, True))[lists >= 0])
        truth_scores = L.score_triples(model, h, r, t, side=side, kernel_scores=True)
        known, triples = known_for(L, cs, side)
        for kn, tr in ((None, None), (known, triples)):
            keep = LC.keep_mask(lists, tru, q, r, tr, side)
            for b, m in ((B_MAX, M_MAX), (65, 17), (5, 257)):
                ref = LC.counts(scores[:b, :m], truth_scores[:b], keep[:b, :m])
                res = L.rank_in_lists(model, h[:b], r[:b], t[:b], lists[:b, :m], side=side, known=kn)
                LC.check_ranks(res, ref, f"{side} known {kn is not None} {b} x {m}")
        assert int(keep.sum()) < int(LC.keep_mask(lists, tru).sum())          # the filter dropped listed slots
        assert int(res.kept[ROW_EMPTY]) == 0 == int(res.better[ROW_EMPTY])


def test_dot_under_any_relation_with_a_nan_candidate_and_a_nan_truth(L, gpu_device):
    scoring, n, k, c = SHAPES[3]
    cs = case(L, scoring, n, k, c, 5, gpu_device)
    table = cs["model"].T.clone()
    bad = 17
    table[bad] = float("nan")
    model = Model(table, cs["model"].relation_embed.weight, None, scoring)
    h, t, lists = cs["h"].clone(), cs["t"].clone(), cs["lists"]
    h[h == bad], t[t == bad] = 0, 0                                           # no NaN query; then ONE NaN truth per side
    h[9], t[5] = bad, bad
    assert int((lists == bad).sum()) > B_MAX                                  # NaN candidates in most lists
    for side in SIDES:
        q, tru = ends(side, h, t)
        nan_truth, nan_query = (5, 9) if side == "tail" else (9, 5)
        scores = L.score_lists(model, q, None, lists, side=side, kernel_scores=True)
        truth_scores = L.score_triples(model, h, torch.zeros_like(h), t, side=side, kernel_scores=True)
        assert bool(torch.isnan(truth_scores[nan_truth])) and bool(torch.isnan(scores[lists == bad]).all())
        _, triples = known_for(L, cs, side)
        a, rr, b = (torch.tensor(x, device=gpu_device) for x in zip(*sorted(triples)))
        known = L.KnownTriples(a, rr, b, n, 5)
        for kn, tr in ((None, None), (known, triples)):
            keep = LC.keep_mask(lists, tru, q, None, tr, side)                # r None: known under any relation
            ref = LC.counts(scores, truth_scores, keep)
            res = L.rank_in_lists(model, h, None, t, lists, side=side, known=kn)
            LC.check_ranks(res, ref, f"dot {side} known {kn is not None}")
            assert int(res.better[nan_truth]) == 0 == int(res.equal[nan_truth]) and int(res.kept[nan_truth]) > 0
            assert int(res.better[nan_query]) == 0 == int(res.equal[nan_query])   # every score of a NaN query is NaN
        under_r = LC.keep_mask(lists, tru, q, cs["r"], triples, side)
        assert int(keep.sum()) < int(under_r.sum())                           # any-relation drops more than under r[i]


# ----------------------------------------------------------------------------- 4. agreement with rank_triples
@pytest.mark.parametrize("shape", SHAPES[:2])
def test_whole_table_lists_give_rank_triples_counts(L, gpu_device, shape):
    scoring, n, k, c = shape
    cs = case(L, scoring, n, k, c, 5, gpu_device)
    model, b = cs["model"], 65
    h, r, t = cs["h"][:b], cs["r"][:b], cs["t"][:b]
    lists = torch.arange(n, device=gpu_device).expand(b, n)
    gen = torch.Generator().manual_seed(n)
    pick = torch.randint(0, b, (400,), generator=gen).to(gpu_device)
    other = torch.randint(0, n, (400,), generator=gen).to(gpu_device)
    kh, kr, kt = torch.cat((h[pick[:200]], other[200:], h)), torch.cat((r[pick[:200]], r[pick[200:]], r)), \
        torch.cat((other[:200], t[pick[200:]], t))
    known = L.KnownTriples(kh, kr, kt, n, 5)
    triples = set(zip(kh.tolist(), kr.tolist(), kt.tolist()))
    for side in SIDES:
        q, tru = ends(side, h, t)
        for kn, tr in ((None, None), (known, triples)):
            want = L.ranking.rank_triples(model, h, r, t, side=side, known=kn)
            res = L.rank_in_lists(model, h, r, t, lists, side=side, known=kn)
            assert torch.equal(res.better, want.better) and torch.equal(res.equal, want.equal), (side, kn is not None)
            assert torch.equal(res.rank, want.rank)
            dropped = (~LC.keep_mask(lists, tru, q, r, tr, side)).sum(1) - 1          # (the truth itself is not "dropped")
            assert torch.equal(res.kept.cpu(), n - 1 - dropped), (side, kn is not None)
        assert int(dropped.sum()) > 0


# ----------------------------------------------------------------------------- 5. invariance
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]])
def test_invariance(L, T, gpu_device, monkeypatch, shape):
    scoring, n, k, c = shape
    cs = case(L, scoring, n, k, c, 5, gpu_device)
    model, b, m = cs["model"], 65, 65
    h, r, t, lists = cs["h"][:b], cs["r"][:b], cs["t"][:b], cs["lists"][:b, :m].contiguous()
    gen = cs["gen"]
    for side in SIDES:
        q, _ = ends(side, h, t)
        known, _ = known_for(L, cs, side)

        def run(hh=h, rr=r, tt=t, ll=lists, **kw):
            qq, _ = ends(side, hh, tt)
            return (L.score_lists(model, qq, rr, ll, side=side, **kw),
                    L.rank_in_lists(model, hh, rr, tt, ll, side=side, known=known, **kw))

        def same(got, want, what, rows=None, cols=None):
            sc, res = got
            wsc = want[0] if rows is None else want[0][rows]
            wsc = wsc if cols is None else torch.gather(wsc, 1, cols)
            assert V.same_bits(sc, wsc, f"{side} {what}: scores")
            for name in ("better", "equal", "kept", "rank"):
                w = getattr(want[1], name)
                assert V.same_bits(getattr(res, name), w if rows is None else w[rows], f"{side} {what}: {name}")

        base = run()
        for bs in (1, 7, None):
            same(run(batch_size=bs), base, f"batch_size {bs}")
        perm = torch.randperm(b, generator=gen).to(gpu_device)
        same(run(h[perm], r[perm], t[perm], lists[perm]), base, "permuted queries", rows=perm)
        cols = torch.stack([torch.randperm(m, generator=gen) for _ in range(b)]).to(gpu_device)
        same(run(ll=torch.gather(lists, 1, cols)), base, "permuted slots", cols=cols)
        twice = torch.cat((torch.arange(b), torch.arange(b - 1, -1, -1))).to(gpu_device)
        same(run(h[twice], r[twice], t[twice], lists[twice]), base, "duplicated queries", rows=twice)
        for route in ("full", "distinct"):
            monkeypatch.setattr(T, "PROJECT", route)
            same(run(), base, f"projection {route}")
        monkeypatch.setattr(T, "PROJECT", None)
        with V.poisoned(0xFF):
            got = run()
        same(got, base, "poisoned scratch")
        with V.side_stream():
            with V.poisoned(0x7F):
                got = run()
        same(got, base, "side stream")


# ----------------------------------------------------------------------------- 6. golden models
@pytest.mark.parametrize("name,scoring", [("encoder_gcn_l2_gatenum", "transr"), ("transe_gcn_l1", "transe")])
def test_golden_model(L, gpu_device, name, scoring):
    model, gd = _golden_model(L, name, gpu_device, scoring)
    model.eval()
    h, r, t = (torch.from_numpy(gd[x]).to(gpu_device) for x in ("h", "r", "t"))
    n, n_rel = model.n_entities, model.n_relations
    known = L.KnownTriples(h, r, t, n, n_rel)
    triples = set(zip(h.tolist(), r.tolist(), t.tolist()))
    th, tr, tt = h[:200], r[:200], t[:200]
    neg = {"tail": L.NegativeSampler(n, known, corrupt="tail").sample(th, tr, tt, k=50, seed=7),
           "head": L.NegativeSampler(n, known, corrupt="head").sample(th, tr, tt, k=50, seed=7)}
    assert not bool(neg["tail"].head_side.any()) and bool(neg["head"].head_side.all())
    params = {k_: v.detach().clone() for k_, v in model.state_dict().items()}
    by_side = {}
    for side in SIDES:
        q, tru = ends(side, th, tt)
        lists = neg[side].neg                                                 # a NegativeBatch.neg, as it is
        scores = model.score_lists(q, tr, lists, side=side, kernel_scores=True)
        assert torch.equal(bits(scores), bits(flat_scores(L, model, side, q, tr, lists, True)))
        assert torch.equal(bits(model.score_lists(q, tr, lists, side=side)), bits(flat_scores(L, model, side, q, tr, lists, False)))
        truth_scores = model.score_triples(th, tr, tt, side=side, kernel_scores=True)
        ref = LC.counts(scores, truth_scores, LC.keep_mask(lists, tru, q, tr, triples, side))
        LC.check_ranks(model.rank_in_lists(th, tr, tt, lists, side=side, known=known), ref, f"{name} {side}")
        by_side[side] = ref[:2]
    model.train()
    got = model.evaluate_list_ranking(th, tr, tt, tail_lists=neg["tail"].neg, head_lists=neg["head"].neg, known=known)
    assert model.training                                                     # the mode is restored
    model.eval()
    assert got == LC.metrics(by_side) and got["n"] == 400 and got["tail"]["n"] == 200
    one = L.evaluate_list_ranking(model, th, tr, tt, head_lists=neg["head"].neg, known=known, ks=(1, 5))
    assert one == LC.metrics({"head": by_side["head"]}, ks=(1, 5)) and "tail" not in one and not model.training
    for k_, v in model.state_dict().items():
        v0 = params[k_]
        if v.is_sparse:
            v, v0 = v.coalesce().values(), v0.coalesce().values()
        assert torch.equal(v, v0), k_
    # an id past the entities raises, a negative one is an empty slot
    far = neg["tail"].neg.clone()
    far[3, 4] = n
    with pytest.raises(IndexError):
        model.rank_in_lists(th, tr, tt, far, known=known)
    with pytest.raises(IndexError):
        model.score_lists(th, tr, far)


# ----------------------------------------------------------------------------- 7. 64-bit addressing
@pytest.mark.parametrize("extra", [0, 1])
def test_rows_past_2_31_and_2_32_elements(L, gpu_device, extra):
    """A 33-row table laid over 2^32 elements by its row stride (2^27, or 2^27 + 1: the scalar load path): rows 16 .. 31
    start in [2^31, 2^32), row 32 at or past 2^32.  Every other cell is 0xFF (NaN), so a row offset that went through 32
    bits reads NaN or another row; the compact twin gives the bits and the counts to meet."""
    n, k, n_rel, b, m = 33, 37, 3, 9, 40
    ld = (1 << 27) + extra
    gen = torch.Generator().manual_seed(31 + extra)
    values = torch.randn(n, k, generator=gen).to(gpu_device)
    relemb = (torch.randn(n_rel, k, generator=gen) * 0.3).to(gpu_device)
    store = torch.empty((n - 1) * ld + k, dtype=torch.float32, device=gpu_device)
    store.view(torch.int32).fill_(-1)
    wide = torch.as_strided(store, (n, k), (ld, 1))
    wide.copy_(values)
    assert wide.stride(0) * 16 >= 2 ** 31 and wide.stride(0) * 32 >= 2 ** 32 and wide.data_ptr() % 16 == 0
    h = torch.randint(16, n, (b,), generator=gen).to(gpu_device)
    t = torch.randint(16, n, (b,), generator=gen).to(gpu_device)
    h[0], t[1] = 32, 32
    r = torch.randint(0, n_rel, (b,), generator=gen).to(gpu_device)
    lists = torch.randint(16, n, (b, m), generator=gen)
    lists[torch.rand(b, m, generator=gen) < 0.1] = -1
    lists[:, 3] = 32
    lists = lists.to(gpu_device)
    for scoring in ("transe", "dot"):
        twin, far = StandIn(values, relemb, None, scoring), StandIn(wide, relemb, None, scoring)
        for side in SIDES:
            q, _ = ends(side, h, t)
            for kernel in (False, True):
                want = L.score_lists(twin, q, r, lists, side=side, kernel_scores=kernel)
                got = L.score_lists(far, q, r, lists, side=side, kernel_scores=kernel)
                assert V.same_bits(got, want, f"{scoring} {side} kernel {kernel}")
                assert not bool(torch.isnan(got[lists >= 0]).any())
            want, got = (L.rank_in_lists(x, h, r, t, lists, side=side) for x in (twin, far))
            for name in ("better", "equal", "kept"):
                assert V.same_bits(getattr(got, name), getattr(want, name), f"{scoring} {side} {name}")
            assert int(got.better.sum()) > 0
    assert V.same_bits(wide, values, "the table carries the bits it was given")
    del wide, store
    torch.cuda.empty_cache()
