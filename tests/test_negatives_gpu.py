"""GPU: lkg_sample_negatives, lkg_relation_cardinality and lkg_answer_counts through literalkg_amd/negatives.py against the
reference of tests/negative_cases.py, WITHOUT tolerance, on the graph described there (257 entities, 5 relations; a hub, a
saturated head, a head without triples, an absent relation, 1-to-N and N-to-1 relations, duplicated triples), at G in
{1, 2, 33, 129} x K in {1, 3, 64, 257} (129 x 257 slots cross a 256-thread workgroup both ways).

The saturated head 256 is known with every OTHER entity, and a candidate equal to the anchor is not rejected: with every
entity a candidate its slots are flagged or hold 256 itself; with the pool of every entity but 256 they are all flagged and
hold try 63's candidate.  Both are checked."""
import numpy as np
import pytest
import torch

import invariance as inv
import negative_cases as C

pytestmark = pytest.mark.gpu
SEED = 12345


@pytest.fixture(scope="module")
def L(gpu_device):
    import __graft_entry__ as ge
    ge.build()
    import literalkg_amd
    return literalkg_amd


def _dev(arrays, dev):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


@pytest.fixture(scope="module")
def known(L, gpu_device):
    return L.KnownTriples(*_known_args(gpu_device))


def _known_args(dev, order=None, repeat=1):
    h, r, t = C.graph()
    order = np.arange(h.size) if order is None else order
    h, r, t = (np.tile(x[order], repeat) for x in (h, r, t))
    return (*_dev((h, r, t), dev), C.N_ENT, C.N_REL)


def _pool(kind, dev):
    p = C.pools(kind)
    return None if p is None else _dev(p, dev)


def _sampler(L, known, dev, corrupt, pool=None, any_relation=False, filtered=None):
    return L.NegativeSampler(C.N_ENT, known, corrupt=corrupt, pool=_pool(pool, dev), any_relation=any_relation,
                             filtered=filtered)


def _draw(sampler, pos, g, k, seed=SEED, group_offset=0, g0=0):
    b = sampler.sample(*(x[g0:g0 + g] for x in pos), k, seed=seed, group_offset=group_offset)
    assert b.neg.dtype == torch.int64 and b.head_side.dtype == torch.bool and b.unfiltered.dtype == torch.bool
    assert b.neg.shape == (g, k) and b.head_side.shape == (g,) and b.unfiltered.shape == (g, k)
    assert isinstance(b.n_unfiltered, int) and b.n_unfiltered == int(b.unfiltered.sum())
    return dict(neg=b.neg.cpu().numpy(), head_side=b.head_side.cpu().numpy(), unfiltered=b.unfiltered.cpu().numpy())


def _assert_same(got, want, what):
    for key in ("neg", "head_side", "unfiltered"):
        inv.same_bits(got[key], np.ascontiguousarray(want[key]), f"{what}: {key}")


@pytest.mark.parametrize("corrupt,pool,any_relation", C.CONFIGS)
def test_draw_equals_the_reference_entry_for_entry(L, gpu_device, known, corrupt, pool, any_relation):
    ref = C.reference(corrupt, pool, any_relation)
    pos = _dev(C.positives(), gpu_device)
    sampler = _sampler(L, known, gpu_device, corrupt, pool, any_relation)
    assert sampler.filtered is True
    for g in C.GS:
        for k in C.KS:
            got = _draw(sampler, pos, g, k)
            _assert_same(got, C.cut(ref, g, k), f"G {g} K {k}")
    assert C.violations(got, *C.positives(), C.pools(pool), True, any_relation) == 0            # (the 129 x 257 draw)
    # without the saturated head nothing is flagged -- the condition the host test shows the reference to meet
    clean_ref = C.reference(corrupt, pool, any_relation, saturated=False)
    b = sampler.sample(*_dev(C.positives(False), gpu_device), C.K_MAX, seed=SEED)
    assert b.n_unfiltered == 0 == int(clean_ref["unfiltered"].sum())
    inv.same_bits(b.neg.cpu().numpy(), clean_ref["neg"], "without the saturated head")
    for g, k in ((1, 1), (2, 64)):                                                              # (no saturated head below G = 6)
        assert sampler.sample(*(x[:g] for x in pos), k, seed=SEED).n_unfiltered == 0


@pytest.mark.parametrize("corrupt,with_known", [("tail", False), ("both", False), ("head", True), ("bernoulli", True)])
def test_unfiltered_draw_rejects_the_truth_alone(L, gpu_device, known, corrupt, with_known):
    pos = _dev(C.positives(), gpu_device)
    sampler = L.NegativeSampler(C.N_ENT, known if with_known else None, corrupt=corrupt, pool=_pool("pair", gpu_device),
                                filtered=False)
    ref = C.reference(corrupt, "pair", filtered=False, seed=1)
    for g, k in ((2, 3), (129, 257)):
        got = _draw(sampler, pos, g, k, seed=1)
        _assert_same(got, C.cut(ref, g, k), f"unfiltered G {g} K {k}")
    assert got["unfiltered"].sum() == 0
    assert C.violations(got, *C.positives(), C.pools("pair"), False) == 0


def test_other_seeds_and_a_far_group_offset(L, gpu_device, known):
    pos = _dev(C.positives(), gpu_device)
    h, r, t = C.positives()
    for seed, offset in ((1, 0), (2 ** 63 - 1, 3), (2 ** 64 - 1, 2 ** 40 + 5), (0, 2 ** 62)):
        for corrupt in ("both", "bernoulli"):
            want = C.sample(h[:33], r[:33], t[:33], 3, seed, offset, corrupt=corrupt, known=C.known_set(), pool=C.pools("pair"))
            got = _draw(_sampler(L, known, gpu_device, corrupt, "pair"), pos, 33, 3, seed=seed, group_offset=offset)
            _assert_same(got, want, f"seed {seed} offset {offset} {corrupt}")


def test_saturated_head_and_one_element_pool(L, gpu_device, known):
    pos = _dev(C.positives(), gpu_device)
    ref = C.reference("tail", "no_anchor")
    got = _draw(_sampler(L, known, gpu_device, "tail", "no_anchor"), pos, C.G_MAX, C.K_MAX)
    _assert_same(got, C.cut(ref, C.G_MAX, C.K_MAX), "the pool without the anchor")
    assert got["unfiltered"][[5, 70]].all() and got["unfiltered"].sum() == 2 * C.K_MAX          # all flagged: try 63's candidate
    assert (ref["tries"][[5, 70]] == C.MAX_TRIES).all()
    free = _draw(_sampler(L, known, gpu_device, "tail"), pos, C.G_MAX, 64)                      # every entity a candidate
    assert ((free["neg"][[5, 70]] == C.SATURATED) | free["unfiltered"][[5, 70]]).all() and free["unfiltered"][[5, 70]].any()
    h, r, t = C.positives()
    one = _draw(_sampler(L, known, gpu_device, "tail", "truth"), pos, 1, 9, seed=3, group_offset=5, g0=5)
    assert one["unfiltered"].all() and (one["neg"] == 7).all()                                  # a pool holding only the truth
    _assert_same(one, C.sample(h[5:6], r[5:6], t[5:6], 9, 3, 5, known=C.known_set(), pool=C.pools("truth")), "one-element pool")


@pytest.mark.parametrize("corrupt", ["tail", "bernoulli"])
def test_slots_and_groups_are_independent(L, gpu_device, known, corrupt):
    pos = _dev(C.positives(), gpu_device)
    sampler = _sampler(L, known, gpu_device, corrupt, "pair")
    whole = _draw(sampler, pos, C.G_MAX, C.K_MAX)
    for k in (1, 3, 64):                                # the first K' columns of a K-draw are the K'-draw
        _assert_same(_draw(sampler, pos, C.G_MAX, k), C.cut(whole, C.G_MAX, k), f"prefix {k}")
    for at in (1, 50, 128):                             # a batch cut at any point, the offset carried
        a, b = _draw(sampler, pos, at, 64), _draw(sampler, pos, C.G_MAX - at, 64, group_offset=at, g0=at)
        _assert_same({k_: np.concatenate([a[k_], b[k_]]) for k_ in a}, C.cut(whole, C.G_MAX, 64), f"cut at {at}")
    # a group gives the same row whatever other groups share its batch
    pick = torch.tensor([70, 3, 3, 128, 90], device=gpu_device)
    for i, p in enumerate(pick.tolist()):
        alone = _draw(sampler, pos, 1, 64, group_offset=p, g0=p)
        _assert_same(alone, C.cut(whole, 1, 64, p), f"group {p} alone")
        mixed = sampler.sample(*(x[pick] for x in pos), 64, seed=SEED, group_offset=p - i)      # position i has gid p
        inv.same_bits(mixed.neg[i].cpu().numpy(), whole["neg"][p, :64].copy(), f"group {p} among others")


def test_known_in_another_order_or_duplicated_gives_the_same_bits(L, gpu_device, known):
    pos = _dev(C.positives(), gpu_device)
    want = _draw(_sampler(L, known, gpu_device, "bernoulli", "pair"), pos, C.G_MAX, 64)
    n = C.graph()[0].size
    for order, repeat in ((np.arange(n)[::-1], 1), (np.random.default_rng(5).permutation(n), 1), (None, 3)):
        other = L.KnownTriples(*_known_args(gpu_device, order, repeat))
        _assert_same(_draw(_sampler(L, other, gpu_device, "bernoulli", "pair"), pos, C.G_MAX, 64), want, "rebuilt known")
        card, base = L.relation_cardinalities(other), L.relation_cardinalities(known)
        for name in ("triples", "heads", "tails"):
            inv.same_bits(getattr(card, name), getattr(base, name), name)


def test_poisoned_scratch_and_a_side_stream_give_the_same_bits(L, gpu_device, known):
    pos = _dev(C.positives(), gpu_device)

    def run():
        sampler = _sampler(L, known, gpu_device, "bernoulli", "pair")
        b = sampler.sample(*pos, 64, seed=SEED, group_offset=9)
        card = L.relation_cardinalities(known)
        counts = L.answer_counts(known, *pos)
        w = L.subsampling_weights(known, *pos)
        return [b.neg, b.head_side, b.unfiltered, card.triples, card.heads, card.tails, *counts, w], b.n_unfiltered
    want, n_want = run()
    for byte in (0xFF, 0x7F):
        with inv.poisoned(byte):
            got, n_got = run()
        with inv.side_stream(), inv.poisoned(byte):
            side, n_side = run()
        assert n_got == n_side == n_want
        for i, (a, b, c) in enumerate(zip(got, side, want)):
            inv.same_bits(a, c, f"poisoned 0x{byte:02X}: output {i}")
            inv.same_bits(b, c, f"side stream, poisoned 0x{byte:02X}: output {i}")


def test_cardinalities_answer_counts_and_weights_equal_the_double_loops(L, gpu_device, known):
    kh, kr, kt = C.graph()
    card = L.relation_cardinalities(known)
    want = C.cardinalities(kh, kr, kt)
    for got, w in zip((card.triples, card.heads, card.tails), want):
        assert got.dtype == torch.int64 and got.is_cuda
        inv.same_bits(got.cpu().numpy(), w, "cardinality")
    tph, hpt = card.tails_per_head.cpu().numpy(), card.heads_per_tail.cpu().numpy()
    assert tph.dtype == np.float64 and np.isnan(tph[4]) and np.isnan(hpt[4])
    with np.errstate(invalid="ignore"):
        inv.same_bits(tph[:4], (want[0] / want[1])[:4], "tails per head")
        inv.same_bits(hpt[:4], (want[0] / want[2])[:4], "heads per tail")
    h, r, t = C.positives()
    pos = _dev((h, r, t), gpu_device)
    for any_relation in (False, True):
        got = L.answer_counts(known, *pos, any_relation=any_relation)
        for a, w in zip(got, C.answer_counts(kh, kr, kt, h, r, t, any_relation)):
            inv.same_bits(a.cpu().numpy(), w, f"answer counts, any_relation {any_relation}")
    n_tails, n_heads = C.answer_counts(kh, kr, kt, h, r, t)
    assert n_tails[0] == 200 and n_tails[5] == 256 and n_tails[2] == 0 and n_tails[4] == 0
    for start in (4.0, 1.0, 0.5):
        w = L.subsampling_weights(known, *pos, start=start)
        assert w.dtype == torch.float32
        inv.same_bits(w.cpu().numpy(), C.subsampling_weights(n_tails, n_heads, start), f"weights, start {start}")
    for one in (1, 2):                                   # G = 1 and 2
        inv.same_bits(L.answer_counts(known, *(x[:one] for x in pos))[0].cpu().numpy(), n_tails[:one].copy(), "short")


def test_cardinalities_of_a_hub_row_of_ten_thousand_entries_and_the_last_relation(L, gpu_device):
    """(checked against numpy's unique: the double loops would take minutes here)"""
    rng = np.random.default_rng(11)
    n, n_rel, hub = 12000, 4096, 11999
    rels = np.asarray([0, 31, 32, 63, 64, 2047, 4095])
    h = np.concatenate([np.full(10000, hub), rng.integers(0, n, 6000), np.full(300, hub)])
    t = np.concatenate([np.arange(10000), rng.integers(0, n, 6000), np.full(300, 17)])          # 300 raw edges in one entry
    r = rels[rng.integers(0, rels.size, h.size)]
    known = L.KnownTriples(*_dev((h, r, t), gpu_device), n, n_rel)
    card = L.relation_cardinalities(known)
    for got, cols in ((card.triples, (h, t)), (card.heads, (h,)), (card.tails, (t,))):
        uniq = np.unique(np.stack((r,) + cols, 1), axis=0)
        inv.same_bits(got.cpu().numpy(), np.bincount(uniq[:, 0], minlength=n_rel).astype(np.int64), "hub cardinality")
    with pytest.raises(ValueError, match="at most 4096 relations"):
        L.relation_cardinalities(L.KnownTriples(*_dev((h[:5], r[:5], t[:5]), gpu_device), n, 4097))


def test_ids_out_of_range_are_refused(L, gpu_device, known):
    pos = _dev(C.positives(), gpu_device)
    sampler = _sampler(L, known, gpu_device, "both")
    for i, bump in ((0, C.N_ENT), (2, C.N_ENT), (1, C.N_REL), (0, -300)):
        bad = [x[:33].clone() for x in pos]
        bad[i][7] += bump
        with pytest.raises(IndexError, match="outside"):
            sampler.sample(*bad, 3, seed=1)
        with pytest.raises(IndexError, match="outside"):
            L.answer_counts(known, *bad)
    with pytest.raises(ValueError, match="known triples over 257 entities, the sampler over 300"):
        L.NegativeSampler(300, known)
    with pytest.raises(IndexError, match="the candidate pool has 1 entity id"):
        L.NegativeSampler(C.N_ENT, known, pool=torch.tensor([0, 257], device=gpu_device))
    empty = sampler.sample(*(x[:0] for x in pos), 3, seed=1)
    assert empty.neg.shape == (0, 3) and empty.head_side.shape == (0,) and empty.n_unfiltered == 0
    assert isinstance(sampler.sample(*(x[:2] for x in pos), 3).n_unfiltered, int)              # seed=None: ops.new_seed()
