"""The reference of the negative sampler (lkg_negatives.hip; literalkg_amd/negatives.py), the graph and the cases shared by
test_negatives_host.py and test_negatives_gpu.py.  No GPU, no library.

The stream is restated in numpy uint64 (arithmetic mod 2^64):

    key(seed, gid)      = mix64(seed ^ (0xD1B54A32D192ED03 * (gid + 1)))          gid = group_offset + g
    value(seed, gid, c) = mix64(key + 0x9E3779B97F4A7C15 * c)

counter 0 decides the side, counter 1 + j * MAX_TRIES + i is try i of slot j.  Rejection is a lookup in a Python SET of the
known triples; cardinalities and answer counts are double loops over the triple list.  ``fault=`` plants the mistakes the
checks have to catch.

The graph: 257 entities, 5 relations.  Relation 4 is absent; relation 2 is 1-to-N (heads 10 and 11), relation 3 N-to-1 (tails
12 and 13); head 0 is a hub with the 200 tails 1 .. 200 under relation 0 (57 candidates left: 0 and 201 .. 256); head 256 is
saturated, known with every OTHER entity under relation 1; entity 250 is never a head; ids 0 and 256 are in use; thirty
triples are listed twice.
"""
import functools

import numpy as np

MAX_TRIES = 64
N_ENT, N_REL = 257, 5
CORRUPT = ("tail", "head", "both", "bernoulli")
GS, KS = (1, 2, 33, 129), (1, 3, 64, 257)
G_MAX, K_MAX = 129, 257
SEEDS = (1, 12345, 2 ** 63 - 1)
HUB, SATURATED, NO_TRIPLES = 0, 256, 250
FAULTS = ("wrong_side_structure", "relation_ignored", "truth_not_rejected", "offset_dropped", "shared_slot0",
          "bernoulli_inverted")

_M1, _M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
_GROUP, _STEP = np.uint64(0xD1B54A32D192ED03), np.uint64(0x9E3779B97F4A7C15)


def mix64(z):
    """splitmix64's finaliser on a uint64 array"""
    z = np.asarray(z, dtype=np.uint64)
    z = (z ^ (z >> np.uint64(30))) * _M1
    z = (z ^ (z >> np.uint64(27))) * _M2
    return z ^ (z >> np.uint64(31))


def keys(seed, gids):
    return mix64(np.uint64(seed) ^ (_GROUP * (np.asarray(gids, dtype=np.uint64) + np.uint64(1))))


def values(key, counters):
    return mix64(np.uint64(key) + _STEP * np.asarray(counters, dtype=np.uint64))


def mix64_int(z):
    """the same in Python integers (the cross-check of the numpy form)"""
    m = (1 << 64) - 1
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def value_int(seed, gid, c):
    m = (1 << 64) - 1
    key = mix64_int(seed ^ ((0xD1B54A32D192ED03 * (gid + 1)) & m))
    return mix64_int((key + 0x9E3779B97F4A7C15 * c) & m)


# ----------------------------------------------------------------------------- the graph
@functools.lru_cache(maxsize=None)
def graph():
    """(h, r, t) int64 arrays of the known triples, duplicates included, in a shuffled order"""
    tr = [(HUB, 0, t) for t in range(1, 201)]
    tr += [(SATURATED, 1, t) for t in range(0, 256)]
    tr += [(10, 2, t) for t in range(20, 61)] + [(11, 2, t) for t in range(61, 91)]              # 1-to-N
    tr += [(h, 3, 12) for h in range(100, 161)] + [(h, 3, 13) for h in range(161, 191)]          # N-to-1
    rng = np.random.default_rng(0)
    for _ in range(120):                                # scattered triples of relations 0 and 1 among the other entities
        h, t = (int(x) for x in rng.integers(14, 250, 2))
        tr.append((h, int(rng.integers(0, 2)), t))
    tr += [(40, 0, 41), (40, 1, 41), (40, 3, 41)]       # one pair under three relations
    tr += [tr[int(i)] for i in rng.integers(0, len(tr), 30)]                                     # duplicates
    tr = [tr[int(i)] for i in rng.permutation(len(tr))]
    a = np.asarray(tr, dtype=np.int64)
    assert NO_TRIPLES not in a[:, 0] and 4 not in a[:, 1] and a.min() == 0 and a.max() == 256
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()


@functools.lru_cache(maxsize=None)
def known_set():
    h, r, t = graph()
    return frozenset(zip(h.tolist(), r.tolist(), t.tolist()))


@functools.lru_cache(maxsize=None)
def positives(saturated=True):
    """(h, r, t) of the G_MAX positives the cases draw for; the first G of them are the case of G groups.  Position 0 is a
    hub triple, 1 an N-to-1 triple, 2 an unknown triple of the head without triples, 3 a 1-to-N triple, 4 a triple of the
    absent relation, 5 and 70 triples of the saturated head (saturated=False: replaced by hub triples), the rest known
    triples."""
    h, r, t = graph()
    rng = np.random.default_rng(1)
    pick = rng.integers(0, h.size, G_MAX)
    p = [(int(h[i]), int(r[i]), int(t[i])) for i in pick]
    p = [x if x[0] != SATURATED else (HUB, 0, 1 + i) for i, x in enumerate(p)]
    p[0], p[1], p[2], p[3], p[4] = (HUB, 0, 1), (100, 3, 12), (NO_TRIPLES, 0, 5), (10, 2, 20), (5, 4, 6)
    p[6], p[7] = (0, 0, 256), (12, 0, 256)              # unknown triples on the ids 0 and 256
    if saturated:
        p[5], p[70] = (SATURATED, 1, 7), (SATURATED, 1, 255)
    a = np.asarray(p, dtype=np.int64)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()


def pools(kind):
    """None, or the (tail_pool, head_pool) of a kind: 'pair' = every entity in descending order with 201 .. 256 twice (a
    pool with duplicates) and the even ids (a type constraint); 'truth' = the one-element pool [7] (the truth of the
    saturated positive at position 5)."""
    if kind is None:
        return None
    if kind == "pair":
        return (np.concatenate([np.arange(256, -1, -1), np.arange(201, 257)]).astype(np.int64),
                np.arange(0, 257, 2, dtype=np.int64))
    if kind == "no_anchor":                             # every entity but the saturated head itself
        return (np.arange(0, 256, dtype=np.int64),) * 2
    assert kind == "truth"
    return (np.asarray([7], dtype=np.int64),) * 2


# ----------------------------------------------------------------------------- cardinalities and answer counts
def cardinalities(h, r, t, n_rel=N_REL):
    """(T_r, H_r, Tl_r) as int64[n_rel]: double loops over the triple list"""
    out = np.zeros((3, n_rel), dtype=np.int64)
    for q in range(n_rel):
        triples, heads, tails = set(), set(), set()
        for a, b, c in zip(h.tolist(), r.tolist(), t.tolist()):
            if b == q:
                triples.add((a, c))
                heads.add(a)
                tails.add(c)
        out[:, q] = len(triples), len(heads), len(tails)
    return out[0], out[1], out[2]


def answer_counts(kh, kr, kt, h, r, t, any_relation=False):
    """(n_tails, n_heads) int64[G]: for every query triple a loop over the known triples"""
    n_tails, n_heads = np.zeros(len(h), np.int64), np.zeros(len(h), np.int64)
    known = list(zip(kh.tolist(), kr.tolist(), kt.tolist()))
    for g, (a, b, c) in enumerate(zip(h.tolist(), r.tolist(), t.tolist())):
        n_tails[g] = len({z for x, y, z in known if x == a and (any_relation or y == b)})
        n_heads[g] = len({x for x, y, z in known if z == c and (any_relation or y == b)})
    return n_tails, n_heads


def subsampling_weights(n_tails, n_heads, start=4.0):
    return (1.0 / np.sqrt(np.float64(start) + (n_tails + n_heads).astype(np.float64))).astype(np.float32)


# ----------------------------------------------------------------------------- the draw
def is_known(known, any_relation, h, r, t):
    if any_relation:
        return any((h, q, t) in known for q in range(N_REL))
    return (h, r, t) in known


def sample(h, r, t, k, seed, group_offset=0, n_entities=N_ENT, corrupt="tail", known=None, filtered=None,
           any_relation=False, pool=None, card=None, fault=None):
    """dict(neg int64[G, K], head_side bool[G], unfiltered bool[G, K], tries int64[G, K]) of the draw.  known: a set of
    (h, r, t); card: (H_r, Tl_r) arrays for 'bernoulli' (default: those of `known`)."""
    filtered = known is not None if filtered is None else filtered
    g_n = len(h)
    if corrupt == "bernoulli" and card is None:
        kk = np.asarray(sorted(known), dtype=np.int64).reshape(-1, 3)
        card = cardinalities(kk[:, 0], kk[:, 1], kk[:, 2])[1:]
    neg, tries = np.zeros((g_n, k), np.int64), np.zeros((g_n, k), np.int64)
    head_side, unfiltered = np.zeros(g_n, bool), np.zeros((g_n, k), bool)
    counters = np.uint64(1) + np.arange(k * MAX_TRIES, dtype=np.uint64)
    if fault == "shared_slot0":
        counters = np.uint64(1) + np.tile(np.arange(MAX_TRIES, dtype=np.uint64), k)
    with np.errstate(over="ignore"):
        ks_ = keys(seed, np.arange(g_n, dtype=np.uint64) + np.uint64(0 if fault == "offset_dropped" else group_offset))
        side_values = values(ks_, np.zeros(g_n, np.uint64))
    for g in range(g_n):
        hg, rg, tg = int(h[g]), int(r[g]), int(t[g])
        v0 = int(side_values[g])
        if corrupt == "tail":
            head = False
        elif corrupt == "head":
            head = True
        elif corrupt == "both":
            head = v0 % 2 == 1
        else:
            n_h, n_t = (int(card[0][rg]), int(card[1][rg])) if 0 <= rg < len(card[0]) else (0, 0)
            head = n_h + n_t != 0 and (v0 % (n_h + n_t) < (n_h if fault == "bernoulli_inverted" else n_t))
        head_side[g] = head
        truth = hg if head else tg
        side_pool = pool[1 if head else 0] if pool is not None else None
        span = len(side_pool) if side_pool is not None else n_entities
        with np.errstate(over="ignore"):
            pos = (values(ks_[g], counters) % np.uint64(span)).astype(np.int64)
        cand = side_pool[pos] if side_pool is not None else pos
        rejected = {}                                   # candidate id -> rejected?  (the set decides)
        for c in set(cand.tolist()):
            rej = c == truth and fault != "truth_not_rejected"
            if filtered and not rej:
                anyrel = any_relation or fault == "relation_ignored"
                if fault == "wrong_side_structure":     # the other side's structure, searched in this side's row
                    rej = is_known(known, anyrel, tg, rg, c) if head else is_known(known, anyrel, c, rg, hg)
                else:
                    rej = is_known(known, anyrel, c, rg, tg) if head else is_known(known, anyrel, hg, rg, c)
            rejected[c] = rej
        rej = np.asarray([rejected[c] for c in cand.tolist()], dtype=bool).reshape(k, MAX_TRIES)
        cand = cand.reshape(k, MAX_TRIES)
        first = np.where(rej.all(1), MAX_TRIES - 1, np.argmin(rej, axis=1))
        neg[g] = cand[np.arange(k), first]
        unfiltered[g] = rej.all(1)
        tries[g] = first + 1
    return dict(neg=neg, head_side=head_side, unfiltered=unfiltered, tries=tries)


# ----------------------------------------------------------------------------- the cases
CONFIGS = [(corrupt, pool, any_relation) for corrupt in CORRUPT for pool in (None, "pair") for any_relation in (False, True)]


@functools.lru_cache(maxsize=None)
def reference(corrupt, pool=None, any_relation=False, filtered=True, saturated=True, seed=12345, group_offset=0, fault=None):
    """The G_MAX x K_MAX draw of a configuration, computed once: a case of G groups and K slots is its [:G, :K] (that the
    reference has this property is checked in test_negatives_host.py)."""
    h, r, t = positives(saturated)
    return sample(h, r, t, K_MAX, seed, group_offset, corrupt=corrupt, known=known_set(), filtered=filtered,
                  any_relation=any_relation, pool=pools(pool), fault=fault)


def cut(ref, g, k, g0=0):
    return dict(neg=ref["neg"][g0:g0 + g, :k], head_side=ref["head_side"][g0:g0 + g],
                unfiltered=ref["unfiltered"][g0:g0 + g, :k])


def same_draw(got, want):
    """The first check of the GPU test: entry for entry, no tolerance."""
    return all(np.array_equal(np.asarray(got[key]), np.asarray(want[key])) and
               np.asarray(got[key]).shape == np.asarray(want[key]).shape for key in ("neg", "head_side", "unfiltered"))


def violations(out, h, r, t, pool=None, filtered=True, any_relation=False):
    """The second check: the entries NOT flagged unfiltered that are the truth, known on their side, or outside the pool."""
    known, bad = known_set(), 0
    neg, head_side, unfiltered = (np.asarray(out[key]) for key in ("neg", "head_side", "unfiltered"))
    for g in range(neg.shape[0]):
        hg, rg, tg, head = int(h[g]), int(r[g]), int(t[g]), bool(head_side[g])
        allowed = set(pool[1 if head else 0].tolist()) if pool is not None else None
        for j in range(neg.shape[1]):
            c = int(neg[g, j])
            if unfiltered[g, j]:
                continue
            bad += c == (hg if head else tg) or (allowed is not None and c not in allowed) or not 0 <= c < N_ENT or \
                (filtered and (is_known(known, any_relation, c, rg, tg) if head else is_known(known, any_relation, hg, rg, c)))
    return bad
