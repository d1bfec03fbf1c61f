"""No GPU: the reference of tests/negative_cases.py is a usable generator at the seeds the GPU tests use (chi-square of the
unfiltered draw and of the hub row's kept candidates, no slot out of tries), has the properties the GPU test holds the
kernel to (prefix in K, cut with group_offset, independence of the other groups) and meets the condition n_unfiltered == 0
on every case without the saturated head or the one-element pool; the checks the GPU test applies reject the planted
faults; the fourth ABI table against its header; the error convention of the three entry points; the exports and every
ValueError / IndexError of the Python layer that needs no device.

Measured here (printed by the tests): chi-square of the unfiltered draw 242.6 / 259.1 / 240.5 at seeds 1 / 12345 / 2^63 - 1
(bound 256 +- 90.5); hub row at seed 7: worst slot 41 tries, chi-square 44.6 over the 57 kept candidates (bound 56 +- 42.3).
"""
import math
import os
import re

import numpy as np
import pytest
import torch

import negative_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = "MI355X|no CPU"


# ----------------------------------------------------------------------------- the generator
def test_numpy_stream_is_the_python_integer_stream():
    with np.errstate(over="ignore"):
        for seed in C.SEEDS + (0, 2 ** 64 - 1):
            for gid in (0, 1, 128, 2 ** 40 + 3):
                key = C.keys(seed, [gid])[0]
                for c in (0, 1, 64, 1 + 256 * C.MAX_TRIES + 63):
                    assert int(C.values(key, [c])[0]) == C.value_int(seed, gid, c)
    assert C.mix64_int(0) == 0 and C.mix64_int(1) == 0x5692161D100B05E5           # splitmix64's finaliser


@pytest.mark.parametrize("seed", C.SEEDS)
def test_unfiltered_draw_is_uniform(seed):
    g = np.arange(1024)
    out = C.sample((g * 7) % 257, np.zeros(1024, np.int64), g % 257, 64, seed, filtered=False)
    counts = np.bincount(out["neg"].reshape(-1), minlength=257)
    expect = counts.sum() / 257
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    print(f"seed {seed}: chi-square {chi2:.1f} over 257 candidates")
    assert not out["unfiltered"].any() and counts.sum() == 1024 * 64
    assert abs(chi2 - 256) <= 4 * math.sqrt(512), chi2


def test_hub_row_never_runs_out_of_tries_and_is_uniform_over_what_is_left():
    n = 1024
    out = C.sample(np.full(n, C.HUB), np.zeros(n, np.int64), np.ones(n, np.int64), 8, 7, known=C.known_set())
    kept = [0] + list(range(201, 257))
    assert not out["unfiltered"].any() and set(out["neg"].reshape(-1).tolist()) <= set(kept)
    counts = np.bincount(out["neg"].reshape(-1), minlength=257)[kept]
    expect = n * 8 / 57
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    print(f"worst slot {int(out['tries'].max())} tries, chi-square {chi2:.1f} over 57 candidates")
    assert int(out["tries"].max()) < C.MAX_TRIES
    assert abs(chi2 - 56) <= 4 * math.sqrt(112), chi2


def test_the_graph_is_the_one_the_cases_describe():
    h, r, t = C.graph()
    known = C.known_set()
    assert len(known) < len(h)                                                    # duplicated triples
    triples, heads, tails = C.cardinalities(h, r, t)
    assert triples[4] == heads[4] == tails[4] == 0                                # the absent relation
    assert heads[2] == 2 and tails[2] == 71 and heads[3] == 91 + 1 and tails[3] == 3      # 1-to-N, N-to-1 (+ the pair 40, 41)
    assert sum((C.HUB, 0, c) in known for c in range(257)) == 200
    assert all((C.SATURATED, 1, c) in known for c in range(256)) and (C.SATURATED, 1, C.SATURATED) not in known
    assert C.NO_TRIPLES not in h.tolist() and {0, 256} <= set(h.tolist()) and {0, 256} <= set(t.tolist()) | set(h.tolist())
    ph, pr, pt = C.positives()
    assert (int(ph[2]), int(ph[5]), int(ph[70]), int(pr[4])) == (C.NO_TRIPLES, C.SATURATED, C.SATURATED, 4)
    assert C.SATURATED not in C.positives(False)[0].tolist()


# ----------------------------------------------------------------------------- properties and the condition
@pytest.mark.parametrize("corrupt,pool,any_relation", C.CONFIGS)
def test_reference_properties_and_the_unfiltered_condition(corrupt, pool, any_relation):
    ref = C.reference(corrupt, pool, any_relation)
    h, r, t = C.positives()
    kw = dict(corrupt=corrupt, known=C.known_set(), any_relation=any_relation, pool=C.pools(pool))
    # the first K' columns of a K-draw are the K'-draw; a group's row does not depend on the other groups
    assert C.same_draw(C.sample(h[:33], r[:33], t[:33], 3, 12345, **kw), C.cut(ref, 33, 3))
    pick = np.asarray([40, 5, 128])
    alone = [C.sample(h[i:i + 1], r[i:i + 1], t[i:i + 1], 64, 12345, group_offset=int(i), **kw) for i in pick]
    assert all(C.same_draw(a, C.cut(ref, 1, 64, int(i))) for a, i in zip(alone, pick))
    # a batch cut anywhere, the offset carried
    assert C.same_draw(C.sample(h[50:], r[50:], t[50:], 64, 12345, group_offset=50, **kw), C.cut(ref, 79, 64, 50))
    assert C.violations(ref, h, r, t, C.pools(pool), True, any_relation) == 0
    # the saturated head's groups alone hold the flagged slots; without it nothing is flagged
    flagged = np.flatnonzero(ref["unfiltered"].any(1)).tolist()
    assert set(flagged) <= {5, 70} and (corrupt != "tail" or flagged == [5, 70])
    clean = C.reference(corrupt, pool, any_relation, saturated=False)
    assert int(clean["unfiltered"].sum()) == 0
    assert C.violations(clean, *C.positives(False), C.pools(pool), True, any_relation) == 0


def test_saturated_head_and_one_element_pool_of_the_reference():
    h, r, t = C.positives()
    sat = C.reference("tail", "no_anchor")
    assert sat["unfiltered"][[5, 70]].all() and (sat["tries"][[5, 70]] == C.MAX_TRIES).all()
    free = C.reference("tail")                          # every entity a candidate: only the head itself passes
    assert ((free["neg"][[5, 70]] == C.SATURATED) | free["unfiltered"][[5, 70]]).all()
    one = C.sample(h[5:6], r[5:6], t[5:6], 9, 3, group_offset=5, known=C.known_set(), pool=C.pools("truth"))
    assert one["unfiltered"].all() and (one["neg"] == 7).all()


# ----------------------------------------------------------------------------- planted faults
FAULT_CONFIG = {"wrong_side_structure": ("both", None, False), "relation_ignored": ("both", None, False),
                "truth_not_rejected": ("head", "pair", False), "offset_dropped": ("bernoulli", "pair", True),
                "shared_slot0": ("tail", None, False), "bernoulli_inverted": ("bernoulli", None, False)}


@pytest.mark.parametrize("fault", C.FAULTS)
def test_the_checks_reject_planted_faults(fault):
    corrupt, pool, any_relation = FAULT_CONFIG[fault]
    offset = 17 if fault == "offset_dropped" else 0
    good = C.reference(corrupt, pool, any_relation, group_offset=offset)
    bad = C.reference(corrupt, pool, any_relation, group_offset=offset, fault=fault)
    assert not C.same_draw(bad, good), fault
    for g, k in ((33, 64), (129, 257)):                                           # also at the smaller shapes of the GPU test
        assert not C.same_draw(C.cut(bad, g, k), C.cut(good, g, k)), (fault, g, k)
    if fault in ("wrong_side_structure", "truth_not_rejected"):                   # the property check alone sees these too
        assert C.violations(bad, *C.positives(), C.pools(pool), True, any_relation) > 0
    if fault == "relation_ignored":                                               # (it only rejects MORE: equality sees it)
        assert C.violations(bad, *C.positives(), C.pools(pool), True, any_relation) == 0


# ----------------------------------------------------------------------------- the entry points and the published constants
NAMES = ["lkg_answer_counts", "lkg_relation_cardinality", "lkg_sample_negatives"]


def test_the_three_entry_points_are_declared_and_bound_and_the_header_publishes_the_constants():
    import __graft_entry__ as ge
    ge.build()
    from literalkg_amd import _native, build, negatives
    from wide_cases import prototypes
    assert "lkg_negatives.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "lkg_negatives.hip"))
    assert set(NAMES) <= set(_native.PROTOTYPES) and set(NAMES) <= set(prototypes())
    raw = open(os.path.join(ROOT, "include", "literalkg_hip.h")).read()
    assert int(re.search(r"#define LKG_SAMPLE_MAX_TRIES (\d+)", raw).group(1)) == negatives.MAX_TRIES == C.MAX_TRIES == 64
    for i, mode in enumerate(negatives.CORRUPT):
        assert int(re.search(r"#define LKG_CORRUPT_" + mode.upper() + r" (\d+)", raw).group(1)) == i
    assert negatives.CORRUPT == C.CORRUPT


def _sample(g=1, k=2, n=10, n_rel=3, mode=0, filtered=0, offset=0, pool=None, pool_len=0, some=None):
    s = [some] * 8
    return (g, k, 1, offset, some, some, some, n, n_rel, mode, filtered, 0, *s, some, some, pool, pool_len, None, 0,
            some, some, some, None)


def test_error_convention_of_the_three_entry_points():
    import __graft_entry__ as ge
    ge.build()
    from literalkg_amd import _native
    call, E = _native.call, _native.LkgError
    some = _native.ptr(np.zeros(64, np.int64))                                      # (never reached: the checks come first)
    for bad in (dict(g=-1), dict(k=0), dict(n=0), dict(n_rel=-1), dict(offset=-1), dict(pool_len=-1), dict(g=2 ** 38, k=2)):
        with pytest.raises(E, match="lkg_sample_negatives: bad sizes"):
            call("lkg_sample_negatives", *_sample(**bad))
    for mode in (-1, 4):
        with pytest.raises(E, match="lkg_sample_negatives: unknown mode"):
            call("lkg_sample_negatives", *_sample(mode=mode))
    with pytest.raises(E, match="lkg_sample_negatives: empty pool"):
        call("lkg_sample_negatives", *_sample(pool=some, pool_len=0))
    with pytest.raises(E, match="lkg_sample_negatives: null pointer"):
        call("lkg_sample_negatives", *_sample())
    call("lkg_sample_negatives", *_sample(g=0))                                     # G = 0 returns before the pointer checks
    args = list(_sample(some=some, filtered=1))
    args[12] = None                                                                 # head_rowptr of a filtered tail draw
    with pytest.raises(E, match="lkg_sample_negatives: null structure of a filtered side"):
        call("lkg_sample_negatives", *args)
    args = list(_sample(some=some, mode=3))
    args[20] = None                                                                 # rel_heads of a Bernoulli draw
    with pytest.raises(E, match="lkg_sample_negatives: null relation counts"):
        call("lkg_sample_negatives", *args)

    def card(n=10, n_rel=3, n_raw=5, nnz=4, p=None, out=None):
        return (n, n_rel, n_raw, p, p, p, nnz, p, p, p, out, out, out, None)
    for bad in (dict(n=0), dict(n_rel=-1), dict(n_raw=-1), dict(nnz=6), dict(n_raw=2 ** 31)):
        with pytest.raises(E, match="lkg_relation_cardinality: bad sizes"):
            call("lkg_relation_cardinality", *card(**bad))
    with pytest.raises(E, match="lkg_relation_cardinality: at most 4096 relations"):
        call("lkg_relation_cardinality", *card(n_rel=4097))
    with pytest.raises(E, match="lkg_relation_cardinality: null pointer"):
        call("lkg_relation_cardinality", *card())
    call("lkg_relation_cardinality", *card(n_rel=0))                                # no relation: nothing to count

    def answers(n=1, n_ent=10, p=None):
        return (n, p, p, p, n_ent, p, p, p, p, p, p, p, p, None)
    for bad in (dict(n=-1), dict(n_ent=0), dict(n=2 ** 38)):
        with pytest.raises(E, match="lkg_answer_counts: bad sizes"):
            call("lkg_answer_counts", *answers(**bad))
    with pytest.raises(E, match="lkg_answer_counts: null pointer"):
        call("lkg_answer_counts", *answers())
    call("lkg_answer_counts", *answers(n=0))


# ----------------------------------------------------------------------------- the Python layer
def _stand_in(scoring="transe", n=40, c=8, n_rel=3):
    from types import SimpleNamespace

    def no_table(*a):
        raise AssertionError("the table was asked for")
    gen = torch.Generator().manual_seed(5)
    return SimpleNamespace(entity_embed=SimpleNamespace(weight=torch.randn(n, c, generator=gen)),
                           relation_embed=SimpleNamespace(weight=torch.randn(n_rel, c, generator=gen)),
                           gat_trans_M=None, n_entities=n, n_relations=n_rel, relation_dim=c, scoring=scoring,
                           training=False, _table_for_inference=no_table, _embeddings_and_ids=no_table,
                           gat_embeddings=no_table)


def test_exports_and_argument_errors_come_before_any_device_work():
    import literalkg_amd as L
    from literalkg_amd import negatives as ng
    for name in ("NegativeSampler", "NegativeBatch", "TripleEpoch", "RelationCardinalities", "relation_cardinalities",
                 "answer_counts", "subsampling_weights", "sampled_negative_loss"):
        assert name in L.__all__ and getattr(L, name) is getattr(ng, name)
    assert hasattr(L.LiteralKG, "calc_sampled_negative_loss")
    ids = torch.tensor([0, 1, 2])
    for kw, msg in ((dict(n_entities=0), "n_entities must be an integer"), (dict(n_entities=True), "n_entities must be"),
                    (dict(corrupt="left"), "corrupt must be one of"), (dict(filtered=True), "filtered=True needs the known"),
                    (dict(corrupt="bernoulli"), "corrupt='bernoulli' needs the known"),
                    (dict(known=object()), "as a KnownTriples"), (dict(pool=(ids,)), "a .tail_pool, head_pool. pair"),
                    (dict(pool=ids[:0]), "pool must be a non-empty 1-D int64"),
                    (dict(pool=ids.float()), "pool must be a non-empty 1-D int64"),
                    (dict(pool=(ids, ids.reshape(1, 3))), "the head pool must be")):
        with pytest.raises(ValueError, match=msg):
            ng.NegativeSampler(**{"n_entities": 10, **kw})
    with pytest.raises(IndexError, match="the candidate pool has 1 entity id"):
        ng.NegativeSampler(2, pool=ids)
    with pytest.raises(IndexError, match="the tail pool has 2 entity id"):
        ng.NegativeSampler(10, pool=(torch.tensor([-1, 3, 10]), ids))
    s = ng.NegativeSampler(10, corrupt="both", pool=ids)
    assert s.filtered is False and s.known is None and s.cardinalities is None
    for kw, msg in ((dict(k=0), "k must be an integer >= 1"), (dict(k=2.0), "k must be an integer"),
                    (dict(group_offset=-1), "group_offset must be an integer >= 0"),
                    (dict(seed=-1), "seed must be an integer in"), (dict(seed=2 ** 64), "seed must be an integer in")):
        with pytest.raises(ValueError, match=msg):
            s.sample(ids, ids, ids, **{"k": 2, **kw})
    with pytest.raises(ValueError, match="different lengths"):
        s.sample(ids, ids[:2], ids, 2)
    with pytest.raises(ValueError, match="h must be a 1-D tensor of integer ids"):
        s.sample(ids.float(), ids, ids, 2)
    with pytest.raises(RuntimeError, match=DEVICE):                               # CPU ids: refused, there is no CPU draw
        s.sample(ids, ids, ids, 2)
    for fn in (ng.relation_cardinalities, lambda k: ng.answer_counts(k, ids, ids, ids),
               lambda k: ng.subsampling_weights(k, ids, ids, ids)):
        with pytest.raises(ValueError, match="as a KnownTriples"):
            fn(None)
    for start in (0.0, -1.0, float("inf"), float("nan"), True, "4"):
        with pytest.raises(ValueError, match="start must be a finite number > 0"):
            ng.subsampling_weights(None, ids, ids, ids, start=start)
    for kw, msg in ((dict(batch_groups=0), "batch_groups must be a positive integer"),
                    (dict(seed=-1), "seed must be an integer in"), (dict(seed=1.5), "seed must be an integer in")):
        with pytest.raises(ValueError, match=msg):
            ng.TripleEpoch(ids, ids, ids, **{"batch_groups": 2, "seed": 0, **kw})
    with pytest.raises(ValueError, match="different lengths"):
        ng.TripleEpoch(ids, ids, ids[:1], 2, 0)
    # the epoch: every triple once, the offsets those of the shuffled order, the same order under another cut
    h = torch.arange(10)
    ep = ng.TripleEpoch(h, h + 10, h + 20, 4, seed=3)
    got = list(ep)
    assert len(ep) == len(got) == 3 and [b[3] for b in got] == [0, 4, 8] and [b[0].numel() for b in got] == [4, 4, 2]
    order = torch.cat([b[0] for b in got])
    assert sorted(order.tolist()) == list(range(10)) and order.tolist() != list(range(10))
    assert torch.equal(torch.cat([b[1] for b in got]), order + 10) and torch.equal(torch.cat([b[2] for b in got]), order + 20)
    assert torch.equal(torch.cat([b[0] for b in ng.TripleEpoch(h, h, h, 7, seed=3)]), order)
    # the loss
    model = _stand_in()
    neg = torch.tensor([[6, 7], [8, 9], [10, 11]])
    batch = ng.NegativeBatch(neg, torch.tensor([False, True, False]), torch.zeros(3, 2, dtype=torch.bool), 0)
    for kw, msg in ((dict(scoring="mlp"), "scoring='mlp' has no self-adversarial loss"),
                    (dict(reduction="max"), "reduction must be one of"), (dict(scale=0.0), "scale must be a positive"),
                    (dict(margin=float("nan")), "margin must be a finite number"),
                    (dict(temperature=-0.5), "temperature must be a finite number >= 0"),
                    (dict(scoring="transr"), "needs a model with gat_trans_M"),
                    (dict(weights=torch.ones(2)), "weights must be a float tensor"),
                    (dict(weights=torch.ones(3, dtype=torch.int64)), "weights must be a float tensor")):
        with pytest.raises(ValueError, match=msg):
            ng.sampled_negative_loss(model, ids, ids, ids, batch, **kw)
    for bad in (neg, None, ng.NegativeBatch(neg[:2], batch.head_side, batch.unfiltered, 0),
                ng.NegativeBatch(neg, batch.head_side.long(), batch.unfiltered, 0)):
        with pytest.raises(ValueError, match="batch must be the NegativeBatch of these 3 triples"):
            ng.sampled_negative_loss(model, ids, ids, ids, bad)
    with pytest.raises(NotImplementedError, match="row-sharded"):
        ng.sampled_negative_loss(type("Sharded", (), {"local": model})(), ids, ids, ids, batch)
    from literalkg_amd.distributed import ShardedLiteralKG
    with pytest.raises(NotImplementedError, match="row-sharded"):
        ShardedLiteralKG.calc_sampled_negative_loss(None, ids, ids, ids, batch)
    with pytest.raises(RuntimeError, match=DEVICE):                               # a CPU model: refused, the table never asked for
        ng.sampled_negative_loss(model, ids, ids, ids, batch)
