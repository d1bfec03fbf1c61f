"""No GPU: the checks of tests/relation_loss_cases.py accept a float32 restatement of the relation-loss kernels' steps and
reject planted faults (the mask ignored, the truth masked, the scale ignored, e not added, relation j reading relation
j + 1's block, the one-hot missing from the coefficients) by more than 10 x the bound -- so that a green
test_relation_loss_gpu.py says something about the kernels; the closed-form gradients are the derivative of the dense
torch head; the dropped-relation lists against a Python double loop; the argument checks; the fifth ABI table against its
header; the error convention of the two entry points."""
import importlib
import itertools
import os
from types import SimpleNamespace

import pytest
import torch

import relation_loss_cases as RC
import softmax_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (P, R, D, C or None = shared mode): all filtered, R >= 2, a scale below 1
HOST_SHAPES = [(5, 3, 64, 5), (33, 65, 64, "D"), (2, 130, 300, 5), (5, 64, 17, None), (33, 3, 300, None)]
DEVICE = "MI355X|no CPU"
NAMES = ("c", "G", "gd")


def test_the_cases_cover_every_pair_of_values():
    assert RC.PS == (1, 2, 5, 33) and RC.RS == (1, 2, 3, 64, 65, 130) and RC.DS == (1, 3, 4, 17, 64, 300, 600)
    assert RC.CS == ("D", 5, 300)
    for cases, lists in ((RC.SLAB_CASES, (RC.PS, RC.RS, RC.DS, RC.CS, RC.ALIGNED, RC.FILTERED)),
                         (RC.SHARED_CASES, (RC.PS, RC.RS, RC.DS, RC.ALIGNED, RC.FILTERED))):
        for a, b in itertools.combinations(range(len(lists)), 2):
            met = {(c[a], c[b]) for c in cases}
            assert met == set(itertools.product(lists[a], lists[b])), (a, b)
        assert len(cases) <= 60 and len(set(cases)) == len(cases)
    assert RC.depth(1) == RC.depth(64) == 6 and RC.depth(65) == 7 and RC.depth(130) == 8
    assert RC.logit_roundings(1) == RC.logit_roundings(256) == 14 and RC.logit_roundings(300) == 18
    assert RC.loss_roundings(64, 64) == 40 and RC.grad_roundings(65, 4, "c") == 17
    assert RC.grad_roundings(65, 4, "G") == 19 and RC.grad_roundings(3, 4, "gd") == 20


@pytest.mark.parametrize("p,n_rel,k,c", HOST_SHAPES)
def test_float32_restatement_is_accepted_and_faults_are_rejected(p, n_rel, k, c):
    case = RC.exact_case(p, n_rel, k, c, seed=p + n_rel + k, filtered=True)
    d, w, e, truth, mask, scale = (case[x] for x in ("d", "w", "e", "truth", "mask", "scale"))
    assert scale < 1.0 and bool(mask.any()) and not bool(mask[torch.arange(p), truth].any())
    u3 = RC.slab_of(d, w, n_rel)
    ref = RC.loss_eval(u3, e, truth, mask, scale)
    z32, z64 = RC.logits(u3, e, truth, mask, scale, torch.float32), RC.logits(u3, e, truth, mask, scale)
    assert torch.equal(z32.double(), z64)                                          # the logits ARE exact in float32
    assert bool((ref[0].abs() + ref[1].abs() >= 1.0).all())
    r32 = float(RC.loss_measure(RC.loss_eval(u3, e, truth, mask, scale, torch.float32)[2], ref).max())
    bound = RC.loss_bound(r32, n_rel, k)
    loss, z, _ = RC.kernel_loss_eval(u3, e, truth, mask, scale)
    assert torch.equal(z.double(), z64)
    r = float(RC.loss_measure(loss, ref).max())
    print(f"loss: r {r:.3g}, r_torch32 {r32:.3g}, bound {bound:.3g}")
    assert r <= bound, (r, bound)
    for fault in RC.FAULTS_LOSS:
        bad = RC.loss_eval(u3, e, truth, mask, scale, torch.float32, fault=fault)[2]
        r_bad = float(RC.loss_measure(bad, ref).max())
        assert r_bad > 10 * bound, (fault, r_bad, bound)
    # the gradients
    g = RC.upstream(p, k)
    want = RC.grads_eval(u3, d, w, e, truth, mask, scale, g)
    t32 = RC.grads_eval(u3, d, w, e, truth, mask, scale, g, torch.float32)
    got = RC.kernel_grads_eval(u3, e, truth, mask, scale, g)
    bounds = {}
    for name in NAMES:
        r32 = C.worst(t32[name], want[name], want[name + "_scale"])
        bounds[name] = RC.grad_bound(r32, n_rel, k, name)
        r = C.worst(got[name], want[name], want[name + "_scale"])
        print(f"{name}: r {r:.3g}, r_torch32 {r32:.3g}, bound {bounds[name]:.3g}")
        assert r <= bounds[name], (name, r, bounds[name])
        assert bool((got[name][mask] == 0).all()) if name != "gd" else True        # a dropped relation: exactly zero
    for fault in RC.FAULTS_GRAD:
        bad = RC.grads_eval(u3, d, w, e, truth, mask, scale, g, torch.float32, fault=fault)
        ratio = max(C.worst(bad[name], want[name], want[name + "_scale"]) / bounds[name] for name in NAMES)
        assert ratio > 10, (fault, ratio)


def test_the_truth_alone_is_exactly_zero_in_the_restatement():
    case = RC.exact_case(5, 65, 17, None, seed=3, filtered=True)
    u3 = RC.slab_of(case["d"], None, 65)
    loss, z, lse = RC.kernel_loss_eval(u3, case["e"], case["truth"], case["mask"], case["scale"])
    assert int((z[0] > -float("inf")).sum()) == 1 and float(loss[0]) == 0.0     # pair 0: every relation but the truth dropped
    got = RC.kernel_grads_eval(u3, case["e"], case["truth"], case["mask"], case["scale"], RC.upstream(5, 1))
    assert bool((got["c"][0] == 0).all()) and bool((got["G"][0] == 0).all()) and bool((got["gd"][0] == 0).all())
    one = RC.exact_case(3, 1, 4, None, seed=1)                                   # R = 1: the same without a filter
    loss, _, _ = RC.kernel_loss_eval(RC.slab_of(one["d"], None, 1), one["e"], one["truth"], None, one["scale"])
    assert bool((loss == 0).all())


@pytest.mark.parametrize("c", [5, None])
def test_closed_form_gradients_are_the_derivative_of_the_dense_head(c):
    case = RC.random_case(7, 9, 12, c, seed=3, filtered=True)
    d, w, e, truth, mask, scale, g = (case[x] for x in ("d", "w", "e", "truth", "mask", "scale", "g"))
    want = RC.grads_eval(RC.slab_of(d, w, 9), d, w, e, truth, mask, scale, g)
    dd, dw, de = RC.autograd_eval(d, w, e, truth, mask, scale, g, torch.float64)
    assert C.worst(want["dd"], dd, want["dd_scale"]) <= 1e-12 and C.worst(want["de"], de, want["de_scale"]) <= 1e-12
    if w is not None:
        assert C.worst(want["dw"], dw, want["dw_scale"]) <= 1e-12
    assert bool((want["c"][mask] == 0).all())
    loose = RC.grads_eval(RC.slab_of(d, w, 9), d, w, e, truth, mask, scale, g, fault="no_onehot")
    assert C.worst(loose["de"], de, want["de_scale"]) > 1e-3


def test_dropped_relations_equal_a_python_double_loop():
    n_rel = 5
    # pair 0: every relation known; pair 1: none; pair 2: its truth and one more, the other listed twice; pair 3: (t, h) of
    # pair 2 reversed, which is another pair
    h, t, r = torch.tensor([0, 2, 4, 5]), torch.tensor([1, 3, 5, 4]), torch.tensor([2, 0, 1, 1])
    known = [(0, j, 1) for j in range(n_rel)] + [(4, 1, 5), (4, 3, 5), (4, 3, 5), (9, 0, 3), (2, 4, 7)]
    kh, kr, kt = (torch.tensor([x[i] for x in known]) for i in range(3))
    mask = RC.dropped_mask(kh, kr, kt, h, r, t, n_rel)
    want = torch.zeros((4, n_rel), dtype=torch.bool)
    for i in range(4):
        for j in range(n_rel):
            want[i, j] = j != int(r[i]) and (int(h[i]), j, int(t[i])) in known
    assert torch.equal(mask, want)
    assert mask[0].tolist() == [True, True, False, True, True] and not bool(mask[1].any()) and not bool(mask[3].any())
    assert mask[2].tolist() == [False, False, False, True, False]
    # the triples a mask is turned into give the mask back, duplicate and known truths included
    gen = torch.Generator().manual_seed(2)
    truth = torch.randint(0, 7, (6,), generator=gen)
    m = RC.random_mask(6, 7, truth, gen)
    kh, kr, kt, hh, tt = RC.triples_of_mask(m, truth)
    assert kh.numel() == int(m.sum()) + 3 + 1
    assert torch.equal(RC.dropped_mask(kh, kr, kt, hh, truth, tt, 7), m)


# ----------------------------------------------------------------------------- argument checks
def _stand_in(scoring="transe", n=40, c=8, n_rel=3):
    def no_table(*a):
        raise AssertionError("the table was asked for")
    gen = torch.Generator().manual_seed(5)
    return SimpleNamespace(entity_embed=SimpleNamespace(weight=torch.randn(n, c, generator=gen)),
                           relation_embed=SimpleNamespace(weight=torch.randn(n_rel, c, generator=gen)),
                           gat_trans_M=None, n_entities=n, n_relations=n_rel, relation_dim=c, scoring=scoring,
                           training=False, _table_for_inference=no_table, _embeddings_and_ids=no_table,
                           gat_embeddings=no_table)


def test_argument_errors_come_before_any_device_work():
    import literalkg_amd as L
    rl = importlib.import_module("literalkg_amd.relation_loss")
    for name in ("relation_loss", "relation_softmax_loss"):
        assert name in L.__all__ and getattr(L, name) is getattr(rl, name)
    assert hasattr(L.LiteralKG, "calc_relation_loss")
    model = _stand_in()
    h, r, t = torch.tensor([0, 1, 2]), torch.tensor([0, 1, 2]), torch.tensor([3, 4, 5])
    for kw, msg in ((dict(scoring="dot"), "scoring='dot' has no relation prediction"),
                    (dict(scoring="mlp"), "scoring='mlp' has no triple score"),
                    (dict(scoring="rotate"), "scoring must be one of"),
                    (dict(reduction="max"), "reduction must be one of"), (dict(scale=0.0), "scale must be a positive"),
                    (dict(scale=float("inf")), "scale must be a positive"), (dict(scale=True), "scale must be a positive"),
                    (dict(chunk_bytes=0), "chunk_bytes must be a positive integer"),
                    (dict(scoring="transr"), "needs a model with gat_trans_M"),
                    (dict(known=SimpleNamespace(n_relations=4, n_entities=40, device=torch.device("cpu"))),
                     "known triples over 4 relations"),
                    (dict(known=SimpleNamespace(n_relations=3, n_entities=41, device=torch.device("cpu"))),
                     "known triples over 41 entities"),
                    (dict(known=SimpleNamespace(n_relations=3, n_entities=40, device=torch.device("cuda:0"))),
                     "known triples live on")):
        with pytest.raises(ValueError, match=msg):
            rl.relation_loss(model, h, r, t, **kw)
    with pytest.raises(ValueError, match="different lengths"):
        rl.relation_loss(model, h, r[:2], t)
    with pytest.raises(ValueError, match="must be a 1-D tensor of integer ids"):
        rl.relation_loss(model, h.float(), r, t)
    with pytest.raises(TypeError):
        rl.relation_loss(model, h, r, t, side="tail")                      # the loss has no side
    with pytest.raises(NotImplementedError, match="row-sharded"):
        rl.relation_loss(SimpleNamespace(local=model), h, r, t)
    with pytest.raises(RuntimeError, match=DEVICE):                        # a CPU model: refused, the table never asked for
        rl.relation_loss(model, h, r, t)
    transr = _stand_in("transr")
    transr.gat_trans_M = torch.zeros(3, 8, 6)
    with pytest.raises(ValueError, match=r"one pair's slab takes 72 bytes .* chunk_bytes is 71"):
        rl.relation_loss(transr, h, r, t, chunk_bytes=71)
    empty = rl.relation_loss(model, h[:0], r[:0], t[:0], reduction="none")
    assert empty.shape == (0,) and empty.dtype == torch.float32
    assert rl.relation_loss(model, h[:0], r[:0], t[:0]).shape == ()
    from literalkg_amd.distributed import ShardedLiteralKG
    with pytest.raises(NotImplementedError, match="row-sharded"):
        ShardedLiteralKG.calc_relation_loss(None, h, r, t)


def test_the_op_refuses_bad_arguments():
    rl = importlib.import_module("literalkg_amd.relation_loss")
    d, w, e, truth = torch.randn(3, 8), torch.randn(4, 8, 6), torch.randn(4, 6), torch.tensor([0, 1, 2])
    with pytest.raises(RuntimeError, match=DEVICE):
        rl.relation_softmax_loss(d, w, e, truth)
    for kw, msg in ((dict(scale=-1.0), "scale must be a positive"), (dict(chunk_bytes=-5), "chunk_bytes must be a positive")):
        with pytest.raises(ValueError, match=msg):
            rl.relation_softmax_loss(d, w, e, truth, **kw)
    assert rl.chunk_rows(33, 4, 6, 96 * 5) == 5 and rl.chunk_rows(3, 4, 6, 1 << 20) == 3 and rl.chunk_rows(3, 4, 6, 96) == 1
    with pytest.raises(ValueError, match="one pair's slab takes 96 bytes .* chunk_bytes is 95"):
        rl.chunk_rows(3, 4, 6, 95)
    # the Function lives in its own module, outside the closed list of ops.py's Functions
    from literalkg_amd import ops
    assert issubclass(rl._RelationSoftmaxLoss, torch.autograd.Function) and not hasattr(ops, "_RelationSoftmaxLoss")


# ----------------------------------------------------------------------------- the entry points
ENTRY_POINTS = ["lkg_relation_loss_bwd_f32", "lkg_relation_loss_fwd_f32"]


def test_the_two_entry_points_are_declared_and_bound():
    import __graft_entry__ as ge
    ge.build()
    from literalkg_amd import _native, build
    from wide_cases import prototypes
    assert "lkg_relation_loss.hip" in build.SOURCES
    assert os.path.exists(os.path.join(ROOT, "literalkg_amd", "csrc", "lkg_relation_loss.hip"))
    assert set(ENTRY_POINTS) <= set(_native.PROTOTYPES) and set(ENTRY_POINTS) <= set(prototypes())


def _fwd(n=1, n_rel=2, k=4, ldu=8, rel_stride=4, lde=4, scale=1.0, ldz=2, rowptr=None):
    return (n, n_rel, k, None, ldu, rel_stride, None, lde, None, None, None, rowptr, None, None, None, scale, None, ldz,
            None, None, None)


def _bwd(n=1, n_rel=2, k=4, ldu=8, rel_stride=4, lde=4, scale=1.0, ldz=2, gd=None, ldgd=4, c=None, ldc=2):
    return (n, n_rel, k, None, ldu, rel_stride, None, lde, None, scale, None, None, ldz, gd, ldgd, c, ldc, None)


def test_error_convention_of_the_two_entry_points():
    import __graft_entry__ as ge
    ge.build()
    import numpy as np
    from literalkg_amd import _native
    call, E = _native.call, _native.LkgError
    some = _native.ptr(np.zeros(8, np.float32))                                     # (never reached: the checks come first)
    for bad in (dict(n=-1), dict(n_rel=0), dict(k=0), dict(lde=3), dict(ldz=1), dict(rel_stride=3), dict(ldu=7),
                dict(rel_stride=0, ldu=3), dict(rel_stride=-4)):
        with pytest.raises(E, match="lkg_relation_loss_fwd_f32: bad sizes"):
            call("lkg_relation_loss_fwd_f32", *_fwd(**bad))
        with pytest.raises(E, match="lkg_relation_loss_bwd_f32: bad sizes"):
            call("lkg_relation_loss_bwd_f32", *_bwd(**bad))
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(E, match="lkg_relation_loss_fwd_f32: scale must be positive"):
            call("lkg_relation_loss_fwd_f32", *_fwd(scale=bad))
        with pytest.raises(E, match="lkg_relation_loss_bwd_f32: scale must be positive"):
            call("lkg_relation_loss_bwd_f32", *_bwd(scale=bad))
    with pytest.raises(E, match="lkg_relation_loss_fwd_f32: a filter needs"):
        call("lkg_relation_loss_fwd_f32", *_fwd(rowptr=some))
    with pytest.raises(E, match="lkg_relation_loss_fwd_f32: null pointer"):
        call("lkg_relation_loss_fwd_f32", *_fwd())
    call("lkg_relation_loss_fwd_f32", *_fwd(n=0))                                   # P = 0 returns before the pointer checks
    for bad in (dict(rel_stride=0, gd=some, ldgd=3), dict(rel_stride=0, c=some, ldc=1)):
        with pytest.raises(E, match="lkg_relation_loss_bwd_f32: bad sizes"):
            call("lkg_relation_loss_bwd_f32", *_bwd(**bad))
    with pytest.raises(E, match="lkg_relation_loss_bwd_f32: slab mode .* takes no gd and no c"):
        call("lkg_relation_loss_bwd_f32", *_bwd(gd=some))
    with pytest.raises(E, match="lkg_relation_loss_bwd_f32: null pointer"):
        call("lkg_relation_loss_bwd_f32", *_bwd())
    with pytest.raises(E, match="lkg_relation_loss_bwd_f32: null pointer"):
        call("lkg_relation_loss_bwd_f32", *_bwd(rel_stride=0, gd=some))
    call("lkg_relation_loss_bwd_f32", *_bwd(n=0))
    call("lkg_relation_loss_bwd_f32", *_bwd(rel_stride=0))                          # shared mode, no output asked for
