"""No GPU: the checks of tests/self_adversarial_cases.py accept a float32 restatement of the self-adversarial kernels'
algorithm and reject planted faults (the weights not detached, the temperature ignored, the positive's sign flipped, group
g reading group g + 1's negatives, a division by K on top of the weights) by more than 10 x the bound -- so that a green
test_self_adversarial_gpu.py says something about the kernels; the closed-form gradients are the derivative with the
weights detached; the argument checks; the third ABI table against its header; the error convention of the two entry
points."""
import itertools
import os
from types import SimpleNamespace

import pytest
import torch

import self_adversarial_cases as S
import softmax_cases as C

HOST_SHAPES = [(33, 5, 17), (2, 65, 64), (3, 257, 300), (33, 3, 3)]          # (G, K, k)
DEVICE = "MI355X|no CPU"


def test_the_cases_cover_every_pair_of_values():
    lists = (S.KS_COLS, S.KS_NEG, S.GS, S.ALIGNED, S.DISTANCE, S.TEMPERATURES)
    assert S.KS_COLS[:5] == (1, 3, 17, 64, 300) and S.KS_NEG == (1, 2, 3, 5, 64, 65, 257) and S.GS == (1, 2, 33)
    assert S.TEMPERATURES == (0.0, 0.25, 1.0)
    for a, b in itertools.combinations(range(len(lists)), 2):
        met = {(c[a], c[b]) for c in S.CASES}
        assert met == set(itertools.product(lists[a], lists[b])), (a, b)
    assert len(S.CASES) <= 60 and len(set(S.CASES)) == len(S.CASES)
    assert S.loss_roundings(1) == S.loss_roundings(64) == 24 and S.loss_roundings(257) == 32
    assert S.grad_roundings(3, "dn") == 20 and S.grad_roundings(3, "dq") == 23 and S.grad_roundings(257, "dq") == 91


@pytest.mark.parametrize("temperature", [0.25, 1.0])
@pytest.mark.parametrize("distance", [True, False])
@pytest.mark.parametrize("g,kn,k", HOST_SHAPES)
def test_float32_restatement_is_accepted_and_faults_are_rejected(g, kn, k, distance, temperature):
    q, p, n, margin, scale = S.exact_case(g, kn, k, distance, seed=g + kn + k, temperature=temperature)
    args = (q, p, n, distance, margin, scale, temperature)
    ref = S.loss_eval(*args)
    z32, z64 = S.logits(q, p, n, distance, margin, scale, torch.float32), S.logits(q, p, n, distance, margin, scale)
    assert torch.equal(z32[0].double(), z64[0]) and torch.equal(z32[1].double(), z64[1])    # the logits ARE exact in float32
    r32 = float(S.loss_measure(S.loss_eval(*args, torch.float32)[0], ref).max())
    bound = S.loss_bound(r32, kn)
    loss, w = S.kernel_loss_eval(*args)
    r = float(S.loss_measure(loss, ref).max())
    print(f"loss: r {r:.3g}, r_torch32 {r32:.3g}, bound {bound:.3g}")
    assert r <= bound, (r, bound)
    assert bool((w.sum(1) - 1).abs().max() < 1e-5)
    for fault in S.FAULTS_LOSS:
        bad = S.loss_eval(*args, torch.float32, fault=fault)[0]
        r_bad = float(S.loss_measure(bad, ref).max())
        assert r_bad > 10 * bound, (fault, r_bad, bound)
    # the gradients
    gen = torch.Generator().manual_seed(k)
    up = torch.rand((g,), generator=gen) + 0.5
    want = S.grads_eval(q, p, n, up, distance, margin, scale, temperature)
    auto32 = S.autograd_eval(q, p, n, up, distance, margin, scale, temperature, torch.float32)
    got = S.kernel_grads_eval(q, p, n, up, distance, margin, scale, temperature)
    bounds = {}
    for name, a32 in zip(("dq", "dp", "dn"), auto32):
        r32 = C.worst(a32, want[name], want[name + "_scale"])
        bounds[name] = S.grad_bound(r32, kn, name)
        r = C.worst(got[name], want[name], want[name + "_scale"])
        print(f"{name}: r {r:.3g}, r_torch32 {r32:.3g}, bound {bounds[name]:.3g}")
        assert r <= bounds[name], (name, r, bounds[name])
    for fault in S.FAULTS_GRAD:
        if fault == "weights_not_detached":
            bad = dict(zip(("dq", "dp", "dn"), S.autograd_eval(q, p, n, up, distance, margin, scale, temperature,
                                                               torch.float32, detach=False)))
        else:
            bad = S.grads_eval(q, p, n, up, distance, margin, scale, temperature, torch.float32, fault=fault)
        ratio = max(C.worst(bad[name], want[name], want[name + "_scale"]) / bounds[name] for name in bounds)
        assert ratio > 10, (fault, ratio)


@pytest.mark.parametrize("distance", [True, False])
def test_closed_form_gradients_are_the_derivative_with_detached_weights(distance):
    q, p, n, up = S.random_case(7, 9, 12, seed=3)
    want = S.grads_eval(q, p, n, up, distance, 1.5, 0.37, 0.7)
    for name, a64 in zip(("dq", "dp", "dn"), S.autograd_eval(q, p, n, up, distance, 1.5, 0.37, 0.7, torch.float64)):
        assert C.worst(want[name], a64, want[name + "_scale"]) <= 1e-12, name
    loose = S.autograd_eval(q, p, n, up, distance, 1.5, 0.37, 0.7, torch.float64, detach=False)
    assert C.worst(want["dn"], loose[2], want["dn_scale"]) > 1e-3                  # (the dw term is not small)


def test_special_weights_of_the_restatement():
    q, p, n, margin, scale = S.exact_case(4, 5, 17, True, seed=1)
    _, w = S.kernel_loss_eval(q, p, n, True, margin, scale, 0.0)
    assert torch.equal(w, torch.full((4, 5), 1.0 / 5.0, dtype=torch.float32))     # temperature 0: float32(1 / K)
    q, p, n, margin, scale = S.exact_case(4, 1, 17, True, seed=1)
    for t in (0.0, 0.25, 1.0):
        assert torch.equal(S.kernel_loss_eval(q, p, n, True, margin, scale, t)[1], torch.ones((4, 1)))
    q, p, n, margin, scale, t = S.extreme_case()
    zp, zn = S.logits(q, p, n, True, margin, scale)
    assert float(zn.min()) < -200 and float(torch.cat((zp, zn.reshape(-1))).max()) > 100
    loss, w = S.kernel_loss_eval(q, p, n, True, margin, scale, t)
    assert bool(torch.isfinite(loss).all()) and bool((w == 0).any()) and bool(torch.isfinite(w).all())
    ref = S.loss_eval(q, p, n, True, margin, scale, t)
    r32 = float(S.loss_measure(S.loss_eval(q, p, n, True, margin, scale, t, torch.float32)[0], ref).max())
    assert float(S.loss_measure(loss, ref).max()) <= S.loss_bound(r32, 70)


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
    from literalkg_amd import self_adversarial as sa
    for name in ("self_adversarial_loss", "sampled_sigmoid_loss", "group_sampled_batch"):
        assert name in L.__all__ and getattr(L, name) is getattr(sa, name)
    assert hasattr(L.LiteralKG, "calc_self_adversarial_loss")
    model = _stand_in()
    h, r, t = torch.tensor([0, 1, 2]), torch.tensor([0, 1, 2]), torch.tensor([3, 4, 5])
    neg = torch.tensor([[6, 7], [8, 9], [10, 11]])
    for kw, msg in ((dict(side="both"), "side must be one of"),
                    (dict(scoring="mlp"), "scoring='mlp' has no self-adversarial loss"),
                    (dict(reduction="max"), "reduction must be one of"), (dict(scale=0.0), "scale must be a positive"),
                    (dict(margin=float("inf")), "margin must be a finite number"),
                    (dict(margin=float("nan")), "margin must be a finite number"),
                    (dict(temperature=-0.5), "temperature must be a finite number >= 0"),
                    (dict(temperature=float("inf")), "temperature must be a finite number >= 0"),
                    (dict(temperature=True), "temperature must be a finite number >= 0"),
                    (dict(scoring="transr"), "needs a model with gat_trans_M")):
        with pytest.raises(ValueError, match=msg):
            sa.self_adversarial_loss(model, h, r, t, neg, **kw)
    with pytest.raises(ValueError, match="different lengths"):
        sa.self_adversarial_loss(model, h, r[:2], t, neg)
    for bad in (neg[:2], neg.reshape(-1), neg.float(), neg[:, :0], None):
        with pytest.raises(ValueError, match="neg must be a 2-D tensor of integer ids"):
            sa.self_adversarial_loss(model, h, r, t, bad)
    with pytest.raises(NotImplementedError, match="row-sharded"):
        sa.self_adversarial_loss(SimpleNamespace(local=model), h, r, t, neg)
    with pytest.raises(RuntimeError, match=DEVICE):                 # a CPU model: refused, the table never asked for
        sa.self_adversarial_loss(model, h, r, t, neg)
    empty = sa.self_adversarial_loss(model, h[:0], r[:0], t[:0], neg[:0], reduction="none")
    assert empty.shape == (0,) and empty.dtype == torch.float32
    assert sa.self_adversarial_loss(model, h[:0], r[:0], t[:0], neg[:0]).shape == ()
    from literalkg_amd.distributed import ShardedLiteralKG
    with pytest.raises(NotImplementedError, match="row-sharded"):
        ShardedLiteralKG.calc_self_adversarial_loss(None, h, r, t, neg)


def test_the_op_and_the_batch_helper_refuse_bad_arguments():
    from literalkg_amd import self_adversarial as sa
    q, p, n = torch.randn(3, 8), torch.randn(3, 8), torch.randn(6, 8)
    with pytest.raises(RuntimeError, match=DEVICE):
        sa.sampled_sigmoid_loss(q, p, n)
    for kw, msg in ((dict(scale=-1.0), "scale must be a positive"), (dict(margin="1"), "margin must be a finite number"),
                    (dict(temperature=-1.0), "temperature must be a finite number >= 0")):
        with pytest.raises(ValueError, match=msg):
            sa.sampled_sigmoid_loss(q, p, n, **kw)
    h = torch.tensor([0, 0, 1, 1])
    with pytest.raises(ValueError, match="neg_rate must be a positive integer"):
        sa.group_sampled_batch(h, h, h, h, 0)
    with pytest.raises(ValueError, match="not whole groups of 3"):
        sa.group_sampled_batch(h, h, h, h, 3)
    with pytest.raises(ValueError, match="different lengths"):
        sa.group_sampled_batch(h, h, h, h[:3], 2)
    gh, gr, gt, gn = sa.group_sampled_batch(h, h, h, torch.tensor([5, 6, 7, 8]), 1)      # K = 1: every row a group
    assert gh.tolist() == [0, 0, 1, 1] and gn.tolist() == [[5], [6], [7], [8]]


# ----------------------------------------------------------------------------- the entry points
NAMES = ["lkg_nssa_bwd_f32", "lkg_nssa_fwd_f32"]


def test_the_two_entry_points_are_declared_and_bound():
    import __graft_entry__ as ge
    ge.build()
    from literalkg_amd import _native, build
    from wide_cases import prototypes
    assert "lkg_nssa.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "lkg_nssa.hip"))
    assert set(NAMES) <= set(_native.PROTOTYPES) and set(NAMES) <= set(prototypes())


def _fwd(g=1, kn=2, k=4, ld=4, scale=1.0, temperature=1.0, margin=0.0):
    return (g, kn, k, None, ld, None, ld, None, ld, 1, margin, scale, temperature, None, None, None, None, None)


def _bwd(g=1, kn=2, k=4, ld=4, scale=1.0, out=None, ldo=4):
    return (g, kn, k, None, ld, None, ld, None, ld, 1, scale, None, None, None, None, out, ldo, None, ldo, None, ldo, None)


def test_error_convention_of_the_two_entry_points():
    import __graft_entry__ as ge
    ge.build()
    import numpy as np
    from literalkg_amd import _native
    call, E = _native.call, _native.LkgError
    for bad in (dict(kn=0), dict(k=0), dict(ld=3), dict(g=-1), dict(margin=float("nan"))):
        with pytest.raises(E, match="lkg_nssa_fwd_f32: bad sizes"):
            call("lkg_nssa_fwd_f32", *_fwd(**bad))
    with pytest.raises(E, match="lkg_nssa_fwd_f32: scale must be positive"):
        call("lkg_nssa_fwd_f32", *_fwd(scale=0.0))
    with pytest.raises(E, match="lkg_nssa_fwd_f32: temperature must not be negative"):
        call("lkg_nssa_fwd_f32", *_fwd(temperature=-1.0))
    with pytest.raises(E, match="lkg_nssa_fwd_f32: temperature must not be negative"):
        call("lkg_nssa_fwd_f32", *_fwd(temperature=float("nan")))
    with pytest.raises(E, match="lkg_nssa_fwd_f32: null pointer"):
        call("lkg_nssa_fwd_f32", *_fwd())
    call("lkg_nssa_fwd_f32", *_fwd(g=0))                                            # G = 0 returns before the pointer checks
    some = _native.ptr(np.zeros(8, np.float32))                                     # (never reached: the checks come first)
    for bad in (dict(kn=0), dict(k=0), dict(ld=3), dict(out=some, ldo=3)):
        with pytest.raises(E, match="lkg_nssa_bwd_f32: bad sizes"):
            call("lkg_nssa_bwd_f32", *_bwd(**bad))
    with pytest.raises(E, match="lkg_nssa_bwd_f32: scale must be positive"):
        call("lkg_nssa_bwd_f32", *_bwd(scale=-1.0))
    with pytest.raises(E, match="lkg_nssa_bwd_f32: null pointer"):
        call("lkg_nssa_bwd_f32", *_bwd(out=some))
    call("lkg_nssa_bwd_f32", *_bwd(g=0, out=some))
    call("lkg_nssa_bwd_f32", *_bwd())                                               # no gradient asked for: nothing to do
