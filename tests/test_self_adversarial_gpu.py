"""GPU, op level: lkg_nssa_fwd_f32 / lkg_nssa_bwd_f32 behind literalkg_amd.self_adversarial.sampled_sigmoid_loss against the
float64 references, measures and counted bounds of tests/self_adversarial_cases.py (which test_self_adversarial_host.py
shows to accept a float32 restatement of the kernels and to reject planted faults); the checks that have no tolerance (the
special weights, a group alone against the group in a batch, two runs, partial gradients, the two load paths); extreme
logits; and the bits under the perturbations of tests/invariance.py."""
import contextlib
import itertools

import pytest
import torch

import invariance as V
import self_adversarial_cases as S
import softmax_cases as C

pytestmark = pytest.mark.gpu

MODES = ("poison 0xFF", "poison 0x7F", "side stream + poison 0xFF")
NAMES = ("dq", "dp", "dn")


@pytest.fixture(scope="module")
def sa(gpu_device):
    import __graft_entry__ as ge
    ge.build()
    from literalkg_amd import self_adversarial
    return self_adversarial


def _on_device(dev, aligned, *rows):
    """the rows on the device with a row stride of a multiple of 4 floats (the 16-byte path where k allows it) or not
    (the scalar path)"""
    return [C.strided(x.to(dev), C.aligned_ld(x.shape[1]) if aligned else C.unaligned_ld(x.shape[1])) for x in rows]


def _run(sa, q, p, n, up, distance, margin, scale, temperature, needs=(True, True, True)):
    """(loss, [dq, dp, dn]) of the op with the upstream gradient up; a leaf that needs no gradient gets None"""
    leaves = [x.detach().requires_grad_(need) for x, need in zip((q, p, n), needs)]
    loss = sa.sampled_sigmoid_loss(*leaves, distance=distance, margin=margin, scale=scale, temperature=temperature)
    loss.backward(up)
    return loss.detach(), [x.grad for x in leaves]


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_loss_and_gradients_on_exact_logit_tables(sa, gpu_device, case):
    k, kn, g, aligned, distance, temperature = case
    q, p, n, margin, scale = S.exact_case(g, kn, k, distance, seed=k + 7 * kn + g, temperature=temperature)
    up = torch.rand((g,), generator=torch.Generator().manual_seed(k + kn)) + 0.5
    args = (distance, margin, scale, temperature)
    ref = S.loss_eval(q, p, n, *args)
    want = S.grads_eval(q, p, n, up, *args)
    auto64 = S.autograd_eval(q, p, n, up, *args, torch.float64)
    qd, pd, nd = _on_device(gpu_device, aligned, q, p, n)
    upd = up.to(gpu_device)
    loss, grads = _run(sa, qd, pd, nd, upd, *args)
    _, z_pos, z_neg, w = sa.sampled_sigmoid_forward(qd, pd, nd, *args)
    zp64, zn64 = S.logits(q, p, n, distance, margin, scale)
    assert torch.equal(z_pos.cpu().double(), zp64) and torch.equal(z_neg.cpu().double(), zn64.reshape(-1))     # exact logits
    if kn == 1:
        assert torch.equal(w, torch.ones_like(w))                                  # K = 1: w = 1.0 whatever the temperature
    if temperature == 0.0:
        assert torch.equal(w.cpu(), torch.full((g * kn,), 1.0 / kn, dtype=torch.float32))      # float32(1 / K)
    r32 = float(S.loss_measure(S.loss_eval(qd, pd, nd, *args, torch.float32)[0], ref).max())
    r, bound = float(S.loss_measure(loss, ref).max()), S.loss_bound(r32, kn)
    print(f"loss: r {r:.3g}, r_torch32 {r32:.3g}, bound {bound:.3g} ({S.loss_roundings(kn)} u)")
    assert r <= bound, (r, bound)
    auto32 = S.autograd_eval(qd, pd, nd, upd, *args, torch.float32)
    for name, got, a32, a64 in zip(NAMES, grads, auto32, auto64):
        scale64 = want[name + "_scale"]
        r32 = C.worst(a32.cpu(), want[name], scale64)
        bound = S.grad_bound(r32, kn, name)
        r, r_auto = C.worst(got.cpu(), want[name], scale64), C.worst(got.cpu(), a64, scale64)
        print(f"{name}: r {r:.3g} (autograd64 {r_auto:.3g}), r_torch32 {r32:.3g}, bound {bound:.3g} "
              f"({S.grad_roundings(kn, name)} u)")
        assert r <= bound and r_auto <= bound, (name, r, r_auto, bound)


@pytest.mark.parametrize("k,kn,aligned,distance", [(300, 65, True, True), (17, 5, False, False), (600, 3, True, False),
                                                   (64, 257, False, True)])
def test_a_group_alone_has_the_bits_it_has_in_a_batch_at_any_position(sa, gpu_device, k, kn, aligned, distance):
    g = 33
    q, p, n, up = S.random_case(g, kn, k, seed=k + kn)
    args = (distance, 0.5 * k, 0.37, 0.7)
    qd, pd, nd = _on_device(gpu_device, aligned, q, p, n)
    upd = up.to(gpu_device)
    loss, grads = _run(sa, qd, pd, nd, upd, *args)
    again_loss, again = _run(sa, qd, pd, nd, upd, *args)                           # two runs: the same bits
    assert V.same_bits(loss, again_loss, "loss, second run")
    for name, a, b in zip(NAMES, grads, again):
        assert V.same_bits(a, b, f"{name}, second run")
    for i in (0, 1, 16, 32):                                                       # a view of the batch's own rows
        one_loss, one = _run(sa, qd[i:i + 1], pd[i:i + 1], nd[i * kn:(i + 1) * kn], upd[i:i + 1], *args)
        assert V.same_bits(one_loss, loss[i:i + 1], f"loss of group {i} alone")
        for name, a, b in zip(NAMES, one, grads):
            rows = slice(i * kn, (i + 1) * kn) if name == "dn" else slice(i, i + 1)
            assert V.same_bits(a, b[rows], f"{name} of group {i} alone")
    perm = torch.randperm(g, generator=torch.Generator().manual_seed(1))
    rows = (perm[:, None] * kn + torch.arange(kn)[None, :]).reshape(-1)
    qs, ps, ns = _on_device(gpu_device, aligned, q[perm], p[perm], n[rows])
    moved_loss, moved = _run(sa, qs, ps, ns, upd[perm.to(gpu_device)], *args)      # every group at another position
    assert V.same_bits(moved_loss, loss[perm.to(gpu_device)], "loss, permuted")
    for name, a, b in zip(NAMES, moved, grads):
        assert V.same_bits(a, b[(rows if name == "dn" else perm).to(gpu_device)], f"{name}, permuted")
    # the 16-byte and the scalar path own the same columns in the same order: the same bits
    qo, po, no = _on_device(gpu_device, not aligned, q, p, n)
    other_loss, other = _run(sa, qo, po, no, upd, *args)
    assert V.same_bits(other_loss, loss, "loss, the other load path")
    for name, a, b in zip(NAMES, other, grads):
        assert V.same_bits(a, b, f"{name}, the other load path")


@pytest.mark.parametrize("distance", [True, False])
def test_partial_gradients_are_the_all_trainable_bits_or_none(sa, gpu_device, distance):
    q, p, n, up = (x.to(gpu_device) for x in S.random_case(33, 5, 300, seed=11))
    args = (distance, 150.0, 0.37, 0.7)
    full_loss, full = _run(sa, q, p, n, up, *args)
    assert all(x is not None for x in full)
    for needs in itertools.product((False, True), repeat=3):
        if not any(needs) or all(needs):
            continue
        loss, got = _run(sa, q, p, n, up, *args, needs=needs)
        assert V.same_bits(loss, full_loss, f"loss under {needs}")
        for name, need, a, c in zip(NAMES, needs, got, full):
            if need:
                assert V.same_bits(a, c, f"{name} under {needs}")
            else:
                assert a is None, (name, needs)


def test_extreme_logits_stay_finite_and_the_loss_within_its_bound(sa, gpu_device):
    q, p, n, margin, scale, temperature = S.extreme_case()
    args = (True, margin, scale, temperature)
    g, kn = q.shape[0], n.shape[0] // q.shape[0]
    ref = S.loss_eval(q, p, n, *args)
    qd, pd, nd = (x.to(gpu_device) for x in (q, p, n))
    loss, grads = _run(sa, qd, pd, nd, torch.ones(g, device=gpu_device), *args)
    _, z_pos, z_neg, w = sa.sampled_sigmoid_forward(qd, pd, nd, *args)
    assert float(z_neg.min()) < -200 and float(torch.cat((z_pos, z_neg)).max()) > 100
    assert bool((w == 0).any()) and bool((w.view(g, kn).sum(1) - 1).abs().max() < 1e-5)     # weights underflow, rows sum to 1
    for t in [loss, w] + grads:
        assert bool(torch.isfinite(t).all())
    r32 = float(S.loss_measure(S.loss_eval(qd, pd, nd, *args, torch.float32)[0], ref).max())
    r, bound = float(S.loss_measure(loss, ref).max()), S.loss_bound(r32, kn)
    print(f"loss: r {r:.3g}, r_torch32 {r32:.3g}, bound {bound:.3g}")
    assert r <= bound, (r, bound)


def test_empty_batch_and_shape_errors(sa, gpu_device):
    q = torch.zeros((0, 8), device=gpu_device, requires_grad=True)
    n = torch.zeros((0, 8), device=gpu_device, requires_grad=True)
    loss = sa.sampled_sigmoid_loss(q, q, n)
    assert loss.shape == (0,)
    loss.sum().backward()
    assert q.grad.shape == (0, 8) and n.grad.shape == (0, 8)
    rows = torch.zeros((3, 8), device=gpu_device)
    for bad in (torch.zeros((7, 8), device=gpu_device), torch.zeros((0, 8), device=gpu_device),
                torch.zeros((6, 4), device=gpu_device)):
        with pytest.raises(ValueError, match="sampled_sigmoid_loss: anchors"):
            sa.sampled_sigmoid_loss(rows, rows, bad)


# ----------------------------------------------------------------------------- the harness
@contextlib.contextmanager
def perturbation(mode):
    with contextlib.ExitStack() as stack:
        if mode == "side stream + poison 0xFF":
            stack.enter_context(V.side_stream())
        stack.enter_context(V.poisoned(0x7F if mode == "poison 0x7F" else 0xFF))
        yield
    torch.cuda.synchronize()


@pytest.mark.parametrize("distance", [True, False])
def test_entry_points_keep_their_bits_under_poison_and_on_a_side_stream(sa, gpu_device, distance):
    """lkg_nssa_fwd_f32 (its four outputs are uninitialised allocations) and lkg_nssa_bwd_f32 through the whole backward
    (dq, dp, dn), on both load paths and with one gradient left out."""
    q, p, n, up = S.random_case(33, 65, 300, seed=41)
    up = up.to(gpu_device)
    rows = [_on_device(gpu_device, aligned, q, p, n) for aligned in (True, False)]
    args = (distance, 150.0, 0.37, 0.7)

    def run():
        out = []
        for qd, pd, nd in rows:
            out += list(sa.sampled_sigmoid_forward(qd, pd, nd, *args))
            loss, grads = _run(sa, qd, pd, nd, up, *args)
            out += [loss] + grads
            out += [x for x in _run(sa, qd, pd, nd, up, *args, needs=(True, False, True))[1] if x is not None]
        return out

    plain = run()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in plain)
    for mode in MODES:
        with perturbation(mode):
            got = run()
        for j, (a, c) in enumerate(zip(plain, got)):
            assert V.same_bits(a, c, f"{mode}, result {j}")
