"""GPU: what the closed lists of test_invariance_gpu.py and tests/autograd_cases.py give the other entry points and
Functions, written out for the KvsAll ones (their entry points are in ELSEWHERE of that ledger, their Function in
literalkg_amd/kvs_all.py): every new entry point gives the same bits under the perturbations of tests/invariance.py
(poisoned scratch of either byte, a side stream behind the host with poisoned scratch), and the Function under every
non-empty subset of {q, p, bias} requiring grad gives the needed gradients with the bits of the all-trainable run and None
for the others."""
import contextlib
import itertools

import pytest
import torch

import invariance as V
import kvs_all_cases as K

pytestmark = pytest.mark.gpu

MODES = ("poison 0xFF", "poison 0x7F", "side stream + poison 0xFF")


@pytest.fixture(scope="module")
def kv(gpu_device):
    import __graft_entry__ as ge
    ge.build()
    from literalkg_amd import kvs_all
    return kvs_all


@contextlib.contextmanager
def perturbation(mode):
    with contextlib.ExitStack() as stack:
        if mode == "side stream + poison 0xFF":
            stack.enter_context(V.side_stream())
        stack.enter_context(V.poisoned(0x7F if mode == "poison 0x7F" else 0xFF))
        yield
    torch.cuda.synchronize()


def _case(dev, b=130, n=1100, k=17):
    q, p, bias, g = (x.to(dev) for x in K.random_case(b, n, k, seed=41))
    return q, p, bias, g, K.to_lists(K.patterns(b, n, seed=6), dev)


@pytest.mark.parametrize("distance", [True, False])
def test_entry_points_keep_their_bits_under_poison_and_on_a_side_stream(kv, gpu_device, distance):
    """lkg_sigmoid_all_partial_f32 + lkg_sigmoid_all_finish_f32 (the forward pass: its workspace and its result are
    uninitialised allocations), lkg_sigmoid_all_weights_f32 (its output), and the whole backward loop (V's buffer, the
    tiles' row sums, the dP chunks)."""
    from literalkg_amd import ops
    q, p, bias, g, pos = _case(gpu_device)

    def run():
        pn = ops.rank_sqnorm(p) if distance else None
        out = [kv.sigmoid_all_forward(q, p, pn, bias, pos, 0.37, 0.1, s) for s in (1, 2, 5)]
        out.append(kv.sigmoid_all_weights(q, p, pn, bias, g, pos, 0.37, 0.1))
        out.append(kv.sigmoid_all_weights(q, p, pn, bias, g, pos, 0.37, 0.1, 256, 700))
        q_, p_, b_ = (x.clone().requires_grad_(True) for x in (q, p, bias))
        loss = kv.sigmoid_all_loss(q_, p_, b_, pos, distance=distance, scale=0.37, label_smoothing=0.1,
                                   chunk_bytes=4 * 130 * 512)
        loss.backward(g)
        return out + [loss.detach(), q_.grad, p_.grad, b_.grad]

    plain = run()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in plain)
    for mode in MODES:
        with perturbation(mode):
            got = run()
        for j, (a, c) in enumerate(zip(plain, got)):
            assert V.same_bits(a, c, f"{mode}, result {j}")


@pytest.mark.parametrize("distance", [True, False])
def test_partial_gradients_are_the_all_trainable_bits_or_none(kv, gpu_device, distance):
    q, p, bias, g, pos = _case(gpu_device)

    def grads(needs):
        leaves = [x.clone().requires_grad_(need) for x, need in zip((q, p, bias), needs)]
        loss = kv.sigmoid_all_loss(*leaves, pos, distance=distance, scale=0.37, label_smoothing=0.1,
                                   chunk_bytes=4 * 130 * 512)
        loss.backward(g)
        return loss.detach(), [x.grad for x in leaves]

    full_loss, full = grads((True, True, True))
    assert all(x is not None for x in full)
    for needs in itertools.product((False, True), repeat=3):
        if not any(needs) or all(needs):
            continue
        loss, got = grads(needs)
        assert V.same_bits(loss, full_loss, f"loss under {needs}")
        for name, need, a, c in zip(("dq", "dp", "dbias"), needs, got, full):
            if need:
                assert V.same_bits(a, c, f"{name} under {needs}")
            else:
                assert a is None, (name, needs)


def test_unneeded_products_are_not_launched(kv, gpu_device, monkeypatch):
    """needs_input_grad decides what runs: with only bias trainable no product runs at all (the row sums come from the
    weights kernel), with only p trainable the dQ product does not, with only q trainable the dP product does not (counted
    at ops.gemm)."""
    from literalkg_amd import ops
    q, p, bias, g, pos = _case(gpu_device)
    seen = []
    real = ops.gemm

    def counting(a, b, **kw):
        seen.append(bool(kw.get("trans_a", False)))
        return real(a, b, **kw)
    monkeypatch.setattr(ops, "gemm", counting)
    for needs, want in (((False, False, True), set()), ((False, True, False), {True}), ((True, False, False), {False}),
                        ((True, True, True), {True, False})):
        seen.clear()
        leaves = [x.clone().requires_grad_(need) for x, need in zip((q, p, bias), needs)]
        kv.sigmoid_all_loss(*leaves, pos, scale=0.37).backward(g)
        assert set(seen) == want, (needs, seen)
