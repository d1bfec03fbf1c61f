"""The three training losses under products="ordered" (literalkg_amd/gemm_ordered.py: their long reductions on the ordered
split-K GEMM instead of ops.gemm in slices).  Cases and float64 references are those of softmax_cases.py, kvs_all_cases.py
and relation_loss_cases.py.

  the loss and every gradient whose product did not move keep the bits of the "engine" route
  the gradients that did move (dq; slab mode's dd; shared mode's de) are held per element to the float64 reference under
      bound_for("f32_mfma", r_torch32, per + s_eff) of the product that ran
  everything repeats bit for bit
  a Function follows the route its forward ran under, wherever backward() is called
  at model level every parameter's gradient is within 1e-4 of the parameter's largest entry of the dense torch head"""
import importlib
import math

import pytest
import torch

import invariance as V
import kvs_all_cases as K
import op_audit as OA
import relation_loss_cases as RC
import softmax_cases as C

pytestmark = pytest.mark.gpu

N = 9001
WIDTH = 4608                                   # candidates per chunk: two chunks of N, each wider than one SOFTMAX_DQ_SLICE


@pytest.fixture(scope="module")
def L(gpu_device):
    import __graft_entry__ as ge
    ge.build()
    import literalkg_amd
    return literalkg_amd


@pytest.fixture(scope="module")
def ops(L):
    from literalkg_amd import ops
    return ops


@pytest.fixture(scope="module")
def GO(L):
    return importlib.import_module("literalkg_amd.gemm_ordered")


@pytest.fixture(scope="module")
def rl(L):
    return importlib.import_module("literalkg_amd.relation_loss")


def sliced_chain(GO, k, max_chain):
    """per + s_eff of the product accumulate_ordered runs over a reduction of k with slices of at most max_chain"""
    f = max(16, max_chain // 16 * 16)
    s_eff, per = GO.partition(k, max(1, -(-k // f)))
    assert per <= max_chain or max_chain < 16
    return per + s_eff


# ----------------------------------------------------------------------------- 1-vs-all
def _softmax(ops, q, p, truth, g, distance, scale, b, **kw):
    q_, p_ = q.clone().requires_grad_(True), p.clone().requires_grad_(True)
    loss = ops.softmax_all_loss(q_, p_, truth, distance=distance, scale=scale, chunk_bytes=4 * b * WIDTH, **kw)
    loss.backward(g)
    return loss.detach(), q_.grad, p_.grad


@pytest.mark.parametrize("k", [20, 300])
@pytest.mark.parametrize("b", [1, 5, 130])
def test_one_vs_all_under_the_ordered_route(ops, GO, gpu_device, b, k):
    q, p, truth, g = (x.to(gpu_device) for x in C.random_tables(b, N, k, seed=b + k, std=0.5 if k < 100 else 0.2))
    assert math.ceil(N / ops.softmax_chunk_width(b, N, 4 * b * WIDTH)) == 2
    chain = max(sliced_chain(GO, w, ops.SOFTMAX_DQ_SLICE) for w in (WIDTH, N - WIDTH))
    for distance, scale in ((True, 0.37), (False, 1.7)):
        ref = C.grads_eval(q, p, truth, g, distance, scale)
        rq32 = C.worst(C.autograd_eval(q, p, truth, g, distance, scale, torch.float32)[0], ref["dq"], ref["dq_scale"])
        loss_e, dq_e, dp_e = _softmax(ops, q, p, truth, g, distance, scale, b)
        loss_o, dq_o, dp_o = _softmax(ops, q, p, truth, g, distance, scale, b, products="ordered")
        V.same_bits(loss_o, loss_e, "loss")
        V.same_bits(dp_o, dp_e, "dP")
        bound = OA.bound_for("f32_mfma", rq32, chain)
        r = C.worst(dq_o, ref["dq"], ref["dq_scale"])
        print(f"b {b} k {k} distance {distance}: dq r {r:.3g} (engine route {C.worst(dq_e, ref['dq'], ref['dq_scale']):.3g}), "
              f"torch32 {rq32:.3g}, bound {bound:.3g}")
        assert r <= bound, (distance, r, bound)
        for run in range(2):
            again = _softmax(ops, q, p, truth, g, distance, scale, b, products="ordered")
            for a, o, what in zip(again, (loss_o, dq_o, dp_o), ("loss", "dQ", "dP")):
                V.same_bits(a, o, f"{what}, run {run + 2}")


# ----------------------------------------------------------------------------- KvsAll
def _sigmoid(kv, q, p, bias, lists, g, distance, scale, eps, b, **kw):
    q_, p_, b_ = (x.clone().requires_grad_(True) for x in (q, p, bias))
    loss = kv.sigmoid_all_loss(q_, p_, b_, lists, distance=distance, scale=scale, label_smoothing=eps,
                               chunk_bytes=4 * b * WIDTH, **kw)
    loss.backward(g)
    return loss.detach(), q_.grad, p_.grad, b_.grad


@pytest.mark.parametrize("k", [20, 300])
@pytest.mark.parametrize("b", [1, 5, 130])
def test_kvs_all_under_the_ordered_route(L, GO, ops, gpu_device, b, k):
    kv = importlib.import_module("literalkg_amd.kvs_all")
    dev = gpu_device
    q, p, bias, g = (x.to(dev) for x in K.random_case(b, N, k, seed=2 * b + k, std=0.5 if k < 100 else 0.2))
    rows = K.patterns(b, N, seed=b)
    lists, mask = K.to_lists(rows, dev), K.mask_of(rows, N, dev)
    chain = max(sliced_chain(GO, w, ops.SOFTMAX_DQ_SLICE) for w in (WIDTH, N - WIDTH))
    for distance, scale, eps in ((True, 0.37, 0.1), (False, 1.7, 0.0)):
        ref = K.grads_eval(q, p, bias, mask, g, distance, scale, eps)
        rq32 = C.worst(K.autograd_eval(q, p, bias, mask, g, distance, scale, eps, torch.float32)[0], ref["dq"], ref["dq_scale"])
        eng = _sigmoid(kv, q, p, bias, lists, g, distance, scale, eps, b)
        ordr = _sigmoid(kv, q, p, bias, lists, g, distance, scale, eps, b, products="ordered")
        for j, what in ((0, "loss"), (2, "dP"), (3, "dbias")):
            V.same_bits(ordr[j], eng[j], what)
        bound = OA.bound_for("f32_mfma", rq32, chain)
        r = C.worst(ordr[1], ref["dq"], ref["dq_scale"])
        print(f"b {b} k {k} distance {distance}: dq r {r:.3g} (engine route {C.worst(eng[1], ref['dq'], ref['dq_scale']):.3g}), "
              f"torch32 {rq32:.3g}, bound {bound:.3g}")
        assert r <= bound, (distance, r, bound)
        for run in range(2):
            again = _sigmoid(kv, q, p, bias, lists, g, distance, scale, eps, b, products="ordered")
            for a, o, what in zip(again, ordr, ("loss", "dQ", "dP", "dbias")):
                V.same_bits(a, o, f"{what}, run {run + 2}")


# ----------------------------------------------------------------------------- relation loss
def _relation(rl, dev, case, chunk_bytes, **kw):
    leaves = [None if x is None else x.to(dev).detach().requires_grad_(True) for x in (case["d"], case["w"], case["e"])]
    loss = rl.relation_softmax_loss(*leaves, case["truth"].to(dev), scale=case["scale"], chunk_bytes=chunk_bytes, **kw)
    loss.backward(case["g"].to(dev))
    return loss.detach(), [None if x is None else x.grad for x in leaves]


@pytest.mark.parametrize("shared", [False, True], ids=["slab", "shared"])
@pytest.mark.parametrize("k", [20, 128])
@pytest.mark.parametrize("n_rel", [1, 3, 17])
@pytest.mark.parametrize("p", [1, 5, 130])
def test_relation_loss_under_the_ordered_route(rl, GO, gpu_device, p, n_rel, k, shared):
    """On exact-logit cases, as the op's own gradient test: what is measured is then the products."""
    dev = gpu_device
    case = RC.exact_case(p, n_rel, k, None if shared else "D", seed=p + n_rel + k)
    case["g"] = RC.upstream(p, k)
    d, w, e, truth, scale, g = (case[x] for x in ("d", "w", "e", "truth", "scale", "g"))
    rows = -(-p // 2)                                              # two chunks of pairs in slab mode (one pair: one)
    chunk_bytes = rows * n_rel * k * 4
    if not shared:
        assert rl.chunk_rows(p, n_rel, k, chunk_bytes) == rows
    want = RC.grads_eval(RC.slab_of(d, w, n_rel), d, w, e, truth, None, scale, g)
    a32 = RC.autograd_eval(d.to(dev), None if shared else w.to(dev), e.to(dev), truth.to(dev), None, scale, g.to(dev),
                           torch.float32)
    loss_e, grads_e = _relation(rl, dev, case, chunk_bytes)
    loss_o, grads_o = _relation(rl, dev, case, chunk_bytes, products="ordered")
    V.same_bits(loss_o, loss_e, "loss")
    if shared:
        moved, name, x32 = 2, "de", a32[2]
        s_eff, per = GO.partition(p, GO.gemm_ordered_splits(n_rel, k + 1, p, True, False))
        chain = per + s_eff
        V.same_bits(grads_o[0], grads_e[0], "dd (the kernel's own)")
        assert grads_o[1] is None and grads_e[1] is None
    else:
        moved, name, x32 = 0, "dd", a32[0]
        chain = sliced_chain(GO, n_rel * k, max(1, rl.DD_SLICE // k) * k)
        V.same_bits(grads_o[1], grads_e[1], "dW")
        V.same_bits(grads_o[2], grads_e[2], "de")
    r32 = C.worst(x32.cpu(), want[name], want[name + "_scale"])
    bound = OA.bound_for("f32_mfma", r32, chain)
    r = C.worst(grads_o[moved].cpu(), want[name], want[name + "_scale"])
    print(f"p {p} R {n_rel} k {k} {'shared' if shared else 'slab'}: {name} r {r:.3g}, torch32 {r32:.3g}, bound {bound:.3g}")
    assert r <= bound, (name, r, bound)
    for run in range(2):
        loss_a, grads_a = _relation(rl, dev, case, chunk_bytes, products="ordered")
        V.same_bits(loss_a, loss_o, f"loss, run {run + 2}")
        for j, (a, o) in enumerate(zip(grads_a, grads_o)):
            if o is not None:
                V.same_bits(a, o, f"gradient {j}, run {run + 2}")


# ----------------------------------------------------------------------------- the route is the forward's
def _both_ways(GO, forward, leaves_of):
    """gradients with (forward inside "ordered", backward outside), (forward outside, backward inside), and under the
    explicit keyword of either route"""
    out = {}
    for name, fwd_route, bwd_route, kw in (("ordered kept", "ordered", "engine", {}), ("engine kept", "engine", "ordered", {}),
                                           ("ordered", "engine", "engine", dict(products="ordered")),
                                           ("engine", "engine", "engine", dict(products="engine"))):
        leaves = leaves_of()
        with GO.product_route(fwd_route):
            loss, g = forward(leaves, kw)
        with GO.product_route(bwd_route):
            loss.backward(g)
        out[name] = [x.grad for x in leaves if x is not None]
    return out


def _assert_routes(out, moved):
    for a, b in zip(out["ordered kept"], out["ordered"]):
        V.same_bits(a, b, "forward inside product_route('ordered'), backward outside")
    for a, b in zip(out["engine kept"], out["engine"]):
        V.same_bits(a, b, "forward outside, backward inside product_route('ordered')")
    assert not torch.equal(out["ordered"][moved], out["engine"][moved])     # (the two routes do differ on these operands)


def test_backward_follows_the_route_of_the_forward(ops, GO, rl, gpu_device):
    dev = gpu_device
    b, k = 130, 20
    q, p, truth, g = (x.to(dev) for x in C.random_tables(b, N, k, seed=1))
    out = _both_ways(GO, lambda lv, kw: (ops.softmax_all_loss(lv[0], lv[1], truth, scale=0.37, chunk_bytes=4 * b * WIDTH, **kw), g),
                     lambda: [q.clone().requires_grad_(True), p.clone().requires_grad_(True)])
    _assert_routes(out, 0)
    kv = importlib.import_module("literalkg_amd.kvs_all")
    q, p, bias, g = (x.to(dev) for x in K.random_case(b, N, k, seed=2))
    lists = K.to_lists(K.patterns(b, N, seed=3), dev)
    out = _both_ways(GO, lambda lv, kw: (kv.sigmoid_all_loss(lv[0], lv[1], lv[2], lists, scale=0.37, chunk_bytes=4 * b * WIDTH, **kw), g),
                     lambda: [x.clone().requires_grad_(True) for x in (q, p, bias)])
    _assert_routes(out, 0)
    # slab mode: dd, over R k = 5120 columns (two slices on either route); shared mode: de (w is absent), over 1100 pairs
    # (two splits) -- shapes at which the routes run different chains, so that taking the wrong one shows
    for c, moved, p_, n_rel in (("D", 0, 130, 40), (None, 1, 1100, 17)):
        case = RC.random_case(p_, n_rel, 128, c, seed=4)
        truth = case["truth"].to(dev)
        out = _both_ways(GO, lambda lv, kw: (rl.relation_softmax_loss(*lv, truth, scale=case["scale"], **kw), case["g"].to(dev)),
                         lambda: [None if x is None else x.to(dev).requires_grad_(True) for x in (case["d"], case["w"], case["e"])])
        _assert_routes(out, moved)


# ----------------------------------------------------------------------------- model level
def _grads(model):
    return {k: (v.grad.to_dense() if v.grad.is_sparse else v.grad).clone() for k, v in model.named_parameters() if v.grad is not None}


def _assert_within_1e4(got, want):
    assert set(got) == set(want) and "entity_embed.weight" in got
    for name, w in want.items():
        tol = 1e-4 * float(w.abs().max())
        assert float((got[name] - w).abs().max()) <= tol, (name, float((got[name] - w).abs().max()), tol)


@pytest.mark.parametrize("scoring", ["transe", "dot", "transr"])
def test_model_one_vs_all_gradients_under_the_ordered_route(L, gpu_device, scoring):
    import test_one_vs_all_gpu as T
    model, (h, r, t) = T._synthetic_model(L, gpu_device, scoring)
    model.train()
    bh, br, bt = h[:70], r[:70], t[:70]
    model.zero_grad()
    loss = model.calc_one_vs_all_loss(bh, br, bt, side="both", scale=0.8, scoring=scoring, products="ordered")
    loss.backward()
    got = _grads(model)
    model.zero_grad()
    want_loss = T._dense_head(model, scoring, "both", bh, br, bt, 0.8)[0].mean()
    want_loss.backward()
    assert abs(float(loss) - float(want_loss)) <= 1e-4 * max(1.0, abs(float(want_loss)))
    _assert_within_1e4(got, _grads(model))
    with pytest.raises(ValueError, match="products"):
        model.calc_one_vs_all_loss(bh, br, bt, products="atomic")


@pytest.mark.parametrize("scoring,side", [("transe", "tail"), ("transr", "head"), ("dot", "tail")])
def test_model_kvs_all_gradients_under_the_ordered_route(L, gpu_device, scoring, side):
    import test_kvs_all_gpu as T
    kv = importlib.import_module("literalkg_amd.kvs_all")
    n = 600
    model, (h, r, t) = T._synthetic_model(L, gpu_device, scoring)
    known = L.KnownTriples(h, r, t, n, 5)
    model.train()
    ent, rel = kv.distinct_queries(h[:80] if side == "tail" else t[:80], r[:80])
    margin, scale, eps = 6.0, 0.5, 0.1
    model.zero_grad()
    loss = model.calc_kvs_all_loss(ent, rel, known, side=side, margin=margin, scale=scale, label_smoothing=eps, scoring=scoring,
                                   products="ordered")
    loss.backward()
    got = _grads(model)
    y = T._multi_hot(h, r, t, ent, rel, side, scoring == "dot", n)
    model.zero_grad()
    want_loss = T._dense_head(model, scoring, side, ent, rel, y, margin, scale, eps, None)
    want_loss.backward()
    assert abs(float(loss) - float(want_loss)) <= 1e-4 * max(1.0, abs(float(want_loss)))
    _assert_within_1e4(got, _grads(model))


@pytest.mark.parametrize("scoring", ["transe", "transr"])
def test_model_relation_loss_gradients_under_the_ordered_route(L, gpu_device, scoring):
    import test_relation_loss_model_gpu as T
    model, (kh, kr, kt) = T._synthetic_model(L, gpu_device, scoring)
    model.train()
    h, t = torch.cat((kh[:80], kh[80:100])), torch.cat((kt[:80], kt[80:100]))
    r = torch.cat((kr[:80], (kr[80:100] + 1) % T.N_REL))
    known = L.KnownTriples(kh, kr, kt, T.N_ENT, T.N_REL)
    mask = RC.dropped_mask(kh.cpu(), kr.cpu(), kt.cpu(), h.cpu(), r.cpu(), t.cpu(), T.N_REL).to(gpu_device)
    model.zero_grad()
    loss = model.calc_relation_loss(h, r, t, known=known, scale=0.5, products="ordered")
    loss.backward()
    got = _grads(model)
    model.zero_grad()
    want_rows = T._dense_head(model, scoring, h, r, t, mask, 0.5)
    want_rows.mean().backward()
    want_loss = float(want_rows.mean().detach())
    assert abs(float(loss.detach()) - want_loss) <= 1e-4 * max(1.0, abs(want_loss))
    _assert_within_1e4(got, _grads(model))
    assert ("gat_trans_M" in got) == (scoring == "transr")
