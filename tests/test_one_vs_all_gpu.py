"""GPU: the 1-vs-all loss (lkg_softmax.hip, ops.softmax_all_loss, literalkg_amd/one_vs_all.py) against float64.

References, measures and bounds live in tests/softmax_cases.py (test_softmax_measures_host.py shows on the CPU that they
accept a correct float32 evaluation and reject planted faults).  Loss: per query r = |loss - loss64| / (|lse64| + |z_t|)
<= max(3 r_torch32, 3e-7) on tables whose logits are exact in float32.  No allowance for the kernel's exp was needed: it is
the library expf (1 ulp), the same as torch's.  Gradients: per element against float64 autograd, with the bound of the
engine ops.gemm ran the product on."""
import math

import pytest
import torch

import softmax_cases as C

pytestmark = pytest.mark.gpu


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


def _layouts(q, p, k):
    """(name, q, p): contiguous rows, 16-byte aligned padded rows, rows off the 16-byte grid"""
    yield "contiguous", q, p
    yield "aligned", C.strided(q, C.aligned_ld(k)), C.strided(p, C.aligned_ld(k))
    yield "unaligned", C.strided(q, C.unaligned_ld(k)), C.strided(p, C.unaligned_ld(k))


# ----------------------------------------------------------------------------- 1. exact-logit tables
@pytest.mark.parametrize("b,n,k", C.shapes((1, 3, 4, 16, 17, 300)))
def test_loss_on_exact_logit_tables(ops, gpu_device, b, n, k):
    q, p, truth = (x.to(gpu_device) for x in C.integer_tables(b, n, k, seed=7 * b + n + k))
    scale = C.exact_scale(k)
    s_max = ops.softmax_all_splits(b, n, ops.SOFTMAX_MAX_SPLITS)
    for distance in (True, False):
        ref = C.loss_eval(q, p, truth, distance, scale)                   # float64 of integer scores: exact logits
        lse32, zt32, loss32 = C.loss_eval(q, p, truth, distance, scale, torch.float32)
        assert torch.equal(zt32.double(), ref[1])                         # the logits ARE exact in float32
        bound = C.loss_bound(float(C.loss_measure(loss32, ref).max()))
        pn = ops.rank_sqnorm(p) if distance else None
        for name, q_, p_ in _layouts(q, p, k):
            for splits in sorted({1, min(2, s_max), s_max}):
                lse, loss = ops.softmax_all_forward(q_, p_, pn, truth, scale, splits)
                r = float(C.loss_measure(loss, ref).max())
                print(f"b {b} n {n} k {k} distance {distance} {name} S {splits}: r {r:.3g} bound {bound:.3g}")
                assert r <= bound, (distance, name, splits, r, bound)
                r_lse = float(((lse[0].double() + lse[1].double() - ref[0]).abs()
                               / (ref[0].abs() + ref[1].abs() + 1e-300)).max())
                assert r_lse <= bound, (distance, name, splits, r_lse)    # lse and its remainder: the float64 value


# ----------------------------------------------------------------------------- 2. sharp cases
@pytest.mark.parametrize("distance", [True, False])
def test_one_candidate_gives_exactly_zero(ops, gpu_device, distance):
    """N = 1: loss = z - z_t is 0.0 only if the truth's logit has the bits it has inside a tile; softmax = 1 exactly, so
    every weight and every gradient is exactly 0."""
    for b, k in ((1, 1), (65, 17), (130, 300)):
        gen = torch.Generator().manual_seed(b + k)
        q = (torch.randn((b, k), generator=gen) * 3).to(gpu_device).requires_grad_(True)
        p = (torch.randn((1, k), generator=gen) * 3).to(gpu_device).requires_grad_(True)
        truth = torch.zeros(b, dtype=torch.int64, device=gpu_device)
        loss = ops.softmax_all_loss(q, p, truth, distance=distance, scale=0.7)
        assert torch.equal(loss, torch.zeros_like(loss)), loss
        loss.backward(torch.rand(b, device=gpu_device) + 0.5)
        assert torch.equal(q.grad, torch.zeros_like(q)) and torch.equal(p.grad, torch.zeros_like(p))


@pytest.mark.parametrize("n", [255, 257, 70001])
def test_equal_candidates_give_log_n(ops, gpu_device, n):
    gen = torch.Generator().manual_seed(n)
    q = torch.randn((65, 17), generator=gen).to(gpu_device)
    p = torch.randn((1, 17), generator=gen).to(gpu_device).expand(n, 17).contiguous()
    truth = C.truths(65, n, gen).to(gpu_device)
    for distance in (True, False):
        ref = C.loss_eval(q, p, truth, distance, 0.5)
        loss = ops.softmax_all_loss(q, p, truth, distance=distance, scale=0.5)
        r32 = float(C.loss_measure(C.loss_eval(q, p, truth, distance, 0.5, torch.float32)[2], ref).max())
        assert float(C.loss_measure(loss, ref).max()) <= C.loss_bound(r32)
        scale_ = ref[0].abs() + ref[1].abs()
        assert bool(((loss.double() - math.log(n)).abs() <= C.loss_bound(r32) * scale_ + 1e-12).all())


def test_wide_logit_spread_underflows_quietly(ops, gpu_device):
    """Logits more than 200 apart: the far terms underflow to 0, nothing is NaN or inf, and a query whose truth is its own
    row among far candidates has a loss of about 0."""
    gen = torch.Generator().manual_seed(3)
    b, n, k = 65, 1000, 16
    p = (torch.randn((n, k), generator=gen) * 8).to(gpu_device)
    q = p[:b].clone()
    truth = torch.arange(b, device=gpu_device)
    z = C.logits(q, p, True, 1.0)
    assert float((z.max(1).values - z.min(1).values).min()) > 200
    q_ = q.clone().requires_grad_(True)
    p_ = p.clone().requires_grad_(True)
    loss = ops.softmax_all_loss(q_, p_, truth, distance=True, scale=1.0)
    loss.sum().backward()
    for t_ in (loss, q_.grad, p_.grad):
        assert bool(torch.isfinite(t_).all())
    ref = C.loss_eval(q, p, truth, True, 1.0)
    assert float(loss.abs().max()) <= 1e-6 and float(ref[2].abs().max()) <= 1e-6
    # and a truth FAR from the query: a large finite loss, still within the bound
    far = truth.flip(0) + 500
    ref = C.loss_eval(q, p, far, True, 1.0)
    r32 = float(C.loss_measure(C.loss_eval(q, p, far, True, 1.0, torch.float32)[2], ref).max())
    loss = ops.softmax_all_loss(q, p, far, distance=True, scale=1.0)
    assert float(ref[2].min()) > 200 and float(C.loss_measure(loss, ref).max()) <= C.loss_bound(r32)


def test_nan_query_poisons_its_own_row_only(ops, gpu_device):
    q, p, truth, g = (x.to(gpu_device) for x in C.random_tables(130, 1000, 17, seed=9))
    q[70, 5] = float("nan")
    q_ = q.clone().requires_grad_(True)
    p_ = p.clone().requires_grad_(True)
    loss = ops.softmax_all_loss(q_, p_, truth, splits=2)
    bad = torch.isnan(loss)
    assert bad.tolist() == [i == 70 for i in range(130)]
    g[70] = 0.0                                   # (an upstream 0 does not unpoison the row: 0 * NaN)
    loss.backward(g)
    rows = torch.isnan(q_.grad).any(1)
    assert rows.tolist() == [i == 70 for i in range(130)]


def test_two_runs_give_the_same_bits(ops, gpu_device):
    q, p, truth, g = (x.to(gpu_device) for x in C.random_tables(130, 70001, 300, seed=11))
    outs = []
    for _ in range(2):
        q_ = q.clone().requires_grad_(True)
        p_ = p.clone().requires_grad_(True)
        loss = ops.softmax_all_loss(q_, p_, truth, scale=0.25, chunk_bytes=130 * 4 * 20000)
        loss.backward(g)
        outs.append((loss.detach(), q_.grad, p_.grad))
    for a, b_ in zip(*outs):
        assert torch.equal(a, b_)


# ----------------------------------------------------------------------------- 3. gradients
def _engines(ops, q, p, b, n, k, width, distance=True):
    """the engines ops.gemm runs the backward's two products on (as the op does: alpha 2, beta 1, onto an output; dQ in
    slices of SOFTMAX_DQ_SLICE candidates, dP with the column of ones that carries colsum V when there is a norm term)"""
    dev = q.device
    w = min(width, n)
    v = torch.empty((b, w), device=dev)
    ws = min(w, ops.SOFTMAX_DQ_SLICE)
    e_q = ops.gemm_engine(v[:, :ws], p[:ws], alpha=2.0, beta=1.0, out=torch.empty((b, k), device=dev))
    kq = k + 1 if distance else k
    e_p = ops.gemm_engine(v, torch.empty((b, kq), device=dev), trans_a=True, alpha=2.0, beta=1.0,
                          out=torch.empty((w, kq), device=dev))
    return e_q, e_p


@pytest.mark.parametrize("b,n,k", C.shapes((3, 17, 300)))
def test_gradients_against_float64_autograd(ops, gpu_device, b, n, k):
    q, p, truth, g = (x.to(gpu_device) for x in C.random_tables(b, n, k, seed=3 * b + n + k, std=0.5 if k < 100 else 0.2))
    for distance, scale in ((True, 1.0), (False, 1.0), (True, 0.37), (False, 1.7)):
        ref = C.grads_eval(q, p, truth, g, distance, scale)
        dq32, dp32 = C.autograd_eval(q, p, truth, g, distance, scale, torch.float32)
        rq32, rp32 = C.worst(dq32, ref["dq"], ref["dq_scale"]), C.worst(dp32, ref["dp"], ref["dp_scale"])
        e_q, e_p = _engines(ops, q, p, b, n, k, ops.softmax_chunk_width(b, n), distance)
        bq, bp = C.gemm_bound(e_q, rq32, n), C.gemm_bound(e_p, rp32, b)
        q_ = q.clone().requires_grad_(True)
        p_ = p.clone().requires_grad_(True)
        ops.softmax_all_loss(q_, p_, truth, distance=distance, scale=scale).backward(g)
        rq, rp = C.worst(q_.grad, ref["dq"], ref["dq_scale"]), C.worst(p_.grad, ref["dp"], ref["dp_scale"])
        print(f"b {b} n {n} k {k} distance {distance} scale {scale}: dq r {rq:.3g} bound {bq:.3g} [{e_q}, torch32 "
              f"{rq32:.3g}]  dp r {rp:.3g} bound {bp:.3g} [{e_p}, torch32 {rp32:.3g}]")
        assert rq <= bq, ("dq", distance, scale, rq, bq, e_q)
        assert rp <= bp, ("dp", distance, scale, rp, bp, e_p)


@pytest.mark.parametrize("distance", [True, False])
def test_chunking_keeps_dp_bits_and_v_rows_sum_to_zero(ops, gpu_device, distance):
    b, n, k = 130, 1100, 17
    q, p, truth, g = (x.to(gpu_device) for x in C.random_tables(b, n, k, seed=21))
    ref = C.grads_eval(q, p, truth, g, distance, 0.37)
    grads = []
    for n_chunks, width in ((1, 1280), (2, 768), (5, 256)):
        assert math.ceil(n / ops.softmax_chunk_width(b, n, 4 * b * width)) == n_chunks
        q_ = q.clone().requires_grad_(True)
        p_ = p.clone().requires_grad_(True)
        ops.softmax_all_loss(q_, p_, truth, distance=distance, scale=0.37, chunk_bytes=4 * b * width).backward(g)
        grads.append((q_.grad, p_.grad))
        e_q, _ = _engines(ops, q, p, b, n, k, width, distance)
        rq32 = C.worst(C.autograd_eval(q, p, truth, g, distance, 0.37, torch.float32)[0], ref["dq"], ref["dq_scale"])
        assert C.worst(q_.grad, ref["dq"], ref["dq_scale"]) <= C.gemm_bound(e_q, rq32, n)
    assert torch.equal(grads[0][1], grads[1][1]) and torch.equal(grads[0][1], grads[2][1])
    # the weights themselves: every row sums to zero within N u max|V|, whatever B
    pn = ops.rank_sqnorm(p) if distance else None
    lse, _ = ops.softmax_all_forward(q, p, pn, truth, 0.37)
    v = ops.softmax_all_weights(q, p, pn, truth, lse, g, 0.37)
    assert v.shape == (b, n)
    assert bool((v.double().sum(1).abs() <= n * C.U * v.abs().max(1).values.double()).all())
    # a chunk written into a wider buffer touches nothing past its columns
    wide = torch.full((b, 300), 7.0, device=gpu_device)
    ops.softmax_all_weights(q, p, pn, truth, lse, g, 0.37, 256, 513, out=wide[:, :257])
    assert torch.equal(wide[:, :257], v[:, 256:513]) and bool((wide[:, 257:] == 7.0).all())


# ----------------------------------------------------------------------------- 4. model level
def _synthetic_model(L, dev, scoring, n=600, dim=8, n_rel=5, seed=0):
    from oracle import literalkg_oracle as O
    from literalkg_amd import io
    from literalkg_amd.synth import make_kg
    h, t, r = make_kg(n, 4000, seed=seed + 1)
    r = r % n_rel
    cfg = O.default_cfg(embed_dim=dim, relation_dim=2 * dim if scoring != "transr" else 12, conv_dim=dim, n_conv_layers=1,
                        device=dev)
    torch.manual_seed(seed)
    m = L.LiteralKG(cfg, n, n_rel, io.initial_a_in(n, h, t, r), scoring="transr" if scoring == "transr" else "transe")
    return m.to(dev), tuple(torch.from_numpy(x).to(dev) for x in (h, r, t))


def _dense_head(model, scoring, side, h, r, t, scale, dtype=torch.float32):
    """(loss per triple, sum of |lse| + |z_t| over the sides): the same encoder -- the library's gat_embeddings() -- and the
    head in dense torch ops of dtype on the device: cdist / matmul, cross_entropy"""
    table = model.gat_embeddings().to(dtype)
    e = model.relation_embed.weight.to(dtype)
    total, denom = 0.0, 0.0
    sides = ("tail", "head") if side == "both" else (side,)

    def ce(z, truth):
        with torch.no_grad():
            d = torch.logsumexp(z, 1).abs() + z.gather(1, truth[:, None])[:, 0].abs()
        return torch.nn.functional.cross_entropy(z, truth, reduction="none"), d

    def sqdist(a, b):
        return torch.cdist(a, b, compute_mode="donot_use_mm_for_euclid_dist") ** 2
    for s_ in sides:
        ent, truth, sign = (h, t, 1.0) if s_ == "tail" else (t, h, -1.0)
        if scoring == "dot":
            loss, d = ce(scale * (table[ent] @ table.t()), truth)
        elif scoring == "transe":
            loss, d = ce(-scale * sqdist(table[ent] + sign * e[r], table), truth)
        else:
            loss = torch.zeros(h.numel(), device=h.device, dtype=dtype)
            d = torch.zeros(h.numel(), device=h.device, dtype=dtype)
            for rr in r.unique().tolist():
                pos = (r == rr).nonzero()[:, 0]
                p_r = table @ model.gat_trans_M[rr].to(dtype)
                part, dd = ce(-scale * sqdist(p_r[ent[pos]] + sign * e[rr], p_r), truth[pos])
                loss = loss.index_put((pos,), part)
                d = d.index_put((pos,), dd)
        total, denom = total + loss, denom + d
    return total / len(sides), denom


@pytest.mark.parametrize("side", ["tail", "head", "both"])
@pytest.mark.parametrize("scoring", ["transe", "dot", "transr"])
def test_model_loss_and_parameter_gradients_against_a_dense_head(L, gpu_device, scoring, side):
    model, (h, r, t) = _synthetic_model(L, gpu_device, scoring)
    model.train()
    bh, br, bt = h[:70], r[:70], t[:70]
    model.zero_grad()
    loss = model.calc_one_vs_all_loss(bh, br, bt, side=side, scale=0.8, scoring=scoring)
    loss.backward()
    got = {k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None}
    same = None
    if (side, scoring) == ("tail", model.scoring):          # the mode's defaults: tail, scale 1, mean, the model's scoring
        same = (model(bh, br, bt, device=gpu_device, mode="one_vs_all"), model.calc_one_vs_all_loss(bh, br, bt))
    model.zero_grad()
    want_loss = _dense_head(model, scoring, side, bh, br, bt, 0.8)[0].mean()
    want_loss.backward()
    want = {k: v.grad for k, v in model.named_parameters() if v.grad is not None}
    assert abs(float(loss) - float(want_loss)) <= 1e-4 * max(1.0, abs(float(want_loss)))
    assert set(got) == set(want) and "entity_embed.weight" in got
    for name, w in want.items():
        w = w.to_dense() if w.is_sparse else w
        gq = got[name].to_dense() if got[name].is_sparse else got[name]
        tol = 1e-4 * float(w.abs().max())                  # the fixture-gradient tolerance of the README
        assert float((gq - w).abs().max()) <= tol, (name, float((gq - w).abs().max()), tol)
    if same is not None:
        assert float(same[0]) == float(same[1])             # mode='one_vs_all' is the method


@pytest.mark.parametrize("scoring", ["transe", "dot", "transr"])
def test_eval_mode_no_grad_gives_the_per_triple_nll(L, ops, gpu_device, scoring):
    model, (h, r, t) = _synthetic_model(L, gpu_device, scoring, seed=2)
    bh, br, bt = h[:70], r[:70], t[:70]
    for was_training in (True, False):
        model.train(was_training)
        with torch.no_grad():
            model.eval()
            nll = model.calc_one_vs_all_loss(bh, br, bt, side="both", reduction="none", scoring=scoring)
            model.train(was_training)
        assert model.training == was_training and nll.shape == (70,) and not nll.requires_grad
    model.eval()
    with torch.no_grad():
        want, denom = _dense_head(model, scoring, "both", bh, br, bt, 1.0, torch.float64)
        want32, _ = _dense_head(model, scoring, "both", bh, br, bt, 1.0, torch.float32)
        nll = model.calc_one_vs_all_loss(bh, br, bt, side="both", reduction="none", scoring=scoring)
        total = model.calc_one_vs_all_loss(bh, br, bt, side="both", reduction="sum", scoring=scoring)
    # the bound of test 1, both sides' |lse| + |z_t| in the scale (the loss is their mean)
    r32 = float(((want32.double() - want).abs() / denom).max())
    r = float(((nll.double() - want).abs() / denom).max())
    assert r <= C.loss_bound(r32), (r, r32)
    assert abs(float(total) - float(want.sum())) <= C.loss_bound(r32) * float(denom.sum())


# ----------------------------------------------------------------------------- 5. training
def test_twenty_adam_steps_lower_the_loss(L, gpu_device):
    model, (h, r, t) = _synthetic_model(L, gpu_device, "transe", seed=4)
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    bh, br, bt = h[:256], r[:256], t[:256]
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = model(bh, br, bt, device=gpu_device, mode="one_vs_all")
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert math.isfinite(losses[-1]) and losses[-1] < losses[0], losses
