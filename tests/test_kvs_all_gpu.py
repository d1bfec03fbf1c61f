"""GPU: the KvsAll loss (lkg_kvsall.hip, literalkg_amd/kvs_all.py) against float64.

References, list patterns, measures and bounds live in tests/kvs_all_cases.py (test_kvs_all_host.py shows on the CPU that
they accept a float32 restatement of the kernels' algorithm and reject planted faults).  Loss: per query
r = |L - L64| / sum_c |term64_c| <= max(3 r_torch32, 3e-7) on tables whose logits are exact in float32; the kernel's expf and
log1pf are the library's, so no allowance is added.  Gradients: per element against the float64 closed form, dq and dp
with the bound of the engine ops.gemm ran the product on, dbias (the weights kernel's own row sums) with
kvs_all_cases.dbias_bound.  Then what holds without any tolerance."""
import math

import pytest
import torch

import kvs_all_cases as K
import softmax_cases as C
import softmax_filtered_cases as F

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


@pytest.fixture(scope="module")
def kv(L):
    from literalkg_amd import kvs_all
    return kvs_all


def _splits(ops, b, n):
    s_max = ops.softmax_all_splits(b, n, ops.SOFTMAX_MAX_SPLITS)
    return sorted({1, min(2, s_max), s_max})


# ----------------------------------------------------------------------------- 1. the loss on exact-logit tables
@pytest.mark.parametrize("b,n,k", K.SHAPES)
def test_loss_on_exact_logit_tables(ops, kv, gpu_device, b, n, k):
    rows = K.patterns(b, n, seed=n + k)
    mask = K.mask_of(rows, n, gpu_device)
    pos = K.to_lists(rows, gpu_device)
    no_lists = K.to_lists([[] for _ in range(b)], gpu_device)
    for distance in (True, False):
        q, p, bias, scale = (x.to(gpu_device) if isinstance(x, torch.Tensor) else x
                             for x in K.exact_case(b, n, k, distance, seed=7 * b + n + k))
        assert torch.equal(K.logits(q, p, bias, distance, scale, torch.float32).double(),
                           K.logits(q, p, bias, distance, scale))            # the logits ARE exact in float32
        pn = ops.rank_sqnorm(p) if distance else None
        for eps in (0.0, 0.1):
            ref = K.loss_eval(q, p, bias, mask, distance, scale, eps)
            r32 = float(K.loss_measure(K.loss_eval(q, p, bias, mask, distance, scale, eps, torch.float32)[0], ref).max())
            bound = C.loss_bound(r32)
            for splits in _splits(ops, b, n):
                loss = kv.sigmoid_all_forward(q, p, pn, bias, pos, scale, eps, splits)
                r = float(K.loss_measure(loss, ref).max())
                print(f"b {b} n {n} k {k} distance {distance} eps {eps} S {splits}: r {r:.3g} bound {bound:.3g} "
                      f"[torch32 {r32:.3g}]")
                assert r <= bound, (distance, eps, splits, r, bound)
        # NULL lists give the bits of empty lists, a NULL bias those of a zero bias
        for splits in _splits(ops, b, n):
            a = kv.sigmoid_all_forward(q, p, pn, bias, None, scale, 0.1, splits)
            assert torch.equal(a, kv.sigmoid_all_forward(q, p, pn, bias, no_lists, scale, 0.1, splits))
            z0 = kv.sigmoid_all_forward(q, p, pn, torch.zeros_like(bias), pos, scale, 0.0, splits)
            assert torch.equal(z0, kv.sigmoid_all_forward(q, p, pn, None, pos, scale, 0.0, splits))


# ----------------------------------------------------------------------------- 2. gradients
def _engines(ops, q, p, b, n, k, width, distance):
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


@pytest.mark.parametrize("b,n,k", K.SHAPES)
def test_gradients_against_float64(ops, kv, gpu_device, b, n, k):
    q, p, bias, g = (x.to(gpu_device) for x in K.random_case(b, n, k, seed=3 * b + n + k, std=0.5 if k < 100 else 0.2))
    rows = K.patterns(b, n, seed=n + k)
    mask = K.mask_of(rows, n, gpu_device)
    pos = K.to_lists(rows, gpu_device)
    for distance, scale, eps in ((True, 1.0, 0.0), (False, 1.0, 0.1), (True, 0.37, 0.1), (False, 1.7, 0.0)):
        ref = K.grads_eval(q, p, bias, mask, g, distance, scale, eps)
        g32 = dict(zip(("dq", "dp", "dbias"), K.autograd_eval(q, p, bias, mask, g, distance, scale, eps, torch.float32)))
        r32 = {name: C.worst(g32[name], ref[name], ref[name + "_scale"]) for name in g32}
        e_q, e_p = _engines(ops, q, p, b, n, k, ops.softmax_chunk_width(b, n), distance)
        bound = {"dq": C.gemm_bound(e_q, r32["dq"], n), "dp": C.gemm_bound(e_p, r32["dp"], b),
                 "dbias": K.dbias_bound(r32["dbias"])}
        q_, p_, b_ = (x.clone().requires_grad_(True) for x in (q, p, bias))
        kv.sigmoid_all_loss(q_, p_, b_, pos, distance=distance, scale=scale, label_smoothing=eps).backward(g)
        got = {"dq": q_.grad, "dp": p_.grad, "dbias": b_.grad}
        for name in got:
            r = C.worst(got[name], ref[name], ref[name + "_scale"])
            print(f"b {b} n {n} k {k} distance {distance} scale {scale} eps {eps}: {name} r {r:.3g} bound "
                  f"{bound[name]:.3g} [{dict(dq=e_q, dp=e_p, dbias='row sums')[name]}, torch32 {r32[name]:.3g}]")
            assert r <= bound[name], (name, distance, scale, eps, r, bound[name])
        # the weights themselves: every column written, and the sign of each
        pn = ops.rank_sqnorm(p) if distance else None
        v = kv.sigmoid_all_weights(q, p, pn, bias, g, pos, scale, eps)
        assert v.shape == (b, n)
        if eps == 0.0:                              # without smoothing the sign of every weight is known
            assert bool((v[mask] <= 0).all()) and bool((v[~mask] >= 0).all())


def test_chunking_keeps_dp_bits_and_chunks_write_inside_their_columns(ops, kv, gpu_device):
    b, n, k = 130, 1100, 17
    q, p, bias, g = (x.to(gpu_device) for x in K.random_case(b, n, k, seed=21))
    rows = K.patterns(b, n, seed=5)
    pos = K.to_lists(rows, gpu_device)
    grads = []
    for n_chunks, width in ((1, 1280), (2, 768), (5, 256)):
        assert math.ceil(n / ops.softmax_chunk_width(b, n, 4 * b * width)) == n_chunks
        q_, p_, b_ = (x.clone().requires_grad_(True) for x in (q, p, bias))
        kv.sigmoid_all_loss(q_, p_, b_, pos, scale=0.37, label_smoothing=0.1, chunk_bytes=4 * b * width).backward(g)
        grads.append(p_.grad)
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2])
    pn = ops.rank_sqnorm(p)
    v = kv.sigmoid_all_weights(q, p, pn, bias, g, pos, 0.37, 0.1)
    wide = torch.full((b, 300), 7.0, device=gpu_device)
    kv.sigmoid_all_weights(q, p, pn, bias, g, pos, 0.37, 0.1, 256, 513, out=wide[:, :257])
    assert torch.equal(wide[:, :257], v[:, 256:513]) and bool((wide[:, 257:] == 7.0).all())    # n of the whole table


# ----------------------------------------------------------------------------- 3. without tolerance
def test_rows_do_not_depend_on_each_other_and_runs_repeat(ops, kv, gpu_device):
    b, n, k = 130, 1000, 17
    q, p, bias, g = (x.to(gpu_device) for x in K.random_case(b, n, k, seed=31))
    rows = K.patterns(b, n, seed=9)
    pn = ops.rank_sqnorm(p)
    pos = K.to_lists(rows, gpu_device)
    pick = torch.tensor([129, 3, 3, 77, 8, 0, 64, 65, 8], device=gpu_device)              # another order, duplicates
    sub = K.to_lists([rows[i] for i in pick.tolist()], gpu_device)
    for splits in (1, 2, 4):
        for eps in (0.0, 0.1):
            full = kv.sigmoid_all_forward(q, p, pn, bias, pos, 0.37, eps, splits)
            part = kv.sigmoid_all_forward(q[pick], p, pn, bias[pick], sub, 0.37, eps, splits)
            assert torch.equal(full[pick], part), (splits, eps)
    v = kv.sigmoid_all_weights(q, p, pn, bias, g, pos, 0.37, 0.1)
    assert torch.equal(v[pick], kv.sigmoid_all_weights(q[pick], p, pn, bias[pick], g[pick], sub, 0.37, 0.1))
    outs = []
    for _ in range(2):
        q_, p_, b_ = (x.clone().requires_grad_(True) for x in (q, p, bias))
        loss = kv.sigmoid_all_loss(q_, p_, b_, pos, scale=0.37, label_smoothing=0.1, chunk_bytes=4 * b * 512)
        loss.backward(g)
        outs.append((loss.detach(), q_.grad, p_.grad, b_.grad))
    for a, c in zip(*outs):
        assert torch.equal(a, c)


def test_nan_query_poisons_its_own_row_only(kv, gpu_device):
    q, p, bias, g = (x.to(gpu_device) for x in K.random_case(130, 1000, 17, seed=9))
    q[70, 5] = float("nan")
    pos = K.to_lists(K.patterns(130, 1000, seed=2), gpu_device)
    loss = kv.sigmoid_all_loss(q, p, bias, pos, splits=2)
    assert torch.isnan(loss).tolist() == [i == 70 for i in range(130)]


def _tiny_graph(L, dev, n=600, n_rel=5, seed=1):
    from literalkg_amd.synth import make_kg
    h, t, r = make_kg(n, 4000, seed=seed)
    r = r % n_rel
    h, r, t = (torch.from_numpy(x).to(dev) for x in (h, r, t))
    return h, r, t, L.KnownTriples(h, r, t, n, n_rel)


def test_positive_lists_equal_a_python_double_loop(L, ops, gpu_device):
    n = 600
    h, r, t, known = _tiny_graph(L, gpu_device)
    ent, rel = h[:97], r[:97]
    none = torch.full_like(ent, -1)
    cand = torch.randperm(n, generator=torch.Generator().manual_seed(0))[:250].sort().values.to(gpu_device)
    pos = torch.full((n,), -1, dtype=torch.int32, device=gpu_device)
    pos[cand] = torch.arange(250, dtype=torch.int32, device=gpu_device)
    for side, ids in (("tail", h[:97]), ("head", t[:97])):
        for frel in (rel, none):
            for pp, n_c in ((None, n), (pos, 250)):
                yptr, ycol = ops.softmax_excluded(known.for_side(side), ids, frel, none, n_c, pp)
                want = F.excluded_reference(known.for_side(side), ids, frel, none, n_c, pp)
                got = [ycol[yptr[i]:yptr[i + 1]].tolist() for i in range(97)]
                assert got == want and any(len(x) > 1 for x in want)
                assert all(x == sorted(set(x)) for x in got)


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


def _multi_hot(h, r, t, ent, rel, side, any_relation, n):
    """bool[len(ent), n] by a Python loop over the triples"""
    y = torch.zeros((ent.numel(), n), dtype=torch.bool)
    trip = list(zip(h.tolist(), r.tolist(), t.tolist()))
    for i, (e, rr) in enumerate(zip(ent.tolist(), rel.tolist())):
        for hh, r2, tt in trip:
            key, ans = (hh, tt) if side == "tail" else (tt, hh)
            if key == e and (any_relation or r2 == rr):
                y[i, ans] = True
    return y.to(ent.device)


def _dense_head(model, scoring, side, ent, rel, y, margin, scale, eps, cand=None):
    """the mean over the rows of the per-row BCE sums: the library's encoder, the head in dense torch ops"""
    table = model.gat_embeddings()
    e = model.relation_embed.weight
    sign = 1.0 if side == "tail" else -1.0
    bce = torch.nn.functional.binary_cross_entropy_with_logits

    def rows_loss(q, p, yy):
        if cand is not None:
            p, yy = p[cand], yy[:, cand]
        if scoring == "dot":
            z = scale * (margin + q @ p.t())
        else:
            z = scale * (margin - torch.cdist(q, p, compute_mode="donot_use_mm_for_euclid_dist") ** 2)
        target = (1.0 - eps) * yy.float() + eps / p.shape[0]
        return bce(z, target, reduction="none").sum(1)
    if scoring == "dot":
        loss = rows_loss(table[ent], table, y)
    elif scoring == "transe":
        loss = rows_loss(table[ent] + sign * e[rel], table, y)
    else:
        loss = torch.zeros(ent.numel(), device=ent.device)
        for rr in rel.unique().tolist():
            at = (rel == rr).nonzero()[:, 0]
            p_r = table @ model.gat_trans_M[rr]
            loss = loss.index_put((at,), rows_loss(p_r[ent[at]] + sign * e[rr], p_r, y[at]))
    return loss.mean()


@pytest.mark.parametrize("with_candidates", [False, True])
@pytest.mark.parametrize("scoring,side", [("transe", "tail"), ("transr", "head"), ("dot", "tail")])
def test_model_parameter_gradients_against_a_dense_bce_head(L, kv, gpu_device, scoring, side, with_candidates):
    n = 600
    model, (h, r, t) = _synthetic_model(L, gpu_device, scoring)
    known = L.KnownTriples(h, r, t, n, 5)
    model.train()
    ids = h[:80] if side == "tail" else t[:80]
    ent, rel = kv.distinct_queries(ids, r[:80])
    ent, rel = torch.cat((ent, ent[:3])), torch.cat((rel, rel[:3]))             # duplicates: rows of their own
    cand = None
    if with_candidates:
        cand = torch.randperm(n, generator=torch.Generator().manual_seed(1))[:333].to(gpu_device)
    margin, scale, eps = 6.0, 0.5, 0.1
    model.zero_grad()
    loss = model.calc_kvs_all_loss(ent, rel, known, side=side, margin=margin, scale=scale, label_smoothing=eps,
                                   scoring=scoring, candidates=cand)
    loss.backward()
    got = {k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None}
    per_row = model.calc_kvs_all_loss(ent, rel, known, side=side, margin=margin, scale=scale, label_smoothing=eps,
                                      scoring=scoring, candidates=cand, reduction="none", splits=2)
    assert torch.equal(per_row[-3:], per_row[:3])                               # duplicates get equal values
    if cand is not None:                    # any order of the candidates: the same bits
        again = model.calc_kvs_all_loss(ent, rel, known, side=side, margin=margin, scale=scale, label_smoothing=eps,
                                        scoring=scoring, candidates=cand.flip(0), reduction="none", splits=2)
        assert torch.equal(per_row, again)
    y = _multi_hot(h, r, t, ent, rel, side, scoring == "dot", n)
    assert int(y.sum(1).max()) > 1                                              # some query has several answers
    model.zero_grad()
    want_loss = _dense_head(model, scoring, side, ent, rel, y, margin, scale, eps,
                            None if cand is None else cand.sort().values)
    want_loss.backward()
    want = {k: v.grad for k, v in model.named_parameters() if v.grad is not None}
    assert abs(float(loss) - float(want_loss)) <= 1e-4 * max(1.0, abs(float(want_loss)))
    assert set(got) == set(want) and "entity_embed.weight" in got
    for name, w in want.items():
        w = w.to_dense() if w.is_sparse else w
        gq = got[name].to_dense() if got[name].is_sparse else got[name]
        tol = 1e-4 * float(w.abs().max())
        assert float((gq - w).abs().max()) <= tol, (name, float((gq - w).abs().max()), tol)


def test_twenty_adam_steps_lower_the_loss(L, kv, gpu_device):
    model, (h, r, t) = _synthetic_model(L, gpu_device, "transe", seed=4)
    known = L.KnownTriples(h, r, t, 600, 5)
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    ent, rel = kv.distinct_queries(h[:256], r[:256])
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = model.calc_kvs_all_loss(ent, rel, known, margin=6.0, label_smoothing=0.1)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert math.isfinite(losses[-1]) and losses[-1] < losses[0], losses
