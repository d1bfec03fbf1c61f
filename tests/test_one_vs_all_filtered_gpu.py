"""GPU: the FILTERED 1-vs-all loss -- the masked kernels of lkg_softmax.hip, ops.softmax_excluded, ops.softmax_all_loss(
exclude=) and one_vs_all_loss(known=, candidates=) -- against float64 with -inf at the excluded positions.

References and exclusion patterns live in tests/softmax_filtered_cases.py (test_softmax_filtered_host.py shows on the CPU
that they accept a correct float32 masked evaluation and reject planted faults); measures and bounds are those of
tests/softmax_cases.py, unchanged: the loss per query within max(3 r_torch32, 3e-7), a gradient per element within the
bound of the engine ops.gemm ran the product on."""
import math

import numpy as np
import pytest
import torch

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


def _layouts(q, p, k):
    """(name, q, p): contiguous rows, 16-byte aligned padded rows, rows off the 16-byte grid"""
    yield "contiguous", q, p
    yield "aligned", C.strided(q, C.aligned_ld(k)), C.strided(p, C.aligned_ld(k))
    yield "unaligned", C.strided(q, C.unaligned_ld(k)), C.strided(p, C.unaligned_ld(k))


def _offsets(b):
    return (0, 3, 5, 6, 8) if b == 1 else (0,)      # one row: the patterns one after the other


# ----------------------------------------------------------------------------- 1. exact-logit tables
@pytest.mark.parametrize("b,n,k", F.shapes())
def test_masked_loss_on_exact_logit_tables(ops, gpu_device, b, n, k):
    q, p, truth = (x.to(gpu_device) for x in C.integer_tables(b, n, k, seed=7 * b + n + k))
    scale = C.exact_scale(k)
    s_max = ops.softmax_all_splits(b, n, ops.SOFTMAX_MAX_SPLITS)
    for offset in _offsets(b):
        ex = F.patterns(b, n, truth.cpu(), seed=b + n + k, offset=offset)
        mask, lists = F.mask_of(ex, n, gpu_device), F.to_lists(ex, gpu_device)
        for distance in (True, False):
            ref = F.loss_eval(q, p, truth, mask, distance, scale)
            loss32 = F.loss_eval(q, p, truth, mask, distance, scale, torch.float32)[2]
            bound = C.loss_bound(float(C.loss_measure(loss32, ref).max()))
            pn = ops.rank_sqnorm(p) if distance else None
            for name, q_, p_ in _layouts(q, p, k):
                for splits in sorted({1, min(2, s_max), s_max}):
                    lse, loss = ops.softmax_all_forward(q_, p_, pn, truth, scale, splits, exclude=lists)
                    r = float(C.loss_measure(loss, ref).max())
                    print(f"b {b} n {n} k {k} offset {offset} distance {distance} {name} S {splits}: r {r:.3g} "
                          f"bound {bound:.3g}")
                    assert r <= bound, (offset, distance, name, splits, r, bound)
                    r_lse = float(((lse[0].double() + lse[1].double() - ref[0]).abs()
                                   / (ref[0].abs() + ref[1].abs() + 1e-300)).max())
                    assert r_lse <= bound, (offset, distance, name, splits, r_lse)


# ----------------------------------------------------------------------------- 2. gradients
def _engines(ops, q, p, b, n, k, width, distance=True):
    """the engines ops.gemm runs the backward's two products on (as the op does; test_one_vs_all_gpu.py)"""
    dev = q.device
    w = min(width, n)
    v = torch.empty((b, w), device=dev)
    ws = min(w, ops.SOFTMAX_DQ_SLICE)
    e_q = ops.gemm_engine(v[:, :ws], p[:ws], alpha=2.0, beta=1.0, out=torch.empty((b, k), device=dev))
    kq = k + 1 if distance else k
    e_p = ops.gemm_engine(v, torch.empty((b, kq), device=dev), trans_a=True, alpha=2.0, beta=1.0,
                          out=torch.empty((w, kq), device=dev))
    return e_q, e_p


@pytest.mark.parametrize("b,n,k", F.shapes())
def test_masked_gradients_against_float64_autograd(ops, gpu_device, b, n, k):
    q, p, truth, g = (x.to(gpu_device) for x in C.random_tables(b, n, k, seed=3 * b + n + k, std=0.5 if k < 100 else 0.2))
    for offset in _offsets(b)[:3]:
        ex = F.patterns(b, n, truth.cpu(), seed=b + n + k, offset=offset)
        mask, lists = F.mask_of(ex, n, gpu_device), F.to_lists(ex, gpu_device)
        for distance, scale in ((True, 1.0), (False, 1.7), (True, 0.37)):
            ref = F.grads_eval(q, p, truth, g, mask, distance, scale)
            dq32, dp32 = F.autograd_eval(q, p, truth, g, mask, distance, scale, torch.float32)
            rq32, rp32 = C.worst(dq32, ref["dq"], ref["dq_scale"]), C.worst(dp32, ref["dp"], ref["dp_scale"])
            e_q, e_p = _engines(ops, q, p, b, n, k, ops.softmax_chunk_width(b, n), distance)
            bq, bp = C.gemm_bound(e_q, rq32, n), C.gemm_bound(e_p, rp32, b)
            for name, q0, p0 in list(_layouts(q, p, k))[:1 if n > 1000 else 3]:
                q_ = q0.clone().requires_grad_(True) if name == "contiguous" else q0.detach().requires_grad_(True)
                p_ = p0.clone().requires_grad_(True) if name == "contiguous" else p0.detach().requires_grad_(True)
                ops.softmax_all_loss(q_, p_, truth, distance=distance, scale=scale, exclude=lists).backward(g)
                rq, rp = C.worst(q_.grad, ref["dq"], ref["dq_scale"]), C.worst(p_.grad, ref["dp"], ref["dp_scale"])
                print(f"b {b} n {n} k {k} offset {offset} distance {distance} scale {scale} {name}: dq r {rq:.3g} bound "
                      f"{bq:.3g} [{e_q}]  dp r {rp:.3g} bound {bp:.3g} [{e_p}]")
                assert rq <= bq, ("dq", offset, distance, scale, name, rq, bq, e_q)
                assert rp <= bp, ("dp", offset, distance, scale, name, rp, bp, e_p)
        # the weights themselves: exact zeros at the excluded positions, in chunks as in one piece
        pn = ops.rank_sqnorm(p)
        lse, _ = ops.softmax_all_forward(q, p, pn, truth, 0.37, exclude=lists)
        v = ops.softmax_all_weights(q, p, pn, truth, lse, g, 0.37, exclude=lists)
        assert bool((v[mask] == 0).all()) and (n == 1 or bool((v[~mask] != 0).any()))
        if n > 300:
            part = ops.softmax_all_weights(q, p, pn, truth, lse, g, 0.37, 256, n - 3, exclude=lists)
            assert torch.equal(part, v[:, 256:n - 3])


# ----------------------------------------------------------------------------- 3. exact checks
@pytest.mark.parametrize("b,n,k", [(130, 70001, 17), (65, 1000, 300), (1, 257, 1)])
def test_empty_lists_give_the_bits_of_the_unmasked_kernels(ops, gpu_device, b, n, k):
    q, p, truth, g = (x.to(gpu_device) for x in C.random_tables(b, n, k, seed=b + n))
    lists = F.to_lists([[] for _ in range(b)], gpu_device)
    s_max = ops.softmax_all_splits(b, n, ops.SOFTMAX_MAX_SPLITS)
    for distance in (True, False):
        pn = ops.rank_sqnorm(p) if distance else None
        for name, q_, p_ in _layouts(q, p, k):
            for splits in sorted({1, s_max}):
                lse, loss = ops.softmax_all_forward(q_, p_, pn, truth, 0.7, splits)
                lse_m, loss_m = ops.softmax_all_forward(q_, p_, pn, truth, 0.7, splits, exclude=lists)
                assert torch.equal(lse, lse_m) and torch.equal(loss, loss_m), (distance, name, splits)
            v = ops.softmax_all_weights(q_, p_, pn, truth, lse, g, 0.7)
            v_m = ops.softmax_all_weights(q_, p_, pn, truth, lse, g, 0.7, exclude=lists)
            assert torch.equal(v, v_m), (distance, name)


@pytest.mark.parametrize("distance", [True, False])
def test_everything_but_the_truth_excluded_gives_exactly_zero(ops, gpu_device, distance):
    for b, n, k in ((65, 1000, 17), (130, 257, 300), (1, 70001, 17)):
        q, p, truth, g = (x.to(gpu_device) for x in C.random_tables(b, n, k, seed=b + k))
        lists = F.to_lists(F.all_but_truth(n, truth.cpu()), gpu_device)
        for splits in (1, None):
            q_ = q.clone().requires_grad_(True)
            p_ = p.clone().requires_grad_(True)
            loss = ops.softmax_all_loss(q_, p_, truth, distance=distance, scale=0.7, splits=splits, exclude=lists)
            assert torch.equal(loss, torch.zeros_like(loss)), (b, n, k, splits, loss)
            loss.backward(g)
            assert torch.equal(q_.grad, torch.zeros_like(q)) and torch.equal(p_.grad, torch.zeros_like(p))
        pn = ops.rank_sqnorm(p) if distance else None
        lse, _ = ops.softmax_all_forward(q, p, pn, truth, 0.7, exclude=lists)
        v = ops.softmax_all_weights(q, p, pn, truth, lse, g, 0.7, exclude=lists)
        assert torch.equal(v, torch.zeros_like(v))


@pytest.mark.parametrize("b,n,k", [(65, 1000, 17), (130, 70001, 17)])
def test_masking_equals_moving_the_excluded_rows_out_of_reach(ops, gpu_device, b, n, k):
    """One exclusion set for all rows, distance scoring: the masked loss on p has the bits of the unmasked loss on a copy
    of p whose excluded rows sit so far away that their exp underflows to exactly 0 (in float64 the dropped logits lie more
    than 200 below each row's maximum; float32's exp is 0 below -104)."""
    q, p, truth, _ = C.random_tables(b, n, k, seed=5 * b + n)
    gen = torch.Generator().manual_seed(n)
    shared = {0, n - 1, 63, 64, 255, 256, *range(64, 128), *range(n // 2 - 300, n // 2 + 300),
              *torch.randint(0, n, (40,), generator=gen).tolist()} - set(truth.tolist())
    shared = sorted(c for c in shared if 0 <= c < n)
    far = p.clone()
    far[torch.tensor(shared)] += 1000.0
    z = C.logits(q, far, True, 0.5)
    gap = z.max(1).values[:, None] - z[:, torch.tensor(shared)]
    assert float(gap.min()) > 200, float(gap.min())
    assert bool(torch.isfinite(C.logits(q, far, True, 0.5, torch.float32)).all())
    q, p, far, truth = (x.to(gpu_device) for x in (q, p, far, truth))
    lists = F.to_lists([shared] * b, gpu_device)
    s_max = ops.softmax_all_splits(b, n, ops.SOFTMAX_MAX_SPLITS)
    for splits in sorted({1, min(3, s_max), s_max}):
        masked = ops.softmax_all_loss(q, p, truth, distance=True, scale=0.5, splits=splits, exclude=lists)
        moved = ops.softmax_all_loss(q, far, truth, distance=True, scale=0.5, splits=splits)
        assert torch.equal(masked, moved), (splits, float((masked - moved).abs().max()))
        assert bool(torch.isfinite(masked).all())


def test_a_nan_table_row_poisons_only_the_rows_that_keep_it(ops, gpu_device):
    b, n, k = 130, 1000, 17
    q, p, truth, g = (x.to(gpu_device) for x in C.random_tables(b, n, k, seed=9))
    bad = 300
    truth[truth == bad] = bad + 1
    p[bad, 5] = float("nan")
    drops = [i % 3 != 1 for i in range(b)]                   # two rows of three exclude the NaN row
    lists = F.to_lists([[bad] if d else [7 if int(truth[i]) != 7 else 8] for i, d in enumerate(drops)], gpu_device)
    for distance in (True, False):              # (the loss; the backward's products still meet the row: 0 * NaN)
        for splits in (1, 2):
            loss = ops.softmax_all_loss(q, p, truth, distance=distance, splits=splits, exclude=lists)
            assert torch.isnan(loss).tolist() == [not d for d in drops]
    pn = ops.rank_sqnorm(p)
    lse, _ = ops.softmax_all_forward(q, p, pn, truth, exclude=lists)
    v = ops.softmax_all_weights(q, p, pn, truth, lse, g, exclude=lists)
    assert torch.isnan(v).any(1).tolist() == [not d for d in drops]        # the weights: an exact 0 at the dropped NaN


def test_two_runs_give_the_same_bits(ops, gpu_device):
    b, n, k = 130, 70001, 300
    q, p, truth, g = (x.to(gpu_device) for x in C.random_tables(b, n, k, seed=11))
    lists = F.to_lists(F.patterns(b, n, truth.cpu(), seed=2), gpu_device)
    outs = []
    for _ in range(2):
        q_ = q.clone().requires_grad_(True)
        p_ = p.clone().requires_grad_(True)
        loss = ops.softmax_all_loss(q_, p_, truth, scale=0.25, chunk_bytes=130 * 4 * 20000, exclude=lists)
        loss.backward(g)
        outs.append((loss.detach(), q_.grad, p_.grad))
    for a, b_ in zip(*outs):
        assert torch.equal(a, b_)


# ----------------------------------------------------------------------------- 4. the exclusion lists
def _known_case(L, dev, n=300, n_rel=3, e=3000, seed=0):
    gen = torch.Generator().manual_seed(seed)
    h = (n * torch.rand(e, generator=gen) ** 2).long()        # a few heads with long rows
    t = torch.randint(0, n, (e,), generator=gen)
    r = torch.randint(0, n_rel, (e,), generator=gen)
    h, t, r = torch.cat((h, h[:200])), torch.cat((t, t[:200])), torch.cat((r, r[:200]))       # duplicates
    return L.KnownTriples(h.to(dev), r.to(dev), t.to(dev), n, n_rel), (h, r, t)


@pytest.mark.parametrize("side", ["tail", "head"])
def test_softmax_excluded_equals_the_double_loop(L, ops, gpu_device, side):
    n, n_rel = 300, 3
    known, (h, r, t) = _known_case(L, gpu_device)
    filt = known.for_side(side)
    gen = torch.Generator().manual_seed(4)
    for b in (1, 65, 130):
        rows = torch.cat((torch.tensor([0, 1, 2])[:b], torch.randint(0, n, (max(b - 3, 0),), generator=gen)))
        rels = torch.randint(0, n_rel, (b,), generator=gen)
        rels[::4] = -1                                          # under any relation
        truth = torch.randint(0, n, (b,), generator=gen)
        truth[:min(b, 50)] = (t if side == "tail" else h)[:min(b, 50)]      # some truths that ARE known answers
        rows[:min(b, 50)] = (h if side == "tail" else t)[:min(b, 50)]
        args = [x.to(gpu_device) for x in (rows, rels, truth)]
        xptr, xcol = ops.softmax_excluded(filt, *args, n)
        want = F.excluded_reference(filt, rows, rels, truth, n)
        wp, wc = F.to_lists(want)
        assert xptr.dtype == torch.int32 and xcol.dtype == torch.int32
        assert torch.equal(xptr.cpu(), wp) and torch.equal(xcol.cpu(), wc), (side, b)
        assert xcol.numel() > 0 or b == 1
        # with a candidate map: 120 candidates, the truths given as positions
        cand = torch.sort(torch.randperm(n, generator=gen)[:120]).values
        pos = torch.full((n,), -1, dtype=torch.int32)
        pos[cand] = torch.arange(120, dtype=torch.int32)
        tpos = torch.randint(0, 120, (b,), generator=gen)
        xptr, xcol = ops.softmax_excluded(filt, args[0], args[1], tpos.to(gpu_device), 120, pos.to(gpu_device))
        wp, wc = F.to_lists(F.excluded_reference(filt, rows, rels, tpos, 120, pos))
        assert torch.equal(xptr.cpu(), wp) and torch.equal(xcol.cpu(), wc), (side, b, "pos")
    empty = ops.softmax_excluded(filt, args[0][:0], args[1][:0], args[2][:0], n)
    assert empty[0].tolist() == [0] and empty[1].numel() == 0
    # the tiny structure: an empty row, an entry under another relation only, any relation
    th, tr, tt = (torch.tensor(x, device=gpu_device) for x in F.TINY_TRIPLES)
    tiny = L.KnownTriples(th, tr, tt, 5, 2).for_side(side)
    rows, rels, truth = (torch.tensor(x) for x in F.TINY_QUERIES)
    xptr, xcol = ops.softmax_excluded(tiny, *(x.to(gpu_device) for x in (rows, rels, truth)), 5)
    want = F.excluded_reference(tiny, rows, rels, truth, 5)
    assert want == ([[], [1], [3], []] if side == "tail" else [[], [], [3], [0]])
    wp, wc = F.to_lists(want)
    assert torch.equal(xptr.cpu(), wp) and torch.equal(xcol.cpu(), wc), (side, "tiny")


# ----------------------------------------------------------------------------- 5. model level
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


def _dense_known(h, r, t, n, n_rel):
    k = torch.zeros((n_rel, n, n), dtype=torch.bool, device=h.device)
    k[r, h, t] = True
    return k


def _dense_masked_head(model, scoring, side, h, r, t, scale, kd, cand=None, dtype=torch.float32):
    """(loss per triple, |lse| + |z_t|): the library's encoder, then the head of ONE side in dense torch ops of dtype with
    the known answers (kd bool[rel, head, tail], None: no filter) other than the truth at -inf, over the sorted candidates"""
    table = model.gat_embeddings().to(dtype)
    e = model.relation_embed.weight.to(dtype)
    n = table.shape[0]
    cols = torch.arange(n, device=h.device) if cand is None else torch.sort(cand).values
    ent, truth, sign = (h, t, 1.0) if side == "tail" else (t, h, -1.0)
    tpos = torch.searchsorted(cols, truth)
    mask = torch.zeros((h.numel(), cols.numel()), dtype=torch.bool, device=h.device)
    if kd is not None:
        if scoring == "dot":
            ka = kd.any(0)
            mask = (ka[ent] if side == "tail" else ka[:, ent].t())[:, cols]
        else:
            mask = (kd[r, ent] if side == "tail" else kd[r, :, ent])[:, cols]
        mask = mask.clone()
        mask[torch.arange(h.numel(), device=h.device), tpos] = False

    def sqdist(a, b):
        return torch.cdist(a, b, compute_mode="donot_use_mm_for_euclid_dist") ** 2
    if scoring == "dot":
        z = scale * (table[ent] @ table[cols].t())
    elif scoring == "transe":
        z = -scale * sqdist(table[ent] + sign * e[r], table[cols])
    else:
        z = torch.zeros((h.numel(), cols.numel()), device=h.device, dtype=dtype)
        for rr in r.unique().tolist():
            at = (r == rr).nonzero()[:, 0]
            w = model.gat_trans_M[rr].to(dtype)
            z = z.index_put((at,), -scale * sqdist(table[ent[at]] @ w + sign * e[rr], table[cols] @ w))
    z = z.masked_fill(mask, -math.inf)
    lse, zt = torch.logsumexp(z, 1), z.gather(1, tpos[:, None])[:, 0]
    return lse - zt, (lse.abs() + zt.abs()).detach()


def _candidates(h, t, side, n, dev, seed=0):
    """300 entities that hold every truth of the side, in a shuffled order"""
    gen = torch.Generator().manual_seed(seed)
    truth = (t if side == "tail" else h).cpu()
    rest = torch.randperm(n, generator=gen)[:300]
    cand = torch.unique(torch.cat((truth, rest)))
    return cand[torch.randperm(cand.numel(), generator=gen)].to(dev)


@pytest.mark.parametrize("side", ["tail", "head"])
@pytest.mark.parametrize("scoring", ["transe", "dot", "transr"])
def test_filtered_nll_against_a_dense_masked_head(L, gpu_device, scoring, side):
    model, (h, r, t) = _synthetic_model(L, gpu_device, scoring, seed=2)
    known = L.KnownTriples(h, r, t, model.n_entities, model.n_relations)
    kd = _dense_known(h, r, t, model.n_entities, model.n_relations)
    bh, br, bt = h[:70], r[:70], t[:70]
    model.eval()
    with torch.no_grad():
        plain = model.calc_one_vs_all_loss(bh, br, bt, side=side, reduction="none", scoring=scoring)
        for cand in (None, _candidates(bh, bt, side, model.n_entities, gpu_device)):
            want, denom = _dense_masked_head(model, scoring, side, bh, br, bt, 1.0, kd, cand, torch.float64)
            want32, _ = _dense_masked_head(model, scoring, side, bh, br, bt, 1.0, kd, cand, torch.float32)
            nll = model.calc_one_vs_all_loss(bh, br, bt, side=side, reduction="none", scoring=scoring, known=known,
                                             candidates=cand)
            assert nll.shape == (70,) and not nll.requires_grad
            r32 = float(((want32.double() - want).abs() / denom).max())
            rr = float(((nll.double() - want).abs() / denom).max())
            print(f"{scoring} {side} candidates {cand is not None}: r {rr:.3g} r_torch32 {r32:.3g}")
            assert rr <= C.loss_bound(r32), (rr, r32)
            assert bool((nll.double() <= plain.double() + C.loss_bound(r32) * denom).all())     # fewer negatives, row by row
            assert cand is not None or bool((nll < plain).any())                              # (the filter does bite)
    # both sides: the mean of the two
    with torch.no_grad():
        both = model.calc_one_vs_all_loss(bh, br, bt, side="both", reduction="none", scoring=scoring, known=known)
        tail = model.calc_one_vs_all_loss(bh, br, bt, side="tail", reduction="none", scoring=scoring, known=known)
        head = model.calc_one_vs_all_loss(bh, br, bt, side="head", reduction="none", scoring=scoring, known=known)
    assert torch.equal(both, 0.5 * (tail + head))


@pytest.mark.parametrize("with_candidates", [False, True])
@pytest.mark.parametrize("scoring", ["transe", "dot", "transr"])
def test_filtered_parameter_gradients_against_a_dense_masked_head(L, gpu_device, scoring, with_candidates):
    model, (h, r, t) = _synthetic_model(L, gpu_device, scoring)
    known = L.KnownTriples(h, r, t, model.n_entities, model.n_relations)
    kd = _dense_known(h, r, t, model.n_entities, model.n_relations)
    bh, br, bt = h[:70], r[:70], t[:70]
    side = "head" if with_candidates else "tail"
    cand = _candidates(bh, bt, side, model.n_entities, gpu_device) if with_candidates else None
    model.train()
    model.zero_grad()
    loss = model.calc_one_vs_all_loss(bh, br, bt, side=side, scale=0.8, scoring=scoring, known=known, candidates=cand)
    loss.backward()
    got = {k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None}
    model.zero_grad()
    want_loss = _dense_masked_head(model, scoring, side, bh, br, bt, 0.8, kd, cand)[0].mean()
    want_loss.backward()
    want = {k: v.grad for k, v in model.named_parameters() if v.grad is not None}
    assert abs(float(loss.detach()) - float(want_loss.detach())) <= 1e-4 * max(1.0, abs(float(want_loss.detach())))
    assert set(got) == set(want) and "entity_embed.weight" in got
    for name, w in want.items():
        w = w.to_dense() if w.is_sparse else w
        gq = got[name].to_dense() if got[name].is_sparse else got[name]
        tol = 1e-4 * float(w.abs().max())                  # the bound of test_one_vs_all_gpu.py
        assert float((gq - w).abs().max()) <= tol, (name, float((gq - w).abs().max()), tol)


@pytest.mark.parametrize("scoring", ["transe", "transr"])
def test_candidates_keep_the_table_gradient_on_candidate_and_query_rows(L, gpu_device, scoring):
    model, (h, r, t) = _synthetic_model(L, gpu_device, scoring, seed=3)
    known = L.KnownTriples(h, r, t, model.n_entities, model.n_relations)
    bh, br, bt = h[:70], r[:70], t[:70]
    cand = _candidates(bh, bt, "tail", model.n_entities, gpu_device)
    model.train()
    table = model.gat_embeddings()
    table.retain_grad()
    model._table_for_inference = lambda: table               # the table of the step, kept to read its gradient
    model.calc_one_vs_all_loss(bh, br, bt, scoring=scoring, known=known, candidates=cand).backward()
    reached = torch.zeros(model.n_entities, dtype=torch.bool, device=gpu_device)
    reached[cand] = True
    reached[bh] = True
    assert torch.equal(table.grad[~reached], torch.zeros_like(table.grad[~reached])) and bool((~reached).any())
    assert bool((table.grad[reached] != 0).any())


def test_the_bits_ignore_what_must_not_matter(L, gpu_device):
    """the order of candidates, duplicates in known, the trained triples present in known or absent from it, two runs"""
    model, (h, r, t) = _synthetic_model(L, gpu_device, "transe", seed=5)
    n, n_rel = model.n_entities, model.n_relations
    # a batch of distinct (h, r): no row's truth is another row's "other answer", so taking the batch out of known
    # changes no row's list
    first = np.unique((h * n_rel + r).cpu().numpy(), return_index=True)[1][:70]
    first = torch.from_numpy(first).to(gpu_device)
    bh, br, bt = h[first], r[first], t[first]
    cand = _candidates(bh, bt, "tail", n, gpu_device)
    model.eval()

    def run(known, cand_):
        with torch.no_grad():
            return model.calc_one_vs_all_loss(bh, br, bt, reduction="none", splits=2, known=known, candidates=cand_)
    full = L.KnownTriples(h, r, t, n, n_rel)
    doubled = L.KnownTriples(torch.cat((h, h[:500])), torch.cat((r, r[:500])), torch.cat((t, t[:500])), n, n_rel)
    # the batch's own triples taken out of known (every copy of them)
    key = (h * n_rel + r) * n + t
    keep = ~torch.isin(key, (bh * n_rel + br) * n + bt)
    without = L.KnownTriples(h[keep], r[keep], t[keep], n, n_rel)
    assert int(keep.sum()) < h.numel()
    for cand_ in (None, cand):
        base = run(full, cand_)
        assert torch.equal(base, run(full, cand_)) and torch.equal(base, run(doubled, cand_))
        assert torch.equal(base, run(without, cand_))
    assert torch.equal(run(full, cand), run(full, cand.flip(0)))
    assert torch.equal(run(full, cand), run(full, torch.sort(cand).values))
    assert not torch.equal(run(full, None), run(None, None))


def test_a_few_adam_steps_lower_the_filtered_loss(L, gpu_device):
    model, (h, r, t) = _synthetic_model(L, gpu_device, "transe", seed=4)
    known = L.KnownTriples(h, r, t, model.n_entities, model.n_relations)
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    bh, br, bt = h[:256], r[:256], t[:256]
    losses = []
    for _ in range(8):
        opt.zero_grad()
        loss = model.calc_one_vs_all_loss(bh, br, bt, known=known)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert math.isfinite(losses[-1]) and losses[-1] < losses[0], losses


def test_error_paths(L, gpu_device):
    model, (h, r, t) = _synthetic_model(L, gpu_device, "transe", seed=6)
    n, n_rel = model.n_entities, model.n_relations
    bh, br, bt = h[:20], r[:20], t[:20]
    cand = _candidates(bh, bt, "tail", n, gpu_device)
    model._table_for_inference = None                        # no error path may reach the table
    with pytest.raises(ValueError, match="every truth must be a candidate"):
        model.calc_one_vs_all_loss(bh, br, bt, candidates=cand[cand != bt[3]])
    with pytest.raises(ValueError, match="with candidates"):
        model.calc_one_vs_all_loss(bh, br, bt, side="both", candidates=cand)
    with pytest.raises(ValueError, match="candidates must be unique"):
        model.calc_one_vs_all_loss(bh, br, bt, candidates=torch.cat((cand, cand[:1])))
    with pytest.raises(ValueError, match="known triples live on"):
        model.calc_one_vs_all_loss(bh, br, bt, known=type("K", (), dict(n_entities=n, device=torch.device("cpu")))())
    with pytest.raises(ValueError, match="known triples over"):
        model.calc_one_vs_all_loss(bh, br, bt, known=L.KnownTriples(h % 50, r, t % 50, 50, n_rel))
    with pytest.raises(ValueError, match="has no 1-vs-all loss"):
        model.calc_one_vs_all_loss(bh, br, bt, scoring="mlp", known=L.KnownTriples(h, r, t, n, n_rel))
