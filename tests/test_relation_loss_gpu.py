"""GPU, op level: lkg_relation_loss_fwd_f32 / lkg_relation_loss_bwd_f32 on a given slab and in shared mode against the
float64 references, measures and counted bounds of tests/relation_loss_cases.py (which test_relation_loss_host.py shows to
accept a float32 restatement of the kernels and to reject planted faults); the checks that have no tolerance (an empty or
edge-less filter, the truth alone, masking against a far-away e_j, a pair alone against the pair in a batch, two runs, the
two load paths, duplicate known triples, NaN isolation); the whole op literalkg_amd.relation_loss.relation_softmax_loss
(its gradients under the bounds of the engines that run its products, partial gradients, chunking); and the bits under the
perturbations of tests/invariance.py."""
import contextlib
import importlib
import itertools
import math

import pytest
import torch

import invariance as V
import relation_loss_cases as RC
import softmax_cases as C

pytestmark = pytest.mark.gpu

MODES = ("poison 0xFF", "poison 0x7F", "side stream + poison 0xFF")


@pytest.fixture(scope="module")
def rl(gpu_device):
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("literalkg_amd.relation_loss")


@pytest.fixture(scope="module")
def ops(rl):
    from literalkg_amd import ops
    return ops


def _rows(x, dev, aligned):
    return C.strided(x.to(dev), C.aligned_ld(x.shape[1]) if aligned else C.unaligned_ld(x.shape[1]))


def _slab(u3, dev, aligned):
    """(u[P, R rs] on the device, rs): the blocks of u3[P, R, D] rs elements apart in rows of R rs (+ a gap) elements, rs
    and the row stride multiples of 4 floats (the 16-byte path where D allows it) or not (the scalar path)"""
    p, n_rel, k = u3.shape
    rs = (k + 3) // 4 * 4 if aligned else C.unaligned_ld(k)
    buf = torch.zeros((p, n_rel * rs + (4 if aligned else 1)), dtype=torch.float32, device=dev)
    u = buf[:, :n_rel * rs]
    u.view(p, n_rel, rs)[:, :, :k] = u3.float().to(dev)
    return u, rs


def _blocks(u, rs, k):
    return u.reshape(u.shape[0], -1, rs)[:, :, :k]


def _filter(ops, mask, truth, dev):
    """(filt, filter_row, filter_col) on the device for the mask (tests/relation_loss_cases.triples_of_mask: a duplicate
    and known truths included), or three None"""
    if mask is None:
        return None, None, None
    kh, kr, kt, h, t = RC.triples_of_mask(mask, truth)
    filt = ops.csr_build_device(2 * mask.shape[0], kh.to(dev), kt.to(dev), kr.to(dev))
    return filt, h.to(dev), t.to(dev)


def _check_kernels(rl, ops, dev, case, u3, aligned, shared):
    d, w, e, truth, mask, scale = (case[x] for x in ("d", "w", "e", "truth", "mask", "scale"))
    p, n_rel, k = u3.shape
    g = RC.upstream(p, k + n_rel)
    ref = RC.loss_eval(u3, e, truth, mask, scale)
    want = RC.grads_eval(u3, None, None, e, truth, mask, scale, g)
    ed, td, gdv = _rows(e, dev, aligned), truth.to(dev), g.to(dev)
    filt, frow, fcol = _filter(ops, mask, truth, dev)
    if shared:
        u, rs = _rows(d, dev, aligned), 0
    else:
        u, rs = _slab(u3, dev, aligned)
    loss, z, lse = rl.relation_softmax_forward(u, rs, ed, td, scale, filt, frow, fcol)
    z64 = RC.logits(u3, e, truth, mask, scale)
    assert torch.equal(z.cpu().double(), z64)                                      # exact logits, -inf where dropped
    u3d, e32, m_d = u3.float().to(dev), e.to(dev), None if mask is None else mask.to(dev)
    l32 = RC.loss_eval(u3d, e32, td, m_d, scale, torch.float32)
    r32 = float(RC.loss_measure(l32[2], ref).max())
    r, bound = float(RC.loss_measure(loss, ref).max()), RC.loss_bound(r32, n_rel, k)
    r_lse = float(RC.loss_measure(lse - l32[1], ref).max())
    print(f"loss: r {r:.3g} (lse - z_t: {r_lse:.3g}), r_torch32 {r32:.3g}, bound {bound:.3g} ({RC.loss_roundings(n_rel, k)} u)")
    assert r <= bound and r_lse <= bound, (r, r_lse, bound)
    if mask is not None or n_rel == 1:                                             # pair 0: the truth alone
        assert float(loss[0]) == 0.0
    t32 = RC.grads_eval(u3d, None, None, e32, td, m_d, scale, gdv, torch.float32)
    if shared:
        gd, c = rl.relation_softmax_backward(u, 0, ed, td, scale, gdv, z)
        got = dict(gd=gd, c=c)
    else:
        got = dict(G=_blocks(rl.relation_softmax_backward(u, rs, ed, td, scale, gdv, z), rs, k))
    for name, x in got.items():
        scale64 = want[name + "_scale"]
        r32 = C.worst(t32[name].cpu(), want[name], scale64)
        r, bound = C.worst(x.cpu(), want[name], scale64), RC.grad_bound(r32, n_rel, k, name)
        print(f"{name}: r {r:.3g}, r_torch32 {r32:.3g}, bound {bound:.3g} ({RC.grad_roundings(n_rel, k, name)} u)")
        assert r <= bound, (name, r, bound)
        if mask is not None and name != "gd":
            assert bool((x[m_d] == 0).all())                                       # a dropped relation: exactly zero
        if mask is not None or n_rel == 1:
            assert bool((x[0] == 0).all())                                         # the truth alone: exactly zero


@pytest.mark.parametrize("case", RC.SLAB_CASES, ids=RC.slab_id)
def test_kernels_on_a_given_slab(rl, ops, gpu_device, case):
    p, n_rel, k, c, aligned, filtered = case
    drawn = RC.exact_case(p, n_rel, k, c, seed=p + 3 * n_rel + 7 * k, filtered=filtered)
    _check_kernels(rl, ops, gpu_device, drawn, RC.slab_of(drawn["d"], drawn["w"], n_rel), aligned, shared=False)


@pytest.mark.parametrize("case", RC.SHARED_CASES, ids=RC.shared_id)
def test_kernels_in_shared_mode(rl, ops, gpu_device, case):
    p, n_rel, k, aligned, filtered = case
    drawn = RC.exact_case(p, n_rel, k, None, seed=p + 3 * n_rel + 7 * k, filtered=filtered)
    _check_kernels(rl, ops, gpu_device, drawn, RC.slab_of(drawn["d"], None, n_rel), aligned, shared=True)


# ----------------------------------------------------------------------------- without tolerance
def _kernels(rl, dev, u3, d, e, truth, scale, g, aligned, shared, filt=None, frow=None, fcol=None):
    """[z, lse, loss, G] (slab) or [z, lse, loss, gd, c] (shared) of the two entry points"""
    p, n_rel, k = u3.shape
    ed = _rows(e, dev, aligned)
    if shared:
        u, rs = _rows(d, dev, aligned), 0
    else:
        u, rs = _slab(u3, dev, aligned)
    loss, z, lse = rl.relation_softmax_forward(u, rs, ed, truth, scale, filt, frow, fcol)
    back = rl.relation_softmax_backward(u, rs, ed, truth, scale, g, z)
    return [z, lse, loss] + (list(back) if shared else [_blocks(back, rs, k).contiguous()])


def _same(a, b, what):
    for j, (x, y) in enumerate(zip(a, b)):
        assert V.same_bits(x, y, f"{what}, result {j}")


@pytest.mark.parametrize("shared,k,n_rel,aligned", [(False, 300, 65, True), (True, 600, 3, True), (False, 17, 130, False),
                                                    (True, 64, 64, False)])
def test_a_pair_alone_has_the_bits_it_has_in_a_batch_and_filters_that_drop_nothing_change_no_bit(rl, ops, gpu_device, shared,
                                                                                                 k, n_rel, aligned):
    dev, p = gpu_device, 33
    case = RC.random_case(p, n_rel, k, None if shared else 5, seed=k + n_rel, filtered=True)
    d, w, e, truth, mask, scale, g = (case[x] for x in ("d", "w", "e", "truth", "mask", "scale", "g"))
    u3 = RC.slab_of(d, w, n_rel).float()
    td, gd_ = truth.to(dev), g.to(dev)
    filt, frow, fcol = _filter(ops, mask, truth, dev)
    run = lambda rows=slice(None), al=aligned, f=(filt, frow, fcol): _kernels(        # noqa: E731
        rl, dev, u3[rows], d[rows], e, td[rows], scale, gd_[rows], al, shared, f[0],
        None if f[1] is None else f[1][rows], None if f[2] is None else f[2][rows])
    full = run()
    _same(full, run(), "second run")
    _same(full, run(al=not aligned), "the other load path")
    for i in (0, 1, 16, 32):
        _same([x[i:i + 1] for x in full], run(slice(i, i + 1)), f"pair {i} alone")
    perm = torch.randperm(p, generator=torch.Generator().manual_seed(1))
    _same([x[perm.to(dev)] for x in full], run(perm), "permuted")
    # the filter: a rebuilt one, one with every known triple listed three times, the raw edges in another order
    kh, kr, kt, h, t = RC.triples_of_mask(mask, truth)
    for name, (a, b, c_) in (("rebuilt", (kh, kr, kt)), ("tripled", (kh.repeat(3), kr.repeat(3), kt.repeat(3))),
                             ("reversed", (kh.flip(0), kr.flip(0), kt.flip(0)))):
        other = ops.csr_build_device(2 * p, a.to(dev), c_.to(dev), b.to(dev))
        _same(full, run(f=(other, frow, fcol)), f"{name} filter")
    # no filter, an empty one, one without an edge of these pairs, one whose rows h_i hold other tails than t_i (h_i <
    # t_i: the search ends past the row; every second row also t_i + 1: it ends on another entry), one that knows only
    # the truths: the same bits
    plain = run(f=(None, None, None))
    z0 = torch.zeros(0, dtype=torch.int64, device=dev)
    empty = ops.csr_build_device(2 * p, z0, z0, z0)
    elsewhere = ops.csr_build_device(2 * p, (h + 1).to(dev) % (2 * p), h.to(dev), torch.zeros(p, dtype=torch.int64, device=dev))
    ah, at = RC.tails_around(h, t, 2 * p)
    around = ops.csr_build_device(2 * p, ah.to(dev), at.to(dev), torch.zeros(ah.numel(), dtype=torch.int64, device=dev))
    truths = ops.csr_build_device(2 * p, h.to(dev), t.to(dev), td)
    for name, f in (("empty", empty), ("edge-less", elsewhere), ("other tails", around), ("truths only", truths)):
        _same(plain, run(f=(f, frow, fcol)), f"{name} filter")
    assert not torch.equal(plain[2], full[2])                 # (the real filter does change the loss)


@pytest.mark.parametrize("shared", [False, True])
def test_masking_equals_an_e_row_so_far_away_that_its_exp_underflows(rl, ops, gpu_device, shared):
    dev, p, n_rel, k = gpu_device, 33, 65, 64
    case = RC.random_case(p, n_rel, k, None if shared else 5, seed=11)
    d, w, e, scale, g = (case[x] for x in ("d", "w", "e", "scale", "g"))
    dropped = torch.tensor([3, 17, 64])
    truth = torch.randint(0, n_rel, (p,), generator=torch.Generator().manual_seed(2))
    truth[torch.isin(truth, dropped)] = 5
    mask = torch.zeros((p, n_rel), dtype=torch.bool)
    mask[:, dropped] = True
    u3 = RC.slab_of(d, w, n_rel).float()
    td, gd_ = truth.to(dev), g.to(dev)
    filt, frow, fcol = _filter(ops, mask, truth, dev)
    masked = _kernels(rl, dev, u3, d, e, td, scale, gd_, True, shared, filt, frow, fcol)
    far = e.clone()
    far[dropped, 0] += 1.0e4                                  # z about -3.7e7: expf underflows to exactly 0
    moved = _kernels(rl, dev, u3, d, far, td, scale, gd_, True, shared)
    keep = torch.ones(n_rel, dtype=torch.bool)
    keep[dropped] = False
    keep = keep.to(dev)
    assert bool((masked[0][:, ~keep] == -math.inf).all()) and bool((moved[0][:, ~keep] < -1e6).all())
    assert V.same_bits(masked[0][:, keep], moved[0][:, keep], "z of the kept relations")
    assert V.same_bits(masked[1], moved[1], "lse") and V.same_bits(masked[2], moved[2], "loss")
    if shared:
        assert V.same_bits(masked[3], moved[3], "gd") and V.same_bits(masked[4][:, keep], moved[4][:, keep], "c")
        assert bool((masked[4][:, ~keep] == 0).all()) and bool((moved[4][:, ~keep] == 0).all())
    else:
        assert V.same_bits(masked[3][:, keep], moved[3][:, keep], "G of the kept relations")
        assert bool((masked[3][:, ~keep] == 0).all()) and bool((moved[3][:, ~keep] == 0).all())


@pytest.mark.parametrize("shared", [False, True])
def test_a_nan_in_one_pair_leaves_the_other_pairs_bits(rl, gpu_device, shared):
    dev, p, n_rel, k = gpu_device, 9, 5, 20
    case = RC.random_case(p, n_rel, k, None if shared else 7, seed=4)
    leaves = lambda dd: [x.to(dev).requires_grad_(True) if x is not None else None     # noqa: E731
                         for x in (dd, case["w"], case["e"])]
    clean = rl.relation_softmax_loss(*leaves(case["d"]), case["truth"].to(dev), scale=case["scale"])
    bad = case["d"].clone()
    bad[4, 2] = float("nan")
    got = rl.relation_softmax_loss(*leaves(bad), case["truth"].to(dev), scale=case["scale"])
    keep = torch.arange(p) != 4
    assert bool(torch.isnan(got[4])) and bool(torch.isfinite(clean).all())
    assert V.same_bits(got[keep.to(dev)], clean[keep.to(dev)], "the other pairs' losses")


# ----------------------------------------------------------------------------- the whole op
def _engines(ops, rl, p, c, n_rel, k, rows, dev, shared):
    """the engines of the backward products of the op, asked for with the shapes it launches"""
    if shared:
        e_de = ops.gemm_engine(torch.empty((p, n_rel), device=dev), torch.empty((p, k + 1), device=dev), trans_a=True,
                               beta=1.0, out=torch.empty((n_rel, k + 1), device=dev))
        return None, e_de
    rows = min(rows, p)
    gm, wcat = torch.empty((rows, n_rel * k), device=dev), torch.empty((c, n_rel * k), device=dev)
    ws = min(max(1, rl.DD_SLICE // k) * k, n_rel * k)
    e_dd = ops.gemm_engine(gm[:, :ws], wcat[:, :ws], trans_b=True, beta=1.0, out=torch.empty((p, c), device=dev)[:rows])
    e_acc = ops.gemm_engine(torch.empty((p, c + 1), device=dev)[:rows], gm, trans_a=True, beta=1.0,
                            out=torch.empty((c + 1, n_rel * k), device=dev))
    return e_dd, e_acc


def _loss32(dev, d, w, e, truth, mask, scale):
    """the loss of the dense float32 torch head on the device (its own product included)"""
    u3 = RC.slab_of(d.to(dev), None if w is None else w.to(dev), e.shape[0], torch.float32)
    return RC.loss_eval(u3, e.to(dev), truth.to(dev), None if mask is None else mask.to(dev), scale, torch.float32)[2]


def _op_loss_bound(ops, r32, n_rel, k, engine, cw):
    """max(3 r_torch32, the kernels' count + twice the forward product's own bound at r_torch32 = 0): the product hands the
    kernels blocks within its bound of sum |d| |W|, and a logit takes a block's relative error twice (the square)"""
    return max(3.0 * r32, RC.loss_roundings(n_rel, k) * RC.U + (0.0 if engine is None else 2.0 * C.gemm_bound(engine, 0.0, cw)))


def _run_op(rl, dev, case, needs=(True, True, True), chunk_bytes=None, filt=None, frow=None, fcol=None, g=None):
    """(loss, [dd, dw, de]) of the op; a leaf that needs no gradient (or w in shared mode) gets None"""
    leaves = [None if x is None else x.to(dev).detach().requires_grad_(need)
              for x, need in zip((case["d"], case["w"], case["e"]), needs)]
    kw = {} if chunk_bytes is None else dict(chunk_bytes=chunk_bytes)
    loss = rl.relation_softmax_loss(*leaves, case["truth"].to(dev), scale=case["scale"], filt=filt, filter_row=frow,
                                    filter_col=fcol, **kw)
    if any(x is not None and x.requires_grad for x in leaves):
        loss.backward((case["g"] if g is None else g).to(dev))
    return loss.detach(), [None if x is None else x.grad for x in leaves]


OP_SHAPES = [(33, 65, 64, "D", True), (5, 3, 300, 5, False), (33, 130, 17, 300, True), (2, 2, 4, 5, True),
             (33, 65, 300, None, True), (5, 3, 17, None, False), (33, 130, 64, None, True)]


@pytest.mark.parametrize("p,n_rel,k,c,filtered", OP_SHAPES)
def test_op_gradients_against_float64_under_the_bounds_of_their_engines(rl, ops, gpu_device, p, n_rel, k, c, filtered):
    """On exact-logit cases, for the reason the kernels' checks use them: a float32 logit of magnitude 55 is rounded by
    2^-19 whoever computes it, every softmax takes that as a relative error, and the ratio of two float32 evaluations'
    errors is then chance, not a property of the products.  With exact logits what is measured is the products."""
    dev = gpu_device
    case = RC.exact_case(p, n_rel, k, c, seed=p + n_rel + k, filtered=filtered)
    case["g"] = RC.upstream(p, k)
    d, w, e, truth, mask, scale, g = (case[x] for x in ("d", "w", "e", "truth", "mask", "scale", "g"))
    shared = w is None
    u3 = RC.slab_of(d, w, n_rel)
    ref = RC.loss_eval(u3, e, truth, mask, scale)
    want = RC.grads_eval(u3, d, w, e, truth, mask, scale, g)
    a64 = RC.autograd_eval(d, w, e, truth, mask, scale, g, torch.float64)
    a32 = RC.autograd_eval(d.to(dev), None if shared else w.to(dev), e.to(dev), truth.to(dev), mask, scale, g.to(dev),
                           torch.float32)
    filt, frow, fcol = _filter(ops, mask, truth, dev)
    loss, grads = _run_op(rl, dev, case, filt=filt, frow=frow, fcol=fcol)
    r32 = float(RC.loss_measure(_loss32(dev, d, w, e, truth, mask, scale), ref).max())
    cw = d.shape[1]
    e_fwd = None if shared else ops.gemm_engine(d.to(dev), torch.empty((cw, n_rel * k), device=dev))
    bound = _op_loss_bound(ops, r32, n_rel, k, e_fwd, cw)
    r = float(RC.loss_measure(loss, ref).max())
    print(f"loss: r {r:.3g}, r_torch32 {r32:.3g}, bound {bound:.3g} (forward engine {e_fwd})")
    assert r <= bound, (r, bound)
    e_dd, e_acc = _engines(ops, rl, p, cw, n_rel, k, rl.chunk_rows(p, n_rel, k), dev, shared)
    for name, got, x32, x64, engine, depth in (("dd", grads[0], a32[0], a64[0], e_dd, n_rel * k),
                                               ("dw", grads[1], a32[1], a64[1], e_acc, p),
                                               ("de", grads[2], a32[2], a64[2], e_acc, p)):
        if got is None:
            assert name == "dw" and shared
            continue
        scale64 = want[name + "_scale"]
        r32 = C.worst(x32.cpu(), want[name], scale64)
        if engine is None:                                       # shared mode's dd is the kernel's own gd
            bound = RC.grad_bound(r32, n_rel, k, "gd")
        else:
            bound = C.gemm_bound(engine, r32, depth)
        r, r_auto = C.worst(got.cpu(), want[name], scale64), C.worst(got.cpu(), x64, scale64)
        print(f"{name}: r {r:.3g} (autograd64 {r_auto:.3g}), r_torch32 {r32:.3g}, bound {bound:.3g} (engine {engine})")
        assert r <= bound and r_auto <= bound, (name, r, r_auto, bound)


@pytest.mark.parametrize("c", [5, None])
def test_every_subset_of_gradients_keeps_the_bits_of_the_others(rl, ops, gpu_device, c):
    dev = gpu_device
    case = RC.random_case(33, 65, 64, c, seed=9, filtered=True)
    filt, frow, fcol = _filter(ops, case["mask"], case["truth"], dev)
    loss, full = _run_op(rl, dev, case, filt=filt, frow=frow, fcol=fcol)
    again_loss, again = _run_op(rl, dev, case, filt=filt, frow=frow, fcol=fcol)
    assert V.same_bits(loss, again_loss, "loss, second run")
    for needs in itertools.product((True, False), repeat=3):
        one_loss, some = _run_op(rl, dev, case, needs=needs, filt=filt, frow=frow, fcol=fcol)
        assert V.same_bits(loss, one_loss, f"loss, needs {needs}")
        for j, (need, a, b, b2) in enumerate(zip(needs, some, full, again)):
            if not need or b is None:
                assert a is None, (needs, j)
            else:
                assert V.same_bits(a, b, f"gradient {j}, needs {needs}") and V.same_bits(b, b2, f"gradient {j}, second run")


def test_chunking(rl, ops, gpu_device):
    dev, p, n_rel, k = gpu_device, 33, 5, 20
    one = n_rel * k * 4
    # shared mode: no slab, chunk_bytes changes no bit (and bounds nothing: one pair's would-be slab may exceed it)
    case = RC.random_case(p, n_rel, k, None, seed=5, filtered=True)
    filt, frow, fcol = _filter(ops, case["mask"], case["truth"], dev)
    loss, grads = _run_op(rl, dev, case, filt=filt, frow=frow, fcol=fcol)
    for cb in (one, 7 * one, 1):
        l2, g2 = _run_op(rl, dev, case, chunk_bytes=cb, filt=filt, frow=frow, fcol=fcol)
        assert V.same_bits(loss, l2, f"shared mode, chunk_bytes {cb}")
        assert V.same_bits(grads[0], g2[0], "dd") and V.same_bits(grads[2], g2[2], "de")
    # slab mode: the same bounds hold one pair per chunk and with several chunks; the loss from a GIVEN slab is identical
    case = RC.random_case(p, n_rel, k, 7, seed=6, filtered=True)
    d, w, e, truth, mask, scale, g = (case[x] for x in ("d", "w", "e", "truth", "mask", "scale", "g"))
    filt, frow, fcol = _filter(ops, mask, truth, dev)
    u3 = RC.slab_of(d, w, n_rel)
    ref = RC.loss_eval(u3, e, truth, mask, scale)
    want = RC.grads_eval(u3, d, w, e, truth, mask, scale, g)
    a32 = RC.autograd_eval(d.to(dev), w.to(dev), e.to(dev), truth.to(dev), mask, scale, g.to(dev), torch.float32)
    r32 = float(RC.loss_measure(_loss32(dev, d, w, e, truth, mask, scale), ref).max())
    e_fwd = {cb: ops.gemm_engine(d.to(dev)[:rl.chunk_rows(p, n_rel, k, cb)], torch.empty((7, n_rel * k), device=dev))
             for cb in (one, 7 * one, rl.CHUNK_BYTES)}
    for cb in (one, 7 * one, rl.CHUNK_BYTES):
        rows = rl.chunk_rows(p, n_rel, k, cb)
        assert rows == {one: 1, 7 * one: 7}.get(cb, p)
        loss, grads = _run_op(rl, dev, case, chunk_bytes=cb, filt=filt, frow=frow, fcol=fcol)
        bound = _op_loss_bound(ops, r32, n_rel, k, e_fwd[cb], 7)
        r = float(RC.loss_measure(loss, ref).max())
        assert r <= bound, (cb, r, bound)
        e_dd, e_acc = _engines(ops, rl, p, 7, n_rel, k, rows, dev, False)
        for name, got, x32, engine, depth in (("dd", grads[0], a32[0], e_dd, n_rel * k), ("dw", grads[1], a32[1], e_acc, p),
                                              ("de", grads[2], a32[2], e_acc, p)):
            bound = C.gemm_bound(engine, C.worst(x32.cpu(), want[name], want[name + "_scale"]), depth)
            r = C.worst(got.cpu(), want[name], want[name + "_scale"])
            print(f"chunk_bytes {cb} ({rows} pairs): {name} r {r:.3g}, bound {bound:.3g} (engine {engine})")
            assert r <= bound, (cb, name, r, bound)
    u, rs = _slab(u3.float(), dev, True)
    ed, td = e.to(dev), truth.to(dev)
    whole = rl.relation_softmax_forward(u, rs, ed, td, scale, filt, frow, fcol)
    for rows in (1, 7):
        parts = [rl.relation_softmax_forward(u[lo:lo + rows], rs, ed, td[lo:lo + rows], scale, filt, frow[lo:lo + rows],
                                             fcol[lo:lo + rows]) for lo in range(0, p, rows)]
        for j in range(3):
            assert V.same_bits(torch.cat([x[j] for x in parts]), whole[j], f"{rows} pairs per launch, result {j}")
    # one pair's slab beyond chunk_bytes: refused, both numbers named
    with pytest.raises(ValueError, match=f"one pair's slab takes {one} bytes .* chunk_bytes is {one - 1}"):
        _run_op(rl, dev, case, chunk_bytes=one - 1, filt=filt, frow=frow, fcol=fcol)


def test_empty_batch_and_operand_errors(rl, gpu_device):
    dev = gpu_device
    d, w, e = torch.randn(0, 8, device=dev, requires_grad=True), torch.randn(4, 8, 6, device=dev, requires_grad=True), \
        torch.randn(4, 6, device=dev, requires_grad=True)
    loss = rl.relation_softmax_loss(d, w, e, torch.zeros(0, dtype=torch.int64, device=dev))
    assert loss.shape == (0,) and loss.dtype == torch.float32
    loss.sum().backward()
    assert d.grad.shape == (0, 8) and bool((w.grad == 0).all()) and bool((e.grad == 0).all())
    d = torch.randn(3, 8, device=dev)
    t3 = torch.zeros(3, dtype=torch.int64, device=dev)
    for args, msg in (((d, w[:, :, :5], e, t3), "w is"), ((d, None, e, t3), "shared mode"), ((d, w, e, t3[:2]), "2 truths for 3"),
                      ((d, w, e[:0], t3), "at least one relation")):
        with pytest.raises(ValueError, match=msg):
            rl.relation_softmax_loss(*args)
    with pytest.raises(ValueError, match="a filter needs filter_row and filter_col"):
        rl.relation_softmax_loss(d, w.detach(), e.detach(), t3, filt=(t3, t3, t3, t3))


# ----------------------------------------------------------------------------- perturbations
@contextlib.contextmanager
def perturbation(mode):
    with contextlib.ExitStack() as stack:
        if mode == "side stream + poison 0xFF":
            stack.enter_context(V.side_stream())
        stack.enter_context(V.poisoned(0x7F if mode == "poison 0x7F" else 0xFF))
        yield
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", [5, None])
def test_the_op_keeps_its_bits_under_poison_and_on_a_side_stream(rl, ops, gpu_device, c):
    """forward (z, lse, loss and the slab are uninitialised allocations) and the whole backward, several chunks in slab
    mode, with a filter, and with one gradient left out"""
    dev, p, n_rel, k = gpu_device, 33, 65, 300
    case = RC.random_case(p, n_rel, k, c, seed=41, filtered=True)
    filt, frow, fcol = _filter(ops, case["mask"], case["truth"], dev)
    torch.cuda.synchronize()

    def run():
        out = []
        for needs in ((True, True, True), (False, True, True)):
            loss, grads = _run_op(rl, dev, case, needs=needs, chunk_bytes=8 * n_rel * k * 4, filt=filt, frow=frow, fcol=fcol)
            out += [loss] + [x for x in grads if x is not None]
        return out

    plain = run()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in plain)
    for mode in MODES:
        with perturbation(mode):
            got = run()
        for j, (a, b) in enumerate(zip(plain, got)):
            assert V.same_bits(a, b, f"{mode}, result {j}")
