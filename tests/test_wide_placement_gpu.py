"""GPU: every row-strided operand of every C entry point, spread over more than 2^32 elements (wide_cases.py holds the
placement and the harness).

A case is the body of an existing test, called with explicit arguments at the smallest shapes that enter each dispatch
branch (the table in the docstring of test_invariance_gpu.py), with its own float64 oracle and bound unchanged.  The
harness runs it once with every strided operand on its narrow twin placement and once per operand with that operand alone
on the wide placement; it substitutes the placements at the C boundary, so a wrapper that would copy a strided view
cannot hide the operand, and the pointer record of each wide pass proves a launch received an address inside the store.

  judged in every pass       the body's own assertions: the family's float64 bound (op_audit.bound_for, rowwise_cases,
                             index_cases, softmax_cases, ...), in the twin pass and in each wide pass
  bit for bit                every output of every launch (strided and flat) of the wide pass against the same launch of
                             the twin pass, and the results a query-side judge returns; only the outputs of
                             wide_cases.WAIVED (float atomics in the launches that use them, buffers filled through an
                             atomic slot counter) are exempt, by (entry point, output); a launch whose inputs differ from
                             the twin pass's (downstream of such an output) is counted as skipped
  gathered operands          wide_cases.GATHERED: the pass fails unless the case's ids hit a row past 2^32 elements and one
                             in [2^31, 2^32)
  expected operands          EXPECT: the operands a case must run wide (C under each tiling, the weights of both losses, ...)
  poison                     after each pass the whole 28 GB store is 0xFF again
  ledger                     test_ledger: every (entry point, operand) of include/*.h that takes a row stride was run wide
                             in this process or is in EXEMPT with one of three kinds of reason

The module allocates the store once (26.6 GiB); with less than 40 GiB free it skips and says so."""
import contextlib
import functools
import re

import numpy as np
import pytest
import torch

import invariance as V
import wide_cases as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(gpu_device):
    import __graft_entry__ as ge
    ge.build()
    import literalkg_amd
    return literalkg_amd


@pytest.fixture(scope="module")
def H(L, gpu_device):
    """the harness over the one store of this module"""
    from literalkg_amd import _native
    free, _ = torch.cuda.mem_get_info()
    if free < 40 * 2 ** 30:
        pytest.skip(f"the wide placement needs a 26.6 GiB store and 40 GiB free; {free / 2 ** 30:.1f} GiB are free")
    store = W.new_store(32, gpu_device)
    W.poison(store)
    h = W.Harness(_native, store)
    yield h
    del h.store, store
    torch.cuda.empty_cache()


@contextlib.contextmanager
def patched(module, **attrs):
    """a test module's shape lists, narrowed for the duration of one case"""
    saved = {k: getattr(module, k) for k in attrs}
    for k, v in attrs.items():
        setattr(module, k, v)
    try:
        yield
    finally:
        for k, v in saved.items():
            setattr(module, k, v)


def _fixture_body(f):
    return getattr(f, "__wrapped__", f)


# ----------------------------------------------------------------------------- the operands each case must run wide
def _ops(entry, *labels):
    return {(entry, x) for x in labels}


# case-name prefix -> the (entry point, operand) pairs the case must have resolved for a wide pass (an operand the harness
# could not resolve, or refused, fails the case instead of being printed only); every matching prefix applies
EXPECT = {
    "gather_rows d": _ops("lkg_gather_rows_f32", "src", "dst"),
    "gather_rows_range": _ops("lkg_gather_rows_range_f32", "src", "dst"),
    "fill_rows": _ops("lkg_fill_rows_f32", "dst"),
    "scatter_add_rows": _ops("lkg_scatter_add_rows_f32", "src", "dst"),
    "scatter_add repeated": _ops("lkg_scatter_add_rows_range_f32", "src", "dst"),
    "spmm_scatter_bwd": _ops("lkg_spmm_csr_scatter_bwd_f32", "g_out", "g_x"),
    "layernorm 9 x": _ops("lkg_act_layernorm_fwd_f32", "z", "y", "yn") | _ops("lkg_act_layernorm_bwd_f32", "z", "y", "g_y", "g_yn", "g_z"),
    "layernorm 257 x": _ops("lkg_act_layernorm_fwd_f32", "z", "y", "yn") | _ops("lkg_act_layernorm_bwd_f32", "z", "y", "g_y", "g_yn", "g_z"),
    "layernorm narrow": _ops("lkg_act_layernorm_fwd_f32", "z", "y", "yn") | _ops("lkg_narrow_layer_bwd_f32", "x", "w", "z", "y", "g_y", "g_x"),
    "relu batchnorm": _ops("lkg_relu_batchnorm_fwd_f32", "z", "y") | _ops("lkg_relu_batchnorm_bwd_f32", "z", "g_y", "g_z"),
    "elementwise": _ops("lkg_eltwise_f32", "a", "b", "out") | _ops("lkg_gate_blend_fwd_f32", "x", "gpre", "zpre", "out") |
    _ops("lkg_bi_mix_fwd_f32", "ego", "side", "h0p", "out_sum", "out_prod"),
    "column sums": _ops("lkg_colsum_f32", "x") | _ops("lkg_colsum_weighted_f32", "x", "w", "out_w"),
    "spmm d": _ops("lkg_spmm_csr_fused_f32", "x", "out"),
    "spmm epilogues": _ops("lkg_spmm_csr_fused_f32", "x", "out", "self", "add2"),
    "spmm plain": _ops("lkg_spmm_csr_f32", "x", "out", "self") | _ops("lkg_spmm_csr_fused_f32", "copy_src", "copy_dst"),
    "attention refresh": _ops("lkg_edge_softmax_f32", "ent", "relemb"),
    "table scores transe": _ops("lkg_transe_score_fwd_f32", "emb", "relemb") |
    _ops("lkg_transe_score_bwd_f32", "emb", "relemb", "g_emb", "g_rel"),
    "table scores dot": _ops("lkg_dot_score_fwd_f32", "emb") | _ops("lkg_dot_score_bwd_f32", "emb", "g_emb"),
    "transr scores": _ops("lkg_dense_score_fwd_f32", "ph+pp+pn", "relemb") |
    _ops("lkg_dense_score_bwd_f32", "ph+pp+pn", "relemb", "g_ph+g_pp+g_pn", "g_rel") | _ops("lkg_grouped_gemm_f32", "a", "b", "c"),
    "grouped rows": _ops("lkg_grouped_gemm_f32", "a", "b", "c"),
    "gemm layouts": _ops("lkg_gemm_f32", "a", "b", "c"),
    "engine bf16x3": _ops("lkg_gemm_f32", "a", "b", "c"), "engine f32_mfma": _ops("lkg_gemm_f32", "a", "b", "c"),
    "engine longk": _ops("lkg_gemm_longk_f32", "a", "b", "c"), "engine skinny": _ops("lkg_gemm_skinny_f32", "a", "b", "c"),
    "engine smallm": _ops("lkg_gemm_smallm_f32", "a", "b", "c"), "gemm f64acc": _ops("lkg_gemm_f64acc_f32", "a", "b", "c"),
    "wgrad": _ops("lkg_gemm_wgrad_f32", "a", "b", "c"),
    "ordered": _ops("lkg_gemm_ordered_f32", "a", "b", "c"),
    "tall ": _ops("lkg_gemm_tall_f32", "a[0]", "b[0]", "c"),                       # A and C under each tiling
    "tall gate epilogue": _ops("lkg_gemm_tall_f32", "a[1]", "b[1]", "b[2]", "b[3]", "gate_g", "gate_z"),
    "fused layer": _ops("lkg_linear_act_layernorm_fwd_f32", "a[0]", "w[0]", "y", "yn"),
    "fused layer two panels": _ops("lkg_linear_act_layernorm_fwd_f32", "a[1]", "w[1]"),
    "narrow layer backward": _ops("lkg_narrow_layer_bwd_f32", "x", "w", "z", "y", "g_y", "g_yn", "g_x"),
    "kvs_all": _ops("lkg_sigmoid_all_partial_f32", "q", "p") | _ops("lkg_sigmoid_all_weights_f32", "q", "p", "v"),
    "self-adversarial": _ops("lkg_nssa_fwd_f32", "q", "p", "n") | _ops("lkg_nssa_bwd_f32", "q", "p", "n", "dq", "dp", "dn"),
    "relation loss": _ops("lkg_relation_loss_fwd_f32", "u", "e", "z") | _ops("lkg_relation_loss_bwd_f32", "u", "e", "z"),
    "relation loss 33 x 65 x 300 c None": _ops("lkg_relation_loss_bwd_f32", "gd", "c"),
    "gate statistics, separate": _ops("lkg_gate_blend_bwd_stats_f32", "x", "gpre", "zpre", "g_out", "g_x", "g_gpre", "g_zpre", "w"),
    "row and column maxima": _ops("lkg_row_absmax_f32", "x") | _ops("lkg_col_absmax_f32", "x"),
    "attention row range": _ops("lkg_edge_softmax_f32", "ent"),
    "grouped k": _ops("lkg_grouped_gemm_f32", "a", "b"),
    "fused linear layernorm edges": _ops("lkg_linear_act_layernorm_fwd_f32", "a[0]", "w[0]", "y"),
    "gate backward statistics": _ops("lkg_gate_blend_bwd_stats_f32", "x", "gpre", "zpre", "g_out", "g_x", "w"),
    # the query side
    "test_ranking": _ops("lkg_rank_queries_f32", "p", "q") | _ops("lkg_rank_prepare_f32", "q", "p") | _ops("lkg_rank_count_f32", "q", "p"),
    # (the distance scorings; 'dot', the third width, has no relation row and no squared norms)
    "test_ranking-0": _ops("lkg_rank_queries_f32", "e") | _ops("lkg_rank_sqnorm_f32", "p"),
    "test_ranking-1": _ops("lkg_rank_queries_f32", "e") | _ops("lkg_rank_sqnorm_f32", "p"),
    "test_topk": _ops("lkg_topk_select_f32", "q", "p"), "test_accepted": _ops("lkg_accept_count_f32", "q", "p") |
    _ops("lkg_accept_emit_f32", "q", "p"),
    "test_retrieval": _ops("lkg_retrieval_prepare_f32", "q", "p") | _ops("lkg_retrieval_count_f32", "q", "p"),
    "test_triples": _ops("lkg_triple_scores_f32", "p"),
    "test_triples-0": _ops("lkg_triple_scores_f32", "e"), "test_triples-1": _ops("lkg_triple_scores_f32", "e"),
    "test_relations": _ops("lkg_relation_scores_f32", "p", "e", "out") | _ops("lkg_relation_order_f32", "scores"),
    "test_pair_head": _ops("lkg_pair_mlp_scores_f32", "uq", "v", "out") | _ops("lkg_pair_mlp_select_f32", "uq", "v") |
    _ops("lkg_pair_mlp_prepare_f32", "uq", "v") | _ops("lkg_pair_mlp_count_f32", "uq", "v") | _ops("lkg_pair_mlp_pairs_f32", "u", "v"),
    "test_softmax_op": _ops("lkg_softmax_all_finish_f32", "q", "p"),
    "test_softmax_op-0": _ops("lkg_softmax_all_partial_f32", "q", "p") | _ops("lkg_softmax_all_weights_f32", "q", "p", "v"),
    "test_softmax_op-2": _ops("lkg_softmax_all_partial_f32", "q", "p") | _ops("lkg_softmax_all_weights_f32", "q", "p", "v"),
    "test_softmax_op-1": _ops("lkg_softmax_all_partial_masked_f32", "q", "p") | _ops("lkg_softmax_all_weights_masked_f32", "q", "p", "v"),
    "test_softmax_op-3": _ops("lkg_softmax_all_partial_masked_f32", "q", "p") | _ops("lkg_softmax_all_weights_masked_f32", "q", "p", "v"),
}


def expected_ran_wide(name, resolved):
    want = set().union(*[v for k, v in EXPECT.items() if name.startswith(k)])
    assert want, f"{name}: no operands declared in EXPECT"
    assert want <= set(resolved), f"{name}: operands that had to run wide and were not resolved: {sorted(want - set(resolved))}"


RAN = []

# ----------------------------------------------------------------------------- a. the harness on the device
def test_store_and_placement(H, gpu_device):
    """The store is poison; a placed table carries its values, its base is 16-byte aligned, its rows start where
    check_geometry says; cleared, the store is poison again; a stray write is found and named."""
    assert W.all_poison(H.store)
    for n, d in ((9, 5), (257, 32)):
        values = torch.randn(n, d, device=gpu_device)
        view = W.place(H.store, values)
        assert view.data_ptr() % 16 == 0 and view.stride(0) % 4 == 0 and W.inside(H.store, view.data_ptr())
        assert view.data_ptr() == H.store.data_ptr() + 4 * W.pad_elems(32)
        assert (n - 1) * view.stride(0) >= 2 ** 32 and W.carries(view, values) and not W.all_poison(H.store)
        t = W.twin(values)
        assert t.stride(0) == 4 * -(-d // 4) + 4 and t.data_ptr() % 16 == 0 and W.carries(t, values)
        W.clear(view)
        assert W.all_poison(H.store)
    H.store[W.pad_elems(32) + 2 ** 32 + 7] = 1.0
    assert not W.all_poison(H.store) and W.first_stain(H.store, 32) == 2 ** 32 + 7
    W.poison(H.store)
    assert W.all_poison(H.store)


# ----------------------------------------------------------------------------- b. the query side and the softmax loss
QUERY = [("test_ranking", w) for w in range(3)] + [("test_topk", w) for w in range(3)] + \
        [("test_accepted", w) for w in range(3)] + [("test_retrieval", w) for w in range(3)] + \
        [("test_triples", w) for w in range(3)] + [("test_relations", w) for w in range(2)] + [("test_pair_head", 0)] + \
        [("test_softmax_op", w) for w in range(4)]


@pytest.mark.parametrize("name,which", QUERY, ids=[f"{n}-{w}" for n, w in QUERY])
def test_query_side(H, L, gpu_device, name, which):
    """The cases of test_invariance_gpu.py (65 queries x 257 candidates, k = 17 and 32, splits 1 and 3, with and without a
    KnownTriples filter), their oracles unchanged: its four_ways is replaced by the harness's twin and wide passes."""
    import test_invariance_gpu as TIV
    from literalkg_amd import ops, ranking
    args = {"test_ranking": lambda: (L, ranking, gpu_device) + TIV.WIDTHS[which],
            "test_topk": lambda: (L, ranking, gpu_device) + TIV.WIDTHS[which],
            "test_accepted": lambda: (L, ranking, gpu_device) + TIV.WIDTHS[which],
            "test_retrieval": lambda: (L, ranking, gpu_device) + TIV.WIDTHS[which],
            "test_triples": lambda: (L, gpu_device) + [("transr", 120, 37, 32), ("transe", 128, 33, 33),
                                                        ("dot", 100, 64, 64)][which],
            "test_relations": lambda: (L, gpu_device) + [("transr", 11), ("transe", 11)][which],
            "test_pair_head": lambda: (L, ranking, gpu_device),
            "test_softmax_op": lambda: (ops, gpu_device) + [(17, False), (17, True), (32, False), (32, True)][which]}[name]()
    seen = []
    # (11 relations instead of 5: a relation table needs 9 rows to be spread over the store)
    with patched(TIV, N_REL=11, four_ways=lambda run, judge: seen.append(H.case(run, judge, f"{name}-{which}"))):
        getattr(TIV, name)(*args)
    print(f"{name}-{which}: operands run wide: {sorted({p for tw in seen for p in tw.pairs})}; "
          f"unresolved {sorted({p for tw in seen for p in tw.unresolved})}")
    expected_ran_wide(f"{name}-{which}", {p for tw in seen for p in tw.pairs})
    RAN.append((name, which))


# ----------------------------------------------------------------------------- c. the training side
def gemm_layouts(ops, dev, k):
    """lkg_gemm_f32 (or the engine ops.gemm picks) in its four layouts at m, n = 129, 130, with beta = 1 and a bias, against
    float64 under the engine's bound (test_conditioning_gpu.check)."""
    import test_conditioning_gpu as TC
    m, n = 129, 130
    gen = torch.Generator(device=dev).manual_seed(k)
    a_op, b_op = torch.randn(m, k, device=dev, generator=gen), torch.randn(k, n, device=dev, generator=gen)
    bias = torch.randn(n, device=dev, generator=gen)
    for ta in (False, True):
        for tb in (False, True):
            a = a_op.t().contiguous() if ta else a_op
            b = b_op.t().contiguous() if tb else b_op
            engine = ops.gemm_engine(a, b, trans_a=ta, trans_b=tb)
            got = ops.gemm(a, b, trans_a=ta, trans_b=tb)
            TC.check(engine, got, a_op, b_op, f"gemm {'T' if ta else 'N'}{'T' if tb else 'N'} k {k}")
            got = ops.gemm(a, b, trans_a=ta, trans_b=tb, bias=bias)
            TC.check(ops.gemm_engine(a, b, trans_a=ta, trans_b=tb, bias=bias), got, a_op, b_op, f"gemm + bias k {k}", bias=bias)


def spmm_plain(ops, N, dev, structure, d):
    """lkg_spmm_csr_f32, which no Python caller reaches (every SpMM goes through the fused entry point): the same structure
    and operands through both entry points, the plain one held to the fused one's float64 check (rowwise_cases.check_spmm)."""
    import rowwise_cases as C
    g = structure
    lines = []
    for draw in C.SPMM_DRAWS[:2]:
        case = C.draw_spmm(dev, g.n, g.nnz, d, draw, False)
        self_ = torch.randn(g.n, d, device=dev, generator=C.gen_for(dev, 77 + d))
        for lr in (None, g.long_rows(False)):
            out = torch.empty(g.n, d, device=dev)
            N.call("lkg_spmm_csr_f32", g.n, d, N.ptr(g.rowptr), N.ptr(g.col), N.ptr(case.val), N.ptr(case.x), d, N.ptr(out), d,
                   None, 0, N.ptr(lr), lr.numel() if lr is not None else 0, ops.LONG_ROW_THRESHOLD if lr is not None else 0,
                   ops._stream())
            C.check_spmm(lines, f"plain {case.what}", g.rowptr, g.col, case.val, case.x, g.n, out)
            both = torch.empty(g.n, d, device=dev)
            N.call("lkg_spmm_csr_f32", g.n, d, N.ptr(g.rowptr), N.ptr(g.col), N.ptr(case.val), N.ptr(case.x), d, N.ptr(both), d,
                   N.ptr(self_), d, N.ptr(lr), lr.numel() if lr is not None else 0,
                   ops.LONG_ROW_THRESHOLD if lr is not None else 0, ops._stream())
            want = ops.spmm_raw(g.rowptr, g.col, case.val, case.x, g.n, long_rows=lr, add_self=self_)
            V.same_bits(both, want, f"plain + self {case.what}")
            cdst = torch.empty(g.n, d, device=dev)                  # the copy that rides along in the fused epilogue
            again = ops.spmm_raw(g.rowptr, g.col, case.val, case.x, g.n, long_rows=lr, add_self=self_, copy=(self_, cdst))
            V.same_bits(again, want, f"fused + copy {case.what}")
            V.same_bits(cdst, self_, f"the copied rows {case.what}")


def gate_stats_separate(ops, N, dev, d, n_w):
    """lkg_gate_blend_bwd_stats_f32 with g_gpre and g_zpre in tensors of their own (the model writes them side by side in
    one): the three gradients carry the bits of lkg_gate_blend_bwd_f32 -- which test_elementwise holds to float64 -- and
    the statistics meet the float64 checks of test_gpu_parity.test_gate_backward_statistics_ride_along."""
    torch.manual_seed(d)
    n = 1027
    x, gt, zs, go = (torch.randn(n, d, device=dev) for _ in range(4))
    gt, zs = torch.tanh(gt), torch.sigmoid(zs)
    w = torch.rand(n, max(n_w, 1), device=dev)
    outs = []
    for stats_mode in (False, True):
        gx, gg, gz = (torch.empty(n, d, device=dev) for _ in range(3))
        rm = torch.empty(n, device=dev)
        if stats_mode:
            n_stats = (5 + 2 * n_w) * d
            ws, st = torch.empty(1024 * n_stats, device=dev), torch.empty(n_stats, device=dev)
            N.call("lkg_gate_blend_bwd_stats_f32", n, d, N.ptr(x), d, N.ptr(gt), d, N.ptr(zs), d, N.ptr(go), d, N.ptr(gx), d,
                   N.ptr(gg), d, N.ptr(gz), d, 1, N.ptr(rm), N.ptr(w) if n_w else None, w.shape[1], n_w, N.ptr(ws), ws.numel(),
                   N.ptr(st), None)
        else:
            N.call("lkg_gate_blend_bwd_f32", n, d, N.ptr(x), d, N.ptr(gt), d, N.ptr(zs), d, N.ptr(go), d, N.ptr(gx), d,
                   N.ptr(gg), d, N.ptr(gz), d, 1, N.ptr(rm), None)
        outs.append((gx, gg, gz, rm))
    for a, b, what in zip(*outs, ("g_x", "g_gpre", "g_zpre", "rowmax")):
        V.same_bits(a, b, f"gate backward with statistics: {what}")
    gpz64 = torch.cat([outs[0][1], outs[0][2]], 1).double()
    assert float((st[:2 * d].double() - gpz64.sum(0)).abs().max()) <= 2e-6 * float(gpz64.abs().sum(0).max())
    assert torch.equal(st[2 * d:4 * d], gpz64.float().abs().amax(0)) and torch.equal(st[4 * d:5 * d], x.abs().amax(0))
    if n_w:
        want = gpz64.t() @ w[:, :n_w].double()
        got = st[5 * d:].view(n_w, 2 * d).t().double()
        assert float((got - want).abs().max()) <= 2e-6 * float((gpz64.abs().t() @ w[:, :n_w].double()).max())


@pytest.fixture(scope="module")
def bodies(L, gpu_device):
    import index_cases as I
    import rowwise_cases as RWC
    import self_adversarial_cases as S
    import test_conditioning_gpu as TC
    import test_gemm_ordered_gpu as TGO
    import test_gpu_parity as TG
    import test_index_kernels_gpu as TI
    import test_kvs_all_gpu as TK
    import test_relation_loss_gpu as TRL
    import test_rowwise_conditioning_gpu as TW
    import test_self_adversarial_gpu as TS
    from literalkg_amd import _native as N
    import importlib
    GO = importlib.import_module("literalkg_amd.gemm_ordered")
    from literalkg_amd import kvs_all as kv
    from literalkg_amd import ops
    g = gpu_device
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(g)
    spmm = _fixture_body(TW.spmm_structure)(ops, g)
    att = _fixture_body(TW.att_structures)(ops, g)
    sa = _fixture_body(TS.sa)(g)
    rl = _fixture_body(TRL.rl)(g)
    pairs = [(0, 0), (-90, 80)]                                  # two of the 17 scale pairs of test_conditioning_gpu.py
    sa_cases = [c for c in S.CASES if c[2] == 33][:3]            # 33 groups: q, p of 33 rows, 33 K negatives

    def scaled(fn, *a):
        def run():
            with patched(TC, SCALE_PAIRS=pairs):
                fn(ops, g, *a)
        return run

    def relations11(fn):
        def run():                                                   # (11 relations: a relation table of 9 rows or more)
            with patched(RWC, draw_triples=functools.partial(RWC.draw_triples, n_rel=11)):
                fn()
        return run

    def ordered(layout):
        def run():
            with patched(TGO, MS=(129,), NS=(130,), KS=(33, 4097), SPLITS=(1, 3)):
                TGO.test_every_element_is_within_the_stated_bound_of_float64(GO, g, layout)
        return run

    out = {
        # the row gathers and scatters, the fill, the transposed scatter of the SpMM backward
        **{f"gather_rows d {d}": (lambda d=d: TI.test_gather_rows(ops, N, dev, g, d)) for d in (3, 64)},
        **{f"gather_rows_range d {d}": (lambda d=d: TI.test_gather_rows_range(ops, N, dev, g, d)) for d in (5, 64)},
        **{f"fill_rows d {d}": (lambda d=d: TI.test_fill_rows(ops, N, dev, g, d)) for d in (5, 64)},
        **{f"scatter_add_rows d {d}": (lambda d=d: TI.test_scatter_add_rows_with_perm(ops, N, g, d)) for d in (5, 130)},
        "scatter_add repeated ids": lambda: TC.test_scatter_add_rows_with_repeated_ids(ops, g),
        **{f"spmm_scatter_bwd d {d}": (lambda d=d: TI.test_spmm_scatter_bwd(ops, N, g, d)) for d in (1, 5, 64, 130)},
        # the row-wise kernels: n = 9 and 257, d in {5, 64, 257} (LayerNorm refuses 257: widths above 256 need d % 4 == 0; 260)
        **{f"layernorm {n} x {d}": (lambda n=n, d=d: TW.test_layernorm(ops, g, n, d, False, False, False))
           for n in (9, 257) for d in (5, 64, 260)},
        "layernorm narrow": lambda: TW.test_layernorm(ops, g, 4099, 32, False, True, False),
        **{f"relu batchnorm {n} x {d}": (lambda n=n, d=d: TW.test_relu_batchnorm(ops, g, n, d, 0, True))
           for n in (9, 257) for d in (5, 64, 257)},
        "relu batchnorm eval": lambda: TW.test_relu_batchnorm(ops, g, 257, 64, 0, False),
        **{f"elementwise d {d}": (lambda d=d: TW.test_elementwise(ops, N, g, d, False)) for d in (3, 32, 300)},
        "column sums": lambda: TC.test_column_sums_under_cancellation(ops, g, 300_001),
        "row and column maxima": lambda: TC.test_row_and_column_maxima_are_exact(ops, g),
        # SpMM: the narrow-row, the wave-per-row and the slab paths, forward and transpose, the epilogues and flagged forms
        **{f"spmm d {d}": (lambda d=d: TW.test_spmm_conditioning(ops, g, spmm, d, False)) for d in (1, 8, 32, 130, 256)},
        **{f"spmm epilogues d {d}": (lambda d=d: TW.test_spmm_epilogues(ops, g, spmm, d, False)) for d in (1, 8, 32, 130, 256)},
        **{f"spmm plain d {d}": (lambda d=d: spmm_plain(ops, N, g, spmm, d)) for d in (8, 130)},
        # the attention refresh and the score kernels
        **{f"attention refresh d {d}": (lambda d=d, o=o: TW.test_attention_refresh(ops, g, att, d, o))
           for d, o in ((4, False), (30, True), (128, False))},
        "attention row range": lambda: TW.test_attention_row_range(ops, g, att),
        **{f"table scores {f} dim {dim}": relations11(lambda f=f, dim=dim: TW.test_table_scores_and_losses(ops, g, f, dim, 17, False))
           for f in ("transe", "dot") for dim in (3, 32)},
        **{f"transr scores dim {dim}": relations11(lambda dim=dim: TW.test_transr_scores_and_losses(ops, g, dim, 17, 7))
           for dim in (3, 32)},
        # the GEMM families
        "grouped rows": lambda: TW.test_grouped_rows(ops, g, 33, 70, False, 0.0),
        "grouped rows trans_b": lambda: TW.test_grouped_rows(ops, g, 33, 70, True, 0.0),
        "grouped k": lambda: TW.test_grouped_k(ops, g, 40, 24, 1.0, 0.0),
        "gemm layouts k 33": lambda: gemm_layouts(ops, g, 33),
        "gemm layouts k 8003": lambda: gemm_layouts(ops, g, 8003),
        **{f"engine {c}": scaled(TC.test_other_engines_scale_sweep, c)
           for c in ("bf16x3_rows", "bf16x3_kmajor", "longk", "f32_mfma", "skinny", "smallm")},
        "gemm f64acc": lambda: TC.test_gemm_f64acc_is_one_rounding_of_float64(ops, g),
        "wgrad f16x2": scaled(TC.test_wgrad_f16x2_scale_sweep, 16 * 2500),
        "wgrad f16x2 k + 5": scaled(TC.test_wgrad_f16x2_scale_sweep, 16 * 2500 + 5),
        **{f"ordered {i}": ordered(lay) for i, lay in zip(TGO.LAYOUT_IDS, TGO.LAYOUTS)},
        **{f"tall {v}": scaled(TC.test_tall_scale_sweep, v) for v in (None, "256x2", "128x1", "256x1")},
        "tall gate epilogue": scaled(TC.test_tall_gate_epilogue_scale_sweep, None),
        "fused linear layernorm edges": lambda: TC.test_fused_linear_act_layernorm_at_the_range_edges(ops, g),
        "fused layer epilogue": lambda: TG.test_fused_layer_epilogue_matches_the_unfused_pair(ops, g, 16384 + 5, (32,), 32, 0.0),
        "fused layer two panels": lambda: TG.test_fused_layer_epilogue_matches_the_unfused_pair(ops, g, 16384 + 5, (64, 64), 128,
                                                                                               0.0),
        "narrow layer backward": lambda: TG.test_narrow_layer_backward_in_one_launch_matches_the_unfused_passes(
            ops, g, 4096 + 7, "both", 0.0),
        # the losses that test_query_side does not reach
        **{f"kvs_all {b} x {n} x {k}": (lambda b=b, n=n, k=k: TK.test_gradients_against_float64(ops, kv, g, b, n, k))
           for b, n, k in ((65, 257, 17), (130, 255, 32))},
        **{f"self-adversarial {i}": (lambda c=c: TS.test_loss_and_gradients_on_exact_logit_tables(sa, g, c))
           for i, c in enumerate(sa_cases)},
        **{f"relation loss {p} x {r} x {k} c {c}": (lambda p=p, r=r, k=k, c=c: TRL.test_op_gradients_against_float64_under_the_bounds_of_their_engines(
            rl, ops, g, p, r, k, c, True)) for p, r, k, c in ((33, 65, 64, "D"), (33, 130, 17, 300), (33, 65, 300, None))},
        # the gate backward with its column statistics
        **{f"gate backward statistics d {d}": (lambda d=d, n_w=n_w: TG.test_gate_backward_statistics_ride_along(ops, g, d, n_w))
           for d, n_w in ((64, 2), (100, 1))},
        **{f"gate statistics, separate outputs d {d}": (lambda d=d, n_w=n_w: gate_stats_separate(ops, N, g, d, n_w))
           for d, n_w in ((64, 2), (100, 1))},
    }
    assert list(out) == BODIES, sorted(set(out) ^ set(BODIES))
    return out


BODIES = (
    [f"gather_rows d {d}" for d in (3, 64)] + [f"gather_rows_range d {d}" for d in (5, 64)] +
    [f"fill_rows d {d}" for d in (5, 64)] + [f"scatter_add_rows d {d}" for d in (5, 130)] + ["scatter_add repeated ids"] +
    [f"spmm_scatter_bwd d {d}" for d in (1, 5, 64, 130)] +
    [f"layernorm {n} x {d}" for n in (9, 257) for d in (5, 64, 260)] + ["layernorm narrow"] +
    [f"relu batchnorm {n} x {d}" for n in (9, 257) for d in (5, 64, 257)] + ["relu batchnorm eval"] +
    [f"elementwise d {d}" for d in (3, 32, 300)] + ["column sums", "row and column maxima"] +
    [f"spmm d {d}" for d in (1, 8, 32, 130, 256)] + [f"spmm epilogues d {d}" for d in (1, 8, 32, 130, 256)] +
    [f"spmm plain d {d}" for d in (8, 130)] +
    [f"attention refresh d {d}" for d in (4, 30, 128)] + ["attention row range"] +
    [f"table scores {f} dim {dim}" for f in ("transe", "dot") for dim in (3, 32)] +
    [f"transr scores dim {dim}" for dim in (3, 32)] +
    ["grouped rows", "grouped rows trans_b", "grouped k", "gemm layouts k 33", "gemm layouts k 8003"] +
    [f"engine {c}" for c in ("bf16x3_rows", "bf16x3_kmajor", "longk", "f32_mfma", "skinny", "smallm")] +
    ["gemm f64acc", "wgrad f16x2", "wgrad f16x2 k + 5"] + [f"ordered {i}" for i in ("NN", "NT", "TN", "TT")] +
    [f"tall {v}" for v in (None, "256x2", "128x1", "256x1")] +
    ["tall gate epilogue", "fused linear layernorm edges", "fused layer epilogue", "fused layer two panels",
     "narrow layer backward"] +
    [f"kvs_all {b} x {n} x {k}" for b, n, k in ((65, 257, 17), (130, 255, 32))] +
    [f"self-adversarial {i}" for i in range(3)] +
    [f"relation loss {p} x {r} x {k} c {c}" for p, r, k, c in ((33, 65, 64, "D"), (33, 130, 17, 300), (33, 65, 300, None))] +
    [f"gate backward statistics d {d}" for d in (64, 100)] + [f"gate statistics, separate outputs d {d}" for d in (64, 100)])


@pytest.mark.parametrize("name", BODIES)
def test_training_side(H, bodies, name):
    """An existing body, its own float64 assertions unchanged, in the twin pass and with each strided operand wide."""
    try:
        tw = H.case(bodies[name], None, name)
    except AssertionError as e:
        raise AssertionError(f"{name}: {e}") from e
    print(f"{name}: {len(tw.pairs)} operands run wide: {tw.pairs}; unresolved {tw.unresolved}")
    expected_ran_wide(name, tw.pairs)
    RAN.append(name)


# ----------------------------------------------------------------------------- d. the ledger
# (entry point, operand) -> reason.  Three kinds only, each to be checked in the header:
#   host-only      the entry point launches nothing (it answers a question about a shape or an alignment)
#   one row        the operand has one row by contract
#   capped         the header caps the operand's extent below 2^31 bytes (the line is quoted)
HOST_ONLY = ("lkg_gemm_longk_ok", "lkg_gemm_smallm_ok", "lkg_gemm_skinny_ok", "lkg_narrow_layer_bwd_ok")
EXEMPT = {
    **{pair: "host-only: include/literalkg_hip.h declares it without a stream; it tests shapes and alignments and launches nothing"
       for pair in sorted(W.ledger_pairs()) if pair[0] in HOST_ONLY},
}


def test_ledger(H):
    """Every (entry point, operand) that include/*.h declares with a row stride was run wide by a case of this process --
    its pass judged by the case's oracle and its pointer record -- or is in EXEMPT; everything run wide outside the
    outputs of WAIVED was also compared bit for bit, in a launch that received it.  Run the module whole."""
    wanted = set(QUERY) | set(BODIES)
    assert wanted <= set(RAN), f"the ledger counts the cases that ran before it in this process: not run {sorted(wanted - set(RAN), key=str)}"
    pairs = W.ledger_pairs()
    assert len(pairs) >= 200 and set(EXEMPT) <= pairs
    covered = {(e, re.sub(r"\[\d+\]$", "", o)) for e, o in H.covered}
    print(f"{H.passes} passes; {len(covered)} of {len(pairs)} (entry point, operand) pairs run wide, {len(EXEMPT)} exempt")
    for pair in sorted(H.covered):
        print("  ", pair, sorted(H.covered[pair]))
    shapes = {s for v in H.covered.values() for s in v}
    assert shapes <= set(W.SHAPES), f"shapes placed wide that wide_cases.SHAPES (the host test's list) lacks: {sorted(shapes - set(W.SHAPES))}"
    stray = covered & set(EXEMPT)
    assert not stray, f"exempt, yet run wide: {sorted(stray)}"
    missing = pairs - covered - set(EXEMPT)
    assert not missing, f"{len(missing)} strided operands were never run wide: {sorted(missing)}"
    # bit equality: a comparison of a launch that received the operand wide, or every output of those launches waived
    unjudged = {p: t for p, t in H.judged.items() if not t[0] and (t[2] or not t[1])}
    waived_only = sorted(p for p, t in H.judged.items() if not t[0])
    print(f"every output waived (float64 bound only): {waived_only}")
    print(f"launches skipped because their inputs differed from the twin pass: { {p: t[2] for p, t in H.judged.items() if t[2]} }")
    assert not unjudged, f"run wide, yet no output of a launch that received it was compared (compared, waived, skipped): {unjudged}"
    assert {p[0] for p in waived_only} <= {e for e, _ in W.WAIVED}
