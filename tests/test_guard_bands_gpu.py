"""GPU: every pointer argument of every device entry point between guard bands (guard_cases.py holds the placement and the
harness).

A case is the body of an existing test -- the case tables of test_wide_placement_gpu.py and test_invariance_gpu.py, whose
shapes are the smallest that enter each dispatch branch, and the direct-drive bodies of the families that module leaves to
their own files -- with its float64 oracle and bound unchanged.  The harness runs it once plain and once flush: in the flush
pass every tensor a launch receives lies band | extent | band in a fresh 0xFF buffer, its end flush against the band.

  judged in both passes      the body's own assertions
  bands, gaps, const inputs  after every launch of the flush pass, byte for byte
  bit for bit                every output of every launch of the flush pass against the same launch of the plain pass, and
                             the results a query-side judge returns; the exemptions are wide_cases.WAIVED, launches
                             downstream of a waived output (skipped), and `workspace` arguments (scratch)
  flat lengths, splits       test_flat_lengths_and_splits: existing bodies swept over elements (0, 1, 3, 4, 5, 63 .. 1025,
                             aligned and 4 bytes off), queries (1 .. 257), candidates, rows, and split counts 1 and the
                             largest; DESIGN.md 3.5e lists what is swept and what is not
  planted faults             three stand-in launches in torch, each with a correct twin
  ledger                     test_ledger, last: every required (entry point, pointer parameter) of include/literalkg_hip.h
                             was placed flush in this process.  Run the module whole.

There is no tolerance in this module: every check of its own is an equality of bits or of band bytes."""
import contextlib
import time

import numpy as np
import pytest
import torch

import guard_cases as G
import test_invariance_gpu as TIV
import test_wide_placement_gpu as TWP
import wide_cases as W

pytestmark = pytest.mark.gpu
T0 = time.time()
RAN = []


@pytest.fixture(scope="module")
def L(gpu_device):
    import __graft_entry__ as ge
    ge.build()
    import literalkg_amd
    return literalkg_amd


@pytest.fixture(scope="module")
def H(L, gpu_device):
    from literalkg_amd import _native
    return G.Flush(_native)


def _fixture_body(f):
    return getattr(f, "__wrapped__", f)


@contextlib.contextmanager
def patched(module, **attrs):
    saved = {k: getattr(module, k) for k in attrs}
    for k, v in attrs.items():
        setattr(module, k, v)
    try:
        yield
    finally:
        for k, v in saved.items():
            setattr(module, k, v)


def told(name, passes):
    print(f"{name}: " + "; ".join(f"{p.launches} launches, {p.compared} outputs compared, {p.waived} waived, {p.skipped} skipped, "
                                  f"unresolved {sorted(p.unresolved)}" for p in passes))


# ----------------------------------------------------------------------------- a. the harness sees planted faults, on the device
FAULTS = {"write past the end": "parameter dst: the band behind was written, the first byte at offset 0 ",
          "write before the start": "parameter dst: the band in front was written, the first byte at offset -4 ",
          "read past the end": "elements differ"}


@pytest.mark.parametrize("n", [1, 5, 257])
def test_planted_faults_and_their_twins(gpu_device, tmp_path, n):
    """Stand-in launches in torch that reach memory through Flush.table alone (the arena of the launch, or the slab the
    test owns): every access stays inside owned memory.  The caller's tensors are slices of slabs of ordinary numbers."""
    from test_guard_bands_host import HEADER, MARGIN
    (tmp_path / "standins.h").write_text(HEADER)
    protos = W.prototypes(str(tmp_path))

    class Native:
        def ptr(self, t):
            return None if t is None else t.data_ptr()

        def call(self, name, *args):
            k_map(*args)

    N = Native()
    H = G.Flush(N, protos, W.strided_operands(protos))
    slabs = []

    def f32(addr, m):
        return H.table(addr, 4 * m, slabs).view(torch.float32)

    def k_map(n, src, dst, fault, home, stream):
        x = f32(src, n).clone()
        if fault == "read past the end":
            x[n - 1] = f32(src + 4 * n, 1)[0]
        f32(dst, n).copy_(x * 2 + 1)
        if fault == "write past the end":
            f32(dst + 4 * n, 1).zero_()
        if fault == "write before the start":
            f32(dst - 4, 1).zero_()

    def carve(seed):
        slab = torch.randn(n + 2 * MARGIN, device=gpu_device, generator=torch.Generator(device=gpu_device).manual_seed(seed))
        slabs.append(slab)
        return slab[MARGIN:MARGIN + n]

    def case(fault):
        def run():
            src, dst = carve(n), carve(n + 1)
            N.call("lkg_t_map_f32", n, N.ptr(src), N.ptr(dst), fault, N.ptr(dst), None)
            return dst
        return H.case(run, lambda res, mode: dict(dst=res), f"map {fault}")

    fl = case(0)
    assert fl.launches == 1 and fl.compared == 1 and not H.unresolved
    assert H.tally[("lkg_t_map_f32", "src")]["held"] == 1 and H.tally[("lkg_t_map_f32", "dst")]["held"] == 1
    for fault, message in FAULTS.items():
        with pytest.raises(AssertionError, match=message):
            case(fault)


# ----------------------------------------------------------------------------- b. the query side
QUERY = [("test_ranking", w) for w in range(3)] + [("test_topk", w) for w in range(3)] + \
        [("test_accepted", w) for w in range(3)] + [("test_retrieval", w) for w in range(3)] + \
        [("test_triples", w) for w in range(3)] + [("test_relations", w) for w in range(2)] + [("test_pair_head", 0)] + \
        [("test_softmax_op", w) for w in range(4)] + [("test_softmax_excluded_lists", 0)] + \
        [("test_curve_fit_and_order_kernels", w) for w in range(2)] + \
        [("test_device_structure_and_laplacian", w) for w in range(2)] + \
        [("test_golden_model_queries", w) for w in range(3)] + [("test_golden_mlp_head", w) for w in range(2)]


@pytest.mark.parametrize("name,which", QUERY, ids=[f"{n}-{w}" for n, w in QUERY])
def test_query_side(H, L, gpu_device, name, which):
    """The cases of test_invariance_gpu.py, their oracles unchanged: its four_ways is replaced by the plain and flush passes."""
    from literalkg_amd import ops, ranking
    g = gpu_device
    widths = lambda: (L, ranking, g) + TIV.WIDTHS[which]
    args = {"test_ranking": widths, "test_topk": widths, "test_accepted": widths, "test_retrieval": widths,
            "test_triples": lambda: (L, g) + [("transr", 120, 37, 32), ("transe", 128, 33, 33), ("dot", 100, 64, 64)][which],
            "test_relations": lambda: (L, g) + [("transr", 5), ("transe", 300)][which],
            "test_pair_head": lambda: (L, ranking, g),
            "test_softmax_op": lambda: (ops, g) + [(17, False), (17, True), (32, False), (32, True)][which],
            "test_softmax_excluded_lists": lambda: (L, ops, ranking, g),
            "test_curve_fit_and_order_kernels": lambda: (ops, g, (1, 7)[which]),
            "test_device_structure_and_laplacian": lambda: (L, g, ("random-walk", "symmetric")[which]),
            "test_golden_model_queries": lambda: (L, ranking, g) + [("encoder_gcn_l2_gatenum", "transr"), ("transe_gcn_l1", "transe"),
                                                                     ("encoder_gcn_l1", "dot")][which],
            "test_golden_mlp_head": lambda: (L, ranking, g, ("mlp_model_gcn_l1_scale", "mlp_bce_gcn_l2_scale")[which])}[name]()
    seen = []
    with patched(TIV, four_ways=lambda run, judge: seen.append(H.case(run, judge, f"{name}-{which}"))):
        getattr(TIV, name)(*args)
    assert seen and all(p.launches for p in seen), f"{name}-{which}: a case launched nothing"
    told(f"{name}-{which}", seen)
    RAN.append((name, which))


# ----------------------------------------------------------------------------- c. the training side
FLAT_N = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
OTHERS = ["negatives tail", "negatives bernoulli pool", "cardinalities and answer counts", "neighbour sample f 4",
          "neighbour sample f 64", "pair accept 65 x 257", "pair accept 1 x 3", "lists transr", "lists dot",
          "kvs_all entry points", "bi-interaction d 32", "adam second betas", "lists reported transe",
          "retrieval candidate subset", "last layer backward on the listed rows", "narrow layer backward, flagged rows"]
FLAT = ["flat group_by_key", "flat gather_i64 and permute", "flat check_grouped", "flat sanitize_ids",
        "flat gather_i64 past the grid cap"]


@pytest.fixture(scope="module")
def bodies(L, gpu_device):
    import index_cases as I
    import test_index_kernels_gpu as TI
    import test_dropout_mask_gpu as TD
    import test_gpu_parity as TG
    import test_kvs_all_surface_gpu as TKS
    import test_lists_gpu as TLS
    import test_negatives_gpu as TN
    import test_neighbors_gpu as TNB
    import test_pair_accepted_gpu as TPA
    import test_retrieval_gpu as TR
    import test_rowwise_conditioning_gpu as TW
    import negative_cases as NC
    import neighbor_cases as NBC
    from literalkg_amd import _native as N
    from literalkg_amd import kvs_all as kv
    from literalkg_amd import ops, ranking
    g = gpu_device
    dev = dev0 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(g)
    out = {f"wide: {k}": v for k, v in _fixture_body(TWP.bodies)(L, g).items()}
    out.update({f"invariance: {k}": v for k, v in _fixture_body(TIV.bodies)(L, ops, N, g).items()})
    known = _fixture_body(TN.known)(L, g)
    graph = _fixture_body(TNB.device_graph)(dev)
    tail = next(c for c in NC.CONFIGS if c[0] == "tail")
    bern = next((c for c in NC.CONFIGS if c[0] == "bernoulli" and c[1] is not None), NC.CONFIGS[-1])
    sel = list(NBC.SELECTIONS)[0]

    def gather_and_permute(n, shifted=False):
        """the two launches of TI.test_gather_i64_and_permute with its checks, at any length (its own assertion on the
        number of planted indices holds from 6 elements on); shifted: every input one element in from its allocation,
        so the int32 and float32 arrays start 4 bytes off the 16-byte grid"""
        dev = (lambda a: torch.cat([dev0(a)[:1], dev0(a)])[1:]) if shifted else dev0
        rng = np.random.default_rng(n)
        src = rng.integers(-2 ** 62, 2 ** 62, n + 3, dtype=np.int64)
        perm = rng.integers(0, n + 3, n).astype(np.int32)
        perm[-1] = n + 2
        dst = TI.ibuf(g, n, torch.int64)
        sd, pd = dev(src), dev(perm)
        N.call("lkg_gather_i64", n, N.ptr(sd), N.ptr(pd), N.ptr(dst), ops._stream())
        I.check_gather_i64(f"gather_i64 n {n}", src, perm, TI.host(dst))
        perm, n_src, srcf, planted = I.draw_permute(n)
        out = TI.fbuf(g, n + I.PAD)
        pd, sd = dev(perm), dev(srcf)
        N.call("lkg_permute_f32", n, N.ptr(pd), n_src, N.ptr(sd), N.ptr(out), ops._stream())
        I.check_permute(f"permute n {n}", perm, n_src, srcf, TI.host(out))

    def lengths(fn):
        def run():
            for n in FLAT_N:
                fn(n)
        return run

    out.update({
        "negatives tail": lambda: TN.test_draw_equals_the_reference_entry_for_entry(L, g, known, *tail),
        "negatives bernoulli pool": lambda: TN.test_draw_equals_the_reference_entry_for_entry(L, g, known, *bern),
        "cardinalities and answer counts": lambda: TN.test_cardinalities_answer_counts_and_weights_equal_the_double_loops(L, g, known),
        "neighbour sample f 4": lambda: TNB.test_sample_equals_the_reference(ops, N, dev, graph, sel, 4),
        "neighbour sample f 64": lambda: TNB.test_sample_equals_the_reference(ops, N, dev, graph, sel, 64),
        "pair accept 65 x 257": lambda: TPA.test_exact_integer_op(L, ranking, ops, g, 65, 257),
        "pair accept 1 x 3": lambda: TPA.test_exact_integer_op(L, ranking, ops, g, 1, 3),
        "lists transr": lambda: TLS.test_counts_on_the_devices_own_scores(L, g, *TLS.SHAPES[0], 5),
        "lists dot": lambda: TLS.test_counts_on_the_devices_own_scores(L, g, *TLS.SHAPES[-1], 1),
        "kvs_all entry points": lambda: TKS.test_partial_gradients_are_the_all_trainable_bits_or_none(kv, g, True),
        "bi-interaction d 32": lambda: TW.test_elementwise(ops, N, g, 32, True),
        "adam second betas": lambda: TI.test_adam_against_float64(ops, N, g, _fixture_body(TI.adam_big)(g), 2, (0.8, 0.95), 0.01),
        "lists reported transe": lambda: TLS.test_bits_of_score_triples(L, g, *next(s for s in TLS.SHAPES if s[0] == "transe"), 5),
        "retrieval candidate subset": lambda: TR.test_candidate_subset(L, ranking, g, "transe"),
        "last layer backward on the listed rows": lambda: TG.test_last_layer_backward_on_the_listed_rows_equals_the_dense_backward(ops, g),
        "narrow layer backward, flagged rows": lambda: TD.test_narrow_layer_draws_the_ports_mask(ops, g, 4099),
        "flat group_by_key": lengths(lambda n: TI.test_group_by_key(ops, N, dev, n, 100)),
        "flat gather_i64 and permute": lengths(lambda n: (gather_and_permute(n), gather_and_permute(n, True))),
        "flat check_grouped": lengths(lambda n: TI.test_check_grouped(ops, N, dev, g, n, "last")),
        "flat sanitize_ids": lengths(lambda n: TI.test_sanitize_ids(ops, N, dev, g, n, "last")),
        "flat gather_i64 past the grid cap": lambda: gather_and_permute(2048 * 256 + 3),
    })
    return out


BODIES = [f"wide: {n}" for n in TWP.BODIES] + [f"invariance: {n}" for n in TIV.BODIES] + OTHERS + FLAT


@pytest.mark.parametrize("body", BODIES)
def test_training_side(H, bodies, body):
    """An existing body, its own float64 assertions unchanged, plain and flush."""
    try:
        fl = H.case(bodies[body], None, body)
    except AssertionError as e:
        raise AssertionError(f"{body}: {e}") from e
    assert fl.launches, f"{body}: nothing was launched"
    told(body, [fl])
    RAN.append(body)


# ----------------------------------------------------------------------------- c2. flat lengths and split counts
QUERY_COUNTS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257)      # (the case tables hold 257 queries at the most)
SWEEPS = ["expand_groups", "index kernels, empty and 4 bytes off", "adam", "curve, fit and order", "topk by query count",
          "softmax finish by query count", "pair head by query count", "pair accept by query count",
          "pair accept by candidate count", "neighbour sample", "list counts", "topk splits", "softmax splits",
          "pair head splits", "ordered gemm splits", "ranking by query count", "accepted by query count",
          "retrieval by query count", "relations by query count", "excluded lists by query count",
          "loss reduce and table scores by batch", "kvs_all finish by query count", "extract rows",
          "csr_check by rows", "csr_check past the grid cap", "structure build, transpose and Laplacian", "sampler by groups",
          "negatives by groups and slots", "cardinalities by triples", "answer counts by groups",
          "elementwise past the grid cap"]


@pytest.fixture(scope="module")
def sweeps(L, H, gpu_device):
    """name -> a function that runs its cases through H.case itself: an existing body (or its launches and checks) at
    every length on both sides of a block or vector edge, empty, and one element off its allocation where it can be"""
    import index_cases as I
    import list_cases as LC
    import neighbor_cases as NBC
    import test_gemm_ordered_gpu as TGO
    import test_index_kernels_gpu as TI
    import test_lists_gpu as TLS
    import test_neighbors_gpu as TNB
    import test_pair_accepted_gpu as TPA
    import importlib
    from literalkg_amd import _native as N
    from literalkg_amd import ops, ranking
    import invariance as V
    import negative_cases as NC
    import test_kvs_all_gpu as TK
    import test_negatives_gpu as TN
    import test_rowwise_conditioning_gpu as TW
    from literalkg_amd import kvs_all as kv
    GO = importlib.import_module("literalkg_amd.gemm_ordered")
    FEW = (1, 3, 4, 5, 63, 64, 65, 257)
    g = gpu_device
    dev0 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(g)
    shifted = lambda a: torch.cat([dev0(a)[:1], dev0(a)])[1:] if np.asarray(a).size else dev0(a)
    seen, rewritten = [], []

    def case(run, judge=None, what=""):
        seen.append(H.case(run, judge, what))

    def through(what):
        return lambda run, judge: case(run, judge, what)

    def by_length(fn, lengths=(0,) + FLAT_N):
        def sweep():
            for n in lengths:
                case(lambda: fn(n), None, f"n {n}")
        return sweep

    def index_edges():
        for n in (0, 1, 5, 65, 257):
            for dev in (dev0, shifted):
                case(lambda: TI.test_group_by_key(ops, N, dev, n, 100), None, f"group_by_key n {n}")
                case(lambda: TI.test_check_grouped(ops, N, dev, g, n, "last"), None, f"check_grouped n {n}")
                case(lambda: TI.test_sanitize_ids(ops, N, dev, g, n, "last"), None, f"sanitize_ids n {n}")

    def adam(n):
        lines, hp = [], I.adam_hyper((0.9, 0.999), 0.01, 2)
        for draw in I.ADAM_DRAWS[:2]:
            c = I.draw_adam(g, n, draw)
            I.check_adam(lines, c, hp, *TI.run_adam(ops, N, c, hp))

    def curve_fit_order():
        for n in FLAT_N:
            for n_rel in (1, 7) if n >= 63 else (1,):
                with patched(TIV, N_KERNEL=n, four_ways=through(f"curve n {n} n_rel {n_rel}")):
                    TIV.test_curve_fit_and_order_kernels(ops, g, n_rel)

    def by_query_count(name, args, counts=QUERY_COUNTS):
        def sweep():
            for b in counts:
                with patched(TIV, B=b, four_ways=through(f"{name} B {b}")):
                    getattr(TIV, name)(*args)
        return sweep

    def neighbours():
        graph = _fixture_body(TNB.device_graph)(dev0)
        for sel in NBC.SELECTIONS:                                       # ("none": an empty selection)
            for f in (1, 4, 64, 65):
                case(lambda: TNB.test_sample_equals_the_reference(ops, N, dev0, graph, sel, f), None, f"sample {sel} f {f}")

    def list_counts():
        cs = TLS.case(L, *TLS.SHAPES[-1], 1, g)
        model, h, r, t, lists = cs["model"], cs["h"], cs["r"], cs["t"], cs["lists"]
        for side in TLS.SIDES:
            q, tru = TLS.ends(side, h, t)
            scores = L.score_lists(model, q, r, lists, side=side, kernel_scores=True)
            truth_scores = L.score_triples(model, h, r, t, side=side, kernel_scores=True)
            keep = LC.keep_mask(lists, tru, q, r, None, side)
            for b in QUERY_COUNTS:
                for m in (1, 17, 65):
                    ref = LC.counts(scores[:b, :m], truth_scores[:b], keep[:b, :m])

                    def run():
                        LC.check_ranks(L.rank_in_lists(model, h[:b], r[:b], t[:b], lists[:b, :m], side=side), ref,
                                       f"{side} {b} x {m}")
                    case(run, None, f"lists {side} {b} x {m}")

    def resplit(fn, to, position=None):
        """the body's three splits become `to`: no result depends on the split count, so its oracle stands"""
        def f(*a, **kw):
            a = list(a)
            if kw.get("splits") == 3:
                kw["splits"] = to
                rewritten.append(to)
            if position is not None and len(a) > position and a[position] == 3:
                a[position] = to
                rewritten.append(to)
            return fn(*a, **kw)
        return f

    def resplit_ran(what):
        assert rewritten, f"{what}: no call of the body carried splits = 3: the sweep ran at the body's own count"
        del rewritten[:]

    def topk_splits():
        with patched(L, predict_topk=resplit(L.predict_topk, ops.TOPK_MAX_SPLITS)), patched(TIV, four_ways=through("topk splits")):
            TIV.test_topk(L, ranking, g, *TIV.WIDTHS[2])
        resplit_ran("topk")

    def pair_head_splits():
        with patched(L, predict_topk=resplit(L.predict_topk, ops.TOPK_MAX_SPLITS)), patched(TIV, four_ways=through("pair head splits")):
            TIV.test_pair_head(L, ranking, g)
        resplit_ran("pair head")

    def softmax_splits():
        top = ops.SOFTMAX_MAX_SPLITS
        with patched(ops, softmax_all_forward=resplit(ops.softmax_all_forward, top, 5),
                     softmax_all_loss=resplit(ops.softmax_all_loss, top)), patched(TIV, four_ways=through("softmax splits")):
            for filtered in (False, True):
                TIV.test_softmax_op(ops, g, 17, filtered)
                resplit_ran("softmax")

    def ordered_splits():
        for layout in TGO.LAYOUTS[:2]:
            with patched(TGO, MS=(129,), NS=(130,), KS=(33, 4097), SPLITS=(1, 256)):
                case(lambda: TGO.test_every_element_is_within_the_stated_bound_of_float64(GO, g, layout), None, "ordered")

    def csr_check():
        for n_rows in (0,) + FLAT_N:
            rowptr, col = I.valid_csr(n_rows, 90, seed=n_rows)
            if n_rows == 0:
                col = I.valid_csr(5, 90)[1]                               # (no rows: the entries are not looked at)
            if col.size == 0:
                continue
            col = col.copy()
            if n_rows:
                col[-1] = 90                                              # a bad column in the last entry of the last row
            want = I.csr_check_ref(rowptr, n_rows, col.size, col, 0, 90)
            assert want == (1 if n_rows else 0)
            for dev in (dev0, shifted):                                   # (int32 arrays: the shifted ones start 4 bytes off)
                case(lambda: check(TI.run_csr_check(ops, N, dev, g, rowptr, n_rows, col, 0, 90), want), None,
                     f"csr_check {n_rows} rows")

    def check(got, want):
        assert got == want, (got, want)

    def structure():
        """KGStructure.from_triples on the device and the device Laplacian against the host build, array by array (the
        checks of TIV.test_device_structure_and_laplacian), at n entities and e triples, duplicates among them"""
        from literalkg_amd import io
        for n, e in [(1, 0), (1, 1), (3, 4), (5, 3)] + [(x, 4 * x) for x in (63, 64, 65, 255, 256, 257)] + [(17, 1025)]:
            rng = np.random.default_rng(1000 * n + e)
            h, t, r = rng.integers(0, n, e), rng.integers(0, n, e), rng.integers(0, 3, e)
            if e >= 4:
                h[-2:], t[-2:], r[-2:] = h[:2], t[:2], (r[:2] + 1) % 3   # two pairs twice, under another relation
            gh = L.KGStructure.from_triples(n, h, t, r, device="cpu")
            hd, td, rd = (dev0(x) for x in (h, t, r))
            for kind in ("random-walk", "symmetric"):
                want_val = io.laplacian_values(gh, kind)

                def run():
                    gd = L.KGStructure.from_triples(n, hd, td, rd, device=g)
                    return gd, io.laplacian_values(gd, kind), gd.coo_indices()

                def judge(res, mode):
                    gd, val, coo = res
                    assert (gd.n, gd.nnz, gd.n_raw, gd.has_dups) == (gh.n, gh.nnz, gh.n_raw, gh.has_dups), mode
                    out = dict(values=val, coo=coo, order=gd.order)
                    for name in TIV.STRUCTURE_ARRAYS:
                        a, b_ = gd.host(name), gh.host(name)
                        assert (a is None) == (b_ is None), (mode, name)
                        if a is not None:
                            assert a.dtype == b_.dtype and np.array_equal(a, b_), (mode, name)
                            out[name] = a
                    assert np.array_equal(gd.order, gh.order), mode
                    assert torch.equal(val.cpu(), want_val) and torch.equal(coo.cpu(), gh.coo_indices()), mode
                    return out
                case(run, judge, f"structure n {n} e {e} {kind}")

    def sampler():
        graphs = _fixture_body(TI.sampler_graphs)(ops, g)
        for name in ("dups", "no dups"):
            kind, bad = I.SAMPLER_CASES[name]
            gs, n, h, t, r = graphs[kind]
            heads_all = I.sampler_heads(kind, bad, n, h)
            for groups in (1, 3, 4, 5, 63, 64, 65, 255, 256, 257):
                for dev in (dev0, shifted):
                    heads, k, seed = heads_all[:groups], 5, 1
                    want = I.sampler_replica(seed, heads, k, h, t, r, gs.order)

                    def run():
                        out = torch.full((4, groups * k + I.PAD), I.ISENT, dtype=torch.int64, device=g)
                        hd = dev(heads)
                        N.call("lkg_sample_kg_batch", groups, k, seed, N.ptr(hd), gs.n, N.ptr(gs.rowptr), N.ptr(gs.col),
                               N.ptr(gs.eptr), N.ptr(gs.rel), gs.nnz, gs.n_raw, N.ptr(out[0]), N.ptr(out[1]), N.ptr(out[2]),
                               N.ptr(out[3]), ops._stream())
                        out = TI.host(out)
                        assert (out[:, groups * k:] == I.ISENT).all()
                        I.check_sampler(f"{name} groups {groups}", tuple(out[i, :groups * k] for i in range(4)), want)
                    case(run, None, f"sampler {name} groups {groups}")

    def negatives():
        known = _fixture_body(TN.known)(L, g)
        for corrupt, pool in (("tail", None), ("bernoulli", "pair")):
            ref = NC.reference(corrupt, pool, False)
            sampler_ = TN._sampler(L, known, g, corrupt, pool, False)
            for make in (lambda x: x, lambda x: torch.cat([x[:1], x])[1:]):       # (aligned; one element in)
                pos = tuple(make(x) for x in TN._dev(NC.positives(), g))
                for gr, k in [(gr, 5) for gr in (1, 3, 4, 5, 63, 64, 65, 129)] + [(5, k) for k in (1, 3, 4, 63, 64, 65, 255, 256, 257)]:
                    case(lambda: TN._assert_same(TN._draw(sampler_, pos, gr, k), NC.cut(ref, gr, k), f"G {gr} K {k}"), None,
                         f"negatives {corrupt} G {gr} K {k}")

    def cardinalities():
        kh, kr, kt = NC.graph()
        for e in [x for x in FLAT_N if x <= kh.size] + [kh.size]:
            want = NC.cardinalities(kh[:e], kr[:e], kt[:e])

            def run():
                known = L.KnownTriples(*TN._dev((kh[:e], kr[:e], kt[:e]), g), NC.N_ENT, NC.N_REL)
                card = L.relation_cardinalities(known)
                for got, w in zip((card.triples, card.heads, card.tails), want):
                    V.same_bits(got.cpu().numpy(), w, f"cardinality of {e} triples")
            case(run, None, f"cardinalities e {e}")

    def answer_counts():
        known = _fixture_body(TN.known)(L, g)
        kh, kr, kt = NC.graph()
        h, r, t = NC.positives()
        pos = TN._dev((h, r, t), g)
        for any_relation in (False, True):
            want = NC.answer_counts(kh, kr, kt, h, r, t, any_relation)
            for gr in (1, 3, 4, 5, 63, 64, 65, 129):
                def run():
                    for a, w in zip(L.answer_counts(known, *(x[:gr] for x in pos), any_relation=any_relation), want):
                        V.same_bits(a.cpu().numpy(), w[:gr].copy(), f"answer counts G {gr}")
                case(run, None, f"answer counts G {gr}")

    out = {
        "expand_groups": by_length(lambda n: [TI.test_expand_groups(ops, N, d, g, n, 3, 5) for d in (dev0, shifted)]),
        "index kernels, empty and 4 bytes off": index_edges,
        "adam": by_length(adam, FLAT_N),
        "curve, fit and order": curve_fit_order,
        "topk by query count": by_query_count("test_topk", (L, ranking, g) + TIV.WIDTHS[2]),
        "softmax finish by query count": by_query_count("test_softmax_op", (ops, g, 17, False)),
        "pair head by query count": by_query_count("test_pair_head", (L, ranking, g), (1, 3, 5, 64, 65)),
        "pair accept by query count": by_length(lambda n: TPA.test_exact_integer_op(L, ranking, ops, g, n, 17), QUERY_COUNTS),
        "pair accept by candidate count": by_length(lambda n: TPA.test_exact_integer_op(L, ranking, ops, g, 5, n), FLAT_N),
        "neighbour sample": neighbours, "list counts": list_counts, "topk splits": topk_splits,
        "softmax splits": softmax_splits, "pair head splits": pair_head_splits, "ordered gemm splits": ordered_splits,
        "ranking by query count": by_query_count("test_ranking", (L, ranking, g) + TIV.WIDTHS[2], FEW),
        "accepted by query count": by_query_count("test_accepted", (L, ranking, g) + TIV.WIDTHS[2], FEW),
        "retrieval by query count": by_query_count("test_retrieval", (L, ranking, g) + TIV.WIDTHS[2], FEW),
        "relations by query count": by_query_count("test_relations", (L, g, "transe", 5), FEW),
        "excluded lists by query count": by_query_count("test_softmax_excluded_lists", (L, ops, ranking, g), FEW),
        "loss reduce and table scores by batch": by_length(
            lambda n: [TW.test_table_scores_and_losses(ops, g, f, 3, n, False) for f in ("transe", "dot")], FLAT_N),
        "kvs_all finish by query count": by_length(lambda n: TK.test_gradients_against_float64(ops, kv, g, n, 255, 17), FEW),
        "extract rows": lambda: [case(lambda: TI.test_csr_extract_rows(ops, N, dev0, g, sel), None, f"extract {sel}")
                                 for sel in I.EXTRACT_SELECTIONS],
        "csr_check by rows": csr_check,
        "csr_check past the grid cap": lambda: case(lambda: TI.test_csr_check_second_trip(ops, N, dev0, g), None, "second trip"),
        "structure build, transpose and Laplacian": structure, "sampler by groups": sampler,
        "negatives by groups and slots": negatives, "cardinalities by triples": cardinalities,
        "answer counts by groups": answer_counts,
        "elementwise past the grid cap": lambda: case(lambda: TW.test_elementwise_grid_stride(ops, N, g, 32, 8192 * 32 + 3), None,
                                                      "grid stride"),
    }
    assert list(out) == SWEEPS
    return out, seen


@pytest.mark.parametrize("name", SWEEPS)
def test_flat_lengths_and_splits(sweeps, name):
    """Lengths on both sides of every block and vector edge, empty arrays, bases 4 bytes off the 16-byte grid, and split
    counts 1 and the largest: each case under its own oracle, plain and flush."""
    table, seen = sweeps
    del seen[:]
    try:
        table[name]()
    except AssertionError as e:
        raise AssertionError(f"{name}: {e}") from e
    assert seen and any(p.launches for p in seen), f"{name}: nothing was launched"
    print(f"{name}: {len(seen)} cases, {sum(p.launches for p in seen)} launches, {sum(p.compared for p in seen)} outputs compared")
    RAN.append(name)


# ----------------------------------------------------------------------------- d. what the pass and its reading found
# lkg_gemm_tall.hip loads A in 16-byte windows clamped to the panel's last whole window, a + 4 ((m - 1) lda + ka - 4) bytes:
# for a panel that ends before its fourth float that lies 4 .. 12 bytes IN FRONT of the panel, and every window of the
# launch is loaded from there.  The columns past ka are masked to zero, so no value changes and no value-based check can
# see it (the limit guard_cases.py states); the entry point now refuses such a panel before any launch, and ops.gemm_tall
# widens it with zero columns to one window.
SHORT_PANELS = [(1, 1), (1, 2), (1, 3), (2, 1), (3, 1)]             # (m, ka) with lda = ka: (m - 1) lda + ka < 4
SMALLEST_PANELS = [(1, 4), (1, 5), (2, 2), (2, 3), (4, 1), (5, 1)]  # one whole window, and one float more


def _tall_operands(dev, m, k):
    gen = torch.Generator().manual_seed(100 * m + k)
    a = torch.randint(-3, 4, (m, k), generator=gen).float().to(dev)        # (integers: every product and sum is exact)
    b = torch.randint(-3, 4, (k, 5), generator=gen).float().to(dev)
    return a, b


@pytest.mark.parametrize("m,k", SHORT_PANELS)
def test_tall_gemm_answers_a_panel_shorter_than_one_window(H, L, gpu_device, m, k):
    """ops.gemm_tall widens such a panel (and its block of B) with zero columns to one window: the same exact product, plain
    and between bands; the entry point itself refuses the bare panel before any launch."""
    import ctypes as C
    from literalkg_amd import _native, ops
    a, b = _tall_operands(gpu_device, m, k)

    def judge(out, mode):
        assert torch.equal(out.double(), a.double() @ b.double()), mode
        return dict(out=out)
    fl = H.case(lambda: ops.gemm_tall([a], [[b]], False), judge, f"tall {m} x {k}")
    assert fl.launches and not [key for key in fl.unresolved if key[0] == "lkg_gemm_tall_f32"], fl.unresolved
    assert H.panels.get(("lkg_gemm_tall_f32", "a[0]")) and H.panels.get(("lkg_gemm_tall_f32", "b[0]"))
    out, rm, ws = torch.empty(m, 5, device=gpu_device), a.abs().amax(1), torch.empty(1 << 20, dtype=torch.uint8, device=gpu_device)
    with pytest.raises(_native.LkgError, match="spans fewer than 4 floats"):
        _native.call("lkg_gemm_tall_f32", m, 5, 1, (C.c_void_p * 1)(a.data_ptr()), (C.c_int64 * 1)(k), (C.c_int32 * 1)(k),
                     rm.data_ptr(), 1, (C.c_void_p * 1)(b.data_ptr()), (C.c_int64 * 1)(5), 0, 1.0, 0.0, out.data_ptr(), 5, None, 0,
                     None, 0, None, 0, None, 0, ws.data_ptr(), ws.numel(), None)


@pytest.mark.parametrize("m,k", SMALLEST_PANELS)
def test_tall_gemm_on_the_smallest_panels_it_accepts(H, L, gpu_device, m, k):
    """The last window starts at the panel's first float, or one float in: exact products, plain and between bands."""
    from literalkg_amd import ops
    a, b = _tall_operands(gpu_device, m, k)

    def judge(out, mode):
        assert torch.equal(out.double(), a.double() @ b.double()), mode
        return dict(out=out)
    fl = H.case(lambda: ops.gemm_tall([a], [[b]], False), judge, f"tall {m} x {k}")
    told(f"tall {m} x {k}", [fl])


# ----------------------------------------------------------------------------- e. the ledger
def test_ledger(H):
    """Every required (entry point, pointer parameter) of the header was placed flush, alone in its placement, in a launch
    of this process whose bands were checked; every non-const one was also compared bit for bit, or is waived (its case's
    float64 bound judged it) or scratch.  A parameter only ever placed together with another (shared) is listed."""
    wanted = set(QUERY) | set(BODIES) | set(SWEEPS)
    assert wanted <= set(RAN), f"the ledger counts the cases that ran before it in this process: not run {sorted(wanted - set(RAN), key=str)}"
    counts, unheld, uncompared, shared_only = H.report()
    print(f"ledger: {counts}")
    print(f"module wall time so far: {time.time() - T0:.0f} s")
    print(f"shared only (placed, never alone): {shared_only}")
    print(f"panels behind host arrays: {sorted(H.panels)}")
    print(f"addresses no tensor answered for: {H.unresolved}")
    by_file = {}
    for (entry, param), t in H.tally.items():
        if t["held"]:
            by_file[entry] = by_file.get(entry, 0) + 1
    print(f"parameters held per entry point: {by_file}")
    print(f"UNHELD {len(unheld)}: {unheld}")
    print(f"UNCOMPARED {len(uncompared)}: {uncompared}")
    assert not set(G.EXEMPT) & set(H.tally), "exempt, yet placed"
    assert not unheld, f"{len(unheld)} required parameters were never placed flush: {unheld}"
    assert not uncompared, f"placed, yet never compared, waived or scratch: {uncompared}"
