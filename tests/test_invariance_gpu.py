"""GPU: every op under poisoned scratch memory and on a side stream (invariance.py holds the harness).

The suite's other modules run on the default stream and mostly on fresh, zero scratch.  Here every case runs four times --
plain, poisoned(0xFF), poisoned(0x7F) and side_stream() with poisoned(0xFF) -- and every run is judged twice: by the
oracle its family already has (imported from the family's test module or *_cases.py, no assertion changed) and, for every
output that is deterministic, by same_bits against the plain run.

  a. planted faults (pure torch, wrong values only): a leak, three wrong-stream producers, a wrong-stream consumer, each
     with a correct twin
  b. the query side through the public functions and the ops wrappers
  c. the training side: the bodies of the existing direct-drive tests, called with explicit arguments
  d. the ledger: which C entry point was launched under which perturbation (REQUIRED / HOST_ONLY / NOT_REACHED /
     ELSEWHERE: the case is in the family's own module)

Which shape enters which branch (from the kernels' dispatch code):

  rank / top-k / accept / retrieval / softmax tiles   64 query rows x 256 candidates a workgroup: 65 x 257 is one past both
  row paths of the query kernels                      table rows of 17 floats (off the 16-byte grid: scalar loads) and of 32
                                                      floats on 16-byte rows (vector loads); transr projects 32 -> 17
  candidate splits                                    splits = 1 (no partial buffers) and 3 (lkg_topk_merge_f32, the split
                                                      counters of accept, the partial (max, sum) pairs of the softmax)
  softmax backward                                    chunk_bytes = 1 gives chunks of 256 candidates: two for 257
  filter                                              none, KnownTriples (built on the device inside every run), a
                                                      candidate subset of 200 unsorted ids
  relation slot                                       n_rel = 5 (one chunk) and 300
  retrieval                                           queries of 1, 33 / 34 and 98 / 99 answers: RETRIEVAL_SLICE = 32 keys
                                                      fill one row of the counting kernel, 33 need a second; an EMPTY query,
                                                      whose only answer is a NaN table row: no key, no bucket row, the
                                                      m_keys == 0 path of retrieval_finish_kernel, where a_before / a_position
                                                      (full -1), the metrics (zeros) and buckets (empty) are as allocated
  binary_curve / threshold_fit / accept_order         n = 5000 (BC_TILE 1024, 256-key groups of the fit, three radix tiles),
                                                      five distinct values and both zeros; 1 and 7 relations / rows, one of
                                                      the 7 without an entry (an empty row of the order)
  device structure build, Laplacian                   n = 300, e = 5300 with 300 repeated pairs: RS_TILE = 2048 gives three
                                                      tiles, ceil(log2(300^2) / 8) = three radix passes"""
import contextlib
import inspect
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import invariance as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(gpu_device):
    import __graft_entry__ as ge
    ge.build()
    import literalkg_amd
    return literalkg_amd


@pytest.fixture(scope="module")
def ops(L):
    from literalkg_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def R(L):
    from literalkg_amd import ranking
    return ranking


@pytest.fixture(scope="module")
def N(L):
    from literalkg_amd import _native
    return _native


# ----------------------------------------------------------------------------- the perturbations and the ledger
MODES = ("plain", "poison 0xFF", "poison 0x7F", "side stream + poison 0xFF")
PERTURBED = MODES[1:]
LAUNCHED = {m: set() for m in MODES}            # mode -> the C entry points _native.call launched under it
RAN = []                                        # the cases that have run in this process (test_ledger needs them all)


@contextlib.contextmanager
def recorded(mode):
    from literalkg_amd import _native
    real = _native.call

    def call(name, *args):
        LAUNCHED[mode].add(name)
        return real(name, *args)
    _native.call = call
    try:
        yield
    finally:
        _native.call = real


@contextlib.contextmanager
def perturbation(mode, sleep=V.SLEEP_CYCLES):
    with contextlib.ExitStack() as stack:
        stack.enter_context(recorded(mode))
        if mode == "side stream + poison 0xFF":
            stack.enter_context(V.side_stream(sleep))
        if mode != "plain":
            stack.enter_context(V.poisoned(0x7F if mode == "poison 0x7F" else 0xFF))
        yield
    torch.cuda.synchronize()


def four_ways(run, judge):
    """run() under each mode; judge(result, mode) -- outside the perturbation -- holds the result to the family's oracle and
    returns {name: tensor} of the outputs that are deterministic: those must carry the plain run's bits in every mode."""
    RAN.append(inspect.stack()[1].function)
    base = None
    for mode in MODES:
        with perturbation(mode):
            res = run()
        out = judge(res, mode)
        if base is None:
            base = out
            continue
        assert out.keys() == base.keys(), mode
        for name in base:
            V.same_bits(out[name], base[name], f"{mode}: {name}")


# ----------------------------------------------------------------------------- a. the harness sees planted faults
def planted_want(src):
    return src * 2 + 1


def _elsewhere(wrong):
    """the null stream when the fault is planted, the current one for the correct twin"""
    return torch.cuda.stream(torch.cuda.default_stream()) if wrong else contextlib.nullcontext()


def plant_leak(src, wrong):
    out = torch.empty_like(src)
    out[::2] = src[::2] * 2 + 1
    if not wrong:
        out[1::2] = src[1::2] * 2 + 1
    return out


def _two_halves(out, src, wrong):
    half = src.numel() // 2
    out[:half] = src[:half] * 2 + 1
    with _elsewhere(wrong):                      # the second launch forgets its stream
        out[half:] = src[half:] * 2 + 1
    return out


def plant_producer_empty(src, wrong):
    return _two_halves(torch.empty_like(src), src, wrong)


def plant_producer_zeros(src, wrong):
    return _two_halves(torch.zeros_like(src), src, wrong)


def plant_producer_after_sync(src, wrong):
    n = int((src >= 0).sum().item())             # the op reads a count back: the side stream has caught up here
    assert n == src.numel()
    return _two_halves(torch.zeros_like(src), src, wrong)


def plant_consumer(src, wrong):
    t = torch.zeros_like(src)
    t += 5
    assert float(t[0].item()) == 5.0             # t holds 5 everywhere, the stream is idle
    step = torch.zeros_like(src)                 # ... and behind again
    step += src - 5
    t += step                                    # t = src, produced on the current stream
    with _elsewhere(wrong):                      # the consumer forgets its stream: it reads the 5s
        out = t * 2 + 1
    return out


def _side(sleep):
    return V.side_stream(sleep)


@contextlib.contextmanager
def _side_poisoned(sleep):
    with V.side_stream(sleep), V.poisoned(0xFF):
        yield


PLANTED = {
    "leak": (plant_leak, lambda sleep: V.poisoned(0xFF)),
    "leak 0x7F": (plant_leak, lambda sleep: V.poisoned(0x7F)),
    "producer into empty": (plant_producer_empty, _side_poisoned),
    "producer into zeros": (plant_producer_zeros, _side),
    "producer after a host sync": (plant_producer_after_sync, _side),
    "consumer": (plant_consumer, _side),
}


@pytest.mark.parametrize("name", list(PLANTED))
def test_planted_fault_is_caught_and_its_twin_passes(gpu_device, name):
    """Pure torch, wrong values only: the leak under poisoned(), the four wrong-stream launches under side_stream()."""
    fn, perturb = PLANTED[name]
    src = torch.arange(4096, dtype=torch.float32, device=gpu_device)
    want = planted_want(src)
    torch.cuda.synchronize()
    assert V.same_bits(fn(src, False), want)                          # unperturbed, the twin is right
    with perturb(V.SLEEP_CYCLES):
        twin = fn(src, False)
    torch.cuda.synchronize()
    assert V.same_bits(twin, want, f"{name}: the correct twin")
    with perturb(V.SLEEP_CYCLES):
        got = fn(src, True)
    torch.cuda.synchronize()
    with pytest.raises(AssertionError, match="elements differ"):
        V.same_bits(got, want)


# ----------------------------------------------------------------------------- the ledger
# no stream argument: nothing to launch on another stream, no device memory of the caller's choosing
HOST_ONLY = {
    "lkg_version", "lkg_last_error", "lkg_preload",
    "lkg_csr_build", "lkg_csr_transpose", "lkg_row_partition", "lkg_laplacian_f32",                       # host structure
    "lkg_triples_count", "lkg_triples_read", "lkg_triples_dedup",                                         # files
    "lkg_csr_build_device_workspace", "lkg_csr_transpose_device_workspace", "lkg_gemm_tall_workspace",
    "lkg_linear_act_layernorm_workspace", "lkg_gemm_workspace", "lkg_narrow_layer_bwd_workspace",
    "lkg_binary_curve_workspace", "lkg_threshold_fit_workspace", "lkg_accept_order_workspace",
    "lkg_topk_splits", "lkg_pair_mlp_splits", "lkg_softmax_all_splits",
    "lkg_gemm_longk_ok", "lkg_gemm_smallm_ok", "lkg_gemm_skinny_ok", "lkg_narrow_layer_bwd_ok", "lkg_gemm_f32_engine",
    "lkg_gemm_ordered_splits", "lkg_gemm_ordered_partition", "lkg_gemm_ordered_workspace",
}
# takes a stream, not launched by any case of this module: name -> why
NOT_REACHED = {
    "lkg_spmm_csr_f32": "no caller in literalkg_amd/*.py: every SpMM goes through lkg_spmm_csr_fused_f32 (ops.spmm_raw); only "
                        "the argument checks of test_native_abi.py and test_gpu_parity.py name it, and those launch nothing",
}
# the entry points of lkg_rank, lkg_topk, lkg_pairmlp, lkg_triples, lkg_relations, lkg_accept, lkg_retrieval, lkg_softmax and
# lkg_csr_device (.hip) that take a stream: none of them may be in NOT_REACHED
QUERY_SIDE = {
    "lkg_rank_sqnorm_f32", "lkg_rank_queries_f32", "lkg_rank_prepare_f32", "lkg_rank_count_f32",
    "lkg_topk_select_f32", "lkg_topk_merge_f32",
    "lkg_pair_mlp_scores_f32", "lkg_pair_mlp_select_f32", "lkg_pair_mlp_prepare_f32", "lkg_pair_mlp_count_f32",
    "lkg_pair_mlp_pairs_f32", "lkg_triple_scores_f32", "lkg_relation_scores_f32", "lkg_relation_order_f32",
    "lkg_accept_count_f32", "lkg_accept_emit_f32", "lkg_retrieval_prepare_f32", "lkg_retrieval_count_f32",
    "lkg_retrieval_finish", "lkg_softmax_all_partial_f32", "lkg_softmax_all_finish_f32", "lkg_softmax_all_weights_f32",
    "lkg_softmax_excluded", "lkg_softmax_all_partial_masked_f32", "lkg_softmax_all_weights_masked_f32",
    "lkg_csr_build_device", "lkg_csr_transpose_device", "lkg_csr_coo_indices_i64", "lkg_laplacian_device_f32",
    "lkg_binary_curve_f32", "lkg_threshold_fit_f32", "lkg_accept_order",
}
TRAINING_SIDE = {
    "lkg_spmm_csr_f32", "lkg_spmm_csr_fused_f32", "lkg_csr_extract_rows", "lkg_spmm_csr_scatter_bwd_f32",
    "lkg_edge_softmax_f32", "lkg_permute_f32", "lkg_csr_check_i32", "lkg_transe_score_fwd_f32", "lkg_loss_reduce_f32",
    "lkg_transe_score_bwd_f32", "lkg_group_by_key_i64", "lkg_gather_rows_f32", "lkg_scatter_add_rows_f32",
    "lkg_fill_rows_f32", "lkg_gather_i64", "lkg_gather_rows_range_f32", "lkg_scatter_add_rows_range_f32",
    "lkg_sample_kg_batch", "lkg_grouped_gemm_f32", "lkg_dense_score_fwd_f32", "lkg_dense_score_bwd_f32",
    "lkg_check_grouped_i64", "lkg_sanitize_ids_i64", "lkg_expand_groups_i32", "lkg_act_layernorm_fwd_f32",
    "lkg_act_layernorm_bwd_f32", "lkg_dot_score_fwd_f32", "lkg_dot_score_bwd_f32", "lkg_relu_batchnorm_fwd_f32",
    "lkg_relu_batchnorm_bwd_f32", "lkg_gate_blend_fwd_f32", "lkg_gate_blend_bwd_f32", "lkg_gate_blend_bwd_stats_f32",
    "lkg_row_absmax_f32", "lkg_gemm_tall_f32", "lkg_linear_act_layernorm_fwd_f32", "lkg_gemm_f32", "lkg_gemm_f64acc_f32",
    "lkg_colsum_f32", "lkg_col_absmax_f32", "lkg_gemm_longk_f32", "lkg_gemm_skinny_f32", "lkg_gemm_smallm_f32",
    "lkg_gemm_wgrad_f32", "lkg_narrow_layer_bwd_f32", "lkg_colsum_weighted_f32", "lkg_eltwise_f32", "lkg_bi_mix_fwd_f32",
    "lkg_bi_mix_bwd_f32", "lkg_adam_step_f32",
}
# launched under every perturbation by the cases of this module (test_ledger asserts it)
REQUIRED = (QUERY_SIDE | TRAINING_SIDE) - set(NOT_REACHED)
# takes a stream; its poison and side-stream case lives in its family's own module: name -> "file::test"
# (test_invariance_host.py holds every named test to it: it exists, enters both perturbations and reaches the caller)
_KVS_ALL = "test_kvs_all_surface_gpu.py::test_entry_points_keep_their_bits_under_poison_and_on_a_side_stream"
_NSSA = "test_self_adversarial_gpu.py::test_entry_points_keep_their_bits_under_poison_and_on_a_side_stream"
_NEGATIVES = "test_negatives_gpu.py::test_poisoned_scratch_and_a_side_stream_give_the_same_bits"
_RELATION_LOSS = "test_relation_loss_gpu.py::test_the_op_keeps_its_bits_under_poison_and_on_a_side_stream"
ELSEWHERE = {
    "lkg_sigmoid_all_partial_f32": _KVS_ALL, "lkg_sigmoid_all_finish_f32": _KVS_ALL, "lkg_sigmoid_all_weights_f32": _KVS_ALL,
    "lkg_nssa_fwd_f32": _NSSA, "lkg_nssa_bwd_f32": _NSSA,
    "lkg_sample_negatives": _NEGATIVES, "lkg_relation_cardinality": _NEGATIVES, "lkg_answer_counts": _NEGATIVES,
    "lkg_relation_loss_fwd_f32": _RELATION_LOSS, "lkg_relation_loss_bwd_f32": _RELATION_LOSS,
    "lkg_gemm_ordered_f32": "test_gemm_ordered_gpu.py::test_runs_poison_and_a_side_stream_change_no_bit",
    "lkg_csr_sample_rows": "test_neighbors_gpu.py::test_a_rows_sample_depends_on_the_row_alone",
    "lkg_pair_mlp_accept_count_f32": "test_pair_accepted_gpu.py::test_invariance",
    "lkg_pair_mlp_accept_append_f32": "test_pair_accepted_gpu.py::test_invariance",
    "lkg_pair_mlp_accept_emit_f32": "test_pair_accepted_gpu.py::test_invariance",
    "lkg_list_scores_f32": "test_lists_gpu.py::test_invariance", "lkg_list_count_f32": "test_lists_gpu.py::test_invariance",
}


def check_ledger_partition(prototypes):
    names = set(prototypes)
    sets = {"REQUIRED": set(REQUIRED), "HOST_ONLY": set(HOST_ONLY), "NOT_REACHED": set(NOT_REACHED),
            "ELSEWHERE": set(ELSEWHERE)}
    for a in sets:
        assert sets[a] <= names, (a, sorted(sets[a] - names))
        for b in sets:
            assert a >= b or not sets[a] & sets[b], (a, b, sorted(sets[a] & sets[b]))
    left = names - set().union(*sets.values())
    assert not left, f"entry points the ledger does not classify: {sorted(left)}"


# ----------------------------------------------------------------------------- b. the query side
B, N_CAND = 65, 257                            # one past the 64-query x 256-candidate tile
N_REL = 5
# (scoring, relation width k, table width c): 17 floats -- rows off the 16-byte grid, the scalar path -- and 32 floats on
# 16-byte rows, the vector path
WIDTHS = [("transr", 17, 32), ("transe", 32, 32), ("dot", 17, 17)]


def _query_case(TT, scoring, k, c, dev, seed):
    gen = torch.Generator().manual_seed(seed)
    model = TT.random_model(gen, scoring, N_CAND, k, c, N_REL, dev)
    model.T[N_CAND - 5:N_CAND - 2] = model.T[2:5]                       # bit-identical rows: ties between candidates
    ids = torch.randint(0, N_CAND, (B,), generator=gen).to(dev)
    r = torch.randint(0, N_REL, (B,), generator=gen).to(dev)
    other = torch.randint(0, N_CAND, (B,), generator=gen).to(dev)
    subset = torch.randperm(N_CAND, generator=gen)[:200].to(dev)        # unsorted entity ids
    return SimpleNamespace(gen=gen, model=model, ids=ids, r=r, other=other, subset=subset)


@pytest.mark.parametrize("scoring,k,c", WIDTHS)
def test_ranking(L, R, gpu_device, scoring, k, c):
    """rank_triples on both sides, raw and filtered, against the float64 oracle of test_ranking_gpu.py; the filter (two
    device structure builds) is made inside every run."""
    import test_ranking_gpu as TRK
    cs = _query_case(TRK, scoring, k, c, gpu_device, 100 + k)
    h, r, t = cs.ids, cs.r, cs.other
    known = TRK.draw_known(cs.gen, N_CAND, N_REL, h, r, t, extra=4 * B)
    table, relemb, trans_m = cs.model.T, cs.model.relation_embed.weight, cs.model.gat_trans_M
    for kn in (None, known):
        want = [TRK.oracle(table, relemb, trans_m, scoring, side, h, r, t, kn) for side in ("tail", "head")]

        def run():
            kt_ = R.KnownTriples(*kn, N_CAND, N_REL) if kn is not None else None
            return R.rank_triples(cs.model, h, r, t, side="both", known=kt_, scoring=scoring)

        def judge(res, mode):
            for j, side in enumerate(("tail", "head")):
                TRK.check(res.better[j], res.equal[j], want[j], what=f"{mode} {scoring} {side}")
            return dict(better=res.better, equal=res.equal, rank=res.rank)
        four_ways(run, judge)


@pytest.mark.parametrize("scoring,k,c", WIDTHS)
def test_topk(L, R, gpu_device, scoring, k, c):
    """predict_topk against the float64 margin check of test_topk_gpu.py: tail side raw over all candidates in one split,
    head side filtered over a candidate subset in three splits (lkg_topk_merge_f32)."""
    import test_topk_gpu as TT
    cs = _query_case(TT, scoring, k, c, gpu_device, 200 + k)
    known = TT.draw_known(cs.gen, N_CAND, N_REL, cs.ids, cs.r, 3 * B)
    table, relemb, trans_m = cs.model.T, cs.model.relation_embed.weight, cs.model.gat_trans_M
    for side, kn, cand, splits in (("tail", None, None, 1), ("head", known, cs.subset, 3), ("tail", known, None, 3)):
        chunks = TT.oracle(table, relemb, trans_m, scoring, side, cs.ids, cs.r, kn, cand)

        def run():
            kt_ = R.KnownTriples(*kn, N_CAND, N_REL) if kn is not None else None
            return L.predict_topk(cs.model, cs.ids, cs.r, side=side, k=10, known=kt_, scoring=scoring, candidates=cand,
                                  splits=splits)

        def judge(res, mode):
            TT.check_topk(res, chunks, 10, scoring, f"{mode} {scoring} {side}")
            return dict(ids=res.ids, scores=res.scores, kernel_scores=res.kernel_scores)
        four_ways(run, judge)


@pytest.mark.parametrize("scoring,k,c", WIDTHS)
def test_accepted(L, R, gpu_device, scoring, k, c):
    """predict_accepted / count_accepted against accepted_cases.accepted_lists over the dense scores of score_triples
    (computed once, unperturbed): filtered in three splits on the tail side, a candidate subset in one on the head side."""
    import accepted_cases as AC
    import test_accepted_gpu as TA
    cs = _query_case(TA, scoring, k, c, gpu_device, 300 + k)
    lower = scoring != "dot"
    known = TA.draw_known(cs.gen, N_CAND, N_REL, cs.ids, cs.r, 3 * B)
    for side, kn, cand, splits in (("tail", known, None, 3), ("head", None, cs.subset, 1)):
        values, keys = TA.dense_scores(L, cs.model, cs.ids, cs.r, side, scoring)
        thr = TA.observed_thresholds(values, cs.r, N_REL, lower)
        sets = TA.known_sets(kn, cs.ids, cs.r, side) if kn is not None else None
        want = AC.accepted_lists(values, keys, np.arange(N_CAND), thr.numpy()[cs.r.cpu().numpy()], lower, sets)
        if cand is not None:                                            # the full lists, restricted: the order is kept
            inside = set(cand.cpu().tolist())
            keep = [np.array([x in inside for x in w[0].tolist()], dtype=bool) for w in want]
            want = [(w[0][m], w[1][m], w[2][m]) for w, m in zip(want, keep)]
        assert sum(w[0].size for w in want) > 0
        thr_d = thr.to(gpu_device)

        def run():
            kt_ = R.KnownTriples(*kn, N_CAND, N_REL) if kn is not None else None
            kw = dict(side=side, known=kt_, scoring=scoring, candidates=cand)
            return (L.predict_accepted(cs.model, cs.ids, cs.r, thr_d, splits=splits, **kw),
                    L.count_accepted(cs.model, cs.ids, cs.r, thr_d, **kw))

        def judge(out, mode):
            res, counts = out
            TA.assert_lists(res, want, f"{mode} {scoring} {side}")
            assert torch.equal(counts, res.counts), mode
            return dict(rowptr=res.rowptr, ids=res.ids, scores=res.scores, kernel_scores=res.kernel_scores, counts=counts)
        four_ways(run, judge)


@pytest.mark.parametrize("scoring,k,c", WIDTHS)
def test_retrieval(L, R, gpu_device, scoring, k, c):
    """rank_answers / evaluate_retrieval against retrieval_cases over the dense kernel scores: queries with 1, 33 or 34
    (past the 32 keys of a row of the counting kernel) and 98 or 99 answers next to 65 single triples, six queries with a
    NaN row among their answers and one EMPTY query -- its only answer is the NaN row, which leaves it without a key: no
    bucket row is written for it and lkg_retrieval_finish takes its m_keys == 0 path, where every output is what the
    Python side initialised (the case of test_retrieval_gpu.test_nan_rows)."""
    import test_retrieval_gpu as TV
    gen = torch.Generator().manual_seed(400 + k)
    model = TV.random_model(gen, scoring, N_CAND, k, c, N_REL, gpu_device)
    tee = L.ops.RETRIEVAL_SLICE
    for side in ("tail", "head"):
        h, r, t = TV.draw_triples(gen, N_CAND, N_REL, B, (1, tee + 2, 3 * tee + 3), side)
        ent, ans = (h, t) if side == "tail" else (t, h)
        free = sorted(set(range(N_CAND)) - set(ent.tolist()))           # entities that are no query's
        nan_row, lone = free[0], free[1]
        keep = ans != nan_row                                           # (a long query may lose one answer: 33 and 98 stay)
        ent, r, ans = ent[keep], r[keep], ans[keep]
        ent = torch.cat([ent, ent[:6], torch.tensor([lone])])           # six queries with the NaN answer among theirs ...
        r = torch.cat([r, r[:6], torch.tensor([1])])
        ans = torch.cat([ans, torch.full((6,), nan_row), torch.tensor([nan_row])])   # ... and one whose only answer it is
        h, t = (ent, ans) if side == "tail" else (ans, ent)
        table = model.T.clone()
        table[nan_row] = float("nan")
        model_s = TV.StandIn(table, model.relation_embed.weight, model.gat_trans_M, scoring)
        known = TV.draw_known(gen, N_CAND, N_REL, h, r, t, 2 * B)
        q_ent, q_rel, query, _ = TV.queries_of(h, r, t, side, N_CAND)
        dense = TV.dense_scores(L, model_s, q_ent, q_rel, side, scoring)
        assert np.isnan(dense[:, nan_row]).all() and int(np.isnan(dense).sum()) == q_ent.size
        exp = TV.expected(h, r, t, side, N_CAND, dense, np.arange(N_CAND), known)
        u = int(np.flatnonzero(q_ent == lone)[0])
        assert exp.n_answers[u] == 1 and (exp.position[query == u] < 0).all()                 # the empty query
        assert (exp.n_answers > tee).sum() >= 2 and exp.n_answers.max() > 3 * tee
        hd, rd, td = (x.to(gpu_device) for x in (h, r, t))
        kd = tuple(x.to(gpu_device) for x in known)

        def run():
            kt_ = R.KnownTriples(*kd, N_CAND, N_REL)
            return (L.rank_answers(model_s, hd, rd, td, side=side, known=kt_, scoring=scoring, ks=TV.KS),
                    L.evaluate_retrieval(model_s, hd, rd, td, known=kt_, ks=TV.KS, side=side, scoring=scoring))

        def judge(out, mode):
            res, agg = out
            TV.check(res, exp, f"{mode} {scoring} {side}")
            TV.check_aggregates(agg, exp, f"{mode} {scoring} {side}")
            assert int(res.nan.sum()) == 7 and bool((res.before[res.nan] == -1).all()), mode
            # (ndcg, ap and rr are summed in a fixed order: their bits repeat too)
            names = ("query", "before", "position", "nan", "q_ids", "q_rel", "n_answers", "a_query", "a_ids", "a_before",
                     "a_position", "hits", "ndcg", "ap", "rr")
            return {name: getattr(res, name) for name in names}
        four_ways(run, judge)


@pytest.mark.parametrize("n_rel", [5, 300])
@pytest.mark.parametrize("scoring", ["transr", "transe"])
def test_relations(L, gpu_device, scoring, n_rel):
    """score_relations, rank_relations and predict_relations on exact integer tables against relation_cases (the check of
    test_relations_gpu.py, run whole under each perturbation): 5 relations and 300, raw and filtered, both sides."""
    import test_relations_gpu as TL
    gen = torch.Generator().manual_seed(500 + n_rel)
    model, table, e, w = TL.integer_model(gen, scoring, 50, 8, 8, n_rel, gpu_device)
    h, t = TL.pairs(gen, 50, B, gpu_device)
    r = torch.randint(0, n_rel, (B,), generator=gen).to(gpu_device)
    want = TL.integer_scores(table, e, w, h, t)
    known = TL.some_known(gen, h, r, t, n_rel, 100)

    def run():
        out = {}
        for side in ("tail", "head"):
            got = L.score_relations(model, h, t, side=side)
            assert np.array_equal(got.cpu().numpy().astype(np.float64), want.astype(np.float64)), side
            TL.check_against_references(L, model, h, r, t, want.astype(np.float32), known, side)
            kt_ = L.KnownTriples(*known, model.n_entities, n_rel)
            res = L.rank_relations(model, h, r, t, known=kt_, side=side)
            top = L.predict_relations(model, h, t, k=3, known=kt_, side=side)
            out.update({f"{side} scores": got, f"{side} better": res.better, f"{side} equal": res.equal,
                        f"{side} top ids": top.ids, f"{side} top scores": top.scores})
        return out
    four_ways(run, lambda out, mode: out)


@pytest.mark.parametrize("scoring,n,k,c", [("transr", 120, 37, 32), ("transe", 128, 33, 33), ("dot", 100, 64, 64)])
def test_triples(L, gpu_device, scoring, n, k, c):
    """score_triples, evaluate_triple_classification and fit_triple_thresholds on 257 triples of the cases of
    test_triples_gpu.py: the scores within the float64 margin of the top-k oracle, the counts and the fit those of
    triple_cases on the scores."""
    import pair_cases as PC
    import test_topk_gpu as TT
    import test_triples_gpu as TR
    import triple_cases as TC
    cs = TR.case(scoring, n, k, c, N_REL, gpu_device)
    model, p, lower = cs["model"], 257, scoring != "dot"
    h, r, t, y = (cs[x][:p] for x in ("h", "r", "t", "y"))
    cand = torch.unique(t)
    uq, inv = torch.unique(h * N_REL + r, return_inverse=True)
    chunks = TT.oracle(model.T, model.relation_embed.weight, model.gat_trans_M, scoring, "tail", uq // N_REL, uq % N_REL,
                       cand=cand)
    d64 = torch.stack([next(iter(chunks(i)))[1] for i in range(uq.numel())])
    e64 = torch.stack([next(iter(chunks(i)))[2] for i in range(uq.numel())])
    slot = torch.full((n,), -1, dtype=torch.int64, device=gpu_device)
    slot[cand] = torch.arange(cand.numel(), device=gpu_device)
    d, e = d64[inv, slot[t]], e64[inv, slot[t]]

    def run():
        s = L.score_triples(model, h, r, t)
        fit = L.fit_triple_thresholds(model, h, r, t, y)
        return s, L.score_triples(model, h, r, t, kernel_scores=True), fit, \
            L.evaluate_triple_classification(model, h, r, t, y, fit)

    def judge(out, mode):
        s, ks, fit, got = out
        if scoring == "dot":
            err, bound = (s.double() - (-0.5 * d)).abs(), 0.5 * e + 1e-30
        else:
            err, bound = (s.double() - d).abs(), e + 4 * TT.U * d.abs() + 1e-30
        assert bool((err <= bound).all()), (mode, float((err / bound).max()))
        sn, rn, yn = s.cpu().numpy(), r.cpu().numpy(), y.cpu().numpy()
        want = TC.fit_by_definition(sn, rn, yn, N_REL, lower)
        TR.same_fit(fit, want)
        curve = PC.curve_reference(-sn if lower else sn, yn)
        TC.same_metrics(got, TC.metrics(TC.decisions(sn, rn, yn, want["thresholds"], lower, N_REL), yn, curve), curve[3])
        return dict(scores=s, kernel_scores=ks, thresholds=fit.thresholds, n=fit.n, correct=fit.correct,
                    counts=torch.tensor([got[x] for x in ("tp", "fp", "tn", "fn", "nan")]))
    four_ways(run, judge)


def test_pair_head(L, R, gpu_device):
    """mlp_scores, predict_topk(scoring='mlp'), rank_pairs_mlp, score_pairs_mlp and evaluate_mlp_classification on 65
    queries x 257 entities of width 37: every logit within its float64 bound (ref64 of test_pairmlp_gpu.py), the lists by
    that module's check_topk, the ranks counted from the stored logits, the confusion counts and the curve by pair_cases."""
    import pair_cases as PC
    import test_pairmlp_gpu as TP
    import test_pairmlp_pairs_gpu as TPP
    import test_pairmlp_rank_gpu as TPR
    dev, n = gpu_device, N_CAND
    model, gen = TPP.make_model(600, n, 37, dev)
    n_rel = model.n_relations
    q = torch.randint(0, n, (B,), generator=gen).to(dev)
    truth = torch.randint(0, n, (B,), generator=gen).to(dev)
    r = torch.randint(0, n_rel, (B,), generator=gen).to(dev)
    y = torch.randint(0, 2, (B,), generator=gen).to(torch.uint8).to(dev)
    every = torch.arange(n, device=dev)
    subset = torch.cat([truth, torch.randperm(n, generator=gen)[:150].to(dev)]).unique().flip(0)      # holds every truth
    zt, et = TP.ref64(model, q, every)
    zh, eh = TP.ref64(model, every, q, chunk=512)
    cs = SimpleNamespace(model=model, gen=gen, q=q, n=n, Z=dict(tail=zt, head=zh.T.contiguous()),
                         E=dict(tail=et, head=eh.T.contiguous()), D={})
    for side in ("tail", "head"):
        known = None

        def run():
            dense = L.mlp_scores(model, q, every, logits=True) if side == "tail" else \
                L.mlp_scores(model, every, q, logits=True).T.contiguous()
            kt_ = R.KnownTriples(*known, n, n_rel)
            top = L.predict_topk(model, q, r, side=side, k=10, scoring="mlp", known=kt_, candidates=subset, splits=3)
            h_, t_ = (q, truth) if side == "tail" else (truth, q)
            rank = L.rank_pairs_mlp(model, h_, t_, r, side=side, known=kt_, candidates=subset)
            agg = L.evaluate_mlp_ranking(model, h_, t_, r, known=kt_, side=side, candidates=subset)
            z = L.score_pairs_mlp(model, h_, t_, logits=True)
            ev = L.evaluate_mlp_classification(model, h_, t_, y, logit_threshold=0.0)
            return dense, top, rank, agg, z, ev

        def judge(out, mode):
            dense, top, rank, agg, z, ev = out
            what = f"{mode} {side}"
            assert bool(((dense.double() - cs.Z[side]).abs() <= cs.E[side]).all()), what
            cs.D[side] = dense
            elig = TP.eligibility(n, side, q, subset, known, r)
            TP.check_topk(top, cs, side, 10, subset, elig, what)
            pos_of = torch.full((n,), -1, dtype=torch.int64, device=dev)
            pos_of[subset] = torch.arange(subset.numel(), device=dev)
            kept = TPR.eligibility(n, n_rel, side, q, r, subset, known)
            wb, we = TPR.counts_from(dense[:, subset], pos_of[truth], kept)
            assert torch.equal(rank.better, wb) and torch.equal(rank.equal, we), what
            assert agg["n"] == B and agg["mr"] == pytest.approx(float(rank.rank.mean()), rel=1e-12), what
            rows = torch.arange(B, device=dev)
            assert torch.equal(z, dense[rows, truth]), what             # the pair's logit is the matrix's entry
            zn, yn = z.cpu().numpy(), y.cpu().numpy()
            curve = PC.curve_reference(zn, yn)
            TPP.same_metrics(ev, PC.metrics_reference(zn, yn, 0.0, curve), curve[3])
            return dict(logits=dense, ids=top.ids, scores=top.scores, kernel_scores=top.kernel_scores, better=rank.better,
                        equal=rank.equal, pair_logits=z, counts=torch.tensor([ev[x] for x in ("tp", "fp", "tn", "fn", "nan")]))
        # the filter: some of float64's best candidates per query, under the query's relation or another one
        known = TP.draw_known(cs, side, r, n_rel, every)
        h_, t_ = (q, truth) if side == "tail" else (truth, q)
        known = tuple(torch.cat([a, b_]) for a, b_ in zip(known, (h_, r, t_)))      # ... and the truths themselves
        four_ways(run, judge)


@pytest.mark.parametrize("k", [17, 32])
@pytest.mark.parametrize("filtered", [False, True], ids=["all", "filtered"])
def test_softmax_op(ops, gpu_device, k, filtered):
    """ops.softmax_all_forward / softmax_all_loss with its backward in two chunks (chunk_bytes = 1: 256 candidates a chunk,
    257 candidates) in 1 and 3 splits, distance and dot logits: the loss against float64 within the bound of softmax_cases
    (lse by its bits alone: its own float64 bound holds on exact-logit tables only, test_one_vs_all_gpu.py), dQ and dP
    against float64 autograd within the bound of the engine that ran each product; with exclusion lists, the masked
    kernels against softmax_filtered_cases."""
    import softmax_cases as C
    import softmax_filtered_cases as F
    import test_one_vs_all_filtered_gpu as TF
    b, n = B, N_CAND
    q, p, truth, g = (x.to(gpu_device) for x in C.random_tables(b, n, k, seed=700 + k))
    assert ops.softmax_chunk_width(b, n, 1) == 256 < n
    lists = mask = None
    if filtered:
        ex = F.patterns(b, n, truth.cpu(), seed=k)
        mask, lists = F.mask_of(ex, n, gpu_device), F.to_lists(ex, gpu_device)
    for distance, scale in ((True, 0.37), (False, 1.7)):
        if filtered:
            ref = F.loss_eval(q, p, truth, mask, distance, scale)
            loss32 = F.loss_eval(q, p, truth, mask, distance, scale, torch.float32)[2]
            gref = F.grads_eval(q, p, truth, g, mask, distance, scale)
            dq32, dp32 = F.autograd_eval(q, p, truth, g, mask, distance, scale, torch.float32)
        else:
            ref = C.loss_eval(q, p, truth, distance, scale)
            loss32 = C.loss_eval(q, p, truth, distance, scale, torch.float32)[2]
            gref = C.grads_eval(q, p, truth, g, distance, scale)
            dq32, dp32 = C.autograd_eval(q, p, truth, g, distance, scale, torch.float32)
        bound = C.loss_bound(float(C.loss_measure(loss32, ref).max()))
        e_q, e_p = TF._engines(ops, q, p, b, n, k, 256, distance)
        bq = C.gemm_bound(e_q, C.worst(dq32, gref["dq"], gref["dq_scale"]), n)
        bp = C.gemm_bound(e_p, C.worst(dp32, gref["dp"], gref["dp_scale"]), b)
        for splits in (1, 3):
            def run():
                pn = ops.rank_sqnorm(p) if distance else None
                lse, loss = ops.softmax_all_forward(q, p, pn, truth, scale, splits, exclude=lists)
                q_, p_ = q.clone().requires_grad_(True), p.clone().requires_grad_(True)
                out = ops.softmax_all_loss(q_, p_, truth, distance=distance, scale=scale, splits=splits, chunk_bytes=1,
                                           exclude=lists)
                out.backward(g)
                return lse, loss, out.detach(), q_.grad, p_.grad

            def judge(res, mode):
                lse, loss, out, dq, dp = res
                what = (mode, distance, splits)
                assert float(C.loss_measure(loss, ref).max()) <= bound, what
                assert torch.equal(out, loss), what
                assert C.worst(dq, gref["dq"], gref["dq_scale"]) <= bq, ("dq", what, e_q)
                assert C.worst(dp, gref["dp"], gref["dp_scale"]) <= bp, ("dp", what, e_p)
                return dict(lse=lse, loss=loss, dq=dq, dp=dp)
            four_ways(run, judge)


def test_softmax_excluded_lists(L, ops, R, gpu_device):
    """ops.softmax_excluded over a filter built inside the run, against softmax_filtered_cases.excluded_reference, with and
    without a candidate subset."""
    import softmax_filtered_cases as F
    import test_topk_gpu as TT
    gen = torch.Generator().manual_seed(800)
    n = N_CAND
    ids = torch.randint(0, n, (B,), generator=gen).to(gpu_device)
    r = torch.randint(0, N_REL, (B,), generator=gen).to(gpu_device)
    truth = torch.randint(0, n, (B,), generator=gen).to(gpu_device)
    known = TT.draw_known(gen, n, N_REL, ids, r, 6 * B)
    subset = torch.cat([truth, torch.randperm(n, generator=gen)[:150].to(gpu_device)]).unique()
    pos_of = torch.full((n,), -1, dtype=torch.int32, device=gpu_device)
    pos_of[subset] = torch.arange(subset.numel(), dtype=torch.int32, device=gpu_device)
    for cand in (None, subset):
        n_cand = n if cand is None else cand.numel()
        pos = None if cand is None else pos_of
        tpos = truth if cand is None else pos_of[truth].long()

        def run():
            filt = R.KnownTriples(*known, n, N_REL).for_side("tail")
            return filt, ops.softmax_excluded(filt, ids, r, tpos, n_cand, pos)

        def judge(res, mode):
            filt, (xptr, xcol) = res
            wp, wc = F.to_lists(F.excluded_reference(filt, ids.cpu(), r.cpu(), tpos.cpu(), n_cand,
                                                     None if pos is None else pos.cpu()))
            assert xptr.dtype == torch.int32 and xcol.dtype == torch.int32 and xcol.numel() > 0
            assert torch.equal(xptr.cpu(), wp) and torch.equal(xcol.cpu(), wc), mode
            return dict(xptr=xptr, xcol=xcol)
        four_ways(run, judge)


N_KERNEL = 5000


@pytest.mark.parametrize("n_rel", [1, 7])
def test_curve_fit_and_order_kernels(ops, gpu_device, n_rel):
    """ops.binary_curve, ops.threshold_fit and ops.accept_order on 5000 scores with heavy ties and both zeros, 1 and 7
    relations (rows, for the order), one of the 7 without a triple (an empty row): the counts and AP of pair_cases, the
    fit of triple_cases, numpy's stable sort."""
    import pair_cases as PC
    import test_pairmlp_pairs_gpu as TPP
    import triple_cases as TC
    from fractions import Fraction
    n = N_KERNEL
    rng = np.random.default_rng(900 + n_rel)
    draws = {name: (s, y) for name, s, y in TPP.curve_draws(rng, n) if name in ("five values", "signed zeros among others")}
    for name, (s, y) in draws.items():
        rel = rng.integers(0, n_rel, n)
        if n_rel > 1:
            rel[rel == 3] = 4                   # relation 3 has no triple: an unfitted threshold, an empty row of the order
            assert np.bincount(rel, minlength=n_rel)[3] == 0
        want_curve = PC.curve_reference(s, y)
        fit = {lower: TC.fit_by_definition(s, rel, y, n_rel, lower) for lower in (True, False)}
        # accept_order: rows = relations, ids unique within a row, keys = the scores, values = other floats
        order = np.argsort(rel, kind="stable")
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(rel, minlength=n_rel))]).astype(np.int64)
        ids = rng.permutation(n).astype(np.int64)[order]
        keys, vals = s[order], rng.standard_normal(n).astype(np.float32)
        want_order = np.concatenate([a + np.lexsort((ids[a:b_], keys[a:b_] + np.float32(0.0)))
                                     for a, b_ in zip(rowptr[:-1], rowptr[1:])])
        st, yt, rt = (torch.from_numpy(x).to(gpu_device) for x in (s, y, rel))
        rp, it, kt_, vt = (torch.from_numpy(x).to(gpu_device) for x in (rowptr, ids, keys, vals))

        def run():
            return (ops.binary_curve(st, yt), [ops.threshold_fit(st, yt, rt, n_rel, lower) for lower in (True, False)],
                    ops.accept_order(rp, it, kt_, vt, n))

        def judge(res, mode):
            curve, fits, (oi, ok, ov) = res
            what = (mode, name)
            assert curve[:5] == want_curve[:5], what
            assert abs(Fraction(curve[5]) - want_curve[5]) <= (want_curve[3] + 4) * Fraction(1, 2 ** 53) * want_curve[5], what
            out = dict(curve=np.array(curve[:5]), ap=np.array(curve[5]), ids=oi, keys=ok, values=ov)
            for lower, (thr, stats) in zip((True, False), fits):
                assert np.array_equal(thr.cpu().numpy().view(np.uint32), fit[lower]["fitted"].view(np.uint32)), what
                stats_n = stats.cpu().numpy()
                assert stats_n[:, 0].tolist() == fit[lower]["n"].tolist(), what
                assert stats_n[:, 2].tolist() == fit[lower]["correct"].tolist(), what
                out[f"thr {lower}"], out[f"stats {lower}"] = thr, stats
            assert oi.cpu().numpy().tolist() == ids[want_order].tolist(), what
            assert np.array_equal(ok.cpu().numpy().view(np.uint32), keys[want_order].view(np.uint32)), what
            assert np.array_equal(ov.cpu().numpy().view(np.uint32), vals[want_order].view(np.uint32)), what
            return out
        four_ways(run, judge)


STRUCTURE_ARRAYS = ("rowptr", "col", "eptr", "rel", "rel_first", "dup_entries", "dup_rows", "t_rowptr", "t_col", "t_perm")


@pytest.mark.parametrize("kind", ["random-walk", "symmetric"])
def test_device_structure_and_laplacian(L, gpu_device, kind):
    """KGStructure.from_triples(device=gpu) and the device Laplacian at n = 300, e = 5000 plus 300 duplicate pairs (three
    radix tiles of 2048 keys, three passes): every array is the host build's, the values are the host form's bits."""
    from literalkg_amd import io
    n, e, n_rel, dup = 300, 5000, 6, 200
    rng = np.random.default_rng(n + e)
    h, t, r = rng.integers(0, n, e), rng.integers(0, n, e), rng.integers(0, n_rel, e)
    h[: e // 5] = rng.integers(0, 3, e // 5)
    src = rng.integers(0, e, dup)
    h = np.concatenate([h, h[src], h[src[: dup // 2]]])
    t = np.concatenate([t, t[src], t[src[: dup // 2]]])
    r = np.concatenate([r, (r[src] + 1) % n_rel, r[src[: dup // 2]]])
    gh = L.KGStructure.from_triples(n, h, t, r, device="cpu")
    want_val = io.laplacian_values(gh, kind)
    hd, td, rd = (torch.from_numpy(x).to(gpu_device) for x in (h, t, r))

    def run():
        g = L.KGStructure.from_triples(n, hd, td, rd, device=gpu_device)
        return g, io.laplacian_values(g, kind), g.coo_indices()

    def judge(res, mode):
        g, val, coo = res
        assert (g.n, g.nnz, g.n_raw) == (gh.n, gh.nnz, gh.n_raw) and g.has_dups, mode
        out = dict(values=val, coo=coo, order=g.order)
        for name in STRUCTURE_ARRAYS:
            a, b_ = g.host(name), gh.host(name)
            assert a is not None and b_ is not None and a.dtype == b_.dtype and np.array_equal(a, b_), (mode, name)
            out[name] = a
        assert np.array_equal(g.order, gh.order), mode
        assert torch.equal(val.cpu(), want_val), mode
        assert torch.equal(coo.cpu(), gh.coo_indices()), mode
        return out
    four_ways(run, judge)


# ----------------------------------------------------------------------------- b. whole models from the golden fixtures
def _golden(L, name, dev, scoring):
    import test_topk_gpu as TT
    model, gd = TT._golden_model(L, name, dev, "transr" if scoring == "dot" else scoring)    # ('dot' is a query-side scoring)
    return model.eval(), gd


def _same_numbers(got, want, what):
    """a metrics dict against the plain run's: integers and lists exactly, floats to 1e-12 relative (the tolerance
    test_retrieval_gpu.py and test_pairmlp_rank_gpu.py hold such aggregates to)"""
    assert got.keys() == want.keys(), what
    for key, w in want.items():
        g = got[key]
        if isinstance(w, dict):
            _same_numbers(g, w, f"{what} {key}")
        elif isinstance(w, torch.Tensor):
            if w.dtype.is_floating_point:
                torch.testing.assert_close(g, w, rtol=1e-12, atol=0, equal_nan=True, msg=f"{what} {key}")
            else:
                assert torch.equal(g, w), (what, key)
        elif isinstance(w, np.ndarray):
            if w.dtype.kind == "f":
                np.testing.assert_allclose(g, w, rtol=1e-12, atol=0, equal_nan=True, err_msg=f"{what} {key}")
            else:
                assert np.array_equal(g, w), (what, key)
        elif isinstance(w, float):
            assert (math.isnan(g) and math.isnan(w)) or g == pytest.approx(w, rel=1e-12), (what, key, g, w)
        else:
            assert g == w, (what, key, g, w)


@pytest.mark.parametrize("name,scoring", [("encoder_gcn_l2_gatenum", "transr"), ("transe_gcn_l1", "transe"),
                                          ("encoder_gcn_l1", "dot")])
def test_golden_model_queries(L, R, gpu_device, name, scoring):
    """One small model per scoring from the golden fixtures, through the LiteralKG-level evaluations: every perturbed run
    gives the plain run's numbers (the inference table is rebuilt inside each run: model.train(); model.eval())."""
    model, gd = _golden(L, name, gpu_device, scoring)
    h, r, t = (torch.from_numpy(gd[x]).to(gpu_device) for x in ("h", "r", "t"))
    n, n_rel = model.n_entities, model.n_relations
    nv = 40
    vh, vr, vt = h[:nv], r[:nv], t[:nv]
    gen = torch.Generator().manual_seed(1)
    corrupt = torch.randint(0, n, (nv,), generator=gen).to(gpu_device)
    th, tr_, tt = torch.cat([vh, vh]), torch.cat([vr, vr]), torch.cat([vt, corrupt])
    labels = torch.cat([torch.ones(nv), torch.zeros(nv)]).to(torch.uint8).to(gpu_device)

    def run():
        model.train()
        model.eval()                                                    # (drops the cached inference table)
        known = R.KnownTriples(h[nv:], r[nv:], t[nv:], n, n_rel)
        fitted = L.fit_triple_thresholds(model, th, tr_, tt, labels, scoring=scoring)
        top = L.predict_topk(model, vh, vr, k=10, known=known, scoring=scoring)
        acc = L.predict_accepted(model, vh, vr, fitted, known=known, scoring=scoring)
        out = dict(ranking=L.evaluate_ranking(model, vh, vr, vt, known=known, scoring=scoring),
                   retrieval=L.evaluate_retrieval(model, vh, vr, vt, known=known, scoring=scoring),
                   triples=L.evaluate_triple_classification(model, th, tr_, tt, labels, fitted, scoring=scoring))
        if scoring != "dot":
            out["relations"] = L.evaluate_relation_prediction(model, vh, vr, vt, known=known, scoring=scoring)
        loss = L.one_vs_all_loss(model, vh, vr, vt, scoring=scoring, known=known)         # forward and backward
        grads = torch.autograd.grad(loss, [p for p in model.parameters() if p.requires_grad and not p.is_sparse],
                                    allow_unused=True)
        return out, dict(thresholds=fitted.thresholds, top_ids=top.ids, top_scores=top.scores, acc_rowptr=acc.rowptr,
                         acc_ids=acc.ids, acc_scores=acc.scores), loss.detach(), [x for x in grads if x is not None]

    base = {}

    def judge(res, mode):
        out, bits, loss, grads = res
        assert grads and bool(torch.isfinite(loss))
        if mode == "plain":
            base.update(out=out, loss=loss, grads=grads)
        _same_numbers(out, base["out"], f"{mode} {name}")
        # the loss and its gradients at the tolerance the fixture gradients are held to (test_gpu_parity.GRAD_TOL: 1e-4 of
        # the largest entry)
        import test_gpu_parity as TG
        np.testing.assert_allclose(float(loss), float(base["loss"]), rtol=1e-5)
        for i, (g_, w_) in enumerate(zip(grads, base["grads"])):
            TG.fixture_grad_close(g_.cpu().numpy(), w_.cpu().numpy(), name, f"one_vs_all grad {i}")
        return bits
    four_ways(run, judge)


@pytest.mark.parametrize("name", ["mlp_model_gcn_l1_scale", "mlp_bce_gcn_l2_scale"])
def test_golden_mlp_head(L, R, gpu_device, name):
    """The MLP head of the golden fixtures: evaluate_mlp_ranking and evaluate_mlp_classification, perturbed against plain."""
    import test_pairmlp_gpu as TP
    model, gd = TP._golden_mlp_model(L, name, gpu_device)
    model.eval()
    n = model.n_entities
    gen = torch.Generator().manual_seed(2)
    h = torch.randint(0, n, (40,), generator=gen).to(gpu_device)
    t = torch.randint(0, n, (40,), generator=gen).to(gpu_device)
    y = torch.randint(0, 2, (40,), generator=gen).to(torch.uint8).to(gpu_device)

    def run():
        model.train()
        model.eval()
        return (dict(ranking=L.evaluate_mlp_ranking(model, h, t), pairs=L.evaluate_mlp_classification(model, h, t, y)),
                dict(logits=L.score_pairs_mlp(model, h, t, logits=True)))

    base = {}

    def judge(res, mode):
        out, bits = res
        base.setdefault("out", out)
        _same_numbers(out, base["out"], f"{mode} {name}")
        return bits
    four_ways(run, judge)


# ----------------------------------------------------------------------------- c. the training side
def _fixture_body(f):
    """the function behind a pytest fixture of another test module"""
    return getattr(f, "__wrapped__", f)


def _update_att(L, O, gpu_device, name):
    """one update_att step of a golden configuration against the oracle's refresh (the first part of
    test_gpu_parity.test_update_att_through_module, at its tolerances)"""
    import test_gpu_parity as TG
    from conftest import golden_params, load_golden
    gd = load_golden(name)
    m = TG._build_model(L, gd, gpu_device, "transr")
    h, t, r = (torch.from_numpy(gd[k]).to(gpu_device) for k in "htr")
    m(h, t, r, list(range(int(gd["n_rel"]))), device=gpu_device, mode="update_att")
    p = golden_params(gd)
    want = O.attention_refresh(int(gd["n"]), p["entity_embed.weight"], p["relation_embed.weight"],
                               *(torch.from_numpy(gd[k]) for k in "htr")).coalesce()
    a = m.A_in.data
    assert torch.equal(a.indices().cpu(), want.indices())
    torch.testing.assert_close(a.values().cpu(), want.values(), rtol=1e-5, atol=1e-7)


@pytest.fixture(scope="module")
def bodies(L, ops, N, gpu_device):
    """name -> the body of an existing direct-drive test at its smallest parameter that still launches (n = 0 cases aside),
    called with explicit arguments; its own oracle and bound judge."""
    import index_cases as I
    import test_conditioning_gpu as TC
    import test_gpu_parity as TG
    import test_index_kernels_gpu as TI
    import test_op_audit_gpu as TA
    import test_rowwise_conditioning_gpu as TW
    from oracle import literalkg_oracle as O
    from test_gpu_fuzz import draw
    g = gpu_device
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(g)
    graphs = _fixture_body(TI.sampler_graphs)(ops, g)
    adam_big = _fixture_body(TI.adam_big)(g)
    spmm = _fixture_body(TW.spmm_structure)(ops, g)
    att = _fixture_body(TW.att_structures)(ops, g)
    audit_seed = min((81374, 44053, 3130), key=lambda s: draw(s)["e"])
    out = {
        # test_index_kernels_gpu.py
        "group_by_key": lambda: TI.test_group_by_key(ops, N, dev, 1, 1),
        "group_by_key 65 x 100": lambda: TI.test_group_by_key(ops, N, dev, 65, 100),
        "group_by_key bad keys": lambda: TI.test_group_by_key_counts_keys_outside_the_range(ops, N, dev, 1),
        "group_by_key through ops": lambda: TI.test_group_by_key_through_ops(ops, dev, 1),
        "expand_groups": lambda: TI.test_expand_groups(ops, N, dev, g, 1, 1, 2),
        "gather_i64 and permute": lambda: TI.test_gather_i64_and_permute(ops, N, dev, g, 1),
        "check_grouped": lambda: TI.test_check_grouped(ops, N, dev, g, 1, "last"),
        "sanitize_ids": lambda: TI.test_sanitize_ids(ops, N, dev, g, 1, "last"),
        "gather_rows": lambda: TI.test_gather_rows(ops, N, dev, g, 1),
        "gather_rows float4": lambda: TI.test_gather_rows(ops, N, dev, g, 4),
        "gather_rows_range": lambda: TI.test_gather_rows_range(ops, N, dev, g, 1),
        "fill_rows": lambda: TI.test_fill_rows(ops, N, dev, g, 1),
        "scatter_add_rows": lambda: TI.test_scatter_add_rows_with_perm(ops, N, g, 5),
        "csr_check": lambda: TI.test_csr_check(ops, N, dev, g),
        "csr_extract_rows": lambda: TI.test_csr_extract_rows(ops, N, dev, g, "every third row"),
        "spmm_scatter_bwd": lambda: TI.test_spmm_scatter_bwd(ops, N, g, 1),
        "sampler": lambda: TI.test_sampler_follows_its_documented_stream(ops, N, dev, g, graphs, "dups", 0, 1),
        "adam": lambda: TI.test_adam_against_float64(ops, N, g, adam_big, 1, (0.9, 0.999), 0.0),
        # test_rowwise_conditioning_gpu.py
        "grouped rows": lambda: TW.test_grouped_rows(ops, g, 33, 70, False, 0.0),
        "grouped k": lambda: TW.test_grouped_k(ops, g, 40, 24, 0.0, 0.0),
        "elementwise": lambda: TW.test_elementwise(ops, N, g, 1, False),
        "layernorm": lambda: TW.test_layernorm(ops, g, 257, 32, False, False, False),
        "layernorm narrow": lambda: TW.test_layernorm(ops, g, 4099, 32, False, True, False),
        "layernorm parameter gradients": lambda: TW.test_layernorm_parameter_gradients_under_cancellation(ops, N, g, 32, False,
                                                                                                          False),
        "relu batchnorm": lambda: TW.test_relu_batchnorm(ops, g, 2, 1, 0, True),
        "spmm": lambda: TW.test_spmm_conditioning(ops, g, spmm, 1, False),
        "spmm epilogues": lambda: TW.test_spmm_epilogues(ops, g, spmm, 8, False),
        "attention refresh": lambda: TW.test_attention_refresh(ops, g, att, 4, False),
        "attention row range": lambda: TW.test_attention_row_range(ops, g, att),
        "table scores transe": lambda: TW.test_table_scores_and_losses(ops, g, "transe", 3, 1, False),
        "table scores dot": lambda: TW.test_table_scores_and_losses(ops, g, "dot", 3, 1, False),
        "transr scores": lambda: TW.test_transr_scores_and_losses(ops, g, 3, 1, 1),
        # test_conditioning_gpu.py: the variant sweep of the tall GEMM and the per-op cases
        **{f"tall {v}": (lambda v=v: TC.test_tall_scale_sweep(ops, g, v))
           for v in (None, "256x2", "128x1", "256x1")},
        "tall gate epilogue": lambda: TC.test_tall_gate_epilogue_scale_sweep(ops, g, None),
        "wgrad f16x2": lambda: TC.test_wgrad_f16x2_scale_sweep(ops, g, 16 * 2500),
        **{f"engine {c}": (lambda c=c: TC.test_other_engines_scale_sweep(ops, g, c))
           for c in ("bf16x3_rows", "bf16x3_kmajor", "longk", "f32_mfma", "skinny", "smallm")},
        "gemm f64acc": lambda: TC.test_gemm_f64acc_is_one_rounding_of_float64(ops, g),
        "column sums": lambda: TC.test_column_sums_under_cancellation(ops, g, 300_001),
        "zero rows and columns": lambda: TC.test_zero_rows_columns_and_sparse_k(ops, g),
        "row and column maxima": lambda: TC.test_row_and_column_maxima_are_exact(ops, g),
        "fused linear layernorm edges": lambda: TC.test_fused_linear_act_layernorm_at_the_range_edges(ops, g),
        "scatter_add repeated ids": lambda: TC.test_scatter_add_rows_with_repeated_ids(ops, g),
        # test_gpu_parity.py
        "fused layer epilogue": lambda: TG.test_fused_layer_epilogue_matches_the_unfused_pair(ops, g, 16384 + 5, (32,), 32, 0.0),
        "narrow layer backward": lambda: TG.test_narrow_layer_backward_in_one_launch_matches_the_unfused_passes(
            ops, g, 4096 + 7, "both", 0.0),
        "pre-training gcn_l2_gatenum": lambda: TG.test_module_matches_reference_fixture(L, g, "encoder_gcn_l2_gatenum"),
        "pre-training transe_gcn_l1": lambda: TG.test_module_matches_reference_fixture(L, g, "transe_gcn_l1"),
        "fine-tuning gcn_l2_gatenum": lambda: TG.test_fine_tuning_head_matches_reference_fixture(L, g, "encoder_gcn_l2_gatenum"),
        "fine-tuning gcn_l1": lambda: TG.test_fine_tuning_head_matches_reference_fixture(L, g, "encoder_gcn_l1"),
        "update_att gcn_l1": lambda: TG.test_update_att_through_module(L, O, g),
        "update_att gcn_l2_gatenum": lambda: _update_att(L, O, g, "encoder_gcn_l2_gatenum"),
        # test_op_audit_gpu.py / op_audit.py
        "op audit": lambda: TA.test_every_device_op_of_a_model_step_is_within_its_bound(L, O, g, draw(audit_seed), audit_seed),
    }
    assert set(out) == set(BODIES), ("BODIES (the names pytest parametrises over, needed before any fixture exists) and the "
                                     f"bodies built here differ in {sorted(set(out) ^ set(BODIES))}: name each body in both")
    return out


BODIES = [
    "group_by_key", "group_by_key 65 x 100", "group_by_key bad keys", "group_by_key through ops", "expand_groups",
    "gather_i64 and permute", "check_grouped", "sanitize_ids", "gather_rows", "gather_rows float4", "gather_rows_range",
    "fill_rows", "scatter_add_rows", "csr_check", "csr_extract_rows", "spmm_scatter_bwd", "sampler", "adam",
    "grouped rows", "grouped k", "elementwise", "layernorm", "layernorm narrow", "layernorm parameter gradients",
    "relu batchnorm", "spmm", "spmm epilogues", "attention refresh", "attention row range", "table scores transe",
    "table scores dot", "transr scores",
    "tall None", "tall 256x2", "tall 128x1", "tall 256x1", "tall gate epilogue",
    "wgrad f16x2", "engine bf16x3_rows", "engine bf16x3_kmajor", "engine longk", "engine f32_mfma", "engine skinny",
    "engine smallm", "gemm f64acc", "column sums", "zero rows and columns", "row and column maxima",
    "fused linear layernorm edges", "scatter_add repeated ids",
    "fused layer epilogue", "narrow layer backward", "pre-training gcn_l2_gatenum", "pre-training transe_gcn_l1",
    "fine-tuning gcn_l2_gatenum", "fine-tuning gcn_l1", "update_att gcn_l1", "update_att gcn_l2_gatenum", "op audit",
]


@pytest.mark.parametrize("name", BODIES)
def test_training_side_body(bodies, name):
    """The existing body, its own assertions unchanged, under each perturbation in turn.

    The 'tall 256x1w' body, which once missed test_tall_scale_sweep's bound in one of four runs, left with its tiling,
    the cause unfound (DESIGN_HISTORY.md, "Tall GEMM: tilings and diagnostic builds removed")."""
    RAN.append(name)
    for mode in PERTURBED:
        try:
            with perturbation(mode):
                bodies[name]()
        except AssertionError as e:                 # (the body's own message, with the perturbation it failed under)
            raise AssertionError(f"{name} under '{mode}': {e}") from e


# ----------------------------------------------------------------------------- d. the ledger
def test_ledger(N):
    """Every entry point is classified, and every one that takes a stream (NOT_REACHED aside, and ELSEWHERE, whose cases
    other modules hold) was launched under all three perturbations by the cases above: run the module whole."""
    check_ledger_partition(N.PROTOTYPES)
    assert len(NOT_REACHED) <= 8 and not set(NOT_REACHED) & QUERY_SIDE, sorted(NOT_REACHED)
    ran = set(RAN)
    wanted = {"test_ranking", "test_topk", "test_accepted", "test_retrieval", "test_relations", "test_triples",
              "test_pair_head", "test_softmax_op", "test_softmax_excluded_lists", "test_curve_fit_and_order_kernels",
              "test_device_structure_and_laplacian", "test_golden_model_queries", "test_golden_mlp_head"} | set(BODIES)
    assert wanted <= ran, ("the ledger counts the launches of the cases that ran before it in this process: run the module "
                           f"whole and in file order (no -k, --lf, reordering or xdist); not run: {sorted(wanted - ran)}")
    for mode in PERTURBED:
        missing = REQUIRED - LAUNCHED[mode]
        assert not missing, f"never launched under '{mode}': {sorted(missing)}"
        stray = (LAUNCHED[mode] & set(NOT_REACHED))
        assert not stray, f"listed as not reached, yet launched under '{mode}': {sorted(stray)}"
    print("side_stream(): streams drawn per entry", {d: V.DRAWS.count(d) for d in sorted(set(V.DRAWS))})
