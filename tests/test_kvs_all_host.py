"""No GPU: the checks of tests/kvs_all_cases.py accept a float32 tiled restatement of the KvsAll kernels' algorithm and
reject planted faults (positives ignored, lists shifted by one column, bias dropped, smoothing with the wrong sign, weights
without the positives, dbias dropped) by more than 10 x the bound -- so that a green test_kvs_all_gpu.py says something
about the kernels; the closed-form gradients are the derivative; the argument checks; the second ABI table against its
header; the error convention of the three entry points; and the registers of the kernels from the code-object metadata."""
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import pytest
import torch

import kvs_all_cases as K
import softmax_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_SHAPES = [(65, 257, 17), (130, 255, 32), (20, 2000, 16), (7, 1000, 300)]
DEVICE = "MI355X|no CPU"


def test_the_patterns_cover_what_the_kernels_can_get_wrong():
    n, b = 70001, 130
    rows = K.patterns(b, n, seed=1)
    assert rows[0] == [] and rows[10] == [] and rows[1] == [0] and rows[2] == [n - 1]
    assert rows[3] == [63, 64, 255, 256] and rows[4] == list(range(64, 128)) and rows[5] == list(range(256, 512))
    assert len(rows[6]) == 1200 and rows[6][0] // 1024 != rows[6][-1] // 1024     # (64 splits of 274 tiles: 4-5 tiles each)
    assert rows[7] == list(range(n))                                               # every candidate a positive
    assert len(rows[8]) > 30000 and rows[9] and len(rows[9]) <= 5                  # a long list next to short and empty ones
    for row in rows:
        assert row == sorted(set(row)) and all(0 <= c < n for c in row)
    yptr, ycol = K.to_lists(rows)
    assert yptr.dtype == torch.int32 and int(yptr[-1]) == ycol.numel() == sum(map(len, rows))
    assert int(K.mask_of(rows, n).sum()) == ycol.numel()
    assert K.patterns(3, 1, seed=0) == [[], [0], [0]]                              # n = 1: what falls outside is dropped
    assert K.SHAPES == [(1, 1, 1), (65, 257, 17), (130, 255, 32), (130, 1000, 300), (65, 70001, 17)]


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("distance", [True, False])
@pytest.mark.parametrize("b,n,k", HOST_SHAPES)
def test_tiled_float32_restatement_is_accepted_and_faults_are_rejected(b, n, k, distance, eps):
    q, p, bias, scale = K.exact_case(b, n, k, distance, seed=b + n + k)
    mask = K.mask_of(K.patterns(b, n, seed=n + k), n)
    ref = K.loss_eval(q, p, bias, mask, distance, scale, eps)
    z32 = K.logits(q, p, bias, distance, scale, torch.float32)
    assert torch.equal(z32.double(), K.logits(q, p, bias, distance, scale))        # the logits ARE exact in float32
    r32 = float(K.loss_measure(K.loss_eval(q, p, bias, mask, distance, scale, eps, torch.float32)[0], ref).max())
    bound = C.loss_bound(r32)
    for splits in (1, 2):
        r = float(K.loss_measure(K.tiled_eval(q, p, bias, mask, distance, scale, eps, splits), ref).max())
        assert r <= bound, (splits, r, bound)
    for fault in K.FAULTS_LOSS:
        if fault == "smoothing_sign" and eps == 0:
            continue                                                               # (no smoothing term to get wrong)
        bad = K.loss_eval(q, p, bias, mask, distance, scale, eps, torch.float32, fault=fault)[0]
        r_bad = float(K.loss_measure(bad, ref).max())
        assert r_bad > 10 * bound, (fault, r_bad, bound)


def test_eps_zero_and_null_bias_are_the_plain_sum_in_the_restatement():
    q, p, bias, scale = K.exact_case(9, 300, 16, True, seed=3)
    mask = K.mask_of(K.patterns(9, 300, seed=4), 300)
    a = K.tiled_eval(q, p, torch.zeros(9), mask, True, scale, 0.0)
    assert torch.equal(a, K.tiled_eval(q, p, None, mask, True, scale, 0.0))
    one = K.loss_eval(q[:1], p[:1], bias[:1], torch.ones((1, 1), dtype=torch.bool), True, scale, 0.0)
    z = K.logits(q[:1], p[:1], bias[:1], True, scale)
    assert torch.equal(one[0], K.softplus(-z)[:, 0])                               # a positive's term is softplus(-z)


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("distance", [True, False])
@pytest.mark.parametrize("b,n,k", HOST_SHAPES[:3])
def test_gradient_references_agree_and_reject_faults(b, n, k, distance, eps):
    q, p, bias, g = K.random_case(b, n, k, seed=b + n + k)
    mask = K.mask_of(K.patterns(b, n, seed=n + k), n)
    scale = 0.37
    ref = K.grads_eval(q, p, bias, mask, g, distance, scale, eps)
    dq64, dp64, db64 = K.autograd_eval(q, p, bias, mask, g, distance, scale, eps, torch.float64)
    assert C.worst(ref["dq"], dq64, ref["dq_scale"]) <= 1e-12                      # the closed form IS the derivative
    assert C.worst(ref["dp"], dp64, ref["dp_scale"]) <= 1e-12
    assert C.worst(ref["dbias"], db64, ref["dbias_scale"]) <= 1e-12
    if eps == 0:                                                                   # the sign of every weight
        assert bool((ref["v"][mask] <= 0).all()) and bool((ref["v"][~mask] >= 0).all())
    dq32, dp32, db32 = K.autograd_eval(q, p, bias, mask, g, distance, scale, eps, torch.float32)
    r32 = {"dq": C.worst(dq32, ref["dq"], ref["dq_scale"]), "dp": C.worst(dp32, ref["dp"], ref["dp_scale"]),
           "dbias": C.worst(db32, ref["dbias"], ref["dbias_scale"])}
    bounds = {"dq": C.gemm_bound("f32_mfma", r32["dq"], n), "dp": C.gemm_bound("f32_mfma", r32["dp"], b),
              "dbias": K.dbias_bound(r32["dbias"])}
    got32 = K.grads_eval(q, p, bias, mask, g, distance, scale, eps, torch.float32)
    for name in bounds:
        assert C.worst(got32[name], ref[name], ref[name + "_scale"]) <= bounds[name], name
    for fault in K.FAULTS_GRAD:
        bad = K.grads_eval(q, p, bias, mask, g, distance, scale, eps, torch.float32, fault=fault)
        ratio = max(C.worst(bad[name], ref[name], ref[name + "_scale"]) / bounds[name] for name in bounds)
        assert ratio > 10, (fault, ratio)


# ----------------------------------------------------------------------------- argument checks
def _stand_in(scoring="transe", n=40, c=8, n_rel=3):
    def no_table():
        raise AssertionError("the table was asked for")
    gen = torch.Generator().manual_seed(5)
    return SimpleNamespace(entity_embed=SimpleNamespace(weight=torch.randn(n, c, generator=gen)),
                           relation_embed=SimpleNamespace(weight=torch.randn(n_rel, c, generator=gen)),
                           gat_trans_M=None, n_entities=n, n_relations=n_rel, relation_dim=c, scoring=scoring,
                           training=False, _table_for_inference=no_table, gat_embeddings=no_table)


def test_argument_errors_come_before_any_device_work():
    import literalkg_amd as L
    from literalkg_amd import kvs_all
    for name in ("kvs_all_loss", "sigmoid_all_loss", "distinct_queries"):
        assert name in L.__all__ and getattr(L, name) is getattr(kvs_all, name)
    assert hasattr(L.LiteralKG, "calc_kvs_all_loss")
    model = _stand_in()
    ent, r = torch.tensor([0, 1, 2]), torch.tensor([0, 1, 2])
    known = SimpleNamespace(n_entities=40, device=torch.device("cpu"), for_side=lambda s: None)
    for kw, msg in ((dict(side="both"), "side must be one of"), (dict(scoring="mlp"), "scoring='mlp' has no KvsAll loss"),
                    (dict(reduction="max"), "reduction must be one of"), (dict(scale=0.0), "scale must be a positive"),
                    (dict(margin=float("inf")), "margin must be a finite number"),
                    (dict(label_smoothing=1.0), r"label_smoothing must be a number in \[0, 1\)"),
                    (dict(label_smoothing=-0.1), r"label_smoothing must be a number in \[0, 1\)"),
                    (dict(splits=65), "splits must be None or an integer"),
                    (dict(scoring="transr"), "needs a model with gat_trans_M"),
                    (dict(candidates=torch.tensor([1.0])), "candidates must be a 1-D tensor of integer ids")):
        with pytest.raises(ValueError, match=msg):
            kvs_all.kvs_all_loss(model, ent, r, known, **kw)
    with pytest.raises(ValueError, match="different lengths"):
        kvs_all.kvs_all_loss(model, ent, r[:2], known)
    with pytest.raises(ValueError, match="known must be the KnownTriples"):
        kvs_all.kvs_all_loss(model, ent, r, None)
    with pytest.raises(ValueError, match="known triples over 41 entities"):
        kvs_all.kvs_all_loss(model, ent, r, SimpleNamespace(n_entities=41, for_side=None))
    with pytest.raises(NotImplementedError, match="row-sharded"):
        kvs_all.kvs_all_loss(SimpleNamespace(local=model), ent, r, known)
    with pytest.raises(RuntimeError, match=DEVICE):                 # a CPU model: refused, the table never asked for
        kvs_all.kvs_all_loss(model, ent, r, known)
    empty = kvs_all.kvs_all_loss(model, ent[:0], r[:0], known, reduction="none")
    assert empty.shape == (0,) and empty.dtype == torch.float32
    from literalkg_amd.distributed import ShardedLiteralKG
    with pytest.raises(NotImplementedError, match="row-sharded"):
        ShardedLiteralKG.calc_kvs_all_loss(None, ent, r, known)


def test_distinct_queries_orders_by_relation_then_entity():
    from literalkg_amd.kvs_all import distinct_queries
    ent = torch.tensor([5, 2, 5, 9, 2, 5])
    rel = torch.tensor([1, 0, 1, 0, 1, 0])
    e, r = distinct_queries(ent, rel)
    assert e.tolist() == [2, 5, 9, 2, 5] and r.tolist() == [0, 0, 0, 1, 1]
    e, r = distinct_queries(ent[:0], rel[:0])
    assert e.numel() == 0 and r.numel() == 0
    with pytest.raises(ValueError, match="different lengths"):
        distinct_queries(ent, rel[:3])


def test_ops_refuse_cpu_tensors_and_bad_lists():
    from literalkg_amd import kvs_all
    q, p, bias = torch.randn(3, 8), torch.randn(10, 8), torch.zeros(3)
    pos = K.to_lists([[1], [], [3, 4]])
    with pytest.raises(RuntimeError, match=DEVICE):
        kvs_all.sigmoid_all_loss(q, p, bias, pos)
    with pytest.raises(RuntimeError, match=DEVICE):
        kvs_all.sigmoid_all_forward(q, p, None, bias, pos)
    with pytest.raises(RuntimeError, match=DEVICE):
        kvs_all.sigmoid_all_weights(q, p, None, bias, torch.ones(3), pos)
    with pytest.raises(ValueError, match="label_smoothing"):
        kvs_all.sigmoid_all_loss(q, p, bias, pos, label_smoothing=True)


# ----------------------------------------------------------------------------- the entry points
NAMES = ["lkg_sigmoid_all_finish_f32", "lkg_sigmoid_all_partial_f32", "lkg_sigmoid_all_weights_f32"]


def test_the_three_entry_points_are_declared_and_bound():
    import __graft_entry__ as ge
    ge.build()
    from literalkg_amd import _native, build
    from wide_cases import prototypes
    assert "lkg_kvsall.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "lkg_kvsall.hip"))
    assert set(NAMES) <= set(_native.PROTOTYPES) and set(NAMES) <= set(prototypes())


def test_error_convention_of_the_three_entry_points():
    import __graft_entry__ as ge
    ge.build()
    from literalkg_amd import _native
    call, E = _native.call, _native.LkgError
    with pytest.raises(E, match="lkg_sigmoid_all_partial_f32: bad sizes"):
        call("lkg_sigmoid_all_partial_f32", 1, 0, 4, None, 4, None, 4, None, None, 1.0, 0.0, 1, None, None, 0, None, None)
    with pytest.raises(E, match="lkg_sigmoid_all_partial_f32: scale must be positive"):
        call("lkg_sigmoid_all_partial_f32", 1, 5, 4, None, 4, None, 4, None, None, 0.0, 0.0, 1, None, None, 0, None, None)
    with pytest.raises(E, match=r"lkg_sigmoid_all_partial_f32: eps must lie in \[0, 1\)"):
        call("lkg_sigmoid_all_partial_f32", 1, 5, 4, None, 4, None, 4, None, None, 1.0, 1.0, 1, None, None, 0, None, None)
    with pytest.raises(E, match="splits must come from lkg_softmax_all_splits"):
        call("lkg_sigmoid_all_partial_f32", 1, 5, 4, None, 4, None, 4, None, None, 1.0, 0.0, 2, None, None, 0, None, None)
    with pytest.raises(E, match="lkg_sigmoid_all_partial_f32: null pointer"):
        call("lkg_sigmoid_all_partial_f32", 1, 5, 4, None, 4, None, 4, None, None, 1.0, 0.0, 1, None, None, 0, None, None)
    call("lkg_sigmoid_all_partial_f32", 0, 5, 4, None, 4, None, 4, None, None, 1.0, 0.0, 1, None, None, 0, None, None)
    with pytest.raises(E, match="lkg_sigmoid_all_finish_f32: bad sizes"):
        call("lkg_sigmoid_all_finish_f32", 1, 0, None, None, None)
    with pytest.raises(E, match="lkg_sigmoid_all_finish_f32: bad sizes"):
        call("lkg_sigmoid_all_finish_f32", -1, 1, None, None, None)
    with pytest.raises(E, match="lkg_sigmoid_all_finish_f32: null pointer"):
        call("lkg_sigmoid_all_finish_f32", 1, 1, None, None, None)
    call("lkg_sigmoid_all_finish_f32", 0, 1, None, None, None)
    with pytest.raises(E, match="lkg_sigmoid_all_weights_f32: bad sizes"):       # the chunk does not lie in the table
        call("lkg_sigmoid_all_weights_f32", 1, 5, 4, None, 4, None, 4, None, None, 3, 7, None, 1.0, 0.0, None, None, 0,
             None, 5, None, None)
    with pytest.raises(E, match="lkg_sigmoid_all_weights_f32: bad sizes"):       # ldv < the chunk's width
        call("lkg_sigmoid_all_weights_f32", 1, 5, 4, None, 4, None, 4, None, None, 0, 5, None, 1.0, 0.0, None, None, 0,
             None, 4, None, None)
    with pytest.raises(E, match="lkg_sigmoid_all_weights_f32: null pointer"):
        call("lkg_sigmoid_all_weights_f32", 1, 5, 4, None, 4, None, 4, None, None, 0, 5, None, 1.0, 0.0, None, None, 0,
             None, 5, None, None)
    call("lkg_sigmoid_all_weights_f32", 0, 5, 4, None, 4, None, 4, None, None, 0, 5, None, 1.0, 0.0, None, None, 0, None,
         5, None, None)                                                            # n_q = 0 returns at once


# ----------------------------------------------------------------------------- resources
def test_kvs_all_kernel_registers():
    """From the code-object metadata of lkg_kvsall.hip: the forward kernel stays within 256 VGPRs (two workgroups per CU
    are gone beyond, as for the masked softmax kernel), neither path of any kernel spills or uses scratch, and the source
    is part of the library's build."""
    from literalkg_amd import build
    assert "lkg_kvsall.hip" in build.SOURCES
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "literalkg_amd", "csrc", "lkg_kvsall.hip")
    asm = subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-S", "-o", "-", src],
                         check=True, capture_output=True, text=True).stdout
    found = {}
    for m in re.finditer(r"\.name:\s+\S*?\d+(sigmoid_[a-z_]+_kernel)(?:ILb([01])E)?\S*\n(?:.*\n)*?\s*\.vgpr_count:\s+(\d+)",
                         asm):
        found[(m.group(1), int(m.group(2) or 0))] = int(m.group(3))
    print(found)
    assert set(found) == {("sigmoid_partial_kernel", 0), ("sigmoid_partial_kernel", 1), ("sigmoid_weights_kernel", 0),
                          ("sigmoid_weights_kernel", 1), ("sigmoid_finish_kernel", 0)}, found
    assert found[("sigmoid_partial_kernel", 1)] <= 256 and found[("sigmoid_partial_kernel", 0)] <= 256, found
    assert found[("sigmoid_weights_kernel", 1)] <= 256 and found[("sigmoid_weights_kernel", 0)] <= 256, found
    assert not re.search(r"\.vgpr_spill_count:\s+[1-9]", asm) and not re.search(r"\.private_segment_fixed_size:\s+[1-9]", asm)
