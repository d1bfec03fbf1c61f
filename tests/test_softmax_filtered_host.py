"""No GPU: the checks of tests/softmax_filtered_cases.py accept a correct float32 evaluation of the FILTERED 1-vs-all loss
and its gradients and reject planted faults (mask ignored, truth masked, mask shifted by one column, mask applied in the
forward pass but not in the weights) -- so that a green test_one_vs_all_filtered_gpu.py says something about the kernels;
the exclusion-list reference on a hand-made structure; the argument checks of the new keywords; the ABI's new rows; and
the registers of the softmax kernels from the code-object metadata."""
import math
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import pytest
import torch

import softmax_cases as C
import softmax_filtered_cases as F

SHAPES = [(65, 1000, 17), (130, 257, 3), (20, 2000, 16)]
DEVICE = "MI355X|no CPU"


def _exact(b, n, k, distance):
    q, p, truth = C.integer_tables(b, n, k, seed=b + n + k)
    scale = C.exact_scale(k)
    mask = F.mask_of(F.patterns(b, n, truth, seed=n + k), n)
    ref = F.loss_eval(q, p, truth, mask, distance, scale)
    r32 = float(C.loss_measure(F.loss_eval(q, p, truth, mask, distance, scale, torch.float32)[2], ref).max())
    return q, p, truth, mask, scale, ref, C.loss_bound(r32)


def _online_masked(q, p, truth, mask, distance, scale):
    """the kernel's algorithm in float32 torch: 256-wide tiles, a running (m, l), a masked logit -inf before either"""
    z = C.logits(q, p, distance, scale, torch.float32)
    zt = z.gather(1, truth[:, None])[:, 0]
    z = z.masked_fill(mask, -math.inf)
    m = torch.full((z.shape[0],), -math.inf)
    l_ = torch.zeros(z.shape[0])
    for c0 in range(0, z.shape[1], C.TILE):
        zt_ = z[:, c0:c0 + C.TILE]
        mn = torch.maximum(m, zt_.max(1).values)
        ref = torch.where(torch.isinf(mn), torch.zeros_like(mn), mn)           # safe_ref: an all -inf tile
        l_ = l_ * torch.exp(m - ref) + torch.exp(zt_ - ref[:, None]).sum(1)
        m = mn
    lse = m + torch.log(l_)
    return lse, zt, lse - zt


def test_the_patterns_cover_what_the_kernels_can_get_wrong():
    n, b = 70001, 130
    truth = C.truths(b, n, torch.Generator().manual_seed(0))
    ex = F.patterns(b, n, truth, seed=1)
    assert ex[0] == [] and ex[10] == [] and ex[1] == [0] and ex[2] == [n - 1]
    assert ex[3] == [63, 64, 255, 256] and ex[4] == list(range(64, 128)) and ex[5] == list(range(256, 512))
    assert len(ex[6]) == 1200 and ex[6][0] // 1024 != ex[6][-1] // 1024       # (64 splits of 274 tiles: 4-5 tiles each)
    assert set(ex[17]) == {int(truth[17]) - 1, int(truth[17]) + 1}
    assert len(ex[8]) > 30000 and ex[9] and len(ex[9]) <= 5                    # a long list next to short and empty ones
    for i, row in enumerate(ex):
        assert row == sorted(set(row)) and int(truth[i]) not in row and all(0 <= c < n for c in row)
    xptr, xcol = F.to_lists(ex)
    assert xptr.dtype == torch.int32 and int(xptr[-1]) == xcol.numel() == sum(map(len, ex))
    assert int(F.mask_of(ex, n).sum()) == xcol.numel()
    assert {b_ for b_, _, _ in F.shapes()} == {1, 65, 130} and {k for _, _, k in F.shapes()} == {1, 17, 300}
    assert {n_ for _, n_, _ in F.shapes()} == {1, 255, 257, 1000, 70001} and (130, 70001, 300) in F.shapes()


@pytest.mark.parametrize("distance", [True, False])
@pytest.mark.parametrize("b,n,k", SHAPES)
def test_masked_float32_evaluation_is_accepted_and_faults_are_rejected(b, n, k, distance):
    q, p, truth, mask, scale, ref, bound = _exact(b, n, k, distance)
    r = float(C.loss_measure(_online_masked(q, p, truth, mask, distance, scale)[2], ref).max())
    assert r <= bound and r <= 1e-7, (r, bound)
    for fault in ("mask_ignored", "truth_masked", "mask_shifted"):
        bad = F.loss_eval(q, p, truth, mask, distance, scale, torch.float32, fault=fault)[2]
        r_bad = float(C.loss_measure(bad, ref).max())
        assert r_bad > 10 * bound, (fault, r_bad, bound)


@pytest.mark.parametrize("distance", [True, False])
@pytest.mark.parametrize("b,n,k", SHAPES)
def test_masked_gradient_references_agree_and_reject_faults(b, n, k, distance):
    q, p, truth, g = C.random_tables(b, n, k, seed=b + n + k)
    mask = F.mask_of(F.patterns(b, n, truth, seed=n + k), n)
    scale = 0.37
    ref = F.grads_eval(q, p, truth, g, mask, distance, scale)
    dq64, dp64 = F.autograd_eval(q, p, truth, g, mask, distance, scale, torch.float64)
    assert C.worst(ref["dq"], dq64, ref["dq_scale"]) <= 1e-12             # the closed form IS the derivative
    assert C.worst(ref["dp"], dp64, ref["dp_scale"]) <= 1e-12
    assert bool((ref["v"][mask] == 0).all())                              # exact zeros at the excluded positions
    dq32, dp32 = F.autograd_eval(q, p, truth, g, mask, distance, scale, torch.float32)
    rq, rp = C.worst(dq32, ref["dq"], ref["dq_scale"]), C.worst(dp32, ref["dp"], ref["dp_scale"])
    bq, bp = C.gemm_bound("f32_mfma", rq, n), C.gemm_bound("f32_mfma", rp, b)
    got32 = F.grads_eval(q, p, truth, g, mask, distance, scale, torch.float32)
    assert C.worst(got32["dq"], ref["dq"], ref["dq_scale"]) <= bq
    assert C.worst(got32["dp"], ref["dp"], ref["dp_scale"]) <= bp
    for fault in F.FAULTS_MASK:
        bad = F.grads_eval(q, p, truth, g, mask, distance, scale, torch.float32, fault=fault)
        rq_bad = C.worst(bad["dq"], ref["dq"], ref["dq_scale"])
        rp_bad = C.worst(bad["dp"], ref["dp"], ref["dp_scale"])
        assert max(rq_bad / bq, rp_bad / bp) > 10, (fault, rq_bad, rp_bad)
        if fault == "weights_unmasked":
            assert not bool((bad["v"][mask] == 0).all())


def test_all_but_the_truth_excluded_is_a_zero_loss_in_the_reference():
    q, p, truth, g = C.random_tables(7, 300, 5, seed=1)
    mask = F.mask_of(F.all_but_truth(300, truth), 300)
    assert torch.equal(F.loss_eval(q, p, truth, mask, True, 1.0)[2], torch.zeros(7, dtype=torch.float64))
    ref = F.grads_eval(q, p, truth, g, mask, True, 1.0)
    assert not bool(ref["v"].any()) and not bool(ref["dq"].any()) and not bool(ref["dp"].any())


def test_excluded_reference_on_a_hand_made_structure():
    # entity 0 knows tails 1 (r 0), 2 (r 0 and r 1), 4 (r 1); entity 3 knows tail 0 (r 2)
    filt = (torch.tensor([0, 3, 3, 3, 4, 4]), torch.tensor([1, 2, 4, 0]), torch.tensor([0, 1, 3, 4, 5]),
            torch.tensor([0, 0, 1, 1, 2]))
    rows, rels, truth = torch.tensor([0, 0, 0, 3, 1]), torch.tensor([0, 1, -1, 2, 0]), torch.tensor([1, 4, 2, 2, 0])
    assert F.excluded_reference(filt, rows, rels, truth, 5) == [[2], [2], [1, 4], [0], []]
    pos = torch.tensor([-1, 0, 1, -1, 2], dtype=torch.int32)               # candidates 1, 2, 4
    assert F.excluded_reference(filt, rows, rels, torch.tensor([0, 2, 1, 1, 0]), 3, pos) == [[1], [1], [0, 2], [], []]


# ----------------------------------------------------------------------------- the front end's new checks
def _stand_in(scoring="transe", n=40, c=8, n_rel=3):
    def no_table():
        raise AssertionError("the table was asked for")
    gen = torch.Generator().manual_seed(5)
    return SimpleNamespace(entity_embed=SimpleNamespace(weight=torch.randn(n, c, generator=gen)),
                           relation_embed=SimpleNamespace(weight=torch.randn(n_rel, c, generator=gen)),
                           gat_trans_M=None, n_entities=n, n_relations=n_rel, relation_dim=c, scoring=scoring,
                           training=False, _table_for_inference=no_table, gat_embeddings=no_table)


def test_new_keyword_errors_come_before_any_device_work():
    from literalkg_amd.one_vs_all import one_vs_all_loss
    model = _stand_in()
    ids, r, t = torch.tensor([0, 1, 2]), torch.tensor([0, 1, 2]), torch.tensor([3, 4, 5])
    known = SimpleNamespace(n_entities=41, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="known triples over 41 entities"):
        one_vs_all_loss(model, ids, r, t, known=known)
    with pytest.raises(ValueError, match="candidates must be a 1-D tensor of integer ids"):
        one_vs_all_loss(model, ids, r, t, candidates=torch.tensor([3.0, 4.0]))
    with pytest.raises(ValueError, match="side must be 'tail' or 'head' with candidates"):
        one_vs_all_loss(model, ids, r, t, side="both", candidates=torch.tensor([3, 4, 5]))
    with pytest.raises(ValueError, match="scoring='mlp' has no 1-vs-all loss"):
        one_vs_all_loss(model, ids, r, t, scoring="mlp", candidates=torch.tensor([3, 4, 5]))
    with pytest.raises(RuntimeError, match=DEVICE):                 # a CPU model: refused, the table never asked for
        one_vs_all_loss(model, ids, r, t, candidates=torch.tensor([3, 4, 5]))


def test_ops_refuse_cpu_tensors_and_bad_lists():
    from literalkg_amd import _native, ops
    q, p, truth = torch.randn(3, 8), torch.randn(10, 8), torch.tensor([0, 1, 2])
    ex = F.to_lists([[1], [], [3, 4]])
    with pytest.raises(RuntimeError, match=DEVICE):
        ops.softmax_all_loss(q, p, truth, exclude=ex)
    with pytest.raises(RuntimeError, match=DEVICE):
        ops.softmax_all_forward(q, p, None, truth, exclude=ex)
    filt = tuple(torch.zeros(3, dtype=torch.int32) for _ in range(4))
    with pytest.raises(RuntimeError, match=DEVICE):
        ops.softmax_excluded(filt, truth, truth, truth, 10)
    for name in ("lkg_softmax_excluded", "lkg_softmax_all_partial_masked_f32", "lkg_softmax_all_weights_masked_f32"):
        assert name in _native.PROTOTYPES
    import __graft_entry__ as ge
    ge.build()
    with pytest.raises(_native.LkgError, match="bad sizes"):
        _native.call("lkg_softmax_all_partial_masked_f32", 1, 0, 4, None, 4, None, 4, None, 1.0, 1, None, None, 0, None,
                     None, None)
    with pytest.raises(_native.LkgError, match="null pointer"):
        _native.call("lkg_softmax_all_weights_masked_f32", 1, 5, 4, None, 4, None, 4, None, 0, None, None, None, None, 1.0,
                     None, None, 0, None, 5, None)
    with pytest.raises(_native.LkgError, match="either count"):
        _native.call("lkg_softmax_excluded", 1, 5, 5, None, None, None, None, None, None, None, None, None, None, None,
                     None)
    _native.call("lkg_softmax_all_partial_masked_f32", 0, 5, 4, None, 4, None, 4, None, 1.0, 1, None, None, 0, None, None,
                 None)                                                      # n_q = 0 returns at once


# ----------------------------------------------------------------------------- resources
def test_softmax_kernel_registers():
    """From the code-object metadata (.vgpr_count) of lkg_softmax.hip, keyed on (kernel, VEC, MASKED) -- the partial and
    the weights kernel are one text each with both template parameters, the others have the first only: the masked
    forward instantiations stay within 256 VGPRs (two workgroups per CU are gone beyond), and the unmasked instantiations
    keep the counts of the kernels that had no mask parameter: softmax_partial_kernel 228, softmax_finish_kernel 44,
    softmax_weights_kernel 168 on the 16-byte path and 164 on the scalar path.  (DESIGN 3.6k once recorded 160 for the
    16-byte path; the compiler reports 168, and the section now says so.)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "literalkg_amd", "csrc",
                       "lkg_softmax.hip")
    asm = subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-S", "-o", "-", src],
                         check=True, capture_output=True, text=True).stdout
    found = {}
    for m in re.finditer(r"\.name:\s+\S*?\d+(softmax_[a-z_]+_kernel)ILb([01])E(?:Lb([01])E)?E\S*\n(?:.*\n)*?"
                         r"\s*\.vgpr_count:\s+(\d+)", asm):
        found[(m.group(1), int(m.group(2)), int(m.group(3) or 0))] = int(m.group(4))
    print(found)
    assert found[("softmax_partial_kernel", 1, 1)] <= 256 and found[("softmax_partial_kernel", 0, 1)] <= 256, found
    assert found[("softmax_partial_kernel", 1, 0)] == 228 and found[("softmax_partial_kernel", 0, 0)] == 228, found
    assert found[("softmax_finish_kernel", 1, 0)] == 44 and found[("softmax_finish_kernel", 0, 0)] == 44, found
    assert found[("softmax_weights_kernel", 1, 0)] == 168 and found[("softmax_weights_kernel", 0, 0)] == 164, found
    assert ("softmax_weights_kernel", 1, 1) in found and ("softmax_weights_kernel", 0, 1) in found, found
    assert ("softmax_excluded_kernel", 1, 0) in found, found
    assert len(found) == 12, found            # 4 + 4 instantiations of the two texts, finish x 2, excluded x 2
