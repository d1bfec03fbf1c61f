"""No GPU: the checks of tests/softmax_cases.py accept a correct float32 evaluation of the 1-vs-all loss and its gradients
and reject planted faults -- so that a green test_one_vs_all_gpu.py says something about the kernels."""
import pytest
import torch

import softmax_cases as C

SHAPES = [(65, 1000, 17), (130, 257, 3), (63, 2000, 16), (7, 600, 300)]


def _exact(b, n, k, distance):
    q, p, truth = C.integer_tables(b, n, k, seed=b + n + k)
    scale = C.exact_scale(k)
    ref = C.loss_eval(q, p, truth, distance, scale)
    r32 = float(C.loss_measure(C.loss_eval(q, p, truth, distance, scale, torch.float32)[2], ref).max())
    return q, p, truth, scale, ref, C.loss_bound(r32)


@pytest.mark.parametrize("distance", [True, False])
@pytest.mark.parametrize("b,n,k", SHAPES)
def test_online_float32_evaluation_is_accepted(b, n, k, distance):
    q, p, truth, scale, ref, bound = _exact(b, n, k, distance)
    r = float(C.loss_measure(C.online_eval(q, p, truth, distance, scale)[2], ref).max())
    assert r <= bound, (r, bound)
    assert r <= 1e-7, r            # the margin the device test relies on: a correct online evaluation is a third of 3e-7


# (a maximum that is not carried shows only where a later tile raises it: the shapes of three tiles and more)
LOSS_FAULT_CASES = [(b, n, k, f) for b, n, k in SHAPES for f in C.FAULTS_LOSS if f != "max_not_carried" or n > 2 * C.TILE]


@pytest.mark.parametrize("distance", [True, False])
@pytest.mark.parametrize("b,n,k,fault", LOSS_FAULT_CASES)
def test_loss_faults_are_rejected(b, n, k, distance, fault):
    q, p, truth, scale, ref, bound = _exact(b, n, k, distance)
    if fault == "max_not_carried":
        got = C.online_eval(q, p, truth, distance, scale, fault=fault)[2]
    else:
        got = C.loss_eval(q, p, truth, distance, scale, torch.float32, fault=fault)[2]
    r = float(C.loss_measure(got, ref).max())
    assert r > 10 * bound, (fault, r, bound)


def test_mean_over_the_wrong_count_is_rejected():
    q, p, truth, scale, ref, bound = _exact(65, 1000, 17, True)
    loss32 = C.loss_eval(q, p, truth, True, scale, torch.float32)[2]
    want = float(C.reduce_eval(ref[2], "mean"))
    denom = float(ref[0].abs().mean() + ref[1].abs().mean())
    assert abs(float(C.reduce_eval(loss32, "mean")) - want) / denom <= bound
    assert abs(float(C.reduce_eval(loss32, "mean", fault="mean_count")) - want) / denom > 10 * bound
    assert abs(float(C.reduce_eval(loss32, "sum")) - float(ref[2].sum())) / (denom * 65) <= bound
    assert torch.equal(C.reduce_eval(loss32, "none"), loss32)


@pytest.mark.parametrize("distance", [True, False])
@pytest.mark.parametrize("b,n,k", SHAPES)
def test_gradient_references_agree_and_reject_faults(b, n, k, distance):
    q, p, truth, g = C.random_tables(b, n, k, seed=b + n + k)
    scale = 0.37
    ref = C.grads_eval(q, p, truth, g, distance, scale)
    dq64, dp64 = C.autograd_eval(q, p, truth, g, distance, scale, torch.float64)
    # the closed form IS the derivative (float64 against float64 autograd)
    assert C.worst(ref["dq"], dq64, ref["dq_scale"]) <= 1e-12
    assert C.worst(ref["dp"], dp64, ref["dp_scale"]) <= 1e-12
    # torch's float32 autograd is accepted by the f32-MFMA engine's bound, every planted fault is far outside it
    dq32, dp32 = C.autograd_eval(q, p, truth, g, distance, scale, torch.float32)
    rq, rp = C.worst(dq32, ref["dq"], ref["dq_scale"]), C.worst(dp32, ref["dp"], ref["dp_scale"])
    bq, bp = C.gemm_bound("f32_mfma", rq, n), C.gemm_bound("f32_mfma", rp, b)
    got32 = C.grads_eval(q, p, truth, g, distance, scale, torch.float32)
    assert C.worst(got32["dq"], ref["dq"], ref["dq_scale"]) <= bq
    assert C.worst(got32["dp"], ref["dp"], ref["dp_scale"]) <= bp
    for fault in C.FAULTS_GRAD:
        if fault == "no_diag" and not distance:
            continue                                  # (dot scoring has no norm term to drop)
        bad = C.grads_eval(q, p, truth, g, distance, scale, torch.float32, fault=fault)
        rq_bad = C.worst(bad["dq"], ref["dq"], ref["dq_scale"])
        rp_bad = C.worst(bad["dp"], ref["dp"], ref["dp_scale"])
        assert max(rq_bad / bq, rp_bad / bp) > 10, (fault, rq_bad, rp_bad)
    # each row of V sums to zero within N u max|V|
    v = got32["v"]
    assert bool((v.sum(1).abs() <= n * C.U * v.abs().max(1).values).all())
    bad_v = C.grads_eval(q, p, truth, g, distance, scale, torch.float32, fault="truth_in_weights")["v"]
    assert not bool((bad_v.sum(1).abs() <= n * C.U * bad_v.abs().max(1).values).all())


def test_the_shape_list_covers_every_size():
    sh = C.shapes((1, 3, 4, 16, 17, 300))
    assert {b for b, _, _ in sh} == {1, 63, 64, 65, 130}
    assert {n for _, n, _ in sh} == {1, 255, 256, 257, 1000, 70001}
    assert {k for _, _, k in sh} == {1, 3, 4, 16, 17, 300}
    assert (130, 70001, 300) in sh
