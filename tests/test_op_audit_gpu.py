"""Every product and reduction of a real model step, checked per element against float64 on the inputs the model hands it
(op_audit.audit_ops): a pre-training step (forward + backward), a fine-tuning step and an eval forward of the fuzz seeds
whose end-to-end misses were investigated (81374, 44053, 3130), the reference-default architecture and a pruned,
row-sparse case.  An end-to-end parity check cannot say WHICH op lost digits -- near a LeakyReLU kink every upstream
gradient legitimately moves -- a check of each op on its own inputs is not affected by kinks.  Every scale hint the tall
and weight-gradient engines are handed (rowmax, a_colmax, b_colmax) must bound the tensor it describes."""
import pytest
import torch

import op_audit
from test_gpu_fuzz import build_case, draw

pytestmark = pytest.mark.gpu

REFERENCE_DEFAULT = dict(agg="gcn", layers=8, dim=300, conv=32, residual=False, gate="mul", txt_dim=300, scale=300,
                         scoring="transr", rel_dim=300, n=20_000, e=150_000, n_rel=16, batch=200, neg=1, prune=False,
                         mlp_hidden=64, skew="zipf", weight_scale=1.0, batch_pool=0,
                         cfg=dict(num_lit_dim=2, n_mlp_layers=2, alpha=0.1, lamda=0.5))


def configurations():
    out = [pytest.param(draw(s), s, id=f"fuzz{s}") for s in (81374, 44053, 3130)]
    out.append(pytest.param(dict(REFERENCE_DEFAULT), 5, id="reference-default"))
    pruned = draw(1020)
    pruned.update(n=35_000, e=105_000, prune=True, batch=17, layers=2)
    out.append(pytest.param(pruned, 1020, id="pruned-row-sparse"))
    return out


@pytest.fixture(scope="module")
def L(gpu_device):
    import __graft_entry__ as ge
    ge.build()
    import literalkg_amd
    return literalkg_amd


@pytest.fixture(scope="module")
def O():
    from oracle import literalkg_oracle
    return literalkg_oracle


@pytest.mark.parametrize("c,seed", configurations())
def test_every_device_op_of_a_model_step_is_within_its_bound(L, O, gpu_device, c, seed):
    from literalkg_amd import ops
    k = build_case(L, O, gpu_device, c, seed, seed)
    m = k.m
    dev = lambda *xs: [x.to(gpu_device) for x in xs]
    pre_batch = dev(k.bh, k.br, k.bp, k.bn)
    plain = m(*pre_batch, device=gpu_device, mode="pre_training").detach().clone()      # (with grad: the audited path)
    with op_audit.audit_ops(ops) as audit:
        m.zero_grad(set_to_none=True)
        loss = m(*pre_batch, device=gpu_device, mode="pre_training")
        audited = loss.detach().clone()
        loss.backward()
        m.zero_grad(set_to_none=True)
        m(*dev(k.bh, k.bp, k.bn), device=gpu_device, mode="fine_tuning").backward()
        with torch.no_grad():
            m.calc_score(*dev(k.bh[:50], k.bp[:70]))
    print(f"case {seed}: {sum(audit.calls.values())} audited calls {audit.calls}")
    worst = sorted(audit.records, key=lambda r: -(r.r / r.bound if r.bound else 0.0))[:6]
    for r in worst:
        print(f"  {r.op:28s} {r.engine:12s} {str(r.shape):40s} r {r.r:.3g} (bound {r.bound:.3g})  {r.site}")
    for note in audit.hint_notes:
        print("  hint:", note)
    print(f"  calls made from inside ops.py: {audit.inner}")
    # the audit only observes: the audited step computes the same loss, bit for bit
    assert torch.equal(plain, audited), (float(plain), float(audited))
    # the wrappers sit on the module globals, so the calls ops makes to itself are audited too: the Linear backward's
    # weight_grads (ops.py) reaches gemm and the bias gradient's column sums, the gate's backward its weight gradient
    assert audit.inner.get("gemm", 0) > 0, audit.inner
    assert audit.inner.get("colsum", 0) + audit.inner.get("narrow_weight_grad", 0) > 0, audit.inner
    if c["gate"] is not None:
        assert audit.inner.get("gemm_wgrad", 0) + audit.inner.get("narrow_weight_grad", 0) > 0, audit.inner
    if c["scoring"] == "transr":        # the TransR loss's projections and gradients: lkg_grouped_gemm_f32, rows and k mode
        assert audit.calls.get("grouped", 0) > 0, audit.calls
    assert not audit.failures, f"case {seed}:\n" + op_audit.report(audit)
    # a scale hint far above its tensor's maximum costs bits of the split: none in these steps
    assert not audit.hint_notes, audit.hint_notes
