"""GPU: every torch.autograd.Function of ops.py under every subset of inputs that require a gradient and every subset of
outputs that are used (autograd_cases.py holds the registry, the enumerators and the judge).

Every other test of the suite makes every floating-point input trainable.  Here one test is one Function variant; it loops
over input_subsets x output_subsets, runs the Function through its public wrapper with exactly that subset requiring a
gradient, backs the used outputs with fixed upstream gradients, and judges each run five ways:

  1. structure    a slot asked for has a gradient of the input's shape and dtype; a slot not asked for has .grad None (not
                  zeros); a by-design-none slot (attention values, running buffers, slot0) has None even when it requires one
  2. launches     _native.call is wrapped (as test_invariance_gpu.recorded does) and the entry points the branch must take are
                  present, those it must not take absent, per subset (autograd_cases' expect of each entry)
  3. bits         where the subset's gradients come from the launches of the all-trainable run on the same operands and the
                  kernels add in a fixed order, they carry that run's bits (invariance.same_bits)
  4. float64      every gradient against torch's float64 autograd of the restatement on the same float32 operands: largest
                  absolute error over the largest absolute entry of the float64 gradient, against the bound the existing test
                  of that Function applies to its all-trainable gradients -- asserted for the all-trainable subset first
  5. scratch      a variant that goes through _RowScratch: the partial step is followed by an all-trainable step on other ids;
                  that step's table gradients carry the bits of the same step run first on a fresh registry

Dropout (one variant each of _ActLayerNorm and _NarrowLayer, the kernel's own mask): 1, 2 and bits / closeness against the
all-trainable run with the same seed.

Measured on an MI355X (the measure of 4; `all`: every input trainable, `partial`: the worst partial subset, `torch f32`:
torch's float32 autograd of the restatement on the device -- for _BiMix and _GateBlend the shared references evaluate in
float64 whatever the leaves' type, so that column is one rounding of the result):

  Function          all        partial    torch f32  | Function          all        partial    torch f32
  _MultiLinear      6.17e-07   6.17e-07   5.31e-06   | _FusedGate        1.16e-06   1.16e-06   4.30e-06
  _StackedLinear    9.56e-07   9.56e-07   3.89e-06   | _Aggregate        2.34e-07   3.34e-07   1.30e-07
  _MatMul           3.59e-07   3.59e-07   3.34e-07   | _AggregateKeep    1.32e-07   (1 slot)   1.31e-07
  _FoldNT           2.72e-08   2.72e-08   8.55e-08   | _Fanout           4.57e-08   (1 slot)   4.57e-08
  _Axpby            4.99e-08   4.99e-08   4.99e-08   | _AssembleCat      0          0          0
  _Mul              3.59e-08   3.59e-08   3.59e-08   | _TransELoss       4.86e-07   4.86e-07   6.52e-07
  _LeakySum         7.74e-10   7.74e-10   7.74e-10   | _TransRLoss       5.06e-07   5.06e-07   4.46e-07
  _BiMix            7.25e-08   7.25e-08   4.61e-08   | _DotLoss          1.54e-07   (1 slot)   1.44e-07
  _ActLayerNorm     4.92e-07   5.84e-07   2.65e-07   | _GatherPair       5.48e-08   (1 slot)   5.48e-08
  _NarrowLayer      2.71e-07   5.95e-07   3.06e-06   | _ReluBatchNorm    1.15e-07   1.15e-07   1.41e-07
  _FusedLayer       1.27e-06   1.66e-06   3.26e-06   | _SoftmaxAllLoss   7.57e-07   7.57e-07   7.57e-07
  _GateBlend        1.31e-07   1.31e-07   4.85e-08   |

The bounds (1e-4 for the products, rtol 1e-3 / atol 1e-6 for the losses) are inherited from the direct tests: the table
shows the room they leave.  On the parent commit the eight literal-table cases of _FusedGate fail (a slot asked for, no
gradient); nothing else did.

The model-level test freezes parameter groups of two configurations and holds the loss and every remaining gradient to the
float64 oracle on the CPU, at the tolerance of test_gpu_parity._module_against_oracle (loss 1e-4, gradients 2e-3 of the
largest entry).  Measured: the worst gradient over all freeze sets is 1.1e-6 of its largest entry (bi-interaction, gate,
TransR) and 3.2e-5 (GCN with residual, TransE; aggregator_layers.0.layer_normalize.weight), the same with everything
trainable."""
import re

import numpy as np
import pytest
import torch

import autograd_cases as AC

pytestmark = pytest.mark.gpu
MEASURES = {}


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
def O():
    from oracle import literalkg_oracle
    return literalkg_oracle


def _fresh_scratch(ops):
    ops._RowScratch._tables = {}


CASES = [(n, v) for n, e in AC.REGISTRY.items() for v in e.variants]


@pytest.mark.parametrize("name,variant", CASES)
def test_function_under_partial_gradients(ops, gpu_device, monkeypatch, name, variant):
    assert set(AC.functions(ops)) == set(AC.REGISTRY)
    monkeypatch.setattr(ops._RowScratch, "_tables", {})
    if name == "_FusedLayer":
        monkeypatch.setattr(ops, "FUSED_LAYER", True)
    assert ops._WGRAD_ENGINE == "longk" and ops._ENGINE == "f16x2"        # (the defaults: the branches of the table are theirs)
    e = AC.REGISTRY[name]
    inp = e.build(gpu_device, variant)
    faults = AC.run_matrix(e, ops, inp, MEASURES)
    if e.scratch(inp):
        faults += AC.scratch_check(e, ops, gpu_device, variant, lambda: _fresh_scratch(ops))
    torch.cuda.synchronize()
    ops.check_deferred_errors()
    m = MEASURES.get(name, [0, 0, 0])
    print(f"{name} [{variant}]: all {m[0]:.3g} partial {m[1]:.3g} torch f32 {m[2]:.3g}")
    assert not faults, f"{len(faults)} fault(s):\n" + "\n".join(faults[:12])


def test_measures_are_reported():
    """the table of the module docstring, from this run (python -m pytest -s shows it)"""
    for name in AC.REGISTRY:
        m = MEASURES.get(name)
        if m is not None:
            print(f"  {name:<16} all {m[0]:<9.3g} partial {m[1]:<9.3g} torch f32 {m[2]:<9.3g}")


# ----------------------------------------------------------------------------- the literal tables of the fused gate
@pytest.mark.parametrize("variant", list(AC.FG))
def test_fused_gate_literal_gradients_agree_with_the_unfused_path(ops, gpu_device, monkeypatch, variant):
    """From 16 384 rows on the gate is one launch (ops.fused_gate); below, ops.multi_linear + ops.gate_blend (gate.py:64),
    whose literal tables get their gradient from _MultiLinear.  Both paths on the same 16 387-row operands with the
    literal tables trainable: the same literal gradients (1e-4 of the largest entry, the bound of the fused gate's other
    gradients), and float64's.  With the literals frozen -- the model's case -- the backward's launches are as before."""
    monkeypatch.setattr(ops._RowScratch, "_tables", {})
    e = AC.REGISTRY["_FusedGate"]
    inp = e.build(gpu_device, variant)
    lits = AC.fg_lits(inp)
    nl = len(lits)
    want64 = AC.restated_grads(e, inp, frozenset(inp.slots), ("out",), torch.float64)
    for subset in (frozenset(lits), frozenset(inp.slots), frozenset(lits[:1] + ["x"])):
        fused = AC.applied(e, ops, inp, subset, ("out",))
        lv = inp.leaves(subset)
        panels = [lv.t["x"]] + [lv.t[s] for s in lits]
        gpre = ops.multi_linear(panels, [lv.t[f"wg{i}"] for i in range(nl + 1)], lv.t["bg"])
        zpre = ops.multi_linear(panels, [lv.t[f"wz{i}"] for i in range(nl + 1)], lv.t["bz"])
        out = ops.gate_blend(lv.t["x"], gpre, zpre)
        out.backward(AC.upstream_for(ops, lv, ("out",))["out"])
        for s in lits:
            if s in subset:
                g = fused.grads[s]
                assert g is not None and g.shape == inp.t[s].shape, (variant, sorted(subset), s)
                assert AC.norm_measure(g, lv.t[s].grad.double()) <= AC.PRODUCT, (variant, sorted(subset), s)
                assert AC.norm_measure(g, want64[s]) <= AC.PRODUCT, (variant, sorted(subset), s)
            else:
                assert fused.grads[s] is None
    model_case = AC.applied(e, ops, inp, AC.fg_model_subset(inp), ("out",))
    assert all(model_case.grads[s] is None for s in lits)
    if AC.fg_no_stats(inp, AC.fg_model_subset(inp)):     # the blend kernel without its statistics: autograd_cases._fg_expect
        assert model_case.bwd[:2] == ["lkg_gate_blend_bwd_f32", "lkg_gemm_tall_f32"] and "lkg_gemm_wgrad_f32" not in model_case.bwd
    elif "tagged" not in variant:
        assert model_case.bwd == ["lkg_gate_blend_bwd_stats_f32", "lkg_gemm_tall_f32", "lkg_gemm_wgrad_f32", "lkg_gemm_wgrad_f32"]
    else:
        assert "g_gate_lit0" not in model_case.pools and model_case.bwd.count("lkg_scatter_add_rows_range_f32") == 1


@pytest.mark.parametrize("variant", ["16387xd32 lits (2,12)", "16387xd32 lit (5)"])
def test_literal_caches_follow_an_update_of_a_trainable_literal_table(L, ops, gpu_device, variant):
    """The fused gate keeps the row maxima (_lkg_rowmax) and, for a wide table, the column maxima (tagged_colmax(cache=True))
    of a literal table on the tensor, keyed by its version.  Two steps with a trainable literal table and an Adam step of
    lr = 3 in between (every entry moves by 3: the old maxima are far too small): the second step's output and gradients
    equal float64 on the UPDATED table."""
    from literalkg_amd.optim import Adam
    e = AC.REGISTRY["_FusedGate"]
    inp = e.build(gpu_device, variant)
    lv = inp.leaves(frozenset(inp.slots))
    lits = AC.fg_lits(inp)
    opt = Adam([lv.t[s] for s in lits], lr=3.0)
    before = [lv.t[s].detach().clone() for s in lits]
    for step in range(2):
        for s in inp.slots:
            lv.t[s].grad = None
        out = e.apply(ops, lv)["out"]
        out.backward(inp.upstream["out"])
        if step == 0:
            opt.step()
            assert all(float((lv.t[s].detach() - b).abs().median()) > 2.9 for s, b in zip(lits, before))
            assert all(ops.tagged_colmax(lv.t[s]) is None for s in lits)           # (the cached maxima are of the old version)
    now = AC.Inputs(variant, inp.slots, inp.outputs, {k: (v.detach() if torch.is_tensor(v) else v) for k, v in lv.t.items()},
                    inp.cfg, inp.upstream, inp.rows)
    l64 = now.leaves(frozenset(inp.slots), torch.float64)
    out64 = e.restate(l64, torch.float64)["out"]
    out64.backward(inp.upstream["out"].double())
    # the output per element, by op_audit's allowances (the updated literals are at +-3, the pre-activations at +-10: the absolute
    # tolerance of test_gpu_parity.py:510 is for operands below 1): the tall engine's componentwise bound on each
    # pre-activation carried through the blend's derivatives, plus the blend kernel's own roundings and activation allowances.
    # Row maxima of the old table (3 x too small or worse) push the fp16 planes past their range: errors of order 1 or inf.
    import op_audit as A
    nl = len(lits)
    t64 = {k: v.detach() for k, v in l64.t.items() if torch.is_tensor(v)}
    panels = [t64["x"]] + [t64[s] for s in lits]
    pre = {}
    for name, b in (("wg", "bg"), ("wz", "bz")):
        v64 = sum(p @ t64[f"{name}{i}"].t() for i, p in enumerate(panels)) + t64[b]
        sc = sum(p.abs() @ t64[f"{name}{i}"].abs().t() for i, p in enumerate(panels)) + t64[b].abs()
        v32 = sum(p.float() @ t64[f"{name}{i}"].float().t() for i, p in enumerate(panels)) + t64[b].float()
        pre[name] = (v64, sc, A.bound_for("tall_f16x2", A.componentwise(v32, v64, sc)[0]))
    want, scale, n_round, extra = A.gate_blend_fwd_ref(t64["x"], pre["wg"][0], pre["wz"][0])
    s_, t_ = torch.sigmoid(pre["wz"][0]), torch.tanh(pre["wg"][0])
    allow = (A.units(n_round) * scale + extra + pre["wg"][2] * s_ * (1 - t_ * t_) * pre["wg"][1]
             + pre["wz"][2] * (t_ - t64["x"]).abs() * s_ * (1 - s_) * pre["wz"][1])
    excess = (out.detach().double() - want).abs() - allow
    assert torch.isfinite(out).all() and float(excess.max()) <= 0.0, (variant, float(excess.max()), float(allow.max()))
    torch.testing.assert_close(want, out64.detach(), rtol=1e-12, atol=1e-14)         # (the restatement the gradients are held to)
    for s in inp.slots:
        assert AC.norm_measure(lv.t[s].grad, l64.t[s].grad) <= AC.PRODUCT, (variant, s)


# ----------------------------------------------------------------------------- the model under frozen parameter groups
FREEZE = {
    "entity table": lambda k: k == "entity_embed.weight",
    "gate": lambda k: k.startswith(("emb_mul_lit.", "emb_num_lit.", "emb_txt_lit.")),
    "aggregator Linear weights": lambda k: bool(re.fullmatch(r"aggregator_layers\.\d+\.linear\w*\.weight", k)),
    "LayerNorm affine pairs": lambda k: ".layer_normalize." in k,
    "relation table + gat_trans_M": lambda k: k in ("relation_embed.weight", "gat_trans_M"),
    "everything except linear_gat": lambda k: not k.startswith("linear_gat."),
}


@pytest.mark.parametrize("agg,gate,scoring,residual", [("bi-interaction", "mul", "transr", False), ("gcn", None, "transe", True)])
def test_model_with_frozen_parameter_groups_matches_the_float64_oracle(L, O, gpu_device, agg, gate, scoring, residual):
    """One pre-training step per freeze set (and one with everything trainable, asserted first) against the oracle in float64
    on the CPU with the same leaves frozen: the loss, every remaining gradient, .grad None for the frozen ones, and an Adam
    step over ALL parameters afterwards leaves the frozen ones bit-identical."""
    from literalkg_amd import io
    from literalkg_amd.optim import Adam
    from literalkg_amd.synth import make_batch, make_kg
    n, n_rel, dim = AC.N_BIG, 16, 32
    h, t, r = make_kg(n, 60_000, seed=5)
    cfg = O.default_cfg(embed_dim=dim, relation_dim=dim, conv_dim=dim, n_conv_layers=2, aggregation_type=agg, scale_gat_dim=dim,
                        use_num_lit=gate == "mul", use_txt_lit=gate == "mul", txt_lit_dim=12, use_residual=residual,
                        mlp_hidden_dim=48, kg_l2loss_lambda=1e-4, device=gpu_device)
    torch.manual_seed(3)
    num = torch.rand(n, 2) if gate else None
    txt = torch.randn(n, cfg.txt_lit_dim) if gate else None
    a_in = io.initial_a_in(n, h, t, r)
    m = L.LiteralKG(cfg, n, n_rel, a_in, num, txt, scoring=scoring)
    with torch.no_grad():
        m.entity_embed.weight.mul_(30)
        m.relation_embed.weight.mul_(3)
    params = {k: v.detach().clone() for k, v in m.state_dict().items() if k != "A_in"}
    m.to(gpu_device).eval()
    batch = [torch.from_numpy(x) for x in make_batch(n, 200, 3, seed=9)]
    names = [k for k, v in m.named_parameters() if k != "A_in" and v.is_floating_point()]
    a64 = a_in.double() if a_in.is_floating_point() else a_in
    n64 = lambda x: x.double() if x is not None else None
    steps = []
    for what, frozen_if in [("nothing", lambda k: False)] + list(FREEZE.items()):
        frozen = {k for k in names if frozen_if(k)}
        if what != "nothing" and not frozen:
            assert what == "gate" and gate is None, what          # (the only group a configuration may lack)
            continue
        for k, v in m.named_parameters():
            if k != "A_in":
                v.requires_grad_(k not in frozen)
                v.grad = None
        loss = m(*[b.to(gpu_device) for b in batch], device=gpu_device, mode="pre_training")
        loss.backward()
        p = {k: v.double().clone().requires_grad_(v.is_floating_point() and k not in frozen) for k, v in params.items()}
        want = O.pre_training_loss(p, cfg, a64, *batch, num=n64(num), txt=n64(txt), form=scoring)
        want.backward()
        np.testing.assert_allclose(float(loss.detach()), float(want.detach()), rtol=1e-4, err_msg=what)
        steps.append(what)
        worst = (0.0, None)
        for k, v in m.named_parameters():
            if k == "A_in":
                continue
            if k in frozen:
                assert v.grad is None, (what, k)
                continue
            ref = p[k].grad
            if ref is None:                     # (a parameter the step does not reach)
                assert v.grad is None or float(v.grad.abs().max()) == 0.0, (what, k)
                continue
            assert v.grad is not None, (what, k)
            err = float((v.grad.double().cpu() - ref).abs().max()) / (float(ref.abs().max()) + 1e-12)
            assert err < 2e-3, (what, k, err)
            worst = max(worst, (err, k))
        print(f"{agg} / {scoring}, frozen: {what} ({len(frozen)} of {len(names)} parameters): loss {float(loss.detach()):.6f} "
              f"(float64 {float(want.detach()):.6f}), worst gradient {worst[0]:.3g} of its largest entry ({worst[1]})")
        held ={k: v.detach().clone() for k, v in m.named_parameters() if k in frozen}
        moving = {k: v.detach().clone() for k, v in m.named_parameters() if k in names and k not in frozen and v.grad is not None}
        Adam([v for k, v in m.named_parameters() if k != "A_in"], lr=1e-3).step()
        for k, v in m.named_parameters():
            if k in held:
                assert torch.equal(v.detach(), held[k]), (what, k)
        assert any(not torch.equal(v.detach(), moving[k]) for k, v in m.named_parameters() if k in moving), what
        with torch.no_grad():                   # back to the drawn parameters for the next freeze set
            for k, v in m.named_parameters():
                if k in params:
                    v.copy_(params[k])
    assert len(steps) == (7 if gate else 6), steps
