"""CPU tier of the autograd surface (autograd_cases.py; the device tier is test_autograd_surface_gpu.py):

  1. the registry is complete: every torch.autograd.Function subclass of literalkg_amd/ops.py, found by introspection, has
     an entry, and every parameter of its forward is classified (differentiable / by design without a gradient, with the
     line that says so / not a tensor); a Function added without an entry fails here
  2. every restatement, in float64 on a cut-down shape: its gradients under every input subset x output subset equal the
     all-trainable ones exactly (plain torch does not care which leaves are frozen: this pins the restatement), and
     torch.autograd.gradcheck passes
  3. the comparator rejects planted faults: pure-torch stand-in Functions that produce wrong values only, each beside a
     correct twin that passes -- a needed gradient returned as None, two same-shaped weight gradients in each other's slots,
     the gradient of an unused output taken as ones, a bias sum that rides on a weight gradient and is dropped with it, a
     second step that reads a table the first step left dirty"""
import pytest
import torch

import autograd_cases as AC


@pytest.fixture(scope="module")
def ops():
    from literalkg_amd import ops as _ops
    return _ops


# ----------------------------------------------------------------------------- 1. completeness
def test_every_function_of_ops_has_an_entry_and_every_parameter_a_class(ops):
    found = AC.functions(ops)
    assert len(found) >= 23
    assert set(found) == set(AC.REGISTRY), (f"without an entry: {sorted(set(found) - set(AC.REGISTRY))}; entries without a "
                                            f"Function: {sorted(set(AC.REGISTRY) - set(found))}")
    for name, cls in found.items():
        e = AC.REGISTRY[name]
        assert AC.forward_params(cls) == list(e.params), (name, AC.forward_params(cls), list(e.params))
        assert set(e.params.values()) <= {"diff", "none", "config"}, name
        for p, kind in e.params.items():
            if kind == "none":
                why = e.by_design_none.get(p, "")
                assert "model.py" in why or "ops.py" in why, f"{name}.{p}: by design without a gradient needs the line that says so"
        assert set(e.by_design_none) <= set(e.params), name
        fixed = {p for p, k in e.params.items() if k == "diff" and not p.startswith("*")}
        varargs = [p for p, k in e.params.items() if p.startswith("*")]
        assert all(e.params[p] == "diff" for p in varargs), name
        seen = set()
        for v in e.variants:
            inp = e.build("cpu", v, small=True)
            assert inp.slots and inp.outputs and set(inp.upstream) == set(inp.outputs), (name, v)
            rest = [s for s in inp.slots if s not in fixed]           # the varargs of this variant
            assert not rest or varargs, f"{name} [{v}]: slots {rest} are no parameter of forward"
            assert not varargs or rest, f"{name} [{v}]: no slot for {varargs}"
            assert all(inp.t[s].is_floating_point() for s in inp.slots), (name, v)
            seen |= set(inp.slots) & fixed
        assert seen == fixed, f"{name}: no variant makes {sorted(fixed - seen)} a slot"


def test_enumerators():
    e = AC.REGISTRY["_FusedGate"]
    inp = e.build("cpu", e.variants[0], small=True)
    subs = AC.input_subsets(e, inp)
    assert len(inp.slots) == 11 and len(set(subs)) == len(subs)
    for s in inp.slots:
        assert frozenset([s]) in subs and frozenset(inp.slots) - {s} in subs
    assert frozenset(("lit0", "lit1")) in subs and AC.fg_model_subset(inp) in subs and frozenset(inp.slots) in subs
    e = AC.REGISTRY["_TransRLoss"]
    inp = e.build("cpu", "group 7", small=True)
    assert len(AC.input_subsets(e, inp)) == 7                      # every non-empty subset of three slots
    e = AC.REGISTRY["_StackedLinear"]
    assert len(AC.output_subsets(e, e.build("cpu", e.variants[0], small=True))) == 7


# ----------------------------------------------------------------------------- 2. the restatements
CASES = [(n, v) for n, e in AC.REGISTRY.items() for v in e.variants if "drop" not in v]


@pytest.mark.parametrize("name,variant", CASES)
def test_restatement_in_float64(name, variant):
    e = AC.REGISTRY[name]
    inp = e.build("cpu", variant, small=True)
    allset = frozenset(inp.slots)
    for outs in AC.output_subsets(e, inp):
        full = AC.restated_grads(e, inp, allset, outs, torch.float64)
        assert any(g is not None for g in full.values())
        for subset in AC.input_subsets(e, inp):
            part = AC.restated_grads(e, inp, subset, outs, torch.float64)
            for s in inp.slots:
                if s in subset and full[s] is not None:
                    assert part[s] is not None and part[s].dtype == torch.float64 and torch.equal(part[s], full[s]), (outs, subset, s)
                else:
                    assert part[s] is None, (outs, subset, s)
    lv = inp.leaves(allset, torch.float64)

    def f(*xs):
        t = dict(lv.t)
        t.update(zip(inp.slots, xs))
        res = e.restate(AC.Inputs(variant, inp.slots, inp.outputs, t, inp.cfg, inp.upstream, inp.rows), torch.float64)
        return tuple(res[o] for o in inp.outputs)
    assert torch.autograd.gradcheck(f, [lv.t[s] for s in inp.slots], eps=1e-6, atol=1e-5, rtol=1e-4, fast_mode=True)


# ----------------------------------------------------------------------------- 3. planted faults
class _Toy(torch.autograd.Function):
    """(y1, y2) = (x wg^T + x wz^T + bias, x wz^T): two same-shaped weights, a bias, two outputs -- the skeleton of the fused
    gate's backward in plain torch.  ``fault`` plants one mistake of the kind the matrix is there to catch."""

    @staticmethod
    def forward(ctx, x, wg, wz, bias, fault):
        ctx.save_for_backward(x, wg, wz)
        ctx.fault = fault
        ctx.set_materialize_grads(False)
        return x @ wg.t() + x @ wz.t() + bias, x @ wz.t()

    @staticmethod
    def backward(ctx, g1, g2):
        x, wg, wz = ctx.saved_tensors
        need, fault = ctx.needs_input_grad, ctx.fault
        if g1 is None and g2 is None:
            return None, None, None, None, None
        zeros = torch.zeros(x.shape[0], wg.shape[0], dtype=x.dtype)
        if g2 is None and fault == "unused output as ones":
            g2 = torch.ones_like(zeros)
        g1 = zeros if g1 is None else g1
        g2 = zeros if g2 is None else g2
        gx = g1 @ wg + (g1 + g2) @ wz if need[0] else None
        g_wg = g1.t() @ x if need[1] else None
        g_wz = (g1 + g2).t() @ x if (need[2] and fault != "needed gradient is None") else None
        if fault == "weight gradients swapped":
            g_wg, g_wz = ((g1 + g2).t() @ x if need[1] else None), (g1.t() @ x if need[2] else None)
        gb = None
        if need[3]:
            gb = g1.sum(0)
            if fault == "bias sum rides on a weight gradient" and not need[1]:
                gb = torch.zeros_like(gb)           # (the pass that would have carried it did not run)
        return gx, g_wg, g_wz, gb, None


FAULTS = ("needed gradient is None", "weight gradients swapped", "unused output as ones", "bias sum rides on a weight gradient")


def _toy_entry(fault):
    def build(device, variant, small=True, seed=0):
        gen = torch.Generator().manual_seed(3 + seed)
        rn = lambda *s: torch.randn(*s, generator=gen)
        t = {"x": rn(9, 4), "wg": rn(4, 4), "wz": rn(4, 4), "bias": rn(4)}
        return AC.Inputs(variant, list(t), ["y1", "y2"], t, {}, {"y1": rn(9, 4), "y2": rn(9, 4)})
    e = AC.Entry("_Toy", {}, ["9x4"], build, lambda ops, inp: dict(zip(("y1", "y2"), _Toy.apply(*[inp.t[s] for s in inp.slots], fault))),
                 lambda inp, dtype: {"y1": inp.t["x"] @ inp.t["wg"].t() + inp.t["x"] @ inp.t["wz"].t() + inp.t["bias"],
                                     "y2": inp.t["x"] @ inp.t["wz"].t()}, AC.PRODUCT)
    del AC.REGISTRY["_Toy"]                 # (a stand-in: not a Function of ops.py)
    return e


def test_the_twin_without_a_fault_passes():
    e = _toy_entry(None)
    assert AC.run_matrix(e, None, e.build("cpu", "9x4")) == []


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_fault_is_caught(fault):
    e = _toy_entry(fault)
    faults = AC.run_matrix(e, None, e.build("cpu", "9x4"))
    assert faults, fault
    where = {"needed gradient is None": "wz: asked for, no gradient", "weight gradients swapped": "wg: error",
             "unused output as ones": "outputs y1", "bias sum rides on a weight gradient": "bias: error"}[fault]
    assert any(where in f for f in faults), faults
    if fault == "bias sum rides on a weight gradient":          # all trainable passes: only a partial subset shows it
        assert not any("all trainable" in f for f in faults) and all("wg" not in f.split("{")[1].split("}")[0] for f in faults), faults
    if fault == "unused output as ones":
        assert not any("outputs y1+y2" in f for f in faults), faults


class _ToyTable(torch.autograd.Function):
    """table[ids] with the backward of _RowScratch in miniature: the gradient is scattered into ONE table kept all-zero
    between steps; each step first clears the rows the previous one touched.  fault: the rows are put on record only when
    the table needs a gradient -- a step with the table frozen (its rows scattered all the same) leaves them dirty."""
    kept = {}

    @staticmethod
    def forward(ctx, table, scale, ids, fault):
        ctx.save_for_backward(ids, scale, table)
        ctx.fault = fault
        return table[ids] * scale

    @staticmethod
    def backward(ctx, g):
        ids, scale, table = ctx.saved_tensors
        st = _ToyTable.kept.setdefault("t", dict(buf=torch.zeros_like(table), dirty=[]))
        for old in st["dirty"]:
            st["buf"][old] = 0
        st["dirty"] = []
        st["buf"].index_add_(0, ids, g * scale)
        if ctx.needs_input_grad[0] or not ctx.fault:
            st["dirty"].append(ids)
        return st["buf"].clone(), ((g * table[ids]).sum() if ctx.needs_input_grad[1] else None), None, None


def _table_entry(fault):
    def build(device, variant, small=True, seed=0):
        gen = torch.Generator().manual_seed(5 + seed)
        ids = torch.randperm(12, generator=gen)[:4] if seed else torch.randint(0, 12, (4,), generator=gen)
        t = {"table": torch.randn(12, 3, generator=gen), "scale": torch.randn((), generator=gen), "ids": ids}
        return AC.Inputs(variant, ["table", "scale"], ["rows"], t, {}, {"rows": torch.randn(4, 3, generator=gen)})
    e = AC.Entry("_ToyTable", {}, ["12x3"], build, lambda ops, inp: {"rows": _ToyTable.apply(inp.t["table"], inp.t["scale"], inp.t["ids"], fault)},
                 lambda inp, dtype: {"rows": inp.t["table"][inp.t["ids"]] * inp.t["scale"]}, AC.PRODUCT)
    del AC.REGISTRY["_ToyTable"]
    return e


@pytest.mark.parametrize("fault", [False, True], ids=["twin", "dirty table"])
def test_a_table_left_dirty_by_a_partial_step_is_caught(fault):
    e = _table_entry(fault)
    faults = AC.scratch_check(e, None, "cpu", "12x3", reset=_ToyTable.kept.clear)
    if not fault:
        assert faults == []
    else:
        assert faults and all("after a step with trainable {scale}" in f for f in faults), faults
