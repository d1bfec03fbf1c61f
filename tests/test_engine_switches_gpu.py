"""GPU: every path a process-wide engine switch of literalkg_amd/ops.py selects, held to float64 (the CPU tier
is test_engine_switches_host.py).  Every other test of the suite runs the defaults; here the switches are flipped with
monkeypatch.setattr(ops, NAME, value) -- every use reads the module global at call time -- and every tensor and model is built
AFTER the switch is set (row and column maxima are cached on tensor objects).

    S0 defaults            S3 _ENGINE = "f16x2-all"          S6 NARROW_LAYER = False
    S1 _ENGINE = "bf16x3"  S4 _WGRAD_ENGINE = "bf16x3"       S7 FOLD_F64 = False
    S2 _ENGINE = "f32"     S5 S2 and S4 together             S8 CHECK_STRUCTURES = False (the benchmarked launch sequence)

1. dispatch (S0..S5)   ops.gemm_engine names the engine of DISPATCH below for every (setting, shape); the lkg_gemm* launches
                       recorded during ops.gemm / ops.multi_linear are that engine's entry point; the result meets op_audit's
                       componentwise allowance for that engine against the float64 product.
2. Functions           the autograd registry (autograd_cases.py) under the switches: structure, float64 at the entry's own
                       bound, and the setting's own launch expectations (run_matrix's ``expect``), over every input subset x
                       output subset.  Under S1 / S2 (and S5) the fused gate, the fused layer and (S2) the narrow layer are not
                       taken (gate_fusable / fused_layer_ok / narrow_layer_ok say no): the routes gate.py and model.py fall back
                       to -- multi_linear + gate_blend, multi_linear + act_layernorm, linear + act_layernorm -- are judged on
                       the operands of those entries against the same float64 restatements.  Dropout variants are left out
                       (no float64 reference).  A guard runs every Function outside the list under S0 and asserts that it
                       launches no lkg_gemm* / lkg_gate_blend_bwd* entry point: a Function that starts using an engine must
                       join the list.
3. the model           one pre-training step per (configuration, setting) against the float64 oracle on the CPU: loss
                       rtol 1e-4, every gradient within 2e-3 of the float64 gradient's largest entry
                       (test_gpu_parity._module_against_oracle); and the switch is LIVE: the entry points it removes are present
                       under S0 in the configuration that has them, absent under the setting.
4. the C-level three   LKG_GEMM_F32_ONLY, LKG_ACTLN_NARROW_OFF, LKG_SMALLM_BLOCKS, each in a fresh child (switch_child.py).

What the dispatch table shows: S1 and S2 never reach lkg_gemm_tall_f32; S2 never reaches lkg_gemm_skinny_f32 and hands
lkg_gemm_f32 no workspace, so its row-major products are f32_mfma; S4 never reaches lkg_gemm_longk_f32 or lkg_gemm_smallm_f32;
S3 sends the plain 16461 x 256 product to the tall engine even untagged.  Under S5 a long weight gradient (A^T B, k = 4099) is
bf16x3_kmajor, NOT exact f32: no Python switch makes a long weight gradient exact f32, only the C-level LKG_GEMM_F32_ONLY.

What the Function tier shows: under S3 the data gradients of _MultiLinear's 32- and 12-wide
panels go to lkg_gemm_skinny_f32 exactly as under S0 (ops._skinny is asked before tall_ok); the 2-wide panel's, and
_StackedLinear's, stay on lkg_gemm_tall_f32.  _SoftmaxAllLoss reaches ops.gemm too (65 x 257 tables: f32_mfma under every
setting) and is run under S1, S2 and S4.

What the model tier shows: neither configuration of the frozen-groups test runs a narrow layer (bi-interaction projects through
ops.linear + leaky_relu_sum, the residual through the folded Linear), so a third one -- gcn, no residual, TransE -- carries
lkg_narrow_layer_bwd_f32 for S2 and S6.  lkg_gemm_longk_f32 is launched by NO configuration at 16 387 rows (it needs k in
whole 16-row tiles): its absence under S4 would be vacuous there, the test asserts it is absent under S0 as well, and the
dispatch tier holds it (shape i).

What the children cannot prove: the library has no query for LKG_ACTLN_NARROW_OFF and LKG_SMALLM_BLOCKS.  A child shows that the
results hold under them, not that the other kernel ran.  (LKG_GEMM_F32_ONLY has one: lkg_gemm_f32_engine reports 0.)

What was shown able to fail (each on a scratch copy, one narrow run on an MI355X): tall_ok made to ignore _ENGINE fails
test_dispatch_table[S1] ('a tagged': tall_f16x2 named where bf16x3_rows is written), the S1 launch expectations of
_MultiLinear (both 16 387-row variants), _StackedLinear and the layer route ("fwd lkg_gemm_tall_f32: 1 launched, expected
none"), the gate route's gate_fusable assertion, and the liveness check of both model configurations under S1;
`bias if i == 0 else None` made `bias` in _MultiLinear.forward's loop fails the forward float64 judge of
test_function_under_a_switch[S1-_MultiLinear-16387x(32,2,12)->32] (error 0.116 of the largest entry > 1e-4; tagged: 0.078) and
shape d of test_dispatch_table[S1]; gb[:d] for both bias halves in the no-statistics branch of _FusedGate.backward fails the two
new FG variants of test_function_under_partial_gradients under S0 (bz: error 2.39 / 2.95 of the largest entry > 1e-4).

Measured on an MI355X.  Functions (the measure of autograd_cases.judge64; `all`: every input trainable, `partial`: the worst
partial subset, `torch f32`: torch's float32 autograd of the restatement; bound 1e-4):

  setting Function        all       partial   torch f32 | setting Function        all       partial   torch f32
  S1 _MultiLinear         6.17e-07  8.09e-07  5.31e-06  | S3 _MultiLinear         6.17e-07  6.17e-07  5.31e-06
  S1 _StackedLinear       9.26e-07  9.32e-07  3.89e-06  | S3 _StackedLinear       9.13e-07  9.32e-07  3.89e-06
  S1 _MatMul              3.59e-07  3.59e-07  3.34e-07  | S3 _MatMul              3.59e-07  3.59e-07  3.34e-07
  S1 _SoftmaxAllLoss      7.57e-07  7.57e-07  7.57e-07  | S4 _MultiLinear         1.00e-06  1.05e-06  5.31e-06
  S1 gate route           9.90e-07  1.27e-06  4.30e-06  | S4 _StackedLinear       9.13e-07  9.32e-07  3.89e-06
  S1 layer route          9.09e-07  1.39e-06  3.26e-06  | S4 _MatMul              3.59e-07  3.59e-07  3.34e-07
  S2 _MultiLinear         6.17e-07  6.28e-07  5.31e-06  | S4 _SoftmaxAllLoss      7.57e-07  7.57e-07  7.57e-07
  S2 _StackedLinear       9.13e-07  9.32e-07  3.89e-06  | S4 _FusedGate           1.33e-06  1.33e-06  4.30e-06
  S2 _MatMul              3.59e-07  3.59e-07  3.34e-07  | S4 _FusedLayer          1.05e-06  1.42e-06  3.26e-06
  S2 _SoftmaxAllLoss      7.57e-07  7.57e-07  7.57e-07  | S4 _NarrowLayer         2.71e-07  5.84e-07  3.06e-06
  S2 gate route           9.99e-07  1.17e-06  4.30e-06  | S5 _MultiLinear         1.02e-06  1.02e-06  5.31e-06
  S2 layer route          1.29e-06  1.90e-06  3.26e-06  | S5 gate route           1.21e-06  1.21e-06  4.30e-06
  S2 narrow route         4.36e-07  6.96e-07  3.06e-06  | S7 fold route           8.93e-08  8.93e-08  8.55e-08

The model (loss equal to float64's to six digits everywhere; worst gradient over its largest entry, bound 2e-3; S7 meets it,
so no bound had to be measured):

  configuration                        S0        S1        S2        S3        S4        S5        S6        S7        S8        S8 side stream
  bi-interaction + mul gate + TransR   1.01e-06  1.25e-06  1.10e-06  1.01e-06  1.01e-06  1.10e-06  1.01e-06  -         1.01e-06  1.01e-06
  gcn + residual + TransE              3.17e-05  2.57e-05  2.11e-05  3.26e-05  3.09e-05  2.05e-05  3.21e-05  3.13e-05  3.19e-05  3.20e-05
  gcn + TransE (narrow layer)          1.30e-06  -         1.18e-06  -         -         -         1.44e-06  -         -         -
  gcn + residual + TransE, width 64    6.44e-05  -         -         2.39e-04  -         -         -         -         -         -

(the residual rows: aggregator_layers.0.layer_normalize.weight / .bias, whose float-atomic column sums move in the last digit
from run to run.)  lkg_gemm_tall_f32 launches of one step, (S0, S3): gate configuration (2, 2), residual (1, 1), width 64 (2, 5).

The children (engine of the two lkg_gemm_f32 products; their error next to torch's float32; the worst r / bound of the six
row-wise cases; r of lkg_gemm_smallm_f32 32 x 32 / 64 x 96 and whether two runs agree bit for bit):

  unset                    1, 2   5.58e-07 (7.44e-07), 3.17e-07 (2.11e-06)   0.470   2.64e-08 / 3.00e-08   no / no
  LKG_GEMM_F32_ONLY=1      0, 0   7.44e-07 (7.44e-07), 3.38e-07 (2.11e-06)   0.470   2.49e-08 / 2.91e-08   no / no
  LKG_ACTLN_NARROW_OFF=1   1, 2   5.58e-07 (7.44e-07), 3.17e-07 (2.11e-06)   0.470   2.70e-08 / 2.91e-08   no / no
  LKG_SMALLM_BLOCKS=1      1, 2   5.58e-07 (7.44e-07), 3.17e-07 (2.11e-06)   0.470   1.13e-07 / 2.57e-07   yes / yes
  LKG_SMALLM_BLOCKS=100000 1, 2   5.58e-07 (7.44e-07), 3.17e-07 (2.11e-06)   0.470   2.70e-08 / 2.81e-08   no / no"""
import contextlib
import json
import os
import subprocess
import sys

import pytest
import torch

import autograd_cases as AC
import op_audit as A

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

SETTINGS = {
    "S0": {}, "S1": {"_ENGINE": "bf16x3"}, "S2": {"_ENGINE": "f32"}, "S3": {"_ENGINE": "f16x2-all"},
    "S4": {"_WGRAD_ENGINE": "bf16x3"}, "S5": {"_ENGINE": "f32", "_WGRAD_ENGINE": "bf16x3"}, "S6": {"NARROW_LAYER": False},
    "S7": {"FOLD_F64": False}, "S8": {"CHECK_STRUCTURES": False},
}


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


@contextlib.contextmanager
def switched(ops, setting):
    """the module globals of one setting (and a fresh scratch registry), put back on the way out"""
    assert (ops._ENGINE, ops._WGRAD_ENGINE, ops.NARROW_LAYER, ops.FOLD_F64, ops.CHECK_STRUCTURES) == \
        ("f16x2", "longk", True, True, True), "the suite runs the defaults (tests/conftest.py turns the structure check on)"
    with pytest.MonkeyPatch.context() as mp:
        for name, value in SETTINGS[setting].items():
            mp.setattr(ops, name, value)
        mp.setattr(ops._RowScratch, "_tables", {})
        yield


# ============================================================================= 1. the dispatch table
ENTRY_POINT = {"skinny": "lkg_gemm_skinny_f32", "tall_f16x2": "lkg_gemm_tall_f32", "smallm": "lkg_gemm_smallm_f32",
               "longk": "lkg_gemm_longk_f32", "f32_mfma": "lkg_gemm_f32", "bf16x3_rows": "lkg_gemm_f32",
               "bf16x3_kmajor": "lkg_gemm_f32"}
T, R, KM, F, SK, SM, LK = "tall_f16x2", "bf16x3_rows", "bf16x3_kmajor", "f32_mfma", "skinny", "smallm", "longk"
# shape -> the engine under S0 .. S5, derived from ops.gemm_engine (ops.py) and lkg_gemm_f32_engine / lkg_gemm_*_ok (csrc):
#   skinny   not trans_a, alpha 1, _ENGINE != f32, k n <= 2048 or m < 16384, lkg_gemm_skinny_ok (m >= 4096, k, n <= 64 in fours)
#   tall     not trans_a, tall_ok: _ENGINE f16x2 / f16x2-all, m >= 16384, one panel only when tagged with row maxima or f16x2-all
#   smallm / longk   trans_a, not trans_b, alpha 1, beta 0, no bias, _WGRAD_ENGINE longk; m <= 64 and k >= 4096 / k >= 8192 in
#            whole 16-row tiles
#   lkg_gemm_f32     with the workspace (m >= 16384 rows, not trans_a) unless _ENGINE is f32: bf16x3_rows; else trans_a, not
#            trans_b, k >= 2048: bf16x3_kmajor; else f32_mfma
# d (ops.multi_linear, three panels): one tall launch, or the loop of accumulating products, one engine per panel
DISPATCH = {
    "a tagged":   (T, R, F, T, T, F),           # 16461 x 256 . 256^T, row maxima on the operand
    "a untagged": (R, R, F, T, R, F),
    "b":          (F, F, F, F, F, F),           # 300 x 40 . 40 x 24
    "c":          (SK, SK, F, SK, SK, F),       # 4099 x 32 . 32^T
    "d":          (T, (SK, R, SK), (F, F, F), T, T, (F, F, F)),      # 16461 x (32, 2, 12) -> 32
    "e":          (KM, KM, KM, KM, KM, KM),     # A^T B, k = 4099, 256 x 128
    "f":          (SM, SM, SM, SM, KM, KM),     # A^T B, k = 4099, 32 x 32
    "g":          (F, F, F, F, F, F),           # A^T B, k = 2000, 96 x 40
    "h tagged":   (T, R, F, T, T, F),           # a with alpha = 0.5, beta = 2, bias, out=
    "h untagged": (R, R, F, T, R, F),
    "i":          (LK, LK, LK, LK, KM, KM),     # A^T B, k = 8192, 96 x 40 (the one shape of the table lkg_gemm_longk_f32 takes)
}


def _draw(shape, dev):
    """(a, b, kwargs of ops.gemm, k) -- or for d (panels, weights, bias, k)"""
    gen = torch.Generator(device=dev).manual_seed(21 + len(shape) + ord(shape[0]))
    rn = lambda *s, std=1.0: torch.randn(*s, device=dev, generator=gen) * std
    base = shape.split()[0]
    if base in ("a", "h"):
        a, b = rn(16461, 256), rn(256, 256, std=0.1)
        kw = dict(trans_b=True)
        if base == "h":
            kw.update(alpha=0.5, beta=2.0, bias=rn(256), out=rn(16461, 256))
        return a, b, kw, 256
    if base == "b":
        return rn(300, 40), rn(40, 24, std=0.2), {}, 40
    if base == "c":
        return rn(4099, 32), rn(32, 32, std=0.2), dict(trans_b=True), 32
    if base == "d":
        ks = (32, 2, 12)
        return [rn(16461, k) for k in ks], [rn(32, k, std=0.2) for k in ks], rn(32, std=0.1), sum(ks)
    k, m, n = {"e": (4099, 256, 128), "f": (4099, 32, 32), "g": (2000, 96, 40), "i": (8192, 96, 40)}[base]
    return rn(k, m), rn(k, n), dict(trans_a=True), k


def _componentwise_fault(what, names, got, want64, scale64, ref32, k):
    r32 = A.componentwise(ref32, want64, scale64)[0]
    r = A.componentwise(got, want64, scale64)[0]
    bound = max(A.bound_for(e, r32, k) for e in names)
    print(f"  {what:<16} {'+'.join(names):<28} r {r:.3g}  torch f32 {r32:.3g}  bound {bound:.3g}")
    return None if r <= bound else f"{what}: r {r:.3g} > {bound:.3g} ({'+'.join(names)}, torch f32 {r32:.3g})"


@pytest.mark.parametrize("setting", ["S0", "S1", "S2", "S3", "S4", "S5"])
def test_dispatch_table(ops, gpu_device, setting):
    col = int(setting[1])
    faults = []
    with switched(ops, setting):
        for shape, row in DISPATCH.items():
            want = row[col]
            if shape == "d":
                xs, ws, bias, k = _draw(shape, gpu_device)
                with AC.launches() as seen:
                    got = ops.multi_linear(xs, ws, bias)
                if want == T:
                    assert ops.tall_ok(16461, 32, (32, 2, 12)), (setting, shape)
                    names = (T,)
                else:       # the loop of _MultiLinear.forward: product i accumulates onto the output of product i - 1
                    assert not ops.tall_ok(16461, 32, (32, 2, 12)), (setting, shape)
                    names = tuple(ops.gemm_engine(x, w, trans_b=True, beta=0.0 if i == 0 else 1.0, out=None if i == 0 else got,
                                                  bias=bias if i == 0 else None) for i, (x, w) in enumerate(zip(xs, ws)))
                    assert names == want, (setting, shape, names, want)
                x64 = [x.double() for x in xs]
                want64 = sum(x @ w.double().t() for x, w in zip(x64, ws)) + bias.double()
                scale64 = sum(x.abs() @ w.double().abs().t() for x, w in zip(x64, ws)) + bias.double().abs()
                ref32 = sum(x @ w.t() for x, w in zip(xs, ws)) + bias
            else:
                a, b, kw, k = _draw(shape, gpu_device)
                if "tagged" in shape and "untagged" not in shape:
                    ops.tag_rowmax(a, ops.row_absmax(a))
                c0 = kw["out"].clone() if "out" in kw else None
                name = ops.gemm_engine(a, b, **kw)
                assert name == want, (setting, shape, name, want)
                names = (name,)
                with AC.launches() as seen:
                    got = ops.gemm(a, b, **kw)
                a_, b_ = (a.t() if kw.get("trans_a") else a), (b.t() if kw.get("trans_b") else b)
                alpha, beta = kw.get("alpha", 1.0), kw.get("beta", 0.0)
                want64 = alpha * (a_.double() @ b_.double())
                scale64 = abs(alpha) * (a_.double().abs() @ b_.double().abs())
                ref32 = alpha * (a_ @ b_)
                if c0 is not None:
                    want64 = want64 + beta * c0.double() + kw["bias"].double()
                    scale64 = scale64 + abs(beta) * c0.double().abs() + kw["bias"].double().abs()
                    ref32 = ref32 + beta * c0 + kw["bias"]
            products = [n for n in seen if n.startswith("lkg_gemm")]
            assert products == [ENTRY_POINT[n] for n in names], (setting, shape, products, names)
            bad = _componentwise_fault(f"{setting} {shape}", names, got, want64, scale64, ref32, k)
            if bad:
                faults.append(bad)
    torch.cuda.synchronize()
    ops.check_deferred_errors()
    assert not faults, "\n".join(faults)


def test_what_the_dispatch_table_shows():
    """the sentences of the module docstring, read off the table"""
    flat = lambda v: v if isinstance(v, tuple) else (v,)
    col = lambda s: [n for row in DISPATCH.values() for n in flat(row[s])]
    assert T not in col(1) and T not in col(2) and T not in col(5)
    assert SK not in col(2) and R not in col(2) and SK not in col(5) and R not in col(5)
    assert not {LK, SM} & set(col(4)) and not {LK, SM} & set(col(5))
    assert DISPATCH["a untagged"][3] == T and DISPATCH["a untagged"][0] == R
    assert DISPATCH["e"][5] == KM                       # S5: a long weight gradient is bf16 x 3, not exact f32
    for s in range(6):
        assert {T, R, F, SK, KM} & set(col(s)), s
    assert {T, R, KM, F, SK, SM, LK} == set(col(0))     # every engine ops.gemm_engine can name is in the S0 column


# ============================================================================= 2. the Functions under the switches
MEASURES = {}           # (setting, name) -> [all-trainable, worst partial, torch float32]
NO_LONG_WGRAD = ("lkg_gemm_longk_f32", "lkg_gemm_smallm_f32", "lkg_gemm_wgrad_f32", "lkg_gate_blend_bwd_stats_f32")


def _absent(*names):
    return {(phase, n): False for phase in ("fwd", "bwd") for n in names}


def _expect_for(setting, entry):
    """the launch expectations of one setting for one entry (an ``expect`` of autograd_cases.run_matrix)"""
    name = entry.name

    def expect(inp, subset, outs):
        e = {}
        if setting == "S3":
            # f16x2-all changes nothing the registry's shapes reach except one-panel untagged products of >= 16 384 rows that are
            # no skinny ones: _StackedLinear's data gradient (its forward asks for the tall engine under S0 too)
            e = dict(entry.expect(inp, subset, outs))
            if name == "_StackedLinear":
                e[("fwd", "lkg_gemm_tall_f32")] = 1
                e[("bwd", "lkg_gemm_tall_f32")] = int("x" in subset)
            return e
        if setting in ("S1", "S2", "S5"):
            e.update(_absent("lkg_gemm_tall_f32", "lkg_linear_act_layernorm_fwd_f32"))
            if name == "_MultiLinear" and "tagged" in inp.variant:      # still _backward_on_rows
                e[("bwd", "lkg_gather_rows_range_f32")] = True
                e[("bwd", "lkg_scatter_add_rows_range_f32")] = sum(1 for s in subset if s[0] == "x")
        if setting in ("S2", "S5"):
            e.update(_absent("lkg_gemm_skinny_f32", "lkg_narrow_layer_bwd_f32"))
        if setting in ("S4", "S5"):
            e.update(_absent(*NO_LONG_WGRAD))
            if name in ("_FusedGate", "gate route"):
                e[("bwd", "lkg_gate_blend_bwd_f32")] = 1
        if name == "_SoftmaxAllLoss":
            e.update(entry.expect(inp, subset, outs))
        return e
    return expect


def _route(name, base, apply):
    """an entry that is not a Function of ops.py: the route the model takes where ``base``'s Function is not available, on
    base's operands, against base's float64 restatement at base's bound"""
    e = AC.Entry(name, base.params, base.variants, base.build, apply, base.restate, base.bound, named=base.named)
    del AC.REGISTRY[name]
    return e


def _gate_route(ops, inp):                  # gate.py: multi_linear + gate_blend
    nl = inp.cfg["n_lit"]
    x, lits = inp.t["x"], [inp.t[f"lit{i}"] for i in range(nl)]
    assert not ops.gate_fusable(x, lits, x.shape[1])
    gpre = ops.multi_linear([x] + lits, [inp.t[f"wg{i}"] for i in range(nl + 1)], inp.t["bg"])
    zpre = ops.multi_linear([x] + lits, [inp.t[f"wz{i}"] for i in range(nl + 1)], inp.t["bz"])
    return {"out": ops.gate_blend(x, gpre, zpre)}


def _layer_route(ops, inp):                 # model.py, Aggregator._linear_finish: multi_linear + act_layernorm
    xs, ws = [inp.t["x0"], inp.t["x1"]], [inp.t["w0"], inp.t["w1"]]
    assert not ops.fused_layer_ok(xs[0].shape[0], ws[0].shape[0], [x.shape[1] for x in xs])
    assert not ops.fused_layer_wanted(xs, ws, (inp.t["bias"], inp.t["gamma"], inp.t["beta"]))
    y, yn = ops.act_layernorm(ops.multi_linear(xs, ws, inp.t["bias"]), inp.t["gamma"], inp.t["beta"])
    return {"y": y, "yn": yn}


def _narrow_route(ops, inp):                # model.py, Aggregator._linear_finish: linear + act_layernorm
    assert not ops.narrow_layer_ok(inp.t["x"], inp.t["w"]) and not ops._skinny(inp.t["x"], 32)
    y, yn = ops.act_layernorm(ops.linear(inp.t["x"], inp.t["w"], inp.t.get("bias")), inp.t["gamma"], inp.t["beta"])
    return {"y": y, "yn": yn}


ROUTES = {"gate route": _route("gate route", AC.REGISTRY["_FusedGate"], _gate_route),
          "layer route": _route("layer route", AC.REGISTRY["_FusedLayer"], _layer_route),
          "narrow route": _route("narrow route", AC.REGISTRY["_NarrowLayer"], _narrow_route)}
PRODUCTS = ("_MultiLinear", "_StackedLinear", "_MatMul", "_SoftmaxAllLoss")
PAIRS = {
    "S1": PRODUCTS + ("gate route", "layer route"),
    "S2": PRODUCTS + ("gate route", "layer route", "narrow route"),
    "S3": ("_MultiLinear", "_StackedLinear", "_MatMul"),
    "S4": PRODUCTS + ("_FusedGate", "_FusedLayer", "_NarrowLayer"),
    # the combination.  gate_fusable is False under _ENGINE = "f32": what runs on _FusedGate's operands is the gate's route
    "S5": ("_MultiLinear", "gate route"),
}
# every Function an engine switch can reach: those of PAIRS, _FoldNT (S7), and the two the routes go through
LISTED = set(PRODUCTS) | {"_FusedGate", "_FusedLayer", "_NarrowLayer", "_FoldNT", "_GateBlend", "_ActLayerNorm"}


def _entry(name):
    return ROUTES.get(name) or AC.REGISTRY[name]


def _forward_faults(e, ops, inp):
    """the outputs themselves (run_matrix judges gradients): each against the float64 restatement, by the measure and at the
    bound of the entry's gradients"""
    none = frozenset()
    got = e.apply(ops, inp.leaves(none))
    want = e.restate(inp.leaves(none, torch.float64), torch.float64)
    faults = []
    for o in inp.outputs:
        r = AC.norm_measure(got[o], want[o])
        if not r <= e.bound:
            faults.append(f"{e.name} [{inp.variant}] output {o}: error {r:.3g} of the largest entry > {e.bound:.3g}")
    return faults


FUNCTION_CASES = [(s, n, v) for s, names in PAIRS.items() for n in names for v in _entry(n).variants if "drop" not in v]


@pytest.mark.parametrize("setting,name,variant", FUNCTION_CASES)
def test_function_under_a_switch(ops, gpu_device, monkeypatch, setting, name, variant):
    e = _entry(name)
    with switched(ops, setting):
        if name == "_FusedLayer":
            monkeypatch.setattr(ops, "FUSED_LAYER", True)
        inp = e.build(gpu_device, variant)
        if name == "gate route" or name == "_FusedGate":
            lits = [inp.t[s] for s in AC.fg_lits(inp)]
            assert ops.gate_fusable(inp.t["x"], lits, inp.t["x"].shape[1]) == (setting in ("S0", "S3", "S4"))
        faults = _forward_faults(e, ops, inp)
        faults += AC.run_matrix(e, ops, inp, MEASURES.setdefault(setting, {}), expect=_expect_for(setting, e))
        torch.cuda.synchronize()
        ops.check_deferred_errors()
    m = MEASURES[setting].get(e.name, [0, 0, 0])
    print(f"{setting} {name} [{variant}]: all {m[0]:.3g} partial {m[1]:.3g} torch f32 {m[2]:.3g}")
    assert not faults, f"{len(faults)} fault(s):\n" + "\n".join(faults[:12])


def test_fold_in_float32(ops, gpu_device):
    """S7: ops.fold_nt through matmul(a, b.t()) on _FoldNT's operands -- no lkg_gemm_f64acc_f32, both gradients at the bound of
    the products (2 units of the largest entry is the float64 fold's promise, not this path's)"""
    base = AC.REGISTRY["_FoldNT"]
    e = AC.Entry("fold route", base.params, base.variants, base.build, lambda ops_, inp: {"c": ops_.fold_nt(inp.t["a"], inp.t["b"])},
                 base.restate, AC.PRODUCT)
    del AC.REGISTRY["fold route"]
    with switched(ops, "S7"):
        inp = e.build(gpu_device, e.variants[0])
        assert tuple(inp.t["a"].shape) == (8, 6) and tuple(inp.t["b"].shape) == (5, 6)
        faults = _forward_faults(e, ops, inp) + AC.run_matrix(e, ops, inp, MEASURES.setdefault("S7", {}),
                               expect=lambda inp_, subset, outs: {**_absent("lkg_gemm_f64acc_f32"), ("fwd", "products"): 1,
                                                                  ("bwd", "products"): len(subset)})
        torch.cuda.synchronize()
        ops.check_deferred_errors()
    assert not faults, "\n".join(faults)


def test_no_other_function_reaches_an_engine(ops, gpu_device):
    """Every registry entry outside LISTED, once, all-trainable, first variant, under the defaults: no lkg_gemm* and no
    lkg_gate_blend_bwd* entry point.  A Function that starts using an engine fails here and must join the list."""
    assert LISTED <= set(AC.REGISTRY)
    with switched(ops, "S0"):
        for name, e in AC.REGISTRY.items():
            if name in LISTED:
                continue
            inp = e.build(gpu_device, e.variants[0])
            run = AC.applied(e, ops, inp, frozenset(inp.slots), tuple(inp.outputs))
            hit = [n for n in run.fwd + run.bwd if n.startswith(("lkg_gemm", "lkg_gate_blend_bwd"))]
            assert not hit, (name, hit)
        torch.cuda.synchronize()
        ops.check_deferred_errors()


def test_function_measures_are_reported():
    """the table of the module docstring, from this run (python -m pytest -s shows it)"""
    for setting in sorted(MEASURES):
        for name, m in MEASURES[setting].items():
            print(f"  {setting} {name:<16} all {m[0]:<9.3g} partial {m[1]:<9.3g} torch f32 {m[2]:<9.3g}")


# ============================================================================= 3. one model step per setting
# (aggregator, gate, scoring, residual, width).  The first two are those of the frozen-groups test; neither runs a narrow layer,
# and at width 32 every one-panel product of theirs is a skinny one whatever the engine, so two more carry what they cannot:
GATE = ("bi-interaction", "mul", "transr", False, 32)
RES = ("gcn", None, "transe", True, 32)
NARROW = ("gcn", None, "transe", False, 32)     # the 32 -> 32 layer in one launch backward: lkg_narrow_layer_bwd_f32 (S2, S6)
WIDE = ("gcn", None, "transe", True, 64)        # 64 x 64 Linears on untagged inputs: bf16x3_rows under S0, the tall engine under S3
MODEL_CASES = ([(c, s) for c in (GATE, RES) for s in ("S0", "S1", "S2", "S3", "S4", "S5", "S6", "S8")] + [(RES, "S7")]
               + [(NARROW, s) for s in ("S0", "S2", "S6")] + [(WIDE, s) for s in ("S0", "S3")])
# setting -> (entry point, the configuration that launches it under S0; None: none does at 16 387 rows)
LIVE = {
    "S1": [("lkg_gemm_tall_f32", GATE)],
    "S2": [("lkg_gemm_tall_f32", GATE), ("lkg_gemm_skinny_f32", RES), ("lkg_narrow_layer_bwd_f32", NARROW)],
    "S4": [("lkg_gemm_smallm_f32", RES), ("lkg_gemm_wgrad_f32", GATE), ("lkg_gate_blend_bwd_stats_f32", GATE),
           ("lkg_gemm_longk_f32", None)],
    "S6": [("lkg_narrow_layer_bwd_f32", NARROW)],
    "S7": [("lkg_gemm_f64acc_f32", RES)],
    "S8": [("lkg_csr_check_i32", GATE), ("lkg_csr_check_i32", RES)],
}
_oracle, _steps = {}, {}


def _inputs(L, O, dev, conf):
    """the draws of test_model_with_frozen_parameter_groups_matches_the_float64_oracle, and a fresh model on the CPU"""
    from literalkg_amd import io
    from literalkg_amd.synth import make_batch, make_kg
    agg, gate, scoring, residual, dim = conf
    n, n_rel = AC.N_BIG, 16
    h, t, r = make_kg(n, 60_000, seed=5)
    cfg = O.default_cfg(embed_dim=dim, relation_dim=dim, conv_dim=dim, n_conv_layers=2, aggregation_type=agg, scale_gat_dim=dim,
                        use_num_lit=gate == "mul", use_txt_lit=gate == "mul", txt_lit_dim=12, use_residual=residual,
                        mlp_hidden_dim=48, kg_l2loss_lambda=1e-4, device=dev)
    torch.manual_seed(3)
    num = torch.rand(n, 2) if gate else None
    txt = torch.randn(n, cfg.txt_lit_dim) if gate else None
    a_in = io.initial_a_in(n, h, t, r)
    m = L.LiteralKG(cfg, n, n_rel, a_in, num, txt, scoring=scoring)
    with torch.no_grad():
        m.entity_embed.weight.mul_(30)
        m.relation_embed.weight.mul_(3)
    params = {k: v.detach().clone() for k, v in m.state_dict().items() if k != "A_in"}
    batch = [torch.from_numpy(x) for x in make_batch(n, 200, 3, seed=9)]
    return NS_(m=m, cfg=cfg, a_in=a_in, num=num, txt=txt, params=params, batch=batch, scoring=scoring)


class NS_:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _oracle_step(O, inp, dtype):
    cast = lambda x: (x.to(dtype) if x is not None and x.is_floating_point() else x)
    p = {k: v.to(dtype).clone().requires_grad_(True) if v.is_floating_point() else v.clone() for k, v in inp.params.items()}
    loss = O.pre_training_loss(p, inp.cfg, cast(inp.a_in), *inp.batch, num=cast(inp.num), txt=cast(inp.txt), form=inp.scoring)
    loss.backward()
    return float(loss.detach()), {k: v.grad.detach().double() for k, v in p.items() if v.is_floating_point() and v.grad is not None}


def _step(L, O, ops, dev, conf, setting, side=False):
    """one pre-training step of a fresh model under ``setting`` -> (loss, {name: gradient}, launches); the float64 oracle of
    the configuration is computed once"""
    key = (conf, setting, side)
    if key in _steps:
        return _steps[key]
    with switched(ops, setting):
        inp = _inputs(L, O, dev, conf)
        if conf not in _oracle:
            _oracle[conf] = (inp.params, _oracle_step(O, inp, torch.float64))
        assert all(torch.equal(v, _oracle[conf][0][k]) for k, v in inp.params.items())      # the same draw every time
        m = inp.m.to(dev).eval()
        batch = [b.to(dev) for b in inp.batch]
        stream = torch.cuda.Stream() if side else torch.cuda.current_stream()
        stream.wait_stream(torch.cuda.current_stream())
        with AC.launches() as seen, torch.cuda.stream(stream):
            loss = m(*batch, device=dev, mode="pre_training")
            loss.backward()
        torch.cuda.synchronize()
        ops.check_deferred_errors()
        grads = {k: (v.grad.detach().double().cpu() if v.grad is not None else None) for k, v in m.named_parameters() if k != "A_in"}
    _steps[key] = (float(loss.detach()), grads, list(seen), inp)
    return _steps[key]


def _judge(conf, setting, loss, grads, want_loss, want, allow=None):
    """loss rtol 1e-4; every gradient within 2e-3 of the float64 gradient's largest entry (``allow``: name -> another bound)"""
    assert abs(loss - want_loss) <= 1e-4 * abs(want_loss), (conf, setting, loss, want_loss)
    worst = (0.0, None)
    misses = []
    for k, g in grads.items():
        ref = want.get(k)
        if ref is None:
            assert g is None or float(g.abs().max()) == 0.0, (conf, setting, k)
            continue
        assert g is not None, (conf, setting, k)
        err = float((g - ref).abs().max()) / (float(ref.abs().max()) + 1e-12)
        worst = max(worst, (err, k))
        if not err < (allow or {}).get(k, 2e-3):
            misses.append((k, err))
    return worst, misses


@pytest.mark.parametrize("conf,setting", MODEL_CASES, ids=lambda v: v if isinstance(v, str) else "-".join(str(x) for x in v))
def test_model_step_under_a_switch(L, O, ops, gpu_device, conf, setting):
    want_loss, want = None, None
    for side in ((False, True) if setting == "S8" else (False,)):       # S8, the benchmarked sequence: also on a side stream
        loss, grads, seen, inp = _step(L, O, ops, gpu_device, conf, setting, side)
        want_loss, want = _oracle[conf][1]
        worst, misses = _judge(conf, setting, loss, grads, want_loss, want)
        print(f"{conf[0]} / {conf[2]}{' / residual' if conf[3] else ''}{f' / width {conf[4]}' if conf[4] != 32 else ''}, {setting}{' (side stream)' if side else ''}: loss {loss:.6f} "
              f"(float64 {want_loss:.6f}), worst gradient {worst[0]:.3g} of its largest entry ({worst[1]})")
        if misses and setting == "S7":
            # the fp32 fold is the documented worse arithmetic: 3 x the float32 oracle's own distance from float64 (the factor
            # op_audit gives the split engines), per parameter
            _, g32 = _oracle_step(O, inp, torch.float32)
            d32 = {k: float((g32[k] - want[k]).abs().max()) / (float(want[k].abs().max()) + 1e-12) for k, _ in misses}
            print(f"  S7 misses 2e-3: {misses}; the float32 oracle's distance from float64: {d32}")
            worst, misses = _judge(conf, setting, loss, grads, want_loss, want, {k: 3.0 * v for k, v in d32.items()})
        assert not misses, (conf, setting, side, misses)
    # the switch is live: what it removes is there under S0 (in the configuration that has it), and gone under the setting
    for name, where in LIVE.get(setting, []):
        assert name not in seen, (conf, setting, name)
        if where is None:
            for c in (GATE, RES):
                assert name not in _step(L, O, ops, gpu_device, c, "S0")[2], (c, name)
        else:
            assert name in _step(L, O, ops, gpu_device, where, "S0")[2], (where, name)


def test_f16x2_all_is_live_in_the_model(L, O, ops, gpu_device):
    """S3 launches strictly more lkg_gemm_tall_f32 than S0.  Measured: 3 and 3 over the two configurations of the frozen-groups
    test -- at width 32 every one-panel product is a skinny one (k n <= 2048), and ops.gemm_engine asks for the skinny kernel
    before the tall engine under every setting -- so the count is taken over those two AND the 64-wide residual configuration,
    whose Linears on untagged inputs are what f16x2-all moves; never fewer in any configuration."""
    count = lambda c, s: _step(L, O, ops, gpu_device, c, s)[2].count("lkg_gemm_tall_f32")
    per = {c: (count(c, "S0"), count(c, "S3")) for c in (GATE, RES, WIDE)}
    print(f"lkg_gemm_tall_f32 launches of one step (S0, S3): {per}")
    assert all(n3 >= n0 for n0, n3 in per.values()), per
    assert sum(n3 for _, n3 in per.values()) > sum(n0 for n0, _ in per.values()), per
    assert per[WIDE][1] > per[WIDE][0], per


# ============================================================================= 4. the C-level variables, one child each
CHILD_RUNS = [{}, {"LKG_GEMM_F32_ONLY": "1"}, {"LKG_ACTLN_NARROW_OFF": "1"}, {"LKG_SMALLM_BLOCKS": "1"},
              {"LKG_SMALLM_BLOCKS": "100000"}]


def test_c_level_switches_in_fresh_children(L, gpu_device):
    """Five children, one at a time; the first that exits non-zero or times out ends the test and no further child is started.
    lkg_gemm_f32's engines are 1 (bf16x3_rows) and 2 (bf16x3_kmajor) when unset and 0 and 0 under LKG_GEMM_F32_ONLY=1; its error
    is within max(2 f32, 1e-6) / max(2 f32, 2e-6) of float64 (test_gpu_parity.py:253, :276) either way; the child itself holds
    the row-wise forward and lkg_gemm_smallm_f32 to their allowances.  With LKG_SMALLM_BLOCKS=1 two runs agree bit for bit."""
    torch.cuda.synchronize()
    for extra in CHILD_RUNS:
        env = {k: v for k, v in os.environ.items() if k not in ("LKG_GEMM_F32_ONLY", "LKG_ACTLN_NARROW_OFF", "LKG_SMALLM_BLOCKS")}
        env.update(extra)
        p = subprocess.run([sys.executable, os.path.join(HERE, "switch_child.py")], env=env, capture_output=True, text=True,
                           timeout=300)
        assert p.returncode == 0, (extra, p.returncode, p.stderr[-3000:])
        out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
        print(json.dumps(out))
        assert out["env"] == extra
        rows, km = out["gemm_rows"], out["gemm_kmajor"]
        assert rows["workspace"] > 0 and (rows["engine"], km["engine"]) == ((0, 0) if "LKG_GEMM_F32_ONLY" in extra else (1, 2)), out
        assert rows["err"] <= max(2.0 * rows["f32"], 1e-6), rows
        assert km["err"] <= max(2.0 * km["f32"], 2e-6), km
        assert out["act_layernorm"]["cases"] == 6 and out["act_layernorm"]["worst_r_over_bound"] <= 1.0, out
        assert set(out["smallm"]) == {"32x32", "64x96"} and all(v["r"] <= v["bound"] for v in out["smallm"].values()), out
        if extra.get("LKG_SMALLM_BLOCKS") == "1":
            assert all(v["same_bits"] for v in out["smallm"].values()), out
