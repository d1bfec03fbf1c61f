"""One entry per torch.autograd.Function of literalkg_amd/ops.py: the inputs of each branch its backward can take, the
call through the public wrapper, and the same function restated in plain torch ops (differentiable by torch's own
autograd, usable in float64).  Shared by test_autograd_surface_host.py (on the CPU: the registry is complete, every
restatement is pinned by gradcheck, the comparator rejects planted faults) and test_autograd_surface_gpu.py (the
Functions on the device under every subset of inputs that require a gradient and every subset of outputs that are used).

This file is about STRUCTURE -- which gradient is produced, in which slot, by which launches -- not about conditioning:
the draws are the benign seeded ones of the direct tests (test_gpu_parity.py), and the float64 references are those of
op_audit.py / softmax_cases.py / softmax_filtered_cases.py wherever one exists.

An entry:

  params            forward's parameters classified: "diff" (a differentiable slot), "none" (a tensor that never gets a
                    gradient: named in by_design_none with the line that says so) or "config" (not a tensor / an id list)
  variants          the names of the shapes; build(device, variant, small, seed) draws one (small: a few rows, for the CPU)
  apply(ops, inp)   {output name: tensor} through the public wrapper
  restate(inp, dt)  the same in torch ops on inp.t's tensors (already of dtype dt)
  named(inp)        the named subsets of a Function with more than 4 slots (input_subsets adds singletons and complements)
  same_launches(inp, subset)   are the gradients the subset asks for produced by the launches of the all-trainable run, on
                    the same operands?
  deterministic(inp)           the slots whose producing kernels add in a fixed order (no float atomics): with
                    same_launches their gradient carries the bits of the all-trainable run
  expect(inp, subset, outs)    {(phase, entry point): True | False | count}: launches of the forward ("fwd") / backward
                    ("bwd") pass that must be present / absent / that many; ("pool", name): a _RowScratch pool that must
                    (not) have been drawn from during the backward
  scratch(inp)      does the backward go through _RowScratch?

Measure (judge64): largest absolute error over the largest absolute entry of the float64 gradient -- the measure of the
existing direct tests -- against the entry's ``bound``; ("close", rtol, atol) is torch.testing.assert_close at the
tolerances of test_gpu_parity.test_triple_losses.  ELTWISE is for the Functions whose backward is one element-wise
kernel: at most 5 roundings per element (op_audit.eltwise_ref / bi_mix_bwd_ref count them) of terms whose |.|-sum is at
most 3 x the largest entry on these draws: 16 units of 2^-24."""
import contextlib
import inspect
import itertools
from types import SimpleNamespace as NS

import numpy as np
import torch

import op_audit as A
import softmax_cases as S
import softmax_filtered_cases as SF

ELTWISE = A.units(16)
PRODUCT = 1e-4                 # test_gpu_parity.py: narrow layer (line 489), fused gate (515), fused layer
LOSS = ("close", 1e-3, 1e-6)   # test_gpu_parity.test_triple_losses
ATOMIC_SUMS = 5e-5             # test_gpu_parity.py:2422: two runs of the float-atomic column sums of act_layernorm's backward
N_BIG = 16387                  # one past TALL_MIN_ROWS + 2: tall products, rows_worth_compacting with 600 listed rows
N_TAGGED = 600
REGISTRY = {}


# ----------------------------------------------------------------------------- inputs
class Inputs:
    """t: name -> tensor (the differentiable slots, the by-design-none tensors, id lists); cfg: everything else;
    upstream: output name -> the fixed gradient handed to torch.autograd.backward; rows: output name -> the int64 ids
    outside which that gradient is zero (two outputs that share one id tensor share one RowSet)."""

    def __init__(self, variant, slots, outputs, t, cfg=None, upstream=None, rows=None):
        self.variant, self.slots, self.outputs = variant, list(slots), list(outputs)
        self.t, self.cfg, self.upstream, self.rows = dict(t), dict(cfg or {}), dict(upstream or {}), dict(rows or {})

    def leaves(self, subset, dtype=torch.float32, also=()):
        """fresh copies: floating tensors in ``dtype``, the slots of ``subset`` (and ``also``) requiring a gradient"""
        t = {}
        for k, v in self.t.items():
            if torch.is_tensor(v) and v.is_floating_point():
                t[k] = v.detach().clone().to(dtype).requires_grad_(k in subset or k in also)
            else:
                t[k] = v
        return Inputs(self.variant, self.slots, self.outputs, t, self.cfg, self.upstream, self.rows)

    def to(self, device):
        moved = {}

        def mv(v):                      # (one copy per tensor object: outputs that share an id list keep sharing it)
            if not torch.is_tensor(v):
                return v
            if id(v) not in moved:
                moved[id(v)] = v.to(device)
            return moved[id(v)]
        return Inputs(self.variant, self.slots, self.outputs, {k: mv(v) for k, v in self.t.items()}, self.cfg,
                      {k: mv(v) for k, v in self.upstream.items()}, {k: mv(v) for k, v in self.rows.items()})


class Entry:
    def __init__(self, name, params, variants, build, apply, restate, bound, by_design_none=None, named=None,
                 same_launches=None, deterministic=None, expect=None, scratch=None, judge=None, vs_base=None):
        self.name, self.params, self.variants = name, params, tuple(variants)
        self.build, self.apply, self.restate, self.bound = build, apply, restate, bound
        self.by_design_none = dict(by_design_none or {})
        self.named = named or (lambda inp: [])
        self.same_launches = same_launches or (lambda inp, subset: True)
        self.deterministic = deterministic or (lambda inp: set())
        self.expect = expect or (lambda inp, subset, outs: {})
        self.scratch = scratch or (lambda inp: False)
        self.judge = judge                      # (ops, inp, slot, got, want64, ref32) -> message or None, instead of judge64
        self.vs_base = vs_base                  # slot -> bound on the distance from the all-trainable run (dropout variants)
        REGISTRY[name] = self


def functions(ops):
    """every torch.autograd.Function subclass defined in ops.py, by introspection"""
    return {n: c for n, c in vars(ops).items()
            if inspect.isclass(c) and issubclass(c, torch.autograd.Function) and c.__module__ == ops.__name__}


def forward_params(cls):
    """forward's parameters after ctx; a *name for the varargs"""
    out = []
    for p in list(inspect.signature(cls.forward).parameters.values())[1:]:
        out.append("*" + p.name if p.kind is inspect.Parameter.VAR_POSITIONAL else p.name)
    return out


# ----------------------------------------------------------------------------- the enumerators
def input_subsets(entry, inp):
    """frozensets of slot names: with at most 4 slots every non-empty subset; with more each slot alone, each slot alone
    frozen, the entry's named subsets and all of them together"""
    slots = inp.slots
    if len(slots) <= 4:
        out = [frozenset(c) for r in range(1, len(slots) + 1) for c in itertools.combinations(slots, r)]
    else:
        out = [frozenset([s]) for s in slots] + [frozenset(slots) - {s} for s in slots]
        out += [frozenset(s) for s in entry.named(inp)] + [frozenset(slots)]
    seen, res = set(), []
    for s in out:
        if s and s not in seen:
            seen.add(s)
            res.append(s)
    return res


def output_subsets(entry, inp):
    """every non-empty subset of the outputs (the unused ones are not passed to torch.autograd.backward)"""
    o = inp.outputs
    return [tuple(c) for r in range(len(o), 0, -1) for c in itertools.combinations(o, r)]


# ----------------------------------------------------------------------------- running and judging
def backward(res, upstream, outs, dtype=None):
    outs = [o for o in outs if res.get(o) is not None and res[o].requires_grad]     # (a restated output no trainable leaf reaches)
    if outs:
        torch.autograd.backward([res[o] for o in outs],
                                [upstream[o] if dtype is None else upstream[o].to(dtype) for o in outs])


def restated_grads(entry, inp, subset, outs, dtype):
    """{slot: gradient or None} of torch's own autograd of the restatement, with exactly ``subset`` requiring a gradient"""
    lv = inp.leaves(subset, dtype)
    backward(entry.restate(lv, dtype), lv.upstream, outs, dtype)
    return {s: lv.t[s].grad for s in lv.slots}


def norm_measure(got, want64):
    """largest absolute error over the largest absolute entry of the float64 gradient"""
    if want64.numel() == 0:
        return 0.0
    d = (got.detach().double().cpu() - want64.detach().double().cpu()).abs().max()
    d = float(torch.nan_to_num(d, nan=float("inf")))
    return d / (float(want64.detach().abs().max()) + 1e-20)


def judge64(bound, got, want64):
    """None when got meets the bound against want64, else what is wrong"""
    if isinstance(bound, tuple):
        try:
            torch.testing.assert_close(got.detach().double().cpu(), want64.detach().double().cpu(), rtol=bound[1], atol=bound[2])
        except AssertionError as e:
            return str(e).replace("\n", " ")
        return None
    r = norm_measure(got, want64)
    return None if r <= bound else f"error {r:.3g} of the largest entry > {bound:.3g}"


def compare(inp, subset, got, want64, bound, judge=None):
    """The comparator of the matrix: ``got`` {slot: gradient or None} of a run in which exactly ``subset`` required a
    gradient, against ``want64`` {slot: float64 gradient or None} of the all-trainable restatement (None altogether: the
    structure alone).  Returns the list of faults: a slot asked for without a gradient, or with one of the wrong shape /
    dtype, or off by more than the bound; a slot not asked for that has one.  (A slot no used output depends on has no
    float64 gradient: None and exact zeros both pass.)"""
    faults = []
    for s in inp.slots:
        g = got.get(s)
        if s in subset:
            w = want64.get(s) if want64 is not None else None
            if g is None:
                if want64 is None or w is not None:
                    faults.append(f"{s}: asked for, no gradient")
            elif tuple(g.shape) != tuple(inp.t[s].shape) or g.dtype != inp.t[s].dtype:
                faults.append(f"{s}: gradient of shape {tuple(g.shape)} / {g.dtype} for an input of {tuple(inp.t[s].shape)} / "
                              f"{inp.t[s].dtype}")
            elif want64 is not None:
                if w is None:
                    bad = None if not bool(g.detach().ne(0).any()) else "no used output depends on it, yet its gradient is not zero"
                else:
                    bad = judge(s, g, w) if judge is not None else judge64(bound, g, w)
                if bad:
                    faults.append(f"{s}: {bad}")
        elif g is not None:
            faults.append(f"{s}: not asked for, yet it has a gradient")
    return faults


@contextlib.contextmanager
def launches():
    """the C entry points _native.call launches inside the block, in order (test_invariance_gpu.recorded keeps a set)"""
    from literalkg_amd import _native
    real, seen = _native.call, []

    def call(name, *args):
        seen.append(name)
        return real(name, *args)
    _native.call = call
    try:
        yield seen
    finally:
        _native.call = real


def n_products(seen):
    return sum(1 for n in seen if n.startswith("lkg_gemm"))


@contextlib.contextmanager
def pools_drawn(ops):
    """the pools _RowScratch.acquire is asked for inside the block (ops None: a stand-in without the package)"""
    seen = []
    if ops is None:
        yield seen
        return
    real = ops._RowScratch.acquire

    def acquire(n, c, device, pool="loss"):
        seen.append(pool)
        return real(n, c, device, pool)
    ops._RowScratch.acquire = staticmethod(acquire)
    try:
        yield seen
    finally:
        ops._RowScratch.acquire = classmethod(real.__func__)


def upstream_for(ops, inp, outs):
    """fresh copies of the fixed upstream gradients, tagged with their row sets (outputs that share an id list share the
    RowSet object, as two gradients that came down one path do)"""
    up, sets = {}, {}
    for o in outs:
        g = inp.upstream[o].clone()
        ids = inp.rows.get(o)
        if ids is not None:
            if id(ids) not in sets:
                flags = torch.zeros(g.shape[0], dtype=torch.uint8, device=g.device)
                flags[ids] = 1
                sets[id(ids)] = ops.RowSet(flags, [ids])
            assert ops.rows_worth_compacting(sets[id(ids)], g.shape[0])
            ops.tag_rows(g, sets[id(ids)])
        if inp.cfg.get("tag_rowmax"):
            ops.tag_rowmax(g, ops.row_absmax(g))
        up[o] = g
    return up


def applied(entry, ops, inp, subset, outs, also=()):
    """one step through the Function with exactly ``subset`` (and ``also``) requiring a gradient ->
    NS(grads {slot: clone or None}, fwd, bwd [launches], pools [drawn in the backward], leaves)"""
    lv = inp.leaves(subset, torch.float32, also)
    up = upstream_for(ops, lv, outs)
    with launches() as fwd:
        res = entry.apply(ops, lv)
    with launches() as bwd, pools_drawn(ops) as pools:
        backward(res, up, outs)
    grads = {s: (lv.t[s].grad.detach().clone() if lv.t[s].grad is not None else None) for s in lv.slots}
    return NS(grads=grads, fwd=fwd, bwd=bwd, pools=pools, leaves=lv)


def check_expect(exp, run):
    faults = []
    for (phase, name), want in exp.items():
        seen = {"fwd": run.fwd, "bwd": run.bwd, "pool": run.pools}[phase]
        if name == "exactly":
            if list(seen) != list(want):
                faults.append(f"{phase}: launched {seen}, expected exactly {want}")
            continue
        n = n_products(seen) if name == "products" else len(seen) if name == "launches" else seen.count(name)
        ok = (n > 0) == want if isinstance(want, bool) else n == want
        if not ok:
            faults.append(f"{phase} {name}: {n} launched, expected {'some' if want is True else 'none' if want is False else want}"
                          f" (all: {seen})")
    return faults


def same_bits_fault(a, b, what):
    import invariance as V
    try:
        V.same_bits(a, b, what)
    except AssertionError as e:
        return str(e)
    return None


def run_matrix(entry, ops, inp, measures=None, expect=None):
    """Every input subset x output subset of one Function variant, judged by structure, launch record, bits and float64
    (module docstring of test_autograd_surface_gpu.py).  Returns the list of faults, each named by its subsets.
    measures: {entry name: [all-trainable, worst partial, torch float32]} is updated with the largest figures seen.
    expect: (inp, subset, outs) -> launch expectations that REPLACE the entry's own -- those of another setting of the engine
    switches (test_engine_switches_gpu.py); the bit comparison against the all-trainable run, which rests on the default
    launches (same_launches), is then left out.  None: the entry's own, and every judge."""
    faults = []
    default_launches = expect is None
    expect = entry.expect if expect is None else expect
    allset = frozenset(inp.slots)
    dropout = inp.cfg.get("drop_p", 0.0) > 0
    det = entry.deterministic(inp)
    also = [k for k in entry.by_design_none if torch.is_tensor(inp.t.get(k)) and inp.t[k].is_floating_point()]
    m = measures.setdefault(entry.name, [0.0, 0.0, 0.0]) if measures is not None else [0.0, 0.0, 0.0]
    for outs in output_subsets(entry, inp):
        tag = f"{entry.name} [{inp.variant}] outputs {'+'.join(outs)}"
        want64 = ref32 = judge = None
        if not dropout:
            want64 = restated_grads(entry, inp, allset, outs, torch.float64)
            ref32 = restated_grads(entry, inp, allset, outs, torch.float32)
            if entry.judge is not None:
                judge = lambda s, g, w: entry.judge(ops, inp, s, g, w, ref32[s])
            for s in inp.slots:
                if want64[s] is not None:
                    m[2] = max(m[2], norm_measure(ref32[s], want64[s]))
        base = applied(entry, ops, inp, allset, outs, also)
        for k in also:              # by design no gradient, even when it requires one
            if base.leaves.t[k].requires_grad and base.leaves.t[k].grad is not None:
                faults.append(f"{tag}: {k} never gets a gradient ({entry.by_design_none[k]}), yet it has one")
        first = compare(inp, allset, base.grads, want64, entry.bound, judge) + check_expect(expect(inp, allset, outs), base)
        if first:                   # the all-trainable run first: a partial-gradient failure is then not one of the measure
            faults += [f"{tag}, all trainable: {f}" for f in first]
            continue
        if want64 is not None:
            m[0] = max([m[0]] + [norm_measure(base.grads[s], want64[s]) for s in inp.slots if want64[s] is not None])
        for subset in input_subsets(entry, inp):
            if subset == allset:
                continue
            run = applied(entry, ops, inp, subset, outs)
            here = compare(inp, subset, run.grads, want64, entry.bound, judge) + check_expect(expect(inp, subset, outs), run)
            for s in sorted(subset):
                g, b = run.grads[s], base.grads[s]
                if g is None or b is None:
                    continue
                if want64 is not None and want64[s] is not None:
                    m[1] = max(m[1], norm_measure(g, want64[s]))
                if default_launches and s in det and entry.same_launches(inp, subset):
                    bad = same_bits_fault(g, b, f"{s} against the all-trainable run")
                    if bad:
                        here.append(bad)
                elif dropout:
                    r = norm_measure(g, b.double())
                    if r > entry.vs_base(s):
                        here.append(f"{s}: {r:.3g} from the all-trainable run with the same seed > {entry.vs_base(s):.3g}")
            faults += [f"{tag}, trainable {{{', '.join(sorted(subset))}}}: {f}" for f in here]
    return faults


def scratch_check(entry, ops, device, variant, reset):
    """A partial-gradient step, then -- same process, same stream -- an all-trainable step on other ids (seed 1: ids that occur
    once, so every table row is one add onto zero): the second step's table-shaped gradients must carry the bits of the
    same step run first after reset() (a fresh scratch registry), and every gradient must meet float64.  A table handed to
    autograd for a frozen input is dropped unconsumed: it has to come back clean."""
    first, second = entry.build(device, variant, seed=0), entry.build(device, variant, seed=1)
    allset, outs = frozenset(second.slots), tuple(second.outputs)
    reset()
    fresh = applied(entry, ops, second, allset, outs)
    want64 = restated_grads(entry, second, allset, outs, torch.float64)
    faults = [f"{entry.name} [{variant}] second step alone: {f}" for f in compare(second, allset, fresh.grads, want64, entry.bound)]
    n_rows = max(second.t[s].shape[0] for s in second.slots if second.t[s].dim() == 2)
    for subset in input_subsets(entry, first):
        reset()
        applied(entry, ops, first, subset, tuple(first.outputs))
        again = applied(entry, ops, second, allset, outs)
        here = compare(second, allset, again.grads, want64, entry.bound)
        for s in second.slots:
            if second.t[s].dim() == 2 and second.t[s].shape[0] == n_rows and again.grads[s] is not None:
                bad = same_bits_fault(again.grads[s], fresh.grads[s], f"{s} of the second step")
                if bad:
                    here.append(bad)
        faults += [f"{entry.name} [{variant}] after a step with trainable {{{', '.join(sorted(subset))}}}: {f}" for f in here]
    return faults


# ----------------------------------------------------------------------------- draws
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rn(gen, *shape, std=1.0):
    return torch.randn(*shape, generator=gen) * std


def _rows(n, small):
    return 5 if small else n


def tagged_upstream(gen, n, d, n_ids=N_TAGGED, unique=False):
    """(ids with repeats, a gradient that is zero outside them)"""
    k = min(n_ids, max(1, n // 2))
    ids = torch.randperm(n, generator=gen)[:k] if unique else torch.randint(0, n, (k,), generator=gen)
    g = torch.zeros(n, d)
    u = torch.unique(ids)
    g[u] = _rn(gen, u.numel(), d)
    return ids, g


_graphs = {}


def graph(device, small):
    """(n, rowptr, col [int32, on device], KGStructure or None): synth.make_kg(16 387, 60 000) on the device, a 7-row graph
    in plain numpy on the CPU (the host tier needs no library)"""
    key = (str(device), small)
    if key not in _graphs:
        if small:
            import rowwise_cases as RC
            n = 7
            rng = np.random.default_rng(5)
            h, t = rng.integers(0, n, 18), rng.integers(0, n, 18)
            c = RC.csr_of(n, h, t, np.zeros_like(h), device)
            _graphs[key] = (n, c.rowptr, c.col, None)
        else:
            from literalkg_amd.graph import KGStructure
            from literalkg_amd.synth import make_kg
            h, t, r = make_kg(N_BIG, 60_000, seed=11)
            g = KGStructure.from_triples(N_BIG, h, t, r, device=device)
            _graphs[key] = (N_BIG, g.rowptr, g.col, g)
    return _graphs[key]


# ============================================================================= the entries
# ----------------------------------------------------------------------------- _MultiLinear
ML = {"257x20->24": (257, (20,), 24), "16387x(32,2,12)->32": (N_BIG, (32, 2, 12), 32), "4099x32->32 skinny": (4099, (32,), 32),
      "16387x(32,2,12)->32 tagged": (N_BIG, (32, 2, 12), 32)}


def _ml_build(device, variant, small=False, seed=0):
    n, ks, d = ML[variant]
    n = _rows(n, small)
    gen = _gen(100 + seed + len(variant))
    t = {"bias": _rn(gen, d, std=0.1)}
    for i, k in enumerate(ks):
        t[f"x{i}"] = _rn(gen, n, k, std=0.7)
    for i, k in enumerate(ks):
        t[f"w{i}"] = _rn(gen, d, k, std=0.2)
    rows = {}
    if "tagged" in variant:
        ids, gy = tagged_upstream(gen, n, d, unique=seed > 0)
        rows = {"y": ids}
    else:
        gy = _rn(gen, n, d)
    return Inputs(variant, list(t), ["y"], t, dict(n_terms=len(ks), tag_rowmax=variant == "16387x(32,2,12)->32"),
                  {"y": gy}, rows).to(device)


def _ml_apply(ops, inp):
    n = inp.cfg["n_terms"]
    xs, ws = [inp.t[f"x{i}"] for i in range(n)], [inp.t[f"w{i}"] for i in range(n)]
    return {"y": ops.linear(xs[0], ws[0], inp.t["bias"]) if n == 1 else ops.multi_linear(xs, ws, inp.t["bias"])}


def _ml_restate(inp, dtype):
    n = inp.cfg["n_terms"]
    return {"y": sum(inp.t[f"x{i}"] @ inp.t[f"w{i}"].t() for i in range(n)) + inp.t["bias"]}


def _ml_expect(inp, subset, outs):
    v = inp.variant
    if v == "257x20->24":
        return {("fwd", "lkg_gemm_f32"): True}
    if v == "4099x32->32 skinny":
        return {("fwd", "lkg_gemm_skinny_f32"): True}
    if "tagged" in v:
        return {("fwd", "lkg_gemm_tall_f32"): True, ("bwd", "lkg_gather_rows_range_f32"): True,
                ("bwd", "lkg_scatter_add_rows_range_f32"): sum(1 for s in subset if s[0] == "x"),
                ("bwd", "lkg_colsum_weighted_f32"): False, ("bwd", "lkg_gemm_tall_f32"): False}
    # the 2-wide panel: its data gradient is the tall product (the 32- and 12-wide ones go to the skinny kernel), its weight
    # gradient carries the bias sum; with it frozen the bias sum is lkg_colsum_f32's
    return {("fwd", "lkg_gemm_tall_f32"): True, ("bwd", "lkg_gemm_tall_f32"): "x1" in subset,
            ("bwd", "lkg_colsum_weighted_f32"): "w1" in subset,
            ("bwd", "lkg_colsum_f32"): "bias" in subset and "w1" not in subset}


Entry("_MultiLinear", {"bias": "diff", "n_terms": "config", "*xw": "diff"}, ML, _ml_build, _ml_apply, _ml_restate, PRODUCT,
      named=lambda inp: [[s for s in inp.slots if s[0] == "w"], [s for s in inp.slots if s[0] == "x"], ["bias", "w1"],
                         ["bias", "w0", "w2"], ["bias", "x1"]] if len(inp.slots) > 4 else [],
      same_launches=lambda inp, subset: not ("bias" in subset and "w1" in inp.slots and "w1" not in subset),
      expect=_ml_expect, scratch=lambda inp: "tagged" in inp.variant)


# ----------------------------------------------------------------------------- _StackedLinear
def _sl_build(device, variant, small=False, seed=0):
    n = _rows(N_BIG, small)
    gen = _gen(200 + seed)
    widths = (32, 32, 16)
    t = {"x": _rn(gen, n, 32, std=0.7)}
    for i, wd in enumerate(widths):
        t[f"w{i}"] = _rn(gen, wd, 32, std=0.2)
    for i, wd in enumerate(widths):
        t[f"b{i}"] = _rn(gen, wd, std=0.1)
    up = {f"y{i}": _rn(gen, n, wd) for i, wd in enumerate(widths)}
    return Inputs(variant, list(t), list(up), t, {}, up).to(device)


def _sl_apply(ops, inp):
    ys = ops.stacked_linear(inp.t["x"], [inp.t[f"w{i}"] for i in range(3)], [inp.t[f"b{i}"] for i in range(3)])
    return {f"y{i}": y for i, y in enumerate(ys)}


def _sl_expect(inp, subset, outs):
    return {("bwd", "products"): int("x" in subset) + int(any(s[0] == "w" for s in subset)),
            ("bwd", "lkg_colsum_f32"): int(any(s[0] == "b" for s in subset))}


Entry("_StackedLinear", {"x": "diff", "n_lin": "config", "*wb": "diff"}, ["16387x32->(32,32,16)"], _sl_build, _sl_apply,
      lambda inp, dtype: {f"y{i}": inp.t["x"] @ inp.t[f"w{i}"].t() + inp.t[f"b{i}"] for i in range(3)}, PRODUCT,
      named=lambda inp: [["w0", "w1", "w2"], ["b0", "b1", "b2"], ["x", "b1"], ["w2", "b0"]], expect=_sl_expect)


# ----------------------------------------------------------------------------- _MatMul, _FoldNT
def _mm_build(device, variant, small=False, seed=0):
    gen = _gen(300 + seed)
    m = _rows(300, small)
    t = {"a": _rn(gen, m, 40, std=0.7), "b": _rn(gen, 40, 24, std=0.2)}
    return Inputs(variant, ["a", "b"], ["c"], t, {}, {"c": _rn(gen, m, 24)}).to(device)


Entry("_MatMul", {"a": "diff", "b": "diff"}, ["300x40@40x24"], _mm_build, lambda ops, inp: {"c": ops.matmul(inp.t["a"], inp.t["b"])},
      lambda inp, dtype: {"c": inp.t["a"] @ inp.t["b"]}, PRODUCT,
      expect=lambda inp, subset, outs: {("bwd", "products"): len(subset)})


def _fold_build(device, variant, small=False, seed=0):
    gen = _gen(310 + seed)
    t = {"a": _rn(gen, 8, 6, std=0.7), "b": _rn(gen, 5, 6, std=0.2)}
    return Inputs(variant, ["a", "b"], ["c"], t, {}, {"c": _rn(gen, 8, 5)}).to(device)


# (one float32 rounding of a float64 sum: op_audit's gemm_f64acc allowance is 2^-24 of the entry; 2 units of the largest)
def _fold_apply(ops, inp):
    assert ops.FOLD_F64
    return {"c": ops.fold_nt(inp.t["a"], inp.t["b"])}


Entry("_FoldNT", {"a": "diff", "b": "diff"}, ["8x6"], _fold_build, _fold_apply,
      lambda inp, dtype: {"c": inp.t["a"] @ inp.t["b"].t()}, A.units(2),
      deterministic=lambda inp: {"a", "b"},
      expect=lambda inp, subset, outs: {("bwd", "lkg_gemm_f64acc_f32"): len(subset)})


# ----------------------------------------------------------------------------- _Axpby, _Mul, _LeakySum
def _elt_build(device, variant, small=False, seed=0):
    tagged = "tagged" in variant
    n, d = (_rows(N_BIG, small), 32) if tagged else (_rows(257, small), 20)
    gen = _gen(400 + seed + len(variant))
    t = {"a": _rn(gen, n, d)}
    if "one" not in variant and "a only" not in variant:
        t["b"] = _rn(gen, n, d)
    rows = {}
    if tagged:
        ids, g = tagged_upstream(gen, n, d, unique=seed > 0)
        rows = {"y": ids}
    else:
        g = _rn(gen, n, d)
    return Inputs(variant, list(t), ["y"], t, dict(alpha=0.75, beta=-1.25, slope=0.01), {"y": g}, rows).to(device)


def _dense_elt(inp, subset, outs):
    return {("bwd", "lkg_eltwise_f32"): len(subset)}


Entry("_Axpby", {"a": "diff", "b": "diff", "alpha": "config", "beta": "config"}, ["257x20", "257x20 a only"], _elt_build,
      lambda ops, inp: {"y": ops.axpby(inp.t["a"], inp.t.get("b"), inp.cfg["alpha"], inp.cfg["beta"])},
      lambda inp, dtype: {"y": inp.cfg["alpha"] * inp.t["a"] + (inp.cfg["beta"] * inp.t["b"] if "b" in inp.t else inp.cfg["beta"])},
      ELTWISE, deterministic=lambda inp: set(inp.slots), expect=_dense_elt)

Entry("_Mul", {"a": "diff", "b": "diff"}, ["257x20"], _elt_build, lambda ops, inp: {"y": ops.mul(inp.t["a"], inp.t["b"])},
      lambda inp, dtype: {"y": inp.t["a"] * inp.t["b"]}, ELTWISE, deterministic=lambda inp: set(inp.slots), expect=_dense_elt)


def _leaky_expect(inp, subset, outs):
    if "tagged" not in inp.variant:
        return _dense_elt(inp, subset, outs)
    return {("bwd", "lkg_gather_rows_range_f32"): 1 + len(subset), ("bwd", "lkg_scatter_add_rows_range_f32"): len(subset),
            ("bwd", "lkg_eltwise_f32"): len(subset)}


Entry("_LeakySum", {"a": "diff", "b": "diff", "slope": "config"},
      ["257x20 one", "257x20 two", "16387x32 tagged one", "16387x32 tagged two"], _elt_build,
      lambda ops, inp: {"y": (ops.leaky_relu_sum(inp.t["a"], inp.t["b"], inp.cfg["slope"]) if "b" in inp.t
                              else ops.leaky_relu(inp.t["a"], inp.cfg["slope"]))},
      lambda inp, dtype: {"y": A.leaky(inp.t["a"], inp.cfg["slope"]) + (A.leaky(inp.t["b"], inp.cfg["slope"]) if "b" in inp.t else 0.0)},
      ELTWISE, deterministic=lambda inp: set(inp.slots), expect=_leaky_expect, scratch=lambda inp: "tagged" in inp.variant)


# ----------------------------------------------------------------------------- _BiMix
def _bimix_build(device, variant, small=False, seed=0):
    n, d = _rows(257, small), 32
    gen = _gen(500 + seed + len(variant))
    t = {"ego": _rn(gen, n, d), "side": _rn(gen, n, d)}
    if variant == "257x32 h0p":
        t["h0p"] = _rn(gen, n, d)
    up = {"sum": _rn(gen, n, d), "prod": _rn(gen, n, d)}
    return Inputs(variant, list(t), ["sum", "prod"], t, dict(alpha=0.3 if "h0p" in t else 0.0), up).to(device)


def _bimix_restate(inp, dtype):
    r = A.bi_mix_fwd_ref(inp.t["ego"], inp.t["side"], inp.t.get("h0p"), inp.cfg["alpha"])
    return {"sum": r["sum"][0], "prod": r["prod"][0]}


Entry("_BiMix", {"ego": "diff", "side": "diff", "h0p": "diff", "alpha": "config"}, ["257x32", "257x32 h0p"], _bimix_build,
      lambda ops, inp: dict(zip(("sum", "prod"), ops.bi_mix(inp.t["ego"], inp.t["side"], inp.t.get("h0p"), inp.cfg["alpha"]))),
      _bimix_restate, ELTWISE, deterministic=lambda inp: set(inp.slots),
      expect=lambda inp, subset, outs: {("bwd", "lkg_bi_mix_bwd_f32"): 1})


# ----------------------------------------------------------------------------- _ActLayerNorm, _NarrowLayer, _FusedLayer
LN_CFG = dict(slope=0.01, eps=1e-5, norm_eps=1e-12)


def _ln_params(gen, d):
    return {"gamma": 1 + 0.1 * _rn(gen, d), "beta": 0.1 * _rn(gen, d)}


def _ln_out(inp, z, dtype):
    r = A.layernorm_fwd_eval(z, inp.t["gamma"], inp.t["beta"], LN_CFG["slope"], LN_CFG["eps"], LN_CFG["norm_eps"], dtype)
    return {k: r[k] for k in inp.outputs}


def _aln_build(device, variant, small=False, seed=0):
    n = _rows(4099 if variant.startswith("4099") else 257, small)
    gen = _gen(600 + seed + len(variant))
    t = {"z": _rn(gen, n, 32, std=0.7), **_ln_params(gen, 32)}
    outs = ["yn"] if "yn only" in variant else ["y", "yn"]
    up = {o: _rn(gen, n, 32) for o in outs}
    return Inputs(variant, list(t), outs, t, dict(drop_p=0.25 if "drop" in variant else 0.0, seed=99, want_y="y" in outs), up).to(device)


def _aln_apply(ops, inp):
    y, yn = ops.act_layernorm(inp.t["z"], inp.t["gamma"], inp.t["beta"], drop_p=inp.cfg["drop_p"], seed=inp.cfg["seed"],
                              want_y=inp.cfg["want_y"])
    return {"y": y, "yn": yn}


Entry("_ActLayerNorm", {"z": "diff", "gamma": "diff", "beta": "diff", "want_norm": "config", "slope": "config", "eps": "config",
                        "norm_eps": "config", "drop_p": "config", "seed": "config", "yn_out": "none", "want_y": "config"},
      ["257x32", "4099x32", "257x32 yn only", "257x32 drop 0.25"], _aln_build, _aln_apply,
      lambda inp, dtype: _ln_out(inp, inp.t["z"], dtype), PRODUCT,
      by_design_none={"yn_out": "a destination: 'yn_out: a column slice of the concat buffer (CatBuffer), written in place' "
                                "(ops.py, _ActLayerNorm.forward; the reference's torch.cat, model.py:309)"},
      deterministic=lambda inp: {"z"},         # (g_gamma / g_beta: float atomics, test_gpu_parity.py:2422)
      vs_base=lambda slot: ATOMIC_SUMS, expect=lambda inp, subset, outs: {("bwd", "lkg_act_layernorm_bwd_f32"): 1})


def _nl_build(device, variant, small=False, seed=0):
    n = _rows(4103, small)
    gen = _gen(700 + seed + len(variant))
    t = {"x": _rn(gen, n, 32, std=0.7), "w": _rn(gen, 32, 32, std=0.2)}
    if "no bias" not in variant:
        t["bias"] = _rn(gen, 32, std=0.1)
    t.update(_ln_params(gen, 32))
    up = {"y": _rn(gen, n, 32), "yn": _rn(gen, n, 32)}
    return Inputs(variant, list(t), ["y", "yn"], t, dict(drop_p=0.25 if "drop" in variant else 0.0, seed=99), up).to(device)


def _nl_apply(ops, inp):
    assert ops.narrow_layer_ok(inp.t["x"], inp.t["w"])
    y, yn = ops.narrow_layer(inp.t["x"], inp.t["w"], inp.t.get("bias"), inp.t["gamma"], inp.t["beta"], drop_p=inp.cfg["drop_p"],
                             seed=inp.cfg["seed"])
    return {"y": y, "yn": yn}


def _nl_fused(subset):
    return "x" in subset and "w" in subset


Entry("_NarrowLayer", {"x": "diff", "w": "diff", "bias": "diff", "gamma": "diff", "beta": "diff", "want_norm": "config",
                       "slope": "config", "eps": "config", "norm_eps": "config", "drop_p": "config", "seed": "config",
                       "yn_out": "none", "want_y": "config"},
      ["4103x32 bias", "4103x32 no bias", "4103x32 bias drop 0.25"], _nl_build, _nl_apply,
      lambda inp, dtype: _ln_out(inp, inp.t["x"] @ inp.t["w"].t() + (inp.t["bias"] if "bias" in inp.t else 0.0), dtype), PRODUCT,
      by_design_none={"yn_out": "a destination, as _ActLayerNorm's (ops.py, _NarrowLayer.forward; model.py:309)"},
      named=lambda inp: [["x", "w"], ["x", "w", "bias"], ["gamma", "beta"], ["x", "gamma", "beta"]],
      same_launches=lambda inp, subset: _nl_fused(subset),
      deterministic=lambda inp: set(inp.slots),      # (the one-launch backward adds its sums in a fixed order: test_gpu_parity.py:479)
      vs_base=lambda slot: 2e-6 if slot == "x" else 2e-5,      # (one launch against the unfused passes: test_gpu_parity.py:458)
      expect=lambda inp, subset, outs: {("bwd", "lkg_narrow_layer_bwd_f32"): _nl_fused(subset),
                                        ("bwd", "lkg_act_layernorm_bwd_f32"): not _nl_fused(subset)})


def _fl_build(device, variant, small=False, seed=0):
    n, ks, d = _rows(N_BIG, small), (32, 8), 48
    gen = _gen(800 + seed + len(variant))
    t = {"bias": _rn(gen, d, std=0.1), **_ln_params(gen, d)}
    for i, k in enumerate(ks):
        t[f"x{i}"] = _rn(gen, n, k, std=0.7)
    for i, k in enumerate(ks):
        t[f"w{i}"] = _rn(gen, d, k, std=0.2)
    rows = {}
    if "tagged" in variant:
        ids, gy = tagged_upstream(gen, n, d, unique=seed > 0)
        gyn = torch.zeros(n, d)
        u = torch.unique(ids)
        gyn[u] = _rn(gen, u.numel(), d)
        rows = {"y": ids, "yn": ids}
    else:
        gy, gyn = _rn(gen, n, d), _rn(gen, n, d)
    return Inputs(variant, list(t), ["y", "yn"], t, {}, {"y": gy, "yn": gyn}, rows).to(device)


def _fl_apply(ops, inp):
    xs, ws = [inp.t["x0"], inp.t["x1"]], [inp.t["w0"], inp.t["w1"]]
    assert ops.fused_layer_ok(xs[0].shape[0], ws[0].shape[0], [x.shape[1] for x in xs])
    y, yn = ops.linear_act_layernorm(xs, ws, inp.t["bias"], inp.t["gamma"], inp.t["beta"])
    return {"y": y, "yn": yn}


def _fl_expect(inp, subset, outs):
    if "tagged" in inp.variant:       # z on the listed rows, then the unfused pair's backward on them
        return {("fwd", "lkg_linear_act_layernorm_fwd_f32"): 1, ("bwd", "lkg_gemm_tall_f32"): False,
                ("bwd", "lkg_gather_rows_range_f32"): True, ("bwd", "lkg_act_layernorm_bwd_f32"): 1}
    return {("fwd", "lkg_linear_act_layernorm_fwd_f32"): 1, ("bwd", "lkg_gemm_tall_f32"): 1, ("bwd", "lkg_act_layernorm_bwd_f32"): 1,
            ("bwd", "lkg_colsum_weighted_f32"): "w1" in subset}


Entry("_FusedLayer", {"bias": "diff", "gamma": "diff", "beta": "diff", "n_terms": "config", "slope": "config", "eps": "config",
                      "norm_eps": "config", "drop_p": "config", "seed": "config", "yn_out": "none", "want_y": "config",
                      "want_norm": "config", "*xw": "diff"},
      ["16387x(32,8)->48", "16387x(32,8)->48 tagged"], _fl_build, _fl_apply,
      lambda inp, dtype: _ln_out(inp, inp.t["x0"] @ inp.t["w0"].t() + inp.t["x1"] @ inp.t["w1"].t() + inp.t["bias"], dtype), PRODUCT,
      by_design_none={"yn_out": "a destination, as _ActLayerNorm's (ops.py, linear_act_layernorm_fwd; model.py:309)"},
      named=lambda inp: [["x0", "x1"], ["w0", "w1"], ["bias", "w1"], ["bias", "w0"], ["gamma", "beta"], ["x0", "w0"]],
      expect=_fl_expect, scratch=lambda inp: "tagged" in inp.variant)


# ----------------------------------------------------------------------------- _GateBlend, _FusedGate
def _gb_build(device, variant, small=False, seed=0):
    n, d = _rows(257, small), 32
    gen = _gen(900 + seed)
    t = {"x": _rn(gen, n, d, std=0.5), "gpre": _rn(gen, n, d), "zpre": _rn(gen, n, d)}
    return Inputs(variant, list(t), ["out"], t, {}, {"out": _rn(gen, n, d)}).to(device)


Entry("_GateBlend", {"x": "diff", "gpre": "diff", "zpre": "diff", "out": "none"}, ["257x32"], _gb_build,
      lambda ops, inp: {"out": ops.gate_blend(inp.t["x"], inp.t["gpre"], inp.t["zpre"])},
      lambda inp, dtype: {"out": A.gate_blend_fwd_ref(inp.t["x"], inp.t["gpre"], inp.t["zpre"])[0]}, PRODUCT,
      by_design_none={"out": "a destination: the gate writes into a column slot of the concatenated table (model.py:300-309)"},
      deterministic=lambda inp: set(inp.slots), expect=lambda inp, subset, outs: {("bwd", "lkg_gate_blend_bwd_f32"): 1})

FG = {"16387xd32 lits (2,12)": (2, 12), "16387xd32 lit (5)": (5,), "16387xd32 lits (2,12) tagged": (2, 12),
      "16387xd32 lit (5) tagged": (5,),
      # the dense backward WITHOUT the blend kernel's statistics (ops.py, _FusedGate.backward): a width that is no multiple of
      # 4, and two literal panels of <= 4 columns that both want a weight gradient
      "16387xd30 lits (2,12)": (2, 12), "16387xd32 lits (2,3)": (2, 3)}


def fg_width(variant):
    return int(variant.split("xd")[1].split()[0])


def _fg_build(device, variant, small=False, seed=0):
    n, d, ks = _rows(N_BIG, small), fg_width(variant), FG[variant]
    gen = _gen(1000 + seed + len(variant))
    t = {"x": _rn(gen, n, d, std=0.5)}
    for i, k in enumerate(ks):
        t[f"lit{i}"] = torch.rand(n, k, generator=gen) if i == 0 and len(ks) > 1 else _rn(gen, n, k)
    for name in ("wg", "wz"):
        for i, k in enumerate((d,) + ks):
            t[f"{name}{i}"] = _rn(gen, d, k, std=0.2)
    t["bg"], t["bz"] = _rn(gen, d, std=0.1), _rn(gen, d, std=0.1)
    rows = {}
    if "tagged" in variant:
        ids, go = tagged_upstream(gen, n, d, unique=seed > 0)
        rows = {"out": ids}
    else:
        go = _rn(gen, n, d)
    return Inputs(variant, list(t), ["out"], t, dict(n_lit=len(ks)), {"out": go}, rows).to(device)


def _fg_apply(ops, inp):
    nl = inp.cfg["n_lit"]
    lits = [inp.t[f"lit{i}"] for i in range(nl)]
    assert ops.gate_fusable(inp.t["x"], lits, inp.t["x"].shape[1])
    return {"out": ops.fused_gate(inp.t["x"], lits, [inp.t[f"wg{i}"] for i in range(nl + 1)],
                                  [inp.t[f"wz{i}"] for i in range(nl + 1)], inp.t["bg"], inp.t["bz"])}


def _fg_restate(inp, dtype):
    nl = inp.cfg["n_lit"]
    panels = [inp.t["x"]] + [inp.t[f"lit{i}"] for i in range(nl)]
    gpre = sum(p @ inp.t[f"wg{i}"].t() for i, p in enumerate(panels)) + inp.t["bg"]
    zpre = sum(p @ inp.t[f"wz{i}"].t() for i, p in enumerate(panels)) + inp.t["bz"]
    return {"out": A.gate_blend_fwd_ref(inp.t["x"], gpre, zpre)[0]}


def fg_lits(inp):
    return [s for s in inp.slots if s.startswith("lit")]


def fg_model_subset(inp):
    """the model's case: everything but the literal tables"""
    return frozenset(inp.slots) - set(fg_lits(inp))


def fg_no_stats(inp, subset):
    """Does the dense backward of this subset run without the blend kernel's statistics?  (ops.py, _FusedGate.backward: they
    need a width that is a multiple of 4 and carry the weight gradient of at most ONE literal panel of <= 4 columns)"""
    nl = inp.cfg["n_lit"]
    narrow = [i for i in range(nl) if (f"wg{i + 1}" in subset or f"wz{i + 1}" in subset) and inp.t[f"lit{i}"].shape[1] <= 4]
    return "tagged" not in inp.variant and (inp.t["x"].shape[1] % 4 != 0 or len(narrow) > 1)


def _fg_expect(inp, subset, outs):
    nl = inp.cfg["n_lit"]
    want = [f"wg{i}" in subset or f"wz{i}" in subset for i in range(nl + 1)]       # a panel's [2d x k] product: either half wanted
    n_lits = sum(1 for s in fg_lits(inp) if s in subset)
    if "tagged" in inp.variant:
        return {("bwd", "lkg_gate_blend_bwd_stats_f32"): False, ("bwd", "lkg_gate_blend_bwd_f32"): 1,
                ("bwd", "lkg_gemm_tall_f32"): False, ("pool", "g_gate_x"): "x" in subset,
                ("bwd", "lkg_colsum_f32"): int("bg" in subset or "bz" in subset),
                ("bwd", "products"): 2 * int("x" in subset) + sum(want) + n_lits,
                ("bwd", "lkg_scatter_add_rows_range_f32"): int("x" in subset) + n_lits}
    widths = [inp.t["x"].shape[1]] + [inp.t[f"lit{i}"].shape[1] for i in range(nl)]
    if fg_no_stats(inp, subset):
        # the blend kernel without its statistics, the data gradient still ONE tall product; the bias sums and the weight
        # gradients are ops.weight_grads': every wanted panel of <= 8 columns one lkg_colsum_weighted_f32 (the first carries the
        # bias sums; lkg_colsum_f32 when there is none), every wider one a product through ops.gemm
        want_bias = "bg" in subset or "bz" in subset
        n_narrow = sum(1 for i in range(nl + 1) if want[i] and widths[i] <= 8)
        return {("bwd", "lkg_gate_blend_bwd_f32"): 1, ("bwd", "lkg_gate_blend_bwd_stats_f32"): False,
                ("bwd", "lkg_gemm_wgrad_f32"): False, ("bwd", "lkg_gemm_tall_f32"): int("x" in subset),
                ("bwd", "lkg_colsum_weighted_f32"): n_narrow, ("bwd", "lkg_colsum_f32"): int(want_bias and n_narrow == 0),
                ("bwd", "products"): int("x" in subset) + sum(1 for i in range(nl + 1) if want[i] and widths[i] > 8) + n_lits}
    # the statistics of the blend kernel carry the bias sums and the weight gradient of the one literal panel of <= 4 columns:
    # neither a column sum nor a product is launched for them; every other wanted panel is one fp16 weight-gradient product
    wide =[i for i in range(nl + 1) if i == 0 or inp.t[f"lit{i - 1}"].shape[1] > 4]
    n_wgrad = sum(1 for i in wide if want[i])
    e = {("bwd", "lkg_gate_blend_bwd_stats_f32"): 1, ("bwd", "lkg_gate_blend_bwd_f32"): False,
         ("bwd", "lkg_gemm_tall_f32"): int("x" in subset), ("bwd", "lkg_gemm_wgrad_f32"): n_wgrad,
         ("bwd", "lkg_colsum_f32"): 0, ("bwd", "lkg_colsum_weighted_f32"): 0,
         ("bwd", "products"): int("x" in subset) + n_wgrad + n_lits}
    if subset == fg_model_subset(inp):
        # the launches of the backward before the literal tables could get a gradient: the blend kernel with its statistics
        # (bias sums, the 2-wide panel's weight gradient, the column maxima), the tall data gradient, one fp16 weight-gradient
        # product per remaining panel -- unchanged
        e[("bwd", "exactly")] = ["lkg_gate_blend_bwd_stats_f32", "lkg_gemm_tall_f32", "lkg_gemm_wgrad_f32", "lkg_gemm_wgrad_f32"]
    return e


Entry("_FusedGate", {"out": "none", "bg": "diff", "bz": "diff", "n_lit": "config", "grad_mode": "config", "x": "diff", "*rest": "diff"},
      FG, _fg_build, _fg_apply, _fg_restate, PRODUCT,
      by_design_none={"out": "a destination: 'the result written straight into ``out`` (a column slot of the concatenated "
                             "table)' (ops.py, _FusedGate; model.py:300-309)"},
      named=lambda inp: [[s for s in inp.slots if s.startswith("wg")], [s for s in inp.slots if s.startswith("wz")], ["bg", "bz"],
                         fg_lits(inp), fg_model_subset(inp), ["x"] + fg_lits(inp), ["wg1", "wz1"], ["wg0"], ["bz", "wz0"]],
      expect=_fg_expect, scratch=lambda inp: "tagged" in inp.variant)


# ----------------------------------------------------------------------------- _Aggregate, _AggregateKeep
AGG = [f"{'bias' if b else 'no bias'}{' +self' if s else ''}{' tagged' if t else ''}" for b in (1, 0) for s in (0, 1) for t in (0, 1)]


def _agg_build(device, variant, small=False, seed=0):
    n, rowptr, col, g = graph(device, small)
    gen = _gen(1100 + seed + len(variant))
    d = 32
    nnz = int(col.numel())
    t = {"ego": _rn(gen, n, d, std=0.7), "val": torch.rand(nnz, generator=gen)}
    if variant.startswith("bias"):
        t["bias"] = _rn(gen, d, std=0.1)
    rows = {}
    if "tagged" in variant:
        ids, go = tagged_upstream(gen, n, d, unique=seed > 0)
        rows = {"side": ids}
    else:
        go = _rn(gen, n, d)
    inp = Inputs(variant, [s for s in t if s != "val"], ["side"], t, dict(plus_self="+self" in variant, g=g, n=n),
                 {"side": go}, rows).to(device)
    inp.t.update(rowptr=rowptr, col=col)
    return inp


def _agg_apply(ops, inp):
    g = inp.cfg["g"]
    val_t = ops.permute_values(inp.t["val"].detach(), g.t_perm).requires_grad_(inp.t["val"].requires_grad)
    inp.t["val_t"] = val_t
    return {"side": ops.aggregate(inp.t["ego"], g, inp.t["val"], val_t, inp.cfg["plus_self"], inp.t.get("bias"))}


def _agg_restate(inp, dtype):
    ego = inp.t["ego"]
    return {"side": A.spmm_eval(inp.t["rowptr"], inp.t["col"], inp.t["val"].detach(), ego, inp.cfg["n"], dtype,
                                add_self=ego if inp.cfg["plus_self"] else None, bias=inp.t.get("bias"))}


def _agg_expect(inp, subset, outs):
    tagged = "tagged" in inp.variant
    e = {("bwd", "lkg_spmm_csr_fused_f32"): 1, ("pool", "g_agg"): tagged}
    if "bias" in inp.slots:
        e[("bwd", "lkg_colsum_f32")] = int("bias" in subset)
        e[("bwd", "lkg_gather_rows_range_f32")] = int(tagged and "bias" in subset)
    return e


A_NONE = {"val": "'A carries no gradient' (ops.py, _Aggregate; model.py:261: the attention values are refreshed under no_grad)",
          "val_t": "the same values in CSC order (model.py:261)"}
Entry("_Aggregate", {"ego": "diff", "g": "config", "val": "none", "val_t": "none", "plus_self": "config", "bias": "diff"}, AGG,
      _agg_build, _agg_apply, _agg_restate, PRODUCT, by_design_none=A_NONE, expect=_agg_expect,
      scratch=lambda inp: "tagged" in inp.variant)

AGK = [f"{'slot' if k else 'no keep_dst'}{' +self' if s else ''}{' tagged' if t else ''}" for k in (0, 1) for s in (0, 1) for t in (0, 1)]


def _agk_build(device, variant, small=False, seed=0):
    inp = _agg_build(device, "no " + variant, small, seed)          # (no bias)
    inp.variant, inp.outputs = variant, ["side", "kept"]
    gen = _gen(1200 + seed + len(variant))
    n, d = inp.t["ego"].shape
    if "tagged" in variant:
        ids = inp.rows["side"]
        gk = torch.zeros(n, d)
        u = torch.unique(ids.cpu())
        gk[u] = _rn(gen, u.numel(), d)
        inp.rows["kept"] = ids
    else:
        gk = _rn(gen, n, d)
    inp.upstream["kept"] = gk.to(device)
    inp.cfg["slot"] = variant.startswith("slot")
    return inp


def _agk_apply(ops, inp):
    g = inp.cfg["g"]
    ego = inp.t["ego"].view_as(inp.t["ego"])       # (not a leaf: the frontier form is for a table a gate's backward follows)
    val_t = ops.permute_values(inp.t["val"].detach(), g.t_perm).requires_grad_(inp.t["val"].requires_grad)
    inp.t["val_t"] = val_t
    keep_dst = None
    if inp.cfg["slot"]:
        keep_dst = torch.zeros((ego.shape[0], 3 * ego.shape[1]), dtype=torch.float32, device=ego.device)[:, 32:64]
    side, kept = ops.aggregate_keep(ego, g, inp.t["val"], val_t, inp.cfg["plus_self"], keep_dst)
    assert torch.equal(kept.detach(), inp.t["ego"].detach())
    return {"side": side, "kept": kept}


def _agk_expect(inp, subset, outs):
    return {("bwd", "lkg_spmm_csr_fused_f32"): int("side" in outs), ("pool", "g_agg_keep"): "tagged" in inp.variant and "side" in outs}


Entry("_AggregateKeep", {"ego": "diff", "g": "config", "val": "none", "val_t": "none", "plus_self": "config", "keep_dst": "none"}, AGK,
      _agk_build, _agk_apply, lambda inp, dtype: {**_agg_restate(inp, dtype), "kept": inp.t["ego"] * 1.0}, PRODUCT,
      by_design_none={**A_NONE, "keep_dst": "a destination: column slot 0 of the concatenated table (model.py:300-309)"},
      expect=_agk_expect, scratch=lambda inp: "tagged" in inp.variant)


# ----------------------------------------------------------------------------- _Fanout, _AssembleCat
def _fan_build(device, variant, small=False, seed=0):
    n, d = _rows(N_BIG, small), 80
    gen = _gen(1300 + seed + len(variant))
    t = {"x": _rn(gen, n, d)}
    if "tagged" in variant:
        (ia, ga), (ib, gb) = (tagged_upstream(gen, n, d, unique=seed > 0) for _ in range(2))
        rows = {"a": ia, "b": ib}
    else:
        ga, gb, rows = _rn(gen, n, d), _rn(gen, n, d), {}
    return Inputs(variant, ["x"], ["a", "b"], t, {}, {"a": ga, "b": gb}, rows).to(device)


def _fan_expect(inp, subset, outs):
    both = len(outs) == 2
    if "tagged" in inp.variant:
        return {("pool", "g_fanout"): both, ("bwd", "lkg_scatter_add_rows_range_f32"): 2 * both, ("bwd", "lkg_eltwise_f32"): 0}
    return {("bwd", "lkg_eltwise_f32"): int(both), ("bwd", "launches"): int(both)}      # one gradient: handed through


Entry("_Fanout", {"x": "diff"}, ["16387x80", "16387x80 tagged"], _fan_build,
      lambda ops, inp: dict(zip("ab", ops.fanout(inp.t["x"]))), lambda inp, dtype: {"a": inp.t["x"] * 1.0, "b": inp.t["x"] * 1.0},
      ELTWISE, deterministic=lambda inp: {"x"}, same_launches=lambda inp, subset: True, expect=_fan_expect,
      scratch=lambda inp: "tagged" in inp.variant)


def _cat_build(device, variant, small=False, seed=0):
    n = _rows(N_BIG, small)
    gen = _gen(1400 + seed)
    t = {f"p{i}": _rn(gen, n, w) for i, w in enumerate((32, 32, 16))}
    return Inputs(variant, list(t), ["table"], t, {}, {"table": _rn(gen, n, 80)}).to(device)


def _cat_apply(ops, inp):
    parts = [inp.t[f"p{i}"] for i in range(3)]
    holder = ops.CatBuffer(parts[0].shape[0], [p.shape[1] for p in parts], parts[0].device)
    out = ops.assemble_cat(holder, parts)
    assert torch.equal(out.detach(), torch.cat([p.detach() for p in parts], 1))
    return {"table": out}


Entry("_AssembleCat", {"holder": "config", "pending": "config", "*parts": "diff"}, ["16387x(32+32+16)"], _cat_build, _cat_apply,
      lambda inp, dtype: {"table": torch.cat([inp.t[f"p{i}"] for i in range(3)], 1)}, 0.0,
      deterministic=lambda inp: set(inp.slots), expect=lambda inp, subset, outs: {("bwd", "launches"): 0})


# ----------------------------------------------------------------------------- the losses
def _loss_build(kind):
    def build(device, variant, small=False, seed=0):
        n, c, n_rel = (_rows(N_BIG, small) + (20 if small else 0)), 32, 16
        group = 7 if "group 7" in variant else 1
        b = (14 if group == 7 else 6) if small else 203
        dout = 24 if kind == "transr" else c
        if small:
            c, dout, n_rel = 4, (3 if kind == "transr" else 4), 3
        gen = _gen(1500 + seed + len(variant) + len(kind))
        t = {"emb": _rn(gen, n, c, std=0.4)}
        if kind != "dot":
            t["relemb"] = _rn(gen, n_rel, dout, std=0.4)
        if kind == "transr":
            t["trans_m"] = _rn(gen, n_rel, c, dout, std=0.2)
        n_g = b // group
        if seed > 0:            # the second step of the scratch check: ids that occur once (every table row gets one add)
            perm = torch.randperm(n, generator=gen)
            h, pt, nt = perm[:n_g], perm[n_g:2 * n_g], perm[2 * n_g:2 * n_g + b]
        else:
            h, pt, nt = (torch.randint(0, n, (k,), generator=gen) for k in (n_g, n_g, b))
        r = torch.randint(0, n_rel - 1, (n_g,), generator=gen)       # (the last relation never occurs: an empty group)
        h, pt, r = (v.repeat_interleave(group) for v in (h, pt, r))
        t.update(h=h, r=r, pt=pt, nt=nt)
        cfg = dict(lam=1e-3, group=group, sparse="sparse" in variant, w0=0)
        if "slot0" in variant:
            cfg["w0"] = 8 if not small else 2
            t["slot0"] = t["emb"][:, :cfg["w0"]].clone()      # (the pending columns of emb hold what slot0 holds)
        slots = [s for s in ("emb", "relemb", "trans_m") if s in t]
        return Inputs(variant, slots, ["loss"], t, cfg, {"loss": torch.tensor(1.7)}).to(device)
    return build


def _loss_apply(kind):
    def apply(ops, inp):
        t, c = inp.t, inp.cfg
        if kind == "transe":
            return {"loss": ops.transe_loss(t["emb"], t["relemb"], t["h"], t["r"], t["pt"], t["nt"], c["lam"], None, c["sparse"])}
        if kind == "dot":
            return {"loss": ops.dot_loss(t["emb"], t["h"], t["pt"], t["nt"], c["lam"], c["sparse"])}
        return {"loss": ops.transr_loss(t["emb"], t["relemb"], t["trans_m"], t["h"], t["r"], t["pt"], t["nt"], c["lam"], None,
                                        c["group"], c["sparse"], t.get("slot0"))}
    return apply


def _loss_restate(kind):
    def restate(inp, dtype):
        t, lam = inp.t, inp.cfg["lam"]
        eh, ep, en = t["emb"][t["h"]], t["emb"][t["pt"]], t["emb"][t["nt"]]
        if kind == "dot":
            s, _ = A.dot_scores_eval(eh, ep, en, dtype)
            margin = s["pos"] - s["neg"]
        else:
            if kind == "transr":
                w_r = t["trans_m"][t["r"]]
                eh, ep, en = (torch.bmm(v.unsqueeze(1), w_r).squeeze(1) for v in (eh, ep, en))
            s, _ = A.trans_scores_eval(eh, t["relemb"][t["r"]], ep, en, dtype)
            margin = s["neg"] - s["pos"]
        return {"loss": A.loss_eval(A.rank_eval(margin, dtype)[0], s["reg"], lam, dtype)[0]}
    return restate


def _loss_expect(inp, subset, outs):
    return {("pool", "loss"): inp.cfg["sparse"]}


L_CFG = {"h": "config", "r": "config", "pt": "config", "nt": "config", "lam": "config", "keep": "config", "sparse_rows": "config"}
Entry("_TransELoss", {"emb": "diff", "relemb": "diff", **L_CFG}, ["dense", "sparse_rows"], _loss_build("transe"), _loss_apply("transe"),
      _loss_restate("transe"), LOSS, expect=_loss_expect, scratch=lambda inp: inp.cfg["sparse"])
Entry("_TransRLoss", {"emb": "diff", "relemb": "diff", "trans_m": "diff", **{k: v for k, v in L_CFG.items() if k != "sparse_rows"},
                      "group": "config", "sparse_rows": "config", "slot0": "none"},
      ["group 1", "group 1 sparse_rows", "group 7", "group 7 sparse_rows", "group 1 slot0"], _loss_build("transr"),
      _loss_apply("transr"), _loss_restate("transr"), LOSS,
      by_design_none={"slot0": "detached by the wrapper: 'slot0.detach() if slot0 is not None' (ops.py, transr_loss): its gradient "
                               "arrives through emb's first columns (the raw entity table is slot 0 of the concatenated table, "
                               "model.py:300-309)"},
      expect=_loss_expect, scratch=lambda inp: inp.cfg["sparse"])
Entry("_DotLoss", {"emb": "diff", **{k: v for k, v in L_CFG.items() if k not in ("r", "keep")}}, ["dense", "sparse_rows"],
      _loss_build("dot"), _loss_apply("dot"), _loss_restate("dot"), LOSS, expect=_loss_expect, scratch=lambda inp: inp.cfg["sparse"])


# ----------------------------------------------------------------------------- _GatherPair
def _gp_build(device, variant, small=False, seed=0):
    n, d = _rows(N_BIG, small) + (4 if small else 0), 32 if not small else 3
    k = 4 if small else 300
    gen = _gen(1600 + seed + len(variant))
    t = {"table": _rn(gen, n, d)}
    if seed > 0:
        perm = torch.randperm(n, generator=gen)
        t["ids_a"], t["ids_b"] = perm[:k], perm[k:2 * k]
    else:
        t["ids_a"], t["ids_b"] = torch.randint(0, n, (k,), generator=gen), torch.randint(0, n // 8 + 1, (k,), generator=gen)
    return Inputs(variant, ["table"], ["a", "b"], t, dict(sparse="sparse" in variant), {"a": _rn(gen, k, d), "b": _rn(gen, k, d)}).to(device)


Entry("_GatherPair", {"table": "diff", "ids_a": "config", "ids_b": "config", "sparse_rows": "config"}, ["dense", "sparse_rows"],
      _gp_build, lambda ops, inp: dict(zip("ab", ops.gather_rows_pair(inp.t["table"], inp.t["ids_a"], inp.t["ids_b"], inp.cfg["sparse"]))),
      lambda inp, dtype: {"a": inp.t["table"][inp.t["ids_a"]], "b": inp.t["table"][inp.t["ids_b"]]}, ELTWISE,
      expect=lambda inp, subset, outs: {("bwd", "lkg_scatter_add_rows_f32"): len(outs), ("pool", "loss"): inp.cfg["sparse"]},
      scratch=lambda inp: inp.cfg["sparse"])


# ----------------------------------------------------------------------------- _ReluBatchNorm
def _bn_build(device, variant, small=False, seed=0):
    n, d = _rows(257, small), 65 if not small else 3
    gen = _gen(1700 + seed + len(variant))
    t = {"z": _rn(gen, n, d), "gamma": 1 + 0.1 * _rn(gen, d), "beta": 0.1 * _rn(gen, d), "running_mean": 0.1 * _rn(gen, d),
         "running_var": 1 + 0.5 * torch.rand(d, generator=gen)}
    return Inputs(variant, ["z", "gamma", "beta"], ["y"], t, dict(training=variant == "training", momentum=0.1, eps=1e-5),
                  {"y": _rn(gen, n, d)}).to(device)


def _bn_apply(ops, inp):
    t, c = inp.t, inp.cfg
    bn = NS(weight=t["gamma"], bias=t["beta"], running_mean=t["running_mean"], running_var=t["running_var"], training=c["training"],
            momentum=c["momentum"], eps=c["eps"], track_running_stats=True, num_batches_tracked=torch.zeros((), dtype=torch.int64))
    return {"y": ops.relu_batchnorm(t["z"], bn)}


Entry("_ReluBatchNorm", {"z": "diff", "gamma": "diff", "beta": "diff", "running_mean": "none", "running_var": "none",
                         "training": "config", "momentum": "config", "eps": "config"}, ["training", "eval"], _bn_build, _bn_apply,
      lambda inp, dtype: {"y": A.batchnorm_fwd_eval(inp.t["z"], inp.t["gamma"], inp.t["beta"], inp.t["running_mean"].detach(),
                                                    inp.t["running_var"].detach(), inp.cfg["training"], inp.cfg["momentum"],
                                                    inp.cfg["eps"], dtype)["y"]}, PRODUCT,
      by_design_none={"running_mean": "a buffer, not a parameter: nn.BatchNorm1d's running statistics (model.py:515-516)",
                      "running_var": "a buffer, as running_mean (model.py:515-516)"},
      expect=lambda inp, subset, outs: {("bwd", "lkg_relu_batchnorm_bwd_f32"): 1})


# ----------------------------------------------------------------------------- _SoftmaxAllLoss
SM = [f"k {k} {'distance' if dist else 'dot'}{' excluded' if ex else ''}" for k in (17, 32) for dist in (1, 0) for ex in (0, 1)]


def _sm_build(device, variant, small=False, seed=0):
    b, n = (4, 9) if small else (65, 257)
    k = 3 if small else int(variant.split()[1])
    q, p, truth, g = S.random_tables(b, n, k, 1800 + seed + len(variant))
    t = {"q": q, "p": p, "truth": truth}
    cfg = dict(distance="distance" in variant, scale=0.5, chunk_bytes=1, excluded="excluded" in variant)
    if cfg["excluded"]:
        excl = SF.patterns(b, n, truth, 7 + seed)
        t["mask"] = SF.mask_of(excl, n)
        t["xptr"], t["xcol"] = SF.to_lists(excl)
    return Inputs(variant, ["q", "p"], ["loss"], t, cfg, {"loss": g}).to(device)


def _sm_apply(ops, inp):
    t, c = inp.t, inp.cfg
    return {"loss": ops.softmax_all_loss(t["q"], t["p"], t["truth"], distance=c["distance"], scale=c["scale"], chunk_bytes=c["chunk_bytes"],
                                         exclude=(t["xptr"], t["xcol"]) if c["excluded"] else None)}


def _sm_restate(inp, dtype):
    t, c = inp.t, inp.cfg
    if c["excluded"]:
        return {"loss": SF.loss_eval(t["q"], t["p"], t["truth"], t["mask"], c["distance"], c["scale"], dtype)[2]}
    return {"loss": S.loss_eval(t["q"], t["p"], t["truth"], c["distance"], c["scale"], dtype)[2]}


def _sm_expect(inp, subset, outs):
    # 257 candidates in chunks of 256 (chunk_bytes = 1): two chunks; dQ one product per chunk (slices of 4096), dP one
    # per chunk -- onto [2 V^T Q | 2 colsum V] with the column of ones when there is a norm term and p needs a gradient
    return {("bwd", "products"): 2 * len(subset), ("bwd", "lkg_colsum_f32"): 0}


def _sm_judge(ops, inp, slot, got, want64, ref32):
    """per element over the |.|-sum of the closed form's terms, against the bound of the engine that ran the product
    (test_one_vs_all_gpu.test_gradients_against_float64)"""
    from test_one_vs_all_gpu import _engines
    t, c = inp.t, inp.cfg
    b, k = t["q"].shape
    n = t["p"].shape[0]
    args = (t["q"], t["p"], t["truth"], inp.upstream["loss"])
    ref = (SF.grads_eval(*args, t["mask"], c["distance"], c["scale"]) if c["excluded"]
           else S.grads_eval(*args, c["distance"], c["scale"]))
    e_q, e_p = _engines(ops, t["q"], t["p"], b, n, k, ops.softmax_chunk_width(b, n, c["chunk_bytes"]), c["distance"])
    key, engine, kk = ("dq", e_q, n) if slot == "q" else ("dp", e_p, b)
    r32 = S.worst(ref32, ref[key], ref[key + "_scale"])
    r, bound = S.worst(got, ref[key], ref[key + "_scale"]), S.gemm_bound(engine, r32, kk)
    return None if r <= bound else f"r {r:.3g} > {bound:.3g} [{engine}, torch32 {r32:.3g}]"


Entry("_SoftmaxAllLoss", {"q": "diff", "p": "diff", "truth": "config", "distance": "config", "scale": "config", "splits": "config",
                          "chunk_bytes": "config", "xptr": "config", "xcol": "config"}, SM, _sm_build, _sm_apply, _sm_restate,
      PRODUCT, deterministic=lambda inp: {"q", "p"}, expect=_sm_expect, judge=_sm_judge)
