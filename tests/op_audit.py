"""Componentwise accuracy of the device ops against float64, shared by test_conditioning_gpu.py (each engine on operands
chosen to break it) and test_op_audit_gpu.py (every product and reduction of a real model step, on the inputs the model
hands it).

The measure is per ELEMENT, never against the largest entry:

    r = |got - x64| / (|alpha| |A||B| + |beta| |C0| + |bias| + TINY)

x64 is float64 evaluated on the same float32 inputs, and an engine passes when  max r <= max(F * r_torch32, FLOOR)  with
r_torch32 the same measure of torch's float32 result on the device (``BOUNDS`` holds F and FLOOR per engine).  Reductions
divide by the column's sum of |x|."""
import contextlib
import inspect
import math
import sys
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import torch

TINY = 1e-300

# engine -> (F, FLOOR): the factor over torch's float32 error and the floor of the bound (those of the older engine tests).
# Engine names are ops.gemm_engine's (the engine ops.gemm dispatches on) plus the fixed-engine ops.
BOUNDS = {
    "tall_f16x2": (3.0, 5e-7),          # lkg_gemm_tall_f32 (products carry 2^-22), every tiling variant, every epilogue
    "wgrad_f16x2": (3.0, 5e-7),         # lkg_gemm_wgrad_f32 (both its kernels); plus the chain term below
    "longk": (3.0, 5e-7),               # lkg_gemm_longk_f32 (bf16 x 3)
    "bf16x3_rows": (3.0, 5e-7),         # lkg_gemm_f32's split engines (bf16 x 3)
    "bf16x3_kmajor": (3.0, 5e-7),
    "f32_mfma": (2.0, 3e-7),            # lkg_gemm_f32's f32-input MFMA engine; plus the chain term below
    "skinny": (2.0, 3e-7),              # lkg_gemm_skinny_f32 (VALU fmaf)
    "smallm": (2.0, 3e-7),              # lkg_gemm_smallm_f32 (VALU fmaf)
    "colsum": (3.0, 3e-7),              # lkg_colsum_f32 / lkg_colsum_weighted_f32, per column over sum |x|
}
BF16X3 = ("longk", "bf16x3_rows", "bf16x3_kmajor")
U = 2.0 ** -24


def chain_term(engine: str, k: int) -> float:
    """The stated K-dependent part of an engine's bound (lkg_gemm.hip / lkg_gemm_wgrad.hip headers): the
    f32-input MFMA adds the k products of an output in ONE k-ordered chain of k roundings, the f16 x 2 weight gradient in
    a chain of 3 MFMA roundings per 16 rows, and their rounding errors add up like a random walk over the chain:
    2 sqrt(chain) u of sum |a||b| (6 sigma when every partial sum is as large as the final one, i.e. same-sign terms);
    the weight gradient's split adds its one-signed 2^-22 per product (round-toward-zero mids).  torch's blocked
    reductions keep their chains short, so at long k these terms, not 2-3 x torch, are the engines' limit."""
    if engine == "f32_mfma":
        return 2.0 * math.sqrt(k) * U
    if engine == "wgrad_f16x2":
        return 2.0 ** -22 + 2.0 * math.sqrt(3 * math.ceil(k / 16)) * U
    return 0.0


def componentwise(got: torch.Tensor, want64: torch.Tensor, scale64: torch.Tensor):
    """(max r, flat index of the worst element) over the elements where the reference is finite."""
    fin = torch.isfinite(want64)
    r = (got.double() - want64).abs() / (scale64 + TINY)
    r = torch.where(fin, r, torch.zeros_like(r))
    r = torch.nan_to_num(r, nan=math.inf)
    i = int(r.argmax()) if r.numel() else 0
    return (float(r.reshape(-1)[i]) if r.numel() else 0.0), i


def bound_for(engine: str, r_torch32: float, k: int = 0) -> float:
    f, floor = BOUNDS[engine]
    return max(f * r_torch32, floor, chain_term(engine, k))


# ----------------------------------------------------------------------------------------------------- the audit
@dataclass
class Record:
    op: str
    site: str
    engine: str
    shape: tuple
    r: float
    bound: float
    worst: str
    hint: Optional[str] = None


@dataclass
class Audit:
    records: List[Record] = field(default_factory=list)
    calls: Dict[str, int] = field(default_factory=dict)
    failures: List[str] = field(default_factory=list)
    hint_notes: List[str] = field(default_factory=list)

    inner: Dict[str, int] = field(default_factory=dict)      # calls made from inside ops.py itself

    def fail(self, rec: Record, what: str):
        self.failures.append(f"{rec.op} at {rec.site} [{rec.engine}] shape {rec.shape}: {what}")


HINT_SLACK = 2.0        # a scale hint more than this far above the true maximum costs bits: reported (hint_notes)


def _site():
    """the first caller outside ops.py and this module"""
    for fr in inspect.stack()[2:]:
        fn = fr.filename
        if not (fn.endswith("ops.py") or fn.endswith("op_audit.py") or "torch" in fn.split("/")[-3:-1]):
            return f"{fn.split('/')[-1]}:{fr.lineno} {fr.function}"
    return "?"


def _ops_site():
    """the calling function inside the package (ops.py / model.py / gate.py ...), for the report"""
    for fr in inspect.stack()[2:]:
        fn = fr.filename
        if "literalkg_amd" in fn and not fn.endswith("op_audit.py"):
            return f"{fn.split('/')[-1]}:{fr.lineno} {fr.function}"
    return _site()


def _worst(got, want64, scale64, i):
    g = got.reshape(-1)[i].item()
    w = want64.reshape(-1)[i].item()
    s = scale64.reshape(-1)[i].item()
    return f"element {i}: got {g!r}, x64 {w!r}, scale {s!r}"


def _check_hint(audit: Audit, rec: Record, name: str, hint: Optional[torch.Tensor], true_max: torch.Tensor):
    if hint is None:
        return
    h, t = hint.double(), true_max.double()
    below = h < t
    if bool(below.any()):
        i = int(below.nonzero()[0])
        audit.fail(rec, f"scale hint {name}[{i}] = {h[i].item()!r} is below the true maximum {t[i].item()!r}")
    over = (h > HINT_SLACK * t) & (t > 0)
    if bool(over.any()):
        i = int(over.nonzero()[0])
        audit.hint_notes.append(f"{rec.op} at {rec.site}: {name} exceeds the true maximum {HINT_SLACK}x or more at "
                                f"{int(over.sum())} entries (first: {h[i].item()!r} vs {t[i].item()!r})")


def _measure(audit, rec, got, want64, scale64, ref32, k=0):
    r, i = componentwise(got, want64, scale64)
    r32, _ = componentwise(ref32, want64, scale64)
    rec.r = r
    rec.bound = bound_for(rec.engine, r32, k)
    rec.worst = _worst(got, want64, scale64, i)
    nonfinite = ~torch.isfinite(got) & torch.isfinite(want64)
    if bool(nonfinite.any()):
        audit.fail(rec, f"{int(nonfinite.sum())} non-finite outputs where float64 is finite")
    if r > rec.bound:
        audit.fail(rec, f"r = {r:.3g} > bound {rec.bound:.3g} (torch f32: {r32:.3g}); worst {rec.worst}")
    audit.records.append(rec)


@contextlib.contextmanager
def audit_ops(ops):
    """Wrap ops.gemm, gemm_tall, gemm_wgrad, colsum, narrow_weight_grad, gemm_f64acc and linear_act_layernorm_fwd: every
    call clones its inputs, runs the real op, and checks the result against float64 with the bound of the engine that
    ran and every scale hint against the true maximum.  Yields the Audit."""
    audit = Audit()
    real = {name: getattr(ops, name) for name in ("gemm", "gemm_tall", "gemm_wgrad", "colsum", "narrow_weight_grad",
                                                   "gemm_f64acc", "linear_act_layernorm_fwd")}
    depth = [0]

    def count(name):
        audit.calls[name] = audit.calls.get(name, 0) + 1
        if sys._getframe(2).f_code.co_filename == ops.__file__:      # (frame 0: count, 1: the wrapper, 2: its caller)
            audit.inner[name] = audit.inner.get(name, 0) + 1

    def gemm(a, b, trans_a=False, trans_b=False, alpha=1.0, beta=0.0, out=None, bias=None):
        count("gemm")
        if depth[0]:
            return real["gemm"](a, b, trans_a, trans_b, alpha, beta, out, bias)
        engine = ops.gemm_engine(a, b, trans_a, trans_b, alpha, beta, out, bias)
        c0 = out.detach().clone() if (out is not None and beta != 0.0) else None
        a64 = (a.t() if trans_a else a).double()
        b64 = (b.t() if trans_b else b).double()
        depth[0] += 1
        try:
            res = real["gemm"](a, b, trans_a, trans_b, alpha, beta, out, bias)
        finally:
            depth[0] -= 1
        want = alpha * (a64 @ b64)
        scale = abs(alpha) * (a64.abs() @ b64.abs())
        ref32 = alpha * ((a.t() if trans_a else a).float() @ (b.t() if trans_b else b).float())
        if c0 is not None:
            want = want + beta * c0.double()
            scale = scale + abs(beta) * c0.double().abs()
            ref32 = ref32 + beta * c0
        if bias is not None:
            want = want + bias.double()
            scale = scale + bias.double().abs()
            ref32 = ref32 + bias
        rec = Record("gemm", _ops_site(), engine, (tuple(a64.shape), tuple(b64.shape)), 0.0, 0.0, "")
        if engine == "tall_f16x2":
            _check_hint(audit, rec, "rowmax", ops.tagged_rowmax(a), a.abs().amax(1) if a.shape[1] else a.new_zeros(a.shape[0]))
        _measure(audit, rec, res.detach(), want, scale, ref32, a64.shape[1])
        return res

    def gemm_tall(a_panels, b_blocks, trans_b, bias=None, alpha=1.0, beta=0.0, out=None, rowmax=None, gate_x=None,
                  keep=None, variant=None):
        count("gemm_tall")
        if depth[0]:
            return real["gemm_tall"](a_panels, b_blocks, trans_b, bias, alpha, beta, out, rowmax, gate_x, keep, variant)
        hint = rowmax if rowmax is not None else None
        tags = [ops.tagged_rowmax(p) for p in a_panels]
        c0 = out.detach().clone() if (out is not None and beta != 0.0) else None
        a64 = torch.cat([p.double() for p in a_panels], 1)
        gate = gate_x is not None
        gx = gate_x.detach().clone() if gate else None
        depth[0] += 1
        try:
            res = real["gemm_tall"](a_panels, b_blocks, trans_b, bias, alpha, beta, out, rowmax, gate_x, keep, variant)
        finally:
            depth[0] -= 1
        rec = Record("gemm_tall" + ("/gate" if gate else ""), _ops_site(), "tall_f16x2",
                     (tuple(a64.shape), len(b_blocks)), 0.0, 0.0, "")
        true_max = a64.abs().amax(1).float()
        if hint is not None:
            _check_hint(audit, rec, "rowmax", hint, true_max)
        for p, t in zip(a_panels, tags):
            if t is not None:
                _check_hint(audit, rec, "tagged rowmax", t, p.abs().amax(1))
        pre = []
        for gi, grp in enumerate(b_blocks):
            b64 = torch.cat([(b.double().t() if trans_b else b.double()) for b in grp], 0)        # [K, rows]
            rows = b64.shape[1]
            bs = bias.double()[gi * rows:(gi + 1) * rows] if bias is not None else None
            want = alpha * (a64 @ b64) + (bs if bs is not None else 0.0)
            scale = abs(alpha) * (a64.abs() @ b64.abs()) + (bs.abs() if bs is not None else 0.0)
            ref32 = alpha * (a64.float() @ b64.float()) + (bs.float() if bs is not None else 0.0)
            pre.append((want, scale, ref32))
        if not gate:
            want, scale, ref32 = pre[0]
            if c0 is not None:
                want, scale, ref32 = want + beta * c0.double(), scale + abs(beta) * c0.double().abs(), ref32 + beta * c0
            _measure(audit, rec, res.detach(), want, scale, ref32)
        elif keep is not None and keep[0] is not None and keep[1] is not None:
            # the blend's inputs: tanh(g) and sigmoid(z) kept for the backward -- back through the (monotone) functions
            # would amplify noise at saturation, so the pre-activations are checked through the derivative instead:
            # |f(got) - f(x64)| <= bound * f'(x64) * scale + the transcendental approximations' own 2e-7 / 1e-6
            for (want, scale, ref32), kept, f, df, eps in (
                    (pre[0], keep[0], torch.tanh, lambda x: 1 - torch.tanh(x) ** 2, 4e-7),
                    (pre[1], keep[1], torch.sigmoid, lambda x: torch.sigmoid(x) * (1 - torch.sigmoid(x)), 2e-6)):
                r32, _ = componentwise(ref32, want, scale)
                bound = bound_for("tall_f16x2", r32)
                err = (kept.detach().double() - f(want)).abs()
                allow = bound * df(want) * scale + eps * (1 + f(want).abs())
                excess = err - allow
                i = int(excess.argmax())
                rec.r, rec.bound = float((err / (df(want) * scale + eps + TINY)).reshape(-1)[i]), bound
                rec.worst = _worst(kept.detach(), f(want), scale, i)
                if float(excess.reshape(-1)[i]) > 0:
                    audit.fail(rec, f"kept {f.__name__} off by {float(err.reshape(-1)[i]):.3g} > {float(allow.reshape(-1)[i]):.3g}; "
                               f"worst {rec.worst}")
            audit.records.append(rec)
        return res

    def gemm_wgrad(a, b, a_colmax, b_colmax):
        count("gemm_wgrad")
        a64, b64 = a.double(), b.double()
        res = real["gemm_wgrad"](a, b, a_colmax, b_colmax)
        rec = Record("gemm_wgrad", _ops_site(), "wgrad_f16x2", (tuple(a.shape), tuple(b.shape)), 0.0, 0.0, "")
        _check_hint(audit, rec, "a_colmax", a_colmax, a.abs().amax(0))
        _check_hint(audit, rec, "b_colmax", b_colmax, b.abs().amax(0))
        _measure(audit, rec, res, a64.t() @ b64, a64.abs().t() @ b64.abs(), a.t() @ b, a.shape[0])
        return res

    def colsum(x):
        count("colsum")
        x64 = x.double()
        res = real["colsum"](x)
        rec = Record("colsum", _ops_site(), "colsum", tuple(x.shape), 0.0, 0.0, "")
        _measure(audit, rec, res, x64.sum(0), x64.abs().sum(0), x.sum(0))
        return res

    def narrow_weight_grad(gy, panel, want_sum):
        count("narrow_weight_grad")
        g64, p64 = gy.double(), panel.double()
        gw, gs = real["narrow_weight_grad"](gy, panel, want_sum)
        rec = Record("narrow_weight_grad", _ops_site(), "colsum", (tuple(gy.shape), tuple(panel.shape)), 0.0, 0.0, "")
        _measure(audit, rec, gw, g64.t() @ p64, g64.abs().t() @ p64.abs(), gy.t() @ panel)
        if gs is not None:
            rec2 = Record("narrow_weight_grad/sum", rec.site, "colsum", rec.shape, 0.0, 0.0, "")
            _measure(audit, rec2, gs, g64.sum(0), g64.abs().sum(0), gy.sum(0))
        return gw, gs

    def gemm_f64acc(a, b, trans_a=False, trans_b=False):
        count("gemm_f64acc")
        a64 = (a.t() if trans_a else a).double()
        b64 = (b.t() if trans_b else b).double()
        res = real["gemm_f64acc"](a, b, trans_a, trans_b)
        want = a64 @ b64
        rec = Record("gemm_f64acc", _ops_site(), "f64acc", (tuple(a64.shape), tuple(b64.shape)), 0.0, 0.0, "")
        # one f32 rounding of the float64 sum, plus the float64 accumulation's own k * 2^-53 of sum |a||b|
        err = (res.double() - want).abs()
        allow = want.abs() * 2.0 ** -24 + (a64.shape[1] + 2) * 2.0 ** -53 * (a64.abs() @ b64.abs()) + 2.0 ** -150
        excess = err - allow
        i = int(excess.argmax()) if excess.numel() else 0
        rec.r, rec.bound = (float(excess.reshape(-1)[i]) if excess.numel() else 0.0), 0.0
        rec.worst = _worst(res, want, allow, i) if excess.numel() else ""
        if excess.numel() and rec.r > 0:
            audit.fail(rec, f"more than one f32 rounding from float64; worst {rec.worst}")
        audit.records.append(rec)
        return res

    def linear_act_layernorm_fwd(a_panels, w_blocks, bias, gamma, beta, slope, eps, norm_eps, drop_p, seed, want_y=True,
                                 want_norm=True, yn_out=None, rowmax=None):
        count("linear_act_layernorm_fwd")
        a64 = torch.cat([p.double() for p in a_panels], 1)
        w64 = torch.cat([w.double() for w in w_blocks], 1)
        res = real["linear_act_layernorm_fwd"](a_panels, w_blocks, bias, gamma, beta, slope, eps, norm_eps, drop_p, seed,
                                               want_y, want_norm, yn_out, rowmax)
        rec = Record("linear_act_layernorm_fwd", _ops_site(), "tall_f16x2", (tuple(a64.shape), tuple(w64.shape)), 0.0, 0.0, "")
        if rowmax is not None:
            _check_hint(audit, rec, "rowmax", rowmax, a64.abs().amax(1).float())
        for p in a_panels:
            t = ops.tagged_rowmax(p)
            if t is not None:
                _check_hint(audit, rec, "tagged rowmax", t, p.abs().amax(1))
        # y / yn against LayerNorm(LeakyReLU(.)) of the float64 product: never further than 3 x the unfused pair (the tall
        # product, then torch's float32 LeakyReLU + LayerNorm), floor 2e-6 -- the bound of
        # test_fused_linear_act_layernorm_at_the_range_edges.  (With dropout the mask is the kernel's own: hints only.)
        rec.r, rec.bound, rec.worst = 0.0, 0.0, "(dropout: hints only)"
        if drop_p == 0.0:
            n = w64.shape[0]
            fn = torch.nn.functional

            def ln(z, dt):
                y_ = fn.layer_norm(fn.leaky_relu(z, slope), (n,), gamma.to(dt), beta.to(dt), eps)
                return y_, y_ / y_.norm(dim=1, keepdim=True).clamp_min(norm_eps)
            y64, yn64 = ln(a64 @ w64.t() + (bias.double() if bias is not None else 0.0), torch.float64)
            y32, yn32 = ln(real["gemm_tall"](a_panels, (tuple(w_blocks),), True, bias), torch.float32)
            for what, got, want, unfused in (("y", res[0], y64, y32), ("yn", res[1], yn64, yn32)):
                if got is None:
                    continue
                err = float((got.double() - want).abs().max())
                allow = max(3.0 * float((unfused.double() - want).abs().max()), 2e-6)
                rec.r, rec.bound, rec.worst = max(rec.r, err), allow, what
                if err > allow:
                    audit.fail(rec, f"fused {what} {err:.3g} from float64, the unfused pair's bound {allow:.3g}")
        audit.records.append(rec)
        return res

    wrappers = dict(gemm=gemm, gemm_tall=gemm_tall, gemm_wgrad=gemm_wgrad, colsum=colsum,
                    narrow_weight_grad=narrow_weight_grad, gemm_f64acc=gemm_f64acc,
                    linear_act_layernorm_fwd=linear_act_layernorm_fwd)
    for name, w in wrappers.items():
        setattr(ops, name, w)
    try:
        yield audit
    finally:
        for name, f in real.items():
            setattr(ops, name, f)


def report(audit: Audit, limit: int = 12) -> str:
    lines = list(audit.failures[:limit])
    if len(audit.failures) > limit:
        lines.append(f"... and {len(audit.failures) - limit} more")
    return "\n".join(lines)
