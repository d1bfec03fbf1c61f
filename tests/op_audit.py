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


# ------------------------------------------------------------------------------- row-wise, sparse and grouped families
# Plain references of the kernels outside the GEMM engines (test_rowwise_conditioning_gpu.py on the device,
# test_rowwise_measures_host.py for the measures themselves).  Each is a function of the float32 inputs only, works on CPU
# and GPU tensors alike, and comes as  X_eval(..., dtype)  -- the expression evaluated in ``dtype`` (torch.float64: the
# reference; torch.float32: torch's own float32 evaluation, the r_torch32 of the bound) -- and  X_scale(...)  -- the sum of
# the absolute values of the terms of the float64 expression, per output element.
def f32(x: float) -> float:
    """the float32 a kernel receives when it is handed the Python float x"""
    return float(torch.tensor(x, dtype=torch.float32))


def leaky(x: torch.Tensor, slope: float) -> torch.Tensor:
    return torch.where(x > 0, x, x * slope)


def units(n: int) -> float:
    """n roundings of float32, each at most 2^-24 of the scale, with their second-order product"""
    return n * U * (1.0 + n * U)


def within_units(got, want64, scale64, n_units: float, extra=None):
    """(worst |err| / allowance, flat index) with allowance = n_units 2^-24 scale (+ extra, an absolute per-element term)"""
    allow = units(n_units) * scale64 + (extra if extra is not None else 0.0) + TINY
    q = (got.double() - want64).abs() / allow
    q = torch.nan_to_num(q, nan=math.inf)
    i = int(q.argmax()) if q.numel() else 0
    return (float(q.reshape(-1)[i]) if q.numel() else 0.0), i


# allowances of the kept activations (the gate epilogue's, above): absolute error of tanh_fast / sigmoid_fast
def tanh_allow(t64):
    return 4e-7 * (1 + t64.abs())


def sigmoid_allow(s64):
    return 2e-6 * (1 + s64.abs())


# ---- grouped GEMM (lkg_grouped_gemm_f32)
def grouped_blocks(mode, seg, a, b, trans_b, b_period):
    """[(group, row slice, A operand [m, k], B operand [k, n])] in math layout, float32 views"""
    sg = [int(v) for v in seg.tolist()]
    out = []
    for g in range(len(sg) - 1):
        lo_, hi_ = sg[g], sg[g + 1]
        if mode == 1:
            blk = b[g % b_period if b_period > 0 else g] if b.dim() == 3 else b
            out.append((g, slice(lo_, hi_), a[lo_:hi_], blk.t() if trans_b else blk))
        else:
            out.append((g, slice(lo_, hi_), a[lo_:hi_].t(), b[lo_:hi_]))
    return out


def grouped_eval(mode, seg, a, b, c0, beta, trans_b, b_period, dtype):
    """rows mode: {group: C rows of the segment}; k mode: {group: C block}.  c0: C before the call (rows mode: the whole
    [M, n] view; k mode: [G, m, n]) or None with beta = 0."""
    res = {}
    for g, rows, am, bm in grouped_blocks(mode, seg, a, b, trans_b, b_period):
        v = am.to(dtype) @ bm.to(dtype)
        if beta != 0.0:
            v = v + beta * (c0[rows] if mode == 1 else c0[g]).to(dtype)
        res[g] = v
    return res


def grouped_scale(mode, seg, a, b, c0, beta, trans_b, b_period):
    res = {}
    for g, rows, am, bm in grouped_blocks(mode, seg, a, b, trans_b, b_period):
        v = am.double().abs() @ bm.double().abs()
        if beta != 0.0:
            v = v + abs(beta) * (c0[rows] if mode == 1 else c0[g]).double().abs()
        res[g] = v
    return res


# ---- LeakyReLU + LayerNorm + normalised copy (lkg_act_layernorm_*), BatchNorm(ReLU) (lkg_relu_batchnorm_*)
def layernorm_fwd_eval(z, gamma, beta, slope, eps, norm_eps, dtype, mean_over=None, drop=None):
    """{mean, rstd, y, yn}.  mean_over: a planted fault for the host test (the row mean taken over that many elements).
    drop: the dropout scale per element (0 or 1 / (1 - p), as float32 holds it), applied to y before the normalised copy."""
    a = leaky(z.to(dtype), slope)
    d = a.shape[1]
    mean = a.sum(1) / (mean_over or d)
    c = a - mean[:, None]
    rstd = 1.0 / torch.sqrt((c * c).sum(1) / d + eps)
    y = c * rstd[:, None] * gamma.to(dtype) + beta.to(dtype)
    if drop is not None:
        y = y * drop.to(dtype)
    nrm = torch.sqrt((y * y).sum(1))
    yn = y / nrm.clamp_min(norm_eps)[:, None]
    return dict(mean=mean, rstd=rstd, y=y, yn=yn)


def layernorm_fwd_scale(z, gamma, beta, slope, eps, norm_eps, drop=None):
    w = layernorm_fwd_eval(z, gamma, beta, slope, eps, norm_eps, torch.float64, drop=drop)
    a = leaky(z.double(), slope).abs()
    ma = a.mean(1)
    sy = (a + ma[:, None]) * w["rstd"][:, None] * gamma.double().abs() + beta.double().abs()
    if drop is not None:
        sy = sy * drop.double()
    nrm = torch.sqrt((w["y"] * w["y"]).sum(1)).clamp_min(norm_eps)
    return dict(mean=ma, rstd=w["rstd"], y=sy, yn=sy / nrm[:, None])


def _ln_upstream(y, gy, gyn, norm_eps, dtype):
    """G = g_y + d(yn)/dy applied to g_yn, and the |.|-sum of its terms"""
    g = torch.zeros_like(y, dtype=dtype) if gy is None else gy.to(dtype)
    ag = g.abs()
    if gyn is not None:
        yy, gn = y.to(dtype), gyn.to(dtype)
        nrm = torch.sqrt((yy * yy).sum(1, keepdim=True))
        big = nrm > norm_eps
        inv = 1.0 / torch.where(big, nrm, torch.full_like(nrm, norm_eps))
        dot = (yy * gn).sum(1, keepdim=True)
        adot = (yy * gn).abs().sum(1, keepdim=True)
        g = g + gn * inv - torch.where(big, yy * dot * inv ** 3, torch.zeros_like(yy))
        ag = ag + gn.abs() * inv + torch.where(big, yy.abs() * adot * inv ** 3, torch.zeros_like(yy))
    return g, ag


def layernorm_bwd_eval(z, gamma, mean, rstd, y, gy, gyn, slope, norm_eps, dtype, drop=None):
    """{gz, g_gamma, g_beta} from the backward kernel's own float32 inputs (z, gamma, the saved mean / rstd / y, g_y, g_yn).
    drop: the dropout scale per element; y, g_y and g_yn then refer to the MASKED output, and G goes through the mask."""
    zz = z.to(dtype)
    xh = (leaky(zz, slope) - mean.to(dtype)[:, None]) * rstd.to(dtype)[:, None]
    g, _ = _ln_upstream(y, gy, gyn, norm_eps, dtype)
    if drop is not None:
        g = g * drop.to(dtype)
    dxh = g * gamma.to(dtype)
    da = rstd.to(dtype)[:, None] * (dxh - dxh.mean(1, keepdim=True) - xh * (dxh * xh).mean(1, keepdim=True))
    gz = da * torch.where(zz > 0, torch.ones_like(zz), torch.full_like(zz, slope))
    return dict(gz=gz, g_gamma=(g * xh).sum(0), g_beta=g.sum(0))


def layernorm_bwd_scale(z, gamma, mean, rstd, y, gy, gyn, slope, norm_eps, drop=None):
    zz = z.double()
    xh = ((leaky(zz, slope) - mean.double()[:, None]) * rstd.double()[:, None]).abs()
    _, ag = _ln_upstream(y, gy, gyn, norm_eps, torch.float64)
    if drop is not None:
        ag = ag * drop.double()
    adx = ag * gamma.double().abs()
    gz = rstd.double()[:, None] * (adx + adx.mean(1, keepdim=True) + xh * (adx * xh).mean(1, keepdim=True))
    gz = gz * torch.where(zz > 0, torch.ones_like(zz), torch.full_like(zz, slope))
    return dict(gz=gz, g_gamma=(ag * xh).sum(0), g_beta=ag.sum(0))


def batchnorm_fwd_eval(z, gamma, beta, run_mean, run_var, training, momentum, eps, dtype, mean_over=None):
    """{mean, invstd, y, run_mean, run_var} of BatchNorm1d(relu(z)) (the running buffers after the step; unbiased variance)"""
    a = torch.relu(z.to(dtype))
    n = a.shape[0]
    if training:
        mean = a.sum(0) / (mean_over or n)
        var = ((a - mean) ** 2).sum(0) / n
        new_mean = (1 - momentum) * run_mean.to(dtype) + momentum * mean
        new_var = (1 - momentum) * run_var.to(dtype) + momentum * var * (n / max(n - 1, 1))
    else:
        mean, var = run_mean.to(dtype), run_var.to(dtype)
        new_mean, new_var = mean, var
    invstd = 1.0 / torch.sqrt(var + eps)
    y = (a - mean) * invstd * gamma.to(dtype) + beta.to(dtype)
    return dict(mean=mean, invstd=invstd, y=y, run_mean=new_mean, run_var=new_var)


def batchnorm_fwd_scale(z, gamma, beta, run_mean, run_var, training, momentum, eps):
    w = batchnorm_fwd_eval(z, gamma, beta, run_mean, run_var, training, momentum, eps, torch.float64)
    a = torch.relu(z.double())
    n = a.shape[0]
    ma = a.mean(0) if training else run_mean.double().abs()
    sy = (a + ma) * w["invstd"] * gamma.double().abs() + beta.double().abs()
    if training:
        var = ((a - w["mean"]) ** 2).sum(0) / n
        s_rm = (1 - momentum) * run_mean.double().abs() + momentum * ma
        s_rv = (1 - momentum) * run_var.double().abs() + momentum * var * (n / max(n - 1, 1))
    else:
        s_rm, s_rv = run_mean.double().abs(), run_var.double().abs()
    return dict(mean=ma, invstd=w["invstd"], y=sy, run_mean=s_rm, run_var=s_rv)


def batchnorm_bwd_eval(z, gamma, mean, invstd, gy, training, dtype):
    """{gz, g_gamma, g_beta} from the backward kernel's own float32 inputs (z, gamma, the saved mean / invstd, g_y)"""
    zz, dy = z.to(dtype), gy.to(dtype)
    xh = (torch.relu(zz) - mean.to(dtype)) * invstd.to(dtype)
    s1, s2 = dy.sum(0), (dy * xh).sum(0)
    n = zz.shape[0]
    da = gamma.to(dtype) * invstd.to(dtype) * ((dy - s1 / n - xh * s2 / n) if training else dy)
    return dict(gz=torch.where(zz > 0, da, torch.zeros_like(da)), g_gamma=s2, g_beta=s1)


def batchnorm_bwd_scale(z, gamma, mean, invstd, gy, training):
    zz, dy = z.double(), gy.double().abs()
    xh = ((torch.relu(zz) - mean.double()) * invstd.double()).abs()
    s1, s2 = dy.sum(0), (dy * xh).sum(0)
    n = zz.shape[0]
    da = gamma.double().abs() * invstd.double() * ((dy + s1 / n + xh * s2 / n) if training else dy)
    return dict(gz=torch.where(zz > 0, da, torch.zeros_like(da)), g_gamma=s2, g_beta=s1)


# ---- SpMM (lkg_spmm_csr_fused_f32)
def spmm_eval(rowptr, col, val, x, n_rows, dtype, add_self=None, add2=None, bias=None, absolute=False, drop_last_of=None):
    """out[i] = sum_j val[j] x[col[j]] (+ add_self[i] + add2[i] | bias).  absolute: every term by its absolute value (the
    scale).  drop_last_of: a planted fault for the host test (the last entry of that row left out)."""
    rp = rowptr.long()
    cnt = rp[1:n_rows + 1] - rp[:n_rows]
    rows = torch.repeat_interleave(torch.arange(n_rows, device=x.device), cnt)
    lo_, hi_ = int(rp[0]), int(rp[n_rows])
    cc, vv = col.long()[lo_:hi_], val.to(dtype)[lo_:hi_]
    terms = vv[:, None] * x.to(dtype)[cc]
    if drop_last_of is not None:
        terms[int(rp[drop_last_of + 1]) - 1 - lo_] = 0
    if absolute:
        terms = terms.abs()
    out = torch.zeros(n_rows, x.shape[1], dtype=dtype, device=x.device).index_add_(0, rows, terms)
    for t in (add_self, add2, bias):
        if t is not None:
            out = out + (t.to(dtype).abs() if absolute else t.to(dtype))
    return out


# ---- element-wise row walkers (lkg_eltwise_f32, lkg_bi_mix_*, lkg_gate_blend_*): (want64, scale64, roundings)
def eltwise_ref(op, a, b, alpha, beta):
    """lkg_eltwise_f32's four ops; the rounding count is that of the kernel's expression (lkg_rowwise.hip)"""
    x, al, be = a.double(), f32(alpha), f32(beta)
    y = b.double() if b is not None else None
    if op == 0:
        if y is None:
            return al * x + be, (al * x).abs() + abs(be), 1                 # fmaf(alpha, x, beta)
        return al * x + be * y, (al * x).abs() + (be * y).abs(), 2          # fmaf(alpha, x, beta * y)
    if op == 1:
        return x * y, (x * y).abs(), 1                                      # x * y
    if op == 2:
        lx = leaky(x, al)
        if y is None:
            return lx, lx.abs(), 1                                          # alpha * x (+ 0)
        ly = leaky(y, al)
        return lx + ly, lx.abs() + ly.abs(), 3                              # alpha * x, alpha * y, the sum
    w = x * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, al))
    return w, w.abs(), 1                                                    # x * (1 | alpha)


def bi_mix_fwd_ref(ego, side, h0p, alpha):
    """{sum, prod} -> (want64, scale64, roundings): fmaf(c, e + s, alpha * h) with c = 1 - alpha is c, e + s, alpha * h and
    the fma: 4; the product form likewise (e * s in place of e + s); without h0p c = 1 and the added term is 0: 1"""
    e, s = ego.double(), side.double()
    if h0p is None:
        return dict(sum=(e + s, e.abs() + s.abs(), 1), prod=(e * s, (e * s).abs(), 1))
    al = f32(alpha)
    c, hh = 1.0 - al, al * h0p.double()
    return dict(sum=(c * (e + s) + hh, c * (e.abs() + s.abs()) + hh.abs(), 4),
                prod=(c * e * s + hh, c * (e * s).abs() + hh.abs(), 4))


def bi_mix_bwd_ref(ego, side, g_sum, g_prod, has_h0, alpha):
    """{g_ego, g_side, g_h0p}: c * fmaf(gp, s, gs) is c, the fma and the product: 3 (1 without h0p: c = 1);
    alpha * (gs + gp): 2"""
    e, s, gs, gp = ego.double(), side.double(), g_sum.double(), g_prod.double()
    al = f32(alpha)
    c = 1.0 - al if has_h0 else 1.0
    n_r = 3 if has_h0 else 1
    res = dict(g_ego=(c * (gp * s + gs), c * ((gp * s).abs() + gs.abs()), n_r),
               g_side=(c * (gp * e + gs), c * ((gp * e).abs() + gs.abs()), n_r))
    if has_h0:
        res["g_h0p"] = (al * (gs + gp), al * (gs.abs() + gp.abs()), 2)
    return res


def gate_blend_fwd_ref(x, gpre, zpre):
    """(want64, scale64, roundings, extra): out = (1 - s) x + s t with s = sigmoid(z), t = tanh(g): 1 - s, its product,
    s * t and the sum: 4; the activations' allowances through the derivative: s dt + |t - x| ds"""
    xx = x.double()
    s, t = torch.sigmoid(zpre.double()), torch.tanh(gpre.double())
    want = (1 - s) * xx + s * t
    scale = (1 + s) * xx.abs() + s * t.abs()          # (1 - s is itself a difference: |1| + |s|)
    return want, scale, 4, s * tanh_allow(t) + (t - xx).abs() * sigmoid_allow(s)


def gate_blend_bwd_ref(x, gpre, zpre, go):
    """{g_x, g_gpre, g_zpre} -> (want64, scale64, roundings, extra) of lkg_gate_blend_bwd_f32 (activated = 0):
    g_x = go (1 - s): 2;  g_gpre = go s (1 - t t): 4;  g_zpre = go (t - x) s (1 - s): 5"""
    xx, g = x.double(), go.double()
    s, t = torch.sigmoid(zpre.double()), torch.tanh(gpre.double())
    ds, dt = sigmoid_allow(s), tanh_allow(t)
    ag = g.abs()
    return dict(
        g_x=(g * (1 - s), ag * (1 + s), 2, ag * ds),
        g_gpre=(g * s * (1 - t * t), ag * s * (1 + t * t), 4, ag * ((1 - t * t) * ds + s * 2 * t.abs() * dt + s * dt * dt)),
        g_zpre=(g * (t - xx) * s * (1 - s), ag * (t.abs() + xx.abs()) * s * (1 + s), 5,
                ag * (s * (1 - s) * dt + (t - xx).abs() * ((1 - 2 * s).abs() * ds + ds * ds) + dt * ds * (1 + 2 * ds))))


# ---- attention refresh (lkg_edge_softmax_f32)
def _entry_edges(rowptr, col, eptr, n_rows):
    """(head row of every raw edge, stored entry of every raw edge, entry offsets)"""
    dev = col.device
    nnz = col.numel()
    rp = rowptr.long()
    rows = torch.repeat_interleave(torch.arange(n_rows, device=dev), rp[1:n_rows + 1] - rp[:n_rows])
    ep = eptr.long() if eptr is not None else torch.arange(nnz + 1, device=dev)
    entry = torch.repeat_interleave(torch.arange(nnz, device=dev), ep[1:] - ep[:-1])
    return rows[entry], entry, ep


def attention_logits_eval(rowptr, col, eptr, rel, ent, relemb, dtype, tanh=torch.tanh):
    """(logits, scale, allowance) per stored entry:  sum over the entry's raw edges of  sum_d t_d tanh(h_d + r_d);
    scale  sum |t_d| |tanh|;  allowance (float64 only): tanh_fast's 4e-7 (1 + |tanh|) and the rounding of h + r through
    tanh' = 1 - tanh^2, each times |t_d|.  tanh: a planted fault for the host test."""
    head, entry, _ = _entry_edges(rowptr, col, eptr, ent.shape[0])
    e_, r_ = ent.to(dtype), relemb.to(dtype)
    h, t, r = e_[head], e_[col.long()[entry]], r_[rel.long()[:entry.numel()]]
    th = tanh(h + r)
    nnz = col.numel()
    z = lambda: torch.zeros(nnz, dtype=dtype, device=ent.device)
    logits = z().index_add_(0, entry, (t * th).sum(1))
    scale = z().index_add_(0, entry, (t * th).abs().sum(1))
    allow = z().index_add_(0, entry, (t.abs() * (tanh_allow(th) + (1 - th * th) * U * (h.abs() + r.abs()))).sum(1))
    return logits, scale, allow


# roundings of one logit (lkg_attention.hip): the product, the lane's own chain (at most 4 chunks of 4 on the 16-byte path, 4
# elements on the scalar one), the 6 butterfly steps, and the merge of up to 3 raw edges with the pre-pass' own wave sum
def attention_logit_units(vec: bool) -> int:
    return 1 + (16 if vec else 4) + 6 + 3


def row_softmax_eval(rowptr, logits, n_rows, dtype, subtract_max=True):
    """softmax of the stored logits over each row's entries.  subtract_max=False: a planted fault for the host test."""
    rp = rowptr.long()
    rows = torch.repeat_interleave(torch.arange(n_rows, device=logits.device), rp[1:n_rows + 1] - rp[:n_rows])
    lo_, hi_ = int(rp[0]), int(rp[n_rows])
    l = logits.to(dtype)[lo_:hi_]
    mx = torch.full((n_rows,), -math.inf, dtype=dtype, device=l.device).scatter_reduce_(0, rows, l, "amax")
    sh = l - mx[rows] if subtract_max else l
    e = torch.exp(sh)
    s = torch.zeros(n_rows, dtype=dtype, device=l.device).index_add_(0, rows, e)
    return e / s[rows], (l - mx[rows]).abs()


def softmax_excess(got, want64, ref32, spread):
    """worst  |got - want| / allowed  with the allowed relative error  max(3 r_torch32, 2^-24 (4 + |l - max l|))  per entry
    (one rounding of the exponent's argument carried through exp, plus exp, the sum and the division), and float32's
    subnormal spacing 2^-149 as the absolute floor"""
    rel32 = (ref32.double() - want64).abs() / (want64 + TINY)
    allow = want64 * torch.maximum(3.0 * rel32, U * (4.0 + spread)) + 2.0 ** -149
    q = torch.nan_to_num((got.double() - want64).abs() / allow, nan=math.inf)
    i = int(q.argmax()) if q.numel() else 0
    return (float(q[i]) if q.numel() else 0.0), i


# ---- triple scores and losses (lkg_score.hip)
def softplus_neg(x):
    """-logsigmoid(x) = softplus(-x), stable in both tails"""
    return torch.clamp(-x, min=0) + torch.log1p(torch.exp(-x.abs()))


def trans_scores_eval(eh, er, ep, en, dtype):
    """rows of h, r, t+, t- (one per triple) -> {pos, neg, reg} and their scales: sum (|h| + |r| + |t|)^2, reg"""
    h, r, p, n = (t.to(dtype) for t in (eh, er, ep, en))
    pos, neg = ((h + r - p) ** 2).sum(1), ((h + r - n) ** 2).sum(1)
    reg = 0.5 * ((h * h).sum(1) + (r * r).sum(1) + (p * p).sum(1) + (n * n).sum(1))
    scale = dict(pos=((h.abs() + r.abs() + p.abs()) ** 2).sum(1), neg=((h.abs() + r.abs() + n.abs()) ** 2).sum(1), reg=reg)
    return dict(pos=pos, neg=neg, reg=reg), scale


def dot_scores_eval(eh, ep, en, dtype):
    h, p, n = (t.to(dtype) for t in (eh, ep, en))
    reg = 0.5 * ((h * h).sum(1) + (p * p).sum(1) + (n * n).sum(1))
    return (dict(pos=(h * p).sum(1), neg=(h * n).sum(1), reg=reg),
            dict(pos=(h * p).abs().sum(1), neg=(h * n).abs().sum(1), reg=reg))


def rank_eval(margin, dtype):
    """(rank, scale) of -logsigmoid(margin): |margin| + log 2"""
    m = margin.to(dtype)
    return softplus_neg(m), m.abs() + math.log(2.0)


def loss_eval(rank, reg, lam, dtype):
    a, b = rank.to(dtype).mean(), reg.to(dtype).mean()
    return a + lam * b, a.abs() + abs(lam) * b.abs()


def trans_grads_eval(eh, er, ep, en, pos, neg, lam, g, dtype, sigmoid=torch.sigmoid):
    """Per-triple gradient rows {h, r, p, n} of the TransE / TransR score loss from the backward kernel's own inputs (the
    rows and the float32 pos / neg it kept), with the |.|-sums of their terms and the allowance for sigmoidf_'s
    2e-6 (1 + |sigmoid|) through the terms it multiplies:
        dp = g sigmoid(pos - neg) / B,  u = h + r - p,  w = h + r - n
        g_h = g_r' = 2 (u - w) dp + lr h | r ;  g_p = -2 u dp + lr p ;  g_n = 2 w dp + lr n ;  lr = g lam / B"""
    h, r, p, n = (t.to(dtype) for t in (eh, er, ep, en))
    b = h.shape[0]
    sg = sigmoid((pos.to(dtype) - neg.to(dtype)))[:, None]
    dp, lr = g * sg / b, g * lam / b
    u, w = h + r - p, h + r - n
    su, sw = h.abs() + r.abs() + p.abs(), h.abs() + r.abs() + n.abs()
    common, s_common = 2 * (u * dp - w * dp), 2 * (su + sw) * dp.abs()
    val = dict(h=common + lr * h, r=common + lr * r, p=-2 * u * dp + lr * p, n=2 * w * dp + lr * n)
    scale = dict(h=s_common + (lr * h).abs(), r=s_common + (lr * r).abs(), p=2 * su * dp.abs() + (lr * p).abs(),
                 n=2 * sw * dp.abs() + (lr * n).abs())
    ds = abs(g) / b * sigmoid_allow(sg)
    allow = dict(h=2 * (u - w).abs() * ds, r=2 * (u - w).abs() * ds, p=2 * u.abs() * ds, n=2 * w.abs() * ds)
    return val, scale, allow


def dot_grads_eval(eh, ep, en, pos, neg, lam, g, dtype, sigmoid=torch.sigmoid):
    """dn = g sigmoid(neg - pos) / B, dp = -dn:  g_h = dp p + dn n + lr h ;  g_p = dp h + lr p ;  g_n = dn h + lr n"""
    h, p, n = (t.to(dtype) for t in (eh, ep, en))
    b = h.shape[0]
    sg = sigmoid((neg.to(dtype) - pos.to(dtype)))[:, None]
    dn, lr = g * sg / b, g * lam / b
    val = dict(h=dn * (n - p) + lr * h, p=-dn * h + lr * p, n=dn * h + lr * n)
    scale = dict(h=dn.abs() * (n.abs() + p.abs()) + (lr * h).abs(), p=(dn * h).abs() + (lr * p).abs(),
                 n=(dn * h).abs() + (lr * n).abs())
    ds = abs(g) / b * sigmoid_allow(sg)
    allow = dict(h=(n - p).abs() * ds, p=h.abs() * ds, n=h.abs() * ds)
    return val, scale, allow


def scatter_rows(n_rows, parts, dtype):
    """sum of the per-triple rows into a table: parts = [(ids, rows)]"""
    d = parts[0][1].shape[1]
    out = torch.zeros(n_rows, d, dtype=dtype, device=parts[0][1].device)
    for ids, rows in parts:
        out.index_add_(0, ids.long(), rows.to(dtype))
    return out


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
    """Wrap ops.gemm, gemm_tall, gemm_wgrad, colsum, narrow_weight_grad, gemm_f64acc, linear_act_layernorm_fwd and
    _grouped (the TransR loss's grouped products, counted as "grouped"): every call clones its inputs, runs the real op,
    and checks the result against float64 with the bound of the engine that ran and every scale hint against the true
    maximum.  Yields the Audit."""
    audit = Audit()
    real = {name: getattr(ops, name) for name in ("gemm", "gemm_tall", "gemm_wgrad", "colsum", "narrow_weight_grad",
                                                   "gemm_f64acc", "linear_act_layernorm_fwd", "_grouped")}
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

    def _grouped(mode, seg, max_len, a, b, out, m, n, k, trans_a, trans_b, beta, stride_b=0, stride_c=0, b_period=0):
        count("grouped")
        c0 = out.detach().clone() if beta != 0.0 else None
        real["_grouped"](mode, seg, max_len, a, b, out, m, n, k, trans_a, trans_b, beta, stride_b, stride_c, b_period)
        if seg.numel() < 2 or out.numel() == 0:
            return
        args = (mode, seg, a, b, c0, beta, trans_b, b_period)
        want = grouped_eval(*args, torch.float64)
        scale = grouped_scale(*args)
        ref32 = grouped_eval(*args, torch.float32)
        site = _ops_site()
        for g, rows, am, bm in grouped_blocks(mode, seg, a, b, trans_b, b_period):
            if want[g].numel() == 0:
                continue
            rec = Record("grouped/" + ("rows" if mode == 1 else "k"), site, "f32_mfma", (tuple(am.shape), tuple(bm.shape)),
                         0.0, 0.0, "")
            _measure(audit, rec, (out[rows] if mode == 1 else out[g]).detach(), want[g], scale[g], ref32[g], am.shape[1])

    wrappers = dict(gemm=gemm, gemm_tall=gemm_tall, gemm_wgrad=gemm_wgrad, colsum=colsum,
                    narrow_weight_grad=narrow_weight_grad, gemm_f64acc=gemm_f64acc,
                    linear_act_layernorm_fwd=linear_act_layernorm_fwd, _grouped=_grouped)
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
