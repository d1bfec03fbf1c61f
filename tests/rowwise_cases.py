"""Inputs and checks shared by test_rowwise_conditioning_gpu.py (the HIP kernels on the device) and
test_rowwise_measures_host.py (torch's float32 and planted faults on the CPU, through the SAME draws and the SAME checks):
the row-wise, sparse and grouped kernels against float64 per element (op_audit.py holds the references, scales and bounds).

A draw_* function makes the float32 inputs of one case on a device; a check_* function takes those inputs and the outputs
of an implementation, asserts every bound and appends one line per output to ``lines``:  (what, r, bound)."""
import math
from types import SimpleNamespace as NS

import numpy as np
import torch

import op_audit as A
from op_audit import U, TINY, bound_for, componentwise

SENTINEL = -7.25


def finite(t) -> bool:
    return bool(torch.isfinite(t).all())


def gen_for(device, seed):
    return torch.Generator(device=device).manual_seed(seed)


def table_view(gen, device, n, d, offset, scale=1.0):
    """an [n, d] float32 operand: contiguous (16-byte rows when d % 4 == 0), or -- offset -- a view starting one float into
    a wider table (the scalar path)"""
    if not offset:
        return torch.randn(n, d, device=device, generator=gen) * scale
    return (torch.randn(n, d + 3, device=device, generator=gen) * scale)[:, 1:1 + d]


def report(lines, limit=None):
    rows = sorted(lines, key=lambda l: -(l[1] / l[2] if l[2] else 0.0))
    return "\n".join(f"  {w:58s} r {r:.3g}  bound {b:.3g}  r/bound {(r / b if b else 0.0):.3f}" for w, r, b in rows[:limit])


def check_reduction(lines, what, got, want64, scale64, ref32, engine="colsum", k=0, extra=None):
    """max r <= max(F r_torch32, FLOOR, chain term) per element; extra: an absolute per-element allowance on top"""
    assert finite(want64), f"{what}: the float64 reference is not finite"
    assert finite(ref32), f"{what}: torch's float32 result is not finite"
    assert got.shape == want64.shape, (what, tuple(got.shape), tuple(want64.shape))
    r32, _ = componentwise(ref32, want64, scale64)
    bound = bound_for(engine, r32, k)
    if extra is None:
        r, i = componentwise(got, want64, scale64)
    else:       # |err| <= bound scale + extra, reported on the scale of the bound
        q = torch.nan_to_num((got.double() - want64).abs() / (bound * scale64 + extra + TINY), nan=math.inf)
        i = int(q.argmax()) if q.numel() else 0
        r = (float(q.reshape(-1)[i]) if q.numel() else 0.0) * bound
    lines.append((what, r, bound))
    assert r <= bound, (f"{what}: r = {r:.3g} > bound {bound:.3g} (torch f32 {r32:.3g}); worst element {i}: got "
                        f"{got.reshape(-1)[i].item()!r}, x64 {want64.reshape(-1)[i].item()!r}, scale "
                        f"{scale64.reshape(-1)[i].item()!r}")


def check_units(lines, what, got, want64, scale64, n_units, extra=None):
    """|err| <= n_units 2^-24 scale (+ extra): the counted roundings of an element-wise expression"""
    assert finite(want64), f"{what}: the float64 reference is not finite"
    assert got.shape == want64.shape, (what, tuple(got.shape), tuple(want64.shape))
    q, i = A.within_units(got, want64, scale64, n_units, extra)
    lines.append((what, q * n_units * U, n_units * U))
    assert q <= 1.0, (f"{what}: {q:.3g} x the allowance of {n_units} roundings; worst element {i}: got "
                      f"{got.reshape(-1)[i].item()!r}, x64 {want64.reshape(-1)[i].item()!r}, scale "
                      f"{scale64.reshape(-1)[i].item()!r}")


# =============================================================================================== (a) grouped GEMM
ROWS_START, ROWS_LENGTHS, ROWS_TRAIL = 3, (1, 127, 0, 128, 129, 300, 2, 0, 61), 6     # starts 3 4 131 131 259 388 688 690 690
ROWS_LAYOUT = {(33, 70): (40, 4, 76, 4), (300, 256): (303, 1, 259, 2), (64, 520): (72, 4, 528, 4)}   # lda, col0, ldc, col0
K_START, K_LENGTHS, K_TRAIL = 2, (0, 1, 15, 16, 17, 2000), 3


def seg_of(start, lengths, device):
    return torch.tensor(np.concatenate([[start], start + np.cumsum(lengths)]), dtype=torch.int32, device=device)


def cancelling(b, dim):
    """pair up the entries along ``dim`` with opposite signs: against a large common part of the other operand the
    products cancel to the noise"""
    idx_even = [slice(None)] * b.dim()
    idx_odd = list(idx_even)
    n2 = b.shape[dim] // 2
    idx_even[dim], idx_odd[dim] = slice(0, 2 * n2, 2), slice(1, 2 * n2, 2)
    b[tuple(idx_odd)] = -b[tuple(idx_even)]
    return b


def draw_grouped_rows(device, k, n, trans_b, mu=0.0, seed=0):
    gen = gen_for(device, 1000 + seed + k + n)
    lda, a0, ldc, c0 = ROWS_LAYOUT[(k, n)]
    seg = seg_of(ROWS_START, ROWS_LENGTHS, device)
    m = int(seg[-1]) + ROWS_TRAIL
    a = (mu + torch.randn(m, lda, device=device, generator=gen))[:, a0:a0 + k]
    b = torch.randn(3, n, k, device=device, generator=gen) if trans_b else torch.randn(3, k, n, device=device, generator=gen)
    if mu:
        b = cancelling(b, 2 if trans_b else 1)
    c_table = torch.full((m, ldc), SENTINEL, device=device)
    return NS(mode=1, seg=seg, a=a, b=b, k=k, n=n, trans_b=trans_b, b_period=3, c_table=c_table, c0=c0, beta=0.0,
              max_len=max(ROWS_LENGTHS), what=f"grouped rows k {k} n {n} trans_b {int(trans_b)} mu {mu:g}")


def grouped_rows_f32(case, neighbour_of=None):
    """torch's float32 on the case's device (the host test's stand-in for the kernel).  neighbour_of: a planted fault --
    that segment takes the next group's B block"""
    table = case.c_table.clone()
    c = table[:, case.c0:case.c0 + case.n]
    for g, rows, am, bm in A.grouped_blocks(1, case.seg, case.a, case.b, case.trans_b, case.b_period):
        if g == neighbour_of:
            blk = case.b[(g + 1) % case.b_period]
            bm = blk.t() if case.trans_b else blk
        c[rows] = am @ bm
    return table


def check_grouped_rows(lines, case, table):
    c = table[:, case.c0:case.c0 + case.n]
    args = (1, case.seg, case.a, case.b, None, 0.0, case.trans_b, case.b_period)
    want, scale, ref32 = A.grouped_eval(*args, torch.float64), A.grouped_scale(*args), A.grouped_eval(*args, torch.float32)
    touched = torch.zeros(table.shape, dtype=torch.bool, device=table.device)
    for g, rows, am, bm in A.grouped_blocks(*args[:4], *args[6:]):
        touched[rows, case.c0:case.c0 + case.n] = True
        if rows.stop > rows.start:
            check_reduction(lines, f"{case.what} segment {g} ({rows.stop - rows.start} rows from {rows.start})", c[rows],
                            want[g], scale[g], ref32[g], "f32_mfma", case.k)
    # rows in no segment and the columns beside the slice keep the sentinel, bit for bit
    assert torch.equal(table[~touched], torch.full_like(table[~touched], SENTINEL)), f"{case.what}: wrote outside its segments"


def draw_grouped_k(device, m, n, beta, mu=0.0, seed=0):
    gen = gen_for(device, 2000 + seed + m + n)
    seg = seg_of(K_START, K_LENGTHS, device)
    rows = int(seg[-1]) + K_TRAIL
    a = mu + torch.randn(rows, m, device=device, generator=gen)           # A^T, k-major
    b = torch.randn(rows, n, device=device, generator=gen)
    if mu:
        b = cancelling(b, 0)
    c0 = torch.randn(len(K_LENGTHS), m + 2, n, device=device, generator=gen)      # stride_c = (m + 2) n: two guard rows per block
    return NS(mode=2, seg=seg, a=a, b=b, m=m, n=n, beta=beta, c0=c0, rows=rows,
              what=f"grouped k m {m} n {n} beta {beta:g} mu {mu:g}")


def grouped_k_f32(case):
    out = case.c0.clone()
    for g, rows, am, bm in A.grouped_blocks(2, case.seg, case.a, case.b, False, 0):
        out[g, :case.m] = am @ bm + (case.beta * case.c0[g, :case.m] if case.beta else 0.0)
    return out


def check_grouped_k(lines, case, out):
    c0 = case.c0[:, :case.m]
    args = (2, case.seg, case.a, case.b, c0, case.beta, False, 0)
    want, scale, ref32 = A.grouped_eval(*args, torch.float64), A.grouped_scale(*args), A.grouped_eval(*args, torch.float32)
    for g, rows, am, bm in A.grouped_blocks(2, case.seg, case.a, case.b, False, 0):
        length = rows.stop - rows.start
        if length == 0:     # an empty segment: exactly beta * C0
            assert torch.equal(out[g, :case.m], case.beta * c0[g]), f"{case.what}: empty segment {g} is not beta * C0"
            continue
        check_reduction(lines, f"{case.what} segment {g} ({length} rows)", out[g, :case.m], want[g], scale[g], ref32[g],
                        "f32_mfma", length)
    assert torch.equal(out[:, case.m:], case.c0[:, case.m:]), f"{case.what}: wrote between the blocks (stride_c)"


# =============================================================================================== (b) element-wise row walkers
ALPHA, BETA, SLOPE, MIX = 0.3, -1.7, 0.01, 0.1
GATE_G = (0.2499, -0.2499, 0.25, -0.25, 0.2501, -0.2501, 0.26, 9.99, 10.5, -10.5, 30.0, -30.0)
GATE_Z = (30.0, -30.0, 90.0, -90.0, 80.5, -80.5, 79.5, 17.0, -17.0)


def draw_eltwise(device, n, d, offset, seed=0):
    gen = gen_for(device, 3000 + seed + 7 * d + n + int(offset))
    t = lambda s=1.0: table_view(gen, device, n, d, offset, s)
    inp = NS(a=t(), b=t(), h=t(), g1=t(), g2=t(), x=t(), gpre=t(2.0), zpre=t(3.0), go=t(), n=n, d=d, offset=offset)
    # the gate's pre-activations: both sides of tanh_fast's series switch and its clamp at 10; sigmoid_fast's clamp at 80
    # and the saturation of 1 - s
    pos = torch.arange(n * d, device=device).reshape(n, d)
    for k, v in enumerate(GATE_G):
        inp.gpre[pos % 41 == k] = v
    for k, v in enumerate(GATE_Z):
        inp.zpre[pos % 43 == k] = v
    return inp


def eltwise_expected(inp, which=None):
    """name -> (want64, scale64, roundings, extra) of every output of the family"""
    e = {}
    e["axpby"] = A.eltwise_ref(0, inp.a, inp.b, ALPHA, BETA)
    e["axpby.g_a"] = A.eltwise_ref(0, inp.g1, None, ALPHA, 0.0)
    e["axpby.g_b"] = A.eltwise_ref(0, inp.g1, None, BETA, 0.0)
    e["axpb"] = A.eltwise_ref(0, inp.a, None, ALPHA, BETA)
    e["mul"] = A.eltwise_ref(1, inp.a, inp.b, 0, 0)
    e["mul.g_a"] = A.eltwise_ref(1, inp.g1, inp.b, 0, 0)
    e["mul.g_b"] = A.eltwise_ref(1, inp.g1, inp.a, 0, 0)
    e["leaky"] = A.eltwise_ref(2, inp.a, None, SLOPE, 0)
    e["leaky.g_a"] = A.eltwise_ref(3, inp.g1, inp.a, SLOPE, 0)
    e["leaky_sum"] = A.eltwise_ref(2, inp.a, inp.b, SLOPE, 0)
    e["leaky_sum.g_a"] = A.eltwise_ref(3, inp.g1, inp.a, SLOPE, 0)
    e["leaky_sum.g_b"] = A.eltwise_ref(3, inp.g1, inp.b, SLOPE, 0)
    for tag, h in (("bi_mix", None), ("bi_mix_h0", inp.h)):
        for k, v in A.bi_mix_fwd_ref(inp.a, inp.b, h, MIX).items():
            e[f"{tag}.{k}"] = v
        for k, v in A.bi_mix_bwd_ref(inp.a, inp.b, inp.g1, inp.g2, h is not None, MIX).items():
            e[f"{tag}.{k}"] = v
    e["gate"] = A.gate_blend_fwd_ref(inp.x, inp.gpre, inp.zpre)
    for k, v in A.gate_blend_bwd_ref(inp.x, inp.gpre, inp.zpre, inp.go).items():
        e[f"gate.{k}"] = v
    e = {k: (v if len(v) == 4 else v + (None,)) for k, v in e.items()}
    return e if which is None else {k: v for k, v in e.items() if k in which}


def rnd(x64):
    """one float32 rounding of a float64 value (the host stand-in evaluates the kernels' expressions rounding by rounding)"""
    return x64.float().double()


def eltwise_f32(inp, tanh=torch.tanh):
    """The kernels' expressions with float32 roundings where the kernels round (fmaf = one rounding of the exact product
    and sum), on the case's device: the host test's stand-in.  tanh: a planted fault"""
    D = lambda t: t.double()
    al, be, sl, mx = A.f32(ALPHA), A.f32(BETA), A.f32(SLOPE), A.f32(MIX)
    a, b, h, g1, g2 = D(inp.a), D(inp.b), D(inp.h), D(inp.g1), D(inp.g2)
    lk = lambda v: torch.where(v > 0, v, rnd(sl * v))
    dl = lambda g, v: rnd(g * torch.where(v > 0, torch.ones_like(v), torch.full_like(v, sl)))
    o = {"axpby": rnd(al * a + rnd(be * b)), "axpby.g_a": rnd(al * g1), "axpby.g_b": rnd(be * g1), "axpb": rnd(al * a + be),
         "mul": rnd(a * b), "mul.g_a": rnd(g1 * b), "mul.g_b": rnd(g1 * a), "leaky": lk(a), "leaky.g_a": dl(g1, a),
         "leaky_sum": rnd(lk(a) + lk(b)), "leaky_sum.g_a": dl(g1, a), "leaky_sum.g_b": dl(g1, b)}
    c = rnd(torch.tensor(1.0 - mx, dtype=torch.float64))
    for tag, cc, hh in (("bi_mix", 1.0, None), ("bi_mix_h0", c, rnd(mx * h))):
        add = hh if hh is not None else 0.0
        o[f"{tag}.sum"] = rnd(cc * rnd(a + b) + add)
        o[f"{tag}.prod"] = rnd(cc * rnd(a * b) + add)
        o[f"{tag}.g_ego"] = rnd(cc * rnd(g2 * b + g1))
        o[f"{tag}.g_side"] = rnd(cc * rnd(g2 * a + g1))
        if hh is not None:
            o[f"{tag}.g_h0p"] = rnd(mx * rnd(g1 + g2))
    x, go = inp.x.float(), inp.go.float()
    s, t = torch.sigmoid(inp.zpre.float()), tanh(inp.gpre.float())
    o["gate"] = (1 - s) * x + s * t
    o["gate.g_x"] = go * (1 - s)
    o["gate.g_gpre"] = go * s * (1 - t * t)
    o["gate.g_zpre"] = go * (t - x) * s * (1 - s)
    return {k: v.float() for k, v in o.items()}


def check_eltwise(lines, what, got, expected):
    for name, (want, scale, n_units, extra) in expected.items():
        assert name in got, f"{what}: output {name} missing"
        check_units(lines, f"{what} {name}", got[name], want, scale, n_units, extra)


# =============================================================================================== (c) LayerNorm
LN_ROWS = ("mean 1e3 std", "all z < -10", "2^-60", "2^60", "constant", "all z < 0")


def draw_layernorm(device, n, d, offset=False, beta_zero=False, seed=0):
    gen = gen_for(device, 4000 + seed + 3 * d + n + int(offset))
    z = table_view(gen, device, n, d, offset)
    r = lambda: torch.randn(d, device=device, generator=gen)
    z[0] = 1e3 + r()                                   # mean = 1e3 std
    z[1] = -10.0 - 10.0 * r().abs()                    # far behind the negative slope
    z[2] = torch.ldexp(r(), torch.tensor(-60, device=device))
    z[3] = torch.ldexp(r(), torch.tensor(60, device=device))
    z[4] = 1.5                                         # constant: var = 0, rstd = 1 / sqrt(eps); y = beta exactly
    z[5] = -r().abs() - 0.1
    gamma = 1.0 + 0.1 * r()
    beta = torch.zeros(d, device=device) if beta_zero else 0.1 * r()
    gy = table_view(gen, device, n, d, offset)
    gyn = table_view(gen, device, n, d, offset)
    gyn[4] *= 1e-12                                    # (behind g_yn / norm_eps: keeps the column sums on the other rows' scale;
    gyn[2] *= 1e-12                                    #  with beta = 0 the 2^-60 row's |y| is below norm_eps too)
    return NS(z=z, gamma=gamma, beta=beta, gy=gy, gyn=gyn, n=n, d=d, slope=A.f32(SLOPE), eps=A.f32(1e-5), norm_eps=A.f32(1e-12),
              beta_zero=beta_zero, special=True,
              what=f"layernorm n {n} d {d}{' offset' if offset else ''}{' beta 0' if beta_zero else ''}")


def ln_row_groups(case):
    """every special row on its own (its conditioning sets torch's float32 error, hence its bound), the ordinary rows together"""
    if not getattr(case, "special", False):
        return [("", slice(0, case.n))]
    return [(f" row {i} ({w})", slice(i, i + 1)) for i, w in enumerate(LN_ROWS)] + [(" other rows", slice(len(LN_ROWS), case.n))]


def layernorm_fwd_f32(case, mean_over=None):
    return A.layernorm_fwd_eval(case.z, case.gamma, case.beta, case.slope, case.eps, case.norm_eps, torch.float32, mean_over,
                                drop=drop_of(case))


def drop_of(case):
    """the dropout scale per element of a case that has one (test_dropout_mask_gpu.py sets it from the host port), else None"""
    return getattr(case, "drop", None)


def check_layernorm_fwd(lines, case, got):
    """got: {mean, rstd, y, yn} (yn / y may be absent)"""
    args = (case.z, case.gamma, case.beta, case.slope, case.eps, case.norm_eps)
    want, scale = A.layernorm_fwd_eval(*args, torch.float64, drop=drop_of(case)), A.layernorm_fwd_scale(*args, drop=drop_of(case))
    ref32 = layernorm_fwd_f32(case)
    for k in ("mean", "rstd", "y", "yn"):
        if got.get(k) is not None:
            for tag, rows in ln_row_groups(case):
                check_reduction(lines, f"{case.what} {k}{tag}", got[k][rows], want[k][rows], scale[k][rows], ref32[k][rows])
    # the constant row: no variance -- rstd is 1 / sqrt(eps), and with beta = 0 its y and yn are exact zeros
    r_const = 1.0 / math.sqrt(case.eps)
    assert abs(float(got["rstd"][4]) - r_const) <= 2 * U * r_const, (case.what, float(got["rstd"][4]), r_const)
    if case.beta_zero:
        for k in ("y", "yn"):
            if got.get(k) is not None:
                assert float(got[k][4].abs().max()) == 0.0, f"{case.what}: {k} of the constant row is not exactly zero"


def layernorm_bwd_f32(case, mean, rstd, y, use_gy=True, use_gyn=True):
    return A.layernorm_bwd_eval(case.z, case.gamma, mean, rstd, y, case.gy if use_gy else None, case.gyn if use_gyn else None,
                                case.slope, case.norm_eps, torch.float32, drop=drop_of(case))


def check_layernorm_bwd(lines, case, mean, rstd, y, got, use_gy=True, use_gyn=True, only=("gz", "g_gamma", "g_beta")):
    """got: {gz, g_gamma, g_beta}; mean / rstd / y: what the forward kept (the backward kernel's inputs)"""
    args = (case.z, case.gamma, mean, rstd, y, case.gy if use_gy else None, case.gyn if use_gyn else None, case.slope,
            case.norm_eps)
    want, scale = A.layernorm_bwd_eval(*args, torch.float64, drop=drop_of(case)), A.layernorm_bwd_scale(*args, drop=drop_of(case))
    ref32 = A.layernorm_bwd_eval(*args, torch.float32, drop=drop_of(case))
    for k in only:
        for tag, rows in (ln_row_groups(case) if k == "gz" else [("", slice(None))]):
            check_reduction(lines, f"{case.what} {k}{tag}", got[k][rows], want[k][rows], scale[k][rows], ref32[k][rows])


def draw_layernorm_sums(device, n, d, mu, offset=False, seed=0):
    """g_gamma / g_beta under cancellation: an upstream gradient of +-mu + noise over n rows"""
    gen = gen_for(device, 4500 + seed + d + int(mu) % 1000 + int(offset))
    z = table_view(gen, device, n, d, offset)
    r = lambda: torch.randn(d, device=device, generator=gen)
    gamma, beta = 1.0 + 0.1 * r(), 0.1 * r()
    sign = torch.where(torch.rand(n, 1, device=device, generator=gen) < 0.5, -1.0, 1.0)
    gy = table_view(gen, device, n, d, offset)
    gy += sign * mu
    return NS(z=z, gamma=gamma, beta=beta, gy=gy, gyn=None, n=n, d=d, slope=A.f32(SLOPE), eps=A.f32(1e-5), norm_eps=A.f32(1e-12),
              beta_zero=False, what=f"layernorm sums n {n} d {d} mu {mu:g}{' offset' if offset else ''}")


# =============================================================================================== (d) BatchNorm(ReLU)
BN_EPS, BN_MOMENTUM = A.f32(1e-5), A.f32(0.1)


def column_kind(j, shift):
    return {1: "nonpositive", 2: "offset"}.get((j + shift) % 5, "plain")


def draw_batchnorm(device, n, d, shift=0, seed=0):
    gen = gen_for(device, 5000 + seed + 11 * d + n + shift)
    z = torch.randn(n, d, device=device, generator=gen)
    for j in range(d):
        kind = column_kind(j, shift)
        if kind == "nonpositive":
            z[:, j] = -z[:, j].abs()                   # relu = 0 everywhere: variance 0
            z[0, j] = 0.0
        elif kind == "offset":
            z[:, j] += 1e3                             # a common offset of 1e3 std
    r = lambda s=1.0: torch.randn(d, device=device, generator=gen) * s
    return NS(z=z, gamma=1.0 + 0.1 * r(), beta=r(0.1), run_mean=r(), run_var=torch.rand(d, device=device, generator=gen) + 0.5,
              gy=torch.randn(n, d, device=device, generator=gen), n=n, d=d, shift=shift,
              what=f"batchnorm n {n} d {d} shift {shift}")


def bn_column_groups(case):
    kinds = [column_kind(j, case.shift) for j in range(case.d)]
    dev = case.z.device
    return [(f" {k} columns", torch.tensor([j for j, kk in enumerate(kinds) if kk == k], device=dev))
            for k in ("plain", "nonpositive", "offset") if k in kinds]


def batchnorm_fwd_f32(case, training, mean_over=None):
    return A.batchnorm_fwd_eval(case.z, case.gamma, case.beta, case.run_mean, case.run_var, training, BN_MOMENTUM, BN_EPS,
                                torch.float32, mean_over)


def check_batchnorm_fwd(lines, case, training, got):
    """got: {mean, invstd, y, run_mean, run_var}"""
    args = (case.z, case.gamma, case.beta, case.run_mean, case.run_var, training, BN_MOMENTUM, BN_EPS)
    want, scale, ref32 = A.batchnorm_fwd_eval(*args, torch.float64), A.batchnorm_fwd_scale(*args), batchnorm_fwd_f32(case, training)
    mode = "train" if training else "eval"
    for k in ("mean", "invstd", "y", "run_mean", "run_var"):
        for tag, cols in bn_column_groups(case):
            check_reduction(lines, f"{case.what} {mode} {k}{tag}", got[k][..., cols], want[k][..., cols], scale[k][..., cols],
                            ref32[k][..., cols])
    if training:
        for j in range(case.d):
            if column_kind(j, case.shift) == "nonpositive":      # variance 0: invstd = 1 / sqrt(eps), y = beta exactly
                assert float(got["mean"][j]) == 0.0 and torch.equal(got["y"][:, j], case.beta[j].expand(case.n)), (case.what, j)


def check_batchnorm_bwd(lines, case, training, mean, invstd, got):
    args = (case.z, case.gamma, mean, invstd, case.gy, training)
    want, scale = A.batchnorm_bwd_eval(*args, torch.float64), A.batchnorm_bwd_scale(*args)
    ref32 = A.batchnorm_bwd_eval(*args, torch.float32)
    mode = "train" if training else "eval"
    for k in ("gz", "g_gamma", "g_beta"):
        for tag, cols in bn_column_groups(case):
            check_reduction(lines, f"{case.what} {mode} {k}{tag}", got[k][..., cols], want[k][..., cols], scale[k][..., cols],
                            ref32[k][..., cols])


# =============================================================================================== graphs (SpMM, attention)
def rand_graph(rng, n, e, n_rel=5, long_rows=()):
    """the recipe of test_gpu_parity.rand_graph: skewed head ids, rows 5, 42, 79, ... empty, rows of a given length"""
    h = (n * rng.random(e) ** 1.7).astype(np.int64)
    t = rng.integers(0, n, e)
    r = rng.integers(0, n_rel, e)
    for row, deg in long_rows:
        h = np.concatenate([h, np.full(deg, row)])
        t = np.concatenate([t, rng.choice(n, deg, replace=deg > n)])
        r = np.concatenate([r, rng.integers(0, n_rel, deg)])
    trip = np.unique(np.stack([h, r, t], 1), axis=0)
    trip = trip[(trip[:, 0] % 37) != 5]
    trip = trip[rng.permutation(len(trip))]
    return trip[:, 0].copy(), trip[:, 2].copy(), trip[:, 1].copy()


def csr_of(n, h, t, r, device):
    """Plain numpy CSR of the triples, entries sorted by (row, col), one stored entry per (h, t) pair with its raw edges'
    relations behind eptr -- the layout of KGStructure, for the host test (the device tests take KGStructure's own)"""
    order = np.lexsort((r, t, h))
    h, t, r = h[order], t[order], r[order]
    key = h * n + t
    first = np.concatenate([[True], key[1:] != key[:-1]])
    rowptr = np.zeros(n + 1, np.int64)
    np.add.at(rowptr, h[first] + 1, 1)
    eptr = np.flatnonzero(np.concatenate([first, [True]]))
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x).astype(np.int32)).to(device)
    return NS(n=n, nnz=int(first.sum()), rowptr=T(np.cumsum(rowptr)), col=T(t[first]), eptr=T(eptr), rel=T(r))


# =============================================================================================== (f) SpMM
SPMM_DRAWS = ("mixed", "common 1e3", "2^-100 / 2^100", "val 2^-140")


def spmm_graph(seed=0, n=700, e=6000, long_rows=((3, 65), (10, 200), (501, 640))):
    return (n,) + rand_graph(np.random.default_rng(6000 + seed), n, e, long_rows=long_rows)


def draw_spmm(device, n, nnz, d, draw, offset=False, seed=0):
    gen = gen_for(device, 6100 + seed + d + SPMM_DRAWS.index(draw))
    val = torch.randn(nnz, device=device, generator=gen)                  # mixed signs
    x = table_view(gen, device, n, d, offset)
    if draw == "common 1e3":
        x += 1e3
    elif draw == "2^-100 / 2^100":
        ex = torch.tensor([-100, 0, 100], dtype=torch.int32, device=device)[torch.arange(n, device=device) % 3]
        x.copy_(torch.ldexp(x, ex[:, None]))
    elif draw == "val 2^-140":
        val[::5] = 2.0 ** -140
    t = lambda: table_view(gen, device, n, d, offset)
    return NS(val=val, x=x, add_self=t(), add2=t(), bias=torch.randn(d, device=device, generator=gen), n=n, d=d,
              what=f"spmm d {d} {draw}{' offset' if offset else ''}")


def check_spmm(lines, what, rowptr, col, val, x, n_rows, got, **epi):
    want = A.spmm_eval(rowptr, col, val, x, n_rows, torch.float64, **epi)
    scale = A.spmm_eval(rowptr, col, val, x, n_rows, torch.float64, absolute=True, **epi)
    ref32 = A.spmm_eval(rowptr, col, val, x, n_rows, torch.float32, **epi)
    # (a row made of 2^-140 values alone is a subnormal: float32 rounds it to 2^-150, i.e. 2^-24 of 2^-126, not of the row)
    check_reduction(lines, what, got, want, scale.clamp_min(2.0 ** -126), ref32)


# =============================================================================================== (e) attention refresh
ATT_DRAWS = ("small", "small + 0.26", "3 randn")


def attention_graph(long_threshold, seed=0, n=800, e=5000, n_rel=3):
    """test_attention_refresh_random's recipe (duplicate (h, t) pairs, some tripled) with rows of 1, 63, 64, 65, the long-row
    threshold, one more, and 700 entries (row 5 stays empty); 800 entities, so that a row can hold 700 distinct tails"""
    rng = np.random.default_rng(7000 + seed)
    lens = ((11, 1), (12, 63), (13, 64), (14, 65), (15, long_threshold), (16, long_threshold + 1), (17, 700))
    h, t, r = rand_graph(rng, n, e, n_rel=n_rel, long_rows=())
    keep = ~np.isin(h, [row for row, _ in lens])
    h, t, r = h[keep], t[keep], r[keep]
    for row, deg in lens:                       # exactly deg distinct tails (n_rel relations over them: no duplicates here)
        tails = rng.choice(n, deg, replace=False)
        h = np.concatenate([h, np.full(deg, row)])
        t = np.concatenate([t, tails])
        r = np.concatenate([r, rng.integers(0, n_rel, deg)])
    if n_rel > 1:
        extra = np.stack([h[:40], (r[:40] + 1) % n_rel, t[:40]], 1)
        extra2 = np.stack([h[:10], (r[:10] + 2) % n_rel, t[:10]], 1) if n_rel > 2 else extra[:0]
        trip = np.unique(np.concatenate([np.stack([h, r, t], 1), extra, extra2]), axis=0)
        h, r, t = trip[:, 0].copy(), trip[:, 1].copy(), trip[:, 2].copy()
    return n, h, t, r, dict(lens)


def draw_attention(device, n, n_rel, d, draw, offset=False, seed=0):
    gen = gen_for(device, 7100 + seed + d + 13 * n_rel + ATT_DRAWS.index(draw))
    if draw == "3 randn":       # saturation, values past tanh_fast's clamp at 10, logit spreads over 100
        ent = table_view(gen, device, n, d, offset, 3.0)
        rel = table_view(gen, device, n_rel, d, offset, 3.0)
    else:                       # every |h + r| < 0.2: the series side of the wave ballot ...
        ent = ((torch.rand(n, d + 3, device=device, generator=gen) - 0.5) * 0.2)
        rel = ((torch.rand(n_rel, d + 3, device=device, generator=gen) - 0.5) * 0.2)
        ent, rel = (ent[:, 1:1 + d], rel[:, 1:1 + d]) if offset else (ent[:, :d].contiguous(), rel[:, :d].contiguous())
        if draw == "small + 0.26":      # ... with one coordinate of every 64th entity at 0.26 (relation 0 adds nothing there)
            ent[::64, (d - 1) // 2] = 0.26
            rel[:, (d - 1) // 2] = 0.0
    return NS(ent=ent, rel=rel, d=d, n=n, what=f"attention d {d} n_rel {n_rel} {draw}{' offset' if offset else ''}")


def check_attention(lines, what, g, ent, rel, val, logits, vec, row_lo=0, row_hi=None):
    """g: rowptr / col / eptr / rel of the structure; val / logits: the refresh's outputs over entries of rows [row_lo, row_hi)"""
    row_hi = g.n if row_hi is None else row_hi
    rp = g.rowptr.long()
    e_lo, e_hi = int(rp[row_lo]), int(rp[row_hi])
    want, scale, allow = A.attention_logits_eval(g.rowptr, g.col, g.eptr, g.rel, ent, rel, torch.float64)
    assert finite(want), f"{what}: the float64 logits are not finite"
    sl = slice(e_lo, e_hi)
    check_units(lines, f"{what} logits", logits[sl], want[sl], scale[sl], A.attention_logit_units(vec), allow[sl])
    # the softmax stage on its own: against float64 over the logits the kernel itself returned
    n_rows = row_hi - row_lo
    want_v, spread = A.row_softmax_eval(g.rowptr[row_lo:], logits, n_rows, torch.float64)
    ref32, _ = A.row_softmax_eval(g.rowptr[row_lo:], logits, n_rows, torch.float32)
    assert finite(want_v) and finite(ref32), f"{what}: softmax reference not finite"
    q, i = A.softmax_excess(val[sl], want_v, ref32, spread)
    lines.append((f"{what} values", q, 1.0))
    assert q <= 1.0, (f"{what}: softmax value {i} off by {q:.3g} x its allowance: got {val[sl][i].item()!r}, x64 "
                      f"{want_v[i].item()!r}, l - max {spread[i].item()!r}")
    # an underflowed value is exactly what float64 rounds to
    under = want_v < 2.0 ** -152
    assert float(val[sl][under].abs().max() if bool(under.any()) else 0.0) == 0.0, f"{what}: an underflowed value is not zero"
    return spread


# =============================================================================================== (g) scores and losses
def draw_triples(device, form, dim, b, group=1, offset=False, seed=0, n_rel=3):
    """Trained-like tables: a small pool of heads (ids repeated hundreds of times at b = 1025); for every (h, r) a tail whose
    row is h + r + 1e-3 noise; far rows at a distance^2 of 50 .. 250, so that neg - pos reaches +-90.  A third of the triples
    has the near tail as t+ (neg - pos >> 0), a third as t- (<< 0), the rest two far rows.  form: transe | dot | transr
    (rows are then the PROJECTED rows' stand-ins: the caller projects with identity-like matrices)"""
    gen = gen_for(device, 8000 + seed + dim + 3 * b + group + int(offset))
    n_heads, n_far = 4, 40
    n_ent = n_heads + n_heads * n_rel + n_far
    emb = table_view(gen, device, n_ent, dim, offset)
    rel = table_view(gen, device, n_rel, dim, offset, 0.5)
    far0 = n_heads + n_heads * n_rel
    emb[far0:] *= torch.sqrt((50.0 + 200.0 * torch.rand(n_far, 1, device=device, generator=gen)) / dim)
    if form == "dot":       # dot scores: |h|^2 ~ 120, so that h . (its near tail) - h . (a far row) passes +-90
        emb[:n_heads] *= math.sqrt(120.0 / dim)
    for hh in range(n_heads):
        for rr in range(n_rel):
            noise = 1e-3 * torch.randn(dim, device=device, generator=gen)
            emb[n_heads + hh * n_rel + rr] = emb[hh] + rel[rr] + noise if form != "dot" else emb[hh] * (1.0 + noise)
    n_g = b // group
    ri = lambda hi, n_: torch.randint(0, hi, (n_,), device=device, generator=gen)
    h, r = ri(n_heads, n_g), ri(n_rel, n_g)
    near = n_heads + h * n_rel + r
    kind = torch.arange(n_g, device=device) % 3
    far_a = far0 + ri(n_far, n_g)
    pos_t = torch.where(kind == 0, near, far_a)
    h, r, pos_t, kind_b, near_b = (v.repeat_interleave(group) for v in (h, r, pos_t, kind, near))
    far_b = far0 + ri(n_far, n_g * group)
    neg_t = torch.where(kind_b == 1, near_b, far_b)
    return NS(emb=emb, rel=rel, h=h, r=r, pos_t=pos_t, neg_t=neg_t, lam=A.f32(1e-2), n_ent=n_ent, n_rel=n_rel, dim=dim,
              b=n_g * group, group=group, form=form,
              what=f"{form} dim {dim} b {n_g * group}{f' group {group}' if group > 1 else ''}{' offset' if offset else ''}")


def check_scores(lines, case, rows, got, g_loss=1.0):
    """rows: (eh, er, ep, en) per triple (er None for dot) -- the float32 rows the score kernels read.
    got: {pos, neg, reg, rank, loss} and the gradients {g_h, g_r, g_p, g_n} per TABLE row (scattered) or per triple.
    Returns nothing; the kernels' own pos / neg (their backward's inputs) carry the gradient references."""
    eh, er, ep, en = rows
    dot = er is None
    ev = (lambda dt: A.dot_scores_eval(eh, ep, en, dt)) if dot else (lambda dt: A.trans_scores_eval(eh, er, ep, en, dt))
    (want, scale), (ref32, _) = ev(torch.float64), ev(torch.float32)
    for k in ("pos", "neg", "reg"):
        check_reduction(lines, f"{case.what} {k}", got[k], want[k], scale[k], ref32[k])
    # rank = -logsigmoid(margin) from the kernel's own pos / neg: finite, and softplus in both tails
    margin = (got["pos"] - got["neg"]) if dot else (got["neg"] - got["pos"])
    rk, rk_s = A.rank_eval(margin, torch.float64)
    assert finite(got["rank"]), f"{case.what}: rank is not finite"
    check_reduction(lines, f"{case.what} rank", got["rank"], rk, rk_s, A.rank_eval(margin, torch.float32)[0])
    ls, ls_s = A.loss_eval(got["rank"], got["reg"], case.lam, torch.float64)
    check_reduction(lines, f"{case.what} loss", got["loss"].reshape(1), ls.reshape(1), ls_s.reshape(1),
                    A.loss_eval(got["rank"], got["reg"], case.lam, torch.float32)[0].reshape(1))
    return float(margin.min()), float(margin.max())


def triple_grads(case, rows, pos, neg, dtype, g_loss=1.0, sigmoid=torch.sigmoid):
    eh, er, ep, en = rows
    if er is None:
        return A.dot_grads_eval(eh, ep, en, pos, neg, case.lam, g_loss, dtype, sigmoid)
    return A.trans_grads_eval(eh, er, ep, en, pos, neg, case.lam, g_loss, dtype, sigmoid)


def check_table_grads(lines, case, rows, pos, neg, got_emb, got_rel):
    """TransE / dot: the gradient rows scattered into the entity table (h, t+, t-) and the relation table"""
    v64, s64, al = triple_grads(case, rows, pos, neg, torch.float64)
    v32, _, _ = triple_grads(case, rows, pos, neg, torch.float32)
    ids = dict(h=case.h, p=case.pos_t, n=case.neg_t)
    sc = lambda d_, dt: A.scatter_rows(case.n_ent, [(ids[k], d_[k]) for k in ("h", "p", "n")], dt)
    check_reduction(lines, f"{case.what} g_emb", got_emb, sc(v64, torch.float64), sc(s64, torch.float64), sc(v32, torch.float32),
                    extra=sc(al, torch.float64))
    if got_rel is not None:
        sr = lambda d_, dt: A.scatter_rows(case.n_rel, [(case.r, d_["r"])], dt)
        check_reduction(lines, f"{case.what} g_rel", got_rel, sr(v64, torch.float64), sr(s64, torch.float64), sr(v32, torch.float32),
                        extra=sr(al, torch.float64))
