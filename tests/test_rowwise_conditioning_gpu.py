"""The row-wise, sparse and grouped kernels, each against float64 per ELEMENT on operands chosen to break it (the references,
scales and bounds are op_audit.py's, the draws and checks rowwise_cases.py's -- the same ones test_rowwise_measures_host.py
shows to tell a wrong kernel from a right one on the CPU).

Which case enters which dispatch branch (from the kernels' dispatch code):

  lkg_grouped_gemm_f32 (lkg_gemm.hip: run() on 128 x 128 x 16 tiles; 16-byte loads need ld % 4 == 0, an aligned base, a full tile)
    rows mode, trans_b 0 / 1          test_grouped_rows: (k, n) = (33, 70) partial tiles only; (300, 256) two n tiles, A at
                                      ld 303 one float in (guarded loads); (64, 520) five n tiles, aligned, full k tiles
    segment inside a 128-row tile     lengths 1, 127, 128, 129, 300 (3 m tiles), 0; starts 3, 131, 259, 690 (% 4 != 0)
    b_period                          9 groups over 3 blocks
    k mode, beta 0 / 1, stride_c      test_grouped_k: segments 0, 1, 15, 16 (one k tile), 17, 2000 (125 k tiles)
  lkg_eltwise_f32 / lkg_bi_mix_* / lkg_gate_blend_* (lkg_rowwise.hip: vec = d % 4 == 0 and every ld % 4 == 0 and aligned;
  log_threads_per_row(units) = ceil(log2(units)) capped at 8, units = d / 4 (vec) or d; blocks capped at 8192)
    vec, log_tpr 0 1 3 5 6 7 8        test_elementwise[aligned] d = 4, (8: none), 20 -> 3, 32 -> 3, 100 -> 5, 256 -> 6, 300 -> 7, 1024 -> 8
    vec, two column passes            d = 1028 (257 units > 256 threads)
    scalar (d % 4 != 0)               d = 1, 3 (log_tpr 0, 2)
    scalar (offset views)             test_elementwise[offset] every d; log_tpr 0 .. 8; two passes at d >= 257 (300), five at 1024 / 1028
    grid-stride row loop              test_elementwise_grid_stride: d = 1024, n = 8192 + 3 (1 row per block);
                                      d = 32, n = 8192 * 32 + 3 (32 rows per block)
    pre_rowmax                        test_elementwise_grid_stride and test_elementwise (lkg_gate_blend_bwd_f32 called with it)
  lkg_act_layernorm_fwd_f32           vec and d <= 128: act_ln_fwd_narrow_kernel LPR 8 (d 32), 32 (d 100); else act_ln_fwd_kernel
                                      <4, 2> (d 300), <1, 1> / <1, 2> (offset d 32 / 100)
  lkg_act_layernorm_bwd_f32           vec, d <= 128, n >= 4096: act_ln_bwd_narrow_kernel (n = 4099, 300 001; d 32, 100); else
                                      act_ln_bwd_kernel (n = 257 every d; offset views; d 300)
  lkg_narrow_layer_bwd_f32            ops.narrow_layer_ok: d = 32, n >= 4096 (n = 4099, 300 001)
  lkg_relu_batchnorm_*                one workgroup per 64 columns: d = 1, 63, 64, 65 (2 workgroups), 200 (4); 4 row chains: n = 2
                                      (two empty), 5, 257, 8195
  lkg_edge_softmax_f32 (lkg_attention.hip dispatch<V>: LPE by nchunk; RLDS when n_rel * nchunk * chunk_bytes <= 16 KB)
    float4 LPE 8 / 16 / 32 / 64       d = 4, 32 (8), 64 (16), 68 (32), 128 (32), 260 (CPL 2), 516 (CPL 3), 772 / 1024 (CPL 4, U 1)
    float  LPE 8 / 32 / 64 CPL 2      d = 1, 30, 100 (ld % 4 != 0)
    RLDS on / off                     n_rel = 3 and the smallest n_rel with n_rel * d * 4 > 16 KB (none below 2 at d >= 2052)
    in-register rows / parked / team  rows of 1, 63, 64 | 65, LONG_ROW_THRESHOLD | LONG_ROW_THRESHOLD + 1, 700
    DUPS (extra_relations_kernel)     the duplicated and tripled (h, t) pairs; test_attention_row_range with row_lo > 0
    tanh_dot's wave ballot            draws "small" (series), "small + 0.26" (one lane over), "3 randn" (exp branch, clamp)
  lkg_spmm_csr_fused_f32 (lkg_spmm.hip dispatch<V>: nchunk <= 8 several rows per wave; else wave per row LPE 16 / 32 / 64;
  slabs of 128 (vec) / 256 (scalar) columns; rows over LONG_ROW_THRESHOLD on team workgroups)
    float  grouped / LPE 16..64       d = 1, 5 (grouped), 100 offset (CPL 2), 300 offset (256 + 44)
    float4 grouped                    d = 8, 32
    float4 wave per row               d = 64 (16), 100 (32), 256 (2 equal slabs), 300 (128 + 128 + 44), 1028 (8 slabs + 4)
    team workgroups                   long_rows = g.long_rows() (row 501: 640 entries)
    epilogues                         add_self, add2, bias, rowmax, row lists, x_rows (+ out_rows on the 16-byte path)
  lkg_transe_score_* / lkg_dot_score_* / lkg_dense_score_* / lkg_loss_reduce_f32 (lkg_score.hip: vec_ok)
    VEC / scalar                      dim = 32, 100, 300 | dim = 3 and the offset tables
    loss_reduce, > 1 element / thread b = 1025 (1029 with groups of 7)
    score_bwd_grouped_kernel          transr with group = 7

Every case asserts that its float64 reference and torch's float32 result are finite wherever an output is compared."""
import math

import numpy as np
import pytest
import torch

import op_audit as A
import rowwise_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(gpu_device):
    import __graft_entry__ as ge
    ge.build()
    from literalkg_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def N(ops):
    from literalkg_amd import _native
    return _native


def show(lines, limit=None):
    print(C.report(lines, limit))


def leaf(t):
    return t.detach().requires_grad_()


# =============================================================================================== (a) grouped GEMM
def run_grouped_rows(ops, case, max_len):
    table = case.c_table.clone()
    c = table[:, case.c0:case.c0 + case.n]
    ops._grouped(1, case.seg, max_len, case.a, case.b, c, 0, case.n, case.k, False, case.trans_b, 0.0,
                 stride_b=case.b.stride(0), b_period=case.b_period)
    return table


@pytest.mark.parametrize("mu", [0.0, 1e3])
@pytest.mark.parametrize("trans_b", [False, True])
@pytest.mark.parametrize("k,n", [(33, 70), (300, 256), (64, 520)])
def test_grouped_rows(ops, gpu_device, k, n, trans_b, mu):
    """Rows mode (the TransR projections and their data gradient): each segment against its own B block, the rows of no
    segment and the columns beside the slice untouched, a larger max_seg_len changes no bit; mu: rows sharing a large
    common part that the B block cancels."""
    case = C.draw_grouped_rows(gpu_device, k, n, trans_b, mu)
    assert case.a.stride(0) > k and case.c_table.shape[1] > n
    lines = []
    table = run_grouped_rows(ops, case, case.max_len)
    C.check_grouped_rows(lines, case, table)
    assert torch.equal(run_grouped_rows(ops, case, case.max_len + 77), table)
    show(lines)


def run_grouped_k(ops, case):
    out = case.c0.clone()
    ops._grouped(2, case.seg, case.rows, case.a, case.b, out[:, :case.m], case.m, case.n, 0, True, False, case.beta,
                 stride_c=out.stride(0))
    return out


@pytest.mark.parametrize("mu", [0.0, 1e3])
@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("m,n", [(40, 24), (300, 256)])
def test_grouped_k(ops, gpu_device, m, n, beta, mu):
    """k mode (g_W[r] = X_r^T G_r): segments of 0 .. 2000 rows, accumulation onto C0, blocks stride_c apart."""
    case = C.draw_grouped_k(gpu_device, m, n, beta, mu)
    lines = []
    C.check_grouped_k(lines, case, run_grouped_k(ops, case))
    show(lines)


# =============================================================================================== (b) element-wise row walkers
WIDTHS = [1, 3, 4, 20, 32, 100, 256, 300, 1024, 1028]


def gate_bwd_native(ops, N, inp, n_guard=0):
    """lkg_gate_blend_bwd_f32 with the row maxima it can return; outputs with n_guard sentinel rows behind them"""
    n, d = inp.n, inp.d
    x, g, z, go = (ops._f32_rows(t) for t in (inp.x, inp.gpre, inp.zpre, inp.go))
    outs = [torch.full((n + n_guard, d), C.SENTINEL, device=x.device) for _ in range(3)]
    rm = torch.full((n + n_guard,), C.SENTINEL, device=x.device)
    N.call("lkg_gate_blend_bwd_f32", n, d, N.ptr(x), ops._ld(x), N.ptr(g), ops._ld(g), N.ptr(z), ops._ld(z), N.ptr(go),
           ops._ld(go), N.ptr(outs[0]), d, N.ptr(outs[1]), d, N.ptr(outs[2]), d, 0, N.ptr(rm), ops._stream())
    return outs, rm


def run_eltwise(ops, N, inp):
    o = {}
    a, b = leaf(inp.a), leaf(inp.b)
    o["axpby"] = ops.axpby(a, b, C.ALPHA, C.BETA)
    o["axpby.g_a"], o["axpby.g_b"] = torch.autograd.grad(o["axpby"], (a, b), inp.g1)
    o["axpb"] = ops.axpby(a, None, C.ALPHA, C.BETA)
    o["mul"] = ops.mul(a, b)
    o["mul.g_a"], o["mul.g_b"] = torch.autograd.grad(o["mul"], (a, b), inp.g1)
    o["leaky"] = ops.leaky_relu(a, C.SLOPE)
    o["leaky.g_a"], = torch.autograd.grad(o["leaky"], (a,), inp.g1)
    o["leaky_sum"] = ops.leaky_relu_sum(a, b, C.SLOPE)
    o["leaky_sum.g_a"], o["leaky_sum.g_b"] = torch.autograd.grad(o["leaky_sum"], (a, b), inp.g1)
    for tag, h in (("bi_mix", None), ("bi_mix_h0", leaf(inp.h))):
        s, p = ops.bi_mix(a, b, h, C.MIX)
        o[f"{tag}.sum"], o[f"{tag}.prod"] = s, p
        gr = torch.autograd.grad((s, p), (a, b) + ((h,) if h is not None else ()), (inp.g1, inp.g2))
        o[f"{tag}.g_ego"], o[f"{tag}.g_side"] = gr[0], gr[1]
        if h is not None:
            o[f"{tag}.g_h0p"] = gr[2]
    x, g, z = leaf(inp.x), leaf(inp.gpre), leaf(inp.zpre)
    o["gate"] = ops.gate_blend(x, g, z)
    o["gate.g_x"], o["gate.g_gpre"], o["gate.g_zpre"] = torch.autograd.grad(o["gate"], (x, g, z), inp.go)
    return {k: v.detach() for k, v in o.items()}


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset"])
@pytest.mark.parametrize("d", WIDTHS)
def test_elementwise(ops, N, gpu_device, d, offset):
    """ops.axpby / mul / leaky_relu / leaky_relu_sum / bi_mix / gate_blend, forward and backward, at n = 257: each output
    within the counted roundings of its expression (and the allowances of tanh_fast / sigmoid_fast through the gate)."""
    inp = C.draw_eltwise(gpu_device, 257, d, offset)
    assert (inp.a.data_ptr() % 16 != 0) == offset
    lines = []
    C.check_eltwise(lines, f"d {d}", run_eltwise(ops, N, inp), C.eltwise_expected(inp))
    # the row maxima lkg_gate_blend_bwd_f32 returns for the data-gradient product: exact over what it wrote
    (gx, gg, gz), rm = gate_bwd_native(ops, N, inp)
    assert torch.equal(rm, torch.maximum(gg.abs().amax(1), gz.abs().amax(1)))
    show(lines)


@pytest.mark.parametrize("d,n", [(1024, 8192 + 3), (32, 8192 * 32 + 3)])
def test_elementwise_grid_stride(ops, N, gpu_device, d, n):
    """More rows than 8192 workgroups cover in one pass: the grid-stride loop's second pass writes the last rows, and a
    guard row behind every output stays untouched."""
    inp = C.draw_eltwise(gpu_device, n, d, False)
    names = ["axpby", "bi_mix_h0.sum", "bi_mix_h0.prod", "bi_mix_h0.g_ego", "bi_mix_h0.g_side", "bi_mix_h0.g_h0p", "gate",
             "gate.g_x", "gate.g_gpre", "gate.g_zpre"]
    exp = C.eltwise_expected(inp, names)
    buf = lambda: torch.full((n + 1, d), C.SENTINEL, device=gpu_device)
    o = {k: buf() for k in names}
    s = ops._stream()
    P = N.ptr
    N.call("lkg_eltwise_f32", 0, n, d, P(inp.a), d, P(inp.b), d, C.ALPHA, C.BETA, P(o["axpby"]), d, s)
    N.call("lkg_bi_mix_fwd_f32", n, d, P(inp.a), d, P(inp.b), d, P(inp.h), d, C.MIX, P(o["bi_mix_h0.sum"]), d,
           P(o["bi_mix_h0.prod"]), d, s)
    N.call("lkg_bi_mix_bwd_f32", n, d, P(inp.a), d, P(inp.b), d, P(inp.g1), d, P(inp.g2), d, 1, C.MIX, P(o["bi_mix_h0.g_ego"]),
           P(o["bi_mix_h0.g_side"]), P(o["bi_mix_h0.g_h0p"]), s)
    ops.gate_blend(inp.x, inp.gpre, inp.zpre, out=o["gate"][:n])
    (o["gate.g_x"], o["gate.g_gpre"], o["gate.g_zpre"]), rm = gate_bwd_native(ops, N, inp, n_guard=1)
    lines = []
    for k in names:
        assert torch.equal(o[k][n], torch.full((d,), C.SENTINEL, device=gpu_device)), f"{k}: the guard row was written"
    C.check_eltwise(lines, f"d {d} n {n}", {k: v[:n] for k, v in o.items()}, exp)
    C.check_eltwise(lines, f"d {d} n {n} last rows", {k: v[n - 3:n] for k, v in o.items()},
                    {k: (w[n - 3:], sc[n - 3:], u_, ex[n - 3:] if ex is not None else None) for k, (w, sc, u_, ex) in exp.items()})
    assert float(rm[n]) == C.SENTINEL
    assert torch.equal(rm[:n], torch.maximum(o["gate.g_gpre"][:n].abs().amax(1), o["gate.g_zpre"][:n].abs().amax(1)))
    show(lines)


# =============================================================================================== (c) LayerNorm
def run_layernorm(ops, case, narrow, use_gy=True, use_gyn=True):
    """(forward outputs, the kept mean / rstd / y, backward outputs) of ops.act_layernorm, or of ops.narrow_layer with the
    identity as its weight (the product x @ I is exact: the same z reaches the same row-wise kernels, and the backward is
    lkg_narrow_layer_bwd_f32's)"""
    z, gamma, beta = leaf(case.z), leaf(case.gamma), leaf(case.beta)
    if narrow:
        w = leaf(torch.eye(case.d, device=z.device))
        assert ops.narrow_layer_ok(z, w)
        y, yn = ops.narrow_layer(z, w, None, gamma, beta)
        saved = y.grad_fn.saved_tensors
        assert torch.equal(saved[2], case.z)
        mean, rstd = saved[5], saved[6]
    else:
        y, yn = ops.act_layernorm(z, gamma, beta)
        saved = y.grad_fn.saved_tensors
        mean, rstd = saved[3], saved[4]
    fwd = dict(mean=mean, rstd=rstd, y=y.detach(), yn=yn.detach())
    outs, gos = ((y,) if use_gy else ()) + ((yn,) if use_gyn else ()), ((case.gy,) if use_gy else ()) + ((case.gyn,) if use_gyn else ())
    gz, gg, gb = torch.autograd.grad(outs, (z, gamma, beta) + ((w,) if narrow else ()), gos)[:3]
    return fwd, dict(gz=gz, g_gamma=gg, g_beta=gb)


@pytest.mark.parametrize("beta_zero", [False, True], ids=["beta", "beta0"])
@pytest.mark.parametrize("n,d,offset,narrow", [
    (257, 32, False, False), (257, 100, False, False), (257, 300, False, False), (257, 32, True, False), (257, 100, True, False),
    (4099, 32, False, False), (4099, 100, False, False), (4099, 32, False, True)])
def test_layernorm(ops, gpu_device, n, d, offset, narrow, beta_zero):
    """ops.act_layernorm / ops.narrow_layer on rows with mean = 1e3 std, at 2^-60 and 2^60, a constant row (with beta = 0: y
    exactly zero, the g_yn / eps branch of the backward) and a row behind the negative slope: every output per element."""
    case = C.draw_layernorm(gpu_device, n, d, offset, beta_zero)
    fwd, bwd = run_layernorm(ops, case, narrow)
    lines = []
    C.check_layernorm_fwd(lines, case, fwd)
    C.check_layernorm_bwd(lines, case, fwd["mean"], fwd["rstd"], fwd["y"], bwd)
    show(lines)


@pytest.mark.parametrize("d,offset,narrow", [(32, False, False), (100, False, False), (100, True, False), (32, False, True)])
def test_layernorm_parameter_gradients_under_cancellation(ops, N, gpu_device, d, offset, narrow):
    """g_gamma / g_beta over 300 001 rows of +-mu + noise (test_column_sums_under_cancellation's table): per column against
    float64; the row maxima of g_z that ride along are exact."""
    n = 300_001
    lines = []
    for mu in (1e3, 1e5):
        case = C.draw_layernorm_sums(gpu_device, n, d, mu, offset)
        fwd, bwd = run_layernorm(ops, case, narrow, use_gyn=False)
        C.check_layernorm_bwd(lines, case, fwd["mean"], fwd["rstd"], fwd["y"], bwd, use_gyn=False)
        if not narrow:      # lkg_act_layernorm_bwd_f32 with the row maxima it can return: the same g_z, its exact maxima
            z, gy = ops._f32_rows(case.z), ops._f32_rows(case.gy)
            gz = torch.empty(n, d, device=gpu_device)
            gg, gb, rm = torch.zeros(d, device=gpu_device), torch.zeros(d, device=gpu_device), torch.empty(n, device=gpu_device)
            N.call("lkg_act_layernorm_bwd_f32", n, d, N.ptr(z), ops._ld(z), case.slope, N.ptr(case.gamma), N.ptr(case.beta),
                   N.ptr(fwd["y"]), d, N.ptr(fwd["mean"]), N.ptr(fwd["rstd"]), N.ptr(gy), ops._ld(gy), None, 0, case.norm_eps,
                   N.ptr(gz), d, N.ptr(gg), N.ptr(gb), 0.0, 0, N.ptr(rm), None, 0, None, 0, ops._stream())
            assert torch.equal(gz, bwd["gz"]) and torch.equal(rm, gz.abs().amax(1))
    show(lines)


# =============================================================================================== (d) BatchNorm(ReLU)
def run_batchnorm(ops, case, training):
    bn = torch.nn.BatchNorm1d(case.d, eps=C.BN_EPS, momentum=C.BN_MOMENTUM).to(case.z.device)
    with torch.no_grad():
        bn.weight.copy_(case.gamma)
        bn.bias.copy_(case.beta)
        bn.running_mean.copy_(case.run_mean)
        bn.running_var.copy_(case.run_var)
    bn.train(training)
    z = leaf(case.z)
    y = ops.relu_batchnorm(z, bn)
    _, _, mean, invstd = y.grad_fn.saved_tensors
    gz, gg, gb = torch.autograd.grad(y, (z, bn.weight, bn.bias), case.gy)
    return (dict(mean=mean, invstd=invstd, y=y.detach(), run_mean=bn.running_mean.clone(), run_var=bn.running_var.clone()),
            dict(gz=gz, g_gamma=gg, g_beta=gb))


BN_CASES = [(n, d, 0) for n in (2, 5, 257, 8192 + 3) for d in (1, 63, 64, 65, 200)] + \
           [(n, 1, s) for n in (5, 8192 + 3) for s in (1, 2)]          # (the single column as the all-<= 0 and the offset one)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("n,d,shift", BN_CASES)
def test_relu_batchnorm(ops, gpu_device, n, d, shift, training):
    """ops.relu_batchnorm: outputs, saved statistics, the running buffers after one step and the three gradients, with
    columns that are all <= 0 (variance 0) and columns with a common offset of 1e3 std."""
    case = C.draw_batchnorm(gpu_device, n, d, shift)
    fwd, bwd = run_batchnorm(ops, case, training)
    lines = []
    C.check_batchnorm_fwd(lines, case, training, fwd)
    C.check_batchnorm_bwd(lines, case, training, fwd["mean"], fwd["invstd"], bwd)
    show(lines)


# =============================================================================================== (f) SpMM
@pytest.fixture(scope="module")
def spmm_structure(ops, gpu_device):
    from literalkg_amd.graph import KGStructure
    n, h, t, r = C.spmm_graph()
    g = KGStructure.from_triples(n, h, t, r, device=gpu_device)
    assert g.long_rows(False) is not None and 501 in g.long_rows(False).tolist()
    return g


SPMM_WIDTHS = [(1, False), (5, False), (8, False), (32, False), (64, False), (100, False), (256, False), (300, False),
               (1028, False), (100, True), (300, True)]


@pytest.mark.parametrize("d,offset", SPMM_WIDTHS)
def test_spmm_conditioning(ops, gpu_device, spmm_structure, d, offset):
    """ops.spmm_raw, forward and transpose (through permute_values), with and without the long-row list: mixed-sign values,
    x rows sharing a common part, x at 2^-100 / 2^100, values of 2^-140 next to ordinary ones -- per element over
    sum |val| |x|."""
    g = spmm_structure
    lines = []
    for draw in C.SPMM_DRAWS:
        case = C.draw_spmm(gpu_device, g.n, g.nnz, d, draw, offset)
        val_t = ops.permute_values(case.val, g.t_perm)
        assert torch.equal(val_t, case.val[g.t_perm.long()])
        for tag, rowptr, col, val, lr in (("", g.rowptr, g.col, case.val, g.long_rows(False)),
                                          (" transpose", g.t_rowptr, g.t_col, val_t, g.long_rows(True))):
            for use_long in (False, True):
                got = ops.spmm_raw(rowptr, col, val, case.x, g.n, long_rows=lr if use_long else None)
                C.check_spmm(lines, f"{case.what}{tag}{' long rows' if use_long else ''}", rowptr, col, val, case.x, g.n, got)
    show(lines)


@pytest.mark.parametrize("d,offset", SPMM_WIDTHS)
def test_spmm_epilogues(ops, gpu_device, spmm_structure, d, offset):
    """add_self, add2, bias, rowmax (exact), the row-list form and the x_rows / out_rows flagged forms."""
    g = spmm_structure
    n = g.n
    case = C.draw_spmm(gpu_device, n, g.nnz, d, "mixed", offset, seed=1)
    lr = g.long_rows(False)
    lines = []
    run = lambda **kw: ops.spmm_raw(g.rowptr, g.col, case.val, case.x, n, long_rows=lr, **kw)
    chk = lambda what, got, **epi: C.check_spmm(lines, f"{case.what} {what}", g.rowptr, g.col, case.val, case.x, n, got, **epi)
    chk("add_self", run(add_self=case.add_self), add_self=case.add_self)
    chk("add_self + add2", run(add_self=case.add_self, add2=case.add2), add_self=case.add_self, add2=case.add2)
    chk("bias", run(bias=case.bias), bias=case.bias)
    rm = torch.full((n,), C.SENTINEL, device=gpu_device)
    got = run(add_self=case.add_self, rowmax=rm)
    chk("add_self + rowmax", got, add_self=case.add_self)
    assert torch.equal(rm, got.abs().amax(1))
    cnt = (g.rowptr[1:] - g.rowptr[:-1])
    lists = (torch.nonzero(cnt > 0, as_tuple=True)[0].int(), torch.nonzero(cnt == 0, as_tuple=True)[0].int())
    assert lists[1].numel() > 0
    chk("row lists", run(add_self=case.add_self, bias=case.bias, row_lists=lists), add_self=case.add_self, bias=case.bias)
    # row-sparse x: the unflagged rows hold NaN and must not be read; out_rows marks the rows that got a contribution
    rng = np.random.default_rng(d)
    ids = torch.from_numpy(rng.choice(n, 80, replace=False)).to(gpu_device)
    flags = torch.zeros(n, dtype=torch.uint8, device=gpu_device)
    flags[ids] = 1
    x0 = torch.zeros_like(case.x)
    x0[ids] = case.x[ids]
    junk = torch.full_like(case.x, float("nan"))
    junk[ids] = case.x[ids]
    got = ops.spmm_raw(g.rowptr, g.col, case.val, junk, n, long_rows=lr, x_rows=flags)
    C.check_spmm(lines, f"{case.what} x_rows", g.rowptr, g.col, case.val, x0, n, got)
    got = ops.spmm_raw(g.rowptr, g.col, case.val, junk, n, long_rows=lr, add_self=junk, x_rows=flags, self_rows=flags)
    C.check_spmm(lines, f"{case.what} x_rows + self_rows", g.rowptr, g.col, case.val, x0, n, got, add_self=x0)
    if d % 4 == 0 and not offset and d <= 1024:
        out = torch.zeros(n, d, device=gpu_device)
        marks = torch.full((n,), 9, dtype=torch.uint8, device=gpu_device)
        ops.spmm_raw(g.rowptr, g.col, case.val, junk, n, out=out, long_rows=lr, x_rows=flags, out_rows=marks)
        C.check_spmm(lines, f"{case.what} x_rows + out_rows", g.rowptr, g.col, case.val, x0, n, out)
        reached = A.spmm_eval(g.rowptr, g.col, torch.ones_like(case.val), flags.float()[:, None], n, torch.float64)[:, 0] > 0
        assert bool((marks <= 1).all()) and bool((marks[reached] == 1).all()) and float(out[marks == 0].abs().max()) == 0.0
    show(lines)


# =============================================================================================== (e) attention refresh
ATT_VEC = [4, 32, 64, 68, 128, 260, 516, 772, 1024]
ATT_SCALAR = [1, 30, 100]


def lds_limit_relations(d):
    """the smallest relation count whose table (n_rel x d floats, either path) exceeds REL_LDS_BYTES = 16 KB"""
    return 16 * 1024 // (4 * d) + 1


@pytest.fixture(scope="module")
def att_structures(ops, gpu_device):
    from literalkg_amd.graph import KGStructure, LONG_ROW_THRESHOLD
    cache = {}

    def get(n_rel):
        if n_rel not in cache:
            n, h, t, r, lens = C.attention_graph(LONG_ROW_THRESHOLD, n_rel=n_rel)
            g = KGStructure.from_triples(n, h, t, r, device=gpu_device)
            cnt = (g.rowptr[1:] - g.rowptr[:-1]).tolist()
            assert all(cnt[row] == deg for row, deg in lens.items()) and cnt[5] == 0 and (n_rel < 2 or g.has_dups)
            cache[n_rel] = g
        return cache[n_rel]
    return get


def run_attention(ops, g, case, lines, vec, **kw):
    val, logits = ops.edge_softmax(g, case.ent, case.rel, want_logits=True, **kw)
    view = C.NS(n=g.n, rowptr=g.rowptr, col=g.col, eptr=g.eptr, rel=g.rel)
    return val, logits, C.check_attention(lines, case.what, view, case.ent, case.rel, val, logits, vec,
                                          kw.get("row_lo", 0), kw.get("row_hi"))


@pytest.mark.parametrize("d,offset", [(d, False) for d in ATT_VEC] + [(d, True) for d in ATT_SCALAR])
def test_attention_refresh(ops, gpu_device, att_structures, d, offset):
    """ops.edge_softmax(want_logits=True): the logits within tanh_fast's allowance and their counted roundings, the values
    against the float64 softmax of the kernel's own logits; relation table in LDS and (where one exists) past its limit."""
    vec = not offset
    counts = [3, lds_limit_relations(d)]
    assert 3 * d * 4 <= 16 * 1024 < counts[1] * d * 4 and (counts[1] - 1) * d * 4 <= 16 * 1024
    lines = []
    for n_rel in counts:
        g = att_structures(3)                       # (the relation TABLE has n_rel rows; the edges use the first three)
        for draw in C.ATT_DRAWS:
            case = C.draw_attention(gpu_device, g.n, n_rel, d, draw, offset)
            assert (case.ent.data_ptr() % 16 == 0 and case.ent.stride(0) % 4 == 0 and d % 4 == 0) == vec
            if draw != "3 randn":
                s = (case.ent.abs().max() + case.rel.abs().max()).item()
                assert s < 0.2 or draw == "small + 0.26"
            val, logits, spread = run_attention(ops, g, case, lines, vec)
            if draw == "3 randn" and d >= 64:
                assert float(spread.max()) > 100.0 and bool((val == 0).any())      # values underflow: exact zeros
    show(lines)


def test_attention_row_range(ops, gpu_device, att_structures):
    """A refresh of rows [row_lo, row_hi) with duplicates in range: the same bounds, and every entry outside stays put."""
    g = att_structures(3)
    lo_, hi_ = 9, 300
    rp = g.host("rowptr")
    a, b = int(rp[lo_]), int(rp[hi_])
    assert bool(((g.dup_rows >= lo_) & (g.dup_rows < hi_)).any())
    lines = []
    for d, offset in ((64, False), (30, True)):
        case = C.draw_attention(gpu_device, g.n, 3, d, "3 randn", offset)
        out = torch.full((g.nnz,), C.SENTINEL, device=gpu_device)
        val, logits, _ = run_attention(ops, g, case, lines, not offset, row_lo=lo_, row_hi=hi_, out=out)
        assert val is out or val.data_ptr() == out.data_ptr()
        assert torch.equal(out[:a], torch.full_like(out[:a], C.SENTINEL)) and torch.equal(out[b:], torch.full_like(out[b:], C.SENTINEL))
    show(lines)


# =============================================================================================== (g) scores and losses
def saved_buf(loss, b):
    return next(t for t in loss.grad_fn.saved_tensors if t.dim() == 2 and tuple(t.shape) == (4, b) and t.dtype == torch.float32)


SCORE_SHAPES = [(dim, b, False) for dim in (3, 32, 100, 300) for b in (1, 17, 1025)] + [(32, 1025, True), (100, 17, True)]


@pytest.mark.parametrize("form", ["transe", "dot"])
@pytest.mark.parametrize("dim,b,offset", SCORE_SHAPES)
def test_table_scores_and_losses(ops, gpu_device, form, dim, b, offset):
    """ops.transe_loss / ops.dot_loss on trained-like tables with heavily repeated ids: pos / neg / reg, the rank's softplus
    in both tails, the loss reduction, and every gradient row per element."""
    case = C.draw_triples(gpu_device, form, dim, b, offset=offset)
    emb, rel = leaf(case.emb), leaf(case.rel)
    keep = {}
    if form == "transe":
        loss = ops.transe_loss(emb, rel, case.h, case.r, case.pos_t, case.neg_t, case.lam, keep=keep)
    else:
        loss = ops.dot_loss(emb, case.h, case.pos_t, case.neg_t, case.lam)
    buf = saved_buf(loss, b)
    if keep:
        assert torch.equal(keep["pos"], buf[0]) and torch.equal(keep["neg"], buf[1])
    rows = (case.emb[case.h], case.rel[case.r] if form == "transe" else None, case.emb[case.pos_t], case.emb[case.neg_t])
    lines = []
    lo_, hi_ = C.check_scores(lines, case, rows, dict(pos=buf[0], neg=buf[1], reg=buf[2], rank=buf[3], loss=loss.detach()))
    if b >= 17:
        assert lo_ < -90.0 and hi_ > 90.0, (lo_, hi_)
    grads = torch.autograd.grad(loss, (emb, rel) if form == "transe" else (emb,))
    C.check_table_grads(lines, case, rows, buf[0], buf[1], grads[0], grads[1] if form == "transe" else None)
    show(lines)


@pytest.mark.parametrize("group", [1, 7])
@pytest.mark.parametrize("dim,n_groups", [(dim, g_) for dim in (3, 32, 100, 300) for g_ in (1, 17, 1025)])
def test_transr_scores_and_losses(ops, gpu_device, dim, n_groups, group):
    """ops.transr_loss (group 1 and 7): the dense score kernels on the projected rows the loss itself kept -- pos / neg /
    reg / rank / loss and g_rel per element -- and g_emb / g_W through the grouped products, within the f32-MFMA engine's
    bound over the |.|-sum of the whole chain."""
    if group == 7 and n_groups == 1025:
        n_groups = 147                              # b = 1029: loss_reduce still takes more than one element per thread
    b = n_groups * group
    case = C.draw_triples(gpu_device, "transr", dim, b, group=group)
    gen = C.gen_for(gpu_device, dim + b)
    w = torch.eye(dim, device=gpu_device).repeat(case.n_rel, 1, 1) + 0.01 * torch.randn(case.n_rel, dim, dim, device=gpu_device,
                                                                                       generator=gen)
    relp = torch.stack([case.rel[i] @ w[i] for i in range(case.n_rel)])        # so that h W + r ~ t+ W on the trained triples
    emb, rel, wm = leaf(case.emb), leaf(relp), leaf(w)
    keep = {}
    loss = ops.transr_loss(emb, rel, wm, case.h, case.r, case.pos_t, case.neg_t, case.lam, keep=keep, group=group)
    sv = loss.grad_fn.saved_tensors
    hg, pg, nt, rs, perm, seg, perm_n, seg_n, x, p, buf = sv[3:14]
    n_g = b // group
    ph, pp, pn = p[:n_g], p[n_g:2 * n_g], p[2 * n_g:]
    rep = lambda t: t.repeat_interleave(group, 0)
    rows = (rep(ph), rep(relp[rs]), rep(pp), pn)
    lines = []
    lo_, hi_ = C.check_scores(lines, case, rows, dict(pos=buf[0], neg=buf[1], reg=buf[2], rank=buf[3], loss=loss.detach()))
    if n_g >= 17:
        assert lo_ < -90.0 and hi_ > 90.0, (lo_, hi_)
    assert torch.equal(keep["pos"].sort().values, buf[0].sort().values) and torch.equal(keep["neg"].sort().values, buf[1].sort().values)
    g_emb, g_rel, g_w = torch.autograd.grad(loss, (emb, rel, wm))
    rs_b = rep(rs)
    ids = (rep(hg[perm.long()]), rep(pg[perm.long()]), nt[perm_n.long()])

    def chain(dtype, which):
        """(g_rel, g_emb, g_w) in dtype: values (0), |.|-sums (1) or sigmoid allowances (2) carried through the same maps"""
        v = C.triple_grads(case, rows, buf[0], buf[1], dtype)[which]
        lin = (lambda a_, b_: a_ @ b_) if which == 0 else (lambda a_, b_: a_.abs() @ b_.abs())
        wd, xd = w.to(dtype), x.to(dtype)
        gr = A.scatter_rows(case.n_rel, [(rs_b, v["r"])], dtype)
        ge = torch.zeros(case.n_ent, dim, dtype=dtype, device=gpu_device)
        gw = torch.zeros(case.n_rel, dim, dim, dtype=dtype, device=gpu_device)
        xrows = (rep(xd[:n_g]), rep(xd[n_g:2 * n_g]), xd[2 * n_g:])
        for key, idv, xr in zip(("h", "p", "n"), ids, xrows):
            for r_ in range(case.n_rel):
                m_ = rs_b == r_
                ge.index_add_(0, idv[m_], lin(v[key][m_], wd[r_].t()))
                gw[r_] += lin(xr[m_].t(), v[key][m_])
        return gr, ge, gw
    (r64, e64, w64), (rs_, es_, ws_), (ra_, ea_, wa_) = chain(torch.float64, 0), chain(torch.float64, 1), chain(torch.float64, 2)
    r32, e32, w32 = chain(torch.float32, 0)
    C.check_reduction(lines, f"{case.what} g_rel", g_rel, r64, rs_, r32, extra=ra_)
    k_w = int(torch.bincount(rs_b, minlength=case.n_rel).max()) * 3
    C.check_reduction(lines, f"{case.what} g_emb", g_emb, e64, es_, e32, "f32_mfma", dim, extra=ea_)
    C.check_reduction(lines, f"{case.what} g_W", g_w, w64, ws_, w32, "f32_mfma", k_w, extra=wa_)
    show(lines)
