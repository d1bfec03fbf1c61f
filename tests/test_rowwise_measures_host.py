"""Can the measures of test_rowwise_conditioning_gpu.py tell a wrong kernel from a right one?  For every family, on a small
CPU instance made by the SAME draw functions and judged by the SAME check functions (rowwise_cases.py, op_audit.py):
torch's float32 evaluation passes every bound, and each planted fault -- the last entry of a row dropped, a segment with
its neighbour's B block, a mean over one element too many, tanh by its series outside the series' range, one output off by
8 units of 2^-24 of its scale, a softmax without the maximum subtracted -- fails one.

(tanh's series AT |x| = 0.3 is off by 1.6e-8, a quarter of a float32 rounding of tanh(0.3): no float32 measure can see it,
and a kernel that took the series there would not be wrong.  The planted fault takes the series over the whole draw.)"""
import numpy as np
import pytest
import torch

import op_audit as A
import rowwise_cases as C

CPU = torch.device("cpu")


def rejected(fn, *args, **kw):
    with pytest.raises(AssertionError):
        fn([], *args, **kw)


def bump(t, scale64, n_units=8, want64=None, where=None):
    """One element off by n_units 2^-24 of its scale more than it is: with want64 the element where float32 is furthest from
    float64 already (within ``where``), pushed further the same way -- 8 units more than torch's float32 are over 3 x torch's
    float32 while that is under 4 units; without want64 the element with the largest scale."""
    out = t.clone()
    sc = scale64.reshape(-1).clamp_min(1e-300)
    if want64 is None:
        pick, sign = scale64.reshape(-1).clone(), torch.ones_like(sc)
    else:
        diff = t.reshape(-1).double() - want64.reshape(-1)
        pick, sign = diff.abs() / sc, torch.where(diff < 0, -1.0, 1.0)
    if where is not None:
        pick = torch.where(where.reshape(-1), pick, torch.full_like(pick, -1.0))
    i = int(pick.argmax())
    out.view(-1)[i] = float(t.reshape(-1)[i].double() + sign[i] * n_units * A.U * sc[i])
    assert out.view(-1)[i] != t.reshape(-1)[i]
    return out


def rows_mask(like, rows):
    m = torch.zeros_like(like, dtype=torch.bool)
    m[rows] = True
    return m


def tanh_series(x):
    x2 = x * x
    return x * (1 + x2 * (-1 / 3 + x2 * (2 / 15 + x2 * (-17 / 315 + x2 * 62 / 2835))))


# ------------------------------------------------------------------------------------------------- (a) grouped GEMM
@pytest.mark.parametrize("trans_b", [False, True])
@pytest.mark.parametrize("mu", [0.0, 1e3])
def test_grouped_rows_measure(trans_b, mu):
    case = C.draw_grouped_rows(CPU, 33, 70, trans_b, mu)
    good = C.grouped_rows_f32(case)
    lines = []
    C.check_grouped_rows(lines, case, good)
    assert len(lines) == sum(1 for n_ in C.ROWS_LENGTHS if n_)
    for g in (0, 4, 8):                                              # segments of 1, 129 and 61 rows with block g + 1
        rejected(C.check_grouped_rows, case, C.grouped_rows_f32(case, neighbour_of=g))
    c = slice(case.c0, case.c0 + case.n)
    args = (1, case.seg, case.a, case.b, None, 0.0, case.trans_b, case.b_period)
    scale = A.grouped_scale(*args)[5]
    bad = good.clone()
    bad[388:688, c] = bump(good[388:688, c].contiguous(), scale, 8 if mu == 0 else 64)    # (2 sqrt(33) u = 11.5 units)
    if mu == 0:
        bad[388:688, c] = bump(good[388:688, c].contiguous(), scale, 16)
    rejected(C.check_grouped_rows, case, bad)
    bad = good.clone()
    bad[1, c.start] = 0.0                                            # a row of no segment written
    rejected(C.check_grouped_rows, case, bad)
    bad = good.clone()
    bad[400, c.stop] = 0.0                                           # the column beside the slice written
    rejected(C.check_grouped_rows, case, bad)


@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_grouped_k_measure(beta):
    case = C.draw_grouped_k(CPU, 40, 24, beta)
    good = C.grouped_k_f32(case)
    C.check_grouped_k([], case, good)
    bad = good.clone()
    bad[0, 0, 0] += 1e-3                                             # the empty segment: exactly beta * C0
    rejected(C.check_grouped_k, case, bad)
    bad = good.clone()
    bad[3, :case.m] = case.a[18:34].t() @ case.b[18:34] + beta * case.c0[3, :case.m] - case.a[18:19].t() @ case.b[18:19]
    rejected(C.check_grouped_k, case, bad)                           # a segment that skipped its first row
    bad = good.clone()
    bad[2, case.m] = 0.0                                             # a guard row between the blocks
    rejected(C.check_grouped_k, case, bad)


# ------------------------------------------------------------------------------------------------- (b) element-wise
@pytest.mark.parametrize("d,offset", [(20, False), (33, True)])
def test_elementwise_measure(d, offset):
    inp = C.draw_eltwise(CPU, 37, d, offset)
    exp = C.eltwise_expected(inp)
    good = C.eltwise_f32(inp)
    lines = []
    C.check_eltwise(lines, "f32", good, exp)
    assert len(lines) == len(exp) == 25
    for name, (want, scale, n_units, extra) in exp.items():
        if extra is None:                                            # (the gate's own allowances exceed 8 units: below)
            rejected(C.check_eltwise, name, dict(good, **{name: bump(good[name], scale)}), {name: exp[name]})
    # the series beyond |x| < 0.25: the draw holds |g| up to 30
    series = C.eltwise_f32(inp, tanh=tanh_series)
    for name in ("gate", "gate.g_gpre", "gate.g_zpre"):
        rejected(C.check_eltwise, name, series, {name: exp[name]})
    # a sigmoid that saturates early (clamped at |z| = 10 instead of 80)
    clamped = C.draw_eltwise(CPU, 37, d, offset)
    clamped.zpre = inp.zpre.clamp(-10, 10)
    for name in ("gate", "gate.g_x"):
        rejected(C.check_eltwise, name, C.eltwise_f32(clamped), {name: exp[name]})


# ------------------------------------------------------------------------------------------------- (c) LayerNorm
@pytest.mark.parametrize("d,beta_zero", [(32, False), (100, True)])
def test_layernorm_measure(d, beta_zero):
    case = C.draw_layernorm(CPU, 40, d, beta_zero=beta_zero)
    fwd = C.layernorm_fwd_f32(case)
    C.check_layernorm_fwd([], case, fwd)
    rejected(C.check_layernorm_fwd, case, C.layernorm_fwd_f32(case, mean_over=d + 1))
    scale = A.layernorm_fwd_scale(case.z, case.gamma, case.beta, case.slope, case.eps, case.norm_eps)
    want = A.layernorm_fwd_eval(case.z, case.gamma, case.beta, case.slope, case.eps, case.norm_eps, torch.float64)
    # (y and yn carry five roundings of their own: torch's float32 is 4.4 units off there and the bound 13 -- 16 units more)
    for k, n_units in (("mean", 8), ("rstd", 8), ("y", 16), ("yn", 16)):
        bad = bump(fwd[k], scale[k], n_units, want[k], rows_mask(fwd[k], slice(6, None)))
        rejected(C.check_layernorm_fwd, case, dict(fwd, **{k: bad}))
    m, r, y = fwd["mean"], fwd["rstd"], fwd["y"]
    bwd = C.layernorm_bwd_f32(case, m, r, y)
    C.check_layernorm_bwd([], case, m, r, y, bwd)
    bs = A.layernorm_bwd_scale(case.z, case.gamma, m, r, y, case.gy, case.gyn, case.slope, case.norm_eps)
    bw = A.layernorm_bwd_eval(case.z, case.gamma, m, r, y, case.gy, case.gyn, case.slope, case.norm_eps, torch.float64)
    for k in ("gz", "g_gamma", "g_beta"):
        where = rows_mask(bwd[k], slice(6, None)) if k == "gz" else None
        rejected(C.check_layernorm_bwd, case, m, r, y, dict(bwd, **{k: bump(bwd[k], bs[k], 8, bw[k], where)}))
    # the last row left out of the parameter gradients
    short = C.draw_layernorm(CPU, 40, d, beta_zero=beta_zero)
    short.gy[-1], short.gyn[-1] = 0.0, 0.0
    part = C.layernorm_bwd_f32(short, m, r, y)
    rejected(C.check_layernorm_bwd, case, m, r, y, dict(bwd, g_beta=part["g_beta"]))
    rejected(C.check_layernorm_bwd, case, m, r, y, dict(bwd, g_gamma=part["g_gamma"]))


def test_layernorm_sums_measure():
    case = C.draw_layernorm_sums(CPU, 20_001, 32, 1e3)
    fwd = C.layernorm_fwd_f32(case)
    m, r, y = fwd["mean"], fwd["rstd"], fwd["y"]
    bwd = C.layernorm_bwd_f32(case, m, r, y, use_gyn=False)
    C.check_layernorm_bwd([], case, m, r, y, bwd, use_gyn=False)
    # one sequential float32 chain over the 20 001 rows: the order a kernel must not take
    chain = torch.zeros(32)
    for blk in case.gy.split(1):
        chain += blk[0]
    err = (chain.double() - case.gy.double().sum(0)).abs() / case.gy.double().abs().sum(0)
    if float(err.max()) > 3e-7:
        rejected(C.check_layernorm_bwd, case, m, r, y, dict(bwd, g_beta=chain), use_gyn=False, only=("g_beta",))
    bs = A.layernorm_bwd_scale(case.z, case.gamma, m, r, y, case.gy, None, case.slope, case.norm_eps)
    bw = A.layernorm_bwd_eval(case.z, case.gamma, m, r, y, case.gy, None, case.slope, case.norm_eps, torch.float64)
    rejected(C.check_layernorm_bwd, case, m, r, y, dict(bwd, g_beta=bump(bwd["g_beta"], bs["g_beta"], 8, bw["g_beta"])), use_gyn=False)


# ------------------------------------------------------------------------------------------------- (d) BatchNorm
@pytest.mark.parametrize("n,d,shift", [(5, 7, 0), (257, 65, 0), (257, 1, 2)])
def test_batchnorm_measure(n, d, shift):
    case = C.draw_batchnorm(CPU, n, d, shift)
    for training in (True, False):
        fwd = C.batchnorm_fwd_f32(case, training)
        C.check_batchnorm_fwd([], case, training, fwd)
        scale = A.batchnorm_fwd_scale(case.z, case.gamma, case.beta, case.run_mean, case.run_var, training, C.BN_MOMENTUM, C.BN_EPS)
        want = A.batchnorm_fwd_eval(case.z, case.gamma, case.beta, case.run_mean, case.run_var, training, C.BN_MOMENTUM, C.BN_EPS,
                                    torch.float64)
        plain = torch.tensor([C.column_kind(j, shift) != "nonpositive" for j in range(d)])
        for k in ("y",) + (("mean", "invstd", "run_mean", "run_var") if training else ()):
            where = plain.expand_as(fwd[k])
            rejected(C.check_batchnorm_fwd, case, training, dict(fwd, **{k: bump(fwd[k], scale[k], 8, want[k], where)}))
        bwd = A.batchnorm_bwd_eval(case.z, case.gamma, fwd["mean"], fwd["invstd"], case.gy, training, torch.float32)
        C.check_batchnorm_bwd([], case, training, fwd["mean"], fwd["invstd"], bwd)
        bs = A.batchnorm_bwd_scale(case.z, case.gamma, fwd["mean"], fwd["invstd"], case.gy, training)
        bw = A.batchnorm_bwd_eval(case.z, case.gamma, fwd["mean"], fwd["invstd"], case.gy, training, torch.float64)
        for k in ("gz", "g_gamma", "g_beta"):
            where = (bs[k] > 0) & plain.expand_as(bwd[k])
            rejected(C.check_batchnorm_bwd, case, training, fwd["mean"], fwd["invstd"], dict(bwd, **{k: bump(bwd[k], bs[k], 8, bw[k], where)}))
    rejected(C.check_batchnorm_fwd, case, True, C.batchnorm_fwd_f32(case, True, mean_over=n + 1))
    # the biased variance in the running estimate
    fwd = C.batchnorm_fwd_f32(case, True)
    biased = (1 - C.BN_MOMENTUM) * case.run_var + C.BN_MOMENTUM * torch.relu(case.z).var(0, unbiased=False)
    rejected(C.check_batchnorm_fwd, case, True, dict(fwd, run_var=biased))


# ------------------------------------------------------------------------------------------------- (f) SpMM
@pytest.mark.parametrize("draw", C.SPMM_DRAWS)
def test_spmm_measure(draw):
    n, h, t, r = C.spmm_graph(n=120, e=700, long_rows=((3, 65), (10, 100)))
    g = C.csr_of(n, h, t, r, CPU)
    case = C.draw_spmm(CPU, n, g.nnz, 20, draw)
    good = A.spmm_eval(g.rowptr, g.col, case.val, case.x, n, torch.float32)
    C.check_spmm([], case.what, g.rowptr, g.col, case.val, case.x, n, good)
    scale = A.spmm_eval(g.rowptr, g.col, case.val, case.x, n, torch.float64, absolute=True)
    for row in (3, 10, 0):                                           # the last entry of a long and of a short row dropped
        assert int(g.rowptr[row + 1]) > int(g.rowptr[row])
        j = int(g.rowptr[row + 1]) - 1
        term = (case.val[j] * case.x[int(g.col[j])]).abs().double()
        if float((term / scale[row]).max()) < 1e-5:
            continue                                                 # (a 2^-140 value, a 2^-100 row: below the row's rounding)
        bad = A.spmm_eval(g.rowptr, g.col, case.val, case.x, n, torch.float32, drop_last_of=row)
        rejected(C.check_spmm, case.what, g.rowptr, g.col, case.val, case.x, n, bad)
    scale = A.spmm_eval(g.rowptr, g.col, case.val, case.x, n, torch.float64, absolute=True)
    want = A.spmm_eval(g.rowptr, g.col, case.val, case.x, n, torch.float64)
    rejected(C.check_spmm, case.what, g.rowptr, g.col, case.val, case.x, n, bump(good, scale, 8, want, scale > 2.0 ** -100))
    epi = dict(add_self=case.add_self, bias=case.bias)
    with_epi = A.spmm_eval(g.rowptr, g.col, case.val, case.x, n, torch.float32, **epi)
    C.check_spmm([], case.what, g.rowptr, g.col, case.val, case.x, n, with_epi, **epi)
    rejected(C.check_spmm, case.what, g.rowptr, g.col, case.val, case.x, n, good, **epi)       # the epilogue forgotten


# ------------------------------------------------------------------------------------------------- (e) attention
@pytest.mark.parametrize("draw", C.ATT_DRAWS)
def test_attention_measure(draw):
    n, h, t, r, lens = C.attention_graph(70, n=800, e=1500)
    g = C.csr_of(n, h, t, r, CPU)
    cnt = (g.rowptr[1:] - g.rowptr[:-1]).tolist()
    assert all(cnt[row] == deg for row, deg in lens.items()) and int(g.eptr[-1]) > g.nnz      # duplicates present
    d = 64
    case = C.draw_attention(CPU, n, 3, d, draw)
    logits = A.attention_logits_eval(g.rowptr, g.col, g.eptr, g.rel, case.ent, case.rel, torch.float32)[0]
    val, spread = A.row_softmax_eval(g.rowptr, logits, n, torch.float32)
    C.check_attention([], case.what, g, case.ent, case.rel, val, logits, True)
    # the last raw edge of the tripled / doubled pairs left out of its entry's logit
    ep = g.eptr.long()
    dup = int(torch.nonzero(ep[1:] - ep[:-1] > 1)[0])
    short = logits.clone()
    head = int(torch.searchsorted(g.rowptr.long(), torch.tensor(dup), right=True)) - 1
    e_last = int(ep[dup + 1]) - 1
    short[dup] -= float((case.ent[int(g.col[dup])] * torch.tanh(case.ent[head] + case.rel[int(g.rel[e_last])])).sum())
    if draw == "3 randn":
        rejected(C.check_attention, case.what, g, case.ent, case.rel, val, short, True)
    # tanh by its series over the whole draw: only where |h + r| leaves the series' range
    series = A.attention_logits_eval(g.rowptr, g.col, g.eptr, g.rel, case.ent, case.rel, torch.float32, tanh=tanh_series)[0]
    if draw == "3 randn":
        assert not C.finite(series) or float((series - logits).abs().max()) > 1.0
        with pytest.raises(AssertionError):
            C.check_attention([], case.what, g, case.ent, case.rel, A.row_softmax_eval(g.rowptr, torch.nan_to_num(series), n,
                                                                                     torch.float32)[0], torch.nan_to_num(series), True)
    else:
        C.check_attention([], case.what, g, case.ent, case.rel, A.row_softmax_eval(g.rowptr, series, n, torch.float32)[0], series, True)
    # the softmax stage: one value off by 8 units at its row's maximum; the maximum not subtracted on the wide draw
    top = int(torch.nonzero((spread == 0) & (val > 0.01))[0])
    bad = val.clone()
    bad[top] *= 1 + 8 * A.U
    rejected(C.check_attention, case.what, g, case.ent, case.rel, bad, logits, True)
    if draw == "3 randn":
        assert float(spread.max()) > 100.0
        naive, _ = A.row_softmax_eval(g.rowptr, logits, n, torch.float32, subtract_max=False)
        rejected(C.check_attention, case.what, g, case.ent, case.rel, naive, logits, True)
        flushed = torch.where(val < 1e-30, torch.full_like(val, 1e-44), val)          # an underflowed value that is not zero
        rejected(C.check_attention, case.what, g, case.ent, case.rel, flushed, logits, True)


# ------------------------------------------------------------------------------------------------- (g) scores and losses
def scores_f32(case, rows):
    eh, er, ep, en = rows
    dot = er is None
    v, _ = A.dot_scores_eval(eh, ep, en, torch.float32) if dot else A.trans_scores_eval(eh, er, ep, en, torch.float32)
    margin = (v["pos"] - v["neg"]) if dot else (v["neg"] - v["pos"])
    v["rank"] = A.rank_eval(margin, torch.float32)[0]
    v["loss"] = A.loss_eval(v["rank"], v["reg"], case.lam, torch.float32)[0]
    return v


@pytest.mark.parametrize("form,dim,b", [("transe", 3, 17), ("transe", 32, 1025), ("dot", 32, 1025), ("dot", 100, 17)])
def test_scores_measure(form, dim, b):
    case = C.draw_triples(CPU, form, dim, b)
    rows = (case.emb[case.h], case.rel[case.r] if form == "transe" else None, case.emb[case.pos_t], case.emb[case.neg_t])
    good = scores_f32(case, rows)
    lo_, hi_ = C.check_scores([], case, rows, good)
    assert lo_ < -90.0 and hi_ > 90.0
    want, scale = (A.dot_scores_eval(rows[0], rows[2], rows[3], torch.float64) if form == "dot"
                   else A.trans_scores_eval(*rows, torch.float64))
    for k in ("pos", "neg", "reg"):
        rejected(C.check_scores, case, rows, dict(good, **{k: bump(good[k], scale[k], 8, want[k])}))
    # a rank through log(1 + exp(-x)) as written: overflows in the negative tail
    margin = (good["pos"] - good["neg"]) if form == "dot" else (good["neg"] - good["pos"])
    rejected(C.check_scores, case, rows, dict(good, rank=torch.log(1 + torch.exp(-margin))))
    # ... and one that drops the tail term: log1p(exp(-|x|)) missing where x > 0 is small
    if float(margin.abs().min()) < 5.0:
        rejected(C.check_scores, case, rows, dict(good, rank=torch.clamp(-margin, min=0)))
    rejected(C.check_scores, case, rows, dict(good, loss=good["rank"][:-1].mean() + case.lam * good["reg"].mean()))
    # the gradients: float32 passes; the last triple left out of the scatter fails
    v32, _, _ = C.triple_grads(case, rows, good["pos"], good["neg"], torch.float32)
    ids = dict(h=case.h, p=case.pos_t, n=case.neg_t)
    g_emb = A.scatter_rows(case.n_ent, [(ids[k], v32[k]) for k in ("h", "p", "n")], torch.float32)
    g_rel = A.scatter_rows(case.n_rel, [(case.r, v32["r"])], torch.float32) if form == "transe" else None
    C.check_table_grads([], case, rows, good["pos"], good["neg"], g_emb, g_rel)
    part = A.scatter_rows(case.n_ent, [(ids[k][:-1], v32[k][:-1]) for k in ("h", "p", "n")], torch.float32)
    rejected(C.check_table_grads, case, rows, good["pos"], good["neg"], part, g_rel)
    # a sigmoid that is off by 1e-4 (say, a coarse approximation)
    vbad, _, _ = C.triple_grads(case, rows, good["pos"], good["neg"], torch.float32, sigmoid=lambda x: torch.sigmoid(x) + 1e-4)
    bad = A.scatter_rows(case.n_ent, [(ids[k], vbad[k]) for k in ("h", "p", "n")], torch.float32)
    rejected(C.check_table_grads, case, rows, good["pos"], good["neg"], bad, g_rel)
