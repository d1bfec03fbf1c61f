"""Every product and reduction engine on operands chosen to break it, checked per ELEMENT against float64 (op_audit.py):

  (a) scale sweep: whole rows / columns with their maximum at 2^-149 (subnormal) .. 2^120, partners chosen so that the exact
      result is a normal float32 -- the power-of-two operand scales of the fp16 split engines (scale_exponent) must follow;
  (b) range within a row / column: small elements next to one large one that meets a zero partner, so that the small ones
      make the whole result -- down to the stated limit of each split engine, and the stated absolute bound beyond it;
  (c) a large common part that cancels (products and column sums over up to 1 M rows);
  (d) all-zero rows and columns, row-sparse K;
  (e) one NaN / +-inf element: exactly the outputs torch makes non-finite are non-finite, no other is touched.

The engine that ran is asserted through the lkg_*_ok predicates; the bound is  max r <= max(F * r_torch32, FLOOR)."""
import pytest
import torch

from op_audit import BF16X3, BOUNDS, bound_for, chain_term, componentwise

pytestmark = pytest.mark.gpu

# (row / column maximum of the first operand, of the second) as powers of two: every edge of the old +-100 clamp, the
# subnormal and the smallest normal maxima, each on either side of the product
SCALE_PAIRS = [(-149, 126), (-126, 110), (-110, 100), (-90, 80), (0, 0), (100, -110), (113, -116), (116, -120), (120, -126)]
SCALE_PAIRS = SCALE_PAIRS + [(b, a) for a, b in SCALE_PAIRS if a != b]


def lo(e: int) -> int:
    """a partner exponent, never below the smallest subnormal"""
    return max(e, -149)


@pytest.fixture(scope="module")
def ops(gpu_device):
    import __graft_entry__ as ge
    ge.build()
    from literalkg_amd import ops as _ops
    return _ops


def at_max(x: torch.Tensor, e: int, dim: int) -> torch.Tensor:
    """x scaled so that every row (dim=1) / column (dim=0) has its largest magnitude at exactly 2^e (one rounding to f32)"""
    x64 = x.double()
    x64 = x64 / x64.abs().amax(dim, keepdim=True)
    return torch.ldexp(x64, torch.tensor(e, dtype=torch.int32)).float()


# The bf16 x 3 engines (lkg_gemm_f32's split engines, lkg_gemm_longk_f32) carry no operand scales: an element x is split into
# three bf16 terms whose last one falls below bf16's normal range once |x| < 2^-110 -- the element then carries an absolute
# error <= 2^-134 (half of bf16's smallest subnormal 2^-133), elements below 2^-134 are dropped.  Bound of the product:
# the componentwise one plus  2^-133 (sum_k |b_kj| + sum_k |a_ik|)  (negligible unless an operand is that small).  So these
# engines do NOT carry operands below about 2^-126 at all: at the scale pairs with such an operand this bound admits any
# output (DESIGN 3.5 states it); what the pairs check there is only that nothing overflows or turns non-finite.
BF16X3_ABS = 2.0 ** -133


def check(engine, got, a, b, what, bias=None, ref32=None):
    """got ~ a @ b (+ bias) componentwise; a [m, k], b [k, n] float32 (math layout)"""
    a64, b64 = a.double(), b.double()
    want = a64 @ b64
    scale = a64.abs() @ b64.abs()
    ref32 = a @ b if ref32 is None else ref32
    if bias is not None:
        want, scale, ref32 = want + bias.double(), scale + bias.double().abs(), ref32 + bias
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) < 3e38, what
    r32, _ = componentwise(ref32, want, scale)
    bound = bound_for(engine, r32, a.shape[1])
    if engine in BF16X3:
        absolute = BF16X3_ABS * (b64.abs().sum(0, keepdim=True) + a64.abs().sum(1, keepdim=True))
        excess = (got.double() - want).abs() - (bound * scale + absolute)
        i = int(excess.argmax())
        assert float(excess.reshape(-1)[i]) <= 0, (f"{engine} {what}: beyond the stated bound at element {i}: got "
                                                   f"{got.reshape(-1)[i].item()!r}, x64 {want.reshape(-1)[i].item()!r}")
        return 0.0, r32
    r, i = componentwise(got, want, scale)
    assert r <= bound, (f"{engine} {what}: r = {r:.3g} > {bound:.3g} (torch f32 {r32:.3g}); worst element {i}: "
                        f"got {got.reshape(-1)[i].item()!r}, x64 {want.reshape(-1)[i].item()!r}, "
                        f"scale {scale.reshape(-1)[i].item()!r}")
    return r, r32


# ------------------------------------------------------------------------------------------------ (a) scale sweep
TALL_M, TALL_K, TALL_N = 16384 + 77, 96, 256


@pytest.mark.parametrize("variant", [None, "256x2", "128x1", "256x1"])
def test_tall_scale_sweep(ops, gpu_device, variant):
    """lkg_gemm_tall_f32, every tiling: rows of A and rows of B (output columns) at every edge of the exponent range."""
    assert ops.tall_ok(TALL_M, TALL_N, (TALL_K,), True)
    gen = torch.Generator(device=gpu_device).manual_seed(5)
    a0 = torch.randn(TALL_M, TALL_K, device=gpu_device, generator=gen)
    w0 = torch.randn(TALL_N, TALL_K, device=gpu_device, generator=gen)
    for ea, eb in SCALE_PAIRS:
        a, w = at_max(a0, ea, 1), at_max(w0, eb, 1)
        got = ops.gemm_tall((a,), ((w,),), True, variant=variant)
        check("tall_f16x2", got, a, w.t(), f"variant {variant}, row max 2^{ea}, B row max 2^{eb}")


@pytest.mark.parametrize("variant", [None, "256x2"])
def test_tall_gate_epilogue_scale_sweep(ops, gpu_device, variant):
    """The gate epilogue (two interleaved weight groups, each row group with its own exponents) at the range edges: the
    kept tanh(g) / sigmoid(z) through their derivatives, the blend against float64.  Every allowance is RELATIVE where the
    values are small (tanh_fast's series below 0.25 is accurate to its own roundings, 5e-7 |t|), so a g lost at the small
    exponents (2^-149 .. 2^-110 rows: g ~ 1e-7 .. 1e-3) fails here.  z enters only through sigmoid, which cannot show a z
    below ~2^-24 (sigmoid(z) rounds to 1/2): at those pairs z's group is checked at the large exponents only, through the
    same per-row exponent code as g's."""
    m, k, d = TALL_M, 16, 128                      # A = [x | literals]: the gate blends its first panel x
    gen = torch.Generator(device=gpu_device).manual_seed(6)
    a0 = torch.randn(m, d + k, device=gpu_device, generator=gen)
    wg0, wz0 = (torch.randn(d, d + k, device=gpu_device, generator=gen) for _ in range(2))
    f_tall, floor = BOUNDS["tall_f16x2"]
    for ea, eb in SCALE_PAIRS:
        a, wg, wz = at_max(a0, ea, 1), at_max(wg0, eb, 1), at_max(wz0, lo(eb - 1), 1)
        x, lit = a[:, :d].contiguous(), a[:, d:].contiguous()
        go, zo = torch.empty_like(x), torch.empty_like(x)
        out = ops.gemm_tall((x, lit), ((wg[:, :d], wg[:, d:]), (wz[:, :d], wz[:, d:])), True, gate_x=x, keep=(go, zo),
                            variant=variant)
        a64 = a.double()
        g64, z64 = a64 @ wg.double().t(), a64 @ wz.double().t()
        sg, sz = a64.abs() @ wg.double().abs().t(), a64.abs() @ wz.double().abs().t()
        r32 = max(componentwise(a @ wg.t(), g64, sg)[0], componentwise(a @ wz.t(), z64, sz)[0])
        bound = max(f_tall * r32, floor)
        tg, sgm = torch.tanh(g64), torch.sigmoid(z64)
        x64 = x.double()
        allow_t = bound * (1 - tg ** 2) * sg + torch.where(g64.abs() < 0.25, 5e-7 * tg.abs(), torch.full_like(tg, 4e-7))
        allow_s = bound * sgm * (1 - sgm) * sz + 2e-6 * sgm
        for what, got, want, allow in (
                ("tanh(g)", go, tg, allow_t),
                ("sigmoid(z)", zo, sgm, allow_s),
                ("blend", out, (1 - sgm) * x64 + sgm * tg,
                 sgm * allow_t + (x64 - tg).abs() * allow_s + 2.0 ** -22 * (x64.abs() + tg.abs()))):
            err = (got.double() - want).abs()
            i = int((err - allow).argmax())
            assert float((err - allow).reshape(-1)[i]) <= 0, (f"gate {variant} 2^{ea} x 2^{eb}: {what} off by "
                                                              f"{err.reshape(-1)[i].item():.3g} > {allow.reshape(-1)[i].item():.3g}")


@pytest.mark.parametrize("k", [16 * 2500, 16 * 2500 + 5])       # lkg_gemm_longk f16 kernel / the 128 x 128 f16x2 kernel
def test_wgrad_f16x2_scale_sweep(ops, gpu_device, k):
    """lkg_gemm_wgrad_f32 (both kernels): columns of both operands at every edge of the exponent range; the column maxima
    from lkg_col_absmax_f32, which must be exact for subnormal columns too."""
    from literalkg_amd import _native as N
    m, n = 160, 136
    gen = torch.Generator(device=gpu_device).manual_seed(k)
    a0 = torch.randn(k, m, device=gpu_device, generator=gen)
    b0 = torch.randn(k, n, device=gpu_device, generator=gen)
    a_ = a0.contiguous()
    assert bool(N.load().lkg_gemm_longk_ok(m, n, k, N.ptr(a_), m, N.ptr(b0), n)) == (k % 16 == 0)
    for ea, eb in SCALE_PAIRS:
        ea_, eb_ = ea, lo(eb - 16)         # (k = 40 000 terms: keep the exact result inside the float32 range)
        a, b = at_max(a0, ea_, 0), at_max(b0, eb_, 0)
        ca, cb = ops.col_absmax(a), ops.col_absmax(b)
        assert torch.equal(ca, a.abs().amax(0)) and torch.equal(cb, b.abs().amax(0))
        got = ops.gemm_wgrad(a, b, ca, cb)
        check("wgrad_f16x2", got, a.t(), b, f"k {k}, A columns at 2^{ea_}, B columns at 2^{eb_}", ref32=a.t() @ b)


@pytest.mark.parametrize("case", ["bf16x3_rows", "bf16x3_kmajor", "longk", "f32_mfma", "skinny", "smallm"])
def test_other_engines_scale_sweep(ops, gpu_device, case):
    """lkg_gemm_f32's split engines and its f32-input MFMA engine, lkg_gemm_longk_f32, the skinny and small-m VALU kernels:
    the same exponent edges (these engines carry no operand scales; they must keep the range of an f32 GEMM)."""
    gen = torch.Generator(device=gpu_device).manual_seed(9)
    shapes = {"bf16x3_rows": (20000, 96, 128, False), "bf16x3_kmajor": (96, 8000 + 3, 112, True),
              "longk": (128, 16 * 520, 96, True), "f32_mfma": (3000, 96, 130, False), "skinny": (20000, 40, 32, False),
              "smallm": (48, 16 * 300, 80, True)}
    m, k, n, ta = shapes[case]
    a0 = torch.randn(k, m, device=gpu_device, generator=gen) if ta else torch.randn(m, k, device=gpu_device, generator=gen)
    b0 = torch.randn(k, n, device=gpu_device, generator=gen)
    for ea, eb in SCALE_PAIRS:
        eb_ = lo(eb - 12) if ta else eb
        a = at_max(a0, ea, 0 if ta else 1)
        b = at_max(b0, eb_, 0)
        engine = ops.gemm_engine(a, b, trans_a=ta)
        assert engine == case, (case, engine)
        got = ops.gemm(a, b, trans_a=ta)
        am = a.t() if ta else a
        check(engine, got, am, b, f"{case}: A at 2^{ea}, B at 2^{eb_}")


@pytest.mark.parametrize("case", ["f32_mfma k 1200", "f32_mfma k 6000", "wgrad k 35008", "wgrad k 35005"])
def test_long_accumulation_chains_meet_their_stated_bound(ops, gpu_device, case):
    """Same-sign operands (every partial sum as large as the result: the worst case of a long accumulation chain) at the
    K of the model's longest chains -- the link scores' K = 1200 on the f32-input MFMA, a 35 000-row weight gradient on
    both f16 x 2 kernels: within the engine's stated bound max(F r_torch32, FLOOR, chain term) (op_audit.chain_term)."""
    gen = torch.Generator(device=gpu_device).manual_seed(len(case))
    kind, k = case.split(" k ")[0], int(case.split(" k ")[1])
    if kind == "f32_mfma":
        a = torch.rand(40, k, device=gpu_device, generator=gen) + 0.5
        b = torch.rand(k, 30, device=gpu_device, generator=gen) + 0.5
        assert ops.gemm_engine(a, b) == "f32_mfma"
        got, am, bm = ops.gemm(a, b), a, b
    else:
        kind = "wgrad_f16x2"
        x = torch.rand(k, 256, device=gpu_device, generator=gen)
        y = torch.rand(k, 128, device=gpu_device, generator=gen) + 0.25
        got, am, bm = ops.gemm_wgrad(x, y, ops.col_absmax(x), ops.col_absmax(y)), x.t(), y
    r, r32 = check(kind, got, am, bm, case)
    f, floor = BOUNDS[kind]
    print(f"{case}: r {r:.3g}, torch f32 {r32:.3g}, F r32 / floor {max(f * r32, floor):.3g}, chain term "
          f"{chain_term(kind, k):.3g}")


def test_gemm_f64acc_is_one_rounding_of_float64(ops, gpu_device):
    """lkg_gemm_f64acc_f32 (the residual's weight fold): within one f32 rounding of float64, plus float64's own
    accumulation error, across the exponent edges and under cancellation."""
    gen = torch.Generator(device=gpu_device).manual_seed(3)
    for ea, eb in SCALE_PAIRS + [(0, 0)]:
        a = at_max(torch.randn(40, 300, device=gpu_device, generator=gen), ea, 1)
        b = at_max(torch.randn(300, 24, device=gpu_device, generator=gen), lo(eb - 4), 0)
        for ta, tb in ((False, False), (True, False), (False, True)):
            aa = a.t().contiguous() if ta else a
            bb = b.t().contiguous() if tb else b
            got = ops.gemm_f64acc(aa, bb, trans_a=ta, trans_b=tb).double()
            want = a.double() @ b.double()
            allow = want.abs() * 2.0 ** -24 + 302 * 2.0 ** -53 * (a.double().abs() @ b.double().abs()) + 2.0 ** -150
            assert bool(((got - want).abs() <= allow).all()), (ea, eb, ta, tb, float(((got - want).abs() / allow).max()))
    # cancellation: a row and its negative plus a tiny remainder
    a = torch.randn(2, 500, device=gpu_device, generator=gen)
    b = torch.randn(500, 3, device=gpu_device, generator=gen)
    a[1] = -a[0] * (1 + 2.0 ** -20)
    got = ops.gemm_f64acc(a, b).double()
    want = a.double() @ b.double()
    assert bool(((got - want).abs() <= want.abs() * 2.0 ** -24 + 502 * 2.0 ** -53 * (a.double().abs() @ b.double().abs())).all())


# ------------------------------------------------------------------------------------- (b) range within a row / column
# Each split engine carries every element with the full 22 bits down to a stated fraction of its row's (column's)
# maximum; below it the element's error is bounded in absolute terms relative to that maximum.  (header comments of
# lkg_gemm_tall.hip / lkg_gemm_wgrad.hip)
TALL_FULL = {None: 16, "256x2": 27, "128x1": 16, "256x1": 16}


def range_case(gen, device, m, k, j, rows_major=True):
    """an operand whose every row has one element at 2^j (index 0) and the rest ~N(0, 1); the partner meets index 0 with 0"""
    x = torch.randn(m, k, device=device, generator=gen)
    x[:, 0] = 2.0 ** j
    return x if rows_major else x.t().contiguous()


@pytest.mark.parametrize("variant", [None, "256x2", "128x1", "256x1"])
def test_tall_range_within_a_row(ops, gpu_device, variant):
    """Rows whose maximum (one element, meeting a zero weight) is 2^j above the elements that make the result: up to the
    stated limit the small elements keep the componentwise bound, beyond it the absolute bound 2^-34 rowmax sum|w|."""
    gen = torch.Generator(device=gpu_device).manual_seed(21)
    m, k, n = TALL_M, 64, 128
    w = torch.randn(n, k, device=gpu_device, generator=gen)
    w[:, 0] = 0.0
    full = TALL_FULL[variant]
    for j in (4, 8, 12, 16, 20, 24, 27, 32, 40):
        a = range_case(gen, gpu_device, m, k, j)
        got = ops.gemm_tall((a,), ((w,),), True, variant=variant)
        if j <= full:
            check("tall_f16x2", got, a, w.t(), f"variant {variant}, elements 2^-{j} of the row maximum")
        else:
            want = a.double() @ w.double().t()
            err = (got.double() - want).abs()
            allow = 2.0 ** -22 * (a.double().abs() @ w.double().abs().t()) + 2.0 ** (j - 34) * w.double().abs().sum(1)
            assert bool((err <= allow).all()), (variant, j, float((err / allow).max()))


@pytest.mark.parametrize("k", [16 * 2500, 16 * 2500 + 5])
def test_wgrad_range_within_a_column(ops, gpu_device, k):
    """lkg_gemm_wgrad_f32: a column's maximum 2^j above the elements that make the result (the maximum's row meets zeros
    in the other operand)."""
    gen = torch.Generator(device=gpu_device).manual_seed(22)
    m, n = 64, 128
    b = torch.randn(k, n, device=gpu_device, generator=gen)
    b[0] = 0.0
    for j in (4, 8, 12, 16, 20, 27, 32, 40):
        a = torch.randn(k, m, device=gpu_device, generator=gen)
        a[0] = 2.0 ** j
        got = ops.gemm_wgrad(a, b, ops.col_absmax(a), ops.col_absmax(b))
        if j <= 16:
            check("wgrad_f16x2", got, a.t(), b, f"k {k}: elements 2^-{j} of the column maximum")
        else:
            want = a.double().t() @ b.double()
            err = (got.double() - want).abs()
            allow = 2.0 ** -22 * (a.double().abs().t() @ b.double().abs()) + 2.0 ** (j - 35) * b.double().abs().sum(0)
            assert bool((err <= allow).all()), (k, j, float((err / allow).max()))


# ------------------------------------------------------------------------------------------ (c) cancellation
@pytest.mark.parametrize("mu", [1e3, 1e5])
def test_tall_and_wgrad_cancellation(ops, gpu_device, mu):
    """mu + noise operands whose products cancel to near zero: the result is the noise's, the error bound the products'."""
    gen = torch.Generator(device=gpu_device).manual_seed(int(mu))
    m, k, n = TALL_M, 64, 128
    a = mu + torch.randn(m, k, device=gpu_device, generator=gen)
    w = torch.randn(n, k, device=gpu_device, generator=gen)
    w[:, 1::2] = -w[:, 0::2]                               # sum_k a_k w_k = sum over pairs (a_2i - a_2i+1) w_2i
    for variant in (None, "256x2"):
        check("tall_f16x2", ops.gemm_tall((a,), ((w,),), True, variant=variant), a, w.t(), f"{variant} mu {mu}")
    kk = 16 * 4000
    x = mu + torch.randn(kk, 96, device=gpu_device, generator=gen)
    y = torch.randn(kk, 64, device=gpu_device, generator=gen)
    y[1::2] = -y[0::2]
    check("wgrad_f16x2", ops.gemm_wgrad(x, y, ops.col_absmax(x), ops.col_absmax(y)), x.t(), y, f"wgrad mu {mu}")


@pytest.mark.parametrize("n", [1 << 20, 300_001])
def test_column_sums_under_cancellation(ops, gpu_device, n):
    """lkg_colsum_f32 and lkg_colsum_weighted_f32 (the Linear bias gradients, the numeric literals' weight gradient) over
    up to 1 M rows of +-mu + noise, per column against sum |x|.  (Their block partials meet in f32 atomics, so two calls may
    differ in the last bits; both are within the bound.)"""
    gen = torch.Generator(device=gpu_device).manual_seed(n)
    d = 72
    for mu in (1e3, 1e5):
        sign = torch.where(torch.rand(n, 1, device=gpu_device, generator=gen) < 0.5, -1.0, 1.0)
        x = sign * mu + torch.randn(n, d, device=gpu_device, generator=gen)
        x[:, 5] = 0.0                                          # an all-zero column
        x64 = x.double()
        want, scale = x64.sum(0), x64.abs().sum(0)
        got = ops.colsum(x)
        r, i = componentwise(got, want, scale)
        r32, _ = componentwise(x.sum(0), want, scale)
        assert r <= bound_for("colsum", r32), ("colsum", n, mu, r, r32, i)
        assert float(got[5]) == 0.0
        p = mu * 1e-3 * torch.randn(n, 2, device=gpu_device, generator=gen) + 1.0
        gw, gs = ops.narrow_weight_grad(x, p, True)
        r, i = componentwise(gw, x64.t() @ p.double(), x64.abs().t() @ p.double().abs())
        r32, _ = componentwise(x.t() @ p, x64.t() @ p.double(), x64.abs().t() @ p.double().abs())
        assert r <= bound_for("colsum", r32), ("colsum_weighted", n, mu, r, r32, i)
        r, _ = componentwise(gs, want, scale)
        assert r <= bound_for("colsum", r32), ("colsum_weighted sums", n, mu, r)


# ------------------------------------------------------------------------------------------ (d) zeros, (e) NaN / inf
def test_zero_rows_columns_and_sparse_k(ops, gpu_device):
    gen = torch.Generator(device=gpu_device).manual_seed(31)
    a = torch.randn(TALL_M, 80, device=gpu_device, generator=gen)
    w = torch.randn(200, 80, device=gpu_device, generator=gen)
    a[7], a[100:300] = 0.0, 0.0
    w[3] = 0.0
    for variant in (None, "256x2", "128x1"):
        got = ops.gemm_tall((a,), ((w,),), True, variant=variant)
        check("tall_f16x2", got, a, w.t(), f"zero rows {variant}")
        assert float(got[7].abs().max()) == 0.0 and float(got[:, 3].abs().max()) == 0.0
    k = 16 * 3000
    x = torch.randn(k, 96, device=gpu_device, generator=gen)
    y = torch.randn(k, 130, device=gpu_device, generator=gen)
    keep = torch.zeros(k, 1, device=gpu_device)
    keep[torch.randint(0, k, (k // 200,), device=gpu_device, generator=gen)] = 1.0
    x = x * keep
    x[:, 4] = 0.0
    for kk in (k, k - 3):
        xs, ys = x[:kk], y[:kk]
        got = ops.gemm_wgrad(xs, ys, ops.col_absmax(xs), ops.col_absmax(ys))
        check("wgrad_f16x2", got, xs.t(), ys, f"row-sparse k {kk}")
        assert float(got[4].abs().max()) == 0.0


def test_non_finite_elements_stay_where_torch_puts_them(ops, gpu_device):
    gen = torch.Generator(device=gpu_device).manual_seed(41)
    a = torch.randn(TALL_M, 64, device=gpu_device, generator=gen)
    w = torch.randn(256, 64, device=gpu_device, generator=gen)
    a[11, 5], a[900, 0], a[901, 63] = float("nan"), float("inf"), -float("inf")
    w[17, 9] = float("inf")
    ref = a @ w.t()
    fin = torch.isfinite(ref)
    for variant in (None, "256x2", "128x1", "256x1"):
        got = ops.gemm_tall((a,), ((w,),), True, variant=variant)
        assert torch.equal(torch.isfinite(got), fin), variant
        a0 = torch.where(torch.isfinite(a), a, torch.zeros_like(a))
        w0 = torch.where(torch.isfinite(w), w, torch.zeros_like(w))
        want = a0.double() @ w0.double().t()
        scale = a0.double().abs() @ w0.double().abs().t()
        r, _ = componentwise(torch.where(fin, got, torch.zeros_like(got)), torch.where(fin, want, torch.zeros_like(want)),
                             scale)
        r32, _ = componentwise(torch.where(fin, ref, torch.zeros_like(ref)), torch.where(fin, want, torch.zeros_like(want)), scale)
        assert r <= bound_for("tall_f16x2", r32), (variant, r, r32)
    k = 16 * 2000
    for kk in (k, k + 3):
        x = torch.randn(kk, 64, device=gpu_device, generator=gen)
        y = torch.randn(kk, 96, device=gpu_device, generator=gen)
        x[10, 3], y[20, 7], y[30, 8] = float("nan"), float("inf"), -float("inf")
        ref = x.t() @ y
        got = ops.gemm_wgrad(x, y, ops.col_absmax(x), ops.col_absmax(y))
        assert torch.equal(torch.isfinite(got), torch.isfinite(ref)), kk


def test_row_and_column_maxima_are_exact(ops, gpu_device):
    """lkg_row_absmax_f32 / lkg_col_absmax_f32 (the scale hints of the split engines): exact, subnormal rows included."""
    gen = torch.Generator(device=gpu_device).manual_seed(51)
    x = torch.randn(20000, 70, device=gpu_device, generator=gen)
    x[0] = at_max(x[:1], -149, 1)[0]
    x[1] = at_max(x[1:2], -140, 1)[0]
    x[2] = at_max(x[2:3], 127, 1)[0]
    x[3] = 0.0
    x[:, 6] = at_max(x[:, 6:7], -135, 0)[:, 0]
    assert torch.equal(ops.row_absmax(x), x.abs().amax(1))
    assert torch.equal(ops.col_absmax(x), x.abs().amax(0))
    assert torch.equal(ops.row_absmax(x[:, 3:40]), x[:, 3:40].abs().amax(1))


def test_fused_linear_act_layernorm_at_the_range_edges(ops, gpu_device):
    """linear_act_layernorm_fwd (the tall engine with the LeakyReLU + LayerNorm epilogue) against the unfused pair at the
    exponent edges: never further from float64 than the unfused path's own error (x 3, floor 2e-6)."""
    gen = torch.Generator(device=gpu_device).manual_seed(61)
    m, k, n = TALL_M, 64, 128
    a0 = torch.randn(m, k, device=gpu_device, generator=gen)
    w0 = torch.randn(n, k, device=gpu_device, generator=gen)
    bias = torch.randn(n, device=gpu_device, generator=gen) * 0.1
    gamma = 1.0 + 0.1 * torch.randn(n, device=gpu_device, generator=gen)
    beta = 0.1 * torch.randn(n, device=gpu_device, generator=gen)
    assert ops.fused_layer_ok(m, n, (k,))
    for ea, eb in SCALE_PAIRS:
        a, w = at_max(a0, ea, 1), at_max(w0, lo(eb - 3), 1)
        y, _, _, _ = ops.linear_act_layernorm_fwd((a,), (w,), bias, gamma, beta, 0.01, 1e-5, 1e-12, 0.0, 0, want_norm=False)
        z = ops.gemm_tall((a,), ((w,),), True, bias)
        z64 = a.double() @ w.double().t() + bias.double()

        def ln(z_):
            h = torch.nn.functional.leaky_relu(z_, 0.01)
            return torch.nn.functional.layer_norm(h, (n,), gamma.to(h.dtype), beta.to(h.dtype), 1e-5)
        y64 = ln(z64)
        e_fused = float((y.double() - y64).abs().max())
        e_unfused = float((ln(z).double() - y64).abs().max())
        assert e_fused <= max(3 * e_unfused, 2e-6), (ea, eb, e_fused, e_unfused)


def test_scatter_add_rows_with_repeated_ids(ops, gpu_device):
    """lkg_scatter_add_rows_f32 with ids repeated thousands of times (a batch pool of a few entities): per element against
    float64 over sum |src|."""
    from literalkg_amd import _native as N
    gen = torch.Generator(device=gpu_device).manual_seed(71)
    n, d, rows = 50, 64, 200_000
    ids = torch.randint(0, 5, (rows,), device=gpu_device, generator=gen)
    ids[::7] = 49
    src = 1e3 * torch.where(torch.rand(rows, 1, device=gpu_device, generator=gen) < 0.5, -1.0, 1.0) + \
        torch.randn(rows, d, device=gpu_device, generator=gen)
    dst = torch.zeros(n, d, device=gpu_device)
    N.call("lkg_scatter_add_rows_f32", rows, d, N.ptr(src), d, N.ptr(ids), None, N.ptr(dst), d, ops._stream())
    want = torch.zeros(n, d, dtype=torch.float64, device=gpu_device).index_add_(0, ids, src.double())
    scale = torch.zeros(n, d, dtype=torch.float64, device=gpu_device).index_add_(0, ids, src.double().abs())
    ref32 = torch.zeros(n, d, device=gpu_device).index_add_(0, ids, src)
    r, _ = componentwise(dst, want, scale)
    r32, _ = componentwise(ref32, want, scale)
    assert r <= bound_for("colsum", r32), (r, r32)
    assert float(dst[5:49].abs().max()) == 0.0
    # the range form (the model's row-sparse backward and the sharded table): rows [lo, hi) only, dst at row lo, the
    # repeated ids outside the range skipped
    lo_, hi_ = 3, 45
    table = torch.zeros(n, d + 4, device=gpu_device)
    N.call("lkg_scatter_add_rows_range_f32", rows, d, N.ptr(src), d, N.ptr(ids), lo_, hi_, N.ptr(table[lo_:, 2:]), d + 4,
           ops._stream())
    inside = (ids >= lo_) & (ids < hi_)
    want_r = torch.zeros(n, d, dtype=torch.float64, device=gpu_device).index_add_(0, ids[inside], src[inside].double())
    scale_r = torch.zeros(n, d, dtype=torch.float64, device=gpu_device).index_add_(0, ids[inside], src[inside].double().abs())
    ref_r = torch.zeros(n, d, device=gpu_device).index_add_(0, ids[inside], src[inside])
    r, _ = componentwise(table[:, 2:2 + d], want_r, scale_r)
    r32, _ = componentwise(ref_r, want_r, scale_r)
    assert r <= bound_for("colsum", r32), ("range", r, r32)
    assert float(table[:lo_].abs().max()) == 0.0 and float(table[hi_:].abs().max()) == 0.0
    assert float(table[:, :2].abs().max()) == 0.0 and float(table[:, 2 + d:].abs().max()) == 0.0
    assert float(table[lo_:5, 2:2 + d].abs().max()) > 0.0       # ids 3 and 4 are in the range and repeated
