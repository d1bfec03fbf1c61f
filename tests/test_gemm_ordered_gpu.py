"""Device tier of the ordered split-K GEMM (literalkg_amd/gemm_ordered.py; the host tier is test_gemm_ordered_host.py).

Every operand is a view into a wider tensor: its row stride is larger than its row, and unless a test says otherwise it
starts one column in, 4 bytes off the 16-byte grid, so the clamped scalar load path runs; ``out`` is an inner block of a
larger tensor whose border must keep its sentinel.

  exact          integer operands in [-3, 3] (sums below 2^24): the result equals the integer product for every ``splits``
  defined order  gemm_ordered(splits=S) has the bits of the splits=1 results over the k-slices partition(k, S) names,
                 added in ascending z with torch float32 adds
  float64        per element r = |err| / (|A||B| + |beta c| + |bias|) <= bound_for("f32_mfma", r_torch32, per + s_eff)
  no tolerance   runs, poison, a side stream, row permutation, a row alone, a column subset, alignment, out given or fresh
  matmul_ordered gradients under every subset of trainable inputs"""
import contextlib
import importlib
import itertools

import pytest
import torch

import invariance as V
import op_audit as OA

pytestmark = pytest.mark.gpu

LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]
LAYOUT_IDS = ["NN", "NT", "TN", "TT"]
MS, NS, KS = (1, 127, 129), (1, 129, 300), (1, 17, 4097)
LONG = (129, 300, 76800)                       # NT only
SPLITS = (1, 2, 3, 7, 256, None)
SENTINEL = -777.0


@pytest.fixture(scope="module")
def GO(gpu_device):
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("literalkg_amd.gemm_ordered")


def embed(x, off=1, pad=3):
    """x as a view of a wider tensor: row stride cols + off + pad (odd for the sizes used), starting ``off`` columns in.
    off = 0 with a row stride of a multiple of 4 is the aligned form."""
    rows, cols = x.shape
    ld = cols + off + pad
    if off == 0:
        ld = (ld + 3) // 4 * 4
    wide = torch.full((rows, ld), float("nan"), dtype=x.dtype, device=x.device)
    view = wide[:, off:off + cols]
    view.copy_(x)
    return view


def stored(op_x, trans):
    """the stored form of an operand given as op(X)"""
    return op_x.t().contiguous() if trans else op_x.contiguous()


def out_block(m, n, dev, fill=None):
    """(big, view): an m x n inner block of a sentinel-filled tensor"""
    big = torch.full((m + 2, n + 5), SENTINEL, dtype=torch.float32, device=dev)
    view = big[1:m + 1, 2:n + 2]
    if fill is not None:
        view.copy_(fill)
    return big, view


def border_intact(big, m, n):
    ref = torch.full_like(big, SENTINEL)
    ref[1:m + 1, 2:n + 2] = big[1:m + 1, 2:n + 2]
    return torch.equal(big, ref)


def k_slice(x, trans_stored_k_first, lo, hi):
    return x[lo:hi] if trans_stored_k_first else x[:, lo:hi]


def shapes():
    for m, n, k in itertools.product(MS, NS, KS):
        yield m, n, k


def ints(shape, lo, hi, gen, dev):
    return torch.randint(lo, hi + 1, shape, generator=gen, device="cpu").float().to(dev)


# ----------------------------------------------------------------------------- exact
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_integer_products_are_exact_for_every_split(GO, gpu_device, layout):
    """The reference is the integer product: float64 on the device is exact here (every partial sum below 2^53), converted
    to int64 and compared with torch.equal."""
    ta, tb = layout
    dev = gpu_device
    gen = torch.Generator().manual_seed(11)
    cases = list(shapes()) + ([LONG] if layout == (False, True) else [])
    for (m, n, k) in cases:
        a_op, b_op = ints((m, k), -3, 3, gen, dev), ints((k, n), -3, 3, gen, dev)
        c0, bias = ints((m, n), -5, 5, gen, dev), ints((n,), -5, 5, gen, dev)
        a, b = embed(stored(a_op, ta)), embed(stored(b_op, tb))
        prod = (a_op.double() @ b_op.double()).long()
        assert int(prod.abs().max()) <= 9 * k <= 691200
        for splits in SPLITS:
            for alpha, beta in ((1.0, 0.0), (2.0, 1.0), (1.0, 1.0), (2.0, 0.0)):
                use_bias = beta == 1.0
                big, out = out_block(m, n, dev, c0)
                got = GO.gemm_ordered(a, b, ta, tb, alpha=alpha, beta=beta, out=out, bias=bias if use_bias else None,
                                      splits=splits)
                assert got is out
                want = int(alpha) * prod + int(beta) * c0.long() + (bias.long() if use_bias else 0)
                assert torch.equal(out.long(), want) and torch.equal(out, want.float()), (layout, m, n, k, splits, alpha, beta)
                assert border_intact(big, m, n), (layout, m, n, k, splits)


def test_k_zero_gives_beta_c_plus_bias(GO, gpu_device):
    dev = gpu_device
    c0 = torch.randn(5, 7, device=dev)
    bias = torch.randn(7, device=dev)
    for ta, tb in LAYOUTS:
        a = torch.empty((0, 5) if ta else (5, 0), device=dev)
        b = torch.empty((7, 0) if tb else (0, 7), device=dev)
        out = c0.clone()
        GO.gemm_ordered(a, b, ta, tb, alpha=3.0, beta=2.0, out=out, bias=bias, splits=4)
        V.same_bits(out, torch.addcmul(bias.expand(5, 7), torch.full_like(c0, 2.0), c0), "k = 0")
        V.same_bits(GO.gemm_ordered(a, b, ta, tb), torch.zeros(5, 7, device=dev), "k = 0, no C")


# ----------------------------------------------------------------------------- defined order
def operands(kind, m, n, k, seed, dev):
    gen = torch.Generator().manual_seed(seed)
    if kind == "normal":
        return torch.randn(m, k, generator=gen).to(dev), torch.randn(k, n, generator=gen).to(dev)
    return torch.rand(m, k, generator=gen).to(dev), torch.rand(k, n, generator=gen).to(dev)     # same sign: the sum only grows


@pytest.mark.parametrize("kind", ["normal", "uniform"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_the_splits_are_added_in_ascending_order(GO, gpu_device, layout, kind):
    """splits = S against the unsplit results of the k-slices the partition names, added ((p0 + p1) + p2) + ... by torch in
    float32: a tree sum, a descending sum or a boundary off the stated one changes bits of these operands."""
    ta, tb = layout
    dev = gpu_device
    cases = [(127, 129, 17), (129, 300, 4097), (1, 1, 4097), (127, 1, 4097)] + ([LONG] if layout == (False, True) else [])
    distinct = 0
    for (m, n, k) in cases:
        a_op, b_op = operands(kind, m, n, k, 5 + k, dev)
        a, b = embed(stored(a_op, ta)), embed(stored(b_op, tb))
        whole = GO.gemm_ordered(a, b, ta, tb, splits=1)
        for splits in (2, 3, 7, 256):
            s_eff, per = GO.partition(k, splits)
            got = GO.gemm_ordered(a, b, ta, tb, splits=splits)
            want = None
            parts = []
            for z in range(s_eff):
                lo, hi = z * per, min(k, (z + 1) * per)
                p = GO.gemm_ordered(k_slice(a, ta, lo, hi), k_slice(b, not tb, lo, hi), ta, tb, splits=1)
                parts.append(p)
                want = p if want is None else want + p
            V.same_bits(got, want, f"{layout} {m}x{n}x{k} splits {splits}")
            if s_eff > 2 and m * n > 1000:
                back = parts[-1]
                for p in reversed(parts[:-1]):
                    back = back + p
                distinct += int(not torch.equal(back, want)) + int(not torch.equal(whole, want))
    assert distinct > 0          # the check can tell: descending order / the unsplit chain differ somewhere on these operands


# ----------------------------------------------------------------------------- float64, per element
def reference(a_op, b_op, alpha=1.0, beta=0.0, c0=None, bias=None):
    """(float64 result, per-element scale, r of torch's own float32 evaluation) on the same float32 inputs"""
    a64, b64 = a_op.double(), b_op.double()
    want = alpha * (a64 @ b64)
    scale = abs(alpha) * (a64.abs() @ b64.abs())
    t32 = alpha * (a_op @ b_op)
    if c0 is not None and beta != 0.0:
        want = want + beta * c0.double()
        scale = scale + abs(beta) * c0.double().abs()
        t32 = t32 + beta * c0
    if bias is not None:
        want = want + bias.double()
        scale = scale + bias.double().abs()
        t32 = t32 + bias
    return want, scale, OA.componentwise(t32, want, scale)[0]


def measure(got, a_op, b_op):
    want, scale, r32 = reference(a_op, b_op)
    return OA.componentwise(got, want, scale)[0], r32


WORST = {"ratio": 0.0}


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_every_element_is_within_the_stated_bound_of_float64(GO, gpu_device, layout):
    ta, tb = layout
    dev = gpu_device
    prev = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        cases = list(shapes()) + ([LONG] if layout == (False, True) else [])
        for (m, n, k) in cases:
            for kind in ("normal", "uniform"):
                a_op, b_op = operands(kind, m, n, k, 3 + m + n + k, dev)
                gen = torch.Generator().manual_seed(m * n + k)
                c0, bias = torch.randn(m, n, generator=gen).to(dev), torch.randn(n, generator=gen).to(dev)
                a, b = embed(stored(a_op, ta)), embed(stored(b_op, tb))
                for alpha, beta, use in ((1.0, 0.0, False), (2.0, 1.0, True)):
                    want, scale, r32 = reference(a_op, b_op, alpha, beta, c0, bias if use else None)      # once per case
                    for splits in SPLITS:
                        s = splits if splits is not None else GO.gemm_ordered_splits(m, n, k, ta, tb)
                        s_eff, per = GO.partition(k, s)
                        _, out = out_block(m, n, dev, c0)
                        GO.gemm_ordered(a, b, ta, tb, alpha=alpha, beta=beta, out=out, bias=bias if use else None,
                                        splits=splits)
                        r = OA.componentwise(out, want, scale)[0]
                        limit = OA.bound_for("f32_mfma", r32, per + s_eff)
                        WORST["ratio"] = max(WORST["ratio"], r / limit)
                        assert r <= limit, (layout, m, n, k, kind, splits, alpha, beta, r, r32, limit)
    finally:
        torch.backends.cuda.matmul.allow_tf32 = prev
    print(f"gemm_ordered {LAYOUT_IDS[LAYOUTS.index(layout)]}: worst r / bound so far {WORST['ratio']:.3f}")


# ----------------------------------------------------------------------------- without tolerance
@pytest.fixture(scope="module")
def fixed(gpu_device):
    m, n, k = 129, 300, 4097
    a_op, b_op = operands("normal", m, n, k, 77, gpu_device)
    return m, n, k, a_op, b_op


@pytest.mark.parametrize("splits", [1, 7, None])
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_runs_poison_and_a_side_stream_change_no_bit(GO, gpu_device, fixed, layout, splits):
    ta, tb = layout
    m, n, k, a_op, b_op = fixed
    a, b = embed(stored(a_op, ta)), embed(stored(b_op, tb))
    first = GO.gemm_ordered(a, b, ta, tb, splits=splits)
    for run in range(2):
        V.same_bits(GO.gemm_ordered(a, b, ta, tb, splits=splits), first, f"run {run + 2}")
    with V.poisoned():
        V.same_bits(GO.gemm_ordered(a, b, ta, tb, splits=splits), first, "poisoned scratch")
    with V.side_stream():
        got = GO.gemm_ordered(a, b, ta, tb, splits=splits)
    V.same_bits(got, first, "side stream")
    with V.side_stream(), V.poisoned(0x7F):
        got = GO.gemm_ordered(a, b, ta, tb, splits=splits)
    V.same_bits(got, first, "side stream, poisoned")


@pytest.mark.parametrize("splits", [1, 7])
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_an_element_depends_on_its_row_its_column_and_the_partition_alone(GO, gpu_device, fixed, layout, splits):
    ta, tb = layout
    dev = gpu_device
    m, n, k, a_op, b_op = fixed
    a, b = embed(stored(a_op, ta)), embed(stored(b_op, tb))
    first = GO.gemm_ordered(a, b, ta, tb, splits=splits)
    # rows of op(A) permuted
    perm = torch.randperm(m, generator=torch.Generator().manual_seed(1)).to(dev)
    V.same_bits(GO.gemm_ordered(embed(stored(a_op[perm], ta)), b, ta, tb, splits=splits), first[perm], "rows permuted")
    # one row alone (m = 1: another tile shape, another count of workgroups)
    for i in (0, 77, m - 1):
        V.same_bits(GO.gemm_ordered(embed(stored(a_op[i:i + 1], ta)), b, ta, tb, splits=splits), first[i:i + 1], f"row {i} alone")
    # a column subset of op(B)
    cols = torch.tensor([299, 0, 128, 127, 5], device=dev)
    V.same_bits(GO.gemm_ordered(a, embed(stored(b_op[:, cols], tb)), ta, tb, splits=splits), first[:, cols], "column subset")
    # aligned copies (the 16-byte load path) against the misaligned ones
    a_al, b_al = embed(stored(a_op, ta), off=0), embed(stored(b_op, tb), off=0)
    assert a_al.data_ptr() % 16 == 0 and a_al.stride(0) % 4 == 0 and a.data_ptr() % 16 != 0
    V.same_bits(GO.gemm_ordered(a_al, b_al, ta, tb, splits=splits), first, "aligned operands")
    V.same_bits(GO.gemm_ordered(a_al, b, ta, tb, splits=splits), first, "a aligned, b not")
    # out given (an inner block of a larger tensor) against a fresh output
    big, out = out_block(m, n, dev)
    GO.gemm_ordered(a, b, ta, tb, out=out, splits=splits)
    V.same_bits(out, first, "out given")
    assert border_intact(big, m, n)


# ----------------------------------------------------------------------------- matmul_ordered
@pytest.mark.parametrize("needs", [(True, True), (True, False), (False, True)], ids=["a+b", "a", "b"])
def test_matmul_ordered_gradients(GO, gpu_device, needs):
    dev = gpu_device
    m, k, n = 1030, 1100, 70
    a_op, b_op = operands("normal", m, n, k, 21, dev)
    g = torch.randn(m, n, generator=torch.Generator().manual_seed(22)).to(dev)
    a, b = a_op.clone().requires_grad_(needs[0]), b_op.clone().requires_grad_(needs[1])
    y = GO.matmul_ordered(a, b)
    assert y.requires_grad

    def bound(got, x_op, y_op, red):
        r, r32 = measure(got, x_op, y_op)
        s_eff, per = GO.partition(red, GO.gemm_ordered_splits(got.shape[0], got.shape[1], red))
        limit = OA.bound_for("f32_mfma", r32, per + s_eff)
        assert r <= limit, (r, r32, limit)

    bound(y.detach(), a_op, b_op, k)
    y.backward(g)
    if needs[0]:
        bound(a.grad, g, b_op.t(), n)
    else:
        assert a.grad is None
    if needs[1]:
        bound(b.grad, a_op.t(), g, m)
    else:
        assert b.grad is None
    # a gradient nobody needs is None at the Function itself, and is not launched
    calls = []
    real = GO.gemm_ordered
    with contextlib.ExitStack() as stack:
        GO.gemm_ordered = lambda *args, **kw: (calls.append((kw.get("trans_a", False), kw.get("trans_b", False))), real(*args, **kw))[1]
        stack.callback(setattr, GO, "gemm_ordered", real)
        a2, b2 = a_op.clone().requires_grad_(needs[0]), b_op.clone().requires_grad_(needs[1])
        GO.matmul_ordered(a2, b2).backward(g)
    assert calls == [(False, False)] + ([(False, True)] if needs[0] else []) + ([(True, False)] if needs[1] else []), calls
    if needs[0]:
        V.same_bits(a2.grad, a.grad, "dA repeats")
    if needs[1]:
        V.same_bits(b2.grad, b.grad, "dB repeats")
