"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle and the golden fixtures
generated from the reference.  Tolerances: integer indices bit-exact; fp32 values within 1e-4
(BASELINE.json north_star), most checks far tighter.  Run with ``-m gpu`` on the MI355X box."""
import os

import numpy as np
import pytest
import torch

from conftest import golden_cfg, golden_names, golden_params, load_golden

pytestmark = pytest.mark.gpu

TOL = 1e-4


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


def rand_graph(rng, n, e, n_rel=5, long_rows=()):
    h = (n * rng.random(e) ** 1.7).astype(np.int64)
    t = rng.integers(0, n, e)
    r = rng.integers(0, n_rel, e)
    for row, deg in long_rows:
        h = np.concatenate([h, np.full(deg, row)])
        t = np.concatenate([t, rng.choice(n, deg, replace=deg > n)])
        r = np.concatenate([r, rng.integers(0, n_rel, deg)])
    trip = np.unique(np.stack([h, r, t], 1), axis=0)
    trip = trip[(trip[:, 0] % 37) != 5]                     # rows 5, 42, 79, ... stay empty
    trip = trip[rng.permutation(len(trip))]
    return trip[:, 0].copy(), trip[:, 2].copy(), trip[:, 1].copy()


def coo_of(graph, val):
    return torch.sparse_coo_tensor(graph.coo_indices().cpu(), val.cpu(), (graph.n, graph.n)).coalesce()


# ----------------------------------------------------------------------------- K3/K4 SpMM
@pytest.mark.parametrize("d", [1, 4, 5, 7, 8, 16, 20, 30, 32, 64, 100, 128, 256, 300, 512, 1028])
def test_spmm_matches_oracle(L, ops, O, gpu_device, d):
    rng = np.random.default_rng(d)
    n = 700
    h, t, r = rand_graph(rng, n, 6000, long_rows=[(3, 65), (10, 200), (501, 640)])
    g = L.KGStructure.from_triples(n, h, t, r, device=gpu_device)
    val = torch.rand(g.nnz, device=gpu_device)
    x = torch.randn(n, d, device=gpu_device)
    want = O.aggregate(coo_of(g, val), x.cpu())
    got = ops.spmm_raw(g.rowptr, g.col, val, x, n)
    torch.testing.assert_close(got.cpu(), want, rtol=1e-5, atol=5e-5)   # 640-term fp32 sums, other order
    # the long-row workgroup path (row 501 holds > 256 entries) gives the same result
    assert g.long_rows(False) is not None and 501 in g.long_rows(False).tolist()
    got_l = ops.spmm_raw(g.rowptr, g.col, val, x, n, long_rows=g.long_rows(False))
    torch.testing.assert_close(got_l.cpu(), want, rtol=1e-5, atol=5e-5)
    # rows without entries are exact zeros
    empty = (g.rowptr[1:] == g.rowptr[:-1]).cpu()
    assert empty.any() and float(got.cpu()[empty].abs().max()) == 0.0
    # transpose pass == A^T @ grad
    gt = ops.spmm_raw(g.t_rowptr, g.t_col, ops.permute_values(val, g.t_perm), x, n)
    torch.testing.assert_close(gt.cpu(), torch.matmul(coo_of(g, val).t(), x.cpu()), rtol=1e-5, atol=5e-5)


@pytest.mark.parametrize("d", [12, 32, 48, 256])
def test_spmm_self_add_row_ranges_and_offsets(L, ops, O, gpu_device, d):
    """The forms the layers and the sharded paths use: out = self + A @ x, a row sub-range through a rowptr view
    (with its own long-row list), and a source table handed over as a row block with x_row_offset."""
    rng = np.random.default_rng(100 + d)
    n = 900
    h, t, r = rand_graph(rng, n, 9000, long_rows=[(7, 300), (450, 700), (899, 1)])
    g = L.KGStructure.from_triples(n, h, t, r, device=gpu_device)
    val = torch.rand(g.nnz, device=gpu_device)
    x = torch.randn(n, d, device=gpu_device)
    own = torch.randn(n, d, device=gpu_device)
    full = O.aggregate(coo_of(g, val), x.cpu())
    got = ops.spmm_raw(g.rowptr, g.col, val, x, n, long_rows=g.long_rows(False), add_self=own)
    torch.testing.assert_close(got.cpu(), full + own.cpu(), rtol=1e-5, atol=5e-5)
    # in place: out = out + A @ x
    acc = own.clone()
    ops.spmm_raw(g.rowptr, g.col, val, x, n, out=acc, long_rows=g.long_rows(False), add_self=acc)
    torch.testing.assert_close(acc.cpu(), full + own.cpu(), rtol=1e-5, atol=5e-5)
    for lo, hi in ((0, 13), (5, 460), (449, 451), (600, 900), (123, 123)):
        part = ops.spmm_raw(g.rowptr[lo:hi + 1], g.col, val, x, hi - lo, long_rows=g.long_rows(False, lo, hi))
        torch.testing.assert_close(part.cpu(), full[lo:hi], rtol=1e-5, atol=5e-5)
    # transpose pass restricted to the heads [lo, hi): the source is only that row block (ShardedAggregation)
    lo, hi = 200, 640
    keep = (h >= lo) & (h < hi)
    gs = L.KGStructure.from_triples(n, h[keep], t[keep], r[keep], device=gpu_device)
    vs = torch.rand(gs.nnz, device=gpu_device)
    grad_rows = torch.randn(hi - lo, d, device=gpu_device)
    got_t = ops.spmm_raw(gs.t_rowptr, gs.t_col, ops.permute_values(vs, gs.t_perm), grad_rows, n, x_row_offset=lo,
                         long_rows=gs.long_rows(True))
    padded = torch.zeros(n, d)
    padded[lo:hi] = grad_rows.cpu()
    torch.testing.assert_close(got_t.cpu(), torch.matmul(coo_of(gs, vs).t(), padded), rtol=1e-5, atol=5e-5)


def test_spmm_narrow_rows_agree_with_the_wave_per_row_kernel_at_scale(L, ops, gpu_device):
    """The rows-per-wave kernel (rows of <= 32 floats: the D/G slabs of the feature-sharded run) against the
    wave-per-row kernel on a large skewed graph: the same 32 columns, once alone and once as the left half of a
    64-column table, forward and transpose, long rows included -- bit-identical row sums are not required (other
    summation order), 1e-5 relative is."""
    rng = np.random.default_rng(77)
    n, e = 2_000_000, 40_000_000
    perm = rng.permutation(n)
    h = perm[np.minimum((n * rng.random(e) ** 1.75).astype(np.int64), n - 1)]
    t = rng.integers(0, n, e, dtype=np.int64)
    g = L.KGStructure.from_triples(n, h, t, None, device=gpu_device)
    del h, t
    assert g.long_rows(False) is not None
    gen = torch.Generator(device=gpu_device).manual_seed(5)
    wide = torch.rand((n, 64), generator=gen, device=gpu_device)
    wide[:, 32:] = 0
    narrow = wide[:, :32].contiguous()
    val = torch.rand(g.nnz, generator=gen, device=gpu_device)
    val_t = ops.permute_values(val, g.t_perm)
    for rp, cl, vl, lr in ((g.rowptr, g.col, val, g.long_rows(False)), (g.t_rowptr, g.t_col, val_t, g.long_rows(True))):
        a = ops.spmm_raw(rp, cl, vl, narrow, n, long_rows=lr)
        b = ops.spmm_raw(rp, cl, vl, wide, n, long_rows=lr)
        assert float(b[:, 32:].abs().max()) == 0.0
        scale = float(b.abs().max())
        assert float((a - b[:, :32]).abs().max()) <= 1e-5 * scale
        deg = (rp[1:] - rp[:-1])
        empty = (deg == 0)
        assert float(a[empty].abs().max()) == 0.0 if bool(empty.any()) else True

def test_spmm_strided_views_and_autograd(L, ops, O, gpu_device):
    rng = np.random.default_rng(5)
    n, d = 300, 64
    h, t, r = rand_graph(rng, n, 2500)
    g = L.KGStructure.from_triples(n, h, t, r, device=gpu_device)
    val = torch.rand(g.nnz, device=gpu_device)
    big = torch.randn(n, 3 * d, device=gpu_device)
    x = big[:, d:2 * d]                       # column slice: row stride 3d
    outbuf = torch.zeros(n, 2 * d, device=gpu_device)
    ops.spmm_raw(g.rowptr, g.col, val, x, n, out=outbuf[:, d:])
    want = O.aggregate(coo_of(g, val), x.cpu())
    torch.testing.assert_close(outbuf[:, d:].cpu(), want, rtol=1e-5, atol=1e-5)
    assert float(outbuf[:, :d].abs().max()) == 0.0
    from literalkg_amd.model import AttentionCSR
    att = AttentionCSR(g, val)
    xg = x.clone().requires_grad_(True)
    w = torch.randn(n, d, device=gpu_device)
    (att.aggregate(xg) * w).sum().backward()
    xc = x.cpu().clone().requires_grad_(True)
    (O.aggregate(coo_of(g, val), xc) * w.cpu()).sum().backward()
    torch.testing.assert_close(xg.grad.cpu(), xc.grad, rtol=1e-5, atol=1e-5)


def test_spmm_empty_and_ragged(L, ops, gpu_device):
    n = 9
    g = L.KGStructure.from_triples(n, np.array([8, 8, 8]), np.array([0, 4, 8]), np.array([0, 0, 1]), device=gpu_device)
    x = torch.arange(n * 4, dtype=torch.float32, device=gpu_device).reshape(n, 4)
    val = torch.tensor([1.0, 2.0, 3.0], device=gpu_device)
    got = ops.spmm_raw(g.rowptr, g.col, val, x, n).cpu()
    assert float(got[:8].abs().max()) == 0.0
    torch.testing.assert_close(got[8], (x[0] + 2 * x[4] + 3 * x[8]).cpu())
    g0 = L.KGStructure.from_triples(n, np.zeros(0, np.int64), np.zeros(0, np.int64), None, device=gpu_device)
    z = ops.spmm_raw(g0.rowptr, g0.col, torch.zeros(0, device=gpu_device), x, n)
    assert float(z.abs().max()) == 0.0


# ----------------------------------------------------------------------------- K1+K2 attention
@pytest.mark.parametrize("name", golden_names("attention_"))
def test_attention_refresh_golden(L, ops, gpu_device, name):
    gd = load_golden(name)
    n = int(gd["n"])
    g = L.KGStructure.from_triples(n, gd["h"], gd["t"], gd["r"], device=gpu_device)
    ent, rel = torch.from_numpy(gd["entity"]).to(gpu_device), torch.from_numpy(gd["relation"]).to(gpu_device)
    val, logits = ops.edge_softmax(g, ent, rel, want_logits=True)
    assert np.array_equal(g.coo_indices().cpu().numpy(), gd["a_indices"])          # int64, bit-exact
    np.testing.assert_allclose(val.cpu().numpy(), gd["a_values"], rtol=1e-5, atol=1e-7)
    # merged logits: sum the reference's per-edge logits over duplicate (h,t) pairs
    key = gd["h"] * n + gd["t"]
    uk, inv = np.unique(key, return_inverse=True)
    merged = np.zeros(len(uk))
    np.add.at(merged, inv, gd["logits"].astype(np.float64))
    np.testing.assert_allclose(logits.cpu().numpy(), merged, rtol=1e-5, atol=1e-6)
    assert g.has_dups == (len(uk) < len(key))


@pytest.mark.parametrize("d", [8, 64, 100, 128, 256, 512])
def test_attention_refresh_random(L, ops, O, gpu_device, d):
    rng = np.random.default_rng(100 + d)
    n = 500
    h, t, r = rand_graph(rng, n, 5000, n_rel=6, long_rows=[(7, 70), (9, 333)])
    # force duplicate (h,t) pairs, some tripled
    extra = np.stack([h[:40], (r[:40] + 1) % 6, t[:40]], 1)
    extra2 = np.stack([h[:10], (r[:10] + 2) % 6, t[:10]], 1)
    trip = np.unique(np.concatenate([np.stack([h, r, t], 1), extra, extra2]), axis=0)
    h, r, t = trip[:, 0].copy(), trip[:, 1].copy(), trip[:, 2].copy()
    ent = torch.randn(n, d) * 0.5
    rel = torch.randn(6, d) * 0.5
    g = L.KGStructure.from_triples(n, h, t, r, device=gpu_device)
    assert g.has_dups
    val, _ = ops.edge_softmax(g, ent.to(gpu_device), rel.to(gpu_device))
    rows, cols, want = O.attention_refresh_explicit(n, ent, rel, *(torch.from_numpy(a) for a in (h, t, r)))
    assert torch.equal(g.coo_indices().cpu(), torch.stack([rows, cols]))
    torch.testing.assert_close(val.cpu(), want, rtol=1e-4, atol=1e-6)
    ref = O.attention_refresh(n, ent, rel, *(torch.from_numpy(a) for a in (h, t, r))).coalesce()
    torch.testing.assert_close(val.cpu(), ref.values(), rtol=1e-4, atol=1e-6)


# ----------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("m,n,k", [(1, 1, 1), (130, 70, 33), (257, 300, 558), (1000, 256, 256), (64, 128, 16),
                                   (5, 260, 1030)])
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm(ops, gpu_device, m, n, k, ta, tb):
    gen = torch.Generator().manual_seed(m * 7 + n * 3 + k + ta * 2 + tb)
    a = torch.randn((k, m) if ta else (m, k), generator=gen)
    b = torch.randn((n, k) if tb else (k, n), generator=gen)
    bias = torch.randn(n, generator=gen)
    c0 = torch.randn(m, n, generator=gen)
    want = (a.t() if ta else a).double() @ (b.t() if tb else b).double()
    got = ops.gemm(a.to(gpu_device), b.to(gpu_device), bool(ta), bool(tb))
    torch.testing.assert_close(got.cpu().double(), want, rtol=1e-5, atol=1e-4 * max(1, k) ** 0.5)
    got2 = ops.gemm(a.to(gpu_device), b.to(gpu_device), bool(ta), bool(tb), alpha=0.5, beta=2.0,
                    out=c0.clone().to(gpu_device), bias=bias.to(gpu_device))
    torch.testing.assert_close(got2.cpu().double(), 0.5 * want + 2.0 * c0.double() + bias.double(), rtol=1e-5,
                               atol=1e-4 * max(1, k) ** 0.5)


@pytest.mark.parametrize("k,n,tb", [(256, 256, True), (300, 256, True), (558, 200, True), (128, 128, False), (2, 256, True),
                                     (17, 40, False)])
def test_gemm_split_engine_is_f32_accurate(ops, gpu_device, k, n, tb):
    """Tall products with a small B run on the bf16 x 3 engine (m >= 16384 rows): it must be as close to the f64
    product as an f32 GEMM is (a few 1e-7 of the result's scale), also on edge tiles, partial k tiles, column slices
    and with alpha / beta / bias; below the row threshold the f32-MFMA engine gives the same numbers."""
    gen = torch.Generator().manual_seed(k * 1000 + n)
    m = 16384 + 77
    a = torch.randn(m, k + 4, generator=gen)[:, 4:].to(gpu_device) if k % 4 == 0 else torch.randn(m, k, generator=gen).to(gpu_device)
    b = torch.randn((n, k) if tb else (k, n), generator=gen).to(gpu_device) * 0.1
    want = a.double() @ (b.double().t() if tb else b.double())
    scale = float(want.abs().max())
    got = ops.gemm(a, b, trans_b=tb)
    err = float((got.double() - want).abs().max()) / scale
    f32 = float((torch.matmul(a, b.t() if tb else b).double() - want).abs().max()) / scale
    assert err <= max(2.0 * f32, 1e-6), (err, f32)
    small = ops.gemm(a[:300], b, trans_b=tb)                  # under the threshold: f32 MFMA engine
    torch.testing.assert_close(small, got[:300], rtol=1e-5, atol=2e-6 * scale)
    bias = torch.randn(n, generator=gen).to(gpu_device)
    c0 = torch.randn(m, n, generator=gen).to(gpu_device)
    got2 = ops.gemm(a, b, trans_b=tb, alpha=0.5, beta=2.0, out=c0.clone(), bias=bias)
    torch.testing.assert_close(got2.double(), 0.5 * want + 2.0 * c0.double() + bias.double(), rtol=1e-5,
                               atol=4e-6 * scale)


@pytest.mark.parametrize("m,n,k", [(256, 256, 30000), (96, 300, 5000), (130, 70, 2048), (256, 128, 4099)])
def test_gemm_weight_gradient_engine_is_f32_accurate(ops, gpu_device, m, n, k):
    """A^T B with both operands k-major and k >= 2048 (nn.Linear weight gradients) runs on the second bf16 x 3 engine
    (transposing LDS reads, split-K atomics): as close to f64 as torch's f32 result, edge tiles and partial k tiles
    included; below the k threshold the f32-MFMA engine gives the same numbers."""
    gen = torch.Generator().manual_seed(m + n + k)
    a = torch.randn(k, m, generator=gen).to(gpu_device)
    b = torch.randn(k, n, generator=gen).to(gpu_device)
    want = a.double().t() @ b.double()
    scale = float(want.abs().max())
    got = ops.gemm(a, b, trans_a=True)
    err = float((got.double() - want).abs().max()) / scale
    f32 = float((torch.matmul(a.t(), b).double() - want).abs().max()) / scale
    assert err <= max(2.0 * f32, 2e-6), (err, f32)
    head = ops.gemm(a[:2000], b[:2000], trans_a=True)          # k < 2048: f32 MFMA engine
    want_head = a[:2000].double().t() @ b[:2000].double()
    torch.testing.assert_close(head.double(), want_head, rtol=1e-5, atol=2e-6 * float(want_head.abs().max()))


@pytest.mark.parametrize("ks,n,tb", [((256,), 256, True), ((256, 2, 300), 256, True), ((64, 64), 128, True), ((30, 7), 50, True),
                                     ((256,), 256, False), ((512,), 300, True), ((3,), 5, False), ((128, 128), 64, False)])
def test_gemm_tall_f16x2_engine_is_f32_accurate(ops, gpu_device, ks, n, tb):
    """lkg_gemm_tall_f32 (row-scaled fp16 hi/mid split, 3 MFMAs per product): against f64 it is within a small factor
    of an f32 GEMM's own rounding error -- multi-panel A from different arrays, unaligned / odd widths, edge tiles,
    alpha / beta / bias -- and rows spanning 60 orders of magnitude keep that accuracy relative to their own scale."""
    gen = torch.Generator().manual_seed(sum(ks) * 1000 + n)
    m = 16384 + 77
    panels = [torch.randn(m, k + 3, generator=gen)[:, 3:].to(gpu_device) if i % 2 else torch.randn(m, k, generator=gen).to(gpu_device)
              for i, k in enumerate(ks)]
    blocks = [(torch.randn((n, k) if tb else (k, n), generator=gen) * 0.1).to(gpu_device) for k in ks]
    a64 = torch.cat([p.double() for p in panels], 1)
    b64 = torch.cat([b.double() if tb else b.double().t() for b in blocks], 1)          # [n, K]
    want = a64 @ b64.t()
    scale = float(want.abs().max())
    got = ops.gemm_tall(panels, (blocks,), tb)
    err = float((got.double() - want).abs().max()) / scale
    f32 = float(((a64.float() @ b64.float().t()).double() - want).abs().max()) / scale
    assert err <= max(3.0 * f32, 1e-6), (err, f32)
    bias = torch.randn(n, generator=gen).to(gpu_device)
    c0 = torch.randn(m, n + 5, generator=gen).to(gpu_device)[:, 5:]                     # strided output
    got2 = ops.gemm_tall(panels, (blocks,), tb, bias, alpha=0.5, beta=2.0, out=c0.clone())
    torch.testing.assert_close(got2.double(), 0.5 * want + 2.0 * c0.double() + bias.double(), rtol=1e-5,
                               atol=4e-6 * scale)
    # per-row dynamic range: every row is accurate relative to ITS OWN magnitude (power-of-two row scaling)
    exps = torch.randint(-30, 30, (m, 1), generator=gen).float()
    mags = torch.pow(torch.tensor(10.0), exps).to(gpu_device)
    mags[5] = 0.0                                                                       # an all-zero row
    scaled = [p * mags for p in panels]
    got3 = ops.gemm_tall(scaled, (blocks,), tb)
    want3 = torch.cat([p.double() for p in scaled], 1) @ b64.t()
    row_scale = want3.abs().amax(dim=1, keepdim=True).clamp_min(1e-300)
    rel = ((got3.double() - want3).abs() / row_scale)
    assert float(rel.max()) <= max(30.0 * f32, 1e-5), float(rel.max())
    assert float(got3[5].abs().max()) == 0.0
    # one huge element in a row of small ones: the small ones keep ~f32 accuracy (22 bits down to 2^-27 of the row max)
    spiky = [p.clone() for p in panels]
    spiky[0][:, 0] = 3000.0
    blocks0 = [b.clone() for b in blocks]
    if tb:
        blocks0[0][:, 0] = 0.0
    else:
        blocks0[0][0, :] = 0.0                                                          # the spike meets a zero weight
    got4 = ops.gemm_tall(spiky, (blocks0,), tb)
    b0 = torch.cat([b.double() if tb else b.double().t() for b in blocks0], 1)
    want4 = torch.cat([p.double() for p in spiky], 1) @ b0.t()
    err4 = float((got4.double() - want4).abs().max()) / float(want4.abs().max())
    assert err4 <= max(10.0 * f32, 5e-6), (err4, f32)


@pytest.mark.parametrize("variant", ["256x2", "256x1", "128x1"])
@pytest.mark.parametrize("ks,n,tb", [((256,), 256, True), ((256, 2, 300), 256, True), ((512,), 300, True), ((30, 7), 50, False),
                                     ((40,), 200, True), ((16,), 600, True), ((3, 5, 2), 130, False)])
def test_gemm_tall_every_tiling_variant_is_f32_accurate(ops, gpu_device, variant, ks, n, tb):
    """Every tiling of lkg_gemm_tall_f32 (bits 8-15 of its `epilogue` argument) against float64 on the same operands: the
    two-accumulator form, the one-accumulator form and the 128-column form -- plain product, alpha / beta / bias into a
    strided output, rows of very different magnitude."""
    gen = torch.Generator().manual_seed(sum(ks) * 1000 + n + 7)
    m = 16384 + 131
    panels = [torch.randn(m, k + 1, generator=gen)[:, 1:].to(gpu_device) if i % 2 else torch.randn(m, k, generator=gen).to(gpu_device)
              for i, k in enumerate(ks)]
    blocks = [(torch.randn((n, k) if tb else (k, n), generator=gen) * 0.1).to(gpu_device) for k in ks]
    a64 = torch.cat([p.double() for p in panels], 1)
    b64 = torch.cat([b.double() if tb else b.double().t() for b in blocks], 1)
    want = a64 @ b64.t()
    scale = float(want.abs().max())
    f32 = float(((a64.float() @ b64.float().t()).double() - want).abs().max()) / scale
    got = ops.gemm_tall(panels, (blocks,), tb, variant=variant)
    err = float((got.double() - want).abs().max()) / scale
    assert err <= max(3.0 * f32, 1e-6), (variant, err, f32)
    bias = torch.randn(n, generator=gen).to(gpu_device)
    c0 = torch.randn(m, n + 5, generator=gen).to(gpu_device)[:, 5:]
    got2 = ops.gemm_tall(panels, (blocks,), tb, bias, alpha=0.5, beta=2.0, out=c0.clone(), variant=variant)
    torch.testing.assert_close(got2.double(), 0.5 * want + 2.0 * c0.double() + bias.double(), rtol=1e-5, atol=4e-6 * scale)
    mags = torch.pow(torch.tensor(10.0), torch.randint(-30, 30, (m, 1), generator=gen).float()).to(gpu_device)
    mags[9] = 0.0
    scaled = [p * mags for p in panels]
    got3 = ops.gemm_tall(scaled, (blocks,), tb, variant=variant)
    want3 = torch.cat([p.double() for p in scaled], 1) @ b64.t()
    rel = (got3.double() - want3).abs() / want3.abs().amax(dim=1, keepdim=True).clamp_min(1e-300)
    assert float(rel.max()) <= max(30.0 * f32, 1e-5), (variant, float(rel.max()))
    assert float(got3[9].abs().max()) == 0.0


@pytest.mark.parametrize("variant", ["256x2", "256x1"])
def test_fused_gate_every_tiling_variant(L, ops, O, gpu_device, variant):
    """The gate's one-launch stacked product (blend epilogue) on every 256-column tiling against the oracle's gate."""
    torch.manual_seed(4)
    n, d = 16384 + 77, 300
    old = ops.DEFAULT_TALL_VARIANT
    ops.DEFAULT_TALL_VARIANT = variant
    try:
        gate = L.gate.GateMul(d, 2, 300).to(gpu_device)
        x = (torch.randn(n, d) * 0.3).to(gpu_device)
        num, txt = torch.rand(n, 2).to(gpu_device), torch.randn(n, 300).to(gpu_device)
        got = gate(x, num, txt)
        sd = {k: v.detach().cpu() for k, v in gate.state_dict().items()}
        want = O.gate_mul(sd, "", x.cpu(), num.cpu(), txt.cpu())
    finally:
        ops.DEFAULT_TALL_VARIANT = old
    torch.testing.assert_close(got.cpu(), want.float(), rtol=1e-4, atol=2e-5)


def test_gemm_tall_default_dispatch(ops, gpu_device):
    """What `variant=None` launches: "256x1" above 128 plain output columns, "128x1" up to 128, "256x1" under the gate
    epilogue -- the same bits as the tiling named outright, and finite."""
    gen = torch.Generator().manual_seed(11)
    m, k = 129, 17
    a = torch.randn(m, k, generator=gen).to(gpu_device)

    def same(named, **kw):
        got, want = ops.gemm_tall(variant=None, **kw), ops.gemm_tall(variant=named, **kw)
        assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(want).all()), named
        assert torch.equal(got, want), named
    for n, named in ((130, "256x1"), (128, "128x1")):
        w = torch.randn(n, k, generator=gen).to(gpu_device)
        same(named, a_panels=(a,), b_blocks=((w,),), trans_b=True, bias=torch.randn(n, generator=gen).to(gpu_device))
    d, lits = 32, (2, 5)
    panels = [torch.randn(m, w_, generator=gen).to(gpu_device) for w_ in (d,) + lits]
    groups = [[(torch.randn(d, w_, generator=gen) * 0.3).to(gpu_device) for w_ in (d,) + lits] for _ in range(2)]
    same("256x1", a_panels=panels, b_blocks=groups, trans_b=True, bias=torch.randn(2 * d, generator=gen).to(gpu_device),
         gate_x=panels[0])


@pytest.mark.parametrize("m", [16384 + 5, 40_000])
@pytest.mark.parametrize("ks,n", [((256,), 256), ((64, 64), 128), ((300,), 32), ((256, 300), 200), ((40,), 7), ((128,), 256), ((32,), 32)])
@pytest.mark.parametrize("drop_p", [0.0, 0.25])
def test_fused_layer_epilogue_matches_the_unfused_pair(ops, gpu_device, m, ks, n, drop_p):
    """K5 in one launch (lkg_linear_act_layernorm_fwd_f32: Linear + LeakyReLU + LayerNorm + dropout + normalised copy in the
    tall GEMM's epilogue) against the unfused pair lkg_gemm_tall_f32 + lkg_act_layernorm_fwd_f32 on the
    same operands and the same dropout seed: y, yn, mean, rstd -- and against float64 LayerNorm of the float64 product."""
    gen = torch.Generator().manual_seed(m + n + sum(ks))
    panels = [torch.randn(m, k, generator=gen).to(gpu_device) * (0.5 + i) for i, k in enumerate(ks)]
    ws = [(torch.randn(n, k, generator=gen) * 0.08).to(gpu_device) for k in ks]
    bias = torch.randn(n, generator=gen).to(gpu_device) * 0.1
    gamma = (1 + 0.1 * torch.randn(n, generator=gen)).to(gpu_device)
    beta = (0.1 * torch.randn(n, generator=gen)).to(gpu_device)
    seed = 1234567
    slot = torch.zeros((m, n + 9), device=gpu_device)[:, 4:4 + n]                       # a strided destination, like a CatBuffer slot
    y, yn, mean, rstd = ops.linear_act_layernorm_fwd(panels, ws, bias, gamma, beta, 0.01, 1e-5, 1e-12, drop_p, seed, yn_out=slot)
    z = ops.gemm_tall(panels, (ws,), True, bias) if ops.tall_ok(m, n, ks, True) else \
        sum(p @ w.t() for p, w in zip(panels, ws)) + bias
    y0, yn0 = ops.act_layernorm(z, gamma, beta, want_norm=True, drop_p=drop_p, seed=seed)
    kept = (y0 != 0) == (y != 0)
    assert bool(kept.all()), "the two paths must draw the same dropout mask"
    if n % 4 == 0 and ops.tall_ok(m, n, ks, True) and n > 128:
        # the same GEMM tiling and the row-wise kernel's own arithmetic: bit for bit
        assert torch.equal(y, y0) and torch.equal(yn, yn0), (float((y - y0).abs().max()), float((yn - yn0).abs().max()))
    torch.testing.assert_close(y, y0, rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(yn, yn0, rtol=2e-5, atol=2e-6)
    assert yn.data_ptr() == slot.data_ptr()
    z64 = sum(p.double() @ w.double().t() for p, w in zip(panels, ws)) + bias.double()
    a64 = torch.where(z64 > 0, z64, 0.01 * z64)
    mu, var = a64.mean(1, keepdim=True), a64.var(1, unbiased=False, keepdim=True)
    torch.testing.assert_close(mean.double(), mu[:, 0], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(rstd.double(), (var[:, 0] + 1e-5).rsqrt(), rtol=2e-5, atol=1e-6)
    if drop_p == 0.0:
        want = (a64 - mu) / (var + 1e-5).sqrt() * gamma.double() + beta.double()
        torch.testing.assert_close(y.double(), want, rtol=1e-4, atol=1e-4)     # (fp32 statistics over as few as 7 columns)
        _, yn_only, _, _ = ops.linear_act_layernorm_fwd(panels, ws, bias, gamma, beta, 0.01, 1e-5, 1e-12, 0.0, 0, want_y=False)
        torch.testing.assert_close(yn_only, yn, rtol=0, atol=0)


@pytest.mark.parametrize("n", [4096 + 7, 50_000])
@pytest.mark.parametrize("which", ["both", "y only", "yn only", "yn on some rows"])
@pytest.mark.parametrize("drop_p", [0.0, 0.25])
def test_narrow_layer_backward_in_one_launch_matches_the_unfused_passes(ops, gpu_device, n, which, drop_p):
    """lkg_narrow_layer_bwd_f32 (a 32 -> 32 layer's row-wise backward, data gradient, weight gradient and bias sum in one launch,
    g_z kept in LDS, the two products as f32 MFMAs) against the unfused passes on the same operands and the same dropout seed:
    g_x, g_W, g_b, g_gamma, g_beta to summation-order rounding; and against float64 autograd of the same function."""
    gen = torch.Generator().manual_seed(n + len(which))
    x = (torch.randn(n, 32, generator=gen) * 0.7).to(gpu_device)
    w = (torch.randn(32, 32, generator=gen) * 0.2).to(gpu_device)
    bias = (torch.randn(32, generator=gen) * 0.1).to(gpu_device)
    gamma = (1 + 0.1 * torch.randn(32, generator=gen)).to(gpu_device)
    beta = (0.1 * torch.randn(32, generator=gen)).to(gpu_device)
    gy = torch.randn(n, 32, generator=gen).to(gpu_device) if which in ("both", "y only") else None
    gyn = torch.randn(n, 32, generator=gen).to(gpu_device) if which != "y only" else None
    if which == "yn on some rows":                     # a loss's row-sparse gradient of the normalised copy, too many rows to compact
        keep = (torch.rand(n, generator=gen) < 0.6).to(gpu_device)
        gyn = gyn * keep[:, None]
    seed = 99
    got = {}
    for fused in (True, False):
        leaves = [t.detach().clone().requires_grad_(True) for t in (x, w, bias, gamma, beta)]
        xx, ww, bb, gg, be = leaves
        if fused:
            assert ops.narrow_layer_ok(xx, ww)
            y, yn = ops.narrow_layer(xx, ww, bb, gg, be, drop_p=drop_p, seed=seed)
        else:
            y, yn = ops.act_layernorm(ops.linear(xx, ww, bb), gg, be, drop_p=drop_p, seed=seed)
        torch.autograd.backward([t for t, g in ((y, gy), (yn, gyn)) if g is not None], [g for g in (gy, gyn) if g is not None])
        got[fused] = (y.detach(), yn.detach(), [t.grad for t in leaves])
    assert torch.equal(got[True][0], got[False][0]) and torch.equal(got[True][1], got[False][1])
    for name, a, b in zip(("g_x", "g_w", "g_bias", "g_gamma", "g_beta"), got[True][2], got[False][2]):
        scale = float(b.abs().max()) + 1e-20
        err = float((a - b).abs().max()) / scale
        assert err < (2e-6 if name == "g_x" else 2e-5), (name, err)
    if which == "yn on some rows":
        # the row flags of g_yn (rows whose g_yn is zero are not read at all): the same sums as without them
        from literalkg_amd import _native as N
        z = ops.linear(x, w, bias)
        y, mean, rstd = torch.empty_like(z), torch.empty(n, device=gpu_device), torch.empty(n, device=gpu_device)
        N.call("lkg_act_layernorm_fwd_f32", n, 32, N.ptr(z), 32, 0.01, N.ptr(gamma), N.ptr(beta), 1e-5, N.ptr(y), 32, None, 0, 1e-12,
               N.ptr(mean), N.ptr(rstd), float(drop_p), seed, None)
        torch.cuda.synchronize()
        outs = []
        for flags in (None, keep.to(torch.uint8)):
            gx = torch.empty_like(x)
            sums = torch.empty(1024 + 96, device=gpu_device)
            scratch = torch.empty(int(N.load().lkg_narrow_layer_bwd_workspace(n)), device=gpu_device)
            garbage = gyn if flags is None else torch.where(keep[:, None], gyn, torch.full_like(gyn, float("nan")))
            N.call("lkg_narrow_layer_bwd_f32", n, 32, 32, N.ptr(x), 32, N.ptr(w), 32, N.ptr(z), 32, 0.01, N.ptr(gamma), N.ptr(y), 32,
                   N.ptr(mean), N.ptr(rstd), None, 0, N.ptr(garbage), 32, 1e-12, float(drop_p), seed, N.ptr(flags), N.ptr(gx), 32,
                   N.ptr(sums[:1024]), N.ptr(sums[1024:1056]), N.ptr(sums[1056:1088]), N.ptr(sums[1088:]), N.ptr(scratch),
                   scratch.numel(), None)
            torch.cuda.synchronize()
            outs.append((gx, sums))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])     # (the sums are added in a fixed order)
    if drop_p == 0.0:
        l64 = [t.detach().double().cpu().requires_grad_(True) for t in (x, w, bias, gamma, beta)]
        z64 = l64[0] @ l64[1].t() + l64[2]
        y64 = torch.nn.functional.layer_norm(torch.nn.functional.leaky_relu(z64, 0.01), (32,), l64[3], l64[4], 1e-5)
        yn64 = y64 / y64.norm(dim=1, keepdim=True).clamp_min(1e-12)
        torch.autograd.backward([t for t, g in ((y64, gy), (yn64, gyn)) if g is not None],
                                [g.double().cpu() for g in (gy, gyn) if g is not None])
        for name, a, b in zip(("g_x", "g_w", "g_bias", "g_gamma", "g_beta"), got[True][2], l64):
            err = float((a.double().cpu() - b.grad).abs().max()) / (float(b.grad.abs().max()) + 1e-20)
            assert err < 1e-4, (name, err)


def test_fused_gate_matches_oracle_and_the_unfused_path(L, ops, O, gpu_device):
    """GateMul / Gate through the one-launch stacked GEMM with the blend epilogue (rows >= 16384) against the oracle's
    gate (forward, input gradient, every weight gradient), with literal widths that are not multiples of 4."""
    torch.manual_seed(2)
    n = 16384 + 333
    # (300 / 320 / 288 wide: the last column tile of the stacked product is mostly padding)
    for d, nn_, nt in ((64, 2, 300), (48, 3, 7), (256, 2, 20), (300, 2, 300), (320, 3, 16), (288, 2, 5)):
        gate = L.GateMul(d, nn_, nt).to(gpu_device)
        x = (torch.randn(n, d) * 0.5).to(gpu_device).requires_grad_(True)
        num, txt = torch.rand(n, nn_).to(gpu_device), torch.randn(n, nt).to(gpu_device)
        assert ops.gate_fusable(x, (num, txt), d)
        out = gate(x, num, txt)
        w = torch.randn(n, d, device=gpu_device)
        (out * w).sum().backward()
        p = {("emb_mul_lit." + k): v.detach().cpu().clone().requires_grad_(True) for k, v in gate.state_dict().items()}
        xc = x.detach().cpu().clone().requires_grad_(True)
        ref = O.gate_mul(p, "emb_mul_lit.", xc, num.cpu(), txt.cpu())
        (ref * w.cpu()).sum().backward()
        torch.testing.assert_close(out.detach().cpu(), ref.detach(), rtol=1e-5, atol=2e-6)
        torch.testing.assert_close(x.grad.cpu(), xc.grad, rtol=1e-4, atol=1e-5)
        for k, v in gate.named_parameters():
            ref_g = p["emb_mul_lit." + k].grad
            err = float((v.grad.cpu() - ref_g).abs().max()) / (float(ref_g.abs().max()) + 1e-12)
            assert err < 1e-4, (d, k, err)
    # single-literal gate, written into a column slot of a wider buffer
    gate = L.Gate(32, 5).to(gpu_device)
    x = (torch.randn(n, 32) * 0.5).to(gpu_device)
    lit = torch.randn(n, 5).to(gpu_device)
    buf = torch.zeros(n, 96, device=gpu_device)
    with torch.no_grad():
        out = gate(x, lit, buf[:, 32:64])
    p = {("g." + k): v.detach().cpu() for k, v in gate.state_dict().items()}
    ref = O.gate_single(p, "g.", x.cpu(), lit.cpu())
    torch.testing.assert_close(buf[:, 32:64].cpu(), ref, rtol=1e-5, atol=2e-6)
    assert float(buf[:, :32].abs().max()) == 0.0 and float(buf[:, 64:].abs().max()) == 0.0


def test_gemm_full_size_products_of_the_dense_layer(ops, gpu_device):
    """The three products of one nn.Linear at the BASELINE shape (1 M rows, 256 x 256): every row tile of the forward
    and the data gradient is checked on a strided row sample against f64, the weight gradient as a whole."""
    gen = torch.Generator(device=gpu_device).manual_seed(11)
    n, d = 1_000_000, 256
    x = torch.randn((n, d), generator=gen, device=gpu_device)
    gy = torch.randn((n, d), generator=gen, device=gpu_device)
    w = torch.randn((d, d), generator=gen, device=gpu_device) * 0.06
    b = torch.randn(d, generator=gen, device=gpu_device)
    rows = torch.arange(0, n, 127, device=gpu_device)                 # 7875 rows, every 128-row tile is hit
    y = ops.gemm(x, w, trans_b=True, bias=b)
    want = x[rows].double() @ w.double().t() + b.double()
    torch.testing.assert_close(y[rows].double(), want, rtol=1e-5, atol=2e-6 * float(want.abs().max()))
    gx = ops.gemm(gy, w)
    want = gy[rows].double() @ w.double()
    torch.testing.assert_close(gx[rows].double(), want, rtol=1e-5, atol=2e-6 * float(want.abs().max()))
    gw = ops.gemm(gy, x, trans_a=True)
    want = gy.double().t() @ x.double()
    torch.testing.assert_close(gw.double(), want, rtol=1e-5, atol=4e-6 * float(want.abs().max()))


def test_gemm_split_k_and_slices(ops, gpu_device):
    gen = torch.Generator().manual_seed(3)
    gy = torch.randn(40000, 96, generator=gen)
    x = torch.randn(40000, 200, generator=gen)[:, 8:136]           # column slice, ld 200
    got = ops.gemm(gy.to(gpu_device), x.to(gpu_device), trans_a=True)      # weight-gradient shape, K = 40000
    want = gy.double().t() @ x.double()
    torch.testing.assert_close(got.cpu().double(), want, rtol=1e-4, atol=2e-2)
    w = torch.randn(64, 558, generator=gen)
    xx = torch.randn(300, 256, generator=gen)
    got = ops.gemm(xx.to(gpu_device), w.to(gpu_device)[:, 2:258], trans_b=True)   # unaligned column panel
    torch.testing.assert_close(got.cpu().double(), xx.double() @ w[:, 2:258].double().t(), rtol=1e-5, atol=1e-3)


# ----------------------------------------------------------------------------- K5 / K6 epilogues
@pytest.mark.parametrize("d,n", [(1, 257), (2, 257), (3, 257), (5, 257), (8, 257), (30, 257), (32, 257), (64, 257), (100, 257), (128, 257), (132, 257), (256, 257),
                                 (300, 257), (1024, 257),
                                 (8, 5001), (32, 5001), (64, 5001), (100, 5001), (128, 5001)])      # several rows per wave, both ways
@pytest.mark.parametrize("with_norm", [True, False])
def test_act_layernorm(ops, gpu_device, d, n, with_norm):
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(d)
    z = torch.randn(n, d, generator=gen)
    gamma, beta = torch.randn(d, generator=gen), torch.randn(d, generator=gen)
    wy, wn = torch.randn(n, d, generator=gen), torch.randn(n, d, generator=gen)

    def ref(z, gamma, beta):
        y = F.layer_norm(F.leaky_relu(z, 0.01), (d,), gamma, beta, 1e-5)
        return y, F.normalize(y, p=2.0, dim=1)
    zc, gc, bc = (t.clone().requires_grad_(True) for t in (z, gamma, beta))
    y, yn = ref(zc, gc, bc)
    ((y * wy).sum() + ((yn * wn).sum() if with_norm else 0)).backward()
    zg, gg, bg = (t.clone().to(gpu_device).requires_grad_(True) for t in (z, gamma, beta))
    y2, yn2 = ops.act_layernorm(zg, gg, bg, want_norm=with_norm)
    loss = (y2 * wy.to(gpu_device)).sum()
    if with_norm:
        loss = loss + (yn2 * wn.to(gpu_device)).sum()
        torch.testing.assert_close(yn2.cpu(), yn.detach(), rtol=1e-5, atol=1e-6)
    loss.backward()
    torch.testing.assert_close(y2.cpu(), y.detach(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(zg.grad.cpu(), zc.grad, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(gg.grad.cpu(), gc.grad, rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(bg.grad.cpu(), bc.grad, rtol=1e-4, atol=1e-3)


def test_gates_match_oracle(L, O, gpu_device):
    gen = torch.Generator().manual_seed(9)
    n, d = 333, 48
    x = torch.randn(n, d, generator=gen) * 0.3
    num, txt = torch.rand(n, 2, generator=gen), torch.randn(n, 300, generator=gen)
    for mod, lits, prefix in ((L.GateMul(d, 2, 300), (num, txt), "gm."), (L.Gate(d, 300), (txt,), "g1.")):
        with torch.no_grad():
            mod.gate_bias.normal_(0, 0.1)
        p = {prefix + k: v.detach().clone().requires_grad_(True) for k, v in mod.state_dict().items()}
        xc = x.clone().requires_grad_(True)
        want = O.gate_mul(p, prefix, xc, *lits) if len(lits) == 2 else O.gate_single(p, prefix, xc, *lits)
        w = torch.randn(n, d, generator=gen)
        (want * w).sum().backward()
        mod = mod.to(gpu_device)
        xg = x.clone().to(gpu_device).requires_grad_(True)
        got = mod(xg, *(l.to(gpu_device) for l in lits))
        (got * w.to(gpu_device)).sum().backward()
        torch.testing.assert_close(got.cpu(), want.detach(), rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(xg.grad.cpu(), xc.grad, rtol=1e-4, atol=1e-5)
        for k, v in mod.named_parameters():
            torch.testing.assert_close(v.grad.cpu(), p[prefix + k].grad, rtol=1e-4, atol=1e-4, msg=k)


# ----------------------------------------------------------------------------- K7/K8 scoring
@pytest.mark.parametrize("form", ["transe", "transr"])
@pytest.mark.parametrize("c,dout,b", [(32, 32, 17), (96, 64, 300), (200, 128, 1000)])
def test_triple_losses(ops, O, gpu_device, form, c, dout, b):
    from types import SimpleNamespace
    if form == "transe":
        dout = c
    gen = torch.Generator().manual_seed(c + b)
    n, n_rel = 400, 7
    gat = torch.randn(n, c, generator=gen) * 0.4
    p = {"relation_embed.weight": torch.randn(n_rel, dout, generator=gen) * 0.4,
         "gat_trans_M": torch.randn(n_rel, c, dout, generator=gen) * 0.2}
    ids = [torch.randint(0, n, (b,), generator=gen) for _ in range(3)]
    r = torch.randint(0, n_rel - 1, (b,), generator=gen)          # relation n_rel-1 never occurs: empty group
    cfg = SimpleNamespace(kg_l2loss_lambda=1e-3)
    gc = gat.clone().requires_grad_(True)
    pc = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    fn = O.triple_loss_transe if form == "transe" else O.triple_loss_transr
    sc = O.triple_scores_transe if form == "transe" else O.triple_scores_transr
    want = fn(pc, cfg, gc, ids[0], r, ids[1], ids[2])
    (want * 1.7).backward()
    pos_w, neg_w, _ = sc(p, gat, ids[0], r, ids[1], ids[2])
    gg = gat.clone().to(gpu_device).requires_grad_(True)
    pg = {k: v.clone().to(gpu_device).requires_grad_(True) for k, v in p.items()}
    dev_ids = [i.to(gpu_device) for i in ids]
    keep = {}
    if form == "transe":
        got = ops.transe_loss(gg, pg["relation_embed.weight"], dev_ids[0], r.to(gpu_device), dev_ids[1], dev_ids[2],
                              1e-3, keep)
    else:
        got = ops.transr_loss(gg, pg["relation_embed.weight"], pg["gat_trans_M"], dev_ids[0], r.to(gpu_device),
                              dev_ids[1], dev_ids[2], 1e-3, keep)
    (got * 1.7).backward()
    torch.testing.assert_close(keep["pos"].cpu(), pos_w, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(keep["neg"].cpu(), neg_w, rtol=1e-4, atol=1e-4)
    assert abs(float(got) - float(want)) <= 1e-5 * max(1.0, abs(float(want)))
    torch.testing.assert_close(gg.grad.cpu(), gc.grad, rtol=1e-3, atol=1e-6)
    torch.testing.assert_close(pg["relation_embed.weight"].grad.cpu(), pc["relation_embed.weight"].grad, rtol=1e-3,
                               atol=1e-6)
    if form == "transr":
        torch.testing.assert_close(pg["gat_trans_M"].grad.cpu(), pc["gat_trans_M"].grad, rtol=1e-3, atol=1e-6)


@pytest.mark.parametrize("c,dout,groups,k", [(40, 24, 37, 3), (96, 64, 50, 7), (300, 256, 9, 64), (64, 520, 5, 2)])
def test_transr_group_reuse_matches_oracle_and_general_path(ops, O, gpu_device, c, dout, groups, k):
    """a12 layout (dataloader.py:318-330): K consecutive rows share (h, r, t+); h and t+ are then projected once per
    group.  Same loss / scores / gradients as the oracle and as the general (ungrouped) evaluation of the same batch."""
    from types import SimpleNamespace
    from literalkg_amd.synth import make_batch
    gen = torch.Generator().manual_seed(k)
    n, n_rel = 500, 16
    gat = torch.randn(n, c, generator=gen) * 0.4
    p = {"relation_embed.weight": torch.randn(n_rel, dout, generator=gen) * 0.4,
         "gat_trans_M": torch.randn(n_rel, c, dout, generator=gen) * 0.2}
    bh, br, bp, bn = (torch.from_numpy(x) for x in make_batch(n, groups, k, seed=k))
    cfg = SimpleNamespace(kg_l2loss_lambda=1e-3)

    def oracle(dtype):
        gc = gat.clone().to(dtype).requires_grad_(True)
        pc = {kk: v.clone().to(dtype).requires_grad_(True) for kk, v in p.items()}
        want = O.triple_loss_transr(pc, cfg, gc, bh, br, bp, bn)
        want.backward()
        return want.detach(), gc.grad, pc["relation_embed.weight"].grad, pc["gat_trans_M"].grad
    w64 = oracle(torch.float64)                      # what both f32 evaluations approximate
    w32 = oracle(torch.float32)
    pos_w, neg_w, _ = O.triple_scores_transr(p, gat, bh, br, bp, bn)
    dev = [x.to(gpu_device) for x in (bh, br, bp, bn)]
    assert ops.is_grouped_batch(dev[0], dev[1], dev[2], k)
    assert not ops.is_grouped_batch(dev[0], dev[1], dev[2], k + 1)
    broken = dev[2].clone()
    broken[k - 1] = (broken[k - 1] + 1) % n
    assert not ops.is_grouped_batch(dev[0], dev[1], broken, k)

    def rel_err(got, ref):
        return float((got.double().cpu() - ref).abs().max()) / (float(ref.abs().max()) + 1e-30)
    for group in (k, 1):
        gg = gat.clone().to(gpu_device).requires_grad_(True)
        pg = {kk: v.clone().to(gpu_device).requires_grad_(True) for kk, v in p.items()}
        keep = {}
        got = ops.transr_loss(gg, pg["relation_embed.weight"], pg["gat_trans_M"], dev[0], dev[1], dev[2], dev[3],
                              1e-3, keep, group)
        got.backward()
        assert abs(float(got) - float(w64[0])) <= 1e-5 * max(1.0, abs(float(w64[0])))
        torch.testing.assert_close(keep["pos"].cpu(), pos_w, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(keep["neg"].cpu(), neg_w, rtol=1e-4, atol=1e-4)
        # every gradient as close to the f64 result as an f32 evaluation gets (the CPU f32 oracle's own distance is
        # the yardstick: sums of K products with cancellation, e.g. |S| << sum |terms| in the grouped head gradient)
        for got_g, i, name in ((gg.grad, 1, "emb"), (pg["relation_embed.weight"].grad, 2, "rel"),
                               (pg["gat_trans_M"].grad, 3, "W")):
            e_hip, e_cpu = rel_err(got_g, w64[i]), rel_err(w32[i], w64[i])
            assert e_hip <= max(8.0 * e_cpu, 2e-6), (group, name, e_hip, e_cpu)


def test_out_of_range_relation_raises_one_call_later(ops, gpu_device):
    """gat_trans_M[r] with r outside [0, n_relations) is an IndexError in the reference; here the kernel counts such
    keys and the error surfaces without a host sync in the step: at the next op, or at check_deferred_errors()."""
    gen = torch.Generator().manual_seed(0)
    emb = (torch.randn(50, 16, generator=gen)).to(gpu_device)
    rel = torch.randn(4, 8, generator=gen).to(gpu_device)
    wm = torch.randn(4, 16, 8, generator=gen).to(gpu_device)
    ids = [torch.randint(0, 50, (12,), generator=gen).to(gpu_device) for _ in range(3)]
    r = torch.tensor([0, 1, 2, 3, 4, 1, 2, 3, 0, 1, 2, -1], device=gpu_device)
    ops.transr_loss(emb, rel, wm, ids[0], r, ids[1], ids[2], 1e-3)
    with pytest.raises(IndexError, match="2 relation id"):
        ops.check_deferred_errors()
    ops.check_deferred_errors()          # reported once; the library stays usable
    ok = ops.transr_loss(emb, rel, wm, ids[0], r.clamp(0, 3), ids[1], ids[2], 1e-3)
    assert torch.isfinite(ok)


@pytest.mark.parametrize("scoring", ["transr", "transe"])
def test_out_of_range_entity_ids_never_reach_a_kernel(L, ops, O, gpu_device, scoring):
    """An entity id outside [0, n_entities) in a batch (h / pos_t / neg_t), in the fine-tuning triples or in the head /
    tail lists of calc_score is an IndexError in the reference (bounds-checked embedding lookup).  The HIP kernels would
    gather and atomically add out of bounds: the model replaces such ids by row 0 on the device before any kernel uses
    them (lkg_sanitize_ids_i64) and raises IndexError once the counter has been read -- forward AND backward run on safe
    ids, nothing faults, the module stays usable."""
    from literalkg_amd.synth import make_batch, make_kg
    from literalkg_amd import io
    n, dim = 3000, 16
    h, t, r = make_kg(n, 20_000, seed=3)
    cfg = O.default_cfg(embed_dim=dim, relation_dim=dim if scoring == "transr" else 2 * dim, conv_dim=dim,
                        n_conv_layers=1, device=gpu_device)
    torch.manual_seed(0)
    m = L.LiteralKG(cfg, n, 16, io.initial_a_in(n, h, t, r), scoring=scoring).to(gpu_device)
    bh, br, bp, bn = (torch.from_numpy(x).to(gpu_device) for x in make_batch(n, 20, 3, seed=1))
    ops.check_deferred_errors()
    bad_h, bad_n = bh.clone(), bn.clone()
    bad_h[3:6] = n + 10_000_000          # (a whole group: the layout check still sees groups)
    bad_n[7] = -5

    def surfaces(match, fn):
        """the error is raised by a later poll inside the same call (the check kernel is long done by then) or, at the
        latest, by check_deferred_errors() -- exactly once"""
        with pytest.raises(IndexError, match=match):
            fn()
            torch.cuda.synchronize()
            ops.check_deferred_errors()
        ops.check_deferred_errors()

    surfaces("4 entity id", lambda: m(bad_h, br, bp, bad_n, device=gpu_device, mode="pre_training").backward())
    if scoring == "transe":              # relation ids of the TransE form go straight into its score kernel
        bad_r = br.clone()
        bad_r[0:3] = 16
        surfaces("3 relation id", lambda: m(bh, bad_r, bp, bn, device=gpu_device, mode="pre_training").backward())
    surfaces("3 entity id", lambda: m(bad_h, bp, bn, device=gpu_device, mode="fine_tuning").backward())
    if scoring == "transr":
        m.eval()
        surfaces("2 entity id", lambda: m(torch.tensor([1, n, 5], device=gpu_device), torch.tensor([-1, 2], device=gpu_device),
                                          device=gpu_device, mode="predict"))
        m.train()
    # forward AND backward on the sanitised ids (the scatter of the row gradients included): nothing faults
    ops._Deferred.pending.clear()
    m.zero_grad(set_to_none=True)
    hs, ns = ops.checked_ids(n, bad_h, bad_n)
    assert int(hs.max()) < n and int(ns.min()) >= 0 and int((hs != bad_h).sum()) == 3 and int((ns != bad_n).sum()) == 1
    ops._Deferred.pending.clear()
    m.zero_grad(set_to_none=True)
    ok = m(bh, br, bp, bn, device=gpu_device, mode="pre_training")
    ok.backward()
    ops.check_deferred_errors()
    assert torch.isfinite(ok) and all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)


# ----------------------------------------------------------------------------- whole module vs golden
def _build_model(L, gd, device, scoring):
    cfg = golden_cfg(gd)
    n, n_rel = int(gd["n"]), int(gd["n_rel"])
    a_in = torch.sparse_coo_tensor(torch.from_numpy(gd["a_indices"]), torch.from_numpy(gd["a_values"]), (n, n)).coalesce()
    num = torch.from_numpy(gd["num"]) if "num" in gd else None
    txt = torch.from_numpy(gd["txt"]) if "txt" in gd else None
    m = L.LiteralKG(cfg, n, n_rel, a_in, num, txt, scoring=scoring)
    params = golden_params(gd)
    own = set(m.state_dict().keys())
    missing = m.load_state_dict({k: v for k, v in params.items() if k in own}, strict=False)
    assert missing.missing_keys == ["A_in"], missing
    return m.to(device).eval()


# Gradients of the reference-generated fixtures: within GRAD_TOL of the parameter's LARGEST gradient entry -- 1e-4, the north
# star's tolerance, for every parameter but the ones listed (measured on MI355X, LKG_GRAD_REPORT=1 prints every distance).
GRAD_TOL = 1e-4
GRAD_TOL_EXCEPTIONS = {}        # (fixture name or "*", parameter name substring) -> tolerance; filled from the measured run
GRAD_REPORT = bool(os.environ.get("LKG_GRAD_REPORT"))


def fixture_grad_close(got, want, name, key):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = float(np.abs(want).max()) + 1e-30
    err = float(np.abs(got - want).max()) / scale
    tol = GRAD_TOL
    for (fx, sub), t in GRAD_TOL_EXCEPTIONS.items():
        if (fx == "*" or fx == name) and sub in key:
            tol = max(tol, t)
    if GRAD_REPORT:
        print(f"GRAD {name} {key} {err:.3e} largest {scale:.3e}")
        return
    assert err <= tol, (name, key, err, tol)


@pytest.mark.parametrize("name", golden_names("encoder_") + golden_names("transe_"))
def test_module_matches_reference_fixture(L, gpu_device, name):
    gd = load_golden(name)
    form = str(gd["form"])
    m = _build_model(L, gd, gpu_device, form)
    batch = [torch.from_numpy(gd[k]).to(gpu_device) for k in ("bh", "br", "bp", "bn")]
    loss = m(*batch, device=gpu_device, mode="pre_training")
    np.testing.assert_allclose(m.gat_embed.detach().cpu().numpy(), gd["gat"], rtol=TOL, atol=TOL)
    np.testing.assert_allclose(m.last_scores["pos"].cpu().numpy(), gd["pos"], rtol=TOL, atol=TOL)
    np.testing.assert_allclose(m.last_scores["neg"].cpu().numpy(), gd["neg"], rtol=TOL, atol=TOL)
    np.testing.assert_allclose(float(loss), float(gd["loss"]), rtol=1e-5)
    loss.backward()
    grads = {k: v.grad for k, v in m.named_parameters() if v.grad is not None}
    n_checked = 0
    for k, want in gd.items():
        if k.startswith("g/"):
            assert k[2:] in grads, k
            fixture_grad_close(grads[k[2:]].cpu().numpy(), want, name, k[2:])
            n_checked += 1
    assert n_checked >= 4
    if form == "transr":
        hid, tid = torch.from_numpy(gd["score_heads"]).to(gpu_device), torch.from_numpy(gd["score_tails"]).to(gpu_device)
        with torch.no_grad():
            np.testing.assert_allclose(m.calc_score(hid, tid).cpu().numpy(), gd["score"], rtol=TOL, atol=TOL)
            assert np.array_equal(m(hid, tid, device=gpu_device, mode="predict").cpu().numpy(), gd["predict"])


def test_update_att_through_module(L, O, gpu_device):
    gd = load_golden("encoder_gcn_l1")
    m = _build_model(L, gd, gpu_device, "transr")
    h, t, r = (torch.from_numpy(gd[k]).to(gpu_device) for k in "htr")
    n_rel = int(gd["n_rel"])
    out = m(h, t, r, list(range(n_rel)), device=gpu_device, mode="update_att")
    assert out is None
    p = golden_params(gd)
    want = O.attention_refresh(int(gd["n"]), p["entity_embed.weight"], p["relation_embed.weight"],
                               *(torch.from_numpy(gd[k]) for k in "htr")).coalesce()
    a = m.A_in.data
    assert a.is_sparse and a.dtype == torch.float32 and a.indices().dtype == torch.int64
    assert torch.equal(a.indices().cpu(), want.indices())
    torch.testing.assert_close(a.values().cpu(), want.values(), rtol=1e-5, atol=1e-7)
    # training consumes the refreshed values; state_dict round-trips the sparse parameter
    batch = [torch.from_numpy(gd[k]).to(gpu_device) for k in ("bh", "br", "bp", "bn")]
    loss = m(*batch, device=gpu_device, mode="pre_training")
    want_loss = O.pre_training_loss(p, golden_cfg(gd), want, *(torch.from_numpy(gd[k]) for k in ("bh", "br", "bp", "bn")))
    np.testing.assert_allclose(float(loss), float(want_loss), rtol=1e-5)
    sd = m.state_dict()
    assert sd["A_in"].is_sparse and sd["A_in"]._nnz() == want._nnz()
    # only a subset of relations: the reference silently drops the other edges (model.py:451)
    m(h, t, r, [0, 2], device=gpu_device, mode="update_att")
    keep = (r == 0) | (r == 2)
    want2 = O.attention_refresh(int(gd["n"]), p["entity_embed.weight"], p["relation_embed.weight"],
                                h[keep].cpu(), t[keep].cpu(), r[keep].cpu(), [0, 2]).coalesce()
    assert torch.equal(m.A_in.data.indices().cpu(), want2.indices())
    torch.testing.assert_close(m.A_in.data.values().cpu(), want2.values(), rtol=1e-5, atol=1e-7)
    assert m(h, device=gpu_device, mode="no_such_mode") is None


def test_training_mode_dropout_statistics(L, gpu_device):
    gd = load_golden("encoder_gcn_l1")
    m = _build_model(L, gd, gpu_device, "transr")
    m.aggregator_layers[0].dropout = 0.5
    m.train()
    torch.manual_seed(0)
    e = m.gat_embeddings()
    layer_out = e[:, 16:]                                    # normalised copy of the dropped-out layer output
    frac = float((layer_out == 0).float().mean())
    assert 0.45 < frac < 0.55
    torch.testing.assert_close(layer_out.norm(dim=1), torch.ones(layer_out.shape[0], device=gpu_device),
                               rtol=1e-5, atol=1e-5)
    torch.manual_seed(0)
    e2 = m.gat_embeddings()
    assert torch.equal(e, e2)                                # mask follows torch.manual_seed
    e3 = m.gat_embeddings()
    assert not torch.equal(e2, e3)                           # and changes from call to call


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_fused_dropout_forward_backward(ops, gpu_device, p):
    """Dropout fused in the LN epilogue: the mask is a pure function of (seed, index), the kept fraction is
    1-p, kept values are LN/(1-p), and the backward equals autograd through the same explicit mask."""
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(1)
    n, d = 6000, 64                     # (narrow rows, several per wave, in both directions)
    z = torch.randn(n, d, generator=gen).to(gpu_device)
    gamma, beta = torch.randn(d, generator=gen).to(gpu_device), torch.randn(d, generator=gen).to(gpu_device)
    wy, wn = torch.randn(n, d, generator=gen).to(gpu_device), torch.randn(n, d, generator=gen).to(gpu_device)
    zg, gg, bg = (t.clone().requires_grad_(True) for t in (z, gamma, beta))
    y, yn = ops.act_layernorm(zg, gg, bg, want_norm=True, drop_p=p, seed=1234)
    ((y * wy).sum() + (yn * wn).sum()).backward()
    full, _ = ops.act_layernorm(z, gamma, beta, want_norm=False)
    mask = (y != 0).float()
    assert abs(float(mask.mean()) - (1 - p)) < 0.01
    torch.testing.assert_close(y, full * mask / (1 - p), rtol=1e-5, atol=1e-6)
    y_again, _ = ops.act_layernorm(z, gamma, beta, want_norm=False, drop_p=p, seed=1234)
    assert torch.equal(y.detach(), y_again)
    # reference gradient: torch autograd through LN * explicit mask
    zc, gc, bc = (t.clone().requires_grad_(True) for t in (z, gamma, beta))
    yr = F.layer_norm(F.leaky_relu(zc, 0.01), (d,), gc, bc, 1e-5) * mask / (1 - p)
    ((yr * wy).sum() + (F.normalize(yr, p=2.0, dim=1) * wn).sum()).backward()
    torch.testing.assert_close(zg.grad, zc.grad, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(gg.grad, gc.grad, rtol=1e-3, atol=1e-2)
    torch.testing.assert_close(bg.grad, bc.grad, rtol=1e-3, atol=1e-2)


@pytest.mark.parametrize("name", golden_names("encoder_"))
def test_fine_tuning_head_matches_reference_fixture(L, gpu_device, name):
    gd = load_golden(name)
    m = _build_model(L, gd, gpu_device, "transr")
    bh, bp, bn = (torch.from_numpy(gd[k]).to(gpu_device) for k in ("bh", "bp", "bn"))
    loss = m(bh, bp, bn, device=gpu_device, mode="fine_tuning")
    np.testing.assert_allclose(float(loss), float(gd["ft_loss"]), rtol=1e-5)
    loss.backward()
    np.testing.assert_allclose(m.entity_embed.weight.grad.cpu().numpy(), gd["ft_g/entity_embed.weight"], rtol=2e-3,
                               atol=2e-6)


@pytest.mark.parametrize("name", golden_names("trajectory_"))
def test_training_trajectory_matches_reference(L, gpu_device, name):
    """The drop-in module driven like pre_training_train (main_pretraining.py:86-139): Adam steps on the device,
    update_att in the middle, against the losses / final weights / final A_in the REFERENCE produced."""
    gd = load_golden(name)
    m = _build_model(L, gd, gpu_device, "transr")
    m.train()                                            # mess_dropout = 0 in this fixture
    opt = torch.optim.Adam(m.parameters(), lr=float(gd["lr"]))
    h, t, r = (torch.from_numpy(gd[k]).to(gpu_device) for k in "htr")
    for step, b in enumerate(gd["batches"]):
        opt.zero_grad()
        loss = m(*[torch.from_numpy(x).to(gpu_device) for x in b], device=gpu_device, mode="pre_training")
        assert not np.isnan(loss.cpu().detach().numpy())          # the caller's NaN check, main_pretraining.py:112
        loss.backward()
        opt.step()
        np.testing.assert_allclose(loss.item(), gd["losses"][step], rtol=1e-4, err_msg=f"step {step}")
        if step == int(gd["refresh_after"]):
            m(h, t, r, list(range(int(gd["n_rel"]))), device=gpu_device, mode="update_att")
    a = m.A_in.data.cpu().coalesce()
    assert np.array_equal(a.indices().numpy(), gd["final_a_indices"])
    np.testing.assert_allclose(a.values().numpy(), gd["final_a_values"], rtol=1e-3, atol=1e-6)
    sd = m.state_dict()
    for k, want in gd.items():
        if k.startswith("f/") and k[2:] in sd:
            np.testing.assert_allclose(sd[k[2:]].cpu().numpy(), want, rtol=2e-3, atol=2e-5, err_msg=k)


# ----------------------------------------------------------------------------- f4 fused Adam
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_fused_adam_matches_torch(L, gpu_device, wd):
    from literalkg_amd.optim import Adam
    gen = torch.Generator().manual_seed(0)
    shapes = [(1000, 64), (257,), (3, 5, 7)]
    ref = [torch.randn(s, generator=gen).requires_grad_(True) for s in shapes]
    mine = [p.detach().clone().to(gpu_device).requires_grad_(True) for p in ref]
    o_ref = torch.optim.Adam(ref, lr=3e-3, betas=(0.8, 0.95), eps=1e-7, weight_decay=wd)
    o_mine = Adam(mine, lr=3e-3, betas=(0.8, 0.95), eps=1e-7, weight_decay=wd)
    for step in range(7):
        for p, q in zip(ref, mine):
            g = torch.randn(p.shape, generator=gen) * (10.0 ** (step - 3))
            p.grad, q.grad = g.clone(), g.clone().to(gpu_device)
        o_ref.step()
        o_mine.step()
        for p, q in zip(ref, mine):
            torch.testing.assert_close(q.detach().cpu(), p.detach(), rtol=2e-6, atol=2e-7)
    sd_ref, sd_mine = o_ref.state_dict(), o_mine.state_dict()
    assert sd_ref["state"][0].keys() == sd_mine["state"][0].keys()            # interchangeable optimizer state
    torch.testing.assert_close(sd_mine["state"][0]["exp_avg_sq"].cpu(), sd_ref["state"][0]["exp_avg_sq"], rtol=1e-5,
                               atol=1e-9)
    o_back = Adam(mine, lr=3e-3, betas=(0.8, 0.95), eps=1e-7, weight_decay=wd)
    o_back.load_state_dict(sd_ref)                                            # torch's Adam state loads into ours


# ----------------------------------------------------------------------------- f2 device-side sampler
def test_kg_batch_sampler_contract(L, gpu_device):
    from literalkg_amd.sampler import KGBatchSampler
    rng = np.random.default_rng(3)
    n, n_rel = 600, 5
    h, t, r = rand_graph(rng, n, 7000, n_rel=n_rel, long_rows=[(11, 300)])
    extra = np.stack([h[:60], (r[:60] + 1) % n_rel, t[:60]], 1)                       # duplicate (h,t) pairs
    trip = np.unique(np.concatenate([np.stack([h, r, t], 1), extra]), axis=0)
    h, r, t = trip[:, 0].copy(), trip[:, 1].copy(), trip[:, 2].copy()
    g = L.KGStructure.from_triples(n, h, t, r, device=gpu_device)
    assert g.has_dups
    positives = set(map(tuple, trip.tolist()))
    k = 7
    s = KGBatchSampler(g, k)
    bh, br, bp, bn = (x.cpu().numpy() for x in s.sample(k * 150, seed=42))
    assert bh.shape == br.shape == bp.shape == bn.shape == (150 * k,)
    gh, gr, gp = bh.reshape(-1, k), br.reshape(-1, k), bp.reshape(-1, k)
    assert (gh == gh[:, :1]).all() and (gr == gr[:, :1]).all() and (gp == gp[:, :1]).all()   # repeated K times
    assert len(set(gh[:, 0].tolist())) == 150                                             # heads without replacement
    for hh, rr, pp, negs in zip(gh[:, 0], gr[:, 0], gp[:, 0], bn.reshape(-1, k)):
        assert (hh, rr, pp) in positives
        assert len(set(negs.tolist())) == k                                               # distinct inside the group
        assert all((hh, rr, x) not in positives for x in negs)                            # filtered against positives
    # the batch is a pure function of (torch RNG state for the head draw, seed for the kernel)
    torch.manual_seed(5)
    a1 = s.sample(k * 40, seed=7)
    torch.manual_seed(5)
    a2 = s.sample(k * 40, seed=7)
    assert all(torch.equal(x, y) for x, y in zip(a1, a2))
    torch.manual_seed(5)
    a3 = s.sample(k * 40, seed=8)
    assert torch.equal(a1[0], a3[0]) and not torch.equal(a1[3], a3[3])
    # negatives follow training_tails (in-degree weighted): frequent tails are drawn more often
    big = s.sample(k * 400, seed=1)[3].cpu().numpy()
    indeg = np.bincount(t, minlength=n).astype(float)
    drawn = np.bincount(big, minlength=n).astype(float)
    assert np.corrcoef(indeg, drawn)[0, 1] > 0.5
    # more groups than heads: sampling with replacement still fills the batch
    few = s.sample(k * 50, heads=torch.tensor([11, 12], device=gpu_device), seed=3)
    assert few[0].numel() == 50 * k and set(few[0].tolist()) <= {11, 12}
    # caller-supplied heads without a triple / outside the id range: KeyError like kg_dict[h] (dataloader.py:291)
    empty_head = int(np.flatnonzero(np.bincount(h, minlength=n) == 0)[0])
    for bad in ([11, empty_head], [11, n], [-1]):
        with pytest.raises(KeyError):
            s.sample(k * 2, heads=torch.tensor(bad, device=gpu_device), seed=3)


def test_kg_batch_sampler_distribution_matches_the_oracle(L, gpu_device):
    """f2: the device sampler against oracle/sampler_oracle.py (the restatement of dataloader.py:249-330 that is pinned
    bit for bit on a batch of the reference): ~1e6 draws from each, chi-square two-sample tests per head class on
    (a) which positive triple a head gets (uniform over its triples), (b) which tails come out as negatives (tail
    multiplicity in the triple list, minus the head's (tail, relation) positives, distinct inside a group)."""
    import random
    from literalkg_amd.sampler import KGBatchSampler
    from oracle import sampler_oracle as S
    rng = np.random.default_rng(12)
    n, n_rel, k = 400, 4, 5
    h, t, r = rand_graph(rng, n, 6000, n_rel=n_rel, long_rows=[(7, 250)])
    t = np.minimum((n * rng.random(len(t)) ** 2).astype(np.int64), n - 1)            # skewed tail multiplicity
    extra = np.stack([h[:80], (r[:80] + 1) % n_rel, t[:80]], 1)                       # (h,t) under two relations
    trip = np.unique(np.concatenate([np.stack([h, r, t], 1), extra]), axis=0)
    h, r, t = trip[:, 0].copy(), trip[:, 1].copy(), trip[:, 2].copy()
    g = L.KGStructure.from_triples(n, h, t, r, device=gpu_device)
    kg = S.build_kg_dict(h, t, r)
    deg = np.bincount(h, minlength=n)
    classes = {"low (1-4 triples)": np.flatnonzero((deg >= 1) & (deg <= 4))[:12],
               "mid (10-30 triples)": np.flatnonzero((deg >= 10) & (deg <= 30))[:12],
               "long row": np.array([7])}
    sampler = KGBatchSampler(g, k)
    triple_id = {tr: i for i, tr in enumerate(map(tuple, trip.tolist()))}

    def chi2_two_sample(a, b):
        keep = (a + b) > 0
        a, b = a[keep].astype(float), b[keep].astype(float)
        ka, kb = np.sqrt(b.sum() / a.sum()), np.sqrt(a.sum() / b.sum())
        return float((((ka * a - kb * b) ** 2) / (a + b)).sum()), int(keep.sum()) - 1

    for name, heads in classes.items():
        groups = 70_000 if len(heads) > 1 else 40_000
        random.seed(5)
        np.random.seed(5)
        pool = {int(x): kg[int(x)] for x in heads}
        # the oracle draws heads with random.choice when there are more groups than heads: same head law as the device
        oh, orr, op, on = S.generate_kg_batch(pool, groups * k, k, t.tolist())
        dh, dr, dp, dn = (x.cpu().numpy() for x in
                          sampler.sample(groups * k, heads=torch.from_numpy(heads).to(gpu_device), seed=77))
        assert dh.shape == oh.shape
        # (a) positive triples: counts per (h, r, t+) over the class
        cnt = lambda hh, rr, pp: np.bincount([triple_id[x] for x in zip(hh[::k].tolist(), rr[::k].tolist(),
                                                                    pp[::k].tolist())], minlength=len(trip))
        stat, df = chi2_two_sample(cnt(dh, dr, dp), cnt(oh, orr, op))
        assert stat < df + 5 * np.sqrt(2 * df) + 10, (name, "positives", stat, df)
        # uniform over the head's triples, head by head (device alone, exact expectation)
        dc = cnt(dh, dr, dp)
        for hh in heads[:4]:
            ids = [triple_id[(int(hh), rr, tt)] for tt, rr in kg[int(hh)]]
            obs = dc[ids].astype(float)
            exp = obs.sum() / len(ids)
            s = float(((obs - exp) ** 2 / exp).sum())
            assert s < (len(ids) - 1) + 5 * np.sqrt(2 * max(len(ids) - 1, 1)) + 10, (name, "uniform positives", s)
        # (b) negative tails
        stat, df = chi2_two_sample(np.bincount(dn, minlength=n), np.bincount(on, minlength=n))
        assert stat < df + 5 * np.sqrt(2 * df) + 10, (name, "negatives", stat, df)


def test_attention_row_range_refresh_leaves_other_rows_alone(L, ops, gpu_device):
    """A row-range refresh into an existing value array (out=) on a graph WITH duplicate (h,t) pairs: the entries of
    the other rows keep their values (only this call's entry range is cleared for the duplicate pre-pass)."""
    rng = np.random.default_rng(8)
    n, d = 300, 64
    h, t, r = rand_graph(rng, n, 4000, n_rel=6, long_rows=[(5, 400)])
    extra = np.stack([h[:80], (r[:80] + 1) % 6, t[:80]], 1)
    trip = np.unique(np.concatenate([np.stack([h, r, t], 1), extra]), axis=0)
    g = L.KGStructure.from_triples(n, trip[:, 0].copy(), trip[:, 2].copy(), trip[:, 1].copy(), device=gpu_device)
    assert g.has_dups
    ent = torch.randn(n, d, device=gpu_device) * 0.3
    rel = torch.randn(6, d, device=gpu_device) * 0.3
    full, _ = ops.edge_softmax(g, ent, rel)
    out = torch.full((g.nnz,), -7.0, device=gpu_device)
    lo, hi = 100, 220
    ops.edge_softmax(g, ent, rel, row_lo=lo, row_hi=hi, out=out)
    rp = g.host("rowptr")
    a, b = int(rp[lo]), int(rp[hi])
    torch.testing.assert_close(out[a:b], full[a:b], rtol=1e-6, atol=1e-8)
    assert float((out[:a] + 7.0).abs().max()) == 0.0 and float((out[b:] + 7.0).abs().max()) == 0.0


# ----------------------------------------------------------------------------- device-side structure build
@pytest.mark.parametrize("n,e,n_rel,dup", [(1, 1, 1, 0), (7, 40, 3, 10), (300, 5000, 6, 200), (5000, 2049, 4, 0),
                                            (70000, 300000, 16, 3000), (2_000_000, 150_000, 5, 50)])
def test_device_csr_build_is_bit_exact_with_the_host_build(L, gpu_device, n, e, n_rel, dup):
    """lkg_csr_build_device / lkg_csr_transpose_device (radix sort + scans on the GPU) against lkg_csr_build /
    lkg_csr_transpose (host): every array identical -- sorted order, merged duplicate pairs, tie order of the raw
    edges (input order), CSC with ascending heads -- for device AND host inputs."""
    rng = np.random.default_rng(n + e)
    h = rng.integers(0, n, e)
    t = rng.integers(0, n, e)
    r = rng.integers(0, n_rel, e)
    if n > 10:
        h[: e // 5] = rng.integers(0, 3, e // 5)                  # a few very long rows (> 256 entries)
    if dup:
        src = rng.integers(0, e, dup)
        h = np.concatenate([h, h[src], h[src[: dup // 2]]])       # repeated (h, t) pairs, some three times
        t = np.concatenate([t, t[src], t[src[: dup // 2]]])
        r = np.concatenate([r, (r[src] + 1) % n_rel, r[src[: dup // 2]]])
    gh = L.KGStructure.from_triples(n, h, t, r, device="cpu")
    for inputs in ((h, t, r), tuple(torch.from_numpy(x).to(gpu_device) for x in (h, t, r))):
        gd = L.KGStructure.from_triples(n, *inputs, device=gpu_device)
        assert (gd.n, gd.nnz, gd.n_raw) == (gh.n, gh.nnz, gh.n_raw)
        for name in ("rowptr", "col", "eptr", "rel", "rel_first", "dup_entries", "dup_rows", "t_rowptr", "t_col",
                     "t_perm"):
            a, b = gd.host(name), gh.host(name)
            assert (a is None) == (b is None), name
            if a is not None:
                assert a.dtype == b.dtype and np.array_equal(a, b), name
        assert np.array_equal(gd.order, gh.order)
    none = L.KGStructure.from_triples(5, np.zeros(0, np.int64), np.zeros(0, np.int64), None, device=gpu_device)
    assert none.nnz == 0 and none.host("rowptr").tolist() == [0] * 6 and none.host("t_rowptr").tolist() == [0] * 6
    bad_t = t.copy()
    bad_t[0] = n
    from literalkg_amd._native import LkgError
    with pytest.raises(LkgError, match="outside"):
        L.KGStructure.from_triples(n, h, bad_t, r, device=gpu_device)


def test_device_csr_build_at_full_size_is_fast(L, gpu_device):
    """1 M entities / 10 M triples: same arrays as the host build, and the build (what the first update_att of an
    edge list pays) takes milliseconds, not a host sort."""
    import time
    from literalkg_amd.synth import make_kg
    n = 1_000_000
    h, t, r = make_kg(n, 10_000_000)
    gh = L.KGStructure.from_triples(n, h, t, r, device="cpu")
    dev = tuple(torch.from_numpy(x).to(gpu_device) for x in (h, t, r))
    L.KGStructure.from_triples(n, *dev, device=gpu_device)           # warm-up (allocator)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    gd = L.KGStructure.from_triples(n, *dev, device=gpu_device)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    for name in ("rowptr", "col", "eptr", "rel", "t_rowptr", "t_col", "t_perm"):
        assert np.array_equal(gd.host(name), gh.host(name)), name
    assert ms < 50.0, f"device structure build took {ms:.1f} ms"
    print(f"device CSR+CSC build, 10 M triples: {ms:.2f} ms")


# ----------------------------------------------------------------------------- full-size properties
def test_full_size_properties(L, ops, gpu_device):
    """BASELINE config shape (1M entities / 10M edges / D=256): size-independent properties."""
    from literalkg_amd.synth import make_kg, xavier_table
    n, e, d = 1_000_000, 10_000_000, 256
    h, t, r = make_kg(n, e)
    g = L.KGStructure.from_triples(n, h, t, r, device=gpu_device)
    assert g.nnz < e and g.has_dups                                     # forced duplicate pairs were merged
    rp, col = g.rowptr.cpu().numpy(), g.col.cpu().numpy()
    assert rp[0] == 0 and rp[-1] == g.nnz and np.all(np.diff(rp) >= 0)
    rows = np.repeat(np.arange(n), np.diff(rp))
    key = rows.astype(np.int64) * n + col
    assert np.all(np.diff(key) > 0)                                     # sorted by (h,t), no duplicate pair
    assert np.array_equal(np.unique(h * n + t), key)                    # exactly the distinct input pairs
    ent = xavier_table(n, d, gpu_device)
    rel = xavier_table(16, d, gpu_device, seed=7)
    val, _ = ops.edge_softmax(g, ent, rel)
    ones = torch.ones(n, 8, device=gpu_device)
    rs = ops.spmm_raw(g.rowptr, g.col, val, ones, n)[:, 0]
    nonempty = torch.from_numpy(np.diff(rp) > 0).to(gpu_device)
    assert float((rs[nonempty] - 1).abs().max()) < 1e-5                 # softmax rows sum to one
    assert float(rs[~nonempty].abs().max()) == 0.0
    x1, x2 = torch.randn(n, d, device=gpu_device), torch.randn(n, d, device=gpu_device)
    a = ops.spmm_raw(g.rowptr, g.col, val, x1, n)
    b = ops.spmm_raw(g.rowptr, g.col, val, x2, n)
    ab = ops.spmm_raw(g.rowptr, g.col, val, x1 + 2 * x2, n)
    assert float((ab - (a + 2 * b)).abs().max()) < 1e-4                 # linearity
    # <A x, y> == <x, A^T y>  (forward kernel against the transpose kernel)
    y = torch.randn(n, d, device=gpu_device)
    aty = ops.spmm_raw(g.t_rowptr, g.t_col, ops.permute_values(val, g.t_perm), y, n)
    lhs, rhs = float((a.double() * y.double()).sum()), float((x1.double() * aty.double()).sum())
    assert abs(lhs - rhs) <= 1e-6 * max(abs(lhs), abs(rhs), 1.0) + 1e-2
    # spot-check 200 rows against a direct evaluation
    pick = np.random.default_rng(0).choice(np.flatnonzero(np.diff(rp) > 0), 200, replace=False)
    for i in pick[:200]:
        sl = slice(rp[i], rp[i + 1])
        want = (val[sl][:, None] * x1[torch.from_numpy(col[sl]).long().to(gpu_device)]).sum(0)
        assert float((a[i] - want).abs().max()) < 1e-4


# ----------------------------------------------------------------------------- C-ABI error convention on the device side
def test_device_entry_points_reject_bad_arguments(L, ops, gpu_device):
    from literalkg_amd import _native as N
    x = torch.zeros(4, 8, device=gpu_device)
    rp = torch.zeros(5, dtype=torch.int32, device=gpu_device)
    with pytest.raises(N.LkgError, match="row strides"):
        N.call("lkg_spmm_csr_f32", 4, 8, N.ptr(rp), None, None, N.ptr(x), 4, N.ptr(x), 8, None, 0, None, 0, 0, None)
    with pytest.raises(N.LkgError, match="long-row list"):
        N.call("lkg_spmm_csr_f32", 4, 8, N.ptr(rp), None, None, N.ptr(x), 8, N.ptr(x), 8, None, 0, None, 3, 0, None)
    with pytest.raises(N.LkgError, match="empty batch"):
        N.call("lkg_loss_reduce_f32", 0, N.ptr(x), N.ptr(x), 0.0, N.ptr(x), None)
    with pytest.raises(N.LkgError, match="dropout probability"):
        ops.act_layernorm(x, torch.ones(8, device=gpu_device), torch.zeros(8, device=gpu_device), drop_p=1.5, seed=1)
    with pytest.raises(N.LkgError, match="mode must be"):
        N.call("lkg_grouped_gemm_f32", 3, 1, N.ptr(rp), 4, 0, 0, 4, 8, 8, 1.0, N.ptr(x), 8, N.ptr(x), 8, 0, 0, 0.0,
               N.ptr(x), 8, 0, None)
    with pytest.raises(ValueError, match="inner dimensions"):
        ops.gemm(x, x)
    with pytest.raises(ValueError, match="embed_dim must equal relation_dim"):
        g = L.KGStructure.from_triples(4, np.array([0]), np.array([1]), np.array([0]), device=gpu_device)
        ops.edge_softmax(g, x, torch.zeros(2, 4, device=gpu_device))
    with pytest.raises(TypeError, match="float32"):
        ops.gemm(x.double(), x.double().t())
    # a failed call leaves the library usable
    y = ops.gemm(x, x, trans_b=True)
    assert y.shape == (4, 4)


# ----------------------------------------------------------------------------- mid-size module vs the oracle (vector paths)
@pytest.mark.parametrize("agg,layers,dim,gate,scale,scoring", [
    ("gcn", 2, 128, "mul", 64, "transr"),
    ("graphsage", 1, 64, "txt", None, "transr"),
    ("bi-interaction", 2, 64, None, None, "transr"),
    ("gin", 2, 64, "num", None, "transr"),
    ("gcn", 1, 256, None, 256, "transe"),
    ("gcn", 2, 30, "mul", 18, "transr"),            # widths that are not multiples of 4: every scalar code path
    ("bi-interaction", 1, 50, "num", None, "transe"),
])
def test_module_matches_oracle_at_realistic_widths(L, O, gpu_device, agg, layers, dim, gate, scale, scoring):
    _module_against_oracle(L, O, gpu_device, agg, layers, dim, dim, gate, scale, scoring)


def test_fused_layer_launch_is_chosen_for_evaluation_of_wide_layers_only(ops, gpu_device, monkeypatch):
    """ops.FUSED_LAYER = "auto" (the default): the one-launch layer where it is the faster way -- no gradient to come and rows
    of 129-256 columns; the GEMM + row-wise pair everywhere else (training needs z, which the fused launch does not write)."""
    monkeypatch.setattr(ops, "FUSED_LAYER", "auto")
    m = ops.TALL_MIN_ROWS
    x = torch.randn(m, 256, device=gpu_device)
    w = torch.nn.Parameter(torch.randn(256, 256, device=gpu_device))
    w_narrow = torch.nn.Parameter(torch.randn(64, 256, device=gpu_device))
    assert not ops.fused_layer_wanted((x,), (w,))
    with torch.no_grad():
        assert ops.fused_layer_wanted((x,), (w,))
        assert not ops.fused_layer_wanted((x,), (w_narrow,))
        assert not ops.fused_layer_wanted((x[:m // 2],), (w,))
    assert ops.fused_layer_wanted((x,), (w.detach(),))
    assert not ops.fused_layer_wanted((x,), (w.detach(),), (torch.nn.Parameter(torch.zeros(256, device=gpu_device)),))
    monkeypatch.setattr(ops, "FUSED_LAYER", False)
    with torch.no_grad():
        assert not ops.fused_layer_wanted((x,), (w,))


@pytest.mark.parametrize("n_rel,c,dout,k", [(1, 64, 8, 3), (4, 64, 8, 3), (1, 64, 8, 1), (16, 300, 300, 3)])
def test_transr_matrix_gradient_keeps_the_reference_order_conditioning(ops, gpu_device, n_rel, c, dout, k):
    """gat_trans_M's gradient sums x_h^T g_h + x_+^T g_+ + x_-^T g_- over the batch, and g_h = -(g_+ + sum g_-) up to the
    regulariser: when the table's rows share a large common part the three blocks nearly cancel.  The reference adds them per
    sample first (autograd over model.py:391-397), so its fp32 result stays accurate; block after block it was 60 x worse than
    that (fuzz seed 44053: one relation, 683 groups).  The common part is taken out before the products: as accurate as the
    reference's order (fp32 autograd on the CPU) against float64."""
    torch.manual_seed(c + n_rel)
    n, n_g = 9000, 683
    emb = (torch.randn(n, c) * 0.01 + torch.randn(1, c)).to(gpu_device).requires_grad_(True)       # rows = common part + 1 %
    rel = (torch.randn(n_rel, dout) * 0.1).to(gpu_device).requires_grad_(True)
    M = (torch.randn(n_rel, c, dout) * 0.1).to(gpu_device).requires_grad_(True)
    hg, rg, pg = torch.randint(0, n, (n_g,)), torch.randint(0, n_rel, (n_g,)), torch.randint(0, n, (n_g,))
    h, r, pt = (t.repeat_interleave(k) for t in (hg, rg, pg))
    nt = torch.randint(0, n, (n_g * k,))
    ops.transr_loss(emb, rel, M, h.to(gpu_device), r.to(gpu_device), pt.to(gpu_device), nt.to(gpu_device), 1e-5, None, k, False).backward()

    def grads(dtype):
        e, rr, mm = (t.detach().to(dtype).cpu().requires_grad_(True) for t in (emb, rel, M))
        w = mm[r]
        a, b_, c_ = (torch.bmm(e[i].unsqueeze(1), w).squeeze(1) for i in (h, pt, nt))
        d = rr[r]
        l2 = lambda x: (x ** 2).sum(1).mean() / 2
        loss = (-torch.nn.functional.logsigmoid(((a + d - c_) ** 2).sum(1) - ((a + d - b_) ** 2).sum(1))).mean() \
            + 1e-5 * (l2(a) + l2(d) + l2(b_) + l2(c_))
        loss.backward()
        return mm.grad, e.grad, rr.grad
    want, ref32 = grads(torch.float64), grads(torch.float32)
    for name, got, w64, r32 in zip(("gat_trans_M", "table", "relation_embed"), (M.grad, emb.grad, rel.grad), want, ref32):
        scale = float(w64.abs().max())
        mine = float((got.double().cpu() - w64).abs().max()) / scale
        theirs = float((r32.double() - w64).abs().max()) / scale
        assert mine <= max(4 * theirs, 2e-6), (name, mine, theirs)


@pytest.mark.parametrize("agg,layers,group", [("gcn", 3, True), ("bi-interaction", 2, False)])
def test_projection_on_the_batch_rows_equals_the_projection_of_the_whole_table(L, O, gpu_device, agg, layers, group):
    """calc_triplet_loss applies linear_gat + its activation (model.py:309-310) to the <= 3B rows the TransR loss reads instead
    of all N (project_batch_rows_only): the same loss, the same gradients and -- read afterwards -- the same self.gat_embed as
    with the whole table projected first, which is what the reference does (model.py:380)."""
    from literalkg_amd.synth import make_batch, make_kg
    from literalkg_amd import io
    n, e = 20_000, 150_000
    h, t, r = make_kg(n, e, seed=5)
    cfg = O.default_cfg(embed_dim=48, relation_dim=40, conv_dim=32, n_conv_layers=layers, aggregation_type=agg, scale_gat_dim=56,
                        use_num_lit=True, use_txt_lit=False, device=gpu_device)
    torch.manual_seed(3)
    num = torch.rand(n, 2)
    a_in = io.initial_a_in(n, h, t, r)
    batch = [torch.from_numpy(x).to(gpu_device) for x in make_batch(n, 200, 3, seed=9)]
    if not group:          # no (h, r, t+) groups: every triple on its own
        perm = torch.randperm(batch[0].numel(), generator=torch.Generator().manual_seed(1)).to(gpu_device)
        batch = [b[perm] for b in batch]
    got = {}
    for rows_only in (True, False):
        torch.manual_seed(11)
        m = L.LiteralKG(cfg, n, 16, a_in, num, None).to(gpu_device).eval()
        m.project_batch_rows_only = rows_only
        loss = m(*batch, device=gpu_device, mode="pre_training")
        loss.backward()
        got[rows_only] = (float(loss), {k: v.grad.detach().clone() for k, v in m.named_parameters() if v.grad is not None},
                          m.gat_embed.detach().clone())
        assert tuple(got[rows_only][2].shape) == (n, 56)
    assert abs(got[True][0] - got[False][0]) <= 2e-6 * abs(got[False][0])
    torch.testing.assert_close(got[True][2], got[False][2], rtol=1e-5, atol=1e-6)
    assert got[True][1].keys() == got[False][1].keys()
    for k, g in got[False][1].items():
        err = float((got[True][1][k] - g).abs().max()) / (float(g.abs().max()) + 1e-30)
        assert err < 2e-5, (k, err)


@pytest.mark.parametrize("agg,layers,dim,gate", [("gcn", 2, 128, "mul"), ("graphsage", 2, 64, None), ("gcn", 1, 256, None)])
def test_module_with_the_fused_layer_launch_matches_oracle_and_the_unfused_pair(L, O, ops, gpu_device, agg, layers, dim, gate):
    """ops.FUSED_LAYER: an aggregation layer's Linear + LeakyReLU + LayerNorm (+ normalised copy) as ONE launch whose backward
    recomputes z (on the listed rows under the loss's row-sparse gradients): against the oracle like every module test, and
    against the same module on the unfused pair -- loss and the propagated table bit for bit, gradients to rounding."""
    from literalkg_amd.synth import make_batch, make_kg
    from literalkg_amd import io
    old = ops.FUSED_LAYER
    try:
        ops.FUSED_LAYER = True
        _module_against_oracle(L, O, gpu_device, agg, layers, dim, dim, gate, None, "transr")
        n, e = 20_000, 150_000
        h, t, r = make_kg(n, e, seed=5)
        cfg = O.default_cfg(embed_dim=dim, relation_dim=dim, conv_dim=dim, n_conv_layers=layers, aggregation_type=agg,
                            use_num_lit=gate == "mul", use_txt_lit=gate == "mul", txt_lit_dim=300, device=gpu_device)
        torch.manual_seed(3)
        num = torch.rand(n, 2) if cfg.use_num_lit else None
        txt = torch.randn(n, 300) if cfg.use_txt_lit else None
        a_in = io.initial_a_in(n, h, t, r)
        batch = [torch.from_numpy(x).to(gpu_device) for x in make_batch(n, 200, 3, seed=9)]
        got = {}
        for fused in (True, False):
            ops.FUSED_LAYER = fused
            torch.manual_seed(11)
            m = L.LiteralKG(cfg, n, 16, a_in, num, txt).to(gpu_device).eval()
            loss = m(*batch, device=gpu_device, mode="pre_training")
            loss.backward()
            got[fused] = (float(loss), m.gat_embed.detach().clone(), {k: v.grad.detach().clone() for k, v in m.named_parameters() if v.grad is not None})
    finally:
        ops.FUSED_LAYER = old
    if dim > 128:      # the unfused Linear runs on the same 256-column tiling: bit for bit (narrower ones: another tile's rounding)
        assert got[True][0] == got[False][0]
        assert torch.equal(got[True][1], got[False][1])
    assert abs(got[True][0] - got[False][0]) <= 1e-6 * abs(got[False][0])
    torch.testing.assert_close(got[True][1], got[False][1], rtol=1e-5, atol=1e-6)
    for k, g_f in got[True][2].items():
        g_u = got[False][2][k]
        assert float((g_f - g_u).abs().max()) <= 2e-5 * (float(g_u.abs().max()) + 1e-12), k


@pytest.mark.parametrize("shape", [(300, 300, 300), (32, 300, 300), (7, 5, 3), (256, 64, 256), (1, 1, 1)])
def test_small_product_with_float64_accumulation(ops, gpu_device, shape):
    """lkg_gemm_f64acc_f32 (the residual's weight fold): every layout against float64 on the host, rounded once"""
    m, n, k = shape
    gen = torch.Generator().manual_seed(m * 7 + n)
    a, b = torch.randn(m, k, generator=gen), torch.randn(k, n, generator=gen)
    want = (a.double() @ b.double()).float()
    for ta, tb in ((False, False), (True, False), (False, True), (True, True)):
        aa = (a.t().contiguous() if ta else a).to(gpu_device)
        bb = (b.t().contiguous() if tb else b).to(gpu_device)
        got = ops.gemm_f64acc(aa, bb, trans_a=ta, trans_b=tb).cpu()
        ulp = torch.finfo(torch.float32).eps * want.abs().clamp_min(1e-30)
        assert bool(((got - want).abs() <= ulp).all()), (ta, tb, float((got - want).abs().max()))
    x = a.to(gpu_device).requires_grad_(True)
    y = b.t().contiguous().to(gpu_device).requires_grad_(True)
    ops.fold_nt(x, y).square().sum().backward()
    xr, yr = a.double().requires_grad_(True), b.t().double().requires_grad_(True)
    (xr @ yr.t()).square().sum().backward()
    torch.testing.assert_close(x.grad.cpu().double(), xr.grad, rtol=1e-5, atol=1e-6 * float(xr.grad.abs().max()) + 1e-30)
    torch.testing.assert_close(y.grad.cpu().double(), yr.grad, rtol=1e-5, atol=1e-6 * float(yr.grad.abs().max()) + 1e-30)


@pytest.mark.parametrize("agg", ["gcn", "graphsage", "bi-interaction"])
def test_residual_layers_in_the_reference_association(L, O, gpu_device, agg):
    """args.reference_association: residual layers evaluated as the reference writes them (Linear(mixed @ W'), model.py:95-98)
    instead of through the folded weight.  Both forms against the oracle in float64 -- the propagated table within 1e-4 of the
    largest entry either way -- and the reference-association form at least as close to the fp32 oracle as the fold."""
    from literalkg_amd.synth import make_kg
    from literalkg_amd import io
    n, dim = 20_000, 64
    h, t, r = make_kg(n, 150_000, seed=5)
    a_in = io.initial_a_in(n, h, t, r)
    got = {}
    for ref_assoc in (False, True):
        cfg = O.default_cfg(embed_dim=dim, relation_dim=dim, conv_dim=dim, n_conv_layers=3, aggregation_type=agg,
                            use_residual=True, mlp_hidden_dim=48, device=gpu_device, reference_association=ref_assoc)
        torch.manual_seed(3)
        m = L.LiteralKG(cfg, n, 16, a_in, None, None)
        params = {k: v.detach().clone() for k, v in m.state_dict().items() if k != "A_in"}
        m.to(gpu_device).eval()
        with torch.no_grad():
            got[ref_assoc] = m.gat_embeddings().cpu()
    want32 = O.gat_embeddings(params, cfg, a_in, None, None)
    want64 = O.gat_embeddings({k: v.double() if v.is_floating_point() else v for k, v in params.items()}, cfg, a_in.double(), None, None)
    scale = float(want64.abs().max())
    e_fold = float((got[False].double() - want64).abs().max()) / scale
    e_ref = float((got[True].double() - want64).abs().max()) / scale
    e_o32 = float((want32.double() - want64).abs().max()) / scale
    print(f"{agg}: vs float64 -- fold {e_fold:.2e}, reference association {e_ref:.2e}, fp32 oracle {e_o32:.2e}")
    assert e_fold <= max(1e-4, 10 * e_o32) and e_ref <= max(1e-4, 10 * e_o32)
    d_ref = float((got[True] - want32).abs().max()) / scale
    assert d_ref <= max(1e-4, 10 * e_o32)


def test_module_matches_oracle_at_the_reference_default_architecture(L, O, gpu_device):
    """argument_pretraining.py's defaults (lines 34-62): embed_dim = relation_dim = scale_gat_dim = 300, EIGHT gcn layers of
    conv_dim 32 (concatenated width 300 + 8 * 32 = 556 -> linear_gat -> 300), GateMul over 2 numeric + 300 text literals,
    TransR with a 300 x 300 matrix per relation -- what a user of the reference runs when no flag is given."""
    _module_against_oracle(L, O, gpu_device, "gcn", 8, 300, 32, "mul", 300, "transr")


def test_module_matches_oracle_with_a_hundred_relations(L, O, gpu_device):
    """total_rel = 100 (argument_pretraining.py:31): a hundred W_r matrices / relation rows through the grouped projection
    and the attention refresh, on a narrowing two-layer model."""
    _module_against_oracle(L, O, gpu_device, "gcn", 2, 128, 32, "num", 64, "transr", n_rel=100)


@pytest.mark.parametrize("gate,scale", [(None, None), (None, 48), ("txt", None)])
def test_narrowing_gcn_layers_project_before_they_aggregate(L, O, gpu_device, gate, scale):
    """gcn layers whose Linear narrows (128 -> 32) run it BEFORE the aggregation ((ego + A ego) W^T + b = p + A p + b): without a
    gate the first layer's input is the raw entity table (kept as slot 0 of the concatenated table by a copy or, for the
    TransR loss, not at all), with one the gate's output."""
    _module_against_oracle(L, O, gpu_device, "gcn", 2, 128, 32, gate, scale, "transr")


def _module_against_oracle(L, O, gpu_device, agg, layers, dim, conv_dim, gate, scale, scoring, n_rel=16):
    from literalkg_amd.synth import make_batch, make_kg
    from literalkg_amd import io
    n, e = 20_000, 150_000
    h, t, r = make_kg(n, e, seed=5)
    if n_rel != 16:
        r = np.random.default_rng(17).integers(0, n_rel, len(r))
        _, first = np.unique(np.stack([h, r, t], 1), axis=0, return_index=True)
        h, t, r = h[first], t[first], r[first]
    cfg = O.default_cfg(embed_dim=dim, relation_dim=dim if scoring == "transr" else (scale or dim + conv_dim * layers),
                        conv_dim=conv_dim, n_conv_layers=layers, aggregation_type=agg, scale_gat_dim=scale,
                        use_num_lit=gate in ("mul", "num"), use_txt_lit=gate in ("mul", "txt"),
                        txt_lit_dim=300 if dim % 4 == 0 else 7,
                        mlp_hidden_dim=48, kg_l2loss_lambda=1e-4, device=gpu_device)
    torch.manual_seed(3)
    num = torch.rand(n, 2) if cfg.use_num_lit else None
    txt = torch.randn(n, cfg.txt_lit_dim) if cfg.use_txt_lit else None
    a_in = io.initial_a_in(n, h, t, r)
    m = L.LiteralKG(cfg, n, n_rel, a_in, num, txt, scoring=scoring)
    with torch.no_grad():                      # larger-than-xavier values so every term matters
        m.entity_embed.weight.mul_(30)
        m.relation_embed.weight.mul_(3)
    params = {k: v.detach().clone() for k, v in m.state_dict().items() if k != "A_in"}
    m.to(gpu_device).eval()
    batch = [torch.from_numpy(x) for x in make_batch(n, 200, 3, seed=9)]
    if n_rel != 16:
        batch[1] = torch.from_numpy(np.repeat(np.random.default_rng(23).integers(0, n_rel, 200), 3))
    loss = m(*[b.to(gpu_device) for b in batch], device=gpu_device, mode="pre_training")
    loss.backward()
    p = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in params.items()}
    want = O.pre_training_loss(p, cfg, a_in, *batch, num=num, txt=txt, form=scoring)
    want.backward()
    np.testing.assert_allclose(float(loss), float(want), rtol=1e-4)
    gat = O.gat_embeddings(params, cfg, a_in, num, txt)
    torch.testing.assert_close(m.gat_embed.detach().cpu(), gat, rtol=1e-4, atol=1e-4)
    for k, v in m.named_parameters():
        if v.grad is not None and k != "A_in":
            ref = p[k].grad
            scale_ = float(ref.abs().max()) + 1e-12
            err = float((v.grad.cpu() - ref).abs().max()) / scale_
            assert err < 2e-3, (k, err)
    # update_att on the device, then the refreshed values drive the next forward
    hd, td, rd = (torch.from_numpy(x).to(gpu_device) for x in (h, t, r))
    if cfg.relation_dim != cfg.embed_dim:       # the reference cannot add the two embeddings either (model.py:441)
        with pytest.raises(ValueError, match="embed_dim must equal relation_dim"):
            m(hd, td, rd, list(range(n_rel)), device=gpu_device, mode="update_att")
        return
    m(hd, td, rd, list(range(n_rel)), device=gpu_device, mode="update_att")
    ref_a = O.attention_refresh(n, params["entity_embed.weight"], params["relation_embed.weight"],
                                torch.from_numpy(h), torch.from_numpy(t), torch.from_numpy(r)).coalesce()
    got_a = m.A_in.data.cpu()
    assert torch.equal(got_a.indices(), ref_a.indices())
    torch.testing.assert_close(got_a.values(), ref_a.values(), rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("agg,conv_dim,gate", [("gcn", 32, "mul"), ("gcn", 128, "num"), ("graphsage", 128, "txt"),
                                               ("bi-interaction", 128, "num"), ("gin", 128, "num"), ("gcn", 32, None)])
def test_forward_without_backward_leaves_nothing_behind(L, O, gpu_device, agg, conv_dim, gate):
    """Forwards with grad enabled and NO backward (an evaluation loop that forgot no_grad, a timing loop): every call must
    free the graph of the previous one.  The concatenated table's slots are views of one buffer; with that buffer itself as
    the output of the concatenation node, a consumer that saved a slot for its backward (graphsage's / gin's Linear and
    bi-interaction's product over the gate's output, a narrowing gcn layer's Linear) closed a cycle of C++ references
    that only a backward pass would break -- 7 GiB per call at the reference's default architecture on 1 M entities."""
    import gc
    from literalkg_amd.synth import make_batch, make_kg
    from literalkg_amd import io
    n, dim = 30_000, 128
    h, t, r = make_kg(n, 200_000, seed=2)
    cfg = O.default_cfg(embed_dim=dim, relation_dim=dim, conv_dim=conv_dim, n_conv_layers=2, aggregation_type=agg,
                        use_num_lit=gate in ("mul", "num"), use_txt_lit=gate in ("mul", "txt"), txt_lit_dim=40,
                        mlp_hidden_dim=48, mess_dropout=0.1, device=gpu_device)
    torch.manual_seed(0)
    num = torch.rand(n, 2) if cfg.use_num_lit else None
    txt = torch.randn(n, 40) if cfg.use_txt_lit else None
    m = L.LiteralKG(cfg, n, 16, io.initial_a_in(n, h, t, r), num, txt).to(gpu_device).train()
    batch = [torch.from_numpy(x).to(gpu_device) for x in make_batch(n, 100, 3, seed=1)]
    sizes = []
    for _ in range(5):
        loss = m(*batch, device=gpu_device, mode="pre_training")
        torch.cuda.synchronize()
        sizes.append(torch.cuda.memory_allocated())
    assert max(sizes[1:]) - min(sizes[1:]) < 4 << 20, [s_ >> 20 for s_ in sizes]      # (steady from the second call on)
    before = torch.cuda.memory_allocated()
    del loss
    m.zero_grad(set_to_none=True)
    gc.collect()
    # the model keeps its last table (gat_embed) and the layers' last normalised outputs, nothing else of the graph
    assert before - torch.cuda.memory_allocated() >= 0


def test_inference_heads_reuse_the_table_until_something_changes(L, O, gpu_device):
    """evaluate() (utils/model_utils.py:40-75) calls mode='predict' once per batch of heads under eval() + no_grad; the
    encoder's table is recomputed only when a parameter, A_in or a literal table changed since the last call."""
    from literalkg_amd.synth import make_kg
    from literalkg_amd import io
    n, dim = 5000, 32
    h, t, r = make_kg(n, 40_000, seed=4)
    cfg = O.default_cfg(embed_dim=dim, relation_dim=dim, conv_dim=dim, n_conv_layers=2, use_num_lit=True, device=gpu_device)
    torch.manual_seed(0)
    num = torch.rand(n, 2)
    m = L.LiteralKG(cfg, n, 16, io.initial_a_in(n, h, t, r), num, None).to(gpu_device)
    calls = []
    real = m.gat_embeddings
    m.gat_embeddings = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    heads = [torch.arange(i, i + 50, device=gpu_device) for i in (0, 50, 100)]
    tails = torch.arange(200, 700, device=gpu_device)
    m.eval()
    with torch.no_grad():
        s0 = [m(hh, tails, device=gpu_device, mode="predict") for hh in heads]
        assert len(calls) == 1                                   # three batches of heads, ONE encoder pass
        m.entity_embed.weight.mul_(1.5)                          # an in-place edit (an optimizer step is one)
        s1 = m(heads[0], tails, device=gpu_device, mode="predict")
        assert len(calls) == 2
        hd, td, rd = (torch.from_numpy(x).to(gpu_device) for x in (h, t, r))
        m(hd, td, rd, list(range(16)), device=gpu_device, mode="update_att")      # A_in replaced
        m(heads[0], tails, device=gpu_device, mode="predict")
        assert len(calls) == 3
        m.numerical_literals_embed.add_(0.25)                    # a literal table edited in place
        m(heads[0], tails, device=gpu_device, mode="predict")
        m(heads[1], tails, device=gpu_device, mode="predict")
        assert len(calls) == 4
    m(heads[0], tails, device=gpu_device, mode="predict")        # grad enabled: never cached
    m(heads[0], tails, device=gpu_device, mode="predict")
    assert len(calls) == 6
    m.train()
    with torch.no_grad():
        m(heads[0], tails, device=gpu_device, mode="predict")    # training mode (dropout): never cached
        m(heads[0], tails, device=gpu_device, mode="predict")
    assert len(calls) == 8
    # and the cached answers are the uncached ones
    m.eval()
    del m.gat_embeddings
    with torch.no_grad():
        a = m(heads[2], tails, device=gpu_device, mode="predict")
        m._eval_cache = None
        b = m(heads[2], tails, device=gpu_device, mode="predict")
    assert torch.equal(a, b) and s0[0].shape == (50, 500) and s1.shape == (50, 500)


def test_inference_table_is_dropped_by_training_steps_with_the_fused_adam(L, O, gpu_device):
    """predict -> 3 pre_training steps with literalkg_amd.optim.Adam (which writes the parameters through raw pointers), NO
    update_att in between -> predict: the second answer is an uncached recompute on the trained weights, not the table
    kept from the first call (round 2 returned the pre-training scores here)."""
    from literalkg_amd.optim import Adam
    from literalkg_amd.synth import make_batch, make_kg
    from literalkg_amd import io
    n, dim = 5000, 32
    h, t, r = make_kg(n, 40_000, seed=4)
    for form in ("transr", "transe"):
        cfg = O.default_cfg(embed_dim=dim, relation_dim=dim, conv_dim=dim, n_conv_layers=1 if form == "transr" else 2,
                            scale_gat_dim=None if form == "transr" else dim, device=gpu_device)
        torch.manual_seed(0)
        m = L.LiteralKG(cfg, n, 16, io.initial_a_in(n, h, t, r), scoring=form).to(gpu_device)
        heads, tails = torch.arange(0, 50, device=gpu_device), torch.arange(200, 700, device=gpu_device)
        m.eval()
        with torch.no_grad():
            s0 = m.calc_score(heads, tails).clone()
        assert m.__dict__.get("_eval_cache") is not None
        opt = Adam(m.parameters(), lr=1e-2)
        batch = [torch.from_numpy(x).to(gpu_device) for x in make_batch(n, 100, 3, seed=1)]
        versions = [p._version for p in m.parameters() if p.requires_grad]
        m.train()
        assert m.__dict__.get("_eval_cache") is None              # entering training mode lets the N x C table go
        for _ in range(3):
            opt.zero_grad(set_to_none=True)
            m(*batch, device=gpu_device, mode="pre_training").backward()
            opt.step()
        after = [p._version for p in m.parameters() if p.requires_grad]
        assert all(b_ > a_ for a_, b_, p in zip(versions, after, [p for p in m.parameters() if p.requires_grad])
                   if p.grad is not None)                          # the raw-pointer update shows in the version counter
        m.eval()
        with torch.no_grad():
            s1 = m.calc_score(heads, tails).clone()
            m._eval_cache = None
            s2 = m.calc_score(heads, tails)
        assert torch.equal(s1, s2)
        assert float((s1 - s0).abs().max()) > 1e-4
        # ... and WITHOUT leaving eval mode (a driver that trains under eval(), dropout off): the cache key alone must see it
        with torch.no_grad():
            m.calc_score(heads, tails)
        assert m.__dict__.get("_eval_cache") is not None
        opt.zero_grad(set_to_none=True)
        m(*batch, device=gpu_device, mode="pre_training").backward()
        kept = m.__dict__.get("_eval_cache")
        opt.step()
        with torch.no_grad():
            s3 = m.calc_score(heads, tails).clone()
            m._eval_cache = None
            s4 = m.calc_score(heads, tails)
        assert torch.equal(s3, s4) and float((s3 - s1).abs().max()) > 1e-5
        if kept is not None:                                       # (had the table survived the step, its key must not match)
            assert kept[0] != m._eval_key()


def test_out_of_range_ids_raise_inside_the_call(L, O, gpu_device):
    """The reference's embedding lookups raise before anything is updated (model.py:366-384); here the ids are sanitised on
    the device and the count is read behind the encoder's launches -- still inside the SAME call, before a loss exists."""
    from literalkg_amd.synth import make_batch, make_kg
    from literalkg_amd import io, ops
    n, dim = 3000, 32
    h, t, r = make_kg(n, 20_000, seed=4)
    for form, rate in (("transr", 3), ("transr", 1), ("transe", 3)):
        cfg = O.default_cfg(embed_dim=dim, relation_dim=dim, conv_dim=dim, n_conv_layers=1, pre_training_neg_rate=rate,
                            scale_gat_dim=None if form == "transr" else dim, device=gpu_device)
        m = L.LiteralKG(cfg, n, 16, io.initial_a_in(n, h, t, r), scoring=form).to(gpu_device).train()
        bh, br, bp, bn = [torch.from_numpy(x).to(gpu_device) for x in make_batch(n, 60, 3, seed=1)]
        bad = bn.clone()
        bad[7] = n + 5
        with pytest.raises(IndexError):
            m(bh, br, bp, bad, device=gpu_device, mode="pre_training")
        ops.check_deferred_errors()                                # nothing left pending: the error was raised where it belongs
        float(m(bh, br, bp, bn, device=gpu_device, mode="pre_training"))
        with pytest.raises(IndexError):
            m(bh, bp, bad, device=gpu_device, mode="fine_tuning")
        m.eval()
        with torch.no_grad(), pytest.raises(IndexError):
            m(bad[:20], bp[:10], device=gpu_device, mode="predict")
        ops.check_deferred_errors()


def test_module_moves_and_reloads_on_device(L, O, gpu_device):
    gd = load_golden("encoder_gcn_l2_scale")
    m = _build_model(L, gd, torch.device("cpu"), "transr")            # built and loaded on the CPU
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m.to(gpu_device)                                                  # model.to(device), main_pretraining.py:74
    batch = [torch.from_numpy(gd[k]).to(gpu_device) for k in ("bh", "br", "bp", "bn")]
    l1 = float(m(*batch, device=gpu_device, mode="pre_training"))
    np.testing.assert_allclose(l1, float(gd["loss"]), rtol=1e-5)
    m2 = L.LiteralKG(golden_cfg(gd), int(gd["n"]), int(gd["n_rel"])).to(gpu_device).eval()
    m2.load_state_dict(sd)                                            # CPU checkpoint into a device module
    assert m2.A_in.is_sparse and m2.A_in.device.type == "cuda"
    np.testing.assert_allclose(float(m2(*batch, device=gpu_device, mode="pre_training")), l1, rtol=1e-6)
    m2.A_in.data._values().mul_(2.0)                                  # in-place edit of the values is picked up
    l3 = float(m2(*batch, device=gpu_device, mode="pre_training"))
    assert abs(l3 - l1) > 1e-6


# ----------------------------------------------------------------------------- batch-pruned step == dense step
@pytest.mark.parametrize("name", ["encoder_gcn_l1", "encoder_gcn_l2_scale", "encoder_gcn_l2_res_wide", "encoder_sage_l2",
                                  "encoder_sage_l1_res", "encoder_bi_l2", "encoder_bi_l1_res", "encoder_gcn_l1_gatemul",
                                  "encoder_gcn_l2_gatenum", "encoder_gcn_l1_gatetxt_scale", "transe_gcn_l2_gatemul"])
def test_pruned_step_matches_reference_fixture(L, gpu_device, name):
    """prune_to_batch evaluates each layer on the batch's L-hop frontier only; loss, scores and every
    parameter gradient must equal what the REFERENCE produced with its full-graph recompute."""
    gd = load_golden(name)
    form = str(gd["form"])
    m = _build_model(L, gd, gpu_device, form)
    m.prune_to_batch = True
    m.prune_max_fraction = 1.0                     # tiny fixture graph: keep the compact path even at ~100 % coverage
    batch = [torch.from_numpy(gd[k]).to(gpu_device) for k in ("bh", "br", "bp", "bn")]
    loss = m(*batch, device=gpu_device, mode="pre_training")
    assert m.gat_rows is not None and m.gat_embed.shape[0] == m.gat_rows.numel() < int(gd["n"])
    np.testing.assert_allclose(m.gat_embed.detach().cpu().numpy(), gd["gat"][m.gat_rows.cpu().numpy()], rtol=TOL,
                               atol=TOL)
    np.testing.assert_allclose(m.last_scores["pos"].cpu().numpy(), gd["pos"], rtol=TOL, atol=TOL)
    np.testing.assert_allclose(float(loss.detach()), float(gd["loss"]), rtol=1e-5)
    loss.backward()
    grads = {k: v.grad for k, v in m.named_parameters() if v.grad is not None}
    for k, want in gd.items():
        if k.startswith("g/"):
            assert k[2:] in grads, k
            fixture_grad_close(grads[k[2:]].cpu().numpy(), want, name + " (pruned)", k[2:])
    if form == "transr":
        hid, tid = torch.from_numpy(gd["score_heads"]).to(gpu_device), torch.from_numpy(gd["score_tails"]).to(gpu_device)
        with torch.no_grad():
            np.testing.assert_allclose(m.calc_score(hid, tid).cpu().numpy(), gd["score"], rtol=TOL, atol=TOL)
        m.zero_grad()
        ft = m(batch[0], batch[2], batch[3], device=gpu_device, mode="fine_tuning")
        np.testing.assert_allclose(float(ft.detach()), float(gd["ft_loss"]), rtol=1e-5)
        ft.backward()
        np.testing.assert_allclose(m.entity_embed.weight.grad.cpu().numpy(), gd["ft_g/entity_embed.weight"],
                                   rtol=2e-3, atol=2e-6)


def test_pruned_step_backs_off_when_the_frontier_covers_the_graph(L, gpu_device):
    """prune_to_batch on a model whose frontier outgrows prune_max_fraction (here: the fixture graph with the fraction set to a
    few rows): the step falls back to the dense path with the dense path's results, and the next PRUNE_RETRY_EVERY - 1 calls
    of forward() do not pay for another attempt; then pruning is tried again."""
    gd = load_golden("encoder_gcn_l2_gatenum")
    m = _build_model(L, gd, gpu_device, "transr")
    batch = [torch.from_numpy(gd[k]).to(gpu_device) for k in ("bh", "br", "bp", "bn")]
    m.prune_to_batch = True
    m.prune_max_fraction = 1e-3                    # nothing fits: every attempt gives up at its first level
    m.PRUNE_RETRY_EVERY = 3
    loss = m(*batch, device=gpu_device, mode="pre_training")
    np.testing.assert_allclose(float(loss.detach()), float(gd["loss"]), rtol=1e-5)
    assert m.gat_rows is None and m._prune_skip == 3 and not m._can_prune()
    for left in (2, 1):
        again = m(*batch, device=gpu_device, mode="pre_training")
        assert m._prune_skip == left and float(again.detach()) == pytest.approx(float(loss.detach()), rel=1e-6)
    m(*batch, device=gpu_device, mode="pre_training")     # the back-off is over: this call tries again (and backs off again)
    assert m._prune_skip == 3
    m.prune_max_fraction = 1.0                     # ... and prunes when the frontier fits
    m._prune_skip = 0
    pruned_loss = m(*batch, device=gpu_device, mode="pre_training")
    assert m.gat_rows is not None
    np.testing.assert_allclose(float(pruned_loss.detach()), float(gd["loss"]), rtol=1e-5)


def test_pruned_trajectory_matches_reference(L, gpu_device):
    gd = load_golden("trajectory_gcn_l2_gatemul_scale")
    m = _build_model(L, gd, gpu_device, "transr")
    m.prune_to_batch = True
    m.prune_max_fraction = 1.0
    m.train()
    opt = torch.optim.Adam(m.parameters(), lr=float(gd["lr"]))
    h, t, r = (torch.from_numpy(gd[k]).to(gpu_device) for k in "htr")
    for step, b in enumerate(gd["batches"]):
        opt.zero_grad()
        loss = m(*[torch.from_numpy(x).to(gpu_device) for x in b], device=gpu_device, mode="pre_training")
        loss.backward()
        opt.step()
        np.testing.assert_allclose(loss.item(), gd["losses"][step], rtol=1e-4, err_msg=f"step {step}")
        if step == int(gd["refresh_after"]):
            m(h, t, r, list(range(int(gd["n_rel"]))), device=gpu_device, mode="update_att")
    np.testing.assert_allclose(m.entity_embed.weight.detach().cpu().numpy(), gd["f/entity_embed.weight"], rtol=2e-3,
                               atol=2e-5)


def test_pruning_falls_back_when_the_frontier_is_large(L, gpu_device):
    gd = load_golden("encoder_gcn_l2_scale")
    m = _build_model(L, gd, gpu_device, "transr")
    m.prune_to_batch = True
    m.prune_max_fraction = 0.05                     # the 2-hop frontier of 120 triples covers far more than 5 %
    batch = [torch.from_numpy(gd[k]).to(gpu_device) for k in ("bh", "br", "bp", "bn")]
    loss = m(*batch, device=gpu_device, mode="pre_training")
    assert m.gat_rows is None and m.gat_embed.shape[0] == int(gd["n"])
    np.testing.assert_allclose(float(loss.detach()), float(gd["loss"]), rtol=1e-5)


def test_pruned_step_on_a_batch_whose_rows_have_no_edges(L, O, gpu_device):
    """prune_to_batch with a batch made of entities that are nobody's head (found by the randomised sweep, seed 6217: 9 000
    entities / 9 000 triples, a batch of one): the compact sub-structures hold rows and no entries; forward and backward run,
    and loss and gradients equal the unpruned step's."""
    from literalkg_amd import io
    n, dim = 400, 32
    rng = np.random.default_rng(4)
    h, t, r = rng.integers(200, n, 1500), rng.integers(0, n, 1500), rng.integers(0, 3, 1500)      # heads among 200..399 only
    trip = np.unique(np.stack([h, r, t], 1), axis=0)
    h, r, t = trip[:, 0].copy(), trip[:, 1].copy(), trip[:, 2].copy()
    cfg = O.default_cfg(embed_dim=dim, relation_dim=dim, conv_dim=16, n_conv_layers=2, aggregation_type="gcn", scale_gat_dim=24,
                        use_num_lit=True, device=gpu_device)
    torch.manual_seed(0)
    m = L.LiteralKG(cfg, n, 3, io.initial_a_in(n, h, t, r), torch.rand(n, 2), None).to(gpu_device).eval()
    ids = [torch.tensor(x, device=gpu_device) for x in ([3, 3], [0, 1], [7, 11], [19, 5])]          # all below 200: no out-edges
    res = {}
    for prune in (True, False):
        m.prune_to_batch = prune
        out = []
        for mode, args in (("pre_training", ids), ("fine_tuning", [ids[0], ids[2], ids[3]])):
            m.zero_grad(set_to_none=True)
            loss = m(*args, device=gpu_device, mode=mode)
            loss.backward()
            out.append((float(loss.detach()), {k: v.grad.clone() for k, v in m.named_parameters() if v.grad is not None}))
        res[prune] = out
    for (lp, gp), (ld, gd) in zip(res[True], res[False]):
        assert abs(lp - ld) <= 1e-6 * max(1.0, abs(ld))
        assert gp.keys() == gd.keys()
        for k in gd:
            torch.testing.assert_close(gp[k], gd[k], rtol=1e-4, atol=1e-7, msg=k)


def test_gin_ignores_prune_flag(L, gpu_device):
    gd = load_golden("encoder_gin_l2")
    m = _build_model(L, gd, gpu_device, "transr")
    m.prune_to_batch = True
    batch = [torch.from_numpy(gd[k]).to(gpu_device) for k in ("bh", "br", "bp", "bn")]
    loss = m(*batch, device=gpu_device, mode="pre_training")
    assert m.gat_rows is None and m.gat_embed.shape[0] == int(gd["n"])
    np.testing.assert_allclose(float(loss.detach()), float(gd["loss"]), rtol=1e-5)


# ----------------------------------------------------------------------------- HIP path vs the plain-C oracle
@pytest.mark.parametrize("d", [128, 256])
def test_hip_matches_plain_c_oracle(L, ops, gpu_device, d):
    """oracle/lkg_oracle.c: scalar C loops with double accumulation, independent of ATen."""
    from oracle import c_oracle
    rng = np.random.default_rng(d)
    n = 4000
    h, t, r = rand_graph(rng, n, 50000, n_rel=8, long_rows=[(17, 700)])
    extra = np.stack([h[:100], (r[:100] + 3) % 8, t[:100]], 1)
    trip = np.unique(np.concatenate([np.stack([h, r, t], 1), extra]), axis=0)
    h, r, t = trip[:, 0].copy(), trip[:, 1].copy(), trip[:, 2].copy()
    ent = (rng.standard_normal((n, d)) * 0.3).astype(np.float32)
    rel = (rng.standard_normal((8, d)) * 0.3).astype(np.float32)
    g = L.KGStructure.from_triples(n, h, t, r, device=gpu_device)
    val, _ = ops.edge_softmax(g, torch.from_numpy(ent).to(gpu_device), torch.from_numpy(rel).to(gpu_device))
    rows, cols, want = c_oracle.attention(h, t, r, ent, rel)
    assert np.array_equal(g.coo_indices().cpu().numpy(), np.stack([rows, cols]))
    np.testing.assert_allclose(val.cpu().numpy(), want, rtol=1e-4, atol=1e-7)
    x = rng.standard_normal((n, d)).astype(np.float32)
    got = ops.spmm_raw(g.rowptr, g.col, val, torch.from_numpy(x).to(gpu_device), n, long_rows=g.long_rows(False))
    ref = c_oracle.spmm(g.host("rowptr"), g.host("col"), val.cpu().numpy(), x)
    np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=1e-5, atol=1e-5)


# ----------------------------------------------------------------------------- edge cases the reference's loops tolerate
def test_edge_cases_small_batches_dtypes_and_empty_graphs(L, ops, O, gpu_device):
    gd = load_golden("encoder_gcn_l1")
    m = _build_model(L, gd, gpu_device, "transr")
    p = golden_params(gd)
    cfg = golden_cfg(gd)
    n = int(gd["n"])
    a = torch.sparse_coo_tensor(torch.from_numpy(gd["a_indices"]), torch.from_numpy(gd["a_values"]), (n, n)).coalesce()
    # a single triple, ids given as int32 (the module widens them)
    one = [torch.tensor([x], dtype=torch.int32, device=gpu_device) for x in (3, 1, 5, 7)]
    got = m(*one, device=gpu_device, mode="pre_training")
    want = O.pre_training_loss(p, cfg, a, *[torch.tensor([x]) for x in (3, 1, 5, 7)])
    np.testing.assert_allclose(float(got.detach()), float(want), rtol=1e-5)
    got.backward()
    # all triples identical: duplicate rows scatter-add into the same gradient rows
    same = [torch.full((64,), x, dtype=torch.int64, device=gpu_device) for x in (3, 1, 5, 7)]
    m.zero_grad()
    l2 = m(*same, device=gpu_device, mode="pre_training")
    l2.backward()
    pc = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in p.items()}
    w2 = O.pre_training_loss(pc, cfg, a, *[torch.full((64,), x) for x in (3, 1, 5, 7)])
    w2.backward()
    np.testing.assert_allclose(float(l2.detach()), float(w2), rtol=1e-5)
    torch.testing.assert_close(m.gat_trans_M.grad.cpu(), pc["gat_trans_M"].grad, rtol=1e-3, atol=1e-7)
    torch.testing.assert_close(m.entity_embed.weight.grad.cpu(), pc["entity_embed.weight"].grad, rtol=1e-3, atol=1e-7)
    # update_att on an edge list that leaves most rows (or all rows) empty
    e = torch.zeros(0, dtype=torch.int64, device=gpu_device)
    m(e, e, e, [0, 1], device=gpu_device, mode="update_att")
    assert m.A_in._nnz() == 0
    z = m(*same, device=gpu_device, mode="pre_training")           # side = 0 everywhere: still a finite loss
    assert torch.isfinite(z)
    hh = torch.tensor([n - 1], device=gpu_device)
    m(hh, torch.tensor([0], device=gpu_device), torch.tensor([2], device=gpu_device), [2], device=gpu_device,
      mode="update_att")
    av = m.A_in.data
    assert av._nnz() == 1 and float(av.values()[0]) == 1.0 and av.indices().flatten().tolist() == [n - 1, 0]
    with pytest.raises(ValueError, match="empty graph"):
        from literalkg_amd.sampler import KGBatchSampler
        KGBatchSampler(L.KGStructure.from_triples(4, np.zeros(0, np.int64), np.zeros(0, np.int64), None,
                                                  device=gpu_device), 3)


@pytest.mark.parametrize("d", [64, 256, 32, 30])
def test_spmm_over_mostly_empty_rows_takes_the_row_lists(L, ops, gpu_device, d):
    """A structure whose rows are mostly empty (the reference's sparse id spaces, dataloader.py:405-418) is aggregated row list
    by row list: same bits as the one-wave-per-row launch, with every epilogue extra (self, second addend / bias row, row copy,
    row maxima), on the 16-byte and the scalar path, forward and transpose."""
    rng = np.random.default_rng(d)
    n, e = 60_000, 40_000
    used = rng.choice(n, 8_000, replace=False)
    h, t, r = used[rng.integers(0, len(used), e)], rng.integers(0, n, e), rng.integers(0, 4, e)
    h[:600] = used[0]                                           # one row beyond the long-row threshold
    g = L.KGStructure.from_triples(n, h, t, r, device=gpu_device)
    lists = g.row_lists(False)
    assert lists is not None and lists[0].numel() + lists[1].numel() == n and lists[0].numel() <= 8_000
    assert g.row_lists(True) is None or g.row_lists(True)[0].numel() + g.row_lists(True)[1].numel() == n
    val = torch.rand(g.nnz, device=gpu_device)
    val_t = ops.permute_values(val, g.t_perm)
    x = torch.randn(n, d, device=gpu_device)
    add2 = torch.randn(n, d, device=gpu_device)
    bias = torch.randn(d, device=gpu_device)
    for rowptr, col, v, transposed in ((g.rowptr, g.col, val, False), (g.t_rowptr, g.t_col, val_t, True)):
        rl = g.row_lists(transposed)
        if rl is None:
            continue
        long_rows = g.long_rows(transposed)
        for kw in (dict(), dict(add_self=x), dict(add_self=x, add2=add2), dict(bias=bias), dict(add_self=x, want_copy=True),
                   dict(add_self=x, want_rowmax=True)):
            kw = dict(kw)
            outs = []
            for use in (None, rl):
                k2 = {k_: v_ for k_, v_ in kw.items() if not k_.startswith("want_")}
                cdst = torch.zeros(n, d, device=gpu_device) if kw.get("want_copy") else None
                rm = torch.empty(n, device=gpu_device) if kw.get("want_rowmax") else None
                out = torch.full((n, d), 7.0, device=gpu_device)
                ops.spmm_raw(rowptr, col, v, x, n, out=out, long_rows=long_rows, row_lists=use,
                             copy=(x, cdst) if cdst is not None else None, rowmax=rm, **k2)
                outs.append((out, cdst, rm))
            (o0, c0, m0), (o1, c1, m1) = outs
            if d == 32:       # (8 chunks: the unlisted launch is the eight-rows-per-wave kernel, another order of the float sums)
                torch.testing.assert_close(o0, o1, rtol=1e-5, atol=1e-5)
            else:
                assert torch.equal(o0, o1), (d, transposed, sorted(kw))
            assert c0 is None or (torch.equal(c0, c1) and torch.equal(c1, x))
            assert m0 is None or (torch.allclose(m0, m1, rtol=1e-5, atol=1e-6) if d == 32 else torch.equal(m0, m1))


def test_module_step_on_a_sparse_id_space_equals_the_unlisted_launches(L, O, gpu_device):
    """BASELINE config[0]'s shape in small: most entity rows never occur as a head.  The module's step with the row lists
    (default from 50 % empty rows on) equals the step with them switched off, bit for bit in the loss and to float-atomics
    noise in the gradients."""
    from literalkg_amd.synth import make_batch
    from literalkg_amd import io
    rng = np.random.default_rng(3)
    n, e, dim = 50_000, 30_000, 64
    used = rng.choice(n, 6_000, replace=False)
    h, t, r = used[rng.integers(0, len(used), e)], used[rng.integers(0, len(used), e)], rng.integers(0, 16, e)
    cfg = O.default_cfg(embed_dim=dim, relation_dim=dim, conv_dim=dim, n_conv_layers=1, aggregation_type="gcn",
                        kg_l2loss_lambda=1e-4, device=gpu_device)
    a_in = io.initial_a_in(n, h, t, r)
    batch = [torch.from_numpy(x).to(gpu_device) for x in make_batch(n, 100, 3, seed=2)]
    res = []
    saved = L.KGStructure.EMPTY_ROWS_LISTED_FROM
    try:
        for frac in (saved, 2.0):
            L.KGStructure.EMPTY_ROWS_LISTED_FROM = frac
            torch.manual_seed(1)
            m = L.LiteralKG(cfg, n, 16, a_in).to(gpu_device).eval()
            assert (m._attention().graph.row_lists(False) is not None) == (frac <= 1.0)
            loss = m(*batch, device=gpu_device, mode="pre_training")
            loss.backward()
            res.append((float(loss.detach()), {k: v.grad.clone() for k, v in m.named_parameters() if v.grad is not None}))
    finally:
        L.KGStructure.EMPTY_ROWS_LISTED_FROM = saved
    (l1, g1), (l0, g0) = res
    assert l1 == l0
    for k in g0:
        scale = float(g0[k].abs().max()) + 1e-30
        assert float((g1[k] - g0[k]).abs().max()) <= 5e-5 * scale, k


@pytest.mark.parametrize("kind", ["random-walk", "symmetric"])
def test_device_laplacian_matches_the_reference_loader_and_the_host_form(L, gpu_device, kind):
    """io.initial_a_in on the device (radix-sort structure build + lkg_laplacian_device_f32) against the fixture the
    reference's own create_adjacency_dict / create_laplacian_dict produced (dataloader.py:449-495), and bit for bit against
    the host form on a graph with duplicate (h, t) pairs, empty rows and tails without out-edges."""
    from literalkg_amd import io
    from literalkg_amd.synth import make_kg
    gd = load_golden("laplacian_rand260")
    n = int(gd["n"])
    key = kind.replace("-", "_")
    a = io.initial_a_in(n, gd["h"], gd["t"], gd["r"], kind, device=gpu_device)
    assert a.is_cuda and a.is_coalesced()
    assert np.array_equal(a.indices().cpu().numpy(), gd[key + "_indices"])
    np.testing.assert_allclose(a.values().cpu().numpy(), gd[key + "_values"], rtol=1e-6, atol=1e-7)
    n2 = 30_000
    h, t, r = make_kg(n2, 200_000, seed=8, dup_frac=5e-3)
    h = np.where(h % 7 == 0, h // 7, h)                      # more empty rows, heavier heads
    host = io.initial_a_in(n2, h, t, r, kind)
    dev = io.initial_a_in(n2, h, t, r, kind, device=gpu_device)
    assert torch.equal(dev.indices().cpu(), host.indices())
    assert torch.equal(dev.values().cpu(), host.values())     # same f64 arithmetic: same bits


def test_update_att_structure_cache_follows_content(L, O, gpu_device):
    """The (h,t)-sorted structure is cached across epochs by CONTENT of the edge lists: a re-uploaded copy reuses
    it, a different list of the same length (possibly at the same address) does not."""
    gd = load_golden("encoder_gcn_l1")
    m = _build_model(L, gd, gpu_device, "transr")
    n, n_rel = int(gd["n"]), int(gd["n_rel"])
    rel = list(range(n_rel))
    h, t, r = (torch.from_numpy(gd[k]).to(gpu_device) for k in "htr")
    m(h, t, r, rel, device=gpu_device, mode="update_att")
    g1 = m._triple_graph
    m(h.clone(), t.clone(), r.clone(), rel, device=gpu_device, mode="update_att")
    assert m._triple_graph is g1                                   # same content, new tensors: reused
    t2 = t.clone()
    t2[:50] = (t2[:50] + 1) % n
    t.copy_(t2)                                                    # same tensor object and address, new content
    m(h, t, r, rel, device=gpu_device, mode="update_att")
    assert m._triple_graph is not g1
    # two edges swap their tails: every per-list sum stays the same, only an exact compare sees the change
    g2 = m._triple_graph
    i, j = 0, int(torch.nonzero((h != h[0]) & (t != t[0]))[0])
    t3 = t.clone()
    t3[i], t3[j] = t[j], t[i]
    t.copy_(t3)
    m(h, t, r, rel, device=gpu_device, mode="update_att")
    assert m._triple_graph is not g2
    p = golden_params(gd)
    want = O.attention_refresh(n, p["entity_embed.weight"], p["relation_embed.weight"], h.cpu(), t.cpu(), r.cpu()).coalesce()
    assert torch.equal(m.A_in.data.indices().cpu(), want.indices())
    torch.testing.assert_close(m.A_in.data.values().cpu(), want.values(), rtol=1e-5, atol=1e-7)


def test_runs_under_autograd_anomaly_mode(L, gpu_device):
    """The reference's driver keeps torch.autograd.set_detect_anomaly(True) on (main_pretraining.py:45)."""
    gd = load_golden("encoder_gcn_l2_gatenum")
    m = _build_model(L, gd, gpu_device, "transr")
    m.train()
    batch = [torch.from_numpy(gd[k]).to(gpu_device) for k in ("bh", "br", "bp", "bn")]
    with torch.autograd.detect_anomaly(check_nan=True):
        loss = m(*batch, device=gpu_device, mode="pre_training")
        loss.backward()
    np.testing.assert_allclose(loss.item(), float(gd["loss"]), rtol=1e-5)
    assert all(torch.isfinite(p.grad).all() for k, p in m.named_parameters() if p.grad is not None)


# ----------------------------------------------------------------------------- f1 MLP head (mode='mlp')
@pytest.mark.parametrize("name", golden_names("mlp_"))
def test_mlp_head_matches_reference_fixture(L, gpu_device, name):
    gd = load_golden(name)
    scoring = "transr" if bool(gd["init_mlp"]) else "transe"      # model.py builds the head on demand, model_bce.py in its ctor
    cfg = golden_cfg(gd)
    n = int(gd["n"])
    a_in = torch.sparse_coo_tensor(torch.from_numpy(gd["a_indices"]), torch.from_numpy(gd["a_values"]), (n, n)).coalesce()
    m = L.LiteralKG(cfg, n, int(gd["n_rel"]), a_in, scoring=scoring)
    if scoring == "transr":
        with pytest.raises(AttributeError, match="initialize_MLP"):
            m.train_MLP(torch.zeros(2, dtype=torch.long), torch.zeros(2, dtype=torch.long))
        m.initialize_MLP()
    params = golden_params(gd)
    res = m.load_state_dict(params, strict=False)
    assert res.missing_keys == ["A_in"] and not res.unexpected_keys, res          # same keys as the reference
    m.to(gpu_device).train()
    heads, tails = (torch.from_numpy(gd[k]).to(gpu_device) for k in ("heads", "tails"))
    out = m(heads, tails, device=gpu_device, mode="mlp")
    assert out.shape == (96, 1)
    np.testing.assert_allclose(out.detach().cpu().numpy().reshape(-1), gd["out_train"], rtol=1e-4, atol=1e-5)
    loss = torch.nn.functional.binary_cross_entropy(out.reshape(-1), torch.from_numpy(gd["labels"]).to(gpu_device))
    np.testing.assert_allclose(loss.item(), float(gd["loss"]), rtol=1e-5)
    loss.backward()
    grads = {k: v.grad for k, v in m.named_parameters() if v.grad is not None}
    for k, want in gd.items():
        if k.startswith("g/"):
            assert k[2:] in grads, k
            fixture_grad_close(grads[k[2:]].cpu().numpy(), want, "mlp head", k[2:])
    sd = m.state_dict()
    for k, want in gd.items():
        if k.startswith("after/"):                               # running statistics and the batch counter
            np.testing.assert_allclose(sd[k[6:]].cpu().numpy(), want, rtol=1e-4, atol=1e-6, err_msg=k)
    m.eval()
    with torch.no_grad():
        out_eval = m(heads, tails, device=gpu_device, mode="mlp")
    np.testing.assert_allclose(out_eval.cpu().numpy().reshape(-1), gd["out_eval"], rtol=1e-4, atol=1e-5)


# ----------------------------------------------------------------------------- bench.py output contract
def test_bench_prints_one_contract_line(gpu_device):
    """`python bench.py --full` prints exactly one JSON line with the driver's keys plus `roofline` and `cpu_baseline`
    (small graph here; the default run uses the BASELINE shape)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--full", "--steps", "3", "--warmup", "1",
                          "--entities", "50000", "--edges", "500000"], capture_output=True, text=True, timeout=600,
                         cwd=root)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    j = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in j, key
    assert j["metric"] == "kg_edges_aggregated_per_sec" and j["unit"] == "edges/s"
    assert j["n_gpus"] == 1 and j["steps"] == 3 and j["warmup"] == 1 and j["higher_is_better"] is True
    assert j["dtype"] == "f32" and j["data"] == "synthetic" and "workload" in j["config"]
    assert j["config"]["spot_check"] == "ok"
    assert abs(j["value"] - j["config"]["edge_aggregations_per_step"] / j["ms_per_step"] * 1e3) < 1e-6 * j["value"]
    r = j["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in r, key
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    c = j["cpu_baseline"]
    for key in ("value", "unit", "cores", "kind", "sample"):
        assert key in c, key
    assert c["kind"] in ("port", "reference") and c["value"] > 0


def test_bench_plain_run_is_the_headline_and_dumps_its_outputs(gpu_device, tmp_path):
    """A plain `python bench.py` times the steps it is given and reports them, and nothing else (no spot check, no
    `cpu_baseline`, no `extra`); `--dump-outputs DIR` writes what the last timed step computed -- the same seeded rows of
    the forward `side` and the backward `grad_ego`, float32, 64 MB at most -- and a second run writes the same arrays."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dumps = []
    for k in range(2):
        out = tmp_path / f"run{k}"
        res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "4", "--warmup", "1",
                              "--entities", "50000", "--edges", "500000", "--dump-outputs", str(out)],
                             capture_output=True, text=True, timeout=600, cwd=root)
        assert res.returncode == 0, res.stderr[-2000:]
        lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, lines
        j = json.loads(lines[0])
        assert j["steps"] == 4 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["dtype"] == "f32"
        assert abs(j["value"] - j["config"]["edge_aggregations_per_step"] / j["ms_per_step"] * 1e3) < 1e-6 * j["value"]
        assert "cpu_baseline" not in j and "extra" not in j and j["config"]["spot_check"].startswith("not run")
        assert sorted(os.listdir(out)) == ["grad_ego.npy", "side.npy"]
        dumps.append({name: np.load(out / f"{name}.npy") for name in ("side", "grad_ego")})
    assert sum(a.nbytes for a in dumps[0].values()) <= 64 << 20
    for name, a in dumps[0].items():
        assert a.dtype == np.float32 and a.shape == (16384, 256) and np.isfinite(a).all() and np.abs(a).max() > 0
        np.testing.assert_allclose(dumps[1][name], a, rtol=1e-5, atol=1e-6)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world,dim", [(2, 256), (4, 128)])
def test_bench_multi_rank_path_on_one_gpu(gpu_device, world, dim):
    """The N > 1 path of bench.py end to end (its own launcher, both sharding schemes, the pipelined exchanges -- at world 4
    and 32 columns per rank the head-part backward of the N = 8 run --, the integrated sharded step) with all ranks on the one
    GPU over gloo: exit code 0, one JSON line, both schemes at the top level, every spot check ok, no phase reported as failed.
    (The numbers of such a run mean nothing; the line says so in `data`.)"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(world), "--rehearse-on-one-gpu", "--steps", "2",
                          "--warmup", "1", "--entities", "30000", "--edges", "300000", "--dim", str(dim)],
                         capture_output=True, text=True, timeout=560, cwd=root)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["n_gpus"] == world and j["n_ranks_seen"] == world and j["scaling"] == "weak" and "REHEARSAL" in j["data"]
    assert j["value"] > 0 and j["value_rows"] > 0 and j["value_features"] > 0 and "rccl_version" in j
    assert j["config"]["value_scheme"] in ("features", "rows") and j["config"]["value_scheme"] in j["config"]["workload"]
    assert j["config"]["spot_check"] == "ok" and j["rows_scheme"]["spot_check"] == "ok"
    fx = j["features_exchanges"]
    assert fx["features"]["spot_check"] == "ok" and fx["features_pipelined"]["spot_check"] == "ok"
    assert "pipelined_exchange_error" not in fx and "hung_phase" not in j
    st = j["sharded_pre_training_step"]
    assert "error" not in st and st["rows"]["ms_per_step"] > 0 and st["features"]["ms_per_step"] > 0
    for scheme in ("rows", "features"):
        sent = st[scheme]["bytes_sent_per_step_rank0"]
        assert sent["head_rows"] > 0 and sent["weight_gradients"] > 0 and sent["aggregate_forward"] > 0


# ----------------------------------------------------------------------------- the loss's row-sparse table gradient
@pytest.mark.parametrize("scoring,layers,gate", [("transr", 1, None), ("transe", 2, "mul")])
def test_loss_row_scratch_equals_a_fresh_zero_table(L, ops, O, gpu_device, scoring, layers, gate):
    """The shared all-zero gradient table (ops._RowScratch: rows of the previous step reset, row flags for act_ln backward
    and the first layer's transpose SpMM) against a zeros_like table per step, three different batches in a row."""
    from literalkg_amd.synth import make_batch, make_kg
    from literalkg_amd import io
    n, e, dim = 20_000, 150_000, 64
    h, t, r = make_kg(n, e, seed=5)
    cfg = O.default_cfg(embed_dim=dim, relation_dim=dim if scoring == "transr" else dim * (layers + 1), conv_dim=dim,
                        n_conv_layers=layers, aggregation_type="gcn", use_num_lit=gate == "mul",
                        use_txt_lit=gate == "mul", txt_lit_dim=300, kg_l2loss_lambda=1e-4, device=gpu_device)
    torch.manual_seed(3)
    num = torch.rand(n, 2) if gate else None
    txt = torch.randn(n, 300) if gate else None
    m = L.LiteralKG(cfg, n, 16, io.initial_a_in(n, h, t, r), num, txt, scoring=scoring).to(gpu_device).eval()
    assert m._table_grad_stays_inside.__func__ is L.LiteralKG._table_grad_stays_inside
    ops._RowScratch._tables.clear()

    def grads(batch, sparse):
        m.zero_grad(set_to_none=True)
        m._table_grad_stays_inside = (lambda: m.gat_rows is None) if sparse else (lambda: False)
        m(*batch, device=gpu_device, mode="pre_training").backward()
        return {k: v.grad.clone() for k, v in m.named_parameters() if v.grad is not None}

    try:
        for seed in (9, 10, 11):
            batch = [torch.from_numpy(x).to(gpu_device) for x in make_batch(n, 150, 3, seed=seed)]
            got, want = grads(batch, True), grads(batch, False)
            assert got.keys() == want.keys()
            for k in want:     # same kernels on the same values; only the order of the float atomics differs (a stale or
                scale = float(want[k].abs().max()) + 1e-30      # missing row would show at 1e-3 .. 1 of the scale)
                assert float((got[k] - want[k]).abs().max()) <= 5e-5 * scale, k
        loss_tables = [e for k, e in ops._RowScratch._tables.items() if k[3] == "loss"]
        (ent,) = loss_tables
        assert int(ent.flags.sum()) > 0 and ops._storage_users(ent.buf) == ent.users    # nothing holds a view any more
        n_, c_, dev_ = ent.buf.shape[0], ent.buf.shape[1], ent.buf.device
        held = ent.table(ops.RowSet(ent.flags, ent.dirty))   # somebody keeps the gradient: the table must not be re-used
        ent2 = ops._RowScratch.acquire(n_, c_, dev_)
        assert ent2 is not ent and float(ent2.buf.abs().sum()) == 0.0
        del held
        ent3 = ops._RowScratch.acquire(n_, c_, dev_)
        assert ent3 is ent2
        ops._RowScratch._tables[(dev_, n_, c_, "loss", ops._stream())] = ent
        assert len(ent.dirty) == 3                           # the first table: its touched rows are reset on re-use
        assert ops._RowScratch.acquire(n_, c_, dev_) is ent
        assert float(ent.buf.abs().sum()) == 0.0 and int(ent.flags.sum()) == 0
        for k, e in list(ops._RowScratch._tables.items()):   # the last layer's g_z / g_x tables: zero again once their rows are reset
            if k[3] != "loss":
                assert ops._RowScratch.acquire(k[1], k[2], k[0], k[3]) is e and float(e.buf.abs().sum()) == 0.0, k
    finally:
        del m._table_grad_stays_inside
        ops._RowScratch._tables.clear()


def test_row_scratch_is_per_stream_and_survives_two_models_and_a_torch_without_the_use_count(L, ops, O, gpu_device):
    """The kept-zero tables under the call patterns a process can produce: two models of the SAME shape trained alternately
    (they share tables, step by step), the same two models on two different streams (a table belongs to one stream: its
    reset / scatter launches are ordered by that stream only), replica threads (the registry's lock), and a torch build
    without the storage use count (no table is ever re-used then; same gradients)."""
    import threading
    from literalkg_amd.synth import make_batch, make_kg
    from literalkg_amd import io
    n, e, dim = 20_000, 150_000, 64
    h, t, r = make_kg(n, e, seed=5)
    cfg = O.default_cfg(embed_dim=dim, relation_dim=dim, conv_dim=dim, n_conv_layers=2, aggregation_type="gcn",
                        kg_l2loss_lambda=1e-4, device=gpu_device)
    a_in = io.initial_a_in(n, h, t, r)
    models = []
    for seed in (1, 2):
        torch.manual_seed(seed)
        models.append(L.LiteralKG(cfg, n, 16, a_in).to(gpu_device).eval())
    batches = [[torch.from_numpy(x).to(gpu_device) for x in make_batch(n, 120, 3, seed=s_)] for s_ in (20, 21, 22, 23)]

    def step(m, batch):
        m.zero_grad(set_to_none=True)
        m(*batch, device=gpu_device, mode="pre_training").backward()
        return {k: v.grad.clone() for k, v in m.named_parameters() if v.grad is not None}

    def close(got, want):
        assert got.keys() == want.keys()
        for k in want:
            scale = float(want[k].abs().max()) + 1e-30
            assert float((got[k] - want[k]).abs().max()) <= 5e-5 * scale, k

    ops._RowScratch._tables.clear()
    try:
        # reference answers: every (model, batch) on fresh tables
        want = {}
        for i, m in enumerate(models):
            for j, b in enumerate(batches):
                ops._RowScratch._tables.clear()
                want[i, j] = step(m, b)
        # (1) alternating models on one stream, tables shared and re-used
        ops._RowScratch._tables.clear()
        for j, b in enumerate(batches):
            for i, m in enumerate(models):
                close(step(m, b), want[i, j])
        n_tables = len(ops._RowScratch._tables)
        assert n_tables >= 2 and len({k[4] for k in ops._RowScratch._tables}) == 1
        # (2) the two models on two side streams, interleaved: one set of tables per stream
        streams = [torch.cuda.Stream(device=gpu_device) for _ in models]
        got = {}
        for j, b in enumerate(batches):
            for i, m in enumerate(models):
                streams[i].wait_stream(torch.cuda.current_stream(gpu_device))
                with torch.cuda.stream(streams[i]):
                    got[i, j] = step(m, b)
        torch.cuda.synchronize()
        for key, g_ in got.items():
            close(g_, want[key])
        assert len({k[4] for k in ops._RowScratch._tables}) == 3
        # (3) replica threads (each on its own stream) hammering the registry
        errors = []

        def worker(i):
            try:
                with torch.cuda.stream(streams[i]):
                    for j, b in enumerate(batches):
                        close(step(models[i], b), want[i, j])
                    torch.cuda.synchronize()
            except Exception as exc:   # noqa: BLE001
                errors.append(repr(exc))
        threads = [threading.Thread(target=worker, args=(i,)) for i in range(len(models))]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        # (4) a torch without the storage use count: nothing is re-used, the answers stay
        ops._RowScratch._tables.clear()
        saved = ops._HAS_USE_COUNT
        ops._HAS_USE_COUNT = False
        try:
            first = None
            for j, b in enumerate(batches[:2]):
                close(step(models[0], b), want[0, j])
                ent = next(e for k, e in ops._RowScratch._tables.items() if k[3] == "loss")
                assert ent.users == -1 and ent is not first
                first = ent
        finally:
            ops._HAS_USE_COUNT = saved
    finally:
        ops._RowScratch._tables.clear()


@pytest.mark.parametrize("layers", [1, 2])
def test_row_sparse_backward_under_unusual_autograd_sequences(L, ops, O, gpu_device, layers):
    """The kept-zero gradient tables and row sets (ops._RowScratch / RowSet / the gradient frontier) under call sequences a
    plain training loop does not produce -- two forwards before ONE backward of the summed loss, gradient accumulation over
    two backward calls, a retained graph walked twice, the table's gradient held by the caller across the next step --
    each against the dense path (zeros_like table per step, no row sets)."""
    from literalkg_amd.synth import make_batch, make_kg
    from literalkg_amd import io
    n, e, dim = 40_000, 300_000, 64
    h, t, r = make_kg(n, e, seed=6)
    cfg = O.default_cfg(embed_dim=dim, relation_dim=dim, conv_dim=dim, n_conv_layers=layers, aggregation_type="gcn",
                        kg_l2loss_lambda=1e-4, device=gpu_device)
    torch.manual_seed(4)
    m = L.LiteralKG(cfg, n, 16, io.initial_a_in(n, h, t, r)).to(gpu_device).eval()
    b1, b2 = ([torch.from_numpy(x).to(gpu_device) for x in make_batch(n, 150, 3, seed=sd)] for sd in (21, 22))
    ops._RowScratch._tables.clear()

    def step(batch):
        return m(*batch, device=gpu_device, mode="pre_training")

    def run(seq, sparse):
        m.zero_grad(set_to_none=True)
        m._table_grad_stays_inside = (lambda: m.gat_rows is None) if sparse else (lambda: False)
        seq()
        return {k: v.grad.clone() for k, v in m.named_parameters() if v.grad is not None}

    def summed():
        (step(b1) + step(b2)).backward()

    def accumulated():
        step(b1).backward()
        step(b2).backward()

    def retained():
        loss = step(b1)
        loss.backward(retain_graph=True)
        loss.backward()

    held = {}

    def holding():
        loss = step(b1)
        table = m._gat_state[0]
        (g_table,) = torch.autograd.grad(loss, table, retain_graph=True)
        held["g"], held["copy"] = g_table, g_table.clone()
        loss.backward()
        step(b2).backward()                     # the next step must not touch the gradient the caller still holds

    try:
        for seq in (summed, accumulated, retained, holding):
            got, want = run(seq, True), run(seq, False)
            assert got.keys() == want.keys(), seq.__name__
            for k in want:
                scale = float(want[k].abs().max()) + 1e-30
                assert float((got[k] - want[k]).abs().max()) <= 5e-5 * scale, (seq.__name__, k)
            if seq is holding:
                assert torch.equal(held["g"], held["copy"])
        a, b = run(summed, True), run(accumulated, True)
        for k in a:
            assert float((a[k] - b[k]).abs().max()) <= 5e-5 * (float(a[k].abs().max()) + 1e-30), k
    finally:
        del m._table_grad_stays_inside
        held.clear()
        ops._RowScratch._tables.clear()


def test_row_flag_consumers_skip_exactly_the_zero_rows(ops, gpu_device):
    """lkg_fill_rows_f32 + the row-flag forms of act_ln backward and of the SpMM's second addend against the dense forms."""
    from literalkg_amd import _native as N
    from literalkg_amd.graph import KGStructure
    rng = np.random.default_rng(2)
    n, d = 3000, 96
    ids = torch.from_numpy(rng.choice(n, 40)).to(gpu_device)             # with duplicates
    table = torch.ones(n, d + 4, device=gpu_device)
    flags = torch.zeros(n, dtype=torch.uint8, device=gpu_device)
    N.call("lkg_fill_rows_f32", ids.numel(), d, N.ptr(ids), N.ptr(table), table.stride(0), 0.0, N.ptr(flags), 1, None)
    want = torch.ones(n, d + 4)
    want[ids.cpu(), :d] = 0
    assert torch.equal(table.cpu(), want)
    wf = torch.zeros(n, dtype=torch.uint8)
    wf[ids.cpu()] = 1
    assert torch.equal(flags.cpu(), wf)
    # act_ln backward: g_yn zero outside the flagged rows, with and without a dense g_y
    z = torch.randn(n, d, device=gpu_device, requires_grad=True)
    gamma = torch.rand(d, device=gpu_device, requires_grad=True)
    beta = torch.randn(d, device=gpu_device, requires_grad=True)
    gyn = torch.zeros(n, d, device=gpu_device)
    gyn[ids] = torch.randn(ids.numel(), d, device=gpu_device)
    gy = torch.randn(n, d, device=gpu_device)
    for use_gy in (False, True):
        res = []
        for tagged in (False, True):
            y, yn = ops.act_layernorm(z, gamma, beta)
            g2 = ops.tag_rows(gyn.clone(), ops.RowSet(flags, [ids])) if tagged else gyn
            res.append(torch.autograd.grad([y, yn] if use_gy else [yn], [z, gamma, beta], [gy, g2] if use_gy else [g2]))
        for a, b in zip(*res):
            assert torch.equal(a, b) or float((a - b).abs().max()) <= 5e-5 * float(b.abs().max())   # gamma / beta: float atomics, any order
        assert torch.equal(res[0][0], res[1][0])
    # SpMM second addend
    h, t = rng.integers(0, n, 20000), rng.integers(0, n, 20000)
    g = KGStructure.from_triples(n, h, t, np.zeros_like(h), device=gpu_device)
    val = torch.rand(g.nnz, device=gpu_device)
    x = torch.randn(n, d, device=gpu_device)
    for dd in (d, 32):
        a = ops.spmm_raw(g.rowptr, g.col, val, x[:, :dd], n, add2=gyn[:, :dd])
        b = ops.spmm_raw(g.rowptr, g.col, val, x[:, :dd], n, add2=gyn[:, :dd], add2_rows=flags)
        assert torch.equal(a, b)
        junk = torch.full((n, dd), float("nan"), device=gpu_device)      # unflagged rows are not even read
        junk[ids] = gyn[ids][:, :dd]
        c = ops.spmm_raw(g.rowptr, g.col, val, x[:, :dd], n, add2=junk, add2_rows=flags)
        assert torch.equal(a, c)


@pytest.mark.parametrize("n_w,d,n", [(1, 64, 5000), (2, 512, 70_001), (3, 100, 2048), (8, 256, 33_333)])
def test_narrow_panel_weight_gradient_and_bias_in_one_pass(ops, gpu_device, n_w, d, n):
    """lkg_colsum_weighted_f32 (gy^T @ narrow panel + column sums of gy) against f64, on strided views."""
    torch.manual_seed(n_w)
    gy = torch.randn(n, d + 8, device=gpu_device)[:, 4:4 + d]
    w = torch.rand(n, n_w + 3, device=gpu_device)[:, 1:1 + n_w]
    gw, gs = ops.narrow_weight_grad(gy, w, True)
    want_w = gy.double().t() @ w.double()
    want_s = gy.double().sum(0)
    scale_w = float((gy.double().abs().t() @ w.double().abs()).max())
    assert gw.shape == (d, n_w) and float((gw.double() - want_w).abs().max()) <= 2e-6 * scale_w
    assert float((gs.double() - want_s).abs().max()) <= 2e-6 * float(gy.double().abs().sum(0).max())
    gw2, none = ops.narrow_weight_grad(gy, w, False)
    assert none is None and float((gw2 - gw).abs().max()) <= 2e-6 * scale_w
    # through the Linear: y = x1 w1^T + x2 w2^T + b with a narrow second panel
    x1 = torch.randn(n, 32, device=gpu_device, requires_grad=True)
    w1 = torch.randn(d, 32, device=gpu_device, requires_grad=True)
    w2 = torch.randn(d, n_w, device=gpu_device, requires_grad=True)
    b = torch.randn(d, device=gpu_device, requires_grad=True)
    y = ops.multi_linear([x1, w.contiguous()], [w1, w2], b)
    g = torch.randn(n, d, device=gpu_device)
    got = torch.autograd.grad(y, [w1, w2, b], g)
    refs = torch.autograd.grad((x1.double() @ w1.double().t() + w.double() @ w2.double().t() + b.double()), [w1, w2, b],
                               g.double())
    for a, r in zip(got, refs):
        assert float((a.double() - r).abs().max()) <= 1e-5 * float(r.abs().max())


@pytest.mark.parametrize("d", [64, 128, 256, 300, 512])
def test_spmm_over_row_sparse_input_skips_exactly_the_zero_rows(ops, gpu_device, d):
    """x_rows / self_rows of lkg_spmm_csr_fused_f32: entries whose source row is unflagged are not gathered (NaN there
    must not leak), the result equals the dense product over the zero-filled table; long rows and empty rows included."""
    from literalkg_amd.graph import KGStructure
    rng = np.random.default_rng(d)
    n = 6000
    h, t, r = rand_graph(rng, n, 60_000, long_rows=((7, 900), (4001, 300)))
    g = KGStructure.from_triples(n, h, t, r, device=gpu_device)
    val = torch.rand(g.nnz, device=gpu_device)
    ids = torch.from_numpy(rng.choice(n, 80)).to(gpu_device)
    flags = torch.zeros(n, dtype=torch.uint8, device=gpu_device)
    flags[ids] = 1
    x = torch.zeros(n, d, device=gpu_device)
    x[ids] = torch.randn(ids.numel(), d, device=gpu_device)
    junk = torch.full((n, d), float("nan"), device=gpu_device)
    junk[ids] = x[ids]
    for rowptr, col, lr in ((g.rowptr, g.col, g.long_rows(False)), (g.t_rowptr, g.t_col, g.long_rows(True))):
        v = val if rowptr is g.rowptr else val[g.t_perm.long()] if hasattr(g, "t_perm") else val
        want = ops.spmm_raw(rowptr, col, v, x, n, long_rows=lr, add_self=x)
        got = ops.spmm_raw(rowptr, col, v, junk, n, long_rows=lr, add_self=junk, x_rows=flags, self_rows=flags)
        assert not torch.isnan(got).any()
        scale = float(want.abs().max())
        assert float((got - want).abs().max()) <= 1e-6 * scale      # (same products; the order of a row's sum may differ)
        got2 = ops.spmm_raw(rowptr, col, v, junk, n, long_rows=lr, x_rows=flags)
        want2 = ops.spmm_raw(rowptr, col, v, x, n, long_rows=lr)
        assert float((got2 - want2).abs().max()) <= 1e-6 * scale


def test_last_layer_backward_on_the_listed_rows_equals_the_dense_backward(ops, gpu_device):
    """act_ln backward with sparse_out + the Linear's backward over the listed rows (gathered once) against the dense forms."""
    torch.manual_seed(0)
    n, d_in, d_out = 40_000, 96, 64
    ids_lists = [torch.randint(0, n, (500,), device=gpu_device), torch.randint(0, n, (700,), device=gpu_device)]
    flags = torch.zeros(n, dtype=torch.uint8, device=gpu_device)
    for i in ids_lists:
        flags[i] = 1
    x = torch.randn(n, d_in, device=gpu_device, requires_grad=True)
    w = torch.randn(d_out, d_in, device=gpu_device, requires_grad=True)
    b = torch.randn(d_out, device=gpu_device, requires_grad=True)
    gamma = torch.rand(d_out, device=gpu_device, requires_grad=True)
    beta = torch.randn(d_out, device=gpu_device, requires_grad=True)
    gyn = torch.zeros(n, d_out, device=gpu_device)
    rows_idx = torch.nonzero(flags).flatten()
    gyn[rows_idx] = torch.randn(rows_idx.numel(), d_out, device=gpu_device)
    res = []
    for tagged in (False, True):
        y, yn = ops.act_layernorm(ops.linear(x, w, b), gamma, beta)
        g2 = ops.tag_rows(gyn.clone(), ops.RowSet(flags, ids_lists)) if tagged else gyn
        res.append(torch.autograd.grad([yn], [x, w, b, gamma, beta], [g2]))
    assert ops.rows_worth_compacting(ops.RowSet(flags, ids_lists), n)
    for name, a, r in zip("x w b gamma beta".split(), res[1], res[0]):
        assert float((a - r).abs().max()) <= 2e-5 * float(r.abs().max()), name
    assert float(res[1][0][flags == 0].abs().max()) == 0.0


@pytest.mark.parametrize("m,n,k,tb", [(50_000, 32, 32, 1), (50_000, 32, 32, 0), (9_001, 64, 16, 1), (4_096, 20, 44, 0),
                                      (30_000, 48, 64, 1), (12_345, 8, 60, 0)])
def test_skinny_products_on_the_valu(ops, gpu_device, m, n, k, tb):
    """lkg_gemm_skinny_f32 (A[m, k] . op(B) for k, n <= 64 over many rows: the Linears / data gradients / residual mixes of
    32-wide layers) through ops.gemm, against f64: plain, with bias, accumulating (beta = 1), on column slices of wider
    tables."""
    from literalkg_amd import _native as N
    torch.manual_seed(m + n)
    wide = torch.randn(m, k + 8, device=gpu_device)
    b = torch.randn((n, k) if tb else (k, n), device=gpu_device)
    bias = torch.randn(n, device=gpu_device)
    for a in (wide[:, :k].contiguous(), wide[:, 4:4 + k]):
        out_wide = torch.randn(m, n + 12, device=gpu_device)
        out = out_wide[:, 8:8 + n]
        assert N.load().lkg_gemm_skinny_ok(m, n, k, N.ptr(a), ops._ld(a), N.ptr(out), ops._ld(out))
        old = out.clone()
        want = a.double() @ (b.double().t() if tb else b.double())
        got = ops.gemm(a, b, trans_b=bool(tb))
        scale = (a.double().abs() @ (b.double().abs().t() if tb else b.double().abs())) + 1e-300
        ref32 = (a @ (b.t() if tb else b)).double()                                       # hipBLASLt f32
        e_f32 = float(((ref32 - want).abs() / scale).max())
        assert float(((got.double() - want).abs() / scale).max()) <= max(2 * e_f32, 5e-7)
        got_b = ops.gemm(a, b, trans_b=bool(tb), bias=bias)
        assert float(((got_b.double() - want - bias.double()).abs() / (scale + bias.abs().double())).max()) <= max(2 * e_f32, 5e-7)
        ops.gemm(a, b, trans_b=bool(tb), beta=1.0, out=out)
        assert float(((out.double() - want - old.double()).abs() / (scale + old.abs().double())).max()) <= max(2 * e_f32, 5e-7)
        assert torch.equal(out_wide[:, :8], out_wide[:, :8]) and float(out_wide[:, 8 + n:].abs().max()) > 0


@pytest.mark.parametrize("m,n,k", [(32, 32, 100_000), (32, 300, 50_001), (64, 64, 20_000), (16, 8, 4096), (48, 132, 9_999),
                                   (64, 556, 30_000)])
def test_narrow_weight_gradient_on_the_valu(ops, gpu_device, m, n, k):
    """lkg_gemm_smallm_f32 (dW = dY^T X for a dY of <= 64 columns: exact f32 FMAs over LDS-staged row tiles, slices of k
    combined by atomics) against f64, through ops.gemm(trans_a=True) -- contiguous operands and column slices of wider
    tables (a CatBuffer slot), row counts that are not whole tiles."""
    from literalkg_amd import _native as N
    torch.manual_seed(m * n)
    wide_a = torch.randn(k, m + 8, device=gpu_device)
    wide_b = torch.randn(k, n + 12, device=gpu_device)
    for a, b in ((wide_a[:, :m].contiguous(), wide_b[:, :n].contiguous()), (wide_a[:, 4:4 + m], wide_b[:, 8:8 + n])):
        assert N.load().lkg_gemm_smallm_ok(m, n, k, N.ptr(a), ops._ld(a), N.ptr(b), ops._ld(b))
        got = ops.gemm(a, b, trans_a=True).double()
        want = a.double().t() @ b.double()
        scale = a.double().abs().t() @ b.double().abs() + 1e-300
        ref32 = (a.t() @ b).double()
        e_got, e_f32 = float(((got - want).abs() / scale).max()), float(((ref32 - want).abs() / scale).max())
        assert e_got <= max(2 * e_f32, 3e-7), (e_got, e_f32)


@pytest.mark.parametrize("m,n,k", [(256, 256, 40_000), (512, 300, 33_333), (64, 2, 5000), (130, 257, 16 * 700 + 5)])
def test_weight_gradient_f16x2_engine_is_f32_accurate(ops, gpu_device, m, n, k):
    """lkg_gemm_wgrad_f32 (column-scaled exact fp16 hi/mid split, 3 MFMAs per product) against f64: within 3x of an f32
    GEMM's own error, also with columns 40 orders of magnitude apart, rows that are almost all zero, strided views."""
    torch.manual_seed(m + n)
    a = torch.randn(k, m + 4, device=gpu_device)[:, 2:2 + m]
    b = torch.randn(k, n, device=gpu_device)
    col_scale_a = torch.logspace(-20, 20, m, device=gpu_device)
    for variant in ("plain", "columns 1e-20 .. 1e20", "row-sparse"):
        aa, bb = a, b
        if variant != "plain":
            aa = a * col_scale_a
        if variant == "row-sparse":
            keep = torch.zeros(k, 1, device=gpu_device)
            keep[torch.randint(0, k, (k // 100,), device=gpu_device)] = 1
            aa = aa * keep
        got = ops.gemm_wgrad(aa, bb, ops.col_absmax(aa), ops.col_absmax(bb)).double()
        want = aa.double().t() @ bb.double()
        ref32 = (aa.t() @ bb).double()                      # hipBLASLt f32
        scale = aa.double().abs().t() @ bb.double().abs() + 1e-300          # componentwise error scale of a dot product
        e_got = float(((got - want).abs() / scale).max())
        e_f32 = float(((ref32 - want).abs() / scale).max())
        assert e_got <= max(3 * e_f32, 4e-7), (variant, e_got, e_f32)     # (the split products carry 2^-22)
    cm = ops.col_absmax(a)
    assert torch.equal(cm.cpu(), a.abs().amax(0).cpu())


@pytest.mark.parametrize("agg,residual,n_rows_paths", [("gcn", False, 2), ("graphsage", False, None), ("gcn", True, None),
                                                       ("bi-interaction", False, None)])
def test_gradient_frontier_two_layers_equals_the_dense_backward(L, ops, O, gpu_device, agg, residual, n_rows_paths):
    """Two aggregation layers under a loss on a few rows: the last layer's backward runs on those rows, the transpose SpMM
    hands the rows it reached (the frontier, flagged by the kernel) to the layer below, which runs on them as well.  All
    parameter gradients against the same model with the row-sparse machinery switched off."""
    from literalkg_amd.synth import make_batch, make_kg
    from literalkg_amd import io
    n, e, dim = 60_000, 240_000, 64
    h, t, r = make_kg(n, e, seed=11)
    cfg = O.default_cfg(embed_dim=dim, relation_dim=dim, conv_dim=dim, n_conv_layers=2, aggregation_type=agg,
                        use_residual=residual, kg_l2loss_lambda=1e-4, device=gpu_device)
    torch.manual_seed(1)
    m = L.LiteralKG(cfg, n, 16, io.initial_a_in(n, h, t, r), None, None, scoring="transr").to(gpu_device).eval()
    batch = [torch.from_numpy(x).to(gpu_device) for x in make_batch(n, 40, 3, seed=2)]
    seen = {}
    real = ops._MultiLinear._backward_on_rows

    def spy(ctx, gy, rows, xs, ws):
        seen[gy.shape[0], rows.n_max] = seen.get((gy.shape[0], rows.n_max), 0) + 1
        return real(ctx, gy, rows, xs, ws)

    def grads(sparse):
        m.zero_grad(set_to_none=True)
        m._table_grad_stays_inside = (lambda: m.gat_rows is None) if sparse else (lambda: False)
        m(*batch, device=gpu_device, mode="pre_training").backward()
        return {k: v.grad.clone() for k, v in m.named_parameters() if v.grad is not None}

    ops._MultiLinear._backward_on_rows = staticmethod(spy)
    try:
        got = grads(True)
    finally:
        ops._MultiLinear._backward_on_rows = staticmethod(real)
    want = grads(False)
    del m._table_grad_stays_inside
    if n_rows_paths is not None:                # both layers' Linears took the rows path: 120 + 2 * 40 ids, then the frontier
        assert len({k[1] for k in seen}) == n_rows_paths, seen
    assert got.keys() == want.keys()
    for k in want:
        scale = float(want[k].abs().max()) + 1e-30
        assert float((got[k] - want[k]).abs().max()) <= 5e-5 * scale, k
    ops._RowScratch._tables.clear()


@pytest.mark.parametrize("variant", ["dropout_train", "gin", "scale_gat_dim", "gatemul_3layers", "transe", "fine_tuning",
                                     "sage_res_dropout", "gatenum_scale_dropout", "mlp_head", "one_layer_gate_narrow",
                                     "one_layer_gate_wide", "narrow_two_layers"])
def test_row_sparse_machinery_across_model_variants(L, ops, O, gpu_device, variant):
    """The row-sparse backward (kept-zero tables, row sets, gradient frontier, Linear backward on listed rows) is active
    from 16 384 entity rows on -- sizes the reference-fixture tests do not reach.  Here every model family runs at 40 k
    rows against ITSELF with the machinery off (zeros_like table, no row sets): training-mode dropout (the masks are
    regenerated from the step's seed in the sparse backward too), gin's stacked sums, linear_gat, the gates, three
    layers, the TransE form and the fine-tuning head."""
    from literalkg_amd.synth import make_batch, make_kg
    from literalkg_amd import io
    n, e, dim = 40_000, 240_000, 64
    h, t, r = make_kg(n, e, seed=13)
    over = dict(embed_dim=dim, relation_dim=dim, conv_dim=dim, n_conv_layers=2, aggregation_type="gcn",
                kg_l2loss_lambda=1e-4, fine_tuning_l2loss_lambda=1e-4, device=gpu_device)
    scoring, mode, train = "transr", "pre_training", False
    if variant == "dropout_train":
        over.update(mess_dropout=0.3); train = True
    elif variant == "gin":
        over.update(aggregation_type="gin", mlp_hidden_dim=48)
    elif variant == "scale_gat_dim":
        over.update(scale_gat_dim=96)
    elif variant == "gatemul_3layers":
        over.update(n_conv_layers=3, use_num_lit=True, use_txt_lit=True, txt_lit_dim=40)
    elif variant == "transe":
        over.update(relation_dim=dim * 3); scoring = "transe"
    elif variant == "fine_tuning":
        mode = "fine_tuning"
    elif variant == "sage_res_dropout":
        over.update(aggregation_type="graphsage", use_residual=True, mess_dropout=0.2); train = True
    elif variant == "gatenum_scale_dropout":
        over.update(use_num_lit=True, scale_gat_dim=80, mess_dropout=0.1); train = True
    elif variant == "mlp_head":
        over.update(scale_gat_dim=48); mode = "mlp"
    elif variant == "one_layer_gate_narrow":
        # argument_finetuning.py's shape: ONE narrowing gcn layer behind GateMul, linear_gat on top, the fine-tuning head --
        # the 32-wide transpose SpMM follows the gradient's frontier, the gate's two consumers are joined row-sparsely
        # (ops.fanout) and the gate's backward runs on the listed rows
        over.update(n_conv_layers=1, conv_dim=32, use_num_lit=True, use_txt_lit=True, txt_lit_dim=40, scale_gat_dim=64)
        mode = "fine_tuning"
    elif variant == "one_layer_gate_wide":
        over.update(n_conv_layers=1, use_num_lit=True, use_txt_lit=True, txt_lit_dim=40)       # (the SpMM that also keeps slot 0)
    elif variant == "narrow_two_layers":
        over.update(conv_dim=32)                      # 64 -> 32 -> 32: the frontier through 32-wide tables
    cfg = O.default_cfg(**over)
    torch.manual_seed(5)
    num = torch.rand(n, 2) if cfg.use_num_lit else None
    txt = torch.randn(n, cfg.txt_lit_dim) if cfg.use_txt_lit else None
    m = L.LiteralKG(cfg, n, 16, io.initial_a_in(n, h, t, r), num, txt, scoring=scoring).to(gpu_device)
    if mode == "mlp":
        torch.manual_seed(6)
        m.initialize_MLP()
    m.train(train)
    bh, br, bp, bn = (torch.from_numpy(x).to(gpu_device) for x in make_batch(n, 60, 3, seed=3))
    args = (bh, br, bp, bn) if mode == "pre_training" else ((bh, bp) if mode == "mlp" else (bh, bp, bn))
    weights = torch.linspace(-1.0, 1.0, bh.numel(), device=gpu_device).reshape(-1, 1)
    ops._RowScratch._tables.clear()

    def grads(sparse):
        m.zero_grad(set_to_none=True)
        m._table_grad_stays_inside = (lambda: m.gat_rows is None) if sparse else (lambda: False)
        out = []
        for step in range(2):                       # two steps: the second re-uses the kept-zero tables of the first
            torch.manual_seed(100 + step)           # the dropout seeds follow torch's CPU generator
            loss = m(*args, device=gpu_device, mode=mode)
            if mode == "mlp":                       # (B x 1 sigmoid outputs: a weighted sum stands in for the driver's BCE)
                loss = (loss * weights).sum()
            loss.backward()
            out.append(float(loss.detach()))
        return out, {k: v.grad.clone() for k, v in m.named_parameters() if v.grad is not None}

    try:
        l1, got = grads(True)
        pools = {k[3] for k in ops._RowScratch._tables}
        l0, want = grads(False)
    finally:
        del m._table_grad_stays_inside
        ops._RowScratch._tables.clear()
    if variant == "one_layer_gate_narrow":
        assert {"g_agg", "g_fanout", "g_gate_x"} <= pools, pools
    elif variant == "one_layer_gate_wide":
        assert {"g_agg_keep", "g_gate_x"} <= pools, pools
    elif variant == "narrow_two_layers":
        assert "g_agg" in pools, pools
    assert l1 == l0 and all(np.isfinite(l1)), (l1, l0)
    assert got.keys() == want.keys() and len(want) >= 4
    for k in want:
        scale = float(want[k].abs().max()) + 1e-30
        assert float((got[k] - want[k]).abs().max()) <= 5e-5 * scale, k


@pytest.mark.parametrize("d,n_w", [(64, 2), (256, 0), (100, 1), (512, 4)])
def test_gate_backward_statistics_ride_along(ops, gpu_device, d, n_w):
    """lkg_gate_blend_bwd_stats_f32: the same three outputs as lkg_gate_blend_bwd_f32, and its column statistics (bias
    sums, column maxima of [g_gpre | g_zpre] and of x, the narrow panel's weight gradient) against torch in f64."""
    from literalkg_amd import _native as N
    torch.manual_seed(d)
    n = 7001
    x, gt, zs, go = (torch.randn(n, d, device=gpu_device) for _ in range(4))
    gt, zs = torch.tanh(gt), torch.sigmoid(zs)
    w = torch.rand(n, max(n_w, 1), device=gpu_device)
    outs = []
    for stats_mode in (False, True):
        gx = torch.empty(n, d, device=gpu_device)
        gpz = torch.empty(n, 2 * d, device=gpu_device)
        rm = torch.empty(n, device=gpu_device)
        if stats_mode:
            n_stats = (5 + 2 * n_w) * d
            ws = torch.empty(1024 * n_stats, device=gpu_device)
            st = torch.empty(n_stats, device=gpu_device)
            N.call("lkg_gate_blend_bwd_stats_f32", n, d, N.ptr(x), d, N.ptr(gt), d, N.ptr(zs), d, N.ptr(go), d, N.ptr(gx), d,
                   N.ptr(gpz), 2 * d, gpz.data_ptr() + 4 * d, 2 * d, 1, N.ptr(rm), N.ptr(w) if n_w else None, w.shape[1], n_w,
                   N.ptr(ws), ws.numel(), N.ptr(st), None)
        else:
            N.call("lkg_gate_blend_bwd_f32", n, d, N.ptr(x), d, N.ptr(gt), d, N.ptr(zs), d, N.ptr(go), d, N.ptr(gx), d,
                   N.ptr(gpz), 2 * d, gpz.data_ptr() + 4 * d, 2 * d, 1, N.ptr(rm), None)
        outs.append((gx, gpz, rm))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    gpz64 = outs[0][1].double()
    tol = lambda ref: 2e-6 * float(ref.abs().max()) + 1e-30
    assert float((st[:2 * d].double() - gpz64.sum(0)).abs().max()) <= 2e-6 * float(gpz64.abs().sum(0).max())
    assert torch.equal(st[2 * d:4 * d], outs[0][1].abs().amax(0))
    assert torch.equal(st[4 * d:5 * d], x.abs().amax(0))
    if n_w:
        want = (gpz64.t() @ w[:, :n_w].double())                       # [2d x n_w]
        got = st[5 * d:].view(n_w, 2 * d).t().double()
        assert float((got - want).abs().max()) <= 2e-6 * float((gpz64.abs().t() @ w[:, :n_w].double()).max())


def test_deferred_slot0_copy_is_made_on_demand(L, ops, O, gpu_device):
    """pre_training with TransR and no gate: the copy of the raw entity table into slot 0 of the concatenated table is not
    made by the step; `model.gat_embed` completes the table on first access -- also between forward and backward -- and
    the module's parameter / state_dict surface is untouched."""
    from literalkg_amd.synth import make_batch, make_kg
    from literalkg_amd import io
    n, dim = 30_000, 64
    h, t, r = make_kg(n, 120_000, seed=3)
    cfg = O.default_cfg(embed_dim=dim, relation_dim=dim, conv_dim=dim, n_conv_layers=1, aggregation_type="gcn",
                        kg_l2loss_lambda=1e-4, device=gpu_device)
    torch.manual_seed(2)
    m = L.LiteralKG(cfg, n, 16, io.initial_a_in(n, h, t, r), None, None, scoring="transr").to(gpu_device).eval()
    keys = set(m.state_dict().keys())
    n_params = len(list(m.parameters()))
    batch = [torch.from_numpy(x).to(gpu_device) for x in make_batch(n, 50, 3, seed=4)]
    loss = m(*batch, device=gpu_device, mode="pre_training")
    table, raw = m._gat_state
    assert raw is not None                                      # pending: the step did not copy
    ops.fill_slot(table, 0, torch.full((n, dim), float("nan"), device=gpu_device))   # whatever was there must not matter
    got = m.gat_embed                                           # ... completes the table
    assert m._gat_state[1] is None and torch.equal(got[:, :dim].detach(), m.entity_embed.weight.detach())
    loss.backward()                                             # (no version-counter complaint: the fill is a library kernel)
    g_sparse = {k: v.grad.clone() for k, v in m.named_parameters() if v.grad is not None}
    assert set(m.state_dict().keys()) == keys and len(list(m.parameters())) == n_params
    # the same step with the copy made by the SpMM epilogue (the other losses' path)
    m.zero_grad(set_to_none=True)
    full = m.gat_embeddings()
    loss2 = ops.transr_loss(full, m.relation_embed.weight, m.gat_trans_M, *batch, m.kg_l2loss_lambda)
    loss2.backward()
    assert abs(float(loss) - float(loss2)) <= 1e-6 * abs(float(loss2))
    assert torch.equal(full.detach(), got.detach())
    for k, v in m.named_parameters():
        if v.grad is not None:
            assert float((v.grad - g_sparse[k]).abs().max()) <= 5e-5 * (float(v.grad.abs().max()) + 1e-30), k


# ----------------------------------------------------------------------------- degenerate but legal shapes
@pytest.mark.parametrize("agg", ["gcn", "graphsage", "bi-interaction", "gin"])
@pytest.mark.parametrize("prune", [False, True])
def test_degenerate_shapes_against_the_oracle(L, O, gpu_device, agg, prune):
    """Shapes the reference's code tolerates and a randomised sweep rarely draws: a graph of ONE entity with a self-loop, a
    batch whose ids are all the same entity, a refresh over relations that match no triple (the matrix becomes empty and every
    aggregation returns zero rows) followed by the losses on that empty matrix -- full-graph and pruned."""
    from literalkg_amd import io
    torch.manual_seed(3)
    # ---- one entity, one self-loop
    cfg = O.default_cfg(embed_dim=8, relation_dim=8, conv_dim=8, n_conv_layers=2, aggregation_type=agg, mlp_hidden_dim=8,
                        device=gpu_device)
    one = np.zeros(1, np.int64)
    a_in = io.initial_a_in(1, one, one, one)
    m = L.LiteralKG(cfg, 1, 1, a_in)
    params = {k: v.detach().clone() for k, v in m.state_dict().items() if k != "A_in"}
    m.to(gpu_device).eval()
    m.prune_to_batch = prune
    z = torch.zeros(2, dtype=torch.long)
    loss = m(*[z.to(gpu_device)] * 4, device=gpu_device, mode="pre_training")
    p = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in params.items()}
    want = O.pre_training_loss(p, cfg, a_in, z, z, z, z)
    np.testing.assert_allclose(float(loss.detach()), float(want.detach()), rtol=1e-5)
    loss.backward()
    want.backward()
    for k, v in m.named_parameters():
        if v.grad is not None and k != "A_in":
            torch.testing.assert_close(v.grad.cpu(), p[k].grad, rtol=1e-3, atol=1e-6, msg=k)

    # ---- 50 entities; every batch id the same entity; then a refresh over a relation nobody uses
    n, dim = 50, 12
    rng = np.random.default_rng(1)
    h, t, r = rng.integers(0, n, 200), rng.integers(0, n, 200), rng.integers(0, 2, 200)           # relations 0 and 1 of 4
    trip = np.unique(np.stack([h, r, t], 1), axis=0)
    h, r, t = trip[:, 0].copy(), trip[:, 1].copy(), trip[:, 2].copy()
    cfg = O.default_cfg(embed_dim=dim, relation_dim=dim, conv_dim=dim, n_conv_layers=2, aggregation_type=agg, mlp_hidden_dim=8,
                        use_num_lit=True, scale_gat_dim=10, device=gpu_device)
    num = torch.rand(n, 2)
    a_in = io.initial_a_in(n, h, t, r)
    m = L.LiteralKG(cfg, n, 4, a_in, num, None)
    params = {k: v.detach().clone() for k, v in m.state_dict().items() if k != "A_in"}
    m.to(gpu_device).eval()
    m.prune_to_batch = prune
    same = torch.full((6,), 7, dtype=torch.long)
    rel = torch.zeros(6, dtype=torch.long)

    def both(a_ref):
        out = []
        for mode, args, ref in (("pre_training", (same, rel, same, same), lambda q: O.pre_training_loss(q, cfg, a_ref, same, rel, same, same, num=num)),
                                ("fine_tuning", (same, same, same), lambda q: O.prediction_loss(cfg, O.gat_embeddings(q, cfg, a_ref, num, None), same, same, same))):
            m.zero_grad(set_to_none=True)
            got = m(*[x.to(gpu_device) for x in args], device=gpu_device, mode=mode)
            got.backward()
            q = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in params.items()}
            want_ = ref(q)
            want_.backward()
            np.testing.assert_allclose(float(got.detach()), float(want_.detach()), rtol=1e-5, err_msg=mode)
            for k, v in m.named_parameters():
                if v.grad is not None and k != "A_in" and q[k].grad is not None:
                    torch.testing.assert_close(v.grad.cpu(), q[k].grad, rtol=2e-3, atol=1e-6, msg=f"{mode} {k}")
            out.append(float(got.detach()))
        return out
    both(a_in)
    dev = lambda x: torch.from_numpy(x).to(gpu_device)
    m(dev(h), dev(t), dev(r), [3], device=gpu_device, mode="update_att")                         # relation 3: no triple
    empty = m.A_in.data.cpu().coalesce()
    assert empty._nnz() == 0 and tuple(empty.shape) == (n, n)
    both(torch.sparse_coo_tensor(torch.zeros((2, 0), dtype=torch.long), torch.zeros(0), (n, n)).coalesce())
    with torch.no_grad():
        s = m.calc_score(same[:2].to(gpu_device), torch.arange(5, device=gpu_device))
    gat = O.gat_embeddings(params, cfg, torch.sparse_coo_tensor(torch.zeros((2, 0), dtype=torch.long), torch.zeros(0), (n, n)).coalesce(), num, None)
    torch.testing.assert_close(s.cpu(), O.link_scores(gat, same[:2], torch.arange(5)), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("layers,dim,residual", [(0, 6, False), (1, 2, False), (2, 3, True), (1, 5, True)])
def test_degenerate_architectures_against_the_oracle(L, O, gpu_device, layers, dim, residual):
    """No aggregation layer at all (the encoder is the gate's output alone), two- and three-wide embeddings, a single residual
    layer (no stacked h0 projection): loss and gradients against the oracle, full-graph and pruned.  (One-wide embeddings are
    left out: LayerNorm over one element returns its bias, zero at initialisation, F.normalize divides that by its 1e-12
    clamp, and the reference's gradients become 1e12 x rounding dust -- 3.6e5 where exact arithmetic, and this package, give 0.)"""
    from literalkg_amd import io
    from literalkg_amd.synth import make_batch
    n = 60
    rng = np.random.default_rng(layers * 10 + dim)
    trip = np.unique(np.stack([rng.integers(0, n, 300), rng.integers(0, 3, 300), rng.integers(0, n, 300)], 1), axis=0)
    h, r, t = trip[:, 0].copy(), trip[:, 1].copy(), trip[:, 2].copy()
    cfg = O.default_cfg(embed_dim=dim, relation_dim=dim, conv_dim=dim, n_conv_layers=layers, aggregation_type="gcn",
                        use_residual=residual, use_txt_lit=True, txt_lit_dim=3, device=gpu_device)
    torch.manual_seed(layers + dim)
    txt = torch.randn(n, 3)
    a_in = io.initial_a_in(n, h, t, r)
    m = L.LiteralKG(cfg, n, 3, a_in, None, txt)
    params = {k: v.detach().clone() for k, v in m.state_dict().items() if k != "A_in"}
    m.to(gpu_device).eval()
    bh, br, bp, bn = (torch.from_numpy(x) for x in make_batch(n, 9, 2, seed=3))
    br = br % 3
    for prune in (False, True):
        m.prune_to_batch = prune
        m.zero_grad(set_to_none=True)
        loss = m(*[x.to(gpu_device) for x in (bh, br, bp, bn)], device=gpu_device, mode="pre_training")
        loss.backward()
        p = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in params.items()}
        want = O.pre_training_loss(p, cfg, a_in, bh, br, bp, bn, txt=txt)
        want.backward()
        np.testing.assert_allclose(float(loss.detach()), float(want.detach()), rtol=1e-5)
        for k, v in m.named_parameters():
            if v.grad is not None and k != "A_in" and p[k].grad is not None:
                torch.testing.assert_close(v.grad.cpu(), p[k].grad, rtol=2e-3, atol=1e-6,
                                           msg=lambda s_: f"prune={prune} {k}: {s_} got {v.grad.cpu().flatten()[:4]} want {p[k].grad.flatten()[:4]}")


# ----------------------------------------------------------------------------- a longer trajectory than the fixtures hold
@pytest.mark.parametrize("agg,gate,scoring", [("gcn", "mul", "transr"), ("graphsage", None, "transe"), ("bi-interaction", "num", "transr")])
def test_forty_step_trajectory_with_the_fused_adam_follows_the_oracle(L, O, gpu_device, agg, gate, scoring):
    """Forty pre-training steps the way main_pretraining.py:86-139 runs them -- the package's fused Adam, update_att every ten
    steps, a prediction between steps (the inference heads' kept table must follow every update) -- against the oracle under
    torch.optim.Adam on the CPU: every loss to 2e-3, the scores of the first ten steps and the first refresh's attention values
    to 1e-3; the kept inference table equals a recomputation bit for bit at every prediction."""
    from literalkg_amd import io
    from literalkg_amd.optim import Adam
    from literalkg_amd.synth import make_batch
    n, dim, n_rel = 1500, 32, 5
    rng = np.random.default_rng(11)
    trip = np.unique(np.stack([rng.integers(0, n, 9000), rng.integers(0, n_rel, 9000), rng.integers(0, n, 9000)], 1), axis=0)
    h, r, t = trip[:, 0].copy(), trip[:, 1].copy(), trip[:, 2].copy()
    cfg = O.default_cfg(embed_dim=dim, relation_dim=dim if scoring == "transr" else 24, conv_dim=dim, n_conv_layers=2,
                        aggregation_type=agg, scale_gat_dim=24, use_num_lit=gate in ("mul", "num"), use_txt_lit=gate == "mul",
                        txt_lit_dim=12, kg_l2loss_lambda=1e-4, device=gpu_device)
    torch.manual_seed(9)
    num = torch.rand(n, 2) if cfg.use_num_lit else None
    txt = torch.randn(n, 12) if cfg.use_txt_lit else None
    a_in = io.initial_a_in(n, h, t, r)
    m = L.LiteralKG(cfg, n, n_rel, a_in, num, txt, scoring=scoring)
    p = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in m.state_dict().items() if k != "A_in"}
    m.to(gpu_device).train()
    lr = 2e-3
    opt = Adam([q for q in m.parameters() if not q.is_sparse], lr=lr)
    names = [k for k, v in m.named_parameters() if k != "A_in"]
    ref_opt = torch.optim.Adam([p[k] for k in names], lr=lr)
    hd, td, rd = (torch.from_numpy(x).to(gpu_device) for x in (h, t, r))
    a_ref = a_in
    heads, tails = torch.arange(0, 40), torch.arange(100, 160)
    for step in range(40):
        bh, br, bp, bn = (torch.from_numpy(x) for x in make_batch(n, 64, 3, seed=100 + step))
        br = br % n_rel
        opt.zero_grad(set_to_none=True)
        loss = m(*[x.to(gpu_device) for x in (bh, br, bp, bn)], device=gpu_device, mode="pre_training")
        loss.backward()
        opt.step()
        ref_opt.zero_grad(set_to_none=True)
        want = O.pre_training_loss(p, cfg, a_ref, bh, br, bp, bn, num=num, txt=txt, form=scoring)
        want.backward()
        ref_opt.step()
        np.testing.assert_allclose(float(loss.detach()), float(want.detach()), rtol=2e-3, err_msg=f"step {step}")
        if step % 10 == 9 and cfg.relation_dim == cfg.embed_dim:
            m(hd, td, rd, list(range(n_rel)), device=gpu_device, mode="update_att")
            with torch.no_grad():
                a_ref = O.attention_refresh(n, p["entity_embed.weight"].detach(), p["relation_embed.weight"].detach(),
                                            torch.from_numpy(h), torch.from_numpy(t), torch.from_numpy(r)).coalesce()
            got_a = m.A_in.data.cpu().coalesce()
            assert torch.equal(got_a.indices(), a_ref.indices())
            if step == 9:                        # (later refreshes sit on embeddings that have drifted: see the scores below)
                torch.testing.assert_close(got_a.values(), a_ref.values(), rtol=1e-3, atol=1e-6)
            assert bool(torch.isfinite(got_a.values()).all())
        if step % 7 == 3:                        # a prediction between steps: eval mode, no_grad, the kept table
            m.eval()
            with torch.no_grad():
                s = m.calc_score(heads.to(gpu_device), tails.to(gpu_device)).cpu()
                gat = O.gat_embeddings({k: v.detach() for k, v in p.items()}, cfg, a_ref, num, txt)
                fresh = m.gat_embeddings()       # (the kept table against a recomputation: equal bit for bit, whatever the drift)
                s_fresh = ops_gemm_rows(fresh, heads.to(gpu_device), tails.to(gpu_device)).cpu()
            assert torch.equal(s, s_fresh), f"the inference heads' kept table is stale after step {step}"
            # Against the oracle the scores are compared over the first ten steps only: Adam divides by the root of its second
            # moment, so where a gradient entry is rounding noise the parameter still moves by ~lr per step in a direction the
            # noise picks, and ANY two fp32 trajectories part ways -- the oracle in fp32 against itself in float64 on this very
            # setup: scores 1e-6 apart at step 10, 3e-4 at 17, 1.4e-2 at 24, 4e-2 at 31 (bi-interaction), the losses within 1e-3
            # all the way.
            if step <= 10:
                ref_s = O.link_scores(gat, heads, tails)
                assert float((s - ref_s).abs().max()) <= 1e-3 * (float(ref_s.abs().max()) + 1e-30), f"scores after step {step}"
            m.train()
    assert all(bool(torch.isfinite(v).all()) for k, v in m.state_dict().items() if k != "A_in" and v.is_floating_point())


def ops_gemm_rows(table, head_ids, tail_ids):
    """table[head_ids] @ table[tail_ids]^T on the library's ops (what calc_score computes from its table)"""
    from literalkg_amd import ops
    return ops.gemm(ops.gather_rows(table, head_ids), ops.gather_rows(table, tail_ids), trans_b=True)
