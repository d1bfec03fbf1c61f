"""The kernels that move rows and ids around, the batch sampler and Adam, each driven through its C entry point and held to
an exact reference (index_cases.py holds the references, draws and checks -- the same ones test_index_measures_host.py shows
to tell a wrong implementation from a right one on the CPU).  Integer and copied outputs are compared bit for bit, every
destination has a sentinel guard beside and behind it, the two atomics kernels and Adam are measured per element against
float64.

Which case enters which dispatch branch (from the entry points' dispatch code):

  lkg_group_by_key_i64 (one workgroup of 16 waves, each wave a chunk of ceil(n / 16) rounded up to 64 elements;
  4 (16 n_keys + 1) bytes of dynamic LDS)
    no element / fewer than 16 waves      n = 0, 1, 63, 64, 65 (one wave has work), 1023 / 1024 (16 chunks of 64), 1025 (9 of 128)
    partial last ballot                   n % 64 != 0: 1, 63, 65, 1023, 1025, 3089, 70 001
    every wave busy, several ballots      n = 16 * 64 * 3 + 17 (chunks of 256), 70 001 (chunks of 4416)
    counters across waves                 draw "wave chunks": the same <= 5 keys in every wave's chunk
    LDS 65 540 bytes (over 64 KiB)        n_keys = 1024; 65 476 bytes at 1023
    n_bad given / NULL                    test_group_by_key / test_group_by_key_through_ops
  lkg_expand_groups_i32 (grid over max(n_groups k, n_seg))
    n_groups k > n_seg | < n_seg          (37, 7, 4), (1000, 64, 17), (1, 1, 2) | (0, 3, 5), (5, 2, 300)
  lkg_gather_i64 / lkg_permute_f32 / lkg_csr_check_i32 (grid-stride, 2048 blocks of 256 = 524 288 threads)
    one trip | a second trip              n = 1, 255, 257 | 524 288 + 77 (nnz = 524 288 + 77 for the CSR check)
  lkg_check_grouped_i64 / lkg_sanitize_ids_i64 (one ballot per wave, one atomic per wave with a fault)
    no launch                             n = 0 (the counter is still reset)
    partial wave / block                  n = 1, 65, 257, 5000; full: 64, 256
  lkg_gather_rows_f32 (float4 kernel when d % 4 == 0, lds % 4 == 0, ldd % 4 == 0 and both bases 16-byte aligned)
    float4                                d = 4, 64, 68, 260, 300 with the views "contiguous" and "four floats in"
    scalar: d % 4 != 0                    d = 1, 3 (every view)
    scalar: base not aligned              view "one float in" (ld = d + 3)
    scalar: ld % 4 != 0, base aligned     view "odd ld" (ld = d + 5)
    more than one pass over the columns   d = 260, 300 (float4: 65, 75 chunks for 64 lanes), d = 68 .. 300 (scalar)
    idx / perm NULL or given              forms idx, perm, both, neither
  lkg_gather_rows_range_f32 / lkg_fill_rows_f32 / lkg_scatter_add_rows_f32 / lkg_csr_extract_rows /
  lkg_spmm_csr_scatter_bwd_f32            one kernel each (a wave per row, 64 columns or entries per pass): widths and row
                                          lengths below, at and above 64
  lkg_sample_kg_batch
    eptr NULL | given                     cases "no dups", "bad heads" | "dups", "full head"
    sentinel group                        "bad heads": an entity without triples, n_entities, -1, 2^40
    accept after 256 rejections           "full head"
  lkg_adam_step_f32 (float4 body + scalar tail, 4096 blocks of 256)
    tail only | body only | both          n = 1, 3 | 4 | 7, 1027
    second trip of the stride loop        n = 4 * 256 * 4096 + 4 * 300 + 3 (body: 1 048 876 float4 > 1 048 576 threads; tail 3)"""
import numpy as np
import pytest
import torch

import index_cases as I
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


@pytest.fixture(scope="module")
def dev(gpu_device):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)


def host(t):
    return t.cpu().numpy()


def ibuf(device, n, dtype=torch.int32):
    return torch.full((n + I.PAD,), I.ISENT, dtype=dtype, device=device)


def fbuf(device, *shape):
    return torch.full(shape, I.SENTINEL, device=device)


# =============================================================================================== group by key
def run_group_by_key(ops, N, dev, keys, n_keys, counter=True):
    kd = dev(keys)
    perm, seg = ibuf(kd.device, keys.shape[0]), ibuf(kd.device, n_keys + 1)
    bad = torch.full((1 + I.PAD,), I.ISENT, dtype=torch.int32, device=kd.device)
    N.call("lkg_group_by_key_i64", keys.shape[0], n_keys, N.ptr(kd), N.ptr(perm), N.ptr(seg), N.ptr(bad) if counter else None,
           ops._stream())
    bad = host(bad)
    assert (bad[1:] == I.ISENT).all()
    return host(perm), host(seg), int(bad[0])


@pytest.mark.parametrize("n_keys", I.GB_KEYS)
@pytest.mark.parametrize("n", I.GB_N)
def test_group_by_key(ops, N, dev, n, n_keys):
    """perm and seg against numpy's stable argsort and searchsorted, every key draw; n_bad = 0."""
    for draw in I.GB_DRAWS:
        keys = I.draw_keys(n, n_keys, draw)
        perm, seg, bad = run_group_by_key(ops, N, dev, keys, n_keys)
        I.check_group_by_key(f"n {n} n_keys {n_keys} {draw}", keys, n_keys, perm, seg, bad)


@pytest.mark.parametrize("n_keys", I.GB_KEYS)
def test_group_by_key_counts_keys_outside_the_range(ops, N, dev, n_keys):
    """keys of -1, n_keys and 2^40 planted: the exact count, perm still a permutation, seg non-decreasing up to n."""
    for n in (3, 65, 1025, 70_001):
        keys = I.draw_keys(n, n_keys, "uniform")
        keys[[0, n // 2, n - 1]] = [-1, n_keys, 2 ** 40]
        perm, seg, bad = run_group_by_key(ops, N, dev, keys, n_keys)
        I.check_group_by_key_bad(f"n {n} n_keys {n_keys}", keys, n_keys, perm, seg, bad)
        I.check_group_by_key(f"n {n} n_keys {n_keys}", keys, n_keys, perm, seg, bad)     # (grouped with the nearest valid key)


@pytest.mark.parametrize("n_keys", [1, 100, 1024])
def test_group_by_key_through_ops(ops, dev, n_keys):
    """ops.group_by_key: the same launch with n_bad = NULL."""
    for n in (0, 65, 3089):
        keys = I.draw_keys(n, n_keys, "uniform")
        perm, seg = ops.group_by_key(dev(keys), n_keys)
        want_p, want_s, _ = I.group_by_key_ref(keys, n_keys)
        assert np.array_equal(host(perm), want_p) and np.array_equal(host(seg), want_s)


# =============================================================================================== small integer kernels
@pytest.mark.parametrize("n_groups,k,n_seg", I.EXPAND_CASES)
def test_expand_groups(ops, N, dev, gpu_device, n_groups, k, n_seg):
    perm, seg = I.draw_expand(n_groups, k, n_seg)
    po, so = ibuf(gpu_device, n_groups * k), ibuf(gpu_device, n_seg)
    pd, sd = dev(perm), dev(seg)                                    # (held until the call: a freed operand's memory is reused)
    N.call("lkg_expand_groups_i32", n_groups, k, n_seg, N.ptr(pd) if n_groups else None, N.ptr(sd),
           N.ptr(po), N.ptr(so), ops._stream())
    I.check_expand(f"expand {n_groups} x {k}, {n_seg}", perm, seg, k, host(po), host(so))


@pytest.mark.parametrize("n", I.STRIDE_N)
def test_gather_i64_and_permute(ops, N, dev, gpu_device, n):
    """dst[i] = src[perm[i]] over one trip and two trips of the stride loop; the float form stores NaN for an index outside
    the source (-1, n_src, INT32_MAX) and the source's bits elsewhere."""
    rng = np.random.default_rng(n)
    src = rng.integers(-2 ** 62, 2 ** 62, n + 3, dtype=np.int64)
    perm = rng.integers(0, n + 3, n).astype(np.int32)
    perm[-1] = n + 2
    dst = ibuf(gpu_device, n, torch.int64)
    sd, pd = dev(src), dev(perm)
    N.call("lkg_gather_i64", n, N.ptr(sd), N.ptr(pd), N.ptr(dst), ops._stream())
    I.check_gather_i64(f"gather_i64 n {n}", src, perm, host(dst))
    perm, n_src, srcf, planted = I.draw_permute(n)
    assert len(planted) == (1 if n == 1 else 3)
    out = fbuf(gpu_device, n + I.PAD)
    pd, sd = dev(perm), dev(srcf)
    N.call("lkg_permute_f32", n, N.ptr(pd), n_src, N.ptr(sd), N.ptr(out), ops._stream())
    I.check_permute(f"permute n {n}", perm, n_src, srcf, host(out))


@pytest.mark.parametrize("fault", I.FAULTS)
@pytest.mark.parametrize("n", I.COUNT_N)
def test_check_grouped(ops, N, dev, gpu_device, n, fault):
    """the exact count of rows that differ from their group's first row; a second call on the same counter does not add."""
    counter = ibuf(gpu_device, 1)
    for k in (1, 2, 7):
        for field in ("h", "r", "pos_t"):
            h, r, p = I.draw_grouped_batch(n, k, fault, field)
            want = I.check_grouped_ref(h, r, p, k)
            hd, rd, pd = dev(h), dev(r), dev(p)
            for _ in range(2):
                N.call("lkg_check_grouped_i64", n, k, N.ptr(hd), N.ptr(rd), N.ptr(pd), N.ptr(counter), ops._stream())
                got = host(counter)
                assert int(got[0]) == want and (got[1:] == I.ISENT).all(), (n, k, field, fault, got[:2].tolist(), want)


@pytest.mark.parametrize("fault", I.FAULTS)
@pytest.mark.parametrize("n", I.COUNT_N)
def test_sanitize_ids(ops, N, dev, gpu_device, n, fault):
    """out = where(bad, lo, ids) with lo != 0 and the exact count; a second call on the same counter does not add."""
    counter = ibuf(gpu_device, 1)
    for lo, hi in ((3, 50), (-5, 1)):
        ids = I.draw_ids(n, lo, hi, fault)
        idd = dev(ids)
        for _ in range(2):
            out = ibuf(gpu_device, n, torch.int64)
            N.call("lkg_sanitize_ids_i64", n, N.ptr(idd), lo, hi, N.ptr(out), N.ptr(counter), ops._stream())
            got = host(counter)
            assert (got[1:] == I.ISENT).all()
            I.check_sanitize(f"sanitize n {n} [{lo}, {hi}) {fault}", ids, lo, hi, host(out), got[0])


# =============================================================================================== row gathers and fills
@pytest.mark.parametrize("d", I.GATHER_D)
def test_gather_rows(ops, N, dev, gpu_device, d):
    """dst[i] = src[idx[perm[i]]] bit for bit, idx / perm given or NULL, on every operand view (see the table above for the
    kernel each takes); the columns beside d and the rows behind n keep the sentinel."""
    for view in I.GATHER_VIEWS:
        for form in I.GATHER_FORMS:
            for n in I.GATHER_N:
                case = I.draw_gather(n, d, form, view)
                src, dst = dev(case.table), fbuf(gpu_device, n + I.PAD, case.ld)
                s, o = src[:, case.c0:], dst[:, case.c0:]
                vec = d % 4 == 0 and case.ld % 4 == 0 and s.data_ptr() % 16 == 0 and o.data_ptr() % 16 == 0
                assert vec == I.gather_vec(d, view), case.what
                idx = dev(case.idx) if case.idx is not None else None
                perm = dev(case.perm) if case.perm is not None else None
                N.call("lkg_gather_rows_f32", n, d, N.ptr(s), case.ld, N.ptr(idx), N.ptr(perm), N.ptr(o), case.ld, ops._stream())
                I.check_gather_rows(case, host(dst))


@pytest.mark.parametrize("d", [1, 5, 64, 300])
def test_gather_rows_range(ops, N, dev, gpu_device, d):
    """this rank's rows [lo, hi) of a table (src points at row lo): ids below, inside and above the range and -1; rows
    outside come out as exact +0.0; the empty range takes src = NULL."""
    n_table, c0 = 30, 1
    for n in (3, 6, 1027):
        for lo, hi in ((0, n_table), (7, 19), (7, 7)):
            table, ids = I.draw_gather_range(n, d, lo, hi, n_table)
            td, idd, dst = dev(table), dev(ids), fbuf(gpu_device, n + I.PAD, d + 3)
            src = N.ptr(td[lo:, c0:]) if hi > lo else None
            N.call("lkg_gather_rows_range_f32", n, d, src, d + 3, N.ptr(idd), lo, hi, N.ptr(dst[:, c0:]), d + 3,
                   ops._stream())
            I.check_gather_range(f"gather range n {n} d {d} [{lo}, {hi})", table, c0, d, ids, lo, hi, host(dst))


@pytest.mark.parametrize("d", I.FILL_D)
def test_fill_rows(ops, N, dev, gpu_device, d):
    """ids with duplicates and -1 padding; dst and flags, dst only, flags only with d = 0, flag 0 after flag 1."""
    n_rows, c0, value = 50, 2, 2.5
    for n in (1, 4, 60, 1027):
        ids = I.draw_fill_ids(n_rows, n)
        idd = dev(ids)
        what = f"fill n {n} d {d}"
        # row 0 lies I.PAD rows into the table and the flags: a row filled for the -1 padding would land in that guard
        mk = lambda: (fbuf(gpu_device, I.PAD + n_rows + I.PAD, d + 4),
                      torch.full((I.PAD + n_rows + I.PAD,), 9, dtype=torch.uint8, device=gpu_device))
        call = lambda dd, dst, flags, flag: N.call(
            "lkg_fill_rows_f32", n, dd, N.ptr(idd), N.ptr(dst[I.PAD:, c0:]) if dst is not None else None, d + 4, value,
            N.ptr(flags[I.PAD:]) if flags is not None else None, flag, ops._stream())
        dst, flags = mk()
        call(d, dst, flags, 1)
        I.check_fill(what + " dst + flags", ids, d, c0, value, host(dst), host(flags), 1)
        dst, _ = mk()
        call(d, dst, None, 1)
        I.check_fill(what + " dst", ids, d, c0, value, host(dst), None, 1)
        _, flags = mk()
        call(0, None, flags, 7)                                     # (any flag != 0 is stored as 1)
        I.check_fill(what + " flags", ids, 0, c0, value, None, host(flags), 1)
        call(0, None, flags, 0)
        I.check_fill(what + " flags reset", ids, 0, c0, value, None, host(flags), 0)


@pytest.mark.parametrize("d", [5, 130])
def test_scatter_add_rows_with_perm(ops, N, gpu_device, d):
    """dst[idx[perm[i]]] += src[i] on strided operands: per element against float64 over sum |src| (the measure of
    test_scatter_add_rows_with_repeated_ids)."""
    case = I.draw_scatter_add_perm(gpu_device, d)
    table = fbuf(gpu_device, case.n_x + I.PAD, d + 4)
    table[:case.n_x, 2:2 + d] = 0.0
    N.call("lkg_scatter_add_rows_f32", case.rows, d, N.ptr(case.src), d + 3, N.ptr(case.idx), N.ptr(case.perm),
           N.ptr(table[:, 2:]), d + 4, ops._stream())
    lines = []
    I.check_scatter_add_perm(lines, case, table)
    print(C.report(lines))


# =============================================================================================== CSR helpers
def run_csr_check(ops, N, dev, gpu_device, rowptr, n_rows, col, col_offset, n_cols):
    counter = ibuf(gpu_device, 1)
    rp, cl = dev(rowptr), dev(col)
    for _ in range(2):                                               # (the second call must not add to the first)
        N.call("lkg_csr_check_i32", n_rows, N.ptr(rp), col.size, N.ptr(cl), col_offset, n_cols, N.ptr(counter), ops._stream())
    got = host(counter)
    assert (got[1:] == I.ISENT).all()
    return int(got[0])


def test_csr_check(ops, N, dev, gpu_device):
    """exact counts of bad offsets and bad columns, one planted at a time; a row-range view; a column offset; no rows."""
    n_cols = 90
    rowptr, col = I.valid_csr(700, n_cols)
    nnz = col.size
    run = lambda rp, n_rows, cl, off=0, nc=n_cols: run_csr_check(ops, N, dev, gpu_device, rp, n_rows, cl, off, nc)
    assert run(rowptr, 700, col) == 0
    planted = {}
    rp = rowptr.copy()
    rp[300] = rp[301] + 1                                            # a decreasing offset
    planted["decreasing offset"] = (rp, col)
    rp = rowptr.copy()
    rp[0] = -1                                                       # a negative offset
    planted["negative offset"] = (rp, col)
    rp = rowptr.copy()
    rp[700] = nnz + 1                                                # an offset beyond nnz
    planted["offset beyond nnz"] = (rp, col)
    for name, v in (("column -1", -1), ("column n_cols", n_cols)):
        cl = col.copy()
        cl[nnz // 2] = v
        planted[name] = (rowptr, cl)
    for name, (rp, cl) in planted.items():
        want = I.csr_check_ref(rp, 700, nnz, cl, 0, n_cols)
        assert want >= 1 and run(rp, 700, cl) == want, (name, want)
    cl = col.copy()
    cl[0] = n_cols                                                   # a bad column outside the view of rows 100 .. 299
    assert rowptr[100] > 0 and run(rowptr[100:], 200, cl) == 0 and run(rowptr, 700, cl) == 1
    cl[rowptr[150]] = -1                                             # ... and one inside it
    assert rowptr[151] > rowptr[150] and run(rowptr[100:], 200, cl) == 1
    assert run(rowptr, 700, col + 5, off=5) == 0                     # a table handed over with a row offset
    want = int((col < 5).sum()) + int((col >= n_cols - 4).sum())
    assert want > 0 and run(rowptr, 700, col, off=5, nc=n_cols - 9) == I.csr_check_ref(rowptr, 700, nnz, col, 5, n_cols - 9) == want
    assert run(rowptr, 0, col) == 0                                  # n_rows = 0
    assert run(rowptr[5:], 0, cl) == 0


def test_csr_check_second_trip(ops, N, dev, gpu_device):
    """more entries than the 524 288 threads of the capped grid: a bad column in the last entry is counted."""
    n_rows, per = 8193, 65
    rowptr = (np.arange(n_rows + 1) * per).astype(np.int32)
    nnz = int(rowptr[-1])
    assert nnz > 524_288 + 64
    col = (np.arange(nnz) % 1000).astype(np.int32)
    assert run_csr_check(ops, N, dev, gpu_device, rowptr, n_rows, col, 0, 1000) == 0
    col[-1] = 1000
    assert run_csr_check(ops, N, dev, gpu_device, rowptr, n_rows, col, 0, 1000) == 1
    col[524_288] = -1
    assert run_csr_check(ops, N, dev, gpu_device, rowptr, n_rows, col, 0, 1000) == 2


@pytest.mark.parametrize("sel", list(I.EXTRACT_SELECTIONS))
def test_csr_extract_rows(ops, N, dev, gpu_device, sel):
    """rows of 0, 1, 63, 64, 65 and 300 entries copied into a compact CSR bit for bit, nothing past out_rowptr[-1]."""
    rowptr, col, val = I.draw_extract()
    rows = I.EXTRACT_SELECTIONS[sel](18)
    out_rowptr, want_c, _ = I.extract_ref(rowptr, col, val, rows)
    oc, ov = ibuf(gpu_device, want_c.size), fbuf(gpu_device, want_c.size + I.PAD)
    sel_d, rp, cl, vl, orp = (dev(x) for x in (rows.astype(np.int64), rowptr, col, val, out_rowptr))
    N.call("lkg_csr_extract_rows", rows.size, N.ptr(sel_d) if rows.size else None, N.ptr(rp), N.ptr(cl), N.ptr(vl), N.ptr(orp),
           N.ptr(oc), N.ptr(ov), ops._stream())
    I.check_extract(sel, rowptr, col, val, rows, host(oc), host(ov))


@pytest.mark.parametrize("d", I.SCATTER_BWD_D)
def test_spmm_scatter_bwd(ops, N, gpu_device, d):
    """g_x = A^T g_out of a sub-CSR with empty rows, a 300-entry row and repeated columns, values +-1e3 + noise: per element
    against float64 over |A|^T |g|, bound 3 x torch's float32 index_add_ (floor 3e-7); rows no column names stay zero."""
    case = I.draw_scatter_bwd(gpu_device, d)
    table = I.scatter_bwd_table(case)
    N.call("lkg_spmm_csr_scatter_bwd_f32", case.n_rows, d, N.ptr(case.rowptr), N.ptr(case.col), N.ptr(case.val), N.ptr(case.g),
           d + 3, N.ptr(table[:, 2:]), d + 4, ops._stream())
    lines = []
    I.check_scatter_bwd(lines, case, table)
    print(C.report(lines))


# =============================================================================================== the sampler
@pytest.fixture(scope="module")
def sampler_graphs(ops, gpu_device):
    from literalkg_amd.graph import KGStructure
    out = {}
    for kind in ("plain", "dups", "full head"):
        n, h, t, r = I.sampler_graph(kind)
        g = KGStructure.from_triples(n, h, t, r, device=gpu_device)
        assert g.n_raw == h.shape[0] and g.has_dups == (kind != "plain")
        out[kind] = (g, n, h, t, r)
    return out


@pytest.mark.parametrize("k", I.SAMPLER_RATES)
@pytest.mark.parametrize("seed", I.SAMPLER_SEEDS)
@pytest.mark.parametrize("case", list(I.SAMPLER_CASES))
def test_sampler_follows_its_documented_stream(ops, N, dev, gpu_device, sampler_graphs, case, seed, k):
    """All four outputs of lkg_sample_kg_batch equal, element for element, the plain-Python restatement of the stream the
    header documents -- on a graph without duplicate pairs (eptr = NULL), with them, with a head whose every candidate is
    rejected (the 256th is kept), and with heads that have no triple or lie outside the id range (sentinel groups)."""
    kind, bad = I.SAMPLER_CASES[case]
    g, n, h, t, r = sampler_graphs[kind]
    assert (g.eptr is None) == (kind == "plain")
    heads = I.sampler_heads(kind, bad, n, h)
    groups = heads.shape[0]
    assert groups == I.SAMPLER_GROUPS
    out = torch.full((4, groups * k + I.PAD), I.ISENT, dtype=torch.int64, device=gpu_device)
    hd = dev(heads)
    N.call("lkg_sample_kg_batch", groups, k, seed, N.ptr(hd), g.n, N.ptr(g.rowptr), N.ptr(g.col), N.ptr(g.eptr),
           N.ptr(g.rel), g.nnz, g.n_raw, N.ptr(out[0]), N.ptr(out[1]), N.ptr(out[2]), N.ptr(out[3]), ops._stream())
    out = host(out)
    assert (out[:, groups * k:] == I.ISENT).all()
    got = tuple(out[i, :groups * k] for i in range(4))
    want = I.sampler_replica(seed, heads, k, h, t, r, g.order)
    I.check_sampler(f"{case} seed {seed} k {k}", got, want)
    if bad:
        sentinel = np.repeat(np.isin(np.arange(groups), (3, 100, 299, 17)), k)
        assert np.array_equal(got[1] == -1, sentinel) and np.array_equal(got[2] == -1, sentinel) and np.array_equal(got[3] == -1, sentinel)
        assert np.array_equal(got[0], np.repeat(heads, k))
    elif kind == "plain":
        I.check_sampler_contract(got, k, h, t, r)


# =============================================================================================== Adam
def run_adam(ops, N, case, hp):
    """one lkg_adam_step_f32 on clones with a sentinel tail behind p, m and v; returns (p', m', v')"""
    n = case.n
    bufs = []
    for x in (case.p, case.m, case.v):
        b = torch.full((n + 8,), I.SENTINEL, device=x.device)
        b[:n] = x
        bufs.append(b)
    g = case.g.clone()
    N.call("lkg_adam_step_f32", n, N.ptr(bufs[0]), N.ptr(g), N.ptr(bufs[1]), N.ptr(bufs[2]), hp.lr, hp.b1, hp.b2, hp.eps, hp.wd,
           hp.step, ops._stream())
    assert torch.equal(g.view(torch.int32), case.g.view(torch.int32)), f"{case.what}: the gradient was written"
    for b in bufs:
        assert bool((b[n:] == I.SENTINEL).all()), f"{case.what}: wrote behind its {n} elements"
    return tuple(b[:n] for b in bufs)


@pytest.fixture(scope="module")
def adam_big(gpu_device):
    return I.draw_adam(gpu_device, I.ADAM_BIG, "mixed")


@pytest.mark.parametrize("wd", I.ADAM_WD)
@pytest.mark.parametrize("betas", I.ADAM_BETAS)
@pytest.mark.parametrize("step", I.ADAM_STEPS)
def test_adam_against_float64(ops, N, gpu_device, adam_big, step, betas, wd):
    """One step from given p, g, m, v against Adam in float64 with the hyper-parameters rounded to float32 (index_cases.
    check_adam counts the roundings): every draw at n = 1, 3, 4, 7, 1027, and the mixed draw at the size of the entity table,
    where the stride loop takes its second trip and the scalar tail is not empty; g is left as it was."""
    hp = I.adam_hyper(betas, wd, step)
    lines = []
    for n in I.ADAM_SMALL:
        for draw in I.ADAM_DRAWS:
            case = I.draw_adam(gpu_device, n, draw)
            I.check_adam(lines, case, hp, *run_adam(ops, N, case, hp))
    assert adam_big.n // 4 > 256 * 4096 and adam_big.n % 4 == 3
    out = run_adam(ops, N, adam_big, hp)
    I.check_adam(lines, adam_big, hp, *out)
    tail = I.NS(n=1203, what=f"{adam_big.what} (the last 1203)", **{k: getattr(adam_big, k)[-1203:] for k in "pgmv"})
    I.check_adam(lines, tail, hp, *(x[-1203:] for x in out))
    print(C.report(lines, 6))
