"""Can the checks of test_index_kernels_gpu.py tell a wrong kernel from a right one?  On the CPU, through the SAME draws and
the SAME check functions (index_cases.py): a plain implementation of every entry point -- numpy loops for the index kernels, a
port of the sampler onto the CSR arrays, float32 evaluations of Adam and the two scatters -- passes every check, and each
planted fault fails one: an unstable sort that swaps two equal-key neighbours, seg off by one for one key, a row gathered
through idx[i] instead of idx[perm[i]], a write into the sentinel column, a filled row at the -1 padding, a count off by
one, a sampler that takes a candidate draw before the positive draw, Adam with eps inside the square root, Adam without bias
correction at step 2, a scatter backward that drops the last entry of the 300-entry row."""
import numpy as np
import pytest
import torch

import index_cases as I
import rowwise_cases as C

CPU = torch.device("cpu")


def rejected(fn, *args, **kw):
    with pytest.raises(AssertionError):
        fn(*args, **kw)


def guarded(want, sent=None, pad=I.PAD):
    """a 1-D destination holding `want` with its guard behind it"""
    want = np.asarray(want)
    sent = (I.SENTINEL if want.dtype == np.float32 else I.ISENT) if sent is None else sent
    return np.concatenate([want, np.full(pad, sent, want.dtype)])


# ------------------------------------------------------------------------------------------------- group by key
def counting_sort(keys, n_keys):
    """the kernel's plan in plain Python: count per key, prefix sum, place in input order"""
    kc = [min(max(int(k), 0), n_keys - 1) for k in keys]
    cnt = [0] * (n_keys + 1)
    for k in kc:
        cnt[k + 1] += 1
    seg = np.cumsum(cnt).astype(np.int32)
    nxt = seg.copy()
    perm = np.zeros(len(kc), np.int32)
    for i, k in enumerate(kc):
        perm[nxt[k]] = i
        nxt[k] += 1
    return perm, seg, sum(1 for k in keys if k < 0 or k >= n_keys)


@pytest.mark.parametrize("draw", I.GB_DRAWS)
@pytest.mark.parametrize("n,n_keys", [(0, 1), (65, 2), (1025, 100), (3089, 1024)])
def test_group_by_key_measure(n, n_keys, draw):
    keys = I.draw_keys(n, n_keys, draw)
    perm, seg, bad = counting_sort(keys, n_keys)
    I.check_group_by_key(draw, keys, n_keys, guarded(perm), guarded(seg), bad)
    if n < 65:
        return
    same = np.flatnonzero(keys[perm[:-1]] == keys[perm[1:]])
    assert same.size
    swapped = perm.copy()
    j = same[same.size // 2]
    swapped[[j, j + 1]] = swapped[[j + 1, j]]                       # an unstable sort: two equal-key neighbours swapped
    rejected(I.check_group_by_key, draw, keys, n_keys, guarded(swapped), guarded(seg), bad)
    off = seg.copy()
    off[1 + (n_keys - 1) // 2] += 1                                 # seg off by one for one key
    rejected(I.check_group_by_key, draw, keys, n_keys, guarded(perm), guarded(off), bad)
    rejected(I.check_group_by_key, draw, keys, n_keys, guarded(perm), guarded(seg), bad + 1)
    over = guarded(perm)
    over[n] = 0                                                     # one element written behind perm
    rejected(I.check_group_by_key, draw, keys, n_keys, over, guarded(seg), bad)


def test_group_by_key_bad_keys_measure():
    n, n_keys = 1025, 100
    keys = I.draw_keys(n, n_keys, "uniform")
    keys[[0, 500, 1024]] = [-1, n_keys, 2 ** 40]
    perm, seg, bad = counting_sort(keys, n_keys)
    assert bad == 3
    I.check_group_by_key_bad("bad keys", keys, n_keys, guarded(perm), guarded(seg), bad)
    I.check_group_by_key("bad keys", keys, n_keys, guarded(perm), guarded(seg), bad)
    rejected(I.check_group_by_key_bad, "bad keys", keys, n_keys, guarded(perm), guarded(seg), bad - 1)
    twice = perm.copy()
    twice[3] = twice[4]                                             # (a lost element: not a permutation)
    rejected(I.check_group_by_key_bad, "bad keys", keys, n_keys, guarded(twice), guarded(seg), bad)
    short = seg.copy()
    short[-1] -= 1
    rejected(I.check_group_by_key_bad, "bad keys", keys, n_keys, guarded(perm), guarded(short), bad)


# ------------------------------------------------------------------------------------------------- small integer kernels
@pytest.mark.parametrize("n_groups,k,n_seg", I.EXPAND_CASES)
def test_expand_groups_measure(n_groups, k, n_seg):
    perm, seg = I.draw_expand(n_groups, k, n_seg)
    po = np.array([p * k + j for p in perm.tolist() for j in range(k)], np.int32)
    so = np.array([s * k for s in seg.tolist()], np.int32)
    I.check_expand("expand", perm, seg, k, guarded(po), guarded(so))
    bad = so.copy()
    bad[-1] += 1
    rejected(I.check_expand, "expand", perm, seg, k, guarded(po), guarded(bad))
    if n_groups * k > 1:
        bad = po.copy()
        bad[[0, 1]] = bad[[1, 0]]
        rejected(I.check_expand, "expand", perm, seg, k, guarded(bad), guarded(so))
    bad = guarded(po)
    bad[po.size] = 0
    rejected(I.check_expand, "expand", perm, seg, k, bad, guarded(so))


def test_gather_i64_and_permute_measure():
    rng = np.random.default_rng(0)
    for n in (1, 257):
        src = rng.integers(-2 ** 40, 2 ** 40, n + 3, dtype=np.int64)
        perm = rng.integers(0, n + 3, n).astype(np.int32)
        dst = np.array([src[p] for p in perm], np.int64)
        I.check_gather_i64("gather_i64", src, perm, guarded(dst))
        rejected(I.check_gather_i64, "gather_i64", src, perm, guarded(dst + (np.arange(n) == n - 1)))
        perm, n_src, src, planted = I.draw_permute(n)
        assert len(planted) == (1 if n == 1 else 3)
        dst = np.array([src[p] if 0 <= p < n_src else np.nan for p in perm.tolist()], np.float32)
        I.check_permute("permute", perm, n_src, src, guarded(dst))
        bad = dst.copy()
        bad[planted[0]] = 0.0                                       # a value where the index is outside the source
        rejected(I.check_permute, "permute", perm, n_src, src, guarded(bad))
        if n > 1:
            bad = dst.copy()
            bad[1] = np.nan                                         # NaN where the index is fine
            rejected(I.check_permute, "permute", perm, n_src, src, guarded(bad))
            bad = dst.copy()
            ok = [i for i in range(n) if i not in planted]
            bad[ok[0]] = -bad[ok[0]]                                # (one sign bit)
            rejected(I.check_permute, "permute", perm, n_src, src, guarded(bad))


@pytest.mark.parametrize("fault", I.FAULTS)
@pytest.mark.parametrize("n", [0, 1, 65, 257])
def test_counters_measure(n, fault):
    for k in (1, 2, 7):
        for field in ("h", "r", "pos_t"):
            h, r, p = I.draw_grouped_batch(n, k, fault, field)
            loop = sum(1 for i in range(n) if (h[i], r[i], p[i]) != (h[i // k * k], r[i // k * k], p[i // k * k]))
            assert I.check_grouped_ref(h, r, p, k) == loop
            if k > 1 and fault != "none" and n > 1:
                assert loop > 0
    lo, hi = 3, 50
    ids = I.draw_ids(n, lo, hi, fault)
    out = np.array([v if lo <= v < hi else lo for v in ids.tolist()], np.int64)
    bad = sum(1 for v in ids.tolist() if not lo <= v < hi)
    assert bad == {"none": 0, "last": min(n, 1), "wave": min(n, 64), "all": n}[fault]
    I.check_sanitize("sanitize", ids, lo, hi, guarded(out), bad)
    rejected(I.check_sanitize, "sanitize", ids, lo, hi, guarded(out), bad + 1)          # a count off by one
    if bad:
        zero = np.where((ids < lo) | (ids >= hi), 0, ids)           # the bad ids replaced by 0, not by lo
        rejected(I.check_sanitize, "sanitize", ids, lo, hi, guarded(zero), bad)


# ------------------------------------------------------------------------------------------------- row gathers and fills
def gather_rows_loop(case, through_perm=True):
    dst = np.full((case.n + I.PAD, case.ld), I.SENTINEL, np.float32)
    for i in range(case.n):
        p = int(case.perm[i]) if case.perm is not None and through_perm else i
        r = int(case.idx[p]) if case.idx is not None else p
        dst[i, case.c0:case.c0 + case.d] = case.table[r, case.c0:case.c0 + case.d]
    return dst


@pytest.mark.parametrize("view", list(I.GATHER_VIEWS))
@pytest.mark.parametrize("form", I.GATHER_FORMS)
def test_gather_rows_measure(form, view):
    for n, d in ((1, 1), (5, 4), (37, 68)):
        case = I.draw_gather(n, d, form, view)
        assert I.gather_vec(d, view) == (d % 4 == 0 and view in ("contiguous", "four floats in"))
        good = gather_rows_loop(case)
        I.check_gather_rows(case, good)
        if form == "both" and n > 1:
            rejected(I.check_gather_rows, case, gather_rows_loop(case, through_perm=False))     # idx[i], not idx[perm[i]]
        bad = good.copy()
        bad[n - 1, case.c0 + d] = 0.0                               # a write into the sentinel column
        rejected(I.check_gather_rows, case, bad)
        bad = good.copy()
        bad[n, case.c0] = 0.0                                       # a row too many
        rejected(I.check_gather_rows, case, bad)
        if case.c0:
            bad = good.copy()
            bad[0, case.c0 - 1] = 0.0
            rejected(I.check_gather_rows, case, bad)


def test_gather_range_measure():
    n, d, n_table, c0 = 40, 5, 30, 1
    for lo, hi in ((0, n_table), (7, 19), (7, 7)):
        table, ids = I.draw_gather_range(n, d, lo, hi, n_table)
        dst = np.full((n + I.PAD, d + 3), I.SENTINEL, np.float32)
        for i, v in enumerate(ids.tolist()):
            dst[i, c0:c0 + d] = table[v, c0:c0 + d] if lo <= v < hi else 0.0
        I.check_gather_range("range", table, c0, d, ids, lo, hi, dst)
        bad = dst.copy()
        bad[4, c0] = -0.0                                           # id -1: exactly +0.0 is asked for
        rejected(I.check_gather_range, "range", table, c0, d, ids, lo, hi, bad)
        if hi > lo:
            shifted = dst.copy()
            shifted[1, c0:c0 + d] = table[lo + 1, c0:c0 + d]        # the row of id lo read without subtracting row_lo right
            rejected(I.check_gather_range, "range", table, c0, d, ids, lo, hi, shifted)


def fill_loop(ids, n_rows, d, c0, value, flag, skip_padding=True):
    """the table and the flags with I.PAD guard rows in FRONT of row 0 and behind the last row (as the device test lays them
    out): without the skip, id -1 lands in the guard row before row 0, where a kernel would write"""
    dst = np.full((I.PAD + n_rows + I.PAD, d + 4), I.SENTINEL, np.float32)
    flags = np.full(I.PAD + n_rows + I.PAD, 9, np.uint8)
    for v in ids.tolist():
        if v < 0 and skip_padding:
            continue
        dst[I.PAD + v, c0:c0 + d] = value
        flags[I.PAD + v] = 1 if flag else 0
    return dst, flags


@pytest.mark.parametrize("d", I.FILL_D)
def test_fill_rows_measure(d):
    n_rows, c0 = 50, 2
    ids = I.draw_fill_ids(n_rows, 60)
    assert (ids == -1).any() and np.unique(ids).size < ids.size
    dst, flags = fill_loop(ids, n_rows, d, c0, 2.5, 1)
    I.check_fill("fill", ids, d, c0, 2.5, dst, flags, 1)
    I.check_fill("fill", ids, d, c0, 2.5, dst, None, 1)
    I.check_fill("fill", ids, 0, c0, 2.5, None, flags, 1)
    bad_dst, bad_flags = fill_loop(ids, n_rows, d, c0, 2.5, 1, skip_padding=False)      # a filled row at the -1 padding
    rejected(I.check_fill, "fill", ids, d, c0, 2.5, bad_dst, None, 1)
    rejected(I.check_fill, "fill", ids, 0, c0, 2.5, None, bad_flags, 1)
    wide = dst.copy()
    wide[I.PAD + int(ids[1]), c0 + d] = 2.5                         # a write into the sentinel column
    rejected(I.check_fill, "fill", ids, d, c0, 2.5, wide, flags, 1)
    _, reset = fill_loop(ids, n_rows, d, c0, 0.0, 0)
    I.check_fill("fill", ids, 0, c0, 0.0, None, reset, 0)
    rejected(I.check_fill, "fill", ids, 0, c0, 0.0, None, flags, 0)                     # the flags were not reset


# ------------------------------------------------------------------------------------------------- CSR helpers
def test_csr_check_measure():
    rowptr, col = I.valid_csr(700, 90)
    nnz = col.size
    loop = lambda rp, n_rows, cl, off, n_cols: (
        sum(1 for i in range(n_rows) if rp[i] < 0 or rp[i] > rp[i + 1] or rp[i + 1] > nnz) +
        sum(1 for j in range(min(max(int(rp[0]), 0), nnz), min(max(int(rp[n_rows]), min(max(int(rp[0]), 0), nnz)), nnz))
            if not 0 <= cl[j] - off < n_cols))
    assert I.csr_check_ref(rowptr, 700, nnz, col, 0, 90) == loop(rowptr, 700, col, 0, 90) == 0
    bad = rowptr.copy()
    bad[300] = bad[299] - 1 if bad[299] > 0 else bad[301] + 1
    assert I.csr_check_ref(bad, 700, nnz, col, 0, 90) == loop(bad, 700, col, 0, 90) >= 1
    c2 = col.copy()
    c2[-1] = 90
    assert I.csr_check_ref(rowptr, 700, nnz, c2, 0, 90) == loop(rowptr, 700, c2, 0, 90) == 1
    assert I.csr_check_ref(rowptr[100:], 200, nnz, c2, 0, 90) == 0                     # outside the view: not counted
    assert I.csr_check_ref(rowptr, 700, nnz, col + 5, 5, 90) == 0
    assert I.csr_check_ref(rowptr, 700, nnz, col, 5, 90) == int((col < 5).sum()) > 0


@pytest.mark.parametrize("sel", list(I.EXTRACT_SELECTIONS))
def test_extract_rows_measure(sel):
    rowptr, col, val = I.draw_extract()
    rows = I.EXTRACT_SELECTIONS[sel](18)
    oc, ov = [], []
    for s in rows.tolist():
        oc += col[rowptr[s]:rowptr[s + 1]].tolist()
        ov += val[rowptr[s]:rowptr[s + 1]].tolist()
    oc, ov = np.array(oc, np.int32), np.array(ov, np.float32)
    I.check_extract(sel, rowptr, col, val, rows, guarded(oc), guarded(ov))
    over = guarded(ov)
    over[ov.size] = 0.0                                             # written past out_rowptr[-1]
    rejected(I.check_extract, sel, rowptr, col, val, rows, guarded(oc), over)
    if oc.size > 300:
        short = oc.copy()
        short[-1] = short[-2]                                       # the last entry of the 300-entry row
        if short[-1] != oc[-1]:
            rejected(I.check_extract, sel, rowptr, col, val, rows, guarded(short), guarded(ov))


# ------------------------------------------------------------------------------------------------- the two scatters
@pytest.mark.parametrize("d", [5, 130])
def test_scatter_measures(d):
    case = I.draw_scatter_bwd(CPU, d)
    rp = case.rowptr.tolist()
    assert rp[8] - rp[7] == 300 and rp[1] == rp[0]
    table = I.scatter_bwd_table(case)
    table[:case.n_x, 2:2 + d] = I.scatter_bwd_eval(case, torch.float32)
    lines = []
    I.check_scatter_bwd(lines, case, table)
    assert len(lines) == 1 and lines[0][1] <= lines[0][2]
    dropped = table.clone()
    dropped[:case.n_x, 2:2 + d] = I.scatter_bwd_eval(case, torch.float32, drop_last_of=case.long_row)
    rejected(I.check_scatter_bwd, [], case, dropped)                # the last entry of the 300-entry row dropped
    wide = table.clone()
    wide[3, 2 + d] = 0.0
    rejected(I.check_scatter_bwd, [], case, wide)
    stray = table.clone()
    stray[85, 2] = 1e-30                                            # a row that no column names
    rejected(I.check_scatter_bwd, [], case, stray)
    sc = I.draw_scatter_add_perm(CPU, d)
    t2 = torch.full((sc.n_x + I.PAD, d + 4), I.SENTINEL)
    ids = sc.idx[sc.perm.long()]
    t2[:sc.n_x, 2:2 + d] = torch.zeros(sc.n_x, d).index_add_(0, ids, sc.src)
    I.check_scatter_add_perm([], sc, t2)
    direct = t2.clone()
    direct[:sc.n_x, 2:2 + d] = torch.zeros(sc.n_x, d).index_add_(0, sc.idx, sc.src)     # idx[i], not idx[perm[i]]
    rejected(I.check_scatter_add_perm, [], sc, direct)


# ------------------------------------------------------------------------------------------------- the sampler
def sampler_on_csr(g, seed, heads, k):
    """lkg_sample_kg_batch's plan on the structure's arrays (rowptr, col, eptr, rel), the draws taken from I.Stream"""
    rowptr, col, rel = (g.host(x) for x in ("rowptr", "col", "rel"))
    eptr = g.host("eptr") if g.has_dups else np.arange(g.nnz + 1)
    entry_of = lambda e: int(np.searchsorted(eptr, e, side="right")) - 1
    out = [[], [], [], []]
    for gi, h in enumerate(int(x) for x in heads):
        inside = 0 <= h < g.n
        j0, j1 = (int(rowptr[h]), int(rowptr[h + 1])) if inside else (0, 0)
        e0, e1 = int(eptr[j0]), int(eptr[j1])
        if e1 <= e0:
            for o, v in zip(out, (h, -1, -1, -1)):
                o.extend([v] * k)
            continue
        s = I.Stream(seed, gi)
        ep = e0 + s.below(e1 - e0)
        r, tp = int(rel[ep]), int(col[entry_of(ep)])
        negs = []
        for _ in range(k):
            for _ in range(I.MAX_TRIES):
                cand = int(col[entry_of(s.below(g.n_raw))])
                j = j0 + int(np.searchsorted(col[j0:j1], cand))
                hit = j < j1 and col[j] == cand and r in rel[eptr[j]:eptr[j + 1]].tolist()
                if not hit and cand not in negs:
                    break
            negs.append(cand)
        for o, v in zip(out[:3], (h, r, tp)):
            o.extend([v] * k)
        out[3].extend(negs)
    return tuple(np.array(o, np.int64) for o in out)


@pytest.fixture(scope="module")
def structure_class():
    """KGStructure builds its arrays with the library's host code (lkg_csr_build): the library has to be there"""
    import __graft_entry__ as ge
    ge.build()
    from literalkg_amd.graph import KGStructure
    return KGStructure


@pytest.mark.parametrize("case", list(I.SAMPLER_CASES))
def test_sampler_replica_measure(structure_class, case):
    KGStructure = structure_class
    kind, bad = I.SAMPLER_CASES[case]
    n, h, t, r = I.sampler_graph(kind)
    g = KGStructure.from_triples(n, h, t, r)
    assert g.has_dups == (kind != "plain")
    heads = I.sampler_heads(kind, bad, n, h)
    if kind == "full head":
        heads = heads[:40]                                          # (256 tries per negative: the device test runs all 300)
    for seed, k in ((0, 5), (2 ** 63 + 5, 1)):
        want = I.sampler_replica(seed, heads, k, h, t, r, g.order)
        got = sampler_on_csr(g, seed, heads, k)
        I.check_sampler(case, got, want)
        if bad:
            assert all((want[1][i * k] == -1) == (i in (3, 100, 299, 17)) for i in range(len(heads)))
            assert want[0][3 * k] == 199 and want[0][17 * k] == 2 ** 40 and want[3][100 * k] == -1
        elif kind != "full head":
            I.check_sampler_contract(want, k, h, t, r)
        else:
            assert set(want[3].tolist()) <= {0, 1, 2, 3}            # every candidate was a positive; the 256th was kept
        rejected(I.check_sampler, case, I.sampler_replica(seed, heads, k, h, t, r, g.order, candidate_first=True), want)
        rejected(I.check_sampler, case, sampler_on_csr(g, seed ^ 1, heads, k), want)


# ------------------------------------------------------------------------------------------------- Adam
@pytest.mark.parametrize("wd", I.ADAM_WD)
@pytest.mark.parametrize("betas", I.ADAM_BETAS)
def test_adam_measure(betas, wd):
    lines = []
    for step in I.ADAM_STEPS:
        hp = I.adam_hyper(betas, wd, step)
        for n, draw in [(n, d) for n in (1, 7) for d in I.ADAM_DRAWS] + [(1027, "mixed")]:
            case = I.draw_adam(CPU, n, draw)
            I.check_adam(lines, case, hp, *I.adam_f32(case, hp))
        case = I.draw_adam(CPU, 1027, "mixed")
        p1, m1, v1 = I.adam_f32(case, hp)
        rejected(I.check_adam, [], case, hp, I.adam_f32(case, hp, eps_inside=True)[0], m1, v1)
        if step == 2:
            rejected(I.check_adam, [], case, hp, I.adam_f32(case, hp, no_bias_correction=True)[0], m1, v1)
        # moments 8 roundings of their scale further off than they are
        sgg = (hp.wd * case.p.double()).abs() + case.g.double().abs()
        for name, k_, sc in (("m", 1, hp.b1 * case.m.double().abs() + (1 - hp.b1) * sgg),
                             ("v", 2, hp.b2 * case.v.double().abs() + (1 - hp.b2) * sgg * sgg)):
            out = [p1, m1.clone(), v1.clone()]
            i = int(sc.argmax())
            out[k_][i] = float(out[k_][i].double() + 16 * 2.0 ** -24 * sc[i])
            rejected(I.check_adam, [], case, hp, *out)
    print(C.report(lines, 6))
