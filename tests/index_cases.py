"""References, draws and checks shared by test_index_kernels_gpu.py (the HIP kernels on the device) and
test_index_measures_host.py (plain numpy implementations and planted faults on the CPU, through the SAME checks): the kernels
that move rows and ids around (lkg_batch.hip, the index helpers of lkg_spmm.hip), the batch sampler held to its documented
stream, and Adam against float64.

Everything integer-valued or copied is compared with EXACT equality (floats bit for bit).  Every destination is allocated
longer and wider than what the call may write and pre-filled with a sentinel; every check asserts that the bytes outside the
written region still hold it.  The checks take numpy arrays (the device test copies its buffers back), the two float measures
(scatter backward, scatter-add) and Adam take torch tensors on either device."""
import math
from types import SimpleNamespace as NS

import numpy as np
import torch

import op_audit as A
import rowwise_cases as C

SENTINEL = C.SENTINEL          # float destinations
ISENT = -77                    # integer destinations (no valid id, offset or count)
PAD = 5                        # guard elements / rows behind every destination
INT32_MAX = 2 ** 31 - 1


def bits(a):
    """float32 array -> its bit patterns (NaN payloads and the sign of zero count)"""
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def check_exact(what, buf, want, sent=None):
    """buf[:len(want)] == want bit for bit and buf[len(want):] still holds the sentinel (1-D destinations)"""
    want = np.asarray(want)
    n = want.shape[0]
    assert buf.ndim == 1 and buf.shape[0] > n, f"{what}: the destination has no guard behind it"
    assert buf.dtype == want.dtype, (what, buf.dtype, want.dtype)
    sent = (SENTINEL if buf.dtype == np.float32 else ISENT) if sent is None else sent
    neq = np.flatnonzero(bits(buf[:n]) != bits(want))
    assert neq.size == 0, f"{what}: {neq.size} of {n} elements differ, first at {neq[0]}: got {buf[neq[0]]!r}, want {want[neq[0]]!r}"
    assert (buf[n:] == sent).all(), f"{what}: wrote behind its {n} elements"


def check_exact_rows(what, table, want, c0=0, sent=SENTINEL, rows=None):
    """table[rows, c0:c0 + d] == want bit for bit (rows: the first len(want) rows, or a list of distinct row ids) and
    every other element of the table still holds the sentinel"""
    want = np.asarray(want)
    n, d = want.shape
    rows = np.arange(n) if rows is None else np.asarray(rows)
    assert table.shape[0] > (rows.max() + 1 if n else 0) and table.shape[1] > c0 + d, f"{what}: the destination has no guard"
    got = table[rows, c0:c0 + d]
    neq = np.argwhere(bits(got) != bits(want))
    assert neq.shape[0] == 0, (f"{what}: {neq.shape[0]} elements differ, first at {tuple(neq[0])}: got "
                               f"{got[tuple(neq[0])]!r}, want {want[tuple(neq[0])]!r}")
    mask = np.ones(table.shape, bool)
    mask[rows, c0:c0 + d] = False
    out = np.argwhere(mask & (table != sent))
    assert out.shape[0] == 0, f"{what}: wrote outside its region, first at {tuple(out[0])}: {table[tuple(out[0])]!r}"


# =============================================================================================== lkg_group_by_key_i64
GB_WAVES = 16
GB_N = [0, 1, 63, 64, 65, 1023, 1024, 1025, 16 * 64 * 3 + 17, 70_001]
GB_KEYS = [1, 2, 100, 1023, 1024]
GB_DRAWS = ["uniform", "one key", "descending", "wave chunks"]


def gb_chunk(n):
    """elements per wave of the one sorting workgroup (a multiple of 64)"""
    return ((n + GB_WAVES - 1) // GB_WAVES + 63) // 64 * 64


def draw_keys(n, n_keys, draw, seed=0):
    rng = np.random.default_rng(seed + 131 * n + n_keys)
    i = np.arange(n, dtype=np.int64)
    if draw == "uniform":
        return rng.integers(0, n_keys, n, dtype=np.int64)
    if draw == "one key":
        return np.full(n, n_keys // 2, np.int64)
    if draw == "descending":                       # one key per element, descending (wrapping when n > n_keys)
        return (n_keys - 1 - i % n_keys).astype(np.int64)
    if draw == "wave chunks":                      # every wave's chunk holds the same few keys: the order ACROSS waves decides
        return ((i % max(gb_chunk(n), 1)) * 7 % min(5, n_keys)).astype(np.int64)
    raise ValueError(draw)


def group_by_key_ref(keys, n_keys):
    """(perm, seg, n_bad): stable order by key, first position of every key (and n at the end), keys outside [0, n_keys)
    counted and grouped with the nearest valid key"""
    kc = np.clip(keys, 0, n_keys - 1)
    perm = np.argsort(kc, kind="stable")
    seg = np.searchsorted(kc[perm], np.arange(n_keys + 1))
    return perm.astype(np.int32), seg.astype(np.int32), int(((keys < 0) | (keys >= n_keys)).sum())


def check_group_by_key(what, keys, n_keys, perm_buf, seg_buf, n_bad=None):
    perm, seg, bad = group_by_key_ref(keys, n_keys)
    check_exact(f"{what} perm", perm_buf, perm)
    check_exact(f"{what} seg", seg_buf, seg)
    if n_bad is not None:
        assert int(n_bad) == bad, f"{what}: n_bad {int(n_bad)}, want {bad}"


def check_group_by_key_bad(what, keys, n_keys, perm_buf, seg_buf, n_bad):
    """with keys outside the range: the exact count, perm still a permutation of range(n), seg non-decreasing up to n"""
    n = keys.shape[0]
    bad = int(((keys < 0) | (keys >= n_keys)).sum())
    assert int(n_bad) == bad, f"{what}: n_bad {int(n_bad)}, want {bad}"
    assert np.array_equal(np.sort(perm_buf[:n]), np.arange(n)), f"{what}: perm is not a permutation of range({n})"
    seg = seg_buf[:n_keys + 1]
    assert (np.diff(seg) >= 0).all() and seg[0] == 0 and seg[-1] == n, f"{what}: seg is not non-decreasing from 0 to {n}"
    assert (perm_buf[n:] == ISENT).all() and (seg_buf[n_keys + 1:] == ISENT).all(), f"{what}: wrote behind its outputs"


# =============================================================================================== lkg_expand_groups_i32
EXPAND_CASES = [(0, 3, 5), (1, 1, 2), (37, 7, 4), (5, 2, 300), (1000, 64, 17)]      # (n_groups, k, n_seg)


def draw_expand(n_groups, k, n_seg, seed=0):
    rng = np.random.default_rng(seed + n_groups + k)
    perm = rng.permutation(n_groups).astype(np.int32)
    seg = np.sort(rng.integers(0, n_groups + 1, n_seg)).astype(np.int32)
    return perm, seg


def check_expand(what, perm, seg, k, perm_out, seg_out):
    want = (perm.astype(np.int64)[:, None] * k + np.arange(k)).reshape(-1).astype(np.int32)
    check_exact(f"{what} perm_out", perm_out, want)
    check_exact(f"{what} seg_out", seg_out, (seg * k).astype(np.int32))


# =============================================================================================== lkg_gather_i64 / lkg_permute_f32
STRIDE_N = [1, 255, 257, 524_288 + 77]         # 2048 blocks of 256 cover 524 288: the last size takes a second trip


def check_gather_i64(what, src, perm, dst):
    check_exact(what, dst, src[perm])


def draw_permute(n, seed=0):
    """(perm, n_src, src, planted): a list into n_src values with -1, n_src and INT32_MAX planted (as far as n allows; the
    last one in the last element, i.e. in the stride loop's last trip)"""
    rng = np.random.default_rng(seed + n)
    n_src = n + 11
    src = rng.standard_normal(n_src).astype(np.float32)
    src[0] = -0.0
    perm = rng.integers(0, n_src, n).astype(np.int32)
    planted = {}
    for pos, v in ((n - 1, INT32_MAX), (n // 2, n_src), (n // 3, -1)):
        if pos not in planted and (pos > 0 or n == 1):
            planted[pos] = v
    for pos, v in planted.items():
        perm[pos] = v
    return perm, n_src, src, sorted(planted)


def check_permute(what, perm, n_src, src, dst):
    """NaN at exactly the positions whose index lies outside [0, n_src), the source's bits everywhere else"""
    n = perm.shape[0]
    ok = (perm >= 0) & (perm < n_src)
    got = dst[:n]
    assert np.array_equal(np.isnan(got), ~ok), f"{what}: NaN at {np.flatnonzero(np.isnan(got))[:8]}, want at {np.flatnonzero(~ok)[:8]}"
    want = np.where(ok, src[np.where(ok, perm, 0)], got)
    check_exact(what, dst, want.astype(np.float32))


# =============================================================================================== counters
COUNT_N = [0, 1, 64, 65, 256, 257, 5000]
FAULTS = ["none", "last", "wave", "all"]


def fault_positions(n, fault):
    if fault == "none" or n == 0:
        return np.zeros(0, np.int64)
    if fault == "last":
        return np.array([n - 1])
    if fault == "wave":                            # a full wave of 64 consecutive elements (the second wave where there is one)
        lo = 64 if n >= 128 else 0
        return np.arange(lo, min(lo + 64, n))
    return np.arange(n)


def draw_grouped_batch(n, k, fault, field, seed=0):
    """(h, r, pos_t) of n rows in groups of k rows sharing all three, then `fault` planted in `field`"""
    rng = np.random.default_rng(seed + n + k)
    g = (n + k - 1) // k
    cols = [np.repeat(rng.integers(0, 1000, g, dtype=np.int64), k)[:n].copy() for _ in range(3)]
    pos = fault_positions(n, fault)
    if fault == "last" and k > 1 and n > 1 and (n - 1) % k == 0:
        pos = pos - 1                              # (the last element opens a group of its own: the one before it, then)
    cols["h r pos_t".split().index(field)][pos] += 1 + (pos % 3)
    return cols


def check_grouped_ref(h, r, p, k):
    n = h.shape[0]
    f = np.arange(n) // k * k
    return int(((h != h[f]) | (r != r[f]) | (p != p[f])).sum())


def draw_ids(n, lo, hi, fault, seed=0):
    rng = np.random.default_rng(seed + n)
    ids = rng.integers(lo, hi, n, dtype=np.int64)
    pos = fault_positions(n, fault)
    ids[pos] = np.where(pos % 2 == 0, hi + pos, lo - 1 - pos)
    if pos.size:
        ids[pos[0]] = hi                           # the first value past the range
    return ids


def check_sanitize(what, ids, lo, hi, out, n_bad):
    bad = (ids < lo) | (ids >= hi)
    assert int(n_bad) == int(bad.sum()), f"{what}: n_bad {int(n_bad)}, want {int(bad.sum())}"
    check_exact(what, out, np.where(bad, lo, ids))


# =============================================================================================== row gathers / fills
GATHER_D = [1, 3, 4, 64, 68, 260, 300]
GATHER_N = [1, 3, 4, 5, 1027]
GATHER_FORMS = ["idx", "perm", "both", "neither"]
# view -> (columns beside the d used ones, first used column): both operands of a case use the same view
GATHER_VIEWS = {"contiguous": (4, 0), "one float in": (3, 1), "four floats in": (8, 4), "odd ld": (5, 0)}


def gather_vec(d, view):
    """does lkg_gather_rows_f32 take its float4 kernel?  d % 4 == 0, both leading dimensions % 4 == 0, both bases 16-byte
    aligned (the tables are; a view c0 floats in is when c0 % 4 == 0)"""
    extra, c0 = GATHER_VIEWS[view]
    return d % 4 == 0 and (d + extra) % 4 == 0 and c0 % 4 == 0


def draw_gather(n, d, form, view, seed=0):
    """src table [n_src, d + extra] (the operand is its columns c0 .. c0 + d), idx / perm as the form asks, repeated ids"""
    rng = np.random.default_rng(seed + 7 * n + d)
    extra, c0 = GATHER_VIEWS[view]
    n_src = n + 9
    table = rng.standard_normal((n_src, d + extra)).astype(np.float32)
    table[0, c0] = -0.0
    idx = perm = None
    if form in ("idx", "both"):
        n_idx = n + 5 if form == "both" else n
        idx = rng.integers(0, n_src, n_idx, dtype=np.int64)
        idx[n_idx // 2] = idx[0]                                                   # a repeated id
    if form in ("perm", "both"):
        perm = rng.integers(0, n + 5 if form == "both" else n_src, n).astype(np.int32)
        if n > 1:
            perm[-1] = perm[0]
    return NS(n=n, d=d, table=table, c0=c0, ld=d + extra, idx=idx, perm=perm, what=f"gather_rows n {n} d {d} {form} {view}")


def gather_rows_ref(case):
    p = case.perm.astype(np.int64) if case.perm is not None else np.arange(case.n)
    r = case.idx[p] if case.idx is not None else p
    return case.table[r, case.c0:case.c0 + case.d]


def check_gather_rows(case, dst_table):
    check_exact_rows(case.what, dst_table, gather_rows_ref(case), case.c0)


def draw_gather_range(n, d, lo, hi, n_table, seed=0):
    """ids below, inside and above [lo, hi) (and -1, the padding of id lists)"""
    rng = np.random.default_rng(seed + n + d)
    table = rng.standard_normal((n_table, d + 3)).astype(np.float32)
    ids = rng.integers(0, n_table + 4, n, dtype=np.int64)
    fixed = [lo - 1, lo, hi - 1, hi, -1, n_table + 3]
    ids[:min(n, len(fixed))] = fixed[:n]
    return table, ids


def check_gather_range(what, table, c0, d, ids, lo, hi, dst_table):
    mine = (ids >= lo) & (ids < hi)
    want = np.where(mine[:, None], table[np.where(mine, ids, 0), c0:c0 + d], np.float32(0.0)).astype(np.float32)
    check_exact_rows(what, dst_table, want, c0)


FILL_D = [1, 5, 64, 300]


def draw_fill_ids(n_rows, n, seed=0):
    """ids with duplicates and -1 padding"""
    rng = np.random.default_rng(seed + n)
    ids = rng.integers(0, n_rows, n, dtype=np.int64)
    ids[::5] = -1
    if n > 1:
        ids[1::7] = ids[1]
    return ids


def check_fill(what, ids, d, c0, value, dst_table, flags, flag, flags_before=9):
    """rows named by an id >= 0 hold `value` in their d columns, their flag is (flag != 0); nothing else changed.  The
    table and the flags are handed over WITH the PAD guard rows that lie in front of row 0 (and those behind the last row):
    a row filled for the -1 padding shows up in the guard before row 0."""
    rows = np.unique(ids[ids >= 0]) + PAD
    if dst_table is not None:
        check_exact_rows(what, dst_table, np.full((rows.size, d), value, np.float32), c0, rows=rows)
    if flags is not None:
        want = np.full(flags.shape, flags_before, np.uint8)
        want[rows] = 1 if flag else 0
        assert np.array_equal(flags, want), f"{what}: flags differ at {np.flatnonzero(flags != want)[:8]}"


# =============================================================================================== CSR helpers
def valid_csr(n_rows, n_cols, seed=0, mean=6):
    rng = np.random.default_rng(seed + n_rows)
    cnt = rng.integers(0, 2 * mean, n_rows)
    rowptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    col = rng.integers(0, n_cols, int(rowptr[-1])).astype(np.int32)
    return rowptr, col


def csr_check_ref(rowptr, n_rows, nnz, col, col_offset, n_cols):
    """rows whose offsets are not 0 <= a <= b <= nnz, plus entries of the view's (clamped) range with a column outside the table"""
    a, b = rowptr[:n_rows].astype(np.int64), rowptr[1:n_rows + 1].astype(np.int64)
    bad = int(((a < 0) | (a > b) | (b > nnz)).sum())
    lo = min(max(int(rowptr[0]), 0), nnz)
    hi = min(max(int(rowptr[n_rows]), lo), nnz)
    c = col[lo:hi].astype(np.int64) - col_offset
    return bad + int(((c < 0) | (c >= n_cols)).sum())


EXTRACT_LENGTHS = [0, 1, 63, 64, 65, 300]


def draw_extract(seed=0):
    """a CSR of 18 rows with the lengths above three times over, float values with -0.0 and a NaN among them"""
    rng = np.random.default_rng(seed)
    cnt = np.array(EXTRACT_LENGTHS * 3)
    rowptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    nnz = int(rowptr[-1])
    col = rng.integers(0, 1000, nnz).astype(np.int32)
    val = rng.standard_normal(nnz).astype(np.float32)
    val[0], val[1] = -0.0, np.float32("nan")
    return rowptr, col, val


EXTRACT_SELECTIONS = {"every row": lambda n: np.arange(n), "every third row": lambda n: np.arange(0, n, 3),
                      "one row": lambda n: np.array([5]), "none": lambda n: np.zeros(0, np.int64)}


def extract_ref(rowptr, col, val, sel):
    cnt = rowptr[sel + 1] - rowptr[sel]
    out_rowptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    take = np.concatenate([np.arange(rowptr[s], rowptr[s + 1]) for s in sel] + [np.zeros(0, np.int64)]).astype(np.int64)
    return out_rowptr, col[take], val[take]


def check_extract(what, rowptr, col, val, sel, out_col, out_val):
    _, c, v = extract_ref(rowptr, col, val, sel)
    check_exact(f"{what} out_col", out_col, c)
    check_exact(f"{what} out_val", out_val, v)


# =============================================================================================== float measures (torch)
SCATTER_BWD_D = [1, 5, 64, 100, 130]


def draw_scatter_bwd(device, d, seed=0):
    """A sub-CSR of 40 rows over 90 source rows: empty rows, a 300-entry row (row 7), columns repeated within and across
    rows, source rows 80 .. 89 that no entry names; values of mixed sign with a large common part (as the SpMM cases); g_out
    a view one float into a wider table"""
    rng = np.random.default_rng(seed + d)
    cnt = rng.integers(0, 9, 40)
    cnt[[0, 3, 39]] = 0
    cnt[7] = 300
    rowptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    nnz = int(rowptr[-1])
    col = rng.integers(0, 80, nnz).astype(np.int32)
    col[rowptr[7]:rowptr[7] + 40] = 11                                            # a column 40 times within the long row
    gen = C.gen_for(device, 500 + seed + d)
    sign = torch.where(torch.rand(nnz, device=device, generator=gen) < 0.5, -1.0, 1.0)
    val = 1e3 * sign + torch.randn(nnz, device=device, generator=gen)
    g_table = torch.randn(40, d + 3, device=device, generator=gen)
    return NS(n_rows=40, n_x=90, d=d, rowptr=torch.from_numpy(rowptr).to(device), col=torch.from_numpy(col).to(device),
              val=val, g_table=g_table, g=g_table[:, 1:1 + d], unnamed=slice(80, 90), long_row=7,
              what=f"spmm scatter backward d {d}")


def scatter_bwd_eval(case, dtype, absolute=False, drop_last_of=None):
    """g_x = A^T g: g_x[col[j]] += val[j] g[row(j)].  absolute: |A|^T |g| (the scale).  drop_last_of: a planted fault."""
    rp = case.rowptr.long()
    rows = torch.repeat_interleave(torch.arange(case.n_rows, device=rp.device), rp[1:] - rp[:-1])
    terms = case.val.to(dtype)[:, None] * case.g.to(dtype)[rows]
    if drop_last_of is not None:
        terms[int(rp[drop_last_of + 1]) - 1] = 0
    if absolute:
        terms = terms.abs()
    return torch.zeros(case.n_x, case.d, dtype=dtype, device=rp.device).index_add_(0, case.col.long(), terms)


def scatter_bwd_table(case):
    """the destination: [n_x + PAD, d + 4] holding zeros where the kernel accumulates and the sentinel elsewhere"""
    t = torch.full((case.n_x + PAD, case.d + 4), SENTINEL, device=case.val.device)
    t[:case.n_x, 2:2 + case.d] = 0.0
    return t


def check_scatter_bwd(lines, case, table):
    got = table[:case.n_x, 2:2 + case.d]
    C.check_reduction(lines, case.what, got, scatter_bwd_eval(case, torch.float64), scatter_bwd_eval(case, torch.float64, True),
                      scatter_bwd_eval(case, torch.float32))
    assert float(got[case.unnamed].abs().max()) == 0.0, f"{case.what}: a row that no column names is not zero"
    guard = table.clone()
    guard[:case.n_x, 2:2 + case.d] = SENTINEL
    assert bool((guard == SENTINEL).all()), f"{case.what}: wrote outside the table's d columns"


def draw_scatter_add_perm(device, d, seed=0):
    """dst[idx[perm[i]]] += src[i]: 600 rows into 30 table rows through a permutation, src a view one float into a wider
    table, rows sharing a large common part of either sign; table rows 20 .. 29 are never named"""
    gen = C.gen_for(device, 900 + seed + d)
    rows, n = 600, 30
    idx = torch.randint(0, 20, (rows,), device=device, generator=gen)
    perm = torch.randperm(rows, device=device, generator=gen).int()
    sign = torch.where(torch.rand(rows, 1, device=device, generator=gen) < 0.5, -1.0, 1.0)
    src_table = 1e3 * sign + torch.randn(rows, d + 3, device=device, generator=gen)
    return NS(rows=rows, n_x=n, d=d, idx=idx, perm=perm, src_table=src_table, src=src_table[:, 1:1 + d], unnamed=slice(20, 30),
              what=f"scatter_add_rows perm d {d}")


def check_scatter_add_perm(lines, case, table):
    ids = case.idx[case.perm.long()]
    z = lambda dt: torch.zeros(case.n_x, case.d, dtype=dt, device=ids.device)
    want = z(torch.float64).index_add_(0, ids, case.src.double())
    scale = z(torch.float64).index_add_(0, ids, case.src.double().abs())
    ref32 = z(torch.float32).index_add_(0, ids, case.src)
    got = table[:case.n_x, 2:2 + case.d]
    C.check_reduction(lines, case.what, got, want, scale, ref32)
    assert float(got[case.unnamed].abs().max()) == 0.0, f"{case.what}: a row that no id names is not zero"
    guard = table.clone()
    guard[:case.n_x, 2:2 + case.d] = SENTINEL
    assert bool((guard == SENTINEL).all()), f"{case.what}: wrote outside the table's d columns"


# =============================================================================================== the sampler's stream
# A restatement of the comment above lkg_sample_kg_batch in include/literalkg_hip.h (NOT of the kernel source): 64-bit integer
# arithmetic with masks, dicts and sets for the positives, the structure's `order` for the order of the raw edges.
M64 = (1 << 64) - 1
MAX_TRIES = 256


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


class Stream:
    """value i = mix64(key + 0x9E3779B97F4A7C15 * i), i = 1, 2, ..., with key = mix64(seed ^ (0xD1B54A32D192ED03 * (group + 1)))"""

    def __init__(self, seed, group):
        self.key = mix64((seed ^ ((0xD1B54A32D192ED03 * (group + 1)) & M64)) & M64)
        self.ctr = 0

    def below(self, n):
        self.ctr += 1
        return mix64((self.key + 0x9E3779B97F4A7C15 * self.ctr) & M64) % n


def sampler_replica(seed, heads, neg_rate, h, t, r, order, candidate_first=False):
    """(out_h, out_r, out_pos_t, out_neg_t), int64[len(heads) * neg_rate].  h, t, r: the triples the structure was built from;
    order: sorted raw edge k is input triple order[k].  candidate_first: a planted fault for the host test (the group's first
    candidate draw taken before the positive draw)."""
    sh, st, sr = (np.asarray(x)[order].tolist() for x in (h, t, r))
    n_raw = len(sh)
    edges = {}
    for k, hh in enumerate(sh):
        edges.setdefault(hh, []).append(k)
    positives = set(zip(sh, st, sr))
    out = [[], [], [], []]
    for g, head in enumerate(int(x) for x in heads):
        own = edges.get(head)
        if not own:                                     # outside the id range or without a triple: the sentinel group, no draw
            for o, v in zip(out, (head, -1, -1, -1)):
                o.extend([v] * neg_rate)
            continue
        s = Stream(seed, g)
        early = st[s.below(n_raw)] if candidate_first else None
        e = own[s.below(len(own))]                      # the positive first: uniform over the head's raw triples
        rel, pos = sr[e], st[e]
        negs = []
        for k in range(neg_rate):
            for _ in range(MAX_TRIES):
                if early is not None:
                    cand, early = early, None
                else:
                    cand = st[s.below(n_raw)]           # the tail of a uniformly drawn raw triple
                if (head, cand, rel) not in positives and cand not in negs:
                    break
            negs.append(cand)                           # (after MAX_TRIES rejections: the last candidate, as it is)
        out[0].extend([head] * neg_rate)
        out[1].extend([rel] * neg_rate)
        out[2].extend([pos] * neg_rate)
        out[3].extend(negs)
    return tuple(np.array(o, np.int64) for o in out)


# case -> (graph, heads with an entity without triples and ids outside the range among them)
SAMPLER_CASES = {"no dups": ("plain", False), "dups": ("dups", False), "full head": ("full head", False),
                 "bad heads": ("plain", True)}


def sampler_graph(kind, seed=0):
    """(n_entities, h, t, r) of the three graphs of the sampler tests"""
    rng = np.random.default_rng(40 + seed)
    if kind == "full head":                             # head 0 holds every (tail, relation): every candidate is a positive
        t, r = np.meshgrid(np.arange(4), np.arange(2), indexing="ij")
        return 4, np.zeros(8, np.int64), t.reshape(-1).astype(np.int64), r.reshape(-1).astype(np.int64)
    n, e = 200, 1500
    pairs = rng.choice((n - 1) * n, e, replace=False)   # 1500 distinct (h, t) pairs; entity 199 is nobody's head
    h, t = pairs // n, pairs % n
    r = rng.integers(0, 3, e)
    if kind == "dups":                                  # plus 80 of the pairs under a second relation
        h, t, r = np.concatenate([h, h[:80]]), np.concatenate([t, t[:80]]), np.concatenate([r, (r[:80] + 1) % 3])
    sh = rng.permutation(h.shape[0])                    # (the input order is not the sorted one)
    return n, h[sh].astype(np.int64), t[sh].astype(np.int64), r[sh].astype(np.int64)


SAMPLER_SEEDS = [0, 1, 2 ** 63 + 5]
SAMPLER_RATES = [1, 5]
SAMPLER_GROUPS = 300


def sampler_heads(kind, bad, n, h, seed=0):
    if kind == "full head":
        return np.zeros(SAMPLER_GROUPS, np.int64)
    rng = np.random.default_rng(seed + 9)
    heads = rng.choice(np.unique(h), SAMPLER_GROUPS, replace=True).astype(np.int64)
    if bad:                                             # an entity without triples and ids outside the range, among good ones
        heads[[3, 100, 299, 17]] = [199, n, -1, 2 ** 40]
    return heads


def check_sampler(what, got, want):
    for name, a, b in zip(("h", "r", "pos_t", "neg_t"), got, want):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        neq = np.flatnonzero(a != b)
        assert neq.size == 0, f"{what}: out_{name} differs at {neq.size} of {a.size} places, first {neq[0]}: got {a[neq[0]]}, want {b[neq[0]]}"


def check_sampler_contract(out, k, h, t, r):
    """a group shares h, r and t+ (a positive triple); its negatives are distinct and filtered against the positives"""
    positives = set(zip(h.tolist(), r.tolist(), t.tolist()))
    bh, br, bp, bn = (np.asarray(x).reshape(-1, k) for x in out)
    assert (bh == bh[:, :1]).all() and (br == br[:, :1]).all() and (bp == bp[:, :1]).all()
    for hh, rr, pp, negs in zip(bh[:, 0].tolist(), br[:, 0].tolist(), bp[:, 0].tolist(), bn.tolist()):
        assert (hh, rr, pp) in positives
        assert len(set(negs)) == k
        assert all((hh, rr, x) not in positives for x in negs)


# =============================================================================================== Adam
ADAM_STEPS = [1, 2, 1000]
ADAM_BETAS = [(0.9, 0.999), (0.8, 0.95)]
ADAM_WD = [0.0, 0.01]
ADAM_LR, ADAM_EPS = 1e-3, 1e-8
ADAM_SMALL = [1, 3, 4, 7, 1027]
ADAM_BIG = 4 * 256 * 4096 + 4 * 300 + 3         # the 4096 x 256 grid's stride loop takes a second trip; a scalar tail of 3
ADAM_DRAWS = ["randn", "g 1e-20", "g 1e4", "v 0 g 0", "p 2^60", "p 2^-60", "mixed"]
SUB = 2.0 ** -149                               # float32's subnormal spacing: the absolute floor of a product that underflows


def draw_adam(device, n, draw, seed=0):
    """float32 p, g, m, v (v >= 0).  "mixed": element i takes draw i % 6, so every size holds every edge"""
    gen = C.gen_for(device, 700 + seed + n % 1000)
    p, g, m = (torch.randn(n, device=device, generator=gen) for _ in range(3))
    v = torch.randn(n, device=device, generator=gen) ** 2
    i = torch.arange(n, device=device)
    sel = (lambda k: i % 6 == k) if draw == "mixed" else (lambda k: torch.full((n,), ADAM_DRAWS[k] == draw, device=device))
    sgn = torch.where(g < 0, -1.0, 1.0)
    g = torch.where(sel(1), sgn * 1e-20, g)
    g = torch.where(sel(2), g * 1e4, g)
    g = torch.where(sel(3), torch.zeros_like(g), g)
    v = torch.where(sel(3), torch.zeros_like(v), v)
    p = torch.where(sel(4), p.sign() * 2.0 ** 60, p)
    p = torch.where(sel(5), p.sign() * 2.0 ** -60, p)
    return NS(n=n, p=p, g=g, m=m, v=v, what=f"adam n {n} {draw}")


def adam_hyper(betas, wd, step):
    """the hyper-parameters as float32 (what the C ABI carries), and the bias corrections in float64 from those"""
    lr, b1, b2, eps, wd = (A.f32(x) for x in (ADAM_LR, betas[0], betas[1], ADAM_EPS, wd))
    return NS(lr=lr, b1=b1, b2=b2, eps=eps, wd=wd, step=step, bc1=1.0 - b1 ** step, bc2s=math.sqrt(1.0 - b2 ** step))


def adam_f32(case, hp, eps_inside=False, no_bias_correction=False):
    """one step in float32, operation by operation without contraction (the host test's stand-in for the kernel).
    eps_inside / no_bias_correction: planted faults."""
    f = torch.float32
    t = lambda x: torch.tensor(x, dtype=f, device=case.p.device)
    bc1, bc2s = (t(1.0), t(1.0)) if no_bias_correction else (t(hp.bc1), t(hp.bc2s))
    gg = t(hp.wd) * case.p + case.g
    m = t(hp.b1) * case.m + (t(1.0) - t(hp.b1)) * gg
    v = t(hp.b2) * case.v + (t(1.0) - t(hp.b2)) * gg * gg
    den = torch.sqrt(v + t(hp.eps)) / bc2s if eps_inside else torch.sqrt(v) / bc2s + t(hp.eps)
    return case.p - (t(hp.lr) / bc1) * m / den, m, v


def check_adam(lines, case, hp, p1, m1, v1):
    """lkg_adam_step_f32 against Adam in float64 with the hyper-parameters rounded to float32 (torch's float32 Adam is not the
    stand-in: it forms 1 - beta in double, which at beta2 = 0.999 differs from a float32 coefficient by about 1e-5 relative).
    Counted roundings, each count the larger of the fused and the unfused contraction of the expression:
      gg = wd p + g                          2 (the product, the sum; fused 1) over |wd p| + |g|
      m' = b1 m + (1 - b1) gg                1 - b1, its product with gg, b1 m, the sum: 4, and gg's 2:  6
                                             over b1 |m| + (1 - b1)(|wd p| + |g|)
      v' = b2 v + (1 - b2) gg gg             1 - b2, two products, b2 v, the sum: 5, and gg's 2 twice:   9
                                             over b2 |v| + (1 - b2)(|wd p| + |g|)^2
      p' = p - (lr / bc1) m' / (sqrt(v') / bc2s + eps)   from the kernel's OWN m', v':
           bc1 and bc2s rounded to float32, lr / bc1, sqrt, its quotient, the sum with eps (all terms positive),
           the product with m', the quotient: 8 on the update; the difference: 1                        9
                                             over |p| + |update|
           (an exact count without slack: it takes the device's sqrtf and / as correctly rounded, which is hipcc's
           default -- -fhip-fp32-correctly-rounded-divide-sqrt -- and would have to grow if a build flag changed that)
    plus 2^-149 per operation whose result can be subnormal (the products of g = 1e-20, v' itself, the update)."""
    d = torch.float64
    p, g, m, v = (x.to(d) for x in (case.p, case.g, case.m, case.v))
    gg, sgg = hp.wd * p + g, (hp.wd * p).abs() + g.abs()
    C.check_units(lines, f"{case.what} m'", m1, hp.b1 * m + (1 - hp.b1) * gg, hp.b1 * m.abs() + (1 - hp.b1) * sgg, 6, extra=2 * SUB)
    C.check_units(lines, f"{case.what} v'", v1, hp.b2 * v + (1 - hp.b2) * gg * gg, hp.b2 * v.abs() + (1 - hp.b2) * sgg * sgg, 9,
                  extra=3 * SUB)
    assert bool((v1 >= 0).all()), f"{case.what}: a negative second moment"
    upd = (hp.lr / hp.bc1) * m1.to(d) / (torch.sqrt(v1.to(d)) / hp.bc2s + hp.eps)
    C.check_units(lines, f"{case.what} p'", p1, p - upd, p.abs() + upd.abs(), 9, extra=2 * SUB)
