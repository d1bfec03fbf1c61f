"""Reference, graph and checker shared by test_neighbors_host.py (numpy alone, planted faults) and test_neighbors_gpu.py
(lkg_csr_sample_rows on the device, through the SAME checker): the neighbour sample of include/literalkg_hip.h.

The draw, in numpy uint64 (arithmetic mod 2^64), for row i with d stored entries and fanout f:
    d <= f   every entry kept, col and val untouched
    d >  f   epoch_key = mix64(seed ^ (G * (draw + 1)));  row_key = mix64(epoch_key ^ (G * (i + 1)))
             value(j) = mix64(row_key + S * (j + 1));  kept: the f smallest under (value(j), j) -- a lexsort per row --
             written in ascending j;  rescale: val[j] * (float32(d) / float32(f)), one float32 division, one float32 product
``fault=`` plants the mistakes the checker has to catch; ``patch=(row, a, b)`` makes value(b) of that row equal value(a),
which is the only way to meet a tie.

The graph (600 rows): rows 0 .. 8 hold 0, 1, 3, 4, 5, 63, 64, 65 and 129 entries, row 9 is a hub of 5000, row 10 repeats its
columns, the last row holds 7, every other row 0 .. 10."""
import functools

import numpy as np

import index_cases as I
from negative_cases import mix64, mix64_int

G, S = np.uint64(0xD1B54A32D192ED03), np.uint64(0x9E3779B97F4A7C15)
N_ROWS, HUB, DUP = 600, 9, 10
LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 129, 5000)
FAULTS = ("hash order", "largest", "counter j", "scale f/d", "tie larger j", "short rescaled")


def _u64(x):
    return np.array([int(x) & ((1 << 64) - 1)], dtype=np.uint64)


def row_keys(seed, draw, rows):
    """uint64[len(rows)]: the key of every row under (seed, draw)"""
    epoch = mix64(_u64(seed) ^ (G * (_u64(draw) + np.uint64(1))))
    return mix64(epoch ^ (G * (np.asarray(rows).astype(np.uint64) + np.uint64(1))))


def values(row_key, d, fault=None):
    """uint64[d]: value(j) of one row"""
    j = np.arange(d, dtype=np.uint64)
    return mix64(np.uint64(row_key) + S * (j if fault == "counter j" else j + np.uint64(1)))


def value_int(seed, draw, row, j):
    """the same in Python integers"""
    m = (1 << 64) - 1
    epoch = mix64_int((seed ^ (0xD1B54A32D192ED03 * (draw + 1))) & m)
    key = mix64_int((epoch ^ (0xD1B54A32D192ED03 * (row + 1))) & m)
    return mix64_int((key + 0x9E3779B97F4A7C15 * (j + 1)) & m)


def kept(v, f, fault=None):
    """positions of the f smallest (value, j) of a row longer than f, in the order they are written"""
    j = np.arange(v.shape[0])
    order = np.lexsort((-j if fault == "tie larger j" else j, v))         # primary: the value; then the position
    if fault == "largest":
        return np.sort(order[-f:])
    return order[:f] if fault == "hash order" else np.sort(order[:f])


def scale_of(d, f, fault=None):
    return np.float32(f) / np.float32(d) if fault == "scale f/d" else np.float32(d) / np.float32(f)


def sample_ref(rowptr, col, val, rows, f, seed, draw, rescale, fault=None, patch=None):
    """(out_rowptr int32[len(rows) + 1], out_col int32[m], out_val float32[m])"""
    rows = np.asarray(rows, dtype=np.int64)
    keys = row_keys(seed, draw, rows)
    cols, vals, counts = [], [], []
    for i, key in zip(rows, keys):
        j0, d = int(rowptr[i]), int(rowptr[i + 1] - rowptr[i])
        c, x = col[j0:j0 + d], val[j0:j0 + d].astype(np.float32)
        if d > f:
            v = values(key, d, fault)
            if patch is not None and patch[0] == i:
                v[patch[2]] = v[patch[1]]
            keep = kept(v, f, fault)
            c, x = c[keep], x[keep]
            if rescale:
                x = (x * scale_of(d, f, fault)).astype(np.float32)
        elif fault == "short rescaled" and rescale and d:
            x = (x * scale_of(d, f)).astype(np.float32)
        cols.append(c)
        vals.append(x)
        counts.append(c.shape[0])
    out_rowptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return (out_rowptr, np.concatenate(cols + [np.zeros(0, np.int32)]).astype(np.int32),
            np.concatenate(vals + [np.zeros(0, np.float32)]).astype(np.float32))


def out_rowptr_of(rowptr, rows, f):
    """the caller's part: the exclusive scan of min(d, f)"""
    rows = np.asarray(rows, dtype=np.int64)
    deg = np.minimum(rowptr[rows + 1].astype(np.int64) - rowptr[rows], f)
    return np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)


def check_sample(what, rowptr, col, val, rows, f, seed, draw, rescale, got_col, got_val, patch=None):
    """got_col / got_val: the destinations, allocated longer than written and pre-filled with I.ISENT / I.SENTINEL.  Entry
    for entry against sample_ref, values by their bits, and nothing written behind the last entry."""
    out_rowptr, want_c, want_v = sample_ref(rowptr, col, val, rows, f, seed, draw, rescale, patch=patch)
    assert (out_rowptr == out_rowptr_of(rowptr, rows, f)).all(), what
    I.check_exact(f"{what}: col", got_col, want_c)
    I.check_exact(f"{what}: val", got_val, want_v)
    return out_rowptr, want_c, want_v


def padded(c, v):
    """a result laid out as a device run leaves it: the guard behind it still holding the sentinels"""
    return (np.concatenate([c, np.full(I.PAD, I.ISENT, np.int32)]).astype(np.int32),
            np.concatenate([v, np.full(I.PAD, I.SENTINEL, np.float32)]).astype(np.float32))


@functools.lru_cache(maxsize=None)
def graph():
    """(rowptr int32[601], col int32[nnz], val float32[nnz]); columns ascending inside a row but for row DUP"""
    rng = np.random.default_rng(20220)
    lengths = rng.integers(0, 11, N_ROWS)
    lengths[:len(LENGTHS)] = LENGTHS
    lengths[DUP] = 12
    lengths[-1] = 7
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    col = np.concatenate([np.sort(rng.choice(6000, int(n), replace=False)) for n in lengths]).astype(np.int32)
    col[rowptr[DUP]:rowptr[DUP + 1]] = np.repeat(np.array([3, 3, 17, 599], np.int32), 3)
    val = rng.standard_normal(col.shape[0]).astype(np.float32)
    val[val == 0] = np.float32(1.0)
    for a in (rowptr, col, val):
        a.setflags(write=False)
    return rowptr, col, val


SELECTIONS = {
    "all": lambda: np.arange(N_ROWS),
    "gaps": lambda: np.array([0, 2, 5, 7, 8, HUB, DUP, 11, 300, 301, 598, N_ROWS - 1]),
    "single": lambda: np.array([HUB]),
    "none": lambda: np.zeros(0, np.int64),
}
FANOUTS = (1, 2, 4, 64, 65, 100, 5000, 2 ** 31 - 1)
SEED_DRAWS = ((0, 0), (2022, 7), (2 ** 64 - 1, 2 ** 40 + 3))
