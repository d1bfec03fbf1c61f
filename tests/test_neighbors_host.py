"""CPU tier of neighbour sampling (include/literalkg_hip.h, literalkg_amd/pruned.py; the device tiers are
test_neighbors_gpu.py and test_neighbors_model_gpu.py): the entry point is declared and bound, the reference
of neighbor_cases.py is a usable sampler (every entry of a row kept equally often, the rescaled sum unbiased), the numpy
form agrees with Python integers, and the checker rejects every planted fault."""
import os

import numpy as np
import pytest

import index_cases as I
import neighbor_cases as NC

NAMES = ["lkg_csr_sample_rows"]


def test_the_entry_point_is_declared_and_bound_and_the_package_exports_the_sampler():
    import __graft_entry__ as ge
    ge.build()
    from literalkg_amd import _native, build
    from wide_cases import prototypes
    assert "lkg_neighbors.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "lkg_neighbors.hip"))
    assert set(NAMES) <= set(_native.PROTOTYPES) and set(NAMES) <= set(prototypes())
    import literalkg_amd as L
    from literalkg_amd import pruned
    assert "sample_neighbors" in L.__all__ and L.sample_neighbors is pruned.sample_neighbors


def test_fanout_must_be_a_positive_int():
    from literalkg_amd import pruned
    assert pruned.checked_fanout(1) == 1 and pruned.checked_fanout(2 ** 31 - 1) == 2 ** 31 - 1
    for bad in (0, -1, True, False, 4.0, "4", None, 2 ** 31):
        with pytest.raises(ValueError):
            pruned.checked_fanout(bad)


def test_numpy_values_are_the_integer_ones():
    for seed, draw in NC.SEED_DRAWS + ((5, 3),):
        for row in (0, 1, 599, 2 ** 31 - 2):
            v = NC.values(NC.row_keys(seed, draw, [row])[0], 70)
            assert [int(x) for x in v] == [NC.value_int(seed, draw, row, j) for j in range(70)]
    assert NC.value_int(0, 0, 0, 0) != NC.value_int(0, 1, 0, 0) != NC.value_int(1, 0, 0, 0)


# ----------------------------------------------------------------------------- a usable sampler
D, F, T = 257, 16, 20_000


def keep_counts(keys):
    """how often each of the D positions is kept over the rows / draws that `keys` stand for"""
    j = np.arange(1, D + 1, dtype=np.uint64)
    v = NC.mix64(keys[:, None] + NC.S * j[None, :])
    keep = np.argsort(v, axis=1, kind="stable")[:, :F]
    return np.bincount(keep.reshape(-1), minlength=D), keep


def chi_square(counts, n):
    e = n * F / D
    return float(((counts - e) ** 2 / e).sum())


@pytest.mark.parametrize("case", ["seed 0", "seed 1", "seed 2022", "rows"])
def test_every_entry_is_kept_equally_often(case):
    """chi-square of the per-entry keep counts against T f / d.  Under sampling without replacement its mean is
    d (1 - f / d) = 241 and its standard deviation about 21: the bound is 241 +- 4 standard deviations."""
    if case == "rows":                                   # 20 000 different rows, one draw
        keys = NC.row_keys(5, 3, np.arange(T))
    else:                                                # one row, 20 000 draws
        seed = int(case.split()[1])
        keys = np.concatenate([NC.row_keys(seed, draw, [0]) for draw in range(T)])
    counts, keep = keep_counts(keys)
    assert counts.sum() == T * F and (np.sort(keep[0]) == NC.kept(NC.values(keys[0], D), F)).all()
    chi = chi_square(counts, T)
    print(f"{case}: chi-square {chi:.1f}")
    assert 156.0 <= chi <= 326.0, chi


def test_the_rescaled_sum_is_unbiased():
    """the mean over the draws of the rescaled row sum equals the full row sum within 4 standard errors of that mean"""
    rng = np.random.default_rng(7)
    val = rng.standard_normal(D).astype(np.float32)
    keys = np.concatenate([NC.row_keys(0, draw, [3]) for draw in range(T)])
    _, keep = keep_counts(keys)
    scaled = (val[keep] * NC.scale_of(D, F)).astype(np.float32)
    sums = scaled.astype(np.float64).sum(axis=1)
    full, mean, se = float(val.astype(np.float64).sum()), float(sums.mean()), float(sums.std(ddof=1) / np.sqrt(T))
    print(f"full {full:.6f} mean {mean:.6f} standard error {se:.6f}")
    assert abs(mean - full) <= 4 * se, (mean, full, se)


# ----------------------------------------------------------------------------- the reference and the checker
def test_the_reference_keeps_short_rows_and_csr_order():
    rowptr, col, val = NC.graph()
    rows = NC.SELECTIONS["all"]()
    lengths = np.diff(rowptr)
    assert tuple(lengths[:10]) == NC.LENGTHS and lengths[-1] == 7 and lengths[NC.DUP] == 12
    for f in NC.FANOUTS:
        orp, c, v = NC.sample_ref(rowptr, col, val, rows, f, 2022, 7, True)
        assert (np.diff(orp) == np.minimum(lengths, f)).all()
        for i in rows:
            got_c, got_v = c[orp[i]:orp[i + 1]], v[orp[i]:orp[i + 1]]
            src_c, src_v = col[rowptr[i]:rowptr[i + 1]], val[rowptr[i]:rowptr[i + 1]]
            if lengths[i] <= f:
                assert (got_c == src_c).all() and (I.bits(got_v) == I.bits(src_v)).all()
            elif i != NC.DUP:                                 # (ascending unique columns: CSR order is column order)
                assert (np.diff(got_c) > 0).all() and np.isin(got_c, src_c).all()
    e_orp, e_c, e_v = I.extract_ref(rowptr, col, val, rows)
    orp, c, v = NC.sample_ref(rowptr, col, val, rows, 5000, 0, 0, True)
    assert (orp == e_orp).all() and (c == e_c).all() and (I.bits(v) == I.bits(e_v)).all()


@pytest.mark.parametrize("fault", NC.FAULTS)
def test_the_checker_rejects_a_planted_fault(fault):
    rowptr, col, val = NC.graph()
    rows = NC.SELECTIONS["gaps"]()
    f, seed, draw = 4, 2022, 7
    patch = None
    if fault == "tie larger j":                           # the hub's 4th and 5th smallest values made equal
        v = NC.values(NC.row_keys(seed, draw, [NC.HUB])[0], 5000)
        order = np.lexsort((np.arange(5000), v))
        a, b = sorted((int(order[3]), int(order[4])))
        patch = (NC.HUB, a, b)
    _, c, v = NC.sample_ref(rowptr, col, val, rows, f, seed, draw, True, patch=patch)
    NC.check_sample("sound", rowptr, col, val, rows, f, seed, draw, True, *NC.padded(c, v), patch=patch)
    _, c, v = NC.sample_ref(rowptr, col, val, rows, f, seed, draw, True, fault=fault, patch=patch)
    with pytest.raises(AssertionError):
        NC.check_sample(fault, rowptr, col, val, rows, f, seed, draw, True, *NC.padded(c, v), patch=patch)


def test_the_checker_rejects_a_store_behind_the_result():
    rowptr, col, val = NC.graph()
    rows = NC.SELECTIONS["single"]()
    _, c, v = NC.sample_ref(rowptr, col, val, rows, 4, 0, 0, False)
    pc, pv = NC.padded(c, v)
    pv[-1] = 0.0
    with pytest.raises(AssertionError, match="wrote behind"):
        NC.check_sample("guard", rowptr, col, val, rows, 4, 0, 0, False, pc, pv)
