"""The host port of the dropout mask (dropout_cases.py): is it the hash lkg_common.h describes, is that hash a fair coin, and
can each check tell a wrong mask from a right one?  CPU only, fixed seeds, so every result is deterministic.

Statistics.  For d in {32, 64, 300}, p in {0.1, 0.25, 0.5} and rows 0 .. 4095 under every seed of ``SEEDS``, six families of
counts are held to the EXACT binomial law of an ideal mask, whose draws are independent and kept with probability
q = 1 - ceil(float32(p) 2^24) / 2^24:

  total      kept elements of the mask                          Binomial(4096 d, q)               one count per (d, p, seed)
  columns    kept elements of each column                       Binomial(4096, q)                 d counts
  rows       kept elements of each row                          Binomial(d, q)                    4096 counts
  row pairs  agreements of row r with row r + 1, split by the   Binomial(#pairs d, a)             2 counts
             parity of r (pairs that share no element: without
             the split the count is not binomial unless q = 1/2);
             agreements of rows r and r + 4096, r and r + 2^32  Binomial(4096 d, a)               2 counts
  col pairs  agreements of column c with column c + 1, by the   Binomial(4096 #pairs, a)          2 counts
             parity of c
  seed pairs agreements of the masks of seeds s and s + 1, and  Binomial(4096 d, a)               2 counts
             of s and s with bit 32 flipped (the high word)

with a = q^2 + (1 - q)^2.  No normal approximation anywhere: at d = 32 and q = 0.9 a row keeps all 32 elements with
probability 0.034, and the interval of a row count is [12, 32] -- the normal law would put 32 at 1.9 sigma and 12 at 9.9.

Bounds.  An ideal mask must fail ANY check of this file with probability below ALPHA = 1e-6.  ALPHA is split evenly over
eight families (the six above, the layer check of ``test_layers_draw_their_own_seeds``, one share unused), and a family's
share evenly over its counts (Bonferroni: P(some count outside) <= sum of P(this count outside)); a count's two-sided interval
[lo, hi] has P(X < lo) <= share / 2 and P(X > hi) <= share / 2 from the exact probability mass function
(``dropout_cases.binom_interval``).  With S = len(SEEDS) and the 9 (d, p) pairs that is 9 S counts for the totals, 1188 S for
the columns (3 (32 + 64 + 300) S), 36 864 S for the rows, 36 S for the row pairs and 18 S each for the column and seed pairs.
The layer check takes 1e-9 per pair of layers and runs on 3 pairs here.  The worst normal score of every family is printed
beside its bound; nothing is asserted on it.

Rejection.  Every measure is then shown a port with the fault it is there to catch, and must refuse it: the column term
dropped from the second hash (rows, column pairs), the seed's high word ignored (seed pairs), a row key taken from
row % 4096 or from the row's low word alone (row pairs at distance 4096 and 2^32), the (lane, register) -> column mapping
of the 16-byte kernels transposed (``check_forward_bits``), one seed reused for every layer (``check_layer_seeds``)."""
import math

import numpy as np
import pytest

import dropout_cases as D

WIDTHS, PS, N_ROWS = (32, 64, 300), (0.1, 0.25, 0.5), 4096
SEEDS = [0, 1, 2, 1 << 32, (1 << 32) + 1, (1 << 63) - 1] + \
        [int(s) for s in np.random.default_rng(20240607).integers(0, 1 << 63, 26, dtype=np.int64)]
ALPHA = 1e-6
FAMILIES = ("total", "columns", "rows", "row pairs", "col pairs", "seed pairs", "layers", "spare")
ROWS = np.arange(N_ROWS, dtype=np.uint64)
COLS = np.arange(max(WIDTHS))


def share(family, n_seeds=len(SEEDS)):
    """the part of ALPHA one count of ``family`` may spend"""
    per = {"total": 9, "columns": 3 * sum(WIDTHS), "rows": 9 * N_ROWS, "row pairs": 36, "col pairs": 18, "seed pairs": 18}[family]
    return ALPHA / len(FAMILIES) / (per * n_seeds)


def rejected(fn, *args, **kw):
    with pytest.raises(AssertionError):
        fn(*args, **kw)


def judge(draws_fn, seeds, families, n_seeds=len(SEEDS)):
    """Every count of ``families`` for a port's draws under ``seeds``; returns {family: worst normal score}.  The shares are
    always those of the full seed list: a planted fault is judged by the very bounds the port is."""
    worst = dict.fromkeys(families, 0.0)

    def up(f, v):
        worst[f] = max(worst[f], v)

    for s in seeds:
        u = draws_fn(s, ROWS, COLS)
        others = {}
        if "row pairs" in families:
            others["row pairs"] = [("rows r, r + 4096", draws_fn(s, ROWS + np.uint64(4096), COLS)),
                                   ("rows r, r + 2^32", draws_fn(s, ROWS + np.uint64(1 << 32), COLS))]
        if "seed pairs" in families:
            others["seed pairs"] = [("seeds s, s + 1", draws_fn(s + 1, ROWS, COLS)),
                                    ("seeds s, s ^ 2^32", draws_fn(s ^ (1 << 32), ROWS, COLS))]
        for p in PS:
            q, thr = D.keep_prob(p), np.uint32(D.threshold(p))
            m_all = u >= thr
            for d in WIDTHS:
                m = m_all[:, :d]
                what = f"seed {s} p {p} d {d}"
                if "total" in families:
                    up("total", D.check_count(f"{what}: kept", int(m.sum()), m.size, q, share("total", n_seeds)))
                if "columns" in families:
                    up("columns", D.check_counts(f"{what}: kept per column", m.sum(0), N_ROWS, q, share("columns", n_seeds)))
                if "rows" in families:
                    up("rows", D.check_counts(f"{what}: kept per row", m.sum(1), d, q, share("rows", n_seeds)))
                if "row pairs" in families:
                    up("row pairs", D.check_pair_agreement(f"{what}: rows r, r + 1", m, 0, q, share("row pairs", n_seeds)))
                if "col pairs" in families:
                    up("col pairs", D.check_pair_agreement(f"{what}: columns c, c + 1", m, 1, q, share("col pairs", n_seeds)))
                for f, lst in others.items():
                    for tag, u2 in lst:
                        up(f, D.check_mask_agreement(f"{what}: {tag}", m, (u2 >= thr)[:, :d], q, share(f, n_seeds)))
    return worst


# ------------------------------------------------------------------------------------------------- the port itself
def fmix32_int(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & D.M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & D.M32
    return h ^ (h >> 16)


def draw_int(seed, row, col):
    """the description of lkg_common.h once more, on Python integers (no numpy casting rule can touch it)"""
    inner = ((row & D.M32) * 0x9E3779B1 + (row >> 32) + (seed >> 32)) & D.M32
    key = fmix32_int((seed & D.M32) ^ fmix32_int(inner))
    return fmix32_int(key ^ ((col * 0x27D4EB2F + 0x165667B1) & D.M32)) >> 8


def test_port_agrees_with_plain_integer_arithmetic():
    assert [int(v) for v in D.fmix32(np.array([0, 1, 0xFFFFFFFF], dtype=np.uint32))] == [0, 0x514E28B7, 0x81F16F39]   # murmur3's own
    rng = np.random.default_rng(1)
    rows = np.concatenate([[0, 1, 4095, 4096, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 63) - 1],
                           rng.integers(0, 1 << 63, 20, dtype=np.int64)]).astype(np.uint64)
    cols = np.array([0, 1, 2, 3, 4, 31, 32, 63, 64, 255, 256, 299, 1023])
    for seed in SEEDS[:8] + [(1 << 64) - 1]:
        got = D.draws(seed, rows, cols)
        assert got.dtype == np.uint32 and got.shape == (rows.size, cols.size) and int(got.max()) < 1 << 24
        want = [[draw_int(seed, int(r), int(c)) for c in cols] for r in rows]
        assert got.tolist() == want, seed
    # both words of the seed and of the row reach the key
    base = D.draws(5, rows, cols)
    for other in (D.draws(5 + (1 << 32), rows, cols), D.draws(6, rows, cols), D.draws(5, rows + np.uint64(1 << 32), cols)):
        assert (other != base).mean() > 0.99


@pytest.mark.parametrize("p", [0.0, 0.1, 0.25, 0.5, 0.999, 2.0 ** -24, 1.0 - 2.0 ** -24])
def test_threshold_is_the_float32_compare(p):
    """keep <=> float32(draw) * 2^-24 >= float32(p), and the scale is float32 1 / (1 - p)"""
    thr = D.threshold(p)
    for u in {0, 1, max(thr - 1, 0), thr, min(thr + 1, (1 << 24) - 1), (1 << 24) - 1}:
        kernel = bool(np.float32(u) * np.float32(1.0 / 16777216.0) >= np.float32(p))
        assert kernel == (u >= thr), (p, u)
    assert D.keep_prob(p) == 1.0 - thr / 2.0 ** 24
    ik = D.inv_keep(p)
    assert ik.dtype == np.float32 and ik == np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    sc = D.scale(3, np.arange(64), np.arange(40), p)
    assert sc.dtype == np.float32 and set(np.unique(sc).tolist()) <= {0.0, float(ik)}
    if p == 0.0:
        assert (sc == 1.0).all()


def test_binomial_intervals_are_exact():
    """against sums of the probability mass function in exact rational arithmetic"""
    from fractions import Fraction
    for n, q, alpha in ((32, D.keep_prob(0.1), share("rows")), (32, 0.5, 1e-3), (64, D.keep_prob(0.25), 1e-9), (300, 0.75, 1e-6)):
        qf = Fraction(q)
        pmf = [Fraction(math.comb(n, k)) * qf ** k * (1 - qf) ** (n - k) for k in range(n + 1)]
        lo, hi = D.binom_interval(n, q, alpha)
        assert sum(pmf[:lo]) <= alpha / 2 < sum(pmf[:lo + 1]), (n, q, lo)
        assert sum(pmf[hi + 1:]) <= alpha / 2 < sum(pmf[hi:]), (n, q, hi)
    assert D.binom_interval(32, D.keep_prob(0.1), share("rows"))[1] == 32       # a row that keeps everything is ordinary
    # a large count: the interval sits where the normal law puts it, within a few counts
    n, q = 4096 * 300, D.keep_prob(0.25)
    lo, hi = D.binom_interval(n, q, 2e-9)
    z = 5.9978          # the normal quantile of 1e-9
    assert abs(lo - (n * q - z * math.sqrt(n * q * (1 - q)))) < 8 and abs(hi - (n * q + z * math.sqrt(n * q * (1 - q)))) < 8


# ------------------------------------------------------------------------------------------------- the hash is a fair coin
@pytest.fixture(scope="module")
def scores():
    return judge(D.draws, SEEDS, FAMILIES[:6])


@pytest.mark.parametrize("family", FAMILIES[:6])
def test_mask_statistics(scores, family):
    """(judge asserts every count; a failure of the module fixture shows up under each family)"""
    n = {"total": 4096 * 300, "columns": 4096, "rows": 32, "row pairs": 4096 * 300, "col pairs": 4096 * 150,
         "seed pairs": 4096 * 300}[family]
    lo, hi = D.binom_interval(n, D.keep_prob(0.1) if family in FAMILIES[:3] else D.agree_prob(D.keep_prob(0.1)), share(family))
    print(f"{family}: worst normal score {scores[family]:.2f}; interval at p = 0.1 over {n}: [{lo}, {hi}]")
    assert scores[family] > 0.0


# ------------------------------------------------------------------------------------------------- planted faults
def no_column_term(seed, rows, cols):
    return np.broadcast_to(D.fmix32(D.row_key(seed, rows) ^ D.COL_ADD)[:, None] >> np.uint32(8), (len(rows), len(cols)))


def low_seed_only(seed, rows, cols):
    return D.draws(seed & D.M32, rows, cols)


def row_mod_4096(seed, rows, cols):
    return D.draws(seed, np.asarray(rows, dtype=np.uint64) % np.uint64(4096), cols)


def low_row_only(seed, rows, cols):
    return D.draws(seed, np.asarray(rows, dtype=np.uint64) & np.uint64(D.M32), cols)


def same_draw_every_row(seed, rows, cols):
    return np.broadcast_to(D.draws(seed, [0], cols), (len(rows), len(cols)))


def biased(seed, rows, cols):
    """a coin that keeps 1 % too often (the top draws folded down)"""
    return np.minimum(D.draws(seed, rows, cols) + np.uint32(1 << 24) // np.uint32(100), np.uint32((1 << 24) - 1))


FEW = SEEDS[:3] + SEEDS[-2:]


def test_the_faulty_ports_are_what_they_claim():
    r, c = ROWS[:64], COLS[:40]
    assert np.array_equal(low_seed_only(7, r, c), D.draws(7, r, c)) and np.array_equal(row_mod_4096(7, r, c), D.draws(7, r, c))
    assert np.array_equal(low_row_only(7, r, c), D.draws(7, r, c))


@pytest.mark.parametrize("fault,family", [
    (no_column_term, "rows"), (no_column_term, "col pairs"), (low_seed_only, "seed pairs"), (row_mod_4096, "row pairs"),
    (low_row_only, "row pairs"), (same_draw_every_row, "columns"), (same_draw_every_row, "row pairs"), (biased, "total")],
    ids=lambda v: v.__name__ if callable(v) else v.replace(" ", "_"))
def test_each_measure_rejects_its_fault(fault, family):
    rejected(judge, fault, FEW, (family,))
    judge(D.draws, FEW, (family,))          # ... and passes the port on the same seeds, by the same bounds


def test_the_faults_pass_the_measures_that_cannot_see_them():
    """a fault is refused by ITS measure, not by accident: the seed's high word is invisible to everything under one seed"""
    judge(low_seed_only, FEW, ("total", "columns", "rows", "row pairs", "col pairs"))
    judge(row_mod_4096, FEW, ("total", "columns", "rows", "col pairs", "seed pairs"))


# ---- the column a (lane, register) pair holds in the 16-byte row kernels: lane l keeps elements [(l + 64 i) 4, + 4), i < CPL
def column_of(lane, k, w=4):
    return (lane + 64 * (k // w)) * w + k % w


def column_of_transposed(lane, k, cpl, w=4):
    """the fault: a lane's chunks taken as consecutive (lane-major) -- right for one chunk per lane, wrong beyond"""
    return (lane * cpl + k // w) * w + k % w


@pytest.mark.parametrize("d,cpl", [(256, 1), (512, 2), (516, 3), (1024, 4)])
def test_forward_bits_reject_a_transposed_column_mapping(d, cpl):
    rng = np.random.default_rng(d)
    n, p, seed = 37, 0.5, (1 << 40) + 9
    y0 = rng.standard_normal((n, d)).astype(np.float32)
    sc = D.scale(seed, np.arange(n), np.arange(d), p)
    D.check_forward_bits("port", y0 * sc, y0, sc)
    wrong_cols = np.zeros(d, dtype=np.int64)
    for lane in range(64):
        for k in range(4 * cpl):
            e = column_of(lane, k)
            if e < d:
                wrong_cols[e] = column_of_transposed(lane, k, cpl)
    sc_wrong = D.scale(seed, np.arange(n), wrong_cols, p)
    if cpl == 1:
        assert np.array_equal(wrong_cols, np.arange(d))         # (one chunk per lane: the two mappings are the same)
        D.check_forward_bits("one chunk", y0 * sc_wrong, y0, sc)
    else:
        rejected(D.check_forward_bits, "transposed", y0 * sc_wrong, y0, sc)
    # ... a mask drawn on row r + 1, a scale rounded differently, a lost sign of zero
    rejected(D.check_forward_bits, "next row", y0 * D.scale(seed, np.arange(1, n + 1), np.arange(d), p), y0, sc)
    off = np.nextafter(y0 * sc, np.float32(np.inf))
    off[sc == 0] = (y0 * sc)[sc == 0]
    rejected(D.check_forward_bits, "one ulp off", off, y0, sc)
    D.check_forward_bits("one ulp off, 1 ulp allowed", off, y0, sc, max_ulp=1)
    rejected(D.check_forward_bits, "two ulps off", np.nextafter(off, np.float32(np.inf)), y0, sc, max_ulp=1)
    rejected(D.check_forward_bits, "sign of zero", np.abs(y0 * sc) * np.sign(y0 * sc), y0, sc)


def test_layers_draw_their_own_seeds():
    n, p, widths = 600, 0.1, (64, 32, 32)
    rows, cols = np.arange(n), [np.arange(w) for w in widths]
    seeds = [11, (1 << 62) + 5, 12]
    obs = [D.scale(s, rows, c, p) for s, c in zip(seeds, cols)]
    D.check_layer_seeds("three layers", seeds, obs, rows, cols, p)
    # one seed for every layer
    rejected(D.check_layer_seeds, "one seed", [11, 11, 11], [D.scale(11, rows, c, p) for c in cols], rows, cols, p)
    # distinct seeds recorded, but the layers' masks are one mask
    rejected(D.check_layer_seeds, "one mask", seeds, [D.scale(11, rows, c, p) for c in cols], rows, cols, p)
    # seeds that differ in the high word only, under a port that ignores it: the masks agree everywhere
    hi = [11, 11 + (1 << 32)]
    assert np.array_equal(low_seed_only(hi[0], rows, cols[1]), low_seed_only(hi[1], rows, cols[1]))
    D.check_layer_seeds("high words", hi, [None, None], rows, cols[:2], p)
