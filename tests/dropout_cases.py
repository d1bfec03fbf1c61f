"""The message-dropout mask on the host, and the checks that hold the kernels and the model to it.  numpy only.

The mask is a pure function of (seed, row, column), written here from its description in csrc/lkg_common.h with
uint32 wrap-around arithmetic (nothing of the package is imported):

    fmix32(h)          h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h *= 0xC2B2AE35;  h ^= h >> 16     (murmur3's finaliser)
    row_key(seed, row) fmix32(lo(seed) ^ fmix32(lo(row) * 0x9E3779B1 + hi(row) + hi(seed)))                lo / hi: 32-bit words
    draw(seed, r, c)   fmix32(row_key(seed, r) ^ (c * 0x27D4EB2F + 0x165667B1)) >> 8                      24 bits
    keep(seed, r, c)   float32(draw) * 2^-24 >= float32(p)       <=>   draw >= ceil(float32(p) * 2^24)
    scale              keep ? float32(1) / (float32(1) - float32(p)) : 0

so a draw is kept with probability exactly  q = 1 - ceil(float32(p) 2^24) / 2^24  under an ideal hash.

Three families of checks live here, shared by test_dropout_mask_host.py (the port and planted faults on the CPU),
test_dropout_mask_gpu.py (every kernel that regenerates the mask) and test_dropout_model_gpu.py (a training step):

  * ``check_count(s)`` / ``check_pair_agreement`` / ``check_mask_agreement``: counts of a mask against the EXACT binomial
    law of independent draws (``binom_interval``);
  * ``check_forward_bits``: a masked forward is the unmasked one times the port's scale, bit for bit;
  * ``check_layer_seeds``: the layers of one forward draw distinct seeds and masks that differ as the port says."""
import math

import numpy as np

M32 = 0xFFFFFFFF
C1, C2 = np.uint32(0x85EBCA6B), np.uint32(0xC2B2AE35)
ROW_MUL, COL_MUL, COL_ADD = np.uint32(0x9E3779B1), np.uint32(0x27D4EB2F), np.uint32(0x165667B1)


def fmix32(h):
    """murmur3's 32-bit finaliser on a uint32 array (array arithmetic wraps modulo 2^32)"""
    h = np.asarray(h, dtype=np.uint32)
    h = h ^ (h >> np.uint32(16))
    h = h * C1
    h = h ^ (h >> np.uint32(13))
    h = h * C2
    return h ^ (h >> np.uint32(16))


def _words(x):
    """(low, high) 32-bit words of non-negative integers below 2^64, as uint32 arrays"""
    x = np.atleast_1d(np.asarray(x, dtype=np.uint64))
    return (x & np.uint64(M32)).astype(np.uint32), (x >> np.uint64(32)).astype(np.uint32)


def row_key(seed, rows):
    """uint32 key per row; seed: a Python int below 2^64, rows: integers below 2^64"""
    seed = int(seed)
    assert 0 <= seed < 1 << 64
    lo, hi = _words(rows)
    inner = lo * ROW_MUL + hi + np.uint32(seed >> 32)
    return fmix32(np.uint32(seed & M32) ^ fmix32(inner))


def draws(seed, rows, cols):
    """the 24-bit draw of every (row, column): uint32 [len(rows), len(cols)]"""
    ck = np.atleast_1d(np.asarray(cols, dtype=np.uint64)).astype(np.uint32) * COL_MUL + COL_ADD
    return fmix32(row_key(seed, rows)[:, None] ^ ck[None, :]) >> np.uint32(8)


def threshold(p):
    """smallest draw that is kept: float32(draw) 2^-24 >= float32(p)  (a 24-bit draw and its product with 2^-24 are exact)"""
    return math.ceil(float(np.float32(p)) * 16777216.0)


def keep_prob(p):
    return 1.0 - threshold(p) / 16777216.0


def inv_keep(p):
    """the float32 value 1.f / (1.f - p)"""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def keep(seed, rows, cols, p, draws_fn=draws):
    return draws_fn(seed, rows, cols) >= np.uint32(threshold(p))


def scale(seed, rows, cols, p, draws_fn=draws):
    """float32 [len(rows), len(cols)]: inv_keep where kept, 0 where dropped"""
    return np.where(keep(seed, rows, cols, p, draws_fn), inv_keep(p), np.float32(0.0)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the exact binomial law
def _log_pmf_window(n, q, lo, hi):
    """log P(X = k) for k in [lo, hi]: log-gamma at k = lo, then the ratios P(k + 1) / P(k) = (n - k) / (k + 1) * q / (1 - q)
    summed in float64 (some 1e5 terms at most: a relative error near 1e-10 on a probability, nothing to an integer bound)"""
    k = np.arange(lo, hi + 1, dtype=np.float64)
    first = (math.lgamma(n + 1.0) - math.lgamma(lo + 1.0) - math.lgamma(n - lo + 1.0) + lo * math.log(q)
             + (n - lo) * math.log1p(-q))
    step = np.log(n - k[:-1]) - np.log(k[:-1] + 1.0) + (math.log(q) - math.log1p(-q))
    return first + np.concatenate([[0.0], np.cumsum(step)])


_INTERVALS = {}


def binom_interval(n, q, alpha):
    """[lo, hi] with P(X < lo) <= alpha / 2 and P(X > hi) <= alpha / 2 for X ~ Binomial(n, q), from the exact probability
    mass function, each tail summed from its far end inwards.  The sums run over a window of t = 60 sigma + 60 round the
    mean: by Bernstein's inequality, P(|X - n q| >= t) <= 2 exp(-t^2 / (2 (sigma^2 + t / 3))) <= 2 exp(-85), which is what
    the window leaves out (nothing where it reaches 0 or n)."""
    key = (n, q, alpha)
    if key not in _INTERVALS:
        assert 0.0 < q < 1.0 and n > 0
        w = int(60 * math.sqrt(n * q * (1 - q))) + 60
        a, b = max(0, int(n * q) - w), min(n, int(n * q) + w)
        pmf = np.exp(_log_pmf_window(n, q, a, b))
        below = np.cumsum(pmf)                  # P(a <= X <= k)
        above = np.cumsum(pmf[::-1])[::-1]      # P(k <= X <= b)
        lo = a + int(np.searchsorted(below, alpha / 2, side="right"))         # first k with P(X <= k) > alpha / 2
        hi = b - int(np.searchsorted(above[::-1], alpha / 2, side="right"))   # last k with P(X >= k) > alpha / 2
        _INTERVALS[key] = (lo, hi)
    return _INTERVALS[key]


def normal_score(x, n, q):
    """(x - n q) / sqrt(n q (1 - q)): only printed, never asserted on"""
    return (x - n * q) / math.sqrt(n * q * (1 - q))


def agree_prob(q):
    """probability that two independent draws are both kept or both dropped"""
    return q * q + (1 - q) * (1 - q)


def check_count(what, x, n, q, alpha):
    """one count against its exact two-sided binomial interval; returns its normal score"""
    lo, hi = binom_interval(n, q, alpha)
    assert lo <= x <= hi, f"{what}: {x} of {n} outside [{lo}, {hi}] (q = {q:.6f}, normal score {normal_score(x, n, q):+.2f})"
    return abs(normal_score(x, n, q))


def check_counts(what, xs, n, q, alpha):
    """every count of an array against the same interval; returns the worst normal score"""
    xs = np.asarray(xs)
    lo, hi = binom_interval(n, q, alpha)
    bad = np.flatnonzero((xs < lo) | (xs > hi))
    assert bad.size == 0, (f"{what}: {bad.size} of {xs.size} counts outside [{lo}, {hi}] of {n} (q = {q:.6f}); first at "
                           f"{int(bad[0])}: {int(xs[bad[0]])}")
    return float(np.abs(normal_score(xs.astype(np.float64), n, q)).max())


def check_pair_agreement(what, m, axis, q, alpha):
    """Neighbours along ``axis`` of a boolean mask agree as independent draws do.  The agreements of OVERLAPPING pairs
    (i, i + 1), (i + 1, i + 2) are correlated unless q = 1/2, so the pairs are split by the parity of i: within one
    parity they share no element, and their agreement count is exactly Binomial(#pairs, q^2 + (1 - q)^2)."""
    m = np.moveaxis(m, axis, 0)
    same = m[:-1] == m[1:]
    worst = 0.0
    for par in (0, 1):
        s = same[par::2]
        worst = max(worst, check_count(f"{what}, pairs starting at {'even' if par == 0 else 'odd'} positions", int(s.sum()), s.size,
                                       agree_prob(q), alpha))
    return worst


def check_mask_agreement(what, m1, m2, q, alpha):
    """two masks of independent draws agree on Binomial(size, q^2 + (1 - q)^2) elements"""
    assert m1.shape == m2.shape
    return check_count(what, int((m1 == m2).sum()), m1.size, agree_prob(q), alpha)


# ------------------------------------------------------------------------------------------------ exact checks of a kernel
def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def check_forward_bits(what, y_p, y_0, scale_port, max_ulp=0):
    """y_p = y_0 * scale, one float32 multiply: the same bits (a dropped element keeps the sign of y_0 on its zero).
    max_ulp: the distance allowed where an entry cannot keep the bits (stated at the call)."""
    y_p, y_0 = np.ascontiguousarray(y_p, dtype=np.float32), np.ascontiguousarray(y_0, dtype=np.float32)
    assert y_p.shape == y_0.shape == scale_port.shape, (what, y_p.shape, y_0.shape, scale_port.shape)
    assert np.isfinite(y_0).all(), f"{what}: the unmasked output is not finite"
    want = y_0 * scale_port.astype(np.float32)
    gone = (scale_port == 0) != (y_p == 0)
    gone &= y_0 != 0
    assert not gone.any(), (f"{what}: {int(gone.sum())} elements kept / dropped against the port; first at "
                            f"{tuple(int(i) for i in np.argwhere(gone)[0])}")
    if max_ulp == 0:
        bad = bits(y_p) != bits(want)
    else:
        k = lambda v: np.where(bits(v) >> 31 == 1, -(bits(v) & 0x7FFFFFFF).astype(np.int64), (bits(v) & 0x7FFFFFFF).astype(np.int64))
        bad = np.abs(k(y_p) - k(want)) > max_ulp
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} elements differ from y_0 * scale; first at {i}: got {y_p[i]!r}, "
                             f"want {want[i]!r} (y_0 {y_0[i]!r}, scale {scale_port[i]!r})")


def check_layer_seeds(what, seeds, observed, rows, cols, p, alpha=1e-9):
    """The layers of one forward: distinct seeds, each layer's observed scale the port's for ITS seed, and the masks of any
    two layers agreeing as independent draws do.  observed: float32 [len(rows), len(cols)] per layer, or None to skip the
    comparison for that layer."""
    assert len(set(seeds)) == len(seeds), f"{what}: a seed is used by more than one layer: {seeds}"
    q = keep_prob(p)
    masks = []
    for k, (s, obs) in enumerate(zip(seeds, observed)):
        want = scale(s, rows, cols[k], p)
        if obs is not None:
            assert np.array_equal(bits(obs), bits(want)), f"{what}: layer {k}'s scale is not the port's for seed {s}"
        masks.append(want != 0)
    for i in range(len(masks)):
        for j in range(i + 1, len(masks)):
            w = min(masks[i].shape[1], masks[j].shape[1])
            check_mask_agreement(f"{what}: layers {i} and {j}", masks[i][:, :w], masks[j][:, :w], q, alpha)
