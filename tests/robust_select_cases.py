"""Crafted values for the robust reweighting's select and weight kernels (csrc/robust.hpp), and their reference.  No
device: tests/test_robust_select_cpu.py checks the generators, tests/test_robust_select_gpu.py feeds them to
dbat_hip_debug_robust_from_s.

The select is six radix passes over the IEEE bit patterns of s, of BITS digits at SHIFT from the top.  Every generator
is seeded, returns n float64 values that are finite, below 2^1022 (the sum of two is finite) and have the sign bit
clear, and shuffles them."""
import numpy as np

from dbat_amd.driver import robust_weight_fn
from test_robust_cpu import oracle_scale

SHIFT = (53, 42, 31, 20, 10, 0)             # RSEL_SHIFT
BITS = (11, 11, 11, 11, 10, 10)             # RSEL_BITS
B = int(np.array([1.0]).view(np.uint64)[0])  # the bit pattern of 1.0
SIZES = (1799, 1800, 32000)


def _rng(*key):
    return np.random.default_rng([20240611, *key])


def _from_bits(bits, rng):
    s = np.asarray(bits, np.uint64).view(np.float64).copy()
    rng.shuffle(s)
    return s


def split(n, p):
    """The lower half is 1.0, the rest one unit of pass p's digit above: for even n the two middle order statistics
    part exactly in pass p; for odd n there is one target."""
    bits = np.full(n, B, np.uint64)
    bits[n // 2:] = B + (1 << SHIFT[p])
    return _from_bits(bits, _rng(1, n, p))


def cluster(n, p):
    """Random digits of pass p on a common pattern (1.0; for p = 0 the pattern 0 with digits below 1022, which keeps
    the values below 2^1022): pass p sees a crowded histogram with ties, every other pass a single bucket -- but for
    p = 1, whose digit reaches bit 52, set in 1.0: the digits from 1024 carry, and pass 0 sees two buckets."""
    rng = _rng(2, n, p)
    digit = rng.integers(0, 1022 if p == 0 else 1 << BITS[p], n).astype(np.uint64)
    return _from_bits((0 if p == 0 else B) + (digit << np.uint64(SHIFT[p])), rng)


def crowded(n, p):
    """Buckets that stay crowded down to the last digit, with no digit 0 to fall back on: one seeded non-zero digit in
    every pass above p, one of three seeded non-zero digits in pass p and in every pass below it -- 3^(6 - p) distinct
    values, so the targets' bucket holds several values in every pass and every pass has counts below it to take off
    the rank.  (split and cluster leave the digits of the passes after p at 0, which is also what a pass that finds no
    bucket leaves: a rank carried wrongly out of pass p goes unnoticed there.)"""
    rng = _rng(7, n, p)
    bits = np.zeros(n, np.uint64)
    for q, (sh, nb) in enumerate(zip(SHIFT, BITS)):
        hi = 1022 if q == 0 else 1 << nb            # (pass 0: sign bit clear, below 2^1022)
        lo = 256 if q == 0 else 1                   # (... and no subnormals: the values stay of comparable size)
        alphabet = rng.choice(np.arange(lo, hi), 3 if q >= p else 1, replace=False).astype(np.uint64)
        bits |= alphabet[rng.integers(0, alphabet.size, n)] << np.uint64(sh)
    return _from_bits(bits, rng)


def all_equal(n, v):
    return np.full(n, float(v))


def zeros_majority(n):
    """n // 2 + 1 zeros, the rest positive: the median is 0."""
    rng = _rng(3, n)
    s = np.zeros(n)
    s[n // 2 + 1:] = rng.rayleigh(1.0, n - n // 2 - 1) + 0.01
    rng.shuffle(s)
    return s


def zeros_half(n):
    """n / 2 zeros and n / 2 times the smallest subnormal: the median (0 + 5e-324) / 2 rounds to 0."""
    assert n % 2 == 0
    s = np.zeros(n)
    s[n // 2:] = 5e-324
    _rng(4, n).shuffle(s)
    return s


def extremes(n):
    """Zeros, 5e-324, subnormals, 1.0 and normal values from 2^-1021 up to 2^1021, mixed in equal shares."""
    rng = _rng(5, n)
    kind = rng.integers(0, 5, n)
    sub = rng.integers(1, 1 << 52, n).astype(np.uint64).view(np.float64)
    big = np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(-1021, 1021, n))
    s = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [0.0, 5e-324, sub, 1.0], big)
    s[0] = 2.0 ** 1021
    rng.shuffle(s)
    return s


def rayleigh(n):
    """Continuous, all distinct: the ordinary case."""
    return _rng(6, n).rayleigh(1.0, n)


def cases(n):
    """[(id, s)] of every generator at n values (zeros_half: even n only)."""
    out = [('split%d' % p, split(n, p)) for p in range(6)] + [('cluster%d' % p, cluster(n, p)) for p in range(6)]
    out += [('crowded%d' % p, crowded(n, p)) for p in range(6)]
    out += [('all-one', all_equal(n, 1.0)), ('all-zero', all_equal(n, 0.0)), ('zeros-majority', zeros_majority(n))]
    if n % 2 == 0:
        out.append(('zeros-half', zeros_half(n)))
    return out + [('extremes', extremes(n)), ('rayleigh', rayleigh(n))]


def case_ids(n):
    return ['%s%d' % (g, p) for g in ('split', 'cluster', 'crowded') for p in range(6)] + ['all-one', 'all-zero', 'zeros-majority'] + \
        (['zeros-half'] if n % 2 == 0 else []) + ['extremes', 'rayleigh']


def ref_median(s):
    """The device's formula: the two middle order statistics of the bit patterns, (a + b) / 2.0 in float64."""
    v = np.sort(np.ascontiguousarray(s, np.float64).view(np.uint64)).view(np.float64)
    n = v.size
    return (v[(n - 1) // 2] + v[n // 2]) / 2.0


def ref_scale(s, scale_mode='mad'):
    """oracle_scale of test_robust_cpu: 1 ('apriori') or median / MAD_C, 1 where that is 0."""
    return oracle_scale(np.asarray(s, float), scale_mode)


def ref_weights(s, scale, loss, k):
    """robust_weight_fn(s / scale): s / scale and the Cauchy square may overflow (omega = 0 then)."""
    with np.errstate(over='ignore'):
        return robust_weight_fn(np.asarray(s, float) / scale, loss, k)


def first_pass_differing(a, b):
    """The first pass whose digit differs between the patterns of a and b (None: equal)."""
    a, b = (int(np.array([v], np.float64).view(np.uint64)[0]) for v in (a, b))
    for p, (sh, nb) in enumerate(zip(SHIFT, BITS)):
        if (a >> sh) & ((1 << nb) - 1) != (b >> sh) & ((1 << nb) - 1):
            return p
    return None


def deal_sorted(s, owned):
    """The values of s in IP column order such that the ranks, in order, own ascending runs of the sorted values:
    rank 0 only the smallest, the last rank that owns anything only the largest.  owned: one mask per rank."""
    v = np.sort(np.asarray(s, float))
    out = np.empty_like(v)
    pos = 0
    for m in owned:
        cols = np.flatnonzero(m)
        out[cols] = v[pos:pos + cols.size]
        pos += cols.size
    assert pos == v.size
    return out
