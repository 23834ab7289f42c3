"""The crafted values of tests/robust_select_cases.py are what they claim to be (no device): admissible for
dbat_hip_debug_robust_from_s, their reference median the one NumPy computes, the two targets of split() parting in the
pass asked for, cluster() with ties; and what the debug entry refuses before it touches a device."""
import numpy as np
import pytest

import robust_select_cases as rc
from dbat_amd import _hip
from dbat_amd.driver import MAD_C


@pytest.mark.parametrize('n', rc.SIZES)
def test_values_are_admissible_and_median_is_numpys(n):
    cs = rc.cases(n)
    assert [c[0] for c in cs] == rc.case_ids(n) and len(cs) == 23 + (n % 2 == 0)
    for name, s in cs:
        assert s.dtype == np.float64 and s.shape == (n,), name
        assert np.all(np.isfinite(s)) and not np.any(np.signbit(s)) and np.all(s < 2.0 ** 1022), name
        med = rc.ref_median(s)
        assert med == np.median(s), name
        sc = rc.ref_scale(s)
        assert sc == (1.0 if med == 0 else med / MAD_C) and sc > 0 and np.isfinite(sc), name
        assert rc.ref_scale(s, 'apriori') == 1.0
        for loss, k in (('huber', 1.5), ('cauchy', 2.385)):
            w = rc.ref_weights(s, sc, loss, k)
            assert not np.any(np.isnan(w)) and np.all((w >= 0) & (w <= 1)), (name, loss)
        assert np.array_equal(s, dict(rc.cases(n))[name]), name           # seeded
        assert name.startswith('all-') or not np.array_equal(s, np.sort(s)), name    # shuffled


@pytest.mark.parametrize('n', rc.SIZES)
def test_named_medians(n):
    d = dict(rc.cases(n))
    one_up = np.array([rc.B + 1], np.uint64).view(np.float64)[0]
    assert rc.ref_median(d['all-one']) == 1.0 and rc.ref_median(d['all-zero']) == 0.0
    assert rc.ref_median(d['zeros-majority']) == 0.0 and np.count_nonzero(d['zeros-majority'] == 0) == n // 2 + 1
    assert rc.ref_scale(d['all-zero']) == 1.0 and rc.ref_scale(d['zeros-majority']) == 1.0
    if n % 2 == 0:
        z = d['zeros-half']
        assert np.count_nonzero(z == 0) == n // 2 and np.count_nonzero(z == 5e-324) == n // 2
        assert rc.ref_median(z) == 0.0 and rc.ref_scale(z) == 1.0
        assert rc.ref_median(d['split5']) == (1.0 + one_up) / 2.0 == 1.0     # a tie of the mean, rounded to even
    e = d['extremes']
    assert e.max() == 2.0 ** 1021 and np.count_nonzero(e == 0) > n // 10 and np.count_nonzero(e == 5e-324) > n // 10
    assert np.count_nonzero((e > 5e-324) & (e < 2.0 ** -1022)) > n // 10 and np.count_nonzero(e == 1.0) > n // 10
    assert np.unique(d['rayleigh']).size == n


@pytest.mark.parametrize('p', range(6))
@pytest.mark.parametrize('n', rc.SIZES)
def test_split_parts_in_its_pass(n, p):
    v = np.sort(rc.split(n, p))
    a, b = v[(n - 1) // 2], v[n // 2]
    assert np.unique(v).size == 2 and np.count_nonzero(v == 1.0) == n // 2
    if n % 2 == 0:
        assert a == 1.0 and b > a and rc.first_pass_differing(a, b) == p
        # ... and in no digit but that one
        assert int(np.array([b]).view(np.uint64)[0]) - rc.B == 1 << rc.SHIFT[p]
    else:
        assert a == b and rc.first_pass_differing(a, b) is None


@pytest.mark.parametrize('p', range(6))
@pytest.mark.parametrize('n', rc.SIZES)
def test_cluster_is_crowded_in_one_pass(n, p):
    s = rc.cluster(n, p)
    nd = np.unique(s).size
    assert 2 <= nd < n
    if n <= 1800:
        assert 750 <= nd <= 1250, nd
    bits = s.view(np.uint64)
    for q, (sh, nb) in enumerate(zip(rc.SHIFT, rc.BITS)):       # every other pass sees a single bucket
        if q != p:
            dg = (bits >> np.uint64(sh)) & np.uint64((1 << nb) - 1)
            # (pass 1's digit reaches bit 52, which 1.0 has set: its upper half carries into pass 0's digit)
            assert np.unique(dg).size == (2 if (p, q) == (1, 0) else 1), (p, q)


@pytest.mark.parametrize('p', range(6))
@pytest.mark.parametrize('n', rc.SIZES)
def test_crowded_stays_crowded_to_the_last_digit(n, p):
    s = rc.crowded(n, p)
    bits = np.sort(s.view(np.uint64))
    assert 3 ** (6 - p) // 2 < np.unique(bits).size <= 3 ** (6 - p)       # (1800 draws do not reach all 729)
    targets = {int(bits[(n - 1) // 2]), int(bits[n // 2])}
    for q, (sh, nb) in enumerate(zip(rc.SHIFT, rc.BITS)):
        dg = (bits >> np.uint64(sh)) & np.uint64((1 << nb) - 1)
        assert np.all(dg != 0) and np.unique(dg).size == (3 if q >= p else 1), (p, q)
        if q >= p:          # what the pass sees for each target: several values in two or three buckets, no digit 0
            for tg in targets:
                sel = (bits >> np.uint64(sh + nb)) == np.uint64(tg >> (sh + nb)) if sh + nb < 64 else np.ones(n, bool)
                assert np.unique(dg[sel]).size >= 2 and np.count_nonzero(sel) >= (3 if n < 2000 else 30), (p, q)


def test_first_pass_differing_and_deal_sorted():
    assert rc.first_pass_differing(1.0, 1.0) is None and rc.first_pass_differing(1.0, 2.0) == 0
    assert rc.first_pass_differing(0.0, 5e-324) == 5
    owned = [np.array([0, 1, 0, 0, 1], bool), np.zeros(5, bool), np.array([1, 0, 1, 1, 0], bool)]
    out = rc.deal_sorted(np.array([5.0, 1.0, 4.0, 2.0, 3.0]), owned)
    assert np.array_equal(out, [3.0, 1.0, 4.0, 5.0, 2.0])
    assert out[owned[0]].max() < out[owned[2]].min()


def test_debug_entry_refuses_null_arguments_without_a_device():
    lib = _hip.load()
    assert 'dbat_hip_debug_robust_from_s' in _hip.SYMBOLS
    ro = _hip.robust_options('cauchy', scale='mad')
    s = np.ones(4)
    med, sc, chg = (_hip.C.c_double() for _ in range(3))
    args = lambda h, sp, r: (h, sp, r, None, _hip.C.byref(med), _hip.C.byref(sc), _hip.C.byref(chg), None)
    fake = _hip._H(1)       # never dereferenced: the NULL checks come first
    assert lib.dbat_hip_debug_robust_from_s(*args(None, _hip.dptr(s), ro)) == _hip.EINVAL
    assert lib.dbat_hip_debug_robust_from_s(*args(fake, None, ro)) == _hip.EINVAL
    assert lib.dbat_hip_debug_robust_from_s(*args(fake, _hip.dptr(s), None)) == _hip.EINVAL
