"""Robust forward intersection on the device (dbat_hip_intersect_ransac, csrc/intersect_ransac.hpp; dbat_hip_pointadjust,
csrc/pointadjust.hpp; dbat_amd.initial.forwintersect_robust) against the NumPy restatements of
tests/intersect_ransac_ref.py and tests/pointadjust_ref.py, which share no code with dbat_amd/.  The seeded cases are those
of tests/test_intersect_robust_cpu.py, where the properties their seeds were chosen for are checked without a device.

pointadjust: both stop at the same optimum; the path to it is not compared.  Per case d_dev is the device's distance to
the np.longdouble restatement and d_ref the float64 restatement's distance to it (the largest difference in X over the
size of the scene, 10, and, for the points with noise and at least three rays, relative in sigma0 and Q):
d_dev <= max(10 d_ref, FLOOR).  The factor is this project's margin for two float64 routes on the same conditioning
(test_pairadjust_gpu.py, test_resect_robust_gpu.py).  FLOOR is for the cases whose d_ref sits at rounding: ten times the
largest d_ref of the noise-free seeded cases, 1.180e-16 (r = 3) as test_intersect_robust_cpu.test_noise_free_floor prints
it, so 1.180e-15.  Every run prints both distances (pytest -s).

intersect_ransac: count, sample, inlier and the numbers of hypotheses scored and of usable rays are those of the
restatement, exactly: test_intersect_robust_cpu.check_ransac_seed asserts that no comparison of the seeded cases is closer
than 1e-9 relative.  X passes by the same d_dev <= max(10 d_ref, FLOOR)."""
import copy

import numpy as np
import pytest

import intersect_ransac_ref as ir
import pointadjust_ref as pr
from test_intersect_robust_cpu import (CASES, CRAFTED, RANSAC_CASES, SCALE, check_ransac_seed, crafted, oracle_case, ransac_seeded, seeded, stat_of,
                                       status_cases)

pytestmark = pytest.mark.gpu

FACTOR = 10.0
FLOOR = 1.180e-15


@pytest.fixture(scope='module')
def hip():
    from dbat_amd import _hip
    import torch
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    _hip.load()
    return _hip


def same_bits(a, b):
    return all(a[k] is None or np.array_equal(a[k], b[k], equal_nan=True) for k in a)


OPT = dict(w=pr.WEIGHT, max_iter=pr.MAX_ITER, conv_tol=pr.CONV_TOL)
KEYS = ('f0', 'f', 'sigma0', 'lam', 'code', 'iters', 'trials', 'n_used', 'Q')


def batch_args(cs, **kw):
    """The points cs (cases of pr.seeded_case over the one set of cameras) as one call."""
    rs = np.cumsum([0] + [c['cam'].size for c in cs])
    return rs, {**dict(ray_start=rs, cam=np.concatenate([c['cam'] for c in cs]), xn=np.concatenate([c['x'] for c in cs], 1), P=cs[0]['P'],
                       X=np.stack([c['X0'] for c in cs], 1)), **OPT, **kw}


def as_result(r, k, sl):
    """Point k of a device call in the form of the restatement's result."""
    return dict(X=r['X'][:, k], used=r['used'][sl], sigma0=r['sigma0'][k], Q=r['Q'][k], code=int(r['code'][k]), f=r['f'][k], f0=r['f0'][k],
                n=int(r['n_used'][k]), iters=int(r['iters'][k]), res=None if r['res'] is None else r['res'][:, sl])


def compare(label, dev, ref64, refld, stat, code=0):
    d_ref, d_dev = pr.distance(ref64, refld, stat, SCALE), pr.distance(dev, refld, stat, SCALE)
    print('%s: d_dev %.2e d_ref %.2e (bound %.2e); device %d iterations, restatement %d' % (label, d_dev, d_ref, max(FACTOR * d_ref, FLOOR), dev['iters'], ref64['iters']))
    assert np.array_equal(dev['used'], ref64['used']), label + ': mask'
    assert dev['code'] == ref64['code'] == code, label + ': code %d' % dev['code']
    assert d_dev <= max(FACTOR * d_ref, FLOOR), '%s: device %.2e from the longdouble restatement, float64 restatement %.2e' % (label, d_dev, d_ref)


# ---- pointadjust -----------------------------------------------------------------------------------------------------------

def test_seeded_cases(hip):
    """Ray counts around the 8-lane stride, with and without noise, in one call; two calls; every point alone."""
    cs = [seeded(r, noise)[0] for r, noise in CASES]
    rs, args = batch_args(cs, residuals=True)
    a, b = hip.pointadjust(**args), hip.pointadjust(**args)
    assert same_bits(a, b), 'two identical calls differ'
    failed = []
    for k, (r, noise) in enumerate(CASES):
        c, r64, rld = seeded(r, noise)
        sl = slice(rs[k], rs[k + 1])
        one = hip.pointadjust(**batch_args([c], residuals=True)[1])
        for key in KEYS:
            assert np.array_equal(one[key][0], a[key][k], equal_nan=True), 'r %d noise %g: %s alone and in the batch differ' % (r, noise, key)
        assert np.array_equal(one['X'][:, 0], a['X'][:, k]) and np.array_equal(one['used'], a['used'][sl]) and np.array_equal(one['res'], a['res'][:, sl])
        dev = as_result(a, k, sl)
        assert np.all(np.isfinite(dev['res'])) and np.all(np.isfinite(dev['Q'])) and dev['f'] <= dev['f0']
        try:
            compare('r %3d noise %.0e' % (r, noise), dev, r64, rld, stat_of(r, noise))
        except AssertionError as e:                               # every case is run and printed before the test fails
            failed.append(str(e).splitlines()[0])
    assert not failed, failed


@pytest.mark.parametrize('n', (1, 7, 8, 9, 31, 32, 33))
def test_batch_sizes(hip, n):
    """Batches around the eight points of a wave and the 32 of a workgroup: every point has the bits it has alone, and
    with the order of the batch reversed, where it sits in another group of its wave."""
    cs = [seeded(*CASES[k % len(CASES)])[0] for k in range(n)]
    rs, args = batch_args(cs, residuals=True)
    a = hip.pointadjust(**args)
    rv, args_r = batch_args(cs[::-1], residuals=True)
    b = hip.pointadjust(**args_r)
    for k in range(n):
        m = n - 1 - k
        one = alone(hip, CASES[k % len(CASES)])
        for key in KEYS:
            assert np.array_equal(a[key][k], b[key][m], equal_nan=True), 'point %d of %d: %s changes with its place' % (k, n, key)
            assert np.array_equal(a[key][k], one[key][0], equal_nan=True), 'point %d of %d: %s alone and in the batch differ' % (k, n, key)
        assert np.array_equal(a['X'][:, k], b['X'][:, m]) and np.array_equal(a['X'][:, k], one['X'][:, 0])
        assert np.array_equal(a['res'][:, rs[k]:rs[k + 1]], b['res'][:, rv[m]:rv[m + 1]]) and np.array_equal(a['used'][rs[k]:rs[k + 1]], b['used'][rv[m]:rv[m + 1]])
        assert a['code'][k] == 0


_alone = {}


def alone(hip, key):
    """The device's result of the seeded case `key` in a call of its own (computed once)."""
    if key not in _alone:
        _alone[key] = hip.pointadjust(**batch_args([seeded(*key)[0]], residuals=True)[1])
    return _alone[key]


def test_mask_weights_and_residuals(hip):
    """A mask with holes (one of them NaN), weights of their own per coordinate, and the residuals of every ray."""
    c = seeded(65, 5e-4)[0]
    rng = np.random.default_rng(12)
    use = rng.uniform(size=65) > 0.3
    use[:2] = (False, True)                               # the first used ray is not the first ray
    w = rng.uniform(500.0, 4000.0, (2, 65))
    x = c['x'].copy()
    hole = int(np.flatnonzero(~use)[3])
    x[:, hole] = np.nan
    kw = dict(use=use, w=w, max_iter=pr.MAX_ITER, conv_tol=pr.CONV_TOL)
    r64, rld = pr.adjust(c['cam'], x, c['P'], c['X0'], **kw), pr.adjust(c['cam'], x, c['P'], c['X0'], dtype=np.longdouble, **kw)
    r = hip.pointadjust([0, 65], c['cam'], x, c['P'], c['X0'][:, None], residuals=True, **kw)
    dev = as_result(r, 0, slice(0, 65))
    compare('mask with holes, weights', dev, r64, rld, True)
    assert dev['n'] == use.sum() and not dev['used'][~use].any()
    e_ref, e_dev = np.abs(np.asarray(r64['res'] - rld['res'], float)).max(), np.abs(np.asarray(dev['res'] - rld['res'], float)).max()
    print('residuals of all rays: device %.2e restatement %.2e from the longdouble restatement' % (e_dev, e_ref))
    assert e_dev <= max(FACTOR * e_ref, FLOOR * w.max())              # a residual is the weight times a difference of coordinates
    assert np.all(dev['res'][:, hole] == 0) and np.all(dev['res'][:, ~use & np.isfinite(x[0])] != 0)
    assert abs(float(np.sum(dev['res'][:, dev['used']] ** 2)) / dev['f'] - 1) < 1e-12
    # without weights: ones
    r1 = hip.pointadjust([0, 65], c['cam'], x, c['P'], c['X0'][:, None], use=use, max_iter=pr.MAX_ITER, conv_tol=pr.CONV_TOL)
    r2 = hip.pointadjust([0, 65], c['cam'], x, c['P'], c['X0'][:, None], use=use, w=1.0, max_iter=pr.MAX_ITER, conv_tol=pr.CONV_TOL)
    assert same_bits(r1, r2) and r1['code'][0] == 0


def test_statuses(hip):
    """Every code, each in a call of its own and all in one batch with a sound point."""
    cases = status_cases()
    for label, (kw, code) in cases.items():
        kw = dict(kw)
        X0 = np.asarray(kw.pop('X0'), float)
        r = hip.pointadjust([0, len(kw['cam'])], kw.pop('cam'), kw.pop('xn'), kw.pop('P'), X0[:, None], residuals=True, **kw)
        ref = pr.adjust(X0=X0, **{k: v for k, v in cases[label][0].items() if k != 'X0'})
        print('%s: code %d, %d iterations, %d trials, lambda %.0e (restatement: %d, %d, %d, %.0e)'
              % (label, r['code'][0], r['iters'][0], r['trials'][0], r['lam'][0], ref['code'], ref['iters'], ref['trials'], ref['lam']))
        assert r['code'][0] == code == ref['code'] and np.array_equal(r['used'], ref['used'])
        assert np.all(np.isfinite(r['X'])) and np.all(np.isfinite(r['res']))
        if code in (3, 4):
            assert np.all(np.isnan(r['Q']))
        if code == 1:
            assert r['iters'][0] == 1 and r['f'][0] <= r['f0'][0] and np.all(np.isfinite(r['Q']))
        if code == 2:
            assert r['iters'][0] == 0 and r['trials'][0] == 12 and r['lam'][0] > 1e8 and np.array_equal(r['X'][:, 0], X0)
        if code == 4:
            assert np.array_equal(r['X'][:, 0], X0) and np.isnan(r['f'][0]) and np.isnan(r['sigma0'][0]) and r['lam'][0] == 1e-3
            assert r['n_used'][0] == ref['n'] == (0 if label == 'behind' else 1) and np.all(r['res'] == 0)
    # a point of one usable ray, a point without rays, a point whose start is NaN and has no ray to use, and a sound one
    c8, c9 = seeded(8, 5e-4)[0], seeded(9, 5e-4)[0]
    use = np.concatenate([np.arange(8) == 3, np.zeros(8, bool), np.ones(9, bool)])
    X = np.stack([c8['X0'], c8['X0'], np.full(3, np.nan), c9['X0']], 1)
    r = hip.pointadjust([0, 8, 8, 16, 25], np.concatenate([c8['cam'], c8['cam'], c9['cam']]), np.concatenate([c8['x'], c8['x'], c9['x']], 1),
                        c8['P'], X, use=use, residuals=True, **OPT)
    one = alone(hip, (9, 5e-4))
    assert r['code'].tolist() == [4, 4, 4, 0] and r['n_used'].tolist() == [1, 0, 0, 9]
    assert np.array_equal(r['X'][:, :3], X[:, :3], equal_nan=True) and np.all(np.isnan(r['Q'][:3])) and np.all(r['res'][:, :16] == 0)
    for key in KEYS:
        assert np.array_equal(r[key][3], one[key][0]), key
    assert np.array_equal(r['X'][:, 3], one['X'][:, 0]) and np.array_equal(r['res'][:, 16:], one['res'])
    # no point, and a call without a ray
    r = hip.pointadjust([0], np.zeros(0, int), np.zeros((2, 0)), c8['P'], np.zeros((3, 0)))
    assert r['code'].size == 0
    r = hip.pointadjust([0, 0], np.zeros(0, int), np.zeros((2, 0)), c8['P'], c8['X0'][:, None])
    assert r['code'].tolist() == [4] and np.array_equal(r['X'][:, 0], c8['X0'])


def test_shifted_coordinates(hip):
    """Coordinates shifted by (6.5e5, 6.2e6, 100) m, against the shifted scene's own restatements by the rule of every
    other case, in X, sigma0 and Q.  (P carries -R C, rounded to float64 at 6e6 m: every route gets the same rounded
    cameras, and what the float64 route loses at these coordinates is in d_ref.)"""
    c, r64, rld = seeded(9, 5e-4, True)
    r = hip.pointadjust(**batch_args([c])[1])
    compare('r   9 noise 5e-04 shifted', as_result(r, 0, slice(0, 9)), r64, rld, True)


def test_against_the_engine(hip):
    """The device's bundle() on the project of test_intersect_robust_cpu.test_oracle -- every camera and the IO fixed --
    against pointadjust: the points and the blocks of bundle_cov, within the bounds of that test."""
    from dbat_amd import bundle, bundle_cov
    c = oracle_case()
    res, ok, iters, s0, E = bundle(c['s'], 50, 'gna', 1e-7)
    assert ok and E.code == 0
    order = np.argsort(c['pt'], kind='stable')
    rs = np.concatenate([[0], np.cumsum(np.bincount(c['pt'], minlength=c['npt']))])
    r = hip.pointadjust(rs, c['cam'][order], c['xn'][:, order], c['P'], c['X0'], w=c['w'][:, order], max_iter=50, conv_tol=1e-9)
    COP = np.asarray(bundle_cov(res, E, 'COP').todense())
    dX = np.abs(r['X'] - res.OP.val).max() / SCALE
    dC = max(np.abs(s0 ** 2 * r['Q'][p] - COP[3 * p:3 * p + 3, 3 * p:3 * p + 3]).max() / np.abs(COP[3 * p:3 * p + 3, 3 * p:3 * p + 3]).max() for p in range(c['npt']))
    pooled = np.sqrt(r['f'].sum() / (2 * r['n_used'] - 3).sum())
    print('engine: bundle() %d iterations; differences X %.1e cov %.1e sigma0 (pooled) %.1e' % (iters, dX, dC, abs(pooled / s0 - 1)))
    assert np.all(r['code'] == 0) and dX < 1e-8 and dC < 1e-6 and abs(pooled / s0 - 1) < 1e-10


# ---- intersect_ransac ------------------------------------------------------------------------------------------------------

def check_winner(label, st, X, inl, ssq, ref64, ref, thr2max):
    """Point of a device call (stats, X, inlier, ssq) against the restatement's results."""
    print('%s: device count %d sample %d, %d hypotheses, %d usable; restatement count %d sample %d, %d hypotheses, %d usable'
          % (label, st[0], st[1], st[2], st[3], ref['count'], ref['sample'], ref['scored'], ref['usable']))
    assert tuple(st) == (ref['count'], ref['sample'], ref['scored'], ref['usable']), label
    assert np.array_equal(inl, ref['mask']), label + ': mask'
    if ref['sample'] < 0:
        assert np.all(np.isnan(X)) and ssq == 0 and not inl.any(), label
        return
    d_ref = float(np.abs(np.asarray(ref64['X'], np.longdouble) - ref['X']).max() / SCALE)
    d_dev = float(np.abs(np.asarray(X, np.longdouble) - ref['X']).max() / SCALE)
    print('    X: d_dev %.2e d_ref %.2e (bound %.2e)' % (d_dev, d_ref, max(FACTOR * d_ref, FLOOR)))
    assert d_dev <= max(FACTOR * d_ref, FLOOR), '%s: device %.2e from the longdouble restatement, float64 restatement %.2e' % (label, d_dev, d_ref)
    assert 0 <= ssq <= st[0] * thr2max and abs(ssq - ref['ssq']) <= 1e-9 * ref['ssq'] + 1e-30, label


def ransac_args(cs, lists=True, **kw):
    """The points cs (cases of ir.seeded_case over the one set of cameras) as one call."""
    rs = np.cumsum([0] + [c['cam'].size for c in cs])
    ss = np.cumsum([0] + [len(c['samples']) for c in cs])
    a = dict(ray_start=rs, cam=np.concatenate([c['cam'] for c in cs]), xn=np.concatenate([c['x'] for c in cs], 1), P=cs[0]['P'], thr2=cs[0]['thr2'], **kw)
    if lists:
        a.update(smp_start=ss, samples=np.concatenate([c['samples'] for c in cs], 0))
    return rs, a


def test_ransac_seeded_cases(hip):
    """Enumerated points of 2, 3, 11, 12 and 64 rays and sample lists of 63, 64, 65 and 129 in one call; two calls, and
    every point alone against the batch."""
    cs = [ransac_seeded(*k)[0] for k in RANSAC_CASES]
    thr2 = cs[0]['thr2']                                    # per camera, the same in every case
    rs, args = ransac_args(cs)
    a, b = hip.intersect_ransac(**args), hip.intersect_ransac(**args)
    assert same_bits(a, b), 'two identical calls differ'
    failed = []
    for k, key in enumerate(RANSAC_CASES):
        c, r64, rld = ransac_seeded(*key)
        sl = slice(rs[k], rs[k + 1])
        one = hip.intersect_ransac(**ransac_args([c], lists=len(c['samples']) > 0)[1])
        assert np.array_equal(one['X'][:, 0], a['X'][:, k]) and np.array_equal(one['stats'][0], a['stats'][k]), key
        assert np.array_equal(one['inlier'], a['inlier'][sl]) and one['ssq'][0] == a['ssq'][k], key
        try:
            check_winner('seed %d, %d rays, %d samples' % key, a['stats'][k], a['X'][:, k], a['inlier'][sl], a['ssq'][k], r64, rld, thr2.max())
        except AssertionError as e:
            failed.append(str(e).splitlines()[0])
    assert not failed, failed


@pytest.mark.parametrize('kind', CRAFTED)
def test_ransac_crafted(hip, kind):
    """The tie rule, use, a late winner in a list and in the enumeration, min_angle, two rays of one camera, parallel
    rays, a point of one ray and one of none."""
    kw, want = crafted(kind)
    r64, rld = ir.ransac(dtype=float, **kw), ir.ransac(**kw)
    kw = dict(kw)
    smp = kw.pop('samples', None)
    cam = kw.pop('cam')
    lists = {} if smp is None else dict(smp_start=[0, len(smp)], samples=smp)
    r = hip.intersect_ransac([0, cam.size], cam, kw.pop('xn'), kw.pop('P'), kw.pop('thr2'), **lists, **kw)
    check_winner(kind, r['stats'][0], r['X'][:, 0], r['inlier'], r['ssq'][0], r64, rld, ir.THR ** 2 * 1.25)
    for key, col in (('count', 0), ('sample', 1), ('scored', 2)):
        if key in want:
            assert r['stats'][0][col] == want[key], key


def test_ransac_listed_and_enumerated(hip):
    """The same pair listed and enumerated gives the same bits; and every pair of a point listed in the order of the
    enumeration gives what the enumeration gives."""
    c = ransac_seeded(1, 2, 0)[0]
    a = hip.intersect_ransac([0, 2], c['cam'], c['x'], c['P'], c['thr2'])
    b = hip.intersect_ransac([0, 2], c['cam'], c['x'], c['P'], c['thr2'], smp_start=[0, 1], samples=[[0, 1]])
    assert same_bits(a, b) and a['stats'][0].tolist() == [2, 0, 1, 2]
    c = ransac_seeded(4, 12, 0)[0]
    a = hip.intersect_ransac([0, 12], c['cam'], c['x'], c['P'], c['thr2'])
    b = hip.intersect_ransac([0, 12], c['cam'], c['x'], c['P'], c['thr2'], smp_start=[0, 66], samples=ir.pairs(12))
    assert same_bits(a, b) and a['stats'][0][2] == 66


def test_ransac_shifted_and_empty(hip):
    c, r64, rld = ransac_seeded(3, 11, 0, True)
    r = hip.intersect_ransac([0, 11], c['cam'], c['x'], c['P'], c['thr2'])
    st = r['stats'][0]
    print('11 rays at 6e6 m: device count %d sample %d; restatement %d, %d' % (st[0], st[1], rld['count'], rld['sample']))
    assert tuple(st) == (rld['count'], rld['sample'], rld['scored'], rld['usable']) and np.array_equal(r['inlier'], rld['mask'])
    d_ref = float(np.abs(np.asarray(r64['X'], np.longdouble) - rld['X']).max() / SCALE)
    d_dev = float(np.abs(np.asarray(r['X'][:, 0], np.longdouble) - rld['X']).max() / SCALE)
    print('    X: d_dev %.2e d_ref %.2e' % (d_dev, d_ref))
    assert d_dev <= max(FACTOR * d_ref, FLOOR)
    # no point, and points without rays among others
    r = hip.intersect_ransac([0], np.zeros(0, int), np.zeros((2, 0)), c['P'], c['thr2'])
    assert r['stats'].shape == (0, 4)
    r = hip.intersect_ransac([0, 0, 11, 11], c['cam'], c['x'], c['P'], c['thr2'])
    assert r['stats'][0].tolist() == [0, -1, 0, 0] == r['stats'][2].tolist() and np.all(np.isnan(r['X'][:, [0, 2]]))
    assert tuple(r['stats'][1]) == (rld['count'], rld['sample'], rld['scored'], rld['usable'])


# ---- the clock -------------------------------------------------------------------------------------------------------------

def test_clock(hip):
    c = ransac_seeded(4, 12, 0)[0]
    p = seeded(9, 5e-4)[0]
    ransac = lambda: hip.intersect_ransac([0, 12], c['cam'], c['x'], c['P'], c['thr2'])
    adjust = lambda: hip.pointadjust(**batch_args([p])[1])
    try:
        hip.intersect_robust_timing(True)
        ransac()
        adjust()
        ms = hip.intersect_robust_ms()
        assert ms['ransac'] > 0 and ms['adjust'] > 0
        ransac()
        ms2 = hip.intersect_robust_ms()
        assert ms2['ransac'] > 0 and ms2['adjust'] == ms['adjust']        # a call writes its own slot only
        adjust()
        ms3 = hip.intersect_robust_ms()
        assert ms3['adjust'] > 0 and ms3['ransac'] == ms2['ransac']
        hip.intersect_robust_timing(False)
        ransac()
        ms4 = hip.intersect_robust_ms()
        assert ms4['ransac'] == 0 and ms4['adjust'] == ms3['adjust']
        adjust()
        assert hip.intersect_robust_ms() == dict(ransac=0.0, adjust=0.0)
    finally:
        hip.intersect_robust_timing(False)


# ---- the pipeline ----------------------------------------------------------------------------------------------------------

def test_pipeline_camcal(hip):
    """camcal at its converged EO / IO with three image measurements of different points moved by 50 px:
    forwintersect_robust marks exactly those three columns of IP as outliers, and every point is within its bound of the
    plain forwintersect() of the uncorrupted project; plain forwintersect() of the corrupted one is not, for the three
    points.  The bound of a point, stated before anything ran: five standard deviations of the least-squares point,
    5 sqrt(trace(s^2 Q)) with Q its cofactor matrix (for weights |f| / (pxSize IP.std)) and s its own sigma0, which is
    rms_px / IP.std sqrt(n / (2 n - 3)) of its n inliers (IP.std is 0.1 px throughout, the pixels are square).  Both
    are estimates of the point from the same rays but one or none, so their difference is of the order of one standard
    deviation; the moved measurement shifts the plain point by 50 px / n, more than sixty standard deviations of a
    measurement here."""
    from dbat_amd import bundle
    from dbat_amd import initial as I
    from helpers import camcal_struct
    res, ok, iters, s0, E = bundle(camcal_struct(3), 'gna')
    assert ok
    good = I.forwintersect(res)
    bad = copy.deepcopy(res)
    r = np.bincount(res.IP.pt, minlength=res.OP.val.shape[1])
    moved_pts = np.argsort(-r, kind='stable')[:3]
    cols = np.array([np.flatnonzero(res.IP.pt == p)[2 + 3 * k] for k, p in enumerate(moved_pts)])
    bad.IP.val[:, cols] += np.array([[50.0, -30.0, 0.0], [0.0, 40.0, -50.0]])          # 50 px each
    failed = []
    for n_hyp in (256, 100):                                # every pair enumerated (at most 210 per point); 100 sampled pairs
        s1, info, fail = I.forwintersect_robust(bad, n_hyp=n_hyp)
        out = np.flatnonzero(~info['inlier'])
        n = info['count']
        s_pt = info['rms_px'] / 0.1 * np.sqrt(n / (2 * n - 3.0))
        tol = 5 * np.sqrt(s_pt ** 2 * np.trace(info['Q'], axis1=1, axis2=2))
        d = np.linalg.norm(s1.OP.val - good.OP.val, axis=0)
        d_plain = np.linalg.norm(I.forwintersect(bad).OP.val - good.OP.val, axis=0)
        print('n_hyp %d: outliers %s (moved %s); rms_px %.3f .. %.3f, sigma0 %.2f .. %.2f; distance over bound at most %.3f; plain on the moved points %s bounds'
              % (n_hyp, out.tolist(), np.sort(cols).tolist(), info['rms_px'].min(), info['rms_px'].max(), info['sigma0'].min(), info['sigma0'].max(),
                 (d / tol).max(), np.round(d_plain[moved_pts] / tol[moved_pts], 1).tolist()))
        try:
            assert not fail and np.all(info['code'] == 0) and np.array_equal(info['pts'], np.arange(res.OP.val.shape[1]))
            assert np.array_equal(out, np.sort(cols))
            assert np.array_equal(info['count'], r - np.isin(np.arange(r.size), moved_pts)) and np.array_equal(info['n_rays'], r)
            assert np.allclose(s_pt, info['sigma0'], rtol=1e-6)
            assert np.all(d <= tol), 'points %s beyond their bounds' % np.flatnonzero(d > tol).tolist()
            assert np.all(d_plain[moved_pts] > tol[moved_pts])
            assert np.all(info['sample'] >= 0) and np.all(res.IP.pt[info['sample'][:, 0]] == info['pts']) and np.all(res.IP.pt[info['sample'][:, 1]] == info['pts'])
            assert info['inlier'][info['sample']].all()
        except AssertionError as e:
            failed.append('n_hyp %d: %s' % (n_hyp, str(e).splitlines()[0]))
    assert not failed, failed
    # without refinement: the points of the RANSAC; ids and skipPrior choose the points, the others keep their values
    s3, info3, _ = I.forwintersect_robust(bad, refine=False)
    assert np.all(np.isnan(info3['sigma0'])) and np.all(info3['code'] == 0) and np.array_equal(np.flatnonzero(~info3['inlier']), np.sort(cols))
    ids = res.OP.id[[5, 7]]
    s4, info4, _ = I.forwintersect_robust(bad, ids=ids, reselect=1)
    keep = np.ones(res.OP.val.shape[1], bool)
    keep[[5, 7]] = False
    assert np.array_equal(info4['pts'], [5, 7]) and np.array_equal(s4.OP.val[:, keep], bad.OP.val[:, keep]) and np.all(info4['code'] == 0)
    # a point that no two rays agree on at this threshold: NaN, code -1, fail
    s5, info5, fail5 = I.forwintersect_robust(bad, ids=ids, min_count=50)
    assert fail5 and np.all(info5['code'] == -1) and np.all(np.isnan(s5.OP.val[:, [5, 7]])) and not info5['inlier'].any()
