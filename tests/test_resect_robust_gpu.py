"""Robust resection on the device (dbat_hip_resect_ransac, csrc/resect_ransac.hpp; dbat_hip_poseadjust, csrc/poseadjust.hpp;
dbat_amd.initial.resect_robust) against the NumPy restatements of tests/resect_ransac_ref.py and tests/poseadjust_ref.py,
which share no code with dbat_amd/.  The seeded cases are those of tests/test_resect_robust_cpu.py, where the properties
their seeds were chosen for are checked without a device.

poseadjust: both stop at the same optimum; the path to it is not compared.  Per case d_dev is the device's distance to
the np.longdouble restatement and d_ref the float64 restatement's distance to it (the largest difference in R and C
and, for the cameras with noise and at least four points, relative in sigma0 and Q): d_dev <= max(10 d_ref, FLOOR).  The
factor is this project's margin for two float64 routes on the same conditioning (test_pairadjust_gpu.py,
test_relorient_gpu.py).  FLOOR is for the cases whose d_ref sits at rounding: ten times the largest d_ref of the
noise-free seeded cases, 1.588e-14 (n = 4) as test_resect_robust_cpu.test_noise_free_floor prints it, so 1.588e-13.
Every run prints both distances (pytest -s).

resect_ransac: the winner's sample, count and mask are those of the restatement.  The root is the index among the poses
of the sample in the order each root finder returns them, so it is compared by value: the device's pose is that of the
restatement's root -- no other pose of the sample is as close -- within d_dev <= max(10 d_ref, POSE_FLOOR), with d_ref the
distance in R of the float64 route of the restatement (resect_ransac_ref.poses_float64: the same formulas in float64)
to the np.longdouble pose.  A sample whose quartic has roots 2e-4 apart loses ten digits in any float64 route, and d_ref
says so.  POSE_FLOOR is ten times the largest d_ref of the winners whose roots are more than 1e-2 apart, 1.31e-12
(seed 7) as test_resect_robust_cpu.test_ransac_pose_floor prints it."""
import copy

import numpy as np
import pytest

import poseadjust_ref as po
import resect_ransac_ref as rr
from test_resect_robust_cpu import (CASES, RANSAC_CASES, SHIFT, crafted, oracle_case, ransac_seeded, seeded, swapped_camcal, use_case,
                                    winner_d_ref)

pytestmark = pytest.mark.gpu

FACTOR = 10.0
FLOOR = 1.588e-13
POSE_FLOOR = 1.31e-11


@pytest.fixture(scope='module')
def hip():
    from dbat_amd import _hip
    import torch
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    _hip.load()
    return _hip


def as_result(r, k, sl):
    """Camera k of a device call in the form of the restatement's result."""
    return dict(P=r['P'][k], used=r['used'][sl], sigma0=r['sigma0'][k], Q=r['Q'][k], code=int(r['code'][k]), f=r['f'][k], f0=r['f0'][k],
                n=int(r['n_used'][k]), iters=int(r['iters'][k]), res=None if r['res'] is None else r['res'][:, sl])


def same_bits(a, b):
    return all(a[k] is None or np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def compare(label, dev, ref64, refld, stat, shift=None):
    """The checks of one camera: the distances, the invariants of the pose, the mask, the code."""
    d_ref, d_dev = po.distance(ref64, refld, stat, shift), po.distance(dev, refld, stat, shift)
    print('%s: d_dev %.2e d_ref %.2e (bound %.2e); device %d iterations, restatement %d' % (label, d_dev, d_ref, max(FACTOR * d_ref, FLOOR), dev['iters'], ref64['iters']))
    assert np.array_equal(dev['used'], ref64['used']), label + ': mask'
    assert dev['code'] == ref64['code'] == 0, label + ': code %d' % dev['code']
    assert np.abs(dev['P'][:, :3].T @ dev['P'][:, :3] - np.eye(3)).max() < 1e-13, label
    assert d_dev <= max(FACTOR * d_ref, FLOOR), '%s: device %.2e from the longdouble restatement, float64 restatement %.2e' % (label, d_dev, d_ref)


OPT = dict(w=po.WEIGHT, max_iter=po.MAX_ITER, conv_tol=po.CONV_TOL)


def batch_args(cs, **kw):
    ps = np.cumsum([0] + [c['X'].shape[1] for c in cs])
    cat = lambda k: np.concatenate([c[k] for c in cs], 1)
    return ps, {**dict(pt_start=ps, X=cat('X'), xn=cat('x'), P=np.stack([c['P0'] for c in cs])), **OPT, **kw}


# ---- poseadjust ------------------------------------------------------------------------------------------------------------

def test_seeded_cases(hip):
    cs = [seeded(n, noise)[0] for n, noise in CASES]
    ps, args = batch_args(cs, residuals=True)
    a, b = hip.poseadjust(**args), hip.poseadjust(**args)
    assert same_bits(a, b), 'two identical calls differ'
    failed = []
    for k, (n, noise) in enumerate(CASES):
        c, r64, rld = seeded(n, noise)
        sl = slice(ps[k], ps[k + 1])
        one = hip.poseadjust(**batch_args([c], residuals=True)[1])
        for key in ('P', 'f0', 'f', 'sigma0', 'lam', 'code', 'iters', 'trials', 'n_used', 'Q'):
            assert np.array_equal(one[key][0], a[key][k], equal_nan=True), 'n %d noise %g: %s alone and in the batch differ' % (n, noise, key)
        assert np.array_equal(one['used'], a['used'][sl]) and np.array_equal(one['res'], a['res'][:, sl])
        dev = as_result(a, k, sl)
        assert np.isnan(dev['sigma0']) == (n == 3) and np.all(np.isfinite(dev['res'])) and dev['f'] <= dev['f0']
        try:
            compare('n %4d noise %.0e' % (n, noise), dev, r64, rld, noise > 0 and n >= 4)
        except AssertionError as e:                               # every case is run and printed before the test fails
            failed.append(str(e).splitlines()[0])
    assert not failed, failed


def test_mask_weights_and_residuals(hip):
    """A mask with holes (one of them NaN), weights of their own per coordinate, and the residuals of every point."""
    c = seeded(129, 5e-4)[0]
    rng = np.random.default_rng(12)
    use = rng.uniform(size=129) > 0.3
    use[:2] = (False, True)                               # the first used point is not the first point
    w = rng.uniform(500.0, 4000.0, (2, 129))
    X = c['X'].copy()
    hole = int(np.flatnonzero(~use)[3])
    X[:, hole] = np.nan
    kw = dict(use=use, w=w, max_iter=po.MAX_ITER, conv_tol=po.CONV_TOL)
    r64, rld = po.adjust(X, c['x'], c['P0'], **kw), po.adjust(X, c['x'], c['P0'], dtype=np.longdouble, **kw)
    r = hip.poseadjust([0, 129], X, c['x'], c['P0'][None], residuals=True, **kw)
    dev = as_result(r, 0, slice(0, 129))
    compare('mask with holes, weights', dev, r64, rld, True)
    assert dev['n'] == use.sum() and not dev['used'][~use].any()
    e_ref, e_dev = np.abs(np.asarray(r64['res'] - rld['res'], float)).max(), np.abs(np.asarray(dev['res'] - rld['res'], float)).max()
    print('residuals of all points: device %.2e restatement %.2e from the longdouble restatement' % (e_dev, e_ref))
    assert e_dev <= max(FACTOR * e_ref, FLOOR * w.max())              # a residual is the weight times a difference of coordinates
    assert np.all(dev['res'][:, hole] == 0) and np.all(dev['res'][:, ~use & np.isfinite(X[0])] != 0)
    assert abs(float(np.sum(dev['res'][:, dev['used']] ** 2)) / dev['f'] - 1) < 1e-12
    # without weights: ones
    r1 = hip.poseadjust([0, 129], X, c['x'], c['P0'][None], use=use, max_iter=po.MAX_ITER, conv_tol=po.CONV_TOL)
    r2 = hip.poseadjust([0, 129], X, c['x'], c['P0'][None], use=use, w=1.0, max_iter=po.MAX_ITER, conv_tol=po.CONV_TOL)
    assert same_bits(r1, r2) and r1['code'][0] == 0


def test_statuses(hip):
    c = seeded(64, 5e-4)[0]
    r = hip.poseadjust(**batch_args([c], max_iter=1)[1])
    assert r['code'][0] == 1 and r['iters'][0] == 1 and r['f'][0] <= r['f0'][0] and np.all(np.isfinite(r['P'])) and np.all(np.isfinite(r['Q']))
    # two used points, an empty camera and a sound one in one batch
    c65 = seeded(65, 5e-4)[0]
    r = hip.poseadjust([0, 64, 64, 129], np.concatenate([c['X'], c65['X']], 1), np.concatenate([c['x'], c65['x']], 1),
                       np.stack([c['P0'], c['P0'], c65['P0']]), use=np.concatenate([np.arange(64) < 2, np.ones(65, bool)]), residuals=True, **OPT)
    alone = hip.poseadjust(**batch_args([c65], residuals=True)[1])
    assert r['code'].tolist() == [4, 4, 0] and r['n_used'].tolist() == [2, 0, 65]
    assert np.array_equal(r['P'][0], c['P0']) and np.array_equal(r['P'][1], c['P0']) and np.all(np.isnan(r['Q'][:2]))
    assert np.all(np.isnan(r['f'][:2])) and np.all(np.isnan(r['sigma0'][:2])) and np.all(r['lam'][:2] == 1e-3) and np.all(r['res'][:, :64] == 0)
    for key in ('P', 'f', 'sigma0', 'Q', 'iters', 'trials'):
        assert np.array_equal(r[key][2], alone[key][0]), key
    assert np.array_equal(r['res'][:, 64:], alone['res']) and np.array_equal(r['used'][64:], alone['used'])
    # three collinear control points: the rotation about their line is not determined
    X = np.array([[0.0, 5.0, 10.0], [0.0, 5.0, 10.0], [0.0, 0.0, 0.0]])
    C = np.array([4.0, 7.0, 20.0])
    xn = ((X - C[:, None])[:2] / (X - C[:, None])[2])
    r = hip.poseadjust([0, 3], X, xn, np.hstack([np.eye(3), -C[:, None]])[None], **OPT)
    print('collinear: code %d, %d iterations, f %.2e' % (r['code'][0], r['iters'][0], r['f'][0]))
    assert r['code'][0] in (3, 2) and np.all(np.isfinite(r['P'])) and np.all(np.isnan(r['Q'])) and np.isnan(r['sigma0'][0])
    # no camera, and a call without a point
    r = hip.poseadjust([0], np.zeros((3, 0)), np.zeros((2, 0)), np.zeros((0, 3, 4)))
    assert r['code'].size == 0
    r = hip.poseadjust([0, 0], np.zeros((3, 0)), np.zeros((2, 0)), c['P0'][None])
    assert r['code'].tolist() == [4] and np.array_equal(r['P'][0], c['P0'])


def test_shifted_coordinates(hip):
    """Coordinates shifted by 1e6 m: the unshifted result within the same bound.  What a float64 route returns is
    P = [R | -R C], whose last column carries 1e6 eps; d_ref, the float64 restatement on the same shifted input through
    the same P, has that in it."""
    c, r64, _ = seeded(65, 5e-4, True)
    rld = seeded(65, 5e-4)[2]
    r = hip.poseadjust(**batch_args([c])[1])
    compare('n 65 noise 5e-04 shifted by 1e6 m', as_result(r, 0, slice(0, 65)), r64, rld, True, SHIFT)


def test_against_the_engine(hip):
    """The device's bundle() on the one-camera project of test_resect_robust_cpu.test_oracle -- every object point fixed --
    against poseadjust: the pose, sigma0 and the centre block of bundle_cov, within the bounds of that test."""
    from dbat_amd import bundle, bundle_cov
    from dbat_amd import initial as I
    c = oracle_case()
    res, ok, iters, s0, E = bundle(c['s'], 50, 'gna', 1e-9)
    assert ok and E.code == 0
    r = hip.poseadjust([0, 40], c['X'], c['xn'], c['P0'][None], w=c['w'], max_iter=50, conv_tol=1e-9)
    CEO = np.asarray(bundle_cov(res, E, 'CEO').todense())
    P = r['P'][0]
    cov = r['sigma0'][0] ** 2 * r['Q'][0][:3, :3]
    dist = np.linalg.norm(res.EO.val[:3, 0] - c['X'].mean(1))
    d = (abs(r['sigma0'][0] / s0 - 1), np.abs(P[:, :3] - I.rotmat3d(res.EO.val[3:6, 0])).max(),
         np.abs(-P[:, :3].T @ P[:, 3] - res.EO.val[:3, 0]).max() / dist, np.abs(cov - CEO[:3, :3]).max() / np.abs(CEO[:3, :3]).max())
    print('engine: bundle() %d iterations, poseadjust %d (%d trials); differences sigma0 %.1e R %.1e C %.1e cov %.1e'
          % (iters, r['iters'][0], r['trials'][0], *d))
    assert r['code'][0] == 0 and r['n_used'][0] == 40
    assert d[0] < 1e-10 and d[1] < 1e-8 and d[2] < 1e-8 and d[3] < 1e-6


# ---- resect_ransac ---------------------------------------------------------------------------------------------------------

def check_winner(label, c, st, P, inl, ssq, ref):
    """Camera of a device call (stats, P, inlier, ssq) against the restatement's result ref."""
    print('%s: device count %d sample %d root %d, %d poses; restatement count %d sample %d root %d, %d poses'
          % (label, st[0], st[1], st[2], st[3], ref['count'], ref['sample'], ref['root'], ref['scored']))
    assert (st[0], st[1], st[3]) == (ref['count'], ref['sample'], ref['scored']), label
    assert np.array_equal(inl, ref['mask']), label + ': mask'
    if ref['sample'] < 0:
        assert st[2] == -1 and np.all(np.isnan(P)) and ssq == 0 and not inl.any(), label
        return
    k, d = rr.rotation_distance(P, ref['poses'][ref['sample']])
    d_ref = winner_d_ref(c, ref)
    print('    root: device pose %.2e from the longdouble one, float64 route %.2e (bound %.2e)' % (d[k], d_ref, max(FACTOR * d_ref, POSE_FLOOR)))
    assert 0 <= st[2] < len(d) and k == ref['root'], '%s: root (%s)' % (label, d)
    assert d[k] <= max(FACTOR * d_ref, POSE_FLOOR), '%s: device pose %.2e from the longdouble one, float64 route %.2e' % (label, d[k], d_ref)
    assert 0 <= ssq <= st[0] * c['thr2'], label


def ransac_args(cs, **kw):
    ps = np.cumsum([0] + [c['X'].shape[1] for c in cs])
    ss = np.cumsum([0] + [len(c['samples']) for c in cs])
    return ps, dict(pt_start=ps, X=np.concatenate([c['X'] for c in cs], 1), xn=np.concatenate([c['x'] for c in cs], 1), smp_start=ss,
                    samples=np.concatenate([c['samples'] for c in cs], 0), thr2=[c['thr2'] for c in cs], **kw)


def test_ransac_seeded_cases(hip):
    """Point counts around the stride and the tile, sample counts around the round, a camera of three points (no
    winner) among them; two calls, and every camera alone against the batch."""
    cs = [ransac_seeded(*k)[0] for k in RANSAC_CASES]
    ps, args = ransac_args(cs)
    a, b = hip.resect_ransac(**args), hip.resect_ransac(**args)
    assert same_bits(a, b), 'two identical calls differ'
    failed = []
    for k, key in enumerate(RANSAC_CASES):
        c, _, _, ref = ransac_seeded(*key)
        sl = slice(ps[k], ps[k + 1])
        one = hip.resect_ransac(**ransac_args([c])[1])
        assert np.array_equal(one['P'][0], a['P'][k], equal_nan=True) and np.array_equal(one['stats'][0], a['stats'][k]), key
        assert np.array_equal(one['inlier'], a['inlier'][sl]) and one['ssq'][0] == a['ssq'][k], key
        try:
            check_winner('seed %d, %d points, %d samples' % key, c, a['stats'][k], a['P'][k], a['inlier'][sl], a['ssq'][k], ref)
        except AssertionError as e:
            failed.append(str(e).splitlines()[0])
    assert not failed, failed


@pytest.mark.parametrize('kind', ('late', 'tie'))
def test_ransac_tie_and_rounds(hip, kind):
    """The winning triple at sample 256 alone: the second round; at samples 7 and 200: equal counts give the lower."""
    c, _, _, ref = crafted(kind)
    r = hip.resect_ransac(**ransac_args([c])[1])
    check_winner(kind, c, r['stats'][0], r['P'][0], r['inlier'], r['ssq'][0], ref)
    assert r['stats'][0][1] == c['where'][0]


def test_ransac_use(hip):
    """use takes a point out of sampling and out of counting, whatever it holds."""
    c, use, _, _, ref = use_case()
    X = c['X'].copy()
    X[:, ~use] = np.nan
    r = hip.resect_ransac(**ransac_args([dict(c, X=X)], use=use)[1])
    check_winner('use', c, r['stats'][0], r['P'][0], r['inlier'], r['ssq'][0], ref)
    assert not r['inlier'][~use].any()


def test_ransac_shifted_coordinates(hip):
    c, _, _, ref = ransac_seeded(6, 65, 64, True)
    r = hip.resect_ransac(**ransac_args([c])[1])
    check_winner('65 points at 1e6 m', c, r['stats'][0], r['P'][0], r['inlier'], r['ssq'][0], ref)
    # no camera, and cameras without points or samples
    r = hip.resect_ransac([0], np.zeros((3, 0)), np.zeros((2, 0)), [0], np.zeros((0, 3)), [])
    assert r['stats'].shape == (0, 4)
    r = hip.resect_ransac([0, 0, 65], c['X'], c['x'], [0, 0, 0], np.zeros((0, 3)), c['thr2'])
    assert r['stats'].tolist() == [[0, -1, -1, 0]] * 2 and np.all(np.isnan(r['P'])) and not r['inlier'].any()


# ---- the pipeline ----------------------------------------------------------------------------------------------------------

def test_pipeline_camcal(hip):
    """camcal with the coordinates of three control points swapped among themselves: resect_robust over all object
    points recovers every station (test_resect_robust_cpu.test_camcal_swapped_control_points has the figures of the
    restatements) and bundle() from there converges to the report's sigma0; plain resect(n = 1) from the control points
    does not recover one.  A round of reselection never lowers a count."""
    from dbat_amd import bundle
    from dbat_amd import initial as I
    from helpers import camcal_expected
    good, bad = swapped_camcal()
    blank = I.cleareo(bad)
    cp = good.OP.id[good.prior.OP.isCtrl]
    s1, info, fail = I.resect_robust(blank)
    assert not fail and len(info) == 21
    d = np.linalg.norm(s1.EO.val[:3] - good.EO.val[:3], axis=0)
    print('resect_robust: %.3f .. %.3f from the stations; counts %s; sigma0 %.1f .. %.1f; rms %.2f .. %.2f px'
          % (d.min(), d.max(), [f['count'] for f in info], min(f['sigma0'] for f in info), max(f['sigma0'] for f in info),
             min(f['rms_px'] for f in info), max(f['rms_px'] for f in info)))
    assert d.max() < 0.3 and all(f['code'] == 0 and f['count'] >= 30 and f['rms_px'] < 3.0 for f in info)
    for f in info:
        assert f['inlier'].sum() == f['count'] and f['ids'].size == f['inlier'].size and f['sample'].shape == (3,)
        assert np.allclose(f['cov'], f['sigma0'] ** 2 * f['Q'], rtol=1e-15, atol=0) and np.all(np.isfinite(f['cov']))
    start = copy.deepcopy(good)
    start.EO.val[:6] = s1.EO.val[:6]
    res, ok, iters, s0, E = bundle(start, 'gna')
    assert ok and abs(s0 / camcal_expected()['model3']['sigma0'] - 1) < 1e-4
    s2, rms, fail2 = I.resect(blank, 'all', cp, 1, 0, cp)
    d2 = np.linalg.norm(s2.EO.val[:3] - good.EO.val[:3], axis=0)
    print('plain resect: %.3f .. %.3f from the stations' % (d2.min(), d2.max()))
    assert d2.min() > 1.5
    # without refinement: the poses of the RANSAC; with a round of reselection: no count decreases
    s3, info3, _ = I.resect_robust(blank, refine=False)
    assert all(np.isnan(f['sigma0']) and f['code'] == 0 for f in info3)
    s4, info4, _ = I.resect_robust(blank, reselect=1)
    up = [g['count'] - f['count'] for f, g in zip(info, info4)]
    print('reselect = 1: counts change by %s' % up)
    assert min(up) >= 0 and all(g['code'] == 0 for g in info4)
    # a camera without a winner: three points
    s5, info5, fail5 = I.resect_robust(blank, cams=[0, 1], cpId=good.OP.id[:3])
    assert fail5 and all(f['code'] == -1 and f['sample'] is None for f in info5) and np.all(np.isnan(s5.EO.val[:6, :2]))
