"""Robust resection without a GPU (dbat_hip_resect_ransac, dbat_hip_poseadjust; dbat_amd.initial.resect_robust): the NumPy
restatements of tests/poseadjust_ref.py and tests/resect_ransac_ref.py against the truth and against
oracle/dbat_oracle.bundle on a one-camera project, the seeded cases that tests/test_resect_robust_gpu.py runs on the
device with the properties their seeds were chosen for, the ABI, everything the library refuses before it touches a
device, and draw_triples.

The oracle test: bundle() on one camera with every object point fixed minimises the same objective (no distortion, the
weights |f| / (pxSize IP.std)), so the optimum, sigma0 and the covariance of the centre are the same numbers from
independent code.  The bounds are those test_pairadjust_cpu.test_gauge uses for the same comparison (sigma0 1e-10
relative, R 1e-8, the translation 1e-8 of its length -- here the centre, relative to the camera's distance) and, for the
covariance block, the 1e-6 of its largest entry that test_hip_parity.py uses for bundle_cov."""
import functools
import os
import re

import numpy as np
import pytest

import dbat_oracle as o
import poseadjust_ref as po
import resect_ransac_ref as rr
import resect_ref as rf
from dbat_amd import _hip
from dbat_amd import initial as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1: truth and conditioning of the adjustment --------------------------------------------------------------------------

CASES = [(n, noise) for n in po.SIZES for noise in po.NOISES]


@functools.lru_cache(maxsize=None)
def seeded(n, noise, shifted=False):
    """(the case, the float64 restatement's result, the np.longdouble one's)."""
    c = po.seeded_case(n, noise, shift=SHIFT if shifted else None)
    return c, po.run_case(c), po.run_case(c, np.longdouble)


SHIFT = (1e6, -2e6, 5e5)


@pytest.mark.parametrize('n,noise', CASES)
def test_seeded_cases(n, noise):
    c, a, b = seeded(n, noise)
    stat = noise > 0 and n >= 4
    dC = np.abs(np.asarray(b['C'] - c['C'], float)).max()
    dR = np.abs(np.asarray(b['R'] - c['R'], float)).max()
    print('n %4d noise %.0e: %d / %d iterations, %d / %d trials, sigma0 %.3e, float64 to longdouble %.2e; to the truth R %.2e C %.2e'
          % (n, noise, a['iters'], b['iters'], a['trials'], b['trials'], a['sigma0'], po.distance(a, b, stat), dR, dC))
    assert a['code'] == 0 and b['code'] == 0 and a['n'] == n and np.array_equal(a['used'], b['used'])
    assert np.all(np.isfinite(a['P'])) and np.abs(a['R'].T @ a['R'] - np.eye(3)).max() < 1e-13
    assert po.distance(a, b, stat) < 1e-11
    if noise == 0:
        assert dR < 1e-12 and dC < 1e-11 and a['f'] <= po.FLOOR * 2 * n * 10
    elif n >= 63:
        assert dC < 0.1 and abs(float(a['sigma0']) - 1) < 0.3                # the noise is 5e-4 and the weight 2000
    assert np.isnan(a['sigma0']) == (n == 3)


def test_noise_free_floor():
    """The worst float64-to-longdouble distance of the noise-free cases: what FLOOR of the GPU tests is ten times of."""
    d = {n: po.distance(seeded(n, 0.0)[1], seeded(n, 0.0)[2], False) for n in po.SIZES}
    worst = max(d, key=d.get)
    print('noise-free cases: float64 to longdouble at most %.3e (n = %d)' % (d[worst], worst))
    assert d[worst] < 1e-12


def test_shifted_case_is_the_same_case():
    c, a, b = seeded(65, 5e-4, True)
    _, a0, b0 = seeded(65, 5e-4)
    d = po.distance(a, b0, True, shift=SHIFT)
    print('n 65 shifted by 1e6 m: float64 to the unshifted longdouble %.2e, longdouble to it %.2e'
          % (d, np.abs(b['C'] - np.asarray(SHIFT, np.longdouble) - b0['C']).max()))
    assert a['code'] == 0 and b['code'] == 0
    assert np.abs(np.asarray(b['C'] - np.asarray(SHIFT, np.longdouble) - b0['C'], float)).max() < 1e-12


# ---- 2: the oracle ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def oracle_case(n=40, seed=3, noise_px=0.7):
    """A one-camera struct without distortion, every object point fixed, anisotropic IP.std, noise of 0.7 px, at a
    perturbed start; and the same start as the restatement takes it."""
    from dbat_amd import synth
    from dbat_amd.dbatstruct import make_struct
    c = rf.seeded_case(seed, npt=n)
    rng = np.random.default_rng(300 + seed)
    IO = np.zeros((10, 1))
    IO[0], IO[1], IO[2] = 7.5, 0.11, -0.07
    R = np.asarray(c['R'], float)
    EO = np.zeros((6, 1))
    EO[:3, 0], EO[3:6, 0] = np.asarray(c['C'], float), I.derotmat3d(R)
    cam, pt = np.zeros(n, int), np.arange(n)
    px = 0.005
    ip = synth.project(IO, EO, c['X'], cam, pt, px)[0] + noise_px * rng.normal(size=(2, n))
    std = np.stack([rng.uniform(0.5, 1.0, n), rng.uniform(1.0, 2.0, n)])
    s = make_struct(IO, EO, c['X'], np.asfortranarray(ip), cam, pt, px, ip_std=std, distModel=3, estOP=np.zeros((3, n), bool))
    R0 = po.rodrigues(0.01 * rng.normal(size=3)) @ R
    C0 = EO[:3, 0] + 0.1 * rng.normal(size=3)
    s.EO.val[:3, 0], s.EO.val[3:6, 0] = C0, I.derotmat3d(R0)
    rows, xn, w = I.camera_points(s, 0)
    assert np.array_equal(rows, np.arange(n))
    return dict(s=s, X=c['X'], xn=xn, w=w, P0=np.hstack([R0, -(R0 @ C0)[:, None]]))


def test_oracle():
    c = oracle_case()
    s2, ok, iters, s0, E = o.bundle(c['s'], 50, 'gna', 1e-9)
    assert ok and E.code == 0
    a = po.adjust(c['X'], c['xn'], c['P0'], w=c['w'], max_iter=50, conv_tol=1e-9)
    assert a['code'] == 0 and a['n'] == 40
    CEO = np.asarray(o.bundle_cov(s2, E, 'CEO').todense())
    cov = float(a['sigma0']) ** 2 * a['Q'][:3, :3]
    dist = np.linalg.norm(s2.EO.val[:3, 0] - c['X'].mean(1))
    d = (abs(a['sigma0'] / s0 - 1), np.abs(a['R'] - I.rotmat3d(s2.EO.val[3:6, 0])).max(), np.abs(a['C'] - s2.EO.val[:3, 0]).max() / dist,
         np.abs(cov - CEO[:3, :3]).max() / np.abs(CEO[:3, :3]).max())
    print('oracle: bundle() %d iterations, restatement %d (%d trials); sigma0 %.6f; differences sigma0 %.1e R %.1e C %.1e cov %.1e'
          % (iters, a['iters'], a['trials'], s0, *d))
    assert d[0] < 1e-10 and d[1] < 1e-8 and d[2] < 1e-8 and d[3] < 1e-6


# ---- 3: the RANSAC seeds shared with the GPU tests ------------------------------------------------------------------------

# (seed, points, samples): the point counts around the 64-lane stride and the 256-point tile at 64 samples, and the
# sample counts around the round of 256 at 65 points
RANSAC_CASES = [(1, 3, 64), (2, 4, 64), (3, 5, 64), (4, 63, 64), (5, 64, 64), (6, 65, 64), (7, 129, 64), (8, 257, 64),
                (17, 65, 1), (10, 65, 255), (11, 65, 256), (12, 65, 257)]


@functools.lru_cache(maxsize=None)
def ransac_seeded(seed, n, ns, shifted=False):
    """(the case, the candidate poses and root gaps, the float64 route's result, the np.longdouble one's)."""
    c = rr.seeded_case(seed, n, ns, shift=SHIFT if shifted else None)
    poses, gaps = rr.candidates(c['X'], c['x'], c['samples'])
    return (c, (poses, gaps), rr.ransac(c['X'], c['x'], c['samples'], c['thr2'], dtype=float, poses=poses),
            rr.ransac(c['X'], c['x'], c['samples'], c['thr2'], poses=poses))


def winner_d_ref(c, b):
    """The distance in R of the float64 route's pose (rr.poses_float64) to the winner b of the np.longdouble route: what
    float64 arithmetic makes of the winning sample, whatever the conditioning of its quartic."""
    PP = rr.poses_float64(c['X'], c['x'], c['samples'][b['sample']])
    k, d = rr.rotation_distance(b['P'], PP)
    assert len(PP) == len(b['poses'][b['sample']]) and k >= 0
    return d[k]


def check_ransac_seed(c, cand, a, b):
    assert (a['sample'], a['root'], a['count']) == (b['sample'], b['root'], b['count']) and np.array_equal(a['mask'], b['mask'])
    assert np.min(cand[1]) > 1e-4, 'sample %d has roots %.1e apart' % (int(np.argmin(cand[1])), np.min(cand[1]))
    for r in (a, b):
        for k, q, cnt, e2 in r['e2']:
            assert e2.size == 0 or np.abs(np.asarray(e2, float) / c['thr2'] - 1).min() > 1e-6, 'sample %d root %d: a residual at the threshold' % (k, q)
    # the winning sample has no second root of the same count: the root is then told by its pose alone
    same = [cnt for k, q, cnt, e2 in b['e2'] if k == b['sample'] and q != b['root']]
    assert b['count'] not in same


@pytest.mark.parametrize('seed,n,ns', RANSAC_CASES)
def test_ransac_seeds(seed, n, ns):
    c, cand, a, b = ransac_seeded(seed, n, ns)
    print('seed %d, %d points (%d moved), %d samples: %d poses, winner sample %d root %d with %d inliers; smallest root gap %.1e'
          % (seed, n, c['outliers'].size, ns, b['scored'], b['sample'], b['root'], b['count'], np.min(cand[1])))
    check_ransac_seed(c, cand, a, b)
    if n == 3:
        assert b['sample'] == -1 and b['count'] == 0 and not b['mask'].any()
    elif ns >= 64:
        # every point that was not moved agrees with the winner, and the pose is the truth
        assert b['count'] == n - c['outliers'].size and not b['mask'][c['outliers']].any()
        # (the image points are rounded to float64, and a minimal solution whose quartic has roots 1e-4 apart takes that
        # rounding 1e8 times larger in the worst of these samples: measured 3.7e-9)
        assert rf.pose_err(b['P'][:, :3], c['R']) < 1e-7 and np.abs(rf.centre_ld(b['P']) - c['C']).max() < 1e-6


def test_ransac_pose_floor():
    """The float64 route's distance to the np.longdouble winner, per case: what POSE_FLOOR of the GPU tests is ten times
    the largest of, over the winners whose quartic has its roots more than 1e-2 apart (the others: their own d_ref)."""
    d, gap = {}, {}
    for key in RANSAC_CASES:
        c, cand, a, b = ransac_seeded(*key)
        if b['sample'] >= 0:
            d[key], gap[key] = winner_d_ref(c, b), cand[1][b['sample']]
            print('seed %d, %d points, %d samples: winner\'s roots %.1e apart, float64 route %.2e from the longdouble pose' % (*key, gap[key], d[key]))
    well = [k for k in d if gap[k] > 1e-2]
    worst = max(well, key=d.get)
    print('winners with roots more than 1e-2 apart: at most %.3e (seed %d)' % (d[worst], worst[0]))
    assert len(well) >= 8 and d[worst] < 1e-11


def test_ransac_shifted_seed():
    c, cand, a, b = ransac_seeded(6, 65, 64, True)
    check_ransac_seed(c, cand, a, b)
    b0 = ransac_seeded(6, 65, 64)[3]
    assert (b['sample'], b['root'], b['count']) == (b0['sample'], b0['root'], b0['count']) and np.array_equal(b['mask'], b0['mask'])


@functools.lru_cache(maxsize=None)
def crafted(kind):
    """The case of 257 samples with every sample but the winner's made to hold a moved point, and the winning triple put
    at sample 256 alone ('late': the second round of 256) or at samples 7 and 200 ('tie': equal counts)."""
    c, _, _, b = ransac_seeded(12, 65, 257)
    T = c['samples'][b['sample']].copy()
    S = c['samples'].copy()
    for k in range(len(S)):
        if not np.isin(S[k], c['outliers']).any():
            S[k, 0] = next(q for q in c['outliers'] if q not in S[k])
    where = (256,) if kind == 'late' else (7, 200)
    for k in where:
        S[k] = T
    c2 = dict(c, samples=S, where=where)
    poses, gaps = rr.candidates(c2['X'], c2['x'], S)
    return (c2, (poses, gaps), rr.ransac(c2['X'], c2['x'], S, c2['thr2'], dtype=float, poses=poses),
            rr.ransac(c2['X'], c2['x'], S, c2['thr2'], poses=poses))


@pytest.mark.parametrize('kind', ('late', 'tie'))
def test_crafted_samples(kind):
    c, cand, a, b = crafted(kind)
    check_ransac_seed(c, cand, a, b)
    counts = {k: max(cnt for kk, q, cnt, e2 in b['e2'] if kk == k) for k in c['where']}
    print('%s: winner sample %d with %d inliers; the winning triple at %s counts %s' % (kind, b['sample'], b['count'], c['where'], counts))
    assert b['sample'] == c['where'][0] and b['count'] == 46 and set(counts.values()) == {46}


@functools.lru_cache(maxsize=None)
def use_case():
    """The case of 65 points with two inliers that may not be used, one of them in the winning sample, and NaN in their
    coordinates: (case, use, float64 route, np.longdouble route)."""
    c, _, _, b0 = ransac_seeded(6, 65, 64)
    off = [int(c['samples'][b0['sample']][0])]
    off.append(int(next(q for q in np.flatnonzero(b0['mask']) if q not in c['samples'][b0['sample']])))
    use = np.ones(65, bool)
    use[off] = False
    poses, gaps = rr.candidates(c['X'], c['x'], c['samples'], use)
    return (c, use, (poses, gaps), rr.ransac(c['X'], c['x'], c['samples'], c['thr2'], use, float, poses),
            rr.ransac(c['X'], c['x'], c['samples'], c['thr2'], use, poses=poses))


def test_use_case():
    c, use, cand, a, b = use_case()
    b0 = ransac_seeded(6, 65, 64)[3]
    check_ransac_seed(c, cand, a, b)
    print('use: winner sample %d (all usable: %d) with %d inliers (%d)' % (b['sample'], b0['sample'], b['count'], b0['count']))
    assert b['sample'] != b0['sample'] and b['count'] == b0['count'] - 2 and not b['mask'][~use].any()
    assert use[c['samples'][b['sample']]].all()


# ---- 3b: camcal with three control points swapped ---------------------------------------------------------------------------

def swapped_camcal():
    """(good, bad): camcal_struct() and a copy with the coordinates of its first three control points swapped among
    themselves."""
    import copy
    from helpers import camcal_struct
    good = camcal_struct(3)
    ctrl = np.flatnonzero(good.prior.OP.isCtrl)[:3]
    bad = copy.deepcopy(good)
    bad.OP.val[:, ctrl] = good.OP.val[:, np.roll(ctrl, 1)]
    return good, bad


def test_camcal_swapped_control_points():
    """What the GPU pipeline test asserts, from the restatements: plain resect(n = 1) from the four control points puts
    every camera more than 1.5 units (the control points span a unit square) from PhotoModeler's station, and the
    RANSAC with the least-squares pose on its inliers puts the cameras tried here within 0.3 of it (measured over all
    21: at most 0.212, camera 20; the others at most 0.048).  The bundle from those values converges to the report's
    sigma0 of 1.6148; from the plain ones it does not converge."""
    import initial_oracle as IO_
    good, bad = swapped_camcal()
    blank = I.cleareo(bad)
    cp = good.OP.id[good.prior.OP.isCtrl]
    h, rms, fail = IO_.resect(blank, 'all', cp, 1, 0, cp)
    d_plain = np.linalg.norm(h.EO.val[:3] - good.EO.val[:3], axis=0)
    assert not fail and d_plain.min() > 1.5
    rng = np.random.default_rng(0)
    xy = I.lenscorr1(blank)
    for ci in range(21):
        rows, xn, w = I.camera_points(blank, ci, None, xy)
        S = I.draw_triples(rows.size, 256, rng)
        if ci not in (0, 20):
            continue
        X = blank.OP.val[:, blank.IP.pt[rows]]
        thr = 3.0 * np.mean(blank.IO.sensor.pxSize[:, ci]) / abs(blank.IO.val[0, ci])
        r = rr.ransac(X, xn, S, thr ** 2, dtype=float)
        a = po.adjust(X, xn, np.asarray(r['P'], float), use=r['mask'], w=w)
        d = np.linalg.norm(np.asarray(a['C'], float) - good.EO.val[:3, ci])
        print('camera %d: %d of %d inliers, code %d, sigma0 %.2f, %.3f from the station (plain: %.3f)' % (ci, r['count'], rows.size, a['code'], a['sigma0'], d, d_plain[ci]))
        assert a['code'] == 0 and r['count'] >= 30 and d < 0.3


# ---- 4: the ABI and the refusals, before any device call ------------------------------------------------------------------

def test_symbols_declared():
    hdr = open(os.path.join(ROOT, 'include', 'dbat_hip.h')).read()
    assert re.search(r'#define DBAT_HIP_ABI_VERSION 5\b', hdr) and _hip.ABI_VERSION == 5
    for name in ('dbat_hip_resect_ransac', 'dbat_hip_poseadjust'):
        assert re.search(r'\bint\s+%s\(' % name, hdr), name
        assert name in _hip.SYMBOLS
    lib = _hip.load()
    assert lib.dbat_hip_abi_version() == 5
    import inspect
    sig = inspect.signature(I.resect_robust).parameters
    assert [(k, sig[k].default) for k in list(sig)[1:]] == [('cams', 'all'), ('cpId', None), ('n_hyp', 256), ('thr_px', 3.0), ('seed', 0),
                                                           ('refine', True), ('reselect', 0), ('max_iter', 20), ('conv_tol', 1e-6), ('device', 0)]


def einval(fn, *a, **kw):
    with pytest.raises(_hip.DbatHipError) as ei:
        fn(*a, **kw)
    assert ei.value.code == _hip.EINVAL, ei.value
    return str(ei.value)


def passes_checks(fn, **kw):
    """What passes every check ends at the device: without one that is the only error left."""
    try:
        fn(**kw)
    except _hip.DbatHipError as e:
        assert e.code == _hip.EDEVICE, e


put = lambda a, idx, v: (lambda b: (b.__setitem__(idx, v), b)[1])(np.array(a, float))
two = lambda a: np.concatenate([a, a], 1)


def test_poseadjust_refusals_without_device():
    _hip.load()
    c = po.seeded_case(5, 5e-4)
    P = np.stack([c['P0']] * 2)
    base = dict(pt_start=[0, 5, 10], X=two(c['X']), xn=two(c['x']), P=P)
    call = lambda **kw: einval(_hip.poseadjust, **{**base, **kw})
    for bad in (np.nan, np.inf):
        assert 'not finite' in call(X=put(base['X'], (2, 7), bad))
        assert 'not finite' in call(xn=put(base['xn'], (0, 3), bad))
        assert 'weight' in call(w=put(np.ones((2, 10)), (1, 2), bad))
        assert 'P of camera' in call(P=put(P, (1, 2, 3), bad))
        assert 'P of camera' in call(P=put(P, (0, 1, 1), bad))
    use = np.ones(10, bool)
    use[7] = False                     # a point that is not to be used may be anything
    passes_checks(_hip.poseadjust, **{**base, 'X': put(base['X'], (2, 7), np.nan), 'use': use})
    for w in (0.0, -1.0):
        assert 'weight' in call(w=put(np.ones((2, 10)), (0, 9), w))
    Rbad = P.copy()
    Rbad[1, :, :3] = Rbad[1, :, :3] @ np.diag([1.0, 1.0, 1.0 + 1e-5])
    assert 'rotation' in call(P=Rbad)
    Rneg = P.copy()
    Rneg[0, :, :3] = -Rneg[0, :, :3]
    assert 'rotation' in call(P=Rneg)
    for mi in (0, -1, 201):
        assert 'max_iter' in call(max_iter=mi)
    for tol in (0.0, -1e-6, np.nan):
        assert 'conv_tol' in call(conv_tol=tol)
    for ang in (1e-3, -1e-3, np.nan):
        assert 'min_angle' in call(min_angle=ang)
    assert 'ascend' in call(pt_start=[0, 6, 5], X=base['X'][:, :5], xn=base['xn'][:, :5])
    assert 'start at 0' in call(pt_start=[1, 5, 10])
    passes_checks(_hip.poseadjust, **base)


def test_resect_ransac_refusals_without_device():
    _hip.load()
    c = rr.seeded_case(3, 5, 4)
    smp = np.concatenate([c['samples'], c['samples']])
    base = dict(pt_start=[0, 5, 10], X=two(c['X']), xn=two(c['x']), smp_start=[0, 4, 8], samples=smp, thr2=c['thr2'])
    call = lambda **kw: einval(_hip.resect_ransac, **{**base, **kw})
    for bad in (np.nan, np.inf):
        assert 'not finite' in call(X=put(base['X'], (1, 8), bad))
        assert 'not finite' in call(xn=put(base['xn'], (1, 0), bad))
        assert 'thr2' in call(thr2=[c['thr2'], bad])
    for t in (0.0, -1.0):
        assert 'thr2' in call(thr2=t)
    use = np.ones(10, bool)
    use[8] = False
    passes_checks(_hip.resect_ransac, **{**base, 'X': put(base['X'], (1, 8), np.nan), 'use': use})
    s = smp.copy()
    s[5] = (0, 1, 5)
    assert 'outside' in call(samples=s)
    s[5] = (0, -1, 2)
    assert 'outside' in call(samples=s)
    s[5] = (2, 4, 2)
    assert 'repeats' in call(samples=s)
    assert 'ascend' in call(pt_start=[0, 6, 5], X=base['X'][:, :5], xn=base['xn'][:, :5])
    assert 'ascend' in call(smp_start=[0, 9, 8])
    assert 'start at 0' in call(pt_start=[1, 5, 10])
    assert 'start at 0' in call(smp_start=[1, 4, 8])
    passes_checks(_hip.resect_ransac, **base)


# ---- 5: the samples -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', (3, 4, 15, 16, 1000))
def test_draw_triples(n):
    S = I.draw_triples(n, 300, np.random.default_rng(n))
    assert S.shape == (300, 3) and S.dtype == np.int32 and S.min() >= 0 and S.max() < n
    srt = np.sort(S, 1)
    assert np.all(srt[:, 1:] != srt[:, :-1])
    assert np.array_equal(S, I.draw_triples(n, 300, np.random.default_rng(n)))
    if n >= 4:
        assert len({tuple(r) for r in srt.tolist()}) > 1
    with pytest.raises(ValueError):
        I.draw_triples(2, 1, np.random.default_rng(0))
