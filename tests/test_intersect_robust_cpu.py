"""Robust forward intersection without a GPU (dbat_hip_intersect_ransac, dbat_hip_pointadjust;
dbat_amd.initial.forwintersect_robust): the NumPy restatements of tests/pointadjust_ref.py and
tests/intersect_ransac_ref.py against the truth and against oracle/dbat_oracle.bundle on a project with every camera and
the IO fixed, the seeded cases that tests/test_intersect_robust_gpu.py runs on the device with the properties their seeds
were chosen for, the ABI, what the library refuses before it touches a device (every case of the list but 2^31 samples in one point: test_ray_cap
says why), the sample plan and draw_pairs.

The oracle test: bundle() with every camera and the IO fixed minimises, point by point, the same objective (no
distortion, the weights |f| / (pxSize IP.std)), so the points are the same numbers from independent code, and the 3 x 3
blocks of its OP covariance ('cop': s0^2 times the blocks of inv(J'J), with the oracle's s0 over all points) are
s0^2 Q of every point.  The bounds are those test_resect_robust_cpu.test_oracle uses for the same comparison: the
points 1e-8 of the scene's size, the covariance blocks 1e-6 of their largest entry."""
import functools
import os
import re

import numpy as np
import pytest

import dbat_oracle as o
import intersect_ransac_ref as ir
import pointadjust_ref as pr
from dbat_amd import _hip
from dbat_amd import initial as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = 10.0                                 # the radius of the ring of cameras: the size of the scene
SHIFT = (6.5e5, 6.2e6, 100.0)


# ---- 1: truth and conditioning of the adjustment --------------------------------------------------------------------------

CASES = [(r, noise) for r in pr.RAYS for noise in pr.NOISES]


@functools.lru_cache(maxsize=None)
def seeded(r, noise, shifted=False):
    """(the case, the float64 restatement's result, the np.longdouble one's)."""
    c = pr.seeded_case(r, noise, shift=SHIFT if shifted else None)
    return c, pr.run_case(c), pr.run_case(c, np.longdouble)


def stat_of(r, noise):
    """sigma0 and Q are compared where there is noise and redundancy."""
    return noise > 0 and r >= 3


@pytest.mark.parametrize('r,noise', CASES)
def test_seeded_cases(r, noise):
    c, a, b = seeded(r, noise)
    dX = np.abs(np.asarray(b['X'] - c['X'], float)).max()
    print('r %3d noise %.0e: %d / %d iterations, %d / %d trials, sigma0 %.3e, float64 to longdouble %.2e; to the truth %.2e'
          % (r, noise, a['iters'], b['iters'], a['trials'], b['trials'], a['sigma0'], pr.distance(a, b, stat_of(r, noise), SCALE), dX))
    assert a['code'] == 0 and b['code'] == 0 and a['n'] == r and np.array_equal(a['used'], b['used'])
    assert np.all(np.isfinite(a['X'])) and np.all(np.isfinite(a['Q']))
    assert pr.distance(a, b, stat_of(r, noise), SCALE) < 1e-11
    if noise == 0:
        assert dX < 1e-13 * SCALE and a['f'] <= pr.FLOOR * 2 * r * 10          # rounding
    elif r >= 16:
        assert dX < 0.01 and abs(float(a['sigma0']) - 1) < 0.3                  # the noise is 5e-4 and the weight 2000


def test_noise_free_floor():
    """The worst float64-to-longdouble distance of the noise-free cases: what FLOOR of the GPU tests is ten times of."""
    d = {r: pr.distance(seeded(r, 0.0)[1], seeded(r, 0.0)[2], False, SCALE) for r in pr.RAYS}
    worst = max(d, key=d.get)
    print('noise-free cases: float64 to longdouble at most %.3e (r = %d)' % (d[worst], worst))
    assert d[worst] < 1e-14


def test_shifted_case_is_the_same_case():
    c, a, b = seeded(9, 5e-4, True)
    _, a0, b0 = seeded(9, 5e-4)
    sh = np.asarray(SHIFT, np.longdouble)
    d = np.abs(np.asarray(a['X'], np.longdouble) - sh - b0['X']).max()
    print('r 9 shifted by %s m: float64 to the unshifted longdouble %.2e, longdouble to it %.2e' % (SHIFT, d, np.abs(b['X'] - sh - b0['X']).max()))
    assert a['code'] == 0 and b['code'] == 0
    assert float(np.abs(b['X'] - sh - b0['X']).max()) < 1e-9          # -R C of the cameras is rounded to float64 at 6e6 m
    assert float(d) < 1e-8


# ---- 1b: the statuses --------------------------------------------------------------------------------------------------------

def status_cases():
    """label -> (arguments of pr.adjust, the code): one case per code 1 .. 4.  Code 2 comes from a start far in front of the
    cameras: a start behind them leaves no ray to use -- the selection rule -- and is code 4."""
    c = seeded(8, 5e-4)[0]
    base = dict(cam=c['cam'], xn=c['x'], P=c['P'], X0=c['X0'], w=pr.WEIGHT, conv_tol=pr.CONV_TOL, max_iter=pr.MAX_ITER)
    eye = lambda C: np.hstack([np.eye(3), -np.asarray(C, float)[:, None]])
    # two cameras looking along -z, the point 5 in front; from a start 1e11 in front every damped step (the Gauss-Newton
    # step is z^2 / 5 long and Marquardt's scaling shortens it by 1 + lambda <= 1e8 only) lands behind the cameras
    P2 = np.stack([eye([-1, 0, 0]), eye([1, 0, 0])])
    far = dict(cam=[0, 1], xn=np.array([[-0.2, 0.2], [0.0, 0.0]]), P=P2, X0=[0.0, 0.0, -1e11], w=pr.WEIGHT, conv_tol=pr.CONV_TOL, max_iter=pr.MAX_ITER)
    # two rays that meet at 1e-9 rad, at their intersection, off the cameras' axis: the pivot of the depth is 1e-18 of its
    # diagonal entry (on the axis the entry itself would be as small, and the test is relative)
    Pn = np.stack([eye([0, 0, 0]), eye([1e-8, 0, 0])])
    Xn = np.array([3.0, 1.0, -10.0])
    near = dict(cam=[0, 1], xn=pr.project(Pn, np.array([0, 1]), Xn)[0], P=Pn, X0=Xn, w=pr.WEIGHT, conv_tol=pr.CONV_TOL, max_iter=pr.MAX_ITER)
    one = dict(base, use=np.arange(8) == 3)
    behind = dict(far, X0=[0.0, 0.0, 5.0])                 # the same two rays from a start behind both cameras: no ray to use
    return {'max_iter': (dict(base, max_iter=1), 1), 'no_step': (far, 2), 'singular': (near, 3), 'too_few': (one, 4), 'behind': (behind, 4)}


@pytest.mark.parametrize('label', ('max_iter', 'no_step', 'singular', 'too_few', 'behind'))
def test_statuses(label):
    kw, code = status_cases()[label]
    a, b = pr.adjust(**kw), pr.adjust(dtype=np.longdouble, **kw)
    print('%s: code %d / %d, %d iterations, %d trials, lambda %.0e' % (label, a['code'], b['code'], a['iters'], a['trials'], a['lam']))
    assert a['code'] == b['code'] == code
    assert np.all(np.isfinite(a['X'])) and np.all(np.isfinite(a['res']))
    if code in (3, 4):
        assert np.all(np.isnan(a['Q']))
    if code == 4:
        assert np.array_equal(a['X'], np.asarray(kw['X0'], float)) and np.isnan(a['f']) and a['lam'] == 1e-3
        assert a['n'] == (0 if label == 'behind' else 1)
    if code == 2:
        assert a['iters'] == 0 and a['trials'] == 12 and a['lam'] > 1e8


# ---- 2: the oracle ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def oracle_case(npt=12, seed=4, noise_px=0.7):
    """A project of six cameras without distortion, every camera and the IO fixed, anisotropic IP.std, noise of 0.7 px,
    points of 3 .. 6 rays at perturbed starts; and the same rays as the restatement takes them."""
    from dbat_amd import synth
    from dbat_amd.dbatstruct import make_struct
    nc = 6
    P, C = pr.cameras(seed, nc)
    rng = np.random.default_rng(400 + seed)
    IO = np.zeros((10, nc))
    IO[0], IO[1], IO[2] = 7.5, 0.11, -0.07
    EO = np.zeros((6, nc))
    for i in range(nc):
        EO[:3, i], EO[3:6, i] = C[:, i], I.derotmat3d(P[i][:, :3])
    X = rng.uniform(-2, 2, (3, npt))
    cam, pt = [], []
    for p in range(npt):                                 # image-major below: sorted by camera
        for i in np.sort(rng.choice(nc, int(rng.integers(3, 7)), replace=False)):
            cam.append(int(i)); pt.append(p)
    order = np.lexsort((pt, cam))
    cam, pt = np.array(cam)[order], np.array(pt)[order]
    px = 0.005
    ip = synth.project(IO, EO, X, cam, pt, px)[0] + noise_px * rng.normal(size=(2, cam.size))
    std = np.stack([rng.uniform(0.5, 1.0, cam.size), rng.uniform(1.0, 2.0, cam.size)])
    X0 = X + 0.05 * rng.normal(size=X.shape)
    s = make_struct(IO, EO, X0, np.asfortranarray(ip), cam, pt, px, ip_std=std, distModel=3, estEO=np.zeros((6, nc), bool))
    # the rays as the product forms them, from formulas of this file: no distortion, y up, -f
    xn = np.stack([(px * ip[0] - IO[1, cam]) / -IO[0, cam], (-px * ip[1] - IO[2, cam]) / -IO[0, cam]])
    w = np.abs(IO[0, cam]) / (px * std)
    Pe = np.stack([np.hstack([R, -(R @ EO[:3, i])[:, None]]) for i in range(nc) for R in (I.rotmat3d(EO[3:6, i]),)])
    return dict(s=s, cam=cam, pt=pt, xn=xn, w=w, P=Pe, X0=X0, npt=npt)


def test_oracle():
    c = oracle_case()
    s2, ok, iters, s0, E = o.bundle(c['s'], 50, 'gna', 1e-7)        # (at 1e-9 its line search ends in the noise of the objective)
    assert ok and E.code == 0
    COP = np.asarray(o.bundle_cov(s2, E, 'cop').todense())
    worst = [0.0, 0.0]
    fsum = dof = 0.0
    for p in range(c['npt']):
        rows = np.flatnonzero(c['pt'] == p)
        a = pr.adjust(c['cam'][rows], c['xn'][:, rows], c['P'], c['X0'][:, p], w=c['w'][:, rows], max_iter=50, conv_tol=1e-9)
        assert a['code'] == 0 and a['n'] == rows.size
        blk = COP[3 * p:3 * p + 3, 3 * p:3 * p + 3]
        worst[0] = max(worst[0], np.abs(a['X'] - s2.OP.val[:, p]).max() / SCALE)
        worst[1] = max(worst[1], np.abs(s0 ** 2 * a['Q'] - blk).max() / np.abs(blk).max())
        fsum += float(a['f']); dof += 2 * rows.size - 3
    print('oracle: bundle() %d iterations, sigma0 %.6f; differences X %.1e cov %.1e sigma0 (pooled) %.1e' % (iters, s0, *worst, abs(np.sqrt(fsum / dof) / s0 - 1)))
    assert worst[0] < 1e-8 and worst[1] < 1e-6 and abs(np.sqrt(fsum / dof) / s0 - 1) < 1e-10


# ---- 3: the RANSAC seeds shared with the GPU tests ------------------------------------------------------------------------

# (seed, rays, samples; 0: every pair): enumerated points of 2, 3, 11 (55 pairs), 12 (66: two rounds) and 64 rays, and
# sample lists around the round of 64
RANSAC_CASES = [(1, 2, 0), (2, 3, 0), (3, 11, 0), (4, 12, 0), (5, 64, 0), (6, 20, 63), (7, 20, 64), (8, 20, 65), (9, 30, 129)]
MARGIN = 1e-9


@functools.lru_cache(maxsize=None)
def ransac_seeded(seed, r, ns, shifted=False):
    """(the case, the float64 route's result, the np.longdouble one's)."""
    c = ir.seeded_case(seed, r, ns, shift=SHIFT if shifted else None)
    return c, ir.run_case(c, float), ir.run_case(c)


def check_ransac_seed(a, b):
    """Both routes pick the same winner, and in np.longdouble no ray under any scored hypothesis lies within MARGIN
    relative of its threshold, no pair within MARGIN relative of the parallax cut and no ray that could count within MARGIN
    of the plane of its camera: the device may be compared with them in integers."""
    assert (a['sample'], a['count'], a['scored'], a['usable']) == (b['sample'], b['count'], b['scored'], b['usable']) and np.array_equal(a['mask'], b['mask'])
    for k, cnt, e2 in b['e2']:
        assert e2.size == 0 or np.abs(np.asarray(e2, float) - 1).min() > MARGIN, 'sample %d: a residual at the threshold' % k
    assert b['s2'].size == 0 or np.abs(np.asarray(b['s2'], float) / b['par2'] - 1).min() > MARGIN, 'a pair at the parallax cut'
    # the in-front test decides counts too: the depth of every usable ray is more than MARGIN of the ray's length from
    # zero -- or the ray is no inlier on either side of the camera (a hypothesis at a projection centre: the residual is
    # a quotient by that depth, far above the threshold or not finite, so the comparison with thr2 fails whatever the sign)
    for k, zr, e2 in b['z']:
        zr, e2 = np.asarray(zr, float), np.asarray(e2, float)
        assert np.all((np.abs(zr) > MARGIN) | ~(e2 <= 1 + MARGIN)), 'sample %d: a ray at the plane of its camera that could count' % k


@pytest.mark.parametrize('seed,r,ns', RANSAC_CASES)
def test_ransac_seeds(seed, r, ns):
    c, a, b = ransac_seeded(seed, r, ns)
    print('seed %d, %d rays (%s replaced), %d samples: %d hypotheses, winner sample %d with %d inliers'
          % (seed, r, c['outliers'].tolist(), ns, b['scored'], b['sample'], b['count']))
    check_ransac_seed(a, b)
    assert b['scored'] == (ns if ns else r * (r - 1) // 2)
    # the winner marks exactly the planted rays as outliers, and the point is the truth within the noise
    assert b['count'] == r - c['outliers'].size and np.array_equal(np.flatnonzero(~b['mask']), c['outliers'])
    assert np.abs(np.asarray(b['X'] - c['X'], float)).max() < 0.05
    if ns == 0:
        S = ir.pairs(r)
        assert all(ir.pair_number(i, j, r) == k for k, (i, j) in enumerate(S.tolist()))


def test_ransac_shifted_seed():
    c, a, b = ransac_seeded(3, 11, 0, True)
    check_ransac_seed(a, b)
    b0 = ransac_seeded(3, 11, 0)[2]
    assert (b['sample'], b['count']) == (b0['sample'], b0['count']) and np.array_equal(b['mask'], b0['mask'])


@functools.lru_cache(maxsize=None)
def crafted(kind):
    """kind -> (arguments of ir.ransac, what the test expects of the result).
      tie        four noise-free rays: every pair counts four, the lowest sample wins; listed: the samples (2,3) (0,1) (2,3)
      use        the case (7, 20, 64) with a ray of its winning sample taken out
      late       the case (9, 30, 129) with a replaced ray put into every sample but the last: the third round of 64
      late_enum  twelve noise-free rays of which only the last two may be used: pair number 65 of 66, the second round
      min_angle  three rays, two of them 12 degrees apart, at min_angle = 20 degrees
      same_cam   three rays, the first two of one camera (one of them moved): their pair is the projection centre
      parallel   two parallel rays of two cameras; none: no ray; one: one ray"""
    P = pr.cameras(0)[0]
    eye = lambda C: np.hstack([np.eye(3), -np.asarray(C, float)[:, None]])
    thr2 = ir.THR ** 2
    if kind in ('tie', 'tie_listed'):
        cam = np.array([0, 3, 6, 9])
        x = pr.project(P, cam, [0.3, -0.2, 0.5])[0]
        smp = np.array([[2, 3], [0, 1], [2, 3]], np.int32) if kind == 'tie_listed' else None
        return dict(cam=cam, xn=x, P=P, thr2=thr2, samples=smp), dict(count=4, sample=0)
    if kind == 'use':
        c, _, b = ransac_seeded(7, 20, 64)
        use = np.ones(20, bool)
        use[c['samples'][b['sample']][0]] = False
        return dict(cam=c['cam'], xn=c['x'], P=c['P'], thr2=c['thr2'], samples=c['samples'], use=use), dict(count=b['count'] - 1)
    if kind == 'late':
        c, _, b = ransac_seeded(9, 30, 129)
        S = c['samples'].copy()
        T = S[b['sample']].copy()
        for k in range(len(S)):
            if not np.isin(S[k], c['outliers']).any():
                S[k, 0] = next(q for q in c['outliers'] if q != S[k, 1])
        S[128] = T
        return dict(cam=c['cam'], xn=c['x'], P=c['P'], thr2=c['thr2'], samples=S), dict(count=b['count'], sample=128)
    if kind == 'late_enum':
        cam = (np.arange(12) * 5) % 12
        x = pr.project(P, cam, [0.3, -0.2, 0.5])[0]
        return dict(cam=cam, xn=x, P=P, thr2=thr2, use=np.arange(12) >= 10), dict(count=2, sample=65, scored=1)
    if kind == 'min_angle':
        Pm = np.stack([eye([-1, 0, 0]), eye([1, 0, 0]), eye([9, 0, 0])])        # seen from (0, 0, -9.4): 12 and 37 degrees
        cam = np.array([0, 1, 2])
        x = pr.project(Pm, cam, [0.0, 0.1, -9.4])[0]
        return dict(cam=cam, xn=x, P=Pm, thr2=thr2, min_angle=np.deg2rad(20.0)), dict(count=3, sample=1, scored=2)
    if kind == 'same_cam':
        cam = np.array([2, 2, 7])
        x = pr.project(P, cam, [0.3, -0.2, 0.5])[0]
        x[:, 1] += 0.05
        return dict(cam=cam, xn=x, P=P, thr2=thr2), dict(count=2, sample=1, scored=3)
    if kind == 'parallel':
        return dict(cam=np.array([0, 1]), xn=np.array([[0.1, 0.1], [0.2, 0.2]]), P=np.stack([eye([-1, 0, 0]), eye([1, 0, 0])]), thr2=thr2), dict(count=0, sample=-1, scored=0)
    n = 0 if kind == 'none' else 1
    return dict(cam=np.zeros(n, int), xn=np.full((2, n), 0.1), P=P, thr2=thr2), dict(count=0, sample=-1, scored=0)


CRAFTED = ('tie', 'tie_listed', 'use', 'late', 'late_enum', 'min_angle', 'same_cam', 'parallel', 'none', 'one')


@pytest.mark.parametrize('kind', CRAFTED)
def test_crafted(kind):
    kw, want = crafted(kind)
    a, b = ir.ransac(dtype=float, **kw), ir.ransac(**kw)
    print('%s: winner sample %d with %d inliers of %d usable, %d hypotheses' % (kind, b['sample'], b['count'], b['usable'], b['scored']))
    check_ransac_seed(a, b)
    for key, v in want.items():
        assert b[key] == v, (key, b[key], v)
    if want['count'] == 0:
        assert b['X'] is None and not b['mask'].any() and b['ssq'] == 0
    if kind == 'use':
        assert not b['mask'][~kw['use']].any() and kw['use'][b['samples'][b['sample']]].all() and b['sample'] != ransac_seeded(7, 20, 64)[2]['sample']


# ---- 4: the ABI and the refusals, before any device call ------------------------------------------------------------------

def test_symbols_declared():
    hdr = open(os.path.join(ROOT, 'include', 'dbat_hip.h')).read()
    assert re.search(r'#define DBAT_HIP_ABI_VERSION 5\b', hdr) and _hip.ABI_VERSION == 5
    for name in ('dbat_hip_intersect_ransac', 'dbat_hip_pointadjust'):
        assert re.search(r'\bint\s+%s\(' % name, hdr), name
        assert name in _hip.SYMBOLS
    lib = _hip.load()
    assert lib.dbat_hip_abi_version() == 5
    assert hasattr(lib, 'dbat_hip_debug_intersect_robust_timing') and hasattr(lib, 'dbat_hip_debug_intersect_robust_ms')
    import inspect
    sig = inspect.signature(I.forwintersect_robust).parameters
    assert [(k, sig[k].default) for k in list(sig)[1:]] == [('ids', 'all'), ('skipPrior', False), ('n_hyp', 256), ('thr_px', 3.0), ('min_angle_deg', 0.0),
                                                           ('min_count', 2), ('seed', 0), ('refine', True), ('reselect', 0), ('max_iter', 20),
                                                           ('conv_tol', 1e-6), ('device', 0)]


def einval(fn, *a, **kw):
    with pytest.raises(_hip.DbatHipError) as ei:
        fn(*a, **kw)
    assert ei.value.code == _hip.EINVAL, ei.value
    return str(ei.value)


def passes_checks(fn, **kw):
    """What passes every check ends at the device: without one that is the only error left."""
    import torch
    try:
        fn(**kw)
    except _hip.DbatHipError as e:
        assert e.code == _hip.EDEVICE, e
    else:
        assert torch.cuda.is_available()


put = lambda a, idx, v: (lambda b: (b.__setitem__(idx, v), b)[1])(np.array(a, float))


def refusal_base():
    """Two points of five rays each over the twelve cameras."""
    c = pr.seeded_case(5, 5e-4)
    two = lambda a: np.concatenate([a, a], -1)
    return c, dict(ray_start=[0, 5, 10], cam=two(c['cam']), xn=two(c['x']), P=c['P'])


def bad_poses(P):
    Rbad = P.copy()
    Rbad[1, :, :3] = Rbad[1, :, :3] @ np.diag([1.0, 1.0, 1.0 + 1e-5])
    Rneg = P.copy()
    Rneg[0, :, :3] = -Rneg[0, :, :3]
    return Rbad, Rneg


def test_pointadjust_refusals_without_device():
    _hip.load()
    c, base = refusal_base()
    base['X'] = np.stack([c['X0'], c['X0']], 1)
    call = lambda **kw: einval(_hip.pointadjust, **{**base, **kw})
    for bad in (np.nan, np.inf):
        assert 'xn of ray' in call(xn=put(base['xn'], (0, 3), bad))
        assert 'X of point' in call(X=put(base['X'], (2, 1), bad))
        assert 'weight' in call(w=put(np.ones((2, 10)), (1, 2), bad))
        assert 'P of camera' in call(P=put(base['P'], (1, 2, 3), bad))
        assert 'P of camera' in call(P=put(base['P'], (0, 1, 1), bad))
    use = np.ones(10, bool)
    use[7] = False                     # a ray that is not to be used may be anything
    passes_checks(_hip.pointadjust, **{**base, 'xn': put(base['xn'], (1, 7), np.nan), 'use': use})
    use[5:] = False                    # and so may the start of a point without a ray to use
    passes_checks(_hip.pointadjust, **{**base, 'X': put(base['X'], (0, 1), np.nan), 'use': use})
    for w in (0.0, -1.0):
        assert 'weight' in call(w=put(np.ones((2, 10)), (0, 9), w))
    for Pb in bad_poses(base['P']):
        assert 'rotation' in call(P=Pb)
    for cm in (-1, 12):
        assert 'cam of ray' in call(cam=put(base['cam'], 6, cm).astype(int))
    for mi in (0, -1, 201):
        assert 'max_iter' in call(max_iter=mi)
    for tol in (0.0, -1e-6, np.nan):
        assert 'conv_tol' in call(conv_tol=tol)
    for ang in (1e-3, -1e-3, np.nan):
        assert 'min_angle' in call(min_angle=ang)
    assert 'ray_start' in call(ray_start=[0, 6, 5], cam=base['cam'][:5], xn=base['xn'][:, :5])
    assert 'start at 0' in call(ray_start=[1, 5, 10])
    passes_checks(_hip.pointadjust, **base)


def test_intersect_ransac_refusals_without_device():
    _hip.load()
    c, base = refusal_base()
    base['thr2'] = ir.THR ** 2
    call = lambda **kw: einval(_hip.intersect_ransac, **{**base, **kw})
    for bad in (np.nan, np.inf):
        assert 'xn of ray' in call(xn=put(base['xn'], (1, 0), bad))
        assert 'P of camera' in call(P=put(base['P'], (3, 0, 2), bad))
        assert 'thr2' in call(thr2=put(np.full(12, ir.THR ** 2), 4, bad))
    for t in (0.0, -1.0):
        assert 'thr2' in call(thr2=t)
    for Pb in bad_poses(base['P']):
        assert 'rotation' in call(P=Pb)
    for cm in (-1, 12):
        assert 'cam of ray' in call(cam=put(base['cam'], 6, cm).astype(int))
    for ang in (-1e-3, np.pi / 2, 2.0, np.nan):
        assert 'min_angle' in call(min_angle=ang)
    use = np.ones(10, bool)
    use[8] = False
    passes_checks(_hip.intersect_ransac, **{**base, 'xn': put(base['xn'], (1, 8), np.nan), 'use': use})
    smp = np.array([[0, 1], [1, 2], [3, 4], [4, 0]], np.int32)
    lists = dict(smp_start=[0, 2, 4], samples=smp)
    passes_checks(_hip.intersect_ransac, **{**base, **lists})
    for pair, what in (((0, 5), 'outside'), ((-1, 2), 'outside'), ((2, 2), 'repeats')):
        s = smp.copy()
        s[3] = pair
        assert what in call(smp_start=[0, 2, 4], samples=s)
    assert 'ray_start' in call(ray_start=[0, 6, 5], cam=base['cam'][:5], xn=base['xn'][:, :5])
    assert 'smp_start' in call(smp_start=[0, 3, 2], samples=smp[:2])
    assert 'start at 0' in call(ray_start=[1, 5, 10])
    assert 'start at 0' in call(smp_start=[1, 2, 4], samples=smp)
    # a point of more than 64 rays must bring samples: without a list, and with a list that is empty for it
    c65 = pr.seeded_case(65, 0.0)
    big = dict(ray_start=[0, 65], cam=c65['cam'], xn=c65['x'], P=c65['P'], thr2=ir.THR ** 2)
    assert 'more than 64 rays' in einval(_hip.intersect_ransac, **big)
    two = dict(big, ray_start=[0, 65, 65])
    assert 'more than 64 rays' in einval(_hip.intersect_ransac, **two, smp_start=[0, 0, 0], samples=np.zeros((0, 2)))
    passes_checks(_hip.intersect_ransac, **big, smp_start=[0, 1], samples=[[0, 64]])
    passes_checks(_hip.intersect_ransac, **base)


def test_null_arguments_and_counts():
    """What the Python bindings never pass: null pointers and negative counts, to the library itself."""
    import ctypes as C
    lib = _hip.load()
    rs = np.zeros(2, np.int64)
    d, i32, u8 = np.zeros(12), np.zeros(4, np.int32), np.zeros(1, np.uint8)
    dp, ip, bp, lp = _hip.dptr, lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)), lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8)), \
        lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    opt = _hip.PairOptions(20, 1e-6, 0.0)
    good_r = [0, 1, lp(rs), ip(i32), dp(d), 1, dp(np.array(np.eye(3, 4).flatten('F'))), None, None, None, dp(np.ones(1)), 0.0, dp(d), ip(i32), bp(u8), dp(d)]
    good_a = [0, 1, lp(rs), ip(i32), dp(d), 1, dp(np.array(np.eye(3, 4).flatten('F'))), None, None, C.byref(opt), dp(np.zeros(3)), bp(u8), dp(d), ip(i32), dp(d), dp(d)]
    for name, good, nulls in (('dbat_hip_intersect_ransac', good_r, (2, 6, 10, 12, 13, 15)), ('dbat_hip_pointadjust', good_a, (2, 6, 9, 10, 12, 13, 14))):
        fn = getattr(lib, name)
        assert fn(*good) != _hip.EINVAL
        for k in nulls:
            args = list(good)
            args[k] = None
            assert fn(*args) == _hip.EINVAL, (name, k)
        for k in (1, 5):
            args = list(good)
            args[k] = -1
            assert fn(*args) == _hip.EINVAL, (name, k)


def test_ray_cap():
    """2^29 rays in one point, to the library itself: ray_start = [0, 2^29] over zeroed cam and use that are never written
    (untouched pages), so that no ray is to be used and xn is never read.  For the RANSAC one listed sample keeps the rule
    of 64 rays from answering first.  One ray fewer passes every check (tried without a device only).  (The other cap of the list, 2^31 samples in one
    point, comes after the checks of the sample indices, which read every sample and need two distinct indices in each:
    reaching it takes 16 GiB of written samples, so no test of seconds does; the line that makes it is a copy of the ray
    cap's with the other shift.)"""
    import ctypes as C
    lib = _hip.load()
    n = 1 << 29
    cam, use, x = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros(2)
    d, i32, u8 = np.zeros(12), np.zeros(4, np.int32), np.zeros(1, np.uint8)
    Pf = np.array(np.eye(3, 4).flatten('F'))
    smp, ss = np.array([0, 1], np.int32), np.array([0, 1], np.int64)
    dp, ip, bp, lp = _hip.dptr, lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)), lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8)), \
        lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    opt = _hip.PairOptions(20, 1e-6, 0.0)
    import torch
    # one ray fewer passes every check and goes on to the device, where the call would upload the arrays: that half is
    # for a machine without one only (the xn given here is never read by the checks, and is not 2^30 doubles long)
    for rays, refused in ((n, True),) + (() if torch.cuda.is_available() else ((n - 1, False),)):
        rs = np.array([0, rays], np.int64)
        inl = np.zeros(rays, np.uint8) if not refused else u8          # (written only past the checks)
        code = lib.dbat_hip_intersect_ransac(0, 1, lp(rs), ip(cam), dp(x), 1, dp(Pf), bp(use), lp(ss), ip(smp), dp(np.ones(1)), 0.0, dp(d), ip(i32),
                                             bp(inl), dp(d))
        msg = _hip.last_error()
        if refused:
            assert code == _hip.EINVAL and '2^29 rays' in msg, (code, msg)
        else:
            assert code == _hip.EDEVICE, (code, msg)
        if refused:                                       # (the passing call of pointadjust would need a device to say more)
            code = lib.dbat_hip_pointadjust(0, 1, lp(rs), ip(cam), dp(x), 1, dp(Pf), bp(use), None, C.byref(opt), dp(np.zeros(3)), bp(u8), dp(d), ip(i32),
                                            dp(d), None)
            msg = _hip.last_error()
            assert code == _hip.EINVAL and '2^29 rays' in msg, (code, msg)


def test_pair_plan():
    """Which points bring samples: those with more pairs than n_hyp, and those of more than 64 rays however large n_hyp is
    (the library refuses such a point without samples)."""
    r = np.array([0, 1, 2, 10, 23, 24, 64, 65, 100])
    for n_hyp, listed in ((256, [24, 64, 65, 100]), (45, [23, 24, 64, 65, 100]), (5000, [65, 100]), (2016, [65, 100]), (2015, [64, 65, 100])):
        ns, ss, smp = I.pair_plan(r, n_hyp, np.random.default_rng(3))
        assert r[ns > 0].tolist() == listed and np.all(ns[ns > 0] == n_hyp) and np.array_equal(ss, np.concatenate([[0], np.cumsum(ns)]))
        assert smp.shape == (ss[-1], 2) and smp.dtype == np.int32
        for p in np.flatnonzero(ns):
            part = smp[ss[p]:ss[p + 1]]
            assert part.min() >= 0 and part.max() < r[p] and np.all(part[:, 0] != part[:, 1])
        assert np.all(r[ns == 0] <= I.MAX_EXHAUSTIVE_RAYS) and np.all((r * (r - 1) // 2)[ns == 0] <= n_hyp)
    assert I.MAX_EXHAUSTIVE_RAYS == ir.MAX_EXHAUSTIVE == 64
    ns, ss, smp = I.pair_plan(r[:5], 256, np.random.default_rng(3))
    assert not ns.any() and smp.shape == (0, 2)


# ---- 5: the samples -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', (2, 3, 15, 16, 1000))
def test_draw_pairs(n):
    S = I.draw_pairs(n, 300, np.random.default_rng(n))
    assert S.shape == (300, 2) and S.dtype == np.int32 and S.min() >= 0 and S.max() < n
    assert np.all(S[:, 0] != S[:, 1])
    assert np.array_equal(S, I.draw_pairs(n, 300, np.random.default_rng(n)))
    if n >= 3:
        assert len({tuple(sorted(r)) for r in S.tolist()}) > 1
    with pytest.raises(ValueError):
        I.draw_pairs(1, 1, np.random.default_rng(0))
