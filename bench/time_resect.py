"""Time of the robust resection on one GPU (dbat_hip_resect_ransac, dbat_hip_poseadjust): the device events of their
kernels (k_resect_ransac, k_poseadjust) and the wall time of each call with its copies, on
  small  1000 cameras of 50 points
  large  5000 cameras of 1000 points
(cameras 10 .. 40 m over a field of points, image noise 5e-4, 30 % of the image points moved by 0.05 .. 0.3, threshold
2e-3, 256 samples per camera, weights 2000; the adjustment starts from the RANSAC's poses on its inliers).  After two
warm-up calls every figure is the median of REPS calls, with the smallest and the largest.  Beside each case the only
other route to the least-squares pose: bundle(s1, 20, 'gna') on the one-camera struct of a camera with every object
point fixed, from the same start -- wall time per camera over ten cameras, a warm-up camera before them.
bench/time_resect.py [small | large ...]"""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from dbat_amd import _hip, bundle
from dbat_amd import initial as I
from dbat_amd.dbatstruct import make_struct

SIZES = {'small': (1000, 50), 'large': (5000, 1000)}
REPS, N_HYP, WEIGHT, F_MM, PX, THR, NOISE, OUTLIERS = 10, 256, 2000.0, 10.0, 0.005, 2e-3, 5e-4, 0.3    # WEIGHT = F_MM / PX
BUNDLE_CAMERAS = 10


def stat(v):
    v = np.sort(np.asarray(v, float))
    return '%.3f (%.3f .. %.3f)' % (np.median(v), v[0], v[-1])


def camera(rng, n):
    """(X 3 x n, xn 2 x n): a camera looking down (-z) with up to 0.2 rad of tilt and any heading, n points of 2 m
    relief spread over its image format of +-0.6, noise and moved points as above."""
    C = np.array([rng.uniform(10, 30), rng.uniform(10, 30), rng.uniform(10, 40)])
    R = I.rotmat3d([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(-np.pi, np.pi)])
    x = rng.uniform(-0.6, 0.6, (2, n))
    d = R.T @ np.vstack([x, np.ones((1, n))])
    X = C[:, None] + (rng.uniform(0, 2.0, n) - C[2]) / d[2] * d
    x = x + NOISE * rng.standard_normal((2, n))
    out = rng.choice(n, int(OUTLIERS * n), replace=False)
    ang = rng.uniform(0, 2 * np.pi, out.size)
    x[:, out] += rng.uniform(0.05, 0.3, out.size) * np.stack([np.cos(ang), np.sin(ang)])
    return X, x


def camera_struct(X, xn, P):
    """The camera as a one-image struct with every object point fixed: a camera of 10 mm without distortion, pixels of
    5 um, the image points that normalise to xn, and the start pose P."""
    n = X.shape[1]
    IO = np.zeros((10, 1))
    IO[0] = F_MM
    EO = np.zeros((6, 1))
    EO[:3, 0], EO[3:6, 0] = -P[:, :3].T @ P[:, 3], I.derotmat3d(P[:, :3])
    xy = xn * -F_MM                                                # normalised = (xy - pp) / -f
    ip = np.stack([xy[0] / PX, -xy[1] / PX])
    return make_struct(IO, EO, X, np.asfortranarray(ip), np.zeros(n, int), np.arange(n), PX, ip_std=1.0, distModel=3, estOP=np.zeros((3, n), bool))


for name in sys.argv[1:] or ['small', 'large']:
    n_cams, n = SIZES[name]
    rng = np.random.default_rng(1)
    Xs, xs, smp = [], [], []
    for p in range(n_cams):
        X, x = camera(rng, n)
        Xs.append(X); xs.append(x); smp.append(I.draw_triples(n, N_HYP, rng))
    ps, hs = np.arange(n_cams + 1) * n, np.arange(n_cams + 1) * N_HYP
    X, xn, S = np.asfortranarray(np.concatenate(Xs, 1)), np.asfortranarray(np.concatenate(xs, 1)), np.concatenate(smp, 0)
    print('%s: %d camera(s) of %d points, %d samples each' % (name, n_cams, n, N_HYP), flush=True)
    _hip.resect_robust_timing(True)
    ms, wall, start = [], [], None
    for i in range(2 + REPS):
        t0 = time.perf_counter()
        start = _hip.resect_ransac(ps, X, xn, hs, S, THR ** 2)
        t = (time.perf_counter() - t0) * 1e3
        if i >= 2:
            wall.append(t); ms.append(_hip.resect_robust_ms()['ransac'])
    won = start['stats'][:, 1] >= 0
    print('  resect_ransac: wall %s ms   device: k_resect_ransac %s ms; per camera wall %.4f ms, device %.4f ms; %d of %d with a winner, '
          'inliers median %d, poses scored median %d' % (stat(wall), stat(ms), np.median(wall) / n_cams, np.median(ms) / n_cams, won.sum(), n_cams,
                                                         np.median(start['stats'][:, 0]), np.median(start['stats'][:, 3])), flush=True)
    P0 = np.where(won[:, None, None], start['P'], np.eye(3, 4))
    use = start['inlier']
    ms, wall, out = [], [], None
    for i in range(2 + REPS):
        t0 = time.perf_counter()
        out = _hip.poseadjust(ps, X, xn, P0, use=use, w=WEIGHT)
        t = (time.perf_counter() - t0) * 1e3
        if i >= 2:
            wall.append(t); ms.append(_hip.resect_robust_ms()['adjust'])
    codes = np.bincount(out['code'], minlength=5)
    print('  poseadjust: wall %s ms   device: k_poseadjust %s ms; per camera wall %.4f ms, device %.4f ms; codes 0..4: %s; iterations median %d '
          '(%d .. %d), trials median %d; sigma0 median %.4f' % (stat(wall), stat(ms), np.median(wall) / n_cams, np.median(ms) / n_cams, codes.tolist(),
                                                                np.median(out['iters']), out['iters'].min(), out['iters'].max(),
                                                                np.median(out['trials']), np.nanmedian(out['sigma0'])), flush=True)
    per_cam = np.median(wall) / n_cams
    tb, itb, s0b = [], [], []
    for j, p in enumerate(np.flatnonzero(won)[:BUNDLE_CAMERAS + 1]):
        sl = slice(ps[p], ps[p + 1])
        u = out['used'][sl]
        s1 = camera_struct(X[:, sl][:, u], xn[:, sl][:, u], P0[p])
        t0 = time.perf_counter()
        try:
            res, ok, iters, s0, E = bundle(s1, 20, 'gna')
        except _hip.DbatHipError as e:
            print('  bundle() refuses the one-camera struct: %s' % e, flush=True)
            break
        t = (time.perf_counter() - t0) * 1e3
        if j >= 1:
            tb.append(t); itb.append(iters); s0b.append(s0 / out['sigma0'][p] - 1)
    if tb:
        print('  bundle(s1, 20, \'gna\') on %d cameras: wall per camera %s ms, iterations %s, sigma0 against poseadjust within %.1e'
              % (len(tb), stat(tb), itb, np.abs(s0b).max()), flush=True)
        print('  ratio per camera, bundle() wall to poseadjust wall: %.0f' % (np.median(tb) / per_cam), flush=True)
