"""Time of the robust forward intersection on one GPU (dbat_hip_intersect_ransac, dbat_hip_pointadjust): the device events of
their kernels (k_intersect_ransac, k_pointadjust) and the wall time of each call with its copies, on
  C3  10^6 points x 10 rays from 1000 cameras
  C4  5 10^6 points x 10 rays from 5000 cameras
(the scenes of dbat_amd.synth at their true EO with 0.5 px of image noise; every pair of a point's rays enumerated on the
device, threshold 3 px, the adjustment from the RANSAC's points on its inliers with the weights of IP.std).  After two
warm-up calls every figure is the median of REPS calls, with the smallest and the largest.  Beside each case: the wall time
of Handle.forwintersect on the same scene -- k_forwintersect with the upload of x and the download of the points; the
library has no device events around that kernel (DESIGN.md 8 has its own time from a kernel trace of bench/forwintersect_calls.py) -- and the wall time of
the NumPy restatements (tests/intersect_ransac_ref.py in float64, tests/pointadjust_ref.py) on the first SAMPLE points,
scaled to the scene.
bench/time_intersect.py [C3 | C4 ...]"""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
from dbat_amd import _hip, synth
from dbat_amd import initial as I

REPS, THR_PX, SAMPLE = 10, 3.0, 200


def stat(v):
    v = np.sort(np.asarray(v, float))
    return '%.3f (%.3f .. %.3f)' % (np.median(v), v[0], v[-1])


def timed(fn, slot):
    ms, wall, out = [], [], None
    for i in range(2 + REPS):
        t0 = time.perf_counter()
        out = fn()
        t = (time.perf_counter() - t0) * 1e3
        if i >= 2:
            wall.append(t); ms.append(_hip.intersect_robust_ms()[slot])
    return out, wall, ms


for name in sys.argv[1:] or ['C3', 'C4']:
    t0 = time.perf_counter()
    s, truth = synth.make_scene(name)
    s.EO.val[:6], s.IO.val[:] = truth['EO'][:6], truth['IO']
    n = s.OP.val.shape[1]
    cols, ray_pt, r, ray_start, cam, xn, w, px1, P = I.point_rays(s, np.arange(n))
    thr2 = (THR_PX * px1) ** 2
    print('%s: %d points, %d rays (%d .. %d per point) from %d cameras; scene and rays in %.1f s'
          % (name, n, cam.size, r.min(), r.max(), P.shape[0], time.perf_counter() - t0), flush=True)
    _hip.intersect_robust_timing(True)
    a, wall, ms = timed(lambda: _hip.intersect_ransac(ray_start, cam, xn, P, thr2), 'ransac')
    st = a['stats']
    won = st[:, 1] >= 0
    print('  intersect_ransac: wall %s ms   device: k_intersect_ransac %s ms; per point device %.1f ns; %d of %d with a winner, inliers median %d of %d, '
          'hypotheses median %d' % (stat(wall), stat(ms), np.median(ms) * 1e6 / n, won.sum(), n, np.median(st[:, 0]), np.median(r), np.median(st[:, 2])), flush=True)
    b, wall, ms = timed(lambda: _hip.pointadjust(ray_start, cam, xn, P, a['X'], use=a['inlier'], w=w), 'adjust')
    codes = np.bincount(b['code'], minlength=5)
    err = np.linalg.norm(b['X'] - truth['OP'], axis=0)
    print('  pointadjust: wall %s ms   device: k_pointadjust %s ms; per point device %.1f ns; codes 0..4: %s; iterations median %d (%d .. %d), trials median %d; '
          'sigma0 median %.3f; to the true points median %.4f' % (stat(wall), stat(ms), np.median(ms) * 1e6 / n, codes.tolist(), np.median(b['iters']),
                                                               b['iters'].min(), b['iters'].max(), np.median(b['trials']), np.nanmedian(b['sigma0']),
                                                               np.nanmedian(err)), flush=True)
    _hip.intersect_robust_timing(False)
    h = _hip.Handle(s)
    try:
        x = h.serialize()
        wall = []
        for i in range(2 + REPS):
            t0 = time.perf_counter()
            op = h.forwintersect(x, s.OP.val)
            if i >= 2:
                wall.append((time.perf_counter() - t0) * 1e3)
        print('  Handle.forwintersect (k_forwintersect, x up, points down): wall %s ms; to the robust points median %.2e'
              % (stat(wall), np.nanmedian(np.linalg.norm(op - b['X'], axis=0))), flush=True)
    finally:
        h.close()
    import intersect_ransac_ref as ir
    import pointadjust_ref as pr
    t0 = time.perf_counter()
    for p in range(SAMPLE):
        sl = slice(ray_start[p], ray_start[p + 1])
        q = ir.ransac(cam[sl], xn[:, sl], P, thr2, dtype=float)
    t1 = time.perf_counter()
    for p in range(SAMPLE):
        sl = slice(ray_start[p], ray_start[p + 1])
        pr.adjust(cam[sl], xn[:, sl], P, a['X'][:, p], use=a['inlier'][sl], w=w[:, sl])
    t2 = time.perf_counter()
    print('  NumPy restatements on %d points: RANSAC %.2f ms per point, adjustment %.2f ms per point: %.0f s and %.0f s for the scene'
          % (SAMPLE, (t1 - t0) * 1e3 / SAMPLE, (t2 - t1) * 1e3 / SAMPLE, (t1 - t0) / SAMPLE * n, (t2 - t1) / SAMPLE * n), flush=True)
