"""Time of the image coverage and the marking-residual statistics on one GPU (dbat_hip_coverage, dbat_hip_residual_stats:
Handle.coverage, Handle.residual_stats) from the device events of the calls themselves, four calls each; at C1 also the
host path of the report for the same numbers -- the dense visibility table (report._vis), report._coverage per image
and as a union, and the scatter into the dense residual table with its sums -- for scale, with the agreement of the two.
bench/time_quality.py [C1 | C3 | camcal ...] (several scenes in one run)."""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
from dbat_amd import synth, _hip, report


def scene(name):
    if name == 'camcal':
        from helpers import camcal_struct
        return camcal_struct()
    return synth.make_scene(name)[0]


for name in sys.argv[1:] or ['C1', 'C3']:
    s = scene(name)
    h = _hip.Handle(s)
    try:
        x = h.serialize()
        for i in range(4):                         # (the first call builds the plan of the two calls and its arrays)
            t0 = time.perf_counter()
            cov = h.coverage()
            t1 = time.perf_counter()
            st = h.residual_stats(x)
            t2 = time.perf_counter()
            t = h.quality_ms()
            print('%s images %d points %d nObs %d call %d: coverage %.3f ms (wall %.1f ms, %d hull vertices)  '
                  'residual statistics %.3f ms (wall %.1f ms)'
                  % (name, len(cov['rad_max']), len(st['op_n']), s.IP.val.shape[1], i, t['coverage'], (t1 - t0) * 1e3,
                     sum(len(v) for v in cov['hull']), t['residual_stats'], (t2 - t1) * 1e3), flush=True)
        r, _ = h.residual(x)
    finally:
        h.close()
    if name == 'C1':
        no, nc = s.IP.val.shape[1], s.EO.val.shape[1]
        if not hasattr(s.IO.sensor, 'imSize'):     # the synthetic scenes carry no image size: the box of their points
            s.IO.sensor.imSize = np.tile(np.ceil(np.asarray(s.IP.val, float).max(1))[:, None], (1, nc))
        px = np.asarray(s.IO.sensor.pxSize, float)
        e = np.sqrt(np.sum((r[:2 * no].reshape(2, no, order='F') / (px[:, :1] if px.shape[1] == 1 else px[:, s.IP.cam])) ** 2, 0))
        t0 = time.perf_counter()
        vis, _ = report._vis(s)
        t1 = time.perf_counter()
        c, cr, crr = report._coverage(s, np.arange(nc), False)
        report._coverage(s, np.arange(nc), True)
        t2 = time.perf_counter()
        res = np.zeros(vis.shape)
        res[s.IP.pt, s.IP.cam] = e
        k = int(np.argmax(res.flatten('F')))
        ss_op, ss_cam = (res ** 2).sum(1), (res ** 2).sum(0)
        t3 = time.perf_counter()
        tot = np.prod(np.asarray(s.IO.sensor.imSize, float), 0)
        print('%s host: dense table %.1f ms  report._coverage %.1f ms  residual block %.1f ms  '
              'max |hull area fraction host - device| = %.2e  max rel |sum e^2 per image| = %.2e  per point = %.2e'
              % (name, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, np.max(np.abs(c - cov['hull_area'] / tot)),
                 np.max(np.abs(ss_cam - st['cam_ss']) / ss_cam), np.nanmax(np.abs(ss_op - st['op_ss']) / np.where(ss_op > 0, ss_op, np.nan))),
              flush=True)
