"""Time of the ray intersection angles on one GPU (dbat_hip_ray_angles: Handle.ray_angles) from the device events of
the call itself -- the point kernels, the unit directions of the images, the matrix-core pair kernel -- with the pairs
per second of the pair kernel and its share of the FP64 matrix peak; at C1 also report._angles on the host (the loop
over the points the report uses by default, and the dense visibility table it is fed from), for scale.
bench/time_angles.py [C1 | C3 | camcal ...] (several scenes in one run)."""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
from dbat_amd import synth, _hip, report

FP64_PEAK_TFLOPS = 78.6    # MI355X FP64 matrix peak (vendor), as bench.py
MFMA_FLOPS = 2048          # v_mfma_f64_16x16x4_f64


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
        for i in range(4):                         # (the first call builds the angle plan and its scratch arrays)
            t0 = time.perf_counter()
            op, cam, op_rays, cam_rays = h.ray_angles(x)
            wall = time.perf_counter() - t0
            t = h.ray_angles_ms()
            pairs = 256.0 * t['mfma']
            rate = pairs / (t['cam_pairs'] * 1e-3) if t['cam_pairs'] > 0 else float('nan')
            frac = t['mfma'] * MFMA_FLOPS / (t['cam_pairs'] * 1e-3) / (FP64_PEAK_TFLOPS * 1e12) if t['cam_pairs'] > 0 else float('nan')
            print('%s images %d points %d nObs %d call %d: points %.3f ms  image directions %.3f ms  image pairs %.3f ms '
                  '(%d workgroups, %.3g pairs, %.3g pairs/s, %.3f of the FP64 matrix peak)  wall %.1f ms  '
                  'op %.4f .. %.4f rad  cam %.4f .. %.4f rad'
                  % (name, len(cam), len(op), s.IP.val.shape[1], i, t['points'], t['cam_dirs'], t['cam_pairs'], t['workgroups'],
                     pairs, rate, frac, wall * 1e3, np.nanmin(op), np.nanmax(op), np.nanmin(cam), np.nanmax(cam)), flush=True)
    finally:
        h.close()
    if name == 'C1':
        t0 = time.perf_counter()
        vis, _ = report._vis(s)
        t1 = time.perf_counter()
        a = report._angles(s, vis)
        t2 = time.perf_counter()
        print('%s host: dense table %.1f ms  report._angles %.1f ms  max |a_host - a_device| = %.2e rad'
              % (name, (t1 - t0) * 1e3, (t2 - t1) * 1e3, np.nanmax(np.abs(a - op))), flush=True)
