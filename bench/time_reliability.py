"""Time of bundle_reliability's device part (Handle.redundancy: set-up, inverse, hat blocks) next to the posterior
covariance of the object points (Handle.posterior_cov, what bundle_cov(s, E, 'COP') calls) on the same handle, on one
GPU.  bench/time_reliability.py [C3 | C1 | camcal ...] (several scenes in one run)."""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
from dbat_amd import synth, _hip
from dbat_amd.driver import reliability_stats


def scene(name):
    if name == 'camcal':
        from helpers import camcal_struct
        return camcal_struct()
    return synth.make_scene(name)[0]


for name in sys.argv[1:] or ['C3']:
    s = scene(name)
    h = _hip.Handle(s)
    try:
        x = h.serialize()
        maps = h.index_maps()
        rw = np.zeros(h.m)
        for i in range(3):
            t0 = time.perf_counter()
            h.posterior_cov(x, 1.0)
            t1 = time.perf_counter()
            qvv, rp = h.redundancy(x)
            t2 = time.perf_counter()
            reliability_stats(s, rw, qvv, rp, maps)
            t3 = time.perf_counter()
            r = np.concatenate([qvv[0], qvv[2], rp])
            print('%s nObs %d m %d n %d: posterior_cov %.3f s  redundancy %.3f s (x %.2f)  statistics %.3f s  '
                  'sum r - (m - n) = %.2e' % (name, s.IP.val.shape[1], h.m, h.n, t1 - t0, t2 - t1, (t2 - t1) / (t1 - t0),
                                              t3 - t2, r.sum() - (h.m - h.n)), flush=True)
    finally:
        h.close()
