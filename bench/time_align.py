"""Time of the network transforms on one GPU (dbat_hip_rigidalign, dbat_hip_multixform) at the point and camera counts
of the configurations C3 (1e6 / 1000) and C4 (5e6 / 5000): the device events of each kernel pass, the wall time of each
call with its copies, and the wall time of the float64 NumPy restatement of the reference functions
(tests/test_align_cpu.py) on the same host.  After two warm-up calls every figure is the median of REPS calls, with the
smallest and the largest.  Also the bytes each pass reads and writes over its time, as a share of the HBM peak: a rate, not
an HBM measurement -- the arrays (48 ... 240 MB) have just been uploaded and passes 2 and 3 read them again, so part of
them may come from the 256 MB Infinity Cache.
bench/time_align.py [C1 | C3 | C4 ...] (several sizes in one run; C1, 10^4 points / 100 cameras, measures launches)."""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import numpy as np
from dbat_amd import _hip
from test_align_cpu import ref_rigidalign, ref_multixform, random_rotation, similarity

SIZES = {'C1': (10000, 100), 'C3': (1000000, 1000), 'C4': (5000000, 5000)}
HBM_PEAK = 8.0e12          # bytes/s, MI355X (vendor)
REPS = 10


def stat(v):
    v = np.sort(np.asarray(v, float))
    return '%.3f (%.3f .. %.3f)' % (np.median(v), v[0], v[-1])


def timed(fn, reps=REPS, warm=2):
    """wall ms of every call of fn, and what fn returned last; the calls end in a device-to-host copy"""
    out, t = None, []
    for i in range(warm + reps):
        t0 = time.perf_counter()
        out = fn()
        if i >= warm:
            t.append((time.perf_counter() - t0) * 1e3)
    return t, out


for name in sys.argv[1:] or ['C3', 'C4']:
    npnt, nc = SIZES[name]
    rng = np.random.default_rng(1)
    _hip.align_timing(True)
    off = np.array([1e6, 2e6, 3e2])
    X = np.asfortranarray(off[:, None] + rng.normal(0, 10, (3, npnt)))
    T0 = similarity(random_rotation(rng), 1.3, [5e2, -2e3, 1e3])
    Y = np.asfortranarray(T0[:3, :3] @ X + T0[:3, 3:4] + rng.normal(0, 1e-3, (3, npnt)))
    use = rng.random(npnt) > 1 / 3
    EO = np.asfortranarray(np.vstack([rng.normal(0, 20, (3, nc)), rng.uniform(-1.5, 1.5, (3, nc))]))
    print('%s: %d points, %d cameras' % (name, npnt, nc), flush=True)

    for label, kw in (('all columns, no residuals', dict()), ('mask, residuals', dict(use=use, resid=True))):
        ms = {k: [] for k in ('centroid', 'cross', 'resid')}

        def call():
            r = _hip.rigidalign(X, Y, True, **kw)
            for k in ms:
                ms[k].append(_hip.align_ms()[k])
            return r
        wall, (T, st, resid) = timed(call)
        ms = {k: v[2:] for k, v in ms.items()}
        nbytes = dict(centroid=48.0 * npnt, cross=48.0 * npnt, resid=(48.0 + (24.0 if 'resid' in kw else 0)) * npnt)
        if 'use' in kw:          # a dropped column is not read (its cache lines mostly are): count the mask only
            nbytes = {k: v + npnt for k, v in nbytes.items()}
        print('  rigidalign (%s): wall %s ms   device: ' % (label, stat(wall))
              + '  '.join('%s %s ms [bytes / time: %.2f of the HBM peak]' % (k, stat(v), nbytes[k] / (np.median(v) * 1e-3) / HBM_PEAK)
                          for k, v in ms.items()), flush=True)
        host, ref = timed(lambda: ref_rigidalign(X, Y, True, kw.get('use')), reps=3, warm=1)
        print('  restatement, float64 NumPy (%s): wall %s ms   max |T - T_host| = %.2e, alpha %.12f, rms %.6e (host %.6e)'
              % (label, stat(host), np.abs(T - ref['T']).max(), st['alpha'], st['rms'], ref['rms']), flush=True)

    ms = {k: [] for k in ('points', 'cams')}

    def call():
        r = _hip.multixform(EO, X, T0)
        for k in ms:
            ms[k].append(_hip.align_ms()[k])
        return r
    wall, (EO2, OP2, fail) = timed(call)
    ms = {k: v[2:] for k, v in ms.items()}
    nbytes = dict(points=48.0 * npnt, cams=97.0 * nc)
    print('  multixform: wall %s ms   device: ' % stat(wall)
          + '  '.join('%s %s ms [bytes / time: %.2f of the HBM peak]' % (k, stat(v), nbytes[k] / (np.median(v) * 1e-3) / HBM_PEAK)
                      for k, v in ms.items()), flush=True)
    host, (rEO, rOP, rfail, N) = timed(lambda: ref_multixform(EO, X, T0), reps=3, warm=1)
    print('  restatement, float64 NumPy: wall %s ms (points one matrix product, cameras a Python loop as the reference\'s '
          'MATLAB loop)   max |OP - OP_host| = %.2e   max |centre - centre_host| = %.2e'
          % (stat(host), np.abs(OP2 - rOP).max(), np.abs(EO2[:3] - rEO[:3]).max()), flush=True)
    host, _ = timed(lambda: T0[:3, :3] @ X + T0[:3, 3:4])
    print('  the point product A @ OP + d alone on the host: wall %s ms' % stat(host), flush=True)
