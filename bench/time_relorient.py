"""Time of the relative orientation on one GPU (dbat_hip_relorient): the device events of its three kernel stages -- the
five-point solver (k_essmat5), scoring with the choice of the winner (k_ro_score, k_ro_winner) and the two decomposition
passes (k_ro_cams) -- and the wall time of the call with its copies, on
  one    one pair of 10^4 correspondences with 4096 samples
  many   1000 pairs of 1000 correspondences with 512 samples each
After two warm-up calls every figure is the median of REPS calls, with the smallest and the largest.  Beside the first
case the wall time of the float64 NumPy restatement (tests/relorient_ref.py: one Python loop over the samples) on the
same input, measured on a share of the samples and scaled.
bench/time_relorient.py [one | many ...]"""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
from dbat_amd import _hip
from dbat_amd.initial import draw_samples
import relorient_ref as rr

SIZES = {'one': (1, 10000, 4096), 'many': (1000, 1000, 512)}
REPS = 10
REF_SAMPLES = 64          # samples the restatement is timed on


def stat(v):
    v = np.sort(np.asarray(v, float))
    return '%.3f (%.3f .. %.3f)' % (np.median(v), v[0], v[-1])


for name in sys.argv[1:] or ['one', 'many']:
    n_pairs, n, n_hyp = SIZES[name]
    rng = np.random.default_rng(1)
    x1, x2, smp = [], [], []
    for p in range(n_pairs):
        S = rr.synthetic_pair(rng, n, noise=5e-4)
        bad = rng.random(n) < 0.3
        S['x2'][:, bad] = rng.uniform(-0.5, 0.5, (2, int(bad.sum())))
        x1.append(S['x1']); x2.append(S['x2']); smp.append(draw_samples(n, n_hyp, rng))
    ps, hs = np.arange(n_pairs + 1) * n, np.arange(n_pairs + 1) * n_hyp
    X1, X2, SM = np.asfortranarray(np.concatenate(x1, 1)), np.asfortranarray(np.concatenate(x2, 1)), np.concatenate(smp, 0)
    thr2 = np.full(n_pairs, 4e-6)
    print('%s: %d pair(s) of %d correspondences, %d samples each' % (name, n_pairs, n, n_hyp), flush=True)
    _hip.relorient_timing(True)
    ms, wall, out = {k: [] for k in ('solve', 'score', 'cams')}, [], None
    for i in range(2 + REPS):
        t0 = time.perf_counter()
        out = _hip.relorient_pairs(ps, X1, X2, hs, SM, thr2, 1)
        t = (time.perf_counter() - t0) * 1e3
        if i >= 2:
            wall.append(t)
            for k, v in _hip.relorient_ms().items():
                ms[k].append(v)
    models = int(out['stats'][:, 3].sum())
    print('  wall %s ms   device: ' % stat(wall) + '  '.join('%s %s ms' % (k, stat(v)) for k, v in ms.items()), flush=True)
    print('  %d samples, %d models (%.2f per sample), %.3e model x correspondence tests; inliers of pair 0: %d of %d'
          % (hs[-1], models, models / hs[-1], float(models) * n, out['stats'][0, 0], n), flush=True)
    if name == 'one':
        t0 = time.perf_counter()
        ref = rr.ransac(x1[0], x2[0], smp[0][:REF_SAMPLES], 4e-6)
        t = time.perf_counter() - t0
        print('  restatement, float64 NumPy: %.1f ms for %d samples, %.0f ms scaled to %d (solver and scoring; inliers %d)'
              % (t * 1e3, REF_SAMPLES, t * 1e3 * n_hyp / REF_SAMPLES, n_hyp, ref['count']), flush=True)
