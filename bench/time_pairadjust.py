"""Time of the least-squares relative orientation on one GPU (dbat_hip_pairadjust): the device events of its one kernel
(k_pairadjust) and the wall time of the call with its copies, on the winners of relorient_pairs for
  one    one pair of 10^4 correspondences
  many   1000 pairs of 1000 correspondences
(the pairs of bench/time_relorient.py without its outliers: noise 5e-4, weights 2000, 64 samples per pair).  After two
warm-up calls every figure is the median of REPS calls, with the smallest and the largest.  Beside the second case the
only other route to the same result: bundle(s2, 20, 'gna') on the two-image struct of a pair, camera 0 fixed and the
largest coordinate of the baseline, from the same start -- wall time per pair over ten pairs, a warm-up pair before them.
bench/time_pairadjust.py [one | many ...]"""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
from dbat_amd import _hip, bundle
from dbat_amd import initial as I
from dbat_amd.dbatstruct import make_struct
from dbat_amd.initial import draw_samples
import relorient_ref as rr

SIZES = {'one': (1, 10000), 'many': (1000, 1000)}
REPS, N_HYP, WEIGHT, F_MM, PX = 10, 64, 2000.0, 10.0, 0.005          # WEIGHT = F_MM / PX: image points of one pixel
BUNDLE_PAIRS = 10


def stat(v):
    v = np.sort(np.asarray(v, float))
    return '%.3f (%.3f .. %.3f)' % (np.median(v), v[0], v[-1])


def pair_struct(x1, x2, P2, X):
    """The pair as a two-image struct in the frame of camera 0: a camera of 10 mm without distortion, pixels of 5 um,
    the image points that normalise to x1, x2, and the start values P2, X; the datum of test_relorient_gpu.test_pipeline."""
    n = x1.shape[1]
    IO = np.zeros((10, 2))
    IO[0] = F_MM
    EO = np.zeros((6, 2))
    R, t = P2[:, :3], P2[:, 3]
    EO[:3, 1], EO[3:6, 1] = -R.T @ t, I.derotmat3d(R)
    xy = np.concatenate([x1, x2], 1) * -F_MM                       # normalised = (xy - pp) / -f
    ip = np.stack([xy[0] / PX, -xy[1] / PX])
    s = make_struct(IO, EO, X, np.asfortranarray(ip), np.repeat([0, 1], n), np.tile(np.arange(n), 2), PX, ip_std=1.0, distModel=3)
    s.bundle.est.EO[:, 0] = False
    s.bundle.est.EO[int(np.argmax(np.abs(EO[:3, 1]))), 1] = False
    return s


for name in sys.argv[1:] or ['one', 'many']:
    n_pairs, n = SIZES[name]
    rng = np.random.default_rng(1)
    x1, x2, smp = [], [], []
    for p in range(n_pairs):
        S = rr.synthetic_pair(rng, n, front=-1, noise=5e-4)
        x1.append(S['x1']); x2.append(S['x2']); smp.append(draw_samples(n, N_HYP, rng))
    ps, hs = np.arange(n_pairs + 1) * n, np.arange(n_pairs + 1) * N_HYP
    X1, X2 = np.asfortranarray(np.concatenate(x1, 1)), np.asfortranarray(np.concatenate(x2, 1))
    start = _hip.relorient_pairs(ps, X1, X2, hs, np.concatenate(smp, 0), np.full(n_pairs, 4e-6), -1)
    use = start['inlier'] & start['in_front']
    X0 = np.where(use, start['X'], 0.0)
    print('%s: %d pair(s) of %d correspondences, %d of %d used' % (name, n_pairs, n, use.sum(), use.size), flush=True)
    _hip.pairadjust_timing(True)
    ms, wall, out = [], [], None
    for i in range(2 + REPS):
        t0 = time.perf_counter()
        out = _hip.pairadjust(ps, X1, X2, start['P2'], X0, use=use, w1=WEIGHT, w2=WEIGHT, front_dir=-1)
        t = (time.perf_counter() - t0) * 1e3
        if i >= 2:
            wall.append(t); ms.append(_hip.pairadjust_ms())
    codes = np.bincount(out['code'], minlength=5)
    print('  wall %s ms   device: k_pairadjust %s ms' % (stat(wall), stat(ms)), flush=True)
    print('  per pair: wall %.4f ms, device %.4f ms; codes 0..4: %s; iterations median %d (%d .. %d), trials median %d; sigma0 median %.4f'
          % (np.median(wall) / n_pairs, np.median(ms) / n_pairs, codes.tolist(), np.median(out['iters']), out['iters'].min(), out['iters'].max(),
             np.median(out['trials']), np.nanmedian(out['sigma0'])), flush=True)
    if name == 'many':
        tb, itb, s0b = [], [], []
        for p in range(BUNDLE_PAIRS + 1):
            sl = slice(ps[p], ps[p + 1])
            u = use[sl]
            s2 = pair_struct(x1[p][:, u], x2[p][:, u], start['P2'][p], start['X'][:, sl][:, u])
            t0 = time.perf_counter()
            res, ok, iters, s0, E = bundle(s2, 20, 'gna')
            t = (time.perf_counter() - t0) * 1e3
            if p >= 1:
                tb.append(t); itb.append(iters); s0b.append(s0 / out['sigma0'][p] - 1)
        print('  bundle(s2, 20, \'gna\') on pairs 1 .. %d: wall per pair %s ms, iterations %s, sigma0 against pairadjust within %.1e'
              % (BUNDLE_PAIRS, stat(tb), itb, np.abs(s0b).max()), flush=True)
        print('  ratio per pair, bundle() wall to pairadjust wall: %.0f' % (np.median(tb) / (np.median(wall) / n_pairs)), flush=True)
