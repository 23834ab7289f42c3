"""The calls of tests/test_adjust_bits_gpu.py and the recorder of its fixture, tests/golden/adjust_bits.npz: what
dbat_hip_poseadjust, dbat_hip_pointadjust and dbat_hip_pairadjust return, bit for bit, at the sizes where a lane stride, a
reduction or a branch of their kernels changes.  The other GPU tests compare the device with restatements to within
tolerances and a call with itself; the fixture is what compares the kernels with themselves across a change of their
code.  Nothing here runs a restatement: the module only collects arguments from the builders the tests of the three calls
already have.

The fixture holds, per call: every per-item output in full (a mismatch then shows how far apart the values are), a
SHA-256 of every per-observation output (NaN mapped to the one canonical NaN first) and a SHA-256 of the inputs, so that
a drift of the builders fails as such and not as a change of a kernel.

Recording -- only when the numerics of a kernel are changed on purpose, from a build of the commit whose bits are to be
pinned, on the device:
    python tests/adjust_bits_cases.py --record tests/golden/adjust_bits.npz [--force]"""
import hashlib
import os
import sys

import numpy as np

ITEM = ('f0', 'f', 'sigma0', 'lam', 'code', 'iters', 'trials', 'n_used', 'Q')
# function of dbat_amd._hip -> (outputs stored in full, outputs stored as digests)
OUTPUTS = {'poseadjust': (('P',) + ITEM, ('used', 'res')),
           'pointadjust': (('X',) + ITEM, ('used', 'res')),
           'pairadjust': (('P2',) + ITEM, ('used', 'res', 'X'))}
NOISES = (0.0, 5e-4)
POSE_SIZES = (3, 4, 63, 64, 65, 129)                      # around the 64 lanes of a camera
PAIR_SIZES = (5, 6, 63, 64, 65, 255, 256, 257, 513)       # around the 256 lanes of a pair


def pose_calls():
    import poseadjust_ref as po
    from test_resect_robust_gpu import OPT, batch_args
    case = po.seeded_case
    calls = {'seeded': batch_args([case(n, noise) for n in POSE_SIZES for noise in NOISES], residuals=True)[1]}
    # test_mask_weights_and_residuals: a mask with holes, one of them NaN, and weights per coordinate
    c = case(129, 5e-4)
    rng = np.random.default_rng(12)
    use = rng.uniform(size=129) > 0.3
    use[:2] = (False, True)
    w = rng.uniform(500.0, 4000.0, (2, 129))
    X = c['X'].copy()
    X[:, int(np.flatnonzero(~use)[3])] = np.nan
    calls['mask'] = dict(pt_start=[0, 129], X=X, xn=c['x'], P=c['P0'][None], use=use, w=w, max_iter=po.MAX_ITER, conv_tol=po.CONV_TOL, residuals=True)
    # test_statuses: two used points, an empty camera and a sound one; the collinear triple; one iteration
    c, c65 = case(64, 5e-4), case(65, 5e-4)
    calls['too_few'] = dict(pt_start=[0, 64, 64, 129], X=np.concatenate([c['X'], c65['X']], 1), xn=np.concatenate([c['x'], c65['x']], 1),
                            P=np.stack([c['P0'], c['P0'], c65['P0']]), use=np.concatenate([np.arange(64) < 2, np.ones(65, bool)]), residuals=True, **OPT)
    X = np.array([[0.0, 5.0, 10.0], [0.0, 5.0, 10.0], [0.0, 0.0, 0.0]])
    C = np.array([4.0, 7.0, 20.0])
    calls['collinear'] = dict(pt_start=[0, 3], X=X, xn=(X - C[:, None])[:2] / (X - C[:, None])[2], P=np.hstack([np.eye(3), -C[:, None]])[None], **OPT)
    calls['max_iter_1'] = batch_args([c], max_iter=1)[1]
    calls['plain'] = dict(pt_start=[0, 65], X=c65['X'], xn=c65['x'], P=c65['P0'][None], w=None, use=None, residuals=False,
                          max_iter=po.MAX_ITER, conv_tol=po.CONV_TOL)
    return calls


def point_calls():
    import pointadjust_ref as pr
    from test_intersect_robust_cpu import CASES, status_cases
    from test_intersect_robust_gpu import batch_args
    case = pr.seeded_case
    calls = {'seeded': batch_args([case(r, noise) for r, noise in CASES], residuals=True)[1]}
    for n in (31, 32, 33):                                  # test_batch_sizes: around the 32 points of a workgroup
        calls['batch_%d' % n] = batch_args([case(*CASES[k % len(CASES)]) for k in range(n)], residuals=True)[1]
    for label, (kw, code) in status_cases().items():        # code 4 of one ray and of none, code 2 at 12 trials, codes 1 and 3
        kw = dict(kw)
        X0 = np.asarray(kw.pop('X0'), float)
        calls['status_' + label] = dict(ray_start=[0, len(kw['cam'])], X=X0[:, None], residuals=True, **kw)
    # test_mask_weights_and_residuals
    c = case(65, 5e-4)
    rng = np.random.default_rng(12)
    use = rng.uniform(size=65) > 0.3
    use[:2] = (False, True)
    w = rng.uniform(500.0, 4000.0, (2, 65))
    x = c['x'].copy()
    x[:, int(np.flatnonzero(~use)[3])] = np.nan
    calls['mask'] = dict(ray_start=[0, 65], cam=c['cam'], xn=x, P=c['P'], X=c['X0'][:, None], use=use, w=w, max_iter=pr.MAX_ITER,
                         conv_tol=pr.CONV_TOL, residuals=True)
    calls['plain'] = dict(ray_start=[0, 65], cam=c['cam'], xn=c['x'], P=c['P'], X=c['X0'][:, None], w=None, use=None, residuals=False,
                          max_iter=pr.MAX_ITER, conv_tol=pr.CONV_TOL)
    return calls


def pair_calls():
    import pairadjust_ref as pr
    from test_pairadjust_cpu import filter_case, five_copies
    from test_pairadjust_gpu import P_of, one_args
    case = pr.seeded_case
    cs = [case(n, noise) for n in PAIR_SIZES for noise in NOISES]
    cat = lambda k: np.concatenate([c[k] for c in cs], 1)
    calls = {'seeded': dict(pt_start=np.cumsum([0] + [c['n'] for c in cs]), x1=cat('x1'), x2=cat('x2'), P2=np.stack([P_of(c['R0'], c['t0']) for c in cs]),
                            X=cat('X0'), w1=pr.WEIGHT, w2=pr.WEIGHT, front_dir=-1, max_iter=pr.MAX_ITER, conv_tol=pr.CONV_TOL, min_angle=pr.MIN_ANGLE,
                            residuals=True)}
    calls['filter'] = one_args(filter_case(), residuals=True)               # min_angle > 0 and front take correspondences out
    calls['filter_off'] = one_args(filter_case(), min_angle=0.0, residuals=True)
    # test_statuses: four used points beside a sound pair; one iteration; five copies of one correspondence (code 3)
    c = case(64, 5e-4)
    two = lambda a: np.concatenate([a, a], 1)
    calls['too_few'] = one_args(c, pt_start=[0, 64, 128], x1=two(c['x1']), x2=two(c['x2']), P2=np.stack([P_of(c['R0'], 3.0 * c['t0']), P_of(c['R0'], c['t0'])]),
                                X=two(c['X0']), use=np.concatenate([np.arange(64) < 4, np.ones(64, bool)]), residuals=True)
    calls['max_iter_1'] = one_args(c, max_iter=1)
    calls['five_copies'] = one_args(five_copies())
    c = case(65, 5e-4)
    rng = np.random.default_rng(12)
    calls['weights'] = one_args(c, w1=rng.uniform(500.0, 4000.0, (2, 65)), w2=rng.uniform(500.0, 4000.0, (2, 65)), residuals=True)
    calls['plain'] = one_args(c, w1=None, w2=None, residuals=False)
    return calls


def all_calls():
    """'<function>/<label>' -> (the function's name in dbat_amd._hip, its keyword arguments)."""
    out = {}
    for fn, calls in (('poseadjust', pose_calls()), ('pointadjust', point_calls()), ('pairadjust', pair_calls())):
        for label, kw in calls.items():
            out['%s/%s' % (fn, label)] = (fn, kw)
    return out


def canonical(a):
    """The array with every NaN the one canonical NaN, contiguous: its bytes are what a digest is taken of."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == 'f':
        a = a.copy()
        a[np.isnan(a)] = np.nan
    return a


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is None:
            h.update(b'None')
            continue
        a = canonical(np.asarray(a))
        h.update(('%s %s ' % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def inputs_digest(kw):
    h = hashlib.sha256()
    for k in sorted(kw):
        h.update(('%s=%s;' % (k, digest(kw[k]))).encode())
    return h.hexdigest()


def entries(name, fn, kw, r):
    """What the fixture holds of the result r of the call `name`: (the per-item outputs as one record per item, a field
    per output; the digests, '<name>/<what>' -> SHA-256, of the inputs and of every per-observation output)."""
    full, hashed = OUTPUTS[fn]
    r = dict(r, X=r['X'].T) if fn == 'pointadjust' else r    # (X of pointadjust is 3-by-n: one row per item here)
    items = np.zeros(len(r['code']), [(k, r[k].dtype, r[k].shape[1:]) for k in full])
    for k in full:
        items[k] = r[k]
    digests = {name + '/inputs': inputs_digest(kw)}
    for k in hashed:
        digests['%s/%s' % (name, k)] = digest(r[k])
    return items, digests


def record(path, force=False):
    if os.path.exists(path) and not force:
        raise SystemExit('%s exists: --force overwrites it' % path)
    from dbat_amd import _hip
    _hip.load()
    fixture, digests = {}, {}
    for name, (fn, kw) in all_calls().items():
        fixture[name], d = entries(name, fn, kw, getattr(_hip, fn)(**kw))
        digests.update(d)
    fixture['digests'] = np.array(['%s %s' % kv for kv in sorted(digests.items())])
    with open(path, 'wb') as f:                              # (np.savez appends .npz to a name without it)
        np.savez_compressed(f, **fixture)
    print('%s: %d calls, %d digests, %d bytes' % (path, len(fixture) - 1, len(digests), os.path.getsize(path)))


def load(path):
    """(call -> records, '<call>/<what>' -> digest) of a fixture."""
    with np.load(path) as z:
        items = {k: z[k] for k in z.files if k != 'digests'}
        return items, dict(line.split(' ') for line in z['digests'])


if __name__ == '__main__':
    HERE = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), 'oracle'), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    if len(sys.argv) < 3 or sys.argv[1] != '--record' or sys.argv[3:] not in ([], ['--force']):
        raise SystemExit(__doc__)
    record(sys.argv[2], force=sys.argv[3:] == ['--force'])
