"""Least-squares relative orientation on the device (dbat_hip_pairadjust, csrc/pairadjust.hpp; dbat_amd.initial.refine_pairs,
relorient(refine=True)) against the NumPy restatement of tests/pairadjust_ref.py, which shares no code with dbat_amd/.
The seeded cases are those of tests/test_pairadjust_cpu.py, where the properties their seeds were chosen for are checked
without a device.

Both stop at the same optimum; the path to it is not compared.  Per case d_dev is the device's distance to the
np.longdouble restatement and d_ref the float64 restatement's distance to it (the largest difference in R, t and the used
X and, for the pairs with noise and at least six correspondences, relative in sigma0 and Q): d_dev <= max(10 d_ref,
FLOOR).  The factor is this project's margin for two float64 routes on the same conditioning (FACTOR of
test_relorient_gpu.py).  FLOOR is for the cases whose d_ref sits at rounding: ten times the largest d_ref of the
noise-free seeded cases, 1.486e-13 (n = 63) as the restatement gives it on the CPU, so 1.486e-12.  Every run prints both
distances (pytest -s).

Both the restatement and the device evaluate the objective of the accept test beyond their working precision (pairs of
numbers; tests/pairadjust_ref.py says why): with a plain evaluation the accept test answers at random near the optimum,
the iteration stops where the rounding lets it, and d_ref -- two precisions on one path stopping at one iterate -- says
nothing about how far that is from the optimum (measured on n = 65 with noise: 3.9e-13 between them, 1.05e-9 to the
optimum)."""
import numpy as np
import pytest

import pairadjust_ref as pr
import relorient_ref as rr
from test_pairadjust_cpu import CASES, bundle_in_pair_gauge, filter_case, five_copies, gauge_case, seeded
from test_relorient_cpu import hom, real_pair, scoring_case
from test_relorient_gpu import two_image_struct

pytestmark = pytest.mark.gpu

FACTOR = 10.0
FLOOR = 1.486e-12


@pytest.fixture(scope='module')
def hip():
    from dbat_amd import _hip
    import torch
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    _hip.load()
    return _hip


def P_of(R, t):
    return np.hstack([np.asarray(R, float), np.asarray(t, float)[:, None]])


def as_result(r, k, sl):
    """Pair k of a device call in the form of the restatement's result."""
    return dict(R=r['P2'][k][:, :3], t=r['P2'][k][:, 3], X=r['X'][:, sl], used=r['used'][sl], sigma0=r['sigma0'][k], Q=r['Q'][k],
                code=int(r['code'][k]), f=r['f'][k], f0=r['f0'][k], n=int(r['n_used'][k]), iters=int(r['iters'][k]),
                res=None if r['res'] is None else r['res'][:, :, sl])


def same_bits(a, b):
    for k in a:
        if a[k] is not None and not np.array_equal(a[k], b[k], equal_nan=True):
            return False
    return True


def compare(label, dev, ref64, refld, X0, stat):
    """The checks of one pair: the distances, the invariants of the pose, the mask, the code, the unused points."""
    d_ref, d_dev = pr.distance(ref64, refld, stat), pr.distance(dev, refld, stat)
    print('%s: d_dev %.2e d_ref %.2e (bound %.2e); device %d iterations, restatement %d' % (label, d_dev, d_ref, max(FACTOR * d_ref, FLOOR), dev['iters'], ref64['iters']))
    assert np.array_equal(dev['used'], ref64['used']), label + ': mask'
    assert dev['code'] == ref64['code'] == 0, label + ': code %d' % dev['code']
    assert np.abs(dev['R'].T @ dev['R'] - np.eye(3)).max() < 1e-13 and abs(np.linalg.norm(dev['t']) - 1) < 1e-14, label
    u = dev['used']
    assert np.array_equal(dev['X'][:, ~u], np.asarray(X0, float)[:, ~u], equal_nan=True), label + ': an unused point was touched'
    assert d_dev <= max(FACTOR * d_ref, FLOOR), '%s: device %.2e from the longdouble restatement, float64 restatement %.2e' % (label, d_dev, d_ref)
    return d_dev, d_ref


def seeded_args():
    cs = [seeded(n, noise)[0] for n, noise in CASES]
    ps = np.cumsum([0] + [c['n'] for c in cs])
    cat = lambda k: np.concatenate([c[k] for c in cs], 1)
    return cs, ps, dict(pt_start=ps, x1=cat('x1'), x2=cat('x2'), P2=np.stack([P_of(c['R0'], c['t0']) for c in cs]), X=cat('X0'),
                        w1=pr.WEIGHT, w2=pr.WEIGHT, front_dir=-1, max_iter=pr.MAX_ITER, conv_tol=pr.CONV_TOL, min_angle=pr.MIN_ANGLE)


def one_args(c, **kw):
    return {**dict(pt_start=[0, c['x1'].shape[1]], x1=c['x1'], x2=c['x2'], P2=P_of(c['R0'], c['t0'])[None], X=c['X0'], w1=pr.WEIGHT, w2=pr.WEIGHT,
                   front_dir=-1, max_iter=pr.MAX_ITER, conv_tol=pr.CONV_TOL, min_angle=pr.MIN_ANGLE), **kw}


def test_seeded_cases(hip):
    cs, ps, args = seeded_args()
    a, b = hip.pairadjust(**args), hip.pairadjust(**args)
    assert same_bits(a, b), 'two identical calls differ'
    failed = []
    for k, (n, noise) in enumerate(CASES):
        c, r64, rld = seeded(n, noise)
        sl = slice(ps[k], ps[k + 1])
        one = hip.pairadjust(**one_args(c))
        for key in ('P2', 'f0', 'f', 'sigma0', 'lam', 'code', 'iters', 'trials', 'n_used', 'Q'):
            assert np.array_equal(one[key][0], a[key][k], equal_nan=True), 'n %d noise %g: %s alone and in the batch differ' % (n, noise, key)
        assert np.array_equal(one['X'], a['X'][:, sl]) and np.array_equal(one['used'], a['used'][sl])
        try:
            compare('n %4d noise %.0e' % (n, noise), as_result(a, k, sl), r64, rld, c['X0'], noise > 0 and n >= 6)
        except AssertionError as e:                               # every case is run and printed before the test fails
            failed.append(str(e).splitlines()[0])
    assert not failed, failed


def test_mask_and_outliers(hip):
    c = scoring_case()
    x1, x2 = c['x1'], c['x2']
    ref = rr.ransac(x1, x2, c['samples'], c['thr2'])
    P1, P2, X, fr, sp = rr.camsfrome(ref['e'].reshape(3, 3), hom(x1), hom(x2), 1)
    use = ref['mask'] & fr
    assert 100 < use.sum() < 200
    kw = dict(use=use, w1=pr.WEIGHT, w2=pr.WEIGHT, front=1, max_iter=pr.MAX_ITER, conv_tol=pr.CONV_TOL, min_angle=pr.MIN_ANGLE)
    r64 = pr.adjust(x1, x2, P2[:, :3], P2[:, 3], X, **kw)
    rld = pr.adjust(x1, x2, P2[:, :3], P2[:, 3], X, dtype=np.longdouble, **kw)
    assert r64['code'] == 0 and rld['code'] == 0
    r = hip.pairadjust([0, 200], x1, x2, P2[None], X, use=use, w1=pr.WEIGHT, w2=pr.WEIGHT, front_dir=1, max_iter=pr.MAX_ITER,
                       conv_tol=pr.CONV_TOL, min_angle=pr.MIN_ANGLE, residuals=True)
    dev = as_result(r, 0, slice(0, 200))
    d_dev, d_ref = compare('mask with holes', dev, r64, rld, X, True)
    e_ref, e_dev = np.abs(np.asarray(r64['res'] - rld['res'], float)).max(), np.abs(np.asarray(dev['res'] - rld['res'], float)).max()
    print('residuals: device %.2e restatement %.2e from the longdouble restatement' % (e_dev, e_ref))
    assert e_dev <= max(FACTOR * e_ref, FLOOR * pr.WEIGHT)            # a residual is the weight times a difference of coordinates
    assert np.all(dev['res'][:, :, ~dev['used']] == 0) and not dev['used'][~use].any()
    assert abs(float(np.sum(dev['res'] ** 2)) / dev['f'] - 1) < 1e-12


def test_statuses(hip):
    c = seeded(64, 5e-4)[0]
    r = hip.pairadjust(**one_args(c, max_iter=1))
    assert r['code'][0] == 1 and r['iters'][0] == 1 and r['f'][0] <= r['f0'][0] and np.all(np.isfinite(r['P2'])) and np.all(np.isfinite(r['X']))
    # four used points beside a sound pair
    use = np.concatenate([np.arange(64) < 4, np.ones(64, bool)])
    two = lambda a: np.concatenate([a, a], 1)
    P = np.stack([P_of(c['R0'], 3.0 * c['t0']), P_of(c['R0'], c['t0'])])
    r = hip.pairadjust(**one_args(c, pt_start=[0, 64, 128], x1=two(c['x1']), x2=two(c['x2']), P2=P, X=two(c['X0']), use=use))
    alone = hip.pairadjust(**one_args(c))
    assert r['code'].tolist() == [4, 0] and r['n_used'].tolist() == [4, 64]
    assert np.array_equal(r['P2'][0], P[0]) and np.array_equal(r['X'][:, :64], c['X0']) and np.all(np.isnan(r['Q'][0]))
    for key in ('P2', 'f', 'sigma0', 'Q', 'iters', 'trials'):
        assert np.array_equal(r[key][1], alone[key][0]), key
    assert np.array_equal(r['X'][:, 64:], alone['X'])
    # five copies of one correspondence: converged, and singular
    r = hip.pairadjust(**one_args(five_copies()))
    print('five copies: code %d, %d iterations, f %.2e' % (r['code'][0], r['iters'][0], r['f'][0]))
    assert r['code'][0] == 3 and np.all(np.isfinite(r['P2'])) and np.all(np.isfinite(r['X'])) and np.all(np.isnan(r['Q']))
    assert np.isnan(r['sigma0'][0]) and np.isfinite(r['f'][0])
    # an empty pair and a call without a correspondence
    r = hip.pairadjust([0, 0], np.zeros((2, 0)), np.zeros((2, 0)), P[1:], np.zeros((3, 0)))
    assert r['code'].tolist() == [4] and np.array_equal(r['P2'][0], P[1])


def test_unfiltered_case(hip):
    """The pair that needs the filter (test_pairadjust_cpu.filter_case): without it no code 0 and everything but Q finite,
    with it 61 used and code 0."""
    c = filter_case()
    r = hip.pairadjust(**one_args(c, min_angle=0.0))
    print('filter case, min_angle 0: code %d, %d used, %d iterations, %d trials, f %.4f' % (r['code'][0], r['n_used'][0], r['iters'][0], r['trials'][0], r['f'][0]))
    assert np.all(np.isfinite(r['P2'])) and np.all(np.isfinite(r['X'])) and np.isfinite(r['f'][0]) and np.isfinite(r['sigma0'][0])
    assert r['code'][0] != 0 and r['n_used'][0] == 63 and r['f'][0] <= r['f0'][0]
    r = hip.pairadjust(**one_args(c))
    assert r['code'][0] == 0 and r['n_used'][0] == 61


def test_against_the_engine(hip):
    from dbat_amd import bundle
    c = gauge_case()
    res, ok, iters, s0, E = bundle(c['s'], 50, 'gna', 1e-9)
    assert ok and E.code == 0
    R, t, X = bundle_in_pair_gauge(res)
    r = hip.pairadjust([0, 60], c['x1'], c['x2'], P_of(c['R0'], c['t0'])[None], c['X0'], w1=c['w1'], w2=c['w2'], front_dir=-1, max_iter=50,
                       conv_tol=1e-9)
    d = (abs(r['sigma0'][0] / s0 - 1), np.abs(r['P2'][0][:, :3] - R).max(), np.abs(r['P2'][0][:, 3] - t).max(), np.abs(r['X'] - X).max())
    print('engine: bundle() %d iterations, pairadjust %d (%d trials); differences sigma0 %.1e R %.1e t %.1e X %.1e'
          % (iters, r['iters'][0], r['trials'][0], *d))
    assert r['code'][0] == 0 and r['n_used'][0] == 60
    assert d[0] < 1e-9 and d[1] < 1e-7 and d[2] < 1e-7


def test_pipeline(hip):
    from dbat_amd import bundle, synth, transform_network
    from dbat_amd import initial as I
    s3, truth3 = synth.make_scene('tiny', cams=3, points=300, rays=3, seed=5)
    s, truth = two_image_struct(s3, truth3)
    M0, c0 = I.rotmat3d(truth['EO'][3:6, 0]), truth['EO'][:3, 0]
    base = np.linalg.norm(truth['EO'][:3, 1] - c0)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = M0 / base, -M0 @ c0 / base
    sref = transform_network(s, T)
    sref.bundle.est.EO[:] = True
    sref.bundle.est.EO[:, 0] = False
    sref.bundle.est.EO[int(np.argmax(np.abs(sref.EO.val[:3, 1]))), 1] = False
    s0_ref = bundle(sref, 20, 'gna')[3]
    blank = I.clearop(I.cleareo(two_image_struct(s3, truth3)[0]))
    plain = I.relorient(blank, 0, 1, n_hyp=256, thr_px=3.0, seed=0)
    off = I.relorient(blank, 0, 1, n_hyp=256, thr_px=3.0, seed=0, refine=False)
    assert 'refined' not in off[2] and np.array_equal(plain[0].EO.val, off[0].EO.val, equal_nan=True)
    assert np.array_equal(plain[0].OP.val, off[0].OP.val, equal_nan=True)
    for k in plain[2]:
        assert np.array_equal(plain[2][k], off[2][k], equal_nan=True), k
    s1, ok, info = I.relorient(blank, 0, 1, n_hyp=256, thr_px=3.0, seed=0, refine=True)
    ref = info['refined']
    assert ok and ref['ok'] and ref['code'] == 0 and ref['f'] <= ref['f0']
    assert np.all(s1.EO.val[:6, 0] == 0) and abs(np.linalg.norm(s1.EO.val[:3, 1]) - 1) < 1e-12
    assert np.array_equal(s1.OP.val[:, info['pts'][ref['used']]], ref['X'][:, ref['used']])
    keep = info['in_front'] & ~ref['used']
    assert np.array_equal(s1.OP.val[:, info['pts'][keep]], info['X'][:, keep])
    assert np.allclose(ref['cov'], ref['sigma0'] ** 2 * ref['Q'], rtol=1e-15, atol=0, equal_nan=True) and ref['res'].shape == (2, 2, info['pts'].size)
    its = []
    for start in (s1, plain[0]):
        start.bundle.est.EO[:] = sref.bundle.est.EO
        res, ok2, iters, s0, E = bundle(start, 20, 'gna')
        assert ok2 and E.code == 0 and abs(s0 / s0_ref - 1) < 1e-6
        its.append(iters)
    print('pipeline: refinement code %d in %d iterations, sigma0 %.4f, %d of %d used; bundle() from it %d iterations, from the '
          'unrefined start %d' % (ref['code'], ref['iters'], ref['sigma0'], ref['used'].sum(), info['pts'].size, its[0], its[1]))
    assert its[0] <= its[1]


def test_real_pair_camcal(hip):
    from dbat_amd import initial as I
    c = real_pair('camcal')
    info = I.relorient_pairs(c['s'], [(0, 1)], n_hyp=256, thr_px=3.0, seed=3)[0]
    assert info['ok']
    ref = I.refine_pairs(c['s'], [(0, 1)], [info])[0]
    w1, w2 = I.pair_weights(c['s'], 0, 1)
    use = info['inlier'] & info['in_front']
    kw = dict(use=use, w1=w1, w2=w2, front=-1)
    X0 = np.where(use, info['X'], 0.0)
    r64 = pr.adjust(c['x1'], c['x2'], info['P2'][:, :3], info['P2'][:, 3], X0, **kw)
    rld = pr.adjust(c['x1'], c['x2'], info['P2'][:, :3], info['P2'][:, 3], X0, dtype=np.longdouble, **kw)
    dev = dict(R=ref['P2'][:, :3], t=ref['P2'][:, 3], X=np.where(ref['used'], ref['X'], X0), used=ref['used'], sigma0=ref['sigma0'], Q=ref['Q'],
               code=ref['code'], iters=ref['iters'])
    print('camcal (0, 1): code %d, %d iterations, sigma0 %.4f' % (ref['code'], ref['iters'], ref['sigma0']))
    compare('camcal', dev, r64, rld, X0, True)
    assert ref['ok'] and np.all(np.isfinite(ref['cov']))


def test_real_pair_roma(hip):
    """The pair without a baseline: no code 0, everything but Q finite, the objective not above its start."""
    from dbat_amd import initial as I
    c = real_pair('roma')
    info = I.relorient_pairs(c['s'], [(0, 1)], n_hyp=256, thr_px=3.0, seed=3)[0]
    assert info['ok']                             # 673 of 1189 in front against 515: the candidates do not say
    ref = I.refine_pairs(c['s'], [(0, 1)], [info])[0]
    print('roma (0, 1): code %d, %d iterations, %d trials, f0 %.4g f %.4g, %d used' % (ref['code'], ref['iters'], ref['trials'], ref['f0'], ref['f'], ref['used'].sum()))
    assert ref['code'] != 0 and not ref['ok']
    if ref['code'] != 4:
        assert ref['f'] <= ref['f0'] and np.isfinite(ref['f'])
    assert np.all(np.isfinite(ref['P2'])) and np.all(np.isfinite(ref['X'][:, ref['used']])) and np.all(np.isfinite(ref['res']))
    s1, ok, info1 = I.relorient(c['s'], 0, 1, n_hyp=256, thr_px=3.0, seed=3, refine=True)
    if ok and 'refined' in info1 and not info1['refined']['ok']:
        R = info1['P2'][:, :3]
        assert np.array_equal(s1.EO.val[3:6, 1], I.derotmat3d(R))          # the unrefined values stand
