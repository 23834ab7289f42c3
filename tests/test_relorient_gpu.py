"""Relative orientation on the device (dbat_hip_essmat5, dbat_hip_relorient, csrc/relorient.hpp; dbat_amd.initial.essmat5,
camsfrome, relorient, relorient_pairs) against the NumPy restatement of photogrammetry/essmat5.m and camsfrome.m of
tests/relorient_ref.py, which shares no code with dbat_amd/.  The seeded cases are those of tests/test_relorient_cpu.py,
where the properties their seeds were chosen for are checked without a device.

Accuracy is measured against the truth of the synthetic pair, not against the code under test: the device may be at most
ten times as far from the true E as the restatement is on the same set (two root-finding routes on the same
conditioning), with a floor of 1e-10.  Figures measured on the restatement, float64, the 64 minimal sets of
MINIMAL_SEED: worst distance to the true E 1.95e-10; worst residuals of a solution real to 1e-8: |q2' E q1| 4.5e-16,
|det E| 1.75e-12, |2 E E' E - tr(E E') E| 1.49e-11 (printed again by every run, pytest -s; the bounds are ten times the
figures of the run itself, FACTOR below)."""
import numpy as np
import pytest

import relorient_ref as rr
from test_relorient_cpu import (borderline, hom, minimal_reference, minimal_sets, real_pair, report_relative_rotation,
                                rotation_angle, scoring_case, REAL_HYP, REAL_PX, REAL_SEED)

pytestmark = pytest.mark.gpu

MATCH = 1e-6          # two unit solutions are the same one: ten times the restatement's worst distance to the truth (1.2e-7)
FLOOR = 1e-10
FACTOR = 10.0


@pytest.fixture(scope='module')
def hip():
    from dbat_amd import _hip
    import torch
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    _hip.load()
    return _hip


def device_sets(hip, sets):
    start = np.cumsum([0] + [S['x1'].shape[1] for S in sets])
    Q1 = np.concatenate([hom(S['x1']) for S in sets], 1)
    Q2 = np.concatenate([hom(S['x2']) for S in sets], 1)
    E, ns = hip.essmat5_sets(start, Q1, Q2)
    E2, ns2 = hip.essmat5_sets(start, Q1, Q2)
    assert np.array_equal(E, E2) and np.array_equal(ns, ns2), 'two calls differ'
    return E, ns


def check_sets(sets, ref, E, ns, label):
    """The checks of GPU tests 1 and 2 on the device's answer (E (n, 10, 9), ns (n)) for `sets`."""
    ref_res = np.max(np.vstack([r['res'] for r in ref if r['res'].size]), 0)
    print('%s: restatement worst distance %.2e, worst residuals epipolar %.2e det %.2e trace %.2e'
          % (label, max(r['dist'] for r in ref), *ref_res))
    worst_ratio, worst_res, hist = 0.0, np.zeros(3), {}
    for i, (S, r) in enumerate(zip(sets, ref)):
        k = int(ns[i])
        assert 0 <= k <= 10 and np.all(E[i, k:] == 0) and np.all(np.isfinite(E[i]))
        Ed = E[i, :k].T
        hist[k] = hist.get(k, 0) + 1
        assert np.abs(np.linalg.norm(Ed, axis=0) - 1).max(initial=0) < 1e-14, 'not unit norm'
        for j in range(r['strict'].shape[1]):                     # sandwich, from below
            assert rr.dist_to(r['strict'][:, j], Ed) < MATCH, 'set %d: a real solution of the restatement is missing' % i
        for j in range(k):                                        # and from above
            assert rr.dist_to(Ed[:, j], r['Es']) < MATCH, 'set %d: a device solution the restatement does not have' % i
        d = rr.dist_to(S['e'], Ed)
        worst_ratio = max(worst_ratio, d / max(FACTOR * r['dist'], FLOOR))
        assert d <= max(FACTOR * r['dist'], FLOOR), 'set %d: device %.2e from the true E, restatement %.2e' % (i, d, r['dist'])
        Q1, Q2 = hom(S['x1']), hom(S['x2'])
        for j in range(k):
            worst_res = np.maximum(worst_res, rr.residuals(Ed[:, j], Q1, Q2))
    print('%s: device solutions per set %s, distance / bound at most %.3f, worst residuals epipolar %.2e det %.2e trace %.2e'
          % (label, sorted(hist.items()), worst_ratio, *worst_res))
    assert np.all(worst_res <= FACTOR * ref_res), (worst_res, ref_res)
    return hist


def test_minimal_samples(hip):
    sets, ref = minimal_sets(), minimal_reference()
    E, ns = device_sets(hip, sets)
    hist = check_sets(sets, ref, E, ns, 'minimal')
    assert 10 in hist and 2 in hist


@pytest.mark.parametrize('n', [6, 8, 50])
def test_more_than_five(hip, n):
    sets, ref = minimal_sets(n, 16), minimal_reference(n, 16)
    E, ns = device_sets(hip, sets)
    check_sets(sets, ref, E, ns, 'n = %d' % n)
    assert np.all(ns >= 1)


def test_degenerate_sets(hip):
    rng = np.random.default_rng(2)
    S = rr.synthetic_pair(rng, 5)
    rep1, rep2 = S['x1'].copy(), S['x2'].copy()
    rep1[:, 4], rep2[:, 4] = rep1[:, 0], rep2[:, 0]               # a repeated correspondence: rank four
    X = np.array([0.0, 0.0, 6.0])[:, None] + np.array([1.0, 0.5, 0.2])[:, None] * np.linspace(-2, 2, 5)
    Y = S['R'] @ X + S['t'][:, None]                              # five collinear points
    zero = np.zeros((2, 5))                                       # and all at the principal point
    sets = [dict(x1=rep1, x2=rep2), dict(x1=X[:2] / X[2], x2=Y[:2] / Y[2]), dict(x1=zero, x2=zero), S]
    E, ns = device_sets(hip, sets)
    print('degenerate sets: n_sol', ns.tolist())
    assert np.all(np.isfinite(E)) and np.all((ns >= 0) & (ns <= 10))
    assert ns[0] == 0 and ns[2] == 0, 'a rank-deficient set has no solution'
    assert ns[3] >= 1                                             # the sound set beside them is not disturbed
    for i in range(4):
        assert np.all(E[i, ns[i]:] == 0)
        assert np.abs(np.linalg.norm(E[i, :ns[i]], axis=1) - 1).max(initial=0) < 1e-14


def run_pair(hip, x1, x2, samples, thr2, front=1):
    n = x1.shape[1]
    return hip.relorient_pairs([0, n], x1, x2, [0, len(samples)], samples, [thr2], front)


def test_scoring(hip):
    c = scoring_case()
    x1, x2, smp, thr2 = c['x1'], c['x2'], c['samples'], c['thr2']
    ref = rr.ransac(x1, x2, smp, thr2)
    b = borderline(ref['e'], x1, x2, thr2)
    assert b <= 2
    r = run_pair(hip, x1, x2, smp, thr2)
    st = r['stats'][0]
    mask = rr.sampson2(r['E'][0], x1, x2) < thr2                  # from the RETURNED E
    print('scoring: device count %d (sample %d, solution %d, %d models), restatement %d (sample %d, %d models), b = %d'
          % (st[0], st[1], st[2], st[3], ref['count'], ref['sample'], ref['models'], b))
    assert np.array_equal(r['inlier'], mask) and st[0] == mask.sum()
    assert st[0] >= ref['count'] - b
    assert abs(np.linalg.norm(r['E'][0]) - 1) < 1e-14
    # the tie rule: the winning sample once more, at a later index -- the reported index does not move
    r2 = run_pair(hip, x1, x2, np.vstack([smp, smp[st[1]:st[1] + 1]]), thr2)
    assert np.array_equal(r2['stats'][0][:3], st[:3]) and np.array_equal(r2['E'], r['E'])
    assert r2['stats'][0][3] > st[3]
    # and at an earlier one it does
    r3 = run_pair(hip, x1, x2, np.vstack([smp[st[1]:st[1] + 1], smp]), thr2)
    assert r3['stats'][0][1] == 0 and r3['stats'][0][0] == st[0] and np.array_equal(r3['E'], r['E'])


def test_ranges(hip):
    sizes, hyps = (5, 6, 63, 64, 65, 200, 1000), (1, 3, 64, 65, 256, 256, 256)
    rng = np.random.default_rng(17)
    from dbat_amd.initial import draw_samples
    pairs = []
    for n, h in zip(sizes, hyps):
        S = rr.synthetic_pair(rng, n, noise=5e-4)
        pairs.append((S['x1'], S['x2'], draw_samples(n, h, rng)))
    ps, hs = np.cumsum((0,) + sizes), np.cumsum((0,) + hyps)
    args = (ps, np.concatenate([p[0] for p in pairs], 1), np.concatenate([p[1] for p in pairs], 1), hs,
            np.concatenate([p[2] for p in pairs], 0), [4e-6] * len(sizes), 1)
    a, b = hip.relorient_pairs(*args), hip.relorient_pairs(*args)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), 'two identical calls differ in ' + k
    for i, (x1, x2, smp) in enumerate(pairs):
        one = run_pair(hip, x1, x2, smp, 4e-6)
        sl = slice(ps[i], ps[i + 1])
        assert np.array_equal(one['E'][0], a['E'][i], equal_nan=True) and np.array_equal(one['P2'][0], a['P2'][i], equal_nan=True)
        assert np.array_equal(one['stats'][0], a['stats'][i])
        assert np.array_equal(one['inlier'], a['inlier'][sl]) and np.array_equal(one['in_front'], a['in_front'][sl])
        assert np.array_equal(one['X'], a['X'][:, sl], equal_nan=True)
        assert a['stats'][i][0] >= 5 and a['stats'][i][1] >= 0, 'pair %d found no model' % i


@pytest.mark.parametrize('front', [1, -1])
def test_decomposition(hip, front):
    n = 50
    rng = np.random.default_rng(23)
    S = rr.synthetic_pair(rng, n, front=front)
    from dbat_amd.initial import draw_samples
    smp = draw_samples(n, 16, rng)
    ref = rr.ransac(S['x1'], S['x2'], smp, 1e-12)
    P1, P2r, Xr, frr, spr = rr.camsfrome(ref['e'].reshape(3, 3), hom(S['x1']), hom(S['x2']), front)
    truth = np.hstack([S['R'], S['t'][:, None]])
    eP, eX = np.abs(P2r - truth).max(), np.abs(Xr - S['X']).max()
    r = run_pair(hip, S['x1'], S['x2'], smp, 1e-12, front)
    dP, dX = np.abs(r['P2'][0] - truth).max(), np.abs(r['X'] - S['X']).max()
    print('decomposition, front %+d: |P2 - [R t]| device %.2e restatement %.2e; |X - truth| device %.2e restatement %.2e'
          % (front, dP, eP, dX, eX))
    assert dP <= FACTOR * eP and dX <= FACTOR * eX
    assert r['in_front'].all() and r['inlier'].all()
    sp = r['stats'][0][4:8]
    assert sp[0] == n > sp[1] and np.all(np.diff(sp) <= 0)
    assert abs(np.linalg.norm(r['P2'][0][:, 3]) - 1) < 1e-14
    # the public functions: the layout of essmat5, the convention of camsfrome
    from dbat_amd import initial as I
    Es = I.essmat5(hom(S['x1']), hom(S['x2']))
    e = Es[:, int(np.argmin([rr.dist_to(S['e'], Es[:, i:i + 1]) for i in range(Es.shape[1])]))]
    assert rr.dist_to(S['e'], e[:, None]) < 1e-9
    assert np.abs(sum(e[a + 3 * b] * hom(S['x1'])[a] * hom(S['x2'])[b] for a in range(3) for b in range(3))).max() < 1e-12
    P1d, P2d, Xd, frd, spd = I.camsfrome(e.reshape(3, 3), hom(S['x1']), hom(S['x2']), front)
    assert np.array_equal(P1d, np.eye(3, 4)) and frd.all() and spd[0] == n > spd[1] and Xd.shape == (4, n)
    assert np.abs(P2d - truth).max() < 1e-8 and np.abs(Xd[:3] - S['X']).max() < 1e-6
    # the transposed matrix is another essential matrix: its best candidate is not the true pose
    P2t = I.camsfrome(e.reshape(3, 3).T, hom(S['x1']), hom(S['x2']), front)[1]
    assert np.abs(P2t - truth).max() > 1e-3


def two_image_struct(s, truth, cams=(0, 1), same_centre=False):
    """The observations of two images of a synth scene as a struct of its own (the points seen in both), with the true
    values of the pair as truth; same_centre: the second camera moved to the centre of the first (a pure rotation) and
    its image points projected again, noise-free."""
    from dbat_amd import synth
    from dbat_amd.dbatstruct import make_struct
    sel = np.isin(s.IP.cam, cams)
    cam = np.searchsorted(np.array(cams), s.IP.cam[sel])
    pts, cnt = np.unique(s.IP.pt[sel], return_counts=True)
    both = pts[cnt == 2]
    keep = np.isin(s.IP.pt[sel], both)
    cam, pt = cam[keep], np.searchsorted(both, s.IP.pt[sel][keep])
    ip = s.IP.val[:, sel][:, keep].copy()
    IO, EO, OP = truth['IO'][:, cams].copy(), truth['EO'][:, cams].copy(), truth['OP'][:, both].copy()
    px = float(np.ravel(s.IO.sensor.pxSize)[0])
    if same_centre:
        EO[:3, 1] = EO[:3, 0]
        ip = synth.project(IO, EO, OP, cam, pt, px)[0]
    s2 = make_struct(IO, EO, OP, np.asfortranarray(ip), cam, pt, px, ip_std=1.0, distModel=3)
    return s2, dict(IO=IO, EO=EO, OP=OP)


def test_pipeline(hip):
    from dbat_amd import bundle, synth, transform_network
    from dbat_amd import initial as I
    s3, truth3 = synth.make_scene('tiny', cams=3, points=300, rays=3, seed=5)
    s, truth = two_image_struct(s3, truth3)
    assert s.OP.val.shape[1] == 300
    # the reference run: the true values moved into the frame of the pair -- camera 0 at the origin with zero angles, a
    # baseline of length one -- and the same datum
    M0, c0 = I.rotmat3d(truth['EO'][3:6, 0]), truth['EO'][:3, 0]
    base = np.linalg.norm(truth['EO'][:3, 1] - c0)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = M0 / base, -M0 @ c0 / base
    sref = transform_network(s, T)
    assert np.abs(sref.EO.val[:6, 0]).max() < 1e-12 and abs(np.linalg.norm(sref.EO.val[:3, 1]) - 1) < 1e-12
    sref.bundle.est.EO[:] = True                                   # the datum: camera 0 fixed, and of camera 1 the
    sref.bundle.est.EO[:, 0] = False                               # coordinate of the largest offset (the scale)
    sref.bundle.est.EO[int(np.argmax(np.abs(sref.EO.val[:3, 1]))), 1] = False
    res_ref, ok_ref, it_ref, s0_ref, E_ref = bundle(sref, 20, 'gna')
    assert ok_ref
    # the run from nothing: EO and OP cleared, relative orientation, the same datum
    blank = I.clearop(I.cleareo(two_image_struct(s3, truth3)[0]))
    assert np.isnan(blank.EO.val[:6]).all() and np.isnan(blank.OP.val).all()
    s1, ok, info = I.relorient(blank, 0, 1, n_hyp=256, thr_px=3.0, seed=0)
    assert ok and info['sp'][0] > info['sp'][1] and info['count'] >= 0.9 * 300
    assert np.all(s1.EO.val[:6, 0] == 0) and abs(np.linalg.norm(s1.EO.val[:3, 1]) - 1) < 1e-12
    assert np.isfinite(s1.OP.val[:, info['pts'][info['in_front']]]).all()
    s1.bundle.est.EO[:] = sref.bundle.est.EO                       # camera 0 and the same coordinate of camera 1 fixed
    res, ok2, iters, s0, E = bundle(s1, 20, 'gna')
    print('pipeline: %d inliers of 300, sp %s; bundle code %d in %d iterations, sigma0 %.9f; from the truth %d iterations, sigma0 %.9f'
          % (info['count'], info['sp'].tolist(), E.code, iters, s0, it_ref, s0_ref))
    assert ok2 and E.code == 0
    assert abs(s0 / s0_ref - 1) < 1e-6
    assert abs(iters - it_ref) <= 2


def test_pure_rotation(hip):
    from dbat_amd import synth
    from dbat_amd import initial as I
    s3, truth3 = synth.make_scene('tiny', cams=3, points=300, rays=3, seed=5, noise_px=0.0)
    s, truth = two_image_struct(s3, truth3, same_centre=True)
    s1, ok, info = I.relorient(s, 0, 1, n_hyp=64, thr_px=3.0, seed=0)
    print('pure rotation: ok %s, %d models, count %d, sp %s' % (ok, info['models'], info['count'], info['sp'].tolist()))
    assert not ok and s1 is s


@pytest.mark.parametrize('name', ['roma', 'camcal'])
def test_real_pairs(hip, name):
    from dbat_amd import initial as I
    c = real_pair(name)
    ref = c['ref']
    b = borderline(ref['e'], c['x1'], c['x2'], c['thr2'])
    s1, ok, info = I.relorient(c['s'], 0, 1, n_hyp=REAL_HYP, thr_px=REAL_PX, seed=REAL_SEED)
    assert np.array_equal(info['samples'], c['samples']) and np.array_equal(info['pts'], c['pts'])
    Rrep = report_relative_rotation(name)
    P2r = rr.camsfrome(ref['e'].reshape(3, 3), hom(c['x1']), hom(c['x2']), -1)[1]
    dev_d, ref_d = rotation_angle(info['P2'][:, :3], Rrep), rotation_angle(P2r[:, :3], Rrep)
    print('%s (0, 1): device %d inliers of %d (restatement %d, b = %d), sp %s; rotation against the report: device %.3e rad, '
          'restatement %.3e rad' % (name, info['count'], c['pts'].size, ref['count'], b, info['sp'].tolist(), dev_d, ref_d))
    assert info['count'] >= ref['count'] - b
    assert ok and info['sp'][0] > info['sp'][1]
    assert dev_d <= 2 * ref_d
    assert np.array_equal(info['inlier'], rr.sampson2(info['E'].reshape(-1), c['x1'], c['x2']) < c['thr2'])
