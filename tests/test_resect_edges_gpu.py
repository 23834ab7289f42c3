"""k_resect (csrc/resect.hpp) through the raw ABI, _hip.resect_poses, at its edges: single known triangles against the
longdouble reference tests/resect_ref.py, the scoring loop around its 64-lane stride, the two selection rules, several
triangles per camera, independence of the cameras of one call, cameras without a pose, and project coordinates of
1e6 m.  The seeded cases and their conditioning: tests/initial_cases.py, tests/test_initial_ref_cpu.py.

The 8x rule: the device and the float64 restatement (oracle/initial_oracle.py pm_resect_3pt) evaluate the same formula
in float64 with another root finder and another order of summation, so the device's error against longdouble may be
8 times the restatement's on the same case plus 64 eps * max|P|; a wrong coefficient or frame is off by orders of
magnitude.

The figures in the docstrings were measured on an MI355X (gfx950); every test prints its own (pytest -s)."""
import numpy as np
import pytest

import initial_cases as IC
import resect_ref as RR

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps


@pytest.fixture(scope='module')
def hip():
    from dbat_amd import _hip
    import torch
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    _hip.load()
    return _hip


def _cam(case, tris=None):
    """A camera of a call: (X, x, triangles) of a seeded case; the case's own triangle by default."""
    tris = [case['tri']] if tris is None else tris
    return case['X'], case['x'], np.asarray(tris, np.int32).reshape(-1, 3)


def _run(hip, cams):
    """One call over the cameras [(X 3 x n, x 2 x n, triangles k x 3)]: (P (n, 3, 4), rms (n))."""
    pt_start, tri_start = [0], [0]
    for X, x, T in cams:
        pt_start.append(pt_start[-1] + X.shape[1])
        tri_start.append(tri_start[-1] + len(T))
    X = np.concatenate([c[0] for c in cams], 1)
    x = np.concatenate([c[1] for c in cams], 1)
    T = np.concatenate([c[2] for c in cams], 0) if tri_start[-1] else np.zeros((0, 3), np.int32)
    return hip.resect_poses(pt_start, X, x, tri_start, T)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, float).view(np.int64), np.asarray(b, float).view(np.int64))


def _largest_triangle(x, among):
    from itertools import combinations
    T = np.array(list(combinations(list(among), 3)))
    ax, ay = x[0][T], x[1][T]
    A = np.abs(ax[:, 0] * (ay[:, 1] - ay[:, 2]) + ax[:, 1] * (ay[:, 2] - ay[:, 0]) + ax[:, 2] * (ay[:, 0] - ay[:, 1]))
    return np.sort(T[int(np.argmax(A))])


def _noisy_case(seed, npt=20, noise=1e-3, clean=()):
    """A seeded case with noise on EVERY image point but those of `clean`."""
    c = dict(RR.seeded_case(seed, npt=npt))
    rng = np.random.default_rng(5150 + seed)
    n = noise * rng.standard_normal(c['x'].shape)
    n[:, list(clean)] = 0.0
    c['x'] = c['x'] + n
    return c


def test_one_triangle_exact_scene(hip):
    """Twenty seeded cases, one image and one triangle each, 20 check points: the returned P against the longdouble
    reference's winner under the 8x rule.
    Measured: device error / restatement error between 0.05 and 2.71 over the twenty cases (the largest at seed 5:
    8.8e-12 against 3.2e-12); at most 0.33 of the bound is used."""
    used, _ = IC.resect_cases()
    assert len(used) == 20
    worst_ratio, worst_use = 0.0, 0.0
    for c in used:
        P, rms = _run(hip, [_cam(c)])
        size = float(np.max(np.abs(c['Pref'])))
        e_dev = RR.pose_err(P[0], c['Pref'])
        e_orc = c['oracle_err'][0]
        bound = 8 * e_orc + 64 * EPS * size
        print('seed %2d: device %.3e restatement %.3e ratio %.2f bound %.3e  rms %.2e (ref %.2e)'
              % (c['seed'], e_dev, e_orc, e_dev / e_orc, bound, rms[0], float(c['rms_ref'])))
        worst_ratio, worst_use = max(worst_ratio, e_dev / e_orc), max(worst_use, e_dev / bound)
        assert e_dev <= bound, (c['seed'], e_dev, e_orc)
    print('resection, exact scenes: largest ratio %.2f, largest share of the bound %.2f' % (worst_ratio, worst_use))


def _pose_defects(P, c):
    """(|R'R - I|, |det R - 1|, reprojection of the three triangle points) of a 3 x 4 matrix, in longdouble."""
    P = RR._ld(P)
    R = P[:, :3]
    orth = float(np.max(np.abs(R.T @ R - np.eye(3, dtype=RR.LD))))
    det = float(abs(np.sum(R[0] * RR._cross(R[1], R[2])) - 1))
    tri = list(c['tri'])
    h = R @ RR._ld(c['X'][:, tri]) + P[:, 3:4]
    rep = float(np.max(np.abs(h[:2] / h[2] - RR._ld(c['x'][:, tri]))))
    return orth, det, rep


def test_returned_pose_is_a_pose(hip):
    """R'R = I, det R = +1 and the three triangle points reproject onto their image points -- each defect at most 8
    times the float64 restatement's own on the case plus 64 eps (R and the normalised image points are of size 1).
    Measured: largest defects 4.1e-16 (R'R - I), 4.4e-16 (det R - 1) and 2.2e-12 in the reprojection (seed 17, the
    worst-conditioned case, where the restatement has 8.2e-12)."""
    used, _ = IC.resect_cases()
    worst = np.zeros(3)
    for c in used:
        P, _ = _run(hip, [_cam(c)])
        dev, orc = _pose_defects(P[0], c), _pose_defects(c['Po'], c)
        worst = np.maximum(worst, dev)
        print('seed %2d: device orth %.2e det %.2e reproj %.2e | restatement %.2e %.2e %.2e' % ((c['seed'],) + dev + orc))
        for a, b in zip(dev, orc):
            assert a <= 8 * b + 64 * EPS, (c['seed'], dev, orc)
        assert np.sum(RR._ld(P[0])[0, :3] * RR._cross(RR._ld(P[0])[1, :3], RR._ld(P[0])[2, :3])) > 0
    print('resection, pose defects: orth %.2e det %.2e reproj %.2e' % tuple(worst))


@pytest.mark.parametrize('npt', [3, 4, 63, 64, 65, 129, 200])
def test_rms_is_the_rms_of_the_returned_pose(hip, npt):
    """The returned rms against the rms recomputed from the returned P over all npt check points (noise of 1e-3 on
    the points outside the triangle: a dropped or doubled lane of the 64-lane stride moves the rms by 1 / npt of
    itself), to (npt + 16) eps relative.  The reference is resect_ref.rms_exact: the mean square in rational
    arithmetic rounded to longdouble -- with npt = 3 every check point is one the pose was solved from, the rms is
    1e-15, and a plain longdouble evaluation knows it to 1e-4 only.
    Measured: 1.0 eps at npt = 3, 0.6 eps at 129, 0.1 eps or less elsewhere.  With the residuals evaluated plainly in
    float64 (h = P [Q; 1], h0 / h2 - xn: the kernel before this test) the differences were 1.8e13 eps at npt = 3,
    106 eps at 4, 62 eps at 63 and 21 ... 45 eps beyond: the cancellation in h and in the difference, which k_resect
    now avoids by error-free sums and products (rs_dot2, rs_resid)."""
    c = IC.resect_case(1, npt=npt, noise=1e-3)
    P, rms = _run(hip, [_cam(c)])
    ref = RR.rms_exact(P[0], c['X'], c['x'])
    rel = abs(float((RR.LD(rms[0]) - ref) / ref))
    print('npt %3d: rms %.6e longdouble %.6e relative difference %.3e = %.1f eps (allowed %d eps)'
          % (npt, rms[0], float(ref), rel, rel / EPS, npt + 16))
    assert rel <= (npt + 16) * EPS, (npt, rms[0], float(ref), rel / EPS)


def test_same_triangle_twice_is_the_triangle_once(hip):
    """(a) The first of equal minima: a triangle listed twice gives the bits of the triangle listed once."""
    for seed in (0, 1, 2):
        c = _noisy_case(seed)
        P1, r1 = _run(hip, [_cam(c)])
        P2, r2 = _run(hip, [_cam(c, [c['tri'], c['tri']])])
        assert np.isfinite(P1).all() and _same_bits(P1, P2) and _same_bits(r1, r2)


def test_better_triangle_wins_in_either_order(hip):
    """(b) Two triangles of one camera, noisy image points: the better one wins as [A, B] and as [B, A], with P and rms
    bit-equal to its run alone.  (d) Noisy check points, triangle A on noisy points, triangle B on noise-free ones: B."""
    for seed in (0, 1, 2, 3):
        c = _noisy_case(seed)
        A = c['tri']
        B = _largest_triangle(c['x'], np.setdiff1d(np.arange(20), A))
        (PA, rA), (PB, rB) = _run(hip, [_cam(c, [A])]), _run(hip, [_cam(c, [B])])
        refA = float(RR.best_pose(RR.resect_3pt(c['X'], c['x'], A))[1])
        refB = float(RR.best_pose(RR.resect_3pt(c['X'], c['x'], B))[1])
        assert abs(refA - refB) > 1e-6 * max(refA, refB)            # (the case has a better triangle)
        Pw, rw = (PA, rA) if refA < refB else (PB, rB)
        assert (rA[0] < rB[0]) == (refA < refB)
        for order in ([A, B], [B, A]):
            P, r = _run(hip, [_cam(c, order)])
            assert _same_bits(P, Pw) and _same_bits(r, rw), (seed, order)
        # (d): the case's largest triangle on noise-free points, the largest of the other points on noisy ones
        Bc, An = A, B
        d = _noisy_case(seed, clean=Bc)
        refA = float(RR.best_pose(RR.resect_3pt(d['X'], d['x'], An))[1])
        refB = float(RR.best_pose(RR.resect_3pt(d['X'], d['x'], Bc))[1])
        assert refB < 0.9 * refA, (seed, refA, refB)                 # (the case: the clean triangle fits better)
        Ps, rs = _run(hip, [_cam(d, [Bc])])
        for order in ([An, Bc], [Bc, An]):
            P, r = _run(hip, [_cam(d, order)])
            assert _same_bits(P, Ps) and _same_bits(r, rs), (seed, order)
        assert abs(rs[0] - refB) <= 1e-6 * refB


def test_winner_among_the_candidates_is_the_references_argmin(hip):
    """(c) Of the up to four poses of one triangle the device returns the one the longdouble reference ranks first:
    on the exact cases and on cases with noisy check points, wherever the reference has more than one candidate."""
    used, _ = IC.resect_cases()
    cases = list(used) + [IC.resect_case(seed, noise=1e-3) for seed in range(8)]
    seen = 0
    for c in cases:
        PP, res = c['cands']
        if len(PP) < 2:
            continue
        seen += 1
        P, rms = _run(hip, [_cam(c)])
        k_ref = int(np.argmin(np.array(res, dtype=RR.LD)))
        k_dev = int(np.argmin([RR.pose_err(P[0], Q) for Q in PP]))
        assert k_dev == k_ref, (c['seed'], k_dev, k_ref, [float(r) for r in res])
    assert seen >= 20


def test_several_triangles_per_camera(hip):
    """Triangle ranges of length 0, 1, 5 and 35 mixed in one call: every camera returns the bits of the first
    smallest rms among its triangles run alone, which is the triangle the longdouble reference ranks first; the
    camera without a triangle has no pose."""
    from itertools import combinations
    cs = [_noisy_case(10 + k) for k in range(4)]
    all35 = [np.array(t) for t in combinations(range(7), 3)]
    lists = [[], [cs[1]['tri']], all35[3:8], all35]
    P, rms = _run(hip, [_cam(c, T) for c, T in zip(cs, lists)])
    assert np.isnan(P[0]).all() and np.isposinf(rms[0])
    for k in (1, 2, 3):
        solo = [_run(hip, [_cam(cs[k], [T])]) for T in lists[k]]
        r = np.array([s[1][0] for s in solo])
        w = int(np.argmin(r))                                        # (the first of equal minima)
        assert _same_bits(P[k], solo[w][0][0]) and _same_bits(rms[k], r[w]), (k, w)
        ref = np.array([float(RR.best_pose(RR.resect_3pt(cs[k]['X'], cs[k]['x'], T))[1]) for T in lists[k]])
        order = np.argsort(ref)
        if len(ref) > 1:
            assert ref[order[1]] - ref[order[0]] > 1e-6 * ref[order[0]]
        assert order[0] == w, (k, order[0], w)


def test_cameras_of_one_call_are_independent(hip):
    """100 cameras in one call against every camera alone, bit for bit: uneven numbers of check points (3 ... 200, one
    camera with exactly 3) and one to three triangles per camera."""
    sizes = [3, 4, 63, 64, 65, 129, 200]
    cams = []
    for k in range(100):
        npt = sizes[k % 7] if k < 14 else 5 + (37 * k) % 90
        c = _noisy_case(k, npt=npt)
        T = [c['tri']]
        for j in range(k % 3):
            if npt >= 6 + 3 * j:
                T.append(np.arange(3) + 3 + 3 * j)
        cams.append(_cam(c, T))
    assert cams[0][0].shape[1] == 3
    P, rms = _run(hip, cams)
    assert np.isfinite(rms).sum() >= 95
    for k, cam in enumerate(cams):
        P1, r1 = _run(hip, [cam])
        assert _same_bits(P[k], P1[0]) and _same_bits(rms[k], r1[0]), k


def _degenerate(kind, seed):
    c = _noisy_case(seed)
    X, tri = c['X'].copy(), list(c['tri'])
    if kind == 'collinear':                       # (small dyadic coordinates: the cross product is exactly zero)
        X[:, tri] = np.array([[10.0, 20.0, 30.0], [10.0, 14.0, 18.0], [1.0, 1.0, 1.0]])
    elif kind == 'same12':
        X[:, tri[2]] = X[:, tri[1]]
    elif kind == 'same02':
        X[:, tri[2]] = X[:, tri[0]]
    c['X'] = X
    c['x'] = np.asarray(RR.project_ld(c['R'], c['C'], X), float)
    return c


def test_cameras_without_a_pose(hip):
    """A camera with no triangle, a collinear triangle, a triangle with two identical points (either pair): P all NaN
    and rms = +Inf, as the longdouble reference has no candidate there; the neighbours in the call keep their bits."""
    good = [_noisy_case(30 + k) for k in range(3)]
    bad = [_degenerate(kind, 40 + k) for k, kind in enumerate(('collinear', 'same12', 'same02'))]
    for c in bad:
        assert RR.resect_3pt(c['X'], c['x'], c['tri'])[0] == []
    cams = [_cam(good[0]), _cam(good[1], []), _cam(bad[0]), _cam(good[1]), _cam(bad[1]), _cam(bad[2]), _cam(good[2])]
    P, rms = _run(hip, cams)
    for k in (1, 2, 4, 5):
        assert np.isnan(P[k]).all() and np.isposinf(rms[k]), (k, P[k], rms[k])
    for k, g in ((0, good[0]), (3, good[1]), (6, good[2])):
        P1, r1 = _run(hip, [_cam(g)])
        assert np.isfinite(P1).all() and _same_bits(P[k], P1[0]) and _same_bits(rms[k], r1[0]), k


def test_resect_reports_a_camera_without_a_pose(hip):
    """Through initial.resect: a station whose only three control points are collinear fails (fail = True, its EO all
    NaN, rms = Inf), the other stations get their poses."""
    from dbat_amd import initial as I
    from test_initial import _exact_scene
    s = _exact_scene()
    rows0 = np.flatnonzero(s.IP.cam == 0)
    p = s.IP.pt[rows0][:3]
    OP = s.OP.val.copy()
    OP[:, p[0]] = np.round(OP[:, p[0]] * 32) / 32
    OP[:, p[2]] = np.round(OP[:, p[2]] * 32) / 32
    OP[:, p[1]] = (OP[:, p[0]] + OP[:, p[2]]) / 2
    s.OP.val[:] = OP
    from dbat_amd import synth
    uv, depth = synth.project(s.IO.val, s.EO.val, s.OP.val, s.IP.cam, s.IP.pt, s.IO.sensor.pxSize[0, 0])
    assert (depth < 0).all()
    s.IP.val = uv
    truth = s.EO.val.copy()
    others = np.setdiff1d(np.arange(s.OP.val.shape[1]), s.IP.pt[rows0])
    cp = s.OP.id[np.r_[p, others]]
    s1, rms, fail = I.resect(I.cleareo(s), 'all', cp, 1, 0.0)
    assert fail and np.isnan(s1.EO.val[:6, 0]).all() and np.isposinf(rms[0])
    assert np.isfinite(s1.EO.val[:6, 1:]).all() and np.isfinite(rms[1:]).all()
    assert np.abs(s1.EO.val[:3, 1:] - truth[:3, 1:]).max() < 1e-6


def test_large_coordinates(hip):
    """The seeded cases shifted by (6.5e5, 6.2e6, 100): the rotation part of P and the centre -R't, taken in longdouble
    from the device's P, under the 8x rule against the float64 restatement on the shifted case (floors: 64 eps for R,
    64 eps max|C| for the centre).
    Measured: centre, device / restatement between 0.05 and 2.89 (errors of 1e-10 ... 3e-9 m at 6.2e6 m: the last
    bit or two of the coordinate on either side); rotation, between 0.05 and 2.7 but for seed 1, 11.96 -- 1.1e-14
    against a restatement that happens to be right to 4 eps there (9.0e-16), inside the 64 eps floor."""
    used, _ = IC.resect_cases(IC.SHIFT)
    assert len(used) == 20
    worst = np.zeros(2)
    for c in used:
        P, rms = _run(hip, [_cam(c)])
        _, eR, eC = IC.pose_errors(P[0], c['Pref'])
        _, oR, oC = c['oracle_err']
        sizeC = float(np.max(np.abs(RR.centre_ld(c['Pref']))))
        print('seed %2d: R device %.3e restatement %.3e ratio %.2f | centre device %.3e restatement %.3e ratio %.2f'
              % (c['seed'], eR, oR, eR / oR, eC, oC, eC / oC))
        worst = np.maximum(worst, [eR / oR, eC / oC])
        assert eR <= 8 * oR + 64 * EPS, (c['seed'], eR, oR)
        assert eC <= 8 * oC + 64 * EPS * sizeC, (c['seed'], eC, oC)
    print('resection, 1e6 m: largest ratio R %.2f centre %.2f' % tuple(worst))
