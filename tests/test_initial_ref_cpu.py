"""The references of the initial-value edge tests, checked without a device: the longdouble restatements of
tests/resect_ref.py recover exact scenes, and every seeded case the GPU tests use (tests/initial_cases.py) is one on
which the float64 restatement (oracle/initial_oracle.py pm_resect_3pt, forwintersect) agrees with the longdouble
reference to a cap -- the 'reference alone' condition of the 8x rule those tests apply to the device.

Resection cap: a relative pose error of 1e-9.  Measured over the 40 drawn seeds (heights 10 ... 40 m over a 40 m
field, the largest triangle, every point inside a +-0.6 format): median 1.4e-14, largest 1.5e-11, so all 40 survive;
the test asks for 90 % so that the filter cannot hide a regression.  The symmetric case (a camera over the centre of an
equilateral triangle), tele geometries and rays more than 90 degrees apart are out of scope: resect_ref's docstring.

Forward intersection cap: 64 eps * cond * max|coordinate| per scene (initial_cases.fwd_reference)."""
import numpy as np
import pytest

import initial_cases as IC
import resect_ref as RR


def test_longdouble_is_wider_than_double():
    assert RR.EPS_LD <= 2.0 ** -63, 'np.longdouble is no wider than float64 here: resect_ref is no reference'


def test_resect_ref_recovers_exact_poses():
    """Exact scenes (a true pose, image points projected in longdouble and NOT rounded to float64): the true
    [R | t] is among the candidates to 1e3 longdouble eps of max|[R | t]|.  The bound is one of rounding times
    conditioning, so it is asked of the well-conditioned cases: those on which the float64 restatement, an
    independent code, stays within 1e3 float64 eps (its own rounding is amplified by the same condition number); at
    least a quarter of the drawn seeds are such.  Every drawn case has the true pose among its candidates to 1e-12,
    which a wrong coefficient or frame misses by orders of magnitude."""
    used, drawn = IC.resect_cases()
    well = 0
    for c in drawn:
        PP, res = RR.resect_3pt(c['X'], c['xl'], c['tri'])
        Pt = np.hstack([c['R'], -(c['R'] @ c['C'])[:, None]])
        size = float(np.max(np.abs(Pt)))
        e = [RR.pose_err(P, Pt) for P in PP]
        k = int(np.argmin(e))
        assert e[k] <= 1e-12 * size, (c['seed'], e[k])
        assert int(np.argmin(np.array(res, dtype=RR.LD))) == k and float(res[k]) < 1e-15, (c['seed'], res)
        if c['rel'] <= 1e3 * RR.EPS:
            well += 1
            assert e[k] <= 1e3 * float(RR.EPS_LD) * size, (c['seed'], e[k] / float(RR.EPS_LD) / size)
    assert well >= len(drawn) // 4, well


def test_polished_roots_are_roots():
    """The polished roots satisfy the longdouble quartic to its own rounding: |p(z)| <= 64 eps_ld * sum |c_i| |z|^i."""
    used, _ = IC.resect_cases()
    for c in used:
        rep = {}
        RR.resect_3pt(c['X'], c['x'], c['tri'], root_report=rep)
        co = rep['coeffs']
        assert rep['converged'].all() and rep['roots'].size == 4
        for z in rep['roots']:
            p = sum(RR.CLD(co[i]) * z ** (4 - i) for i in range(5))
            assert abs(p) <= 64 * RR.EPS_LD * sum(abs(co[i]) * abs(z) ** (4 - i) for i in range(5)), (c['seed'], z)


def test_polished_roots_against_mpmath():
    """Where mpmath imports: the polished roots against polyroots at 50 digits, to the root's own conditioning in
    longdouble: 64 eps_ld * sum |c_i| |z|^i / |p'(z)| (the rounding of the polynomial's value moved through the
    slope), and never more than 1e-12 of the root."""
    mp = pytest.importorskip('mpmath')
    used, _ = IC.resect_cases()
    mp.mp.dps = 50
    for c in used:
        rep = {}
        RR.resect_3pt(c['X'], c['x'], c['tri'], root_report=rep)
        co = [mp.mpf(float(v)) + mp.mpf(float(v - RR.LD(float(v)))) for v in rep['coeffs']]
        exact = mp.polyroots(co, maxsteps=200, extraprec=200)
        for z in rep['roots']:
            zz = mp.mpc(mp.mpf(float(z.real)) + mp.mpf(float(z.real - RR.LD(float(z.real)))),
                        mp.mpf(float(z.imag)) + mp.mpf(float(z.imag - RR.LD(float(z.imag)))))
            d = min(abs(zz - r) for r in exact)
            mag = sum(abs(co[i]) * abs(zz) ** (4 - i) for i in range(5))
            slope = abs(sum((4 - i) * co[i] * zz ** (3 - i) for i in range(4)))
            bound = max(64 * float(RR.EPS_LD) * mag / slope, 4 * float(RR.EPS_LD) * abs(zz))
            assert d <= bound and d <= 1e-12 * abs(zz), (c['seed'], float(d), float(bound))


@pytest.mark.parametrize('shift', [None, IC.SHIFT], ids=['origin', 'far'])
def test_resect_cases_are_well_conditioned(shift):
    """The float64 restatement against the longdouble reference on every drawn seed: at least 90 % stay under the cap
    and become GPU cases, 20 of them are used, and each used case has a clear winner (the reference's best rms is
    below 1e-12, as the scene is exact up to the float64 rounding of its image points)."""
    used, drawn = IC.resect_cases(shift)
    rel = np.array([c['rel'] for c in drawn])
    print('float64 restatement against longdouble, relative pose error: median %.2e max %.2e, %d of %d under %.0e'
          % (np.median(rel), rel.max(), np.count_nonzero(rel < IC.RESECT_CAP), rel.size, IC.RESECT_CAP))
    assert np.count_nonzero(rel < IC.RESECT_CAP) >= 0.9 * len(drawn)
    assert len(used) == IC.RESECT_USED
    for c in used:
        assert c['rel'] < IC.RESECT_CAP and float(c['rms_ref']) < 1e-12, (c['seed'], c['rel'], c['rms_ref'])


def test_noisy_and_sized_resect_cases_are_well_conditioned():
    """The other seeded resection cases of the GPU tests: the check-point counts of the rms test (noise of 1e-3 on the
    points outside the triangle) keep the triangle noise-free, so the pose and its conditioning are those of the
    exact case."""
    for npt in (3, 4, 63, 64, 65, 129, 200):
        c = IC.resect_case(1, npt=npt, noise=1e-3)
        assert c['X'].shape[1] == npt
        if npt == 3:          # no check point outside the triangle: every candidate fits, the winner is anybody's
            size = float(np.max(np.abs(c['Pref'])))
            assert min(RR.pose_err(c['Po'], P) for P in c['cands'][0]) < IC.RESECT_CAP * size
            continue
        assert c['rel'] < IC.RESECT_CAP, (npt, c['rel'])
        if npt > 3:
            assert 2e-4 < float(c['rms_ref']) < 3e-3, (npt, c['rms_ref'])


def test_rms_exact_against_longdouble():
    """The rational-arithmetic rms against the plain longdouble one: to 1e-15 where the residuals are 1e-3 (there the
    longdouble evaluation is good to 1e-16), to 1e-2 where every residual is rounding noise of the float64 pose (npt =
    3), and both of the size the case says."""
    for npt, tol in ((3, 1e-2), (4, 1e-15), (65, 1e-15)):
        c = IC.resect_case(1, npt=npt, noise=1e-3)
        a, b = RR.rms_exact(c['Po'], c['X'], c['x']), RR.rms_ld(c['Po'], c['X'], c['x'])
        assert abs(float((a - b) / a)) <= tol, (npt, float(a), float(b))
        assert (float(a) < 1e-13) == (npt == 3)


@pytest.mark.parametrize('name', IC.FWD_SCENES + ('giant',))
def test_forwintersect_oracle_against_longdouble(name):
    """initial_oracle.forwintersect against the longdouble forward intersection on every scene of the GPU tests:
    the same points are NaN, and the largest error stays under the scene's cap."""
    s, Qld, Qo, err, cap, scale = IC.fwd_reference(name)
    print('%s: float64 restatement against longdouble %.3e m, cap %.3e, max|coordinate| %.3g' % (name, err, cap, scale))
    assert err <= cap, (name, err, cap)


def test_forwintersect_ref_two_rays_closed_form():
    """The longdouble forward intersection of a two-ray point is the midpoint of the rays' common perpendicular."""
    s, Qld, _, _, _, scale = IC.fwd_reference('angle-1e-1')
    c, d = RR.rays_ld(s)
    pt = np.asarray(s.IP.pt)
    for p in range(s.OP.val.shape[1]):
        r = np.flatnonzero(pt == p)
        assert r.size == 2
        m = RR.two_ray_midpoint(c[:, r[0]], d[:, r[0]], c[:, r[1]], d[:, r[1]])
        assert float(np.max(np.abs(m - Qld[:, p]))) <= 1e5 * float(RR.EPS_LD) * scale
