"""Network transforms on the device (dbat_hip_rigidalign, dbat_hip_multixform, csrc/align.hpp; dbat_amd.rigidalign,
multixform, multialign, transform_network, align_network) against the NumPy restatement of misc/rigidalign.m,
photogrammetry/pm_multixform.m and pm_multialign.m of tests/test_align_cpu.py.

rigidalign's tolerance is measured, not fixed: the device may differ from the np.longdouble restatement by at most
eight times what the float64 restatement differs from it on the same input (eight: a summation order other than
NumPy's pairwise sums), with a floor of 16 machine epsilons times the magnitude of the quantity -- 1 for R and alpha,
|ym| + alpha |xm| for d, the rms itself for the rms.  The residuals alpha R x + d - y are held to the bound of d: they
are residuals with respect to the T that is returned, and its d is a float64 number of the magnitude |ym| + alpha |xm|,
so a residual is defined to a rounding of that magnitude and no further.  The ratios error / bound that were measured
are printed (pytest -s) and recorded in DESIGN.md."""
import functools

import numpy as np
import pytest

import dbat_oracle as o
from helpers import relerr, synth_struct
from test_align_cpu import (random_rotation, ref_multialign, ref_multixform, ref_rigidalign, similarity)

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
TOL_X = 1e-6           # converged parameters, relative (tests/test_hip_parity.py)
OFFSET = np.array([1e6, 2e6, 3e2])


@pytest.fixture(scope='module')
def hip():
    from dbat_amd import _hip
    import torch
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    _hip.load()
    return _hip


def align_case(n, masked, offset=OFFSET, mirrored=False, seed=0):
    """X, Y, use: n columns at a spread of 10 m about offset, Y a similarity of X (rotation, scale 1.3, shift) with 1 mm
    of noise.  masked: every third column is dropped and holds NaN or a far-off point; the three- and four-column sets,
    which cannot lose a column, get two such columns more instead."""
    rng = np.random.default_rng(1000 * n + seed)
    total = n if (not masked or n > 4) else n + 2
    X = offset[:, None] + rng.normal(0, 10, (3, total))
    R = random_rotation(rng)
    if mirrored:
        R = np.diag([1.0, 1.0, -1.0]) @ R
    Y = 1.3 * R @ (X - offset[:, None]) + (offset[::-1] * 2)[:, None] + rng.normal(0, 1e-3, (3, total))
    if not masked:
        return X, Y, None
    use = np.ones(total, bool)
    use[(np.arange(2, total, 3) if n > 4 else [1, total - 1])] = False
    drop = np.flatnonzero(~use)
    X[:, drop[::2]] = np.nan
    Y[:, drop[1::2]] += 1e4
    return X, Y, use


def check_rigidalign(hip, X, Y, use, scale, label):
    ld = ref_rigidalign(X, Y, scale, use, np.longdouble)
    f64 = ref_rigidalign(X, Y, scale, use, np.float64)
    T, st, resid = hip.rigidalign(X, Y, scale, use=use, resid=True)
    T2, st2, resid2 = hip.rigidalign(X, Y, scale, use=use, resid=True)
    assert np.array_equal(T, T2) and st == st2 and np.array_equal(resid, resid2, equal_nan=True), 'two calls differ'
    alpha = st['alpha']
    R, d = T[:3, :3] / alpha, T[:3, 3]
    mag_d = float(np.linalg.norm(ld['ym']) + abs(ld['alpha']) * np.linalg.norm(ld['xm']))
    used = np.ones(X.shape[1], bool) if use is None else use
    dev = dict(R=R, alpha=alpha, d=d, rms=st['rms'], resid=resid[:, used])
    ratios = {}
    for key, mag in (('R', 1.0), ('alpha', 1.0), ('d', mag_d), ('rms', float(ld['rms'])), ('resid', mag_d)):
        want = ld[key][:, used] if key == 'resid' else ld[key]
        have64 = f64[key][:, used] if key == 'resid' else f64[key]
        err = float(np.max(np.abs(np.asarray(dev[key], np.longdouble) - want)))
        ref_err = float(np.max(np.abs(np.asarray(have64, np.longdouble) - want)))
        bound = max(8 * ref_err, 16 * EPS * mag)
        ratios[key] = (err / bound, err, ref_err)
    print('rigidalign %-28s ' % label + '  '.join('%s %.4f (%.1e | f64 %.1e)' % ((k,) + v) for k, v in ratios.items()))
    for key, v in ratios.items():
        assert v[0] <= 1.0, (label, key, v)
    if not scale:
        assert alpha == 1.0
    assert st['used'] == int(used.sum()) and np.isnan(resid[:, ~used]).all()
    assert abs(st['sv_ratio'] - float(ld['sv'][1] / ld['sv'][0])) < 1e-9
    assert abs(np.linalg.det(R) - 1) < 1e-14 and np.array_equal(T[3], [0, 0, 0, 1])
    return ratios


@pytest.mark.parametrize('n', [3, 4, 255, 256, 257, 65537])
def test_rigidalign_sizes(hip, n):
    """The minimum, the workgroup boundary, more than one level of the reduction tree; each with and without the scale
    and with and without a mask, at 1e6 m."""
    for scale in (False, True):
        for masked in (False, True):
            X, Y, use = align_case(n, masked)
            check_rigidalign(hip, X, Y, use, scale, 'n=%d scale=%d mask=%d' % (n, scale, masked))


def test_rigidalign_about_the_origin(hip):
    for scale in (False, True):
        X, Y, use = align_case(257, True, offset=np.zeros(3), seed=1)
        check_rigidalign(hip, X, Y, use, scale, 'origin n=257 scale=%d mask=1' % scale)


def test_rigidalign_of_a_mirrored_set_is_a_proper_rotation(hip):
    X, Y, use = align_case(257, False, mirrored=True, seed=2)
    check_rigidalign(hip, X, Y, use, True, 'mirrored n=257 scale=1')
    T, st, _ = hip.rigidalign(X, Y, True)
    assert abs(np.linalg.det(T[:3, :3] / st['alpha']) - 1) < 1e-14 and st['rms'] > 1.0


def test_rigidalign_python_signature(hip):
    import dbat_amd
    X, Y, use = align_case(40, True, seed=3)
    T, R, d, alpha = dbat_amd.rigidalign(X, Y, True, use=use)
    ref = ref_rigidalign(X, Y, True, use)
    assert np.abs(R - ref['R']).max() < 1e-13 and abs(alpha - ref['alpha']) < 1e-13
    assert np.abs(T - similarity(R, alpha, d)).max() == 0
    assert dbat_amd.rigidalign(X[:, use], Y[:, use])[3] == 1.0


# ---- multixform ---------------------------------------------------------------------------------------------------

def cameras(rng, nc, rows=6):
    EO = np.zeros((rows, nc), order='F')
    EO[:3] = rng.normal(0, 20, (3, nc))
    EO[3] = rng.uniform(-np.pi, np.pi, nc)
    EO[4] = rng.uniform(-np.pi / 2, np.pi / 2, nc)
    EO[5] = rng.uniform(-np.pi, np.pi, nc)
    if nc > 1:
        EO[4, 1] = np.pi / 2                    # phi = pi/2 exactly
    if nc > 2:
        EO[4, 2] = -np.pi / 2
    if rows > 6:
        EO[6:] = rng.normal(size=(rows - 6, nc))
    return EO


def check_multixform(EO, OP, T, out):
    """out = multixform(EO, OP, T) against the float64 restatement: points and centres to 1e-12 of their magnitude,
    eulerrotmat of the returned angles against M' R' to 1e-12, the angles inside the ranges of derotmat3d.m:9-11."""
    EO2, OP2, fail = out
    rEO, rOP, rfail, N = ref_multixform(EO, OP, T)
    alpha = np.cbrt(np.linalg.det(T[:3, :3]))
    shift = np.linalg.norm(T[:3, 3])
    assert OP2.shape == np.shape(OP) and EO2.shape == np.shape(EO) and np.array_equal(fail, rfail)
    if np.size(OP):
        mag = alpha * np.linalg.norm(OP, axis=0) + shift
        ok = np.isfinite(rOP).all(0)
        assert np.all(np.abs(OP2 - rOP)[:, ok] <= 1e-12 * mag[ok]) and np.isnan(OP2[:, ~ok]).all()
    if np.size(EO):
        good = ~rfail
        mag = alpha * np.linalg.norm(np.asarray(EO)[:3], axis=0) + shift
        assert np.all(np.abs(EO2[:3] - rEO[:3])[:, good] <= 1e-12 * mag[good])
        assert np.array_equal(EO2[:, ~good], np.asarray(EO)[:, ~good], equal_nan=True)
        assert np.array_equal(EO2[6:], np.asarray(EO)[6:])
        a = EO2[3:6, good]
        assert np.all(np.abs(a[0]) <= np.pi) and np.all(np.abs(a[1]) <= np.pi / 2) and np.all(np.abs(a[2]) <= np.pi)
        worst = 0.0
        for i in np.flatnonzero(good):
            worst = max(worst, np.abs(o.eulerrotmat(EO2[3:6, i]).T - N[i]).max())
        assert worst <= 1e-12, worst


@functools.lru_cache(maxsize=None)
def xform_T(alpha):
    return similarity(random_rotation(np.random.default_rng(int(alpha * 10))), alpha, [1e3, -2e3, 5e2])


@pytest.mark.parametrize('nc', [1, 64, 65, 1000])
@pytest.mark.parametrize('npnt', [1, 257, 65537])
def test_multixform_sizes(hip, nc, npnt):
    from dbat_amd import multixform
    rng = np.random.default_rng(nc + npnt)
    EO, OP = cameras(rng, nc), rng.normal(0, 50, (3, npnt))
    check_multixform(EO, OP, xform_T(1.7), multixform(EO, OP, xform_T(1.7)))


@pytest.mark.parametrize('alpha', [1.0, 0.5, 1.7])
def test_multixform_scales_empty_arrays_seven_rows(hip, alpha):
    from dbat_amd import multixform
    rng = np.random.default_rng(11)
    T = xform_T(alpha)
    EO, OP = cameras(rng, 65), rng.normal(0, 50, (3, 257))
    check_multixform(EO, OP, T, multixform(EO, OP, T))
    e0, p0 = np.zeros((6, 0)), np.zeros((3, 0))
    check_multixform(EO, p0, T, multixform(EO, p0, T))                  # an empty OP
    check_multixform(e0, OP, T, multixform(e0, OP, T))                  # an empty EO
    EO7 = cameras(rng, 65, rows=7)
    check_multixform(EO7, OP, T, multixform(EO7, OP, T))                # the seventh row is left alone
    a, b = multixform(EO7, OP, T), multixform(EO7, OP, T)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('alpha', [1.0, 0.5, 1.7])
def test_multixform_nan_and_gimbal_lock(hip, alpha):
    """A NaN point and a NaN camera stay NaN and the camera is flagged.  Cameras at phi = pi/2 exactly (cameras():
    columns 1 and 2) under a general rotation, under scale and shift alone and under a rotation about the world's x
    axis -- the last two leave them at |phi| = pi/2 --, and camera 3 is constructed so that the general rotation takes
    it TO phi = pi/2: the third row of its M' is the first row of R, and M' R' has (1, ~1e-16, ~1e-16) there."""
    from dbat_amd import multixform
    rng = np.random.default_rng(12)
    EO, OP = cameras(rng, 9), rng.normal(0, 50, (3, 20))
    OP[1, 4] = np.nan
    EO[2, 5] = np.nan
    EO[4, 7] = np.nan
    r1 = (xform_T(alpha)[:3, :3] / alpha)[0]
    EO[3, 3], EO[4, 3] = np.arctan2(-r1[1], r1[2]), np.arcsin(r1[0])
    Rx = o.eulerrotmat(np.array([0.3, 0.0, 0.0]))                        # M31 = M'(3,:) R(1,:)' with R(1,:) = e1
    for T in (xform_T(alpha), similarity(np.eye(3), alpha, [1e3, -2e3, 5e2]), similarity(Rx, alpha, [1.0, 2.0, 3.0])):
        EO2, OP2, fail = out = multixform(EO, OP, T)
        check_multixform(EO, OP, T, out)
        if T is xform_T(alpha):
            assert abs(EO2[4, 3] - np.pi / 2) < 1e-7
        assert np.array_equal(np.flatnonzero(fail), [5, 7]) and np.isnan(OP2[:, 4]).all()
        assert np.isnan(EO2[2, 5]) and np.isnan(EO2[4, 7])
    EO2 = multixform(EO, OP, similarity(np.eye(3), alpha, [1e3, -2e3, 5e2]))[0]
    assert abs(EO2[4, 1] - np.pi / 2) < 1e-15 and abs(EO2[4, 2] + np.pi / 2) < 1e-15


@pytest.mark.parametrize('ra', [0.0, np.pi / 2])
def test_multialign(hip, ra):
    from dbat_amd import multialign
    rng = np.random.default_rng(13)
    EO, OP = cameras(rng, 12), rng.normal(0, 50, (3, 30))
    for i in (0, 1, 7):                            # camera 1 is at phi = pi/2
        EO2, OP2, T = multialign(EO, OP, i, ra)
        rEO, rOP, rT = ref_multialign(EO, OP, i, ra)
        assert np.abs(T - rT).max() <= 1e-13 * max(1.0, np.abs(rT).max())
        assert np.abs(EO2[:3, i]).max() <= 1e-12 * np.linalg.norm(EO[:3, i])
        assert np.abs(o.eulerrotmat(EO2[3:6, i]).T - o.eulerrotmat(np.array([0, 0, -ra])).T).max() <= 1e-12
        assert np.abs(EO2[3:6, i] - [0, 0, -ra]).max() <= 1e-12
        check_multixform(EO, OP, T, (EO2, OP2, np.zeros(12, bool)))


# ---- whole structs ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fixed_points_scene():
    """synth 'tiny' with every EO element estimated and five object points fixed at their true values: a datum that is
    invariant under similarities.  Returns (s, truth, the adjusted s, sigma0)."""
    from dbat_amd import bundle
    s, truth = synth_struct('tiny')
    s.bundle.est.EO[:] = True
    k = np.linspace(0, s.OP.val.shape[1] - 1, 5).astype(int)
    s.OP.val[:, k] = truth['OP'][:, k]
    s.bundle.est.OP[:, k] = False
    r, ok, iters, s0, E = bundle(s)
    assert ok
    return s, truth, r, s0


def rotations_of(EO):
    return np.stack([o.eulerrotmat(EO[3:6, i]).T for i in range(EO.shape[1])])


def test_bundle_commutes_with_transform_network(hip):
    """A datum by fixed points is invariant under similarities: bundle(transform_network(s, T)) equals
    transform_network(bundle(s), T).  (The oracle's own bundle() meets the bounds with 1e-13 in the points and 8e-12 in
    the rotation matrices.)"""
    from dbat_amd import bundle, transform_network
    s, truth, r, s0 = fixed_points_scene()
    T = similarity(random_rotation(np.random.default_rng(21)), 1.7, [1e3, -2e3, 5e2])
    a, ok, iters, s0a, E = bundle(transform_network(s, T))
    b = transform_network(r, T)
    assert ok
    print('commute: OP %.2e  centres %.2e  rotations %.2e  sigma0 %.2e'
          % (relerr(a.OP.val, b.OP.val), relerr(a.EO.val[:3], b.EO.val[:3]),
             np.abs(rotations_of(a.EO.val) - rotations_of(b.EO.val)).max(), abs(s0a / s0 - 1)))
    assert relerr(a.OP.val, b.OP.val) <= TOL_X and relerr(a.EO.val[:3], b.EO.val[:3]) <= TOL_X
    assert np.abs(rotations_of(a.EO.val) - rotations_of(b.EO.val)).max() <= TOL_X
    assert abs(s0a / s0 - 1) <= 1e-8
    # what transform_network leaves alone is shared, and the input is not written to
    assert b.IP.val is r.IP.val and b.IO.val is r.IO.val and b.OP.val is not r.OP.val
    assert np.array_equal(b.bundle.est.OP, r.bundle.est.OP)


def test_transform_network_priors(hip):
    """Prior positions are transformed where they are in use and their standard deviations scaled by alpha."""
    from dbat_amd import transform_network
    from test_align_cpu import isotropic_priors_struct
    s = isotropic_priors_struct()
    before = (s.prior.OP.val.copy(), s.prior.EO.val.copy(), s.OP.val.copy())
    T = similarity(random_rotation(np.random.default_rng(22)), 0.5, [1e3, -2e3, 5e2])
    t = transform_network(s, T)
    for P, Q, rows in ((s.prior.OP, t.prior.OP, slice(0, 3)), (s.prior.EO, t.prior.EO, slice(0, 3))):
        u = P.use[rows].all(0)
        assert u.any() and np.array_equal(P.use, Q.use)
        want = T[:3, :3] @ P.val[rows][:, u] + T[:3, 3:4]
        assert np.abs(Q.val[rows][:, u] - want).max() <= 1e-12 * np.abs(want).max()
        assert np.array_equal(Q.val[rows][:, ~u], P.val[rows][:, ~u], equal_nan=True)
        assert np.allclose(Q.std[rows][:, u], 0.5 * P.std[rows][:, u], rtol=1e-15)
    assert np.array_equal(t.prior.EO.val[3:], s.prior.EO.val[3:], equal_nan=True)
    assert np.array_equal(t.prior.EO.std[3:], s.prior.EO.std[3:], equal_nan=True)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(before, (s.prior.OP.val, s.prior.EO.val, s.OP.val)))


def test_align_network_on_the_adjusted_scene(hip):
    from dbat_amd import align_network, transform_network
    s, truth, r, s0 = fixed_points_scene()
    npnt = r.OP.val.shape[1]
    # the adjusted network in another datum, and the truth as the reference for two points in three
    T0 = similarity(random_rotation(np.random.default_rng(23)), 1 / 1.7, [-50.0, 20.0, 7.0])
    moved = transform_network(r, T0)
    ref = truth['OP'].copy()
    ref[:, 1::3] = np.nan
    use = np.ones(npnt, bool)
    use[::10] = False
    ok = np.isfinite(ref).all(0) & use
    s2, T, fit = align_network(moved, ref, use=use)
    want = ref_rigidalign(moved.OP.val, ref, True, ok)
    assert np.abs(T - want['T']).max() <= 1e-11 * np.abs(want['T']).max()
    assert abs(fit.alpha - want['alpha']) <= 1e-13 and abs(fit.rms - want['rms']) <= 1e-12 and fit.used == ok.sum()
    assert np.isnan(fit.resid[:, ~ok]).all() and np.abs(fit.resid - want['resid'])[:, ok].max() <= 1e-11
    nrm = np.linalg.norm(want['resid'][:, ok], axis=0)
    assert fit.argmax == np.flatnonzero(ok)[np.argmax(nrm)] and abs(fit.max - nrm.max()) <= 1e-11
    # the alignment undoes T0 up to the estimation error, and brings the points onto the truth
    unaligned = np.sqrt(np.mean(np.sum((moved.OP.val - ref)[:, ok] ** 2, 0)))
    assert fit.rms < unaligned and fit.rms < 0.1
    assert np.abs(T @ T0 - np.eye(4)).max() < 0.1 and relerr(s2.OP.val, r.OP.val) < 1e-3
    assert np.abs(s2.OP.val[:, ok] - ref[:, ok] - fit.resid[:, ok]).max() <= 1e-10
