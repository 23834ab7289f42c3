"""Least-squares relative orientation without a GPU (dbat_hip_pairadjust; dbat_amd.initial.refine_pairs, relorient(refine=True)):
the NumPy restatement of tests/pairadjust_ref.py against oracle/dbat_oracle.bundle in the other gauge, the seeded cases
that tests/test_pairadjust_gpu.py runs on the device with the properties their seeds were chosen for, the ray-angle
filter and the floor of the stopping rule, the singular case, the ABI, and everything the library refuses before it
touches a device.

The gauge test: bundle() fixes camera 0 and the largest coordinate of the baseline, the restatement fixes camera 0 and
the baseline's length; the two have the same optimum up to the scale of the model.  Figures measured here (printed by
every run, pytest -s): sigma0 agrees to 3.1e-15 relative, R to 1.4e-12, t / |t| to 8.4e-12, the scaled points to
4.3e-11 (on other seeds up to 1e-14, 2e-10, 5e-10 and 8e-9); the bounds are 1e-10, 1e-8, 1e-8 and 1e-6."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import dbat_oracle as o
import pairadjust_ref as pr
import relorient_ref as rr
from dbat_amd import _hip
from dbat_amd import initial as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1: the two gauges have one optimum ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def gauge_case(n=60, seed=14, noise_px=0.7):
    """A two-image struct without distortion -- IO blocks of their own, focal lengths 8 and 12 mm, anisotropic IP.std,
    noise of 0.7 px -- in the frame of camera 0 with a baseline of length one, at a perturbed start, with the datum of
    test_relorient_gpu.test_pipeline (camera 0 fixed, and the coordinate of camera 1 that is largest); and the same
    start as the restatement takes it: x1, x2, w1, w2, R0, t0, X0.  (The seed: at 1e-9 the Gauss-Newton-Armijo iteration
    of bundle() ends on about half of the seeds 1 .. 20 with a line search that finds no step at the rounding of the
    objective, code -3, in the oracle, on the device, or in both; on this one |J p| / |r| falls 1e-4, 1e-6, 2e-8, 5e-10 and
    both converge in 6 iterations.)"""
    from dbat_amd import synth
    from dbat_amd.dbatstruct import make_struct
    rng = np.random.default_rng(seed)
    S = rr.synthetic_pair(rng, n, front=-1)
    IO = np.zeros((10, 2))
    IO[0], IO[1], IO[2] = (8.0, 12.0), (0.11, -0.07), (-0.05, 0.09)
    EO = np.zeros((6, 2))
    EO[:3, 1], EO[3:6, 1] = -S['R'].T @ S['t'], I.derotmat3d(S['R'])
    cam, pt = np.repeat([0, 1], n), np.tile(np.arange(n), 2)
    px = 0.005
    ip = synth.project(IO, EO, S['X'], cam, pt, px)[0] + noise_px * rng.normal(size=(2, 2 * n))
    std = np.stack([rng.uniform(0.5, 1.0, 2 * n), rng.uniform(1.0, 2.0, 2 * n)])
    R0 = rr.rodrigues(0.01 * rng.normal(size=3)) @ S['R']
    t0 = S['t'] + 0.02 * rng.normal(size=3)
    t0 = t0 / np.linalg.norm(t0)
    s = make_struct(IO, EO, S['X'], np.asfortranarray(ip), cam, pt, px, ip_std=std, distModel=3,
                    IOblock=np.tile(np.arange(1, 3), (10, 1)))
    pts, x1, x2 = I.pair_points(s, 0, 1)
    assert np.array_equal(pts, np.arange(n))
    w1, w2 = I.pair_weights(s, 0, 1)
    X0 = rr.forwintersect3([np.eye(3, 4), np.hstack([R0, t0[:, None]])], np.stack([x1, x2], 1))
    s.EO.val[:3, 1], s.EO.val[3:6, 1] = -R0.T @ t0, I.derotmat3d(R0)
    s.OP.val[:] = X0
    s.bundle.est.EO[:, 0] = False
    s.bundle.est.EO[int(np.argmax(np.abs(s.EO.val[:3, 1]))), 1] = False
    return dict(s=s, x1=x1, x2=x2, w1=w1, w2=w2, R0=R0, t0=t0, X0=X0, truth=S)


def bundle_in_pair_gauge(s2):
    """(R, t / |t|, X / |t|) of a converged two-image struct whose camera 0 is the origin."""
    R = I.rotmat3d(s2.EO.val[3:6, 1])
    t = -R @ s2.EO.val[:3, 1]
    return R, t / np.linalg.norm(t), s2.OP.val / np.linalg.norm(t)


def test_gauge():
    c = gauge_case()
    assert np.all(c['s'].IO.val[5:] == 0) and len(set(c['s'].IO.val[0])) == 2 and np.any(c['s'].IP.std[0] != c['s'].IP.std[1])
    s2, ok, iters, s0, E = o.bundle(c['s'], 50, 'gna', 1e-9)
    assert ok and E.code == 0
    a = pr.adjust(c['x1'], c['x2'], c['R0'], c['t0'], c['X0'], w1=c['w1'], w2=c['w2'], front=-1, max_iter=50, conv_tol=1e-9)
    assert a['code'] == 0 and a['n'] == 60
    R, t, X = bundle_in_pair_gauge(s2)
    d = (abs(a['sigma0'] / s0 - 1), np.abs(a['R'] - R).max(), np.abs(a['t'] - t).max(), np.abs(a['X'] - X).max())
    print('gauge: bundle() %d iterations, restatement %d (%d trials); sigma0 %.6f; differences sigma0 %.1e R %.1e t %.1e X %.1e'
          % (iters, a['iters'], a['trials'], s0, *d))
    assert d[0] < 1e-10 and d[1] < 1e-8 and d[2] < 1e-8 and d[3] < 1e-6


# ---- 2: the seeded cases shared with the GPU tests ----------------------------------------------------------------------

CASES = [(n, noise) for n in pr.SIZES for noise in pr.NOISES]


@functools.lru_cache(maxsize=None)
def seeded(n, noise):
    """(the case, the float64 restatement's result, the np.longdouble one's)."""
    c = pr.seeded_case(n, noise)
    return c, pr.run_case(c), pr.run_case(c, np.longdouble)


def rotation_angle(A, B):
    return float(np.arccos(np.clip((np.trace(np.asarray(A, float) @ np.asarray(B, float).T) - 1) / 2, -1, 1)))


@pytest.mark.parametrize('n,noise', CASES)
def test_seeded_cases(n, noise):
    c, a, b = seeded(n, noise)
    s2 = np.sin(pr.ray_angles(c['x1'], c['x2'], c['R0'])) ** 2 / np.sin(pr.MIN_ANGLE) ** 2
    stat = noise > 0 and n >= 6
    print('n %4d noise %.0e: %d used, %d / %d iterations, %d / %d trials, sigma0 %.3e, float64 to longdouble %.2e; rotation '
          'error %.2e -> %.2e' % (n, noise, a['n'], a['iters'], b['iters'], a['trials'], b['trials'], a['sigma0'],
                                  pr.distance(a, b, stat), rotation_angle(c['R0'], c['R']), rotation_angle(a['R'], c['R'])))
    assert a['code'] == 0 and b['code'] == 0
    assert np.abs(s2 - 1).min() > 1e-6, 'a ray angle at the threshold'
    assert np.array_equal(a['used'], b['used'])
    assert np.all(np.isfinite(a['R'])) and np.all(np.isfinite(a['X'])) and abs(np.linalg.norm(a['t']) - 1) < 1e-14
    if noise > 0 and n >= 8:
        assert rotation_angle(a['R'], c['R']) < rotation_angle(c['R0'], c['R'])
    if noise == 0:
        assert a['f'] <= pr.FLOOR * 4 * a['n'] * 10 and rotation_angle(a['R'], c['R']) < 1e-7


def test_noise_free_floor():
    """The worst float64-to-longdouble distance of the noise-free cases: what FLOOR of the GPU tests is ten times of."""
    worst = max(pr.distance(seeded(n, 0.0)[1], seeded(n, 0.0)[2], False) for n in pr.SIZES)
    print('noise-free cases: float64 to longdouble at most %.3e' % worst)
    assert worst < 1e-12


# ---- 3: the filter and the floor ----------------------------------------------------------------------------------------

def test_filter_uses_61_and_converges():
    c, a, _ = seeded(63, 5e-4)
    ang = np.rad2deg(np.sort(pr.ray_angles(c['x1'], c['x2'], c['R0']))[:3])
    print('n = 63: smallest ray angles %s deg; with 0.5 deg %d used, code %d, %d iterations' % (np.round(ang, 3), a['n'], a['code'], a['iters']))
    assert a['n'] == 61 and a['code'] == 0


FILTER_SEED = 1007      # of the seeds 1 .. 4000 at n = 63 one of nine that converge with the filter and not without it


@functools.lru_cache(maxsize=None)
def filter_case():
    """A pair that needs the filter: n = 63 with noise, two correspondences below 0.5 deg (0.338 deg the smallest), both
    in front at the start.  (The seeded case n = 63 does not serve: of its two correspondences below 0.5 deg the one at
    0.395 deg starts behind both cameras -- z = +0.445 / +1.403 where front is -z -- so the selection at the start leaves
    it out whatever min_angle is, 62 are used, and the adjustment converges.)"""
    return pr.seeded_case(63, 5e-4, seed=FILTER_SEED)


def test_unfiltered_case_does_not_converge():
    c = filter_case()
    ang = np.rad2deg(np.sort(pr.ray_angles(c['x1'], c['x2'], c['R0']))[:3])
    for dtype in (float, np.longdouble):
        a, b = pr.run_case(c, dtype, min_angle=0.0), pr.run_case(c, dtype)
        print('seed %d, %s: smallest ray angles %s deg; min_angle 0: %d used, code %d, %d iterations, f %.4f, max |X| %.3g; 0.5 deg: %d '
              'used, code %d, %d iterations, f %.4f' % (FILTER_SEED, np.dtype(dtype).name, np.round(ang, 3), a['n'], a['code'], a['iters'],
                                                        a['f'], np.abs(a['X']).max(), b['n'], b['code'], b['iters'], b['f']))
        assert a['n'] == 63 and a['code'] != 0 and a['iters'] == 100
        assert b['n'] == 61 and b['code'] == 0
        assert np.all(np.isfinite(np.asarray(a['X'], float))) and np.all(np.isfinite(np.asarray(a['R'], float))) and np.isfinite(float(a['f']))


def test_floor_ends_a_noise_free_case():
    c, a, _ = seeded(64, 0.0)
    assert a['code'] == 0 and a['f'] <= pr.FLOOR * 4 * 64
    # without noise q <= tol^2 f is out of reach: the last trial's f is what ended it
    assert a['f'] > 0 and a['sigma0'] < 1e-11


# ---- 4: the singular case -------------------------------------------------------------------------------------------------

def five_copies():
    """Five copies of the first correspondence of the noise-free case n = 8, at its start."""
    c = dict(pr.seeded_case(8, 0.0))
    for k in ('x1', 'x2', 'X0'):
        c[k] = np.repeat(c[k][:, :1], 5, 1)
    return c


def test_singular_case():
    a = pr.run_case(five_copies())
    print('five copies: code %d after %d iterations, f %.2e' % (a['code'], a['iters'], a['f']))
    assert a['code'] == 3 and a['n'] == 5
    assert np.all(np.isfinite(a['R'])) and np.all(np.isfinite(a['t'])) and np.all(np.isfinite(a['X'])) and np.all(np.isnan(a['Q']))


# ---- 5: the ABI and the refusals, before any device call ----------------------------------------------------------------

def test_symbols_declared():
    hdr = open(os.path.join(ROOT, 'include', 'dbat_hip.h')).read()
    assert re.search(r'#define DBAT_HIP_ABI_VERSION 5\b', hdr) and _hip.ABI_VERSION == 5
    for name in ('dbat_hip_pairadjust', 'dbat_hip_default_pair_options'):
        assert re.search(r'\bint\s+%s\(' % name, hdr), name
        assert name in _hip.SYMBOLS
    assert re.search(r'typedef struct dbat_hip_pair_options \{\s*int32_t max_iter;[^}]*double\s+conv_tol;[^}]*double\s+min_angle;', hdr)
    lib = _hip.load()
    assert lib.dbat_hip_abi_version() == 5
    opt = _hip.PairOptions()
    assert lib.dbat_hip_default_pair_options(C.byref(opt)) == 0 and (opt.max_iter, opt.conv_tol, opt.min_angle) == (20, 1e-6, 0.0)
    import inspect
    sig = inspect.signature(I.relorient).parameters
    assert sig['refine'].default is False and sig['min_angle_deg'].default == 0.0
    assert inspect.signature(I.refine_pairs).parameters['min_angle_deg'].default == 0.0
    assert inspect.signature(_hip.pairadjust).parameters['min_angle'].default == 0.0


def einval(fn, *a, **kw):
    with pytest.raises(_hip.DbatHipError) as ei:
        fn(*a, **kw)
    assert ei.value.code == _hip.EINVAL, ei.value
    return str(ei.value)


def passes_checks(**kw):
    """What passes every check ends at the device: without one that is the only error left."""
    try:
        _hip.pairadjust(**kw)
    except _hip.DbatHipError as e:
        assert e.code == _hip.EDEVICE, e


def test_refusals_without_device():
    _hip.load()
    c = pr.seeded_case(8, 5e-4)
    two = lambda a: np.concatenate([a, a], 1)
    P = np.stack([np.hstack([c['R0'], c['t0'][:, None]])] * 2)
    base = dict(pt_start=[0, 8, 16], x1=two(c['x1']), x2=two(c['x2']), P2=P, X=two(c['X0']), front_dir=-1)
    call = lambda **kw: einval(_hip.pairadjust, **{**base, **kw})
    put = lambda a, idx, v: (lambda b: (b.__setitem__(idx, v), b)[1])(np.array(a, float))
    for bad in (np.nan, np.inf):
        assert 'not finite' in call(x1=put(base['x1'], (0, 3), bad))
        assert 'not finite' in call(x2=put(base['x2'], (1, 11), bad))
        assert 'weight' in call(w1=put(np.ones((2, 16)), (1, 2), bad))
        assert 'P2' in call(P2=put(P, (1, 2, 3), bad))
        assert 'P2' in call(P2=put(P, (0, 1, 1), bad))
        assert 'to be used' in call(X=put(base['X'], (2, 9), bad))
    use = np.ones(16, bool)
    use[9] = False                     # a point that is not to be used may be anything
    passes_checks(**{**base, 'X': put(base['X'], (2, 9), np.nan), 'use': use})
    for w in (0.0, -1.0):
        assert 'weight' in call(w2=put(np.ones((2, 16)), (0, 15), w))
    for fd in (0, 2, -3):
        assert 'front_dir' in call(front_dir=fd)
    Rbad = P.copy()
    Rbad[1, :, :3] = Rbad[1, :, :3] @ np.diag([1.0, 1.0, 1.0 + 1e-5])
    assert 'rotation' in call(P2=Rbad)
    Rneg = P.copy()
    Rneg[0, :, :3] = -Rneg[0, :, :3]
    assert 'rotation' in call(P2=Rneg)
    assert 'zero' in call(P2=put(P, (1, slice(None), 3), 0.0))
    for mi in (0, -1, 201):
        assert 'max_iter' in call(max_iter=mi)
    for tol in (0.0, -1e-6, np.nan):
        assert 'conv_tol' in call(conv_tol=tol)
    for ang in (-1e-3, np.pi / 2, 2.0, np.nan):
        assert 'min_angle' in call(min_angle=ang)
    assert 'ascend' in call(pt_start=[0, 9, 8], x1=base['x1'][:, :8], x2=base['x2'][:, :8], X=base['X'][:, :8])
    assert 'start at 0' in call(pt_start=[1, 8, 16])
    passes_checks(**base)
