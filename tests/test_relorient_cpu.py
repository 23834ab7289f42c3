"""Relative orientation without a GPU (dbat_hip_essmat5, dbat_hip_relorient; dbat_amd.initial.essmat5, camsfrome,
relorient, relorient_pairs): the NumPy restatement of photogrammetry/essmat5.m and camsfrome.m of
tests/relorient_ref.py against the truth of a synthetic pair, its RANSAC on the two committed real pairs, the ABI, and
everything the library refuses before it touches a device.  Also the seeded cases that tests/test_relorient_gpu.py runs
on the device, with the properties their seeds were chosen for checked here."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import relorient_ref as rr
from dbat_amd import _hip
from dbat_amd import initial as I
from helpers import GOLDEN, camcal_expected, camcal_struct, roma_expected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
hom = lambda x: np.vstack([x, np.ones((1, x.shape[1]))])


# ---- the seeded cases shared with the GPU tests -----------------------------------------------------------------------

MINIMAL_SEED = 388        # 64 sets of five: one with ten solutions real to 1e-8, one with two (checked below; of the seeds
                          # 1 .. 600 the only one)


@functools.lru_cache(maxsize=None)
def minimal_sets(n=5, count=64, seed=MINIMAL_SEED):
    """count noise-free sets of n correspondences, each from a scene of its own: list of synthetic_pair dicts."""
    rng = np.random.default_rng(seed)
    return [rr.synthetic_pair(rng, n) for _ in range(count)]


@functools.lru_cache(maxsize=None)
def minimal_reference(n=5, count=64, seed=MINIMAL_SEED):
    """Per set of minimal_sets: the restatement's solutions at the reference's tolerance (0.01), those whose eigenvalue is
    real to 1e-8, its distance to the true E, and its worst residuals."""
    out = []
    for S in minimal_sets(n, count, seed):
        Q1, Q2 = hom(S['x1']), hom(S['x2'])
        Es, ratio = rr.essmat5(Q1, Q2, full=True)
        res = np.array([rr.residuals(Es[:, k], Q1, Q2) for k in range(Es.shape[1]) if ratio[k] < 1e-8]).reshape(-1, 3)
        out.append(dict(Es=Es, strict=Es[:, ratio < 1e-8], dist=rr.dist_to(S['e'], Es), res=res))
    return out


SCORING_SEED = 11


@functools.lru_cache(maxsize=None)
def scoring_case(seed=SCORING_SEED, n=200, n_hyp=256, outliers=0.3, noise=5e-4, thr=2e-3):
    """One pair of n correspondences, 30 % of them replaced by uniform outliers, noise 5e-4, and 256 samples."""
    rng = np.random.default_rng(seed)
    S = rr.synthetic_pair(rng, n, noise=noise)
    bad = rng.random(n) < outliers
    x2 = S['x2'].copy()
    x2[:, bad] = rng.uniform(-0.5, 0.5, (2, int(bad.sum())))
    samples = I.draw_samples(n, n_hyp, rng)
    return dict(x1=S['x1'], x2=x2, samples=samples, thr2=thr * thr, truth=S, bad=bad)


def borderline(e, x1, x2, thr2):
    """The number of correspondences whose Sampson distance under e lies within 1e-6 relative of the threshold."""
    return int(np.sum(np.abs(rr.sampson2(e, x1, x2) / thr2 - 1) < 1e-6))


def real_struct(name):
    """The image points and camera of a committed project (no EO, no OP needed): roma or camcal."""
    if name == 'camcal':
        return camcal_struct(3)
    from dbat_amd import loadtables as T
    exp = roma_expected()
    ci = exp['camera_in']
    eo = T.load_table(os.path.join(GOLDEN, 'roma-initial_eo.txt'))
    mk = T.load_table(os.path.join(GOLDEN, 'roma-markpts.txt.xz'))
    h = ci['sensor_height']
    io = T.camera_io(ci['cc'], ci['pp'], ci['K'], ci['P'])
    return T.struct_from_tables(io, (ci['image'][0] * h / ci['image'][1], h), ci['image'], eo, mk, 'im,id,x,y', 1.0,
                                distModel=ci['model'])


REAL_SEED, REAL_HYP, REAL_PX = 3, 256, 3.0


@functools.lru_cache(maxsize=None)
def real_pair(name):
    """Pair (0, 1) of roma / camcal: the struct, the normalised common points, the samples of seed 3, the threshold of
    3 px, and the restatement's RANSAC result."""
    s = real_struct(name)
    pts, x1, x2 = I.pair_points(s, 0, 1)
    samples = I.draw_samples(pts.size, REAL_HYP, np.random.default_rng(REAL_SEED))
    thr2 = I.pair_threshold(s, 0, 1, REAL_PX) ** 2
    return dict(s=s, pts=pts, x1=x1, x2=x2, samples=samples, thr2=thr2, ref=rr.ransac(x1, x2, samples, thr2))


def report_relative_rotation(name):
    """R_1 R_0' from the converged EO of the committed report (angles in degrees, rows of EO_report_deg)."""
    eo = np.array((roma_expected()['report'] if name == 'roma' else camcal_expected()['model3'])['EO_report_deg'])
    M = [I.rotmat3d(np.deg2rad(eo[k, :3])) for k in (0, 1)]
    return M[1] @ M[0].T


def rotation_angle(A, B):
    return float(np.arccos(np.clip((np.trace(A @ B.T) - 1) / 2, -1, 1)))


# ---- 1: the restatement against the truth -----------------------------------------------------------------------------

def test_restatement_recovers_truth():
    ref = minimal_reference()
    worst = max(r['dist'] for r in ref)
    print('restatement, 64 minimal sets: worst distance to the true E %.2e' % worst)
    assert worst < 1e-6
    counts = sorted(set(r['Es'].shape[1] for r in ref))
    assert all(c % 2 == 0 and 2 <= c <= 10 for c in counts), counts
    assert any(r['strict'].shape[1] == 10 for r in ref) and any(r['Es'].shape[1] == 2 for r in ref), 'MINIMAL_SEED: no set of ten / two'
    for front in (1, -1):
        S = rr.synthetic_pair(np.random.default_rng(5), 50, front=front)
        Es = rr.essmat5(hom(S['x1']), hom(S['x2']))
        k = int(np.argmin([rr.dist_to(S['e'], Es[:, i:i + 1]) for i in range(Es.shape[1])]))
        assert rr.dist_to(S['e'], Es[:, k:k + 1]) < 1e-9
        P1, P2, X, fr, sp = rr.camsfrome(Es[:, k].reshape(3, 3), hom(S['x1']), hom(S['x2']), front)
        assert np.array_equal(P1, np.eye(3, 4)) and fr.all() and sp[0] == 50 > sp[1]
        assert np.abs(P2 - np.hstack([S['R'], S['t'][:, None]])).max() < 1e-8
        assert np.abs(X - S['X']).max() < 1e-6


def test_restatement_layout():
    """essmat5 follows sum e[a + 3 b] Q1[a] Q2[b] = 0; camsfrome expects xp' E x = 0: E = e.reshape(3, 3)."""
    S = rr.synthetic_pair(np.random.default_rng(1), 8)
    Q1, Q2 = hom(S['x1']), hom(S['x2'])
    Es = rr.essmat5(Q1, Q2)
    e = Es[:, int(np.argmin([rr.dist_to(S['e'], Es[:, i:i + 1]) for i in range(Es.shape[1])]))]
    assert np.abs(sum(e[a + 3 * b] * Q1[a] * Q2[b] for a in range(3) for b in range(3))).max() < 1e-12
    assert np.abs(np.sum(Q2 * (e.reshape(3, 3) @ Q1), 0)).max() < 1e-12


# ---- 2: the ABI ---------------------------------------------------------------------------------------------------------

def test_symbols_declared():
    hdr = open(os.path.join(ROOT, 'include', 'dbat_hip.h')).read()
    assert re.search(r'#define DBAT_HIP_ABI_VERSION 5\b', hdr) and _hip.ABI_VERSION == 5
    for name in ('dbat_hip_essmat5', 'dbat_hip_relorient'):
        assert re.search(r'\bint\s+%s\(' % name, hdr), name
        assert name in _hip.SYMBOLS
    assert callable(I.essmat5) and callable(I.camsfrome) and callable(I.relorient) and callable(I.relorient_pairs)


# ---- 3: refusals, before any device call ----------------------------------------------------------------------------------

def einval(fn, *a, **kw):
    with pytest.raises(_hip.DbatHipError) as ei:
        fn(*a, **kw)
    assert ei.value.code == _hip.EINVAL, ei.value
    return str(ei.value)


def test_refusals_without_device():
    _hip.load()
    rng = np.random.default_rng(0)
    Q = hom(rng.normal(size=(2, 6)))
    assert 'fewer than five' in einval(_hip.essmat5_sets, [0, 4], Q[:, :4], Q[:, :4])
    assert 'fewer than five' in einval(_hip.essmat5_sets, [0, 6, 10], hom(rng.normal(size=(2, 10))), hom(rng.normal(size=(2, 10))))
    Qn = Q.copy()
    Qn[1, 3] = np.nan
    assert 'not finite' in einval(_hip.essmat5_sets, [0, 6], Qn, Q)
    Qn[1, 3] = np.inf
    assert 'not finite' in einval(_hip.essmat5_sets, [0, 6], Q, Qn)
    x1, x2 = rng.normal(size=(2, 12)), rng.normal(size=(2, 12))
    smp = np.array([[0, 1, 2, 3, 4], [1, 2, 3, 4, 5]], np.int32)
    call = lambda **kw: einval(_hip.relorient_pairs, **{**dict(pt_start=[0, 6, 12], x1=x1, x2=x2, hyp_start=[0, 1, 2], samples=smp,
                                                              thr2=[1e-6, 1e-6], front_dir=1), **kw})
    assert 'fewer than five' in call(pt_start=[0, 4, 12])
    xn = x1.copy()
    xn[0, 7] = np.nan
    assert 'not finite' in call(x1=xn)
    assert 'not finite' in call(x2=np.where(np.arange(12) == 2, np.inf, x2))
    assert 'outside' in call(samples=np.array([[0, 1, 2, 3, 6], [1, 2, 3, 4, 5]], np.int32))
    assert 'outside' in call(samples=np.array([[0, 1, 2, 3, 4], [1, 2, -1, 4, 5]], np.int32))
    assert 'repeats' in call(samples=np.array([[0, 1, 2, 3, 4], [1, 2, 3, 4, 1]], np.int32))
    assert 'thr2' in call(thr2=[1e-6, 0.0])
    assert 'thr2' in call(thr2=[-1.0, 1e-6])
    assert 'thr2' in call(thr2=[np.nan, 1e-6])
    for fd in (0, 2, -3):
        assert 'front_dir' in call(front_dir=fd)
    with pytest.raises(ValueError):
        I.draw_samples(4, 3, rng)


def test_draw_samples():
    for n in (5, 6, 15, 16, 1000):
        a = I.draw_samples(n, 300, np.random.default_rng(9))
        b = I.draw_samples(n, 300, np.random.default_rng(9))
        assert a.shape == (300, 5) and a.dtype == np.int32 and np.array_equal(a, b)
        assert a.min() >= 0 and a.max() < n and all(len(set(r)) == 5 for r in a.tolist())


# ---- 4: the restatement's RANSAC on the committed pairs --------------------------------------------------------------

@pytest.mark.parametrize('name,n', [('roma', 1189), ('camcal', 100)])
def test_restatement_real_pairs(name, n):
    c = real_pair(name)
    assert c['pts'].size == n
    ref = c['ref']
    print('%s (0, 1): %d of %d common points are inliers of the restatement\'s winner (sample %d, %d models)'
          % (name, ref['count'], n, ref['sample'], ref['models']))
    assert ref['count'] == n
    P1, P2, X, fr, sp = rr.camsfrome(ref['e'].reshape(3, 3), hom(c['x1']), hom(c['x2']), -1)
    assert sp[0] > sp[1]
    print('%s: rotation against the report %.3e rad' % (name, rotation_angle(P2[:, :3], report_relative_rotation(name))))


def test_scoring_seed_properties():
    """The scene of the GPU scoring test: the seed gives b <= 2 borderline correspondences under the restatement's winner."""
    c = scoring_case()
    ref = rr.ransac(c['x1'], c['x2'], c['samples'], c['thr2'])
    b = borderline(ref['e'], c['x1'], c['x2'], c['thr2'])
    print('scoring case: restatement count %d of %d (%d true inliers), b = %d' % (ref['count'], 200, int((~c['bad']).sum()), b))
    assert b <= 2 and ref['count'] >= 0.9 * (~c['bad']).sum()
