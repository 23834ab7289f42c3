"""The chirality veto and point_depths() without a GPU: the argument parser, the argument checks that come before any
device work, and the reference value of every depth test -- a NumPy restatement of photogrammetry/pm_multidepth.m with
ptdepth.m (camera matrices P = K R [I, -C], d = -sign(det M) x_3 / X_4 / ||M_(3,:)||), which shares no algebra with the
kernel's d = -R_(3,:) (X - C)."""
import copy

import numpy as np
import pytest

from helpers import synth_struct


def rotmat2d(axis, phi):
    """cammodel/rotmat.m:54-78."""
    R = np.array([[np.cos(phi), -np.sin(phi)], [np.sin(phi), np.cos(phi)]])
    M = np.eye(3)
    ix = {1: [1, 2], 2: [0, 2], 3: [0, 1]}[axis]
    M[np.ix_(ix, ix)] = R
    return M


def rotmat(ang):
    """cammodel/rotmat.m:24-28, sequence 'xyz': world to camera."""
    return rotmat2d(3, -ang[2]) @ rotmat2d(2, ang[1]) @ rotmat2d(1, -ang[0])


def ptdepth(P, X):
    """photogrammetry/ptdepth.m:10-14."""
    X = np.vstack([X, np.ones((1, X.shape[1]))])
    x = P @ X
    M = P[:, :3]
    return np.sign(np.linalg.det(M)) * x[2] / X[3] / np.linalg.norm(M[2])


def ref_depths(s, IO=None, EO=None, OP=None):
    """pm_multidepth.m:19-37 over the IP columns of s (instead of the dense visibility table): the depth of the point of
    every IP column with respect to its camera, positive in front.  IO row 0 is the camera constant, rows 1:3 the
    principal point (pm_multidepth's own IO puts the principal point first)."""
    IO = s.IO.val if IO is None else IO
    EO = s.EO.val if EO is None else EO
    OP = s.OP.val if OP is None else OP
    cam, pt = np.asarray(s.IP.cam), np.asarray(s.IP.pt)
    d = np.full(len(cam), np.nan)
    for i in np.unique(cam):
        K = np.array([[-IO[0, i], 0, IO[1, i]], [0, -IO[0, i], IO[2, i]], [0, 0, 1.0]])
        P = K @ rotmat(EO[3:6, i]) @ np.hstack([np.eye(3), -EO[0:3, i:i + 1]])
        j = cam == i
        d[j] = -ptdepth(P, OP[:, pt[j]])
    return d


def simple_depths(s):
    """d_k = -R_(3,:) (X - C): what the kernel evaluates (with the rotation of the camera model)."""
    import dbat_oracle as o
    cam, pt = np.asarray(s.IP.cam), np.asarray(s.IP.pt)
    d = np.empty(len(cam))
    for k in range(len(cam)):
        M = o.eulerrotmat(s.EO.val[3:6, cam[k]])
        d[k] = -(M.T @ (s.OP.val[:, pt[k]] - s.EO.val[0:3, cam[k]]))[2]
    return d


# the first seed of the recipe below whose start has five observations behind a camera (seeds 0 .. 254 give four at most)
BEHIND_SEED = 255


def near_start(s, seed, sigma=0.0):
    """Eight estimated points of `tiny` (default_rng(seed).choice) pulled to C + 0.05 (X - C) + N(0, sigma) of the first
    camera that sees each: close in front of it, where the first steps of a loop throw some of them behind a camera.
    Returns a copy of s."""
    s = copy.deepcopy(s)
    rng = np.random.default_rng(seed)
    est = np.flatnonzero(np.asarray(s.bundle.est.OP, bool).all(0))
    for p in rng.choice(est, 8, replace=False):
        c = np.asarray(s.IP.cam)[np.flatnonzero(np.asarray(s.IP.pt) == p)[0]]
        C = s.EO.val[0:3, c]
        s.OP.val[:, p] = C + 0.05 * (s.OP.val[:, p] - C) + (rng.normal(0, sigma, 3) if sigma else 0.0)
    return s


def behind_start(s):
    """The start of the tests of points behind a camera: near_start with N(0, 0.5) added, which puts five observations
    behind their cameras (smallest depth -0.467)."""
    return near_start(s, BEHIND_SEED, 0.5)


def shrink_start(s, seed):
    """A bad start whose first steps overshoot: every estimated point shrunk to c + 0.3 (X - c) about the centroid c of
    OP.val, default_rng(seed).normal(0, 6, (3, nImages)) added to the estimated camera positions.  A copy of s."""
    s = copy.deepcopy(s)
    N = np.random.default_rng(seed).normal(0, 6, (3, s.EO.val.shape[1]))
    c = s.OP.val.mean(1, keepdims=True)
    est = np.asarray(s.bundle.est.OP, bool).all(0)
    s.OP.val[:, est] = c + 0.3 * (s.OP.val[:, est] - c)
    s.EO.val[0:3] += N * np.asarray(s.bundle.est.EO, bool)[0:3]
    return s


def test_logical_argument_is_the_veto_flag():
    from dbat_amd.driver import _parse_args
    assert _parse_args((True,))['veto'] is True
    assert _parse_args((False,))['veto'] is False and _parse_args(())['veto'] is False
    assert _parse_args(('lm', 40, np.bool_(True)))['veto'] is True


def test_restatement_agrees_with_the_simplified_formula():
    s = synth_struct('tiny')[0]
    d, ds = ref_depths(s), simple_depths(s)
    assert len(d) == 1800 and np.all(d > 0)
    assert np.max(np.abs(d - ds) / np.abs(d)) < 1e-13


def test_behind_start_is_the_recorded_one():
    s = behind_start(synth_struct('tiny')[0])
    d = ref_depths(s)
    assert np.count_nonzero(d <= 0) == 5 and abs(d.min() + 0.467) < 5e-4
    assert np.min(np.abs(d)) > 1e-9


def test_bad_arguments_raise_before_any_device_work(monkeypatch):
    from dbat_amd import bundle, BadInput, _hip

    def no_device(*a, **k):
        raise AssertionError('device work before the argument check')
    monkeypatch.setattr(_hip, 'acquire', no_device)
    monkeypatch.setattr(_hip, 'Handle', no_device)
    s = synth_struct('tiny')[0]
    with pytest.raises(BadInput, match='robust'):
        bundle(s, True, robust='huber')
    for bad in (np.nan, np.inf, -np.inf, 'x', None, True):
        with pytest.raises(BadInput, match='min_depth'):
            bundle(s, True, min_depth=bad)
    with pytest.raises(BadInput, match='min_depth'):
        bundle(s, min_depth=np.nan)                      # (checked whether or not the flag is set)
    with pytest.raises(BadInput, match='one-rank'):
        bundle(s, True, comm=type('Comm', (), dict(rank=0, world_size=2))())


def test_abi_declares_the_three_calls():
    from dbat_amd import _hip
    lib = _hip.load()
    for name in ('dbat_hip_point_depths', 'dbat_hip_set_chirality', 'dbat_hip_chirality_stats'):
        assert name in _hip.SYMBOLS and hasattr(lib, name)
    assert _hip.ABI_VERSION == 5 and lib.dbat_hip_abi_version() == 5



def oracle_unpack(s):
    """x -> (IO, EO, OP) with the oracle's own index structures (what its vetoFun is handed is the vector x)."""
    import dbat_oracle as o
    sb = copy.deepcopy(s)
    for nm in ('IO', 'EO', 'OP'):
        pr = getattr(sb.prior, nm)
        pr.use = np.asarray(pr.use, bool) & np.asarray(getattr(sb.bundle.est, nm), bool)
    sb = o.buildserialindices(sb)
    return lambda x: o.deserialize(sb, x)


def oracle_veto(s, log=None):
    """vetoFun for the oracle: any(depth <= 0) by the restatement; log collects (n_behind, depth closest to zero)."""
    unpack = oracle_unpack(s)

    def f(x):
        IO, EO, OP = unpack(np.asarray(x, float))
        d = ref_depths(s, IO, EO, OP)
        if log is not None:
            log.append((int(np.count_nonzero(~(d > 0))), float(d[np.argmin(np.abs(d))])))
        return bool(np.any(~(d > 0)))
    return f
