"""Network transforms without a GPU (dbat_hip_rigidalign, dbat_hip_multixform; dbat_amd.rigidalign, multixform,
multialign, transform_network, align_network): a NumPy restatement of misc/rigidalign.m, photogrammetry/pm_multixform.m
and pm_multialign.m in any floating-point type -- the GPU tests measure the device against it in np.longdouble and in
float64 --, its own properties, and everything the library refuses before it touches a device."""
import ctypes as C

import numpy as np
import pytest

import dbat_oracle as o
from dbat_amd import _hip, BadInput
from helpers import synth_struct


# ---- the restatement ----------------------------------------------------------------------------------------------

def rot123(ang, dtype=np.float64):
    """M = R1(omega) R2(phi) R3(kappa) (eulerrotmat.m:81, sequence 123, moving axes) in dtype; pm_eulerrotmat, the
    world-to-camera rotation, is its transpose."""
    a = np.asarray(ang, dtype)
    so, co, sp, cp, sk, ck = np.sin(a[0]), np.cos(a[0]), np.sin(a[1]), np.cos(a[1]), np.sin(a[2]), np.cos(a[2])
    one, zero = dtype(1), dtype(0)
    R1 = np.array([[one, zero, zero], [zero, co, -so], [zero, so, co]], dtype)
    R2 = np.array([[cp, zero, sp], [zero, one, zero], [-sp, zero, cp]], dtype)
    R3 = np.array([[ck, -sk, zero], [sk, ck, zero], [zero, zero, one]], dtype)
    return R1 @ R2 @ R3


def det3(M):
    return (M[0, 0] * (M[1, 1] * M[2, 2] - M[1, 2] * M[2, 1]) - M[0, 1] * (M[1, 0] * M[2, 2] - M[1, 2] * M[2, 0])
            + M[0, 2] * (M[1, 0] * M[2, 1] - M[1, 1] * M[2, 0]))


def svd3(C):
    """P, s, Q with C = P diag(s) Q', s descending, in the type of C: LAPACK for float64, one-sided Jacobi rotations
    for the types LAPACK does not have.  A zero singular value leaves a zero column in P."""
    if C.dtype == np.float64:
        P, s, Qt = np.linalg.svd(C)
        return P, s, Qt.T
    dt = C.dtype.type
    G, V = C.copy(), np.eye(3, dtype=dt)
    for _ in range(60):
        moved = False
        for p in range(2):
            for q in range(p + 1, 3):
                a, b, c = G[:, p] @ G[:, p], G[:, q] @ G[:, q], G[:, p] @ G[:, q]
                if not abs(c) > np.finfo(dt).eps * dt(0.01) * np.sqrt(a * b):
                    continue
                moved = True
                z = (b - a) / (2 * c)
                t = (dt(1) if z >= 0 else dt(-1)) / (abs(z) + np.sqrt(1 + z * z))
                cs = 1 / np.sqrt(1 + t * t)
                sn = cs * t
                for M in (G, V):
                    mp, mq = M[:, p].copy(), M[:, q].copy()
                    M[:, p], M[:, q] = cs * mp - sn * mq, sn * mp + cs * mq
        if not moved:
            break
    s = np.sqrt(np.sum(G * G, 0))
    k = np.argsort(-s, kind='stable')
    s, G, V = s[k], G[:, k], V[:, k]
    P = np.where(s > 0, G / np.where(s > 0, s, dt(1)), dt(0))
    return P, s, V


def ref_rigidalign(X, Y, scale=False, use=None, dtype=np.float64):
    """rigidalign.m:27-61 over the used columns: dict(T, R, d, alpha, rms, resid, xm, ym, sv) in dtype.  resid =
    alpha R x + d - y (NaN in the columns that are not used), rms = sqrt(sum |r|^2 / columns used)."""
    X, Y = np.asarray(X, dtype), np.asarray(Y, dtype)
    use = np.ones(X.shape[1], bool) if use is None else np.asarray(use, bool)
    Xu, Yu = X[:, use], Y[:, use]
    xm, ym = Xu.mean(1), Yu.mean(1)
    A, B = Xu - xm[:, None], Yu - ym[:, None]
    Cm = B @ A.T
    P, s, Q = svd3(Cm)
    if not s[2] > 0:                       # three points, a planar set: the third column of P is free up to its sign,
        P = P.copy()                       # which det(P Q') below takes out again
        P[:, 2] = np.cross(P[:, 0], P[:, 1])
    R = P @ np.diag(np.array([1, 1, det3(P @ Q.T)], dtype)) @ Q.T
    alpha = np.sum(R * Cm) / np.sum(A * A) if scale else dtype(1)       # tr((R A)'B) / tr(A'A)
    d = ym - alpha * (R @ xm)
    T = np.eye(4, dtype=dtype)
    T[:3, :3], T[:3, 3] = alpha * R, d
    r = alpha * (R @ Xu) + d[:, None] - Yu
    resid = np.full(X.shape, np.nan, dtype)
    resid[:, use] = r
    return dict(T=T, R=R, d=d, alpha=alpha, rms=np.sqrt(np.sum(r * r) / Xu.shape[1]), resid=resid, xm=xm, ym=ym, sv=s)


def ref_multixform(EO, OP, T, dtype=np.float64):
    """pm_multixform.m:11-40 with the scale divided out before the angles are taken: (EO, OP, fail, N), fail per camera,
    N[i] the new world-to-camera rotation M' R' of camera i (NaN for a failed one)."""
    EO, OP, T = np.array(EO, dtype), np.array(OP, dtype), np.asarray(T, dtype)
    A, d = T[:3, :3], T[:3, 3]
    alpha = np.cbrt(det3(A))
    R = A / alpha
    if OP.size:
        OP = A @ OP + d[:, None]
    nc = EO.shape[1] if EO.size else 0
    fail, N = np.zeros(nc, bool), np.full((nc, 3, 3), np.nan, dtype)
    for i in range(nc):
        if not np.all(np.isfinite(EO[:6, i])):
            fail[i] = True
            continue
        N[i] = rot123(EO[3:6, i], dtype).T @ R.T
        EO[:3, i] = A @ EO[:3, i] + d
        EO[3:6, i] = [np.arctan2(-N[i][2, 1], N[i][2, 2]), np.arcsin(np.clip(N[i][2, 0], -1, 1)),
                      np.arctan2(-N[i][1, 0], N[i][0, 0])]                  # derotmat3d.m:17-19
    return EO, OP, fail, N


def ref_multialign(EO, OP, i, ra=0.0, dtype=np.float64):
    """pm_multialign.m:19-24: (EO, OP, T)."""
    EO = np.asarray(EO, dtype)
    M = rot123(EO[3:6, i], dtype).T
    RA = rot123([0, 0, -ra], dtype).T
    T = np.eye(4, dtype=dtype)
    T[:3, :3] = RA.T @ M
    T[:3, 3] = -T[:3, :3] @ EO[:3, i]
    EO2, OP2, _, _ = ref_multixform(EO, OP, T, dtype)
    return EO2, OP2, T


def random_rotation(rng):
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return Q * np.sign(np.linalg.det(Q))


def similarity(R, alpha, d):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = alpha * R, d
    return T


# ---- properties of the restatement --------------------------------------------------------------------------------

@pytest.mark.parametrize('n', [3, 4, 257])
@pytest.mark.parametrize('dtype', [np.float64, np.longdouble])
def test_restatement_recovers_a_known_similarity(n, dtype):
    rng = np.random.default_rng(n)
    R, alpha, d = random_rotation(rng), 1.7, np.array([10.0, -20.0, 5.0])
    X = rng.normal(0, 10, (3, n))
    Y = alpha * R @ X + d[:, None]
    a = ref_rigidalign(X, Y, True, dtype=dtype)
    assert a['T'].dtype == dtype
    assert np.abs(a['R'] - R).max() < 1e-13 and abs(a['alpha'] - alpha) < 1e-13
    assert np.abs(a['d'] - d).max() < 1e-11 and a['rms'] < 1e-12
    b = ref_rigidalign(X, R @ X + d[:, None], False, dtype=dtype)
    assert b['alpha'] == 1 and np.abs(b['R'] - R).max() < 1e-13 and np.abs(b['d'] - d).max() < 1e-11


@pytest.mark.parametrize('dtype', [np.float64, np.longdouble])
def test_restatement_gives_a_proper_rotation_for_a_mirrored_set(dtype):
    rng = np.random.default_rng(2)
    X = rng.normal(0, 10, (3, 40))
    Y = np.diag([1.0, 1.0, -1.0]) @ random_rotation(rng) @ X + 3.0
    a = ref_rigidalign(X, Y, True, dtype=dtype)
    assert abs(det3(a['R']) - 1) < 1e-13 and np.abs(a['R'] @ a['R'].T - np.eye(3)).max() < 1e-13
    assert a['rms'] > 1.0                      # no rotation takes a set onto its mirror image


def test_restatement_angles_reproduce_the_rotation():
    """eulerrotmat of the angles that pm_multixform returns is M' R' -- for every scale, because the scale is divided
    out before the angles are taken."""
    rng = np.random.default_rng(3)
    EO = np.vstack([rng.normal(0, 5, (3, 30)), rng.uniform(-3, 3, (1, 30)), rng.uniform(-1.5, 1.5, (1, 30)),
                    rng.uniform(-3, 3, (1, 30))])
    for alpha in (1.0, 0.5, 1.7):
        R = random_rotation(rng)
        EO2, _, fail, N = ref_multixform(EO, np.zeros((3, 0)), similarity(R, alpha, [1.0, 2.0, 3.0]))
        assert not fail.any()
        for i in range(30):
            assert np.abs(N[i] - o.eulerrotmat(EO[3:6, i]).T @ R.T).max() < 1e-14
            assert np.abs(o.eulerrotmat(EO2[3:6, i]).T - N[i]).max() < 1e-12
            assert np.abs(EO2[:3, i] - (alpha * R @ EO[:3, i] + [1.0, 2.0, 3.0])).max() < 1e-12


def test_restatement_multialign_puts_the_camera_at_the_origin():
    rng = np.random.default_rng(4)
    EO = np.vstack([rng.normal(0, 5, (3, 6)), rng.uniform(-1.5, 1.5, (3, 6))])
    for ra in (0.0, np.pi / 2):
        EO2, _, T = ref_multialign(EO, np.zeros((3, 0)), 2, ra)
        assert np.abs(EO2[:, 2] - [0, 0, 0, 0, 0, -ra]).max() < 1e-12
        assert abs(np.linalg.det(T[:3, :3]) - 1) < 1e-13


# ---- the library without a device ---------------------------------------------------------------------------------

def no_gpu():
    import torch
    return not torch.cuda.is_available()


def rc_rigidalign(X, Y, use=None, scale=1):
    lib = _hip.load()
    X, Y = np.asfortranarray(X, float), np.asfortranarray(Y, float)
    n = X.shape[1]
    u = None if use is None else np.ascontiguousarray(use, bool).view(np.uint8)
    T, st = np.zeros(16), np.zeros(4)
    return lib.dbat_hip_rigidalign(0, n, _hip.dptr(X.reshape(-1, order='F')), _hip.dptr(Y.reshape(-1, order='F')),
                                   None if u is None else u.ctypes.data_as(C.POINTER(C.c_uint8)), scale,
                                   _hip.dptr(T), _hip.dptr(st), None)


def rc_multixform(T, rows=6, nc=2, npnt=3):
    lib = _hip.load()
    T = np.asfortranarray(T, float)
    EO, OP = np.zeros(rows * nc), np.zeros(3 * npnt)
    return lib.dbat_hip_multixform(0, _hip.dptr(T.reshape(-1, order='F')), nc, rows, _hip.dptr(EO), npnt, _hip.dptr(OP), None)


def test_symbols_exist():
    lib = _hip.load()
    for name in ('dbat_hip_rigidalign', 'dbat_hip_multixform'):
        assert name in _hip.SYMBOLS and hasattr(lib, name)
    assert _hip.ABI_VERSION == 5 and lib.dbat_hip_abi_version() == 5


def test_rigidalign_refuses_bad_input_before_any_device_call():
    rng = np.random.default_rng(5)
    X = rng.normal(0, 10, (3, 12))
    Y = 1.3 * random_rotation(rng) @ X + 4.0
    accepted = (_hip.EDEVICE,) if no_gpu() else (_hip.OK,)
    assert rc_rigidalign(X, Y) in accepted
    for n in (0, 1, 2):                                        # fewer than three columns
        assert rc_rigidalign(X[:, :n], Y[:, :n]) == _hip.EINVAL
        assert 'fewer than three' in _hip.last_error()
    use = np.zeros(12, bool)
    use[[1, 7]] = True                                         # ... than three USED columns
    assert rc_rigidalign(X, Y, use) == _hip.EINVAL
    for bad in (np.nan, np.inf):                               # a used column that is not finite
        for A, B in ((X.copy(), Y), (X, Y.copy())):
            (A if A is not X else B)[1, 5] = bad
            assert rc_rigidalign(A, B) == _hip.EINVAL and 'not finite' in _hip.last_error()
            use = np.ones(12, bool)
            use[5] = False                                     # the same column, not used: accepted
            assert rc_rigidalign(A, B, use) in accepted
    t = np.arange(12.0) - 6                                    # collinear points (whole numbers: exactly so), here
    for off in (0.0, 1e6):                                     # and at 1e6 m
        L = off + np.outer([1.0, 2.0, -3.0], t)
        assert rc_rigidalign(L, Y) == _hip.EINVAL and 'collinear' in _hip.last_error()
        assert rc_rigidalign(X, L) == _hip.EINVAL
    assert rc_rigidalign(np.ones((3, 12)), Y) == _hip.EINVAL   # coincident points
    assert rc_rigidalign(X + 1e6, Y + 2e6) in accepted         # well spread at 1e6 m: accepted


def test_multixform_refuses_bad_input_before_any_device_call():
    rng = np.random.default_rng(6)
    good = similarity(random_rotation(rng), 1.7, [1e3, -2e3, 5e2])
    accepted = (_hip.EDEVICE,) if no_gpu() else (_hip.OK,)
    assert rc_multixform(good) in accepted and rc_multixform(good, rows=7) in accepted
    assert rc_multixform(good, rows=5) == _hip.EINVAL
    for r, c, v in ((3, 0, 1e-3), (3, 3, 2.0), (3, 3, 0.0)):   # the last row is not [0 0 0 1]
        T = good.copy()
        T[r, c] = v
        assert rc_multixform(T) == _hip.EINVAL and 'last row' in _hip.last_error()
    for v in (np.nan, np.inf):                                 # not finite
        for r, c in ((0, 0), (1, 3), (3, 3)):
            T = good.copy()
            T[r, c] = v
            assert rc_multixform(T) == _hip.EINVAL and 'finite' in _hip.last_error()
    shear = good.copy()
    shear[:3, :3] = shear[:3, :3] @ np.array([[1, 1e-6, 0], [0, 1, 0], [0, 0, 1.0]])
    aniso = good.copy()
    aniso[:3, :3] = aniso[:3, :3] @ np.diag([1, 1, 1 + 1e-6])
    mirror = good.copy()
    mirror[:3, :3] = mirror[:3, :3] @ np.diag([1, 1, -1.0])
    zero = good.copy()
    zero[:3, :3] = 0
    for T in (shear, aniso, mirror, zero):                     # A is not alpha times a proper rotation
        assert rc_multixform(T) == _hip.EINVAL and 'rotation' in _hip.last_error()
    near = good.copy()                                         # ... but within 1e-9 it is
    near[:3, :3] = near[:3, :3] @ np.array([[1, 1e-11, 0], [0, 1, 0], [0, 0, 1.0]])
    assert rc_multixform(near) in accepted


def test_python_functions_raise_badinput():
    import dbat_amd
    rng = np.random.default_rng(7)
    X = rng.normal(0, 10, (3, 8))
    with pytest.raises(BadInput):
        dbat_amd.rigidalign(X[:, :2], X[:, :2])
    with pytest.raises(BadInput):
        dbat_amd.rigidalign(np.outer([1.0, 1, 1], np.arange(8.0)), X, True)
    with pytest.raises(BadInput):
        dbat_amd.multixform(np.zeros((6, 1)), X, np.diag([1.0, 1, -1, 1]))
    with pytest.raises(BadInput):
        dbat_amd.multixform(np.zeros((5, 1)), X, np.eye(4))
    with pytest.raises(BadInput):
        dbat_amd.multialign(np.zeros((6, 2)), X, 2)
    for bad in (lambda: dbat_amd.rigidalign(X[:2], X[:2]), lambda: dbat_amd.rigidalign(X, X[:, :5]),
                lambda: dbat_amd.rigidalign(X, X, use=np.ones(3, bool)), lambda: dbat_amd.multixform(np.zeros((6, 1)), X, np.eye(3)),
                lambda: dbat_amd.multixform(np.zeros((6, 1)), X[:2], np.eye(4))):       # wrong shapes: the same error
        with pytest.raises(BadInput):
            bad()
    s, _ = synth_struct('tiny')
    with pytest.raises(BadInput):
        dbat_amd.align_network(s, np.full((3, 5), np.nan))
    with pytest.raises(BadInput):
        dbat_amd.align_network(s, np.full(s.OP.val.shape, np.nan))       # no column has a reference


def isotropic_priors_struct():
    """synth_struct('tiny', 'priors') with the standard deviations of its object-point priors made equal within every
    column (the variant has 0.01, 0.01, 0.02 m): a struct that a rotation can be applied to."""
    s = synth_struct('tiny', 'priors')[0]
    s.prior.OP.std[:, s.prior.OP.use.all(0)] = 0.01
    return s


def test_transform_network_refuses_priors_that_a_rotation_changes():
    from dbat_amd import transform_network
    rng = np.random.default_rng(8)
    rot = similarity(random_rotation(rng), 1.7, [1e3, -2e3, 5e2])
    s = isotropic_priors_struct()
    k = int(np.flatnonzero(s.prior.OP.use.all(0))[0])
    a = isotropic_priors_struct()                              # anisotropic standard deviations in a used column
    a.prior.OP.std[2, k] *= 2
    with pytest.raises(BadInput, match='anisotropic'):
        transform_network(a, rot)
    a2 = isotropic_priors_struct()                             # ... of a camera position
    a2.prior.EO.std[1, 0] *= 2
    assert a2.prior.EO.use[:3, 0].all()
    with pytest.raises(BadInput, match='anisotropic'):
        transform_network(a2, rot)
    b = isotropic_priors_struct()                              # ... and a column of which only a part is used
    b.prior.OP.use[0, k] = False
    with pytest.raises(BadInput, match='anisotropic'):
        transform_network(b, rot)
    c = isotropic_priors_struct()                              # an angle prior in use
    c.prior.EO.use[4, 0], c.prior.EO.val[4, 0], c.prior.EO.std[4, 0] = True, 0.1, 0.01
    with pytest.raises(BadInput, match='angle'):
        transform_network(c, rot)
    with pytest.raises(BadInput):                              # not a similarity
        transform_network(s, np.diag([1.0, 1.0, -1.0, 1.0]))
    if no_gpu():                                               # what is accepted gets as far as the device: the
        cases = [(s, rot)] + [(t, similarity(np.eye(3), 1.7, [1e3, -2e3, 5e2])) for t in (a, a2, b, c)]
        for t, T in cases:                                     # isotropic priors under a rotation, all without one
            with pytest.raises(_hip.DbatHipError) as e:
                transform_network(t, T)
            assert e.value.code == _hip.EDEVICE
