"""NumPy restatement of the least-squares forward intersection of dbat_hip_pointadjust (csrc/pointadjust.hpp): one object
point from its image rays, damped as Levenberg-Marquardt with Marquardt scaling.  Shares no code with dbat_amd/: the
tests measure the device against it.  Every array is of the dtype asked for (float or np.longdouble), so none of LAPACK
is used: the 3 x 3 system is factored by the scalar Cholesky of pairadjust_ref.

The rules (include/dbat_hip.h has them in full): residuals w (pi(R (X - C)) - xn) with R, C of the ray's camera
P = [R | -R C]; the used rays are chosen once at the start point (use is set and the third row of P [X; 1] is negative);
coordinates are taken relative to the projection centre of the first used ray; lambda starts at 1e-3, /10 (floor 1e-12)
on an accepted trial, x10 on a rejected one; a trial is accepted if its objective is finite and smaller and every used
ray is still in front; the stopping test q <= conv_tol^2 f or f <= 1e-24 * 2 n is made on every trial; codes 0 converged,
1 max_iter, 2 lambda > 1e8, 3 converged but singular, 4 fewer than two rays.

The objective of the accept test is evaluated in pairs of the dtype, and so are the centres -R' t, with the dd_* helpers
of pairadjust_ref, whose docstring has the reason."""
import numpy as np

from pairadjust_ref import FLOOR, LAMBDA0, LAMBDA_MAX, LAMBDA_MIN, chol, chol_solve, dd_add, dd_div, dd_less, dd_mul, dd_neg, dd_sum, two_prod

PIVOT = 1e-10
MIN_RAYS = 2


def centres(R, t):
    """-R' t of every ray (R r x 3 x 3, t r x 3) as a pair of 3 x r arrays."""
    hi, lo = [], []
    for k in range(3):
        s = dd_add(dd_add(two_prod(R[:, 0, k], t[:, 0]), two_prod(R[:, 1, k], t[:, 1])), two_prod(R[:, 2, k], t[:, 2]))
        hi.append(-s[0])
        lo.append(-s[1])
    return np.stack(hi), np.stack(lo)


def objective(xn, w, R, Cr, x):
    """(f as a pair, the depths, the residuals) at the point x; R r x 3 x 3, Cr the pair of the centres (3 x r), both x and
    Cr relative to the origin."""
    z = np.zeros_like(xn[0])
    d = [dd_add((x[k] + z, z), (-Cr[0][k], -Cr[1][k])) for k in range(3)]
    Y = []
    for r in range(3):
        v = dd_mul((R[:, r, 0], z), d[0])
        for c in (1, 2):
            v = dd_add(v, dd_mul((R[:, r, c], z), d[c]))
        Y.append(v)
    sq, res = [], []
    for i in range(2):
        b = dd_add(Y[i], dd_neg(dd_mul(Y[2], (xn[i], z))))
        r = dd_mul(dd_div(b, Y[2]), (w[i], z))
        res.append(r[0])
        sq.append(dd_mul(r, r))
    f = dd_sum((np.concatenate([v[0] for v in sq]), np.concatenate([v[1] for v in sq])))
    return f, Y[2][0], np.stack(res)


def jacobian(xn, w, R, C, x):
    """Residuals (2 x r) and the Jacobian (2 x 3 x r) to X; C 3 x r plain."""
    Y = np.einsum('rij,jr->ir', R, x[:, None] - C)
    r = w * (Y[:2] / Y[2] - xn)
    n = xn.shape[1]
    Pm = np.zeros((2, 3, n), xn.dtype)
    Pm[0, 0] = Pm[1, 1] = 1 / Y[2]
    Pm[0, 2], Pm[1, 2] = -Y[0] / (Y[2] * Y[2]), -Y[1] / (Y[2] * Y[2])
    Pm = w[:, None, :] * Pm
    return r, np.einsum('ijn,njk->ikn', Pm, R)


def adjust(cam, xn, P, X0, use=None, w=None, max_iter=20, conv_tol=1e-6, dtype=float):
    """One point: cam (r camera indices), xn 2 x r, P n_cams x 3 x 4, X0 (3).  dict(X, used, code, iters, trials, n, f0, f,
    sigma0, lam, Q (3 x 3), res (2 x r: of every ray, zero where not finite))."""
    T = np.dtype(dtype).type
    cv = lambda a: np.array(a, dtype)
    cam = np.asarray(cam, int).reshape(-1)
    r_all = cam.size
    xn, X0 = cv(xn).reshape(2, r_all), cv(X0).reshape(3)
    Pr = cv(P).reshape(-1, 3, 4)[cam]
    R, t = Pr[:, :, :3], Pr[:, :, 3]
    w = np.ones((2, r_all), dtype) if w is None else cv(np.broadcast_to(w, (2, r_all)))
    use = np.ones(r_all, bool) if use is None else np.asarray(use, bool)
    with np.errstate(all='ignore'):
        used = use & (R[:, 2] @ X0 + t[:, 2] < 0) if r_all else np.zeros(0, bool)
    n = int(used.sum())
    out = dict(X=X0, used=used, n=n, code=4, iters=0, trials=0, f0=T(np.nan), f=T(np.nan), sigma0=T(np.nan), lam=T(LAMBDA0),
               Q=np.full((3, 3), np.nan, dtype), res=np.zeros((2, r_all), dtype))
    if n < MIN_RAYS:
        return out
    Call = centres(R, t)
    O = Call[0][:, int(np.flatnonzero(used)[0])].copy()
    z = np.zeros_like(Call[0])
    Crel = dd_add(Call, (-O[:, None] + z, z))
    x = X0 - O
    Ru, a, v = R[used], xn[:, used], w[:, used]
    Cu = (Crel[0][:, used], Crel[1][:, used])
    fp = objective(a, v, Ru, Cu, x)[0]
    f = fp[0]
    f0, lam, tol2, floor = f, T(LAMBDA0), T(conv_tol) * T(conv_tol), T(FLOOR) * 2 * n
    iters = trials = 0
    code = None
    while code is None:
        if iters >= max_iter:
            code = 1
            break
        r, J = jacobian(a, v, Ru, Cu[0], x)
        N = np.einsum('ian,ibn->ab', J, J)
        g = np.einsum('ian,in->a', J, r)
        while True:
            trials += 1
            with np.errstate(all='ignore'):
                L, d = chol(N + lam * np.diag(np.diag(N)))
                ok = bool(np.all(d > 0))
                q = T(np.inf)
                if ok:
                    dp = -chol_solve(L, g)
                    ok = bool(np.all(np.isfinite(dp)))
                    q = -(g @ dp)
            if f <= floor or (ok and q <= tol2 * f):
                code = 0
                break
            good = False
            if ok:
                xt = x + dp
                with np.errstate(all='ignore'):
                    fn, zz = objective(a, v, Ru, Cu, xt)[:2]
                    good = bool(np.isfinite(fn[0]) and dd_less(fn, fp) and np.all(zz < 0))
            if good:
                x, fp, f = xt, fn, fn[0]
                lam = max(lam / 10, T(LAMBDA_MIN))
                iters += 1
                break
            lam = lam * 10
            if lam > LAMBDA_MAX:
                code = 2
                break
    # the end: the undamped matrix at the final point and its inverse; the residuals of every ray
    r, J = jacobian(a, v, Ru, Cu[0], x)
    N = np.einsum('ian,ibn->ab', J, J)
    with np.errstate(all='ignore'):
        L, d = chol(N)
        singular = bool(np.any(~(d > PIVOT * np.diag(N))))
        Q = np.full((3, 3), np.nan, dtype)
        if not singular:
            Q = np.stack([chol_solve(L, e) for e in np.eye(3, dtype=dtype)], 1)
            if not np.all(np.isfinite(Q)):
                singular, Q = True, np.full((3, 3), np.nan, dtype)
        res = objective(xn, w, R, Crel, x)[2]
    if code == 0 and singular:
        code = 3
    res = np.where(np.all(np.isfinite(res), 0), res, 0)
    out.update(X=O + x, code=code, iters=iters, trials=trials, f0=f0, f=f, lam=lam, Q=Q, res=res, sigma0=np.sqrt(f / (2 * n - 3)))
    return out


def distance(a, b, stat=True, scale=1.0):
    """The largest difference of two results in X (over scale, the size of the scene) and, where stat, relative in sigma0
    and Q.  (stat is for points with noise and redundancy: the sigma0 of a noise-free point is the rounding of its
    residuals, which no two routes share.)"""
    d = [np.abs(np.asarray(a['X'], np.longdouble) - b['X']).max() / scale]
    if stat:
        d.append(abs(a['sigma0'] / b['sigma0'] - 1))
        d.append(np.abs(a['Q'] - b['Q']).max() / np.abs(b['Q']).max())
    return float(max(d))


# ---- the seeded cases of the tests -----------------------------------------------------------------------------------

RAYS = (2, 3, 7, 8, 9, 16, 17, 65)          # around the 8-lane stride
NOISES = (0.0, 5e-4)
WEIGHT, CONV_TOL, MAX_ITER = 2000.0, 1e-12, 100
N_CAMS = 12


def rodrigues(a):
    from pairadjust_ref import expso3
    return expso3(np.asarray(a, float))


def cameras(seed, n_cams=N_CAMS, shift=None):
    """n_cams cameras on a ring of radius 10 about the origin, 2 above it, looking (along -z) at the origin with a few
    degrees of their own: (P n x 3 x 4 float64, C 3 x n).  shift: the scene translated in the world frame."""
    rng = np.random.default_rng(9000 + seed)
    P, Cs = [], []
    sh = np.zeros(3) if shift is None else np.asarray(shift, float)
    for k in range(n_cams):
        th = 2 * np.pi * (k + rng.uniform(-0.2, 0.2)) / n_cams
        C = np.array([10 * np.cos(th), 10 * np.sin(th), 2.0 + rng.uniform(-1, 1)])
        zc = C / np.linalg.norm(C)                         # the camera's +z points away from the scene
        xc = np.cross([0.0, 0.0, 1.0], zc)
        xc /= np.linalg.norm(xc)
        R = rodrigues(np.deg2rad(3.0) * rng.standard_normal(3)) @ np.stack([xc, np.cross(zc, xc), zc])
        C = C + sh
        t = np.asarray(-(np.asarray(R, np.longdouble) @ np.asarray(C, np.longdouble)), float)
        P.append(np.hstack([R, t[:, None]]))
        Cs.append(C)
    return np.stack(P), np.stack(Cs, 1)


def project(P, cam, X):
    """xn of the point X (3) in the cameras cam, in np.longdouble rounded to float64 once."""
    Pl = np.asarray(P, np.longdouble)[cam]
    Y = Pl[:, :, :3] @ np.asarray(X, np.longdouble) + Pl[:, :, 3]
    return np.asarray((Y[:, :2] / Y[:, 2:3]).T, float), np.asarray(Y[:, 2], float)


def seeded_case(r, noise, seed=0, shift=None):
    """A point within 2 of the origin seen by r rays (camera k mod N_CAMS; from 13 rays on, cameras see it twice) with
    `noise` on every image coordinate, and its start: the truth moved by 0.1 in a random direction."""
    P, C = cameras(seed, shift=shift)
    rng = np.random.default_rng(11000 + 100 * seed + r)
    cam = (np.arange(r) * 5 + int(rng.integers(N_CAMS))) % N_CAMS
    Xt = rng.uniform(-2, 2, 3) + (0 if shift is None else np.asarray(shift, float))
    x, z = project(P, cam, Xt)
    assert np.all(z < 0)
    x = x + noise * rng.standard_normal((2, r))
    dirn = rng.standard_normal(3)
    return dict(cam=cam, x=x, P=P, X=Xt, X0=Xt + 0.1 * dirn / np.linalg.norm(dirn), r=r, noise=noise, shift=shift)


def run_case(c, dtype=float, **kw):
    opt = dict(w=WEIGHT, max_iter=MAX_ITER, conv_tol=CONV_TOL, dtype=dtype)
    opt.update(kw)
    return adjust(c['cam'], c['x'], c['P'], c['X0'], **opt)
