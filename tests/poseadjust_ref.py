"""NumPy restatement of the least-squares space resection of dbat_hip_poseadjust (csrc/poseadjust.hpp): the pose of one
camera from its control points, damped as Levenberg-Marquardt with Marquardt scaling.  Shares no code with dbat_amd/:
the tests measure the device against it.  Every array is of the dtype asked for (float or np.longdouble), so none of
LAPACK is used: the 6 x 6 system is factored by the scalar Cholesky of pairadjust_ref.

The rules (include/dbat_hip.h has them in full): residuals w (pi(R (X - C)) - xn); updates C <- C + c,
R <- exp([a]x) R; the used points are chosen once at the start pose (use is set and the third row of P [X; 1] is
negative); coordinates are taken relative to the first used point; lambda starts at 1e-3, /10 (floor 1e-12) on an
accepted trial, x10 on a rejected one; a trial is accepted if its objective is finite and smaller and every used point
is still in front; the stopping test q <= conv_tol^2 f or f <= 1e-24 * 2 n is made on every trial; codes 0 converged,
1 max_iter, 2 lambda > 1e8, 3 converged but singular, 4 fewer than three.

The objective of the accept test is evaluated in pairs of the dtype and R is such a pair kept orthonormal to the pair's
precision, with the dd_* helpers of pairadjust_ref, whose docstring has the reason."""
import numpy as np

from pairadjust_ref import (FLOOR, LAMBDA0, LAMBDA_MAX, LAMBDA_MIN, chol, chol_solve, dd_add, dd_div, dd_less, dd_matmul, dd_mul,
                            dd_neg, dd_sum, expso3, orthonormalise)

PIVOT = 1e-10
MIN_POINTS = 3


def objective(xn, w, R, C, Xr):
    """(f as a pair, the depths) at the pair R, the centre C and the points Xr (both relative to the origin)."""
    z = np.zeros_like(Xr[0])
    d = [dd_add((Xr[k], z), (-C[k] + z, z)) for k in range(3)]
    Y = []
    for r in range(3):
        v = dd_mul((R[0][r, 0] + z, R[1][r, 0] + z), d[0])
        for c in (1, 2):
            v = dd_add(v, dd_mul((R[0][r, c] + z, R[1][r, c] + z), d[c]))
        Y.append(v)
    sq, res = [], []
    for i in range(2):
        b = dd_add(Y[i], dd_neg(dd_mul(Y[2], (xn[i], z))))
        r = dd_mul(dd_div(b, Y[2]), (w[i], z))
        res.append(r[0])
        sq.append(dd_mul(r, r))
    f = dd_sum((np.concatenate([v[0] for v in sq]), np.concatenate([v[1] for v in sq])))
    return f, Y[2][0], np.stack(res)


def jacobian(xn, w, R, C, Xr):
    """Residuals (2 x n) and the Jacobian (2 x 6 x n) to (c, a)."""
    n = Xr.shape[1]
    Y = R @ (Xr - C[:, None])
    r = w * (Y[:2] / Y[2] - xn)
    Pm = np.zeros((2, 3, n), Xr.dtype)
    Pm[0, 0] = Pm[1, 1] = 1 / Y[2]
    Pm[0, 2], Pm[1, 2] = -Y[0] / (Y[2] * Y[2]), -Y[1] / (Y[2] * Y[2])
    Pm = w[:, None, :] * Pm
    M = np.zeros((3, 6, n), Xr.dtype)
    M[:, :3] = -R[:, :, None]
    for j in range(3):                                   # d(a x Y) / da_j = e_j x Y
        e = np.zeros(3, Xr.dtype)
        e[j] = 1
        M[:, 3 + j] = np.cross(e[:, None], Y, axis=0)
    return r, np.einsum('ijn,jkn->ikn', Pm, M)


def adjust(X, xn, P, use=None, w=None, max_iter=20, conv_tol=1e-6, dtype=float):
    """One camera.  dict(R, C (in the frame of X), P (3 x 4, [R | -R C]), used, code, iters, trials, n, f0, f, sigma0, lam,
    Q (6 x 6), res (2 x n_all: of every point, zero where not finite))."""
    T = np.dtype(dtype).type
    cv = lambda a: np.array(a, dtype)
    n_all = np.asarray(X).shape[1]
    X, xn, P = cv(X), cv(xn), cv(P)
    w = np.ones((2, n_all), dtype) if w is None else cv(np.broadcast_to(w, (2, n_all)))
    use = np.ones(n_all, bool) if use is None else np.asarray(use, bool)
    R, t = P[:, :3], P[:, 3]
    with np.errstate(all='ignore'):
        used = use & (R[2] @ X + t[2] < 0)
    n = int(used.sum())
    out = dict(R=R, C=-R.T @ t, P=P, used=used, n=n, code=4, iters=0, trials=0, f0=T(np.nan), f=T(np.nan), sigma0=T(np.nan),
               lam=T(LAMBDA0), Q=np.full((6, 6), np.nan, dtype), res=np.zeros((2, n_all), dtype))
    if n < MIN_POINTS:
        return out
    O = X[:, int(np.flatnonzero(used)[0])].copy()
    C = -R.T @ t - O
    Xr, a, v = X[:, used] - O[:, None], xn[:, used], w[:, used]
    Rp = orthonormalise((R, np.zeros_like(R)))
    R = Rp[0]
    fp = objective(a, v, Rp, C, Xr)[0]
    f = fp[0]
    f0, lam, tol2, floor = f, T(LAMBDA0), T(conv_tol) * T(conv_tol), T(FLOOR) * 2 * n
    iters = trials = 0
    code = None
    while code is None:
        if iters >= max_iter:
            code = 1
            break
        r, J = jacobian(a, v, R, C, Xr)
        N = np.einsum('ian,ibn->ab', J, J)
        g = np.einsum('ian,in->a', J, r)
        while True:
            trials += 1
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
                E = expso3(dp[3:])
                Rn = orthonormalise(dd_matmul((E, np.zeros_like(E)), Rp))
                Cn = C + dp[:3]
                with np.errstate(all='ignore'):
                    fn, z = objective(a, v, Rn, Cn, Xr)[:2]
                    good = bool(np.isfinite(fn[0]) and dd_less(fn, fp) and np.all(z < 0))
            if good:
                Rp, R, C, fp, f = Rn, Rn[0], Cn, fn, fn[0]
                lam = max(lam / 10, T(LAMBDA_MIN))
                iters += 1
                break
            lam = lam * 10
            if lam > LAMBDA_MAX:
                code = 2
                break
    # the end: the undamped matrix at the final point and its inverse; the residuals of every point
    r, J = jacobian(a, v, R, C, Xr)
    N = np.einsum('ian,ibn->ab', J, J)
    L, d = chol(N)
    singular = bool(np.any(~(d > PIVOT * np.diag(N))))
    Q = np.full((6, 6), np.nan, dtype)
    if not singular:
        Q = np.stack([chol_solve(L, e) for e in np.eye(6, dtype=dtype)], 1)
        if not np.all(np.isfinite(Q)):
            singular, Q = True, np.full((6, 6), np.nan, dtype)
    if code == 0 and singular:
        code = 3
    with np.errstate(all='ignore'):
        res = objective(xn, w, Rp, C, X - O[:, None])[2]
    res = np.where(np.all(np.isfinite(res), 0), res, 0)
    Cw = C + O
    out.update(R=R, C=Cw, P=np.hstack([R, -(R @ O + R @ C)[:, None]]), code=code, iters=iters, trials=trials, f0=f0, f=f, lam=lam, Q=Q, res=res,
               sigma0=np.sqrt(f / (2 * n - 6)) if n > 3 else T(np.nan))
    return out


def centre_of(P):
    """-R' t of a 3 x 4 matrix, in np.longdouble."""
    P = np.asarray(P, np.longdouble)
    return -(P[:, :3].T @ P[:, 3])


def distance(a, b, stat=True, shift=None):
    """The largest difference of two results in R and C and, where stat, relative in sigma0 and Q.  What a float64 route
    returns is its P = [R | -R C], so its centre is taken from that; b, the np.longdouble restatement, has its own.
    shift: a translation of the world frame that b does not have, taken off a's centre.  (stat is for cameras with noise
    and redundancy: the sigma0 of a noise-free camera is the rounding of its residuals, which no two routes share, and
    that of three points is NaN.)"""
    Ca = centre_of(a['P'])
    if shift is not None:
        Ca = Ca - np.asarray(shift, np.longdouble)
    d = [np.abs(np.asarray(a['P'], np.longdouble)[:, :3] - b['R']).max(), np.abs(Ca - b['C']).max()]
    if stat:
        d.append(abs(a['sigma0'] / b['sigma0'] - 1))
        d.append(np.abs(a['Q'] - b['Q']).max() / np.abs(b['Q']).max())
    return float(max(d))


# ---- the seeded cases of the tests -----------------------------------------------------------------------------------

SIZES = (3, 4, 5, 63, 64, 65, 129, 257)
NOISES = (0.0, 5e-4)
WEIGHT, CONV_TOL, MAX_ITER = 2000.0, 1e-12, 100


def rodrigues(a):
    return expso3(np.asarray(a, float))


def seeded_case(n, noise, shift=None):
    """The camera of resect_ref.seeded_case(n, npt=n) with `noise` on every image point, and from
    np.random.default_rng(7000 + n) its start: the true pose turned by 2 degrees about a random axis and moved by 1 % of
    its distance to the centroid of the points.  shift: the same scene translated (exactly) in the world frame."""
    import resect_ref as rf
    c = rf.seeded_case(n, npt=n, shift=shift)
    rng = np.random.default_rng(7000 + n)
    x = np.asarray(c['xl'], float) + noise * rng.standard_normal((2, n))
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    R0 = rodrigues(np.deg2rad(2.0) * axis) @ np.asarray(c['R'], float)
    Cf = np.asarray(c['C'], float)
    dirn = rng.standard_normal(3)
    C0 = Cf + 0.01 * np.linalg.norm(Cf - c['X'].mean(1)) * dirn / np.linalg.norm(dirn)
    # -R0 C0 in np.longdouble, rounded once: the start of the shifted scene is then the start of the scene itself
    t0 = np.asarray(-(np.asarray(R0, np.longdouble) @ np.asarray(C0, np.longdouble)), float)
    return dict(X=c['X'], x=x, R=c['R'], C=c['C'], n=n, noise=noise, P0=np.hstack([R0, t0[:, None]]), shift=shift)


def run_case(c, dtype=float, **kw):
    opt = dict(w=WEIGHT, max_iter=MAX_ITER, conv_tol=CONV_TOL, dtype=dtype)
    opt.update(kw)
    return adjust(c['X'], c['x'], c['P0'], **opt)
