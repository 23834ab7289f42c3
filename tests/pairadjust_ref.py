"""NumPy restatement of the least-squares relative orientation of dbat_hip_pairadjust (csrc/pairadjust.hpp): the
two-view bundle adjustment in the gauge of camsfrome (camera 1 [I | 0], |t| = 1), damped as Levenberg-Marquardt with
Marquardt scaling and solved by Schur elimination of the points.  Shares no code with dbat_amd/: the tests measure the
device against it.  Every array is of the dtype asked for (float or np.longdouble), so none of LAPACK is used: the
3 x 3 point blocks are factored by a vectorised Cholesky, the 5 x 5 reduced system by a scalar one.

The rules (include/dbat_hip.h has them in full): residuals w1 (pi(X) - x1), w2 (pi(R X + t) - x2); updates
R <- exp([a]x) R, t <- (t + B b) / |t + B b| with B = basis(t), X <- X + d; lambda starts at 1e-3, /10 (floor 1e-12)
on an accepted trial, x10 on a rejected one; a trial is accepted if its objective is finite and smaller and every used
point is in front of both cameras; the stopping test q <= conv_tol^2 f or f <= 1e-24 * 4 n is made on every
trial; codes 0 converged, 1 max_iter, 2 lambda > 1e8, 3 converged but singular, 4 fewer than five.

The objective of the accept test is evaluated in pairs of the dtype (error-free sums and products, Dekker's splitting),
and R is such a pair kept orthonormal to the pair's precision: near the optimum a step's decrease is far below the
rounding of a plain evaluation, an accept test that answers at random stops the iteration short of the optimum, and
then two precisions that share a path stop at the same iterate and agree with each other far better than either is
right (n = 65 with noise: float64 and np.longdouble 3.9e-13 apart, both 1.05e-9 from where an accept test in 60 digits
ends).  The linear algebra is plain arithmetic of the dtype."""
import numpy as np

LAMBDA0, LAMBDA_MIN, LAMBDA_MAX = 1e-3, 1e-12, 1e8
FLOOR = 1e-24
V_PIVOT, S_PIVOT = 1e-12, 1e-10


# ---- arithmetic on pairs (hi, lo) of arrays of one dtype -------------------------------------------------------------

def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = a.dtype.type(2 ** ((np.finfo(a.dtype).nmant + 2) // 2) + 1) * a         # 2^27 + 1 for float64, 2^32 + 1 for 64 bits
    hi = c - (c - a)
    return hi, a - hi


def two_prod(a, b):
    a, b = np.asarray(a), np.asarray(b)
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def dd_add(x, y):
    s, e = two_sum(x[0], y[0])
    e = e + (x[1] + y[1])
    h = s + e
    return h, e - (h - s)


def dd_mul(x, y):
    p, e = two_prod(x[0], y[0])
    e = e + (x[0] * y[1] + x[1] * y[0])
    h = p + e
    return h, e - (h - p)


def dd_neg(x):
    return -x[0], -x[1]


def dd_div(x, y):
    q1 = x[0] / y[0]
    r = dd_add(x, dd_neg(dd_mul(y, (q1, np.zeros_like(q1)))))
    return two_sum(q1, r[0] / y[0])


def dd_sum(x):
    """Sum of a pair of one-dimensional arrays, by halves."""
    h, l = x
    while h.shape[0] > 1:
        if h.shape[0] % 2:
            h, l = np.append(h, h.dtype.type(0)), np.append(l, l.dtype.type(0))
        m = h.shape[0] // 2
        h, l = dd_add((h[:m], l[:m]), (h[m:], l[m:]))
    return h[0], l[0]


def dd_less(x, y):
    return bool(x[0] < y[0] or (x[0] == y[0] and x[1] < y[1]))


def dd_matmul(A, B):
    """Product of two 3 x 3 matrices of pairs."""
    H, L = np.zeros_like(A[0]), np.zeros_like(A[0])
    for i in range(3):
        for j in range(3):
            v = (A[0].dtype.type(0), A[0].dtype.type(0))
            for k in range(3):
                v = dd_add(v, dd_mul((A[0][i, k], A[1][i, k]), (B[0][k, j], B[1][k, j])))
            H[i, j], L[i, j] = v
    return H, L


def orthonormalise(R):
    """R (3 I - R'R) / 2 on a pair: one Newton step towards the nearest rotation."""
    G = dd_matmul((R[0].T, R[1].T), R)
    I3 = np.eye(3, dtype=R[0].dtype)
    M = dd_add((3 * I3, 0 * I3), dd_neg(G))
    return dd_matmul(R, (M[0] / 2, M[1] / 2))


def objective(x1, x2, w1, w2, R, t, X):
    """(f as a pair, the depths in image 2) at the pair R."""
    z = np.zeros_like(X[0])
    Y = []
    for r in range(3):
        v = (t[r] + z, z)
        for c in range(3):
            v = dd_add(v, dd_mul((R[0][r, c] + z, R[1][r, c] + z), (X[c], z)))
        Y.append(v)
    sq = []
    for i in range(2):
        a = dd_add((X[i], z), dd_neg(two_prod(x1[i], X[2])))
        b = dd_add(Y[i], dd_neg(dd_mul(Y[2], (x2[i], z))))
        for num, den, w in ((a, (X[2], z), w1[i]), (b, Y[2], w2[i])):
            r = dd_mul(dd_div(num, den), (w, z))
            sq.append(dd_mul(r, r))
    return dd_sum((np.concatenate([v[0] for v in sq]), np.concatenate([v[1] for v in sq]))), Y[2][0]


def basis(t):
    """Orthonormal basis (3 x 2) of the plane across the unit vector t: b1 along t x e_i, i the first axis of smallest
    |t_i|, and b2 = t x b1."""
    i = int(np.argmin(np.abs(t)))
    e = np.zeros(3, t.dtype)
    e[i] = 1
    b1 = np.cross(t, e)
    b1 = b1 / np.sqrt(b1 @ b1)
    return np.stack([b1, np.cross(t, b1)], 1)


def skew(a):
    z = a.dtype.type(0)
    return np.array([[z, -a[2], a[1]], [a[2], z, -a[0]], [-a[1], a[0], z]], a.dtype)


def expso3(a):
    """exp([a]x) by Rodrigues' formula, (1 - cos th) / th^2 as 2 sin^2(th / 2) / th^2; the series' first terms below
    th = 1e-8."""
    th2 = a @ a
    if th2 < 1e-16:
        A, Cc = a.dtype.type(1), a.dtype.type(0.5)
    else:
        th = np.sqrt(th2)
        s = np.sin(th / 2)
        A, Cc = np.sin(th) / th, 2 * s * s / th2
    K = skew(a)
    return np.eye(3, dtype=a.dtype) + A * K + Cc * (K @ K)


def select(x1, x2, R, t, X, use, front, min_angle):
    """The mask of the correspondences used, at the start orientation."""
    Y = R @ X + t[:, None]
    ok = np.asarray(use, bool) & (front * X[2] > 0) & (front * Y[2] > 0)
    one = np.ones((1, x1.shape[1]), x1.dtype)
    d1, d2 = np.vstack([x1, one]), R.T @ np.vstack([x2, one])
    c = np.cross(d1, d2, axis=0)
    s = np.sin(x1.dtype.type(min_angle))
    return ok & (np.sum(c * c, 0) >= s * s * np.sum(d1 * d1, 0) * np.sum(d2 * d2, 0))


def ray_angles(x1, x2, R):
    """The angle between the two rays of every correspondence (radians)."""
    one = np.ones((1, x1.shape[1]))
    d1, d2 = np.vstack([x1, one]), R.T @ np.vstack([x2, one])
    c = np.cross(d1, d2, axis=0)
    return np.arctan2(np.sqrt(np.sum(c * c, 0)), np.sum(d1 * d2, 0))


def residuals(x1, x2, w1, w2, R, t, X):
    Y = R @ X + t[:, None]
    return w1 * (X[:2] / X[2] - x1), w2 * (Y[:2] / Y[2] - x2), Y


def blocks(x1, x2, w1, w2, R, t, B, X):
    """Residuals and Jacobian blocks of every point: r1, r2 (2 x n), J1, J2 (2 x 3 x n, to the point), A (2 x 5 x n, the
    second image's to the pose: rotation vector a, then b)."""
    n = X.shape[1]
    r1, r2, Y = residuals(x1, x2, w1, w2, R, t, X)

    def proj(Y, w):
        P = np.zeros((2, 3, n), X.dtype)
        P[0, 0] = P[1, 1] = 1 / Y[2]
        P[0, 2], P[1, 2] = -Y[0] / (Y[2] * Y[2]), -Y[1] / (Y[2] * Y[2])
        return w[:, None, :] * P
    J1, P2 = proj(X, w1), proj(Y, w2)
    J2 = np.einsum('ijn,jk->ikn', P2, R)
    RX = Y - t[:, None]
    M = np.zeros((3, 5, n), X.dtype)
    for j in range(3):                                   # d(a x RX) / da_j = e_j x RX
        e = np.zeros(3, X.dtype)
        e[j] = 1
        M[:, j] = np.cross(e[:, None], RX, axis=0)
    M[:, 3:] = B[:, :, None]
    return r1, r2, J1, J2, np.einsum('ijn,jkn->ikn', P2, M)


def chol3(V):
    """Vectorised Cholesky of 3 x 3 x n: the factor L (3 x 3 x n, zero above the diagonal) and the pivots (3 x n)."""
    L = np.zeros_like(V)
    d = np.zeros((3, V.shape[2]), V.dtype)
    with np.errstate(all='ignore'):
        d[0] = V[0, 0]
        L[0, 0] = np.sqrt(d[0])
        L[1, 0], L[2, 0] = V[1, 0] / L[0, 0], V[2, 0] / L[0, 0]
        d[1] = V[1, 1] - L[1, 0] * L[1, 0]
        L[1, 1] = np.sqrt(d[1])
        L[2, 1] = (V[2, 1] - L[2, 0] * L[1, 0]) / L[1, 1]
        d[2] = V[2, 2] - L[2, 0] * L[2, 0] - L[2, 1] * L[2, 1]
        L[2, 2] = np.sqrt(d[2])
    return L, d


def solve3(L, b):
    """L L' x = b for b (3 x k x n) or (3 x n)."""
    with np.errstate(all='ignore'):
        y0 = b[0] / L[0, 0]
        y1 = (b[1] - L[1, 0] * y0) / L[1, 1]
        y2 = (b[2] - L[2, 0] * y0 - L[2, 1] * y1) / L[2, 2]
        x2 = y2 / L[2, 2]
        x1 = (y1 - L[2, 1] * x2) / L[1, 1]
        x0 = (y0 - L[1, 0] * x1 - L[2, 0] * x2) / L[0, 0]
    return np.stack([x0, x1, x2])


def chol(S):
    """Scalar Cholesky of a small matrix: (L, pivots); the factor is not to be used where a pivot is not positive."""
    m = S.shape[0]
    L = np.zeros_like(S)
    d = np.zeros(m, S.dtype)
    with np.errstate(all='ignore'):
        for j in range(m):
            d[j] = S[j, j] - L[j, :j] @ L[j, :j]
            L[j, j] = np.sqrt(d[j])
            for i in range(j + 1, m):
                L[i, j] = (S[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return L, d


def chol_solve(L, b):
    m = L.shape[0]
    y = np.zeros_like(b)
    for i in range(m):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros_like(b)
    for i in reversed(range(m)):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def normal_blocks(r1, r2, J1, J2, A):
    U = np.einsum('ian,ibn->ab', A, A)
    V = np.einsum('ian,ibn->abn', J1, J1) + np.einsum('ian,ibn->abn', J2, J2)
    W = np.einsum('ian,ijn->ajn', A, J2)
    gp = np.einsum('ian,in->a', A, r2)
    gk = np.einsum('ian,in->an', J1, r1) + np.einsum('ian,in->an', J2, r2)
    return U, V, W, gp, gk


def reduced(U, V, W, gp, gk, lam):
    """The damped reduced system: (S, rhs, L of the point blocks, their pivots)."""
    Vd = V.copy()
    for i in range(3):
        Vd[i, i] = V[i, i] + lam * V[i, i]
    L, d = chol3(Vd)
    Z = solve3(L, np.swapaxes(W, 0, 1))                  # V^-1 W' : 3 x 5 x n
    S = U + lam * np.diag(np.diag(U)) - np.einsum('ajn,jbn->ab', W, Z)
    rhs = gp - np.einsum('jan,jn->a', Z, gk)
    return S, rhs, L, d


def adjust(x1, x2, R, t, X, use=None, w1=None, w2=None, front=-1, max_iter=20, conv_tol=1e-6, min_angle=0.0, dtype=float):
    """One pair.  dict(R, t, X (3 x n, the unused columns as given), used, code, iters, trials, n, f0, f, sigma0, lam, Q
    (6 x 6), res (2 x 2 x n: image, axis; zero where unused))."""
    T = np.dtype(dtype).type
    cv = lambda a: np.array(a, dtype)
    n_all = np.asarray(x1).shape[1]
    x1, x2, R, t, X = cv(x1), cv(x2), cv(R), cv(t), cv(X)
    w1 = np.ones((2, n_all), dtype) if w1 is None else cv(np.broadcast_to(w1, (2, n_all)))
    w2 = np.ones((2, n_all), dtype) if w2 is None else cv(np.broadcast_to(w2, (2, n_all)))
    use = np.ones(n_all, bool) if use is None else np.asarray(use, bool)
    used = select(x1, x2, R, t, X, use, front, min_angle)
    n = int(used.sum())
    out = dict(R=R, t=t, X=X.copy(), used=used, n=n, code=4, iters=0, trials=0, f0=T(np.nan), f=T(np.nan), sigma0=T(np.nan),
               lam=T(LAMBDA0), Q=np.full((6, 6), np.nan, dtype), res=np.zeros((2, 2, n_all), dtype))
    if n < 5:
        return out
    a1, a2, v1, v2, Xc = x1[:, used], x2[:, used], w1[:, used], w2[:, used], X[:, used]
    B = basis(t)
    Rp = orthonormalise((R, np.zeros_like(R)))              # R as a pair; the linear algebra reads its high word
    R = Rp[0]
    fp = objective(a1, a2, v1, v2, Rp, t, Xc)[0]
    f = fp[0]
    f0, lam, tol2, floor = f, T(LAMBDA0), T(conv_tol) * T(conv_tol), T(FLOOR) * 4 * n
    iters = trials = 0
    code = None
    while code is None:
        if iters >= max_iter:
            code = 1
            break
        U, V, W, gp, gk = normal_blocks(*blocks(a1, a2, v1, v2, R, t, B, Xc))
        while True:
            trials += 1
            S, rhs, L, d = reduced(U, V, W, gp, gk, lam)
            LS, dS = chol(S)
            ok = bool(np.all(d > 0)) and bool(np.all(dS > 0))
            q = T(np.inf)
            if ok:
                dp = -chol_solve(LS, rhs)
                dk = -solve3(L, gk + np.einsum('ajn,a->jn', W, dp))
                q = -(gp @ dp + np.sum(gk * dk))
            if f <= floor or (ok and q <= tol2 * f):
                code = 0
                break
            good = False
            if ok:
                E = expso3(dp[:3])
                Rn = orthonormalise(dd_matmul((E, np.zeros_like(E)), Rp))
                tn = t + B @ dp[3:]
                tn = tn / np.sqrt(tn @ tn)
                Xn = Xc + dk
                with np.errstate(all='ignore'):
                    fn, z2 = objective(a1, a2, v1, v2, Rn, tn, Xn)
                    good = bool(np.isfinite(fn[0]) and dd_less(fn, fp) and np.all(front * Xn[2] > 0) and np.all(front * z2 > 0))
            if good:
                Rp, R, t, Xc, fp, f, B = Rn, Rn[0], tn, Xn, fn, fn[0], basis(tn)
                lam = max(lam / 10, T(LAMBDA_MIN))
                iters += 1
                break
            lam = lam * 10
            if lam > LAMBDA_MAX:
                code = 2
                break
    # the end: the undamped reduced matrix at the final point, its cofactor matrix in ambient coordinates
    r1, r2, J1, J2, A = blocks(a1, a2, v1, v2, R, t, B, Xc)
    U, V, W, gp, gk = normal_blocks(r1, r2, J1, J2, A)
    S0, _, L, d = reduced(U, V, W, gp, gk, T(0))
    singular = bool(np.any(~(d > V_PIVOT * np.stack([V[0, 0], V[1, 1], V[2, 2]]))))
    Q = np.full((6, 6), np.nan, dtype)
    if not singular:
        LS, dS = chol(S0)
        singular = bool(np.any(~(dS > S_PIVOT * np.diag(S0))))
        if not singular:
            Si = np.stack([chol_solve(LS, e) for e in np.eye(5, dtype=dtype)], 1)
            Bf = np.zeros((6, 5), dtype)
            Bf[:3, :3] = np.eye(3, dtype=dtype)
            Bf[3:, 3:] = B
            Q = Bf @ Si @ Bf.T
    if code == 0 and singular:
        code = 3
    Xo = X.copy()
    Xo[:, used] = Xc
    res = np.zeros((2, 2, n_all), dtype)
    res[0][:, used], res[1][:, used] = r1, r2
    out.update(R=R, t=t, X=Xo, code=code, iters=iters, trials=trials, f0=f0, f=f, lam=lam, Q=Q, res=res,
               sigma0=np.sqrt(f / (n - 5)) if n > 5 else T(np.nan))
    return out


# ---- the seeded cases of the tests -----------------------------------------------------------------------------------

SIZES = (5, 6, 8, 63, 64, 65, 255, 256, 257, 1000)
NOISES = (0.0, 5e-4)
WEIGHT, MIN_ANGLE, CONV_TOL, MAX_ITER = 2000.0, np.deg2rad(0.5), 1e-12, 100


def seeded_case(n, noise, seed=None):
    """The synthetic pair of np.random.default_rng(1000 + n) and, from the same generator, its start: R turned by a
    rotation vector 0.01 N(0, I), t moved by 0.02 N(0, I) and renormalised, X from forwintersect3 of the start pair."""
    import relorient_ref as rr
    rng = np.random.default_rng(1000 + n if seed is None else seed)
    S = rr.synthetic_pair(rng, n, front=-1, noise=noise)
    R0 = rr.rodrigues(0.01 * rng.normal(size=3)) @ S['R']
    t0 = S['t'] + 0.02 * rng.normal(size=3)
    t0 = t0 / np.linalg.norm(t0)
    X0 = rr.forwintersect3([np.eye(3, 4), np.hstack([R0, t0[:, None]])], np.stack([S['x1'], S['x2']], 1))
    return dict(S, n=n, noise=noise, R0=R0, t0=t0, X0=X0)


def run_case(c, dtype=float, **kw):
    n = c['x1'].shape[1]
    opt = dict(w1=np.full((2, n), WEIGHT), w2=np.full((2, n), WEIGHT), front=-1, max_iter=MAX_ITER, conv_tol=CONV_TOL,
               min_angle=MIN_ANGLE, dtype=dtype)
    opt.update(kw)
    return adjust(c['x1'], c['x2'], c['R0'], c['t0'], c['X0'], **opt)


def distance(a, b, stat=True):
    """The largest difference of two results in R, t and the used X and, where stat, relative in sigma0 and Q.  (stat is
    for pairs with noise and redundancy: the sigma0 of a noise-free pair is the rounding of its residuals, which no two
    routes share, and that of five points is NaN.)"""
    u = a['used']
    d = [np.abs(a['R'] - b['R']).max(), np.abs(a['t'] - b['t']).max(), np.abs(a['X'][:, u] - b['X'][:, u]).max()]
    if stat:
        d.append(abs(a['sigma0'] / b['sigma0'] - 1))
        d.append(np.abs(a['Q'] - b['Q']).max() / np.abs(b['Q']).max())
    return float(max(d))
