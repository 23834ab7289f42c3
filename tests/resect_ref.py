"""High-precision references of the initial-value stage, for tests only: three-point resection
(photogrammetry/pm_resect_3pt.m: Grunert's solution as in Haralick et al. 1994) and forward intersection
(photogrammetry/forwintersect.m) restated in np.longdouble (64-bit mantissa on x86-64: eps 1.1e-19, 2048 times finer
than float64).  Written from the formulas, separate from oracle/initial_oracle.py: no code is shared, so a slip in one
does not hide in the other.

Resection: the quartic's coefficients are formed in longdouble, np.roots (float64) only supplies the starting roots,
and every root is polished by Newton steps on the longdouble polynomial until the step is below 4 longdouble eps of
the root; frames, poses and rms are longdouble; ALL candidate poses are returned with their rms.

Forward intersection: lens correction, rotation, sum (I - d d') and the 3 x 3 solve by the adjugate (np.linalg has no
longdouble solve), about the first projection centre of each point (the same point mathematically, without the
digits that coordinates of 1e6 m cost the uncentred sum).

Out of scope (the algorithm's own singularities, shared with the reference): a camera exactly over the centre of an
equilateral triangle (Grunert's u is 0/0 there) and tele geometries (flying height many times the triangle's size,
where the quartic's roots crowd together); seeded_case() draws heights of 10 ... 40 m over a 40 m field.  Rays more
than 90 degrees apart are outside the algorithm as well (it takes the angle between the LINES of two rays, the
reference's subspace(), which is the acute one), so the points of a case lie inside an image format of +-FORMAT in
normalised coordinates: any two rays are then less than 81 degrees apart.
"""
import numpy as np

FORMAT = 0.6

LD = np.longdouble
CLD = np.clongdouble
EPS_LD = np.finfo(LD).eps
EPS = np.finfo(np.float64).eps


def _ld(a):
    return np.asarray(a, dtype=LD)


def _norm(v):
    return np.sqrt(np.sum(v * v))


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype=LD)


def rot_ld(ang):
    """World-to-camera rotation of omega, phi, kappa in longdouble: (R1(omega) R2(phi) R3(kappa))'."""
    o, p, k = _ld(ang)
    so, co, sp, cp, sk, ck = np.sin(o), np.cos(o), np.sin(p), np.cos(p), np.sin(k), np.cos(k)
    one, zero = LD(1), LD(0)
    R1 = np.array([[one, zero, zero], [zero, co, -so], [zero, so, co]], dtype=LD)
    R2 = np.array([[cp, zero, sp], [zero, one, zero], [-sp, zero, cp]], dtype=LD)
    R3 = np.array([[ck, -sk, zero], [sk, ck, zero], [zero, zero, one]], dtype=LD)
    return (R1 @ R2 @ R3).T


def quartic(X3, d3):
    """Coefficients (descending powers) of Grunert's quartic in v = s3 / s1 for the triangle X3 (3 x 3, columns are
    points) seen along the unit rays d3 (3 x 3, columns), and the quantities the ray lengths need."""
    a = _norm(X3[:, 2] - X3[:, 1]); b = _norm(X3[:, 2] - X3[:, 0]); c = _norm(X3[:, 1] - X3[:, 0])
    one = LD(1)
    # the cosine of the angle between the LINES the rays span (subspace() in the reference)
    ca = min(one, abs(np.sum(d3[:, 1] * d3[:, 2])))
    cb = min(one, abs(np.sum(d3[:, 0] * d3[:, 2])))
    cg = min(one, abs(np.sum(d3[:, 0] * d3[:, 1])))
    a2, b2, c2 = a * a, b * b, c * c
    m, p = (a2 - c2) / b2, (a2 + c2) / b2
    A4 = (m - 1) ** 2 - 4 * c2 / b2 * ca ** 2
    A3 = 4 * (m * (1 - m) * cb + 2 * c2 / b2 * ca ** 2 * cb - (1 - p) * ca * cg)
    A2 = 2 * (m ** 2 + 2 * m ** 2 * cb ** 2 + 2 * (b2 - c2) / b2 * ca ** 2 + 2 * (b2 - a2) / b2 * cg ** 2
              - 4 * p * ca * cb * cg - 1)
    A1 = 4 * (-m * (1 + m) * cb + 2 * a2 / b2 * cg ** 2 * cb - (1 - p) * ca * cg)
    A0 = (1 + m) ** 2 - 4 * a2 / b2 * cg ** 2
    return np.array([A4, A3, A2, A1, A0], dtype=LD), dict(m=m, b2=b2, ca=ca, cb=cb, cg=cg)


def polish_roots(co, z0, max_steps=60):
    """Newton steps on the longdouble polynomial co (descending) from the starting roots z0 until the step is below
    4 longdouble eps of the root -- or, at a root whose value cannot be told from zero any closer (the rounding of
    p(z) itself, 8 eps sum |c_i| |z|^i, over |p'(z)| is more than that), until the step is inside that noise and has
    stopped shrinking.  Returns (roots as clongdouble, converged mask)."""
    co = _ld(co)
    z = np.asarray(z0, dtype=CLD).copy()
    ok = np.zeros(z.size, bool)
    for k in range(z.size):
        zk = z[k]
        last = np.inf
        for _ in range(max_steps):
            p, dp, mag = CLD(co[0]), CLD(0), abs(co[0])
            for cc in co[1:]:
                dp = dp * zk + p
                p = p * zk + cc
                mag = mag * abs(zk) + abs(cc)
            if p == 0:
                ok[k] = True
                break
            if dp == 0:
                break
            step = p / dp
            zk = zk - step
            if abs(step) <= 4 * EPS_LD * abs(zk) or (abs(step) >= last and abs(step) <= 8 * EPS_LD * mag / abs(dp)):
                ok[k] = True
                break
            last = abs(step)
        z[k] = zk
    return z, ok


def _frame(p0, pb, pc):
    ob, oc = pb - p0, pc - p0
    n1 = _cross(ob, oc)
    n2 = _cross(ob, n1)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.stack([ob / _norm(ob), n1 / _norm(n1), n2 / _norm(n2)], 1)


def rms_ld(P, X, x):
    """rms of the reprojection error of the 3 x 4 matrix P over the points X (3 x n) with image points x (2 x n)."""
    P, X, x = _ld(P), _ld(X), _ld(x)
    h = P[:, :3] @ X + P[:, 3:4]
    e = h[:2] / h[2] - x
    return np.sqrt(np.sum(e * e) / LD(X.shape[1]))


def rms_exact(P, X, x):
    """rms of the reprojection error of the float64 matrix P over the float64 points X, x: the mean square in exact
    rational arithmetic, rounded once to longdouble, then the longdouble square root.  rms_ld evaluates h = P [X; 1]
    with a few longdouble eps of |R X| + |t|, which is 1e-4 of a residual of 1e-15 (a point the pose was solved from):
    where the rms is to be known to float64 rounding whatever its size, only this will do."""
    from fractions import Fraction as F
    P, X, x = np.asarray(P, float), np.asarray(X, float), np.asarray(x, float)
    total = F(0)
    for i in range(X.shape[1]):
        h = [F(P[r, 0]) * F(X[0, i]) + F(P[r, 1]) * F(X[1, i]) + F(P[r, 2]) * F(X[2, i]) + F(P[r, 3]) for r in range(3)]
        e0, e1 = h[0] / h[2] - F(x[0, i]), h[1] / h[2] - F(x[1, i])
        total += e0 * e0 + e1 * e1
    mean = total / X.shape[1]
    hi = float(mean)                                   # (correctly rounded; the remainder is exact)
    lo = float(mean - F(hi))
    return np.sqrt(LD(hi) + LD(lo))


def resect_3pt(X, x, tri, behind=True, root_report=None):
    """All candidate poses of the triangle tri (three columns of X, in this order) with their rms over ALL columns.
    X 3 x n object points, x 2 x n normalised image points (any float type; taken to longdouble as they are).
    Returns (PP, rms): lists of 3 x 4 longdouble matrices and longdouble rms, in the order of the polished roots.  A
    degenerate triangle (collinear or repeated points: no frame, or no quartic) has no candidate."""
    X, x = _ld(X), _ld(x)
    tri = list(tri)
    X3 = X[:, tri]
    d3 = np.vstack([x[:, tri], np.ones((1, 3), dtype=LD)])
    d3 = d3 / np.sqrt(np.sum(d3 * d3, 0))
    with np.errstate(divide='ignore', invalid='ignore'):
        co, q = quartic(X3, d3)
        oR = _frame(X3[:, 0], X3[:, 2], X3[:, 1])
    if not (np.all(np.isfinite(co)) and np.all(np.isfinite(oR))):
        return [], []
    lead = 0
    while lead < 4 and co[lead] == 0:
        lead += 1
    if lead == 4:
        return [], []
    z0 = np.roots(np.asarray(co[lead:], float))
    z, conv = polish_roots(co[lead:], z0)
    if root_report is not None:
        root_report.update(coeffs=co, start=z0, roots=z, converged=conv)
    PP, res = [], []
    m, b2, ca, cb, cg = q['m'], q['b2'], q['ca'], q['cb'], q['cg']
    for zk in z:
        if not abs(zk.imag) / abs(zk) < 1e-3:
            continue
        v = LD(zk.real)
        with np.errstate(divide='ignore', invalid='ignore'):
            u = ((m - 1) * v * v - 2 * m * cb * v + 1 + m) / (2 * (cg - v * ca))
            s1 = np.sqrt(b2 / (1 + v * v - 2 * v * cb))
        s3, s2 = v * s1, u * s1
        if not (s1 >= 0 and s2 >= 0 and s3 >= 0):
            continue
        cx = np.array([s1, s2, s3], dtype=LD)[None, :] * d3
        if behind:
            cx = -cx
        R = _frame(cx[:, 0], cx[:, 2], cx[:, 1]) @ oR.T
        centre = X3[:, 0] - R.T @ cx[:, 0]
        P = np.hstack([R, -(R @ centre)[:, None]])
        if not np.all(np.isfinite(P)):
            continue
        PP.append(P)
        res.append(rms_ld(P, X, x))
    return PP, res


def best_pose(cands):
    """(P, rms) of the first smallest rms among (PP, rms) lists, or (None, inf)."""
    PP, res = cands
    if not PP:
        return None, LD(np.inf)
    k = int(np.argmin(np.array(res, dtype=LD)))
    return PP[k], res[k]


def centre_ld(P):
    """-R' t of a 3 x 4 matrix in longdouble."""
    P = _ld(P)
    return -(P[:, :3].T @ P[:, 3])


def project_ld(R, C, X):
    """Normalised image points of X (3 x n) in the camera [R | -R C], longdouble."""
    h = _ld(R) @ (_ld(X) - _ld(C)[:, None])
    return h[:2] / h[2]


def seeded_case(seed, npt=20, H=(10.0, 40.0), field=40.0, noise=0.0, shift=None):
    """One camera at a height H[0] ... H[1] over a field x field square of npt points (relief 2 m), looking down
    (along -z) with up to 0.2 rad of tilt and any heading; the image points are projected in longdouble.  The largest
    triangle in the image comes first.  Returns a dict: X (3 x npt float64), xl (2 x npt longdouble: exact projections),
    x (xl rounded to float64, with `noise` added to the points outside the triangle), tri (ascending indices), R, C
    (true pose, longdouble; R from float64 angles, C float64).  shift: a translation of the world frame added to X
    and C (both stay exact float64 numbers, so the case is the same scene at large coordinates)."""
    rng = np.random.default_rng(91000 + seed)
    C = np.array([rng.uniform(0.25 * field, 0.75 * field), rng.uniform(0.25 * field, 0.75 * field), rng.uniform(*H)])
    ang = np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(-np.pi, np.pi)])
    C = np.round(C * 1024) / 1024                     # (a shift of 1e6 m then keeps every coordinate exact)
    R = rot_ld(ang)
    # points of the field inside the image format |x|, |y| <= FORMAT: the first npt of one stream of candidates, so
    # the scenes of one seed are nested in npt
    cand = np.vstack([rng.uniform(0, field, (2, 8000)), rng.uniform(0, 2.0, (1, 8000))])
    cand = np.round(cand * 1024) / 1024
    inside = np.flatnonzero(np.all(np.abs(np.asarray(project_ld(R, C, cand), float)) <= FORMAT, 0))
    if inside.size < npt:
        raise ValueError('seeded_case: %d of %d points inside the format' % (inside.size, npt))
    X = cand[:, inside[:npt]]
    if shift is not None:
        X = X + np.asarray(shift, float)[:, None]
        C = C + np.asarray(shift, float)
    xl = project_ld(R, C, X)
    x = np.asarray(xl, float)
    # the largest triangle in the image among the first 20 points (all triplets)
    from itertools import combinations
    T = np.array(list(combinations(range(min(npt, 20)), 3)))
    ax, ay = x[0][T], x[1][T]
    A = np.abs(ax[:, 0] * (ay[:, 1] - ay[:, 2]) + ax[:, 1] * (ay[:, 2] - ay[:, 0]) + ax[:, 2] * (ay[:, 0] - ay[:, 1]))
    tri = np.sort(T[int(np.argmax(A))])
    if noise:
        other = np.setdiff1d(np.arange(npt), tri)
        x[:, other] += noise * rng.standard_normal((2, other.size))
    return dict(X=X, xl=xl, x=x, tri=tri, R=R, C=_ld(C), seed=seed)


def pose_err(P, Pref):
    """max |P - Pref| as float."""
    return float(np.max(np.abs(_ld(P) - _ld(Pref))))


# ---- forward intersection ----------------------------------------------------------------------------------------------

def lenscorr_ld(s):
    """Lens-corrected image points in mm (y up), 2 x n longdouble: the backward Brown polynomial in the measured point."""
    nK, nP = int(s.IO.model.nK), int(s.IO.model.nP)
    cam = np.asarray(s.IP.cam)
    IO = _ld(s.IO.val)[:, cam]
    px = _ld(s.IO.sensor.pxSize)[:, cam]
    if getattr(s.IO.sensor, 'samePxSize', False):
        px = np.vstack([px[0], px[0]])
    uv = _ld(s.IP.val)
    qx, qy = px[0] * uv[0], -px[1] * uv[1]
    xb, yb = qx - IO[1], qy - IO[2]
    r2 = xb * xb + yb * yb
    radial = np.zeros_like(r2)
    for j in range(nK, 0, -1):                         # Horner in r2: K1 r2 + K2 r2^2 + ...
        radial = (radial + IO[4 + j]) * r2
    dx, dy = xb * radial, yb * radial
    if nP >= 2:
        P1, P2 = IO[5 + nK], IO[6 + nK]
        scale = 1 + IO[7 + nK] if nP > 2 else LD(1)
        dx = dx + scale * (P1 * (r2 + 2 * xb * xb) + 2 * P2 * xb * yb)
        dy = dy + scale * (P2 * (r2 + 2 * yb * yb) + 2 * P1 * xb * yb)
    return np.stack([qx - dx, qy - dy]), IO


def rays_ld(s):
    """(c, d): projection centre and unit direction (world frame) of every image point, 3 x n longdouble."""
    xy, IO = lenscorr_ld(s)
    cam = np.asarray(s.IP.cam)
    dc = np.stack([xy[0] - IO[1], xy[1] - IO[2], -IO[0]])
    EO = _ld(s.EO.val)
    M = [rot_ld(EO[3:6, i]).T for i in range(EO.shape[1])]          # camera-to-world
    d = np.stack([M[c] @ dc[:, k] for k, c in enumerate(cam)], 1)
    d = d / np.sqrt(np.sum(d * d, 0))
    return EO[:3, cam], d


def solve3_adj(A, b):
    """A \\ b for a symmetric 3 x 3 A by the adjugate, longdouble."""
    c00 = A[1, 1] * A[2, 2] - A[1, 2] * A[1, 2]
    c01 = A[0, 2] * A[1, 2] - A[0, 1] * A[2, 2]
    c02 = A[0, 1] * A[1, 2] - A[0, 2] * A[1, 1]
    c11 = A[0, 0] * A[2, 2] - A[0, 2] * A[0, 2]
    c12 = A[0, 1] * A[0, 2] - A[0, 0] * A[1, 2]
    c22 = A[0, 0] * A[1, 1] - A[0, 1] * A[0, 1]
    det = A[0, 0] * c00 + A[0, 1] * c01 + A[0, 2] * c02
    adj = np.array([[c00, c01, c02], [c01, c11, c12], [c02, c12, c22]], dtype=LD)
    return (adj @ b) / det


def forwintersect_ld(s, want_cond=False):
    """The point closest to its rays for every object point of s, 3 x n_points longdouble; NaN with fewer than two
    rays.  (sum_j (I - d_j d_j')) (Q - c_1) = sum_j (I - d_j d_j') (c_j - c_1).  want_cond: also the condition
    number of every point's 3 x 3 matrix (float64, NaN without one)."""
    c, d = rays_ld(s)
    pt = np.asarray(s.IP.pt)
    npnt = s.OP.val.shape[1]
    out = np.full((3, npnt), np.nan, dtype=LD)
    cond = np.full(npnt, np.nan)
    order = np.argsort(pt, kind='stable')
    bounds = np.searchsorted(pt[order], np.arange(npnt + 1))
    I3 = np.eye(3, dtype=LD)
    for p in range(npnt):
        rows = order[bounds[p]:bounds[p + 1]]
        if rows.size < 2:
            continue
        c0 = c[:, rows[0]]
        A = np.zeros((3, 3), dtype=LD)
        b = np.zeros(3, dtype=LD)
        for r in rows:
            Pj = I3 - np.outer(d[:, r], d[:, r])
            A += Pj
            b += Pj @ (c[:, r] - c0)
        out[:, p] = c0 + solve3_adj(A, b)
        cond[p] = np.linalg.cond(np.asarray(A, float))
    return (out, cond) if want_cond else out


def two_ray_midpoint(c1, d1, c2, d2):
    """Midpoint of the common perpendicular of the lines c1 + t d1 and c2 + t d2, longdouble (closed form)."""
    c1, d1, c2, d2 = _ld(c1), _ld(d1), _ld(c2), _ld(d2)
    w = c1 - c2
    a, b, c = np.sum(d1 * d1), np.sum(d1 * d2), np.sum(d2 * d2)
    d, e = np.sum(d1 * w), np.sum(d2 * w)
    den = a * c - b * b
    t1, t2 = (b * e - c * d) / den, (a * e - b * d) / den
    return ((c1 + t1 * d1) + (c2 + t2 * d2)) / 2
