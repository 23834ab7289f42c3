"""NumPy restatement of the resection RANSAC of dbat_hip_resect_ransac (csrc/resect_ransac.hpp), for tests only: the
candidate poses of every sample come from resect_ref.resect_3pt (np.longdouble, written from the formulas), every pose
is scored by the number of points that may be used, lie in front (third row of P [X; 1] negative) and have
e0^2 + e1^2 <= thr2, and the winner has the most inliers -- of equal counts the lowest (sample, root) -- and at least
four.  Shares no code with dbat_amd/.

Two routes: dtype np.longdouble scores the longdouble poses in longdouble; dtype float rounds every pose to float64 and
scores it in plain float64.  The seeds of the tests are chosen so that both pick the same winner
(tests/test_resect_robust_cpu.py).

The root of a winner is its index among the poses resect_3pt returns for the sample, in the order of np.roots; the
device numbers the poses in the order of its own root finder.  A test that compares the two matches the device's pose
with poses[root] by value."""
import numpy as np

import resect_ref as rf

MIN_INLIERS = 4


def residuals2(P, X, x):
    """(e0^2 + e1^2, the third row of P [X; 1]) of every point, in the dtype of P."""
    with np.errstate(all='ignore'):
        h = P[:, :3] @ X + P[:, 3:4]
        e = h[:2] / h[2] - x
        return np.sum(e * e, 0), h[2]


def _gap(rep):
    """The smallest relative distance of two roots in resect_3pt's root report (inf with fewer than two)."""
    if 'roots' not in rep or len(rep['roots']) < 2:
        return np.inf
    z = np.asarray(rep['roots'], complex)
    d = np.abs(z[:, None] - z[None, :]) / np.maximum(np.abs(z[:, None]), np.abs(z[None, :]))
    return float(np.min(d[~np.eye(len(z), dtype=bool)]))


def candidates(X, x, samples, use=None):
    """(poses, gaps): per sample the list of np.longdouble poses of resect_3pt (none for a sample with a point that may
    not be used) and the smallest relative distance of two roots of its quartic."""
    use = np.ones(X.shape[1], bool) if use is None else np.asarray(use, bool)
    poses, gaps = [], []
    for tri in np.asarray(samples).reshape(-1, 3):
        rep = {}
        poses.append(rf.resect_3pt(X, x, tri, root_report=rep)[0] if use[tri].all() else [])
        gaps.append(_gap(rep))
    return poses, np.array(gaps)


def ransac(X, x, samples, thr2, use=None, dtype=np.longdouble, poses=None):
    """One camera: X 3 x n, x 2 x n, samples k x 3; poses: candidates(...)[0], if at hand.  dict(P (3 x 4 of dtype, or
    None), count, sample, root, scored, mask, ssq, e2 (per scored pose: (sample, root, count, the squared residuals of the
    usable points in front)), poses)."""
    n = X.shape[1]
    use = np.ones(n, bool) if use is None else np.asarray(use, bool)
    Xd, xd = np.asarray(X, dtype), np.asarray(x, dtype)
    poses = candidates(X, x, samples, use)[0] if poses is None else poses
    best = (0, -1, -1, None)
    scored, e2_all = 0, []
    for k, PP in enumerate(poses):
        for q, P in enumerate(PP):
            P = np.asarray(P, dtype)
            e2, z = residuals2(P, Xd, xd)
            front = use & (z < 0)
            cnt = int((front & (e2 <= thr2)).sum())
            scored += 1
            e2_all.append((k, q, cnt, e2[front]))
            if cnt >= MIN_INLIERS and cnt > best[0]:      # ascending (sample, root): a later one only if strictly larger
                best = (cnt, k, q, P)
    mask = np.zeros(n, bool)
    ssq = 0.0
    if best[3] is not None:
        e2, z = residuals2(best[3], Xd, xd)
        mask = use & (z < 0) & (e2 <= thr2)
        ssq = float(np.sum(e2[mask]))
    return dict(P=best[3], count=best[0], sample=best[1], root=best[2], scored=scored, mask=mask, ssq=ssq, e2=e2_all, poses=poses)


def _frame64(p0, pb, pc):
    ob, oc = pb - p0, pc - p0
    n1 = np.cross(ob, oc)
    n2 = np.cross(ob, n1)
    with np.errstate(all='ignore'):
        return np.stack([ob / np.linalg.norm(ob), n1 / np.linalg.norm(n1), n2 / np.linalg.norm(n2)], 1)


def poses_float64(X, x, tri):
    """The float64 route of resect_ref.resect_3pt, for the conditioning of a sample: the same formulas with every
    quantity in float64 -- the quartic's coefficients formed in float64, its roots those of np.roots, not polished.
    Returns the list of 3 x 4 float64 poses (in front of the camera: behind = True)."""
    X3 = np.asarray(X, float)[:, list(tri)]
    d3 = np.vstack([np.asarray(x, float)[:, list(tri)], np.ones((1, 3))])
    d3 = d3 / np.sqrt(np.sum(d3 * d3, 0))
    with np.errstate(all='ignore'):
        co, q = rf.quartic(X3, d3)                        # float64 in, float64 arithmetic
        oR = _frame64(X3[:, 0], X3[:, 2], X3[:, 1])
    co = np.asarray(co, float)
    m, b2, ca, cb, cg = (float(q[k]) for k in ('m', 'b2', 'ca', 'cb', 'cg'))
    if not (np.all(np.isfinite(co)) and np.all(np.isfinite(oR))) or not np.any(co[:4] != 0):
        return []
    out = []
    for zk in np.roots(co[int(np.flatnonzero(co != 0)[0]):]):
        if not abs(zk.imag) / abs(zk) < 1e-3:
            continue
        v = float(zk.real)
        with np.errstate(all='ignore'):
            u = ((m - 1) * v * v - 2 * m * cb * v + 1 + m) / (2 * (cg - v * ca))
            s1 = np.sqrt(b2 / (1 + v * v - 2 * v * cb))
        s3, s2 = v * s1, u * s1
        if not (s1 >= 0 and s2 >= 0 and s3 >= 0):
            continue
        cx = -np.array([s1, s2, s3])[None, :] * d3
        R = _frame64(cx[:, 0], cx[:, 2], cx[:, 1]) @ oR.T
        centre = X3[:, 0] - R.T @ cx[:, 0]
        P = np.hstack([R, -(R @ centre)[:, None]])
        if np.all(np.isfinite(P)):
            out.append(P)
    return out


def rotation_distance(P, PP):
    """(the index of the pose of PP whose rotation is closest to that of P, the distances to all of them)."""
    d = [float(np.abs(np.asarray(P, np.longdouble)[:, :3] - np.asarray(Q, np.longdouble)[:, :3]).max()) for Q in PP]
    return (int(np.argmin(d)) if d else -1), d


# ---- the seeded cases of the tests -----------------------------------------------------------------------------------

THR = 2e-3                                   # normalised units: 3 px of 5 um at f = 7.5 mm
OUTLIERS = 0.3


def draw(n, k, rng):
    """k rows of three distinct indices below n (the tests' own generator; dbat_amd.initial.draw_triples is the product's)."""
    return np.array([rng.choice(n, 3, replace=False) for _ in range(k)], np.int32).reshape(k, 3)


def seeded_case(seed, n, n_samples, shift=None):
    """The camera of resect_ref.seeded_case(seed, npt=n), noise-free, with 30 % of the image points (rounded down; none for
    n < 5) moved by 0.05 .. 0.3 in a random direction, and n_samples triples from
    np.random.default_rng(5000 + seed)."""
    c = rf.seeded_case(seed, npt=n, shift=shift)
    rng = np.random.default_rng(5000 + seed)
    x = np.array(c['x'])
    n_out = int(OUTLIERS * n) if n >= 5 else 0
    out = np.sort(rng.choice(n, n_out, replace=False))
    ang = rng.uniform(0, 2 * np.pi, n_out)
    x[:, out] += rng.uniform(0.05, 0.3, n_out) * np.stack([np.cos(ang), np.sin(ang)])
    return dict(X=c['X'], x=x, outliers=out, samples=draw(n, n_samples, rng), thr2=THR ** 2, R=c['R'], C=c['C'], seed=seed, n=n)
