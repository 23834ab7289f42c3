"""NumPy restatement of the forward-intersection RANSAC of dbat_hip_intersect_ransac (csrc/intersect_ransac.hpp), for
tests only.  A hypothesis is the middle of the common perpendicular of two rays of the point (centre -R' t, direction
R' (x0, x1, 1), normalised); it is scored only if both rays may be used, |d1 x d2|^2 >= max(sin^2 min_angle, 1e-24) and
the point is finite.  A ray is an inlier if it may be used, the point lies in front of its camera (third row of P [X; 1]
negative) and e0^2 + e1^2 <= thr2[cam].  The winner has the most inliers -- of equal counts the lowest sample -- and at
least two.  A point without samples has its pairs i < j enumerated lexicographically.  Shares no code with dbat_amd/.

Two routes: dtype np.longdouble and dtype float, every quantity in the dtype.  The seeds of the tests are chosen so that
both pick the same winner and no comparison is closer than 1e-9 relative (tests/test_intersect_robust_cpu.py)."""
import numpy as np

MIN_INLIERS = 2
PARALLAX2 = 1e-24
MAX_EXHAUSTIVE = 64


def pairs(r):
    """All pairs i < j of r rays in lexicographic order (k x 2)."""
    return np.array([(i, j) for i in range(r) for j in range(i + 1, r)], np.int32).reshape(-1, 2)


def pair_number(i, j, r):
    return i * (2 * r - i - 1) // 2 + (j - i - 1)


def rays(P, cam, xn, dtype):
    """(centres 3 x r, unit directions 3 x r) of the rays in dtype."""
    Pr = np.asarray(P, dtype).reshape(-1, 3, 4)[np.asarray(cam, int)]
    R, t = Pr[:, :, :3], Pr[:, :, 3]
    x = np.asarray(xn, dtype)
    C = -np.einsum('rji,rj->ir', R, t)
    with np.errstate(all='ignore'):
        d = np.einsum('rji,jr->ir', R, np.vstack([x, np.ones((1, x.shape[1]), dtype)]))
        d = d / np.sqrt(np.sum(d * d, 0))
    return C, d


def midpoint(c1, d1, c2, d2):
    """(the middle of the common perpendicular, |d1 x d2|^2)."""
    cx = np.cross(d1, d2)
    s2 = cx @ cx
    b = c2 - c1
    c = d1 @ d2
    r1, r2 = d1 @ b, d2 @ b
    with np.errstate(all='ignore'):
        al1, al2 = (r1 - c * r2) / s2, (c * r1 - r2) / s2
        return c1 + (al1 * d1 + b + al2 * d2) / 2, s2


def residuals2(P, cam, xn, X, dtype):
    """(e0^2 + e1^2, the third row of P [X; 1], |P [X; 1]|) of every ray, in dtype."""
    Pr = np.asarray(P, dtype).reshape(-1, 3, 4)[np.asarray(cam, int)]
    with np.errstate(all='ignore'):
        h = Pr[:, :, :3] @ np.asarray(X, dtype) + Pr[:, :, 3]
        e = h[:, :2] / h[:, 2:3] - np.asarray(xn, dtype).T
        return np.sum(e * e, 1), h[:, 2], np.sqrt(np.sum(h * h, 1))


def ransac(cam, xn, P, thr2, samples=None, use=None, min_angle=0.0, dtype=np.longdouble):
    """One point: cam (r), xn 2 x r, P n_cams x 3 x 4, thr2 per camera, samples k x 2 or None / empty (every pair).
    dict(X (3 of dtype, or None), count, sample, scored, usable, mask, ssq, e2 (per scored hypothesis: (sample, count, the
    squared residuals over thr2 of the usable rays in front)), z (per scored hypothesis: (sample, the third row of P [X; 1]
    over |P [X; 1]| and the squared residual over thr2 of every usable ray)), s2 (|d1 x d2|^2 of every sample whose rays
    may be used), samples)."""
    cam = np.asarray(cam, int).reshape(-1)
    r = cam.size
    xn = np.asarray(xn, float).reshape(2, r)
    use = np.ones(r, bool) if use is None else np.asarray(use, bool)
    if samples is None or len(samples) == 0:
        samples = pairs(r) if r <= MAX_EXHAUSTIVE else np.zeros((0, 2), np.int32)
    samples = np.asarray(samples, int).reshape(-1, 2)
    t2 = np.broadcast_to(np.asarray(thr2, float), (np.asarray(P).reshape(-1, 3, 4).shape[0],))[cam]
    par2 = max(float(np.sin(dtype(min_angle)) ** 2), PARALLAX2)
    C, d = rays(P, cam, np.where(use, xn, 0.0), dtype) if r else (np.zeros((3, 0), dtype), np.zeros((3, 0), dtype))
    best = (0, -1, None)
    scored, e2_all, s2_all, z_all = 0, [], [], []
    for k, (i, j) in enumerate(samples):
        if not (use[i] and use[j]):
            continue
        X, s2 = midpoint(C[:, i], d[:, i], C[:, j], d[:, j])
        s2_all.append(s2)
        if not (s2 >= par2 and np.all(np.isfinite(X))):
            continue
        e2, z, hn = residuals2(P, cam, xn, X, dtype)
        front = use & (z < 0)
        cnt = int((front & (e2 <= t2)).sum())
        scored += 1
        e2_all.append((k, cnt, e2[front] / t2[front]))
        with np.errstate(all='ignore'):
            z_all.append((k, z[use] / hn[use], e2[use] / t2[use]))
        if cnt >= MIN_INLIERS and cnt > best[0]:          # ascending samples: a later one only if strictly larger
            best = (cnt, k, X)
    mask = np.zeros(r, bool)
    ssq = 0.0
    if best[2] is not None:
        e2, z, _ = residuals2(P, cam, xn, best[2], dtype)
        mask = use & (z < 0) & (e2 <= t2)
        ssq = float(np.sum(e2[mask]))
    return dict(X=best[2], count=best[0], sample=best[1], scored=scored, usable=int(use.sum()), mask=mask, ssq=ssq, e2=e2_all,
                s2=np.array(s2_all, dtype), z=z_all, samples=samples, par2=par2)


# ---- the seeded cases of the tests -----------------------------------------------------------------------------------

THR = 2e-3                                   # normalised units: 3 px of 5 um at f = 7.5 mm
NOISE = 1e-4


def draw(r, k, rng):
    """k rows of two distinct indices below r (the tests' own generator; dbat_amd.initial.draw_pairs is the product's)."""
    return np.array([rng.choice(r, 2, replace=False) for _ in range(k)], np.int32).reshape(k, 2)


def seeded_case(seed, r, n_samples=0, n_out=None, shift=None):
    """A point of pointadjust_ref.seeded_case's scene seen by r rays (camera k mod 12, so from 13 rays on cameras see it
    twice) with NOISE on every coordinate, n_out of them (default: 1 .. 3, none below 4 rays) replaced by rays to a wrong
    place 1 .. 3 away, and n_samples pairs from np.random.default_rng(13000 + seed) (0: every pair, enumerated)."""
    import pointadjust_ref as pr
    P, C = pr.cameras(0, shift=shift)
    rng = np.random.default_rng(13000 + seed)
    cam = (np.arange(r) * 5 + int(rng.integers(pr.N_CAMS))) % pr.N_CAMS
    sh = 0 if shift is None else np.asarray(shift, float)
    Xt = rng.uniform(-2, 2, 3) + sh
    x = pr.project(P, cam, Xt)[0] + NOISE * rng.standard_normal((2, r))
    n_out = (min(int(rng.integers(1, 4)), r - 3) if r >= 4 else 0) if n_out is None else n_out
    out = np.sort(rng.choice(r, n_out, replace=False))
    for q in out:
        dirn = rng.standard_normal(3)
        wrong = Xt + rng.uniform(1, 3) * dirn / np.linalg.norm(dirn)
        x[:, q] = pr.project(P, cam[q:q + 1], wrong)[0][:, 0]
    samples = draw(r, n_samples, rng) if n_samples else np.zeros((0, 2), np.int32)
    thr2 = THR ** 2 * np.random.default_rng(13000).uniform(0.8, 1.25, pr.N_CAMS)      # per camera, the same for every seed
    return dict(cam=cam, x=x, P=P, X=Xt, outliers=out, samples=samples, thr2=thr2, r=r, seed=seed, shift=shift)


def run_case(c, dtype=np.longdouble, **kw):
    return ransac(c['cam'], c['x'], c['P'], c['thr2'], c['samples'], dtype=dtype, **kw)
