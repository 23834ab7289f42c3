"""Initial values for the bundle: spatial resection of the camera stations from
control points and forward intersection of the object points, on the device.

  resect        -> dbat_hip_resect (csrc/resect.hpp k_resect: one wave per image solves the quartics of the
                   candidate triangles and scores the poses); the host keeps what resect.m does with MATLAB
                   built-ins around it: lens correction, the choice of the triangles, centre / angles from the
                   winning 3 x 4 matrix                                  (photogrammetry/resect.m:42-131)
  forwintersect -> dbat_hip_forwintersect (k_forwintersect)              (photogrammetry/forwintersect.m:19-46)
  essmat5       -> dbat_hip_essmat5 (csrc/relorient.hpp k_essmat5)       (photogrammetry/essmat5.m:9-43)
  camsfrome, relorient, relorient_pairs -> dbat_hip_relorient (k_essmat5, k_ro_score, k_ro_cams): relative orientation
                   of image pairs without control points or EO -- a five-point RANSAC over samples drawn here, the
                   camera pair and the points of the winner                (photogrammetry/camsfrome.m:16-59)
  refine_pairs, relorient(refine=True) -> dbat_hip_pairadjust (csrc/pairadjust.hpp k_pairadjust): the least-squares
                   relative orientation of the pairs, one workgroup per pair; the reference refines a pair only through
                   bundle.m on a two-image project
  resect_robust, draw_triples -> dbat_hip_resect_ransac (csrc/resect_ransac.hpp k_resect_ransac: one workgroup per camera, a
                   RANSAC over triples of control points scored by inlier count) and dbat_hip_poseadjust
                   (csrc/poseadjust.hpp k_poseadjust: the least-squares space resection on the winner's inliers, one wave
                   per camera); the reference has neither
  forwintersect_robust, draw_pairs -> dbat_hip_intersect_ransac (csrc/intersect_ransac.hpp k_intersect_ransac: one wave per
                   object point, a RANSAC over pairs of its image rays scored by inlier count) and dbat_hip_pointadjust
                   (csrc/pointadjust.hpp k_pointadjust: the least-squares intersection on the winner's inliers, eight lanes
                   per point); no handle; the reference has neither
  largesttriangle (misc/largesttriangle.m:16-41), derotmat3d (photogrammetry/derotmat3d.m:17-19), rotmat3d (its inverse),
  lenscorr1 (bundle/cammodel/pm_multilenscorr1.m:45-69 + pm_lens1.m:36-72), cleareo, clearop (misc/)

The CPU restatements these are tested against live in oracle/initial_oracle.py.
"""
from itertools import combinations

import numpy as np

def cleareo(s):
    """Set every EO parameter that is estimated and has no prior observation
    to NaN (misc/cleareo.m)."""
    s.EO.val[:s.bundle.est.EO.shape[0]][s.bundle.est.EO & ~s.prior.EO.use] = np.nan
    return s

def clearop(s):
    """Set every OP coordinate that is estimated and has no prior
    observation to NaN (misc/clearop.m)."""
    s.OP.val[s.bundle.est.OP & ~s.prior.OP.use] = np.nan
    return s

def lenscorr1(s):
    """Measured image points in mm (y up), corrected for lens distortion with
    the backward Brown polynomial in the measured point, as
    pm_multilenscorr1.m:45-69 does it for every distortion model (the
    aspect/skew terms are ignored there as well, pm_multilenscorr1.m:161)."""
    nK, nP = s.IO.model.nK, s.IO.model.nP
    cam = s.IP.cam
    IO = s.IO.val[:, cam]
    px = s.IO.sensor.pxSize[:, cam]
    if getattr(s.IO.sensor, 'samePxSize', False):
        px = np.tile(s.IO.sensor.pxSize[0, cam], (2, 1))     # U=sensor.pxSize(1)
    q = np.stack([px[0] * s.IP.val[0], -px[1] * s.IP.val[1]])
    xb, yb = q[0] - IO[1], q[1] - IO[2]
    r2 = xb * xb + yb * yb
    Kr = np.zeros_like(r2)
    pw = np.ones_like(r2)
    for j in range(nK):
        pw = pw * r2
        Kr = Kr + IO[5 + j] * pw
    dx, dy = xb * Kr, yb * Kr
    if nP >= 2:
        P1, P2 = IO[5 + nK], IO[6 + nK]
        P3 = 1 + IO[7 + nK] if nP > 2 else 1.0
        dx = dx + (P1 * (r2 + 2 * xb * xb) + 2 * P2 * xb * yb) * P3
        dy = dy + (P2 * (r2 + 2 * yb * yb) + 2 * P1 * xb * yb) * P3
    return np.stack([q[0] - dx, q[1] - dy])

def _hull(pts):
    """Indices of the points on the convex hull of a 2-by-n point set
    (sorted), standing in for convhulln (largesttriangle.m:20)."""
    n = pts.shape[1]
    if n <= 3:
        return list(range(n))
    order = sorted(range(n), key=lambda i: (pts[0, i], pts[1, i]))

    def half(seq):
        h = []
        for i in seq:
            while len(h) >= 2:
                a, b = pts[:, h[-2]], pts[:, h[-1]]
                if (b[0] - a[0]) * (pts[1, i] - a[1]) - (b[1] - a[1]) * (pts[0, i] - a[0]) <= 0:
                    h.pop()
                else:
                    break
            h.append(i)
        return h
    return sorted(set(half(order)) | set(half(order[::-1])))

def largesttriangle(pts, cHull=True):
    """All point triplets (rows of T, 0-based) sorted by descending area A
    (largesttriangle.m:16-41)."""
    idx = _hull(pts) if cHull else list(range(pts.shape[1]))
    T = np.array(list(combinations(idx, 3)), int).reshape(-1, 3)
    x, y = pts[0][T], pts[1][T]
    A = 0.5 * np.abs(x[:, 0] * (y[:, 1] - y[:, 2]) + x[:, 1] * (y[:, 2] - y[:, 0])
                     + x[:, 2] * (y[:, 0] - y[:, 1]))
    o = np.argsort(-A, kind='stable')
    return T[o], A[o]

def derotmat3d(M):
    """omega, phi, kappa of a world-to-camera rotation (derotmat3d.m:17-19)."""
    return np.array([np.arctan2(-M[2, 1], M[2, 2]), np.arcsin(M[2, 0]),
                     np.arctan2(-M[1, 0], M[0, 0])])

def rotmat3d(ang):
    """World-to-camera rotation M' of omega, phi, kappa (pm_eulerrotmat: the transpose of eulerrotmat.m:81, sequence
    123, moving axes); derotmat3d(rotmat3d(ang)) returns ang."""
    so, co, sp, cp, sk, ck = (f(float(a)) for a in ang for f in (np.sin, np.cos))
    return np.array([[cp * ck, co * sk + so * sp * ck, so * sk - co * sp * ck],
                     [-cp * sk, co * ck - so * sp * sk, so * ck + co * sp * sk],
                     [sp, -so * cp, co * cp]])

def resect(s0, cams='all', cpId=None, n=1, v=0.0, chkId=None, device=0):
    """Spatial resection of the listed camera stations from the control points with ids cpId; returns
    (s, rms, fail) as resect.m:1 does (rms = Inf for a station without a pose, resect.m: bestRes=inf).  The
    per-camera work runs on the GPU (dbat_hip_resect: one wave per camera solves the quartics of the candidate
    triangles and scores the poses against the check points chkId -- default: every object point).  Of the
    triangles of control points seen by a camera, the n largest in the image with at least v times the largest
    area are tried."""
    from . import _hip
    from .dbatstruct import copy_struct
    s = copy_struct(s0)
    nc = s0.EO.val.shape[1]
    cams = list(range(nc)) if isinstance(cams, str) and cams == 'all' else list(cams)
    cpId = np.asarray(cpId)
    chkId = s0.OP.id if chkId is None else np.asarray(chkId)
    keepId = np.union1d(cpId, chkId)
    xy = lenscorr1(s0)
    pt_start, tri_start, Xs, xs, tris = [0], [0], [], [], []
    for ci in cams:
        IO = s0.IO.val[:, ci]
        rows = np.flatnonzero(s0.IP.cam == ci)
        ids = s0.OP.id[s0.IP.pt[rows]]
        is_cp = np.isin(ids, cpId)
        if np.count_nonzero(is_cp) > 3:
            T, A = largesttriangle(xy[:, rows[is_cp]])
            take = (np.arange(len(A)) < n) & (A >= v * A[0])
            tryId = ids[is_cp][T[take]]
        elif np.count_nonzero(is_cp) == 3:
            tryId = ids[is_cp][None, :]
        else:
            tryId = np.zeros((0, 3), int)
        keep = np.isin(ids, keepId)
        pt2 = xy[:, rows[keep]]
        xs.append(np.stack([(pt2[0] - IO[1]) / -IO[0], (pt2[1] - IO[2]) / -IO[0]]))   # K\homogeneous(pt2)
        Xs.append(s0.OP.val[:, s0.IP.pt[rows[keep]]])
        visId = ids[keep]
        for useId in tryId:          # pm_resect_3pt takes the three points in the order they are seen (use mask)
            tris.append(np.flatnonzero(np.isin(visId, useId)))
        pt_start.append(pt_start[-1] + int(np.count_nonzero(keep)))
        tri_start.append(len(tris))
    for t in tris:
        if len(t) != 3:
            raise ValueError('Can only use 3 points for resection')
    P, rms = _hip.resect_poses(pt_start, np.concatenate(Xs, 1) if Xs else np.zeros((3, 0)),
                               np.concatenate(xs, 1) if xs else np.zeros((2, 0)), tri_start,
                               np.array(tris, np.int32).reshape(-1, 3), device=device)
    fail = False
    for k, ci in enumerate(cams):
        if np.all(np.isfinite(P[k])):
            nv = np.linalg.svd(P[k])[2][-1]          # euclidean(null(P)), as resect() above
            s.EO.val[:3, ci] = nv[:3] / nv[3]
            s.EO.val[3:6, ci] = derotmat3d(P[k][:, :3])
        else:
            fail = True
            s.EO.val[:6, ci] = np.nan
    return s, rms, fail

def forwintersect(s0, ids='all', skipPrior=False, device=0):
    """Object points by forward intersection of the lens-corrected image rays: the point minimising the summed
    squared distance to its rays (pm_forwintersect3.m:55-82), the per-point 3 x 3 systems built and solved on
    the GPU (dbat_hip_forwintersect: one lane per image ray in the point-major batches of the bundle core).
    Points seen from fewer than two stations become NaN (pm_multiforwintersect.m:41).  With skipPrior, points
    that are fixed or carry prior observations keep their values (forwintersect.m:32-36)."""
    from . import _hip
    from .dbatstruct import copy_struct
    if not np.all(np.isfinite(s0.EO.val)):
        raise ValueError('Bad or uninitialized EO data')
    if not np.all(np.isfinite(s0.IO.val)):
        raise ValueError('Bad or uninitialized IO data')
    s = copy_struct(s0)
    npnt = s0.OP.val.shape[1]
    do = np.ones(npnt, bool) if isinstance(ids, str) and ids == 'all' else np.isin(s0.OP.id, ids)
    if skipPrior:
        do &= np.all(s0.bundle.est.OP, 0) & ~np.any(s0.prior.OP.use, 0)
    h = _hip.Handle(s0, device=device)
    try:
        s.OP.val = h.forwintersect(h.serialize(), s0.OP.val, skip=~do)
    finally:
        h.close()
    return s

# ---- relative orientation ----------------------------------------------------------------------------------------------

def essmat5(Q1, Q2, device=0):
    """EE = essmat5(Q1, Q2) (photogrammetry/essmat5.m): the essential matrices of n >= 5 correspondences, Q1 and Q2
    3-by-n normalised homogeneous coordinates, as a 9-by-k array (k <= 10) of unit columns, on the device
    (dbat_hip_essmat5).  Layout of the reference (essmat5.m:12-20): a column e satisfies
    sum e[a + 3 b] Q1[a, i] Q2[b, i] = 0, so e.reshape(3, 3) (row-major) is the E with Q2' E Q1 = 0 -- the matrix
    camsfrome(E, Q1, Q2, ...) expects.  Real solutions only, in ascending order of the root."""
    from . import _hip
    Q1 = np.asarray(Q1, float)
    E, ns = _hip.essmat5_sets([0, Q1.shape[1] if Q1.ndim == 2 else 0], Q1, Q2, device=device)
    return E[0, :ns[0]].T.copy()


def camsfrome(E, x, xp, frontDir, device=0):
    """[P1,P2,X,inFront,sp] = camsfrome(E, x, xp, frontDir) (photogrammetry/camsfrome.m): the camera pair [I | 0],
    [R | t] (|t| = 1) of the 3-by-3 essential matrix E with xp' E x = 0, x and xp 3-by-n normalised homogeneous points in
    image 1 and 2, the points X (4-by-n, homogeneous, in the frame of P1) by intersection of the rays, whether each is in
    front of both cameras (frontDir = +1 / -1: the sign of z in front), and the sorted in-front counts sp of the four
    candidates, on the device (dbat_hip_relorient with E as the only model: one sample is not drawn, E is scored as it
    is).  A point of two parallel rays is never in front."""
    from . import _hip
    E, x, xp = np.asarray(E, float), np.asarray(x, float), np.asarray(xp, float)
    if E.shape != (3, 3) or x.ndim != 2 or x.shape[0] != 3 or x.shape != xp.shape:
        raise ValueError('camsfrome: E must be 3-by-3, x and xp 3-by-n')
    r = _hip.cams_from_e(E.reshape(-1), x[:2] / x[2], xp[:2] / xp[2], int(np.sign(frontDir)), device=device)
    n = x.shape[1]
    return np.eye(3, 4), r['P2'], np.vstack([r['X'], np.ones((1, n))]), r['in_front'], r['sp']


def draw_samples(n, n_hyp, rng):
    """n_hyp rows of five distinct indices below n >= 5 from the generator rng: rows with a repeated index are drawn
    again until none is left (n < 16: the head of a permutation per row)."""
    n, n_hyp = int(n), int(n_hyp)
    if n < 5:
        raise ValueError('draw_samples: fewer than five correspondences')
    if n < 16:
        return np.array([rng.permutation(n)[:5] for _ in range(n_hyp)], np.int32).reshape(n_hyp, 5)
    S = rng.integers(0, n, (n_hyp, 5))
    while True:
        srt = np.sort(S, 1)
        bad = np.flatnonzero(np.any(srt[:, 1:] == srt[:, :-1], 1))
        if bad.size == 0:
            return S.astype(np.int32)
        S[bad] = rng.integers(0, n, (bad.size, 5))


def pair_points(s, i, j, xy=None):
    """(pts, x1, x2) of the image pair (i, j), lens-corrected with lenscorr1 (xy: its result, if at hand): the object points seen in both images i and j (columns of OP, ascending) and their lens-corrected image points
    normalised as resect() does: K \\ [x; y; 1] with -f, so that the cameras look along -z (frontDir = -1)."""
    xy = lenscorr1(s) if xy is None else xy
    ri, rj = np.flatnonzero(s.IP.cam == i), np.flatnonzero(s.IP.cam == j)
    common, ai, aj = np.intersect1d(s.IP.pt[ri], s.IP.pt[rj], return_indices=True)
    out = []
    for cam, rows in ((i, ri[ai]), (j, rj[aj])):
        IO = s.IO.val[:, cam]
        out.append(np.stack([(xy[0, rows] - IO[1]) / -IO[0], (xy[1, rows] - IO[2]) / -IO[0]]))
    return common, out[0], out[1]


def pair_threshold(s, i, j, thr_px):
    """thr_px pixels in normalised units: the mean over the two images of pixel size / focal length."""
    u = [np.mean(s.IO.sensor.pxSize[:, c]) / abs(s.IO.val[0, c]) for c in (i, j)]
    return float(thr_px) * 0.5 * (u[0] + u[1])


def relorient_pairs(s, pairs, n_hyp=512, thr_px=3.0, seed=0, device=0):
    """Relative orientation of the image pairs (i, j) of `pairs` in one device call (dbat_hip_relorient); s is not
    touched.  Per pair the object points seen in both images are lens-corrected (lenscorr1) and normalised as resect()
    does (with -f: the cameras look along -z, frontDir = -1), n_hyp samples of five are drawn with
    np.random.default_rng(seed) (draw_samples, pair after pair from the one generator), and the RANSAC winner -- the
    model with the most points whose Sampson distance is below thr_px pixels -- is decomposed.  There is no refit of the
    winner on its inliers: bundle() is the refinement.  Returns a list of info per pair with
      pts       the common object points (columns of s.OP.val)      samples   the samples drawn (n_hyp, 5)
      E         3-by-3, x_j' E x_i = 0 (what camsfrome expects; the device returns the layout of essmat5, its transpose
                as a column-major 3-by-3, and this function does the transposition)
      P2        [R | t], |t| = 1: x_j ~ R X + t for X in the frame of image i       X   3-by-n, frame of image i
      inlier, in_front   masks over pts      count     inliers      models    models scored
      sample, sol        the winning sample (row of samples) and solution, -1 without one
      sp        the four in-front counts, descending
      ok        a model was found and sp[0] > sp[1] strictly
    BadInput (ValueError) for a pair with fewer than five common points."""
    from . import _hip
    xy = lenscorr1(s)
    rng = np.random.default_rng(seed)
    pt_start, hyp_start, x1s, x2s, smps, thr2, pts = [0], [0], [], [], [], [], []
    for i, j in pairs:
        common, a, b = pair_points(s, int(i), int(j), xy)
        if common.size < 5:
            raise ValueError('relorient: images %d and %d share fewer than five points' % (i, j))
        pts.append(common); x1s.append(a); x2s.append(b)
        smps.append(draw_samples(common.size, n_hyp, rng))
        thr2.append(pair_threshold(s, int(i), int(j), thr_px) ** 2)
        pt_start.append(pt_start[-1] + common.size)
        hyp_start.append(hyp_start[-1] + int(n_hyp))
    if not pts:
        return []
    r = _hip.relorient_pairs(pt_start, np.concatenate(x1s, 1), np.concatenate(x2s, 1), hyp_start, np.concatenate(smps, 0),
                             thr2, -1, device=device)
    out = []
    for k in range(len(pts)):
        sl = slice(pt_start[k], pt_start[k + 1])
        st = r['stats'][k]
        out.append(dict(pts=pts[k], samples=smps[k], E=r['E'][k].reshape(3, 3).copy(), P2=r['P2'][k].copy(), X=r['X'][:, sl].copy(),
                        inlier=r['inlier'][sl].copy(), in_front=r['in_front'][sl].copy(), count=int(st[0]), sample=int(st[1]),
                        sol=int(st[2]), models=int(st[3]), sp=st[4:8].copy(), ok=bool(st[1] >= 0 and st[4] > st[5])))
    return out


def pair_weights(s, i, j):
    """(w1, w2), 2-by-n each: the reciprocal standard deviations of the image points of pair_points(s, i, j) in its
    normalised units, |f_c| / (pxSize[axis, c] IP.std[axis, column]), with one pixel size for both axes where the sensor
    says samePxSize (as lenscorr1 takes it)."""
    ri, rj = np.flatnonzero(s.IP.cam == i), np.flatnonzero(s.IP.cam == j)
    _, ai, aj = np.intersect1d(s.IP.pt[ri], s.IP.pt[rj], return_indices=True)
    out = []
    for cam, rows in ((i, ri[ai]), (j, rj[aj])):
        px = np.asarray(s.IO.sensor.pxSize, float)[:, cam]
        if getattr(s.IO.sensor, 'samePxSize', False):
            px = np.array([px[0], px[0]])
        out.append(abs(s.IO.val[0, cam]) / (px[:, None] * np.asarray(s.IP.std, float)[:, rows]))
    return out[0], out[1]


def refine_pairs(s, pairs, infos, max_iter=20, conv_tol=1e-6, min_angle_deg=0.0, device=0):
    """Least-squares refinement of the relative orientations infos = relorient_pairs(s, pairs, ...): per pair a two-view
    bundle adjustment over R, t (|t| = 1, image i at the origin) and the points, all pairs with info['ok'] in one device
    call (dbat_hip_pairadjust; include/dbat_hip.h has the algorithm); s is not touched.  The correspondences that are
    inliers and in front may be used, with the weights of pair_weights.  min_angle_deg leaves out the correspondences
    whose two rays meet at less: such a point is not determined along its ray, and under the iteration it runs towards
    infinity and keeps the pair from converging.  It is off by default -- which angle is too small depends on the
    noise, and no value has been measured on real projects; a pair without a baseline is not repaired by it and ends
    with a code other than 0.  Returns a list of dict per pair with
      P2, X (3-by-n), used       as relorient_pairs; X of a point that is not used is the given one
      sigma0, f0, f              sqrt(f / (n_used - 5)), the weighted sum of squares at the start and at the end
      iters, trials, code, ok    accepted steps, trials, 0 converged / 1 max_iter / 2 no step / 3 singular / 4 fewer than
                                 five points or not info['ok'] (nothing is refined: P2 and X are those of info); ok: code 0
      Q, cov                     6-by-6 cofactor and covariance sigma0^2 Q of the rotation vector a (R <- exp([a]x) R) and t
      res                        2-by-2-by-n weighted residuals (image, axis), zero where not used
    The lens correction is applied to the measurements (lenscorr1), not to the projections: with distortion the
    objective is that of bundle() to first order only."""
    from . import _hip
    pairs, infos = list(pairs), list(infos)
    if len(pairs) != len(infos):
        raise ValueError('refine_pairs: one info per pair')
    nan = np.nan
    out = [dict(P2=np.array(f['P2'], float), X=np.array(f['X'], float), used=np.zeros(f['X'].shape[1], bool), sigma0=nan, f0=nan, f=nan,
                iters=0, trials=0, code=4, ok=False, Q=np.full((6, 6), nan), cov=np.full((6, 6), nan), res=np.zeros((2, 2, f['X'].shape[1])))
           for f in infos]
    todo = [k for k, f in enumerate(infos) if f['ok']]
    if not todo:
        return out
    xy = lenscorr1(s)
    pt_start, x1s, x2s, w1s, w2s = [0], [], [], [], []
    for k in todo:
        i, j = int(pairs[k][0]), int(pairs[k][1])
        common, a, b = pair_points(s, i, j, xy)
        if not np.array_equal(common, infos[k]['pts']):
            raise ValueError('refine_pairs: info %d is not that of the pair (%d, %d) of s' % (k, i, j))
        w1, w2 = pair_weights(s, i, j)
        x1s.append(a); x2s.append(b); w1s.append(w1); w2s.append(w2)
        pt_start.append(pt_start[-1] + common.size)
    X0 = np.concatenate([infos[k]['X'] for k in todo], 1)
    use = np.concatenate([infos[k]['inlier'] & infos[k]['in_front'] for k in todo])
    r = _hip.pairadjust(pt_start, np.concatenate(x1s, 1), np.concatenate(x2s, 1), np.stack([infos[k]['P2'] for k in todo]),
                        np.where(use, X0, 0.0), use=use, w1=np.concatenate(w1s, 1), w2=np.concatenate(w2s, 1), front_dir=-1,
                        max_iter=max_iter, conv_tol=conv_tol, min_angle=np.deg2rad(min_angle_deg), residuals=True, device=device)
    for m, k in enumerate(todo):
        sl = slice(pt_start[m], pt_start[m + 1])
        used = r['used'][sl].copy()
        s0 = float(r['sigma0'][m])
        out[k] = dict(P2=r['P2'][m].copy(), X=np.where(used, r['X'][:, sl], infos[k]['X']), used=used, sigma0=s0, f0=float(r['f0'][m]),
                      f=float(r['f'][m]), iters=int(r['iters'][m]), trials=int(r['trials'][m]), code=int(r['code'][m]),
                      ok=bool(r['code'][m] == 0), Q=r['Q'][m].copy(), cov=s0 * s0 * r['Q'][m], res=r['res'][:, :, sl].copy())
        if out[k]['code'] == 4:
            out[k]['P2'] = np.array(infos[k]['P2'], float)
    return out


def relorient(s0, i, j, n_hyp=512, thr_px=3.0, seed=0, device=0, refine=False, max_iter=20, conv_tol=1e-6, min_angle_deg=0.0):
    """Initial values for the image pair (i, j) of a network without control points or EO: (s, ok, info).  info is that
    of relorient_pairs(s0, [(i, j)], ...).  In s -- a copy -- the EO of image i is the origin with zero angles, the EO of
    image j comes from P2 = [R | t] (centre -R' t, a baseline of length one; omega, phi, kappa of R, as resect() takes
    them), the OP of the common points in front of both cameras are their intersections X, and every other OP is NaN
    (the frame is new: no other point has coordinates in it; forwintersect() fills them once more images are oriented).
    The EO of the other images are left as they are.  ok = False, and s is s0 itself, when no sample gave a model or the
    best of the four camera candidates does not have strictly more points in front than the next (sp[0] > sp[1]): a
    pair without a baseline, for one.
    refine: the winner is refined by least squares (refine_pairs with max_iter, conv_tol, min_angle_deg) and
    info['refined'] is its result.  Where that ends with code 0, the EO of image j and the OP of the points it used come
    from the refined values (a point in front that it did not use keeps its intersection); with any other code the
    unrefined values stand and info['refined']['code'] says why."""
    from .dbatstruct import copy_struct
    info = relorient_pairs(s0, [(i, j)], n_hyp=n_hyp, thr_px=thr_px, seed=seed, device=device)[0]
    if not info['ok']:
        return s0, False, info
    P2, X = info['P2'], info['X']
    if refine:
        ref = refine_pairs(s0, [(i, j)], [info], max_iter=max_iter, conv_tol=conv_tol, min_angle_deg=min_angle_deg, device=device)[0]
        info['refined'] = ref
        if ref['ok']:
            P2, X = ref['P2'], ref['X']
    s = copy_struct(s0)
    R, t = P2[:, :3], P2[:, 3]
    s.EO.val[:6, i] = 0.0
    s.EO.val[:3, j] = -R.T @ t
    s.EO.val[3:6, j] = derotmat3d(R)
    s.OP.val[:] = np.nan
    f = info['in_front']
    s.OP.val[:, info['pts'][f]] = X[:, f]
    return s, True, info


# ---- robust resection --------------------------------------------------------------------------------------------------

def draw_triples(n, n_hyp, rng):
    """n_hyp rows of three distinct indices below n >= 3 from the generator rng, by the rule of draw_samples: rows with a
    repeated index are drawn again until none is left (n < 16: the head of a permutation per row)."""
    n, n_hyp = int(n), int(n_hyp)
    if n < 3:
        raise ValueError('draw_triples: fewer than three points')
    if n < 16:
        return np.array([rng.permutation(n)[:3] for _ in range(n_hyp)], np.int32).reshape(n_hyp, 3)
    S = rng.integers(0, n, (n_hyp, 3))
    while True:
        srt = np.sort(S, 1)
        bad = np.flatnonzero(np.any(srt[:, 1:] == srt[:, :-1], 1))
        if bad.size == 0:
            return S.astype(np.int32)
        S[bad] = rng.integers(0, n, (bad.size, 3))


def camera_points(s, ci, cpId=None, xy=None):
    """(rows, xn, w) of camera ci: the columns of IP of its image points whose object point has an id in cpId (default:
    every object point) and finite coordinates, their lens-corrected coordinates normalised as resect() does (K \\ [x; y; 1]
    with -f), and their weights in these units as pair_weights computes them, |f| / (pxSize[axis] IP.std[axis, column])."""
    xy = lenscorr1(s) if xy is None else xy
    rows = np.flatnonzero(s.IP.cam == ci)
    keep = np.all(np.isfinite(s.OP.val[:, s.IP.pt[rows]]), 0)
    if cpId is not None:
        keep &= np.isin(s.OP.id[s.IP.pt[rows]], cpId)
    rows = rows[keep]
    IO = s.IO.val[:, ci]
    xn = np.stack([(xy[0, rows] - IO[1]) / -IO[0], (xy[1, rows] - IO[2]) / -IO[0]])
    px = np.asarray(s.IO.sensor.pxSize, float)[:, ci]
    if getattr(s.IO.sensor, 'samePxSize', False):
        px = np.array([px[0], px[0]])
    return rows, xn, abs(IO[0]) / (px[:, None] * np.asarray(s.IP.std, float)[:, rows])


def resect_robust(s0, cams='all', cpId=None, n_hyp=256, thr_px=3.0, seed=0, refine=True, reselect=0, max_iter=20, conv_tol=1e-6,
                  device=0):
    """Robust spatial resection of the listed camera stations: (s, info, fail).  Per camera the image points of the object
    points with ids cpId (default: every object point with finite coordinates) are lens-corrected and normalised as
    resect() does, n_hyp triples are drawn with np.random.default_rng(seed) (draw_triples, camera after camera from the
    one generator), and one device call (dbat_hip_resect_ransac) solves every triple and returns the pose with the most
    points within thr_px pixels -- thr_px mean(pxSize) / |f| in normalised units.  With refine the inliers of every
    winner go through the least-squares resection (dbat_hip_poseadjust, all cameras in one call) with the weights of
    IP.std; every one of `reselect` rounds then thresholds the residuals of all the camera's points at the refined pose
    again and refines on the new inliers, where they are not fewer and the adjustment converges.  In s -- a copy -- the EO
    centre and omega, phi, kappa (derotmat3d) of the cameras come from the pose, as resect() writes them.  info[k], for
    camera cams[k]:
      ids, inlier, count   the ids of the object points considered, the mask of the inliers over them, their number
      sample               the winning triple (indices into ids), None without a winner
      P                    the 3-by-4 pose [R | -R C]
      sigma0, Q, cov       of the refinement: sqrt(f / (2 count - 6)), the 6-by-6 cofactor matrix of (centre, rotation
                           vector) and sigma0^2 Q; NaN without refine
      code, iters          of the refinement (0 converged / 1 max_iter / 2 no step / 3 singular); 0 without refine
      rms_px               the rms over the inliers of the residual in pixels
    A camera without a winner -- fewer than four points agree with any sample -- gets NaN in EO and code -1, and fail is
    True.  The lens correction is applied to the measurements (lenscorr1), not to the projections, as in refine_pairs."""
    from . import _hip
    from .dbatstruct import copy_struct
    s = copy_struct(s0)
    nc = s0.EO.val.shape[1]
    cams = list(range(nc)) if isinstance(cams, str) and cams == 'all' else [int(c) for c in cams]
    cpId = None if cpId is None else np.asarray(cpId)
    xy = lenscorr1(s0)
    rng = np.random.default_rng(seed)
    pt_start, smp_start, Xs, xs, ws, smps, thr, ids = [0], [0], [], [], [], [], [], []
    for ci in cams:
        rows, xn, w = camera_points(s0, ci, cpId, xy)
        ids.append(s0.OP.id[s0.IP.pt[rows]])
        Xs.append(s0.OP.val[:, s0.IP.pt[rows]]); xs.append(xn); ws.append(w)
        smps.append(draw_triples(rows.size, n_hyp, rng) if rows.size >= 3 else np.zeros((0, 3), np.int32))
        thr.append(float(thr_px) * np.mean(s0.IO.sensor.pxSize[:, ci]) / abs(s0.IO.val[0, ci]))
        pt_start.append(pt_start[-1] + rows.size)
        smp_start.append(smp_start[-1] + smps[-1].shape[0])
    if not cams:
        return s, [], False
    X, xn, w, thr = np.concatenate(Xs, 1), np.concatenate(xs, 1), np.concatenate(ws, 1), np.array(thr)
    r = _hip.resect_ransac(pt_start, X, xn, smp_start, np.concatenate(smps, 0), thr ** 2, device=device)
    nan = np.nan
    info = []
    for k in range(len(cams)):
        sl = slice(pt_start[k], pt_start[k + 1])
        st = r['stats'][k]
        won = st[1] >= 0
        info.append(dict(ids=ids[k], inlier=r['inlier'][sl].copy(), count=int(st[0]), sample=smps[k][st[1]].copy() if won else None,
                         P=r['P'][k].copy(), sigma0=nan, Q=np.full((6, 6), nan), cov=np.full((6, 6), nan), code=0 if won else -1, iters=0,
                         rms_px=float(np.sqrt(r['ssq'][k] / st[0])) / thr[k] * float(thr_px) if won else nan))
    todo = [k for k in range(len(cams)) if info[k]['code'] == 0]

    def adjust(which):
        """poseadjust of the cameras `which` on their current inliers, from their current poses."""
        ps = np.cumsum([0] + [pt_start[k + 1] - pt_start[k] for k in which])
        cat = lambda a: np.concatenate([a[:, pt_start[k]:pt_start[k + 1]] for k in which], 1)
        a = _hip.poseadjust(ps, cat(X), cat(xn), np.stack([info[k]['P'] for k in which]), use=np.concatenate([info[k]['inlier'] for k in which]),
                            w=cat(w), max_iter=max_iter, conv_tol=conv_tol, residuals=True, device=device)
        return a, ps

    def take(k, a, m, sl):
        """The refinement a[m] becomes the result of camera k."""
        f = info[k]
        wk = w[:, pt_start[k]:pt_start[k + 1]]
        s0k = float(a['sigma0'][m])
        e2 = np.sum((a['res'][:, sl] / wk) ** 2, 0)[a['used'][sl]]
        f.update(P=a['P'][m].copy(), inlier=a['used'][sl].copy(), count=int(a['n_used'][m]), sigma0=s0k, Q=a['Q'][m].copy(),
                 cov=s0k * s0k * a['Q'][m], code=int(a['code'][m]), iters=int(a['iters'][m]),
                 rms_px=float(np.sqrt(np.mean(e2))) / thr[k] * float(thr_px))
        f['res'] = a['res'][:, sl].copy()

    if refine and todo:
        a, ps = adjust(todo)
        for m, k in enumerate(todo):
            if a['code'][m] != 4:
                take(k, a, m, slice(ps[m], ps[m + 1]))
        for _ in range(int(reselect)):
            again = []
            for k in todo:
                f = info[k]
                if 'res' not in f:
                    continue
                sl = slice(pt_start[k], pt_start[k + 1])
                e2 = np.sum((f['res'] / w[:, sl]) ** 2, 0)
                front = f['P'][2, :3] @ X[:, sl] + f['P'][2, 3] < 0
                mask = front & (e2 <= thr[k] ** 2)
                if mask.sum() >= f['count'] and not np.array_equal(mask, f['inlier']):
                    f['_kept'] = (f['inlier'], f['count'])
                    f['inlier'] = mask
                    again.append(k)
            if not again:
                break
            a, ps = adjust(again)
            for m, k in enumerate(again):
                kept = info[k].pop('_kept')
                if a['code'][m] == 0 and a['n_used'][m] >= kept[1]:
                    take(k, a, m, slice(ps[m], ps[m + 1]))
                else:
                    info[k]['inlier'] = kept[0]
    fail = False
    for k, ci in enumerate(cams):
        f = info[k]
        f.pop('res', None)
        if f['code'] >= 0:
            R, t = f['P'][:, :3], f['P'][:, 3]
            s.EO.val[:3, ci] = -R.T @ t
            s.EO.val[3:6, ci] = derotmat3d(R)
        else:
            fail = True
            s.EO.val[:6, ci] = np.nan
    return s, info, fail


# ---- robust forward intersection ---------------------------------------------------------------------------------------

def draw_pairs(n, n_hyp, rng):
    """n_hyp rows of two distinct indices below n >= 2 from the generator rng, by the rule of draw_triples: rows with a
    repeated index are drawn again until none is left (n < 16: the head of a permutation per row)."""
    n, n_hyp = int(n), int(n_hyp)
    if n < 2:
        raise ValueError('draw_pairs: fewer than two rays')
    if n < 16:
        return np.array([rng.permutation(n)[:2] for _ in range(n_hyp)], np.int32).reshape(n_hyp, 2)
    S = rng.integers(0, n, (n_hyp, 2))
    while True:
        bad = np.flatnonzero(S[:, 0] == S[:, 1])
        if bad.size == 0:
            return S.astype(np.int32)
        S[bad] = rng.integers(0, n, (bad.size, 2))


def _pair_of_number(k, r):
    """The pair (i, j), i < j, that is number k = i (2 r - i - 1) / 2 + (j - i - 1) of the pairs of r rays (arrays)."""
    k, r = np.asarray(k, np.int64), np.asarray(r, np.int64)
    i = np.zeros_like(k)
    rest = k.copy()
    while True:
        more = rest >= r - 1 - i
        if not more.any():
            return i, i + 1 + rest
        rest = np.where(more, rest - (r - 1 - i), rest)
        i = i + more


MAX_EXHAUSTIVE_RAYS = 64                # IR_MAX_EXHAUSTIVE of csrc/intersect_ransac.hpp: rays up to which the device enumerates the pairs


def pair_plan(r, n_hyp, rng):
    """The samples of points of r rays each (an array): (ns, smp_start, smp).  A point with r (r - 1) / 2 <= n_hyp and at
    most MAX_EXHAUSTIVE_RAYS rays brings none -- ns = 0: the device enumerates its pairs --, every other point of two rays
    or more n_hyp pairs from draw_pairs(r, n_hyp, rng), point after point."""
    r = np.asarray(r, np.int64)
    heavy = np.flatnonzero((r * (r - 1) // 2 > int(n_hyp)) | (r > MAX_EXHAUSTIVE_RAYS))
    ns = np.zeros(r.size, np.int64)
    ns[heavy] = int(n_hyp)
    smp = np.concatenate([draw_pairs(r[p], n_hyp, rng) for p in heavy], 0) if heavy.size and int(n_hyp) > 0 else np.zeros((0, 2), np.int32)
    return ns, np.concatenate([[0], np.cumsum(ns)]), smp


def point_rays(s0, pts):
    """The image rays of the object points pts (columns of OP, ascending), point-major, as dbat_hip_intersect_ransac and
    dbat_hip_pointadjust take them: (cols, ray_pt, r, ray_start, cam, xn, w, thr, P) -- the columns of IP in the order of
    the points, the place in pts of every ray's point, the rays per point and their ranges, the camera of every ray, the
    lens-corrected coordinates normalised as camera_points does (K \\ [x; y; 1] with -f), the weights
    |f| / (pxSize IP.std), one pixel in normalised units per camera (mean(pxSize) / |f|) and the poses [R | -R C] of EO."""
    pts = np.asarray(pts)
    n = pts.size
    npnt = s0.OP.val.shape[1]
    ipcam, ippt = np.asarray(s0.IP.cam), np.asarray(s0.IP.pt)
    do = np.zeros(npnt, bool)
    do[pts] = True
    # the rays, point-major: the columns of IP of the chosen points in the order of the points
    sel = np.flatnonzero(do[ippt])
    cols = sel[np.argsort(ippt[sel], kind='stable')]
    where = np.full(npnt, -1)
    where[pts] = np.arange(n)
    ray_pt = where[ippt[cols]]
    r = np.bincount(ray_pt, minlength=n)
    ray_start = np.concatenate([[0], np.cumsum(r)])
    cam = ipcam[cols]
    nc = s0.EO.val.shape[1]
    IO = s0.IO.val
    xy = lenscorr1(s0)[:, cols]
    xn = np.stack([(xy[0] - IO[1, cam]) / -IO[0, cam], (xy[1] - IO[2, cam]) / -IO[0, cam]])
    px = np.asarray(s0.IO.sensor.pxSize, float)
    thr = np.mean(px, 0) / np.abs(IO[0])                 # per camera
    if getattr(s0.IO.sensor, 'samePxSize', False):
        px = np.tile(px[0], (2, 1))
    w = np.abs(IO[0, cam]) / (px[:, cam] * np.asarray(s0.IP.std, float)[:, cols])
    P = np.stack([np.hstack([R, -(R @ s0.EO.val[:3, i])[:, None]]) for i in range(nc) for R in (rotmat3d(s0.EO.val[3:6, i]),)])
    return cols, ray_pt, r, ray_start, cam, xn, w, thr, P


def forwintersect_robust(s0, ids='all', skipPrior=False, n_hyp=256, thr_px=3.0, min_angle_deg=0.0, min_count=2, seed=0, refine=True,
                         reselect=0, max_iter=20, conv_tol=1e-6, device=0):
    """Robust forward intersection of the object points: (s, info, fail).  The image points are lens-corrected and
    normalised as camera_points does (lenscorr1, K \\ [x; y; 1] with -f), the poses [R | -R C] come from EO (rotmat3d), and
    one device call (dbat_hip_intersect_ransac) intersects pairs of rays of every point and returns the hypothesis with the
    most rays within thr_px pixels -- thr_px mean(pxSize) / |f| in normalised units, per camera -- among those whose rays
    meet at min_angle_deg or more.  A point of r rays with r (r - 1) / 2 <= n_hyp has every pair tried (enumerated on the
    device); the others, and every point of more than 64 rays, get n_hyp pairs from draw_pairs with
    np.random.default_rng(seed), point after point (pair_plan).  With refine
    the inliers of every winner go through the least-squares intersection (dbat_hip_pointadjust, all points in one call)
    with the weights |f| / (pxSize IP.std); every one of `reselect` rounds then thresholds the residuals of all the point's
    rays at the refined point again and refines on the new inliers, where they are not fewer and the adjustment
    converges.  No handle is created.  ids and skipPrior choose the points as in forwintersect(); the others keep their
    values.  info is a dict of arrays, one entry per chosen point (info['pts']: its column of OP) unless noted:
      count, n_rays        the inliers and the rays of the point
      sample               the winning pair as two columns of IP, -1 without a winner
      sigma0, Q            of the refinement: sqrt(f / (2 count - 3)) and the 3-by-3 cofactor matrix; NaN without refine
      code, iters          of the refinement (0 converged / 1 max_iter / 2 no step / 3 singular); 0 without refine
      rms_px               the rms over the inliers of the residual in pixels
      inlier               over the columns of IP: the rays that agree with their point
    A point without a winner, or with count < min_count, becomes NaN with code -1, and fail is True."""
    from . import _hip
    from .dbatstruct import copy_struct
    if not np.all(np.isfinite(s0.EO.val)):
        raise ValueError('Bad or uninitialized EO data')
    if not np.all(np.isfinite(s0.IO.val)):
        raise ValueError('Bad or uninitialized IO data')
    s = copy_struct(s0)
    npnt = s0.OP.val.shape[1]
    do = np.ones(npnt, bool) if isinstance(ids, str) and ids == 'all' else np.isin(s0.OP.id, ids)
    if skipPrior:
        do &= np.all(s0.bundle.est.OP, 0) & ~np.any(s0.prior.OP.use, 0)
    pts = np.flatnonzero(do)
    n = pts.size
    nan = np.nan
    info = dict(pts=pts, count=np.zeros(n, int), n_rays=np.zeros(n, int), sample=np.full((n, 2), -1), sigma0=np.full(n, nan),
                Q=np.full((n, 3, 3), nan), code=np.full(n, -1), iters=np.zeros(n, int), rms_px=np.full(n, nan),
                inlier=np.zeros(np.asarray(s0.IP.cam).size, bool))
    if n == 0:
        return s, info, False
    cols, ray_pt, r, ray_start, cam, xn, w, thr, P = point_rays(s0, pts)
    thr = float(thr_px) * thr
    ns, smp_start, smp = pair_plan(r, n_hyp, np.random.default_rng(seed))
    a = _hip.intersect_ransac(ray_start, cam, xn, P, thr ** 2, smp_start=smp_start if smp.shape[0] else None, samples=smp,
                              min_angle=np.deg2rad(float(min_angle_deg)), device=device)
    st = a['stats']
    won = st[:, 1] >= 0
    X, inl = a['X'].copy(), a['inlier'].copy()
    info['count'], info['n_rays'] = st[:, 0].astype(int), r
    info['code'] = np.where(won, 0, -1)
    i, j = _pair_of_number(np.where(won & (ns == 0), st[:, 1], 0), np.maximum(r, 2))
    listed = np.flatnonzero(won & (ns > 0))
    i[listed], j[listed] = smp[smp_start[listed] + st[listed, 1]].T
    ww = np.flatnonzero(won)
    info['sample'][ww] = np.stack([cols[ray_start[ww] + i[ww]], cols[ray_start[ww] + j[ww]]], 1)

    def e2_front(Xc):
        """(the squared residual in normalised units, whether the point is in front) of every ray at the points Xc."""
        with np.errstate(all='ignore'):
            Pr = P[cam]
            h = np.einsum('rij,jr->ir', Pr[:, :, :3], Xc[:, ray_pt]) + Pr[:, :, 3].T
            e = h[:2] / h[2] - xn
            return np.sum(e * e, 0), h[2] < 0

    def adjust(which, use):
        """pointadjust of the points `which` on the rays `use` (over all rays), from their current values."""
        pick = np.isin(ray_pt, which)
        rs = np.concatenate([[0], np.cumsum(r[which])])
        b = _hip.pointadjust(rs, cam[pick], xn[:, pick], P, X[:, which], use=use[pick], w=w[:, pick], max_iter=max_iter,
                             conv_tol=conv_tol, device=device)
        return b, pick

    def take(which, b, pick, ok):
        """The refinements b of the points which[ok] become their results."""
        k = which[ok]
        X[:, k] = b['X'][:, ok]
        for key, src in (('count', 'n_used'), ('sigma0', 'sigma0'), ('Q', 'Q'), ('code', 'code'), ('iters', 'iters')):
            info[key][k] = b[src][ok]
        rays_ok = np.isin(ray_pt[pick], k)
        inl[np.flatnonzero(pick)[rays_ok]] = b['used'][rays_ok]

    if refine and won.any():
        which = np.flatnonzero(won)
        b, pick = adjust(which, inl)
        take(which, b, pick, b['code'] != 4)
        for _ in range(int(reselect)):
            e2, front = e2_front(X)
            mask = front & (e2 <= thr[cam] ** 2) & np.isfinite(e2)
            cnt = np.bincount(ray_pt, weights=mask, minlength=n).astype(int)
            changed = np.bincount(ray_pt, weights=mask != inl, minlength=n) > 0
            which = np.flatnonzero((info['code'] >= 0) & (info['code'] != 4) & changed & (cnt >= info['count']))
            if which.size == 0:
                break
            b, pick = adjust(which, mask)
            take(which, b, pick, (b['code'] == 0) & (b['n_used'] >= info['count'][which]))
    bad = ~won | (info['count'] < int(min_count))
    X[:, bad] = nan
    info['code'][bad] = -1
    inl[bad[ray_pt]] = False
    e2, _ = e2_front(X)
    with np.errstate(all='ignore'):
        ssq_px = np.bincount(ray_pt, weights=np.where(inl, e2 / thr[cam] ** 2, 0.0), minlength=n) * float(thr_px) ** 2
        info['rms_px'] = np.where(bad, nan, np.sqrt(ssq_px / np.maximum(info['count'], 1)))
    info['inlier'][cols] = inl
    s.OP.val[:, pts] = X
    return s, info, bool(bad.any())


resect_hip = resect                   # (names of rounds 2-3)
forwintersect_hip = forwintersect
