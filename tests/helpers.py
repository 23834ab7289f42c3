"""Shared test helpers: known-answer project set-up and seeded synthetic scenes."""
import json
import os

import numpy as np

from dbat_amd import loadpm as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _golden_path(name):
    """Path of a fixture; .xz fixtures are unpacked next to pytest's temp files, under a name that carries the hash of
    the packed file (a copy unpacked from another version of the fixture, or by another user, is never taken for it)."""
    path = os.path.join(GOLDEN, name)
    if os.path.exists(path):
        return path
    import hashlib
    import lzma
    import tempfile
    with open(path + '.xz', 'rb') as fh:
        digest = hashlib.sha256(fh.read()).hexdigest()[:16]
    out = os.path.join(tempfile.gettempdir(), 'dbat_amd_golden_%d_%s_%s' % (os.getuid(), digest, name))
    if not os.path.exists(out):
        with lzma.open(path + '.xz', 'rb') as fi, open(out + '.part%d' % os.getpid(), 'wb') as fo:
            fo.write(fi.read())
        os.replace(out + '.part%d' % os.getpid(), out)
    return out


def camcal_struct(model=3, export='camcal-pmexport.txt', ctrl=True):
    """demo/camcaldemo.m:56-100 set-up, starting from PhotoModeler's own EO/OP
    instead of resect/forwintersect (the converged solution is x0-independent
    inside the basin)."""
    prob = L.loadpm(_golden_path(export))
    s = L.prob2dbatstruct(prob, distModel=model)
    s.IO.val[0, :] = 7.3                                   # setcamvals 'default',7.3
    s.IO.val[1:3, :] = 0.5 * np.diag([1, -1]) @ s.IO.sensor.ssSize
    s.IO.val[3:, :] = 0
    s.bundle.est.IO[:] = True                              # setcamest 'all','not','sk'
    s.bundle.est.IO[4, :] = False
    if model < 3:
        s.bundle.est.IO[3, :] = False
    s.bundle.est.EO[:] = True
    if not ctrl:                                           # camcaldemo_no_datum.m:65
        s.proj = type(s.post)(objUnit='m', x0desc='')
        return s
    s.prior.OP.isCtrl = s.OP.id > 1000
    pts = L.loadcpt(os.path.join(GOLDEN, 'camcal-fixed.txt'))
    s.proj = type(s.post)(objUnit='m', x0desc='Camera calibration from EXIF value')      # camcaldemo.m:107
    return L.setcpt(s, pts)


def camcal_failure_struct(kind):
    """The failure-mode demos on their own inputs: camcaldemo_1ray.m (all but
    one observation of OP 88 removed), camcaldemo_missing_obs.m (no observation
    of OP 13 and 60) -- same pipeline as camcaldemo -- and camcaldemo_no_datum.m
    (no control points, PhotoModeler's EO/OP as initial values)."""
    if kind == 'no-datum':
        return camcal_struct(3, ctrl=False)
    return camcal_demo_struct(3, 'camcal-pmexport-%s.txt' % kind)


def camcal_failures_expected():
    with open(os.path.join(GOLDEN, 'camcal_failures_expected.json')) as fh:
        return json.load(fh)


def check_failure_against_report(ok, iters, s0, E, exp):
    assert not ok and E.code == exp['code'] and iters == exp['iterations'] == 0
    assert (E.numParams, E.numObs, E.redundancy) == (exp['numParams'], exp['numObs'], exp['redundancy'])
    if np.isnan(exp['sigma0']):
        assert np.isnan(s0) and np.isnan(E.res[0])
    else:       # values at x0: 1e-5, see check_report_lines
        assert abs(s0 / exp['sigma0'] - 1) < 1e-5 and abs(E.res[0] / exp['firstError'] - 1) < 1e-5
    w = E.weakness
    if exp['structural'] is None:
        assert w.structural is None
    else:
        assert (w.structural.rank, w.structural.deficiency) == (exp['structural']['rank'], exp['structural']['deficiency'])
        assert list(w.structural.suspectedParams) == exp['structural']['suspectedParams']
        assert np.isnan(w.numerical.rank) and exp['numerical_not_tested']
    if exp['numerical'] is not None:
        assert (w.numerical.rank, w.numerical.deficiency) == (exp['numerical']['rank'], exp['numerical']['deficiency'])
        assert len(w.numerical.suspectedParams) == exp['numerical']['deficiency']
        # every null-space vector is one: J v = 0 to rounding, eigenvalues ~ eps
        assert np.abs(w.numerical.d).max() < 1e-12


def camcal_demo_struct(model=3, export='camcal-pmexport.txt'):
    """The whole demo/camcaldemo.m:56-107 set-up: EXIF camera, EO cleared and
    computed by 3-point resection from the four control points, free OP cleared
    and computed by forward intersection.  With these initial values the
    reference's committed report also pins the iteration count and the first
    residual norm."""
    from dbat_amd import initial as I
    import initial_oracle as IO_
    s = I.clearop(I.cleareo(camcal_struct(model, export)))
    assert np.isnan(s.EO.val).all() and np.isnan(s.OP.val[:, ~s.prior.OP.isCtrl]).all()
    cpId = s.OP.id[s.prior.OP.isCtrl]
    s1, rms, fail = IO_.resect(s, 'all', cpId, 1, 0, cpId)
    assert not fail
    return IO_.forwintersect(s1, 'all', True)


def camcal_expected():
    with open(os.path.join(GOLDEN, 'camcal_expected.json')) as fh:
        return json.load(fh)


def check_camcal_against_report(res, s0, E, exp, sig=6):
    """Compare a converged camcal result with the reference report's printed
    values (6 significant digits; bundle_result_file.m:357-358 flips the sign
    of py, K and P for display)."""
    def close(a, b, digits=sig):
        if b == 0:
            return abs(a) < 10.0 ** (-digits)
        # one unit in the last printed digit: the reference stops at convTol=1e-6,
        # so its 7th digit depends on its own x0/iteration path.
        return abs(a - b) <= 1.01 * 10.0 ** (np.floor(np.log10(abs(b))) - digits + 1)
    assert E.numParams == exp['numParams'] and E.numObs == exp['numObs']
    assert E.redundancy == exp['redundancy']
    assert close(s0, exp['sigma0']), (s0, exp['sigma0'])
    io = res.IO.val[:, 0]
    rep = exp['IO_report']
    got = {'cc': io[0], 'px': io[1], 'py': -io[2], 'as': io[3], 'K1': -io[5],
           'K2': -io[6], 'K3': -io[7], 'P1': -io[8], 'P2': -io[9]}
    for k, v in rep.items():
        assert close(got[k], v, 4 if k == 'cc' else sig), (k, got[k], v)
    eo = np.array(exp['EO_report_deg'])
    ang = np.rad2deg(res.EO.val[3:6]).T
    dang = (ang - eo[:, :3] + 180.0) % 360.0 - 180.0     # x0-dependent 2*pi wraps
    assert np.abs(dang).max() < 1e-6
    assert np.abs(res.EO.val[:3].T - eo[:, 3:]).max() < 1e-6


def check_camcal_cov_against_report(s, CIO, CEO, COP, exp):
    """Posterior standard deviations against the "Deviation" values of the
    reference report (3 significant digits; angles printed in degrees) and its
    point-precision summary (2 significant digits, bundle_result_file.m:674-700)."""
    def close(a, b, digits):
        return abs(a - b) <= 0.51 * 10.0 ** (np.floor(np.log10(abs(b))) - digits + 1) * 1.02
    sd_io = np.sqrt(CIO.diagonal()).reshape(s.IO.val.shape, order='F')[:, 0]
    got = {'cc': sd_io[0], 'px': sd_io[1], 'py': sd_io[2], 'as': sd_io[3], 'K1': sd_io[5],
           'K2': sd_io[6], 'K3': sd_io[7], 'P1': sd_io[8], 'P2': sd_io[9]}
    for k, v in exp['IO_deviation'].items():
        assert close(got[k], v, 3), ('IO', k, got[k], v)
    sd_eo = np.sqrt(CEO.diagonal()).reshape(s.EO.val.shape, order='F')[:6].T   # X Y Z om ph ka
    dev = np.array(exp['EO_deviation'], float)                                # om ph ka [deg] X Y Z
    for i in range(dev.shape[0]):
        for j in range(3):
            assert close(np.rad2deg(sd_eo[i, 3 + j]), dev[i, j], 3), ('EO angle', i, j)
            assert close(sd_eo[i, j], dev[i, 3 + j], 3), ('EO pos', i, j)
    var = COP.diagonal().reshape(s.OP.val.shape, order='F')
    var = np.where(np.asarray(s.bundle.est.OP, bool), var, np.nan)
    tstd = np.sqrt(var.sum(0))
    ids = np.asarray(s.OP.id)
    ts = exp['OP_total_std']
    assert close(np.nanmin(tstd), ts['min'], 2) and close(np.nanmax(tstd), ts['max'], 2)
    assert ids[np.nanargmax(tstd)] == ts['max_id']
    for c in range(3):
        assert close(np.sqrt(np.nanmax(var[c])), exp['OP_max_std'][c], 2), ('OP', c)


def check_report_lines(lines, ref_path=os.path.join(GOLDEN, 'camcal-dbatreport.txt'), demo_x0=False,
                       ref_lines=None, x0_lines=('First error:',), x0_tol=1e-5):
    """Every line of dbat_amd.report's output must occur, in order, in the
    reference's committed result file -- verbatim, or with numbers that differ by
    one unit in the last printed digit (the reference stops at convTol 1e-6) or by
    a full turn (angles).  The iteration count and the first error depend on the
    demo's initial values (EXIF + resection): they are compared only with
    demo_x0 (camcal_demo_struct), the first error to 1e-5 -- camera 21's
    resection quartic has a near-triple root, so one ulp in its coefficients moves
    the sixth digit (tests/test_oracle.py::test_resect_first_error_conditioning).
    Returns the number of verbatim matches."""
    import re
    ref = [l.rstrip() for l in (ref_lines if ref_lines is not None else open(ref_path).read().splitlines())]
    num = re.compile(r'[-+]?\d+\.?\d*(?:[eE][-+]?\d+)?')
    skel = lambda l: num.sub('#', l)

    def close(a, b):
        if a == b:
            return True
        fa, fb = float(a), float(b)
        digits = len(re.sub(r'[eE].*$', '', b).replace('-', '').replace('+', '').replace('.', '').lstrip('0')) or 1
        tol = 1.01 * 10.0 ** (np.floor(np.log10(abs(fb))) - digits + 1) if fb != 0 else 1e-12
        return abs(fa - fb) <= tol or abs(abs(fa - fb) - 360.0) <= tol

    pos, verbatim = 0, 0
    for l in lines:
        l = l.rstrip()
        if ('Number of iterations:' in l or 'First error:' in l) and not demo_x0:
            continue
        key = [k for k in x0_lines if l.strip().startswith(k)]
        if key and 'nan' not in l.lower():
            # values at the resected x0 (a failed bundle's sigma0 and last error are such values too)
            want = [float(num.findall(r)[-1]) for r in ref if r.strip().startswith(key[0])][0]
            assert abs(float(num.findall(l)[-1]) / want - 1) < x0_tol, (l, want)
            continue
        hit = None
        for q in range(pos, len(ref)):
            if ref[q] == l:
                hit = q; verbatim += 1
                break
            if skel(ref[q]) == skel(l):
                na, nb = num.findall(l), num.findall(ref[q])
                if len(na) == len(nb) and all(close(a, b) for a, b in zip(na, nb)):
                    hit = q
                    break
        assert hit is not None, 'line not found in the reference report: %r' % l
        pos = hit + 1
    return verbatim


# ---------------------------------------------------------------------------
# seeded synthetic variants used by the parity tests
# ---------------------------------------------------------------------------

def synth_struct(name='tiny', variant='plain', seed=None):
    """Synthetic scene (dbat_amd.synth) with optional complications:
       'plain'    fixed IO, datum by dependency
       'selfcal'  one shared IO block, cc px py K1-3 P1-2 estimated
       'imagevar' image-variant principal point (one px,py block per image),
                  cc,K shared  (demo/romabundledemo_imagevariant.m:42-48)
       'priors'   EO position priors on every 3rd camera, OP priors on control
                  points, a few fixed control points, non-uniform IP.std
       'groups4'  four camera groups with independent self-calibrated IO blocks
                  (BASELINE.json configs[4]; script/setdbatcamsandimages.m:28,
                  buildserialindices.m:162-221)
    """
    from dbat_amd import synth
    if variant == 'groups4':
        return synth.make_scene(name, seed=seed, selfcal=True, groups=4)
    s, truth = synth.make_scene(name, seed=seed)
    nc, npnt = s.EO.val.shape[1], s.OP.val.shape[1]
    rng = np.random.default_rng(12345)
    if variant == 'selfcal':
        s.bundle.est.IO[[0, 1, 2, 5, 6, 7, 8, 9]] = True
    elif variant == 'imagevar':
        s.bundle.est.IO[[0, 1, 2, 5, 6]] = True
        s.IO.struct.block[1:3] = np.arange(1, nc + 1)[None, :]
    elif variant == 'priors':
        s.bundle.est.EO[:] = True                       # datum from priors instead
        cams = np.arange(0, nc, 3)
        s.prior.EO.use[0:3, cams] = True
        s.prior.EO.val[0:3, cams] = truth['EO'][0:3, cams] + rng.normal(0, 0.02, (3, len(cams)))
        s.prior.EO.std[0:3, cams] = 0.02
        cps = np.arange(0, npnt, 37)
        s.prior.OP.use[:, cps] = True
        s.prior.OP.val[:, cps] = truth['OP'][:, cps] + rng.normal(0, 0.01, (3, len(cps)))
        s.prior.OP.std[:, cps] = np.array([[0.01], [0.01], [0.02]])
        fixed = np.arange(5, npnt, 53)
        s.OP.val[:, fixed] = truth['OP'][:, fixed]
        s.bundle.est.OP[:, fixed] = False
        s.IP.std = s.IP.std * (1 + (np.arange(s.IP.std.shape[1]) % 3)[None, :] * 0.5)
        s.IP.sigmas = np.unique(s.IP.std)
    elif variant != 'plain':
        raise ValueError(variant)
    return s, truth


CROWDED_KINDS = ('fixed', 'prior3', 'zprior', 'zfixed')


def crowded_struct(kind, frac=0.85, cams=60, points=3000, control=0, selfcal=False, seed=None):
    """Scene whose batches hold many points: synth.make_scene('small', rays=2) with a fraction `frac` of the points cut
    down to ONE ray (the observation kept is drawn at random).  A single ray fixes two of a point's three coordinates, so
    those points are made determined by `kind`:
       'fixed'   all three coordinates fixed at their true values (a control point measured in one image)
       'prior3'  a prior observation of all three coordinates, estimated
       'zprior'  a prior of Z only, X and Y estimated (mono-plotting with a height prior)
       'zfixed'  Z fixed at its true value, X and Y estimated (mono-plotting on a known height)
    With 'zprior' and 'zfixed' every fourth of these points is fixed instead: such points say nothing of X and Y, and
    two-ray tie points do not carry the scale from one stereo pair to the next, so the block needs control points.
    control > 0: one more point, at the middle of the block, seen in the `control` cameras nearest to it, with a prior
    on all three coordinates -- with DBAT_HIP_CMAX below `control` it is heavy, and the other points, being few, join
    it on the heavy route.  Returns (s, truth)."""
    from dbat_amd import synth
    if kind not in CROWDED_KINDS:
        raise ValueError(kind)
    s, truth = synth.make_scene('small', cams=cams, points=points, rays=2, selfcal=selfcal, seed=seed)
    rng = np.random.default_rng(4321)
    npnt = s.OP.val.shape[1]
    single = rng.random(npnt) < frac
    # the point's two observations: drop one of them at random
    pt = np.asarray(s.IP.pt)
    order = np.argsort(pt, kind='stable')
    first = np.ones(len(pt), bool)
    first[order[1::2]] = False                          # every point has exactly two observations, ascending
    drop_second = rng.random(npnt) < 0.5
    drop = single[pt] & (first == ~drop_second[pt])
    keep = ~drop
    IP = s.IP
    IP.val, IP.std = np.asfortranarray(IP.val[:, keep]), np.asfortranarray(IP.std[:, keep])
    IP.cam, IP.pt = IP.cam[keep], IP.pt[keep]
    est, pr, OPt = s.bundle.est.OP, s.prior.OP, truth['OP']
    sel = np.flatnonzero(single)
    if kind == 'fixed':
        s.OP.val[:, sel] = OPt[:, sel]
        est[:, sel] = False
    elif kind == 'prior3':
        pr.use[:, sel] = True
        pr.std[:, sel] = np.array([[0.02], [0.02], [0.03]])
        pr.val[:, sel] = OPt[:, sel] + rng.normal(0, 1, (3, len(sel))) * pr.std[:, sel]
    elif kind == 'zprior':
        pr.use[2, sel] = True
        pr.std[2, sel] = 0.03
        pr.val[2, sel] = OPt[2, sel] + rng.normal(0, 0.03, len(sel))
    else:
        s.OP.val[2, sel] = OPt[2, sel]
        est[2, sel] = False
    if kind in ('zprior', 'zfixed'):
        ctl = sel[::4]
        s.OP.val[:, ctl] = OPt[:, ctl]
        est[:, ctl] = False
        pr.use[:, ctl] = False
    if control:
        IO, EO = truth['IO'], truth['EO']
        Q = np.array([[EO[0].mean()], [EO[1].mean()], [5.0]])
        cams_c = np.sort(np.argsort(np.hypot(EO[0] - Q[0, 0], EO[1] - Q[1, 0]))[:control]).astype(IP.cam.dtype)
        OPx = np.hstack([OPt, Q])
        px = float(np.ravel(s.IO.sensor.pxSize)[0])
        uv, depth = synth.project(IO, EO, OPx, cams_c, np.full(control, npnt), px, nK=3, nP=2)
        assert np.all(depth < 0), 'control point behind a camera'
        uv = uv + rng.normal(0, 0.5, uv.shape)
        s.OP.val = np.asfortranarray(np.hstack([s.OP.val, Q + rng.normal(0, 0.05, (3, 1))]))
        s.OP.id = np.append(s.OP.id, s.OP.id.max() + 1)
        s.bundle.est.OP = np.asfortranarray(np.hstack([est, np.ones((3, 1), bool)]))
        pr.use = np.asfortranarray(np.hstack([pr.use, np.ones((3, 1), bool)]))
        pr.std = np.asfortranarray(np.hstack([pr.std, np.full((3, 1), 0.01)]))
        pr.val = np.asfortranarray(np.hstack([pr.val, Q + rng.normal(0, 0.01, (3, 1))]))
        truth['OP'] = OPx
        cam = np.concatenate([IP.cam, cams_c])
        pt_ = np.concatenate([IP.pt, np.full(control, npnt, IP.pt.dtype)])
        o = np.lexsort((pt_, cam))                      # image-major, ascending OP inside an image
        IP.val = np.asfortranarray(np.hstack([IP.val, uv])[:, o])
        IP.std = np.asfortranarray(np.hstack([IP.std, np.ones((2, control))])[:, o])
        IP.cam, IP.pt = cam[o], pt_[o]
    return s, truth


def giant_points_struct(cams, points, variant='plain'):
    """synth.make_scene('small', rays=6) with a distortion-free camera (the projections far outside the image format
    stay well defined) and three control points (3, 77, 250) seen in EVERY image: more observations than one batch
    holds.  variant 'selfcal' estimates cc, px, py, K1, K2; 'selfcal-groups3' over three camera groups with IO blocks
    of their own.  Uniform IP.std.  Returns (s, truth)."""
    from dbat_amd import synth
    s, truth = synth.make_scene('small', cams=cams, points=points, rays=6)
    s.IO.val[5:10] = 0.0
    truth['IO'][5:10] = 0.0
    nc = s.EO.val.shape[1]
    if variant != 'plain':
        s.bundle.est.IO[[0, 1, 2, 5, 6]] = True
        if variant == 'selfcal-groups3':
            s.IO.struct.block[:] = (1 + (np.arange(nc) * 3) // nc)[None, :]
        elif variant != 'selfcal':
            raise ValueError(variant)
    px = float(np.ravel(s.IO.sensor.pxSize)[0])
    rng = np.random.default_rng(5)
    add_cam, add_pt = [], []
    for p in (3, 77, 250):
        have = set(s.IP.cam[s.IP.pt == p].tolist())
        for c in range(nc):
            if c not in have:
                add_cam.append(c); add_pt.append(p)
    cam = np.r_[s.IP.cam, np.array(add_cam)]; pt = np.r_[s.IP.pt, np.array(add_pt)]
    order = np.lexsort((pt, cam))                       # image-major, ascending OP
    cam, pt = cam[order], pt[order]
    uv, depth = synth.project(truth['IO'], truth['EO'], truth['OP'], cam, pt, px, nK=3, nP=2)
    assert np.all(depth < 0)
    s.IP.val = uv + rng.normal(0, 0.5, uv.shape)
    s.IP.std = np.ones_like(uv)
    s.IP.cam, s.IP.pt = cam, pt
    assert np.bincount(s.IP.pt).max() == nc
    return s, truth


def mixed_heavy_struct(variant):
    """synth 'small' with every second point thinned out to 4 rays: with DBAT_HIP_CMAX=6 the 8-ray points are heavy,
    next to tiled points in one problem.  Returns (s, truth)."""
    s, truth = synth_struct('small', variant)
    pt, cam = s.IP.pt, s.IP.cam
    rank = np.zeros(len(pt), int)
    order = np.lexsort((cam, pt))
    first = np.r_[True, pt[order][1:] != pt[order][:-1]]
    idx = np.arange(len(pt)) - np.maximum.accumulate(np.where(first, np.arange(len(pt)), 0))
    rank[order] = idx
    keep = ~((pt % 2 == 0) & (rank >= 4))
    s.IP.val, s.IP.std = s.IP.val[:, keep], s.IP.std[:, keep]
    s.IP.cam, s.IP.pt = s.IP.cam[keep], s.IP.pt[keep]
    return s, truth


def all_see_all_scene(cams, points, selfcal, groups=1, seed=3):
    """Every point in every image (the geometry of the reference's calibration demo, demo/camcaldemo.m:56-119)."""
    from dbat_amd import synth
    return synth.make_dense_scene(cams, points, selfcal, groups, seed)


# ---------------------------------------------------------------- per-observation weight factors (tests/test_obs_weights_*.py)
def obs_weight_factors(no, seed, lo=1e-2):
    """Weight factors omega in [lo, 1] of `no` image points: log-uniform, about 10 % exactly 1.0 and about 1 % exactly
    lo -- a spread wide enough that a weight on the wrong observation moves the step far above any tolerance."""
    rng = np.random.default_rng(seed)
    om = np.exp(rng.uniform(np.log(lo), 0.0, no))
    u = rng.random(no)
    om[u < 0.10] = 1.0
    om[(u >= 0.10) & (u < 0.11)] = lo
    return np.minimum(om, 1.0)


def std_pattern(s):
    """A copy of s with the non-uniform IP.std of synth_struct's 'priors' variant: IP.std * (1 + 0.5 * (i % 3))."""
    import copy
    t = copy.deepcopy(s)
    t.IP.std = np.asfortranarray(np.asarray(t.IP.std, float) * (1 + (np.arange(t.IP.std.shape[1]) % 3)[None, :] * 0.5))
    t.IP.sigmas = np.unique(t.IP.std)
    return t


def reweighted_struct(s, omega):
    """The same least-squares problem as s with the weight factor omega_i on image point i: IP.std[:, i] / sqrt(omega_i)."""
    import copy
    t = copy.deepcopy(s)
    t.IP.std = np.asfortranarray(np.asarray(t.IP.std, float) / np.sqrt(np.asarray(omega, float))[None, :])
    t.IP.sigmas = np.unique(t.IP.std)
    return t


def base_image_weights(s):
    """(nObs, 2) base weights 1 / (IP.std * pxSize) of the image rows, in the row order of the residual vector."""
    px = np.asarray(s.IO.sensor.pxSize, float)
    px = px[:, s.IP.cam] if px.shape[1] > 1 else px
    return (1.0 / (np.asarray(s.IP.std, float) * px)).T


def relerr(a, b):
    """misc/relerr.m: Frobenius relative error."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    d = np.linalg.norm(b.ravel())
    return np.linalg.norm((a - b).ravel()) / (d if d > 0 else 1.0)


TOL_LIN = 1e-10         # column norms, trace(J'J), ||J v||^2 and J v: the bars of test_hip_parity.py::test_step_parity


def linearisation_figures(h, J, trace_h):
    """The quantities of handle h's last linearisation that no step shows, against the oracle's weighted sparse J at
    the same point: relative errors of the column norms (sqrt(sum J o J, axis 0)), of trace_h (st['trace'] of that
    linearisation) against (J'J).diagonal().sum(), and with v = default_rng(2).standard_normal(n) of ||J v||^2 and
    of J v (image rows in the reference's row order).  Column norms squared, trace and ||J v||^2 are sums of
    non-negative f64 terms, at most about 1e4 per column: n 2^-53 is about 1e-12, two orders below TOL_LIN.  That
    holds column by column, and the vector's relerr is blind to the point columns beside a distortion column of 1e10
    (a quarter too much on every heavy point's norm is 9e-10 of giant-mfma's vector): 'worst_column' is the largest
    relative error of one column norm."""
    J = J.tocsc()
    Jn = np.sqrt(np.asarray(J.multiply(J).sum(0)).ravel())
    tr = float((J.T @ J).diagonal().sum())
    v = np.random.default_rng(2).standard_normal(J.shape[1])
    Jv = J @ v
    Jn_h = h.colnorms()
    assert Jn.min() > 0
    return dict(colnorms=relerr(Jn_h, Jn), worst_column=float(np.abs(Jn_h / Jn - 1).max()), trace=abs(trace_h - tr) / tr,
                JvJv=abs(h.jtimes_sqnorm(v) - Jv @ Jv) / (Jv @ Jv), Jv=relerr(h.jtimes(v), Jv))


def check_linearisation_figures(fig, label):
    """Prints the figures of linearisation_figures, then holds each to TOL_LIN."""
    print('linearisation %-44s colnorms %.2e  trace %.2e  JvJv %.2e  Jv %.2e  worst column %.2e'
          % (label, fig['colnorms'], fig['trace'], fig['JvJv'], fig['Jv'], fig['worst_column']))
    for k in ('colnorms', 'worst_column', 'trace', 'JvJv', 'Jv'):
        assert fig[k] < TOL_LIN, '%s: %s of the linearisation off by %.2e' % (label, k, fig[k])


def script_forwintersect(s):
    """The script operation forward_intersection: on the device where there is one (the product path,
    dbat_amd.loadtables.forwintersect -> dbat_hip_forwintersect), by the oracle's restatement on the CPU box."""
    import torch
    if torch.cuda.is_available():
        from dbat_amd import loadtables as T
        return T.forwintersect(s)
    import initial_oracle
    return initial_oracle.forwintersect(s, 'all')


def roma_struct():
    """data/script/romabundledemo/romabundledemo.xml: loaded camera and EO,
    OP by forward intersection, estimate cc, pp, K1, K2 (no aspect, skew, P,
    K3), datum by dependency on camera 1."""
    from dbat_amd import loadtables as T
    from dbat_amd.dbatstruct import seteoest_depend
    exp = roma_expected()
    ci = exp['camera_in']
    eo = T.load_table(os.path.join(GOLDEN, 'roma-initial_eo.txt'))
    mk = T.load_table(os.path.join(GOLDEN, 'roma-markpts.txt.xz'))
    h = ci['sensor_height']
    sensor = (ci['image'][0] * h / ci['image'][1], h)          # sensor 'auto,24', aspect 1
    io = T.camera_io(ci['cc'], ci['pp'], ci['K'], ci['P'])
    s = T.struct_from_tables(io, sensor, ci['image'], eo, mk, 'im,id,x,y', 1.0, distModel=ci['model'])
    s = script_forwintersect(s)
    s.bundle.est.IO[[0, 1, 2, 5, 6]] = True
    s.EO.name = exp['image_paths']
    s.proj = type(s.post)(objUnit='m', x0desc='')
    return seteoest_depend(s, 0)


PRAGUE = {'c1': ('cam', 'fixed', False), 'c2': ('cam', 'weighted', True), 's1': ('sxb', 'f-op0', False),
          's2': ('sxb', 'w-op0', True), 's3': ('sxb', 'w-op1', True), 's4': ('sxb', 'wsmart', True)}


def prague_struct(label):
    """demo/prague2016_pm.m:82-190 for experiment label c1, c2, s1..s4: the
    PhotoModeler export with its loaded, fixed camera; control points from
    the reference file, shifted by the mean offset to PhotoModeler's frame
    (:150-166), fixed or weighted; EO by resection, OP by forward intersection.
    The demo runs the legacy lens model 1 (prob2dbatstruct's default), the model
    that model 2 replicates (bundle.m:49-51); oracle and library evaluate it as
    model 2.  Returns (s, path of the committed report)."""
    from dbat_amd import initial as I
    import initial_oracle as IO_
    site, stub, weighted = PRAGUE[label]
    prob = L.loadpm(_golden_path('prague-%s-%s-pmexport.txt' % (site, stub)))
    s = L.prob2dbatstruct(prob, distModel=1)
    s.bundle.est.IO[:] = False                             # setcamvals 'loaded'; setcamest 'not','all'
    pts = L.loadcpt(os.path.join(GOLDEN, 'prague-%s-ctrlpts-%s.txt' % (site, 'weighted' if weighted else 'fixed')))
    pm = prob['ctrlPts']
    assert np.all(np.isin(pm[:, 0], pts['id']))
    _, ia, ib = np.intersect1d(pm[:, 0].astype(int), pts['id'], return_indices=True)
    offset = pm[ia, 1:4].T - pts['pos'][:, ib]
    pts['pos'] = pts['pos'] + offset.mean(1)[:, None]
    s = L.setcpt(s, pts)
    s.proj = type(s.post)(objUnit='m', x0desc='')
    s = I.clearop(I.cleareo(s))
    cpId = s.OP.id[s.prior.OP.isCtrl]
    s, rms, fail = IO_.resect(s, 'all', cpId, 1, 0, cpId)
    assert not fail
    return IO_.forwintersect(s, 'all', True), os.path.join(GOLDEN, 'prague-%s-%s-dbatreport.txt' % (site, stub))


def sxb_prior_eo_struct(use_prior_eo):
    """demo/sxb_prior_eo.m:33-83: the Strasbourg smart-point project in its
    1e6-m frame, weighted control points, loaded fixed camera, and optionally
    prior observations (0.05 m) of four of the five camera positions from
    ref/fake-camera-positions.txt (misc/setprioreo.m).  Returns (s, report)."""
    from dbat_amd import initial as I
    import initial_oracle as IO_
    prob = L.loadpm(_golden_path('prague-sxb-wsmart-with-orient-pmexport.txt'))
    s = L.prob2dbatstruct(prob, distModel=1)               # the demo's model; evaluated as model 2 (bundle.m:49-51)
    s.bundle.est.IO[:] = False
    s = L.setcpt(s, L.loadcpt(os.path.join(GOLDEN, 'prague-sxb-ctrlpts-weighted.txt')))
    s.proj = type(s.post)(objUnit='m', x0desc='')
    if use_prior_eo:
        names = [os.path.basename(n) for n in s.EO.name]
        for line in open(os.path.join(GOLDEN, 'prague-sxb-fake-camera-positions.txt')):
            if line.startswith('#') or not line.strip():
                continue
            tok = [v.strip() for v in line.split(',')]
            i = names.index(tok[0])
            pos, sd = np.array([float(v) for v in tok[1:4]]), float(tok[4])
            s.prior.EO.val[:3, i] = pos
            s.EO.val[:3, i] = pos
            s.prior.EO.std[:3, i] = sd
            s.prior.EO.use[:3, i] = sd != 0
            s.bundle.est.EO[:3, i] = sd != 0
    s = I.clearop(I.cleareo(s))
    cpId = s.OP.id[s.prior.OP.isCtrl]
    s, rms, fail = IO_.resect(s, 'all', cpId, 1, 0, cpId)
    assert not fail
    return IO_.forwintersect(s, 'all', True), os.path.join(
        GOLDEN, 'prague-sxb-%sprior-eo-dbatreport.txt' % ('' if use_prior_eo else 'no-'))


def sxb_expected():
    with open(os.path.join(GOLDEN, 'sxb_expected.json')) as fh:
        return json.load(fh)


def sxb_struct():
    """data/script/sxb/sxb.xml: five aerial images, fixed camera, 14 control
    points as prior observations (0.02/0.02/0.04 m) and two check points, marked
    points at 0.5 px and smart points at 1 px, project coordinates of 1e6 m;
    operations set_initial_values (loaded), set_bundle_estimate_params (io
    false, eo true, op default), spatial_resection, forward_intersection
    (script/parseops.m:36-43)."""
    from dbat_amd import initial as I
    import initial_oracle as IO_
    from dbat_amd import loadtables as T
    exp = sxb_expected()
    cam = exp['camera']
    pts = L.loadcpt(os.path.join(GOLDEN, 'sxb-control.txt'))

    def pick(keep):
        m = np.isin(pts['id'], exp['check_ids']) == keep
        return dict(id=pts['id'][m], name=[n for n, k in zip(pts['name'], m) if k], pos=pts['pos'][:, m],
                    std=pts['std'][:, m])
    io = T.camera_io(cam['cc'], cam['pp'], cam['K'], cam['P'])
    marks = [(T.load_table(os.path.join(GOLDEN, 'sxb-%s.txt' % nm)), 'id,im,x,y', exp['sxy'][nm])
             for nm in ('markpts', 'smartpts')]
    s = T.struct_from_script(io, cam['sensor'], cam['image'], exp['images'], marks, pick(False), pick(True),
                             distModel=cam['model'], im_names=exp['image_paths'])
    s = T.set_script_defaults(s)
    s.proj = type(s.post)(objUnit='m', x0desc='')
    cpId = s.OP.id[s.prior.OP.isCtrl]
    s, rms, fail = IO_.resect(s, 'all', cpId, 1, 0, cpId)
    assert not fail
    return IO_.forwintersect(s, 'all', True)


def check_sxb_against_report(res, s0, E, iters, exp):
    """data/script/sxb/result/report.txt:19-43 and its photo blocks.  The
    converged values are compared to the printed precision; the first error to
    1e-4: the resected camera centres carry |C|^2*eps ~ 1e-4 m of SVD rounding
    noise at these coordinates (dbat_amd/initial.py, resect)."""
    rep = exp['report']
    six = lambda a, b: abs(a - b) <= 1.01 * 10.0 ** (np.floor(np.log10(abs(b))) - 5)
    assert (E.numParams, E.numObs, E.redundancy) == (rep['numParams'], rep['numObs'], rep['redundancy'])
    assert (rep['nIO'], rep['nEO'], rep['nOP']) == (0, 30, 1143)
    assert iters == rep['iterations'] == 4
    assert six(s0, rep['sigma0']) and six(res.post.sigmas[0], rep['sigma0_px'])
    assert abs(E.res[0] / rep['firstError'] - 1) < 1e-4 and six(E.res[-1], rep['lastError'])
    eo = np.array(rep['EO_report_deg'])
    assert np.abs(np.rad2deg(res.EO.val[3:6]).T - eo[:, :3]).max() < 1.5e-6
    assert np.abs(res.EO.val[:3].T - eo[:, 3:]).max() < 2e-6          # metres, at 1e6 m


def roma_demo_struct(variant):
    """demo/romabundledemo{,_selfcal,_imagevariant}.m:57-84: PhotoModeler's
    camera (printed in roma-dbatreport.txt:58-92: 36.036 x 24 mm format as an
    off-unit aspect of 0.000998889 on square 24/3744 mm pixels), fixed or
    self-calibrated without skew, or with one principal point per image; OP by
    forward intersection, datum by dependency on camera 1.  The image points
    are those of the script fixture (same 181 122 observations)."""
    from dbat_amd import loadtables as T
    from dbat_amd.dbatstruct import seteoest_depend
    cam = roma_variants_expected()['fixed']['IO_report']
    eo = T.load_table(os.path.join(GOLDEN, 'roma-initial_eo.txt'))
    mk = T.load_table(os.path.join(GOLDEN, 'roma-markpts.txt.xz'))
    io = T.camera_io(cam['cc'], (cam['px'], cam['py']), [cam['K1'], cam['K2'], cam['K3']], [cam['P1'], cam['P2']],
                     aspect=1.0 - cam['as'])
    s = T.struct_from_tables(io, (36.0, 24.0), (5616, 3744), eo, mk, 'im,id,x,y', 1.0, distModel=3)
    s = script_forwintersect(s)
    if variant != 'fixed':
        s.bundle.est.IO[:] = True                              # setcamest 'all','not','sk'
        s.bundle.est.IO[4] = False
    if variant == 'imagevariant':                              # romabundledemo_imagevariant.m:63
        s.IO.struct.block[1:3] = np.arange(1, s.EO.val.shape[1] + 1)[None, :]
    return seteoest_depend(s, 0)


def roma_variants_expected():
    with open(os.path.join(GOLDEN, 'roma_variants_expected.json')) as fh:
        return json.load(fh)


def check_roma_variant(res, s0, E, exp, CIO=None):
    """sigma0, counts, and -- when estimated -- the camera values (and their
    posterior deviations) of roma-dbatreport{,-selfcal,-imagevariant}.txt, six
    (three) significant digits; report signs as bundle_result_file.m:357-358."""
    close = lambda a, b, d: abs(a - b) <= 1.01 * 10.0 ** (np.floor(np.log10(abs(b))) - d + 1) if b else abs(a) < 1e-12
    assert (E.numParams, E.numObs, E.redundancy) == (exp['numParams'], exp['numObs'], exp['redundancy'])
    assert close(s0, exp['sigma0'], 6), (s0, exp['sigma0'])
    io = res.IO.val[:, 0]
    got = {'cc': io[0], 'px': io[1], 'py': -io[2], 'as': io[3], 'K1': -io[5], 'K2': -io[6], 'K3': -io[7],
           'P1': -io[8], 'P2': -io[9]}
    for k, v in exp['IO_report'].items():
        assert close(got[k], v, 6), (k, got[k], v)
    if CIO is not None:
        sd = np.sqrt(CIO.diagonal()).reshape(res.IO.val.shape, order='F')[:, 0]
        gsd = {'cc': sd[0], 'px': sd[1], 'py': sd[2], 'as': sd[3], 'K1': sd[5], 'K2': sd[6], 'K3': sd[7],
               'P1': sd[8], 'P2': sd[9]}
        assert len(exp['IO_deviation']) >= 8
        for k, v in exp['IO_deviation'].items():
            assert abs(gsd[k] - v) <= 0.52 * 10.0 ** (np.floor(np.log10(abs(v))) - 2), ('dev', k, gsd[k], v)


def roma_expected():
    with open(os.path.join(GOLDEN, 'roma_expected.json')) as fh:
        return json.load(fh)


def check_roma_against_result(res, s0, E, iters, exp):
    rep, cam = exp['report'], exp['camera_out']
    assert E.numParams == rep['numParams'] and E.numObs == rep['numObs']
    assert E.redundancy == rep['redundancy'] and iters == rep['iterations']
    assert abs(s0 - rep['sigma0']) < 1.01e-6
    assert abs(E.res[0] - rep['firstError']) < 0.0051 * 1.01       # printed with 6 significant digits
    assert abs(E.res[-1] - rep['lastError']) < 0.00051 * 1.01
    io = res.IO.val[:, 0]
    # result/EOS5DMarkII.xml is written with %.18g; the reference stops at convTol=1e-6
    assert abs(io[0] - cam['cc']) < 1e-7 * cam['cc']
    assert abs(io[1] - cam['pp'][0]) < 1e-7 * cam['pp'][0]
    assert abs(-io[2] - cam['pp'][1]) < 1e-7 * cam['pp'][1]
    assert abs(-io[5] - cam['K'][0]) < 1e-6 * abs(cam['K'][0])
    assert abs(-io[6] - cam['K'][1]) < 1e-6 * abs(cam['K'][1])
    eo = np.array(rep['EO_report_deg'])
    dang = (np.rad2deg(res.EO.val[3:6]).T - eo[:, :3] + 180.0) % 360.0 - 180.0
    assert np.abs(dang).max() < 1.01e-6
    assert np.abs(res.EO.val[:3].T - eo[:, 3:]).max() < 1.01e-6


# ---------------------------------------------------------------- C ABI driver (tests/abi_c_driver.c)
def build_abi_c_driver():
    """Compile tests/abi_c_driver.c as plain C11 against include/dbat_hip.h and link it with
    libdbat_hip.so.  Returns the path of the executable."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = os.path.join(root, 'tests', 'abi_c_driver.out')
    src = os.path.join(root, 'tests', 'abi_c_driver.c')
    lib = os.path.join(root, 'dbat_amd')
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(
            os.path.join(root, 'include', 'dbat_hip.h'))):
        subprocess.run(['gcc', '-std=c11', '-Wall', '-Wextra', '-pedantic', '-Werror', '-O1', '-I' + os.path.join(root, 'include'),
                        src, '-o', out, '-L' + lib, '-ldbat_hip', '-Wl,-rpath,' + lib, '-Wl,-rpath,/opt/rocm/lib'],
                       check=True, capture_output=True)
    return out


def dump_problem(s, path):
    """The arrays of dbat_hip_problem in declaration order (abi_c_driver.c::load)."""
    from dbat_amd import _hip
    p, keep = _hip.problem_from_struct(s)
    hdr = np.array([p.n_images, p.n_points, p.n_obs, p.dist_model, p.nK, p.nP, 5 + p.nK + p.nP, 0], np.int64)
    order = ['ip_cam', 'ip_pt', 'ip_val', 'ip_std', 'IO_val', 'px_size', 'EO_val', 'OP_val', 'est_IO', 'est_EO',
             'est_OP', 'IO_block', 'EO_block', 'prior_IO_use', 'prior_IO_val', 'prior_IO_std', 'prior_EO_use',
             'prior_EO_val', 'prior_EO_std', 'prior_OP_use', 'prior_OP_val', 'prior_OP_std']
    with open(path, 'wb') as f:
        f.write(hdr.tobytes())
        for k in order:
            f.write(keep[k].tobytes())


def oracle_lm_reordered(s, seed=1, max_iter=20, conv_tol=1e-6):
    """The oracle's Levenberg-Marquardt loop (levenberg_marquardt.m:52-250) on the SAME problem with
    the rows of r and J visited in a different order: every sum over the rows (r'r, J'J, J'r) then
    rounds differently, nothing else changes.  Returns (x, code, iters, rr, lambdas).

    Used to decide where an iteration count is a property of the problem and where it is rounding
    noise of the reference algorithm itself (tests/test_hip_parity.py::check_history)."""
    import copy
    import dbat_oracle as o
    s = copy.deepcopy(s)
    for nm in ('IO', 'EO', 'OP'):
        pr = getattr(s.prior, nm)
        pr.use = np.asarray(pr.use, bool) & np.asarray(getattr(s.bundle.est, nm), bool)
    s = o.buildserialindices(s)
    x0 = o.serialize(s)
    w = o.buildweightvector(s)
    perm = np.random.default_rng(seed).permutation(len(w))

    def res_fun(x, jac):
        if not jac:
            return o.brown_euler_cam4(x, s, False)[perm]
        r, J = o.brown_euler_cam4(x, s, True)
        return r[perm], J.tocsr()[perm].tocsc()

    x, code, n, final, T, rr, lam = o.levenberg_marquardt(res_fun, x0, w[perm], max_iter, o.term_relative(conv_tol),
                                                          -1e-10, -1e-10)
    return x, code, n, rr, lam


def lm_decision_margins(s, max_iter=20, conv_tol=1e-6):
    """The oracle's LM loop with its decisions instrumented: (iters, smallest relative margin |fNew - f| / f of
    any accept/reject decision `fNew < f` (levenberg_marquardt.m:166), distance of the termination test's
    ratio ||Jp|| / (tol ||r||) from 1 (as a factor >= 1) over all its evaluations (:217))."""
    import copy
    import dbat_oracle as o
    s = copy.deepcopy(s)
    for nm in ('IO', 'EO', 'OP'):
        pr = getattr(s.prior, nm)
        pr.use = np.asarray(pr.use, bool) & np.asarray(getattr(s.bundle.est, nm), bool)
    s = o.buildserialindices(s)
    x0 = o.serialize(s)
    w = o.buildweightvector(s)
    state = {'f': None, 'margin': np.inf, 'term': np.inf}

    def res_fun(x, jac):
        out = o.brown_euler_cam4(x, s, jac)
        r = out[0] if jac else out
        f = 0.5 * float(np.sum(w * r * r))
        if jac:
            state['f'] = f
        elif state['f']:
            state['margin'] = min(state['margin'], abs(f - state['f']) / state['f'])
        return out

    def term_fun(Jp, r):
        ratio = np.linalg.norm(Jp) / (conv_tol * np.linalg.norm(r))
        state['term'] = min(state['term'], max(ratio, 1 / ratio) if ratio > 0 else np.inf)
        return ratio <= 1

    x, code, n, final, T, rr, lam = o.levenberg_marquardt(res_fun, x0, w, max_iter, term_fun, -1e-10, -1e-10)
    return n, state['margin'], state['term']


def lm_count_is_stable(s, ito, margin=1e-9):
    """Is the oracle's LM iteration count `ito` a property of the problem?  Yes if every accept/reject decision
    and the termination test were taken with a margin far above rounding: an implementation that agrees with
    the oracle to ~1e-11 per iterate (GPU: different elimination order, closed-form model) then takes the same
    decisions.  Sampling re-ordered summations instead is not enough: camcal model 3 gives 6 iterations under
    five row permutations and 16 under the sixth (its last accepted step lowers ||r|| by 2e-14 relative)."""
    n, m, t = lm_decision_margins(s)
    return n == ito and m > margin and t > 1.0 + 1e-3


# ---------------------------------------------------------------- interior-orientation patterns (tests/test_io_patterns_*.py)
_STD8 = (0, 1, 2, 5, 6, 7, 8, 9)        # cc px py K1 K2 K3 P1 P2 at nK = 3, nP = 2
_ONE, _HALF = 'one', 'half'             # block of camera c: 1 | 1 for c < nc // 2, else 2 | an int k: c % k + 1

# name: (nK, nP, block rule, {block: estimated rows}, rows that take the block rule (None: all; the others block 1))
IO_PATTERNS = {
    'fixed-k0p0': (0, 0, _ONE, {}, None),
    'fixed-k5p5': (5, 5, _ONE, {}, None),
    'cc-only': (3, 2, _ONE, {1: (0,)}, None),
    'as-sk-only': (3, 2, _ONE, {1: (3, 4)}, None),
    'k0p0-cc-pp': (0, 0, _ONE, {1: (0, 1, 2)}, None),
    'k4p0-radial': (4, 0, _ONE, {1: (0, 5, 6, 7, 8)}, None),
    'all10': (3, 2, _ONE, {1: tuple(range(10))}, None),
    'k5p2-11cols': (5, 2, _ONE, {1: (0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11)}, None),
    'k5p2-all12': (5, 2, _ONE, {1: tuple(range(12))}, None),
    'half-fixed-half-std8': (3, 2, _HALF, {2: _STD8}, None),
    'half-cc-half-std8': (3, 2, _HALF, {1: (0,), 2: _STD8}, None),
    'half-std8-half-9': (3, 2, _HALF, {1: _STD8, 2: _STD8 + (3,)}, None),
    '2x-std8-interleaved': (3, 2, 2, {1: _STD8, 2: _STD8}, None),
    '2x-9-interleaved': (3, 2, 2, {1: _STD8 + (3,), 2: _STD8 + (3,)}, None),
    '3x-std8-interleaved': (3, 2, 3, {1: _STD8, 2: _STD8, 3: _STD8}, None),
    'cc-shared-K-per-group': (3, 2, _HALF, {1: _STD8, 2: _STD8}, (5, 6, 7)),
}

# (pattern, IO rows with a prior observation, IO prior rows of the adjustment: leading, estimated entries only)
IO_PRIOR_CASES = (('2x-9-interleaved', (0, 1, 2), 6), ('half-cc-half-std8', (0, 5), 3), ('all10', (3, 4), 2),
                  ('cc-shared-K-per-group', (0, 5, 6, 7), 7))


def io_pattern_struct(name, pattern, priors=None):
    """The synth scene `name` ('tiny', 'small') rebuilt through dbatstruct.make_struct with the interior-orientation
    set-up `pattern` of IO_PATTERNS: lens model (nK, nP), IO blocks and estimated IO rows (rows: 0 cc, 1 px, 2 py, 3 as,
    4 sk, 5.. K1..KnK, then P1..PnP); datum by dependency on camera 0.  The only place that knows the patterns.

    Values: the scene's cc, pp, K1-K3 and P1-P2 where the rows exist; as = 2e-3 and sk = -1e-3 everywhere, as start or as
    fixed values (the image points were made with as = sk = 0: a few pixels of misfit at x0, nothing the adjustment
    cannot absorb or leave in the residuals).  Further K start at 0.  'fixed-k5p5' gives K4, K5 and P3-P5 values at
    which each term moves a point in the image corner (r = 21.6 mm) by about a pixel: K4 = px / r^9, K5 = px / r^11, and --
    the tangential terms past P2 multiply the P1, P2 displacement, which is zero in the scene -- P1 = P2 = px / (3 r^2)
    with P3 = r^-2, P4 = r^-4, P5 = r^-6.  All of these, and cc, differ from camera to camera by the factor
    1 + 0.01 c / nc: the fixed values of a camera are its own, not its block's.

    priors: IO rows that get a prior observation -- use = True for EVERY camera (also where the entry is fixed or not
    the leading one of its block: the adjustment has to mask those), val = IO (1 + 1e-3) + 1e-4, std = |IO| 1e-2 + 1e-3.
    Returns (s, truth)."""
    from dbat_amd import synth
    from dbat_amd.dbatstruct import make_struct, seteoest_depend
    nK, nP, rule, est_rows, rows = IO_PATTERNS[pattern]
    base, truth = synth.make_scene(name)
    nc = base.EO.val.shape[1]
    nrow = 5 + nK + nP
    IO = np.zeros((nrow, nc))
    IO[0:3] = base.IO.val[0:3]
    IO[3], IO[4] = 2e-3, -1e-3
    IO[5:5 + min(nK, 3)] = base.IO.val[5:5 + min(nK, 3)]
    IO[5 + nK:5 + nK + min(nP, 2)] = base.IO.val[8:8 + min(nP, 2)]
    px = float(np.ravel(base.IO.sensor.pxSize)[0])
    if pattern == 'fixed-k5p5':
        r2 = 18.0 ** 2 + 12.0 ** 2
        percam = 1 + 0.01 * np.arange(nc) / nc
        IO[0] *= percam
        IO[8] = px / r2 ** 4.5 * percam
        IO[9] = -px / r2 ** 5.5 * percam
        IO[10] = px / (3 * r2) * percam
        IO[11] = -px / (3 * r2) * percam
        IO[12] = 1 / r2 * percam
        IO[13] = -1 / r2 ** 2 * percam
        IO[14] = 1 / r2 ** 3 * percam
    cam = np.arange(nc)
    group = np.ones(nc, int) if rule == _ONE else (1 + (cam >= nc // 2) if rule == _HALF else cam % rule + 1)
    block = np.ones((nrow, nc), np.int32)
    block[list(range(nrow)) if rows is None else list(rows)] = group[None, :]
    est = np.zeros((nrow, nc), bool)
    for g, rr in est_rows.items():
        est[np.ix_(list(rr), np.flatnonzero(group == g))] = True
    prior = None
    if priors:
        pr = list(priors)
        use, val, std = np.zeros((nrow, nc), bool), np.full((nrow, nc), np.nan), np.full((nrow, nc), np.nan)
        use[pr], val[pr], std[pr] = True, IO[pr] * (1 + 1e-3) + 1e-4, np.abs(IO[pr]) * 1e-2 + 1e-3
        prior = (use, val, std)
    s = make_struct(IO, base.EO.val, base.OP.val, base.IP.val, base.IP.cam, base.IP.pt, px, ip_std=base.IP.std,
                    distModel=3, nK=nK, nP=nP, estIO=est, IOblock=block, priorIO=prior)
    s = seteoest_depend(s, 0)
    s.damping = base.damping
    return s, truth
