"""The seeded cases of the initial-value edge tests (tests/test_initial_ref_cpu.py fixes their conditioning on the CPU;
tests/test_resect_edges_gpu.py and tests/test_forwintersect_edges_gpu.py run them on the device).  References:
tests/resect_ref.py (longdouble) and oracle/initial_oracle.py (the float64 restatement)."""
import numpy as np

import resect_ref as RR

SHIFT = (6.5e5, 6.2e6, 100.0)          # project coordinates of the size the sxb project has
RESECT_DRAWN = 40                      # seeds drawn; the first RESECT_USED survivors go to the device
RESECT_USED = 20
RESECT_CAP = 1e-9                      # float64 restatement against longdouble, relative pose error (see pose_errors)
EPS = np.finfo(float).eps


def pose_errors(P, Pref):
    """(eP, eR, eC): max |P - Pref| over the twelve entries, over the rotation part, and of the centre -R't (taken in
    longdouble from either matrix)."""
    eP = RR.pose_err(P, Pref)
    eR = RR.pose_err(np.asarray(P)[:, :3], np.asarray(Pref)[:, :3])
    eC = float(np.max(np.abs(RR.centre_ld(P) - RR.centre_ld(Pref))))
    return eP, eR, eC


def oracle_pose(case):
    """The float64 restatement's winning pose of a case (initial_oracle.pm_resect_3pt), or None."""
    import initial_oracle as IO_
    use = np.zeros(case['X'].shape[1], bool)
    use[case['tri']] = True
    return IO_.pm_resect_3pt(case['X'], case['x'], use, True)[0]


def resect_case(seed, shift=None, **kw):
    """seeded_case with the longdouble reference's winner (Pref, rms_ref, all candidates) and the float64
    restatement's errors against it: rel = max(eP / max|Pref|) for a case at the origin; for a shifted case
    max(eR, eC / max|C|) -- the matrix's fourth column then only repeats the centre's size."""
    c = RR.seeded_case(seed, shift=shift, **kw)
    c['cands'] = RR.resect_3pt(c['X'], c['x'], c['tri'])
    c['Pref'], c['rms_ref'] = RR.best_pose(c['cands'])
    Po = oracle_pose(c)
    c['Po'] = Po
    if Po is None or c['Pref'] is None:
        c['oracle_err'], c['rel'] = (np.inf, np.inf, np.inf), np.inf
        return c
    eP, eR, eC = pose_errors(Po, c['Pref'])
    c['oracle_err'] = (eP, eR, eC)
    if shift is None:
        c['rel'] = eP / float(np.max(np.abs(c['Pref'])))
    else:
        c['rel'] = max(eR, eC / float(np.max(np.abs(RR.centre_ld(c['Pref'])))))
    return c


_cache = {}


def resect_cases(shift=None):
    """(used, drawn): the first RESECT_USED of the RESECT_DRAWN seeds whose float64 restatement stays under RESECT_CAP,
    and all drawn cases.  Computed once; the callers leave them unchanged."""
    key = ('resect', shift)
    if key not in _cache:
        drawn = [resect_case(seed, shift=shift) for seed in range(RESECT_DRAWN)]
        used = [c for c in drawn if c['rel'] < RESECT_CAP][:RESECT_USED]
        _cache[key] = (used, drawn)
    return _cache[key]


# ---- forward intersection ----------------------------------------------------------------------------------------------

LENS = np.array([3.1e-4, -2.3e-7, 1.7e-10, 2.1e-5, -1.3e-5])      # K1 K2 K3 P1 P2: none of them zero


def set_lens(s, pp_too=False):
    """Non-zero K1..K3, P1, P2 in IO.val (the synthetic default has K3 = P1 = P2 = 0, under which a wrong distortion
    term passes), different in every IO block so that a ray corrected with another camera's lens is seen; pp_too: the
    principal point differs from block to block as well (image-variant IO)."""
    nK, nP = int(s.IO.model.nK), int(s.IO.model.nP)
    assert nK == 3 and nP >= 2
    blk = np.asarray(s.IO.struct.block)
    for j in range(5):
        r = 5 + j
        s.IO.val[r] = LENS[j] * (1.0 + 0.125 * (blk[r] % 5))
    if pp_too:
        for r in (1, 2):
            s.IO.val[r] = s.IO.val[r] + 0.015625 * (blk[r] % 7)
    return s


def _shifted(s, shift):
    s.EO.val[:3] += np.asarray(shift, float)[:, None]
    s.OP.val[:] += np.asarray(shift, float)[:, None]
    return s


def _keep_obs(s, keep):
    s.IP.val, s.IP.std = np.asfortranarray(s.IP.val[:, keep]), np.asfortranarray(s.IP.std[:, keep])
    s.IP.cam, s.IP.pt = s.IP.cam[keep], s.IP.pt[keep]
    return s


def ray_count_scene():
    """'tiny' with object point 0 without any ray, 1 with one, 2 with two and 3 with three."""
    from helpers import synth_struct
    s = synth_struct('tiny')[0]
    pt = np.asarray(s.IP.pt)
    keep = np.ones(pt.size, bool)
    for p in range(4):
        rows = np.flatnonzero(pt == p)
        assert rows.size >= 3
        keep[rows[p:]] = False
    return _keep_obs(s, keep)


def angle_scene(theta, shift=None, points=40):
    """Two images whose rays meet at about theta rad in every one of `points` points: projection centres 40 theta m
    apart at a height of 40 m, the synthetic lens, half a pixel of noise."""
    from dbat_amd import synth
    from dbat_amd.dbatstruct import make_struct, seteoest_depend
    rng = np.random.default_rng(777)
    cam0 = synth.ROMA_CAM
    px = cam0['sensor'][1] / cam0['imsz'][1]
    IO = np.zeros((10, 2))
    IO[0] = cam0['cc']; IO[1] = cam0['pp'][0]; IO[2] = -cam0['pp'][1]
    IO[5:8] = -np.array(cam0['K'])[:, None]
    b = 40.0 * theta
    EO = np.zeros((6, 2))
    EO[0] = [20.0 - b / 2, 20.0 + b / 2]; EO[1] = 20.0; EO[2] = 40.0
    EO[3:5] = rng.uniform(-0.05, 0.05, (2, 2)); EO[5] = rng.uniform(-np.pi, np.pi, 2)
    OP = np.vstack([rng.uniform(12, 28, (2, points)), rng.uniform(0, 2, (1, points))])
    cam = np.repeat(np.arange(2, dtype=np.int32), points)
    pt = np.tile(np.arange(points, dtype=np.int32), 2)
    uv, depth = synth.project(IO, EO, OP, cam, pt, px)
    assert np.all(depth < 0)
    uv = uv + rng.normal(0, 0.5, uv.shape)
    s = seteoest_depend(make_struct(IO, EO, OP, uv, cam, pt, px, ip_std=1.0, distModel=3), 0)
    return s if shift is None else _shifted(s, shift)


def np3_scene():
    """'tiny' with a third tangential coefficient (nP = 3: the radial scaling 1 + P3 of the tangential terms)."""
    from helpers import synth_struct
    from dbat_amd.dbatstruct import make_struct, seteoest_depend
    s = set_lens(synth_struct('tiny')[0])
    IO = np.vstack([s.IO.val, np.full((1, s.IO.val.shape[1]), 0.25)])
    px = float(np.ravel(s.IO.sensor.pxSize)[0])
    return seteoest_depend(make_struct(IO, s.EO.val[:6], s.OP.val, s.IP.val, s.IP.cam, s.IP.pt, px, ip_std=1.0, distModel=3,
                                       nK=3, nP=3), 0)


def camcal_scene(model):
    from helpers import camcal_struct
    s = camcal_struct(model)
    assert int(s.IO.model.nK) == 3 and int(s.IO.model.nP) == 2
    s.IO.val[5:10] = (LENS * np.array([1, 1, 1, 0.1, 0.1]))[:, None]      # (a 7.3 mm lens: r up to 4 mm)
    return s


FWD_SCENES = ('tiny-selfcal', 'tiny-imagevar', 'tiny-groups4', 'tiny-np3', 'camcal-m1', 'camcal-m2', 'camcal-m4', 'camcal-m5',
              'batch-edge', 'ray-counts', 'tiny-far',
              'angle-1e-1', 'angle-1e-2', 'angle-1e-3', 'angle-1e-1-far', 'angle-1e-2-far', 'angle-1e-3-far')


def fwd_scene(name):
    from helpers import synth_struct, giant_points_struct, all_see_all_scene
    if name in ('tiny-selfcal', 'tiny-groups4'):
        return set_lens(synth_struct('tiny', name[5:])[0])
    if name == 'tiny-imagevar':
        return set_lens(synth_struct('tiny', 'imagevar')[0], pp_too=True)
    if name == 'tiny-np3':
        return np3_scene()
    if name.startswith('camcal-m'):
        return camcal_scene(int(name[-1]))
    if name == 'giant':
        return giant_points_struct(140, 500, 'selfcal')[0]
    if name == 'batch-edge':                       # eight rays per point: 32 points fill a batch of 256 exactly
        return all_see_all_scene(8, 70, False)[0]
    if name == 'ray-counts':
        return ray_count_scene()
    if name == 'tiny-far':
        return _shifted(synth_struct('tiny')[0], SHIFT)
    if name.startswith('angle-'):
        far = name.endswith('-far')
        return angle_scene(float(name[6:10]), SHIFT if far else None)
    raise ValueError(name)


def fwd_reference(name):
    """(s, Qld, Qo, oracle_err, cap, scale) of a scene, computed once: the longdouble points, the float64
    restatement's, its largest error against longdouble over the points both have, the cap that error must stay
    under -- 64 eps * cond * max|coordinate| with cond the largest condition number of a point's 3 x 3 matrix (the
    error of solving it in float64 from data of that size; 4 / theta^2 for two rays theta apart) -- and
    max|coordinate| over the projection centres and the points."""
    key = ('fwd', name)
    if key not in _cache:
        import initial_oracle as IO_
        s = fwd_scene(name)
        Qld, cond = RR.forwintersect_ld(s, want_cond=True)
        Qo = IO_.forwintersect(s).OP.val
        ok = np.isfinite(np.asarray(Qld, float)).all(0)
        assert np.array_equal(ok, np.isfinite(Qo).all(0))
        scale = float(max(np.abs(s.EO.val[:3]).max(), np.abs(np.asarray(Qld[:, ok], float)).max()))
        err = float(np.max(np.abs(RR.LD(1) * Qo[:, ok] - Qld[:, ok])))
        cap = 64 * EPS * float(np.max(cond[ok])) * scale
        _cache[key] = (s, Qld, Qo, err, cap, scale)
    return _cache[key]
