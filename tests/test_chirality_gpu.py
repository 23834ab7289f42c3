"""The chirality veto and point_depths() on the device (dbat_hip_point_depths, dbat_hip_set_chirality, csrc/depth.hpp)
against the NumPy restatement of pm_multidepth.m / ptdepth.m of tests/test_chirality_cpu.py: the depths on tiled, heavy
and giant points; counts, minima and the argmin as exact functions of the device's own depths; points behind a camera
and NaN coordinates; the three damping loops with the built-in veto against the oracle with the restatement as its
vetoFun; a start that is behind already; the setting on a cached handle."""
import copy
import functools

import numpy as np
import pytest

import dbat_oracle as o
from helpers import crowded_struct, giant_points_struct, lm_count_is_stable, relerr, synth_struct
from test_chirality_cpu import behind_start, near_start, oracle_veto, ref_depths, shrink_start

pytestmark = pytest.mark.gpu

TOL_X = 1e-6           # converged parameters, relative (tests/test_hip_parity.py)
TOL_HIST = 1e-8        # residual and damping histories, relative


@pytest.fixture(scope='module')
def hip():
    from dbat_amd import _hip
    import torch
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    _hip.load()
    return _hip


@functools.lru_cache(maxsize=None)
def tiny(variant='plain'):
    return synth_struct('tiny', variant)[0]


def check_depths(s, pd):
    """pd = point_depths(s) against the restatement, and its statistics against its own depths."""
    d_ref = ref_depths(s)
    cam, pt = np.asarray(s.IP.cam), np.asarray(s.IP.pt)
    dist = np.linalg.norm(s.OP.val[:, pt] - s.EO.val[0:3, cam], axis=0)
    assert pd.depth.shape == d_ref.shape
    assert np.all(np.abs(pd.depth - d_ref) <= 1e-12 * dist), np.max(np.abs(pd.depth - d_ref) / dist)
    nc = s.EO.val.shape[1]
    img = np.array([pd.depth[cam == i].min() if np.any(cam == i) else np.nan for i in range(nc)])
    assert np.array_equal(pd.image_min, img, equal_nan=True)
    assert pd.min_depth == pd.depth.min() and pd.argmin == int(np.argmin(pd.depth))
    assert pd.n_behind == np.count_nonzero(~(pd.depth > 0)) and np.array_equal(pd.behind, np.flatnonzero(~(pd.depth > 0)))


def same_bits(a, b):
    return all(np.array_equal(np.asarray(getattr(a, k)), np.asarray(getattr(b, k)), equal_nan=True)
               for k in ('depth', 'n_behind', 'behind', 'min_depth', 'argmin', 'image_min'))


@pytest.mark.parametrize('variant', ['plain', 'selfcal', 'priors', 'groups4'])
def test_depths_match_the_reference_definition(hip, variant):
    from dbat_amd import point_depths
    s = tiny(variant)
    a, b = point_depths(s), point_depths(s)
    assert a.depth.shape == (1800,) and a.n_behind == 0 and a.min_depth > 0
    check_depths(s, a)
    assert same_bits(a, b)


@pytest.mark.parametrize('kind', ['crowded-heavy', 'giant'])
def test_depths_on_heavy_and_giant_points(hip, kind, monkeypatch):
    """The plan's reordering of heavy and giant points (the second part of the camera-major copy) against the scatter
    back to IP-column order: the heavy route of tests/test_crowded_batches_gpu.py and the giant points of
    tests/test_hip_parity.py, at their sizes."""
    from dbat_amd import point_depths
    if kind == 'crowded-heavy':
        monkeypatch.setenv('DBAT_HIP_CMAX', '6')
        s = crowded_struct('fixed', control=12, cams=20, points=700)[0]
    else:
        s = giant_points_struct(140, 500)[0]
    hip.clear_cache()
    try:
        h = hip.Handle(s)
        try:
            info = h.info()
        finally:
            h.close()
        assert (info['heavy_tasks'] > 0 and info['n_tiles'] == 0) if kind == 'crowded-heavy' else info['heavy_points'] >= 3
        a, b = point_depths(s), point_depths(s)
        check_depths(s, a)
        assert same_bits(a, b)
    finally:
        hip.clear_cache()


def test_points_behind_a_camera_are_counted_exactly(hip):
    from dbat_amd import point_depths
    s = behind_start(tiny())
    d_ref = ref_depths(s)
    assert np.min(np.abs(d_ref)) > 1e-9                 # (no comparison below hinges on rounding)
    behind = np.flatnonzero(d_ref <= 0)
    assert len(behind) == 5
    pd = point_depths(s)
    check_depths(s, pd)
    assert pd.n_behind == len(behind) and np.array_equal(pd.behind, behind)
    assert pd.argmin == int(np.argmin(d_ref)) and abs(pd.min_depth - d_ref.min()) < 1e-11
    # a NaN coordinate: every observation of that point counts as behind
    p = 17
    cols = np.flatnonzero(np.asarray(s.IP.pt) == p)
    assert len(cols) >= 2 and not np.any(np.isin(cols, behind))
    s.OP.val[1, p] = np.nan
    pn = point_depths(s)
    assert np.all(np.isnan(pn.depth[cols])) and np.count_nonzero(np.isnan(pn.depth)) == len(cols)
    assert pn.n_behind == len(behind) + len(cols) and np.array_equal(pn.behind, np.union1d(behind, cols))
    assert pn.min_depth == pd.min_depth and pn.argmin == pd.argmin          # (the smallest depth that is a number)
    hip.clear_cache()


# The starts.  The recipes of the three loops were to be: (a) 'lm' on shrink_start seed 4, (b) 'lmp' on shrink_start seed 1,
# (c) 'gna' on a start with default_rng(4).normal(0, 0.3, .) added to the estimated camera angles.  On the oracle (b) is as
# recorded below.  (a) and (c) are not: in no run of their recipes that converges is a trial point ever rejected (seeds
# 0 .. 79 of each; the depths of the trial points of (a) stay above 5, the only runs of (c) with a rejection end with code
# -3) -- so a
# test on them would pass with the veto ignored.  Their starts are therefore near_start's (eight points close in front of a
# camera: the first steps throw some of them behind it), the first seeds, counted from 0, that meet the conditions
# asserted below from the oracle's own log: code 0 with the veto, at least one trial point rejected, every depth of every
# trial point farther from zero than 1e-6, and for 'lm' every accept / reject decision and the termination test of both
# courses, with and without the veto, decided by margins far above rounding (helpers.lm_decision_margins: relative margin
# > 1e-9, termination ratio off 1 by more than 1e-3 -- the thresholds of helpers.lm_count_is_stable).  At the default
# convTol = 1e-6 NO `tiny` start meets the last condition (tests/test_abi_cpu.py::test_lm_count_stability_helper: the
# trailing decisions of levenberg_marquardt.m compare values that differ by 1e-14 relative), so (a) runs at convTol = 1e-3,
# where tests/test_hip_parity.py asserts Levenberg-Marquardt counts as well.
# (case, start, seed, damping, extra arguments, oracle with the veto: (code, iterations, tested, rejected), iterations without)
LOOP_CASES = [
    ('a', near_start, 15, 'lm', (1e-3,), (0, 17, 17, 7), 14),
    ('b', shrink_start, 1, 'lmp', (), (0, 8, 8, 2), None),
    ('c', near_start, 20, 'gna', (), (0, 11, 12, 1), None),
]
CASE = {c[0]: c for c in LOOP_CASES}


def lm_margins(s, conv_tol, veto=None):
    """helpers.lm_decision_margins with a vetoFun: (iterations, smallest relative margin of a decision `fNew < f`,
    distance of the termination ratio from 1 as a factor)."""
    s = copy.deepcopy(s)
    for nm in ('IO', 'EO', 'OP'):
        pr = getattr(s.prior, nm)
        pr.use = np.asarray(pr.use, bool) & np.asarray(getattr(s.bundle.est, nm), bool)
    s = o.buildserialindices(s)
    x0, w = o.serialize(s), o.buildweightvector(s)
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
    n = o.levenberg_marquardt(res_fun, x0, w, 40, term_fun, -1e-10, -1e-10, False, veto)[2]
    return n, state['margin'], state['term']


@functools.lru_cache(maxsize=None)
def oracle_run(case):
    """The oracle with the restatement's veto on the start of a case: (s, result tuple, log of the veto)."""
    _, start, seed, damping, extra, _, _ = CASE[case]
    s = start(tiny(), seed)
    log = []
    return s, o.bundle(s, damping, 40, *extra, vetoFun=oracle_veto(s, log)), log


def damping_history(E):
    d = E.damping
    return np.asarray({'gna': lambda: d.alpha, 'lm': lambda: d.__dict__['lambda'], 'lmp': lambda: d.delta}[d.name](), float)


def check_course(E, iters, Eo, ito):
    assert E.code == Eo.code and iters == ito
    assert len(E.res) == len(Eo.res) and relerr(E.res, Eo.res) < TOL_HIST
    n = ito + 1 if E.damping.name == 'lmp' else None
    a, b = damping_history(E)[:n], damping_history(Eo)[:n]
    assert len(a) == len(b) and relerr(a, b) < TOL_HIST


@pytest.mark.parametrize('case', [c[0] for c in LOOP_CASES])
def test_loops_with_the_veto_take_the_oracles_course(hip, case):
    from dbat_amd import bundle
    _, _, _, damping, extra, (code, iters_o, tested, rejected), noveto = CASE[case]
    s, (ro, oko, ito, s0o, Eo), log = oracle_run(case)
    # the oracle's own log first: the recorded counts, and no decision near rounding
    assert (Eo.code, ito, len(log), sum(1 for nb, _ in log if nb)) == (code, iters_o, tested, rejected)
    assert rejected > 0 and min(abs(d) for _, d in log) > 1e-6
    assert np.count_nonzero(ref_depths(s) <= 0) == 0    # (the start itself is in front: the veto acts on trial points)
    if damping == 'lm':
        for veto, n_exp in ((None, noveto), (oracle_veto(s), iters_o)):
            n, margin, term = lm_margins(s, extra[0], veto)
            assert n == n_exp and margin > 1e-9 and term > 1.0 + 1e-3, (n, margin, term)
    res, ok, iters, s0, E = bundle(s, damping, 40, *extra, True)
    assert ok and oko and E.chirality is True
    check_course(E, iters, Eo, ito)
    assert (E.veto.tested, E.veto.rejected) == (tested, rejected)
    last = [(nb, d) for nb, d in log if nb][-1]
    assert E.veto.n_behind == last[0] and E.veto.min_depth < 0
    assert relerr(E.x, Eo.x) < TOL_X
    # the host callback in place of the flag: the same course
    res2, ok2, iters2, _, E2 = bundle(s, damping, 40, *extra, veto_fun=oracle_veto(s))
    assert ok2 and E2.chirality is False and E2.veto is None
    check_course(E2, iters2, Eo, ito)
    # both: either one rejects, so again the same course
    res3, ok3, iters3, _, E3 = bundle(s, damping, 40, *extra, True, veto_fun=oracle_veto(s))
    check_course(E3, iters3, Eo, ito)
    assert (E3.veto.tested, E3.veto.rejected) == (tested, rejected)
    if noveto is not None:                              # neither: the other course
        assert bundle(s, damping, 40, *extra)[2] == noveto != iters_o
    hip.clear_cache()


def test_a_start_that_is_behind_is_rejected_at_every_trial_point(hip):
    from dbat_amd import bundle
    s = behind_start(tiny())
    val0 = [np.array(getattr(s, nm).val) for nm in ('IO', 'EO', 'OP')]
    for damping, code in (('gna', -3), ('lm', -1)):
        log = []
        ro, oko, ito, _, Eo = o.bundle(s, damping, 40, vetoFun=oracle_veto(s, log))
        assert Eo.code == code and not oko and len(log) > 0 and all(nb > 0 for nb, _ in log)
        assert min(abs(d) for _, d in log) > 1e-6
        if damping == 'gna':
            # alpha = 1, 1/2, ... 2^-29 >= alphaMin = 1e-9: 30 trial points; the first fails the test on f and is not shown
            assert ito == 1 and len(log) == 29
        res, ok, iters, s0, E = bundle(s, damping, 40, True)
        assert not ok and E.code == Eo.code == code and iters == ito
        assert E.veto.tested == E.veto.rejected == len(log)
        assert E.veto.n_behind == log[-1][0]
        for nm, v in zip(('IO', 'EO', 'OP'), val0):       # bundle.m:356-358: s is returned as it came
            assert np.array_equal(getattr(res, nm).val, v)
    hip.clear_cache()


def test_the_setting_does_not_leak_into_the_cached_handle(hip):
    from dbat_amd import bundle, BadInput
    s = CASE['a'][1](tiny(), CASE['a'][2])
    hip.clear_cache()
    r1 = bundle(s, 'lm', 40, 1e-3, True)
    assert r1[4].veto.rejected > 0
    r2 = bundle(s, 'lm', 40, 1e-3)
    assert hip.cache_stats['last'] == 'hit' and r2[4].chirality is False and r2[4].veto is None
    r3 = bundle(s, 'lm', 40, 1e-3, reuse_handle=False)
    assert r2[2] == r3[2] != r1[2] and relerr(r2[4].x, r3[4].x) < 1e-9
    # bit for bit: with the sums in a fixed order -- the default mode's atomics reorder them, on one handle as on two
    r1 = bundle(s, 'lm', 40, 1e-3, True, deterministic=True)
    r2 = bundle(s, 'lm', 40, 1e-3, deterministic=True)
    assert hip.cache_stats['last'] == 'hit' and r2[4].veto is None
    r3 = bundle(s, 'lm', 40, 1e-3, deterministic=True, reuse_handle=False)
    assert r2[2] == r3[2] != r1[2]
    assert np.array_equal(r2[4].x, r3[4].x) and np.array_equal(r2[4].res, r3[4].res)
    assert np.array_equal(r2[4].damping.__dict__['lambda'], r3[4].damping.__dict__['lambda'])
    with pytest.raises(BadInput, match='one-rank'):
        bundle(s, 'lm', True, comm=type('Comm', (), dict(rank=0, world_size=2))())
    hip.clear_cache()


def test_c_abi_refuses_what_is_not_built(hip):
    s = tiny()
    h = hip.Handle(s)
    try:
        with pytest.raises(hip.DbatHipError):
            h.set_chirality(True, np.inf)
        h.set_chirality(True, 0.0)
        opt = hip.default_options('lm')
        with pytest.raises(hip.DbatHipError, match='chirality'):
            h.solve_robust(h.serialize(), opt, hip.robust_options('huber'))
        h.set_chirality(False)
        assert h.chirality_stats()[:3] == (0, 0, 0)
    finally:
        h.close()
