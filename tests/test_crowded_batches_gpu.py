"""GPU parity on scenes whose batches hold many points: most points seen in ONE image and held by something else -- fixed
(control points measured in one image), a prior on all three coordinates, a prior or a fixed value of Z (mono-plotting).
A batch is cut at BT = 256 observations, so such points would put up to 256 points into one batch, while the build
kernels that work batch by batch (k_build_tile2, k_build_tile3, k_heavy_z) hold their per-point sums in LDS for
Plan::PMAX = 128 points.  The plan closes a batch at PMAX points (tests/test_batch_points_cpu.py shows that these scenes
reach the cap); here every build route runs them against the oracle's full sparse solve."""
import copy

import numpy as np
import pytest
import scipy.sparse as sp

import dbat_oracle as o
from helpers import check_linearisation_figures, crowded_struct, linearisation_figures, relerr

pytestmark = pytest.mark.gpu

TOL_STEP = 1e-8
TOL_X = 1e-7

# route: (environment, self-calibration, cameras of the control point, (cameras, points), kernel of the tiled points,
# heavy tasks); the same scenes as tests/test_batch_points_cpu.py
ROUTES = {
    'sig': ({}, False, 0, (60, 3000), 'k_build_sig', False),
    'tile3': ({'DBAT_HIP_SIG': '0'}, False, 0, (60, 3000), 'k_build_tile3', False),
    'tile2': ({'DBAT_HIP_SIG': '0'}, True, 0, (60, 3000), 'k_build_tile2', False),
    'heavy': ({'DBAT_HIP_CMAX': '6'}, False, 12, (20, 700), None, True),
    'heavy-selfcal': ({'DBAT_HIP_CMAX': '6'}, True, 12, (20, 700), None, True),
    'columns': ({'DBAT_HIP_CMAX': '6', 'DBAT_HIP_HEAVY': '0', 'DBAT_HIP_SIG': '0'}, False, 12, (60, 3000),
                'k_build_tile3', False),
    'columns-selfcal': ({'DBAT_HIP_CMAX': '6', 'DBAT_HIP_HEAVY': '0', 'DBAT_HIP_SIG': '0'}, True, 12, (60, 3000),
                        'k_build_tile2', False),
    'bt128': ({'DBAT_HIP_BT': '128'}, False, 0, (60, 3000), 'k_build', False),
}
STEP_CASES = [(r, k) for r, kinds in (('sig', ('fixed', 'prior3')),
                                       ('tile3', ('fixed', 'prior3', 'zprior', 'zfixed')),
                                       ('tile2', ('fixed', 'prior3', 'zprior', 'zfixed')),
                                       ('heavy', ('fixed', 'prior3', 'zprior', 'zfixed')),
                                       ('heavy-selfcal', ('fixed', 'zprior')),
                                       ('columns', ('fixed', 'prior3')),
                                       ('columns-selfcal', ('fixed', 'zfixed')),
                                       ('bt128', ('fixed', 'zprior')))
              for k in kinds]


@pytest.fixture(scope='module')
def hip():
    from dbat_amd import _hip
    import torch
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    _hip.load()
    return _hip


def scene(route, kind, monkeypatch):
    """The route's environment set, and its scene."""
    env, selfcal, control, size, _, _ = ROUTES[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s, _ = crowded_struct(kind, selfcal=selfcal, control=control, cams=size[0], points=size[1])
    return s


def check_route(hip, h, s, route):
    """The handle runs the route's kernels, and its batches came up against the point cap."""
    _, _, control, _, kernel, heavy = ROUTES[route]
    info = h.info()
    st = hip.batch_stats(s)
    if heavy:
        assert info['heavy_tasks'] > 0 and info['n_tiles'] == 0
        assert h.build_kernel_name() == 'k_heavy_z + k_heavy_syrk'
        assert st['untiled']['closed_by_cap'] > 0
    else:
        assert info['heavy_tasks'] == 0 and h.build_kernel_name() == kernel
        assert (info['n_tiles'] > 0) == (route != 'bt128')
        if route != 'bt128':                            # (128-observation batches never reach 128 points)
            assert st['tiled']['closed_by_cap'] > 0
        if control:                                     # the control point alone, by column lists (k_build)
            assert st['n_batches_untiled'] == 1 and st['untiled']['max_obs'] == control
    for part in ('tiled', 'untiled'):
        assert st[part]['max_points'] <= st['PMAX'] and st[part]['max_obs'] <= st['BT']


def oracle_setup(s):
    s = copy.deepcopy(s)
    for nm in ('IO', 'EO', 'OP'):
        pr = getattr(s.prior, nm)
        pr.use = np.asarray(pr.use, bool) & np.asarray(getattr(s.bundle.est, nm), bool)
    s = o.buildserialindices(s)
    return s, o.serialize(s), o.buildweightvector(s)


@pytest.mark.parametrize('route,kind', STEP_CASES, ids=['%s-%s' % c for c in STEP_CASES])
def test_step_parity_crowded_batches(hip, route, kind, monkeypatch):
    """One linearisation + solve, scaled Gauss-Newton and damped, against the oracle's full sparse normal equations;
    the gradient and the step's scalars as in test_hip_parity.py::test_step_parity, and its column norms, trace(J'J),
    ||J v||^2 and J v (bar 1e-10; largest on the MI355X over the 22 cases: 5.6e-16, 5.9e-16, 5.8e-16, 1.0e-15)."""
    s = scene(route, kind, monkeypatch)
    so, x0, w = oracle_setup(s)
    R = np.sqrt(w)
    r_o, K = o.brown_euler_cam4(x0, so, jac=True)
    r = R * r_o
    J = (sp.diags(R) @ K).tocsc()
    p_o, *_ = o._scaled_gn(J, r)
    JTJ = (J.T @ J).tocsc()
    lam = 1e-4 * JTJ.diagonal().sum() / J.shape[1]
    q_o, _ = o.normal_solve((JTJ + lam * sp.identity(J.shape[1])).tocsc(), -(J.T @ r))
    h = hip.Handle(s)
    try:
        check_route(hip, h, s, route)
        p_h, st = h.linearize_solve(x0, 0.0, True)
        assert not st['singular']
        assert relerr(p_h, p_o) < TOL_STEP
        Jp = J @ p_o
        assert abs(st['JpJp'] - Jp @ Jp) <= 1e-7 * (Jp @ Jp)
        assert abs(st['rJp'] - r @ Jp) <= 1e-7 * abs(r @ Jp)
        assert abs(st['pp'] - p_o @ p_o) <= 1e-7 * (p_o @ p_o)
        assert relerr(h.gradient(), J.T @ r) < 1e-10
        q_h, st2 = h.linearize_solve(x0, lam, False)
        assert relerr(q_h, q_o) < TOL_STEP
        # what no step shows (the scaled step is invariant under any column scaling): column norms, trace(J'J), J v
        check_linearisation_figures(linearisation_figures(h, J, st2['trace']), '%s-%s' % (route, kind))
    finally:
        h.close()


BUNDLE_CASES = [('tile3', 'fixed'), ('tile3', 'zprior'), ('tile2', 'fixed'), ('tile2', 'prior3'),
                ('heavy', 'fixed'), ('heavy', 'zfixed'), ('heavy-selfcal', 'prior3')]


@pytest.mark.parametrize('route,kind', BUNDLE_CASES, ids=['%s-%s' % c for c in BUNDLE_CASES])
def test_bundle_parity_crowded_batches(hip, route, kind, monkeypatch):
    """The whole adjustment: the same outcome, the same number of iterations and the same parameters as the oracle."""
    from dbat_amd import bundle
    s = scene(route, kind, monkeypatch)
    hip.clear_cache()
    try:
        res, ok, iters, s0, E = bundle(s, 'gna')
    finally:
        hip.clear_cache()
    ro, oko, ito, s0o, Eo = o.bundle(s, 'gna')
    assert ok == oko and E.code == Eo.code and iters == ito
    assert ok and relerr(E.x, Eo.x) < TOL_X


@pytest.mark.parametrize('route,kind', [('tile3', 'prior3'), ('heavy', 'zprior')])
def test_posterior_covariance_crowded_batches(hip, route, kind, monkeypatch):
    """Posterior covariances of single-ray points held by priors: their blocks come from V^-1 of the build."""
    from dbat_amd import bundle, bundle_cov
    s = scene(route, kind, monkeypatch)
    hip.clear_cache()
    try:
        res, ok, iters, s0, E = bundle(s, 'gna')
        got = bundle_cov(res, E, 'COP', 'CEO')
    finally:
        hip.clear_cache()
    ro, oko, ito, s0o, Eo = o.bundle(s, 'gna')
    assert ok and oko
    want = o.bundle_cov(ro, Eo, 'COP', 'CEO')
    for A, B in zip(got, want):
        assert A.shape == B.shape and abs(B).max() > 0
        assert abs(A - B).max() <= 1e-6 * abs(B).max()


@pytest.mark.parametrize('route,kind', [('tile3', 'fixed'), ('tile3', 'zprior'), ('tile2', 'fixed'), ('tile2', 'prior3')])
def test_deterministic_mode_crowded_batches(hip, route, kind, monkeypatch):
    """Deterministic mode (exact sums, its own per-batch lists): three steps repeat bit for bit and agree with the
    default step."""
    s = scene(route, kind, monkeypatch)
    h = hip.Handle(s)
    try:
        check_route(hip, h, s, route)
        x0 = h.serialize()
        p_default, _ = h.linearize_solve(x0, 0.0, True)
        h.set_deterministic(True)
        ref = None
        for _ in range(3):
            p, st = h.linearize_solve(x0, 0.0, True)
            assert not st['singular']
            if ref is None:
                ref = p.copy()
            assert np.array_equal(p, ref), relerr(p, ref)
        assert relerr(ref, p_default) < 1e-8
    finally:
        h.close()
