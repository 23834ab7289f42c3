"""Interior-orientation patterns and prior observations of IO parameters on every device route, against the oracle.

The camera-side column maps (cam_ncol / cam_col / cam_iorow per camera; tile_iocols / tile_cam_io / tile_io_simple per
tile) decide which instantiation of the build, camera-normal and back-substitution kernels runs and which column of
the reduced system every IO derivative lands in.  helpers.IO_PATTERNS spans them: lens models other than nK = 3,
nP = 2, sparse patterns on the select chain of io_columns, more than nine IO columns per camera (nothing tiled),
cameras with different column counts in one project, std8 cameras that take their rows from different blocks, and
interleaved blocks that put 18 or 24 IO columns under one point (heavy).  helpers.IO_PRIOR_CASES adds prior
observations of IO parameters (n_prior[0], the z_prw / z_prv of the IO unknowns).  tests/test_io_patterns_cpu.py pins
the route the plan gives every pattern; the tests here are tests of that route.

All tolerances are the project's own: TOL_BLOCK, TOL_STEP, TOL_X of tests/test_hip_parity.py, 1e-9 between two routes
(test_product_switches_leave_the_result_alone), 1e-6 of the largest entry for covariances
(test_posterior_covariance_synthetic), 1e-9 absolute for redundancy numbers (tests/test_reliability_gpu.py)."""
import functools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import scipy.sparse as sp

import dbat_oracle as o
from helpers import IO_PATTERNS, IO_PRIOR_CASES, io_pattern_struct, relerr
from test_hip_parity import TOL_BLOCK, TOL_STEP, TOL_X, assemble_J, check_history, oracle_setup
from test_io_patterns_cpu import SMALL_LAYOUT, TINY_LAYOUT, UNTILED, routes
from test_reliability_cpu import dense_reliability

pytestmark = pytest.mark.gpu

CASES = [(p, None) for p in IO_PATTERNS] + [(p, rows) for p, rows, _ in IO_PRIOR_CASES]
PRIOR_ROWS = {(p, rows): n for p, rows, n in IO_PRIOR_CASES}
_id = lambda c: c[0] + ('+prior' if c[1] else '')
ALL = pytest.mark.parametrize('case', CASES, ids=[_id(c) for c in CASES])
COV_CASES = [c for c in CASES if c[1] or c[0] in ('all10', 'k5p2-11cols', 'half-cc-half-std8', '2x-9-interleaved',
                                                   'cc-shared-K-per-group')]


@pytest.fixture(scope='module')
def hip():
    from dbat_amd import _hip
    import torch
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    _hip.load()
    return _hip


def _ref(scene, pattern, rows):
    """The oracle's linearisation at x0 and its two steps."""
    s, _ = io_pattern_struct(scene, pattern, rows)
    so, x0, w = oracle_setup(s)
    R = np.sqrt(w)
    r_o, K = o.brown_euler_cam4(x0, so, jac=True)
    r = R * r_o
    J = (sp.diags(R) @ K).tocsc()
    p, sing, Jn, *_ = o._scaled_gn(J, r)
    assert not sing
    JTJ = (J.T @ J).tocsc()
    lam = 1e-4 * JTJ.diagonal().sum() / J.shape[1]
    q, _ = o.normal_solve((JTJ + lam * sp.identity(J.shape[1])).tocsc(), -(J.T @ r))
    for a in (x0, w, r_o, r, p, q, Jn):
        a.setflags(write=False)
    return NS(s=s, so=so, x0=x0, w=w, R=R, r_o=r_o, r=r, J=J, p=p, q=q, Jn=Jn, lam=lam, trace=JTJ.diagonal().sum(),
              no=s.IP.val.shape[1])


@functools.lru_cache(maxsize=None)
def ref(scene, pattern, rows):
    """_ref, computed once per tiny case and shared among the tests (read-only)."""
    return _ref(scene, pattern, rows)


@functools.lru_cache(maxsize=None)
def ref_bundle(pattern, rows, damping):
    return o.bundle(io_pattern_struct('tiny', pattern, rows)[0], damping)


def check_step(h, F):
    """tests/test_hip_parity.py::test_step_parity on handle h against the shared reference F.  Returns the scaled step."""
    p_h, st = h.linearize_solve(F.x0, 0.0, True)
    assert not st['singular']
    print('scaled step %.2e' % relerr(p_h, F.p))
    assert relerr(p_h, F.p) < TOL_STEP
    assert abs(st['f'] - 0.5 * F.r @ F.r) <= 1e-11 * st['f']
    Jp = F.J @ F.p
    assert abs(st['JpJp'] - Jp @ Jp) <= 1e-7 * (Jp @ Jp)
    assert abs(st['rJp'] - F.r @ Jp) <= 1e-7 * abs(F.r @ Jp)
    assert abs(st['pp'] - F.p @ F.p) <= 1e-7 * (F.p @ F.p)
    assert relerr(h.gradient(), F.J.T @ F.r) < 1e-10
    assert relerr(h.colnorms(), F.Jn) < 1e-10
    v = np.random.default_rng(2).standard_normal(len(F.x0))
    Jv = F.J @ v
    assert abs(h.jtimes_sqnorm(v) - Jv @ Jv) <= 1e-10 * (Jv @ Jv)
    assert relerr(h.jtimes(v), Jv) < 1e-10
    q_h, st2 = h.linearize_solve(F.x0, F.lam, False)
    print('damped step %.2e' % relerr(q_h, F.q))
    assert relerr(q_h, F.q) < TOL_STEP
    assert abs(st2['trace'] - F.trace) <= 1e-10 * st2['trace']
    return p_h


@ALL
def test_residual_jacobian(hip, case):
    """(a) sizes, x0, residuals, objective and the per-observation Jacobian blocks (through index_maps, the column
    map of every IO entry) a little away from x0; with IO priors also the prior rows of final_residuals,
    unweighted and weighted, in the oracle's row order.  (The block export evaluates the model per observation and
    returns all IO rows: it checks the model at the pattern's nK, nP and the index maps.  The gather of the estimated
    rows into camera-side columns -- io_columns, the tile maps -- belongs to the build: test_step, test_routes.)"""
    F = ref('tiny', *case)
    s, so, x0, w = F.s, F.so, F.x0, F.w
    h = hip.Handle(s)
    try:
        assert h.n == len(x0) and h.m == so.post.res.ix.n
        assert np.array_equal(h.serialize(), x0)
        rng = np.random.default_rng(5)
        x = x0 + 1e-3 * rng.standard_normal(len(x0)) * np.maximum(1e-3, np.abs(x0)) * 1e-2
        r_o, J_o = o.brown_euler_cam4(x, so, jac=True)
        r_h, f_h = h.residual(x)
        assert relerr(r_h, r_o) < TOL_BLOCK
        assert abs(f_h - 0.5 * np.sum(w * r_o ** 2)) <= 1e-11 * abs(f_h)
        JEO, JOP, JIO = h.jacobian_blocks(x)
        J_h = assemble_J(h, s, JEO, JOP, JIO)
        no2 = 2 * F.no
        assert abs((J_h - J_o[:no2]).tocsc()).max() <= TOL_BLOCK * abs(J_o).max()
        if case[1]:
            nprior = PRIOR_ROWS[case]
            assert h.m == no2 + nprior and np.array_equal(np.asarray(so.post.res.ix.IO), no2 + np.arange(nprior))
            h.linearize_solve(x, 0.0, True)
            ru, rw = h.final_residuals()
            assert np.abs(r_o[no2:]).min() > 0
            assert relerr(ru[no2:], r_o[no2:]) < TOL_BLOCK and relerr(rw[no2:], (F.R * r_o)[no2:]) < TOL_BLOCK
            assert relerr(ru, r_o) < TOL_BLOCK and relerr(rw, F.R * r_o) < TOL_BLOCK
    finally:
        h.close()


@ALL
def test_step(hip, case):
    """(b) one linearisation + solve on the route the plan chooses (test_io_patterns_cpu.TINY_LAYOUT)."""
    F = ref('tiny', *case)
    h = hip.Handle(F.s)
    try:
        info = h.info()
        want = TINY_LAYOUT[case[0]]
        assert (info['n_tiles'] > 0, info['heavy_tasks'] > 0) == (want[1], want[4])
        check_step(h, F)
    finally:
        h.close()


@pytest.mark.parametrize('pattern', list(IO_PATTERNS))
def test_routes(hip, pattern, monkeypatch):
    """(c) the step on every route the pattern can reach: each within TOL_STEP of the oracle and within 1e-9 of the
    default route; the route that ran is asserted, a case that cannot reach its route fails."""
    F = ref('tiny', pattern, None)
    ncolmax = 6 + max([0] + [len(r) for r in IO_PATTERNS[pattern][3].values()])
    p_default = None
    for switch, value, kernel, tiles, heavy, bsig, bksig in routes(pattern):
        if switch:
            monkeypatch.setenv(switch, value)
        L = hip.plan_layout_stats(F.s)
        assert (L['n_tiles'] > 0, L['heavy_tasks'] > 0, L['build_sig'], L['backsub_sig']) == (tiles, heavy, bsig, bksig), (switch, L)
        h = hip.Handle(F.s)
        try:
            info = h.info()
            assert h.build_kernel_name() == kernel, (switch, h.build_kernel_name())
            assert info['ncolmax'] == ncolmax and (ncolmax > 15) == (pattern in UNTILED)
            assert (info['n_tiles'] > 0, info['heavy_tasks'] > 0) == (tiles, heavy) and info['heavy_tasks'] == L['heavy_tasks']
            p_h, st = h.linearize_solve(F.x0, 0.0, True)
            assert not st['singular']
            q_h, _ = h.linearize_solve(F.x0, F.lam, False)
        finally:
            h.close()
        if switch:
            monkeypatch.delenv(switch)
        print('%s %s=%s: oracle %.2e %.2e' % (pattern, switch, value, relerr(p_h, F.p), relerr(q_h, F.q)))
        assert relerr(p_h, F.p) < TOL_STEP and relerr(q_h, F.q) < TOL_STEP
        if p_default is None:
            p_default = p_h
        assert relerr(p_h, p_default) < 1e-9


@pytest.mark.parametrize('pattern', list(SMALL_LAYOUT))
def test_step_small(hip, pattern):
    """(d) 40 cameras, 4000 points: many tiles, those that straddle the two halves of the cameras get
    tile_io_simple == 0; half-std8-half-9 runs k_build_tile2 (NCX = 15) and the heavy route side by side."""
    F = _ref('small', pattern, None)
    want = SMALL_LAYOUT[pattern]
    h = hip.Handle(F.s)
    try:
        info = h.info()
        assert info['n_tiles'] > 8 and (info['heavy_tasks'] > 0) == want[4]
        assert h.build_kernel_name() == ('k_build_sig' if want[2] else 'k_build_tile2')
        check_step(h, F)
    finally:
        h.close()


@ALL
def test_bundle_gna(hip, case):
    """(e) the undamped bundle in the default environment."""
    from dbat_amd import bundle
    s, _ = io_pattern_struct('tiny', *case)
    res, ok, iters, s0, E = bundle(s, 'gna')
    ro, oko, ito, s0o, Eo = ref_bundle(case[0], case[1], 'gna')
    assert ok and oko and E.code == Eo.code == 0
    assert iters == ito
    print('x %.2e sigma0 %.2e' % (relerr(E.x, Eo.x), abs(s0 - s0o) / s0o))
    assert relerr(E.x, Eo.x) < TOL_X
    assert abs(s0 - s0o) < 1e-8 * s0o
    assert (E.numParams, E.numObs, E.redundancy) == (Eo.numParams, Eo.numObs, Eo.redundancy)
    assert relerr(res.IO.val, ro.IO.val) < TOL_X


@pytest.mark.parametrize('case', [('all10', None), ('half-std8-half-9', None), ('cc-shared-K-per-group', (0, 5, 6, 7))],
                         ids=['all10', 'half-std8-half-9', 'cc-shared-K-per-group+prior'])
def test_bundle_lm(hip, case):
    """(e) Levenberg-Marquardt: the damped system (lambda on the IO diagonal, beside the prior weights)."""
    from dbat_amd import bundle
    s, _ = io_pattern_struct('tiny', *case)
    res, ok, iters, s0, E = bundle(s, 'lm')
    ro, oko, ito, s0o, Eo = ref_bundle(case[0], case[1], 'lm')
    assert ok and oko and E.code == Eo.code == 0
    assert relerr(E.x, Eo.x) < TOL_X and abs(s0 - s0o) < 1e-8 * s0o
    check_history(E, Eo, iters, ito, 'lm', s=s)


@pytest.mark.parametrize('case', COV_CASES, ids=[_id(c) for c in COV_CASES])
def test_covariance_and_redundancy(hip, case):
    """(f) posterior covariance blocks of the converged bundle against the oracle's dense inverse (1e-6 of the largest
    entry of each matrix); redundancy numbers at x0 against the dense hat matrix: Qvv of every image point, r of the IO
    prior rows, their sum m - n."""
    from dbat_amd import bundle, bundle_cov
    s, _ = io_pattern_struct('tiny', *case)
    res, ok, iters, s0, E = bundle(s, 'gna')
    ro, oko, ito, s0o, Eo = ref_bundle(case[0], case[1], 'gna')
    assert ok and oko
    got = bundle_cov(res, E, 'CIO', 'CEO', 'COP')
    want = o.bundle_cov(ro, Eo, 'CIO', 'CEO', 'COP')
    for nm, A, B in zip(('CIO', 'CEO', 'COP'), got, want):
        assert A.shape == B.shape and abs(B).max() > 0
        print('%s %s: %.2e of the largest entry' % (_id(case), nm, abs(A - B).max() / abs(B).max()))
        assert abs(A - B).max() <= 1e-6 * abs(B).max()
    so, rw, qvv_o, rp_o, r_o, maps, n = dense_reliability(s)
    x0 = ref('tiny', *case).x0
    h = hip.Handle(s)
    try:
        qvv, rp = h.redundancy(x0)
        m = h.m
        assert (m, h.n) == (r_o.size, n)
    finally:
        h.close()
    assert np.abs(qvv - qvv_o).max() <= 1e-9
    nprior = PRIOR_ROWS.get(case, 0)
    assert rp.shape == rp_o.shape == (nprior,)
    if nprior:
        print('%s r_prior %s' % (_id(case), rp))
        assert np.abs(rp - rp_o).max() <= 1e-9
    tot = qvv[0].sum() + qvv[2].sum() + rp.sum()
    assert abs(tot - (m - n)) <= 1e-9 * m


@pytest.mark.parametrize('pattern', [p for p in IO_PATTERNS if p not in UNTILED])
def test_deterministic(hip, pattern):
    """(g) at most nine IO columns per camera: the exact sums repeat bit for bit and agree with the default step."""
    F = ref('tiny', pattern, None)
    h = hip.Handle(F.s)
    try:
        assert h.info()['ncolmax'] <= 15
        p_default, st0 = h.linearize_solve(F.x0, 0.0, True)
        h.set_deterministic(True)
        ps = [h.linearize_solve(F.x0, 0.0, True)[0] for _ in range(3)]
        assert np.array_equal(ps[0], ps[1]) and np.array_equal(ps[0], ps[2])
        assert relerr(ps[0], p_default) < 1e-8 and relerr(ps[0], F.p) < TOL_STEP
    finally:
        h.close()


@pytest.mark.parametrize('pattern', UNTILED)
def test_deterministic_unsupported(hip, pattern):
    """(g) more than nine IO columns per camera: refused with the condition in words, and the handle goes on."""
    F = ref('tiny', pattern, None)
    h = hip.Handle(F.s)
    try:
        assert h.info()['ncolmax'] > 15
        p0, _ = h.linearize_solve(F.x0, 0.0, True)
        with pytest.raises(hip.DbatHipError, match='at most nine estimated IO columns per camera') as ei:
            h.set_deterministic(True)
        assert ei.value.code == hip.EUNSUPPORTED
        assert 'signature-group' not in str(ei.value)
        p1, st = h.linearize_solve(F.x0, 0.0, True)
        assert not st['singular'] and relerr(p1, p0) < 1e-10 and relerr(p1, F.p) < TOL_STEP
    finally:
        h.close()
