"""Per-observation weights on every build route, against the oracle.

Every build, back-substitution, residual and trace kernel has a variant that reads per-observation weights, kept in
three copies (o_w in processing order, sg_w slot-major, cm_w camera-major) that come into being in two ways: the plan
writes them when IP.std is not uniform per camera, or Core::robust_promote() re-derives the maps cm_map / sg_map and
k_robust_apply scatters base * sqrt(omega) through them.  A weight factor omega_i on image point i is the same
least-squares problem as the struct with IP.std[:, i] / sqrt(omega_i), so the oracle's full sparse solve, bundle and
bundle_cov run unchanged on that struct (helpers.reweighted_struct); nothing on the checking side shares code with
the device.  tests/test_obs_weights_cpu.py checks that reference against dense NumPy.

Three ways to the same system, each against the oracle:
  plan                 a fresh handle on the struct with IP.std / sqrt(omega)
  promoted-uniform     a handle on the struct (uniform IP.std), then set_obs_weights(omega)
  promoted-nonuniform  a handle on the struct with IP.std * (1 + 0.5 * (i % 3)), then set_obs_weights(omega)
                       (the `else` branches of robust_promote and robust_reset)

OMEGA_LO: lower bound of omega per scene (helpers.obs_weight_factors): 1e-2 wherever the reference itself agrees
with dense NumPy to 1e-10 at that bound (tests/test_obs_weights_cpu.py).

Largest relerr of the scaled Gauss-Newton step against the oracle, per route and way (MI355X; the bar is 1e-8):
  route                        plan      promoted-uniform  promoted-nonuniform  promoted against plan (bar 1e-9)
  sig                          1.5e-13   1.4e-13           1.5e-13              4.9e-14
  tile3                        2.1e-13   2.0e-13           1.3e-13              4.5e-14
  tile2                        3.0e-13   2.6e-13           2.9e-13              6.3e-14
  heavy                        1.2e-13   1.4e-13           9.6e-14              5.6e-14
  heavy-selfcal                2.8e-13   2.6e-13           2.8e-13              8.5e-14
  columns                      1.8e-13   1.8e-13           1.5e-13              4.8e-14
  columns-selfcal              2.6e-13   2.6e-13           2.2e-13              6.2e-14
  bt128                        1.6e-13   1.6e-13           1.2e-13              2.4e-14
  giant                        1.5e-11   2.4e-12           1.6e-11              3.3e-12
  giant-selfcal                2.2e-11   7.9e-12           1.3e-11              1.1e-11
  giant-mfma                   3.8e-11   9.4e-12           4.8e-11              1.1e-11
  giant-mfma-selfcal-groups3   9.9e-11   1.0e-10           7.9e-11              1.7e-10
  mixed-heavy                  4.4e-11   4.3e-11           1.5e-11              9.3e-12
  mixed-columns                3.4e-11   3.3e-11           2.0e-11              1.5e-11
  all-see-all                  1.8e-12   1.3e-12           1.7e-12              6.4e-13
Bundle with omega set against the oracle's (relerr of x): tile2 6.8e-17, heavy-selfcal 1.3e-16, giant-selfcal 4.3e-16;
covariance blocks, of the largest entry: 1.7e-12, 1.0e-12, 6.9e-11.

What no step shows -- the scaled step is invariant under any diagonal column scaling, and a wrong trace only sends
Levenberg-Marquardt down another path: per route and way the relative errors of the column norms, of trace(J'J)
(st['trace'] of the damped build), of ||J v||^2 and of J v against the oracle's weighted sparse J
(helpers.linearisation_figures; MI355X; the bar is 1e-10, 'plan' the larger of the two bases).  None is above 1e-11;
the largest, the trace of the self-calibrating giant and mixed scenes, are sums over camera columns of 1e20 and more.
The largest relative error of a single column norm (same bar; the vector's relerr is blind to the point columns
beside such a camera column) over all routes and ways, weighted and on the crowded routes: 1.3e-15 (giant-mfma).
  route                      plan                              promoted-uniform                  promoted-nonuniform
                             colnorms trace  JvJv    Jv        colnorms trace  JvJv    Jv        colnorms trace  JvJv    Jv
  sig                        1.1e-16 0       3.6e-16 2.2e-16   1.1e-16 0       2.0e-16 2.2e-16   1.1e-16 2.1e-16 1.8e-16 2.3e-16
  tile3                      9.9e-17 0       3.7e-16 2.1e-16   1.0e-16 0       1.9e-16 2.3e-16   1.1e-16 0       1.8e-16 2.2e-16
  tile2                      1.2e-16 2.6e-15 5.3e-16 6.1e-16   1.6e-18 2.1e-15 5.3e-16 6.5e-16   2.3e-16 2.7e-15 3.6e-16 4.7e-16
  heavy                      1.3e-16 1.4e-16 3.6e-16 2.1e-16   9.4e-17 0       0       2.3e-16   1.2e-16 0       4.8e-16 2.1e-16
  heavy-selfcal              1.2e-16 9.9e-16 6.1e-16 5.4e-16   1.2e-16 2.7e-16 8.1e-16 3.5e-16   1.1e-18 9.9e-16 4.9e-16 5.4e-16
  columns                    1.2e-16 2.4e-16 5.4e-16 2.2e-16   1.1e-16 1.2e-16 0       2.2e-16   1.1e-16 2.2e-16 5.4e-16 2.3e-16
  columns-selfcal            4.0e-16 2.9e-15 1.2e-15 7.9e-16   4.0e-16 2.9e-15 1.2e-15 6.4e-16   1.1e-20 5.7e-16 4.3e-16 8.0e-16
  bt128                      1.6e-16 2.1e-16 1.8e-16 2.2e-16   1.6e-16 1.2e-16 0       2.3e-16   1.4e-16 2.1e-16 1.8e-16 2.2e-16
  giant                      1.6e-16 0       1.4e-16 2.2e-16   1.5e-16 0       0       2.3e-16   1.6e-16 0       1.2e-16 2.3e-16
  giant-selfcal              4.3e-16 2.1e-14 5.0e-16 2.1e-16   2.1e-16 2.1e-14 1.2e-16 1.9e-16   4.3e-16 1.5e-14 2.5e-16 2.7e-16
  giant-mfma                 3.6e-16 3.7e-16 4.4e-16 4.7e-16   3.1e-16 3.7e-16 2.5e-16 3.4e-16   3.8e-16 2.0e-16 4.4e-16 4.6e-16
  giant-mfma-selfcal-groups3 4.2e-16 3.5e-15 2.3e-16 1.3e-16   2.1e-16 2.8e-15 2.3e-16 6.3e-17   2.1e-16 2.9e-15 2.3e-16 1.2e-16
  mixed-heavy                1.8e-16 9.6e-15 0       6.4e-16   7.0e-19 9.3e-15 0       6.6e-16   1.1e-16 7.3e-15 0       6.3e-16
  mixed-columns              3.5e-16 1.7e-14 0       6.6e-16   7.2e-16 7.4e-15 2.2e-16 6.5e-16   3.5e-16 1.7e-14 1.9e-16 6.8e-16
  all-see-all                1.4e-16 2.0e-15 1.5e-16 4.9e-16   1.4e-16 2.0e-15 1.5e-16 4.9e-16   1.6e-16 2.1e-15 1.3e-16 3.5e-16
The trace-only pass (lambda0 of one LM iteration against the oracle's trace; the bar is 1e-11): at most 1.1e-15 on the
eight routes and three ways, 1.7e-16 from the signature kernel's pass 1 on two ranks.
The damping loops with omega set, both ways (relerr of x against the oracle's loop): 'lm' and 'lmp' at most 5.4e-16
with the oracle's 5 and 3 iterations; 'gm' 1.1e-16 where it runs (tile3, heavy) and the oracle's code -2 at
iteration 0 on the self-calibrating scenes.  LM at convTol = 1e-3 (its margins: the table above
test_lm_iteration_count_with_weights): the oracle's count, objective values to 5.7e-16 of the largest (giant-selfcal
4.2e-12).
"""
import copy
from types import SimpleNamespace as NS

import numpy as np
import pytest
import scipy.sparse as sp

import dbat_oracle as o
from helpers import (TOL_LIN, all_see_all_scene, base_image_weights, camcal_struct, check_linearisation_figures,
                     crowded_struct, giant_points_struct, linearisation_figures, lm_decision_margins, mixed_heavy_struct,
                     obs_weight_factors, relerr, reweighted_struct, std_pattern, sxb_prior_eo_struct, synth_struct)
from test_crowded_batches_gpu import ROUTES, check_route, oracle_setup
from test_crowded_batches_gpu import scene as crowded_scene

pytestmark = pytest.mark.gpu

TOL_STEP = 1e-8
TOL_X = 1e-7

# scene: (environment, builder).  The eight crowded routes with kind 'prior3' (test_crowded_batches_gpu.ROUTES), the
# scenes of test_giant_points / test_giant_points_on_the_matrix_cores / test_mixed_tiled_and_heavy_points, and every
# point in every one of 40 images with three IO blocks.
GIANT_ENV = {'DBAT_HIP_BT': '128', 'DBAT_HIP_GIANT_THREADS': '64'}
MFMA_ENV = {'DBAT_HIP_GIANT_THREADS': '128'}
SCENES = {r: (ROUTES[r][0], None) for r in ROUTES}
SCENES.update({
    'giant': (GIANT_ENV, lambda: giant_points_struct(140, 500, 'plain')[0]),
    'giant-selfcal': (GIANT_ENV, lambda: giant_points_struct(140, 500, 'selfcal')[0]),
    'giant-mfma': (MFMA_ENV, lambda: giant_points_struct(300, 400, 'plain')[0]),
    'giant-mfma-selfcal-groups3': (MFMA_ENV, lambda: giant_points_struct(300, 400, 'selfcal-groups3')[0]),
    'mixed-heavy': ({'DBAT_HIP_CMAX': '6', 'DBAT_HIP_HEAVY': '1'}, lambda: mixed_heavy_struct('selfcal')[0]),
    'mixed-columns': ({'DBAT_HIP_CMAX': '6', 'DBAT_HIP_HEAVY': '0'}, lambda: mixed_heavy_struct('selfcal')[0]),
    'all-see-all': ({'DBAT_HIP_CMAX': '8'}, lambda: all_see_all_scene(40, 150, True, 3)[0]),
})
OMEGA_LO = {name: 1e-2 for name in SCENES}
BASES = ('uniform', 'nonuniform')


def make_scene(name, monkeypatch):
    """The scene's environment set, and its struct (uniform IP.std)."""
    env, make = SCENES[name]
    if make is None:
        return crowded_scene(name, 'prior3', monkeypatch)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return make()


def scene_omega(name, s, seed=0):
    return obs_weight_factors(s.IP.val.shape[1], 100 + seed + sorted(SCENES).index(name), OMEGA_LO[name])


@pytest.fixture(scope='module')
def hip():
    from dbat_amd import _hip
    import torch
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    _hip.load()
    return _hip


def check_ran(hip, h, s, name):
    """The handle runs the kernels the scene is there for."""
    if name in ROUTES:
        return check_route(hip, h, s, name)
    info, rays = h.info(), int(np.bincount(s.IP.pt).max())
    lay = hip.plan_layout_stats(s)
    if name.startswith('giant-mfma'):           # k_heavy_z_giant + k_heavy_syrk beside tiled points
        assert info['BT'] == 256 < rays and info['heavy_tasks'] > 0 and info['heavy_points'] == 3 and info['n_tiles'] > 0
        assert lay['heavy_tasks'] == info['heavy_tasks']
    elif name.startswith('giant'):              # k_build_giant / k_backsub_giant: no matrix-core route at BT = 128
        assert info['BT'] == 128 < rays and info['heavy_tasks'] == 0 and info['n_tiles'] == 0
        assert h.build_kernel_name() == 'k_build' and lay['heavy_tasks'] == 0
    elif name.startswith('mixed'):
        heavy = name == 'mixed-heavy'
        assert 0 < info['n_tiles'] and info['n_batches'] > 0 and (info['heavy_tasks'] > 0) == heavy
        assert hip.batch_stats(s)['n_batches_untiled'] > 0          # (the tiled points: whichever tile kernel the plan picks)
    else:
        assert info['heavy_points'] == 150 and info['n_tiles'] == 0 and info['heavy_row_groups'] >= (40 + 7) // 8 + 1
        assert h.build_kernel_name() == 'k_heavy_z + k_heavy_syrk'


def oracle_system(s_eff):
    """Everything the checks need of the oracle at x0 of the (reweighted) struct."""
    so, x0, w = oracle_setup(s_eff)
    R = np.sqrt(w)
    r_o, K = o.brown_euler_cam4(x0, so, jac=True)
    r = R * r_o
    J = (sp.diags(R) @ K).tocsc()
    p, sing, *_ = o._scaled_gn(J, r)
    assert not sing
    JTJ = (J.T @ J).tocsc()
    lam = 1e-4 * JTJ.diagonal().sum() / J.shape[1]
    q, _ = o.normal_solve((JTJ + lam * sp.identity(J.shape[1])).tocsc(), -(J.T @ r))
    return NS(x0=x0, r=r, J=J, p=p, lam=lam, q=q, g=J.T @ r, Jn=np.sqrt(np.asarray(J.multiply(J).sum(0)).ravel()),
              trace=float(JTJ.diagonal().sum()))


FIGURES = {}
LIN_FIGURES = {}


def check_against_oracle(h, O, w_rows, label):
    """Step, scalars, gradient, damped step, cost and the weighted residual rows of handle h against the oracle's
    system O, and the column norms, trace(J'J), ||J v||^2 and J v of its linearisation (helpers.linearisation_figures);
    w_rows (nObs, 2): the weights base * sqrt(omega) the image rows must carry.  Returns the step."""
    x0 = O.x0
    p_h, st = h.linearize_solve(x0, 0.0, True)
    FIGURES[label] = relerr(p_h, O.p)
    print('relerr step %-48s %.2e' % (label, FIGURES[label]))
    assert not st['singular']
    assert relerr(p_h, O.p) < TOL_STEP
    Jp = O.J @ O.p
    assert abs(st['JpJp'] - Jp @ Jp) <= 1e-7 * (Jp @ Jp)
    assert abs(st['rJp'] - O.r @ Jp) <= 1e-7 * abs(O.r @ Jp)
    assert abs(st['pp'] - O.p @ O.p) <= 1e-7 * (O.p @ O.p)
    assert relerr(h.gradient(), O.g) < 1e-10
    ru, rw = h.final_residuals()                        # rows of the linearisation at x0
    n2 = 2 * w_rows.shape[0]
    assert np.allclose(rw[:n2].reshape(-1, 2), ru[:n2].reshape(-1, 2) * w_rows, rtol=1e-12, atol=1e-300)
    # what no step shows (the scaled step is invariant under any diagonal column scaling): the column norms the build
    # kernels write beside it, below those of the damped build with trace(J'J) and J v
    assert relerr(h.colnorms(), O.Jn) < TOL_LIN
    q_h, st2 = h.linearize_solve(x0, O.lam, False)
    print('relerr damped step %-41s %.2e' % (label, relerr(q_h, O.q)))
    assert relerr(q_h, O.q) < TOL_STEP
    LIN_FIGURES[label] = linearisation_figures(h, O.J, st2['trace'])
    check_linearisation_figures(LIN_FIGURES[label], label)
    _, f = h.residual(x0)
    assert abs(f - 0.5 * (O.r @ O.r)) <= 1e-12 * 0.5 * (O.r @ O.r)
    return p_h


STEP_CASES = [(n, b) for n in SCENES for b in BASES]


@pytest.mark.parametrize('name,base', STEP_CASES, ids=['%s-%s' % c for c in STEP_CASES])
def test_weighted_step_three_ways(hip, name, base, monkeypatch):
    """Way 'plan' and the promoted way of `base` against the oracle on one reweighted struct, and against each other."""
    s = make_scene(name, monkeypatch)
    if base == 'nonuniform':
        s = std_pattern(s)
    om = scene_omega(name, s, BASES.index(base))
    assert om.min() == OMEGA_LO[name] and om.max() == 1.0 and 0.05 < np.mean(om == 1.0) < 0.15
    s_eff = reweighted_struct(s, om)
    O = oracle_system(s_eff)
    h = hip.Handle(s_eff)
    try:
        check_ran(hip, h, s_eff, name)
        p_plan = check_against_oracle(h, O, base_image_weights(s_eff), '%s plan(%s)' % (name, base))
    finally:
        h.close()
    h = hip.Handle(s)
    try:
        h.set_obs_weights(om)
        check_ran(hip, h, s, name)
        p_prom = check_against_oracle(h, O, base_image_weights(s) * np.sqrt(om)[:, None], '%s promoted-%s' % (name, base))
    finally:
        h.close()
    print('relerr promoted against plan %-31s %.2e' % ('%s %s' % (name, base), relerr(p_prom, p_plan)))
    assert relerr(p_prom, p_plan) <= 1e-9


# ---------------------------------------------------------------- the trace-only pass
TRACE_SCENES = ['sig', 'tile3', 'tile2', 'heavy-selfcal', 'columns', 'bt128', 'giant-selfcal', 'all-see-all']
WAYS = ('plan', 'promoted-uniform', 'promoted-nonuniform')


def weighted_handle(hip, s, om, way):
    """A handle that carries omega by `way` ('plan': built on the reweighted struct; else set_obs_weights on the
    struct's own handle), and the struct it was built on."""
    if way == 'plan':
        t = reweighted_struct(s, om)
        return hip.Handle(t), t
    h = hip.Handle(s)
    try:
        h.set_obs_weights(om)
    except BaseException:
        h.close()
        raise
    return h, s


def lm_first_lambda(hip, h, x0):
    """damp[0] of one Levenberg-Marquardt iteration from x0, which must have come from the trace-only pass."""
    opt = hip.default_options('lm')
    opt.store_trace, opt.max_iter = 0, 1
    x, r, rr, damp, aux, T = h.solve(x0, opt)
    assert r.n_trace_only == 1
    return damp[0], abs(opt.lambda0)


@pytest.mark.parametrize('name', TRACE_SCENES)
def test_trace_only_pass_with_weights(hip, name, monkeypatch):
    """Levenberg-Marquardt's lambda0 = c trace(J'J) / n from the streaming pass that forms no normal equations
    (k_trace_cm reading cm_w), with weights set in each of the three ways: the oracle's trace of the weighted J, and
    the trace a full linearisation on the same handle reports.  A wrong lambda0 leaves LM converging by another
    path, so no bundle test sees it."""
    s0 = make_scene(name, monkeypatch)
    for k, way in enumerate(WAYS):
        s = std_pattern(s0) if way == 'promoted-nonuniform' else s0
        om = scene_omega(name, s, 10 + k)
        so, x0o, w = oracle_setup(reweighted_struct(s, om))
        _, K = o.brown_euler_cam4(x0o, so, jac=True)
        tr = float((sp.diags(w) @ K.multiply(K)).sum())
        h, t = weighted_handle(hip, s, om, way)
        try:
            check_ran(hip, h, t, name)
            x0 = h.serialize()
            assert np.array_equal(x0, x0o)
            lam0, c = lm_first_lambda(hip, h, x0)
            print('trace-only pass %-15s %-20s lambda0 off the oracle\'s by %.2e' % (name, way, abs(lam0 - c * tr / h.n) / lam0))
            assert abs(lam0 - c * tr / h.n) <= 1e-11 * lam0, way
            _, st = h.linearize_solve(x0, 0.0, False)
            assert abs(lam0 - c * st['trace'] / h.n) <= 1e-12 * lam0, way
        finally:
            h.close()


@pytest.mark.parametrize('way', WAYS[:2])
def test_trace_only_build_with_weights_two_ranks(hip, way, monkeypatch):
    """With several ranks the trace comes from a build instead of k_trace_cm: on the signature route from
    build_sig_tile's pass 1 (reading sg_w), which leaves before the Schur complement under d.trace_only.  Two ranks
    of one GPU on the 'sig' scene, the same two assertions on every rank."""
    from test_multishard_gpu import _run_ranks
    name = 'sig'
    s = make_scene(name, monkeypatch)
    om = scene_omega(name, s, 13)
    so, x0o, w = oracle_setup(reweighted_struct(s, om))
    _, K = o.brown_euler_cam4(x0o, so, jac=True)
    tr = float((sp.diags(w) @ K.multiply(K)).sum())
    t = reweighted_struct(s, om) if way == 'plan' else s
    assert hip.plan_layout_stats(t, 0, 2)['build_sig'] and hip.plan_layout_stats(t, 1, 2)['build_sig']

    def work(comm):
        hh = hip.Handle(t, shard_rank=comm.rank, shard_count=comm.world_size)
        try:
            hh.set_allreduce(comm.allreduce_ptr)
            if way != 'plan':
                hh.set_obs_weights(om)
            assert hh.build_kernel_name() == 'k_build_sig'
            lam0, c = lm_first_lambda(hip, hh, x0o)
            _, st = hh.linearize_solve(x0o, 0.0, False)
            return lam0, c, st['trace'], hh.n
        finally:
            hh.close()

    out, _ = _run_ranks(s, 2, work)
    for lam0, c, tr_h, n in out:
        print('trace-only build, two ranks, %-17s lambda0 off the oracle\'s by %.2e' % (way, abs(lam0 - c * tr / n) / lam0))
        assert abs(lam0 - c * tr / n) <= 1e-11 * lam0
        assert abs(lam0 - c * tr_h / n) <= 1e-12 * lam0


# ---------------------------------------------------------------- covariance
@pytest.mark.parametrize('name', ['tile2', 'heavy-selfcal', 'giant-selfcal'])
def test_bundle_and_covariance_promoted(hip, name, monkeypatch):
    """Way 2 through the whole adjustment: Handle.solve with omega set, then bundle_cov with the weights re-applied
    on the acquired handle, against the oracle's bundle and bundle_cov of the reweighted struct."""
    from dbat_amd import bundle_cov
    s = make_scene(name, monkeypatch)
    om = scene_omega(name, s)
    ro, oko, ito, s0o, Eo = o.bundle(reweighted_struct(s, om), 'gna')
    want = o.bundle_cov(ro, Eo, 'COP', 'CEO')
    h = hip.Handle(s)
    try:
        h.set_obs_weights(om)
        check_ran(hip, h, s, name)
        opt = hip.default_options('gna')
        opt.max_iter, opt.conv_tol = 20, 1e-6
        x, res, *_ = h.solve(h.serialize(), opt)
        ru, rw = h.final_residuals()
        IO, EO, OP = h.deserialize(x)
        dof = h.m - h.n
    finally:
        h.close()
    ok = res.code == 0
    assert ok == oko and res.code == Eo.code and res.iters == ito
    print('relerr bundle x %-20s %.2e' % (name, relerr(x, Eo.x)))
    assert ok and relerr(x, Eo.x) < TOL_X
    t = copy.deepcopy(s)
    t.IO.val, t.OP.val = IO, OP
    t.EO.val = np.vstack([EO, t.EO.val[6:]]) if t.EO.val.shape[0] > 6 else EO
    E = NS(x=x, s0=float(np.sqrt(rw @ rw / dof)), robust=NS(weights=om), code=0)
    assert abs(E.s0 - s0o) <= 1e-8 * s0o
    hip.clear_cache()
    try:
        got = bundle_cov(t, E, 'COP', 'CEO')
    finally:
        hip.clear_cache()
    for A, B in zip(got, want):
        assert A.shape == B.shape and abs(B).max() > 0
        print('covariance %-20s %.2e of the largest entry' % (name, abs(A - B).max() / abs(B).max()))
        assert abs(A - B).max() <= 1e-6 * abs(B).max()


# ---------------------------------------------------------------- the damping loops with weights set
LOOP_SCENES = ['tile2', 'heavy-selfcal', 'giant-selfcal']
# 'gm' on the three self-calibrating scenes ends in the oracle with code -2 at iteration 0: the UNSCALED normal matrix
# has diagonal entries from 6 to 2e20 (K3 beside an object point), the estimate (min / max diag L)^2 is 5e-18 / 1e-17 /
# 4e-22 against eps = 2.2e-16.  There the case pins the code, the first weighted objective and x = x0; the loop itself
# runs with weights on the two fixed-IO scenes beside them (estimate 8e-8 / 1e-7; 3 and 4 iterations).
# 'tile2' is built smaller for 'gm' (30 cameras, 1500 points through the same builder; check_ran holds it to the route):
# the oracle's analysis of the singular 9361-column matrix takes 30 s of CPU, that of the smaller one 4 s.
GM_SCENES = LOOP_SCENES + ['tile3', 'heavy']
LOOP_CASES = [(n, d) for d in ('lm', 'lmp') for n in LOOP_SCENES] + [(n, 'gm') for n in GM_SCENES]


def loop_scene(name, damping, monkeypatch):
    if (name, damping) == ('tile2', 'gm'):
        for k, v in ROUTES[name][0].items():
            monkeypatch.setenv(k, v)
        return crowded_struct('prior3', selfcal=True, cams=30, points=1500)[0]
    return make_scene(name, monkeypatch)


def solve_promoted(hip, s, om, damping, name, conv_tol=1e-6):
    """Handle.solve with omega set on the handle of s: what bundle() returns as E, as far as the checks read it."""
    h = hip.Handle(s)
    try:
        h.set_obs_weights(om)
        check_ran(hip, h, s, name)
        opt = hip.default_options(damping)
        opt.max_iter, opt.conv_tol, opt.store_trace = 20, conv_tol, 0
        x, res, rr, damp, aux, T = h.solve(h.serialize(), opt)
        ru, rw = h.final_residuals()
        dof = h.m - h.n
    finally:
        h.close()
    E = NS(x=x, code=int(res.code), iters=int(res.iters), res=rr, s0=float(np.sqrt(rw @ rw / dof)))
    if damping == 'lm':
        E.damping = NS(**{'lambda': damp})
    elif damping == 'lmp':
        rho, step = aux[:opt.max_iter + 2], aux[opt.max_iter + 2:]
        E.damping = NS(delta=damp, rho=rho[~np.isnan(rho)], step=step[~np.isnan(step)].astype(int))
    return E


@pytest.mark.parametrize('name,damping', LOOP_CASES, ids=['%s-%s' % c for c in LOOP_CASES])
def test_damping_loops_with_weights(hip, name, damping, monkeypatch):
    """Levenberg-Marquardt, Powell's dog-leg and Gauss-Markov with omega set, both ways, against the oracle's loop of
    that name on the reweighted struct: the trial-point objective, the gain ratio and the trust-region history all
    go through weight-reading kernels.  The plan way is bundle() on the reweighted struct, the promoted way
    Handle.solve after set_obs_weights, as in test_bundle_and_covariance_promoted."""
    from dbat_amd import bundle
    from test_hip_parity import check_history
    s = loop_scene(name, damping, monkeypatch)
    om = scene_omega(name, s)
    s_eff = reweighted_struct(s, om)
    ro, oko, ito, s0o, Eo = o.bundle(s_eff, damping)
    _, ok, iters, s0, E = bundle(s_eff, damping, reuse_handle=False)
    Ep = solve_promoted(hip, s, om, damping, name)
    for way, e, it, sig0 in (('plan', E, iters, s0), ('promoted', Ep, Ep.iters, Ep.s0)):
        print('relerr %s x %-16s %-9s %.2e (code %d, %d iterations; oracle %d, %d)'
              % (damping, name, way, relerr(e.x, Eo.x), e.code, it, Eo.code, ito))
        assert e.code == Eo.code, way
        assert relerr(e.x, Eo.x) < TOL_X, way
        assert abs(sig0 - s0o) <= 1e-8 * s0o, way
        check_history(e, Eo, it, ito, damping)
        if damping == 'lmp':
            assert np.array_equal(e.damping.step, Eo.damping.step), way
            assert relerr(e.damping.delta, Eo.damping.delta) < 1e-9, way
            assert np.abs(e.damping.rho - Eo.damping.rho).max() < 1e-3, way
    assert ok == oko
    assert relerr(Ep.x, E.x) <= 1e-9
    if damping == 'lmp':
        assert Ep.iters == iters
    if damping == 'gm':
        assert (Eo.code, ito) == (-2, 0) if name in LOOP_SCENES else Eo.code == 0 and ito >= 3      # (the comment above GM_SCENES)


# The oracle's LM run at convTol = 1e-3 on the reweighted struct of scene_omega(name, s) (seed 0), helpers.lm_decision_margins:
#   scene           iterations   smallest margin |fNew - f| / f   termination ratio's factor from 1
#   tile2           4            5.0e-9                           14.1
#   heavy-selfcal   4            3.4e-9                           17.2
#   giant-selfcal   4            3.0e-9                           18.1
@pytest.mark.parametrize('name', LOOP_SCENES)
def test_lm_iteration_count_with_weights(hip, name, monkeypatch):
    """test_hip_parity.py::test_lm_iteration_count_where_it_is_a_property_of_the_problem with omega set, both ways: at
    convTol = 1e-3 every accept / reject decision of the oracle has a margin three orders above the 1e-12 by which
    the device's objective values differ from its own (the table above), so the count, the residual history and
    every lambda must be the oracle's."""
    from dbat_amd import bundle
    s = make_scene(name, monkeypatch)
    om = scene_omega(name, s)
    s_eff = reweighted_struct(s, om)
    n_o, margin, term = lm_decision_margins(s_eff, conv_tol=1e-3)
    assert margin > 1e-10 and term > 1.5, 'not a case for this test any more: margin %.1e, termination factor %.2f' % (margin, term)
    ro, oko, ito, s0o, Eo = o.bundle(s_eff, 'lm', 1e-3)
    assert ito == n_o and oko and Eo.code == 0
    _, ok, iters, s0, E = bundle(s_eff, 'lm', 1e-3, reuse_handle=False)
    Ep = solve_promoted(hip, s, om, 'lm', name, conv_tol=1e-3)
    lamo, reso = Eo.damping.__dict__['lambda'], np.asarray(Eo.res)
    for way, e, it in (('plan', E, iters), ('promoted', Ep, Ep.iters)):
        assert e.code == 0, way
        assert it == ito, 'LM iterations (%s): device %d, oracle %d' % (way, it, ito)
        assert len(e.res) == len(reso) and relerr(e.res, reso) < 1e-8, way
        lam = e.damping.__dict__['lambda']
        assert len(lam) == len(lamo) and relerr(lam, lamo) < 1e-8, way
        print('lm at 1e-3 %-16s %-9s objective values off by %.2e of the largest' % (name, way, np.abs(np.asarray(e.res) - reso).max() / reso.max()))
        assert np.abs(np.asarray(e.res) - reso).max() <= 1e-11 * reso.max(), way
        assert relerr(e.x, Eo.x) < TOL_X, way


# ---------------------------------------------------------------- redundancy, weighted Jacobian
def _reliability_scenes():
    return [('tiny-' + v, lambda v=v: synth_struct('tiny', v)[0]) for v in ('plain', 'selfcal', 'imagevar', 'priors', 'groups4')] + \
        [('camcal', camcal_struct), ('sxb-prior-eo', lambda: sxb_prior_eo_struct(True)[0])]


@pytest.mark.parametrize('dense', [False, True], ids=['default', 'cov-dense'])
@pytest.mark.parametrize('name,make', _reliability_scenes(), ids=[n for n, _ in _reliability_scenes()])
def test_redundancy_with_weights(hip, name, make, dense, monkeypatch):
    """h.redundancy with omega set against I - J inv(J'J) J' of the reweighted struct, on the default route (selected
    inverse) and with the dense inverse forced; sum r = m - n."""
    from test_reliability_cpu import dense_reliability
    from test_reliability_gpu import _check_invariants
    s = make()
    om = obs_weight_factors(s.IP.val.shape[1], 7)
    so, rw, qvv_o, rp_o, r_o, maps, n = dense_reliability(reweighted_struct(s, om))
    x0 = oracle_setup(s)[1]
    if dense:
        monkeypatch.setenv('DBAT_HIP_COV_DENSE', '1')
    h = hip.Handle(s)
    try:
        h.set_obs_weights(om)
        qvv, rp = h.redundancy(x0)
        m, nn = h.m, h.n
    finally:
        h.close()
    assert (m, nn) == (r_o.size, n)
    assert np.abs(qvv - qvv_o).max() <= 1e-9
    assert rp.shape == rp_o.shape and (rp.size == 0 or np.abs(rp - rp_o).max() <= 1e-9)
    _check_invariants(qvv, rp, m, nn)
    assert abs(np.concatenate([qvv[0], qvv[2], rp]).sum() - (m - nn)) <= 1e-9 * m


@pytest.mark.parametrize('variant', ['selfcal', 'priors'])
def test_weighted_jacobian_csc_with_weights(hip, variant):
    s = synth_struct('tiny', variant)[0]
    om = obs_weight_factors(s.IP.val.shape[1], 11)
    so, x0, w = oracle_setup(reweighted_struct(s, om))
    x = x0 + 1e-5 * np.random.default_rng(3).standard_normal(len(x0)) * np.maximum(1e-3, np.abs(x0))
    _, K = o.brown_euler_cam4(x, so, jac=True)
    Jo = (sp.diags(np.sqrt(w)) @ K).tocsc()
    h = hip.Handle(s)
    try:
        h.set_obs_weights(om)
        Jw, Ju = h.jacobian_csc(x, True), h.jacobian_csc(x, False)
    finally:
        h.close()
    assert Jw.shape == Jo.shape
    assert abs(Jw - Jo).max() <= 1e-11 * abs(Jo).max()
    assert abs(Ju - K.tocsc()).max() <= 1e-11 * abs(K).max()       # the unweighted one does not see omega


# ---------------------------------------------------------------- state transitions
TRANSITION_SCENES = ['sig', 'tile2', 'heavy', 'giant-mfma']


def _det_step(h, x0):
    p, st = h.linearize_solve(x0, 0.0, True)
    assert not st['singular']
    return p


@pytest.mark.parametrize('name', TRANSITION_SCENES)
def test_reapplied_weights_do_not_compound(hip, name, monkeypatch):
    """set_obs_weights(om1) then set_obs_weights(om2): the bits of a fresh handle with om2 alone (deterministic sums)."""
    s = make_scene(name, monkeypatch)
    om1, om2 = scene_omega(name, s, 3), scene_omega(name, s, 4)
    assert not np.array_equal(om1, om2)
    a, b = hip.Handle(s), hip.Handle(s)
    try:
        x0 = a.serialize()
        a.set_deterministic(True); b.set_deterministic(True)
        a.set_obs_weights(om1)
        p1 = _det_step(a, x0)
        a.set_obs_weights(om2)
        b.set_obs_weights(om2)
        check_ran(hip, a, s, name)
        pa, pb = _det_step(a, x0), _det_step(b, x0)
        assert np.array_equal(pa, pb), relerr(pa, pb)
        assert relerr(p1, pa) > 1e-3                    # (the weights matter)
    finally:
        a.close(); b.close()


@pytest.mark.parametrize('base', BASES)
@pytest.mark.parametrize('name', TRANSITION_SCENES)
def test_reset_restores_the_fresh_handle(hip, name, base, monkeypatch):
    """After set_obs_weights(None) -- and after set_values with the same struct -- a deterministic step has the bits
    of a fresh handle's; info() is the fresh handle's again (it has no field for the weight path: the route fields)."""
    s = make_scene(name, monkeypatch)
    if base == 'nonuniform':
        s = std_pattern(s)
    om = scene_omega(name, s, 5)
    a, b = hip.Handle(s), hip.Handle(s)
    try:
        x0 = a.serialize()
        a.set_deterministic(True); b.set_deterministic(True)
        fresh = _det_step(b, x0)
        a.set_obs_weights(om)
        pw = _det_step(a, x0)
        assert relerr(pw, fresh) > 1e-3
        a.set_obs_weights(None)
        assert a.info() == b.info() and a.build_kernel_name() == b.build_kernel_name()
        check_ran(hip, a, s, name)
        p = _det_step(a, x0)
        assert np.array_equal(p, fresh), relerr(p, fresh)
        a.set_obs_weights(om)
        assert np.array_equal(_det_step(a, x0), pw)
        a.set_values(s)
        p = _det_step(a, x0)
        assert np.array_equal(p, fresh), relerr(p, fresh)
    finally:
        a.close(); b.close()


@pytest.mark.parametrize('name', TRANSITION_SCENES)
def test_invalid_weights_are_refused_and_change_nothing(hip, name, monkeypatch):
    s = make_scene(name, monkeypatch)
    om = scene_omega(name, s, 6)
    h = hip.Handle(s)
    try:
        x0 = h.serialize()
        h.set_deterministic(True)
        h.set_obs_weights(om)
        before = _det_step(h, x0)
        for k, bad in enumerate((0.0, -0.5, 1.0 + 1e-12, np.nan, np.inf)):
            w = om.copy()
            w[(17 * (k + 1)) % w.size] = bad
            with pytest.raises(hip.DbatHipError):
                h.set_obs_weights(w)
            assert hip.last_error() and 'omega' in hip.last_error()
        after = _det_step(h, x0)
        assert np.array_equal(before, after), relerr(after, before)
        # ... and on a handle that was never promoted
        h.set_obs_weights(None)
        fresh = _det_step(h, x0)
        w = om.copy(); w[0] = 0.0
        with pytest.raises(hip.DbatHipError):
            h.set_obs_weights(w)
        assert np.array_equal(_det_step(h, x0), fresh)
    finally:
        h.close()


@pytest.mark.parametrize('name', ['heavy', 'tile2'])
def test_two_ranks_with_weights_match_one(hip, name, monkeypatch):
    """Explicit omega (way 2) on two ranks of one GPU against one rank; tolerances of
    test_robust_gpu.py::test_ranks_match_single."""
    from test_multishard_gpu import _run_ranks
    s = make_scene(name, monkeypatch)
    om = scene_omega(name, s, 8)
    opt1 = hip.default_options('gna')
    h = hip.Handle(s)
    try:
        h.set_obs_weights(om)
        check_ran(hip, h, s, name)
        x0 = h.serialize()
        p1, _ = h.linearize_solve(x0, 0.0, True)
        x1, res1, *_ = h.solve(x0, opt1)
    finally:
        h.close()

    def work(comm):
        hh = hip.Handle(s, shard_rank=comm.rank, shard_count=comm.world_size)
        try:
            hh.set_allreduce(comm.allreduce_ptr)
            hh.set_obs_weights(om)
            p, st = hh.linearize_solve(x0, 0.0, True)
            x, res, *_ = hh.solve(x0, hip.default_options('gna'))
            return p, x, res.code, res.iters, hh.info()
        finally:
            hh.close()

    out, _ = _run_ranks(s, 2, work)
    for p, x, code, iters, info in out:
        assert code == res1.code == 0 and iters == res1.iters
        assert relerr(p, p1) <= 1e-9 and relerr(x, x1) <= 1e-9
    if name == 'heavy':
        assert any(r[4]['heavy_tasks'] > 0 for r in out)


# ---------------------------------------------------------------- the exact median at rounding level
@pytest.mark.parametrize('odd', [False, True], ids=['even', 'odd'])
def test_mad_median_of_rounding_level_residuals(hip, odd):
    """IP.val replaced by the device's own projection: every s is at rounding level or exactly 0, so the radix select
    works in its low passes and the "1 if 0" rule can apply.  Whichever branch the returned s dictates is asserted.
    On the MI355X both counts took the non-zero branch: median(s) = 1.563e-13 for 1800 and for 1799 image points, no s
    exactly 0 (the device's closed-form projection leaves rounding in every row), scale = median / sqrt(2 ln 2) exactly.
    The zero branch is taken on the device by test_robust_select_gpu.py::test_median_and_scale_are_exact (all-zero,
    zeros-majority, zeros-half), which feeds the select crafted values instead of residuals.
    """
    from test_robust_gpu import _drop_last_ip
    s = synth_struct('tiny', 'plain')[0]
    s.IO.val[5:10] = 0.0            # (a fixed distortion-free camera: the projection is reached in one step)
    if odd:
        s = _drop_last_ip(s)
    no = s.IP.val.shape[1]
    assert no % 2 == int(odd)
    px = np.asarray(s.IO.sensor.pxSize, float)[:, :1]
    h = hip.Handle(s)
    try:
        x0 = h.serialize()
        r, _ = h.residual(x0)
    finally:
        h.close()
    # The image rows are in mm with v pointing up.  The image points are part of a handle's structure key
    # (dbat_hip_set_values refuses other ones), so the projected points get a handle of their own.
    t = copy.deepcopy(s)
    t.IP.val = np.asfortranarray(np.asarray(s.IP.val, float) + np.array([[1.0], [-1.0]]) * r[:2 * no].reshape(2, no, order='F') / px)
    h = hip.Handle(t)
    try:
        r2, _ = h.residual(x0)
        assert np.abs(r2[:2 * no]).max() <= 1e-12 * np.abs(r[:2 * no]).max()
        om, sn, sc = h.robust_weights(x0, hip.robust_options('cauchy', scale='mad'))
        med = np.median(sn)
        print('median edge (%s, %d image points): median(s) = %.3e, %d of them exactly 0, scale = %.17g'
              % ('odd' if odd else 'even', no, med, int(np.count_nonzero(sn == 0)), sc))
        if med == 0:
            assert sc == 1.0
        else:
            assert sc == med / np.sqrt(2 * np.log(2))
        assert np.all((om > 0) & (om <= 1))
    finally:
        h.close()
