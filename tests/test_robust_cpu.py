"""CPU tests of robust bundle(): the weight functions and the MAD constant, bundle()'s argument checks (before any
device work), the C boundary (declarations, bindings, struct layout) and a host IRLS restatement on the oracle's
Gauss-Newton-Armijo with scaled weights, which the GPU tests use as their reference."""
import os
import re
import subprocess

import numpy as np
import pytest

import dbat_oracle as o
import dbat_amd
from dbat_amd import _hip
from dbat_amd.driver import MAD_C, robust_weight_fn
from helpers import synth_struct
from test_reliability_cpu import _oracle_setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('dbat_hip_default_robust_options', 'dbat_hip_robust_weights', 'dbat_hip_set_obs_weights', 'dbat_hip_solve_robust')


def blundered(name='tiny', idx=(5, 40, 77), size=20.0, seed=None):
    """synth scene 'plain' with image points idx shifted by size sigma in u."""
    s = synth_struct(name, 'plain', seed=seed)[0]
    s.IP.val = np.array(s.IP.val, float)
    idx = np.asarray(idx)
    s.IP.val[0, idx] += size * np.asarray(s.IP.std, float)[0, idx]
    return s


def oracle_s_norm(so, x, w, no):
    """s_i = ||(w_u v_u, w_v v_v)|| of every image point at x (w: the base weights, the sqrt of the oracle's wdiag)."""
    r = o.brown_euler_cam4(x, so, False)
    R = np.sqrt(w[:2 * no])
    v = (R * r[:2 * no]).reshape(no, 2)
    return np.sqrt(v[:, 0] ** 2 + v[:, 1] ** 2)


def oracle_scale(sn, scale_mode):
    if scale_mode == 'apriori':
        return 1.0
    sc = np.median(sn) / MAD_C
    return 1.0 if sc == 0 else sc


def oracle_inner_solve(damping):
    """solve(res, x, w, max_iter, term) -> (x, code, ...): the oracle's damping loop of that name with the arguments
    its bundle() passes (lambda0 = lambdaMin = -1e-10; delta0 = ||x||, mu = 0.25, eta = 0.75)."""
    if damping == 'gna':
        return o.gauss_newton_armijo
    if damping == 'lm':
        return lambda res, x, w, mi, term: o.levenberg_marquardt(res, x, w, mi, term, -1e-10, -1e-10)
    if damping == 'lmp':
        return lambda res, x, w, mi, term: o.levenberg_marquardt_powell(res, x, w, mi, term, np.linalg.norm(x), 0.25, 0.75)
    raise ValueError(damping)


def oracle_irls(s, loss, k, scale_mode, max_outer=10, tol=1e-3, max_iter=20, conv_tol=1e-6, damping='gna', history=None):
    """The outer loop of dbat_hip_solve_robust on the oracle's Gauss-Newton-Armijo (or, with `damping`, on its loop of
    that name): omega = 1, solve; then evaluate omega' at x, stop if max |omega' - omega| <= tol, else solve again
    from x with the image rows' weights scaled by omega'.  Returns x, omega, outer (solves), converged, scales, last
    max change, last code.  `history`: a dict that receives 'changes' (every max change) and 'inner_iters' (the
    iterations of every solve)."""
    so, x, w = _oracle_setup(s)
    no = s.IP.val.shape[1]
    res = lambda t, jac: o.brown_euler_cam4(t, so, jac)
    term = o.term_relative(conv_tol)
    solve = oracle_inner_solve(damping)
    x, code, n, *_ = solve(res, x, w, max_iter, term)
    hist = dict(changes=[], inner_iters=[n])
    if history is not None:
        history.update(hist)
    om = np.ones(no)
    outer, conv, scales, chg = 1, False, [], np.nan
    for _ in range(max_outer):
        if code != 0:
            break
        sn = oracle_s_norm(so, x, w, no)
        sc = oracle_scale(sn, scale_mode)
        scales.append(sc)
        omn = robust_weight_fn(sn / sc, loss, k)
        chg = float(np.abs(omn - om).max())
        hist['changes'].append(chg)
        if chg <= tol:
            conv = True
            break
        om = omn
        ww = w.copy()
        ww[:2 * no] = w[:2 * no] * np.repeat(om, 2)
        x, code, n, *_ = solve(res, x, ww, max_iter, term)
        hist['inner_iters'].append(n)
        outer += 1
    return x, om, outer, conv, scales, chg, code


def test_weight_functions_closed_forms():
    u = np.array([0.0, 0.3, 1.5, 1.5000001, 3.0, 30.0])
    assert np.array_equal(robust_weight_fn(u, 'huber', 1.5), np.where(u <= 1.5, 1.0, 1.5 / np.maximum(u, 1e-300)))
    assert robust_weight_fn(3.0, 'huber', 1.5) == 0.5
    c = robust_weight_fn(u, 'cauchy', 2.385)
    assert np.allclose(c, 1.0 / (1.0 + (u / 2.385) ** 2), rtol=0, atol=1e-15)
    assert robust_weight_fn(2.385, 'cauchy', 2.385) == 0.5 and robust_weight_fn(0.0, 'cauchy', 2.385) == 1.0
    assert np.all((c > 0) & (c <= 1))
    with pytest.raises(dbat_amd.BadInput):
        robust_weight_fn(u, 'tukey', 4.685)


def test_mad_constant():
    assert MAD_C == np.sqrt(2 * np.log(2))
    # the median of a chi_2 norm (Rayleigh with unit sigma): P(s <= MAD_C) = 1/2
    assert abs((1 - np.exp(-MAD_C ** 2 / 2)) - 0.5) < 1e-15


@pytest.mark.parametrize('kw', [dict(robust='tukey'), dict(robust=1), dict(robust='huber', robust_k=0),
                                dict(robust='cauchy', robust_k=float('nan')), dict(robust='huber', robust_k='2'),
                                dict(robust='huber', robust_scale='mean'), dict(robust='huber', robust_max_outer=0),
                                dict(robust='huber', robust_max_outer=64), dict(robust='huber', robust_max_outer=2.5),
                                dict(robust='huber', robust_tol=-1.0), dict(robust='huber', robust_tol=float('inf')),
                                dict(robust='huber', term_fun=lambda Jp, r: True)])
def test_bad_robust_arguments_raise_before_device(monkeypatch, kw):
    def no_device(*a, **k):
        raise AssertionError('device work before the argument check')
    monkeypatch.setattr(_hip, 'acquire', no_device)
    monkeypatch.setattr(_hip, 'Handle', no_device)
    s = synth_struct('tiny', 'plain')[0]
    with pytest.raises(dbat_amd.BadInput):
        dbat_amd.bundle(s, **kw)


def test_symbols_declared_and_bound():
    hdr = open(os.path.join(ROOT, 'include', 'dbat_hip.h')).read()
    assert re.search(r'#define DBAT_HIP_ABI_VERSION 5\b', hdr) and _hip.ABI_VERSION == 5
    for name in NEW:
        assert re.search(r'\bint\s+%s\s*\(' % name, hdr), name
        assert name in _hip.SYMBOLS, name
    assert re.search(r'typedef struct dbat_hip_robust_options \{\s*int32_t loss;[^}]*double\s+k;[^}]*int32_t scale;'
                     r'[^}]*int32_t max_outer;[^}]*double\s+weight_tol;[^}]*\} dbat_hip_robust_options;', hdr)
    for m in ('HUBER', 'CAUCHY'):
        assert '#define DBAT_HIP_LOSS_%s' % m in hdr
    for m in ('APRIORI', 'MAD'):
        assert '#define DBAT_HIP_SCALE_%s' % m in hdr
    lib = _hip.load()
    ro = _hip.RobustOptions()
    assert lib.dbat_hip_default_robust_options(0, ro) == 0 and (ro.loss, ro.k, ro.scale, ro.max_outer, ro.weight_tol) == (0, 1.5, 0, 10, 1e-3)
    assert lib.dbat_hip_default_robust_options(1, ro) == 0 and ro.k == 2.385
    assert lib.dbat_hip_default_robust_options(7, ro) == _hip.EINVAL
    assert lib.dbat_hip_set_obs_weights(None, None) == _hip.EINVAL
    x = np.zeros(4)
    assert lib.dbat_hip_robust_weights(None, _hip.dptr(x), ro, _hip.dptr(x), None, None) == _hip.EINVAL


def test_struct_layout_matches_c(tmp_path):
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dbat_hip.h"\n'
                   'int main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(dbat_hip_robust_options), offsetof(dbat_hip_robust_options, loss),\n'
                   '         offsetof(dbat_hip_robust_options, k), offsetof(dbat_hip_robust_options, scale),\n'
                   '         offsetof(dbat_hip_robust_options, max_outer), offsetof(dbat_hip_robust_options, weight_tol));\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(dbat_hip_robust_result), offsetof(dbat_hip_robust_result, outer),\n'
                   '         offsetof(dbat_hip_robust_result, converged), offsetof(dbat_hip_robust_result, inner_iters),\n'
                   '         offsetof(dbat_hip_robust_result, scale), offsetof(dbat_hip_robust_result, max_change),\n'
                   '         offsetof(dbat_hip_robust_result, reweight_s), DBAT_HIP_ROBUST_MAX_OUTER);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c11', '-Wall', '-Werror', '-I' + os.path.join(ROOT, 'include'), str(src), '-o', str(exe)],
                   check=True, capture_output=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split('\n')
    O, R = _hip.RobustOptions, _hip.RobustResult
    want_o = [C_sizeof(O)] + [getattr(O, f).offset for f in ('loss', 'k', 'scale', 'max_outer', 'weight_tol')]
    want_r = [C_sizeof(R)] + [getattr(R, f).offset for f in ('outer', 'converged', 'inner_iters', 'scale', 'max_change', 'reweight_s')]
    assert [int(v) for v in lines[0].split()] == want_o
    assert [int(v) for v in lines[1].split()] == want_r + [_hip.ROBUST_MAX_OUTER]


def C_sizeof(t):
    import ctypes
    return ctypes.sizeof(t)


def test_host_irls_inner_loops():
    """oracle_irls(damping=...): 'gna' named is the default bit for bit; around Powell's dog-leg the loop recovers the
    blunders as test_host_irls_recovers_blunders asks of it; an unknown name is refused."""
    s = blundered('tiny')
    a = oracle_irls(s, 'huber', 1.5, 'apriori', max_outer=3)
    b = oracle_irls(s, 'huber', 1.5, 'apriori', max_outer=3, damping='gna')
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
    hist = {}
    x, om, outer, conv, scales, chg, code = oracle_irls(s, 'huber', 1.5, 'apriori', max_outer=20, damping='lmp', history=hist)
    assert code == 0 and conv and outer >= 2 and len(hist['changes']) == len(hist['inner_iters']) == outer and hist['changes'][-1] == chg
    bad = np.array([5, 40, 77])
    assert np.all(om[bad] < 0.2) and np.median(om[np.setdiff1d(np.arange(om.size), bad)]) > 0.9
    with pytest.raises(ValueError):
        oracle_irls(s, 'huber', 1.5, 'apriori', damping='newton')


def test_host_irls_recovers_blunders():
    s = blundered('tiny')
    bad = np.array([5, 40, 77])
    for loss, k, sm in (('huber', 1.5, 'apriori'), ('cauchy', 2.385, 'apriori')):
        x, om, outer, conv, scales, chg, code = oracle_irls(s, loss, k, sm, max_outer=20)
        assert code == 0 and conv and outer >= 2, (loss, outer, conv, code)
        assert np.all(om[bad] < 0.2), (loss, om[bad])
        clean = np.setdiff1d(np.arange(om.size), bad)
        assert np.median(om[clean]) > 0.9
        assert len(scales) == outer and all(sc > 0 for sc in scales)
