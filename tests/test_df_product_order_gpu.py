"""The factorisation with product lists (csrc/chol_df.hpp, DBAT_HIP_DF_SUMS): a listed task of k_chol_df takes the
products of its sum in the order fixed at plan time instead of column order.  Only the rounding of a reordered sum may
differ: one linearize_solve step with the switch at 0 (no lists), 1 (the model's lists), 2 (every task a list in column
order) and 3 (every task a list in descending column order) agrees with the others at 1e-10 and with the oracle's full
sparse solve at the suite's 1e-8; deterministic mode stays bit-identical from run to run; the selected inversion reads
the same factor tiles.  The smallest scenes whose lists differ from column order: C1 (100 cameras, two parts and
separators), 'small' with self-calibration (dense IO rows: the long sums with helpers), roma (irregular pattern).  The
lists themselves: tests/test_df_product_order_cpu.py."""
import copy

import numpy as np
import pytest
import scipy.sparse as sp

import dbat_oracle as o
from helpers import relerr, roma_struct, synth_struct

pytestmark = pytest.mark.gpu

TOL_STEP = 1e-8       # against the oracle, as tests/test_hip_parity.py
TOL_ORDER = 1e-10     # among the switch values: the same sums in another order
TOL_COV = 1e-9
SWITCH = ('0', '1', '2', '3')


@pytest.fixture(scope='module')
def hip():
    from dbat_amd import _hip
    import torch
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    _hip.load()
    return _hip


_scenes = {}


def scene(name):
    """(struct, x0, the oracle's scaled Gauss-Newton step) -- computed once."""
    if name not in _scenes:
        from dbat_amd import synth
        if name == 'C1':
            s, _ = synth.make_scene('C1')
        elif name == 'small-selfcal':
            s, _ = synth_struct('small', 'selfcal')
        else:
            s = roma_struct()
        so = copy.deepcopy(s)
        for nm in ('IO', 'EO', 'OP'):
            pr = getattr(so.prior, nm)
            pr.use = np.asarray(pr.use, bool) & np.asarray(getattr(so.bundle.est, nm), bool)
        so = o.buildserialindices(so)
        x0, w = o.serialize(so), o.buildweightvector(so)
        R = np.sqrt(w)
        r_o, K = o.brown_euler_cam4(x0, so, jac=True)
        p_o = o._scaled_gn((sp.diags(R) @ K).tocsc(), R * r_o)[0]
        _scenes[name] = (s, x0, p_o)
    return _scenes[name]


def step(hip, s, x0, cov=False, deterministic=False, runs=1):
    h = hip.Handle(s)
    try:
        if deterministic:
            h.set_deterministic(True)
        out = []
        for _ in range(runs):
            p, st = h.linearize_solve(x0, 0.0, True)
            assert not st['singular'] and h.structural_rank_ok()
            out.append((p, st))
        if cov:
            return out[0][0], h.posterior_cov(x0, 1.0)
        return out if runs > 1 else out[0]
    finally:
        h.close()


@pytest.mark.parametrize('name', ['C1', 'small-selfcal', 'roma'])
def test_step_with_every_product_order(hip, name, monkeypatch):
    s, x0, p_o = scene(name)
    got = {}
    for sw in SWITCH:
        monkeypatch.setenv('DBAT_HIP_DF_SUMS', sw)
        got[sw] = step(hip, s, x0)
    for sw in SWITCH:
        p, st = got[sw]
        ratio = np.sqrt(st['rcond'])                              # min pivot / max pivot
        print('%s switch %s: against the oracle %.2e, chol_info %d, min / max pivot %.15e' % (name, sw, relerr(p, p_o), st['chol_info'], ratio))
        assert st['chol_info'] == 0
        assert relerr(p, p_o) < TOL_STEP
        for other in SWITCH:
            e = relerr(p, got[other][0])
            ep = abs(ratio - np.sqrt(got[other][1]['rcond'])) / ratio
            if other > sw:
                print('   against switch %s: step %.2e, pivot extremes %.2e' % (other, e, ep))
            assert e < TOL_ORDER and ep < TOL_ORDER, (sw, other, e, ep)


@pytest.mark.parametrize('name', ['C1', 'small-selfcal', 'roma'])
def test_deterministic_mode_is_bit_identical_with_lists(hip, name, monkeypatch):
    s, x0, _ = scene(name)
    monkeypatch.setenv('DBAT_HIP_DF_SUMS', '1')
    (p1, st1), (p2, st2) = step(hip, s, x0, deterministic=True, runs=2)
    assert np.array_equal(p1, p2) and st1 == st2
    p3, st3 = step(hip, s, x0, deterministic=True)                # ... and from one handle to the next
    assert np.array_equal(p1, p3) and st1 == st3


def test_posterior_covariance_with_lists(hip, monkeypatch):
    s, x0, _ = scene('C1')
    monkeypatch.setenv('DBAT_HIP_DF_SUMS', '0')
    p0, C0 = step(hip, s, x0, cov=True)
    monkeypatch.setenv('DBAT_HIP_DF_SUMS', '1')
    p1, C1 = step(hip, s, x0, cov=True)
    assert relerr(p1, p0) < TOL_ORDER
    n = 0
    for a, b, what in zip(C1, C0, ('CEO', 'CIO', 'COP')):
        if np.size(b) and np.any(b):
            print('C1 %s: %.2e' % (what, relerr(a, b)))
            assert relerr(a, b) < TOL_COV, what
            n += 1
    assert n >= 2
