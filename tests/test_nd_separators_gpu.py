"""The factorisation with every kind of separator of the nested dissection (csrc/nd.hpp, DBAT_HIP_ND_SEP = 0, 1, 2): only
the elimination order of the reduced system differs, so one linearize_solve step agrees with the oracle at the suite's 1e-8
and with the step of mode 0 at 1e-10, and the posterior covariance (the selected inversion reads the compact factor) with
mode 0's at 1e-8.  'small' scenes (several tiles, a dissection with separators), fixed IO and self-calibration.  The
orders themselves: tests/test_nd_separators_cpu.py."""
import copy

import numpy as np
import pytest
import scipy.sparse as sp

import dbat_oracle as o
from helpers import relerr

pytestmark = pytest.mark.gpu

TOL_STEP = 1e-8       # against the oracle, as tests/test_hip_parity.py
TOL_ORDER = 1e-10     # against mode 0: the same sums in another order
TOL_COV = 1e-8


@pytest.fixture(scope='module')
def hip():
    from dbat_amd import _hip
    import torch
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    _hip.load()
    return _hip


_scenes = {}


def scene(selfcal):
    """(struct, x0, the oracle's scaled Gauss-Newton step) -- computed once.  selfcal 'C1': the 100-camera scene, fixed
    IO -- 'small' (40 cameras) stays one dense block whatever the separators, C1 is the smallest scene whose orders differ
    (tests/test_nd_separators_cpu.py prints them)."""
    if selfcal not in _scenes:
        from dbat_amd import synth
        if selfcal == 'C1':
            s, _ = synth.make_scene('C1')
        else:
            s, _ = synth.make_scene('small', selfcal=True) if selfcal else synth.make_scene('small')
        so = copy.deepcopy(s)
        for nm in ('IO', 'EO', 'OP'):
            pr = getattr(so.prior, nm)
            pr.use = np.asarray(pr.use, bool) & np.asarray(getattr(so.bundle.est, nm), bool)
        so = o.buildserialindices(so)
        x0, w = o.serialize(so), o.buildweightvector(so)
        R = np.sqrt(w)
        r_o, K = o.brown_euler_cam4(x0, so, jac=True)
        p_o = o._scaled_gn((sp.diags(R) @ K).tocsc(), R * r_o)[0]
        _scenes[selfcal] = (s, x0, p_o)
    return _scenes[selfcal]


def step(hip, s, x0, cov=False):
    h = hip.Handle(s)
    try:
        p, st = h.linearize_solve(x0, 0.0, True)
        assert not st['singular'] and h.structural_rank_ok()
        return (p, h.posterior_cov(x0, 1.0)) if cov else p
    finally:
        h.close()


@pytest.mark.parametrize('selfcal', [False, True, 'C1'], ids=['fixed-io', 'selfcal', 'C1'])
def test_step_with_every_separator_mode(hip, selfcal, monkeypatch):
    s, x0, p_o = scene(selfcal)
    monkeypatch.setenv('DBAT_HIP_ND_SEP', '0')
    ref = step(hip, s, x0)
    for mode in ('0', '1', '2'):
        monkeypatch.setenv('DBAT_HIP_ND_SEP', mode)
        p = step(hip, s, x0)
        e_o, e_0 = relerr(p, p_o), relerr(p, ref)
        print('%s mode %s: against the oracle %.2e, against mode 0 %.2e' % (selfcal, mode, e_o, e_0))
        assert e_o < TOL_STEP and e_0 < TOL_ORDER
    monkeypatch.delenv('DBAT_HIP_ND_SEP')
    assert relerr(step(hip, s, x0), ref) < TOL_ORDER          # the order the model chooses


@pytest.mark.parametrize('selfcal', [False, True, 'C1'], ids=['fixed-io', 'selfcal', 'C1'])
def test_posterior_covariance_with_minimum_cover_separators(hip, selfcal, monkeypatch):
    s, x0, _ = scene(selfcal)
    monkeypatch.setenv('DBAT_HIP_ND_SEP', '0')
    p0, C0 = step(hip, s, x0, cov=True)
    monkeypatch.setenv('DBAT_HIP_ND_SEP', '1')
    p1, C1 = step(hip, s, x0, cov=True)
    assert relerr(p1, p0) < TOL_ORDER
    for a, b, what in zip(C1, C0, ('CEO', 'CIO', 'COP')):
        if np.size(b) and np.any(b):
            print('%s %s: %.2e' % (selfcal, what, relerr(a, b)))
            assert relerr(a, b) < TOL_COV, what


@pytest.mark.parametrize('sep', ['0', '1'])
def test_sums_cut_where_two_parts_meet(hip, sep, monkeypatch):
    """DBAT_HIP_DF_MERGE (csrc/chol_df.hpp build_jobs): the sums of the columns where two parts of the dissection meet go
    to helper tasks in pieces of unequal length, owners of every kind (diagonal sums of the chain role, sum-only tasks,
    off-diagonal tiles) add them.  Forced on and off on the 100-camera scene -- the model takes it at 1000 cameras --
    the step is the oracle's, and the same to rounding."""
    s, x0, p_o = scene('C1')
    monkeypatch.setenv('DBAT_HIP_ND_SEP', sep)
    monkeypatch.setenv('DBAT_HIP_DF_MERGE', '0')
    ref, Cref = step(hip, s, x0, cov=True)
    monkeypatch.setenv('DBAT_HIP_DF_MERGE', '1')
    p, C = step(hip, s, x0, cov=True)
    print('separators %s, sums cut: against the oracle %.2e, against uncut %.2e' % (sep, relerr(p, p_o), relerr(p, ref)))
    assert relerr(ref, p_o) < TOL_STEP and relerr(p, p_o) < TOL_STEP and relerr(p, ref) < TOL_ORDER
    assert relerr(C[0], Cref[0]) < TOL_COV and relerr(C[2], Cref[2]) < TOL_COV
