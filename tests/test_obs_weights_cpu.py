"""The reference of tests/test_obs_weights_gpu.py checked on its own (no GPU): the oracle's step on the struct with
IP.std / sqrt(omega) is the least-squares solution of diag(sqrt(omega) (x) 1_2) applied to the base weighted rows --
by dense numpy.linalg.lstsq where the scene has at most ~4000 unknowns, by a sparse factorisation of the augmented
system [I -J; J' 0] (which never forms J'J) for the 60 x 3000 crowded scenes, by a second factorisation of J'J (pivoted
LU, another ordering) for the 12 000 unknowns of the mixed scene.  Agreement to 1e-10 leaves two orders of
magnitude under the 1e-8 the GPU test allows the device.  The reweighted normal matrix must not be singular."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import dbat_oracle as o
from helpers import obs_weight_factors, relerr, reweighted_struct, std_pattern
from test_obs_weights_gpu import BASES, OMEGA_LO, SCENES, make_scene, oracle_setup, scene_omega

DENSE_MAX_N = 4000
AUGMENTED_MAX_N = 10000      # (beyond that the augmented system's fill takes minutes: a second factorisation of J'J)
# scenes that share one struct are checked once
DISTINCT = [n for n in SCENES if n not in ('tile3', 'bt128', 'mixed-columns')]


def _weighted_system(s):
    so, x0, w = oracle_setup(s)
    R = np.sqrt(w)
    r_o, K = o.brown_euler_cam4(x0, so, jac=True)
    return (sp.diags(R) @ K).tocsc(), R * r_o


def test_weight_factors_are_as_specified():
    om = obs_weight_factors(20000, 1)
    assert om.min() == 1e-2 and om.max() == 1.0
    assert 0.09 < np.mean(om == 1.0) < 0.11 and 0.007 < np.mean(om == 1e-2) < 0.013
    mid = np.log(om[(om > 1e-2) & (om < 1.0)])
    assert abs(mid.mean() - np.log(1e-1)) < 0.05 and np.histogram(mid, 4)[0].min() > 0.22 * mid.size   # log-uniform
    assert np.array_equal(om, obs_weight_factors(20000, 1)) and not np.array_equal(om[:100], obs_weight_factors(100, 2))
    assert obs_weight_factors(5000, 3, lo=0.1).min() == 0.1


@pytest.mark.parametrize('base', BASES)
@pytest.mark.parametrize('name', DISTINCT)
def test_oracle_step_on_reweighted_struct_is_the_row_scaled_problem(name, base, monkeypatch):
    s = make_scene(name, monkeypatch)
    if base == 'nonuniform':
        s = std_pattern(s)
    om = scene_omega(name, s, BASES.index(base))
    assert om.min() == OMEGA_LO[name]
    J, r = _weighted_system(reweighted_struct(s, om))
    p_o, sing, Jn, Jn2, Hs, gs, Js = o._scaled_gn(J, r)
    assert not sing and np.all(np.isfinite(p_o))
    # independent statement: the BASE struct's weighted rows, image rows scaled by sqrt(omega)
    Jb, rb = _weighted_system(s)
    d = np.ones(Jb.shape[0])
    d[:2 * om.size] = np.repeat(np.sqrt(om), 2)
    A = (sp.diags(d) @ Jb).tocsc()
    b = d * rb
    m, n = A.shape
    cn = np.sqrt(np.asarray(A.multiply(A).sum(0)).ravel())            # (column scaling: conditioning only)
    As = (A @ sp.diags(1.0 / cn)).tocsc()
    if n <= DENSE_MAX_N:
        q, _, rank, sv = np.linalg.lstsq(As.toarray(), -b, rcond=None)
        assert rank == n and sv[-1] > 1e-12 * sv[0]                    # the normal matrix is not singular
    elif n > AUGMENTED_MAX_N:
        H = (As.T @ As).tocsc()
        lu = spl.splu(H, permc_spec='COLAMD')                          # (pivoted LU in another order than the oracle's)
        g = -(As.T @ b)
        q = lu.solve(g)
        q += lu.solve(g - H @ q)
        du = np.abs(lu.U.diagonal())
        assert du.min() > 1e-12 * du.max()
    else:
        K = sp.bmat([[sp.identity(m), -As], [As.T, None]], format='csc')
        lu = spl.splu(K)
        rhs = np.concatenate([b, np.zeros(n)])
        y = lu.solve(rhs)
        y += lu.solve(rhs - K @ y)                                     # one step of refinement
        q = y[m:]
        L = spl.splu(Hs, permc_spec='MMD_AT_PLUS_A', diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
        du = np.abs(L.U.diagonal())
        assert du.min() > 1e-12 * du.max()
    p_ref = q / cn
    err = relerr(p_o, p_ref)
    print('%s %s: n = %d, oracle against the row-scaled problem %.2e' % (name, base, n, err))
    assert err <= 1e-10
