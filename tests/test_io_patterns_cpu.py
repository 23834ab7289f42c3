"""Interior-orientation patterns (helpers.IO_PATTERNS) without a device: the route the host plan gives every pattern,
and the preconditions of tests/test_io_patterns_gpu.py on the oracle alone.

The layout table pins which kernels a pattern reaches (tiles or none, signature groups for the build and for the
back-substitution, heavy points): a plan change that silently reroutes a pattern fails here, and the GPU tests stay
tests of the route they name."""
import copy

import numpy as np
import pytest
import scipy.sparse as sp

import dbat_oracle as o
from helpers import IO_PATTERNS, IO_PRIOR_CASES, io_pattern_struct, relerr

# pattern: (nIO, tiles > 0, build_sig, backsub_sig, heavy_tasks > 0) of the tiny scene, default environment
TINY_LAYOUT = {
    'fixed-k0p0': (0, True, True, True, False),
    'fixed-k5p5': (0, True, True, True, False),
    'cc-only': (1, True, True, False, False),
    'as-sk-only': (2, True, True, False, False),
    'k0p0-cc-pp': (3, True, True, False, False),
    'k4p0-radial': (5, True, True, False, False),
    'all10': (10, False, False, False, False),
    'k5p2-11cols': (11, False, False, False, False),
    'k5p2-all12': (12, False, False, False, False),
    'half-fixed-half-std8': (8, True, True, False, False),
    'half-cc-half-std8': (9, True, True, False, False),
    'half-std8-half-9': (17, False, False, False, True),
    '2x-std8-interleaved': (16, True, True, True, False),
    '2x-9-interleaved': (18, False, False, False, True),
    '3x-std8-interleaved': (24, False, False, False, True),
    'cc-shared-K-per-group': (11, True, True, True, False),
}

# the three 'small' cases of the GPU file: tiles that straddle the two halves; the first mixes tile2 and heavy
SMALL_LAYOUT = {
    'half-std8-half-9': (17, True, False, False, True),
    'cc-shared-K-per-group': (11, True, True, True, False),
    'half-cc-half-std8': (9, True, True, False, False),
}


UNTILED = ('all10', 'k5p2-11cols', 'k5p2-all12')                 # ncolmax > 15: CMAX = 0, the MAXCOL instantiations
TILED = tuple(p for p, w in TINY_LAYOUT.items() if w[1])
HEAVY = tuple(p for p, w in TINY_LAYOUT.items() if w[4])


def routes(pattern):
    """(switch, value, expected build kernel, tiles > 0, heavy > 0, build_sig, backsub_sig) of every route the pattern
    can reach."""
    nIO, tiles, bsig, bksig, heavy = TINY_LAYOUT[pattern]
    tile_kernel = 'k_build_tile3' if nIO == 0 else 'k_build_tile2'
    if pattern in TILED:
        return [(None, None, 'k_build_sig', True, False, True, bksig),
                ('DBAT_HIP_SIG', '0', tile_kernel, True, False, False, False),
                ('DBAT_HIP_SIG', '2', 'k_build_sig', True, False, True, bksig),      # backsub_sig: fixed IO or all_std8
                ('DBAT_HIP_SIG_IOS_OFF', '1', 'k_build_sig', True, False, True, bksig),
                ('DBAT_HIP_CMAX', '0', 'k_build', False, False, False, False)]
    if pattern in HEAVY:
        # without the heavy route the column lists take the points with more than 16 IO columns; half-std8-half-9
        # keeps one tile (the points seen by cameras of one half only)
        one_tile = pattern == 'half-std8-half-9'
        return [(None, None, 'k_heavy_z + k_heavy_syrk', False, True, False, False),
                ('DBAT_HIP_HEAVY', '0', 'k_build_tile2' if one_tile else 'k_build', one_tile, False, False, False)]
    return [(None, None, 'k_build', False, False, False, False)]


def oracle_setup(s):
    s = copy.deepcopy(s)
    for nm in ('IO', 'EO', 'OP'):
        pr = getattr(s.prior, nm)
        pr.use = np.asarray(pr.use, bool) & np.asarray(getattr(s.bundle.est, nm), bool)
    s = o.buildserialindices(s)
    return s, o.serialize(s), o.buildweightvector(s)


def weighted_system(s):
    so, x0, w = oracle_setup(s)
    R = np.sqrt(w)
    r_o, K = o.brown_euler_cam4(x0, so, jac=True)
    return so, x0, R * r_o, (sp.diags(R) @ K).tocsc()


def check_layout(s, want, n_oracle=None):
    from dbat_amd import _hip
    nIO, tiles, bsig, bksig, heavy = want
    P, L = _hip.plan(s), _hip.plan_layout_stats(s)
    nEO = int(np.count_nonzero(s.bundle.est.EO))
    assert (P['nIO'], P['nEO'], P['nOP']) == (nIO, nEO, 3 * s.OP.val.shape[1]) and P['n'] == nIO + P['nEO'] + P['nOP']
    if n_oracle is not None:
        assert P['n'] == n_oracle
    assert (L['n_tiles'] > 0) == tiles, L
    assert (L['build_sig'], L['backsub_sig']) == (bsig, bksig), L
    assert (L['heavy_tasks'] > 0) == heavy, L
    assert _hip.plan_structural_rank_ok(s)
    return P, L


def test_the_tables_cover_every_pattern():
    assert set(TINY_LAYOUT) == set(IO_PATTERNS) and len(IO_PATTERNS) == 16
    assert set(SMALL_LAYOUT) <= set(IO_PATTERNS)
    assert [c[0] for c in IO_PRIOR_CASES] == ['2x-9-interleaved', 'half-cc-half-std8', 'all10', 'cc-shared-K-per-group']


@pytest.mark.parametrize('pattern', list(IO_PATTERNS))
def test_tiny_layout_and_oracle_preconditions(pattern):
    """Route of the pattern; and what makes the oracle a reference for it: a non-singular scaled Gauss-Newton step, which
    a random permutation of the rows of r and J moves by less than 1e-10 (measured with this permutation: 8e-14 for
    fixed-k0p0 up to 9.2e-12 for k5p2-all12 -- the noise floor of the reference's own sums, far below the GPU tests'
    1e-8), and an undamped bundle that converges (3 to 8 iterations)."""
    s, _ = io_pattern_struct('tiny', pattern)
    nK, nP = IO_PATTERNS[pattern][:2]
    assert s.IO.val.shape[0] == 5 + nK + nP and (s.IO.model.nK, s.IO.model.nP) == (nK, nP)
    so, x0, r, J = weighted_system(s)
    check_layout(s, TINY_LAYOUT[pattern], len(x0))
    p, sing, *_ = o._scaled_gn(J, r)
    assert not sing and np.all(np.isfinite(p))
    perm = np.random.default_rng(1).permutation(len(r))
    p2, sing2, *_ = o._scaled_gn(J.tocsr()[perm].tocsc(), r[perm])
    assert not sing2
    print('%s: permuted-row step differs by %.2e' % (pattern, relerr(p2, p)))
    assert relerr(p2, p) < 1e-10
    res, ok, iters, s0, E = o.bundle(s, 'gna')
    assert ok and E.code == 0 and 2 <= iters <= 10


@pytest.mark.parametrize('pattern', list(SMALL_LAYOUT))
def test_small_layout(pattern):
    s, _ = io_pattern_struct('small', pattern)
    P, L = check_layout(s, SMALL_LAYOUT[pattern])
    assert L['n_tiles'] > 8                               # many tiles: some lie in one half, some straddle both
    if pattern == 'half-std8-half-9':
        assert 0 < L['n_batches_tiled'] < L['n_batches']  # tiled and heavy points side by side


@pytest.mark.parametrize('pattern', list(IO_PATTERNS))
def test_layout_of_every_route(pattern, monkeypatch):
    """The host half of tests/test_io_patterns_gpu.py::test_routes: what every switch makes of the pattern's layout."""
    from dbat_amd import _hip
    s, _ = io_pattern_struct('tiny', pattern)
    assert len(routes(pattern)) == (5 if pattern in TILED else 2 if pattern in HEAVY else 1)
    assert (pattern in UNTILED) == (not TINY_LAYOUT[pattern][1] and not TINY_LAYOUT[pattern][4])
    for switch, value, kernel, tiles, heavy, bsig, bksig in routes(pattern):
        if switch:
            monkeypatch.setenv(switch, value)
        L = _hip.plan_layout_stats(s)
        assert (L['n_tiles'] > 0, L['heavy_tasks'] > 0, L['build_sig'], L['backsub_sig']) == (tiles, heavy, bsig, bksig), (switch, L)
        if switch:
            monkeypatch.delenv(switch)


@pytest.mark.parametrize('pattern', HEAVY)
def test_heavy_plan_of_the_interleaved_blocks(pattern):
    """17, 18 and 24 IO columns under one point: the row groups, slots and tasks of the heavy route replayed on the
    host against the plain sum of z_p z_p' (tests/test_heavy_plan_cpu.py)."""
    from dbat_amd import _hip
    s, _ = io_pattern_struct('tiny', pattern)
    st = _hip.heavy_plan_selftest(s)
    assert st['on'] and st['tasks'] == _hip.plan_layout_stats(s)['heavy_tasks'] > 0 and st['points'] == s.OP.val.shape[1]
    assert st['max_diff'] <= 1e-10 * max(st['max_abs'], 1.0), st


@pytest.mark.parametrize('pattern,rows,n_prior', IO_PRIOR_CASES, ids=[c[0] for c in IO_PRIOR_CASES])
def test_prior_cases(pattern, rows, n_prior):
    """prior.IO.use is set for every camera of the rows: the reference keeps the leading, estimated entries
    (buildserialindices.m:138, bundle.m's use & est), and so must the plan -- same m, same n."""
    from dbat_amd import _hip
    s, _ = io_pattern_struct('tiny', pattern, rows)
    nc = s.EO.val.shape[1]
    assert int(np.count_nonzero(s.prior.IO.use)) == len(rows) * nc > n_prior
    pr = list(rows)
    assert np.array_equal(s.prior.IO.val[pr], s.IO.val[pr] * (1 + 1e-3) + 1e-4)
    assert np.array_equal(s.prior.IO.std[pr], np.abs(s.IO.val[pr]) * 1e-2 + 1e-3) and s.prior.IO.std[pr].min() >= 1e-3
    so, x0, r, J = weighted_system(s)
    P = _hip.plan(s)
    assert len(so.post.res.ix.IO) == n_prior
    assert (P['m'], P['n']) == (so.post.res.ix.n, len(x0)) and P['m'] == 2 * s.IP.val.shape[1] + n_prior
    p, sing, *_ = o._scaled_gn(J, r)
    assert not sing
    res, ok, iters, s0, E = o.bundle(s, 'gna')
    assert ok and E.code == 0


def test_fixed_k5p5_values_differ_per_camera():
    s, _ = io_pattern_struct('tiny', 'fixed-k5p5')
    nc = s.EO.val.shape[1]
    for row in (0, 8, 9, 10, 11, 12, 13, 14):
        assert len(np.unique(s.IO.val[row])) == nc and np.all(s.IO.val[row] != 0)
    # each term moves an image-corner point (18, 12) mm by about a pixel
    u = np.array([[18.0], [12.0]])
    px = float(s.IO.sensor.pxSize[0, 0])
    io = s.IO.val[:, 0]
    K, P = io[5:10], io[10:15]
    for j in (3, 4):
        Kj = np.zeros(5); Kj[j] = K[j]
        assert 0.5 < np.linalg.norm(o.brown_rad(u, Kj)) / px < 2
    t2 = np.linalg.norm(o.brown_tang(u, P[:2]))
    assert 0.3 < t2 / px < 3
    for j in (2, 3, 4):
        Pj = np.r_[P[:2], np.zeros(3)]; Pj[j] = P[j]
        assert 0.5 < np.linalg.norm(o.brown_tang(u, Pj) - o.brown_tang(u, P[:2])) / t2 < 2


def test_estimated_P3_is_refused_by_the_structure_test():
    """nP > 2 with P3 estimated, at the scene's P1 = P2 = 0.  The reference multiplies the P1, P2 displacement by
    1 + P3 r^2 + ... (brown_tang.m:58-70): its column of J is identically zero, the oracle's scaled step is singular
    (zero column norm).  That is why P3-P5 stay fixed in every pattern.  The plan accepts the struct (dbat_hip_plan
    gives n and m) and reports plan_structural_rank_ok false: the reference's sparse J stores no exact zeros, so its
    sprank(J) at x0 is n - 1 (gauss_newton_armijo.m:132-142, code -4).  (Before this test the plan counted the
    column's entries as structural and reported full rank.)  With a non-zero P1 the same struct has full rank."""
    from dbat_amd import _hip
    from dbat_amd.dbatstruct import make_struct, seteoest_depend
    base, _ = io_pattern_struct('tiny', 'fixed-k0p0')
    nc = base.EO.val.shape[1]
    IO = np.zeros((11, nc))
    IO[0:5] = base.IO.val[0:5]
    est = np.zeros((11, nc), bool)
    est[[0, 8, 9, 10]] = True                               # cc, P1, P2, P3 at nK = 3, nP = 3
    s = seteoest_depend(make_struct(IO, base.EO.val, base.OP.val, base.IP.val, base.IP.cam, base.IP.pt,
                                    float(base.IO.sensor.pxSize[0, 0]), nK=3, nP=3, estIO=est), 0)
    so, x0, r, J = weighted_system(s)
    Jn = np.sqrt(np.asarray(J.multiply(J).sum(0)).ravel())
    assert np.count_nonzero(Jn == 0) == 1 and Jn[3] == 0    # x = [IO; EO; OP]: cc, P1, P2, P3
    with np.errstate(all='ignore'):
        p, sing, *_ = o._scaled_gn(J, r)
    assert sing or not np.all(np.isfinite(p))
    P = _hip.plan(s)
    assert (P['n'], P['m']) == (len(x0), len(r))
    assert not _hip.plan_structural_rank_ok(s)
    s.IO.val[8] = 1e-6
    assert _hip.plan_structural_rank_ok(s)
    s.IO.val[8] = 0.0
    s.bundle.est.IO[10] = False                             # P3 fixed: nothing depends on P1 = P2 = 0
    assert _hip.plan_structural_rank_ok(s)
