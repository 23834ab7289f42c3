"""bundle_reliability on the device (dbat_hip_redundancy): the hat-matrix blocks of every image point and the
redundancy numbers of the prior rows against diag(I - J inv(J'J) J') from the oracle's weighted Jacobian, the
invariants of Qvv, the routes of the covariance machinery against each other (dense inverse, giant points, heavy
points, 2 and 4 ranks), and blunders found by the standardized residuals."""
import numpy as np
import pytest
import scipy.sparse as sp

import dbat_oracle as o
from helpers import camcal_struct, giant_points_struct, roma_struct, sxb_prior_eo_struct, synth_struct
from test_reliability_cpu import _oracle_setup, dense_reliability

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def hip():
    from dbat_amd import _hip
    import torch
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    _hip.load()
    return _hip


def _device(hip, s, x=None):
    h = hip.Handle(s)
    try:
        x = h.serialize() if x is None else x
        qvv, rp = h.redundancy(x)
        return qvv, rp, h.m, h.n
    finally:
        h.close()


def _check_invariants(qvv, rp, m, n):
    r = np.concatenate([qvv[0], qvv[2], rp])
    assert abs(r.sum() - (m - n)) <= 1e-9 * m, (r.sum(), m - n)
    assert r.min() >= -1e-10 and r.max() <= 1 + 1e-10
    # every 2 x 2 Qvv positive semidefinite
    tr, det = qvv[0] + qvv[2], qvv[0] * qvv[2] - qvv[1] ** 2
    assert np.all(tr >= -1e-10) and np.all(det >= -1e-10 * np.maximum(tr, 1) ** 2)


def _scenes():
    return [('tiny-' + v, lambda v=v: synth_struct('tiny', v)[0]) for v in ('plain', 'selfcal', 'imagevar', 'priors', 'groups4')] + \
        [('camcal', camcal_struct), ('sxb-prior-eo', lambda: sxb_prior_eo_struct(True)[0])]


@pytest.mark.parametrize('name,make', _scenes(), ids=[n for n, _ in _scenes()])
def test_dense_parity_and_invariants(hip, name, make):
    s = make()
    so, rw, qvv_o, rp_o, r_o, maps, n = dense_reliability(s)
    _, x0, _ = _oracle_setup(s)
    qvv, rp, m, nn = _device(hip, s, x0)
    assert (m, nn) == (r_o.size, n)
    assert np.abs(qvv - qvv_o).max() <= 1e-9
    assert rp.shape == rp_o.shape and (rp.size == 0 or np.abs(rp - rp_o).max() <= 1e-9)
    _check_invariants(qvv, rp, m, nn)


def test_invariants_roma(hip):
    s = roma_struct()
    _check_invariants(*_device(hip, s))


def test_sampled_at_size_C1(hip):
    """synth C1 with priors (100 cameras, 10 000 points): 200 image points and every prior row against sparse direct
    solves of J'J."""
    import scipy.sparse.linalg as spl
    s = synth_struct('C1', 'priors')[0]
    so, x, w = _oracle_setup(s)
    qvv, rp, m, n = _device(hip, s, x)
    from concurrent.futures import ThreadPoolExecutor
    r_o, K = o.brown_euler_cam4(x, so, jac=True)
    J = (sp.diags(np.sqrt(w)) @ K).tocsr()
    # the point unknowns first: their 3 x 3 blocks eliminate without fill (J'J's default ordering takes 20 s here)
    isop = np.zeros(J.shape[1], bool)
    isop[np.asarray(so.bundle.deserial.OP.src)] = True
    J = J[:, np.r_[np.flatnonzero(isop), np.flatnonzero(~isop)]].tocsr()
    lu = spl.splu((J.T @ J).tocsc(), permc_spec='NATURAL', diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
    no = s.IP.val.shape[1]
    ks = np.sort(np.random.default_rng(11).choice(no, 200, replace=False))
    rows = np.concatenate([np.c_[2 * ks, 2 * ks + 1].ravel(), np.arange(2 * no, m)])
    Jt = J[rows].toarray()
    Bt = Jt.T.copy()
    with ThreadPoolExecutor(8) as ex:                   # inv(J'J) J_t', in column chunks
        X = np.hstack(list(ex.map(lambda c: lu.solve(Bt[:, c:c + 128].copy()), range(0, Bt.shape[1], 128))))
    H = np.einsum('ij,ji->i', Jt, X)
    Huv = np.einsum('ij,ji->i', Jt[0:400:2], X[:, 1:400:2])
    assert np.abs(qvv[0, ks] - (1 - H[0:400:2])).max() <= 1e-8
    assert np.abs(qvv[2, ks] - (1 - H[1:400:2])).max() <= 1e-8
    assert np.abs(qvv[1, ks] + Huv).max() <= 1e-8
    assert rp.size == m - 2 * no > 0 and np.abs(rp - (1 - H[400:])).max() <= 1e-8
    _check_invariants(qvv, rp, m, n)


def _giant_scene():
    """test_giant_points' scene: three control points seen in all 140 images (more than a 128-observation batch)."""
    return giant_points_struct(140, 500, 'selfcal')[0]


def test_routes_agree(hip, monkeypatch):
    """Selected inverse (default) against the dense inverse, giant points forced, heavy points off."""
    s = synth_struct('small', 'priors')[0]
    q1, r1, m, n = _device(hip, s)
    _check_invariants(q1, r1, m, n)
    monkeypatch.setenv('DBAT_HIP_COV_DENSE', '1')
    q2, r2, _, _ = _device(hip, s)
    monkeypatch.delenv('DBAT_HIP_COV_DENSE')
    assert np.abs(q2 - q1).max() <= 1e-10 and np.abs(r2 - r1).max() <= 1e-10
    g = _giant_scene()
    qa, ra, m, n = _device(hip, g)                      # heavy / giant points on the matrix cores for the build
    _check_invariants(qa, ra, m, n)
    monkeypatch.setenv('DBAT_HIP_BT', '128')
    monkeypatch.setenv('DBAT_HIP_GIANT_THREADS', '64')
    qb, rb, _, _ = _device(hip, g)                      # giant points (three chunks of 64 threads each)
    monkeypatch.setenv('DBAT_HIP_HEAVY', '0')
    qc, rc, _, _ = _device(hip, g)
    assert np.abs(qb - qa).max() <= 1e-10 and np.abs(qc - qa).max() <= 1e-10
    monkeypatch.setenv('DBAT_HIP_COV_DENSE', '1')
    qd, rd, _, _ = _device(hip, g)
    assert np.abs(qd - qa).max() <= 1e-10


@pytest.mark.parametrize('world', [2, 4])
def test_ranks_agree(hip, world):
    from test_multishard_gpu import _run_ranks, _scene
    s = _scene('small-priors')
    h = hip.Handle(s)
    try:
        x0 = h.serialize()
        q1, r1 = h.redundancy(x0)
    finally:
        h.close()

    def work(comm):
        hh = hip.Handle(s, shard_rank=comm.rank, shard_count=comm.world_size)
        try:
            hh.set_allreduce(comm.allreduce_ptr)
            return hh.redundancy(x0)
        finally:
            hh.close()

    out, _ = _run_ranks(s, world, work)
    for q, r in out:
        assert np.abs(q - q1).max() <= 1e-10 and np.abs(r - r1).max() <= 1e-10


def test_blunders_are_found_and_handle_is_reused(hip):
    from dbat_amd import _hip, bundle, bundle_reliability
    s, _ = synth_struct('small', 'plain', seed=21)
    res, ok, iters, s0, E = bundle(s, 'gna')
    assert ok
    rel = bundle_reliability(res, E)
    assert _hip.cache_stats['last'] == 'hit'
    no = s.IP.val.shape[1]
    m, n = E.numObs, E.numParams
    assert abs(rel.total - (m - n)) <= 1e-9 * m and rel.r.shape == (m,)
    # no blunders: the number of T above the chi^2(2) quantile stays within a binomial bound
    a = rel.critical.alpha0
    nabove = int(np.count_nonzero(rel.IP.T > rel.critical.chi2_2))
    assert nabove == len(rel.suspects.ip) and nabove <= no * a + 6 * np.sqrt(no * a) + 3
    # five blunders of 15 sigma on u: distinct points with at least 4 rays, distinct images
    rays = np.bincount(s.IP.pt, minlength=s.OP.val.shape[1])
    rng = np.random.default_rng(4)
    pick, used_pt, used_cam = [], set(), set()
    for k in rng.permutation(no):
        if rays[s.IP.pt[k]] >= 4 and s.IP.pt[k] not in used_pt and s.IP.cam[k] not in used_cam:
            pick.append(int(k)); used_pt.add(int(s.IP.pt[k])); used_cam.add(int(s.IP.cam[k]))
            if len(pick) == 5:
                break
    sb, _ = synth_struct('small', 'plain', seed=21)
    sb.IP.val = np.array(sb.IP.val, float)
    sb.IP.val[0, pick] += 15.0 * np.asarray(sb.IP.std, float)[0, pick]
    res, ok, iters, s0, E = bundle(sb, 'gna')
    assert ok
    rel = bundle_reliability(res, E)
    assert _hip.cache_stats['last'] == 'hit'
    assert sorted(rel.suspects.ip[:5].tolist()) == sorted(pick)
    assert np.all(np.diff(rel.suspects.T) <= 0)
    assert np.all(np.isfinite(rel.IP.mdb)) and np.all(rel.IP.mdb > 0)


def test_singular_result_raises(hip):
    from dbat_amd import BadInput, bundle, bundle_reliability
    s, _ = synth_struct('tiny', 'plain')
    p = s.IP.pt[0]                                      # a point measured in one image only: code -4
    keep = ~((s.IP.pt == p) & (np.arange(len(s.IP.pt)) != 0))
    s.IP.val, s.IP.std = s.IP.val[:, keep], s.IP.std[:, keep]
    s.IP.cam, s.IP.pt = s.IP.cam[keep], s.IP.pt[keep]
    res, ok, iters, s0, E = bundle(s, 'gna')
    assert E.code == -4 and not ok
    with pytest.raises(BadInput, match='singular'):
        bundle_reliability(res, E)
