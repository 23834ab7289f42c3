"""dbat_hip_forwintersect (k_forwintersect, k_forwintersect_giant; csrc/kernels.hpp, csrc/initial_host.hpp) at its
edges, against the longdouble forward intersection of tests/resect_ref.py and the float64 restatement
oracle/initial_oracle.py forwintersect: lens terms and IO layouts, the giant-point kernel, batch boundaries, points
with 0 ... 3 rays, near-parallel rays, project coordinates of 1e6 m, and sharded handles.  The scenes and the float64
restatement's own error on each: tests/initial_cases.py, tests/test_initial_ref_cpu.py.

The 8x rule, per scene: the device's largest error against longdouble is at most 8 times the float64 restatement's
plus 16 eps * max|coordinate| -- both evaluate the same sums in float64, in another order and with another 3 x 3 solve.

The figures in the docstrings were measured on an MI355X (gfx950); every test prints its own (pytest -s).  The largest
ratio of all is 3.79, at the two-ray point of the ray-count scene (3.9e-13 m against 1.0e-13 m; 0.40 of the bound)."""
import numpy as np
import pytest

import initial_cases as IC
import resect_ref as RR

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps


@pytest.fixture(scope='module')
def hip():
    from dbat_amd import _hip
    import torch
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    _hip.load()
    return _hip


def _device(hip, s, skip=None, info=None):
    h = hip.Handle(s)
    try:
        if info is not None:
            info.update(h.info())
        return h.forwintersect(h.serialize(), s.OP.val, skip=skip)
    finally:
        h.close()


def _check(name, Qd, tag=''):
    """The 8x rule on a scene; returns (device error, restatement error)."""
    s, Qld, Qo, e_orc, cap, scale = IC.fwd_reference(name)
    ok = np.isfinite(np.asarray(Qld, float)).all(0)
    assert np.array_equal(np.isnan(Qd).all(0), ~ok) and np.array_equal(np.isnan(Qd).any(0), ~ok)
    per_point = np.max(np.abs(RR.LD(1) * Qd[:, ok] - Qld[:, ok]), 0).astype(float)
    e_dev = float(per_point.max())
    bound = 8 * e_orc + 16 * EPS * scale
    print('%s%s: device %.3e restatement %.3e ratio %.2f bound %.3e (share %.2f), worst point %d'
          % (name, tag, e_dev, e_orc, e_dev / e_orc, bound, e_dev / bound, np.flatnonzero(ok)[int(np.argmax(per_point))]))
    assert np.all(per_point <= bound), (name, tag, e_dev, e_orc, bound)
    return e_dev, e_orc


@pytest.mark.parametrize('name', ['tiny-selfcal', 'tiny-imagevar', 'tiny-groups4', 'tiny-np3',
                                  'camcal-m1', 'camcal-m2', 'camcal-m4', 'camcal-m5'])
def test_lens_and_io_variants(hip, name):
    """Self-calibrated, image-variant and four-group IO with K1..K3, P1, P2 all non-zero and different from block to
    block, a third tangential coefficient (nP = 3), and the camcal project under distortion models 1, 2, 4 and 5.
    Measured: device / restatement error between 0.89 and 1.30 (errors of 1.2e-13 ... 1.7e-13 m on the synthetic
    scenes, 8.7e-16 m on camcal), at most 0.14 of the bound.  Without the factor 1 + P3 in fwd_ray_terms the nP = 3
    scene fails and nothing else does."""
    s = IC.fwd_reference(name)[0]
    _check(name, _device(hip, s))


@pytest.mark.parametrize('env', ['', 'DBAT_HIP_BT=128', 'DBAT_HIP_BT=128 DBAT_HIP_GIANT_THREADS=64'])
def test_giant_points(hip, env, monkeypatch):
    """Three points seen in all 140 images: inside a batch by default, through k_forwintersect_giant with batches of
    128 observations (the only place that kernel runs).
    Measured: 3.5e-13 m against the restatement's 2.8e-13 m (ratio 1.23) on all three routes."""
    for kv in env.split():
        monkeypatch.setenv(*kv.split('='))
    s = IC.fwd_reference('giant')[0]
    info = {}
    Q = _device(hip, s, info=info)
    assert info['max_k'] == 140 and info['BT'] == (128 if env else 256)
    _check('giant', Q, ' [%s]' % env)


def test_batch_boundaries(hip):
    """Eight rays per point: 32 points fill a batch of 256 observations exactly, so a point's rays end at the boundary
    and the next point opens the next batch; every point on its own under the rule."""
    s = IC.fwd_reference('batch-edge')[0]
    st = hip.batch_stats(s)
    nb = st['n_batches_tiled'] + st['n_batches_untiled']
    assert max(st['tiled']['max_obs'], st['untiled']['max_obs']) == st['BT'] == 256 and nb >= 3
    assert np.all(np.bincount(s.IP.pt) == 8)
    _check('batch-edge', _device(hip, s))


def test_ray_counts_skip_and_ids(hip):
    """Points with 0, 1, 2 and 3 rays in one scene: NaN, NaN, the midpoint of the common perpendicular (closed form in
    longdouble), the least-squares point.  A skip mask keeps the caller's values bit for bit and leaves the other
    points as they are without it; an id subset through initial.forwintersect does the same."""
    from dbat_amd import initial
    s, Qld, Qo, e_orc, cap, scale = IC.fwd_reference('ray-counts')
    assert list(np.bincount(s.IP.pt, minlength=4)[:4]) == [0, 1, 2, 3]
    Q = _device(hip, s)
    assert np.isnan(Q[:, :2]).all() and np.isfinite(Q[:, 2:]).all()
    _check('ray-counts', Q)
    c, d = RR.rays_ld(s)
    r = np.flatnonzero(s.IP.pt == 2)
    mid = RR.two_ray_midpoint(c[:, r[0]], d[:, r[0]], c[:, r[1]], d[:, r[1]])
    assert float(np.max(np.abs(RR.LD(1) * Q[:, 2] - mid))) <= 8 * e_orc + 16 * EPS * scale
    skip = np.arange(s.OP.val.shape[1]) % 3 == 0                   # (point 0, without rays, among them)
    Qs = _device(hip, s, skip=skip)
    assert np.array_equal(Qs[:, skip].view(np.int64), s.OP.val[:, skip].view(np.int64))
    assert np.array_equal(Qs[:, ~skip].view(np.int64), Q[:, ~skip].view(np.int64))
    ids = s.OP.id[1::2]
    Qi = initial.forwintersect(s, ids=ids).OP.val
    take = np.isin(s.OP.id, ids)
    assert np.array_equal(Qi[:, take].view(np.int64), Q[:, take].view(np.int64))
    assert np.array_equal(Qi[:, ~take].view(np.int64), s.OP.val[:, ~take].view(np.int64))


@pytest.mark.parametrize('name', ['angle-1e-1', 'angle-1e-2', 'angle-1e-3', 'angle-1e-1-far', 'angle-1e-2-far',
                                  'angle-1e-3-far', 'tiny-far'])
def test_geometry(hip, name):
    """Two rays meeting at 1e-1, 1e-2 and 1e-3 rad, at the origin and with the offset of 1e6 m, and the twelve-image
    scene with that offset.  The device and the float64 restatement lose the same digits (4 / theta^2 in the 3 x 3
    matrix, max|coordinate| in the uncentred right-hand side): DESIGN.md 8.
    Measured, device / restatement (m): 1e-1 rad 3.1e-12 / 3.9e-12 (0.79), 1e-2 rad 3.9e-10 / 3.2e-10 (1.23), 1e-3 rad
    3.4e-8 / 2.7e-8 (1.26); with the offset 1.3e-7 / 1.3e-7 (1.00), 1.5e-5 / 9.1e-6 (1.67), 1.5e-3 / 1.3e-3 (1.09);
    the twelve-image scene with the offset 1.1e-8 / 1.5e-8 (0.77).  At most 0.21 of the bound."""
    s = IC.fwd_reference(name)[0]
    _check(name, _device(hip, s))


# ---- sharded handles -----------------------------------------------------------------------------------------------------

def _shard_scene(kind):
    from dbat_amd import synth
    from helpers import synth_struct
    if kind == 'small-priors':
        return synth_struct('small', 'priors')[0]
    # the 15 x 15 grid of tests/test_multishard_gpu.py with a tenth of its points: still four non-empty domains
    return synth.make_scene('C1', cams=225, points=600, rays=6, selfcal=True, groups=4)[0]


def _thinned(s):
    """(s', p0, p1): s with every observation of one point removed and another point cut down to a single ray."""
    import copy
    t = copy.deepcopy(s)
    p0, p1 = 7, 12
    rows1 = np.flatnonzero(t.IP.pt == p1)
    keep = (t.IP.pt != p0) & (t.IP.pt != p1)
    keep[rows1[0]] = True
    return IC._keep_obs(t, keep), p0, p1


def _same(a, b, rel=1e-12):
    nan = np.isnan(b)
    return np.array_equal(np.isnan(a), nan) and np.abs(a[~nan] - b[~nan]).max() <= rel * np.abs(b[~nan]).max()


@pytest.mark.parametrize('kind,world', [('small-priors', 2), ('small-priors', 3), ('grid', 4)])
def test_sharded_handles(hip, kind, world):
    """'Collective on a sharded handle' (include/dbat_hip.h): every rank returns the one-rank result to 1e-12 relative
    -- every point is computed once, by its owner, from ALL its rays (the points seen from cameras of the top
    separators among them), and the sum over the ranks only adds zeros.  With one point's observations removed and one
    point cut down to a single ray, both are NaN on every rank.  The skip mask is honoured on every rank.
    (Before this test the point without observations came back as (0, 0, 0) from a sharded handle: no rank wrote it,
    and the host took every point of the sum for seen.  Whether a point has a ray now rides in the sum.)"""
    from test_multishard_gpu import _run_ranks
    s0 = _shard_scene(kind)
    cam_owner, subtree = hip.plan_domain_map(s0, world)
    assert subtree
    if kind == 'grid':
        assert np.all(np.bincount(cam_owner[cam_owner >= 0], minlength=world) > 0)
    sep = np.unique(s0.IP.pt[cam_owner[s0.IP.cam] < 0])
    assert sep.size > 0                                             # (points with rays from a top-separator camera)
    t, p0, p1 = _thinned(s0)
    skip = np.arange(s0.OP.val.shape[1]) % 5 == 1
    for s, lost in ((s0, []), (t, [p0, p1])):
        h = hip.Handle(s)
        try:
            x0 = h.serialize()
            Q1 = h.forwintersect(x0, s.OP.val)
            Q1s = h.forwintersect(x0, s.OP.val, skip=skip)
        finally:
            h.close()
        assert np.isnan(Q1[:, lost]).all() and np.isfinite(np.delete(Q1, lost, 1)).all()

        def work(comm):
            hh = hip.Handle(s, shard_rank=comm.rank, shard_count=comm.world_size)
            try:
                hh.set_allreduce(comm.allreduce_ptr)
                return hh.forwintersect(x0, s.OP.val), hh.forwintersect(x0, s.OP.val, skip=skip), hh.info()['n_pts_shard']
            finally:
                hh.close()

        out, _ = _run_ranks(s, world, work)
        assert sum(o[2] for o in out) == s.OP.val.shape[1]          # (every point has one owner)
        for rank, (Q, Qs, _) in enumerate(out):
            assert np.isnan(Q[:, lost]).all(), (rank, Q[:, lost])
            assert _same(Q, Q1), (rank, np.nanmax(np.abs(Q - Q1)))
            assert _same(Q[:, sep], Q1[:, sep])
            assert np.array_equal(Qs[:, skip].view(np.int64), s.OP.val[:, skip].view(np.int64)), rank
            assert _same(Qs, Q1s), rank
