"""Image coverage and marking-residual statistics on the device (dbat_hip_coverage, dbat_hip_residual_stats,
csrc/quality.hpp) against the NumPy restatement and the comparison rule of tests/test_quality_cpu.py: every point set
of that module, images at the wave and workgroup edges, circles at the LDS capacity of the hull kernel and beyond it
(the global-memory path), a scene whose points are tiled, heavy and giant, a real project; exact NaN / 0 / -1; handle
reuse; sharded handles; bit-identical repeats; the report's blocks through the quality= keyword.

Residual sums: n terms e^2 >= 0 summed in any fixed order differ from the NumPy sum by at most n eps relative each
way, the terms themselves by 2 eps: |ss - ss_ref| <= 4 n eps ss_ref.  max_e: 4 eps relative, and its column any whose
reference norm is that close to the largest."""
import numpy as np
import pytest

from helpers import camcal_struct, synth_struct
from test_quality_cpu import EPS, check_coverage, circle, cpu_cases, scene_with_points
from test_ray_angles_cpu import edge_scene

pytestmark = pytest.mark.gpu

EDGE_COUNTS = (63, 64, 65, 255, 256, 257)


@pytest.fixture(scope='module')
def hip():
    from dbat_amd import _hip
    import torch
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    _hip.load()
    return _hip


def device_coverage(hip, s):
    h = hip.Handle(s)
    try:
        return h.coverage(), h.info()
    finally:
        h.close()


def check_residual_stats(st, s, res_px):
    """st of Handle.residual_stats against the pixel residuals res_px (2, n_obs) of the same parameters."""
    cam, pt = np.asarray(s.IP.cam), np.asarray(s.IP.pt)
    nc, npnt = s.EO.val.shape[1], s.OP.val.shape[1]
    e2 = np.sum(np.asarray(res_px, float) ** 2, 0)
    cam_n, op_n = np.bincount(cam, minlength=nc), np.bincount(pt, minlength=npnt)
    assert np.array_equal(st['cam_n'], cam_n) and np.array_equal(st['op_n'], op_n)
    cam_ss, op_ss = np.zeros(nc), np.zeros(npnt)
    np.add.at(cam_ss, cam, e2)
    np.add.at(op_ss, pt, e2)
    for got, ref, n in ((st['cam_ss'], cam_ss, cam_n), (st['op_ss'], op_ss, op_n), (st['total_ss'], e2.sum(), len(e2))):
        err = np.abs(got - ref) / np.maximum(ref, np.finfo(float).tiny) / np.maximum(n, 1)
        print('sum of squares: largest relative error per term %.3g eps' % (np.max(err) / EPS))
        assert np.all(np.abs(got - ref) <= 4 * n * EPS * ref)
    assert np.all(st['cam_ss'][cam_n == 0] == 0) and np.all(st['op_ss'][op_n == 0] == 0)
    e = np.sqrt(e2)
    assert abs(st['max_e'] - e.max()) <= 4 * EPS * e.max()
    assert 0 <= st['max_ip'] < len(e) and e.max() - e[st['max_ip']] <= 4 * EPS * e.max()


def pixel_residuals(h, s, x):
    r, _ = h.residual(x)
    no = s.IP.val.shape[1]
    px = np.asarray(s.IO.sensor.pxSize, float)
    return r[:2 * no].reshape(2, no, order='F') / (px[:, :1] if px.shape[1] == 1 else px[:, np.asarray(s.IP.cam)])


def thinned_scene():
    from test_ray_angles_gpu import edges_dense_scene
    return edges_dense_scene()


def test_every_cpu_case_and_the_wave_and_workgroup_edges(hip):
    rng = np.random.default_rng(5)
    sets = cpu_cases() + [np.stack([rng.uniform(0, 3000, n), rng.uniform(0, 2000, n)]) for n in EDGE_COUNTS]
    s = scene_with_points(sets, extra_images=3)
    s.bundle.est.EO[:, :5] = False                   # images with fewer than three points are not adjusted
    got, _ = device_coverage(hip, s)
    assert check_coverage(got, s) == len(sets) + 3
    host = hip.debug_coverage_host(s)
    for k in ('lo', 'hi', 'rad_ip'):
        assert np.array_equal(got[k], host[k], equal_nan=True)
    assert all(np.array_equal(a, b) for a, b in zip(got['hull'], host['hull']))


def test_circles_at_the_lds_capacity_and_beyond(hip):
    """Every point of a circle is a hull vertex and the octagon filter drops none: CAP - 1 and CAP candidates are sorted
    in LDS, CAP + 1 and 2 CAP + 1 in global memory (one and two powers of two above the capacity)."""
    cap = hip.quality_hull_cap()
    counts = (cap - 1, cap, cap + 1, 2 * cap + 1)
    rng = np.random.default_rng(9)
    s = scene_with_points([circle(n, 3000.0, (4000.0, 3500.0))[:, rng.permutation(n)] for n in counts], extra_images=2)
    got, _ = device_coverage(hip, s)
    assert [len(h) for h in got['hull'][:4]] == list(counts)
    assert check_coverage(got, s) == 6


@pytest.mark.parametrize('name', ['thinned', 'camcal'])
def test_tiled_heavy_and_giant_points_and_a_real_project(hip, name):
    s = thinned_scene() if name == 'thinned' else camcal_struct()
    h = hip.Handle(s)
    try:
        info = h.info()
        if name == 'thinned':
            assert info['n_tiles'] > 0 and info['heavy_points'] >= 3
        else:
            assert info['n_tiles'] == 0
        x = h.serialize()
        cov, st = h.coverage(), h.residual_stats(x)
        res = pixel_residuals(h, s, x)
        again = h.coverage(), h.residual_stats(x)
    finally:
        h.close()
    assert check_coverage(cov, s) == s.EO.val.shape[1]
    check_residual_stats(st, s, res)
    # two calls give the same bits
    for a, b in zip((cov, st), again):
        for k in a:
            if k == 'hull':
                assert all(np.array_equal(u, v) for u, v in zip(a[k], b[k]))
            else:
                assert np.array_equal(a[k], b[k], equal_nan=True)


def same_bits(a, b):
    """Two results of the same call (a dict or a tuple of arrays and numbers) are bit-equal, hulls list by list."""
    a, b = (list(r.items()) if isinstance(r, dict) else list(enumerate(r)) for r in (a, b))
    assert [k for k, _ in a] == [k for k, _ in b]
    for (k, u), (_, v) in zip(a, b):
        if k == 'hull':
            assert len(u) == len(v) and all(np.array_equal(p, q) for p, q in zip(u, v))
        else:
            assert np.array_equal(u, v, equal_nan=True), k


def test_the_analyses_share_one_point_index(hip):
    """ray_angles and residual_stats take where every point's observations start, and which points are tiled or heavy,
    from one index that the first of them builds: whichever call comes first on a handle, and whatever ran in between
    (coverage, point_depths), every result has the same bits."""
    s = thinned_scene()
    calls = dict(coverage=lambda h, x: h.coverage(), angles=lambda h, x: h.ray_angles(x),
                 stats=lambda h, x: h.residual_stats(x), depths=lambda h, x: h.point_depths(x))
    runs = [('coverage', 'angles', 'stats', 'depths', 'angles', 'stats')]
    runs += [(lead,) + tuple(k for k in calls if k != lead) for lead in ('angles', 'stats', 'depths')]
    first = {}
    for order in runs:
        h = hip.Handle(s)
        try:
            info, x = h.info(), h.serialize()
            got = [(k, calls[k](h, x)) for k in order]
        finally:
            h.close()
        assert info['n_tiles'] > 0 and info['heavy_points'] >= 3          # both point kernels of both analyses run
        for k, r in got:
            same_bits(first.setdefault(k, r), r)
    assert set(first) == set(calls)
    # a point without a ray and a point with one, the statistics first
    s = edge_scene()
    h = hip.Handle(s)
    try:
        x = h.serialize()
        st = h.residual_stats(x)
        op, cam, opn, camn = h.ray_angles(x)
    finally:
        h.close()
    assert opn[0] == 0 and opn[1] == 1 and np.array_equal(st['op_n'], opn)
    assert np.isnan(op[0]) and op[1] == 0.0 and st['op_ss'][0] == 0.0


def adjustable_thinned_scene():
    """thinned_scene() as a network that can be adjusted: an image with fewer than six points does not determine its
    six exterior parameters well, so those images keep their start values (every point still has two rays or more)."""
    s = thinned_scene()
    few = np.bincount(np.asarray(s.IP.cam), minlength=s.EO.val.shape[1]) < 6
    assert few.any() and not few.all()
    s.bundle.est.EO[:, few] = False
    assert np.bincount(np.asarray(s.IP.pt), minlength=s.OP.val.shape[1]).min() >= 2
    return s


@pytest.mark.parametrize('name', ['small', 'thinned', 'camcal'])
def test_network_quality_after_a_bundle(hip, name):
    """The statistics at the adjusted values against s.post.res.IP, the pixel residuals bundle() leaves, with the
    bounds of check_residual_stats (every sum of n terms within 4 n eps relative, the maximum within 4 eps)."""
    from dbat_amd import bundle, network_quality
    s = synth_struct('small')[0] if name == 'small' else adjustable_thinned_scene() if name == 'thinned' else camcal_struct()
    hip.clear_cache()
    hits = hip.cache_stats['hits']
    res, ok, iters, s0, E = bundle(s, 'gna')
    assert ok, 'the bundle did not converge (code %d after %d iterations)' % (E.code, iters)
    h = hip.acquire(res)
    try:
        info = h.info()
        st = h.residual_stats(h.serialize())
    finally:
        hip.release(h)
    if name == 'thinned':
        assert info['n_tiles'] > 0 and info['heavy_points'] >= 3
    check_residual_stats(st, res, res.post.res.IP)
    q = network_quality(res, E)
    assert hip.cache_stats['hits'] == hits + 2                      # the handle bundle() left behind, twice
    hip.clear_cache()
    # network_quality: the same call, the roots and the NaN of a zero count formed on the host
    r = q.residuals
    no = res.IP.val.shape[1]
    assert r.rms == np.sqrt(st['total_ss'] / no) and r.max == st['max_e'] and r.max_ip == st['max_ip']
    assert np.array_equal(r.op_rays, st['op_n']) and np.array_equal(r.cam_points, st['cam_n'])
    with np.errstate(divide='ignore', invalid='ignore'):
        assert np.array_equal(r.op_rms, np.sqrt(st['op_ss'] / st['op_n']), equal_nan=True)
        assert np.array_equal(r.cam_rms, np.sqrt(st['cam_ss'] / st['cam_n']), equal_nan=True)
    assert not np.isnan(r.cam_rms[st['cam_n'] > 0]).any() and np.isnan(r.cam_rms[st['cam_n'] == 0]).all()


def test_other_pixel_coordinates_are_another_handle(hip):
    """The image points are part of the structure key: changed IP.val cannot reach a handle through set_values, it
    makes a new handle, which gives the new values."""
    from dbat_amd import network_quality
    s, _ = synth_struct('small')
    hip.clear_cache()
    q = network_quality(s)
    t, _ = synth_struct('small')
    t.IP.val = np.asfortranarray(np.asarray(t.IP.val, float) + 1.0)
    q2 = network_quality(t)
    assert hip.cache_stats['last'] == 'miss'
    hip.clear_cache()
    cam = np.asarray(t.IP.cam)
    assert np.array_equal(q2.coverage.lo, np.asarray([t.IP.val[:, cam == i].min(1) for i in range(t.EO.val.shape[1])]).T)
    assert np.array_equal(q2.coverage.lo, q.coverage.lo + 1.0)


@pytest.mark.parametrize('name', ['small', 'camcal'])
def test_set_values_moves_the_principal_point(hip, name):
    """What set_values can change for coverage() is the principal point (IO.val[1:3]; fixed in 'small', estimated in
    camcal): the radii follow it, everything else keeps its bits."""
    import copy
    s = synth_struct('small')[0] if name == 'small' else camcal_struct()
    t = copy.deepcopy(s)
    t.IO.val = np.array(s.IO.val, float, order='F')
    t.IO.val[1] += 0.7
    t.IO.val[2] -= 0.4
    h = hip.Handle(s)
    try:
        before = h.coverage()
        h.set_values(t)
        after = h.coverage()
        h.set_values(s)
        back = h.coverage()
    finally:
        h.close()
    nc = s.EO.val.shape[1]
    assert check_coverage(before, s) == nc and check_coverage(after, t) == nc
    assert np.all(after['rad_max'] != before['rad_max'])
    for k in ('lo', 'hi', 'hull_area'):
        assert np.array_equal(after[k], before[k])
    assert all(np.array_equal(u, v) for u, v in zip(after['hull'], before['hull']))
    assert np.array_equal(back['rad_max'], before['rad_max']) and np.array_equal(back['rad_ip'], before['rad_ip'])


def test_no_point_is_nan_zero_and_minus_one(hip):
    s = edge_scene()
    h = hip.Handle(s)
    try:
        x = h.serialize()
        cov, st = h.coverage(), h.residual_stats(x)
        res = pixel_residuals(h, s, x)
    finally:
        h.close()
    assert np.all(np.isnan(cov['lo'][:, 0])) and np.all(np.isnan(cov['hi'][:, 0])) and np.isnan(cov['rad_max'][0])
    assert cov['rad_ip'][0] == -1 and cov['hull_area'][0] == 0.0 and len(cov['hull'][0]) == 0
    assert len(cov['hull'][1]) == 1 and cov['hull_area'][1] == 0.0
    assert st['cam_n'][0] == 0 and st['cam_ss'][0] == 0.0 and st['op_n'][0] == 0 and st['op_ss'][0] == 0.0 and st['op_n'][1] == 1
    check_coverage(cov, s)
    check_residual_stats(st, s, res)


def test_a_shard_of_two_refuses(hip):
    s, _ = synth_struct('small', 'priors')
    x = hip.plan_serialize(s)
    for rank in range(2):
        h = hip.Handle(s, 0, rank, 2)
        try:
            for call in (h.coverage, lambda: h.residual_stats(x)):
                with pytest.raises(hip.DbatHipError) as e:
                    call()
                assert e.value.code == hip.EINVAL and 'shard' in str(e.value)
        finally:
            h.close()


def report_case(name):
    if name == 'camcal':
        return camcal_struct(3), None
    if name == 'sxb':
        from helpers import sxb_struct
        return sxb_struct(), None
    from helpers import prague_struct
    return prague_struct('c1')


@pytest.mark.parametrize('name', ['camcal', 'sxb', 'prague'])
def test_report_blocks_from_the_device(hip, name, monkeypatch):
    from dbat_amd import bundle, bundle_cov, network_quality, ray_angles, report
    s, _ = report_case(name)
    res, ok, iters, s0, E = bundle(s, 'gna')
    assert ok
    CIO, CEO, COP = bundle_cov(res, E, 'CIOF', 'CEO', 'COP')
    default = report.bundle_result_lines(res, E, CIO, CEO, COP)
    q, ra = network_quality(res, E), ray_angles(res, E)

    def never(*a, **k):
        raise AssertionError('the dense table / the host coverage loop was used')
    monkeypatch.setattr(report, '_vis', never)
    monkeypatch.setattr(report, '_coverage', never)
    lines = report.bundle_result_lines(res, E, CIO, CEO, COP, point_angles=(ra.op, ra.op_rays), quality=q)
    assert lines == default
    assert any('Convex hull:' in ln for ln in lines) and any('Overall point RMS' in ln for ln in lines)
