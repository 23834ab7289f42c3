"""Ray intersection angles on the device (dbat_hip_ray_angles, csrc/angles.hpp) against the NumPy restatement of
photogrammetry/angles.m / camangles.m of tests/test_ray_angles_cpu.py, with that module's cosine bound: the lane-group
kernel of the tiled points, the workgroup kernel of the heavy / giant points, the matrix-core pair kernel of the
images at every tile and workgroup edge; exact NaN / 0.0; ray counts; the report's "Point Angles" block; handle
reuse; sharded handles; bit-identical repeats."""
import os

import numpy as np
import pytest

from helpers import GOLDEN, camcal_struct, synth_struct
from test_ray_angles_cpu import check_angles, edge_scene, ref_angles, thin

pytestmark = pytest.mark.gpu

IMAGE_POINTS = (15, 16, 17, 33, 255, 257)          # images 0 .. 5: the 16-tile edges, a run of 8 tiles, two workgroups
POINT_RAYS = (2, 16, 17, 64, 65, 270, 21, 22)      # points 0 .. 7: 270 = every image (a giant point), 21 | 22: tiled | heavy


@pytest.fixture(scope='module')
def hip():
    from dbat_amd import _hip
    import torch
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    _hip.load()
    return _hip


def edges_dense_scene():
    """An all-see-all scene (270 images x 300 points) thinned by hand to the ray counts above."""
    from dbat_amd import synth
    nc, npnt = 270, 300
    s, _ = synth.make_dense_scene(nc, npnt, False, 1, 3)
    V = np.zeros((npnt, nc), bool)
    V[5, :] = True
    for p, k in enumerate(POINT_RAYS):
        if p != 5:
            V[p, 6:6 + k] = True
    for i, n in enumerate(IMAGE_POINTS):
        V[8:8 + n - 1, i] = True                     # (+ point 5)
    for p in range(8, npnt):                         # eight more rays each: enough tiled observations for tiles to exist
        for t in range(8):
            V[p, 80 + (p + 13 * t) % 190] = True
    return thin(s, V[s.IP.pt, s.IP.cam])


def device_angles(hip, s):
    h = hip.Handle(s)
    try:
        return h.ray_angles(h.serialize()), h.info()
    finally:
        h.close()


@pytest.fixture(scope='module')
def dense():
    s = edges_dense_scene()
    return s, ref_angles(s)


@pytest.mark.parametrize('name', ['tiny', 'small', 'camcal'])
def test_device_matches_the_reference_definition(hip, name):
    s = camcal_struct() if name == 'camcal' else synth_struct(name)[0]
    op_r, cam_r, op_rays, cam_rays = ref_angles(s)
    (op, cam, opn, camn), info = device_angles(hip, s)
    if name == 'camcal':                             # 21 images, every point heavy, about 100 rays per image
        # (at most 21 rays each: heavy not by their count but because the plan sends every point the heavy way where
        # heavy points exist and the others are few -- nothing is tiled)
        assert s.EO.val.shape[1] == 21 and info['n_tiles'] == 0 and info['heavy_points'] == np.count_nonzero(op_rays)
        assert 90 <= cam_rays.mean() <= 110
    else:
        assert info['n_tiles'] > 0
    assert np.array_equal(opn, op_rays) and np.array_equal(camn, cam_rays)
    check_angles(op, op_r, op_rays)
    check_angles(cam, cam_r, cam_rays)               # (cam_angle's known answer: the restatement; the reference prints none)


def test_every_tile_and_threshold_edge_once(hip, dense):
    s, (op_r, cam_r, op_rays, cam_rays) = dense
    assert tuple(cam_rays[:6]) == IMAGE_POINTS and tuple(op_rays[:8]) == POINT_RAYS
    (op, cam, opn, camn), info = device_angles(hip, s)
    assert info['n_tiles'] > 0 and info['heavy_points'] >= 3          # both point kernels ran
    assert np.array_equal(opn, np.bincount(s.IP.pt, minlength=len(op))) and np.array_equal(camn, np.bincount(s.IP.cam, minlength=len(cam)))
    check_angles(op, op_r, op_rays)
    check_angles(cam, cam_r, cam_rays)


def test_no_ray_is_nan_and_one_ray_is_exactly_zero(hip):
    s = edge_scene()
    (op, cam, opn, camn), _ = device_angles(hip, s)
    assert opn[0] == 0 and opn[1] == 1 and camn[0] == 0 and camn[1] == 1
    assert np.isnan(op[0]) and op[1] == 0.0 and np.isnan(cam[0]) and cam[1] == 0.0
    op_r, cam_r, op_rays, cam_rays = ref_angles(s)
    check_angles(op, op_r, op_rays)
    check_angles(cam, cam_r, cam_rays)


def test_two_calls_give_the_same_bits(hip, dense):
    s, _ = dense
    h = hip.Handle(s)
    try:
        x = h.serialize()
        a, b = h.ray_angles(x), h.ray_angles(x)
    finally:
        h.close()
    for u, v in zip(a, b):
        assert np.array_equal(u, v, equal_nan=True)


def test_report_point_angles_block_from_device_angles(hip):
    """The camcal model-3 report with the device's angles through the keyword: its "Point Angles" block is the committed
    reference report's, line for line (the block the default path reproduces too)."""
    from dbat_amd import bundle, bundle_cov, ray_angles, report
    s = camcal_struct(3)
    res, ok, iters, s0, E = bundle(s, 'gna')
    assert ok
    CIO, CEO, COP = bundle_cov(res, E, 'CIOF', 'CEO', 'COP')
    ra = ray_angles(res, E)
    called = []
    orig = report._angles
    report._angles = lambda *a: called.append(1) or orig(*a)
    try:
        lines = report.bundle_result_lines(res, E, CIO, CEO, COP, point_angles=(ra.op, ra.op_rays))
        assert not called
        default = report.bundle_result_lines(res, E, CIO, CEO, COP)
        assert called
    finally:
        report._angles = orig

    def block(ls):
        ls = [ln.rstrip() for ln in ls]
        i0 = ls.index(report._P * 2 + 'Point Angles')
        i1 = next(i for i in range(i0 + 1, len(ls)) if ls[i].startswith(report._P * 2) and not ls[i].startswith(report._P * 3))
        return ls[i0:i1]
    gold = open(os.path.join(GOLDEN, 'camcal-dbatreport.txt')).read().splitlines()
    got = block(lines)
    assert len(got) > 8 and got == block(gold) and got == block(default)


def test_ray_angles_reuses_the_cached_handle(hip):
    from dbat_amd import bundle, ray_angles
    s, _ = synth_struct('small', 'selfcal')
    hip.clear_cache()
    st = dict(hip.cache_stats)
    res, ok, iters, s0, E = bundle(s, 'gna')
    assert hip.cache_stats['misses'] == st['misses'] + 1 and hip.cache_stats['hits'] == st['hits']
    a = ray_angles(res, E)
    assert hip.cache_stats['hits'] == st['hits'] + 1 and hip.cache_stats['misses'] == st['misses'] + 1
    hip.clear_cache()
    b = ray_angles(res, E)                           # a fresh handle
    assert hip.cache_stats['misses'] == st['misses'] + 2
    hip.clear_cache()
    for k in ('op', 'cam', 'op_rays', 'cam_rays'):
        assert np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True)
    op_r, cam_r, op_rays, cam_rays = ref_angles(res)     # at the values in the result struct
    check_angles(a.op, op_r, op_rays)
    check_angles(a.cam, cam_r, cam_rays)


def test_a_shard_of_two_refuses(hip):
    """Two shards on one GPU (the handles test_two_shards_one_gpu_match_single runs its bundle on: shard r of 2 of
    'small' with priors): pairs of rays across ranks are out of scope, and every shard says so before any device work
    (x from the host-only plan: a sharded handle's own serialize() is a collective)."""
    s, _ = synth_struct('small', 'priors')
    x = hip.plan_serialize(s)
    for rank in range(2):
        h = hip.Handle(s, 0, rank, 2)
        try:
            with pytest.raises(hip.DbatHipError) as e:
                h.ray_angles(x)
            assert e.value.code == hip.EINVAL and 'shard' in str(e.value)
        finally:
            h.close()
