"""Ray intersection angles, host side (no GPU): dbat_hip_debug_ray_angles_host -- the definition the device kernels of
csrc/angles.hpp implement, with their arithmetic -- against a NumPy restatement of the reference's
photogrammetry/angles.m:26-46 and camangles.m:26-46 (normalise, Gram matrix, clip, acos(abs), max), and the presence
of the binding.

Comparison rule (shared with tests/test_ray_angles_gpu.py): where the reference angle is finite,
|cos a - cos a_ref| <= 1e-14 -- about ten roundings of a unit-vector dot product (two normalisations and a three-term
sum) with a margin of roughly five; in cosine space, because acos is ill-conditioned at 0 and the bound is not.  NaN
(no ray) and exact 0.0 (one ray) must match exactly."""
import copy

import numpy as np
import pytest

from helpers import camcal_struct, synth_struct

COS_TOL = 1e-14
MIN_ANGLE = 1e-3           # every multi-ray set of a test scene must open wider than this (checked per scene)


def ref_angles(s):
    """(op, cam, op_rays, cam_rays): angles.m and camangles.m restated on the IP columns of s."""
    EO, OP = np.asarray(s.EO.val, float)[:3], np.asarray(s.OP.val, float)
    cam, pt = np.asarray(s.IP.cam), np.asarray(s.IP.pt)

    def side(n, own, other, apex, ends):
        order = np.argsort(own, kind='stable')
        cnt = np.bincount(own, minlength=n)
        start = np.r_[0, np.cumsum(cnt)]
        a = np.full(n, np.nan)
        for i in range(n):
            e = other[order[start[i]:start[i + 1]]]
            if len(e) == 1:
                a[i] = 0.0
            elif len(e) > 1:
                d = apex[:, i:i + 1] - ends[:, e]
                dn = d / np.sqrt(np.sum(d * d, 0))
                a[i] = np.arccos(np.abs(np.clip(dn.T @ dn, -1, 1))).max()
        return a, cnt
    op, op_rays = side(OP.shape[1], pt, cam, OP, EO)
    ca, cam_rays = side(EO.shape[1], cam, pt, EO, OP)
    return op, ca, op_rays, cam_rays


def check_angles(got, ref, rays):
    """The comparison rule of this module's docstring; the scene must keep clear of the ill-conditioned end."""
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    assert got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isnan(ref), rays == 0)
    one = rays == 1
    assert np.all(got[one] == 0.0) and np.all(ref[one] == 0.0)
    multi = rays > 1
    if multi.any():
        assert ref[multi].min() > MIN_ANGLE, 'scene with a multi-ray set below %g rad' % MIN_ANGLE
        err = np.abs(np.cos(got[multi]) - np.cos(ref[multi])).max()
        print('max |cos a - cos a_ref| = %.3g over %d sets' % (err, multi.sum()))
        assert err <= COS_TOL


def thin(s, keep):
    """s with the IP columns of the mask only."""
    t = copy.deepcopy(s)
    keep = np.asarray(keep, bool)
    t.IP.cam, t.IP.pt = np.ascontiguousarray(s.IP.cam[keep]), np.ascontiguousarray(s.IP.pt[keep])
    t.IP.val = np.asfortranarray(np.asarray(s.IP.val)[:, keep])
    t.IP.std = np.asfortranarray(np.broadcast_to(np.asarray(s.IP.std, float), np.asarray(s.IP.val).shape)[:, keep])
    return t


def edge_scene():
    """'tiny' thinned by hand: point 0 has no ray, point 1 one ray, image 0 no point, image 1 one point (that of
    point 1).  Their parameters are fixed: nothing here is meant to be adjusted."""
    s, _ = synth_struct('tiny')
    cam, pt = np.asarray(s.IP.cam), np.asarray(s.IP.pt)
    keep = (pt != 0) & (cam != 0) & (pt != 1) & (cam != 1)
    cols = np.flatnonzero((pt == 1) & (cam != 0))
    if np.any(cam[cols] == 1):
        keep[cols[cam[cols] == 1][0]] = True
    else:                                       # point 1 is not measured in image 1: give image 1 another point's column
        keep[np.flatnonzero((cam == 1) & (pt > 1))[0]] = True
        keep[cols[0]] = True
    t = thin(s, keep)
    t.bundle.est.OP[:, :2] = False
    t.bundle.est.EO[:, :2] = False
    return t


def scene(name):
    if name == 'camcal':
        return camcal_struct()
    if name == 'edges':
        return edge_scene()
    return synth_struct(name)[0]


@pytest.mark.parametrize('name', ['tiny', 'small', 'camcal', 'edges'])
def test_host_restatement_matches_the_reference_definition(name):
    from dbat_amd import _hip
    s = scene(name)
    op_r, cam_r, op_rays, cam_rays = ref_angles(s)
    op, cam = _hip.debug_ray_angles_host(s)
    check_angles(op, op_r, op_rays)
    check_angles(cam, cam_r, cam_rays)
    assert (op_rays > 1).any() and (cam_rays > 1).any()


def test_no_ray_is_nan_and_one_ray_is_exactly_zero():
    from dbat_amd import _hip
    s = edge_scene()
    op_rays = np.bincount(s.IP.pt, minlength=s.OP.val.shape[1])
    cam_rays = np.bincount(s.IP.cam, minlength=s.EO.val.shape[1])
    assert op_rays[0] == 0 and op_rays[1] == 1 and cam_rays[0] == 0 and cam_rays[1] == 1
    op, cam = _hip.debug_ray_angles_host(s)
    assert np.isnan(op[0]) and op[1] == 0.0 and not np.signbit(op[1])
    assert np.isnan(cam[0]) and cam[1] == 0.0 and not np.signbit(cam[1])
    assert np.all(np.isfinite(op[op_rays > 0])) and np.all(np.isfinite(cam[cam_rays > 0]))


def test_the_reference_restatement_is_report_angles():
    """The NumPy restatement above and report._angles (the host loop the report uses by default) are the same numbers."""
    from dbat_amd import report
    s = scene('tiny')
    vis, _ = report._vis(s)
    assert np.array_equal(report._angles(s, vis), ref_angles(s)[0], equal_nan=True)


def test_symbols_and_bindings_are_present():
    import dbat_amd
    from dbat_amd import _hip, driver
    assert callable(dbat_amd.ray_angles) and dbat_amd.ray_angles is driver.ray_angles
    lib = _hip.load()
    for name in ('dbat_hip_ray_angles', 'dbat_hip_debug_ray_angles_host'):
        assert name in _hip.SYMBOLS and hasattr(lib, name)
    assert hasattr(_hip.Handle, 'ray_angles')


def test_report_keyword_reproduces_the_default_point_angles_block():
    """bundle_result_lines(point_angles=...) writes the same lines as the default path from the same numbers, and
    touches neither report._angles nor (for that block) the dense table."""
    from dbat_amd import report
    s = scene('tiny')
    op, _, op_rays, _ = ref_angles(s)
    p = report._P
    ids = np.asarray(s.OP.id)
    called = []
    orig = report._angles
    report._angles = lambda *a: called.append(1) or orig(*a)
    try:
        # the block alone, through the quality section's own code: a struct with the fields that section reads
        import scipy.sparse as sp
        t = copy.deepcopy(s)
        t.post = type(s.prior)(res=type(s.prior)(IP=np.zeros_like(np.asarray(s.IP.val, float))))
        COP = sp.identity(t.OP.val.size, format='csc')
        vop = (np.zeros(0, int), np.zeros(0, int), np.zeros(0))
        a = report._quality_lines(t, None, COP, vop)
        assert called
        del called[:]
        b = report._quality_lines(t, None, COP, vop, point_angles=(op, op_rays))
        assert not called
    finally:
        report._angles = orig
    assert a == b and (p * 2 + 'Point Angles') in b
    i0 = b.index(p * 2 + 'Point Angles')
    assert any('Smallest angles' in ln for ln in b[i0:]) and ids.size == op.size
    with pytest.raises(ValueError):
        report._quality_lines(t, None, COP, vop, point_angles=(op[:-1], op_rays[:-1]))
