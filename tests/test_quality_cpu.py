"""Image coverage, host side (no GPU): dbat_hip_debug_coverage_host -- the code of the device kernel of
csrc/quality.hpp (octagon filter, order, chain scan, shoelace sum) on one thread -- against a NumPy restatement of
photogrammetry/coverage.m:113-185: initial._hull plus a shoelace sum, min / max, the radial arg max.  The restatement
itself is pinned to the reference's output: it reproduces the coverage lines of two committed reports.

Comparison rule (shared with tests/test_quality_gpu.py), eps = 2^-52, W x H the image's bounding box of points:
  lo, hi          equal exactly (min and max round nothing)
  rad_max         within 4 eps relative: two products, two differences, a sum of squares and a square root, each half
                  an eps, with a margin of about two; rad_ip any column whose reference radius is that close to the
                  largest
  hull vertices   equal as a set of coordinates, except points whose orientation test against an edge of the reference
                  hull is within 8 eps W H of zero (the rounding of one test is below 4 eps W H): those may be on either
                  side -- among them every collinear boundary point, which initial._hull keeps for n <= 3
  hull area       |a - a_ref| <= 8 h eps W H for h vertices: every term of the shoelace sum is a test of that kind
"""
import os
import re

import numpy as np
import pytest

from helpers import GOLDEN, camcal_struct
from test_ray_angles_cpu import thin

EPS = 2.0 ** -52


def radii(s, i, pts):
    px, pp = np.asarray(s.IO.sensor.pxSize, float)[:, i], np.asarray(s.IO.val, float)[1:3, i]
    return np.sqrt((pts[0] * px[0] - pp[0]) ** 2 + (-pts[1] * px[1] - pp[1]) ** 2)


def ref_hull(pts):
    """(vertex indices counter-clockwise, area) of a 2-by-n point set: initial._hull and the shoelace sum."""
    from dbat_amd.initial import _hull
    n = pts.shape[1]
    if n == 0:
        return [], 0.0
    h = np.asarray(_hull(pts), np.int64)
    if n < 3:
        return list(h), 0.0
    c = pts[:, h].mean(1)
    h = h[np.argsort(np.arctan2(pts[1, h] - c[1], pts[0, h] - c[0]), kind='stable')]
    q = pts[:, h] - pts.min(1, keepdims=True)
    return list(h), 0.5 * abs(float(np.sum(q[0] * np.roll(q[1], -1) - np.roll(q[0], -1) * q[1])))


def image_columns(s):
    cam = np.asarray(s.IP.cam)
    assert np.all(np.diff(cam) >= 0)
    return np.searchsorted(cam, np.arange(s.EO.val.shape[1] + 1))


def check_coverage(got, s):
    """The comparison rule of this module's docstring, image by image; returns the number of images checked."""
    uv = np.asarray(s.IP.val, float)
    st = image_columns(s)
    nc = len(st) - 1
    assert got['lo'].shape == (2, nc) and len(got['hull']) == nc
    for i in range(nc):
        pts = uv[:, st[i]:st[i + 1]]
        n = pts.shape[1]
        hull = np.asarray(got['hull'][i])
        if n == 0:
            assert np.all(np.isnan(got['lo'][:, i])) and np.all(np.isnan(got['hi'][:, i])) and np.isnan(got['rad_max'][i])
            assert got['rad_ip'][i] == -1 and got['hull_area'][i] == 0.0 and len(hull) == 0
            continue
        assert np.array_equal(got['lo'][:, i], pts.min(1)) and np.array_equal(got['hi'][:, i], pts.max(1))
        r = radii(s, i, pts)
        assert abs(got['rad_max'][i] - r.max()) <= 4 * EPS * r.max()
        k = got['rad_ip'][i] - st[i]
        assert 0 <= k < n and r.max() - r[k] <= 4 * EPS * r.max()
        W, H = pts.max(1) - pts.min(1)
        assert np.all((hull >= st[i]) & (hull < st[i + 1])) and len(set(hull)) == len(hull)
        hv, area = ref_hull(pts)
        a, b = {tuple(pts[:, j]) for j in hull - st[i]}, {tuple(pts[:, j]) for j in hv}
        assert len(a) == len(hull), 'a point listed twice'
        if len(b) >= 2:
            poly = pts[:, hv]
            nxt = np.roll(poly, -1, 1)
            for p in a ^ b:
                cr = (nxt[0] - poly[0]) * (p[1] - poly[1]) - (nxt[1] - poly[1]) * (p[0] - poly[0])
                assert np.abs(cr).min() <= 8 * EPS * W * H, 'image %d: vertex sets differ at %r' % (i, p)
        else:
            assert a == b
        err = abs(got['hull_area'][i] - area)
        print('image %d: %d points, %d vertices, area error %.3g (bound %.3g)' % (i, n, len(hull), err, 8 * len(hull) * EPS * W * H))
        assert err <= 8 * len(hull) * EPS * W * H
        # the listing: counter-clockwise from the lowest (u, v), strictly convex
        if len(hull) >= 3:
            q = uv[:, hull]
            assert tuple(q[:, 0]) == min(a)
            d1, d2 = np.roll(q, -1, 1) - q, np.roll(q, -2, 1) - np.roll(q, -1, 1)
            assert np.all(d1[0] * d2[1] - d1[1] * d2[0] > 0)
    return nc


def circle(n, r=900.0, c=(1000.0, 800.0)):
    t = 2 * np.pi * (np.arange(n) + 0.25) / n
    return np.stack([c[0] + r * np.cos(t), c[1] + r * np.sin(t)])


def cpu_cases():
    """The point sets of this module's cases, one image each: 0, 1, 2, 3 points, 3 collinear, 50 collinear with copies,
    a 5 x 5 grid, a unit square with its centre three times, 257 on a circle, 2 000 uniform random."""
    rng = np.random.default_rng(11)
    t = np.arange(50.0)
    line = np.stack([100 + 7 * t, 50 + 3.5 * t])
    g = np.arange(5.0) * 30
    grid = np.stack([(200 + g)[:, None] + 0 * g, 300 + g[None, :] + 0 * g[:, None]]).reshape(2, -1)
    sq = np.array([[10.0, 11, 11, 10, 10.5, 10.5, 10.5], [20.0, 20, 21, 21, 20.5, 20.5, 20.5]])
    return [np.zeros((2, 0)), np.array([[5.0], [7.0]]), np.array([[5.0, 9], [7.0, 3]]), np.array([[5.0, 9, 2], [7.0, 3, 1]]),
            np.array([[1.0, 2, 3], [2.0, 4, 6]]), np.concatenate([line, line[:, [0, 49, 20, 20]]], 1)[:, rng.permutation(54)],
            grid[:, rng.permutation(25)], sq, circle(257), np.stack([rng.uniform(0, 2000, 2000), rng.uniform(0, 1500, 2000)])]


def scene_with_points(sets, extra_images=0):
    """An all-see-all synthetic scene thinned so that image i holds len(sets[i]) points, their pixel coordinates
    overwritten by sets[i]; extra_images more images keep every point (with their synthetic coordinates)."""
    from dbat_amd import synth
    nc = len(sets) + extra_images
    npnt = max(max(p.shape[1] for p in sets), 8)
    s, _ = synth.make_dense_scene(nc, npnt, False, 1, 3)
    cam, pt = np.asarray(s.IP.cam), np.asarray(s.IP.pt)
    cnt = np.array([p.shape[1] for p in sets] + [npnt] * extra_images)
    t = thin(s, pt < cnt[cam])
    st = image_columns(t)
    val = np.array(t.IP.val, float, order='F')
    for i, p in enumerate(sets):
        val[:, st[i]:st[i + 1]] = p
    t.IP.val = val
    return t


@pytest.fixture(scope='module')
def cases():
    return scene_with_points(cpu_cases())


def test_host_coverage_matches_the_restatement(cases):
    from dbat_amd import _hip
    got = _hip.debug_coverage_host(cases)
    assert check_coverage(got, cases) == 10
    n = [len(h) for h in got['hull']]
    assert n[:5] == [0, 1, 2, 3, 2] and n[5] == 2 and n[6] == 4 and n[7] == 4 and n[8] == 257
    area = got['hull_area']
    assert np.all(area[:6] == [0, 0, 0, area[3], 0, 0]) and area[3] > 0
    assert area[6] == 16 * 30.0 ** 2 and area[7] == 1.0


def test_host_coverage_of_a_real_project():
    from dbat_amd import _hip
    s = camcal_struct()
    assert check_coverage(_hip.debug_coverage_host(s), s) == s.EO.val.shape[1]


def test_union_from_the_hull_vertices_alone():
    """hull(A u B) = hull(hull A u hull B): the union of driver.network_quality, restated on the host's hulls."""
    from dbat_amd import _hip
    from dbat_amd.driver import _hull_area_of
    s = camcal_struct()
    got = _hip.debug_coverage_host(s)
    cols = np.concatenate(got['hull'])
    uv = np.asarray(s.IP.val, float)
    W, H = uv.max(1) - uv.min(1)
    h, a = _hull_area_of(uv[:, cols])
    assert abs(a - ref_hull(uv)[1]) <= 8 * len(h) * EPS * W * H


def coverage_lines(s):
    """The three lines of the report's "Photo point coverage" block from the restatement (one camera)."""
    uv = np.asarray(s.IP.val, float)
    st = image_columns(s)
    nc = len(st) - 1
    im, px = np.asarray(s.IO.sensor.imSize, float), np.asarray(s.IO.sensor.pxSize, float)

    def corner(i):
        cu, cv = np.array([0.5, 0.5, im[0, i] + 0.5, im[0, i] + 0.5]), np.array([0.5, im[1, i] + 0.5, im[1, i] + 0.5, 0.5])
        return radii(s, i, np.stack([cu, cv])).max()

    def one(pts, i):
        return (ref_hull(pts)[1] / im[:, i].prod(), np.prod(pts.max(1) - pts.min(1)) / im[:, i].prod(), radii(s, i, pts).max() / corner(i))
    c, cr, crr = (np.array(v) for v in zip(*[one(uv[:, st[i]:st[i + 1]], i) for i in range(nc)]))
    uc, ucr, ucrr = one(uv, 0)
    rnd = lambda v: int(np.floor(v * 100 + 0.5))
    fmt = lambda a, u: '%d%%-%d%% (%d%% average, %d%% union)' % (rnd(a.min()), rnd(a.max()), rnd(a.mean()), rnd(u))
    return {'Rectangular:': fmt(cr, ucr), 'Convex hull:': fmt(c, uc), 'Radial:': fmt(crr, ucrr)}


def golden_coverage_lines(name):
    out = {}
    for ln in open(os.path.join(GOLDEN, name)).read().splitlines():
        m = re.match(r'\s*(Rectangular:|Convex hull:|Radial:)\s+(.*\S)\s*$', ln)
        if m:
            out[m.group(1)] = m.group(2)
    assert len(out) == 3
    return out


def golden_values(name, heads):
    """The 'Value:' in mm under each heading of heads in a committed report."""
    lines = open(os.path.join(GOLDEN, name)).read().splitlines()
    out = []
    for h in heads:
        k = next(i for i, ln in enumerate(lines) if ln.strip() == h)
        out.append(float(re.match(r'\s*Value:\s+(\S+) mm\s*$', lines[k + 1]).group(1)))
    return out


@pytest.mark.parametrize('name', ['sxb', 'camcal5'])
def test_restatement_reproduces_the_reference_reports(name):
    if name == 'sxb':
        from helpers import sxb_struct
        s, gold = sxb_struct(), golden_coverage_lines('sxb-report.txt')
    else:
        s, gold = camcal_struct(5), golden_coverage_lines('camcal-dbatreport-model5.txt')
        # the report's radii are taken about the ESTIMATED principal point (sxb's camera is fixed): the report itself
        # prints it to six digits, which whole percents tolerate; py is displayed with its sign reversed
        pp = golden_values('camcal-dbatreport-model5.txt', ('px - principal point x:', 'py - principal point y:'))
        s.IO.val = np.array(s.IO.val, float, order='F')
        s.IO.val[1], s.IO.val[2] = pp[0], -pp[1]
    assert coverage_lines(s) == gold
