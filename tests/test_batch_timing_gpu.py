"""The kernel clocks of the calls that take a device index instead of a handle (dbat_hip_debug_align_ / _relorient_ /
_pairadjust_ / _resect_robust_timing and _ms), on the smallest inputs: with timing on a call leaves more than 0 ms in the
slots of the kernels it launched, exactly 0 in the slots it resets, and the slots it does not own as they were; with
timing off the slot of the kernel just run reads 0.  dbat_hip_resect has no clock and touches none.

Which call owns and resets which slot is taken from the host code as it stood before the clocks became one template:
rigidalign writes [0 .. 2] and zeroes [3], [4]; multixform zeroes all five and writes [3] with points, [4] with cameras;
essmat5 writes [0] and zeroes [1], [2]; relorient writes all three; resect_ransac writes [0] only, poseadjust [1] only."""
import numpy as np
import pytest

from dbat_amd import _hip

pytestmark = pytest.mark.gpu


def rotation(a=0.05, b=-0.03):
    ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(b), np.sin(b)
    return np.array([[ca, 0, sa], [0, 1.0, 0], [-sa, 0, ca]]) @ np.array([[1.0, 0, 0], [0, cb, -sb], [0, sb, cb]])


RNG = np.random.default_rng(4)
R, T = rotation(), np.array([0.995, 0.02, 0.1]) / np.linalg.norm([0.995, 0.02, 0.1])
# one pair of 8 correspondences, in front (+z) of [I | 0] and [R | T], with three samples of five
X8 = np.vstack([RNG.uniform(-1, 1, (2, 8)), RNG.uniform(4, 6, (1, 8))])
X1 = X8[:2] / X8[2]
X2 = (R @ X8 + T[:, None])[:2] / (R @ X8 + T[:, None])[2]
SAMPLES5 = np.array([[0, 1, 2, 3, 4], [3, 4, 5, 6, 7], [0, 2, 4, 6, 7]], np.int32)
P2 = np.hstack([R, T[:, None]])[None]
# one camera of 6 control points, with two triangles / three triples
X6, XN6 = X8[:, :6], X2[:, :6]
TRIPLES = np.array([[0, 1, 2], [1, 2, 3], [3, 4, 5]], np.int32)
# 12 points and 2 cameras for the transforms
X12 = RNG.normal(0, 10, (3, 12))
SIM = np.eye(4)
SIM[:3, :3], SIM[:3, 3] = 1.3 * R, (4.0, -2.0, 1.0)
Y12 = SIM[:3, :3] @ X12 + SIM[:3, 3:4]
EO2 = np.vstack([RNG.normal(0, 5, (3, 2)), RNG.uniform(-1, 1, (3, 2))])

hom = lambda x: np.vstack([x, np.ones((1, x.shape[1]))])

CALLS = dict(
    rigidalign=lambda: _hip.rigidalign(X12, Y12, True, resid=True),
    multixform=lambda: _hip.multixform(EO2, X12, SIM),
    multixform_points=lambda: _hip.multixform(np.zeros((6, 0)), X12, SIM),
    essmat5=lambda: _hip.essmat5_sets([0, 8], hom(X1), hom(X2)),
    relorient=lambda: _hip.relorient_pairs([0, 8], X1, X2, [0, 3], SAMPLES5, 1e-6, 1),
    pairadjust=lambda: _hip.pairadjust([0, 8], X1, X2, P2, X8, front_dir=1),
    resect=lambda: _hip.resect_poses([0, 6], X6, XN6, [0, 2], TRIPLES[:2]),
    resect_ransac=lambda: _hip.resect_ransac([0, 6], X6, XN6, [0, 3], TRIPLES, 1e-6),
    poseadjust=lambda: _hip.poseadjust([0, 6], X6, XN6, P2),
)
CLOCKS = dict(align=(_hip.align_timing, _hip.align_ms), relorient=(_hip.relorient_timing, _hip.relorient_ms),
              pairadjust=(_hip.pairadjust_timing, _hip.pairadjust_ms), resect_robust=(_hip.resect_robust_timing, _hip.resect_robust_ms))


def read_all():
    return {k: ms() for k, (_, ms) in CLOCKS.items()}


@pytest.fixture
def timing():
    """Every clock on for the test, off after it."""
    for on, _ in CLOCKS.values():
        on(True)
    yield
    for on, _ in CLOCKS.values():
        on(False)


def test_align_clock(timing):
    others = {k: v for k, v in read_all().items() if k != 'align'}
    CALLS['rigidalign']()
    a = _hip.align_ms()
    print('rigidalign', a)
    assert a['centroid'] > 0 and a['cross'] > 0 and a['resid'] > 0 and a['points'] == 0 and a['cams'] == 0
    CALLS['multixform']()
    m = _hip.align_ms()
    print('multixform', m)
    assert m['centroid'] == 0 and m['cross'] == 0 and m['resid'] == 0 and m['points'] > 0 and m['cams'] > 0
    CALLS['rigidalign']()                              # ... zeroes what multixform left
    a = _hip.align_ms()
    assert a['centroid'] > 0 and a['cross'] > 0 and a['resid'] > 0 and a['points'] == 0 and a['cams'] == 0
    CALLS['multixform_points']()                       # ... and multixform what it does not launch
    m = _hip.align_ms()
    assert m['centroid'] == 0 and m['cross'] == 0 and m['resid'] == 0 and m['points'] > 0 and m['cams'] == 0
    assert {k: v for k, v in read_all().items() if k != 'align'} == others


def test_relorient_clock(timing):
    others = {k: v for k, v in read_all().items() if k != 'relorient'}
    CALLS['relorient']()
    r = _hip.relorient_ms()
    print('relorient', r)
    assert r['solve'] > 0 and r['score'] > 0 and r['cams'] > 0
    CALLS['essmat5']()                                 # zeroes what relorient left in [1], [2]
    e = _hip.relorient_ms()
    print('essmat5', e)
    assert e['solve'] > 0 and e['score'] == 0 and e['cams'] == 0
    assert {k: v for k, v in read_all().items() if k != 'relorient'} == others


def test_pairadjust_clock(timing):
    others = {k: v for k, v in read_all().items() if k != 'pairadjust'}
    CALLS['pairadjust']()
    p = _hip.pairadjust_ms()
    print('pairadjust', p)
    assert isinstance(p, float) and p > 0
    assert {k: v for k, v in read_all().items() if k != 'pairadjust'} == others


def test_resect_robust_clock(timing):
    others = {k: v for k, v in read_all().items() if k != 'resect_robust'}
    before = _hip.resect_robust_ms()
    CALLS['resect_ransac']()                           # writes [0] only
    a = _hip.resect_robust_ms()
    print('resect_ransac', a)
    assert a['ransac'] > 0 and a['adjust'] == before['adjust']
    CALLS['poseadjust']()                              # writes [1] only
    b = _hip.resect_robust_ms()
    print('poseadjust', b)
    assert b['adjust'] > 0 and b['ransac'] == a['ransac']
    CALLS['resect_ransac']()
    c = _hip.resect_robust_ms()
    assert c['ransac'] > 0 and c['adjust'] == b['adjust']
    CALLS['resect']()                                  # no clock: every slot stays
    assert _hip.resect_robust_ms() == c
    assert {k: v for k, v in read_all().items() if k != 'resect_robust'} == others


def test_timing_off():
    for on, _ in CLOCKS.values():                      # leave something in every slot, then switch the clocks off
        on(True)
    try:
        for k in ('rigidalign', 'relorient', 'pairadjust', 'resect_ransac', 'poseadjust'):
            CALLS[k]()
    finally:
        for on, _ in CLOCKS.values():
            on(False)
    left = _hip.resect_robust_ms()
    assert left['ransac'] > 0 and left['adjust'] > 0
    CALLS['rigidalign']()
    assert _hip.align_ms() == dict(centroid=0, cross=0, resid=0, points=0, cams=0)
    CALLS['multixform']()
    assert _hip.align_ms() == dict(centroid=0, cross=0, resid=0, points=0, cams=0)
    CALLS['relorient']()
    assert _hip.relorient_ms() == dict(solve=0, score=0, cams=0)
    CALLS['essmat5']()
    assert _hip.relorient_ms() == dict(solve=0, score=0, cams=0)
    CALLS['pairadjust']()
    assert _hip.pairadjust_ms() == 0
    CALLS['resect_ransac']()                           # its own slot reads 0, the other one stays
    assert _hip.resect_robust_ms() == dict(ransac=0, adjust=left['adjust'])
    CALLS['poseadjust']()
    assert _hip.resect_robust_ms() == dict(ransac=0, adjust=0)
