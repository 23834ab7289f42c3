"""Every refusal of the eight calls that take a device index instead of a handle (dbat_hip_resect, _rigidalign, _multixform,
_essmat5, _relorient, _pairadjust, _resect_ransac, _poseadjust): return code and dbat_hip_last_error() text of one bad call
per check, and of calls that pass every check, against tests/golden/batch_refusals.json.

The fixture was recorded by generate() below from a library built from the commit before these calls were moved onto
csrc/batch_host.hpp, on a machine without a GPU: there a call that passes every check ends in EDEVICE, and so does
everything dbat_hip_resect checks after its device test.  With a device those rows are skipped -- a row recorded as EINVAL
never is.  To record again (by hand, never during the tests), from the tests directory and without a GPU:
    DBAT_AMD_LIB=/path/to/libdbat_hip.so python -c "import test_batch_refusals_cpu as t; t.generate()"
"""
import ctypes as C
import json
import os

import numpy as np

from dbat_amd import _hip

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'batch_refusals.json')
NAN, INF = float('nan'), float('inf')


def put(a, idx, v):
    b = np.array(a)
    b[idx] = v
    return b


def i64(*v):
    return np.array(v, np.int64)


def i32(*v):
    return np.array(v, np.int32)


# ---- the arguments of one good call per entry point, in the order of the C signature ------------------------------------

def rotation(a=0.3, b=-0.2):
    ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(b), np.sin(b)
    return np.array([[ca, -sa, 0], [sa, ca, 0], [0, 0, 1.0]]) @ np.array([[1.0, 0, 0], [0, cb, -sb], [0, sb, cb]])


RNG = np.random.default_rng(20)
PTS = RNG.normal(0, 1, (3, 16))                       # 3-by-16, flattened column-major: 16 points
IMG = RNG.normal(0, 0.2, (2, 16))
IMG2 = RNG.normal(0, 0.2, (2, 16))
POSE = np.hstack([rotation(), [[0.1], [-0.2], [0.97]]])          # [R | t], column-major below
POSES = np.concatenate([POSE.flatten('F')] * 2)
OPT = (20, 1e-6, 0.0)
col = lambda a: np.ascontiguousarray(a.flatten('F'))

BASE = {
    'resect': dict(device=0, n_images=2, pt_start=i64(0, 8, 16), X=col(PTS), xn=col(IMG), tri_start=i64(0, 1, 2),
                   tri=i32(0, 1, 2, 5, 6, 7), P=np.zeros(24), rms=np.zeros(2)),
    'rigidalign': dict(device=0, n=16, X=col(PTS), Y=col(1.3 * rotation() @ PTS + 4.0), use=None, scale=1, T=np.zeros(16),
                       stats=np.zeros(4), resid=None),
    'multixform': dict(device=0, T=col(np.vstack([np.hstack([1.7 * rotation(), [[1e3], [-2e3], [5e2]]]), [[0, 0, 0, 1.0]]])),
                       n_images=2, eo_rows=6, EO=np.zeros(12), n_points=16, OP=col(PTS), fail=None),
    'essmat5': dict(device=0, n_sets=2, set_start=i64(0, 8, 16), Q1=col(PTS), Q2=col(PTS[::-1]), E=np.zeros(180),
                    n_sol=np.zeros(2, np.int32)),
    'relorient': dict(device=0, n_pairs=2, pt_start=i64(0, 8, 16), x1=col(IMG), x2=col(IMG2), hyp_start=i64(0, 1, 2),
                      samples=i32(0, 1, 2, 3, 4, 3, 4, 5, 6, 7), thr2=np.array([1e-6, 1e-6]), front_dir=1, E=np.zeros(18),
                      P2=np.zeros(24), stats=np.zeros(16, np.int32), inlier=np.zeros(16, np.uint8),
                      in_front=np.zeros(16, np.uint8), X=np.zeros(48)),
    'pairadjust': dict(device=0, n_pairs=2, pt_start=i64(0, 8, 16), x1=col(IMG), x2=col(IMG2), use=None, w1=None, w2=None,
                       front_dir=-1, opt=OPT, P2=POSES, X=col(PTS), used=np.zeros(16, np.uint8), dstat=np.zeros(8),
                       istat=np.zeros(8, np.int32), Q=np.zeros(72), res=None),
    'resect_ransac': dict(device=0, n_images=2, pt_start=i64(0, 8, 16), X=col(PTS), xn=col(IMG), use=None,
                          smp_start=i64(0, 2, 4), smp=i32(0, 1, 2, 2, 3, 4, 4, 5, 6, 5, 6, 7), thr2=np.array([1e-6, 1e-6]),
                          P=np.zeros(24), stats=np.zeros(8, np.int32), inlier=np.zeros(16, np.uint8), ssq=np.zeros(2)),
    'poseadjust': dict(device=0, n_images=2, pt_start=i64(0, 8, 16), X=col(PTS), xn=col(IMG), use=None, w=None, opt=OPT,
                       P=POSES, used=np.zeros(16, np.uint8), dstat=np.zeros(8), istat=np.zeros(8, np.int32), Q=np.zeros(72),
                       res=None),
}

ONES = np.ones(32)                                     # weights, 2-by-16
USE = np.ones(16, np.uint8)
LINE = col(np.outer([1.0, 2.0, -3.0], np.arange(16.0) - 8))
SCALED = put(POSES, slice(12, 21), col(rotation() @ np.diag([1.0, 1.0, 1.0 + 1e-5])))
MIRRORED = put(POSES, slice(0, 9), -POSES[:9])
BIG = 1 << 31


def b(name, key):
    return BASE[name][key]


# ---- the table: (entry point, case, the arguments that differ from the good call) ----------------------------------------
# A case that pins the order of two checks fails both; the comment says which one answers.

CASES = [
    # dbat_hip_resect: only the null arguments come before the device
    ('resect', 'good', {}),
    ('resect', 'no images', dict(n_images=0)),
    ('resect', 'null pt_start', dict(pt_start=None)),
    ('resect', 'null rms', dict(rms=None)),
    ('resect', 'negative count', dict(n_images=-1)),
    ('resect', 'pt_start from 1', dict(pt_start=i64(1, 8, 16))),
    ('resect', 'tri_start from 1', dict(tri_start=i64(1, 1, 2))),
    ('resect', 'pt_start descends', dict(pt_start=i64(0, 9, 8))),
    ('resect', 'tri_start descends', dict(tri_start=i64(0, 2, 1))),
    ('resect', 'null X', dict(X=None)),
    ('resect', 'null tri', dict(tri=None)),
    ('resect', 'index past the camera', dict(tri=i32(0, 1, 8, 5, 6, 7))),
    ('resect', 'negative index', dict(tri=i32(0, 1, 2, 5, -1, 7))),
    # dbat_hip_rigidalign
    ('rigidalign', 'good', {}),
    ('rigidalign', 'good with use', dict(use=put(USE, 5, 0), X=put(b('rigidalign', 'X'), 16, NAN))),
    ('rigidalign', 'null T', dict(T=None)),
    ('rigidalign', 'null stats', dict(stats=None)),
    ('rigidalign', 'null X', dict(X=None)),
    ('rigidalign', 'negative count', dict(n=-1)),
    ('rigidalign', 'X not finite', dict(X=put(b('rigidalign', 'X'), 16, NAN))),
    ('rigidalign', 'Y not finite', dict(Y=put(b('rigidalign', 'Y'), 47, INF))),
    ('rigidalign', 'no columns', dict(n=0)),
    ('rigidalign', 'two columns', dict(n=2)),
    ('rigidalign', 'two used', dict(use=put(np.zeros(16, np.uint8), [1, 7], 1))),
    ('rigidalign', 'collinear X', dict(X=LINE)),
    ('rigidalign', 'collinear Y', dict(Y=LINE + 1e6)),
    ('rigidalign', 'coincident', dict(X=np.ones(48))),
    # dbat_hip_multixform
    ('multixform', 'good', {}),
    ('multixform', 'good seven rows', dict(eo_rows=7, EO=np.zeros(14))),
    ('multixform', 'null T', dict(T=None)),
    ('multixform', 'null EO', dict(EO=None)),
    ('multixform', 'null OP', dict(OP=None)),
    ('multixform', 'negative images', dict(n_images=-1)),
    ('multixform', 'negative points', dict(n_points=-1)),
    ('multixform', 'five rows', dict(eo_rows=5)),
    ('multixform', 'T not finite', dict(T=put(b('multixform', 'T'), 13, NAN))),
    ('multixform', 'last row', dict(T=put(b('multixform', 'T'), 3, 1e-3))),
    ('multixform', 'last entry', dict(T=put(b('multixform', 'T'), 15, 2.0))),
    ('multixform', 'mirror', dict(T=put(b('multixform', 'T'), slice(8, 11), -b('multixform', 'T')[8:11]))),
    ('multixform', 'zero', dict(T=put(b('multixform', 'T'), slice(0, 11), 0.0))),
    ('multixform', 'anisotropic', dict(T=put(b('multixform', 'T'), slice(8, 11), (1 + 1e-6) * b('multixform', 'T')[8:11]))),
    # dbat_hip_essmat5
    ('essmat5', 'good', {}),
    ('essmat5', 'no sets', dict(n_sets=0)),
    ('essmat5', 'null set_start', dict(set_start=None)),
    ('essmat5', 'null E', dict(E=None)),
    ('essmat5', 'null n_sol', dict(n_sol=None)),
    ('essmat5', 'negative count', dict(n_sets=-1)),
    ('essmat5', 'from 1', dict(set_start=i64(1, 8, 16))),
    ('essmat5', 'four in a set', dict(set_start=i64(0, 12, 16))),
    ('essmat5', 'descends', dict(set_start=i64(0, 9, 8))),
    ('essmat5', 'null Q1', dict(Q1=None)),
    ('essmat5', 'null Q2', dict(Q2=None)),
    ('essmat5', 'Q1 not finite', dict(Q1=put(b('essmat5', 'Q1'), 10, NAN))),
    ('essmat5', 'Q2 not finite', dict(Q2=put(b('essmat5', 'Q2'), 47, INF))),
    # dbat_hip_relorient
    ('relorient', 'good', {}),
    ('relorient', 'good given E', dict(hyp_start=None, samples=None, E=np.tile(np.arange(1.0, 10.0), 2))),
    ('relorient', 'no pairs', dict(n_pairs=0)),
    ('relorient', 'null pt_start', dict(pt_start=None)),
    ('relorient', 'null thr2', dict(thr2=None)),
    ('relorient', 'null X', dict(X=None)),
    ('relorient', 'negative count', dict(n_pairs=-1)),
    ('relorient', 'front_dir 0', dict(front_dir=0)),
    ('relorient', 'front_dir 2', dict(front_dir=2)),
    ('relorient', 'pt_start from 1', dict(pt_start=i64(1, 8, 16))),
    ('relorient', 'hyp_start from 1', dict(hyp_start=i64(1, 1, 2))),
    ('relorient', 'four in a pair', dict(pt_start=i64(0, 4, 16))),
    ('relorient', 'pt_start descends', dict(pt_start=i64(0, 17, 16))),
    ('relorient', 'hyp_start descends', dict(hyp_start=i64(0, 3, 2))),
    ('relorient', 'too many samples', dict(hyp_start=i64(0, 100000001, 100000002))),
    ('relorient', 'too many points', dict(pt_start=i64(0, BIG, BIG + 8))),
    ('relorient', 'thr2 zero', dict(thr2=np.array([1e-6, 0.0]))),
    ('relorient', 'thr2 negative', dict(thr2=np.array([-1.0, 1e-6]))),
    ('relorient', 'thr2 not finite', dict(thr2=np.array([INF, 1e-6]))),
    ('relorient', 'thr2 before the next pair', dict(thr2=np.array([NAN, 1e-6]), pt_start=i64(0, 12, 16))),       # thr2
    ('relorient', 'given E not finite', dict(hyp_start=None, samples=None, E=put(np.ones(18), 11, NAN))),
    ('relorient', 'null x1', dict(x1=None)),
    ('relorient', 'null samples', dict(samples=None)),
    ('relorient', 'x1 not finite', dict(x1=put(b('relorient', 'x1'), 14, NAN))),
    ('relorient', 'x2 not finite', dict(x2=put(b('relorient', 'x2'), 5, INF))),
    ('relorient', 'sample past the pair', dict(samples=i32(0, 1, 2, 3, 8, 3, 4, 5, 6, 7))),
    ('relorient', 'negative sample', dict(samples=i32(0, 1, 2, 3, 4, 3, 4, -1, 6, 7))),
    ('relorient', 'sample repeats', dict(samples=i32(0, 1, 2, 3, 4, 3, 4, 5, 6, 4))),
    ('relorient', 'repeats before outside', dict(samples=i32(0, 1, 2, 3, 4, 3, 3, 5, 6, 9))),                   # repeats
    ('relorient', 'outside before repeats', dict(samples=i32(0, 1, 2, 3, 4, 3, 9, 5, 6, 3))),                   # outside
    # dbat_hip_pairadjust
    ('pairadjust', 'good', {}),
    ('pairadjust', 'good with all', dict(use=put(USE, 9, 0), X=put(b('pairadjust', 'X'), 29, NAN), w1=ONES, w2=2 * ONES, res=np.zeros(64))),
    ('pairadjust', 'no pairs', dict(n_pairs=0)),
    ('pairadjust', 'no points', dict(pt_start=i64(0, 0, 0))),
    ('pairadjust', 'null pt_start', dict(pt_start=None)),
    ('pairadjust', 'null opt', dict(opt=None)),
    ('pairadjust', 'null Q', dict(Q=None)),
    ('pairadjust', 'negative count', dict(n_pairs=-1)),
    ('pairadjust', 'front_dir 0', dict(front_dir=0)),
    ('pairadjust', 'max_iter 0', dict(opt=(0, 1e-6, 0.0))),
    ('pairadjust', 'max_iter 201', dict(opt=(201, 1e-6, 0.0))),
    ('pairadjust', 'conv_tol 0', dict(opt=(20, 0.0, 0.0))),
    ('pairadjust', 'conv_tol not finite', dict(opt=(20, NAN, 0.0))),
    ('pairadjust', 'conv_tol infinite', dict(opt=(20, INF, 0.0))),
    ('pairadjust', 'min_angle negative', dict(opt=(20, 1e-6, -1e-3))),
    ('pairadjust', 'min_angle pi/2', dict(opt=(20, 1e-6, np.pi / 2))),
    ('pairadjust', 'min_angle not finite', dict(opt=(20, 1e-6, NAN))),
    ('pairadjust', 'front_dir before max_iter', dict(front_dir=0, opt=(0, 1e-6, 0.0))),                        # front_dir
    ('pairadjust', 'from 1', dict(pt_start=i64(1, 8, 16))),
    ('pairadjust', 'descends', dict(pt_start=i64(0, 9, 8))),
    ('pairadjust', 'null x1', dict(x1=None)),
    ('pairadjust', 'null used', dict(used=None)),
    ('pairadjust', 'x1 not finite', dict(x1=put(b('pairadjust', 'x1'), 6, NAN))),
    ('pairadjust', 'x2 not finite', dict(x2=put(b('pairadjust', 'x2'), 23, INF))),
    ('pairadjust', 'w1 not finite', dict(w1=put(ONES, 5, NAN))),
    ('pairadjust', 'w2 zero', dict(w2=put(ONES, 31, 0.0))),
    ('pairadjust', 'w1 negative', dict(w1=put(ONES, 0, -1.0))),
    ('pairadjust', 'weight before a later x1', dict(w2=put(ONES, 4, 0.0), x1=put(b('pairadjust', 'x1'), 10, NAN))),     # weight of 2
    ('pairadjust', 'x2 before its weight', dict(w1=put(ONES, 4, 0.0), x2=put(b('pairadjust', 'x2'), 4, NAN))),          # correspondence 2
    ('pairadjust', 'X not finite', dict(X=put(b('pairadjust', 'X'), 29, NAN))),
    ('pairadjust', 'P2 not finite', dict(P2=put(POSES, 23, INF))),
    ('pairadjust', 'R scaled', dict(P2=SCALED)),
    ('pairadjust', 'R mirrored', dict(P2=MIRRORED)),
    ('pairadjust', 't zero', dict(P2=put(POSES, slice(21, 24), 0.0))),
    ('pairadjust', 't zero before the next R', dict(P2=put(SCALED, slice(9, 12), 0.0))),                        # t of pair 0
    # dbat_hip_resect_ransac
    ('resect_ransac', 'good', {}),
    ('resect_ransac', 'good with use', dict(use=put(USE, 9, 0), X=put(b('resect_ransac', 'X'), 28, NAN))),
    ('resect_ransac', 'no images', dict(n_images=0)),
    ('resect_ransac', 'null pt_start', dict(pt_start=None)),
    ('resect_ransac', 'null smp_start', dict(smp_start=None)),
    ('resect_ransac', 'null thr2', dict(thr2=None)),
    ('resect_ransac', 'negative count', dict(n_images=-1)),
    ('resect_ransac', 'pt_start from 1', dict(pt_start=i64(1, 8, 16))),
    ('resect_ransac', 'pt_start descends', dict(pt_start=i64(0, 9, 8))),
    ('resect_ransac', 'too many points', dict(pt_start=i64(0, 1 << 29, (1 << 29) + 8))),
    ('resect_ransac', 'null X', dict(X=None)),
    ('resect_ransac', 'null xn', dict(xn=None)),
    ('resect_ransac', 'X not finite', dict(X=put(b('resect_ransac', 'X'), 28, NAN))),
    ('resect_ransac', 'xn not finite', dict(xn=put(b('resect_ransac', 'xn'), 1, INF))),
    ('resect_ransac', 'null inlier', dict(inlier=None)),
    ('resect_ransac', 'smp_start from 1', dict(smp_start=i64(1, 2, 4))),
    ('resect_ransac', 'smp_start descends', dict(smp_start=i64(0, 5, 4))),
    ('resect_ransac', 'too many samples', dict(smp_start=i64(0, BIG, BIG + 2))),
    ('resect_ransac', 'thr2 zero', dict(thr2=np.array([1e-6, 0.0]))),
    ('resect_ransac', 'thr2 not finite', dict(thr2=np.array([NAN, 1e-6]))),
    ('resect_ransac', 'thr2 before the next camera', dict(thr2=np.array([-1.0, 1e-6]), smp_start=i64(0, 5, 4))),         # thr2 of camera 0
    ('resect_ransac', 'null smp', dict(smp=None)),
    ('resect_ransac', 'sample past the camera', dict(smp=put(b('resect_ransac', 'smp'), 5, 8))),
    ('resect_ransac', 'negative sample', dict(smp=put(b('resect_ransac', 'smp'), 7, -1))),
    ('resect_ransac', 'sample repeats', dict(smp=put(b('resect_ransac', 'smp'), 11, 5))),
    ('resect_ransac', 'outside although it repeats first', dict(smp=put(b('resect_ransac', 'smp'), slice(3, 6), (2, 2, 9)))),   # outside
    # dbat_hip_poseadjust
    ('poseadjust', 'good', {}),
    ('poseadjust', 'good with all', dict(use=put(USE, 9, 0), X=put(b('poseadjust', 'X'), 28, NAN), w=ONES, res=np.zeros(32))),
    ('poseadjust', 'no images', dict(n_images=0)),
    ('poseadjust', 'no points', dict(pt_start=i64(0, 0, 0))),
    ('poseadjust', 'null pt_start', dict(pt_start=None)),
    ('poseadjust', 'null opt', dict(opt=None)),
    ('poseadjust', 'null dstat', dict(dstat=None)),
    ('poseadjust', 'negative count', dict(n_images=-1)),
    ('poseadjust', 'max_iter 0', dict(opt=(0, 1e-6, 0.0))),
    ('poseadjust', 'max_iter 201', dict(opt=(201, 1e-6, 0.0))),
    ('poseadjust', 'conv_tol negative', dict(opt=(20, -1e-6, 0.0))),
    ('poseadjust', 'conv_tol not finite', dict(opt=(20, NAN, 0.0))),
    ('poseadjust', 'min_angle set', dict(opt=(20, 1e-6, 1e-3))),
    ('poseadjust', 'min_angle not finite', dict(opt=(20, 1e-6, NAN))),
    ('poseadjust', 'from 1', dict(pt_start=i64(1, 8, 16))),
    ('poseadjust', 'descends', dict(pt_start=i64(0, 9, 8))),
    ('poseadjust', 'too many points', dict(pt_start=i64(0, 8, 8 + (1 << 29)))),
    ('poseadjust', 'too many before it descends', dict(pt_start=i64(0, 1 << 29, 8))),                              # too many, camera 0
    ('poseadjust', 'null X', dict(X=None)),
    ('poseadjust', 'X not finite', dict(X=put(b('poseadjust', 'X'), 28, INF))),
    ('poseadjust', 'xn not finite', dict(xn=put(b('poseadjust', 'xn'), 31, NAN))),
    ('poseadjust', 'null used', dict(used=None)),
    ('poseadjust', 'w not finite', dict(w=put(ONES, 5, INF))),
    ('poseadjust', 'w zero', dict(w=put(ONES, 30, 0.0))),
    ('poseadjust', 'P not finite', dict(P=put(POSES, 4, NAN))),
    ('poseadjust', 'R scaled', dict(P=SCALED)),
    ('poseadjust', 'R mirrored', dict(P=MIRRORED)),
]


def run_case(entry, diff):
    """(return code, last error) of the entry point with the good arguments, diff applied."""
    lib = _hip.load()
    fn = getattr(lib, 'dbat_hip_' + entry)
    args = {**BASE[entry], **diff}
    assert list(args) == list(BASE[entry]), 'unknown argument in %s' % sorted(diff)
    keep, cargs = [], []
    for v, t in zip(args.values(), fn.argtypes):
        if isinstance(v, np.ndarray):
            keep.append(np.ascontiguousarray(v).copy())           # the library may write: every call gets its own
            v = keep[-1].ctypes.data_as(t)
        elif isinstance(v, tuple):
            keep.append(_hip.PairOptions(*v))
            v = C.byref(keep[-1])
        cargs.append(v)
    rc = fn(*cargs)
    return int(rc), (_hip.last_error() if rc != 0 else '')


def case_id(entry, name):
    return '%s: %s' % (entry, name)


def generate():
    """Record the fixture from the library dbat_amd._hip loads (DBAT_AMD_LIB: one built from the parent commit), on a
    machine without a GPU.  Run by hand."""
    import torch
    assert not torch.cuda.is_available(), 'record without a GPU: what passes every check is recorded as EDEVICE'
    out = {case_id(e, n): list(run_case(e, d)) for e, n, d in CASES}
    with open(FIXTURE, 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write('\n')
    print('%d cases from %s: %d EINVAL, %d EDEVICE' % (len(out), _hip.LIB_PATH, sum(v[0] == _hip.EINVAL for v in out.values()),
                                                      sum(v[0] == _hip.EDEVICE for v in out.values())))


def test_table_is_the_fixture():
    want = json.load(open(FIXTURE))
    ids = [case_id(e, n) for e, n, _ in CASES]
    assert len(set(ids)) == len(ids) and set(ids) == set(want)
    assert all(rc in (_hip.EINVAL, _hip.EDEVICE) for rc, _ in want.values())
    for e in BASE:                                        # every entry point: a call that passes, and refusals
        assert want[case_id(e, 'good')][0] == _hip.EDEVICE, e
        assert sum(k.startswith(e + ': ') and v[0] == _hip.EINVAL for k, v in want.items()) >= 3, e
    # everything dbat_hip_resect checks after its device test was recorded as what a machine without a device answers
    assert [want[case_id('resect', n)][0] for n in ('pt_start from 1', 'tri_start descends', 'index past the camera')] == [_hip.EDEVICE] * 3


def test_every_refusal():
    import torch
    have_gpu = torch.cuda.is_available()
    want = json.load(open(FIXTURE))
    wrong, checked = [], 0
    for entry, name, diff in CASES:
        rc, text = want[case_id(entry, name)]
        if have_gpu and rc == _hip.EDEVICE:               # with a device these go on to run: the GPU tests' business
            continue
        got = run_case(entry, diff)
        checked += 1
        if got != (rc, text):
            wrong.append((case_id(entry, name), got, (rc, text)))
    assert not wrong, wrong
    assert checked >= sum(v[0] == _hip.EINVAL for v in want.values())
