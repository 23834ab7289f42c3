"""ctypes binding of the C ABI in include/dbat_hip.h (libdbat_hip.so).

The library is the product: there is no Python or CPU fallback.  If the shared
object is missing or cannot be loaded, importing callers get a loud
`DbatHipUnavailable` with the build command.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libdbat_hip.so')
# measurement only (bench/ tools): DBAT_AMD_LIB=prof loads libdbat_hip_prof.so, the same sources built with
# -DDBAT_HIP_PROFILING (make -C dbat_amd/csrc prof) -- the only build that reads DBAT_HIP_ABLATE, _DF_TRACE, ...
if os.environ.get('DBAT_AMD_LIB') == 'prof':
    LIB_PATH = os.path.join(_HERE, 'libdbat_hip_prof.so')
elif os.environ.get('DBAT_AMD_LIB', '').endswith('.so'):          # (a development build to compare with)
    LIB_PATH = os.environ['DBAT_AMD_LIB']
if LIB_PATH != os.path.join(_HERE, 'libdbat_hip.so'):
    # never silently: a stale development build must not stand in for the product library in a test or bench run
    sys.stderr.write('[dbat_amd] DBAT_AMD_LIB: loading %s instead of the product library\n' % LIB_PATH)

ABI_VERSION = 5
DAMP = {'none': 0, 'gm': 0, 'gna': 1, 'lm': 2, 'lmp': 3}

OK, EINVAL, EUNSUPPORTED, EDEVICE, ENOMEM = 0, -101, -102, -103, -104


class DbatHipUnavailable(RuntimeError):
    pass


class DbatHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('dbat_hip error %d: %s' % (code, msg))
        self.code = code


_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lp = C.POINTER(C.c_int64)
_bp = C.POINTER(C.c_uint8)


class Problem(C.Structure):
    _fields_ = [
        ('abi_version', C.c_int32), ('n_images', C.c_int32), ('n_points', C.c_int32),
        ('n_obs', C.c_int64), ('dist_model', C.c_int32), ('nK', C.c_int32), ('nP', C.c_int32),
        ('ip_cam', _ip), ('ip_pt', _ip), ('ip_val', _dp), ('ip_std', _dp),
        ('IO_val', _dp), ('px_size', _dp), ('EO_val', _dp), ('OP_val', _dp),
        ('est_IO', _bp), ('est_EO', _bp), ('est_OP', _bp),
        ('IO_block', _ip), ('EO_block', _ip),
        ('prior_IO_use', _bp), ('prior_IO_val', _dp), ('prior_IO_std', _dp),
        ('prior_EO_use', _bp), ('prior_EO_val', _dp), ('prior_EO_std', _dp),
        ('prior_OP_use', _bp), ('prior_OP_val', _dp), ('prior_OP_std', _dp),
        ('device', C.c_int32), ('shard_rank', C.c_int32), ('shard_count', C.c_int32),
    ]


class Options(C.Structure):
    _fields_ = [
        ('damping', C.c_int32), ('max_iter', C.c_int32), ('conv_tol', C.c_double),
        ('abs_term', C.c_int32), ('singular_test', C.c_int32), ('store_trace', C.c_int32),
        ('mu', C.c_double), ('alpha_min', C.c_double), ('lambda0', C.c_double),
        ('lambda_min', C.c_double), ('rho_bad', C.c_double), ('rho_good', C.c_double),
        ('delta0', C.c_double),
        ('term_fun', C.c_void_p), ('term_user', C.c_void_p), ('veto_fun', C.c_void_p), ('veto_user', C.c_void_p),
        ('trace_fun', C.c_void_p), ('trace_user', C.c_void_p),
    ]


TERM_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, _dp, _dp, C.c_int64)   # dbat_hip_term_fn
VETO_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, _dp, C.c_int64)        # dbat_hip_veto_fn
TRACE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_double)   # dbat_hip_trace_fn


def trace_text(damping, n, res, damp, step, rho):
    """The line the reference's lsa solver prints with 'trace' (gauss_newton_armijo.m:119-128, gauss_markov.m:74-76,
    levenberg_marquardt.m:138-147, levenberg_marquardt_powell.m:160-164), from the arguments of a dbat_hip_trace_fn."""
    from fractions import Fraction
    if damping == DAMP['gna']:
        if damp != damp:
            return 'Gauss-Newton-Armijo: iteration %d, residual norm=%.2g' % (n, res)
        return 'Gauss-Newton-Armijo: iteration %d, residual norm=%.2g, last alpha=%s' % (n, res, Fraction(damp).limit_denominator(1 << 40))   # strtrim(rats(alpha)): alpha = 2^-k
    if damping == DAMP['lm']:
        if damp != damp:
            return 'Levenberg-Marquardt: iteration %d, residual norm=%.2g' % (n, res)
        return 'Levenberg-Marquardt: iteration %d, residual norm=%.2g, lambda=%.2g' % (n, res, damp)
    if damping == DAMP['lmp']:
        return 'Levenberg-Marquardt-Powell: iteration %d, residual norm=%.2g, delta=%.2g, step=%s, rho=%.1f' % (
            n, res, damp, ('GN', 'IP', 'CP')[step] if 0 <= step < 3 else '?', rho)
    return 'Gauss-Markov: iteration %d, residual norm=%.2g' % (n, res)


class Result(C.Structure):
    _fields_ = [
        ('code', C.c_int32), ('iters', C.c_int32), ('n_res', C.c_int32), ('n_damp', C.c_int32),
        ('n_trace', C.c_int32), ('sigma0', C.c_double), ('time_s', C.c_double),
        ('n_residual_evals', C.c_int32), ('n_linearizations', C.c_int32), ('n_solves', C.c_int32),
        ('n_trace_only', C.c_int32), ('stage_s', C.c_double * 5),
    ]


LOSS = {'huber': 0, 'cauchy': 1}
SCALE = {'apriori': 0, 'mad': 1}
ROBUST_MAX_OUTER = 64          # DBAT_HIP_ROBUST_MAX_OUTER


class RobustOptions(C.Structure):
    _fields_ = [
        ('loss', C.c_int32), ('k', C.c_double), ('scale', C.c_int32), ('max_outer', C.c_int32),
        ('weight_tol', C.c_double),
    ]


class PairOptions(C.Structure):           # dbat_hip_pair_options
    _fields_ = [('max_iter', C.c_int32), ('conv_tol', C.c_double), ('min_angle', C.c_double)]


class RobustResult(C.Structure):
    _fields_ = [
        ('outer', C.c_int32), ('converged', C.c_int32), ('inner_iters', C.c_int32 * ROBUST_MAX_OUTER),
        ('scale', C.c_double * ROBUST_MAX_OUTER), ('max_change', C.c_double), ('reweight_s', C.c_double),
    ]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)

# every symbol include/dbat_hip.h declares: name -> (restype, argtypes)
class DepthStats(C.Structure):            # dbat_hip_depth_stats
    _fields_ = [('n_behind', C.c_int64), ('min_depth', C.c_double), ('argmin_column', C.c_int64)]


class VetoStats(C.Structure):             # dbat_hip_veto_stats
    _fields_ = [('tested', C.c_int64), ('rejected', C.c_int64), ('n_behind', C.c_int64), ('min_depth', C.c_double)]


_H = C.c_void_p
SYMBOLS = {
    'dbat_hip_last_error': (C.c_char_p, []),
    'dbat_hip_abi_version': (C.c_int, []),
    'dbat_hip_default_options': (C.c_int, [C.c_int32, C.POINTER(Options)]),
    'dbat_hip_plan': (C.c_int, [C.POINTER(Problem)] + [C.POINTER(C.c_int64)] * 7),
    'dbat_hip_plan_structural_rank_ok': (C.c_int, [C.POINTER(Problem), C.POINTER(C.c_int32)]),
    'dbat_hip_plan_point_owner': (C.c_int, [C.POINTER(Problem), _ip]),
    'dbat_hip_plan_serialize': (C.c_int, [C.POINTER(Problem), _dp]),
    'dbat_hip_plan_layout_stats': (C.c_int, [C.POINTER(Problem), C.POINTER(C.c_int64)]),
    'dbat_hip_plan_domain_map': (C.c_int, [C.POINTER(Problem), _ip, C.POINTER(C.c_int32)]),
    'dbat_hip_create': (C.c_int, [C.POINTER(Problem), C.POINTER(_H)]),
    'dbat_hip_destroy': (None, [_H]),
    'dbat_hip_num_params': (C.c_int64, [_H]),
    'dbat_hip_num_residuals': (C.c_int64, [_H]),
    'dbat_hip_serialize': (C.c_int, [_H, _dp]),
    'dbat_hip_deserialize': (C.c_int, [_H, _dp, _dp, _dp, _dp]),
    'dbat_hip_structural_rank_ok': (C.c_int, [_H, C.POINTER(C.c_int32)]),
    'dbat_hip_residual': (C.c_int, [_H, _dp, _dp, _dp]),
    'dbat_hip_jacobian_blocks': (C.c_int, [_H, _dp, _dp, _dp, _dp]),
    'dbat_hip_jacobian_sample': (C.c_int, [_H, _dp, C.c_int64, C.POINTER(C.c_int64), _dp, _dp, _dp, _dp]),
    'dbat_hip_linearize_solve': (C.c_int, [_H, _dp, C.c_double, C.c_int32, _dp, _dp]),
    'dbat_hip_jacobian_csc': (C.c_int, [_H, _dp, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), _dp]),
    'dbat_hip_gradient': (C.c_int, [_H, _dp]),
    'dbat_hip_colnorms': (C.c_int, [_H, _dp]),
    'dbat_hip_jtimes_sqnorm': (C.c_int, [_H, _dp, _dp]),
    'dbat_hip_jtimes': (C.c_int, [_H, _dp, _dp]),
    'dbat_hip_solve': (C.c_int, [_H, C.POINTER(Options), _dp, C.POINTER(Result), _dp, _dp, _dp, _dp]),
    'dbat_hip_final_residuals': (C.c_int, [_H, _dp, _dp]),
    'dbat_hip_comm_unique_id': (C.c_int, [_bp]),
    'dbat_hip_comm_init': (C.c_int, [_H, _bp]),
    'dbat_hip_comm_allreduce_host': (C.c_int, [_H, _dp, C.c_int64, C.c_int32]),
    'dbat_hip_set_deterministic': (C.c_int, [_H, C.c_int32]),
    'dbat_hip_set_allreduce': (C.c_int, [_H, ALLREDUCE_FN, C.c_void_p]),
    'dbat_hip_owned_mask': (C.c_int, [_H, _bp]),
    'dbat_hip_forwintersect': (C.c_int, [_H, _dp, _bp, _dp]),
    'dbat_hip_resect': (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int64), _dp, _dp, C.POINTER(C.c_int64), _ip, _dp, _dp]),
    'dbat_hip_rigidalign': (C.c_int, [C.c_int32, C.c_int64, _dp, _dp, _bp, C.c_int32, _dp, _dp, _dp]),
    'dbat_hip_multixform': (C.c_int, [C.c_int32, _dp, C.c_int64, C.c_int32, _dp, C.c_int64, _dp, _bp]),
    'dbat_hip_essmat5': (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int64), _dp, _dp, _dp, _ip]),
    'dbat_hip_relorient': (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int64), _dp, _dp, C.POINTER(C.c_int64), _ip, _dp,
                                     C.c_int32, _dp, _dp, _ip, _bp, _bp, _dp]),
    'dbat_hip_default_pair_options': (C.c_int, [C.POINTER(PairOptions)]),
    'dbat_hip_pairadjust': (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int64), _dp, _dp, _bp, _dp, _dp, C.c_int32,
                                      C.POINTER(PairOptions), _dp, _dp, _bp, _dp, _ip, _dp, _dp]),
    'dbat_hip_resect_ransac': (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int64), _dp, _dp, _bp, C.POINTER(C.c_int64), _ip, _dp,
                                         _dp, _ip, _bp, _dp]),
    'dbat_hip_poseadjust': (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int64), _dp, _dp, _bp, _dp, C.POINTER(PairOptions), _dp,
                                      _bp, _dp, _ip, _dp, _dp]),
    'dbat_hip_intersect_ransac': (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int64), _ip, _dp, C.c_int32, _dp, _bp,
                                            C.POINTER(C.c_int64), _ip, _dp, C.c_double, _dp, _ip, _bp, _dp]),
    'dbat_hip_pointadjust': (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int64), _ip, _dp, C.c_int32, _dp, _bp, _dp,
                                       C.POINTER(PairOptions), _dp, _bp, _dp, _ip, _dp, _dp]),
    'dbat_hip_bench_step': (C.c_int, [_H, C.c_double, C.c_int32, _dp]),
    'dbat_hip_structure_key': (C.c_int, [C.POINTER(Problem), C.POINTER(C.c_uint64)]),
    'dbat_hip_handle_key': (C.c_int, [_H, C.POINTER(C.c_uint64)]),
    'dbat_hip_set_values': (C.c_int, [_H, C.POINTER(Problem)]),
    'dbat_hip_set_x': (C.c_int, [_H, _dp]),
    'dbat_hip_info': (C.c_int, [_H, C.POINTER(C.c_int64)]),
    'dbat_hip_build_kernel_name': (C.c_int, [_H, C.c_char_p, C.c_int32]),
    'dbat_hip_chol_stats': (C.c_int, [_H, C.POINTER(C.c_int64)]),
    'dbat_hip_posterior_cov': (C.c_int, [_H, _dp, C.c_double, _dp, _dp, _dp, _dp]),
    'dbat_hip_redundancy': (C.c_int, [_H, _dp, _dp, _dp]),
    'dbat_hip_ray_angles': (C.c_int, [_H, _dp, _dp, _dp, _ip, _ip]),
    'dbat_hip_debug_ray_angles_host': (C.c_int, [C.POINTER(Problem), _dp, _dp]),
    'dbat_hip_point_depths': (C.c_int, [_H, _dp, C.c_double, _dp, _dp, C.POINTER(DepthStats)]),
    'dbat_hip_set_chirality': (C.c_int, [_H, C.c_int32, C.c_double]),
    'dbat_hip_chirality_stats': (C.c_int, [_H, C.POINTER(VetoStats)]),
    'dbat_hip_coverage': (C.c_int, [_H, _dp, _dp, _dp, _lp, _dp, _lp, _lp]),
    'dbat_hip_residual_stats': (C.c_int, [_H, _dp, _lp, _dp, _lp, _dp, _dp, _dp, _lp]),
    'dbat_hip_quality_hull_cap': (C.c_int32, []),
    'dbat_hip_debug_coverage_host': (C.c_int, [C.POINTER(Problem), _dp, _dp, _dp, _lp, _dp, _lp, _lp]),
    'dbat_hip_debug_df_schedule': (C.c_int, [C.POINTER(Problem), _lp, _dp, _ip, C.c_int64, _ip, C.c_int64,
                                             C.POINTER(C.c_uint64), C.c_int64]),
    'dbat_hip_default_robust_options': (C.c_int, [C.c_int32, C.POINTER(RobustOptions)]),
    'dbat_hip_robust_weights': (C.c_int, [_H, _dp, C.POINTER(RobustOptions), _dp, _dp, _dp]),
    'dbat_hip_set_obs_weights': (C.c_int, [_H, _dp]),
    'dbat_hip_solve_robust': (C.c_int, [_H, C.POINTER(Options), C.POINTER(RobustOptions), _dp, C.POINTER(Result),
                                        _dp, _dp, _dp, _dp, C.POINTER(RobustResult), _dp]),
    'dbat_hip_debug_robust_from_s': (C.c_int, [_H, _dp, C.POINTER(RobustOptions), _dp, _dp, _dp, _dp, _bp]),
}
DEBUG_SYMBOLS = {
    'dbat_hip_debug_plan_digest': (C.c_int, [C.POINTER(Problem), C.POINTER(C.c_uint64), C.c_int32, C.c_char_p, C.c_int32]),
    'dbat_hip_debug_heavy_plan_selftest': (C.c_int, [C.POINTER(Problem), _dp]),
    'dbat_hip_debug_batch_stats': (C.c_int, [C.POINTER(Problem), C.POINTER(C.c_int64)]),
    'dbat_hip_debug_nd_stats': (C.c_int, [C.POINTER(Problem), C.c_int32, _dp]),
    'dbat_hip_debug_model_eval_host': (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _dp, _dp, C.c_double,
                                                 _dp, _dp, _dp, _dp, _dp, _dp]),
    'dbat_hip_debug_ray_angles_ms': (C.c_int, [_H, _dp, C.POINTER(C.c_int64)]),
    'dbat_hip_debug_quality_ms': (C.c_int, [_H, _dp]),
    'dbat_hip_debug_point_depths_ms': (C.c_int, [_H, _dp]),
    'dbat_hip_debug_chirality_pass_ms': (C.c_int, [_H, _dp, C.c_int32, _dp]),
    'dbat_hip_debug_align_ms': (C.c_int, [_dp]),
    'dbat_hip_debug_align_timing': (C.c_int, [C.c_int32]),
    'dbat_hip_debug_relorient_ms': (C.c_int, [_dp]),
    'dbat_hip_debug_relorient_timing': (C.c_int, [C.c_int32]),
    'dbat_hip_debug_pairadjust_ms': (C.c_int, [_dp]),
    'dbat_hip_debug_pairadjust_timing': (C.c_int, [C.c_int32]),
    'dbat_hip_debug_resect_robust_ms': (C.c_int, [_dp]),
    'dbat_hip_debug_resect_robust_timing': (C.c_int, [C.c_int32]),
    'dbat_hip_debug_intersect_robust_ms': (C.c_int, [_dp]),
    'dbat_hip_debug_intersect_robust_timing': (C.c_int, [C.c_int32]),
}

_lib = None


def load():
    """Load libdbat_hip.so and bind every declared symbol (fails loudly)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DbatHipUnavailable(
            '%s not built: run `python -c "import __graft_entry__ as g; g.build()"` or '
            '`make -C dbat_amd/csrc` (needs hipcc).  There is no CPU fallback.' % LIB_PATH)
    try:
        # PyTorch-ROCm ships its own HIP runtime; when this library (linked against /opt/rocm) is
        # loaded first and torch afterwards, the second runtime finds no device.  Load order
        # torch -> libdbat_hip works, so make it the order always.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        lib = C.CDLL(LIB_PATH)
    except OSError as e:
        raise DbatHipUnavailable('cannot load %s: %s' % (LIB_PATH, e)) from e
    for name, (res, args) in {**SYMBOLS, **DEBUG_SYMBOLS}.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise DbatHipUnavailable('%s does not export %s' % (LIB_PATH, name)) from e
        fn.restype = res
        fn.argtypes = args
    if lib.dbat_hip_abi_version() != ABI_VERSION:
        raise DbatHipUnavailable('ABI version mismatch')
    _lib = lib
    return lib


UNIQUE_ID_BYTES = 128


def comm_unique_id():
    """A fresh RCCL unique id (rank 0 creates it and hands it to the other ranks)."""
    buf = (C.c_uint8 * UNIQUE_ID_BYTES)()
    check(load().dbat_hip_comm_unique_id(buf))
    return bytes(buf)


def last_error():
    return load().dbat_hip_last_error().decode('utf-8', 'replace')


def check(rc):
    if rc != 0:
        raise DbatHipError(rc, last_error())


def dptr(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def _flat(a, dtype):
    """a as a flat column-major array of dtype -- WITHOUT a copy when it already is one (a Fortran-ordered or
    one-dimensional array of that type: what dbat_amd.dbatstruct builds), so that marshalling a 10 M observation struct
    for a cached handle costs microseconds, not a pass over 500 MB."""
    a = np.asarray(a)
    if a.dtype != dtype:
        a = a.astype(dtype)
    if a.ndim <= 1:
        return np.ascontiguousarray(a)
    if a.flags.f_contiguous:
        return a.reshape(-1, order='F')
    return a.flatten('F')


def _f64(a):
    return _flat(a, np.float64)


def _u8(a):
    a = np.asarray(a)
    if a.dtype != np.bool_:
        a = a.astype(bool)
    return _flat(a, np.bool_).view(np.uint8)


def _i32(a):
    return _flat(a, np.int32)


def problem_from_struct(s, device=0, shard_rank=0, shard_count=1):
    """Flatten a DBAT struct (dbat_amd.dbatstruct) into a `Problem`.

    Returns (Problem, keepalive) -- keepalive holds the numpy buffers the
    pointers refer to.
    """
    nc, npnt, no = s.EO.val.shape[1], s.OP.val.shape[1], s.IP.val.shape[1]
    dm = np.unique(s.IO.model.distModel)
    if dm.size != 1:
        raise ValueError('Mixed lens distortion models not implemented.')   # brown_euler_cam4.m:31-33
    model = int(dm[0])
    if model == 1:
        # legacy model 1 = the model that model 2 replicates (bundle.m:49-51); the library
        # implements 2..5, so a model-1 project runs as model 2
        if np.any(np.asarray(s.IO.val)[3:5] != 0) or np.any(np.asarray(s.bundle.est.IO)[3:5]):
            raise ValueError('lens distortion model 1 has no aspect/skew')
        model = 2
    if npnt >= 2 ** 31 or nc >= 2 ** 31:
        raise ValueError('too many points/images for int32 indices')
    keep = dict(
        ip_cam=_i32(s.IP.cam), ip_pt=_i32(s.IP.pt), ip_val=_f64(s.IP.val), ip_std=_f64(s.IP.std),
        IO_val=_f64(s.IO.val), px_size=_f64(s.IO.sensor.pxSize), EO_val=_f64(s.EO.val[:6]),
        OP_val=_f64(s.OP.val),
        est_IO=_u8(s.bundle.est.IO), est_EO=_u8(s.bundle.est.EO[:6]), est_OP=_u8(s.bundle.est.OP),
        IO_block=_i32(s.IO.struct.block), EO_block=_i32(s.EO.struct.block[:6]),
    )
    for nm in ('IO', 'EO', 'OP'):
        pr = getattr(s.prior, nm)
        rows = slice(0, 6) if nm == 'EO' else slice(None)
        use = np.asarray(pr.use)[rows]
        keep['prior_%s_use' % nm] = _u8(use)
        if use.any():
            keep['prior_%s_val' % nm] = _f64(np.nan_to_num(np.asarray(pr.val, float)[rows]))
            keep['prior_%s_std' % nm] = _f64(np.nan_to_num(np.asarray(pr.std, float)[rows], nan=1.0))
        else:                   # (the library reads value and standard deviation only where `use` is set: no pass over the arrays)
            keep['prior_%s_val' % nm] = _f64(np.asarray(pr.val, float)[rows])
            keep['prior_%s_std' % nm] = _f64(np.asarray(pr.std, float)[rows])
    p = Problem()
    p.abi_version = ABI_VERSION
    p.n_images, p.n_points, p.n_obs = nc, npnt, no
    p.dist_model, p.nK, p.nP = model, int(s.IO.model.nK), int(s.IO.model.nP)
    for k, v in keep.items():
        ptr_t = dict(Problem._fields_)[k]
        setattr(p, k, v.ctypes.data_as(ptr_t))
    p.device, p.shard_rank, p.shard_count = int(device), int(shard_rank), int(shard_count)
    return p, keep


class Handle:
    """RAII wrapper of dbat_hip_handle."""

    def __init__(self, s, device=0, shard_rank=0, shard_count=1, _problem=None):
        self.lib = load()
        self.prob, self._keep = _problem if _problem is not None else problem_from_struct(s, device, shard_rank, shard_count)
        h = _H()
        check(self.lib.dbat_hip_create(C.byref(self.prob), C.byref(h)))
        self.h = h
        self.n = int(self.lib.dbat_hip_num_params(h))
        self.m = int(self.lib.dbat_hip_num_residuals(h))
        self._cb = None

    def close(self):
        if getattr(self, 'h', None):
            self.lib.dbat_hip_destroy(self.h)
            self.h = None

    __del__ = close

    def key(self):
        """The structure key of the problem this handle was created from (dbat_hip_handle_key)."""
        k = (C.c_uint64 * 2)()
        check(self.lib.dbat_hip_handle_key(self.h, k))
        return (int(k[0]), int(k[1]))

    def set_values(self, s=None, _problem=None):
        """New IO / EO / OP values and prior observations of a struct with the same structure (dbat_hip_set_values);
        DbatHipError if the structure differs."""
        prob, keep = _problem if _problem is not None else problem_from_struct(
            s, self.prob.device, self.prob.shard_rank, self.prob.shard_count)
        check(self.lib.dbat_hip_set_values(self.h, C.byref(prob)))
        self.prob, self._keep = prob, keep

    def serialize(self):
        x = np.empty(self.n)
        check(self.lib.dbat_hip_serialize(self.h, dptr(x)))
        return x

    def deserialize(self, x):
        nc, npnt = self.prob.n_images, self.prob.n_points
        R = 5 + self.prob.nK + self.prob.nP
        IO, EO, OP = np.empty(R * nc), np.empty(6 * nc), np.empty(3 * npnt)
        x = np.ascontiguousarray(x, float)
        check(self.lib.dbat_hip_deserialize(self.h, dptr(x), dptr(IO), dptr(EO), dptr(OP)))
        return (IO.reshape(R, nc, order='F'), EO.reshape(6, nc, order='F'),
                OP.reshape(3, npnt, order='F'))

    def structural_rank_ok(self):
        ok = C.c_int32(0)
        check(self.lib.dbat_hip_structural_rank_ok(self.h, C.byref(ok)))
        return bool(ok.value)

    def residual(self, x, want_r=True):
        x = np.ascontiguousarray(x, float)
        r = np.zeros(self.m) if want_r else None
        f = C.c_double(0)
        check(self.lib.dbat_hip_residual(self.h, dptr(x), dptr(r), C.byref(f)))
        return (r, f.value) if want_r else f.value

    def jacobian_blocks(self, x):
        no, R = self.prob.n_obs, 5 + self.prob.nK + self.prob.nP
        x = np.ascontiguousarray(x, float)
        JEO, JOP, JIO = np.zeros(12 * no), np.zeros(6 * no), np.zeros(2 * R * no)
        check(self.lib.dbat_hip_jacobian_blocks(self.h, dptr(x), dptr(JEO), dptr(JOP), dptr(JIO)))
        return (JEO.reshape(no, 6, 2).transpose(0, 2, 1), JOP.reshape(no, 3, 2).transpose(0, 2, 1),
                JIO.reshape(no, R, 2).transpose(0, 2, 1))

    def jacobian_sample(self, x, ip_cols):
        """Residual and Jacobian blocks of the image observations ip_cols (IP columns, 0-based): (r n x 2, JEO n x 2 x 6,
        JOP n x 2 x 3, JIO n x 2 x nIOrows)."""
        idx = np.ascontiguousarray(ip_cols, np.int64)
        n, R = idx.size, 5 + self.prob.nK + self.prob.nP
        x = np.ascontiguousarray(x, float)
        r, JEO, JOP, JIO = np.zeros(2 * n), np.zeros(12 * n), np.zeros(6 * n), np.zeros(2 * R * n)
        check(self.lib.dbat_hip_jacobian_sample(self.h, dptr(x), n, idx.ctypes.data_as(C.POINTER(C.c_int64)), dptr(r), dptr(JEO),
                                                dptr(JOP), dptr(JIO)))
        return (r.reshape(n, 2), JEO.reshape(n, 6, 2).transpose(0, 2, 1), JOP.reshape(n, 3, 2).transpose(0, 2, 1),
                JIO.reshape(n, R, 2).transpose(0, 2, 1))

    def jacobian_csc(self, x, weighted=True):
        """J at x as scipy.sparse.csc_matrix (m x n): E.final.weighted.J / unweighted.J of bundle.m:341-350."""
        import scipy.sparse as sp
        x = np.ascontiguousarray(x, float)
        nnz = C.c_int64(0)
        check(self.lib.dbat_hip_jacobian_csc(self.h, dptr(x), int(bool(weighted)), C.byref(nnz), None, None, None))
        colptr = np.zeros(self.n + 1, np.int64)
        rowidx = np.zeros(max(nnz.value, 1), np.int64)
        val = np.zeros(max(nnz.value, 1))
        i64 = C.POINTER(C.c_int64)
        check(self.lib.dbat_hip_jacobian_csc(self.h, dptr(x), int(bool(weighted)), C.byref(nnz), colptr.ctypes.data_as(i64),
                                             rowidx.ctypes.data_as(i64), dptr(val)))
        return sp.csc_matrix((val[:nnz.value], rowidx[:nnz.value], colptr), shape=(self.m, self.n))

    def linearize_solve(self, x, lam=0.0, scale=True):
        x = np.ascontiguousarray(x, float)
        p, st = np.empty(self.n), np.empty(8)
        check(self.lib.dbat_hip_linearize_solve(self.h, dptr(x), float(lam), int(bool(scale)),
                                                dptr(p), dptr(st)))
        return p, dict(f=st[0], JpJp=st[1], rJp=st[2], pp=st[3], trace=st[4], singular=bool(st[5]), rcond=st[6], chol_info=int(st[7]))

    def gradient(self):
        g = np.empty(self.n)
        check(self.lib.dbat_hip_gradient(self.h, dptr(g)))
        return g

    def colnorms(self):
        g = np.empty(self.n)
        check(self.lib.dbat_hip_colnorms(self.h, dptr(g)))
        return g

    def jtimes_sqnorm(self, v):
        v = np.ascontiguousarray(v, float)
        out = C.c_double(0)
        check(self.lib.dbat_hip_jtimes_sqnorm(self.h, dptr(v), C.byref(out)))
        return out.value

    def jtimes(self, v):
        """J v at the last linearisation point: m weighted rows in the reference's row order."""
        v = np.ascontiguousarray(v, float)
        out = np.zeros(self.m)
        check(self.lib.dbat_hip_jtimes(self.h, dptr(v), dptr(out)))
        return out

    def solve(self, x0, opt, term_fun=None, veto_fun=None, trace_fun=None):
        """term_fun(Jp, r) -> bool and veto_fun(x) -> bool: the caller's own tests (bundle.m:168-192), called from the
        damping loop with numpy views of the library's vectors; an exception inside one ends the run and is re-raised.
        trace_fun(damping, n, res_norm, damp, step_type, rho): called where the reference's solver prints its 'trace' line
        (trace_text formats it)."""
        x = np.ascontiguousarray(x0, float).copy()
        raised = []

        def guarded(fn, *views):
            if raised:
                return 1
            try:
                return int(bool(fn(*views)))
            except BaseException as e:          # (never unwind through the C frames)
                raised.append(e)
                return 1
        keep = []
        if term_fun is not None:
            keep.append(TERM_FN(lambda _u, Jp, r, m: guarded(term_fun, np.ctypeslib.as_array(Jp, (m,)).copy(),
                                                             np.ctypeslib.as_array(r, (m,)).copy())))
            opt.term_fun = C.cast(keep[-1], C.c_void_p)
        if veto_fun is not None:
            keep.append(VETO_FN(lambda _u, xx, n: guarded(veto_fun, np.ctypeslib.as_array(xx, (n,)).copy())))
            opt.veto_fun = C.cast(keep[-1], C.c_void_p)
        if trace_fun is not None:
            def traced(_u, damping, n, res, damp, step, rho):
                if not raised:
                    try:
                        trace_fun(damping, n, res, damp, step, rho)
                    except BaseException as e:
                        raised.append(e)
            keep.append(TRACE_FN(traced))
            opt.trace_fun = C.cast(keep[-1], C.c_void_p)
        try:
            return self._solve(x, opt, raised)
        finally:
            if trace_fun is not None:
                opt.trace_fun = None
            if term_fun is not None:
                opt.term_fun = None
            if veto_fun is not None:
                opt.veto_fun = None

    def _solve(self, x, opt, raised):
        res = Result()
        mi = opt.max_iter
        rr = np.full(mi + 3, np.nan)
        damp = np.full(2 * mi + 4, np.nan)
        aux = np.full(2 * mi + 4, np.nan)
        # (not filled: the library writes n_trace columns and only those are handed on -- filling the 22 columns of a
        # 3 M-unknown project with NaN was 50 ms of every solve)
        trace = np.empty(self.n * (mi + 2)) if opt.store_trace else None
        check(self.lib.dbat_hip_solve(self.h, C.byref(opt), dptr(x), C.byref(res), dptr(rr),
                                      dptr(damp), dptr(aux), dptr(trace)))
        if raised:
            raise raised[0]
        T = (trace[:self.n * res.n_trace].reshape(self.n, res.n_trace, order='F')
             if trace is not None else None)
        return x, res, rr[:res.n_res], damp[:res.n_damp], aux, T

    def final_residuals(self):
        ru, rw = np.empty(self.m), np.empty(self.m)
        check(self.lib.dbat_hip_final_residuals(self.h, dptr(ru), dptr(rw)))
        return ru, rw

    def forwintersect(self, x, OP, skip=None):
        """OP (3 x n_points) with the points of skip == False replaced by the forward
        intersection of their rays at the IO / EO of x."""
        x = np.ascontiguousarray(x, float)
        out = np.ascontiguousarray(np.asarray(OP, float).flatten('F'))
        sk = None if skip is None else np.ascontiguousarray(np.asarray(skip, bool).astype(np.uint8))
        check(self.lib.dbat_hip_forwintersect(self.h, dptr(x), None if sk is None else sk.ctypes.data_as(_bp), dptr(out)))
        return out.reshape(3, -1, order='F')

    def set_deterministic(self, on=True):
        """Exact (order-independent) sums into the reduced system: bit-identical runs.  DbatHipError(EUNSUPPORTED) for
        several ranks, shared EO blocks or more than nine IO columns per camera."""
        check(self.lib.dbat_hip_set_deterministic(self.h, int(bool(on))))

    def build_kernel_name(self):
        buf = C.create_string_buffer(64)
        check(self.lib.dbat_hip_build_kernel_name(self.h, buf, 64))
        return buf.value.decode()

    def comm_init(self, unique_id):
        """Join the RCCL communicator of `unique_id` (128 bytes from comm_unique_id()
        on rank 0) as rank shard_rank of shard_count.  Collective."""
        buf = (C.c_uint8 * UNIQUE_ID_BYTES).from_buffer_copy(bytes(unique_id))
        check(self.lib.dbat_hip_comm_init(self.h, buf))

    def comm_allreduce_host(self, a, op='sum'):
        a = np.ascontiguousarray(a, np.float64).copy()
        check(self.lib.dbat_hip_comm_allreduce_host(self.h, dptr(a), a.size, {'sum': 0, 'max': 1, 'min': 2}[op]))
        return a

    def set_allreduce(self, pyfunc):
        """pyfunc(ptr:int, count:int, stream:int) -> int (0 ok)."""
        def tramp(user, buf, count, stream):
            try:
                return int(pyfunc(int(buf or 0), int(count), int(stream or 0)) or 0)
            except Exception:   # noqa: BLE001 - must not unwind through C
                import traceback
                traceback.print_exc()
                return 1
        self._cb = ALLREDUCE_FN(tramp)
        check(self.lib.dbat_hip_set_allreduce(self.h, self._cb, None))

    def owned_mask(self):
        m = np.zeros(self.n, np.uint8)
        check(self.lib.dbat_hip_owned_mask(self.h, m.ctypes.data_as(_bp)))
        return m.astype(bool)

    def index_maps(self):
        """x index of every IO/EO/OP array entry (-1 = not an unknown); the
        deserial maps of misc/buildserialindices.m:204-221."""
        if getattr(self, '_index_maps', None) is None:     # a matter of the structure: once per handle (read-only arrays)
            big = 1e15
            IO, EO, OP = self.deserialize(big + np.arange(self.n, dtype=float))
            f = lambda a: np.where(a >= big / 2, np.rint(a - big), -1).astype(np.int64)
            maps = f(IO), f(EO), f(OP)
            for a in maps:
                a.setflags(write=False)
            self._index_maps = maps
        return self._index_maps

    def posterior_cov(self, x, sigma0, want_sinv=False):
        """sigma0^2 * blocks of inv(J'J) at x (bundle_cov.m): CEO (nc,6,6), CIOu
        (nIOu,nIOu; IO unknowns in z order, see x2z), COP (np,3,3) and, if asked
        for, inv(S) (NS,NS; symmetrised, not scaled by sigma0^2)."""
        x = np.ascontiguousarray(x, float)
        NS = self.info()['NS']
        nc, npnt = int(self.prob.n_images), int(self.prob.n_points)
        nIOu = NS - 6 * nc
        CEO = np.zeros(36 * nc)
        CIO = np.zeros(max(nIOu * nIOu, 1))
        COP = np.zeros(9 * npnt)
        Sinv = np.zeros(NS * NS) if want_sinv else None
        check(self.lib.dbat_hip_posterior_cov(self.h, dptr(x), float(sigma0), dptr(CEO), dptr(CIO), dptr(COP),
                                              dptr(Sinv) if want_sinv else None))
        out = [CEO.reshape(nc, 6, 6).transpose(0, 2, 1), CIO[:nIOu * nIOu].reshape(nIOu, nIOu).T,
               COP.reshape(npnt, 3, 3).transpose(0, 2, 1)]
        if want_sinv:
            L = np.tril(Sinv.reshape(NS, NS).T)
            out.append(L + np.tril(L, -1).T)
        return tuple(out)

    def redundancy(self, x):
        """Reliability at x (dbat_hip_redundancy): Qvv = I - H of every image point as (3, n_obs) rows r_u, q_uv, r_v
        (IP column order), and the redundancy numbers of the prior rows (m - 2 n_obs,) in the row order of
        final_residuals."""
        x = np.ascontiguousarray(x, float)
        no = int(self.prob.n_obs)
        qvv = np.zeros(3 * max(no, 1))
        rp = np.zeros(max(self.m - 2 * no, 1))
        check(self.lib.dbat_hip_redundancy(self.h, dptr(x), dptr(qvv), dptr(rp)))
        return qvv[:3 * no].reshape(3, no, order='F'), rp[:self.m - 2 * no]

    def ray_angles(self, x):
        """Ray intersection angles at x (dbat_hip_ray_angles): (op, cam, op_rays, cam_rays) -- the largest angle
        [rad] between two rays of every object point and of every image (0 for one ray, NaN for none) and the
        numbers of rays.  DbatHipError on a handle that is one shard of several."""
        x = np.ascontiguousarray(x, float)
        nc, npnt = int(self.prob.n_images), int(self.prob.n_points)
        op, cam = np.zeros(max(npnt, 1)), np.zeros(max(nc, 1))
        opr, camr = np.zeros(max(npnt, 1), np.int32), np.zeros(max(nc, 1), np.int32)
        check(self.lib.dbat_hip_ray_angles(self.h, dptr(x), dptr(op), dptr(cam), opr.ctypes.data_as(_ip),
                                           camr.ctypes.data_as(_ip)))
        return op[:npnt], cam[:nc], opr[:npnt], camr[:nc]

    def ray_angles_ms(self):
        """Device-event milliseconds of the last ray_angles (debug): point kernels, unit directions of the images,
        pair kernel + acos; and the matrix-core instructions (256 pairs each) and workgroups of the pair kernel."""
        ms, info = np.zeros(3), (C.c_int64 * 2)()
        check(self.lib.dbat_hip_debug_ray_angles_ms(self.h, dptr(ms), info))
        return dict(points=float(ms[0]), cam_dirs=float(ms[1]), cam_pairs=float(ms[2]), mfma=int(info[0]),
                    workgroups=int(info[1]))

    def point_depths(self, x, thr=0.0, want_depth=True):
        """Point depths at x (dbat_hip_point_depths): (depth, image_min, n_behind, min_depth, argmin) -- the depth of
        every IP column (None with want_depth=False), the smallest depth per image (NaN for none), the number of
        columns with !(depth > thr), the smallest depth and the smallest column that attains it (-1: none)."""
        x = np.ascontiguousarray(x, float)
        nc, no = int(self.prob.n_images), int(self.prob.n_obs)
        d = np.zeros(max(no, 1)) if want_depth else None
        im = np.zeros(max(nc, 1))
        st = DepthStats()
        check(self.lib.dbat_hip_point_depths(self.h, dptr(x), float(thr), dptr(d), dptr(im), C.byref(st)))
        return (d[:no] if want_depth else None), im[:nc], int(st.n_behind), float(st.min_depth), int(st.argmin_column)

    def point_depths_ms(self):
        """Device-event milliseconds of the kernels of the last point_depths (debug)."""
        ms = np.zeros(1)
        check(self.lib.dbat_hip_debug_point_depths_ms(self.h, dptr(ms)))
        return float(ms[0])

    def chirality_pass_ms(self, x, reps=20):
        """Device-event milliseconds of one pass of the built-in veto at x (debug; the mean of reps passes back to back)
        and the count it found."""
        x = np.ascontiguousarray(x, float)
        ms = np.zeros(2)
        check(self.lib.dbat_hip_debug_chirality_pass_ms(self.h, dptr(x), int(reps), dptr(ms)))
        return float(ms[0]), int(ms[1])

    def set_chirality(self, on=True, min_depth=0.0):
        """The built-in chirality veto of the damping loops (dbat_hip_set_chirality): a trial point with an observation
        whose depth is not above min_depth is rejected.  DbatHipError for a shard of several or a min_depth that is
        not finite."""
        check(self.lib.dbat_hip_set_chirality(self.h, int(bool(on)), float(min_depth)))

    def chirality_stats(self):
        """(tested, rejected, n_behind, min_depth) of the built-in veto during the last solve."""
        st = VetoStats()
        check(self.lib.dbat_hip_chirality_stats(self.h, C.byref(st)))
        return int(st.tested), int(st.rejected), int(st.n_behind), float(st.min_depth)

    def coverage(self):
        """Image coverage by the measured points (dbat_hip_coverage), per image: a dict with lo, hi (2, nImages), rad_max
        [mm], rad_ip, hull_area [px^2] and hull, the list of the hulls' vertices as arrays of IP columns
        (counter-clockwise from the lowest (u, v), closing point not repeated).  DbatHipError on a sharded handle."""
        return _coverage_call(lambda *a: self.lib.dbat_hip_coverage(self.h, *a), int(self.prob.n_images), int(self.prob.n_obs))

    def residual_stats(self, x):
        """Marking-residual statistics at x (dbat_hip_residual_stats): a dict with cam_n, cam_ss (per image), op_n, op_ss
        (per object point), total_ss, max_e and max_ip -- sums of squared pixel residual norms, the largest norm and
        its IP column."""
        x = np.ascontiguousarray(x, float)
        nc, npnt = int(self.prob.n_images), int(self.prob.n_points)
        cam_n, op_n = np.zeros(max(nc, 1), np.int64), np.zeros(max(npnt, 1), np.int64)
        cam_ss, op_ss = np.zeros(max(nc, 1)), np.zeros(max(npnt, 1))
        tot, mx, mip = C.c_double(), C.c_double(), C.c_int64()
        check(self.lib.dbat_hip_residual_stats(self.h, dptr(x), cam_n.ctypes.data_as(_lp), dptr(cam_ss),
                                               op_n.ctypes.data_as(_lp), dptr(op_ss), C.cast(C.byref(tot), _dp),
                                               C.cast(C.byref(mx), _dp), C.cast(C.byref(mip), _lp)))
        return dict(cam_n=cam_n[:nc], cam_ss=cam_ss[:nc], op_n=op_n[:npnt], op_ss=op_ss[:npnt], total_ss=tot.value,
                    max_e=mx.value, max_ip=int(mip.value))

    def quality_ms(self):
        """Device-event milliseconds of the kernels of the last coverage() and the last residual_stats() (debug)."""
        ms = np.zeros(2)
        check(self.lib.dbat_hip_debug_quality_ms(self.h, dptr(ms)))
        return dict(coverage=float(ms[0]), residual_stats=float(ms[1]))

    def robust_weights(self, x, ropt):
        """One reweighting evaluation at x, not applied (dbat_hip_robust_weights): (omega, s_norm, scale), the two
        vectors per IP column."""
        x = np.ascontiguousarray(x, float)
        no = int(self.prob.n_obs)
        om, sn, sc = np.zeros(max(no, 1)), np.zeros(max(no, 1)), C.c_double()
        check(self.lib.dbat_hip_robust_weights(self.h, dptr(x), C.byref(ropt), dptr(om), dptr(sn), C.byref(sc)))
        return om[:no], sn[:no], sc.value

    def set_obs_weights(self, omega):
        """Weight factors omega in (0, 1] per IP column (dbat_hip_set_obs_weights); None: back to the base weights."""
        if omega is None:
            check(self.lib.dbat_hip_set_obs_weights(self.h, None))
            return
        om = np.ascontiguousarray(omega, float).ravel()
        if om.size != int(self.prob.n_obs):
            raise ValueError('set_obs_weights: %d values for %d image points' % (om.size, int(self.prob.n_obs)))
        check(self.lib.dbat_hip_set_obs_weights(self.h, dptr(om)))

    def debug_robust_from_s(self, s, ropt):
        """The select, scale and weight half of a reweighting evaluation on the caller's s per IP column (debug,
        dbat_hip_debug_robust_from_s; not applied): (omega, median, scale, max_change, owned) -- median NaN with the
        a-priori scale, owned the mask of the IP columns this rank holds.  Collective on a sharded handle."""
        s = np.ascontiguousarray(s, float).ravel()
        no = int(self.prob.n_obs)
        if s.size != no:
            raise ValueError('debug_robust_from_s: %d values for %d image points' % (s.size, no))
        om, own = np.zeros(max(no, 1)), np.zeros(max(no, 1), np.uint8)
        med, sc, chg = C.c_double(), C.c_double(), C.c_double()
        check(self.lib.dbat_hip_debug_robust_from_s(self.h, dptr(s), C.byref(ropt), dptr(om), C.byref(med), C.byref(sc),
                                                    C.byref(chg), own.ctypes.data_as(_bp)))
        return om[:no], med.value, sc.value, chg.value, own[:no].astype(bool)

    def solve_robust(self, x0, opt, ropt):
        """The IRLS outer loop (dbat_hip_solve_robust): (x, Result, res, damp, aux, T, RobustResult, omega) -- the
        arrays of the last inner solve, as solve() returns them, and the weight factors per IP column."""
        x = np.ascontiguousarray(x0, float).copy()
        res, rr = Result(), RobustResult()
        mi = opt.max_iter
        r = np.full(mi + 3, np.nan)
        damp = np.full(2 * mi + 4, np.nan)
        aux = np.full(2 * mi + 4, np.nan)
        trace = np.empty(self.n * (mi + 2)) if opt.store_trace else None
        no = int(self.prob.n_obs)
        om = np.ones(max(no, 1))
        check(self.lib.dbat_hip_solve_robust(self.h, C.byref(opt), C.byref(ropt), dptr(x), C.byref(res), dptr(r),
                                             dptr(damp), dptr(aux), dptr(trace), C.byref(rr), dptr(om)))
        T = (trace[:self.n * res.n_trace].reshape(self.n, res.n_trace, order='F')
             if trace is not None else None)
        return x, res, r[:res.n_res], damp[:res.n_damp], aux, T, rr, om[:no]

    def set_x(self, x):
        x = np.ascontiguousarray(x, float)
        check(self.lib.dbat_hip_set_x(self.h, dptr(x)))

    def bench_step(self, lam=0.0, scale=False):
        ms = np.zeros(16)
        check(self.lib.dbat_hip_bench_step(self.h, float(lam), int(bool(scale)), dptr(ms)))
        return ms

    def chol_stats(self):
        a = (C.c_int64 * 6)()
        check(self.lib.dbat_hip_chol_stats(self.h, a))
        keys = ('order_padded', 'tile_tasks', 'tile_products', 'tile_rows', 'nested_dissection', 'dataflow')
        return dict(zip(keys, [int(v) for v in a]))

    def info(self):
        a = (C.c_int64 * 24)()
        check(self.lib.dbat_hip_info(self.h, a))
        keys = ('NS', 'n_batches', 'max_k', 'n_obs_shard', 'n_pts_shard', 'BT', 'ncolmax', 'n_tiles',
                'domain_sharding', 'reduced_doubles_per_factorisation', 'vector_doubles_per_linearisation',
                'n_top_cams', 'factor_tile_rows', 'tasks_domain', 'tasks_top', 'tile_kernel_mfma',
                'heavy_tasks', 'heavy_mfma', 'heavy_row_groups', 'heavy_scratch_bytes', 'heavy_points', 'heavy_obs',
                'heavy_ksteps_per_task', 'heavy_algorithmic_flops')
        return dict(zip(keys, [int(v) for v in a]))


def structure_key(s, device=0, shard_rank=0, shard_count=1, _problem=None):
    """Host-only: the 128-bit key of everything a plan depends on (dbat_hip_structure_key) -- equal keys: one handle
    serves both structs through Handle.set_values."""
    prob, keep = _problem if _problem is not None else problem_from_struct(s, device, shard_rank, shard_count)
    k = (C.c_uint64 * 2)()
    check(load().dbat_hip_structure_key(C.byref(prob), k))
    return (int(k[0]), int(k[1]))


# ---- handle cache: bundle() -> bundle() -> bundle_cov() on one structure build ONE plan (the reference keeps its index
# structures in s.bundle.serial / deserial, bundle.m:156-159).  One handle (it owns device memory in proportion to the
# problem), one-rank handles only; a struct whose structure key differs -- a changed mask, block, observation -- gets a
# new handle and the cached one is destroyed.
_cached = None
cache_stats = {'hits': 0, 'misses': 0}


def acquire(s, device=0):
    """A one-rank handle for s: the cached one with s's values (dbat_hip_set_values) when the structure key matches, a
    new one otherwise.  Give it back with release()."""
    global _cached
    problem = problem_from_struct(s, device)
    h, _cached = _cached, None
    if h is not None and h.h:
        if h.key() == structure_key(None, _problem=problem):
            try:
                h.set_values(_problem=problem)
                cache_stats['hits'] += 1
                cache_stats['last'] = 'hit'
                return h
            except DbatHipError:
                pass
        h.close()
    cache_stats['misses'] += 1
    cache_stats['last'] = 'miss'
    return Handle(None, _problem=problem)


def release(h, keep=True):
    """Return a handle of acquire(): kept for the next acquire() of the same structure (keep=False, or an older cached
    handle: closed)."""
    global _cached
    if not keep or h is None or not h.h:
        if h is not None:
            h.close()
        return
    if _cached is not None and _cached is not h:
        _cached.close()
    h.set_deterministic(False)
    h.set_chirality(False)
    _cached = h


def clear_cache():
    """Destroy the cached handle (frees its device memory)."""
    global _cached
    if _cached is not None:
        _cached.close()
    _cached = None


def default_options(damping='gna'):
    o = Options()
    check(load().dbat_hip_default_options(DAMP[damping.lower()], C.byref(o)))
    return o


def robust_options(loss, k=None, scale='apriori', max_outer=10, weight_tol=1e-3):
    """dbat_hip_robust_options for loss 'huber' | 'cauchy' (k None: the library's default for the loss)."""
    o = RobustOptions()
    check(load().dbat_hip_default_robust_options(LOSS[loss], C.byref(o)))
    if k is not None:
        o.k = float(k)
    o.scale = SCALE[scale]
    o.max_outer = int(max_outer)
    o.weight_tol = float(weight_tol)
    return o


def plan(s, shard_rank=0, shard_count=1):
    """Host-only index plan (no GPU needed): sizes of x and r, shard range."""
    lib = load()
    p, keep = problem_from_struct(s, 0, shard_rank, shard_count)
    v = [C.c_int64(0) for _ in range(7)]
    check(lib.dbat_hip_plan(C.byref(p), *[C.byref(a) for a in v]))
    keys = ('n', 'm', 'nIO', 'nEO', 'nOP', 'pt_lo', 'pt_hi')
    return dict(zip(keys, [a.value for a in v]))


def plan_structural_rank_ok(s):
    """Host-only: does J have full structural rank (sprank(J) == n)?  No GPU needed."""
    lib = load()
    p, keep = problem_from_struct(s)
    ok = C.c_int32(0)
    check(lib.dbat_hip_plan_structural_rank_ok(C.byref(p), C.byref(ok)))
    return bool(ok.value)


def plan_point_owner(s, shard_count):
    """Host-only: rank owning every object point (no GPU needed)."""
    lib = load()
    p, keep = problem_from_struct(s, 0, 0, shard_count)
    owner = np.full(s.OP.val.shape[1], -1, np.int32)
    check(lib.dbat_hip_plan_point_owner(C.byref(p), owner.ctypes.data_as(_ip)))
    return owner


# ---- the calls that take a device index instead of a handle (csrc/batch_host.hpp): what their wrappers share ----

def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _out(n, per=1, dtype=float):
    """Zeros for per values of each of n items -- of one item when n is 0: an output is never a null pointer."""
    return np.zeros(per * max(n, 1), dtype)


def _poses_in(P, n):
    """(n, 3, 4) poses as 12 column-major doubles each: a copy, padded like an output."""
    Pf = np.ascontiguousarray(P.transpose(0, 2, 1)).reshape(-1).copy()
    return np.concatenate([Pf, np.zeros(12)]) if n == 0 else Pf


def _poses_out(Pf, n):
    return Pf[:12 * n].reshape(n, 4, 3).transpose(0, 2, 1)


def _mask(use, total):
    return None if use is None else np.ascontiguousarray(np.broadcast_to(np.asarray(use, bool), (total,))).view(np.uint8)


def _weights(w, total):
    return None if w is None else _f64(np.broadcast_to(np.asarray(w, float), (2, total)))


def _adjust_stats(n, ds, ist, Q):
    """The per-item results dbat_hip_pairadjust and dbat_hip_poseadjust share, from their dstat, istat and Q."""
    ds, ist = ds[:4 * n].reshape(n, 4), ist[:4 * n].reshape(n, 4)
    return dict(f0=ds[:, 0].copy(), f=ds[:, 1].copy(), sigma0=ds[:, 2].copy(), lam=ds[:, 3].copy(), code=ist[:, 0].copy(),
                iters=ist[:, 1].copy(), trials=ist[:, 2].copy(), n_used=ist[:, 3].copy(), Q=Q[:36 * n].reshape(n, 6, 6).transpose(0, 2, 1))


def _kernel_ms(family, slots):
    ms = np.zeros(len(slots))
    check(getattr(load(), 'dbat_hip_debug_%s_ms' % family)(dptr(ms)))
    return dict(zip(slots, map(float, ms)))


def resect_poses(pt_start, X, xn, tri_start, tri, device=0):
    """dbat_hip_resect: best 3 x 4 camera matrix (n, 3, 4) and rms (n) per camera from its candidate triangles."""
    lib = load()
    n = len(pt_start) - 1
    ps, ts = np.ascontiguousarray(pt_start, np.int64), np.ascontiguousarray(tri_start, np.int64)
    Xf = np.ascontiguousarray(np.asarray(X, float).flatten('F'))
    xf = np.ascontiguousarray(np.asarray(xn, float).flatten('F'))
    tf = np.ascontiguousarray(np.asarray(tri, np.int32).reshape(-1))
    P, rms = np.empty(12 * n), np.empty(n)
    check(lib.dbat_hip_resect(int(device), n, _ptr(ps, _lp), dptr(Xf), dptr(xf), _ptr(ts, _lp), _ptr(tf, _ip), dptr(P), dptr(rms)))
    return _poses_out(P, n), rms


def essmat5_sets(set_start, Q1, Q2, device=0):
    """dbat_hip_essmat5 over the sets set_start[i] .. set_start[i + 1] of the columns of Q1, Q2 (3-by-total): (E (n, 10, 9),
    n_sol (n)); E[i, k] is solution k of set i, sum E[i, k, a + 3 b] Q1[a] Q2[b] = 0, zero for k >= n_sol[i]."""
    lib = load()
    ss = np.ascontiguousarray(set_start, np.int64)
    n = len(ss) - 1
    Q1, Q2 = np.asarray(Q1, float), np.asarray(Q2, float)
    if Q1.ndim != 2 or Q1.shape[0] != 3 or Q1.shape != Q2.shape or n < 0 or (n >= 0 and Q1.shape[1] != ss[-1]):
        raise ValueError('essmat5: Q1 and Q2 must both be 3-by-n, n the end of the last set')
    q1, q2 = _f64(Q1), _f64(Q2)
    E, ns = _out(n, 90), _out(n, 1, np.int32)
    check(lib.dbat_hip_essmat5(int(device), n, _ptr(ss, _lp), dptr(q1), dptr(q2), dptr(E), _ptr(ns, _ip)))
    return E[:90 * n].reshape(n, 10, 9), ns[:n]


def relorient_pairs(pt_start, x1, x2, hyp_start, samples, thr2, front_dir, device=0):
    """dbat_hip_relorient over the pairs pt_start[i] .. pt_start[i + 1] of the columns of x1, x2 (2-by-total) with the
    samples hyp_start[i] .. hyp_start[i + 1] of the rows of samples (five indices local to the pair each) and the
    thresholds thr2 (one per pair): dict(E (n, 9), P2 (n, 3, 4), stats (n, 8), inlier, in_front (total booleans),
    X (3, total))."""
    lib = load()
    ps, hs = np.ascontiguousarray(pt_start, np.int64), np.ascontiguousarray(hyp_start, np.int64)
    n = len(ps) - 1
    x1, x2 = np.asarray(x1, float), np.asarray(x2, float)
    smp = np.ascontiguousarray(np.asarray(samples, np.int32).reshape(-1, 5))
    t2 = np.ascontiguousarray(np.broadcast_to(np.asarray(thr2, float), (max(n, 0),)))
    if len(hs) != n + 1 or x1.ndim != 2 or x1.shape[0] != 2 or x1.shape != x2.shape or x1.shape[1] != ps[-1] or smp.shape[0] != hs[-1]:
        raise ValueError('relorient: x1 and x2 must both be 2-by-n and samples k-by-5, n and k the ends of the last ranges')
    total = x1.shape[1]
    a, b = _f64(x1), _f64(x2)
    E, P2, st = _out(n, 9), _out(n, 12), _out(n, 8, np.int32)
    inl, fr, X = _out(total, 1, np.uint8), _out(total, 1, np.uint8), _out(total, 3)
    check(lib.dbat_hip_relorient(int(device), n, _ptr(ps, _lp), dptr(a), dptr(b), _ptr(hs, _lp), _ptr(smp, _ip), dptr(t2),
                                 int(front_dir), dptr(E), dptr(P2), _ptr(st, _ip), _ptr(inl, _bp), _ptr(fr, _bp), dptr(X)))
    return dict(E=E[:9 * n].reshape(n, 9), P2=_poses_out(P2, n), stats=st[:8 * n].reshape(n, 8),
                inlier=inl[:total].astype(bool), in_front=fr[:total].astype(bool), X=X[:3 * total].reshape(3, total, order='F'))


def cams_from_e(e, x1, x2, front_dir, device=0):
    """dbat_hip_relorient without samples (hyp_start NULL) for one pair and the given model e (9: sum e[a + 3 b] q1[a]
    q2[b] = 0): dict(P2 (3, 4), X (3, n), in_front (n), sp (4))."""
    lib = load()
    x1, x2 = np.asarray(x1, float), np.asarray(x2, float)
    if x1.ndim != 2 or x1.shape[0] != 2 or x1.shape != x2.shape:
        raise ValueError('camsfrome: the points must be 2-by-n')
    n = x1.shape[1]
    ps = np.array([0, n], np.int64)
    a, b, E, t2 = _f64(x1), _f64(x2), np.ascontiguousarray(np.asarray(e, float).reshape(9)).copy(), np.ones(1)
    P2, st = _out(1, 12), _out(1, 8, np.int32)
    inl, fr, X = _out(n, 1, np.uint8), _out(n, 1, np.uint8), _out(n, 3)
    check(lib.dbat_hip_relorient(int(device), 1, _ptr(ps, _lp), dptr(a), dptr(b), None, None, dptr(t2), int(front_dir), dptr(E),
                                 dptr(P2), _ptr(st, _ip), _ptr(inl, _bp), _ptr(fr, _bp), dptr(X)))
    return dict(P2=P2.reshape(4, 3).T.copy(), X=X[:3 * n].reshape(3, n, order='F'), in_front=fr[:n].astype(bool), sp=st[4:8].copy())


def relorient_timing(on=True):
    """Device events around the kernels of essmat5_sets / relorient_pairs calls on this thread (debug; off by default)."""
    check(load().dbat_hip_debug_relorient_timing(int(bool(on))))


def relorient_ms():
    """Device-event milliseconds of the kernels of the last essmat5_sets / relorient_pairs call on this thread, after
    relorient_timing(True) (debug)."""
    return _kernel_ms('relorient', ('solve', 'score', 'cams'))


PAIR_CODES = ('converged', 'max_iter', 'no_step', 'singular', 'too_few')


def pairadjust(pt_start, x1, x2, P2, X, use=None, w1=None, w2=None, front_dir=-1, max_iter=20, conv_tol=1e-6, min_angle=0.0,
               residuals=False, device=0):
    """dbat_hip_pairadjust over the pairs pt_start[i] .. pt_start[i + 1] of the columns of x1, x2 (2-by-total), from the
    start values P2 (n, 3, 4: [R | t]) and X (3-by-total); use (total booleans) and the weights w1, w2 (2-by-total, or
    anything that broadcasts to it) are optional, min_angle is in radians.  Nothing given is changed.  Returns
    dict(P2 (n, 3, 4), X (3, total), used (total), f0, f, sigma0, lam (n), code, iters, trials, n_used (n), Q (n, 6, 6),
    res (2, 2, total: image, axis; None unless residuals))."""
    lib = load()
    ps = np.ascontiguousarray(pt_start, np.int64)
    n = len(ps) - 1
    x1, x2, X = np.asarray(x1, float), np.asarray(x2, float), np.asarray(X, float)
    P2 = np.asarray(P2, float).reshape(-1, 3, 4)
    if n < 0 or x1.ndim != 2 or x1.shape[0] != 2 or x1.shape != x2.shape or x1.shape[1] != ps[-1] or X.shape != (3, x1.shape[1]) \
            or P2.shape[0] != n:
        raise ValueError('pairadjust: x1 and x2 must be 2-by-total, X 3-by-total, total the end of the last range, and P2 one 3-by-4 per pair')
    total = x1.shape[1]
    a, b, wa, wb, u = _f64(x1), _f64(x2), _weights(w1, total), _weights(w2, total), _mask(use, total)
    P = _poses_in(P2, n)
    Xf = np.zeros(3) if total == 0 else X.flatten('F')
    used, ds, ist, Q = _out(total, 1, np.uint8), _out(n, 4), _out(n, 4, np.int32), _out(n, 36)
    res = _out(total, 4) if residuals else None
    opt = PairOptions(int(max_iter), float(conv_tol), float(min_angle))
    check(lib.dbat_hip_pairadjust(int(device), n, _ptr(ps, _lp), dptr(a), dptr(b), _ptr(u, _bp), dptr(wa), dptr(wb), int(front_dir),
                                  C.byref(opt), dptr(P), dptr(Xf), _ptr(used, _bp), dptr(ds), _ptr(ist, _ip), dptr(Q), dptr(res)))
    return dict(P2=_poses_out(P, n), X=Xf[:3 * total].reshape(3, total, order='F'), used=used[:total].astype(bool),
                **_adjust_stats(n, ds, ist, Q), res=None if res is None else res[:4 * total].reshape(total, 2, 2).transpose(1, 2, 0))


def pairadjust_timing(on=True):
    """Device events around the kernel of pairadjust calls on this thread (debug; off by default)."""
    check(load().dbat_hip_debug_pairadjust_timing(int(bool(on))))


def pairadjust_ms():
    """Device-event milliseconds of the kernel of the last pairadjust call on this thread, after pairadjust_timing(True)
    (debug)."""
    return _kernel_ms('pairadjust', ('kernel',))['kernel']


def resect_ransac(pt_start, X, xn, smp_start, samples, thr2, use=None, device=0):
    """dbat_hip_resect_ransac over the cameras pt_start[i] .. pt_start[i + 1] of the columns of X (3-by-total) and xn
    (2-by-total) with the samples smp_start[i] .. smp_start[i + 1] of the rows of samples (three indices local to the
    camera each), the thresholds thr2 (one per camera) and the optional mask use (total booleans):
    dict(P (n, 3, 4), stats (n, 4: count, sample, root, poses scored), inlier (total), ssq (n))."""
    lib = load()
    ps, ss = np.ascontiguousarray(pt_start, np.int64), np.ascontiguousarray(smp_start, np.int64)
    n = len(ps) - 1
    X, xn = np.asarray(X, float), np.asarray(xn, float)
    smp = np.ascontiguousarray(np.asarray(samples, np.int32).reshape(-1, 3))
    t2 = np.ascontiguousarray(np.broadcast_to(np.asarray(thr2, float), (max(n, 0),)))
    if n < 0 or len(ss) != n + 1 or X.ndim != 2 or X.shape[0] != 3 or xn.shape != (2, X.shape[1]) or X.shape[1] != ps[-1] or smp.shape[0] != ss[-1]:
        raise ValueError('resect_ransac: X must be 3-by-total, xn 2-by-total and samples k-by-3, total and k the ends of the last ranges')
    total = X.shape[1]
    Xf, xf, u = _f64(X), _f64(xn), _mask(use, total)
    P, st, ssq, inl = _out(n, 12), _out(n, 4, np.int32), _out(n), _out(total, 1, np.uint8)
    check(lib.dbat_hip_resect_ransac(int(device), n, _ptr(ps, _lp), dptr(Xf), dptr(xf), _ptr(u, _bp), _ptr(ss, _lp), _ptr(smp, _ip),
                                     dptr(t2), dptr(P), _ptr(st, _ip), _ptr(inl, _bp), dptr(ssq)))
    return dict(P=_poses_out(P, n), stats=st[:4 * n].reshape(n, 4), inlier=inl[:total].astype(bool), ssq=ssq[:n])


def poseadjust(pt_start, X, xn, P, use=None, w=None, max_iter=20, conv_tol=1e-6, min_angle=0.0, residuals=False, device=0):
    """dbat_hip_poseadjust over the cameras pt_start[i] .. pt_start[i + 1] of the columns of X (3-by-total) and xn
    (2-by-total), from the start poses P (n, 3, 4: [R | -R C]); use (total booleans) and the weights w (2-by-total, or
    anything that broadcasts to it) are optional.  Nothing given is changed.  Returns dict(P (n, 3, 4), used (total), f0,
    f, sigma0, lam (n), code, iters, trials, n_used (n), Q (n, 6, 6: centre, then rotation vector), res (2, total; None
    unless residuals))."""
    lib = load()
    ps = np.ascontiguousarray(pt_start, np.int64)
    n = len(ps) - 1
    X, xn = np.asarray(X, float), np.asarray(xn, float)
    P = np.asarray(P, float).reshape(-1, 3, 4)
    if n < 0 or X.ndim != 2 or X.shape[0] != 3 or xn.shape != (2, X.shape[1]) or X.shape[1] != ps[-1] or P.shape[0] != n:
        raise ValueError('poseadjust: X must be 3-by-total, xn 2-by-total, total the end of the last range, and P one 3-by-4 per camera')
    total = X.shape[1]
    Xf, xf, wt, u = _f64(X), _f64(xn), _weights(w, total), _mask(use, total)
    Pf = _poses_in(P, n)
    used, ds, ist, Q = _out(total, 1, np.uint8), _out(n, 4), _out(n, 4, np.int32), _out(n, 36)
    res = _out(total, 2) if residuals else None
    opt = PairOptions(int(max_iter), float(conv_tol), float(min_angle))
    check(lib.dbat_hip_poseadjust(int(device), n, _ptr(ps, _lp), dptr(Xf), dptr(xf), _ptr(u, _bp), dptr(wt), C.byref(opt), dptr(Pf),
                                  _ptr(used, _bp), dptr(ds), _ptr(ist, _ip), dptr(Q), dptr(res)))
    return dict(P=_poses_out(Pf, n), used=used[:total].astype(bool), **_adjust_stats(n, ds, ist, Q),
                res=None if res is None else res[:2 * total].reshape(total, 2).T)


def resect_robust_timing(on=True):
    """Device events around the kernels of resect_ransac / poseadjust calls on this thread (debug; off by default)."""
    check(load().dbat_hip_debug_resect_robust_timing(int(bool(on))))


def resect_robust_ms():
    """Device-event milliseconds of the kernels of the last resect_ransac and poseadjust calls on this thread, after
    resect_robust_timing(True) (debug)."""
    return _kernel_ms('resect_robust', ('ransac', 'adjust'))


def _rays(who, ray_start, cam, xn, P):
    """The arguments dbat_hip_intersect_ransac and dbat_hip_pointadjust share: (n, total, n_cams, ray_start, cam, xn, P)."""
    rs = np.ascontiguousarray(ray_start, np.int64)
    n = len(rs) - 1
    xn = np.asarray(xn, float)
    cm = np.ascontiguousarray(np.asarray(cam, np.int32).reshape(-1))
    P = np.asarray(P, float).reshape(-1, 3, 4)
    if n < 0 or xn.ndim != 2 or xn.shape[0] != 2 or xn.shape[1] != rs[-1] or cm.size != xn.shape[1]:
        raise ValueError('%s: xn must be 2-by-total and cam hold total indices, total the end of the last range' % who)
    return n, xn.shape[1], P.shape[0], rs, cm, _f64(xn), _poses_in(P, P.shape[0])


def intersect_ransac(ray_start, cam, xn, P, thr2, smp_start=None, samples=None, use=None, min_angle=0.0, device=0):
    """dbat_hip_intersect_ransac over the points ray_start[i] .. ray_start[i + 1] of cam (total camera indices into P) and
    the columns of xn (2-by-total), with the cameras P (n_cams, 3, 4: [R | -R C]), the thresholds thr2 (one per camera),
    the samples smp_start[i] .. smp_start[i + 1] of the rows of samples (two indices local to the point each; smp_start
    None, or an empty range: every pair of the point, enumerated on the device), the optional mask use (total booleans)
    and min_angle in radians: dict(X (3, n), stats (n, 4: count, sample, hypotheses scored, usable rays), inlier (total),
    ssq (n))."""
    lib = load()
    n, total, nc, rs, cm, xf, Pf = _rays('intersect_ransac', ray_start, cam, xn, P)
    ss = None if smp_start is None else np.ascontiguousarray(smp_start, np.int64)
    smp = np.ascontiguousarray(np.asarray(np.zeros((0, 2)) if samples is None else samples, np.int32).reshape(-1, 2))
    t2 = np.ascontiguousarray(np.broadcast_to(np.asarray(thr2, float), (nc,)))
    if (ss is not None and (len(ss) != n + 1 or smp.shape[0] != ss[-1])) or (ss is None and smp.shape[0] != 0):
        raise ValueError('intersect_ransac: smp_start must hold one range per point and samples be k-by-2, k the end of the last range')
    u = _mask(use, total)
    X, st, ssq, inl = _out(n, 3), _out(n, 4, np.int32), _out(n), _out(total, 1, np.uint8)
    check(lib.dbat_hip_intersect_ransac(int(device), n, _ptr(rs, _lp), _ptr(cm, _ip), dptr(xf), nc, dptr(Pf), _ptr(u, _bp),
                                        _ptr(ss, _lp), _ptr(smp, _ip), dptr(t2), float(min_angle), dptr(X), _ptr(st, _ip),
                                        _ptr(inl, _bp), dptr(ssq)))
    return dict(X=X[:3 * n].reshape(3, n, order='F'), stats=st[:4 * n].reshape(n, 4), inlier=inl[:total].astype(bool), ssq=ssq[:n])


def pointadjust(ray_start, cam, xn, P, X, use=None, w=None, max_iter=20, conv_tol=1e-6, min_angle=0.0, residuals=False, device=0):
    """dbat_hip_pointadjust over the points ray_start[i] .. ray_start[i + 1] of cam and the columns of xn (2-by-total), with
    the cameras P (n_cams, 3, 4), from the start points X (3-by-n); use (total booleans) and the weights w (2-by-total, or
    anything that broadcasts to it) are optional.  Nothing given is changed.  Returns dict(X (3, n), used (total), f0, f,
    sigma0, lam (n), code, iters, trials, n_used (n), Q (n, 3, 3), res (2, total; None unless residuals))."""
    lib = load()
    n, total, nc, rs, cm, xf, Pf = _rays('pointadjust', ray_start, cam, xn, P)
    X = np.asarray(X, float)
    if X.shape != (3, max(n, 0)):
        raise ValueError('pointadjust: X must be 3-by-n, one start per point')
    Xf = np.zeros(3) if n == 0 else X.flatten('F')
    wt, u = _weights(w, total), _mask(use, total)
    used, ds, ist, Q = _out(total, 1, np.uint8), _out(n, 4), _out(n, 4, np.int32), _out(n, 9)
    res = _out(total, 2) if residuals else None
    opt = PairOptions(int(max_iter), float(conv_tol), float(min_angle))
    check(lib.dbat_hip_pointadjust(int(device), n, _ptr(rs, _lp), _ptr(cm, _ip), dptr(xf), nc, dptr(Pf), _ptr(u, _bp), dptr(wt),
                                   C.byref(opt), dptr(Xf), _ptr(used, _bp), dptr(ds), _ptr(ist, _ip), dptr(Q), dptr(res)))
    ds, ist = ds[:4 * n].reshape(n, 4), ist[:4 * n].reshape(n, 4)
    return dict(X=Xf[:3 * n].reshape(3, n, order='F'), used=used[:total].astype(bool), f0=ds[:, 0].copy(), f=ds[:, 1].copy(),
                sigma0=ds[:, 2].copy(), lam=ds[:, 3].copy(), code=ist[:, 0].copy(), iters=ist[:, 1].copy(), trials=ist[:, 2].copy(),
                n_used=ist[:, 3].copy(), Q=Q[:9 * n].reshape(n, 3, 3).transpose(0, 2, 1),
                res=None if res is None else res[:2 * total].reshape(total, 2).T)


def intersect_robust_timing(on=True):
    """Device events around the kernels of intersect_ransac / pointadjust calls on this thread (debug; off by default)."""
    check(load().dbat_hip_debug_intersect_robust_timing(int(bool(on))))


def intersect_robust_ms():
    """Device-event milliseconds of the kernels of the last intersect_ransac and pointadjust calls on this thread, after
    intersect_robust_timing(True) (debug)."""
    return _kernel_ms('intersect_robust', ('ransac', 'adjust'))


def rigidalign(X, Y, scale=False, use=None, resid=False, device=0):
    """dbat_hip_rigidalign over 3-by-n X and Y: (T (4, 4), stats, resid) with stats = dict(alpha, rms, used, sv_ratio) and
    resid 3-by-n (NaN in the columns that are not used) or None."""
    lib = load()
    X, Y = np.asarray(X, float), np.asarray(Y, float)
    if X.ndim != 2 or X.shape[0] != 3 or X.shape != Y.shape:
        raise ValueError('rigidalign: X and Y must both be 3-by-n')
    n = X.shape[1]
    Xf, Yf = _f64(X), _f64(Y)
    u = None
    if use is not None:
        u = np.ascontiguousarray(np.asarray(use, bool).ravel()).view(np.uint8)
        if u.shape[0] != n:
            raise ValueError('rigidalign: use must have one entry per column')
    T, st = np.zeros(16), np.zeros(4)
    r = np.empty(3 * n) if resid else None
    check(lib.dbat_hip_rigidalign(int(device), n, dptr(Xf), dptr(Yf), _ptr(u, _bp), int(bool(scale)), dptr(T), dptr(st), dptr(r)))
    return (T.reshape(4, 4, order='F'), dict(alpha=float(st[0]), rms=float(st[1]), used=int(st[2]), sv_ratio=float(st[3])),
            None if r is None else r.reshape(3, n, order='F'))


def multixform(EO, OP, T, device=0):
    """dbat_hip_multixform: (EO, OP, fail) -- new column-major arrays of the shapes given (EO with six rows or more, the
    rows from the seventh on copied) and the per-camera failure flags."""
    lib = load()
    EO, OP, T = np.asarray(EO, float), np.asarray(OP, float), np.asarray(T, float)
    if T.shape != (4, 4):
        raise ValueError('multixform: T must be 4-by-4')
    EO = np.zeros((6, 0)) if EO.size == 0 else EO
    OP = np.zeros((3, 0)) if OP.size == 0 else OP
    if EO.ndim != 2 or OP.ndim != 2 or (OP.size and OP.shape[0] != 3):
        raise ValueError('multixform: EO must be 6-by-M (or more rows), OP 3-by-N')
    nc, npnt = (EO.shape[1] if EO.size else 0), (OP.shape[1] if OP.size else 0)
    rows = EO.shape[0] if nc else 6
    eo, op = np.array(EO, float, order='F'), np.array(OP, float, order='F')
    fail = _out(nc, 1, np.uint8)
    check(lib.dbat_hip_multixform(int(device), dptr(_f64(T)), nc, int(rows), dptr(eo.reshape(-1, order='F')) if nc else None,
                                  npnt, dptr(op.reshape(-1, order='F')) if npnt else None, _ptr(fail, _bp)))
    return eo, op, fail[:nc].astype(bool)


def align_timing(on=True):
    """Device events around the kernels of rigidalign / multixform calls on this thread (debug; off by default)."""
    check(load().dbat_hip_debug_align_timing(int(bool(on))))


def align_ms():
    """Device-event milliseconds of the kernels of the last rigidalign / multixform call on this thread, after
    align_timing(True) (debug)."""
    return _kernel_ms('align', ('centroid', 'cross', 'resid', 'points', 'cams'))


def plan_layout_stats(s, shard_rank=0, shard_count=1):
    """Host-only: which layout (tiles, signature groups, chunk lengths) the plan gives the problem."""
    lib = load()
    p, keep = problem_from_struct(s, 0, shard_rank, shard_count)
    a = (C.c_int64 * 16)()
    check(lib.dbat_hip_plan_layout_stats(C.byref(p), a))
    v = [int(x) for x in a]
    return dict(n_tiles=v[0], n_batches=v[1], n_batches_tiled=v[2], n_groups=v[3], n_group_points=v[4], n_chunks=v[5],
                chunks_by_length={'1-8': v[6], '9-16': v[7], '17-32': v[8], '33-64': v[9]}, chunks_multi_round=v[10],
                k_max=v[11], rows_max=v[12], build_sig=bool(v[13]), backsub_sig=bool(v[14]), heavy_tasks=v[15])


def plan_digest(s, shard_rank=0, shard_count=1):
    """Host-only (debug): {field: hash} of the whole host plan of this shard -- equal digests mean identical plans."""
    lib = load()
    p, keep = problem_from_struct(s, 0, shard_rank, shard_count)
    out = (C.c_uint64 * 96)()
    names = C.create_string_buffer(4096)
    n = lib.dbat_hip_debug_plan_digest(C.byref(p), out, 96, names, 4096)
    if n < 0:
        check(n)
    return dict(zip(names.value.decode().split(','), [int(v) for v in out[:n]]))


def heavy_plan_selftest(s, shard_rank=0, shard_count=1):
    """Host-only (debug): the row groups / slots / pair tasks of the heavy and giant points (csrc/heavy.hpp) replayed on
    the host against the plain sum of z_p z_p' -- see dbat_hip_debug_heavy_plan_selftest."""
    lib = load()
    p, keep = problem_from_struct(s, 0, shard_rank, shard_count)
    out = np.zeros(8)
    check(lib.dbat_hip_debug_heavy_plan_selftest(C.byref(p), dptr(out)))
    return dict(on=bool(out[0]), points=int(out[1]), row_groups=int(out[2]), tasks=int(out[3]), ksteps=int(out[4]),
                max_diff=float(out[5]), max_abs=float(out[6]), entries=int(out[7]))


def nd_stats(s, mode, shard_rank=0, shard_count=1):
    """Host-only (debug): the nested dissection of the camera graph with the separators of `mode` (csrc/nd.hpp: 0 lower
    boundary at the median, 1 minimum vertex cover at the median, 2 minimum cover with slid cuts) and with the ones the
    model of the factorisation chooses, laid out in tiles and scored on the CPU (dbat_hip_debug_nd_stats).  Returns
    (requested, chosen): cameras, blocks, tile_columns, tiles, chain (longest dependent chain of tile columns), products,
    model_us, mode, valid (the independent check of the order: a permutation, no co-visible pair across a cut), run,
    model ('list schedule' or 'estimate')."""
    lib = load()
    p, keep = problem_from_struct(s, 0, shard_rank, shard_count)
    out = np.zeros(24)
    check(lib.dbat_hip_debug_nd_stats(C.byref(p), int(mode), dptr(out)))
    part = lambda v: dict(cameras=int(v[0]), blocks=int(v[1]), tile_columns=int(v[2]), tiles=int(v[3]), chain=int(v[4]),
                          products=int(v[5]), model_us=float(v[6]), mode=int(v[7]), valid=int(v[8]) == 0, run=int(v[9]),
                          model='estimate' if v[10] else 'list schedule')
    return part(out[:12]), part(out[12:])


def df_schedule(s):
    """Host-only (debug): the task list of the factorisation in the compact tile layout on one rank, as a handle would
    schedule it for this struct (dbat_hip_debug_df_schedule; DBAT_HIP_DF_SUMS and DBAT_HIP_DF_MERGE honoured).  Returns a
    dict: nT, W, jobs (int array [tasks, 8]: i, k, jlo, jhi, part, np, mode, p in task order), plist (the product lists),
    listed_bit (the bit of mode that marks a task whose products are plist[jlo:jhi]), rowbits (uint64 [(nT + 1), W]: bit
    k of row i = tile (i, k) exists), cand_us (modelled microseconds of: column order, sums cut at the merge columns,
    product lists, lists and cut sums; < 0: not made), taken (index into cand_us), nparts, products, chain_role,
    chain_tiles, n_listed."""
    lib = load()
    p, keep = problem_from_struct(s)
    hdr = np.zeros(16, np.int64)
    cand = np.zeros(4)
    null_i, null_u = C.cast(None, _ip), C.cast(None, C.POINTER(C.c_uint64))
    check(lib.dbat_hip_debug_df_schedule(C.byref(p), hdr.ctypes.data_as(_lp), dptr(cand), null_i, 0, null_i, 0, null_u, 0))
    nT, W, nt, nl = (int(v) for v in hdr[:4])
    jobs = np.zeros((max(nt, 1), 8), np.int32)
    plist = np.zeros(max(nl, 1), np.int32)
    rb = np.zeros(((nT + 1), W), np.uint64)
    check(lib.dbat_hip_debug_df_schedule(C.byref(p), hdr.ctypes.data_as(_lp), dptr(cand), jobs.ctypes.data_as(_ip), jobs.size,
                                         plist.ctypes.data_as(_ip), plist.size, rb.ctypes.data_as(C.POINTER(C.c_uint64)), rb.size))
    return dict(nT=nT, W=W, jobs=jobs[:nt], plist=plist[:nl], listed_bit=int(hdr[10]), rowbits=rb, cand_us=[float(v) for v in cand],
                taken=int(hdr[4]), nparts=int(hdr[5]), products=int(hdr[6]), chain_role=bool(hdr[7]), chain_tiles=int(hdr[8]),
                n_listed=int(hdr[9]))


def batch_stats(s, shard_rank=0, shard_count=1):
    """Host-only (debug): the sizes of the plan's batches (dbat_hip_debug_batch_stats).  'tiled' and 'untiled' (the
    batches after the tiles: heavy points, or every batch when nothing is tiled): the most points and the most
    observations of one batch, the batches closed by the point cap PMAX rather than by BT, the most batches of one tile;
    then BT, PMAX, the plan's cap of batches per tile and the number of batches of either kind."""
    lib = load()
    p, keep = problem_from_struct(s, 0, shard_rank, shard_count)
    a = (C.c_int64 * 16)()
    check(lib.dbat_hip_debug_batch_stats(C.byref(p), a))
    v = [int(x) for x in a]
    part = lambda q: dict(max_points=v[q], max_obs=v[q + 1], closed_by_cap=v[q + 2], max_tile_batches=v[q + 3])
    return dict(tiled=part(0), untiled=part(4), BT=v[8], PMAX=v[9], tile_bmax=v[10], n_batches_tiled=v[11],
                n_batches_untiled=v[12])


def plan_domain_map(s, shard_count):
    """Host-only: (cam_owner, subtree) -- the rank whose domain every image belongs to (-1: top separator) under
    domain sharding with shard_count ranks, and whether the problem is sharded that way at all."""
    lib = load()
    p, keep = problem_from_struct(s, 0, 0, shard_count)
    owner = np.full(s.EO.val.shape[1], -1, np.int32)
    sub = C.c_int32(0)
    check(lib.dbat_hip_plan_domain_map(C.byref(p), owner.ctypes.data_as(_ip), C.byref(sub)))
    return owner, bool(sub.value)


def plan_serialize(s):
    """Host-only x0 = serialize(s) (no GPU needed)."""
    lib = load()
    p, keep = problem_from_struct(s)
    x0 = np.empty(plan(s)['n'])
    check(lib.dbat_hip_plan_serialize(C.byref(p), dptr(x0)))
    return x0


def debug_model_eval_host(model, nK, nP, EO6, IO, px, Q, uv):
    """Host evaluation of csrc/model.hpp for CPU unit tests of the closed form."""
    lib = load()
    R = 5 + nK + nP
    r, A, B, Cc = np.zeros(2), np.zeros(12), np.zeros(6), np.zeros(2 * R)
    a = [np.ascontiguousarray(v, float) for v in (EO6, IO, Q, uv)]
    check(lib.dbat_hip_debug_model_eval_host(model, nK, nP, dptr(a[0]), dptr(a[1]), float(px),
                                             dptr(a[2]), dptr(a[3]), dptr(r), dptr(A), dptr(B), dptr(Cc)))
    return r, A.reshape(6, 2).T, B.reshape(3, 2).T, Cc.reshape(R, 2).T


def _coverage_call(fn, nc, no):
    lo, hi = np.zeros(2 * max(nc, 1)), np.zeros(2 * max(nc, 1))
    rad, area = np.zeros(max(nc, 1)), np.zeros(max(nc, 1))
    rip, hs, hip = np.zeros(max(nc, 1), np.int64), np.zeros(nc + 1, np.int64), np.zeros(max(no, 1), np.int64)
    lp = lambda a: a.ctypes.data_as(_lp)
    check(fn(dptr(lo), dptr(hi), dptr(rad), lp(rip), dptr(area), lp(hs), lp(hip)))
    return dict(lo=lo[:2 * nc].reshape(2, nc, order='F'), hi=hi[:2 * nc].reshape(2, nc, order='F'), rad_max=rad[:nc],
                rad_ip=rip[:nc], hull_area=area[:nc], hull=[hip[hs[c]:hs[c + 1]].copy() for c in range(nc)])


def quality_hull_cap():
    """Candidates of one image that the coverage kernel sorts in LDS (QUAL_HULL_CAP)."""
    return int(load().dbat_hip_quality_hull_cap())


def debug_coverage_host(s):
    """Host evaluation of dbat_hip_coverage over the struct's own values with the kernel's code (no GPU needed): the
    dict of Handle.coverage()."""
    lib = load()
    p, keep = problem_from_struct(s)
    return _coverage_call(lambda *a: lib.dbat_hip_debug_coverage_host(C.byref(p), *a), int(p.n_images), int(p.n_obs))


def debug_ray_angles_host(s):
    """Host evaluation of the definition of dbat_hip_ray_angles over the struct's own values (no GPU needed):
    (op, cam) in radians."""
    lib = load()
    p, keep = problem_from_struct(s)
    op, cam = np.zeros(max(int(p.n_points), 1)), np.zeros(max(int(p.n_images), 1))
    check(lib.dbat_hip_debug_ray_angles_host(C.byref(p), dptr(op), dptr(cam)))
    return op[:int(p.n_points)], cam[:int(p.n_images)]
