"""`bundle()` -- host-side mirror of DBAT's bundle driver over the HIP core.

Mirrors `bundle/bundle.m:1-132` (argument conventions), `:156-192` (set-up),
`:267-358` (dispatch on damping, result struct E, deserialise only if ok) and
`:449-491` (residual scatter, sigma0); the post-mortem of a rank-deficient
design matrix (`:368-446`) is in dbat_amd.diagnose.  All arithmetic of the path --
residuals, Jacobian blocks, normal equations, Schur solve, damping loops --
runs in libdbat_hip.so through the C ABI of include/dbat_hip.h; nothing here
computes them on the CPU.
"""
from __future__ import annotations

import copy
import time
import types

import numpy as np

from . import _hip, diagnose
from .dbatstruct import share_struct

NS = types.SimpleNamespace


class BadInput(ValueError):
    """error('DBAT:bundle:badInput', ...)  (bundle.m:124,130)."""


def _parse_args(args):
    """bundle.m:78-132: integer => maxIter, non-integer scalar => tol, string =>
    damping / flags, logical => chirality veto."""
    o = dict(maxIter=20, damping='gna', veto=False, singularTest=True, doTrace=False,
             dofVerb=False, pmDof=False, absTerm=False, convTol=1e-6)
    for a in args:
        if isinstance(a, (bool, np.bool_)):
            o['veto'] = bool(a)
        elif isinstance(a, (int, float, np.integer, np.floating)):
            if float(a) == round(float(a)):
                o['maxIter'] = int(a)
            else:
                o['convTol'] = float(a)
        elif isinstance(a, str):
            la = a.lower()
            if la in ('none', 'gm', 'gna', 'lm', 'lmp'):
                o['damping'] = la
            elif la == 'trace':
                o['doTrace'] = True
            elif la == 'singulartest':
                o['singularTest'] = True
            elif la == 'nosingulartest':
                o['singularTest'] = False
            elif la == 'pmdof':
                o['pmDof'] = True
            elif la == 'dofverb':
                o['dofVerb'] = True
            elif la == 'absterm':
                o['absTerm'] = True
            else:
                raise BadInput('DBAT:bundle:badInput: Unknown damping')
        else:
            raise BadInput('DBAT:bundle:badInput: Unknown parameter')
    return o


MAD_C = 1.1774100225154747          # sqrt(2 ln 2): the median of a chi_2-distributed norm (robust scale 'mad')
ROBUST_K = {'huber': 1.5, 'cauchy': 2.385}


def robust_weight_fn(u, loss, k):
    """The weight factor omega(u) in (0, 1] of the robust losses (u = s / scale >= 0): Huber 1 for u <= k, else k / u;
    Cauchy 1 / (1 + (u / k)^2).  Host statement of what dbat_hip_solve_robust applies on the device."""
    u = np.asarray(u, float)
    if loss == 'huber':
        return np.where(u <= k, 1.0, k / np.where(u <= k, 1.0, u))
    if loss == 'cauchy':
        t = u / k
        return 1.0 / (1.0 + t * t)
    raise BadInput("robust: unknown loss '%s' (None, 'huber' or 'cauchy')" % (loss,))


def _robust_args(robust, robust_k, robust_scale, robust_max_outer, robust_tol):
    """Checks bundle()'s robust arguments (before any device work): None or (loss, k, scale, max_outer, tol)."""
    if robust is None:
        return None
    if not isinstance(robust, str) or robust.lower() not in ROBUST_K:
        raise BadInput("bundle: robust must be None, 'huber' or 'cauchy', not %r" % (robust,))
    loss = robust.lower()
    k = ROBUST_K[loss] if robust_k is None else robust_k
    if isinstance(k, bool) or not isinstance(k, (int, float, np.integer, np.floating)) or not np.isfinite(k) or k <= 0:
        raise BadInput('bundle: robust_k must be a positive finite number, not %r' % (robust_k,))
    if not isinstance(robust_scale, str) or robust_scale.lower() not in _hip.SCALE:
        raise BadInput("bundle: robust_scale must be 'apriori' or 'mad', not %r" % (robust_scale,))
    if (isinstance(robust_max_outer, bool) or not isinstance(robust_max_outer, (int, np.integer))
            or not 1 <= robust_max_outer < _hip.ROBUST_MAX_OUTER):
        raise BadInput('bundle: robust_max_outer must be an integer in [1, %d], not %r'
                       % (_hip.ROBUST_MAX_OUTER - 1, robust_max_outer))
    if (isinstance(robust_tol, bool) or not isinstance(robust_tol, (int, float, np.integer, np.floating))
            or not np.isfinite(robust_tol) or robust_tol < 0):
        raise BadInput('bundle: robust_tol must be a finite number >= 0, not %r' % (robust_tol,))
    return loss, float(k), robust_scale.lower(), int(robust_max_outer), float(robust_tol)


def bundle(s, *args, device=None, comm=None, store_trace=True, jacobian=False, deterministic=False,
           term_fun=None, veto_fun=None, reuse_handle=True, robust=None, robust_k=None, robust_scale='apriori',
           robust_max_outer=10, robust_tol=1e-3, min_depth=0.0):
    """[s,ok,iters,s0,E] = bundle(s[,maxIter][,damping][,'trace'][,tol]
    [,'absterm'][,'singulartest'|'nosingulartest'][,veto][,'pmdof'][,'dofverb'])

    `comm` (dbat_amd.parallel.Comm) shards the object points over the ranks of
    a torch.distributed group, one GPU per rank; every rank returns the full
    result.  `store_trace=False` drops E.trace (n x iterations) for very large
    problems.  `deterministic=True` sums the reduced system in a fixed order (dbat_hip_set_deterministic:
    two runs give the same bits; slower; signature-group path only).  `jacobian=True` also returns E.final.weighted.J and E.final.unweighted.J
    (scipy CSC, bundle.m:341-350) -- on request only, the solver never forms J.
    `term_fun(Jp, r) -> bool` replaces the termination test bundle() builds (bundle.m:186-192) and `veto_fun(x) -> bool`
    is the veto the lsa solvers call at every trial point (bundle.m:168-172 only ever passes the undefined `chirality`):
    the two function handles of the reference's solver interface, for callers that used the solvers directly.
    `reuse_handle=False` builds (and destroys) a handle of its own instead of using the cached one (_hip.acquire).
    The returned struct shares the arrays bundle() does not change (IP.*, masks, blocks) with its input.

    The logical `veto` argument turns the chirality veto on (bundle.m:125-127; the reference's own `chirality` is
    undefined, bundle.m:169): the damping loops reject a trial point at which some object point is not in front of a
    camera that sees it -- depth <= `min_depth`, the depths of point_depths() -- with the consequences of a veto_fun
    that returns true.  The test runs on the device (dbat_hip_set_chirality).  E.chirality is then True and E.veto holds
    tested, rejected (trial points) and n_behind, min_depth of the last rejected one.  'gm' has no trial points.  Not
    with `comm` of several ranks, not with `robust=`.

    Robust estimation (iteratively reweighted least squares over the image points, dbat_hip_solve_robust):
    `robust='huber' | 'cauchy'` down-weights image points with large residuals.  Per outer step the weight factor
    omega of every IP column comes from u = s / scale, s the norm of its two residuals weighted by IP.std, scale 1
    (`robust_scale='apriori'`) or median(s) / sqrt(2 ln 2) ('mad'); robust_weight_fn gives omega(u) (`robust_k`:
    default 1.5 / 2.385).  Both rows then have the sigma IP.std / sqrt(omega).  The loop solves with omega = 1,
    then reweights and solves again from the result until max |omega' - omega| <= `robust_tol` or
    `robust_max_outer` reweightings; code, iterations, sigma0 and the trace are the last solve's.  E.robust holds
    loss, k, scale_mode, scale (per reweighting evaluation), weights (omega per IP column), outer (solves),
    converged, inner_iters, max_change, downweighted (IP columns with omega < 0.5, by omega ascending) and
    reweight_time.  The robust loop takes no term_fun / veto_fun and prints no live 'trace'.
    """
    ro = _robust_args(robust, robust_k, robust_scale, robust_max_outer, robust_tol)
    if ro is not None and (term_fun is not None or veto_fun is not None):
        raise BadInput('bundle: robust=... takes no term_fun / veto_fun')
    o = _parse_args(args)
    if (isinstance(min_depth, bool) or not isinstance(min_depth, (int, float, np.integer, np.floating))
            or not np.isfinite(min_depth)):
        raise BadInput('bundle: min_depth must be a finite number, not %r' % (min_depth,))
    if o['veto']:
        # bundle.m:169 references an undefined function `chirality`; here: every point in
        # front of every camera that sees it, tested on the device
        if ro is not None:
            raise BadInput('bundle: the chirality veto is not combined with robust=...')
        if comm is not None and comm.world_size > 1:
            raise BadInput('bundle: the chirality veto runs on one-rank handles only (comm with %d ranks)' % comm.world_size)
    s = share_struct(s)          # (namespaces copied, arrays shared: nothing below writes into an array of the input)
    # bundle.m:137-154: a fixed parameter cannot be used as a prior observation
    for nm in ('IO', 'EO', 'OP'):
        pr = getattr(s.prior, nm)
        est = np.asarray(getattr(s.bundle.est, nm), bool)
        pr.use = np.asarray(pr.use, bool)
        if np.any(pr.use & ~est):
            print("Warning: Some %s parameters are set to both 'fixed' and 'observed'" % nm)
            print('Setting %s parameters to fixed' % nm)
            pr.use = pr.use & est
    rank, world = (comm.rank, comm.world_size) if comm is not None else (0, 1)
    if jacobian and world > 1:
        raise BadInput('bundle(..., jacobian=True): the explicit Jacobian (E.final.*.J) is built by one-rank handles only')
    if device is None:
        # a rank of a multi-GPU run works on the device its process selected
        device = getattr(comm, 'device', None) if comm is not None else 0
        device = 0 if device is None else device
    # Plan reuse (bundle.m:156-159 keeps s.bundle.serial / deserial between calls): one-rank runs take the cached handle
    # when the structure of s -- everything but the parameter and prior values -- is the one it was built for
    # (_hip.acquire: dbat_hip_structure_key + dbat_hip_set_values); a changed mask, block or observation builds a new plan.
    cached = world == 1 and reuse_handle
    t_host = [time.perf_counter()]
    h = _hip.acquire(s, device) if cached else _hip.Handle(s, device=device, shard_rank=rank, shard_count=world)
    t_host.append(time.perf_counter())
    done = False
    try:
        if deterministic:                                            # fixed-order sums: bit-identical runs (parity mode)
            h.set_deterministic(True)
        if world == 1:
            h.set_chirality(o['veto'], float(min_depth))             # (every call: a cached handle keeps no setting)
        if comm is not None and world > 1:
            if hasattr(comm, 'attach'):
                comm.attach(h)                                       # RCCL communicator inside the library
            else:
                h.set_allreduce(comm.allreduce_ptr)                  # test hook
        x0 = h.serialize()                                           # bundle.m:162
        opt = _hip.default_options(o['damping'])
        opt.max_iter = o['maxIter']
        opt.conv_tol = o['convTol']
        opt.abs_term = int(o['absTerm'])
        opt.singular_test = int(o['singularTest'])
        opt.store_trace = int(bool(store_trace))
        # 'trace': the solver's own line per iteration, printed while the loop runs (gauss_newton_armijo.m:119-128 ...)
        live = (lambda *a: print(_hip.trace_text(*a), flush=True)) if o['doTrace'] and rank == 0 else None
        if ro is None:
            x, res, rr, damp, aux, T = h.solve(x0, opt, term_fun=term_fun, veto_fun=veto_fun, trace_fun=live)   # complete on every rank of a sharded run
        else:
            ropt = _hip.robust_options(ro[0], ro[1], ro[2], ro[3], ro[4])
            x, res, rr, damp, aux, T, rres, omega = h.solve_robust(x0, opt, ropt)
        t_host.append(time.perf_counter())
        E = NS(maxIter=o['maxIter'], convTol=o['convTol'], absTerm=o['absTerm'],
               singularTest=o['singularTest'], chirality=o['veto'], veto=None)
        if o['veto']:
            E.veto = NS(**dict(zip(('tested', 'rejected', 'n_behind', 'min_depth'), h.chirality_stats())))
        name = 'gm' if o['damping'] in ('none', 'gm') else o['damping']
        if name == 'gm':
            E.damping = NS(name='gm')
        elif name == 'gna':
            E.damping = NS(name='gna', alpha=damp, mu=opt.mu, alphaMin=opt.alpha_min)
        elif name == 'lm':
            E.damping = NS(name='lm', **{'lambda': damp},
                           lambda0=damp[0] if len(damp) else np.nan,
                           lambdaMin=damp[0] if len(damp) else np.nan)
        else:
            mi = o['maxIter']
            rho = aux[:mi + 2]
            rho = rho[~np.isnan(rho)]
            step = aux[mi + 2:]
            step = step[~np.isnan(step)].astype(int)
            E.damping = NS(name='lmp', delta=damp, rho=rho, delta0=float(np.linalg.norm(x0)),
                           rhoBad=opt.rho_bad, rhoGood=opt.rho_good, step=step)
        E.res, E.trace, E.time = rr, T, res.time_s
        E.robust = None
        if ro is not None:
            n_eval = rres.outer - 1 + rres.converged
            low = np.flatnonzero(omega < 0.5)
            E.robust = NS(loss=ro[0], k=ro[1], scale_mode=ro[2], scale=np.array(rres.scale[:n_eval]), weights=omega,
                          outer=int(rres.outer), converged=bool(rres.converged),
                          inner_iters=np.array(rres.inner_iters[:rres.outer]), max_change=float(rres.max_change),
                          downweighted=low[np.argsort(omega[low], kind='stable')], reweight_time=float(rres.reweight_s))
        # where it went (hipEvent stage timers of the library), the E.time of bundle.m:287-294 by stage
        E.timeStages = dict(zip(('linearise', 'factor_solve', 'backsub', 'residual', 'other'), [float(v) for v in res.stage_s]))
        E.code, E.usedIters = int(res.code), int(res.iters)
        E.counters = NS(residual_evals=res.n_residual_evals, linearizations=res.n_linearizations,
                        solves=res.n_solves)
        ok = E.code == 0
        if ok:                                                       # bundle.m:356-358
            IO, EO, OP = h.deserialize(x)
            s.IO.val, s.OP.val = IO, OP
            s.EO.val = np.vstack([EO, s.EO.val[6:]]) if s.EO.val.shape[0] > 6 else EO
        # residuals at the last linearisation point (bundle.m:449-460)
        # (code -4 stops after the first linearisation: the residual is that of x0,
        # gauss_newton_armijo.m:112-142, and sigma0 below is computed from it)
        ru, rw = h.final_residuals()
        no = s.IP.val.shape[1]
        s.post = getattr(s, 'post', NS())
        s.post.res = NS()
        px = np.asarray(s.IO.sensor.pxSize)
        if px.shape[1] == 1 or not (px != px[:, :1]).any():          # one pixel size for every camera: no 2 x nObs gather
            s.post.res.IP = ru[:2 * no].reshape(2, no, order='F') / px[:, :1]
        else:
            s.post.res.IP = ru[:2 * no].reshape(2, no, order='F') / px[:, s.IP.cam]
        IOix, EOix, OPix = h.index_maps()
        for nm, arr in _place_prior_rows(s, (IOix, EOix, OPix), ru[2 * no:]).items():
            setattr(s.post.res, nm, arr)
        E.final = NS(unweighted=NS(r=ru), weighted=NS(r=rw))
        if jacobian and E.code != -4:
            E.final.weighted.J = h.jacobian_csc(x, True)
            E.final.unweighted.J = h.jacobian_csc(x, False)
        p_extra = 0
        if o['pmDof']:                                               # bundle.m:467-471
            seen_pt = np.zeros(s.OP.val.shape[1], bool); seen_pt[s.IP.pt] = True
            seen_cam = np.zeros(s.EO.val.shape[1], bool); seen_cam[s.IP.cam] = True
            p_extra = int(np.count_nonzero(~np.asarray(s.bundle.est.OP, bool)[:, seen_pt])
                          + np.count_nonzero(~np.asarray(s.bundle.est.EO, bool)[:6, seen_cam]))
        dof = h.m + p_extra - h.n
        # bundle.m:476-483: sqrt(r'r/dof) of the weighted residual (finite for m == n with 'pmdof')
        s0 = float(np.sqrt(rw @ rw / dof)) if dof > 0 else np.nan
        if o['dofVerb']:
            print('bundle: dof=%d+%d-%d=%d.' % (h.m, p_extra, h.n, dof))
        s.post.sigmas = s0 * np.asarray(s.IP.sigmas)
        # sensor format updated by the estimated aspect (bundle.m:360-366)
        aspect = np.ones((2, s.IO.val.shape[1])); aspect[0] = 1.0 + s.IO.val[3]
        if hasattr(s.IO.sensor, 'imSize'):               # structs built without image sizes have no format to update
            s.post.sensor = type(s.post)(imSize=np.array(s.IO.sensor.imSize, float), pxSize=s.IO.sensor.pxSize * aspect,
                                          ssSize=s.IO.sensor.imSize * s.IO.sensor.pxSize * aspect)
        E.numObs, E.numParams, E.redundancy, E.s0 = h.m, h.n, dof, s0
        E.sigmas = s.post.sigmas
        E.x = x
        # post-mortem of a rank-deficient design matrix (bundle.m:368-446)
        maps = (IOix, EOix, OPix)
        E.paramTypes = diagnose.param_types(s, maps, h.n)
        E.weakness = NS(structural=None, numerical=NS(rank=h.n, deficiency=0))
        if E.code == -2:
            E.weakness.numerical = NS(rank=float('nan'), deficiency=float('nan'), suspectedParams=[])
            if world == 1:
                E.weakness.numerical = diagnose.numerical_weakness(
                    diagnose.weighted_jacobian(h, s, x), E.paramTypes)
        elif E.code == -4:
            E.weakness.structural = diagnose.structural_weakness(s, maps, h.n, E.paramTypes)
            E.weakness.numerical = NS(rank=float('nan'), deficiency=float('nan'))
        done = True
        # where the wall time of this call went on the host: the handle (a plan and its uploads, or -- a cached handle of
        # the same structure -- the key and the new values), the solve (E.time of it inside the damping loop), the result
        E.timeHost = dict(handle=t_host[1] - t_host[0], solve=t_host[2] - t_host[1], result=time.perf_counter() - t_host[2],
                          handle_reused=bool(cached and _hip.cache_stats.get('last') == 'hit'))
        return s, ok, E.usedIters, s0, E
    finally:
        if cached:
            _hip.release(h, keep=done)                               # (after an exception: destroyed, not kept)
        else:
            h.close()


def _place_prior_rows(s, maps, vals):
    """The prior rows of a residual-like vector (vals: the rows after the 2 x nObs image rows) placed in the val
    layout of IO, EO (first six rows) and OP: {'IO': ..., 'EO': ..., 'OP': ...}, NaN where there is no prior row."""
    out, ofs = {}, 0
    for nm, ixmap in zip(('IO', 'EO', 'OP'), maps):
        val = getattr(s, nm).val
        rows = slice(0, 6) if nm == 'EO' else slice(None)
        use = np.asarray(getattr(s.prior, nm).use, bool)[rows]
        arr = np.full(val[rows].shape, np.nan)
        if not use.any():                                            # no prior observation of this kind: nothing to place
            out[nm] = arr                                            # (the leading-element map below sorts 3 x points entries)
            continue
        # prior rows = column-major order of use & leading (buildserialindices.m:138-139,200)
        flatmap = ixmap.flatten('F')
        lead = np.zeros(flatmap.shape, bool)
        valid = np.flatnonzero(flatmap >= 0)
        _, first = np.unique(flatmap[valid], return_index=True)
        lead[valid[first]] = True
        pos = np.flatnonzero(use.flatten('F') & lead)
        flat = arr.flatten('F')
        flat[pos] = vals[ofs:ofs + len(pos)]
        ofs += len(pos)
        out[nm] = flat.reshape(arr.shape, order='F')
    return out


CXX_MAX_N = 6000       # unknowns up to which bundle_cov offers the dense matrices 'CXX' / 'COPF' (288 MB)


def bundle_cov(s, E, *names, device=0):
    """C = bundle_cov(s, E, 'CIO' | 'CEO' | 'COP' | 'CIOF' | 'CEOF', ...)
    (bundle/bundle_cov.m:1-31): sigma0^2 times blocks of inv(J'J) at the
    bundle result (s, E) as scipy sparse matrices of size numel(val) x
    numel(val), zero-padded for elements that were not estimated; 'CIO',
    'CEO', 'COP' keep the per-column diagonal blocks only (:9-16), 'CIOF' and
    'CEOF' are the full component matrices.  The blocks come from the device
    (dbat_hip_posterior_cov: Schur pieces and a selected inversion of the compact
    factor); this function only scatters them.
    'CXX' (n x n, not zero-padded) and 'COPF' (3np x 3np) are dense by nature
    ("may require a lot of memory", bundle_cov.m:24): offered up to CXX_MAX_N
    unknowns -- the sizes the reference's own callers use them at -- from the
    weighted Jacobian of the device (dbat_hip_jacobian_csc) by one dense
    factorisation on the host, as bundle_cov.m:63-117 does it in MATLAB."""
    import scipy.sparse as sp
    names = [n.lower() for n in names]
    for n in names:
        if n not in ('cio', 'ceo', 'cop', 'ciof', 'ceof', 'cxx', 'copf'):
            raise BadInput("Bad covariance string '%s'" % n)          # bundle_cov.m:53-55
    if not names:
        return None
    dense = [n for n in names if n in ('cxx', 'copf')]
    h = _hip.acquire(s, device)          # the handle bundle() left behind, with the values of its result: one plan for both
    done = False
    try:
        _reapply_weights(h, E)
        if dense and h.n > CXX_MAX_N:
            raise BadInput("bundle_cov: '%s' is an n x n dense matrix and n = %d (offered up to %d unknowns; "
                           "'CIO', 'CEO', 'COP' give the blocks at any size)" % (dense[0].upper(), h.n, CXX_MAX_N))
        CXX = None
        if dense:
            J = h.jacobian_csc(np.asarray(E.x, float), True)
            N = (J.T @ J).toarray()
            import scipy.linalg as sla
            c, low = sla.cho_factor(N, lower=True)           # (fails loudly if J'J is not positive definite)
            CXX = float(E.s0) ** 2 * sla.cho_solve((c, low), np.eye(N.shape[0]))
        blocks = [n for n in names if n not in dense]
        res = None
        if blocks:
            full = any(n.endswith('f') for n in blocks)
            res = h.posterior_cov(np.asarray(E.x, float), float(E.s0), want_sinv=full)
            CEOb, CIOu, COPb = res[:3]
        ixIO, ixEO, ixOP = h.index_maps()                   # x index of every array entry, -1 = no unknown
        nc = s.EO.val.shape[1]
        done = True
    finally:
        _hip.release(h, keep=done)
    out = []
    for n in names:
        if n == 'cxx':
            out.append(CXX)
            continue
        if n == 'copf':                                      # zero-padded: rows / columns of coordinates that are not estimated
            ix = ixOP.flatten('F')
            est = np.flatnonzero(ix >= 0)
            D = np.zeros((ix.size, ix.size))
            D[np.ix_(est, est)] = CXX[np.ix_(ix[est], ix[est])]
            out.append(sp.csc_matrix(D))
            continue
        comp = n[1:3].upper()
        val = getattr(s, comp).val
        m, ncol = val.shape
        if n == 'cop':
            r = np.arange(3)
            rows = (3 * np.arange(ncol)[:, None, None] + r[None, :, None]) + 0 * r[None, None, :]
            cols = (3 * np.arange(ncol)[:, None, None] + r[None, None, :]) + 0 * r[None, :, None]
            C = sp.csc_matrix((COPb.ravel(), (rows.ravel(), cols.ravel())), shape=(val.size, val.size))
        elif n == 'ceo':
            r = np.arange(6)
            rows = (m * np.arange(ncol)[:, None, None] + r[None, :, None]) + 0 * r[None, None, :]
            cols = (m * np.arange(ncol)[:, None, None] + r[None, None, :]) + 0 * r[None, :, None]
            C = sp.csc_matrix((CEOb.ravel(), (rows.ravel(), cols.ravel())), shape=(val.size, val.size))
        else:
            # IO (shared blocks: several array entries map to one unknown) and the full matrices:
            # entry (a, b) of the result = covariance of the unknowns behind array entries a and b
            ix = (ixIO if comp == 'IO' else ixEO).flatten('F')
            if comp == 'IO':
                M, off = CIOu * 1.0, 0
                src = ix                                     # x index == IO unknown index (IO comes first in x)
            else:
                Sinv = res[3]
                M, off = float(E.s0) ** 2 * Sinv[:6 * nc, :6 * nc], 0
                # EO entry e of the array <-> z index: row r of image c -> 6c + r (rows 0..5)
                src = np.where(ix >= 0, (np.arange(val.size) % m) + 6 * (np.arange(val.size) // m), -1)
                src = np.where((np.arange(val.size) % m) < 6, src, -1)
            if n == 'ciof' and len(res) > 3:
                M = float(E.s0) ** 2 * res[3][6 * nc:, 6 * nc:]
            est = np.flatnonzero(src >= 0)
            D = np.zeros((val.size, val.size))
            if len(est):
                D[np.ix_(est, est)] = M[np.ix_(src[est] - off, src[est] - off)]
            if not n.endswith('f'):
                D *= np.kron(np.eye(ncol), np.ones((m, m)))
            C = sp.csc_matrix(D)
        out.append(C)
    return out[0] if len(out) == 1 else tuple(out)


R_EPS = 1e-12          # redundancy numbers at or below this: an uncontrolled observation (w, T undefined, mdb infinite)


def reliability_critical(alpha0=0.001, beta0=0.80):
    """Critical values of data snooping: the chi^2(2) quantile 1 - alpha0 (the 2-dof test per image point,
    -2 ln alpha0 in closed form), the two-sided normal quantile 1 - alpha0/2 and the non-centrality
    delta0 = z(1 - alpha0/2) + z(beta0) of the minimal detectable blunder (4.13 for 0.001 / 0.80)."""
    from statistics import NormalDist
    if not (0 < alpha0 < 1 and 0 < beta0 < 1):
        raise BadInput('bundle_reliability: alpha0 and beta0 must lie in (0, 1)')
    z = NormalDist()
    normal = z.inv_cdf(1.0 - alpha0 / 2.0)
    return NS(alpha0=float(alpha0), beta0=float(beta0), chi2_2=float(-2.0 * np.log(alpha0)), normal=float(normal),
              delta0=float(normal + z.inv_cdf(beta0)))


def reliability_stats(s, rw, qvv, r_prior, maps, alpha0=0.001, beta0=0.80, omega=None):
    """The statistics of bundle_reliability from the pieces of Qvv = I - J inv(J'J) J' (pure host function).
    rw       (m,) weighted residuals (E.final.weighted.r)
    qvv      (3, nObs) r_u, q_uv, r_v of every image point (IP column order)
    r_prior  (m - 2 nObs,) redundancy numbers of the prior rows, in the row order of rw
    maps     (IOix, EOix, OPix) x index of every IO / EO / OP entry, -1 = not an unknown (Handle.index_maps)
    omega    (nObs,) weight factors of a robust bundle (E.robust.weights) or None: the MDB uses IP.std / sqrt(omega)
    Returns the struct bundle_reliability documents."""
    rw = np.asarray(rw, float)
    no = s.IP.val.shape[1]
    qvv = np.asarray(qvv, float).reshape(3, no)
    r_prior = np.asarray(r_prior, float).ravel()
    if rw.size != 2 * no + r_prior.size:
        raise BadInput('reliability_stats: %d residual rows, %d image and %d prior rows' % (rw.size, 2 * no, r_prior.size))
    crit = reliability_critical(alpha0, beta0)
    ru, quv, rv = qvv
    rIP = np.vstack([ru, rv])
    v = rw[:2 * no].reshape(2, no, order='F')
    ok = rIP > R_EPS
    sq = np.sqrt(np.where(ok, rIP, 1.0))
    w = np.where(ok, v / sq, np.nan)
    std = np.broadcast_to(np.asarray(s.IP.std, float), (2, no))
    if omega is not None:
        std = std / np.sqrt(np.asarray(omega, float).reshape(1, no))
    mdb = np.where(ok, crit.delta0 * std / sq, np.inf)
    # T = v' Qvv^-1 v, chi^2(2) under H0 (a singular 2 x 2 block: undefined)
    det = ru * rv - quv * quv
    okT = ok[0] & ok[1] & (det > R_EPS * ru * rv)
    dets = np.where(okT, det, 1.0)
    T = np.where(okT, (rv * v[0] ** 2 - 2.0 * quv * v[0] * v[1] + ru * v[1] ** 2) / dets, np.nan)
    vp = rw[2 * no:]
    okp = r_prior > R_EPS
    wp = np.where(okp, vp / np.sqrt(np.where(okp, r_prior, 1.0)), np.nan)
    rpl = _place_prior_rows(s, maps, r_prior)
    wpl = _place_prior_rows(s, maps, wp)
    out = NS(r=np.concatenate([rIP.flatten('F'), r_prior]),
             IP=NS(r=rIP, q_uv=quv, w=w, T=T, mdb=mdb),
             IO=NS(r=rpl['IO'], w=wpl['IO']), EO=NS(r=rpl['EO'], w=wpl['EO']), OP=NS(r=rpl['OP'], w=wpl['OP']),
             critical=crit)
    out.total = float(out.r.sum())
    sel = np.flatnonzero(np.nan_to_num(T, nan=-np.inf) > crit.chi2_2)
    sel = sel[np.argsort(-T[sel], kind='stable')]
    op_id = getattr(s.OP, 'id', None)
    pt = np.asarray(s.IP.pt)[sel]
    out.suspects = NS(ip=sel, op_id=np.asarray(op_id)[pt] if op_id is not None else pt,
                      image=np.asarray(s.IP.cam)[sel], T=T[sel], w_u=w[0, sel], w_v=w[1, sel])
    return out


def bundle_reliability(s, E, alpha0=0.001, beta0=0.80, device=0):
    """Internal reliability of the adjustment at E.x, the last linearisation point of bundle(s, ...) (prior sigma0 = 1:
    independent of the estimated sigma0).  The hat-matrix blocks come from the device (dbat_hip_redundancy: the Schur
    pieces of the posterior covariance and a selected inversion of the compact factor), on the handle bundle() left
    behind; this function only forms the statistics (reliability_stats).  Fields:
      r         (m,) redundancy numbers r_i = 1 - h_ii, row order of E.final.weighted.r; sum = m - n
      IP        r (2, nObs), q_uv (nObs,) the off-diagonal of Qvv, w (2, nObs) standardized residuals v / sqrt(r),
                T (nObs,) v' Qvv^-1 v of every image point (chi^2(2) under H0), mdb (2, nObs) minimal detectable
                blunder delta0 sigma / sqrt(r) in pixels (IP.std); NaN / inf where r <= 1e-12
      IO, EO, OP  r and w of the prior rows in the val layout of s.post.res.IO / EO / OP, NaN where there is no prior
      total     sum of r
      critical  alpha0, beta0, chi2_2 (chi^2(2) quantile 1 - alpha0), normal (normal quantile 1 - alpha0/2), delta0
      suspects  image points with T > chi2_2 by T descending: ip (IP column), op_id, image (EO column), T, w_u, w_v
    A bundle that stopped on a singular design matrix (E.code == -4) has no reliability: BadInput."""
    if int(getattr(E, 'code', 0)) == -4:
        raise BadInput('bundle_reliability: the bundle stopped on a singular design matrix (code -4); '
                       'redundancy numbers need J\'J positive definite')
    crit = reliability_critical(alpha0, beta0)        # (bad levels fail before any device work)
    h = _hip.acquire(s, device)          # the handle bundle() left behind, with the values of its result
    done = False
    try:
        rob = _reapply_weights(h, E)
        qvv, rp = h.redundancy(np.asarray(E.x, float))
        maps = h.index_maps()
        done = True
    finally:
        _hip.release(h, keep=done)
    return reliability_stats(s, E.final.weighted.r, qvv, rp, maps, crit.alpha0, crit.beta0,
                             omega=None if rob is None else rob.weights)


def ray_angles(s, E=None, device=0):
    """Ray intersection angles of the network in s, from the device (dbat_hip_ray_angles) on the handle bundle() left
    behind -- the point angles of photogrammetry/angles.m and the image angles of photogrammetry/camangles.m at any
    size, without the dense visibility table.  Evaluated at the values in s (E, the bundle's result struct, is accepted
    so that the call reads like bundle_cov's; the angles depend on s.EO.val and s.OP.val alone).  Fields:
      op        (nOP,) largest angle [rad] between two rays of every object point; 0 for one ray, NaN for none
      cam       (nImages,) largest angle [rad] between two rays of every image; 0 for one point, NaN for none
      op_rays   (nOP,) rays of every object point        cam_rays  (nImages,) points measured in every image"""
    h = _hip.acquire(s, device)
    done = False
    try:
        op, cam, op_rays, cam_rays = h.ray_angles(h.serialize())
        done = True
    finally:
        _hip.release(h, keep=done)
    return NS(op=op, cam=cam, op_rays=op_rays, cam_rays=cam_rays)


def point_depths(s, E=None, device=0):
    """Depth of every object point with respect to every camera that sees it, from the device (dbat_hip_point_depths) on
    the handle bundle() left behind -- photogrammetry/pm_multidepth.m with pointdepth.m / ptdepth.m, sign chosen so
    that a point in front of the camera has a positive depth.  Evaluated at the values in s (E is accepted so that the
    call reads like ray_angles').  Fields:
      depth      (nObs,) depth of every IP column
      n_behind   IP columns with !(depth > 0): a NaN depth counts        behind  those columns, ascending
      min_depth  smallest depth (NaN if none is a number)                argmin  smallest IP column that attains it (-1)
      image_min  (nImages,) smallest depth per image, NaN for an image without points
    This is what the chirality veto of bundle(s, True) tests at every trial point."""
    h = _hip.acquire(s, device)
    done = False
    try:
        depth, image_min, n_behind, min_depth, argmin = h.point_depths(h.serialize(), 0.0)
        done = True
    finally:
        _hip.release(h, keep=done)
    return NS(depth=depth, n_behind=n_behind, behind=np.flatnonzero(~(depth > 0)), min_depth=min_depth, argmin=argmin,
              image_min=image_min)


def _corner_radius(s, i):
    """Largest distance of an image corner to the principal point of image i, mm (coverage.m:140-147 as
    report._coverage restates it)."""
    px, pp, im = s.IO.sensor.pxSize[:, i], s.IO.val[1:3, i], s.IO.sensor.imSize[:, i]
    xx, yy = np.array([0.5, im[0] + 0.5]), np.array([0.5, im[1] + 0.5])
    cu, cv = xx[[0, 0, 1, 1]], yy[[0, 1, 1, 0]]
    return np.sqrt((cu * px[0] - pp[0]) ** 2 + (-cv * px[1] - pp[1]) ** 2).max()


def _hull_area_of(pts):
    """Vertices (indices into the 2-by-n points, counter-clockwise from the lowest (u, v), strictly extreme) and area
    of the convex hull of a small point set on the host: the monotone chain and the shoelace sum relative to the
    minimum, as the device kernel forms them."""
    n = pts.shape[1]
    order = sorted(range(n), key=lambda i: (pts[0, i], pts[1, i], i))
    order = [i for k, i in enumerate(order) if k == 0 or (pts[:, i] != pts[:, order[k - 1]]).any()]
    if len(order) < 3:
        return order, 0.0

    def half(seq):
        h = []
        for i in seq:
            while len(h) >= 2:
                a, b = pts[:, h[-2]], pts[:, h[-1]]
                if (b[0] - a[0]) * (pts[1, i] - a[1]) - (b[1] - a[1]) * (pts[0, i] - a[0]) <= 0:
                    h.pop()
                else:
                    break
            h.append(i)
        return h
    h = half(order)[:-1] + half(order[::-1])[:-1]
    if len(h) < 3:
        return h, 0.0
    q = pts[:, h] - pts.min(1, keepdims=True)
    return h, 0.5 * float(np.sum(q[0] * np.roll(q[1], -1) - np.roll(q[0], -1) * q[1]))


def network_quality(s, E=None, device=0):
    """Image coverage and marking-residual statistics of the network in s, from the device (dbat_hip_coverage,
    dbat_hip_residual_stats) on the handle bundle() left behind -- photogrammetry/coverage.m and the "Point Marking
    Residuals" block of the result file at any size, without the dense visibility table.  Evaluated at the values in s.
      coverage   per image: lo, hi (2, nImages), rad_ip, hull (list of IP-column arrays, counter-clockwise, the closing
                 point not repeated), hull_area [px^2], rad_max [mm], points; with s.IO.sensor.imSize also the
                 fractions c (convex hull), cr (rectangular), crr (radial) of coverage.m -- NaN for an image without
                 points, as coverage.m leaves them
      coverage_union(cams) -> (c, cr, crr, lo, hi, hull_area) for the images cams together (coverage.m, union=true:
                 image size and principal point of the first one; 0 where none has points), from the per-image
                 results alone: the hull over the per-image hull vertices
      residuals  rms, max, max_ip, op_rms, op_rays, cam_rms, cam_points (pixels; NaN for a zero count)"""
    h = _hip.acquire(s, device)
    done = False
    try:
        cov = h.coverage()
        st = h.residual_stats(h.serialize())
        done = True
    finally:
        _hip.release(h, keep=done)
    nc = s.EO.val.shape[1]
    have_im = hasattr(s.IO.sensor, 'imSize')
    cam_n = st['cam_n']
    c = NS(lo=cov['lo'], hi=cov['hi'], rad_ip=cov['rad_ip'], rad_max=cov['rad_max'], hull=cov['hull'],
           hull_area=cov['hull_area'], points=cam_n)
    if have_im:
        tot = np.prod(np.asarray(s.IO.sensor.imSize, float), 0)
        some = cam_n > 0
        c.c = np.where(some, cov['hull_area'] / tot, np.nan)
        with np.errstate(invalid='ignore'):
            c.cr = np.where(some, np.prod(cov['hi'] - cov['lo'], 0) / tot, np.nan)
            c.crr = np.where(some, cov['rad_max'] / np.array([_corner_radius(s, i) for i in range(nc)]), np.nan)
    uv = np.asarray(s.IP.val, float)

    def coverage_union(cams):
        cams = np.asarray(cams, np.int64).ravel()
        used = cams[cam_n[cams] > 0]
        if len(used) == 0:
            return (0.0, 0.0, 0.0, np.full(2, np.nan), np.full(2, np.nan), 0.0)
        i = int(cams[0])
        lo, hi = cov['lo'][:, used].min(1), cov['hi'][:, used].max(1)
        cols = np.concatenate([cov['hull'][k] for k in used])
        area = _hull_area_of(uv[:, cols])[1]
        if not have_im:
            return (np.nan, np.nan, np.nan, lo, hi, area)
        # the largest radius about the FIRST image's principal point: a maximum of a convex function over the points
        # is attained at a vertex of their hull, so the per-image hull vertices suffice
        px, pp = s.IO.sensor.pxSize[:, i], s.IO.val[1:3, i]
        rad = np.sqrt((uv[0, cols] * px[0] - pp[0]) ** 2 + (-uv[1, cols] * px[1] - pp[1]) ** 2).max()
        tot = float(np.prod(s.IO.sensor.imSize[:, i]))
        return (area / tot, float(np.prod(hi - lo)) / tot, rad / _corner_radius(s, i), lo, hi, area)

    no = int(cam_n.sum())
    with np.errstate(divide='ignore', invalid='ignore'):
        res = NS(rms=float(np.sqrt(st['total_ss'] / no)) if no else np.nan, max=st['max_e'], max_ip=st['max_ip'],
                 op_rms=np.sqrt(st['op_ss'] / st['op_n']), op_rays=st['op_n'],
                 cam_rms=np.sqrt(st['cam_ss'] / cam_n), cam_points=cam_n)
    return NS(coverage=c, coverage_union=coverage_union, residuals=res)


def _call(fn, *a, **kw):
    """fn(*a, **kw) with the library's DBAT_HIP_EINVAL, and the binding's complaints about shapes, as BadInput."""
    try:
        return fn(*a, **kw)
    except _hip.DbatHipError as e:
        if e.code == _hip.EINVAL:
            raise BadInput(str(e)) from e
        raise
    except ValueError as e:
        raise BadInput(str(e)) from e


def rigidalign(X, Y, scale=False, use=None, device=0):
    """[T,R,d,alpha] = rigidalign(X, Y, scale) (misc/rigidalign.m) for 3-by-n point sets, the sums on the device
    (dbat_hip_rigidalign): the rigid-body (scale=False: alpha = 1) or similarity transformation that minimises
    sum |alpha R x_i + d - y_i|^2, T = [alpha R, d; 0 0 0 1].  `use` (n booleans) restricts the sum to some columns;
    the others may hold anything.  BadInput for fewer than three used columns, a used column that is not finite, and
    points that are collinear (rigidalign.m returns an arbitrary rotation for those)."""
    T, st, _ = _call(_hip.rigidalign, X, Y, scale, use=use, device=device)
    alpha = st['alpha']
    return T, T[:3, :3] / alpha, T[:3, 3].copy(), alpha


def multixform(EO, OP, T, device=0):
    """[EO,OP,fail] = pm_multixform(EO, OP, T) (photogrammetry/pm_multixform.m) on the device (dbat_hip_multixform): the
    similarity T applied to the object points OP (3-by-N) and the camera stations EO (6- or 7-by-M: centre, omega, phi,
    kappa; rows from the seventh on are left as they are).  Either array may be empty.  fail (M booleans) marks the
    cameras whose values are not finite; they stay as they are.  The angles are those of the rotation M' R' -- the
    reference takes them from M' R' / alpha.  BadInput for a T that is not a similarity."""
    return _call(_hip.multixform, EO, OP, T, device=device)


def multialign(EO, OP, i, ra=0.0, device=0):
    """[EO,OP,T] = pm_multialign(EO, OP, i, ra) (photogrammetry/pm_multialign.m:19-24): camera i to the origin, looking
    down the negative z axis with roll angle ra, T = [RA' M' [I, -C]; 0 0 0 1] applied through multixform."""
    from .initial import rotmat3d
    EO = np.asarray(EO, float)
    if EO.ndim != 2 or EO.shape[0] < 6 or not 0 <= int(i) < EO.shape[1]:
        raise BadInput('multialign: EO must be 6-by-M (or 7-by-M) and i one of its columns')
    T = np.eye(4)
    T[:3, :3] = rotmat3d([0.0, 0.0, -float(ra)]).T @ rotmat3d(EO[3:6, int(i)])      # RA' M'
    T[:3, 3] = -T[:3, :3] @ EO[:3, int(i)]
    EO2, OP2, _ = multixform(EO, OP, T, device=device)
    return EO2, OP2, T


def _similarity_parts(T):
    T = np.asarray(T, float)
    if T.shape != (4, 4) or not np.all(np.isfinite(T)):
        raise BadInput('T must be a finite 4-by-4 matrix')
    det = np.linalg.det(T[:3, :3])
    if not det > 0:
        raise BadInput('T(1:3,1:3) is not a scaled proper rotation')
    alpha = float(np.cbrt(det))
    return T, alpha, T[:3, :3] / alpha


def transform_network(s, T, device=0):
    """The network of s in another coordinate system: a struct copy with EO.val[:6] and OP.val transformed by the
    similarity T (multixform, on the device), prior.OP.val and the position rows of prior.EO.val transformed where
    their `use` is set, and the prior standard deviations of positions multiplied by the scale alpha of T.  The
    interior orientation and the image points are untouched (shared with s).
    BadInput when the rotation of T differs from the identity by more than 1e-12 and either some used prior standard
    deviation is anisotropic within a column (a column used only in part is) or some angle prior is in use: neither
    keeps its meaning under a rotation."""
    T, alpha, R = _similarity_parts(T)
    pOP, pEO = s.prior.OP, s.prior.EO
    if np.abs(R - np.eye(3)).max() > 1e-12:
        if np.any(pEO.use[3:6]):
            raise BadInput('transform_network: a prior observation of an Euler angle does not keep its meaning under a rotation')
        for name, use, std in (('OP', pOP.use, pOP.std), ('EO', pEO.use[:3], pEO.std[:3])):
            some = np.any(use, 0)
            if np.any(some & ~np.all(use, 0)) or np.any(std[:, some] != std[:1, some]):
                raise BadInput('transform_network: prior.%s has a column with anisotropic standard deviations; '
                               'they do not keep their meaning under a rotation' % name)
    s2 = share_struct(s)
    eo, op, _ = multixform(s.EO.val, s.OP.val, T, device=device)
    s2.EO.val, s2.OP.val = eo, op
    # the prior positions go through the device as points: entries that are not in use (NaN as a rule) are held out
    npnt = pOP.val.shape[1]
    pv = np.concatenate([pOP.val, pEO.val[:3]], 1)
    pu = np.concatenate([pOP.use, pEO.use[:3]], 1)
    if pu.any():
        _, q, _ = multixform(np.zeros((6, 0)), np.where(pu, pv, 0.0), T, device=device)
        pv = np.where(pu, q, pv)
    s2.prior.OP.val = np.asfortranarray(pv[:, :npnt])
    s2.prior.OP.std = np.asfortranarray(pOP.std * alpha)
    ev, es = np.array(pEO.val, float, order='F'), np.array(pEO.std, float, order='F')
    ev[:3] = pv[:, npnt:]
    es[:3] *= alpha
    s2.prior.EO.val, s2.prior.EO.std = ev, es
    return s2


def align_network(s, ref_OP, use=None, scale=True, device=0):
    """Brings the network of s onto reference coordinates: ref_OP is 3-by-nOP with NaN columns for the points that
    have none.  The similarity (scale=False: rigid-body transformation) is fitted from s.OP.val to ref_OP over the
    columns that are finite in both and set in `use` (rigidalign) and applied to the whole struct
    (transform_network).  Returns (s2, T, fit) with fit.alpha, fit.rms, fit.used, fit.resid (3-by-nOP: alpha R x + d - y,
    NaN where the column is not used), fit.max and fit.argmax (the largest residual norm and its column)."""
    ref = np.asarray(ref_OP, float)
    if ref.shape != s.OP.val.shape:
        raise BadInput('align_network: ref_OP must be 3-by-nOP')
    ok = np.all(np.isfinite(s.OP.val), 0) & np.all(np.isfinite(ref), 0)
    if use is not None:
        ok &= np.asarray(use, bool).ravel()
    T, st, resid = _call(_hip.rigidalign, s.OP.val, ref, scale, use=ok, resid=True, device=device)
    s2 = transform_network(s, T, device=device)
    nrm = np.where(ok, np.sqrt(np.sum(np.where(ok, resid, 0.0) ** 2, 0)), -1.0)
    k = int(np.argmax(nrm))
    return s2, T, NS(alpha=st['alpha'], rms=st['rms'], used=st['used'], resid=resid, max=float(nrm[k]), argmax=k)


def _reapply_weights(h, E):
    """A robust bundle's weight factors on an acquired handle (acquire() -> set_values restored the base weights):
    covariance and redundancy then describe the final reweighted system.  Returns E.robust."""
    rob = getattr(E, 'robust', None)
    if rob is not None:
        h.set_obs_weights(rob.weights)
    return rob
