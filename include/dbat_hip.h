/*
 * dbat_hip.h -- C ABI of the MI355X-native damped bundle-adjustment core.
 *
 * Drop-in boundary for the hot path of niclasborlin/dbat (MATLAB):
 *   bundle()  ->  lsa/{gauss_markov,gauss_newton_armijo,levenberg_marquardt,
 *                      levenberg_marquardt_powell}.m
 *             ->  resFun = brown_euler_cam4(x,s)  (residual + sparse Jacobian)
 *             ->  (J'*J [+lambda*I]) \ (-J'*r)
 *
 * The reference has no FFI for this path; the seam it replaces is the MATLAB
 * function-handle contract between bundle.m and lsa/ *.m plus the DBAT struct
 * (SURVEY.md section 8(b)).  Every entry point cites the reference interface
 * it stands in for (paths relative to /root/reference/code/).
 *
 * Conventions
 *   - plain C types only; all arrays are caller-owned HOST memory unless a
 *     name ends in _dev; double arrays are column-major like MATLAB's;
 *     indices are 0-based int32 (int64 where a count can exceed 2^31).
 *   - every function returns 0 on success or a negative DBAT_HIP_E* code;
 *     dbat_hip_last_error() gives the message.  Numerical failure of an
 *     adjustment is NOT an error return: it is reported through
 *     dbat_hip_result.code (0,-1,-2,-3,-4) exactly as the reference's
 *     solvers do (gauss_newton_armijo.m:38-46).
 *   - one handle per calling thread; a handle owns its device memory and its
 *     HIP stream.  No call is re-entrant on the same handle.
 *   - all device arithmetic is IEEE double.
 */
#ifndef DBAT_HIP_H
#define DBAT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DBAT_HIP_ABI_VERSION 5   /* 5: dbat_hip_redundancy; additive: dbat_hip_robust_weights / dbat_hip_set_obs_weights / dbat_hip_solve_robust, dbat_hip_intersect_ransac / dbat_hip_pointadjust; 4: dbat_hip_options grew (trace_fun); dbat_hip_structure_key / dbat_hip_handle_key / dbat_hip_set_values; dbat_hip_bench_step ms[16], dbat_hip_info [24]; 3: dbat_hip_options grew (term_fun, veto_fun); 2: dbat_hip_result grew (stage_s, n_trace_only); dbat_hip_info [16]; dbat_hip_bench_step ms[12] */

/* error returns */
#define DBAT_HIP_OK            0
#define DBAT_HIP_EINVAL       -101  /* bad argument / inconsistent struct (DBAT:bundle:badInput) */
#define DBAT_HIP_EUNSUPPORTED -102  /* struct uses a feature outside the hot path */
#define DBAT_HIP_EDEVICE      -103  /* HIP / rocSOLVER failure */
#define DBAT_HIP_ENOMEM       -104

/* damping names of bundle.m:98-101 */
#define DBAT_HIP_DAMP_GM   0   /* 'none' / 'gm'  -> lsa/gauss_markov.m */
#define DBAT_HIP_DAMP_GNA  1   /* 'gna'           -> lsa/gauss_newton_armijo.m */
#define DBAT_HIP_DAMP_LM   2   /* 'lm'            -> lsa/levenberg_marquardt.m */
#define DBAT_HIP_DAMP_LMP  3   /* 'lmp'           -> lsa/levenberg_marquardt_powell.m */

typedef struct dbat_hip_handle dbat_hip_handle;

/*
 * The DBAT struct fields read by the hot path (misc/prob2dbatstruct.m:12-186;
 * list in SURVEY.md 8(b)).  nIOrows = 5+nK+nP.
 */
typedef struct dbat_hip_problem {
    int32_t abi_version;        /* DBAT_HIP_ABI_VERSION */
    int32_t n_images;           /* size(s.EO.val,2) */
    int32_t n_points;           /* size(s.OP.val,2) */
    int64_t n_obs;              /* size(s.IP.val,2) */
    int32_t dist_model;         /* unique(s.IO.model.distModel): 2,3,4 or 5 (brown_euler_cam4.m:122-130) */
    int32_t nK, nP;             /* s.IO.model.nK, .nP */

    /* image observations, image-major, ascending OP inside an image
     * (prob2dbatstruct.m:343-365; multi_res.m:126-135) */
    const int32_t *ip_cam;      /* s.IP.cam - 1          [n_obs] */
    const int32_t *ip_pt;       /* OP column of each IP column (find(s.IP.vis)) [n_obs] */
    const double  *ip_val;      /* s.IP.val  2 x n_obs, pixels */
    const double  *ip_std;      /* s.IP.std  2 x n_obs, pixels (buildweightmatrix.m:16-20) */

    const double  *IO_val;      /* s.IO.val  nIOrows x n_images */
    const double  *px_size;     /* s.IO.sensor.pxSize 2 x n_images */
    const double  *EO_val;      /* s.EO.val(1:6,:) 6 x n_images */
    const double  *OP_val;      /* s.OP.val  3 x n_points */

    const uint8_t *est_IO;      /* s.bundle.est.IO nIOrows x n_images */
    const uint8_t *est_EO;      /* s.bundle.est.EO 6 x n_images */
    const uint8_t *est_OP;      /* s.bundle.est.OP 3 x n_points */
    const int32_t *IO_block;    /* s.IO.struct.block nIOrows x n_images */
    const int32_t *EO_block;    /* s.EO.struct.block 6 x n_images (shared elements -- camera stations -- take the column-list kernels) */

    /* prior observations (lsa/prior_obs.m:26-72; buildweightmatrix.m:25-29) */
    const uint8_t *prior_IO_use; const double *prior_IO_val; const double *prior_IO_std;
    const uint8_t *prior_EO_use; const double *prior_EO_val; const double *prior_EO_std;
    const uint8_t *prior_OP_use; const double *prior_OP_val; const double *prior_OP_std;

    int32_t device;             /* HIP device ordinal this handle runs on */
    int32_t shard_rank;         /* object-point shard owned by this handle ... */
    int32_t shard_count;        /* ... of shard_count (1 = whole problem) */
} dbat_hip_problem;

/* options = the varargin of bundle() (bundle.m:78-132) plus the constants
 * bundle.m hard-codes for each damping scheme (:281-283, :301-304, :321-325). */
/* The caller's own tests, as bundle() hands them to the lsa solvers (bundle.m:168-192):
 *   termFun(Jp, r) -> logical  (gauss_newton_armijo.m:187-191, levenberg_marquardt.m:217, levenberg_marquardt_powell.m:134-140):
 *       Jp = J*p and r, both weighted, n_residuals rows in the reference's row order; != 0 ends the iteration (code 0);
 *   vetoFun(x) -> logical  (gauss_newton_armijo.m:268-271, levenberg_marquardt.m:170-173, levenberg_marquardt_powell.m:146-166):
 *       x = the trial point (n_params, reference order); != 0 rejects it.
 * NULL (the default): the built-in tests of bundle.m:186-192 on ||Jp|| and ||r|| -- no vectors leave the device -- and no veto.
 * With a termFun every termination test costs one pass for J*p, one for r and their copies to the host. */
typedef int32_t (*dbat_hip_term_fn)(void *user, const double *Jp, const double *r, int64_t n_residuals);
typedef int32_t (*dbat_hip_veto_fn)(void *user, const double *x, int64_t n_params);
/* 'trace' (bundle.m:82): called INSIDE the damping loop, at the statement where the lsa solver prints its line
 * (gauss_newton_armijo.m:119-128, gauss_markov.m:74-76, levenberg_marquardt.m:138-147, levenberg_marquardt_powell.m:160-164):
 * iteration n, residual norm rr(end), the damping quantity the line shows (GNA: the last alpha, LM: lambda, LMP: delta;
 * NaN where the reference prints none: GNA's and LM's iteration 0, Gauss-Markov), and for LMP the step type
 * (0 GN, 1 IP, 2 CP; -1 otherwise) and the gain ratio rho (NaN otherwise).  NULL: nothing is reported before the loop returns. */
typedef void (*dbat_hip_trace_fn)(void *user, int32_t damping, int32_t iter, double res_norm, double damp, int32_t step_type, double rho);

typedef struct dbat_hip_options {
    int32_t damping;        /* DBAT_HIP_DAMP_* ; default GNA (bundle.m:79) */
    int32_t max_iter;       /* 20   (bundle.m:78) */
    double  conv_tol;       /* 1e-6 (bundle.m:86) */
    int32_t abs_term;       /* 'absterm' (bundle.m:185-192) */
    int32_t singular_test;  /* 'singulartest' (bundle.m:81) */
    int32_t store_trace;    /* keep every iterate (E.trace); costs n*(iters+1) doubles of host memory */
    double  mu;             /* GNA Armijo constant 0.1 (bundle.m:281) */
    double  alpha_min;      /* GNA shortest step 1e-9 (bundle.m:283) */
    double  lambda0;        /* LM: -1e-10 => 1e-10*trace(J'J)/n (bundle.m:301; levenberg_marquardt.m:88-95) */
    double  lambda_min;     /* LM: = lambda0 (bundle.m:304) */
    double  rho_bad;        /* LMP 0.25 (bundle.m:321) */
    double  rho_good;       /* LMP 0.75 (bundle.m:322) */
    double  delta0;         /* LMP: <=0 => norm(x0) (bundle.m:325) */
    dbat_hip_term_fn term_fun;  /* NULL: bundle.m:186-192 */
    void   *term_user;
    dbat_hip_veto_fn veto_fun;  /* NULL: no veto (bundle.m:168-172; the reference's own 'chirality' is undefined) */
    void   *veto_user;
    dbat_hip_trace_fn trace_fun; /* NULL: no live trace lines */
    void   *trace_user;
} dbat_hip_options;

/* what the lsa solvers return: [x,code,n,final,T,rr,extra...]
 * (gauss_newton_armijo.m:1-2, levenberg_marquardt.m:1-2,
 *  levenberg_marquardt_powell.m:1-2, gauss_markov.m:1) */
typedef struct dbat_hip_result {
    int32_t code;           /* 0 ok, -1 too many iterations, -2 singular normal matrix,
                               -3 no alpha found, -4 structurally rank deficient */
    int32_t iters;          /* n */
    int32_t n_res;          /* #entries written to res[]  (rr) */
    int32_t n_damp;         /* #entries written to damp[] (alphas / lambdas / deltas) */
    int32_t n_trace;        /* #columns written to trace (T) */
    double  sigma0;         /* sqrt(r'*r/(m-n)) at the last linearisation point (bundle.m:476-483) */
    double  time_s;         /* wall seconds inside the damping loop (E.time, bundle.m:287-294) */
    int32_t n_residual_evals;   /* residual-only evaluations (line search / trial points) */
    int32_t n_linearizations;   /* residual+Jacobian+normal-equation builds */
    int32_t n_solves;           /* reduced-system factorisations */
    int32_t n_trace_only;       /* linearisations taken for trace(J'J) alone (LM's first: no reduced system formed) */
    /* Where the time went (the E.time of bundle.m:287-294, by stage): seconds of the handle's stream between
     * hipEvents recorded where a stage is enqueued -- each interval runs to the next stage's first kernel, so
     * it includes whatever wait for the host follows the stage.  [0] linearisation (residual + Jacobian blocks
     * + J'J + Schur complement), [1] factorisation + solve of the reduced system, [2] back-substitution +
     * step norms, [3] residual-only evaluations (line search / trial points), [4] everything else inside the
     * loop (iterate gathers for the trace, set-up copies). */
    double  stage_s[5];
} dbat_hip_result;

const char *dbat_hip_last_error(void);
int  dbat_hip_abi_version(void);

/* default options for a damping scheme (bundle.m:78-86,281-283,301-304,321-325) */
int  dbat_hip_default_options(int32_t damping, dbat_hip_options *opt);

/* ---- set-up: replaces buildserialindices / serialize / buildweightmatrix --- */

/* Host-only part of create(): index maps and sizes, no GPU needed.
 * misc/buildserialindices.m:69-159 (x order [IO;EO;OP], leading elements of
 * parameter blocks, residual row ranges). */
int  dbat_hip_plan(const dbat_hip_problem *prob, int64_t *n_params, int64_t *n_residuals,
                   int64_t *n_io, int64_t *n_eo, int64_t *n_op,
                   int64_t *shard_pt_lo, int64_t *shard_pt_hi);

/* Host-only: the structural rank test of the damping loops at iteration 0
 * (sprank(J) < size(J,2) => code -4; gauss_newton_armijo.m:132-142,
 * levenberg_marquardt.m:126-135, levenberg_marquardt_powell.m:113-122), decided
 * by a maximum matching of the unknowns to the rows of J.  No GPU needed. */
int  dbat_hip_plan_structural_rank_ok(const dbat_hip_problem *prob, int32_t *ok);

/* Host-only: owner[p] = rank (0..prob->shard_count-1) whose shard holds object
 * point p (contiguous ranges of the spatially sorted processing order,
 * balanced by observation count).  prob->shard_rank is ignored. */
int  dbat_hip_plan_point_owner(const dbat_hip_problem *prob, int32_t *owner /*[n_points]*/);

/* Host-only x0 = serialize(s) straight from the problem description
 * (misc/serialize.m:14-18 over the indices of buildserialindices.m); x0 has
 * n_params entries (see dbat_hip_plan).  No GPU needed. */
int  dbat_hip_plan_serialize(const dbat_hip_problem *prob, double *x0);

/* Build the device problem: uploads observations, builds the point-major
 * batches, weights (buildweightmatrix.m:13-43) and index maps.
 * Replaces bundle.m:156-175. */
int  dbat_hip_create(const dbat_hip_problem *prob, dbat_hip_handle **out);
void dbat_hip_destroy(dbat_hip_handle *h);

/* Plan reuse.  The reference re-enters bundle() from any s at no set-up cost: the indices of
 * buildserialindices.m are kept in s.bundle.serial / deserial and only rebuilt when missing (bundle.m:156-159),
 * deserialize.m:31-46 puts any x back into the same struct.  Here the set-up is the plan and its uploads
 * (dbat_hip_create); a handle is re-used for another problem of the SAME STRUCTURE:
 *   dbat_hip_structure_key   host only: 128 bits over everything a plan depends on -- sizes, lens model, ip_cam, ip_pt,
 *                            ip_val, ip_std, px_size, the est_* masks, IO_block / EO_block, the prior_*_use masks, shard_rank /
 *                            shard_count, device and the DBAT_HIP_* switches of the environment.  NOT part of it: IO_val,
 *                            EO_val, OP_val, prior_*_val, prior_*_std.
 *   dbat_hip_handle_key      the key of the problem a handle was created from.
 *   dbat_hip_set_values      new IO_val / EO_val / OP_val and prior values / standard deviations into the handle (its
 *                            serialize() then returns the new x0; a fixed interior orientation with new values has its
 *                            corrected image coordinates recomputed); every state of an earlier solve is dropped.
 *                            DBAT_HIP_EINVAL, and the handle untouched, if the key of prob differs from the handle's:
 *                            a changed mask, block, visibility or observation needs a new handle.
 * One-rank handles and the handles of a sharded run alike (the communicator stays attached). */
int  dbat_hip_structure_key(const dbat_hip_problem *prob, uint64_t *key /*[2]*/);
int  dbat_hip_handle_key(const dbat_hip_handle *h, uint64_t *key /*[2]*/);
int  dbat_hip_set_values(dbat_hip_handle *h, const dbat_hip_problem *prob);

int64_t dbat_hip_num_params(const dbat_hip_handle *h);      /* s.bundle.serial.n */
int64_t dbat_hip_num_residuals(const dbat_hip_handle *h);   /* s.post.res.ix.n */

/* x0 = serialize(s)  (misc/serialize.m:14-18) */
int  dbat_hip_serialize(const dbat_hip_handle *h, double *x /*[n]*/);
/* s = deserialize(s,x)  (misc/deserialize.m:28-30): full IO/EO/OP arrays */
int  dbat_hip_deserialize(const dbat_hip_handle *h, const double *x,
                          double *IO /*nIOrows x nc*/, double *EO /*6 x nc*/, double *OP /*3 x np*/);
/* structural rank test done by the solvers at n==0 (gauss_newton_armijo.m:132-142):
 * 1 = full structural rank, 0 = deficient (code -4). Host only. */
int  dbat_hip_structural_rank_ok(const dbat_hip_handle *h, int32_t *ok);

/* ---- resFun: r = resFun(x) and [r,J] = resFun(x) ------------------------ */

/* r = brown_euler_cam4(x,s) (brown_euler_cam4.m:122-148; multi_res.m:20-55;
 * prior_obs.m:26-43).  r_unweighted [n_residuals] in the reference row order
 * [image rows; IO priors; EO priors; OP priors] (may be NULL);
 * f = 0.5*r'*W*r (gauss_newton_armijo.m:253).  Collective on a sharded handle
 * (every rank calls it and receives the whole vector and the whole f). */
int  dbat_hip_residual(dbat_hip_handle *h, const double *x, double *r_unweighted, double *f);

/* [r,J] = resFun(x), J returned as the per-observation blocks the sparse J is
 * made of (multi_res.m:138-294): for IP column k (reference order)
 *   JEO[12k..] = d r_k / d EO(1:6,cam)   2x6 column-major
 *   JOP[6k..]  = d r_k / d OP(:,pt)      2x3
 *   JIO[2*nIOrows*k..] = d r_k / d IO(:,cam)  2 x nIOrows
 * unweighted, fixed parameters included (the caller applies est masks and
 * block sharing).  Any output may be NULL.  For bundle_cov / parity tests. */
int  dbat_hip_jacobian_blocks(dbat_hip_handle *h, const double *x,
                              double *JEO, double *JOP, double *JIO);

/* ---- normal equations + solve: (J'*J [+lambda*I]) \ (-J'*r) ------------- */

/* One linearisation at x and one solve:
 *   scale_columns=1 : p = D*((D*J'*J*D) \ -(D*J'*r)), D = diag(1/||J(:,j)||)
 *                     (gauss_newton_armijo.m:166-174; levenberg_marquardt_powell.m:267-279)
 *   scale_columns=0 : p = (J'*J + lambda*I) \ (-J'*r)   (levenberg_marquardt.m:119; gauss_markov.m:79)
 * computed by Schur-complement elimination of the object-point blocks.
 * p [n] in x order.  stats[8] = { f=0.5 r'r, ||J p||^2, r'Jp, ||p||^2,
 * trace(J'J), singular flag, the estimate (min pivot / max pivot)^2 the flag is taken from (CHOLMOD's rcond;
 * 0 after a failed factorisation), the factorisation's info (> 0: first non-positive pivot, index in
 * the factorised order) }.  Jp/stats may be NULL. */
int  dbat_hip_linearize_solve(dbat_hip_handle *h, const double *x, double lambda,
                              int32_t scale_columns, double *p, double *stats);

/* g = J'*r at the last linearisation point, x order (levenberg_marquardt.m:82) */
int  dbat_hip_gradient(dbat_hip_handle *h, double *g);
/* Jn = sqrt(sum(J.^2,1)) at the last linearisation point (gauss_newton_armijo.m:166) */
int  dbat_hip_colnorms(dbat_hip_handle *h, double *Jn);
/* ||J*v||^2 at the last linearisation point (Jp, dog-leg g'J'Jg: lmp.m:304-311) */
int  dbat_hip_jtimes_sqnorm(dbat_hip_handle *h, const double *v, double *sqnorm);
/* J*v itself at the last linearisation point: n_residuals weighted rows in the reference's row order (image rows, then the
 * prior rows) -- the vector termFun(Jp, r) of bundle.m:186-192 / gauss_newton_armijo.m:187 receives; a caller with a
 * termination test of its own runs the loop through dbat_hip_linearize_solve and evaluates it on this (the built-in loops
 * only need ||Jp||: dbat_hip_jtimes_sqnorm).  One-rank handles only. */
int  dbat_hip_jtimes(dbat_hip_handle *h, const double *v, double *Jv);

/* The same for a SAMPLE of the image observations -- n IP columns ip_col[i] (0-based, reference order) -- so that
 * the model of a problem with 10^7 ... 10^8 observations can be checked without exporting 12 doubles for each:
 * res[2n] the unweighted residual [mm] (multi_res.m:20-55), JEO[12n], JOP[6n], JIO[2*nIOrows*n] laid out as in
 * dbat_hip_jacobian_blocks but indexed by i.  One-rank handles only. */
int  dbat_hip_jacobian_sample(dbat_hip_handle *h, const double *x, int64_t n, const int64_t *ip_col, double *res,
                              double *JEO, double *JOP, double *JIO);

/* J = [image rows; IO prior rows; EO prior rows; OP prior rows] at x as a compressed-sparse-column matrix of
 * n_residuals x n_params -- what [r,J]=resFun(x) returns (brown_euler_cam4.m:163-182, multi_res.m:300-313) and
 * bundle() hands on as E.final.weighted.J / E.final.unweighted.J (bundle.m:341-350; bundle_cov.m:18-23,68 reads
 * it for 'CXX' / 'COPF').  On request only: the solver itself never forms J.  The 2x6 / 2x3 / 2xnIO blocks come
 * from the device (the kernel of dbat_hip_jacobian_blocks), the assembly is a counting sort on the host.
 * weighted != 0: rows scaled by 1/sigma (chol(W) J, gauss_newton_armijo.m:104,116).
 * Two calls: with colptr == NULL only *nnz is set; then colptr [n_params+1] (int64), rowidx [nnz] (int64, ascending
 * inside a column), val [nnz].  One-rank handles only (DBAT_HIP_EUNSUPPORTED on a sharded one). */
int  dbat_hip_jacobian_csc(dbat_hip_handle *h, const double *x, int32_t weighted, int64_t *nnz,
                           int64_t *colptr, int64_t *rowidx, double *val);

/* ---- the damping loops (host control flow, device arithmetic) ----------- */

/* [x,code,n,final,T,rr,extra] = <solver>(resFun,vetoFun,x0,W,maxIter,termFun,...)
 * dispatched on opt->damping as bundle.m:267-338 does.
 *   x      [n]  in: x0, out: final estimate
 *   res    [max_iter+3]   rr
 *   damp   [2*max_iter+4] alphas (GNA) / lambdas (LM) / deltas (LMP)
 *   aux    [2*max_iter+4] LMP: rhos then (offset max_iter+2) step types; may be NULL
 *   trace  [n*(max_iter+2)] iterates as columns if opt->store_trace, else may be NULL
 */
int  dbat_hip_solve(dbat_hip_handle *h, const dbat_hip_options *opt, double *x,
                    dbat_hip_result *result, double *res, double *damp, double *aux,
                    double *trace);

/* Post-processing of bundle.m:449-460: unweighted residuals at the last
 * linearisation point of dbat_hip_solve, reference row order. */
int  dbat_hip_final_residuals(dbat_hip_handle *h, double *r_unweighted, double *r_weighted);

/* ---- multi-GPU: one handle per rank, object points sharded -------------- */

/* The reference is one MATLAB thread; the sharded path has no
 * counterpart there.  One handle per rank (prob->shard_rank of
 * prob->shard_count, one GPU each); object points and their observations are
 * sharded.  DOMAIN SHARDING (the default): the first levels of the nested
 * dissection of the camera network give every rank a domain of images; an object point
 * goes to the rank whose domain holds its interior images, so a rank builds AND factors
 * its domain of the reduced camera system alone.  What crosses xGMI, all as RCCL
 * all-reduces on the handle's stream: per linearisation the vectors [J_c'r | diag | sums]
 * (2 NS + 8 doubles); per factorisation the ranks' shares of the TOP-SEPARATOR tiles of
 * the factor, one contiguous buffer (16 MB at 1000 images / 8 ranks, where a
 * reduce-scatter of the whole reduced system would carry 288 MB), after which every rank
 * factors the top separators and substitutes back; per solve 8 + 4*shard_count doubles
 * of scalar sums and pivot extremes; per objective value one double.
 * DBAT_HIP_MG_REPLICATED (or a problem without a usable dissection: shared EO blocks):
 * the envelope of the reduced system [S | J_c'r | diag] is summed per linearisation
 * instead and every rank factors all of it.  With a
 * communicator every entry point below "the damping loops", dbat_hip_residual,
 * dbat_hip_final_residuals, dbat_hip_gradient/_colnorms and
 * dbat_hip_posterior_cov is COLLECTIVE: all ranks call it with the same
 * arguments and all receive the complete result (x, residual rows, blocks). */
#define DBAT_HIP_UNIQUE_ID_BYTES 128
/* rank 0: a fresh RCCL unique id (ncclGetUniqueId); the caller hands the 128
 * bytes to the other ranks by whatever channel it has (MPI, a store, a file) */
int  dbat_hip_comm_unique_id(uint8_t *id /*[128]*/);
/* every rank: join the communicator (ncclCommInitRank with the handle's
 * shard_rank / shard_count on the handle's device).  Collective. */
int  dbat_hip_comm_init(dbat_hip_handle *h, const uint8_t *id /*[128]*/);
/* helper for the host side of a multi-rank driver: all-reduce `count` host
 * doubles over the handle's communicator; op 0 = sum, 1 = max, 2 = min
 * (a barrier is a reduce of one double).  Identity without a communicator. */
int  dbat_hip_comm_allreduce_host(dbat_hip_handle *h, double *buf, int64_t count, int32_t op);

/* Deterministic mode: on != 0 makes every later linearisation of this handle give the same bits in every run -- as the
 * reference does by construction, where one MATLAB thread forms J'J (gauss_newton_armijo.m:166-174).  The default
 * mode's atomics reorder f64 sums (steps repeat to 1e-13).  The sums are not ordered but made EXACT: the camera side is
 * summed chunk by chunk in a fixed order; from its column norms every element of the reduced system gets a power-of-two
 * grid on which every Schur contribution is rounded (half a unit in the last place of the element's Cauchy-Schwarz bound
 * sqrt(U_ii U_jj)), and sums of grid multiples below 2^53 grid units carry no rounding, whatever their order.
 * Covers every build path on one rank (signature-group kernel: + 7 % at C3; scenes with irregular visibility run the
 * column-list kernel over all their batches).  The step differs from the default mode's by cond(S) x 1e-15 (C1: 2e-10,
 * C3: 5e-8); converged estimates and sigma0 agree to 1e-9 -- the right-hand side is rounded on the scale of its own
 * summation error.  DBAT_HIP_EUNSUPPORTED for several ranks, shared EO blocks (camera stations), more than nine estimated
 * IO columns per camera. */
int  dbat_hip_set_deterministic(dbat_hip_handle *h, int32_t on);

/* Test hook (gloo on CPU boxes, two shards on one GPU through the host):
 * sum-all-reduce of `count` doubles at device address `buf_dev`, enqueued on
 * `stream` (a hipStream_t), used in place of RCCL when no communicator is set. */
typedef int (*dbat_hip_allreduce_fn)(void *user, void *buf_dev, int64_t count, void *stream);
int  dbat_hip_set_allreduce(dbat_hip_handle *h, dbat_hip_allreduce_fn fn, void *user);

/* Host only: the domain of every image under domain sharding with prob->shard_count ranks (nested dissection of
 * the co-visibility graph, csrc/nd.hpp): cam_owner[n_images] = the rank whose domain the image belongs to, or -1
 * for an image of a top separator (replicated on every rank).  An object point is owned by the rank whose domain
 * holds its interior images (dbat_hip_plan_point_owner); the invariant the scheme rests on -- no point sees
 * interior images of two domains -- is checked by tests/test_parallel_cpu.py.  *subtree = 1 if this problem
 * is sharded that way (0: contiguous point ranges, the whole reduced system summed and factored by every rank:
 * one rank, shared EO blocks, or the environment asked for it). */
int  dbat_hip_plan_domain_map(const dbat_hip_problem *prob, int32_t *cam_owner, int32_t *subtree);

/* mask[n_params]: 1 where this handle's shard owns the x entry (its object
 * points; rank 0 also owns IO and EO).  Host only; results returned by the
 * library are already complete on every rank. */
int  dbat_hip_owned_mask(const dbat_hip_handle *h, uint8_t *mask);

/* ---- initial values ------------------------------------------------------ */

/* s = forwintersect(s0, ids, skipPrior) (photogrammetry/forwintersect.m:27-46;
 * pm_multilenscorr1.m:45-69, pm_multiforwintersect.m:41, pm_forwintersect3.m:55-82): object
 * points by forward intersection of their lens-corrected image rays with the IO / EO of x
 * (the OP part of x is not used).  OP [3*n_points] in: current values, out: intersected
 * points; skip[p] != 0 (may be NULL) leaves point p as it is; a point with fewer than two
 * rays -- one, or none at all -- becomes NaN.  Collective on a sharded handle: every point is
 * intersected once, by the rank that owns it, from all its rays; one sum over the ranks of
 * 4*n_points doubles (the points, and for each whether it has a ray at all) gives every rank
 * the one-rank result. */
int  dbat_hip_forwintersect(dbat_hip_handle *h, const double *x, const uint8_t *skip, double *OP);

/* [s,rms,fail] = resect(s0, cams, cpId, n, v, chkId) (photogrammetry/resect.m:42-131) with the per-camera work on
 * the device: for every camera the candidate triangles of control points are solved by the three-point resection of
 * pm_resect_3pt.m:27-147 (Grunert's quartic, up to four poses each, camera behind the image plane as resect.m:105
 * asks for) and scored by the rms reprojection error over the camera's check points; the best pose wins, a later
 * triangle only if strictly better.  No handle: the inputs are what resect.m has after its MATLAB-side preparation.
 *   pt_start  [n_images+1]  range of every camera's check points in X / xn
 *   X         [3*total]     object coordinates of the check points, per camera
 *   xn        [2*total]     their lens-corrected, normalised image coordinates K \ [x; y; 1] (resect.m:95-99)
 *   tri_start [n_images+1]  range of every camera's candidate triangles in tri
 *   tri       [3*total]     three indices into the camera's point range per triangle, in trial order
 *   P         [12*n_images] out: best 3 x 4 camera matrix (column-major), NaN if the camera has no pose
 *   rms       [n_images]    out: its rms error, Inf if none; the residuals are evaluated in twice the working
 *                           precision, so it is the rms of the returned P to rounding whatever its size
 * Returns DBAT_HIP_EDEVICE without a HIP device (no CPU path). */
int  dbat_hip_resect(int32_t device, int32_t n_images, const int64_t *pt_start, const double *X, const double *xn,
                     const int64_t *tri_start, const int32_t *tri, double *P, double *rms);

/* ---- network transforms (additive to ABI 5; csrc/align.hpp) -------------- */

/* [T,R,d,alpha] = rigidalign(X, Y, scale) (misc/rigidalign.m:27-61; Soderkvist and Wedin 1993) for 3-D points: the
 * similarity (scale != 0) or rigid-body transformation that minimises sum |alpha R x_i + d - y_i|^2 over the used
 * columns.  No handle: the arrays are what the caller has.
 *   X, Y    [3*n] column-major 3 x n          use  [n], 0 drops the column whatever it holds; NULL: all are used
 *   T       [16] out: [alpha R, d; 0 0 0 1], column-major (R = T(1:3,1:3) / alpha, d = T(1:3,4))
 *   stats   [4]  out: alpha; the rms of the residuals, sqrt(sum |r_i|^2 / columns used); the columns used; the ratio
 *                of the second to the first singular value of C
 *   resid   [3*n] out, or NULL: alpha R x + d - y per used column, NaN for the others
 * Three passes over the columns on the device: the count and the centroids xm, ym (rigidalign.m:36-37); the centred
 * C = sum (y - ym)(x - xm)' (:40-43) with sum |x - xm|^2, which is tr(A'A) of :54 without its n x n matrix; and, once
 * the host has R = P diag(1, 1, det(P Q')) Q' from the 3 x 3 SVD C = P S Q' (:46-49, Jacobi rotations, no LAPACK),
 * alpha = tr((R A)'B) / tr(A'A) (:52-55) and d = ym - alpha R xm (:60), the residuals.  Every sum is a tree of fixed
 * shape without floating-point atomics: two calls give the same bits.
 * DBAT_HIP_EINVAL, before any device call (and so without a device): fewer than three used columns; a used column
 * that is not finite; a second singular value of C at or below 1e-12 of the first -- collinear points do not define
 * the rotation, rigidalign.m returns an arbitrary one.  Then DBAT_HIP_EDEVICE without a HIP device (no CPU path). */
int  dbat_hip_rigidalign(int32_t device, int64_t n, const double *X, const double *Y, const uint8_t *use, int32_t scale,
                         double *T, double *stats, double *resid);

/* [EO,OP,fail] = pm_multixform(EO, OP, T) (photogrammetry/pm_multixform.m:11-40): the similarity T = [A d; 0 0 0 1],
 * A = alpha R, applied to every object point (A x + d, :15-17) and every camera station (:20-39), in place.
 *   T     [16] column-major               EO  [eo_rows*n_images], eo_rows >= 6: rows 0 .. 5 centre and omega, phi,
 *   OP    [3*n_points]                        kappa in radians; further rows are not touched
 *   fail  [n_images] out, or NULL: 1 for a camera whose six values are not all finite (:27-34); its column stays as
 *         it is.  A point with a NaN coordinate becomes NaN in all three.
 * The camera matrix M' [I, -c] inv(T) of :23-25 is (M' R' / alpha) [I, -(A c + d)]: the new centre is A c + d, the new
 * world-to-camera rotation M' R', and omega, phi, kappa are those of derotmat3d.m:17-19 for that matrix.  (:37 takes
 * them from M' R' / alpha with the scale still in it: phi = asin(M31 / alpha) is wrong for every alpha != 1.  Here the
 * scale is divided out; for alpha = 1 the two agree.)  alpha = det(A)^(1/3).
 * DBAT_HIP_EINVAL, before any device call: eo_rows < 6; a T that is not finite, whose last row is not [0 0 0 1], or
 * whose A is not alpha times a proper rotation to 1e-9 in || A'A / alpha^2 - I ||_inf.  Then DBAT_HIP_EDEVICE without
 * a HIP device.  n_images and n_points may be 0. */
int  dbat_hip_multixform(int32_t device, const double *T, int64_t n_images, int32_t eo_rows, double *EO, int64_t n_points,
                         double *OP, uint8_t *fail);

/* ---- relative orientation (additive to ABI 5; csrc/relorient.hpp) -------- */

/* EE = essmat5(Q1, Q2) (photogrammetry/essmat5.m:9-43) for many sets of n >= 5 correspondences in one call, one lane
 * per set.  No handle.
 *   set_start [n_sets+1]   range of every set's correspondences in Q1 / Q2
 *   Q1, Q2    [3*total]    normalised homogeneous coordinates K \ [x; y; 1], 3 per correspondence
 *   E         [90*n_sets]  out: up to ten solutions per set, 9 doubles each, at unit norm and in the layout of
 *                          essmat5.m:12-20: sum e[a + 3 b] Q1[a] Q2[b] = 0 (a, b = 0 .. 2); the slots past n_sol are zero
 *   n_sol     [n_sets]     out: the number of solutions, 0 .. 10
 * The design matrix (:12-20) is folded into a 9 x 9 triangle by Givens rotations, row after row, and the four right
 * singular directions of smallest singular value (:23-24; for n = 5 the null space) come from one-sided Jacobi rotations
 * of it -- what the eigenvectors of the Gram matrix give, without its squared condition number.  det E = 0 and
 * 2 E E' E - tr(E E') E = 0 over E = x E1 + y E2 + z E3 + E4 are expanded by polynomial products in code (essmat5.m:45-856
 * keeps the expanded form as tables), reduced with row pivoting (:27), and solved through the tenth-degree polynomial
 * in z of Nister (2004) where :28-43 takes the eigenvalues of an action matrix: its real roots are bracketed between
 * the roots of its derivative and bisected (a fixed number of steps; no complex arithmetic), and each solution is
 * polished against the ten constraints evaluated on the matrix.  The solutions of a set are in ascending order of the
 * root: two calls give the same bits.  Real roots only: :42 also keeps eigenvalues with |imag| / max |lambda| < 0.01 and
 * takes their real part.  A set whose design matrix has rank below five (fifth singular value from below <= 1e-10 of the
 * largest) or whose elimination meets a pivot <= 1e-13 of the largest coefficient has n_sol = 0; nothing returned is
 * ever non-finite.
 * DBAT_HIP_EINVAL, before any device call: a set of fewer than five; a coordinate that is not finite.  Then
 * DBAT_HIP_EDEVICE without a HIP device (no CPU path). */
int  dbat_hip_essmat5(int32_t device, int32_t n_sets, const int64_t *set_start, const double *Q1, const double *Q2,
                      double *E, int32_t *n_sol);

/* Relative orientation of n_pairs image pairs in one call: a RANSAC over the given minimal samples (essmat5.m per
 * sample, as above), every model scored against every correspondence of its pair, and the camera pair and points of
 * the winner, [P1,P2,X,inFront,sp] = camsfrome(E, x, xp, frontDir) (photogrammetry/camsfrome.m:16-59).  No handle.
 *   pt_start  [n_pairs+1]  range of every pair's correspondences in x1 / x2
 *   x1, x2    [2*total]    lens-corrected, normalised image coordinates K \ [x; y; 1] in image 1 and image 2 (the third
 *                          coordinate, 1, is not stored)
 *   hyp_start [n_pairs+1]  range of every pair's samples in samples
 *   samples   [5*total]    five distinct indices into the pair's correspondences per sample: drawn by the caller, so
 *                          the call is deterministic
 *   thr2      [n_pairs]    inlier threshold on the squared Sampson distance, in normalised units; a correspondence is an
 *                          inlier of e if r^2 < thr2 (|(M q2)(1:2)|^2 + |(M' q1)(1:2)|^2), r = q1' M q2, M[a][b] = e[a + 3 b]
 *   front_dir              +1 / -1: the sign of z in front of the cameras (camsfrome.m:8)
 *   E         [9*n_pairs]  out: the winner in the layout of dbat_hip_essmat5 (with q1 from x1, q2 from x2; read row-major
 *                          it is the 3 x 3 matrix with x2' E x1 = 0 that camsfrome expects)
 *   P2        [12*n_pairs] out: [R | t], |t| = 1, column-major 3 x 4, of the candidate of camsfrome.m:33 with the most
 *                          points in front of both cameras (:55-57; of equal counts the first); camera 1 is [I | 0]
 *   stats     [8*n_pairs]  out: the inlier count, the winning sample (local to the pair) and solution, the number of
 *                          models scored, the four in-front counts in descending order (sp, :55-56)
 *   inlier    [total]      out: 1 where the correspondence is an inlier of the returned E
 *   in_front  [total]      out: 1 where the point is in front of both cameras (:49, :58)
 *   X         [3*total]    out: the points in the frame of camera 1 (:59), every correspondence of the pair
 * The winner has the highest inlier count; of equal counts the lowest (sample, solution) wins.  The 3 x 3 SVD of
 * :16-22 is done on the host between launches.  A point is the middle of the common perpendicular of its two rays,
 * which is what the normal equations of pm_forwintersect3.m:55-68 give for two rays; its depths (ptdepth.m:14) are
 * X_z and (R X + t)_z.  Two rays closer to parallel than |d1 x d2|^2 = 1e-24 define no point: it is never in front
 * (a pair without a baseline so gets sp = 0 0 0 0).  A pair for which no sample gave a model returns NaN in E, P2 and
 * X, count 0, sample and solution -1 and all-zero masks.  No floating-point atomics: two calls give the same bits.
 * hyp_start == NULL: E is an input as well, one model per pair in the layout above (camsfrome.m alone: nothing is
 * sampled or scored; samples is not read; sample and solution are 0, the number of models 1).
 * DBAT_HIP_EINVAL, before any device call: a pair of fewer than five correspondences; a coordinate that is not finite;
 * a sample index out of range or repeated inside its sample; thr2 <= 0; front_dir not +-1; a given E that is not
 * finite.  Then DBAT_HIP_EDEVICE
 * without a HIP device (no CPU path). */
int  dbat_hip_relorient(int32_t device, int32_t n_pairs, const int64_t *pt_start, const double *x1, const double *x2,
                        const int64_t *hyp_start, const int32_t *samples, const double *thr2, int32_t front_dir,
                        double *E, double *P2, int32_t *stats, uint8_t *inlier, uint8_t *in_front, double *X);

/* ---- least-squares relative orientation (additive to ABI 5; csrc/pairadjust.hpp) -------- */

typedef struct dbat_hip_pair_options {
    int32_t max_iter;           /* 1 .. 200 accepted steps at most */
    double  conv_tol;           /* > 0: stop when q <= conv_tol^2 f (below) */
    double  min_angle;          /* radians, [0, pi/2): correspondences whose two rays meet at less are not used */
} dbat_hip_pair_options;

/* max_iter = 20, conv_tol = 1e-6, min_angle = 0 (no correspondence is left out for its angle). */
int  dbat_hip_default_pair_options(dbat_hip_pair_options *opt);

/* Least-squares refinement of the relative orientation of n_pairs image pairs in one call: per pair a two-view bundle
 * adjustment in the gauge of camsfrome (photogrammetry/camsfrome.m:16-33: camera 1 is [I | 0], camera 2 [R | t] with
 * |t| = 1) over R, t and the points that pm_forwintersect3.m:55-82 intersects once and camsfrome.m:59 returns.  No
 * handle, no plan; one workgroup per pair runs the whole damped loop.  The reference has no counterpart: it refines a
 * pair only through bundle.m on a two-image project with a datum chosen by the caller (one camera fixed and one
 * baseline coordinate), which has the same optimum up to the scale of the model.
 *   pt_start  [n_pairs+1]  range of every pair's correspondences; a pair may be empty
 *   x1, x2    [2*total]    as dbat_hip_relorient
 *   use       [total]      or NULL (all): correspondences that may be used
 *   w1, w2    [2*total]    or NULL (ones): weights per coordinate, the reciprocal standard deviations in normalised units
 *   front_dir              +1 / -1: the sign of z in front of the cameras
 *   P2        [12*n_pairs] in/out: [R | t], column-major 3 x 4; t of any length but zero comes to unit length
 *   X         [3*total]    in/out: the points in the frame of camera 1; those not used keep their bits
 *   used      [total]      out: the correspondences used, chosen once at the start orientation: use is set, the point
 *                          is in front of both cameras (front_dir z > 0 in both frames), and the rays (x1, 1) and
 *                          R' (x2, 1) satisfy |d1 x d2|^2 >= sin^2(min_angle) |d1|^2 |d2|^2.  A point near the epipole
 *                          is not determined along its ray and runs away under the iteration, taking the pair with it
 *   dstat     [4*n_pairs]  out: the objective at the start, the objective, sigma0, lambda
 *   istat     [4*n_pairs]  out: code, iterations (accepted steps), trials, n (the correspondences used)
 *   Q         [36*n_pairs] out: cofactor matrix, 6 x 6 of rank five, of the rotation vector a (R <- exp([a]x) R) and the
 *                          change of t: blkdiag(I, B) inv(S0) blkdiag(I, B)' with S0 the undamped reduced matrix at the
 *                          returned values and B a basis of the plane across t; in these coordinates it does not depend
 *                          on B.  The covariance is sigma0^2 Q
 *   res       [4*total]    out, or NULL: weighted residuals at the returned values, image 1 x, y, image 2 x, y; zero for
 *                          correspondences not used
 * Residuals: w1 (pi(X) - x1) and w2 (pi(R X + t) - x2), pi(Y) = Y(1:2) / Y(3); f is the sum of their squares.  A step is
 * R <- exp([a]x) R, t <- (t + B b) / |t + B b|, X <- X + d: five unknowns and three per point.  Levenberg-Marquardt with
 * Marquardt's scaling (lambda diag V added to every 3 x 3 point block, lambda diag U to the 5 x 5 pose block), the
 * points eliminated.  lambda starts at 1e-3.  A trial is accepted if its objective is finite and smaller and every used
 * point is in front of both cameras; then lambda <- max(lambda / 10, 1e-12).  Otherwise lambda <- 10 lambda and the same
 * linearisation is solved again.  Every trial tests for the end first, with q = -g' delta the decrease its damped
 * model predicts: q <= conv_tol^2 f, or f <= 1e-24 * 4 n (a noise-free pair never meets the first).
 * The normal equations are float64.  The objective of the accept test is not: near the optimum a step's decrease is
 * below the rounding of a float64 evaluation, and an accept test that answers at random stops the iteration short.  The
 * residuals are formed and summed as pairs of doubles, and R is such a pair kept orthonormal to 1e-31 (its rounding
 * across the rotations would move f as well); the returned f and R are the high words.
 * Codes: 0 converged; 1 max_iter steps done; 2 no acceptable step before lambda > 1e8; 3 converged, but some V_k has a
 * Cholesky pivot <= 1e-12 of its diagonal entry or S0 one <= 1e-10: Q is NaN; 4 fewer than five correspondences used:
 * P2 and X are returned as given, dstat is NaN but for lambda.  Every other code returns the last accepted values.
 * sigma0 = sqrt(f / (n - 5)), NaN for n = 5.  Q is NaN for every singular end, whatever the code.  Nothing else
 * returned is ever non-finite.  The sums have a fixed shape and there are no atomics: two calls give the same bits, and
 * a pair gives the same bits alone and in a batch.
 * DBAT_HIP_EINVAL, before any device call: a coordinate, weight, P2 or point to be used (use) that is not finite; a
 * weight <= 0; front_dir not +-1; an R with |R'R - I| > 1e-6 or det R < 0; t = 0; max_iter outside 1 .. 200;
 * conv_tol <= 0; min_angle outside [0, pi/2); a pt_start that does not ascend from 0.  Then DBAT_HIP_EDEVICE without a
 * HIP device (no CPU path).  What the data of one pair cause -- too few points, no convergence, singularity -- is that
 * pair's code, never an error. */
int  dbat_hip_pairadjust(int32_t device, int32_t n_pairs, const int64_t *pt_start, const double *x1, const double *x2,
                         const uint8_t *use, const double *w1, const double *w2, int32_t front_dir,
                         const dbat_hip_pair_options *opt, double *P2, double *X, uint8_t *used, double *dstat,
                         int32_t *istat, double *Q, double *res);

/* ---- robust resection (additive to ABI 5; csrc/resect_ransac.hpp, csrc/poseadjust.hpp) -------- */

/* Spatial resection of n_images cameras by a RANSAC over triples of control points, in one call.  The reference has no
 * counterpart: resect.m:42-131 tries the largest triangles and keeps the pose of smallest rms over all check points, so
 * that one wrong control point decides the answer (dbat_hip_resect above keeps that behaviour).  No handle: the inputs
 * are what resect.m has after its MATLAB-side preparation.
 *   pt_start  [n_images+1]  range of every camera's points in X / xn; a camera may be empty
 *   X         [3*total]     object coordinates, per camera
 *   xn        [2*total]     lens-corrected, normalised image coordinates K \ [x; y; 1] with -f: the cameras look along
 *                           -z, and a point is in front where the third row of P [X; 1] is negative
 *   use       [total]       or NULL (all): the points that may be sampled and counted
 *   smp_start [n_images+1]  range of every camera's samples in smp
 *   smp       [3*total]     three distinct indices into the camera's point range per sample: drawn by the caller, so the
 *                           call is deterministic
 *   thr2      [n_images]    inlier threshold on the squared residual, in normalised units
 *   P         [12*n_images] out: the winning 3 x 4 camera matrix (column-major), NaN if the camera has no winner
 *   stats     [4*n_images]  out: the inlier count, the winning sample (local to the camera) and root (the index among
 *                           the poses of its sample, in the order rs_poses_3pt returns them), the number of poses scored;
 *                           count 0 and sample and root -1 without a winner
 *   inlier    [total]       out: 1 where the point is an inlier of the returned P; all zero without a winner
 *   ssq       [n_images]    out: the sum of e0^2 + e1^2 over the inliers; 0 without a winner
 * One workgroup per camera; a lane solves one sample by the three-point resection of pm_resect_3pt.m:27-147 (up to four
 * poses) and scores its poses against every point of the camera.  A point is an inlier of a pose if use is set, it is in
 * front, and e0^2 + e1^2 <= thr2 with e = pi(P [X; 1]) - xn evaluated in twice the working precision, as dbat_hip_resect
 * evaluates its rms.  The winner has the highest count; of equal counts the lowest (sample, root) wins; it needs at least
 * four inliers (three is what every sample gets from itself).  A sample with a point that may not be used, with collinear
 * points or without a real root scores nothing.  Counts are integers and the winner is one integer maximum: no
 * floating-point atomics, two calls give the same bits, and a camera gives the same bits alone and in a batch.
 * DBAT_HIP_EINVAL, before any device call: a point that may be used and is not finite; a sample index out of range or
 * repeated inside its sample; thr2 not positive and finite; ranges that do not ascend from 0; 2^29 points or 2^31 samples
 * and more in one camera.  Then DBAT_HIP_EDEVICE without a HIP device (no CPU path). */
int  dbat_hip_resect_ransac(int32_t device, int32_t n_images, const int64_t *pt_start, const double *X, const double *xn,
                            const uint8_t *use, const int64_t *smp_start, const int32_t *smp, const double *thr2, double *P,
                            int32_t *stats, uint8_t *inlier, double *ssq);

/* Least-squares space resection of n_images cameras in one call: the pose of every camera from its control points, with
 * sigma0 and the cofactor matrix.  No handle, no plan; one wave per camera runs the whole damped loop.  The reference has
 * no counterpart: it reaches this pose only through bundle.m on a one-camera project with every object point fixed.
 *   pt_start  [n_images+1]  range of every camera's points; a camera may be empty
 *   X, xn                   as dbat_hip_resect_ransac
 *   use       [total]       or NULL (all): points that may be used
 *   w         [2*total]     or NULL (ones): weights per coordinate, the reciprocal standard deviations in normalised units
 *   opt                     max_iter and conv_tol of dbat_hip_pair_options, with its defaults; min_angle must be 0
 *   P         [12*n_images] in/out: [R | -R C], column-major 3 x 4
 *   used      [total]       out: the points used, chosen once at the start pose: use is set and the point is in front
 *   dstat     [4*n_images]  out: the objective at the start, the objective, sigma0, lambda
 *   istat     [4*n_images]  out: code, iterations (accepted steps), trials, n (the points used)
 *   Q         [36*n_images] out: cofactor matrix, 6 x 6 column-major, of (c, a), centre first: the inverse of the undamped
 *                           normal matrix at the returned values.  The covariance is sigma0^2 Q
 *   res       [2*total]     out, or NULL: weighted residuals at the returned pose of every finite point, used or not (a
 *                           caller can threshold them and call again); zero where they are not finite, and for a
 *                           camera that ends with code 4
 * Residuals: w (pi(R (X - C)) - xn), pi(Y) = Y(1:2) / Y(3); f is the sum of their squares over the n used points.  A step
 * is C <- C + c, R <- exp([a]x) R: six unknowns.  The damping loop is that of dbat_hip_pairadjust point for point:
 * Levenberg-Marquardt with Marquardt's scaling (lambda diag N), lambda from 1e-3, lambda <- max(lambda / 10, 1e-12) on an
 * accepted trial, 10 lambda on a rejected one (the same linearisation is solved again), the end above 1e8; a trial is
 * accepted if its objective is finite and smaller and every used point is still in front; every trial tests for the end
 * first: q <= conv_tol^2 f with q = -g' delta, or f <= 1e-24 * 2 n.
 * The normal equations are float64.  The objective of the accept test is formed and summed in pairs of doubles, and R is
 * such a pair kept orthonormal, for the reason given at dbat_hip_pairadjust; the returned f and R are the high words.
 * Object coordinates and the centre are taken relative to the camera's first used point before anything is multiplied:
 * coordinates of 1e6 m keep their digits.
 * Codes: 0 converged; 1 max_iter steps done; 2 no acceptable step before lambda > 1e8; 3 converged, but the undamped
 * matrix has a Cholesky pivot <= 1e-10 of its diagonal entry: Q is NaN; 4 fewer than three points used: P is returned as
 * given, dstat is NaN but for lambda, Q is NaN.  sigma0 = sqrt(f / (2 n - 6)), NaN for n = 3.  Q is NaN for every singular
 * end, whatever the code.  Nothing else returned is ever non-finite.  The sums have a fixed shape and there are no atomics:
 * two calls give the same bits, and a camera gives the same bits alone and in a batch.
 * DBAT_HIP_EINVAL, before any device call: a point that may be used, a weight or a P that is not finite; a weight <= 0;
 * an R with |R'R - I| > 1e-6 or det R < 0; a pt_start that does not ascend from 0; max_iter outside 1 .. 200;
 * conv_tol <= 0; min_angle != 0.  Then DBAT_HIP_EDEVICE without a HIP device (no CPU path).  What the data of one camera
 * cause -- too few points, no convergence, singularity -- is that camera's code, never an error. */
int  dbat_hip_poseadjust(int32_t device, int32_t n_images, const int64_t *pt_start, const double *X, const double *xn,
                         const uint8_t *use, const double *w, const dbat_hip_pair_options *opt, double *P, uint8_t *used,
                         double *dstat, int32_t *istat, double *Q, double *res);

/* ---- robust forward intersection (additive to ABI 5; csrc/intersect_ransac.hpp, csrc/pointadjust.hpp) -------- */

/* Forward intersection of n_points object points by a RANSAC over pairs of their image rays, in one call.  The reference
 * has no counterpart: pm_forwintersect3.m:55-82 is one linear solve over all rays of a point, so that one mismatched image
 * measurement drags the point away (dbat_hip_forwintersect above keeps that behaviour).  No handle, no plan.
 *   ray_start [n_points+1]  range of every point's rays in cam / xn / use / inlier; a point may have none
 *   cam       [total]       the index of the ray's camera in P and thr2
 *   xn        [2*total]     lens-corrected, normalised image coordinates with the conventions of dbat_hip_resect_ransac:
 *                           K \ [x; y; 1] with -f, so that the cameras look along -z, and a point is in front where the
 *                           third row of P [X; 1] is negative
 *   n_cams, P [12*n_cams]   the cameras: [R | -R C], column-major 3 x 4
 *   use       [total]       or NULL (all): the rays that may be sampled and counted
 *   smp_start [n_points+1]  or NULL: range of every point's samples in smp.  A point whose range is empty -- every point
 *                           when smp_start is NULL -- has all its pairs enumerated on the device, lexicographically over
 *                           i < j: sample k = i (2 r - i - 1) / 2 + (j - i - 1) of its r rays.  That is allowed up to
 *                           64 rays (2016 pairs); a point of more must bring samples
 *   smp       [2*samples]   two distinct indices into the point's ray range per sample: drawn by the caller, so the call
 *                           is deterministic
 *   thr2      [n_cams]      inlier threshold on the squared residual, in normalised units, per camera (focal lengths
 *                           differ)
 *   min_angle               in [0, pi/2): a pair of rays that meet at a smaller angle is not scored
 *   X         [3*n_points]  out: the winning point, NaN without a winner
 *   stats     [4*n_points]  out: the inlier count, the winning sample (local to the point: its place in smp, or k above),
 *                           the number of hypotheses scored, the number of usable rays; count 0 and sample -1 without a
 *                           winner
 *   inlier    [total]       out: 1 where the ray is an inlier of the returned X; all zero without a winner
 *   ssq       [n_points]    out: the sum of e0^2 + e1^2 over the inliers; 0 without a winner
 * One wave per point, four points per workgroup; a lane takes one sample.  A hypothesis is the middle of the common
 * perpendicular of its two rays (centre -R' t, direction R' (x0, x1, 1), normalised): what pm_forwintersect3.m:55-68
 * gives for two rays.  It is scored only if both rays may be used, |d1 x d2|^2 >= max(sin^2 min_angle, 1e-24) on the unit
 * directions, and the point is finite.  A ray is an inlier if use is set, the point is in front of its camera, and
 * e0^2 + e1^2 <= thr2[cam] with e = pi(P [X; 1]) - xn evaluated in twice the working precision, as
 * dbat_hip_resect_ransac scores.  The winner has the highest count and needs at least 2; of equal counts the lowest
 * sample wins.  Counts are integers and the winner is one integer maximum: no floating-point atomics, two calls give the
 * same bits, and a point gives the same bits alone and in a batch.
 * DBAT_HIP_EINVAL, before any device call, in this order: a null argument; negative counts; ranges (ray_start, then
 * smp_start) that do not ascend from 0; cam outside [0, n_cams); an xn of a usable ray, or a P, that is not finite; an R with |R'R - I| > 1e-6 or
 * det R < 0; thr2 not positive and finite; min_angle outside [0, pi/2); a sample index out of range or repeated inside its
 * sample; a point with no samples and more than 64 rays; 2^29 rays or 2^31 samples and more in one point.  Then
 * DBAT_HIP_EDEVICE without a HIP device (no CPU path).  n_points = 0 returns DBAT_HIP_OK. */
int  dbat_hip_intersect_ransac(int32_t device, int32_t n_points, const int64_t *ray_start, const int32_t *cam, const double *xn,
                               int32_t n_cams, const double *P, const uint8_t *use, const int64_t *smp_start, const int32_t *smp,
                               const double *thr2, double min_angle, double *X, int32_t *stats, uint8_t *inlier, double *ssq);

/* Least-squares forward intersection of n_points object points in one call: every point from its image rays, minimising
 * sum |w (pi(R (X - C)) - xn)|^2 over the used rays, with sigma0 and the cofactor matrix.  No handle, no plan; a group of
 * eight lanes per point runs the whole damped loop.  The reference has no counterpart: it reaches this point only through
 * bundle.m on a project with every camera fixed.
 *   ray_start, cam, xn, n_cams, P   as dbat_hip_intersect_ransac
 *   use       [total]       or NULL (all): rays that may be used
 *   w         [2*total]     or NULL (ones): weights per coordinate, the reciprocal standard deviations in normalised units
 *   opt                     max_iter and conv_tol of dbat_hip_pair_options, with its defaults; min_angle must be 0
 *   X         [3*n_points]  in/out; the start of a point that has a ray to use must be finite
 *   used      [total]       out: the rays used, chosen once at the start point: use is set and the point is in front
 *   dstat     [4*n_points]  out: the objective at the start, the objective, sigma0, lambda
 *   istat     [4*n_points]  out: code, iterations (accepted steps), trials, n (the rays used)
 *   Q         [9*n_points]  out: cofactor matrix, 3 x 3 column-major: the inverse of the undamped normal matrix at the
 *                           returned point.  The covariance is sigma0^2 Q
 *   res       [2*total]     out, or NULL: weighted residuals at the returned point of every finite ray, used or not (a
 *                           caller can threshold them and call again); zero where they are not finite, and for a point
 *                           that ends with code 4
 * The damping loop is that of dbat_hip_poseadjust point for point: Levenberg-Marquardt with Marquardt's scaling
 * (lambda diag N), lambda from 1e-3, lambda <- max(lambda / 10, 1e-12) on an accepted trial, 10 lambda on a rejected one
 * (the same linearisation is solved again), the end above 1e8; a trial is accepted if its objective is finite and smaller
 * and every used ray is still in front; every trial tests for the end first: q <= conv_tol^2 f with q = -g' delta, or
 * f <= 1e-24 * 2 n.  The normal equations are float64; the objective of the accept test is formed and summed in pairs of
 * doubles, and the returned f is the high word.  Coordinates are taken relative to the projection centre of the point's
 * first used ray before anything is multiplied: coordinates of 1e6 m keep their digits.
 * Codes: 0 converged; 1 max_iter steps done; 2 no acceptable step before lambda > 1e8; 3 converged, but the undamped
 * matrix has a Cholesky pivot <= 1e-10 of its diagonal entry (near-parallel rays): Q is NaN; 4 fewer than two rays used: X
 * is returned as given, dstat is NaN but for lambda, Q is NaN.  sigma0 = sqrt(f / (2 n - 3)).  Q is NaN for every singular
 * end, whatever the code.  Nothing else returned is ever non-finite.  The sums have a fixed shape and there are no atomics:
 * two calls give the same bits, and a point gives the same bits alone and in a batch, wherever it lands in a wave.
 * DBAT_HIP_EINVAL, before any device call: a null argument; negative counts; max_iter outside 1 .. 200; conv_tol <= 0;
 * min_angle != 0; a ray_start that does not ascend from 0; cam outside [0, n_cams); an xn of a usable ray that is not
 * finite; 2^29 rays and more in one point; an X of a point with a usable ray that is not finite; a weight that is not
 * positive and finite; a P that is not finite or whose R is not a rotation.  Then DBAT_HIP_EDEVICE without a HIP device
 * (no CPU path).  What the data of one point cause -- too few rays, no convergence, singularity -- is that point's code,
 * never an error. */
int  dbat_hip_pointadjust(int32_t device, int32_t n_points, const int64_t *ray_start, const int32_t *cam, const double *xn,
                          int32_t n_cams, const double *P, const uint8_t *use, const double *w,
                          const dbat_hip_pair_options *opt, double *X, uint8_t *used, double *dstat, int32_t *istat,
                          double *Q, double *res);

/* ---- measurement hooks -------------------------------------------------- */

/* One benchmark step = one Levenberg-Marquardt iteration's device work at
 * the current point: J'J build + Schur solve (+ back-substitution) and one
 * residual-only evaluation at the trial point.  x is not advanced, so every
 * step does identical work.  From HIP events on the handle's stream, ms[16]:
 * phases { linearize+Schur build, factor+solve, back-substitution, trial
 * residual } then single kernels { the Schur kernel alone (k_build_sig, or the
 * tile kernel k_build_tile3 / k_build_tile2 where the signature groups are too
 * short, or k_build when nothing is tiled; dbat_hip_build_kernel_name says which),
 * k_chol_df incl. its flag reset, the back-substitution kernels, k_residual_cm },
 * then (several ranks, domain sharding; else 0) { factorisation of the rank's own domain
 * + its shares of the top tiles, the all-reduce of the top tiles as the stream sees it,
 * top separators + backward substitution, 0 }, then (heavy / giant points on the matrix cores, csrc/heavy.hpp;
 * else 0) { camera side of their observations + k_heavy_z / k_heavy_z_giant, k_heavy_syrk, 0, 0 }.  ms[16]. */
int  dbat_hip_bench_step(dbat_hip_handle *h, double lambda, int32_t scale_columns, double *ms);
/* load x into the handle (device resident) before bench steps */
int  dbat_hip_set_x(dbat_hip_handle *h, const double *x);
/* sizes of the internal layout, for roofline accounting:
 * info[0]=NS (reduced system order) info[1]=#batches info[2]=max obs per point
 * info[3]=obs in this shard info[4]=points in this shard info[5]=batch size
 * info[6]=max camera-side columns per observation info[7]=#tiles
 * several ranks: info[8]=1 domain sharding (0: replicated factorisation) info[9]=doubles of the reduced
 * system summed per factorisation (top tiles / the envelope) info[10]=doubles summed as vectors per
 * linearisation info[11]=images in the top separators info[12]=tile rows of the factor
 * info[13], info[14]=tasks of the two launches of the factorisation
 * info[15]=v_mfma_f64_16x16x4_f64 instructions (2048 flops each) one launch of the tile kernel executes (its symmetric
 * products; the algorithmic count of the roofline is the full product)
 * heavy / giant points on the matrix cores (csrc/heavy.hpp; all 0 when the column-list kernels take them):
 * info[16]=tasks of k_heavy_syrk info[17]=its v_mfma_f64_16x16x4_f64 instructions per launch info[18]=row groups
 * info[19]=bytes of the scratch array Zs info[20]=points info[21]=observations info[22]=k-steps per task at most
 * info[23]=algorithmic flops of their Schur terms, sum of 108 k + 216 k^2 */
int  dbat_hip_info(const dbat_hip_handle *h, int64_t *info /*[24]*/);

/* Host only (no GPU): statistics of the layout the plan gives this problem (this shard), so that a test
 * can tell which code path of the signature kernel a scene exercises.  st[16]:
 * [0] tiles [1] batches [2] tiled batches [3] signature groups [4] their points [5] chunks
 * [6..9] chunks of 1-8 / 9-16 / 17-32 / 33-64 points (8, 4, 2, 1 lanes per point in pass 1)
 * [10] chunks that need more than one round of pass 2 [11] most cameras per chunk
 * [12] most rows of a chunk [13] 1 = k_build_sig selected [14] 1 = k_backsub_sig selected
 * [15] tasks of k_heavy_syrk (0: heavy / giant points, if any, take the column-list kernels) */
int  dbat_hip_plan_layout_stats(const dbat_hip_problem *prob, int64_t *st /*[16]*/);

/* name of the kernel that builds the Schur complement of the tiled points in this handle
 * (the dominant kernel of a step; the one the bench's roofline entry is about) */
int  dbat_hip_build_kernel_name(const dbat_hip_handle *h, char *buf, int32_t buf_len);

/* Schedule of the Cholesky of the reduced system (measurement only): st[0] order of the
 * factorised system incl. block padding, st[1] tile tasks, st[2] 64x64x64 tile products of
 * the update phase, st[3] tile rows, st[4] 1 = nested-dissection order, st[5] 1 = dataflow kernel. */
int  dbat_hip_chol_stats(const dbat_hip_handle *h, int64_t *st /*[6]*/);

/* Posterior covariance blocks at x: sigma0^2 * blocks of inv(J'J), J the
 * weighted Jacobian incl. prior rows.  Replaces bundle/bundle_cov.m:63-214
 * ('CIO','CEO','COP'; the native code it stands in for is
 * test/postcov/icpc_mex.c) -- computed from the Schur blocks instead of a
 * Cholesky factor of the full normal matrix:
 *   inv(J'J)[cams,cams] = inv(S),  inv(J'J)[p,p] = V_p^-1 + (W_p V_p^-1)' inv(S) (W_p V_p^-1).
 * CEO  [36*n_images]  6x6 block per image, column-major, rows/columns of fixed elements zero
 * CIO  [nIOu*nIOu]    the IO unknowns in the order of the IO part of x (buildserialindices.m:11-17)
 * COP  [9*n_points]   3x3 block per object point, rows/columns of fixed coordinates zero
 * Sinv [NS*NS]        optional: inv(S) itself (lower triangle valid; NOT scaled by sigma0^2),
 *                     order [EO of image 0..n-1 | IO unknowns], for 'CEOF'/'CIOF'
 * Any output may be NULL.  On a sharded handle (collective) inv(S) is computed on every rank,
 * the per-point blocks by the owning rank, and all ranks receive all blocks. */
int  dbat_hip_posterior_cov(dbat_hip_handle *h, const double *x, double sigma0, double *CEO, double *CIO,
                            double *COP, double *Sinv);

/* Reliability at x (internal reliability of the adjustment; prior sigma0 = 1, independent of the
 * estimated sigma0): the redundancy numbers r_i = 1 - h_ii, h_ii the diagonal of the hat matrix
 * J inv(J'J) J' of the weighted system (J the weighted Jacobian incl. prior rows, as for
 * dbat_hip_posterior_cov).  Same set-up as dbat_hip_posterior_cov (reduced system at x, factor,
 * selected or dense inverse); the 2 x 2 block Qvv = I - H of every image point comes from the
 * Schur pieces, never from J C J'.
 * qvv_ip  [3*n_obs]      per IP column (the caller's order): r_u, q_uv, r_v -- Qvv(0,0), Qvv(0,1), Qvv(1,1)
 * r_prior [m - 2*n_obs]  r of every prior row, in the row order of dbat_hip_final_residuals
 *                        (may be NULL when there are no prior rows)
 * Sum over all m rows: m - n.  If J'J is not positive definite the call fails with DBAT_HIP_EDEVICE and
 * dbat_hip_last_error() "posterior covariance: the reduced normal matrix is not positive definite"
 * (as dbat_hip_posterior_cov).  On a sharded handle (collective) every rank computes the blocks of
 * its own observations and all ranks receive everything. */
int  dbat_hip_redundancy(dbat_hip_handle *h, const double *x, double *qvv_ip, double *r_prior);

/* Ray intersection angles at x: for every object point the largest angle between two of its rays
 * (photogrammetry/angles.m:26-46), for every image the largest angle between two of its rays
 * (photogrammetry/camangles.m:26-46; file/writestats.m:131, plotting/plotimagestats.m:84).  For k rays with
 * directions d_j = Q - c_j normalised to n_j:  max over the pairs of acos(|clip(n_i . n_j, -1, 1)|), computed as
 * acos(min_{i<j} |n_i . n_j|); exactly 0 for k = 1, NaN for k = 0.  Every IP column counts, observations of fixed
 * and control points included.
 *   x          the parameter vector (as for dbat_hip_posterior_cov; fixed values come from the handle)
 *   op_angle   [n_points] radians, or NULL      cam_angle  [n_images] radians, or NULL
 *   op_rays    [n_points] rays of every point, or NULL      cam_rays   [n_images] rays of every image, or NULL
 *              (from the plan: no caller has to build the dense visibility table for them)
 * The point side takes the plan's point-major order, the image side its camera-major copy with the pair products on
 * the f64 matrix cores (csrc/angles.hpp).  Two calls give the same bits.  A handle that is one shard of several
 * (shard_count > 1) returns DBAT_HIP_EINVAL: pairs of rays across shards are not formed. */
int  dbat_hip_ray_angles(dbat_hip_handle *h, const double *x, double *op_angle, double *cam_angle,
                         int32_t *op_rays, int32_t *cam_rays);
/* Host only, one thread, no GPU: the same definition evaluated over the problem's own arrays (OP_val, EO_val, ip_cam,
 * ip_pt), for tests of the definition; never on the product path.  Either output may be NULL. */
int  dbat_hip_debug_ray_angles_host(const dbat_hip_problem *prob, double *op_angle, double *cam_angle);

/* Point depths at x (additive to ABI 5): the depth of every object point with respect to every camera that sees it,
 * d_k = -M'_(3,:) (Q_pt(k) - q0_cam(k)) for IP column k, M' the world-to-camera rotation and q0 the camera centre --
 * -ptdepth(P, X) of photogrammetry/pm_multidepth.m:19-37 (pointdepth.m, ptdepth.m) with P = K M' [I, -q0]; positive
 * in front of the camera.  Every IP column counts.
 *   x            the parameter vector (as for dbat_hip_ray_angles; fixed values come from the handle)
 *   thr          an observation is "behind" when !(d_k > thr); a NaN depth therefore counts as behind.  Not NaN.
 *   depth_out    [n_obs] depths in IP-column order, or NULL
 *   img_min_out  [n_images] smallest depth of every image, NaN for an image without points, or NULL
 *   stats_out    n_behind; min_depth, the smallest depth that is a number (NaN if there is none); argmin_column, the
 *                smallest IP column that attains it (-1 if there is none)
 * One pass over the plan's camera-major copy (csrc/depth.hpp); counts and minima are reduced with integer atomics
 * only, so two calls give the same bits.  Scratch is kept on the handle.  A handle that is one shard of several
 * (shard_count > 1) returns DBAT_HIP_EUNSUPPORTED. */
typedef struct dbat_hip_depth_stats {
    int64_t n_behind;
    double  min_depth;
    int64_t argmin_column;
} dbat_hip_depth_stats;
int  dbat_hip_point_depths(dbat_hip_handle *h, const double *x, double thr, double *depth_out, double *img_min_out,
                           dbat_hip_depth_stats *stats_out);

/* The chirality veto of bundle.m:125-127,168-172 (a handle setting, like dbat_hip_set_deterministic): on != 0 makes the
 * damping loops of every later dbat_hip_solve reject a trial point at which an observation has !(depth > min_depth) --
 * at exactly the places where they consult dbat_hip_options.veto_fun (gauss_newton_armijo.m:268-271,
 * levenberg_marquardt.m:170-173, levenberg_marquardt_powell.m:146-166), with the same consequences; with a veto_fun
 * as well, either one rejects.  The test runs on the device-resident trial point: two words come back, the parameter
 * vector never leaves the device.  Gauss-Markov (damping 0) has no trial points and ignores the setting.  min_depth
 * must be finite (DBAT_HIP_EINVAL); 0 is the reference's meaning of "in front".  DBAT_HIP_EUNSUPPORTED on a handle
 * that is one shard of several; dbat_hip_solve_robust returns DBAT_HIP_EUNSUPPORTED while the setting is on. */
int  dbat_hip_set_chirality(dbat_hip_handle *h, int32_t on, double min_depth);
/* The built-in veto during the last dbat_hip_solve: trial points tested, trial points rejected, and n_behind /
 * min_depth of the last rejected one (0 / NaN if none was). */
typedef struct dbat_hip_veto_stats {
    int64_t tested, rejected, n_behind;
    double  min_depth;
} dbat_hip_veto_stats;
int  dbat_hip_chirality_stats(const dbat_hip_handle *h, dbat_hip_veto_stats *out);

/* Image coverage by the measured points (photogrammetry/coverage.m:113-185), per image, from the pixel coordinates
 * alone (no x).  Image c owns the IP columns of its points (IP is image-major); every index below is an IP column.
 *   lo, hi      [2*n_images] exact min and max of u and v; NaN for an image without points
 *   rad_max     [n_images] largest distance to the principal point, mm: sqrt((u px_u - pp_x)^2 + (-v px_v - pp_y)^2),
 *               pp = IO_val rows 1, 2 of the image's column (the values of the last dbat_hip_set_values); NaN for none
 *   rad_ip      [n_images] the column that attains it (ties: the lowest), -1 for none
 *   hull_area   [n_images] area of the convex hull, px^2: the shoelace sum over its vertices relative to lo; 0 for
 *               fewer than three points or collinear points
 *   hull_start  [n_images+1], hull_ip [n_obs capacity]: the hull of image c is hull_ip[hull_start[c] ..
 *               hull_start[c+1]), counter-clockwise (u to the right, v up) from the lowest (u, v) in lexicographic
 *               order, strictly extreme points only (no collinear boundary points; of equal points the lowest
 *               column); fewer than three distinct points: those points
 * Any output may be NULL.  One workgroup per image (csrc/quality.hpp): the points outside the octagon of the eight
 * extreme points are sorted and scanned (monotone chain), at most dbat_hip_quality_hull_cap() of them in LDS, more in
 * global memory.  The scan ends after a number of steps bounded by the point count for every input.  Two calls give
 * the same bits.  What the call needs beyond the plan's uploads is built by the first call and kept on the handle.
 * A handle that is one shard of several (shard_count > 1) returns DBAT_HIP_EINVAL. */
int  dbat_hip_coverage(dbat_hip_handle *h, double *lo, double *hi, double *rad_max, int64_t *rad_ip, double *hull_area,
                       int64_t *hull_start, int64_t *hull_ip);
/* Marking-residual statistics at x (file/bundle_result_file.m:630-672): with e_i the 2-norm of image point i's
 * residual in pixels (the residual pass's mm rows divided by the image's px_size),
 *   cam_n, cam_ss  [n_images] points of every image and the sum of e^2 over them (IP order)
 *   op_n, op_ss    [n_points] rays of every object point and the sum of e^2 over them (the plan's point-major order)
 *   total_ss       the sum of e^2 over all image points      max_e, max_ip  the largest e and its IP column (ties: the
 *                  lowest column, the order of the reference's res(:)); NaN and -1 without image points
 * Any output may be NULL.  Every sum is a reduction in a fixed order, no floating-point atomics: two calls give the
 * same bits.  RMS values (and the NaN of a zero count) are the caller's.  A handle that is one shard of several
 * returns DBAT_HIP_EINVAL. */
int  dbat_hip_residual_stats(dbat_hip_handle *h, const double *x, int64_t *cam_n, double *cam_ss, int64_t *op_n,
                             double *op_ss, double *total_ss, double *max_e, int64_t *max_ip);
/* Candidates of one image that dbat_hip_coverage sorts in LDS (QUAL_HULL_CAP). */
int32_t dbat_hip_quality_hull_cap(void);
/* Host only, one thread, no GPU: dbat_hip_coverage over the problem's own arrays (ip_cam, ip_val, px_size, IO_val)
 * with the kernel's own filter, order, chain scan and shoelace sum; for tests, never on the product path. */
int  dbat_hip_debug_coverage_host(const dbat_hip_problem *prob, double *lo, double *hi, double *rad_max, int64_t *rad_ip,
                                  double *hull_area, int64_t *hull_start, int64_t *hull_ip);
/* Host only, no GPU (debug / tests; never on the product path): the task list of the factorisation of the reduced
 * system in the compact tile layout on one rank, as a handle would schedule it for this problem.  Product lists are made only
 * where the chain role is on (the kernel without it walks none).
 *   hdr[16]      { tile columns nT, 64-bit words W per row of the pattern, tasks, entries of the product lists, the
 *                  candidate taken, partial-sum slots, tile products, chain role (0 | 1), diagonal tiles of the chain
 *                  role, tasks with a product list, the bit of a task's mode that marks a listed task,
 *                  (nT + 1) * W, 0 ... }
 *   cand_us[4]   modelled time in microseconds of the candidate schedules: 0 every sum in column order, 1 the sums cut
 *                where two parts of the dissection meet, 2 product lists, 3 lists and cut sums (< 0: not made)
 *   jobs         [8 * tasks] i, k, jlo, jhi, part, np, mode, p per task in task order.  Its products are the columns
 *                j in [jlo, jhi) with a tile in both tile rows i and k, in column order -- or, where mode has the
 *                listed bit, the entries [jlo, jhi) of plist in that order
 *   rowbits      [(nT + 1) * W] bit k of row i: tile (i, k) exists after fill (row nT: the right-hand side)
 * jobs, plist and rowbits may be NULL (sizes from hdr first); a capacity that is too small is DBAT_HIP_EINVAL.
 * DBAT_HIP_DF_SUMS and DBAT_HIP_DF_MERGE are honoured as by a handle. */
int  dbat_hip_debug_df_schedule(const dbat_hip_problem *prob, int64_t *hdr, double *cand_us, int32_t *jobs,
                                int64_t jobs_cap, int32_t *plist, int64_t plist_cap, uint64_t *rowbits,
                                int64_t rowbits_cap);

/* ---- robust estimation: iteratively reweighted least squares over the image points -------------------------------
 * For image point i (one IP column, two rows) at parameters x:
 *   s_i   = ||(w_u v_u, w_v v_v)||_2, w = 1 / (IP.std * pxSize) the BASE weights, v the unweighted residual
 *   scale = 1 (DBAT_HIP_SCALE_APRIORI) or median(s) / sqrt(2 ln 2) (DBAT_HIP_SCALE_MAD: the exact median over all
 *           image points, the mean of the two middle values for an even count; 1 if it is 0)
 *   u_i   = s_i / scale;  omega_i in (0, 1]:  Huber  1 for u <= k, else k / u  (default k = 1.5)
 *                                            Cauchy 1 / (1 + (u / k)^2)      (default k = 2.385)
 * Both rows of image point i then carry the weight w * sqrt(omega_i) (effective sigma IP.std / sqrt(omega_i)).
 * Prior observations are never reweighted.  A handle that never sees one of the calls below allocates nothing
 * for them; dbat_hip_set_values and dbat_hip_set_obs_weights(h, NULL) restore the base weights and the
 * uniform-weight path of a fresh handle exactly. */
#define DBAT_HIP_LOSS_HUBER    0
#define DBAT_HIP_LOSS_CAUCHY   1
#define DBAT_HIP_SCALE_APRIORI 0
#define DBAT_HIP_SCALE_MAD     1
#define DBAT_HIP_ROBUST_MAX_OUTER 64   /* capacity of dbat_hip_robust_result's per-step arrays */

typedef struct dbat_hip_robust_options {
    int32_t loss;           /* DBAT_HIP_LOSS_* */
    double  k;              /* tuning constant (> 0) */
    int32_t scale;          /* DBAT_HIP_SCALE_* */
    int32_t max_outer;      /* reweighting steps after the first solve, 1 .. DBAT_HIP_ROBUST_MAX_OUTER - 1; default 10 */
    double  weight_tol;     /* stop when max |omega' - omega| <= weight_tol; default 1e-3 */
} dbat_hip_robust_options;

typedef struct dbat_hip_robust_result {
    int32_t outer;          /* inner solves run (1 + reweighting steps applied) */
    int32_t converged;      /* 1: the weights settled within weight_tol */
    int32_t inner_iters[DBAT_HIP_ROBUST_MAX_OUTER];   /* iterations of every inner solve */
    double  scale[DBAT_HIP_ROBUST_MAX_OUTER];         /* scale of every reweighting evaluation (outer entries at most) */
    double  max_change;     /* max |omega' - omega| of the last evaluation */
    double  reweight_s;     /* wall seconds spent in the reweighting evaluations and applications */
} dbat_hip_robust_result;

/* defaults for a loss: k = 1.5 (Huber) or 2.385 (Cauchy), apriori scale, max_outer 10, weight_tol 1e-3 */
int  dbat_hip_default_robust_options(int32_t loss, dbat_hip_robust_options *ropt);

/* One reweighting evaluation at x, not applied: omega [n_obs] and, if not NULL, s_norm [n_obs] in IP column order,
 * and the scale.  On a sharded handle (collective) every rank receives the full vectors. */
int  dbat_hip_robust_weights(dbat_hip_handle *h, const double *x, const dbat_hip_robust_options *ropt,
                             double *omega, double *s_norm, double *scale);

/* Sets omega [n_obs] (IP column order) directly: every value finite and in (0, 1], else DBAT_HIP_EINVAL.  NULL:
 * back to the base weights and the path of a fresh handle. */
int  dbat_hip_set_obs_weights(dbat_hip_handle *h, const double *omega);

/* The IRLS outer loop: omega = 1, solve (dbat_hip_solve with opt); then up to max_outer times: evaluate omega' at
 * x; stop (converged = 1) if max |omega' - omega| <= weight_tol, keeping the omega of the last solve; else apply
 * omega' and solve again from x.  A nonzero code of an inner solve ends the loop.  result, res, damp, aux, trace
 * are those of the last inner solve, as dbat_hip_solve gives them (sigma0: the reweighted one); the handle keeps
 * the weights of the last solve (dbat_hip_final_residuals, dbat_hip_redundancy use them).  omega_out [n_obs] (IP
 * column order, may be NULL): those weights.  Collective on a sharded handle. */
int  dbat_hip_solve_robust(dbat_hip_handle *h, const dbat_hip_options *opt, const dbat_hip_robust_options *ropt,
                           double *x, dbat_hip_result *result, double *res, double *damp, double *aux, double *trace,
                           dbat_hip_robust_result *rr, double *omega_out);

/* Debug / tests, never on the product path: the second half of a reweighting evaluation on the caller's s instead of
 * the residuals' -- the exact median by radix select, the scale (median / sqrt(2 ln 2), 1 if that is 0; 1 with
 * DBAT_HIP_SCALE_APRIORI), the weights and the largest weight change, by the kernels and host code of
 * dbat_hip_solve_robust.  s_ip [n_obs] in IP column order: every value finite with the sign bit clear (so -0.0 is
 * refused), else DBAT_HIP_EINVAL naming the column, before anything is launched.  The host places the bit patterns of
 * this rank's observations in processing order; nothing else differs from a solve, and nothing is applied to the
 * handle.
 *   omega_ip   [n_obs] or NULL: omega' in IP column order, complete on every rank
 *   median     or NULL: the median of s over all ranks (NaN with DBAT_HIP_SCALE_APRIORI, which selects nothing)
 *   scale, max_change   the scale; max |omega' - omega| over all ranks, omega the factors the handle carries
 *              (dbat_hip_set_obs_weights or a robust solve; 1 on a handle that was never promoted)
 *   owned      [n_obs] or NULL: 1 where this rank holds the IP column
 * Collective on a sharded handle: every rank passes the same s_ip and the same set of non-NULL outputs. */
int  dbat_hip_debug_robust_from_s(dbat_hip_handle *h, const double *s_ip, const dbat_hip_robust_options *ropt,
                                  double *omega_ip, double *median, double *scale, double *max_change, uint8_t *owned);

#ifdef __cplusplus
}
#endif
#endif /* DBAT_HIP_H */
