// What the damped loops of k_pairadjust (pairadjust.hpp), k_poseadjust (poseadjust.hpp) and k_pointadjust
// (pointadjust.hpp) share, so that the rules include/dbat_hip.h promises for the three calls are one piece of code: the
// constants and codes, the packed symmetric factorisation, the group reductions, the decisions of a trial and the statistics
// of an item.  (k_pairadjust takes the constants and the factorisations; pairadjust.hpp says why no more.)
//
// The protocol.  Selection of the observations, once, at the start values; fewer than the problem needs: code 4.  Then
// trials at lambda, from LM_LAMBDA0: solve the normal equations damped with Marquardt's scaling; with q = -g' delta the
// predicted decrease, stop as converged where f <= floor or q <= tol^2 f (lm_converged: on every trial, before the
// step is judged); accept the trial where it solved, left nothing behind a camera and its objective, a finite pair of
// doubles, is strictly smaller (lm_accept); an accepted trial divides lambda by ten and counts as an iteration, a
// rejected one multiplies it by ten (lm_step: code 1 at max_iter iterations, code 2 once lambda exceeds LM_LAMBDA_MAX).
// At the end the undamped matrix at the returned values is factored with the pivot test LM_PIVOT and inverted: where
// that fails Q is NaN and a converged item has code 3 (lm_store_stats).
#pragma once
#include "dd.hpp"

namespace dbat {

constexpr double LM_LAMBDA0 = 1e-3, LM_LAMBDA_MIN = 1e-12, LM_LAMBDA_MAX = 1e8;
constexpr double LM_FLOOR = 1e-24;          // f <= LM_FLOOR * residuals: converged (a noise-free item never meets q <= tol^2 f)
constexpr double LM_PIVOT = 1e-10;          // at the end: a pivot of the undamped matrix at or below this share of its diagonal entry: singular
// Consecutive rejections at most: lambda is at least LM_LAMBDA_MIN, a rejection multiplies it by ten, and the call ends
// once it exceeds LM_LAMBDA_MAX: 1e-12 * 10^21 = 1e9.  An iteration is therefore at most 20 rejected trials and the
// accepted one, or 21 rejected ones and the end: LM_MAX_REJECT * max_iter trials bound the whole loop.
constexpr int LM_MAX_REJECT = 21;
enum { LM_CONVERGED = 0, LM_MAX_ITER = 1, LM_NO_STEP = 2, LM_SINGULAR = 3, LM_TOO_FEW = 4 };

// ---- symmetric N x N matrices, the upper triangle packed by rows ----------------------------------------------------------
template <int N>
__host__ __device__ constexpr int sym_ix(int i, int j) { return i <= j ? i * N - i * (i - 1) / 2 + (j - i) : j * N - j * (j - 1) / 2 + (i - j); }

// Cholesky of S in place, unrolled: false where a pivot is not above tol times its diagonal entry (the pivot is then
// replaced by one, so that everything after it stays finite).
template <int N>
__host__ __device__ __forceinline__ bool sym_chol(double *S, double tol) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const double sjj = S[sym_ix<N>(j, j)];
        double d = sjj;
#pragma unroll
        for (int k = 0; k < j; ++k) d -= S[sym_ix<N>(k, j)] * S[sym_ix<N>(k, j)];
        if (!(d > tol * sjj)) { ok = false; d = 1.0; }
        const double l = sqrt(d);
        S[sym_ix<N>(j, j)] = l;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double v = S[sym_ix<N>(j, i)];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= S[sym_ix<N>(k, i)] * S[sym_ix<N>(k, j)];
            S[sym_ix<N>(j, i)] = v / l;
        }
    }
    return ok;
}

// x <- (L L')^-1 x with the factor of sym_chol (L(i, j) at sym_ix(j, i), j <= i).
template <int N>
__host__ __device__ __forceinline__ void sym_solve(const double *L, double *x) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double v = x[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v -= L[sym_ix<N>(k, i)] * x[k];
        x[i] = v / L[sym_ix<N>(i, i)];
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double v = x[i];
#pragma unroll
        for (int k = i + 1; k < N; ++k) v -= L[sym_ix<N>(i, k)] * x[k];
        x[i] = v / L[sym_ix<N>(i, i)];
    }
}

// Q (N x N, column by column) <- (L L')^-1 through the factor: true where an entry is not finite.
template <int N>
__host__ __device__ __forceinline__ bool sym_inverse(const double *L, double *Q) {
    bool singular = false;
#pragma unroll
    for (int c = 0; c < N; ++c) {
#pragma unroll
        for (int r = 0; r < N; ++r) Q[N * c + r] = r == c ? 1.0 : 0.0;
        sym_solve<N>(L, Q + N * c);
#pragma unroll
        for (int r = 0; r < N; ++r) singular = singular || !(Q[N * c + r] - Q[N * c + r] == 0.0);
    }
    return singular;
}

#if defined(__HIPCC__)

// Cholesky of V + lambda diag V (3 x 3) into L (00 10 20 11 21 22): false where a pivot is not above tol times the
// diagonal entry of V.  (Not sym_chol<3>: lambda is folded in and a failed pivot is not replaced.)
__device__ __forceinline__ bool lm_chol3(const double *V, double lambda, double tol, double *L) {
    const double d0 = V[0] + lambda * V[0];
    bool ok = d0 > tol * V[0];
    L[0] = sqrt(d0); L[1] = V[1] / L[0]; L[2] = V[2] / L[0];
    const double d1 = V[3] + lambda * V[3] - L[1] * L[1];
    ok = ok && d1 > tol * V[3];
    L[3] = sqrt(d1); L[4] = (V[4] - L[2] * L[1]) / L[3];
    const double d2 = V[5] + lambda * V[5] - L[2] * L[2] - L[4] * L[4];
    ok = ok && d2 > tol * V[5];
    L[5] = sqrt(d2);
    return ok;
}

__device__ __forceinline__ void lm_solve3(const double *L, const double *b, double *x) {
    const double y0 = b[0] / L[0];
    const double y1 = (b[1] - L[1] * y0) / L[3];
    const double y2 = (b[2] - L[2] * y0 - L[4] * y1) / L[5];
    x[2] = y2 / L[5];
    x[1] = (y1 - L[4] * x[2]) / L[3];
    x[0] = (y0 - L[1] * x[1] - L[2] * x[2]) / L[0];
}

// ---- reductions over the groups of W consecutive lanes of a wave -----------------------------------------------------------
// __shfl_xor butterflies: a tree of fixed shape that leaves the result in every lane of the group -- the same bits in each,
// since a + b and dd_add(a, b) do not depend on the order of their operands (two-sum returns the exact error either
// way).  Every call must sit where all W lanes of the group are active.
template <int W>
__device__ __forceinline__ double grp_sum(double s) {
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, W);
    return s;
}
template <int W>
__device__ __forceinline__ Dd grp_sum_dd(Dd v) {
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) v = dd_add(v, Dd{__shfl_xor(v.hi, off, W), __shfl_xor(v.lo, off, W)});
    return v;
}
template <int W>
__device__ __forceinline__ long long grp_min(long long v) {
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) { const long long o = __shfl_xor(v, off, W); v = o < v ? o : v; }
    return v;
}

// ---- the decisions of a trial ---------------------------------------------------------------------------------------------
// The state goes in and comes out by value: a reference to a state held in registers is a generic pointer to private
// memory until late in the compilation, and cost k_poseadjust its second wave per SIMD (280 registers for 246).
struct LmState { double lambda; Dd f; int iters, trials, code; bool stop; };       // f: the objective at the accepted values; stop: the loop ends

__device__ __forceinline__ LmState lm_start(Dd f0) { return {LM_LAMBDA0, f0, 0, 0, LM_MAX_ITER, false}; }

// Counts the trial whose step solved (ok) with the predicted decrease q; converged: the loop ends with code 0.
__device__ __forceinline__ LmState lm_converged(LmState s, bool ok, double q, double floor_f, double tol2) {
    s.trials += 1;
    if (s.f.hi <= floor_f || (ok && q <= tol2 * s.f.hi)) { s.code = LM_CONVERGED; s.stop = true; }
    return s;
}

// The accept test of a trial that solved (ok) with objective ft and `bad` observations it may not have.
__device__ __forceinline__ bool lm_accept(LmState s, bool ok, double bad, Dd ft) {
    return ok && bad == 0.0 && (ft.hi - ft.hi == 0.0) && dd_less(ft, s.f);
}

// Takes the trial or not; the loop ends at max_iter iterations (code 1) and where lambda has no room left (code 2).
__device__ __forceinline__ LmState lm_step(LmState s, bool accept, Dd ft, int max_iter) {
    if (accept) {
        s.f = ft; s.lambda = fmax(s.lambda / 10.0, LM_LAMBDA_MIN); s.iters += 1;
        if (s.iters >= max_iter) { s.code = LM_MAX_ITER; s.stop = true; }
    } else {
        s.lambda = s.lambda * 10.0;
        if (s.lambda > LM_LAMBDA_MAX) { s.code = LM_NO_STEP; s.stop = true; }
    }
    return s;
}

// ---- the statistics of item p: dstat (f0, f, sigma0, lambda), istat (code, iterations, trials, n used) ---------------------
__device__ __forceinline__ void lm_store_too_few(double *dstat, int32_t *istat, int64_t p, int n) {
    const double nan = __builtin_nan("");
    dstat[4 * p] = nan; dstat[4 * p + 1] = nan; dstat[4 * p + 2] = nan; dstat[4 * p + 3] = LM_LAMBDA0;
    istat[4 * p] = LM_TOO_FEW; istat[4 * p + 1] = 0; istat[4 * p + 2] = 0; istat[4 * p + 3] = n;
}

// A converged item whose matrix is singular at the end has code 3; sigma0 needs a redundancy dof > 0.
__device__ __forceinline__ void lm_store_stats(double *dstat, int32_t *istat, int64_t p, double f0, LmState s, bool singular, int n, int dof) {
    dstat[4 * p] = f0; dstat[4 * p + 1] = s.f.hi;
    dstat[4 * p + 2] = dof > 0 ? sqrt(s.f.hi / (double)dof) : __builtin_nan("");
    dstat[4 * p + 3] = s.lambda;
    istat[4 * p] = s.code == LM_CONVERGED && singular ? LM_SINGULAR : s.code; istat[4 * p + 1] = s.iters; istat[4 * p + 2] = s.trials; istat[4 * p + 3] = n;
}

#endif  // __HIPCC__

}  // namespace dbat
