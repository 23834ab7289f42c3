// Least-squares space resection of camera stations (dbat_hip_poseadjust, host side: poseadjust_host.hpp): the pose of a
// camera from its control points, for many cameras in one launch.  One wave of 64 lanes per camera; the whole damped
// loop runs inside the kernel, as in pairadjust.hpp, whose protocol this follows point for point.
//
// Unknowns of a camera: R and the projection centre C.  With pi(Y) = Y(1:2) / Y(3) the residuals of a point are
// w (pi(R (X - C)) - xn).  A step is (c, a): C <- C + c, R <- exp([a]x) R: six unknowns, centre first.  The 6 x 6 normal
// equations are damped with Marquardt's scaling (lambda diag N).  Object coordinates and the centre are taken relative
// to the camera's first used point before anything is multiplied, so coordinates of 1e6 m keep their digits.
//
// Lane l takes the points l, l + 64, ... in ascending order; the 27 sums of the normal equations (21 of the symmetric
// matrix, 6 of the gradient) and the objective, a pair of doubles, are reduced by a shuffle tree of fixed shape and
// handed to every lane from lane 0.  Every lane then solves the same 6 x 6 system and takes the same decisions: the
// loop has no workgroup barrier and no LDS, and its trip count is the same in every lane by construction.  The
// linearisation does not depend on lambda, so a rejected trial solves the sums it has again.  No atomics: two calls
// give the same bits, and a camera gives the same bits alone and inside a batch.
//
// Every loop is bounded: the trial loop by PA_MAX_REJECT * max_iter (max_iter is validated to 1 .. 200 by the host),
// the point loops by the camera's size.  No array is indexed by a run-time value: everything below unrolls.
#pragma once
#include "pairadjust.hpp"
#include "resect.hpp"

namespace dbat {

constexpr int PO_WAVE = 64;
constexpr int PO_NSUM = 27;                 // N (21, po_s6 storage), g (6)
constexpr double PO_PIVOT = 1e-10;          // at the end: a pivot of the undamped N at or below this share of its diagonal entry: singular
constexpr int PO_MIN_POINTS = 3;

__host__ __device__ constexpr int po_s6(int i, int j) { return i <= j ? i * 6 - i * (i - 1) / 2 + (j - i) : j * 6 - j * (j - 1) / 2 + (i - j); }

#if defined(__HIPCC__)

// Cholesky of the 6 x 6 matrix S (po_s6 storage) in place, unrolled: false where a pivot is not above tol times its
// diagonal entry (the pivot is then replaced by one, as pa_chol5 does).
__device__ __forceinline__ bool po_chol6(double *S, double tol) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const double sjj = S[po_s6(j, j)];
        double d = sjj;
#pragma unroll
        for (int k = 0; k < j; ++k) d -= S[po_s6(k, j)] * S[po_s6(k, j)];
        if (!(d > tol * sjj)) { ok = false; d = 1.0; }
        const double l = sqrt(d);
        S[po_s6(j, j)] = l;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = S[po_s6(j, i)];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= S[po_s6(k, i)] * S[po_s6(k, j)];
            S[po_s6(j, i)] = v / l;
        }
    }
    return ok;
}

// x <- (L L')^-1 x with the factor of po_chol6 (L(i, j) at po_s6(j, i), j <= i).
__device__ __forceinline__ void po_solve6(const double *L, double *x) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = x[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v -= L[po_s6(k, i)] * x[k];
        x[i] = v / L[po_s6(i, i)];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double v = x[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) v -= L[po_s6(i, k)] * x[k];
        x[i] = v / L[po_s6(i, i)];
    }
}

// The wave's sum in lane 0 by a shuffle tree, then to every lane.
__device__ __forceinline__ double po_wave_sum(double s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    return __shfl(s, 0, 64);
}
__device__ __forceinline__ PaDD po_wave_sum_dd(PaDD v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = pa_dd_add(v, PaDD{__shfl_down(v.hi, off, 64), __shfl_down(v.lo, off, 64)});
    return PaDD{__shfl(v.hi, 0, 64), __shfl(v.lo, 0, 64)};
}
__device__ __forceinline__ long long po_wave_min(long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const long long o = __shfl_down(v, off, 64); v = o < v ? o : v; }
    return __shfl(v, 0, 64);
}

// Y = R ((X - O) - C) as pairs of doubles (R: 18 entries, the low words from [9]; C relative to O) and the weighted
// residuals rr = w ((Y_k - xn_k Y_3) / Y_3): the form of pa_residuals.  X - O is taken without error.
__device__ __forceinline__ void po_residuals(const double *R, const double *C, const double *O, const double *X, const double *m,
                                             const double *w, PaDD *Y, PaDD *rr) {
    PaDD d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = pa_dd_add(pa_two_sum(X[k], -O[k]), PaDD{-C[k], 0.0});
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        PaDD v = pa_dd_mul(PaDD{R[k], R[9 + k]}, d[0]);
        v = pa_dd_add(v, pa_dd_mul(PaDD{R[3 + k], R[12 + k]}, d[1]));
        Y[k] = pa_dd_add(v, pa_dd_mul(PaDD{R[6 + k], R[15 + k]}, d[2]));
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const PaDD b = pa_dd_fma(Y[k], -m[k], Y[2]);
        rr[k] = pa_dd_fma(PaDD{0.0, 0.0}, w[k], pa_dd_div(b, Y[2]));
    }
}

// The rows of the Jacobian of one point to (c, a) at Y = R (X - C) (float64), A[6 i + j] for residual i.
__device__ __forceinline__ void po_jacobian(const double *R, const double *Y, const double *w, double *A) {
    const double iz = 1.0 / Y[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        // row i of diag(w) d pi / d Y: (1/z, 0, -Y0/z^2), (0, 1/z, -Y1/z^2)
        const double p0 = i == 0 ? w[0] * iz : 0.0, p1 = i == 0 ? 0.0 : w[1] * iz, p2 = -w[i] * Y[i] * iz * iz;
        double *a = A + 6 * i;
#pragma unroll
        for (int j = 0; j < 3; ++j) a[j] = -(p0 * R[3 * j] + p1 * R[3 * j + 1] + p2 * R[3 * j + 2]);      // d Y / d C = -R
        a[3] = p2 * Y[1] - p1 * Y[2];                     // d (a x Y) / d a_j = e_j x Y
        a[4] = p0 * Y[2] - p2 * Y[0];
        a[5] = p1 * Y[0] - p0 * Y[1];
    }
}

// The sums N (po_s6), g of the wave's used points at (R, C), in every lane.
__device__ __forceinline__ void po_linearise(const double *R, const double *C, const double *O, int64_t g0, int64_t g1, int lane,
                                             const double *__restrict__ X, const double *__restrict__ xn, const double *__restrict__ wt,
                                             const uint8_t *__restrict__ used, double *acc) {
#pragma unroll
    for (int i = 0; i < PO_NSUM; ++i) acc[i] = 0.0;
    for (int64_t g = g0 + lane; g < g1; g += PO_WAVE) {
        if (!used[g]) continue;
        const double Xg[3] = {X[3 * g], X[3 * g + 1], X[3 * g + 2]}, m[2] = {xn[2 * g], xn[2 * g + 1]};
        const double w[2] = {wt ? wt[2 * g] : 1.0, wt ? wt[2 * g + 1] : 1.0};
        PaDD Y[3], rr[2];
        po_residuals(R, C, O, Xg, m, w, Y, rr);
        const double Yh[3] = {Y[0].hi, Y[1].hi, Y[2].hi};
        double A[12];
        po_jacobian(R, Yh, w, A);
#pragma unroll
        for (int a = 0; a < 6; ++a) {
#pragma unroll
            for (int c = a; c < 6; ++c) acc[po_s6(a, c)] += A[a] * A[c] + A[6 + a] * A[6 + c];
            acc[21 + a] += A[a] * rr[0].hi + A[6 + a] * rr[1].hi;
        }
    }
#pragma unroll
    for (int i = 0; i < PO_NSUM; ++i) acc[i] = po_wave_sum(acc[i]);
}

// Wave p adjusts camera p: points pt_start[p] .. pt_start[p + 1] of X (3 doubles), xn, wt (2 doubles; wt may be null:
// ones), use (may be null: all).  P [12 p] in/out, used [g] out, dstat [4 p], istat [4 p], Q [36 p] out, res [2 g] out
// or null.
__global__ __launch_bounds__(PO_WAVE) void k_poseadjust(const int64_t *__restrict__ pt_start, const double *__restrict__ X,
                                                        const double *__restrict__ xn, const uint8_t *__restrict__ use,
                                                        const double *__restrict__ wt, int max_iter, double tol2,
                                                        double *__restrict__ P, uint8_t *__restrict__ used,
                                                        double *__restrict__ dstat, int32_t *__restrict__ istat,
                                                        double *__restrict__ Q, double *__restrict__ res) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const int64_t g0 = pt_start[p], g1 = pt_start[p + 1];
    double *Pp = P + 12 * (int64_t)p;
    double R[18], G[18], T[18], t[3], C[3], O[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) { R[i] = Pp[i]; R[9 + i] = 0.0; }
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = Pp[9 + i];

    // ---- selection, once, at the start pose: use is set and the point is in front (the third row of P [X; 1] is
    // negative; its sign from an error-free sum, whatever the size of the coordinates) ------------------------------------
    long long first = 0x7fffffffffffffffLL;
    double cnt = 0.0;
    for (int64_t g = g0 + lane; g < g1; g += PO_WAVE) {
        bool u = !use || use[g];
        if (u) {
            const double Xg[3] = {X[3 * g], X[3 * g + 1], X[3 * g + 2]};
            double h, hl;
            rs_dot2(R[2], R[5], R[8], t[2], Xg, h, hl);
            u = h < 0.0;
        }
        used[g] = u ? 1 : 0;
        if (u) { cnt += 1.0; first = g < first ? (long long)g : first; }
    }
    const int n = (int)po_wave_sum(cnt);
    first = po_wave_min(first);
    const double nan = __builtin_nan("");
    if (n < PO_MIN_POINTS) {                              // the same in every lane
        if (lane == 0) {
            dstat[4 * (int64_t)p] = nan; dstat[4 * (int64_t)p + 1] = nan; dstat[4 * (int64_t)p + 2] = nan; dstat[4 * (int64_t)p + 3] = PA_LAMBDA0;
            istat[4 * (int64_t)p] = PA_TOO_FEW; istat[4 * (int64_t)p + 1] = 0; istat[4 * (int64_t)p + 2] = 0; istat[4 * (int64_t)p + 3] = n;
        }
        if (lane < 36) Q[36 * (int64_t)p + lane] = nan;
        if (res)
            for (int64_t g = g0 + lane; g < g1; g += PO_WAVE) { res[2 * g] = 0.0; res[2 * g + 1] = 0.0; }
        return;
    }
    // the origin: the first used point; the centre -R' t relative to it
#pragma unroll
    for (int k = 0; k < 3; ++k) O[k] = X[3 * first + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) C[k] = -(R[3 * k] * t[0] + R[3 * k + 1] * t[1] + R[3 * k + 2] * t[2]) - O[k];
    pa_orthonormalise(R, G, T);

    // the objective at the start
    PaDD fsum = {0.0, 0.0};
    for (int64_t g = g0 + lane; g < g1; g += PO_WAVE) {
        if (!used[g]) continue;
        const double Xg[3] = {X[3 * g], X[3 * g + 1], X[3 * g + 2]}, m[2] = {xn[2 * g], xn[2 * g + 1]};
        const double w[2] = {wt ? wt[2 * g] : 1.0, wt ? wt[2 * g + 1] : 1.0};
        PaDD Y[3], rr[2];
        po_residuals(R, C, O, Xg, m, w, Y, rr);
        fsum = pa_dd_add(fsum, pa_dd_mul(rr[0], rr[0]));
        fsum = pa_dd_add(fsum, pa_dd_mul(rr[1], rr[1]));
    }
    PaDD f = po_wave_sum_dd(fsum);
    const double f0 = f.hi, floor_f = PA_FLOOR * 2.0 * (double)n;
    double lambda = PA_LAMBDA0;
    int iters = 0, trials = 0, code = PA_MAX_ITER;
    bool fresh = false;                                   // acc holds the sums at (R, C)
    double acc[PO_NSUM];

    // ---- the damped loop ------------------------------------------------------------------------------------------------
    const int max_trials = PA_MAX_REJECT * max_iter;
    for (int trial = 0; trial < max_trials; ++trial) {
        if (!fresh) { po_linearise(R, C, O, g0, g1, lane, X, xn, wt, used, acc); fresh = true; }
        double S[21], dp[6];
#pragma unroll
        for (int i = 0; i < 21; ++i) S[i] = acc[i];
#pragma unroll
        for (int a = 0; a < 6; ++a) { S[po_s6(a, a)] = acc[po_s6(a, a)] + lambda * acc[po_s6(a, a)]; dp[a] = acc[21 + a]; }
        bool ok = po_chol6(S, 0.0);
        po_solve6(S, dp);
        double q = 0.0;
#pragma unroll
        for (int a = 0; a < 6; ++a) { dp[a] = -dp[a]; q -= acc[21 + a] * dp[a]; ok = ok && (dp[a] - dp[a] == 0.0); }
        trials += 1;
        if (f.hi <= floor_f || (ok && q <= tol2 * f.hi)) { code = PA_CONVERGED; break; }
        bool accept = false;
        double Rn[18], Cn[3];
        PaDD ft = {0.0, 0.0};
        if (ok) {
#pragma unroll
            for (int k = 0; k < 3; ++k) Cn[k] = C[k] + dp[k];
            pa_rotate_dd(dp + 3, R, Rn, G, T);
            double nbad = 0.0;
            for (int64_t g = g0 + lane; g < g1; g += PO_WAVE) {
                if (!used[g]) continue;
                const double Xg[3] = {X[3 * g], X[3 * g + 1], X[3 * g + 2]}, m[2] = {xn[2 * g], xn[2 * g + 1]};
                const double w[2] = {wt ? wt[2 * g] : 1.0, wt ? wt[2 * g + 1] : 1.0};
                PaDD Y[3], rr[2];
                po_residuals(Rn, Cn, O, Xg, m, w, Y, rr);
                ft = pa_dd_add(ft, pa_dd_mul(rr[0], rr[0]));
                ft = pa_dd_add(ft, pa_dd_mul(rr[1], rr[1]));
                if (!(Y[2].hi < 0.0)) nbad += 1.0;
            }
            ft = po_wave_sum_dd(ft);
            nbad = po_wave_sum(nbad);
            accept = nbad == 0.0 && (ft.hi - ft.hi == 0.0) && pa_dd_less(ft, f);
        }
        if (accept) {
#pragma unroll
            for (int i = 0; i < 18; ++i) R[i] = Rn[i];
#pragma unroll
            for (int k = 0; k < 3; ++k) C[k] = Cn[k];
            f = ft; lambda = fmax(lambda / 10.0, PA_LAMBDA_MIN); iters += 1; fresh = false;
            if (iters >= max_iter) { code = PA_MAX_ITER; break; }
        } else {
            lambda = lambda * 10.0;
            if (lambda > PA_LAMBDA_MAX) { code = PA_NO_STEP; break; }
        }
    }

    // ---- the end: the residuals of every finite point, the undamped matrix at the returned values, its inverse ---------
#pragma unroll
    for (int i = 0; i < PO_NSUM; ++i) acc[i] = 0.0;
    for (int64_t g = g0 + lane; g < g1; g += PO_WAVE) {
        const bool u = used[g] != 0;
        if (!u && !res) continue;
        const double Xg[3] = {X[3 * g], X[3 * g + 1], X[3 * g + 2]}, m[2] = {xn[2 * g], xn[2 * g + 1]};
        const double w[2] = {wt ? wt[2 * g] : 1.0, wt ? wt[2 * g + 1] : 1.0};
        PaDD Y[3], rr[2];
        po_residuals(R, C, O, Xg, m, w, Y, rr);
        if (res) {
            const bool fin = (rr[0].hi - rr[0].hi == 0.0) && (rr[1].hi - rr[1].hi == 0.0);
            res[2 * g] = fin ? rr[0].hi : 0.0; res[2 * g + 1] = fin ? rr[1].hi : 0.0;
        }
        if (!u) continue;
        const double Yh[3] = {Y[0].hi, Y[1].hi, Y[2].hi};
        double A[12];
        po_jacobian(R, Yh, w, A);
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int c = a; c < 6; ++c) acc[po_s6(a, c)] += A[a] * A[c] + A[6 + a] * A[6 + c];
    }
    double S[21];
#pragma unroll
    for (int i = 0; i < 21; ++i) S[i] = po_wave_sum(acc[i]);
    bool singular = !po_chol6(S, PO_PIVOT);
    double Qc[36];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        double e[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) e[r] = r == c ? 1.0 : 0.0;
        po_solve6(S, e);
#pragma unroll
        for (int r = 0; r < 6; ++r) { Qc[6 * c + r] = e[r]; singular = singular || !(e[r] - e[r] == 0.0); }
    }
    if (lane == 0) {
        double *Qp = Q + 36 * (int64_t)p;
#pragma unroll
        for (int i = 0; i < 36; ++i) Qp[i] = singular ? nan : Qc[i];
        if (code == PA_CONVERGED && singular) code = PA_SINGULAR;
#pragma unroll
        for (int i = 0; i < 9; ++i) Pp[i] = R[i];
        // t = -R C with C = O + (C - O): the two products apart, so that the small one keeps its digits
#pragma unroll
        for (int r = 0; r < 3; ++r)
            Pp[9 + r] = -((R[r] * O[0] + R[3 + r] * O[1] + R[6 + r] * O[2]) + (R[r] * C[0] + R[3 + r] * C[1] + R[6 + r] * C[2]));
        dstat[4 * (int64_t)p] = f0; dstat[4 * (int64_t)p + 1] = f.hi;
        dstat[4 * (int64_t)p + 2] = n > 3 ? sqrt(f.hi / (double)(2 * n - 6)) : nan;
        dstat[4 * (int64_t)p + 3] = lambda;
        istat[4 * (int64_t)p] = code; istat[4 * (int64_t)p + 1] = iters; istat[4 * (int64_t)p + 2] = trials; istat[4 * (int64_t)p + 3] = n;
    }
}

#endif  // __HIPCC__

}  // namespace dbat
