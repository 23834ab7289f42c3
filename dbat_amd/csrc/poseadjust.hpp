// Least-squares space resection of camera stations (dbat_hip_poseadjust, host side: poseadjust_host.hpp): the pose of a
// camera from its control points, for many cameras in one launch.  One wave of 64 lanes per camera; the whole damped
// loop runs inside the kernel, by the protocol of lm_core.hpp.
//
// Unknowns of a camera: R and the projection centre C.  With pi(Y) = Y(1:2) / Y(3) the residuals of a point are
// w (pi(R (X - C)) - xn).  A step is (c, a): C <- C + c, R <- exp([a]x) R: six unknowns, centre first.  The 6 x 6 normal
// equations are damped with Marquardt's scaling (lambda diag N).  Object coordinates and the centre are taken relative
// to the camera's first used point before anything is multiplied, so coordinates of 1e6 m keep their digits.
//
// Lane l takes the points l, l + 64, ... in ascending order; the 27 sums of the normal equations (21 of the symmetric
// matrix, 6 of the gradient) and the objective, a pair of doubles, are reduced by __shfl_xor of width 64: a tree of fixed
// shape that leaves the result in every lane (grp_sum of lm_core.hpp), every shuffle in control flow that is uniform over
// the wave.  Every lane then solves the same 6 x 6 system and takes the same decisions: the loop has no workgroup barrier
// and no LDS, and its trip count is the same in every lane by construction.  The linearisation does not depend on lambda,
// so a rejected trial solves the sums it has again.  No atomics: two calls give the same bits, and a camera gives the
// same bits alone and inside a batch.
//
// Every loop is bounded: the trial loop by LM_MAX_REJECT * max_iter (max_iter is validated to 1 .. 200 by the host),
// the point loops by the camera's size.  No array is indexed by a run-time value: everything below unrolls.
#pragma once
#include "lm_core.hpp"
#include "resect.hpp"

namespace dbat {

constexpr int PO_WAVE = 64;
constexpr int PO_NSUM = 27;                 // N (21, sym_ix<6> storage), g (6)
constexpr int PO_MIN_POINTS = 3;

#if defined(__HIPCC__)

// Y = R ((X - O) - C) as pairs of doubles (R: 18 entries, the low words from [9]; C relative to O) and the weighted
// residuals rr = w ((Y_k - xn_k Y_3) / Y_3): the form of pa_residuals (pairadjust.hpp).  X - O is taken without error.
__device__ __forceinline__ void po_residuals(const double *R, const double *C, const double *O, const double *X, const double *m,
                                             const double *w, Dd *Y, Dd *rr) {
    Dd d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = dd_add(dd_two_sum(X[k], -O[k]), Dd{-C[k], 0.0});
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        Dd v = dd_mul(Dd{R[k], R[9 + k]}, d[0]);
        v = dd_add(v, dd_mul(Dd{R[3 + k], R[12 + k]}, d[1]));
        Y[k] = dd_add(v, dd_mul(Dd{R[6 + k], R[15 + k]}, d[2]));
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const Dd b = dd_fma(Y[k], -m[k], Y[2]);
        rr[k] = dd_fma(Dd{0.0, 0.0}, w[k], dd_div(b, Y[2]));
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

// Point g: its coordinates, its image point m and the weights w, ones where none are given.
struct PoObs { double X[3], m[2], w[2]; };
__device__ __forceinline__ PoObs po_load(int64_t g, const double *__restrict__ X, const double *__restrict__ xn, const double *__restrict__ wt) {
    return {{X[3 * g], X[3 * g + 1], X[3 * g + 2]}, {xn[2 * g], xn[2 * g + 1]}, {wt ? wt[2 * g] : 1.0, wt ? wt[2 * g + 1] : 1.0}};
}

// acc[0 .. 20] += A' A of the point's two rows (sym_ix<6> storage)
__device__ __forceinline__ void po_add_normal(const double *A, double *acc) {
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int c = a; c < 6; ++c) acc[sym_ix<6>(a, c)] += A[a] * A[c] + A[6 + a] * A[6 + c];
}

// The sums N, g of the wave's used points at (R, C), in every lane.  END, the pass at the returned values: N alone, and the
// residuals of every finite point, used or not, to res (if not null).
template <bool END>
__device__ __forceinline__ void po_linearise(const double *R, const double *C, const double *O, int64_t g0, int64_t g1, int lane,
                                             const double *__restrict__ X, const double *__restrict__ xn, const double *__restrict__ wt,
                                             const uint8_t *__restrict__ used, double *__restrict__ res, double *acc) {
    constexpr int NS = END ? 21 : PO_NSUM;
#pragma unroll
    for (int i = 0; i < NS; ++i) acc[i] = 0.0;
    for (int64_t g = g0 + lane; g < g1; g += PO_WAVE) {
        const bool u = used[g] != 0;
        if (!u && !(END && res)) continue;
        const PoObs o = po_load(g, X, xn, wt);
        Dd Y[3], rr[2];
        po_residuals(R, C, O, o.X, o.m, o.w, Y, rr);
        if (END && res) {
            const bool fin = (rr[0].hi - rr[0].hi == 0.0) && (rr[1].hi - rr[1].hi == 0.0);
            res[2 * g] = fin ? rr[0].hi : 0.0; res[2 * g + 1] = fin ? rr[1].hi : 0.0;
        }
        if (!u) continue;
        const double Yh[3] = {Y[0].hi, Y[1].hi, Y[2].hi};
        double A[12];
        po_jacobian(R, Yh, o.w, A);
        po_add_normal(A, acc);
#pragma unroll
        for (int a = 0; a < (END ? 0 : 6); ++a) acc[21 + a] += A[a] * rr[0].hi + A[6 + a] * rr[1].hi;
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) acc[i] = grp_sum<PO_WAVE>(acc[i]);
}

// The objective of the wave's used points at (R, C) (a pair of doubles) and the number of them that are not in front.
__device__ __forceinline__ Dd po_objective(const double *R, const double *C, const double *O, int64_t g0, int64_t g1, int lane,
                                           const double *__restrict__ X, const double *__restrict__ xn, const double *__restrict__ wt,
                                           const uint8_t *__restrict__ used, double &nbad) {
    Dd f = {0.0, 0.0};
    double bad = 0.0;
    for (int64_t g = g0 + lane; g < g1; g += PO_WAVE) {
        if (!used[g]) continue;
        const PoObs o = po_load(g, X, xn, wt);
        Dd Y[3], rr[2];
        po_residuals(R, C, O, o.X, o.m, o.w, Y, rr);
        f = dd_add(f, dd_mul(rr[0], rr[0]));
        f = dd_add(f, dd_mul(rr[1], rr[1]));
        if (!(Y[2].hi < 0.0)) bad += 1.0;
    }
    nbad = grp_sum<PO_WAVE>(bad);
    return grp_sum_dd<PO_WAVE>(f);
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
    const int n = (int)grp_sum<PO_WAVE>(cnt);
    first = grp_min<PO_WAVE>(first);

    // ---- too few ----------------------------------------------------------------------------------------------------------
    const double nan = __builtin_nan("");
    if (n < PO_MIN_POINTS) {                              // the same in every lane
        if (lane == 0) lm_store_too_few(dstat, istat, p, n);
        if (lane < 36) Q[36 * (int64_t)p + lane] = nan;
        if (res)
            for (int64_t g = g0 + lane; g < g1; g += PO_WAVE) { res[2 * g] = 0.0; res[2 * g + 1] = 0.0; }
        return;
    }

    // ---- the origin: the first used point; the centre -R' t relative to it ------------------------------------------------
#pragma unroll
    for (int k = 0; k < 3; ++k) O[k] = X[3 * first + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) C[k] = -(R[3 * k] * t[0] + R[3 * k + 1] * t[1] + R[3 * k + 2] * t[2]) - O[k];
    dd_orthonormalise(R, G, T);

    // ---- the objective at the start ---------------------------------------------------------------------------------------
    double behind;                                        // (none: the selection left those out)
    LmState lm = lm_start(po_objective(R, C, O, g0, g1, lane, X, xn, wt, used, behind));
    const double f0 = lm.f.hi, floor_f = LM_FLOOR * 2.0 * (double)n;
    bool fresh = false;                                   // acc holds the sums at (R, C)
    double acc[PO_NSUM];

    // ---- the damped loop ------------------------------------------------------------------------------------------------
    const int max_trials = LM_MAX_REJECT * max_iter;
    for (int trial = 0; trial < max_trials; ++trial) {
        if (!fresh) { po_linearise<false>(R, C, O, g0, g1, lane, X, xn, wt, used, nullptr, acc); fresh = true; }
        double S[21], dp[6];
#pragma unroll
        for (int i = 0; i < 21; ++i) S[i] = acc[i];
#pragma unroll
        for (int a = 0; a < 6; ++a) { S[sym_ix<6>(a, a)] = acc[sym_ix<6>(a, a)] + lm.lambda * acc[sym_ix<6>(a, a)]; dp[a] = acc[21 + a]; }
        bool ok = sym_chol<6>(S, 0.0);
        sym_solve<6>(S, dp);
        double q = 0.0;
#pragma unroll
        for (int a = 0; a < 6; ++a) { dp[a] = -dp[a]; q -= acc[21 + a] * dp[a]; ok = ok && (dp[a] - dp[a] == 0.0); }
        lm = lm_converged(lm, ok, q, floor_f, tol2);
        if (lm.stop) break;                               // before the trial's objective is paid for
        double Rn[18], Cn[3];
        Dd ft = {0.0, 0.0};
        double nbad = 0.0;
        if (ok) {
#pragma unroll
            for (int k = 0; k < 3; ++k) Cn[k] = C[k] + dp[k];
            dd_rotate_dd(dp + 3, R, Rn, G, T);
            ft = po_objective(Rn, Cn, O, g0, g1, lane, X, xn, wt, used, nbad);
        }
        const bool accept = lm_accept(lm, ok, nbad, ft);
        if (accept) {
#pragma unroll
            for (int i = 0; i < 18; ++i) R[i] = Rn[i];
#pragma unroll
            for (int k = 0; k < 3; ++k) C[k] = Cn[k];
            fresh = false;
        }
        lm = lm_step(lm, accept, ft, max_iter);
        if (lm.stop) break;
    }

    // ---- the end: the residuals of every finite point, the undamped matrix at the returned values, its inverse ---------
    po_linearise<true>(R, C, O, g0, g1, lane, X, xn, wt, used, res, acc);
    double Qc[36];
    bool singular = !sym_chol<6>(acc, LM_PIVOT);
    singular = sym_inverse<6>(acc, Qc) || singular;
    if (lane == 0) {
        double *Qp = Q + 36 * (int64_t)p;
#pragma unroll
        for (int i = 0; i < 36; ++i) Qp[i] = singular ? nan : Qc[i];
#pragma unroll
        for (int i = 0; i < 9; ++i) Pp[i] = R[i];
        // t = -R C with C = O + (C - O): the two products apart, so that the small one keeps its digits
#pragma unroll
        for (int r = 0; r < 3; ++r)
            Pp[9 + r] = -((R[r] * O[0] + R[3 + r] * O[1] + R[6 + r] * O[2]) + (R[r] * C[0] + R[3 + r] * C[1] + R[6 + r] * C[2]));
        lm_store_stats(dstat, istat, p, f0, lm, singular, n, 2 * n - 6);
    }
}

#endif  // __HIPCC__

}  // namespace dbat
