// Least-squares forward intersection (dbat_hip_pointadjust, host side: intersect_host.hpp): an object point from its image
// rays, for many points in one launch.  A group of IA_LANES = 8 lanes per point, eight points per wave (the precedent:
// ANG_LIGHT_LANES of angles.hpp); the whole damped loop runs inside the kernel, by the protocol of lm_core.hpp.
//
// Unknowns of a point: X.  With pi(Y) = Y(1:2) / Y(3) the residuals of a ray are w (pi(R (X - C)) - xn), R and C of the
// ray's camera.  The 3 x 3 normal equations are damped with Marquardt's scaling (lambda diag N).  X and the centres are
// taken relative to the projection centre of the point's first used ray before anything is multiplied, so coordinates of
// 1e6 m keep their digits; the centres -R' t are formed as pairs of doubles.
//
// Lane l of a group takes the rays l, l + 8, ... in ascending order; the 9 sums of the normal equations (6 of the
// symmetric matrix, 3 of the gradient) and the objective, a pair of doubles, are reduced by __shfl_xor of width 8: a tree
// of fixed shape that leaves the result in every lane of the group (grp_sum of lm_core.hpp).  The eight lanes then solve the same 3 x 3 system and
// take the same decisions.  The groups of a wave run different trip counts, so every shuffle sits where all eight lanes
// of its group are active: outside the ray loops, in control flow whose conditions are the group's reduced values.  No
// LDS, no barrier, no atomics: two calls give the same bits, and a point gives the same bits alone and in a batch,
// wherever it lands in a wave.
//
// Every loop is bounded: the trial loop by LM_MAX_REJECT * max_iter (max_iter is validated to 1 .. 200 by the host),
// the ray loops by the point's size.  No array is indexed by a run-time value: everything below unrolls.
#pragma once
#include "lm_core.hpp"
#include "resect.hpp"

namespace dbat {

constexpr int IA_WG = 256;
constexpr int IA_LANES = 8;                 // lanes of a point
constexpr int IA_POINTS = IA_WG / IA_LANES; // points of a workgroup
constexpr int IA_NSUM = 9;                  // N (00 01 02 11 12 22), g (3)
constexpr int IA_MIN_RAYS = 2;

#if defined(__HIPCC__)

// The projection centre -R' t of P (column-major 3 x 4) as pairs of doubles.
__device__ __forceinline__ void ia_centre(const double *P, Dd *C) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const Dd s = dd_add(dd_add(dd_two_prod(P[3 * k], P[9]), dd_two_prod(P[3 * k + 1], P[10])), dd_two_prod(P[3 * k + 2], P[11]));
        C[k] = Dd{-s.hi, -s.lo};
    }
}

// Y = R ((x + O) - C) as pairs of doubles (x: the point relative to O; C: the camera's centre) and the weighted residuals
// rr = w ((Y_k - xn_k Y_3) / Y_3): the form of po_residuals (poseadjust.hpp).
__device__ __forceinline__ void ia_residuals(const double *P, const double *x, const double *O, const double *m, const double *w,
                                             Dd *Y, Dd *rr) {
    Dd C[3], d[3];
    ia_centre(P, C);
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = dd_add(Dd{x[k], 0.0}, dd_add(Dd{O[k], 0.0}, Dd{-C[k].hi, -C[k].lo}));
#pragma unroll
    for (int k = 0; k < 3; ++k)
        Y[k] = dd_fma(dd_fma(dd_fma(Dd{0.0, 0.0}, P[k], d[0]), P[3 + k], d[1]), P[6 + k], d[2]);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const Dd b = dd_fma(Y[k], -m[k], Y[2]);
        rr[k] = dd_fma(Dd{0.0, 0.0}, w[k], dd_div(b, Y[2]));
    }
}

// The rows of the Jacobian of one ray to X at Y = R (X - C) (float64), A[3 i + j] for residual i: diag(w) d pi / d Y R.
__device__ __forceinline__ void ia_jacobian(const double *P, const double *Y, const double *w, double *A) {
    const double iz = 1.0 / Y[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const double p0 = i == 0 ? w[0] * iz : 0.0, p1 = i == 0 ? 0.0 : w[1] * iz, p2 = -w[i] * Y[i] * iz * iz;
#pragma unroll
        for (int j = 0; j < 3; ++j) A[3 * i + j] = p0 * P[3 * j] + p1 * P[3 * j + 1] + p2 * P[3 * j + 2];
    }
}

// Ray g: its camera Pc (column-major 3 x 4), its image point m and the weights w, ones where none are given.
struct IaObs { double Pc[12], m[2], w[2]; };
__device__ __forceinline__ IaObs ia_load(int64_t g, const int32_t *__restrict__ cam, const double *__restrict__ xn, const double *__restrict__ P,
                                         const double *__restrict__ wt) {
    const double *pc = P + 12 * (int64_t)cam[g];
    return {{pc[0], pc[1], pc[2], pc[3], pc[4], pc[5], pc[6], pc[7], pc[8], pc[9], pc[10], pc[11]}, {xn[2 * g], xn[2 * g + 1]},
            {wt ? wt[2 * g] : 1.0, wt ? wt[2 * g + 1] : 1.0}};
}

// acc[0 .. 5] += A' A of the ray's two rows (00 01 02 11 12 22)
__device__ __forceinline__ void ia_add_normal(const double *A, double *acc) {
    acc[0] += A[0] * A[0] + A[3] * A[3]; acc[1] += A[0] * A[1] + A[3] * A[4]; acc[2] += A[0] * A[2] + A[3] * A[5];
    acc[3] += A[1] * A[1] + A[4] * A[4]; acc[4] += A[1] * A[2] + A[4] * A[5]; acc[5] += A[2] * A[2] + A[5] * A[5];
}

// The sums N, g of the group's used rays at x, in every lane of the group.  END, the pass at the returned point: N alone,
// and the residuals of every finite ray, used or not, to res (if not null).
template <bool END>
__device__ __forceinline__ void ia_linearise(const double *x, const double *O, int64_t g0, int64_t g1, int l,
                                             const int32_t *__restrict__ cam, const double *__restrict__ xn,
                                             const double *__restrict__ P, const double *__restrict__ wt,
                                             const uint8_t *__restrict__ used, double *__restrict__ res, double *acc) {
    constexpr int NS = END ? 6 : IA_NSUM;
#pragma unroll
    for (int i = 0; i < NS; ++i) acc[i] = 0.0;
    for (int64_t g = g0 + l; g < g1; g += IA_LANES) {
        const bool u = used[g] != 0;
        if (!u && !(END && res)) continue;
        const IaObs o = ia_load(g, cam, xn, P, wt);
        Dd Y[3], rr[2];
        ia_residuals(o.Pc, x, O, o.m, o.w, Y, rr);
        if (END && res) {
            const bool fin = (rr[0].hi - rr[0].hi == 0.0) && (rr[1].hi - rr[1].hi == 0.0);
            res[2 * g] = fin ? rr[0].hi : 0.0; res[2 * g + 1] = fin ? rr[1].hi : 0.0;
        }
        if (!u) continue;
        const double Yh[3] = {Y[0].hi, Y[1].hi, Y[2].hi};
        double A[6];
        ia_jacobian(o.Pc, Yh, o.w, A);
        ia_add_normal(A, acc);
#pragma unroll
        for (int j = 0; j < (END ? 0 : 3); ++j) acc[6 + j] += A[j] * rr[0].hi + A[3 + j] * rr[1].hi;
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) acc[i] = grp_sum<IA_LANES>(acc[i]);
}

// The objective of the group's used rays at x (a pair of doubles) and the number of them that are not in front.
__device__ __forceinline__ Dd ia_objective(const double *x, const double *O, int64_t g0, int64_t g1, int l,
                                             const int32_t *__restrict__ cam, const double *__restrict__ xn,
                                             const double *__restrict__ P, const double *__restrict__ wt,
                                             const uint8_t *__restrict__ used, double &nbad) {
    Dd f = {0.0, 0.0};
    double bad = 0.0;
    for (int64_t g = g0 + l; g < g1; g += IA_LANES) {
        if (!used[g]) continue;
        const IaObs o = ia_load(g, cam, xn, P, wt);
        Dd Y[3], rr[2];
        ia_residuals(o.Pc, x, O, o.m, o.w, Y, rr);
        f = dd_add(f, dd_mul(rr[0], rr[0]));
        f = dd_add(f, dd_mul(rr[1], rr[1]));
        if (!(Y[2].hi < 0.0)) bad += 1.0;
    }
    nbad = grp_sum<IA_LANES>(bad);
    return grp_sum_dd<IA_LANES>(f);
}

// Group q of workgroup b adjusts point p = 32 b + q: rays ray_start[p] .. ray_start[p + 1] of cam, xn, wt (2 doubles; wt
// may be null: ones), use (may be null: all).  P [12 cam].  X [3 p] in/out, used [g] out, dstat [4 p], istat [4 p],
// Q [9 p] out, res [2 g] out or null.
__global__ __launch_bounds__(IA_WG) void k_pointadjust(int n_points, const int64_t *__restrict__ ray_start,
                                                       const int32_t *__restrict__ cam, const double *__restrict__ xn,
                                                       const double *__restrict__ P, const uint8_t *__restrict__ use,
                                                       const double *__restrict__ wt, int max_iter, double tol2,
                                                       double *__restrict__ X, uint8_t *__restrict__ used,
                                                       double *__restrict__ dstat, int32_t *__restrict__ istat,
                                                       double *__restrict__ Q, double *__restrict__ res) {
    const int p = (int)blockIdx.x * IA_POINTS + (int)(threadIdx.x / IA_LANES), l = threadIdx.x % IA_LANES;
    if (p >= n_points) return;                            // the same in the eight lanes of a group
    const int64_t g0 = ray_start[p], g1 = ray_start[p + 1];
    double *Xp = X + 3 * (int64_t)p;
    const double X0[3] = {Xp[0], Xp[1], Xp[2]};

    // ---- selection, once, at the start point: use is set and the point is in front of the ray's camera (the third row
    // of P [X; 1] is negative; its sign from an error-free sum, whatever the size of the coordinates) -----------------------
    long long first = 0x7fffffffffffffffLL;
    double cnt = 0.0;
    for (int64_t g = g0 + l; g < g1; g += IA_LANES) {
        bool u = !use || use[g];
        if (u) {
            const double *pc = P + 12 * (int64_t)cam[g];
            double h, hl;
            rs_dot2(pc[2], pc[5], pc[8], pc[11], X0, h, hl);
            u = h < 0.0;
        }
        used[g] = u ? 1 : 0;
        if (u) { cnt += 1.0; first = g < first ? (long long)g : first; }
    }
    const int n = (int)grp_sum<IA_LANES>(cnt);
    first = grp_min<IA_LANES>(first);

    // ---- too few ----------------------------------------------------------------------------------------------------------
    const double nan = __builtin_nan("");
    if (n < IA_MIN_RAYS) {                                // the same in every lane of the group
        if (l == 0) lm_store_too_few(dstat, istat, p, n);
        Q[9 * (int64_t)p + l] = nan;
        if (l == 0) Q[9 * (int64_t)p + 8] = nan;
        if (res)
            for (int64_t g = g0 + l; g < g1; g += IA_LANES) { res[2 * g] = 0.0; res[2 * g + 1] = 0.0; }
        return;
    }

    // ---- the origin: the projection centre of the first used ray (its high words); the point relative to it -------------
    double O[3], x[3];
    {
        Dd C[3];
        ia_centre(ia_load(first, cam, xn, P, wt).Pc, C);
#pragma unroll
        for (int k = 0; k < 3; ++k) { O[k] = C[k].hi; x[k] = X0[k] - O[k]; }
    }
    // (every loop below reads `used` of the rays its own lane wrote above: lane l always takes the rays l, l + 8, ...)

    // ---- the objective at the start ---------------------------------------------------------------------------------------
    double behind;                                        // (none: the selection left those out)
    LmState lm = lm_start(ia_objective(x, O, g0, g1, l, cam, xn, P, wt, used, behind));
    const double f0 = lm.f.hi, floor_f = LM_FLOOR * 2.0 * (double)n;
    bool fresh = false;                                   // acc holds the sums at x
    double acc[IA_NSUM];

    // ---- the damped loop ------------------------------------------------------------------------------------------------
    const int max_trials = LM_MAX_REJECT * max_iter;
    for (int trial = 0; trial < max_trials; ++trial) {
        if (!fresh) { ia_linearise<false>(x, O, g0, g1, l, cam, xn, P, wt, used, nullptr, acc); fresh = true; }
        double L[6], dp[3];
        bool ok = lm_chol3(acc, lm.lambda, 0.0, L);
        lm_solve3(L, acc + 6, dp);
        double q = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) { dp[a] = -dp[a]; q -= acc[6 + a] * dp[a]; ok = ok && (dp[a] - dp[a] == 0.0); }
        lm = lm_converged(lm, ok, q, floor_f, tol2);
        if (lm.stop) break;                               // before the trial's objective is paid for
        double xt[3] = {x[0] + dp[0], x[1] + dp[1], x[2] + dp[2]};
        Dd ft = {0.0, 0.0};
        double nbad = 0.0;
        if (ok) ft = ia_objective(xt, O, g0, g1, l, cam, xn, P, wt, used, nbad);
        const bool accept = lm_accept(lm, ok, nbad, ft);
        if (accept) {
#pragma unroll
            for (int k = 0; k < 3; ++k) x[k] = xt[k];
            fresh = false;
        }
        lm = lm_step(lm, accept, ft, max_iter);
        if (lm.stop) break;
    }

    // ---- the end: the residuals of every finite ray, the undamped matrix at the returned point, its inverse -------------
    ia_linearise<true>(x, O, g0, g1, l, cam, xn, P, wt, used, res, acc);
    double L[6], Qc[9];
    bool singular = !lm_chol3(acc, 0.0, LM_PIVOT, L);
    singular = sym_inverse<3>(L, Qc) || singular;         // (L is in sym_ix<3> storage)
    if (l == 0) {
        double *Qp = Q + 9 * (int64_t)p;
#pragma unroll
        for (int i = 0; i < 9; ++i) Qp[i] = singular ? nan : Qc[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) Xp[k] = O[k] + x[k];
        lm_store_stats(dstat, istat, p, f0, lm, singular, n, 2 * n - 3);
    }
}

#endif  // __HIPCC__

}  // namespace dbat
