// Least-squares relative orientation of image pairs (dbat_hip_pairadjust, host side: pairadjust_host.hpp): the two-view
// bundle adjustment in the gauge of camsfrome.m:16-33 -- camera 1 is [I | 0], camera 2 [R | t] with |t| = 1 -- for many
// pairs in one launch.  One workgroup of 256 lanes per pair; the whole damped loop runs inside the kernel, by the protocol
// of lm_core.hpp, whose constants and factorisations it uses.  Thread 0 writes the decisions and the statistics out on
// PaState: that keeps the kernel's instructions and so its bits (on LmState and the shared epilogue P2, f, Q moved an ulp).
//
// Unknowns of a pair: R, t on the unit sphere, and X_k for every used correspondence.  With pi(Y) = Y(1:2) / Y(3) the
// residuals are w1_k (pi(X_k) - x1_k) and w2_k (pi(R X_k + t) - x2_k).  A step is (a, b, d_k): R <- exp([a]x) R,
// t <- (t + B b) / |t + B b| with B = pa_basis(t) spanning the plane across t, X_k <- X_k + d_k: five pose unknowns and
// three per point.  The normal equations are damped with Marquardt's scaling (lambda diag V_k, lambda diag U) and the
// points are eliminated: S = U + lambda diag U - sum W_k (V_k + lambda diag V_k)^-1 W_k'.
//
// A trial is two passes over the pair's correspondences (lane l takes l, l + 256, ... in ascending order) and two
// reductions of the fixed shape of pa_reduce: the lane's serial sum, a shuffle tree over the 64 lanes of a wave, the four
// wave partials through LDS added in wave order.  No atomics of any kind: two calls give the same bits, and a pair gives
// the same bits alone and inside a batch.  Thread 0 solves the 5 x 5 system and takes every decision; the other lanes
// read the outcome from LDS, so every barrier sits in uniform control flow.
//
// Every loop is bounded: the trial loop by LM_MAX_REJECT * max_iter (max_iter is validated to 1 .. 200 by the host),
// the point loops by the pair's size.  No communication between workgroups, no spinning, nothing persistent.
#pragma once
#include "lm_core.hpp"

namespace dbat {

constexpr int PA_WG = 256;                  // lanes of a workgroup: four waves of 64
constexpr int PA_NSUM = 41;                 // sums of pass A: U (15), W V^-1 W' (15), g_p (5), W V^-1 g (5), bad blocks (1)
constexpr double PA_V_PIVOT = 1e-12;        // at the end: a pivot of V_k at or below this share of its diagonal entry: singular (of S: LM_PIVOT)
constexpr int PA_TOO_FEW = LM_TOO_FEW;      // (the name pairadjust_host.hpp reads the code by)

// B (3 x 2, column-major): b1 along t x e_i, i the first axis of smallest |t_i|, b2 = t x b1.
__host__ __device__ inline void pa_basis(const double *t, double *B) {
    int i = 0;
    if (fabs(t[1]) < fabs(t[i])) i = 1;
    if (fabs(t[2]) < fabs(t[i])) i = 2;
    const double b0 = i == 0 ? 0.0 : i == 1 ? -t[2] : t[1];          // t x e_i
    const double b1 = i == 0 ? t[2] : i == 1 ? 0.0 : -t[0];
    const double b2 = i == 0 ? -t[1] : i == 1 ? t[0] : 0.0;
    const double n = sqrt(b0 * b0 + b1 * b1 + b2 * b2);
    B[0] = b0 / n; B[1] = b1 / n; B[2] = b2 / n;
    B[3] = t[1] * B[2] - t[2] * B[1]; B[4] = t[2] * B[0] - t[0] * B[2]; B[5] = t[0] * B[1] - t[1] * B[0];
}

#if defined(__HIPCC__)

// Weighted residuals (image 1 x, y, image 2 x, y) of X under [R | t] against m = (x1, x2) -- r in float64 for the normal
// equations, rr as pairs for the objective (rounded to float64 they would leave 1e-16 of f as noise, enough to walk
// 1e-9 away from an optimum already reached) -- and the depth z2.  R has 18 entries: the matrix and, from [9], its
// low words.
__device__ __forceinline__ void pa_residuals(const double *R, const double *t, const double *X, const double *m, const double *w,
                                             double *r, Dd *rr, double &z2) {
    Dd Y[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        Y[k] = dd_fma(dd_fma(dd_fma(Dd{t[k], 0.0}, X[0], Dd{R[k], R[9 + k]}), X[1], Dd{R[3 + k], R[12 + k]}), X[2], Dd{R[6 + k], R[15 + k]});
    z2 = Y[2].hi;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const Dd a = dd_fma(Dd{X[k], 0.0}, -m[k], X[2]), b = dd_fma(Y[k], -m[2 + k], Y[2]);
        rr[k] = dd_fma(Dd{0.0, 0.0}, w[k], dd_div(a, Dd{X[2], 0.0}));
        rr[2 + k] = dd_fma(Dd{0.0, 0.0}, w[2 + k], dd_div(b, Y[2]));
        r[k] = rr[k].hi; r[2 + k] = rr[2 + k].hi;
    }
}

// sum of rr[0 .. 3]^2 added to f
__device__ __forceinline__ Dd pa_dd_sumsq(Dd f, const Dd *rr) {
#pragma unroll
    for (int k = 0; k < 4; ++k) f = dd_add(f, dd_mul(rr[k], rr[k]));
    return f;
}

// The workgroup's sum of a double-double per lane, in the fixed shape of pa_reduce: hi to part[4 wave], lo to [4 wave + 1].
__device__ __forceinline__ void pa_reduce_dd(Dd v, double *part) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = dd_add(v, Dd{__shfl_down(v.hi, off, 64), __shfl_down(v.lo, off, 64)});
    if ((threadIdx.x & 63) == 0) { part[4 * (threadIdx.x >> 6)] = v.hi; part[4 * (threadIdx.x >> 6) + 1] = v.lo; }
}
__device__ __forceinline__ Dd pa_total_dd(const double *part) {
    Dd v = {part[0], part[1]};
#pragma unroll
    for (int wv = 1; wv < 4; ++wv) v = dd_add(v, Dd{part[4 * wv], part[4 * wv + 1]});
    return v;
}

// The blocks of one correspondence at (R, t, B, X): weighted residuals r (image 1 x, y, image 2 x, y), the depths, and
// with JAC the normal-equation blocks V (00 01 02 11 12 22), W (5 x 3, row-major), g (3), A (2 x 5, row-major: the
// second image's Jacobian to the pose).
struct PaBlocks { double r[4], z1, z2, V[6], W[15], g[3], A[10]; Dd rr[4]; };

template <bool JAC>
__device__ __forceinline__ void pa_blocks(const double *R, const double *t, const double *B, const double *X, const double *m,
                                          const double *w, PaBlocks &o) {
    double Y[3], v[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        v[r] = R[r] * X[0] + R[3 + r] * X[1] + R[6 + r] * X[2];      // R X
        Y[r] = v[r] + t[r];
    }
    o.z1 = X[2];
    pa_residuals(R, t, X, m, w, o.r, o.rr, o.z2);
    if (!JAC) return;
    const double i1 = 1.0 / X[2], i2 = 1.0 / Y[2];
    // rows of diag(w) d pi / d Y: (1/z, 0, -Y0/z^2), (0, 1/z, -Y1/z^2)
    const double a0 = w[0] * i1, a2 = -w[0] * X[0] * i1 * i1, b1 = w[1] * i1, b2 = -w[1] * X[1] * i1 * i1;       // image 1: J1
    const double P[6] = {w[2] * i2, 0.0, -w[2] * Y[0] * i2 * i2, 0.0, w[3] * i2, -w[3] * Y[1] * i2 * i2};        // image 2
    double J2[6];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int k = 0; k < 3; ++k) J2[3 * i + k] = P[3 * i] * R[3 * k] + P[3 * i + 1] * R[3 * k + 1] + P[3 * i + 2] * R[3 * k + 2];
        double *A = o.A + 5 * i;
        const double *p = P + 3 * i;
        A[0] = p[2] * v[1] - p[1] * v[2];                 // d (a x R X) / d a_j = e_j x R X
        A[1] = p[0] * v[2] - p[2] * v[0];
        A[2] = p[1] * v[0] - p[0] * v[1];
        A[3] = p[0] * B[0] + p[1] * B[1] + p[2] * B[2];
        A[4] = p[0] * B[3] + p[1] * B[4] + p[2] * B[5];
    }
    o.V[0] = a0 * a0 + J2[0] * J2[0] + J2[3] * J2[3];
    o.V[1] = J2[0] * J2[1] + J2[3] * J2[4];
    o.V[2] = a0 * a2 + J2[0] * J2[2] + J2[3] * J2[5];
    o.V[3] = b1 * b1 + J2[1] * J2[1] + J2[4] * J2[4];
    o.V[4] = b1 * b2 + J2[1] * J2[2] + J2[4] * J2[5];
    o.V[5] = a2 * a2 + b2 * b2 + J2[2] * J2[2] + J2[5] * J2[5];
    o.g[0] = a0 * o.r[0] + J2[0] * o.r[2] + J2[3] * o.r[3];
    o.g[1] = b1 * o.r[1] + J2[1] * o.r[2] + J2[4] * o.r[3];
    o.g[2] = a2 * o.r[0] + b2 * o.r[1] + J2[2] * o.r[2] + J2[5] * o.r[3];
#pragma unroll
    for (int a = 0; a < 5; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) o.W[3 * a + k] = o.A[a] * J2[k] + o.A[5 + a] * J2[3 + k];
}

// Sum of N values per lane over the workgroup, in a fixed shape: a shuffle tree over the 64 lanes of each wave, then the
// wave partials to part[wave * N + i].  The caller's barrier follows; pa_total adds the four partials in wave order.
template <int N>
__device__ __forceinline__ void pa_reduce(double *v, double *part) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double s = v[i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        v[i] = s;
    }
    if ((threadIdx.x & 63) == 0) {
        double *p = part + (threadIdx.x >> 6) * N;
#pragma unroll
        for (int i = 0; i < N; ++i) p[i] = v[i];
    }
}
template <int N>
__device__ __forceinline__ double pa_total(const double *part, int i) { return ((part[i] + part[N + i]) + part[2 * N + i]) + part[3 * N + i]; }

// Two more sums of the workgroup beside a double-double: to part[4 wave + 2] and [4 wave + 3].
__device__ __forceinline__ void pa_reduce_tail(double a, double b, double *part) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_down(a, off, 64); b += __shfl_down(b, off, 64); }
    if ((threadIdx.x & 63) == 0) { part[4 * (threadIdx.x >> 6) + 2] = a; part[4 * (threadIdx.x >> 6) + 3] = b; }
}

struct PaState {
    double part[4 * PA_NSUM];       // wave partials of pass A
    double part2[4 * 4];            // and of pass B, per wave: trial objective (hi, lo), sum g_k' d_k, points not in front or without a step
    double R[18], t[3], B[6];       // the current pose; R as a sum of two doubles, the low words at [9 ..]
    double Rn[18], tn[3], dp[5];    // the trial pose and the pose step
    double G[18], T[18];            // thread 0's work arrays of dd_orthonormalise
    double S[15], gp[5], Si[25], Bf[30], e[5];     // thread 0's work arrays: indexed in loops, so not in registers
    double lambda, f, flo, f0, gpdp;          // f + flo: the objective in double-double
    int n, iters, trials, code, done, solved, accepted;
};

// Workgroup p adjusts pair p: correspondences pt_start[p] .. pt_start[p + 1] of x1, x2, w1, w2 (2 doubles each; w1, w2
// may be null: ones), use (may be null: all).  P2 [12 p] in/out, X [3 g] in/out with Xt [3 g] the trial points, used [g]
// out, dstat [4 p], istat [4 p], Q [36 p] out, res [4 g] out or null (zeroed by the host: only used rows are written).
__global__ __launch_bounds__(PA_WG) void k_pairadjust(const int64_t *__restrict__ pt_start, const double *__restrict__ x1,
                                                      const double *__restrict__ x2, const uint8_t *__restrict__ use,
                                                      const double *__restrict__ w1, const double *__restrict__ w2, int front,
                                                      int max_iter, double tol2, double sin2_min, double *__restrict__ P2,
                                                      double *__restrict__ X, double *__restrict__ Xt, uint8_t *__restrict__ used,
                                                      double *__restrict__ dstat, int32_t *__restrict__ istat,
                                                      double *__restrict__ Q, double *__restrict__ res) {
    __shared__ PaState s;
    const int p = blockIdx.x, tid = threadIdx.x;
    const int64_t g0 = pt_start[p], g1 = pt_start[p + 1];
    const double fr = (double)front;
    if (tid < 12) (tid < 9 ? s.R[tid] : s.t[tid - 9]) = P2[12 * (int64_t)p + tid];
    if (tid < 9) s.R[9 + tid] = 0.0;
    __syncthreads();
    if (tid == 0) dd_orthonormalise(s.R, s.G, s.T);
    __syncthreads();
    double R[18], t[3], B[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 18; ++i) R[i] = s.R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = s.t[i];

    // ---- selection, once, at the start orientation; the objective there --------------------------------------------
    Dd fsum = {0.0, 0.0};
    double cnt = 0.0;
    for (int64_t g = g0 + tid; g < g1; g += PA_WG) {
        const double m[4] = {x1[2 * g], x1[2 * g + 1], x2[2 * g], x2[2 * g + 1]};
        const double Xg[3] = {X[3 * g], X[3 * g + 1], X[3 * g + 2]};
        const double w[4] = {w1 ? w1[2 * g] : 1.0, w1 ? w1[2 * g + 1] : 1.0, w2 ? w2[2 * g] : 1.0, w2 ? w2[2 * g + 1] : 1.0};
        PaBlocks b;
        pa_blocks<false>(R, t, B, Xg, m, w, b);
        // the rays (x1, 1) and R' (x2, 1): |d1 x d2|^2 >= sin^2(min_angle) |d1|^2 |d2|^2
        const double d1[3] = {m[0], m[1], 1.0};
        const double d2[3] = {R[0] * m[2] + R[1] * m[3] + R[2], R[3] * m[2] + R[4] * m[3] + R[5], R[6] * m[2] + R[7] * m[3] + R[8]};
        const double c[3] = {d1[1] * d2[2] - d1[2] * d2[1], d1[2] * d2[0] - d1[0] * d2[2], d1[0] * d2[1] - d1[1] * d2[0]};
        const double lhs = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
        const double rhs = sin2_min * (d1[0] * d1[0] + d1[1] * d1[1] + 1.0) * (d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2]);
        const bool u = (!use || use[g]) && fr * b.z1 > 0 && fr * b.z2 > 0 && lhs >= rhs;
        used[g] = u ? 1 : 0;
        if (u) { cnt += 1.0; fsum = pa_dd_sumsq(fsum, b.rr); }
    }
    pa_reduce_dd(fsum, s.part2);
    pa_reduce_tail(cnt, 0.0, s.part2);
    __syncthreads();
    if (tid == 0) {
        const Dd f0 = pa_total_dd(s.part2);
        s.n = (int)pa_total<4>(s.part2, 2);
        s.f = s.f0 = f0.hi; s.flo = f0.lo;
        s.lambda = LM_LAMBDA0; s.iters = s.trials = 0; s.done = 0; s.code = LM_MAX_ITER;
        pa_basis(s.t, s.B);
        if (s.n < 5) {
            s.code = LM_TOO_FEW;
            const double nan = __builtin_nan("");
            dstat[4 * (int64_t)p] = nan; dstat[4 * (int64_t)p + 1] = nan; dstat[4 * (int64_t)p + 2] = nan; dstat[4 * (int64_t)p + 3] = LM_LAMBDA0;
            istat[4 * (int64_t)p] = LM_TOO_FEW; istat[4 * (int64_t)p + 1] = 0; istat[4 * (int64_t)p + 2] = 0; istat[4 * (int64_t)p + 3] = s.n;
            for (int i = 0; i < 36; ++i) Q[36 * (int64_t)p + i] = nan;
        }
    }
    __syncthreads();
    if (s.code == LM_TOO_FEW) return;                     // uniform: read from LDS
    const int n = s.n;
    const double floor_f = LM_FLOOR * 4.0 * (double)n;

    // ---- the damped loop ------------------------------------------------------------------------------------------------
    const int max_trials = LM_MAX_REJECT * max_iter;
    for (int trial = 0; trial < max_trials; ++trial) {
#pragma unroll
        for (int i = 0; i < 18; ++i) R[i] = s.R[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) t[i] = s.t[i];
#pragma unroll
        for (int i = 0; i < 6; ++i) B[i] = s.B[i];
        const double lambda = s.lambda;
        // pass A: the normal-equation sums of the lane's points
        double acc[PA_NSUM];
#pragma unroll
        for (int i = 0; i < PA_NSUM; ++i) acc[i] = 0.0;
        for (int64_t g = g0 + tid; g < g1; g += PA_WG) {
            if (!used[g]) continue;
            const double m[4] = {x1[2 * g], x1[2 * g + 1], x2[2 * g], x2[2 * g + 1]};
            const double Xg[3] = {X[3 * g], X[3 * g + 1], X[3 * g + 2]};
            const double w[4] = {w1 ? w1[2 * g] : 1.0, w1 ? w1[2 * g + 1] : 1.0, w2 ? w2[2 * g] : 1.0, w2 ? w2[2 * g + 1] : 1.0};
            PaBlocks b;
            pa_blocks<true>(R, t, B, Xg, m, w, b);
#pragma unroll
            for (int a = 0; a < 5; ++a) {
#pragma unroll
                for (int c = a; c < 5; ++c) acc[sym_ix<5>(a, c)] += b.A[a] * b.A[c] + b.A[5 + a] * b.A[5 + c];
                acc[30 + a] += b.A[a] * b.r[2] + b.A[5 + a] * b.r[3];
            }
            double L[6];
            if (!lm_chol3(b.V, lambda, 0.0, L)) { acc[40] += 1.0; continue; }
            double Z[15];                                 // row a: V^-1 W(a, :)'
#pragma unroll
            for (int a = 0; a < 5; ++a) lm_solve3(L, b.W + 3 * a, Z + 3 * a);
#pragma unroll
            for (int a = 0; a < 5; ++a) {
#pragma unroll
                for (int c = a; c < 5; ++c) acc[15 + sym_ix<5>(a, c)] += b.W[3 * a] * Z[3 * c] + b.W[3 * a + 1] * Z[3 * c + 1] + b.W[3 * a + 2] * Z[3 * c + 2];
                acc[35 + a] += Z[3 * a] * b.g[0] + Z[3 * a + 1] * b.g[1] + Z[3 * a + 2] * b.g[2];
            }
        }
        pa_reduce<PA_NSUM>(acc, s.part);
        __syncthreads();
        if (tid == 0) {
            double *S = s.S, *dp = s.dp, *gp = s.gp;
            for (int i = 0; i < 15; ++i) S[i] = pa_total<PA_NSUM>(s.part, i) - pa_total<PA_NSUM>(s.part, 15 + i);
            for (int a = 0; a < 5; ++a) {
                S[sym_ix<5>(a, a)] = pa_total<PA_NSUM>(s.part, sym_ix<5>(a, a)) + lambda * pa_total<PA_NSUM>(s.part, sym_ix<5>(a, a)) - pa_total<PA_NSUM>(s.part, 15 + sym_ix<5>(a, a));
                gp[a] = pa_total<PA_NSUM>(s.part, 30 + a);
                dp[a] = gp[a] - pa_total<PA_NSUM>(s.part, 35 + a);
            }
            bool ok = pa_total<PA_NSUM>(s.part, 40) == 0.0;
            ok = sym_chol<5>(S, 0.0) && ok;
            sym_solve<5>(S, dp);
            double gd = 0.0;
            for (int a = 0; a < 5; ++a) { dp[a] = -dp[a]; gd += gp[a] * dp[a]; ok = ok && (dp[a] - dp[a] == 0.0); }
            if (!ok) for (int a = 0; a < 5; ++a) dp[a] = 0.0;
            const double t0 = s.t[0] + s.B[0] * dp[3] + s.B[3] * dp[4], t1 = s.t[1] + s.B[1] * dp[3] + s.B[4] * dp[4];
            const double t2 = s.t[2] + s.B[2] * dp[3] + s.B[5] * dp[4], nn = sqrt(t0 * t0 + t1 * t1 + t2 * t2);
            s.tn[0] = t0 / nn; s.tn[1] = t1 / nn; s.tn[2] = t2 / nn;
            dd_rotate_dd(dp, s.R, s.Rn, s.G, s.T);
            s.gpdp = gd; s.solved = ok ? 1 : 0;
        }
        __syncthreads();
        // pass B: the point steps, the trial points, the trial objective and the points' share of q = -g' delta
        double Rn[18], tn[3], dp[5];
#pragma unroll
        for (int i = 0; i < 18; ++i) Rn[i] = s.Rn[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) tn[i] = s.tn[i];
#pragma unroll
        for (int i = 0; i < 5; ++i) dp[i] = s.dp[i];
        Dd ft = {0.0, 0.0};
        double qp = 0.0, nbad = 0.0;
        if (s.solved) {                                   // uniform: read from LDS
            for (int64_t g = g0 + tid; g < g1; g += PA_WG) {
                if (!used[g]) continue;
                const double m[4] = {x1[2 * g], x1[2 * g + 1], x2[2 * g], x2[2 * g + 1]};
                const double Xg[3] = {X[3 * g], X[3 * g + 1], X[3 * g + 2]};
                const double w[4] = {w1 ? w1[2 * g] : 1.0, w1 ? w1[2 * g + 1] : 1.0, w2 ? w2[2 * g] : 1.0, w2 ? w2[2 * g + 1] : 1.0};
                PaBlocks b;
                pa_blocks<true>(R, t, B, Xg, m, w, b);
                double L[6], rhs[3], d[3];
                const bool okv = lm_chol3(b.V, lambda, 0.0, L);
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    rhs[k] = b.g[k] + (b.W[k] * dp[0] + b.W[3 + k] * dp[1] + b.W[6 + k] * dp[2] + b.W[9 + k] * dp[3] + b.W[12 + k] * dp[4]);
                lm_solve3(L, rhs, d);
                double Xn[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) { d[k] = okv ? -d[k] : 0.0; Xn[k] = Xg[k] + d[k]; Xt[3 * g + k] = Xn[k]; }
                PaBlocks bn;
                pa_blocks<false>(Rn, tn, B, Xn, m, w, bn);
                ft = pa_dd_sumsq(ft, bn.rr);
                qp += b.g[0] * d[0] + b.g[1] * d[1] + b.g[2] * d[2];
                if (!(okv && fr * bn.z1 > 0 && fr * bn.z2 > 0)) nbad += 1.0;
            }
        }
        pa_reduce_dd(ft, s.part2);
        pa_reduce_tail(qp, nbad, s.part2);
        __syncthreads();
        if (tid == 0) {
            const Dd ft = pa_total_dd(s.part2);
            const double q = -(s.gpdp + pa_total<4>(s.part2, 2)), bad = pa_total<4>(s.part2, 3);
            const bool ok = s.solved != 0;
            s.trials += 1; s.accepted = 0;
            if (s.f <= floor_f || (ok && q <= tol2 * s.f)) { s.code = LM_CONVERGED; s.done = 1; }
            else if (ok && bad == 0.0 && (ft.hi - ft.hi == 0.0) && dd_less(ft, Dd{s.f, s.flo})) {
                for (int i = 0; i < 18; ++i) s.R[i] = s.Rn[i];
                for (int i = 0; i < 3; ++i) s.t[i] = s.tn[i];
                pa_basis(s.t, s.B);
                s.f = ft.hi; s.flo = ft.lo; s.lambda = fmax(s.lambda / 10.0, LM_LAMBDA_MIN); s.iters += 1; s.accepted = 1;
                if (s.iters >= max_iter) { s.code = LM_MAX_ITER; s.done = 1; }
            } else {
                s.lambda = s.lambda * 10.0;
                if (s.lambda > LM_LAMBDA_MAX) { s.code = LM_NO_STEP; s.done = 1; }
            }
        }
        __syncthreads();
        if (s.accepted)                                   // uniform; every lane moves its own points
            for (int64_t g = g0 + tid; g < g1; g += PA_WG)
                if (used[g]) { X[3 * g] = Xt[3 * g]; X[3 * g + 1] = Xt[3 * g + 1]; X[3 * g + 2] = Xt[3 * g + 2]; }
        if (s.done) break;                                // uniform
    }

    // ---- the end: the undamped reduced matrix at the last accepted values, its cofactor matrix, the residuals ----------
#pragma unroll
    for (int i = 0; i < 18; ++i) R[i] = s.R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = s.t[i];
#pragma unroll
    for (int i = 0; i < 6; ++i) B[i] = s.B[i];
    double acc[PA_NSUM];
#pragma unroll
    for (int i = 0; i < PA_NSUM; ++i) acc[i] = 0.0;
    for (int64_t g = g0 + tid; g < g1; g += PA_WG) {
        if (!used[g]) continue;
        const double m[4] = {x1[2 * g], x1[2 * g + 1], x2[2 * g], x2[2 * g + 1]};
        const double Xg[3] = {X[3 * g], X[3 * g + 1], X[3 * g + 2]};
        const double w[4] = {w1 ? w1[2 * g] : 1.0, w1 ? w1[2 * g + 1] : 1.0, w2 ? w2[2 * g] : 1.0, w2 ? w2[2 * g + 1] : 1.0};
        PaBlocks b;
        pa_blocks<true>(R, t, B, Xg, m, w, b);
        if (res) { res[4 * g] = b.r[0]; res[4 * g + 1] = b.r[1]; res[4 * g + 2] = b.r[2]; res[4 * g + 3] = b.r[3]; }
#pragma unroll
        for (int a = 0; a < 5; ++a)
#pragma unroll
            for (int c = a; c < 5; ++c) acc[sym_ix<5>(a, c)] += b.A[a] * b.A[c] + b.A[5 + a] * b.A[5 + c];
        double L[6];
        if (!lm_chol3(b.V, 0.0, PA_V_PIVOT, L)) { acc[40] += 1.0; continue; }
        double Z[15];
#pragma unroll
        for (int a = 0; a < 5; ++a) lm_solve3(L, b.W + 3 * a, Z + 3 * a);
#pragma unroll
        for (int a = 0; a < 5; ++a)
#pragma unroll
            for (int c = a; c < 5; ++c) acc[15 + sym_ix<5>(a, c)] += b.W[3 * a] * Z[3 * c] + b.W[3 * a + 1] * Z[3 * c + 1] + b.W[3 * a + 2] * Z[3 * c + 2];
    }
    pa_reduce<PA_NSUM>(acc, s.part);
    __syncthreads();
    if (tid == 0) {
        double *S = s.S, *Si = s.Si, *Bf = s.Bf, *e = s.e;
        for (int i = 0; i < 15; ++i) S[i] = pa_total<PA_NSUM>(s.part, i) - pa_total<PA_NSUM>(s.part, 15 + i);
        bool singular = pa_total<PA_NSUM>(s.part, 40) != 0.0;
        singular = !sym_chol<5>(S, LM_PIVOT) || singular;
        for (int c = 0; c < 5; ++c) {
            for (int r = 0; r < 5; ++r) e[r] = r == c ? 1.0 : 0.0;
            sym_solve<5>(S, e);
            for (int r = 0; r < 5; ++r) { Si[5 * c + r] = e[r]; singular = singular || !(e[r] - e[r] == 0.0); }
        }
        // Bf = blkdiag(I3, B), 6 x 5 column-major
        for (int i = 0; i < 30; ++i) Bf[i] = 0.0;
        Bf[0] = Bf[7] = Bf[14] = 1.0;
        for (int c = 0; c < 2; ++c) for (int r = 0; r < 3; ++r) Bf[6 * (3 + c) + 3 + r] = s.B[3 * c + r];
        double *Qp = Q + 36 * (int64_t)p;
        for (int c = 0; c < 6; ++c)
            for (int r = 0; r < 6; ++r) {
                double v = 0.0;
                for (int a = 0; a < 5; ++a)
                    for (int b2 = 0; b2 < 5; ++b2) v += Bf[6 * a + r] * Si[5 * b2 + a] * Bf[6 * b2 + c];
                Qp[6 * c + r] = singular ? __builtin_nan("") : v;
            }
        int code = s.code;
        if (code == LM_CONVERGED && singular) code = LM_SINGULAR;
        for (int i = 0; i < 9; ++i) P2[12 * (int64_t)p + i] = s.R[i];
        for (int i = 0; i < 3; ++i) P2[12 * (int64_t)p + 9 + i] = s.t[i];
        dstat[4 * (int64_t)p] = s.f0; dstat[4 * (int64_t)p + 1] = s.f;
        dstat[4 * (int64_t)p + 2] = n > 5 ? sqrt(s.f / (double)(n - 5)) : __builtin_nan("");
        dstat[4 * (int64_t)p + 3] = s.lambda;
        istat[4 * (int64_t)p] = code; istat[4 * (int64_t)p + 1] = s.iters; istat[4 * (int64_t)p + 2] = s.trials; istat[4 * (int64_t)p + 3] = n;
    }
}

#endif  // __HIPCC__

}  // namespace dbat
