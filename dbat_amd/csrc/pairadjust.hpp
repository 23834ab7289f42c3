// Least-squares relative orientation of image pairs (dbat_hip_pairadjust, host side: pairadjust_host.hpp): the two-view
// bundle adjustment in the gauge of camsfrome.m:16-33 -- camera 1 is [I | 0], camera 2 [R | t] with |t| = 1 -- for many
// pairs in one launch.  One workgroup of 256 lanes per pair; the whole damped loop runs inside the kernel.
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
// Every loop is bounded: the trial loop by PA_MAX_REJECT * max_iter (max_iter is validated to 1 .. 200 by the host),
// the point loops by the pair's size.  No communication between workgroups, no spinning, nothing persistent.
#pragma once

namespace dbat {

constexpr int PA_WG = 256;                  // lanes of a workgroup: four waves of 64
constexpr int PA_NSUM = 41;                 // sums of pass A: U (15), W V^-1 W' (15), g_p (5), W V^-1 g (5), bad blocks (1)
constexpr double PA_LAMBDA0 = 1e-3, PA_LAMBDA_MIN = 1e-12, PA_LAMBDA_MAX = 1e8;
constexpr double PA_FLOOR = 1e-24;          // f <= PA_FLOOR * 4 n: converged (a noise-free pair never meets q <= tol^2 f)
constexpr double PA_V_PIVOT = 1e-12;        // at the end: a pivot of V_k at or below this share of its diagonal entry: singular
constexpr double PA_S_PIVOT = 1e-10;        // and of the undamped S
// Consecutive rejections at most: lambda is at least PA_LAMBDA_MIN, a rejection multiplies it by ten, and the call ends
// once it exceeds PA_LAMBDA_MAX: 1e-12 * 10^21 = 1e9.  An iteration is therefore at most 20 rejected trials and the
// accepted one, or 21 rejected ones and the end: PA_MAX_REJECT * max_iter trials bound the whole loop.
constexpr int PA_MAX_REJECT = 21;
enum { PA_CONVERGED = 0, PA_MAX_ITER = 1, PA_NO_STEP = 2, PA_SINGULAR = 3, PA_TOO_FEW = 4 };

__host__ __device__ constexpr int pa_s5(int i, int j) { return i <= j ? i * 5 - i * (i - 1) / 2 + (j - i) : j * 5 - j * (j - 1) / 2 + (i - j); }

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

// Rn = exp([a]x) R (column-major 3 x 3) by Rodrigues' formula, (1 - cos th) / th^2 as 2 sin^2(th / 2) / th^2.
__host__ __device__ inline void pa_rotate(const double *a, const double *R, double *Rn) {
    const double th2 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
    double A = 1.0, C = 0.5;
    if (!(th2 < 1e-16)) {
        const double th = sqrt(th2), s = sin(0.5 * th);
        A = sin(th) / th; C = 2.0 * s * s / th2;
    }
    // E = I + A K + C K K with K = [a]x and K K = a a' - th^2 I
    const double dg = 1.0 - C * th2;
    const double e00 = dg + C * a[0] * a[0], e01 = C * a[0] * a[1] - A * a[2], e02 = C * a[0] * a[2] + A * a[1];
    const double e10 = C * a[1] * a[0] + A * a[2], e11 = dg + C * a[1] * a[1], e12 = C * a[1] * a[2] - A * a[0];
    const double e20 = C * a[2] * a[0] - A * a[1], e21 = C * a[2] * a[1] + A * a[0], e22 = dg + C * a[2] * a[2];
    for (int c = 0; c < 3; ++c) {
        const double r0 = R[3 * c], r1 = R[3 * c + 1], r2 = R[3 * c + 2];
        Rn[3 * c] = e00 * r0 + e01 * r1 + e02 * r2;
        Rn[3 * c + 1] = e10 * r0 + e11 * r1 + e12 * r2;
        Rn[3 * c + 2] = e20 * r0 + e21 * r1 + e22 * r2;
    }
}

// Cholesky of the 5 x 5 matrix S (pa_s5 storage) in place: false where a pivot is not above tol times its diagonal entry.
__host__ __device__ inline bool pa_chol5(double *S, double tol) {
    bool ok = true;
    for (int j = 0; j < 5; ++j) {
        const double sjj = S[pa_s5(j, j)];
        double d = sjj;
        for (int k = 0; k < j; ++k) d -= S[pa_s5(k, j)] * S[pa_s5(k, j)];
        if (!(d > tol * sjj)) { ok = false; d = 1.0; }
        const double l = sqrt(d);
        S[pa_s5(j, j)] = l;
        for (int i = j + 1; i < 5; ++i) {
            double v = S[pa_s5(j, i)];
            for (int k = 0; k < j; ++k) v -= S[pa_s5(k, i)] * S[pa_s5(k, j)];
            S[pa_s5(j, i)] = v / l;
        }
    }
    return ok;
}

// x <- (L L')^-1 x with the factor of pa_chol5 (L(i, j) at pa_s5(j, i), j <= i).
__host__ __device__ inline void pa_solve5(const double *L, double *x) {
    for (int i = 0; i < 5; ++i) {
        double v = x[i];
        for (int k = 0; k < i; ++k) v -= L[pa_s5(k, i)] * x[k];
        x[i] = v / L[pa_s5(i, i)];
    }
    for (int i = 4; i >= 0; --i) {
        double v = x[i];
        for (int k = i + 1; k < 5; ++k) v -= L[pa_s5(i, k)] * x[k];
        x[i] = v / L[pa_s5(i, i)];
    }
}

#if defined(__HIPCC__)

// ---- the objective in double-double ----------------------------------------------------------------------------------
// A trial is accepted only if its objective is smaller, and near the optimum the decrease of a step falls below the
// rounding of a float64 evaluation (a residual is a weight of 1e3 .. 1e4 times the difference of two coordinates of
// order one: 1e-13 of it is noise, and as much of f): the accept test then answers at random and the iteration stops
// sqrt(noise / curvature) short of the optimum, 1e-9 in a weak direction.  So the residuals are formed from
// R X + t - x (R X + t)_3 carried as unevaluated sums of two doubles (error-free products by fma, sums by Knuth's
// two-sum) and f is summed the same way; only the accept test reads the low word.  R itself is such a sum, kept
// orthonormal to 1e-31 (pa_orthonormalise).  The Jacobians and the normal equations are plain float64.
struct PaDD { double hi, lo; };
// (contraction is off in these: fusing a product into the sum that follows it, the compiler's default here, breaks the
// error-free transformations -- two-sum must see the rounded product that two-prod took the error of)
__device__ __forceinline__ PaDD pa_two_sum(double a, double b) {
#pragma clang fp contract(off)
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
__device__ __forceinline__ PaDD pa_two_prod(double a, double b) {
#pragma clang fp contract(off)
    const double p = a * b;
    return {p, __builtin_fma(a, b, -p)};
}
__device__ __forceinline__ PaDD pa_dd_add(PaDD x, PaDD y) {
#pragma clang fp contract(off)
    PaDD s = pa_two_sum(x.hi, y.hi);
    s.lo += x.lo + y.lo;
    const double h = s.hi + s.lo;
    return {h, s.lo - (h - s.hi)};
}
__device__ __forceinline__ PaDD pa_dd_fma(PaDD x, double a, double b) { return pa_dd_add(x, pa_two_prod(a, b)); }        // x + a b
__device__ __forceinline__ PaDD pa_dd_fma(PaDD x, double a, PaDD b) {                                                   // x + a b
#pragma clang fp contract(off)
    PaDD p = pa_two_prod(a, b.hi);
    p.lo = __builtin_fma(a, b.lo, p.lo);
    return pa_dd_add(x, p);
}
__device__ __forceinline__ bool pa_dd_less(PaDD a, PaDD b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }

__device__ __forceinline__ PaDD pa_dd_mul(PaDD a, PaDD b) {
#pragma clang fp contract(off)
    PaDD p = pa_two_prod(a.hi, b.hi);
    const double c = a.hi * b.lo, d = a.lo * b.hi;
    p.lo += c + d;
    const double h = p.hi + p.lo;
    return {h, p.lo - (h - p.hi)};
}

__device__ __forceinline__ PaDD pa_dd_div(PaDD a, PaDD b) {
#pragma clang fp contract(off)
    const double q1 = a.hi / b.hi;
    const PaDD r = pa_dd_fma(a, -q1, b);
    return pa_two_sum(q1, r.hi / b.hi);
}

// Weighted residuals (image 1 x, y, image 2 x, y) of X under [R | t] against m = (x1, x2) -- r in float64 for the normal
// equations, rr as pairs for the objective (rounded to float64 they would leave 1e-16 of f as noise, enough to walk
// 1e-9 away from an optimum already reached) -- and the depth z2.  R has 18 entries: the matrix and, from [9], its
// low words.
__device__ __forceinline__ void pa_residuals(const double *R, const double *t, const double *X, const double *m, const double *w,
                                             double *r, PaDD *rr, double &z2) {
    PaDD Y[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        Y[k] = pa_dd_fma(pa_dd_fma(pa_dd_fma(PaDD{t[k], 0.0}, X[0], PaDD{R[k], R[9 + k]}), X[1], PaDD{R[3 + k], R[12 + k]}), X[2], PaDD{R[6 + k], R[15 + k]});
    z2 = Y[2].hi;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const PaDD a = pa_dd_fma(PaDD{X[k], 0.0}, -m[k], X[2]), b = pa_dd_fma(Y[k], -m[2 + k], Y[2]);
        rr[k] = pa_dd_fma(PaDD{0.0, 0.0}, w[k], pa_dd_div(a, PaDD{X[2], 0.0}));
        rr[2 + k] = pa_dd_fma(PaDD{0.0, 0.0}, w[2 + k], pa_dd_div(b, Y[2]));
        r[k] = rr[k].hi; r[2 + k] = rr[2 + k].hi;
    }
}

// R <- R (3 I - R'R) / 2 on the double-double R (18 entries), one Newton step towards the nearest rotation: a product
// of float64 rotations is orthonormal to 1e-16, after the step to 1e-31.  Why: the six directions in which a 3 x 3 matrix
// leaves the rotations are directions in which f does not have a zero gradient at the optimum, so their rounding --
// drawn anew by every trial -- moves f by 1e-12 and more, and the accept test would again answer at random.  G, T:
// work arrays of 18.  For one thread.
__device__ inline void pa_orthonormalise(double *R, double *G, double *T) {
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            PaDD g = {0.0, 0.0};
            for (int r = 0; r < 3; ++r) g = pa_dd_add(g, pa_dd_mul(PaDD{R[3 * a + r], R[9 + 3 * a + r]}, PaDD{R[3 * b + r], R[9 + 3 * b + r]}));
            g = pa_dd_add(PaDD{a == b ? 3.0 : 0.0, 0.0}, PaDD{-g.hi, -g.lo});
            G[3 * b + a] = 0.5 * g.hi; G[9 + 3 * b + a] = 0.5 * g.lo;
        }
    for (int b = 0; b < 3; ++b)
        for (int r = 0; r < 3; ++r) {
            PaDD v = {0.0, 0.0};
            for (int a = 0; a < 3; ++a) v = pa_dd_add(v, pa_dd_mul(PaDD{R[3 * a + r], R[9 + 3 * a + r]}, PaDD{G[3 * b + a], G[9 + 3 * b + a]}));
            T[3 * b + r] = v.hi; T[9 + 3 * b + r] = v.lo;
        }
    for (int i = 0; i < 18; ++i) R[i] = T[i];
}

// Rn = exp([a]x) R on the double-double R, orthonormalised.  For one thread.
__device__ inline void pa_rotate_dd(const double *a, const double *R, double *Rn, double *G, double *T) {
    double E[9];
    const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    pa_rotate(a, I3, E);                                  // column-major exp([a]x)
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) {
            PaDD v = {0.0, 0.0};
#pragma unroll
            for (int k = 0; k < 3; ++k) v = pa_dd_fma(v, E[3 * k + r], PaDD{R[3 * c + k], R[9 + 3 * c + k]});
            T[3 * c + r] = v.hi; T[9 + 3 * c + r] = v.lo;
        }
    for (int i = 0; i < 18; ++i) Rn[i] = T[i];
    pa_orthonormalise(Rn, G, T);
}

// sum of rr[0 .. 3]^2 added to f
__device__ __forceinline__ PaDD pa_dd_sumsq(PaDD f, const PaDD *rr) {
#pragma unroll
    for (int k = 0; k < 4; ++k) f = pa_dd_add(f, pa_dd_mul(rr[k], rr[k]));
    return f;
}

// The workgroup's sum of a double-double per lane, in the fixed shape of pa_reduce: hi to part[4 wave], lo to [4 wave + 1].
__device__ __forceinline__ void pa_reduce_dd(PaDD v, double *part) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = pa_dd_add(v, PaDD{__shfl_down(v.hi, off, 64), __shfl_down(v.lo, off, 64)});
    if ((threadIdx.x & 63) == 0) { part[4 * (threadIdx.x >> 6)] = v.hi; part[4 * (threadIdx.x >> 6) + 1] = v.lo; }
}
__device__ __forceinline__ PaDD pa_total_dd(const double *part) {
    PaDD v = {part[0], part[1]};
#pragma unroll
    for (int wv = 1; wv < 4; ++wv) v = pa_dd_add(v, PaDD{part[4 * wv], part[4 * wv + 1]});
    return v;
}

// The blocks of one correspondence at (R, t, B, X): weighted residuals r (image 1 x, y, image 2 x, y), the depths, and
// with JAC the normal-equation blocks V (00 01 02 11 12 22), W (5 x 3, row-major), g (3), A (2 x 5, row-major: the
// second image's Jacobian to the pose).
struct PaBlocks { double r[4], z1, z2, V[6], W[15], g[3], A[10]; PaDD rr[4]; };

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

// Cholesky of V + lambda diag V (3 x 3) into L (00 10 20 11 21 22): false where a pivot is not above tol times the
// diagonal entry of V.
__device__ __forceinline__ bool pa_chol3(const double *V, double lambda, double tol, double *L) {
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

__device__ __forceinline__ void pa_solve3(const double *L, const double *b, double *x) {
    const double y0 = b[0] / L[0];
    const double y1 = (b[1] - L[1] * y0) / L[3];
    const double y2 = (b[2] - L[2] * y0 - L[4] * y1) / L[5];
    x[2] = y2 / L[5];
    x[1] = (y1 - L[4] * x[2]) / L[3];
    x[0] = (y0 - L[1] * x[1] - L[2] * x[2]) / L[0];
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
    double G[18], T[18];            // thread 0's work arrays of pa_orthonormalise
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
    if (tid == 0) pa_orthonormalise(s.R, s.G, s.T);
    __syncthreads();
    double R[18], t[3], B[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 18; ++i) R[i] = s.R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = s.t[i];

    // ---- selection, once, at the start orientation; the objective there --------------------------------------------
    PaDD fsum = {0.0, 0.0};
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
        const PaDD f0 = pa_total_dd(s.part2);
        s.n = (int)pa_total<4>(s.part2, 2);
        s.f = s.f0 = f0.hi; s.flo = f0.lo;
        s.lambda = PA_LAMBDA0; s.iters = s.trials = 0; s.done = 0; s.code = PA_MAX_ITER;
        pa_basis(s.t, s.B);
        if (s.n < 5) {
            s.code = PA_TOO_FEW;
            const double nan = __builtin_nan("");
            dstat[4 * (int64_t)p] = nan; dstat[4 * (int64_t)p + 1] = nan; dstat[4 * (int64_t)p + 2] = nan; dstat[4 * (int64_t)p + 3] = PA_LAMBDA0;
            istat[4 * (int64_t)p] = PA_TOO_FEW; istat[4 * (int64_t)p + 1] = 0; istat[4 * (int64_t)p + 2] = 0; istat[4 * (int64_t)p + 3] = s.n;
            for (int i = 0; i < 36; ++i) Q[36 * (int64_t)p + i] = nan;
        }
    }
    __syncthreads();
    if (s.code == PA_TOO_FEW) return;                     // uniform: read from LDS
    const int n = s.n;
    const double floor_f = PA_FLOOR * 4.0 * (double)n;

    // ---- the damped loop ------------------------------------------------------------------------------------------------
    const int max_trials = PA_MAX_REJECT * max_iter;
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
                for (int c = a; c < 5; ++c) acc[pa_s5(a, c)] += b.A[a] * b.A[c] + b.A[5 + a] * b.A[5 + c];
                acc[30 + a] += b.A[a] * b.r[2] + b.A[5 + a] * b.r[3];
            }
            double L[6];
            if (!pa_chol3(b.V, lambda, 0.0, L)) { acc[40] += 1.0; continue; }
            double Z[15];                                 // row a: V^-1 W(a, :)'
#pragma unroll
            for (int a = 0; a < 5; ++a) pa_solve3(L, b.W + 3 * a, Z + 3 * a);
#pragma unroll
            for (int a = 0; a < 5; ++a) {
#pragma unroll
                for (int c = a; c < 5; ++c) acc[15 + pa_s5(a, c)] += b.W[3 * a] * Z[3 * c] + b.W[3 * a + 1] * Z[3 * c + 1] + b.W[3 * a + 2] * Z[3 * c + 2];
                acc[35 + a] += Z[3 * a] * b.g[0] + Z[3 * a + 1] * b.g[1] + Z[3 * a + 2] * b.g[2];
            }
        }
        pa_reduce<PA_NSUM>(acc, s.part);
        __syncthreads();
        if (tid == 0) {
            double *S = s.S, *dp = s.dp, *gp = s.gp;
            for (int i = 0; i < 15; ++i) S[i] = pa_total<PA_NSUM>(s.part, i) - pa_total<PA_NSUM>(s.part, 15 + i);
            for (int a = 0; a < 5; ++a) {
                S[pa_s5(a, a)] = pa_total<PA_NSUM>(s.part, pa_s5(a, a)) + lambda * pa_total<PA_NSUM>(s.part, pa_s5(a, a)) - pa_total<PA_NSUM>(s.part, 15 + pa_s5(a, a));
                gp[a] = pa_total<PA_NSUM>(s.part, 30 + a);
                dp[a] = gp[a] - pa_total<PA_NSUM>(s.part, 35 + a);
            }
            bool ok = pa_total<PA_NSUM>(s.part, 40) == 0.0;
            ok = pa_chol5(S, 0.0) && ok;
            pa_solve5(S, dp);
            double gd = 0.0;
            for (int a = 0; a < 5; ++a) { dp[a] = -dp[a]; gd += gp[a] * dp[a]; ok = ok && (dp[a] - dp[a] == 0.0); }
            if (!ok) for (int a = 0; a < 5; ++a) dp[a] = 0.0;
            const double t0 = s.t[0] + s.B[0] * dp[3] + s.B[3] * dp[4], t1 = s.t[1] + s.B[1] * dp[3] + s.B[4] * dp[4];
            const double t2 = s.t[2] + s.B[2] * dp[3] + s.B[5] * dp[4], nn = sqrt(t0 * t0 + t1 * t1 + t2 * t2);
            s.tn[0] = t0 / nn; s.tn[1] = t1 / nn; s.tn[2] = t2 / nn;
            pa_rotate_dd(dp, s.R, s.Rn, s.G, s.T);
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
        PaDD ft = {0.0, 0.0};
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
                const bool okv = pa_chol3(b.V, lambda, 0.0, L);
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    rhs[k] = b.g[k] + (b.W[k] * dp[0] + b.W[3 + k] * dp[1] + b.W[6 + k] * dp[2] + b.W[9 + k] * dp[3] + b.W[12 + k] * dp[4]);
                pa_solve3(L, rhs, d);
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
            const PaDD ft = pa_total_dd(s.part2);
            const double q = -(s.gpdp + pa_total<4>(s.part2, 2)), bad = pa_total<4>(s.part2, 3);
            const bool ok = s.solved != 0;
            s.trials += 1; s.accepted = 0;
            if (s.f <= floor_f || (ok && q <= tol2 * s.f)) { s.code = PA_CONVERGED; s.done = 1; }
            else if (ok && bad == 0.0 && (ft.hi - ft.hi == 0.0) && pa_dd_less(ft, PaDD{s.f, s.flo})) {
                for (int i = 0; i < 18; ++i) s.R[i] = s.Rn[i];
                for (int i = 0; i < 3; ++i) s.t[i] = s.tn[i];
                pa_basis(s.t, s.B);
                s.f = ft.hi; s.flo = ft.lo; s.lambda = fmax(s.lambda / 10.0, PA_LAMBDA_MIN); s.iters += 1; s.accepted = 1;
                if (s.iters >= max_iter) { s.code = PA_MAX_ITER; s.done = 1; }
            } else {
                s.lambda = s.lambda * 10.0;
                if (s.lambda > PA_LAMBDA_MAX) { s.code = PA_NO_STEP; s.done = 1; }
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
            for (int c = a; c < 5; ++c) acc[pa_s5(a, c)] += b.A[a] * b.A[c] + b.A[5 + a] * b.A[5 + c];
        double L[6];
        if (!pa_chol3(b.V, 0.0, PA_V_PIVOT, L)) { acc[40] += 1.0; continue; }
        double Z[15];
#pragma unroll
        for (int a = 0; a < 5; ++a) pa_solve3(L, b.W + 3 * a, Z + 3 * a);
#pragma unroll
        for (int a = 0; a < 5; ++a)
#pragma unroll
            for (int c = a; c < 5; ++c) acc[15 + pa_s5(a, c)] += b.W[3 * a] * Z[3 * c] + b.W[3 * a + 1] * Z[3 * c + 1] + b.W[3 * a + 2] * Z[3 * c + 2];
    }
    pa_reduce<PA_NSUM>(acc, s.part);
    __syncthreads();
    if (tid == 0) {
        double *S = s.S, *Si = s.Si, *Bf = s.Bf, *e = s.e;
        for (int i = 0; i < 15; ++i) S[i] = pa_total<PA_NSUM>(s.part, i) - pa_total<PA_NSUM>(s.part, 15 + i);
        bool singular = pa_total<PA_NSUM>(s.part, 40) != 0.0;
        singular = !pa_chol5(S, PA_S_PIVOT) || singular;
        for (int c = 0; c < 5; ++c) {
            for (int r = 0; r < 5; ++r) e[r] = r == c ? 1.0 : 0.0;
            pa_solve5(S, e);
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
        if (code == PA_CONVERGED && singular) code = PA_SINGULAR;
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
