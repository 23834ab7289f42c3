// Double-double arithmetic (a number as the unevaluated sum of two doubles) and the rotations kept in it: what the
// adjustment kernels (pairadjust.hpp, poseadjust.hpp, pointadjust.hpp; their shared loop: lm_core.hpp) evaluate their
// objective with.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace dbat {

// Rn = exp([a]x) R (column-major 3 x 3) by Rodrigues' formula, (1 - cos th) / th^2 as 2 sin^2(th / 2) / th^2.
__host__ __device__ inline void dd_rotate(const double *a, const double *R, double *Rn) {
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

#if defined(__HIPCC__)

// ---- the objective in double-double ----------------------------------------------------------------------------------
// A trial is accepted only if its objective is smaller, and near the optimum the decrease of a step falls below the
// rounding of a float64 evaluation (a residual is a weight of 1e3 .. 1e4 times the difference of two coordinates of
// order one: 1e-13 of it is noise, and as much of f): the accept test then answers at random and the iteration stops
// sqrt(noise / curvature) short of the optimum, 1e-9 in a weak direction.  So the residuals are formed from
// R X + t - x (R X + t)_3 carried as unevaluated sums of two doubles (error-free products by fma, sums by Knuth's
// two-sum) and f is summed the same way; only the accept test reads the low word.  R itself is such a sum, kept
// orthonormal to 1e-31 (dd_orthonormalise).  The Jacobians and the normal equations are plain float64.
struct Dd { double hi, lo; };
// (contraction is off in these: fusing a product into the sum that follows it, the compiler's default here, breaks the
// error-free transformations -- two-sum must see the rounded product that two-prod took the error of)
__device__ __forceinline__ Dd dd_two_sum(double a, double b) {
#pragma clang fp contract(off)
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
__device__ __forceinline__ Dd dd_two_prod(double a, double b) {
#pragma clang fp contract(off)
    const double p = a * b;
    return {p, __builtin_fma(a, b, -p)};
}
__device__ __forceinline__ Dd dd_add(Dd x, Dd y) {
#pragma clang fp contract(off)
    Dd s = dd_two_sum(x.hi, y.hi);
    s.lo += x.lo + y.lo;
    const double h = s.hi + s.lo;
    return {h, s.lo - (h - s.hi)};
}
__device__ __forceinline__ Dd dd_fma(Dd x, double a, double b) { return dd_add(x, dd_two_prod(a, b)); }        // x + a b
__device__ __forceinline__ Dd dd_fma(Dd x, double a, Dd b) {                                                   // x + a b
#pragma clang fp contract(off)
    Dd p = dd_two_prod(a, b.hi);
    p.lo = __builtin_fma(a, b.lo, p.lo);
    return dd_add(x, p);
}
__device__ __forceinline__ bool dd_less(Dd a, Dd b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }

__device__ __forceinline__ Dd dd_mul(Dd a, Dd b) {
#pragma clang fp contract(off)
    Dd p = dd_two_prod(a.hi, b.hi);
    const double c = a.hi * b.lo, d = a.lo * b.hi;
    p.lo += c + d;
    const double h = p.hi + p.lo;
    return {h, p.lo - (h - p.hi)};
}

__device__ __forceinline__ Dd dd_div(Dd a, Dd b) {
#pragma clang fp contract(off)
    const double q1 = a.hi / b.hi;
    const Dd r = dd_fma(a, -q1, b);
    return dd_two_sum(q1, r.hi / b.hi);
}

// R <- R (3 I - R'R) / 2 on the double-double R (18 entries), one Newton step towards the nearest rotation: a product
// of float64 rotations is orthonormal to 1e-16, after the step to 1e-31.  Why: the six directions in which a 3 x 3 matrix
// leaves the rotations are directions in which f does not have a zero gradient at the optimum, so their rounding --
// drawn anew by every trial -- moves f by 1e-12 and more, and the accept test would again answer at random.  G, T:
// work arrays of 18.  For one thread.
__device__ inline void dd_orthonormalise(double *R, double *G, double *T) {
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            Dd g = {0.0, 0.0};
            for (int r = 0; r < 3; ++r) g = dd_add(g, dd_mul(Dd{R[3 * a + r], R[9 + 3 * a + r]}, Dd{R[3 * b + r], R[9 + 3 * b + r]}));
            g = dd_add(Dd{a == b ? 3.0 : 0.0, 0.0}, Dd{-g.hi, -g.lo});
            G[3 * b + a] = 0.5 * g.hi; G[9 + 3 * b + a] = 0.5 * g.lo;
        }
    for (int b = 0; b < 3; ++b)
        for (int r = 0; r < 3; ++r) {
            Dd v = {0.0, 0.0};
            for (int a = 0; a < 3; ++a) v = dd_add(v, dd_mul(Dd{R[3 * a + r], R[9 + 3 * a + r]}, Dd{G[3 * b + a], G[9 + 3 * b + a]}));
            T[3 * b + r] = v.hi; T[9 + 3 * b + r] = v.lo;
        }
    for (int i = 0; i < 18; ++i) R[i] = T[i];
}

// Rn = exp([a]x) R on the double-double R, orthonormalised.  For one thread.
__device__ inline void dd_rotate_dd(const double *a, const double *R, double *Rn, double *G, double *T) {
    double E[9];
    const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    dd_rotate(a, I3, E);                                  // column-major exp([a]x)
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) {
            Dd v = {0.0, 0.0};
#pragma unroll
            for (int k = 0; k < 3; ++k) v = dd_fma(v, E[3 * k + r], Dd{R[3 * c + k], R[9 + 3 * c + k]});
            T[3 * c + r] = v.hi; T[9 + 3 * c + r] = v.lo;
        }
    for (int i = 0; i < 18; ++i) Rn[i] = T[i];
    dd_orthonormalise(Rn, G, T);
}

#endif  // __HIPCC__

}  // namespace dbat
