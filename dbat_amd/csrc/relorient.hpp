// Relative orientation of image pairs (dbat_hip_essmat5, dbat_hip_relorient): essential matrices from five or more
// correspondences (photogrammetry/essmat5.m:9-43), a RANSAC over host-drawn minimal samples scored by the Sampson
// distance, and the camera pair and points of the winner (photogrammetry/camsfrome.m:16-59).
//
//   k_essmat5      one lane per sample.  The n x 9 design matrix (essmat5.m:12-20) is folded row by row into a 9 x 9
//                  triangle by Givens rotations (a fixed order: the rows ascending), the triangle's columns are made
//                  orthogonal by one-sided Jacobi rotations (Hestenes), and the four columns of V that belong to the
//                  smallest singular values span E = x E1 + y E2 + z E3 + E4 (:23-24; E4 the smallest).  The same
//                  directions as the eigenvectors of the 9 x 9 Gram matrix, without squaring the condition number.
//                  det E = 0 and E E' E - tr(E E') E / 2 = 0 are expanded by polynomial products (ro_mul11, ro_mul21:
//                  linear x linear, quadratic x linear; the monomial indices are constexpr functions, no table) into
//                  the 10 x 20 matrix, Gauss-Jordan with row pivoting reduces its first ten columns, and the rows of
//                  x^2 z, x^2, y^2 z, y^2, x y z, x y give B(z) [x y 1]' = 0 with det B(z) of degree ten (Nister 2004).
//                  Its real roots come from the chain of its derivatives -- between two neighbouring roots of p' p is
//                  monotone, so a sign change brackets one root and bisection finds it: real arithmetic only, every
//                  loop of a fixed length.  x, y from the null vector of B(z); the solution is then polished by three
//                  Gauss-Newton steps against the constraints evaluated on the matrix itself.  Solutions in ascending z.
//                  The 10 x 20 matrix does not fit a lane's registers: a sample's RO_WS doubles live in LDS, element k of
//                  lane l at [k * RO_WG + l] (a lane's elements 64 doubles apart: every access of a wave is conflict-free).
//   k_ro_score     one lane per model (10 slots per sample), the pair's correspondences tiled through LDS; integer
//                  counts; the winner by a 64-bit integer maximum of (count, -slot): the highest count, ties to the
//                  lowest (sample, solution).  No floating-point atomics.
//   k_ro_winner    per pair: the winning slot's E and the statistics
//   k_ro_cams      one lane per correspondence: the ray-distance intersection of pm_forwintersect3.m:55-82 for two rays
//                  under the four [R | +-u3] of camsfrome.m:33 (first pass: the in-front counts, integer atomics) or
//                  under the chosen one (second pass: X, the in-front mask, the inlier mask)
//
// The host side (relorient_host.hpp) draws nothing: the sample index lists are an input.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

namespace dbat {

constexpr int RO_WG = 64;            // samples of a workgroup of k_essmat5, one lane each
constexpr int RO_WS = 236;           // doubles of LDS per sample: the 10 x 20 matrix (200) and the basis E1 .. E4 (36)
constexpr int RO_BASIS = 200;        // offset of the basis: [9 m + e], m = 0 .. 3 for x, y, z, 1
constexpr int RO_SWEEPS = 15;        // Jacobi sweeps at most (nine columns converge in six to eight)
constexpr int RO_BISECT = 128;       // bisection steps at most per root (an interval of 1e16 down to one ulp: 107)
constexpr int RO_SCORE_WG = 256;     // models of a workgroup of k_ro_score; also the correspondences of an LDS tile
constexpr double RO_RANK_TOL = 1e-10;   // fifth-smallest singular value at or below this share of the largest: no solution
constexpr double RO_PARALLAX2 = 1e-24;  // |d1 x d2|^2 of two unit rays at or below this: the intersection is not defined

// a sample's workspace: element i at p[i * st]
struct RoWs {
    double *p; int st;
    __host__ __device__ double &operator[](int i) const { return p[(size_t)i * st]; }
};

// ---- monomials -------------------------------------------------------------------------------------------------
// Linear forms are over (x, y, z, 1), variables 0 .. 3.  Quadratic monomials: the pairs i <= j in lexicographic order.
// Cubic monomials in the order the elimination wants (the first ten are reduced, the last ten stay):
//   x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1
__host__ __device__ constexpr int ro_q(int i, int j) { return i <= j ? i * 4 - i * (i - 1) / 2 + (j - i) : j * 4 - j * (j - 1) / 2 + (i - j); }
// exponents of x, y, z as 16 a + 4 b + c of cubic monomial m, and back
__host__ __device__ constexpr int ro_code(int m) {
    switch (m) {
        case 0: return 48; case 1: return 12; case 2: return 36; case 3: return 24; case 4: return 33;
        case 5: return 32; case 6: return 9; case 7: return 8; case 8: return 21; case 9: return 20;
        case 10: return 18; case 11: return 17; case 12: return 16; case 13: return 6; case 14: return 5;
        case 15: return 4; case 16: return 3; case 17: return 2; case 18: return 1; default: return 0;
    }
}
__host__ __device__ constexpr int ro_mono(int code) {
    switch (code) {
        case 48: return 0; case 12: return 1; case 36: return 2; case 24: return 3; case 33: return 4;
        case 32: return 5; case 9: return 6; case 8: return 7; case 21: return 8; case 20: return 9;
        case 18: return 10; case 17: return 11; case 16: return 12; case 6: return 13; case 5: return 14;
        case 4: return 15; case 3: return 16; case 2: return 17; case 1: return 18; default: return 19;
    }
}
__host__ __device__ constexpr int ro_pw(int v) { return v == 0 ? 16 : v == 1 ? 4 : v == 2 ? 1 : 0; }
__host__ __device__ constexpr int ro_c(int i, int j, int k) { return ro_mono(ro_pw(i) + ro_pw(j) + ro_pw(k)); }

// q += sg * a * b (linear x linear), c += q * l (quadratic x linear)
__host__ __device__ __forceinline__ void ro_mul11(const double *a, const double *b, double *q, double sg) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) q[ro_q(i, j)] = __builtin_fma(sg * a[i], b[j], q[ro_q(i, j)]);
}
__host__ __device__ __forceinline__ void ro_mul21(const double *q, const double *l, double *c) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) c[ro_c(i, j, k)] = __builtin_fma(q[ro_q(i, j)], l[k], c[ro_c(i, j, k)]);
}

// ---- the four smallest right singular directions ------------------------------------------------------------------
// One row (q1, q2) of the design matrix, essmat5.m:12-20: w[a + 3 b] = q1[a] q2[b]
__host__ __device__ __forceinline__ void ro_design_row(const double *q1, const double *q2, double *w) {
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
        for (int a = 0; a < 3; ++a) w[a + 3 * b] = q1[a] * q2[b];
}

// Folds w into the upper triangle T (ws[9 r + c], r <= c) by nine Givens rotations.
__host__ __device__ inline void ro_fold_row(const RoWs &ws, double *w) {
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const double a = ws[10 * k], b = w[k], r = hypot(a, b);
        if (!(r > 0)) continue;
        const double cs = a / r, sn = b / r;
        ws[10 * k] = r;
#pragma unroll
        for (int c = k + 1; c < 9; ++c) {
            const double t = ws[9 * k + c];
            ws[9 * k + c] = __builtin_fma(cs, t, sn * w[c]);
            w[c] = __builtin_fma(cs, w[c], -sn * t);
        }
    }
}

// T (ws[0 .. 80], rows below the diagonal zero, rows from nr on zero altogether) -> the basis at RO_BASIS.  V at ws[81 + 9 col + row].  False: the
// sample is rank-deficient (or not finite).
__host__ __device__ inline bool ro_basis(const RoWs &ws, int nr) {
    double fro = 0;
    for (int i = 0; i < 81; ++i) { fro = __builtin_fma(ws[i], ws[i], fro); ws[81 + i] = (i % 10 == 0) ? 1.0 : 0.0; }
    if (!(fro > 0) || !(fro < INFINITY)) return false;
    const double tiny = 4.9e-32 * fro;                    // a column of this squared length is a null column already
    for (int sweep = 0; sweep < RO_SWEEPS; ++sweep) {
        bool moved = false;
        for (int p = 0; p < 8; ++p)
            for (int q = p + 1; q < 9; ++q) {
                double a = 0, b = 0, c = 0;
                for (int i = 0; i < nr; ++i) {
                    const double gp = ws[9 * i + p], gq = ws[9 * i + q];
                    a = __builtin_fma(gp, gp, a); b = __builtin_fma(gq, gq, b); c = __builtin_fma(gp, gq, c);
                }
                if (!(a > tiny) || !(b > tiny) || !(fabs(c) > 2.220446049250313e-16 * (sqrt(a) * sqrt(b)))) continue;
                moved = true;
                const double zeta = (b - a) / (2 * c);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1 + zeta * zeta));
                const double cs = 1 / sqrt(1 + t * t), sn = cs * t;
                for (int i = 0; i < nr; ++i) {
                    const double gp = ws[9 * i + p], gq = ws[9 * i + q];
                    ws[9 * i + p] = cs * gp - sn * gq; ws[9 * i + q] = sn * gp + cs * gq;
                }
                for (int i = 0; i < 9; ++i) {
                    const double vp = ws[81 + 9 * p + i], vq = ws[81 + 9 * q + i];
                    ws[81 + 9 * p + i] = cs * vp - sn * vq; ws[81 + 9 * q + i] = sn * vp + cs * vq;
                }
            }
        if (!moved) break;
    }
    // the squared column lengths, in ws[162 .. 170]; the four smallest by selection, the largest of them first
    double top = 0;
    for (int j = 0; j < 9; ++j) {
        double a = 0;
        for (int i = 0; i < nr; ++i) a = __builtin_fma(ws[9 * i + j], ws[9 * i + j], a);
        ws[162 + j] = a;
        top = fmax(top, a);
    }
    for (int m = 3; m >= 0; --m) {                        // m = 3: the smallest of all (E4), the first of equal ones
        int arg = -1;
        double best = INFINITY;
        for (int j = 0; j < 9; ++j) { const double a = ws[162 + j]; if (a >= 0 && a < best) { best = a; arg = j; } }
        if (arg < 0) return false;
        ws[162 + arg] = -1.0;
        for (int i = 0; i < 9; ++i) ws[RO_BASIS + 9 * m + i] = ws[81 + 9 * arg + i];
    }
    double fifth = INFINITY;
    for (int j = 0; j < 9; ++j) { const double a = ws[162 + j]; if (a >= 0) fifth = fmin(fifth, a); }
    return fifth > RO_RANK_TOL * RO_RANK_TOL * top;
}

// ---- the constraints ---------------------------------------------------------------------------------------------
// The basis at RO_BASIS -> the 10 x 20 matrix A(row, col) = ws[10 col + row]: row 0 det E, rows 1 .. 9 the entries of
// (E E' - tr(E E') / 2 I) E.  E(r, c) = e[r + 3 c]; the constraints hold for E' as well as for E.
__host__ __device__ inline void ro_constraints(const RoWs &ws) {
    double E[9][4];
#pragma unroll
    for (int e = 0; e < 9; ++e)
#pragma unroll
        for (int m = 0; m < 4; ++m) E[e][m] = ws[RO_BASIS + 9 * m + e];
    {
        double cub[20];
#pragma unroll
        for (int k = 0; k < 20; ++k) cub[k] = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {                     // E(0, c) times its cofactor
            const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
            double q[10];
#pragma unroll
            for (int k = 0; k < 10; ++k) q[k] = 0;
            ro_mul11(E[1 + 3 * c1], E[2 + 3 * c2], q, 1.0);
            ro_mul11(E[1 + 3 * c2], E[2 + 3 * c1], q, -1.0);
            ro_mul21(q, E[3 * c], cub);
        }
#pragma unroll
        for (int k = 0; k < 20; ++k) ws[10 * k] = cub[k];
    }
    double S[6][10];                                      // E E' (symmetric: (r, s), r <= s, at ro_s below)
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int s = r; s < 3; ++s) {
            double *q = S[r * 3 - r * (r - 1) / 2 + (s - r)];
#pragma unroll
            for (int k = 0; k < 10; ++k) q[k] = 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) ro_mul11(E[r + 3 * c], E[s + 3 * c], q, 1.0);
        }
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        const double ht = 0.5 * (S[0][k] + S[3][k] + S[5][k]);
        S[0][k] -= ht; S[3][k] -= ht; S[5][k] -= ht;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double cub[20];
#pragma unroll
            for (int k = 0; k < 20; ++k) cub[k] = 0;
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const int lo = r < s ? r : s, hi = r < s ? s : r;
                ro_mul21(S[lo * 3 - lo * (lo - 1) / 2 + (hi - lo)], E[s + 3 * c], cub);
            }
#pragma unroll
            for (int k = 0; k < 20; ++k) ws[10 * k + 1 + r + 3 * c] = cub[k];
        }
}

// Gauss-Jordan with row pivoting on the first ten columns.  False: a pivot at or below 1e-13 of the largest entry.
__host__ __device__ inline bool ro_eliminate(const RoWs &ws) {
    double big = 0;
    for (int i = 0; i < 200; ++i) big = fmax(big, fabs(ws[i]));
    if (!(big > 0) || !(big < INFINITY)) return false;
    for (int k = 0; k < 10; ++k) {
        int arg = k;
        double best = fabs(ws[10 * k + k]);
        for (int r = k + 1; r < 10; ++r) { const double v = fabs(ws[10 * k + r]); if (v > best) { best = v; arg = r; } }
        if (!(best > 1e-13 * big)) return false;
        const double inv = 1.0 / ws[10 * k + arg];
        for (int c = k; c < 20; ++c) {
            const double v = ws[10 * c + arg] * inv;
            ws[10 * c + arg] = ws[10 * c + k];
            ws[10 * c + k] = v;
        }
        for (int r = 0; r < 10; ++r) {
            if (r == k) continue;
            const double f = ws[10 * k + r];
            for (int c = k; c < 20; ++c) ws[10 * c + r] = __builtin_fma(-f, ws[10 * c + k], ws[10 * c + r]);
        }
    }
    return true;
}

// ---- the tenth-degree polynomial and its real roots --------------------------------------------------------------
// The first hundred doubles (columns 0 .. 9, the identity after the elimination) are free from here on:
//   [0 .. 38]  B(z): row t (the pairs of rows 4/5, 6/7, 8/9) at 13 t: the x cubic (z^3 .. 1), the y cubic, the quartic
//   [39 .. 49] p, ascending powers     [50 .. 60] the derivative at hand     [61 .. 70], [71 .. 80] two root lists
constexpr int RO_P = 39, RO_D = 50, RO_RA = 61, RO_RB = 71;
#define RO_C(row, j) ws[10 * (10 + (j)) + (row)]     // the reduced matrix: entry of monomial 10 + j in a row

__host__ __device__ inline void ro_hidden_variable(const RoWs &ws) {
    for (int t = 0; t < 3; ++t) {
        const int e = 4 + 2 * t, f = 5 + 2 * t;              // row(e) - z row(f)
        for (int g = 0; g < 2; ++g) {                        // the x and the y cubic
            ws[13 * t + 4 * g + 0] = -RO_C(f, 3 * g);
            ws[13 * t + 4 * g + 1] = RO_C(e, 3 * g) - RO_C(f, 3 * g + 1);
            ws[13 * t + 4 * g + 2] = RO_C(e, 3 * g + 1) - RO_C(f, 3 * g + 2);
            ws[13 * t + 4 * g + 3] = RO_C(e, 3 * g + 2);
        }
        ws[13 * t + 8] = -RO_C(f, 6);
        ws[13 * t + 9] = RO_C(e, 6) - RO_C(f, 7);
        ws[13 * t + 10] = RO_C(e, 7) - RO_C(f, 8);
        ws[13 * t + 11] = RO_C(e, 8) - RO_C(f, 9);
        ws[13 * t + 12] = RO_C(e, 9);
    }
    for (int i = 0; i <= 10; ++i) ws[RO_P + i] = 0;
    for (int t = 0; t < 3; ++t) {                            // det B: the quartic of row t times its cofactor
        const int t1 = (t + 1) % 3, t2 = (t + 2) % 3;
        double m[7] = {0, 0, 0, 0, 0, 0, 0};                 // x(t1) y(t2) - x(t2) y(t1), descending powers z^6 .. 1
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                m[i + j] += ws[13 * t1 + i] * ws[13 * t2 + 4 + j] - ws[13 * t2 + i] * ws[13 * t1 + 4 + j];
#pragma unroll
        for (int i = 0; i < 7; ++i)
#pragma unroll
            for (int j = 0; j < 5; ++j) ws[RO_P + 10 - (i + j)] += m[i] * ws[13 * t + 8 + j];
    }
}

// value of the polynomial of degree m at RO_D (ascending powers)
__host__ __device__ __forceinline__ double ro_horner(const RoWs &ws, int m, double z) {
    double v = ws[RO_D + m];
    for (int i = m - 1; i >= 0; --i) v = __builtin_fma(v, z, ws[RO_D + i]);
    return v;
}

// Real roots of p (RO_P) in ascending order into RO_RA or RO_RB; returns their number, the list through at.
__host__ __device__ inline int ro_real_roots(const RoWs &ws, int &at) {
    int deg = 10;
    double big = 0;
    for (int i = 0; i <= 10; ++i) big = fmax(big, fabs(ws[RO_P + i]));
    if (!(big > 0) || !(big < INFINITY)) return 0;
    while (deg > 0 && !(fabs(ws[RO_P + deg]) > 0)) --deg;
    if (deg < 1) return 0;
    double bound = 0;
    for (int i = 0; i < deg; ++i) bound = fmax(bound, fabs(ws[RO_P + i] / ws[RO_P + deg]));
    const double R = 1.0 + bound;                          // Cauchy: every root of p and of its derivatives is inside
    if (!(R < 1e150)) return 0;
    int prev = RO_RA, cur = RO_RB, nprev = 0;
    for (int m = 1; m <= deg; ++m) {                       // the derivative of order deg - m: degree m
        const int k = deg - m;
        for (int j = 0; j <= m; ++j) {
            double ff = 1;
            for (int i = 0; i < k; ++i) ff *= (double)(j + k - i);
            ws[RO_D + j] = ws[RO_P + j + k] * ff;
        }
        int ncur = 0;
        double lo = -R, flo = ro_horner(ws, m, lo);
        for (int s = 0; s <= nprev; ++s) {
            const double hi = s < nprev ? ws[prev + s] : R, fhi = ro_horner(ws, m, hi);
            if ((flo > 0) != (fhi > 0)) {
                double a = lo, b = hi;
                const bool up = fhi > 0;
                for (int it = 0; it < RO_BISECT; ++it) {
                    const double mid = 0.5 * (a + b);
                    if (!(mid > a) || !(mid < b)) break;
                    if ((ro_horner(ws, m, mid) > 0) == up) b = mid; else a = mid;
                }
                ws[cur + ncur++] = 0.5 * (a + b);
            }
            lo = hi; flo = fhi;
        }
        const int t = prev; prev = cur; cur = t;
        nprev = ncur;
    }
    at = prev;
    return nprev;
}

// ---- from a root to a solution -----------------------------------------------------------------------------------
// 3 x 3 products of column-major matrices: A B' and A B
__host__ __device__ __forceinline__ void ro_abt(const double *A, const double *B, double *o) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int s = 0; s < 3; ++s) o[r + 3 * s] = __builtin_fma(A[r], B[s], __builtin_fma(A[r + 3], B[s + 3], A[r + 6] * B[s + 6]));
}
__host__ __device__ __forceinline__ void ro_ab(const double *A, const double *B, double *o) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) o[r + 3 * c] = __builtin_fma(A[r], B[3 * c], __builtin_fma(A[r + 3], B[3 * c + 1], A[r + 6] * B[3 * c + 2]));
}

// The ten constraints at E = sum c[m] E_m (|c| = 1), evaluated on the matrix itself: r[0] = det E, r[1 ..] =
// E E' E - tr(E E') E / 2.  With J: also their derivatives along the four basis directions, J[m][.].  Returns |r|^2.
__host__ __device__ inline double ro_on_matrix(const RoWs &ws, const double *c, double *r, double (*J)[10]) {
    double E[9], S[9], SE[9], cof[9];
#pragma unroll
    for (int i = 0; i < 9; ++i)
        E[i] = __builtin_fma(c[0], ws[RO_BASIS + i], __builtin_fma(c[1], ws[RO_BASIS + 9 + i], __builtin_fma(c[2], ws[RO_BASIS + 18 + i], c[3] * ws[RO_BASIS + 27 + i])));
    ro_abt(E, E, S);
    ro_ab(S, E, SE);
    const double h = 0.5 * (S[0] + S[4] + S[8]);
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) {                      // cofactors: d det / d E(r, c)
        const int c1 = (cc + 1) % 3, c2 = (cc + 2) % 3;
#pragma unroll
        for (int rr = 0; rr < 3; ++rr) {
            const int r1 = (rr + 1) % 3, r2 = (rr + 2) % 3;
            cof[rr + 3 * cc] = E[r1 + 3 * c1] * E[r2 + 3 * c2] - E[r1 + 3 * c2] * E[r2 + 3 * c1];
        }
    }
    r[0] = E[0] * cof[0] + E[3] * cof[3] + E[6] * cof[6];
    double sum = r[0] * r[0];
#pragma unroll
    for (int i = 0; i < 9; ++i) { r[1 + i] = __builtin_fma(-h, E[i], SE[i]); sum = __builtin_fma(r[1 + i], r[1 + i], sum); }
    if (!J) return sum;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        double D[9], G[9], dS[9], t1[9], t2[9];
        double dd = 0;
#pragma unroll
        for (int i = 0; i < 9; ++i) { D[i] = ws[RO_BASIS + 9 * m + i]; dd = __builtin_fma(cof[i], D[i], dd); }
        ro_abt(D, E, G);                                  // d(E E') = G + G'
#pragma unroll
        for (int rr = 0; rr < 3; ++rr)
#pragma unroll
            for (int s = 0; s < 3; ++s) dS[rr + 3 * s] = G[rr + 3 * s] + G[s + 3 * rr];
        ro_ab(dS, E, t1);
        ro_ab(S, D, t2);
        const double dh = G[0] + G[4] + G[8];
        J[m][0] = dd;
#pragma unroll
        for (int i = 0; i < 9; ++i) J[m][1 + i] = t1[i] + t2[i] - dh * E[i] - h * D[i];
    }
    return sum;
}

// The solution of the root z: (x, y, 1) from the null vector of B(z), taken homogeneously (no division), then three
// Gauss-Newton steps on the unit sphere of c, E = c1 E1 + c2 E2 + c3 E3 + c4 E4, against the ten constraints evaluated
// on the matrix -- the reduced cubics carry the rounding of the elimination, the matrix does not.  A step is kept only
// if it lowers |r|^2.  e: E at unit norm (the basis is orthonormal: |E| = |c|).  False: no finite solution.
__host__ __device__ inline bool ro_solution(const RoWs &ws, double z, double *e) {
    double B[3][3];
    for (int t = 0; t < 3; ++t) {
        for (int g = 0; g < 2; ++g) {
            double v = ws[13 * t + 4 * g];
            for (int i = 1; i < 4; ++i) v = __builtin_fma(v, z, ws[13 * t + 4 * g + i]);
            B[t][g] = v;
        }
        double v = ws[13 * t + 8];
        for (int i = 1; i < 5; ++i) v = __builtin_fma(v, z, ws[13 * t + 8 + i]);
        B[t][2] = v;
    }
    double c[4] = {0, 0, 0, 0}, bestn = -1;
#pragma unroll
    for (int t = 0; t < 3; ++t) {                             // the cross product of two rows: the longest of the three
        const int t1 = (t + 1) % 3, t2 = (t + 2) % 3;
        const double n0 = B[t1][1] * B[t2][2] - B[t1][2] * B[t2][1], n1 = B[t1][2] * B[t2][0] - B[t1][0] * B[t2][2];
        const double w = B[t1][0] * B[t2][1] - B[t1][1] * B[t2][0];
        const double len = fabs(n0) + fabs(n1) + fabs(w);
        if (len > bestn) { bestn = len; c[0] = n0 / len; c[1] = n1 / len; c[3] = w / len; }
    }
    c[2] = z * c[3];
    double cn = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2] + c[3] * c[3]);
    if (!(cn > 0) || !(cn < INFINITY)) return false;
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] /= cn;
    double r[10], J[4][10];
    double rr = ro_on_matrix(ws, c, r, J);
    for (int it = 0; it < 3; ++it) {
        // (J'J + c c') d = -J'r: the step in the tangent plane of the sphere; Cholesky of the 4 x 4
        double N[4][4], g[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < 10; ++k) s = __builtin_fma(J[i][k], r[k], s);
            g[i] = -s;
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                double a = c[i] * c[j];
#pragma unroll
                for (int k = 0; k < 10; ++k) a = __builtin_fma(J[i][k], J[j][k], a);
                N[i][j] = a;
            }
        }
        bool pd = true;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double d = N[j][j];
#pragma unroll
            for (int k = 0; k < j; ++k) d -= N[j][k] * N[j][k];
            pd = pd && d > 0;
            d = sqrt(d);
            N[j][j] = d;
#pragma unroll
            for (int i = j + 1; i < 4; ++i) {
                double a = N[i][j];
#pragma unroll
                for (int k = 0; k < j; ++k) a -= N[i][k] * N[j][k];
                N[i][j] = a / d;
            }
        }
        if (!pd) break;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int k = 0; k < i; ++k) g[i] -= N[i][k] * g[k];
            g[i] /= N[i][i];
        }
#pragma unroll
        for (int i = 3; i >= 0; --i) {
#pragma unroll
            for (int k = i + 1; k < 4; ++k) g[i] -= N[k][i] * g[k];
            g[i] /= N[i][i];
        }
        double w[4], wn = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) { w[i] = c[i] + g[i]; wn = __builtin_fma(w[i], w[i], wn); }
        wn = sqrt(wn);
        if (!(wn > 0) || !(wn < INFINITY)) break;
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] /= wn;
        double r2[10], J2[4][10];
        const double rr2 = ro_on_matrix(ws, w, r2, J2);
        if (!(rr2 < rr)) break;                               // no better (or not finite): keep what there is
        rr = rr2;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            c[i] = w[i];
#pragma unroll
            for (int k = 0; k < 10; ++k) J[i][k] = J2[i][k];
        }
#pragma unroll
        for (int k = 0; k < 10; ++k) r[k] = r2[k];
    }
    double n2 = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        e[i] = __builtin_fma(c[0], ws[RO_BASIS + i], __builtin_fma(c[1], ws[RO_BASIS + 9 + i], __builtin_fma(c[2], ws[RO_BASIS + 18 + i], c[3] * ws[RO_BASIS + 27 + i])));
        n2 = __builtin_fma(e[i], e[i], n2);
    }
    const double n = sqrt(n2);
    if (!(n > 0) || !(n < INFINITY)) return false;
#pragma unroll
    for (int i = 0; i < 9; ++i) e[i] /= n;
    return true;
}
#undef RO_C

// The solver after the rows have been folded in (nr = min(n, 9) of the triangle's rows are not zero): store(k, e) per
// solution, returns their number.
template <class Store>
__host__ __device__ inline int ro_solve(const RoWs &ws, int nr, Store &&store) {
    if (!ro_basis(ws, nr)) return 0;
    ro_constraints(ws);
    if (!ro_eliminate(ws)) return 0;
    ro_hidden_variable(ws);
    int at = 0;
    const int nroot = ro_real_roots(ws, at);
    int ns = 0;
    for (int k = 0; k < nroot; ++k) {
        double e[9];
        if (ro_solution(ws, ws[at + k], e)) store(ns++, e);
    }
    return ns;
}

// ---- scoring -------------------------------------------------------------------------------------------------------
// Is the correspondence (u1, v1, 1), (u2, v2, 1) within thr2 of the model e (sum e[a + 3 b] q1[a] q2[b] = 0) by the
// squared Sampson distance r^2 / (|(M q2)(1:2)|^2 + |(M' q1)(1:2)|^2)?  Compared as r^2 < thr2 * denominator.
__host__ __device__ __forceinline__ bool ro_inlier(const double *e, double u1, double v1, double u2, double v2, double thr2) {
    const double a0 = __builtin_fma(e[0], u2, __builtin_fma(e[3], v2, e[6]));     // M q2
    const double a1 = __builtin_fma(e[1], u2, __builtin_fma(e[4], v2, e[7]));
    const double a2 = __builtin_fma(e[2], u2, __builtin_fma(e[5], v2, e[8]));
    const double b0 = __builtin_fma(e[0], u1, __builtin_fma(e[1], v1, e[2]));     // M' q1
    const double b1 = __builtin_fma(e[3], u1, __builtin_fma(e[4], v1, e[5]));
    const double r = __builtin_fma(a0, u1, __builtin_fma(a1, v1, a2));
    const double den = __builtin_fma(a0, a0, __builtin_fma(a1, a1, __builtin_fma(b0, b0, b1 * b1)));
    return r * r < thr2 * den;
}

// ---- the two-ray intersection --------------------------------------------------------------------------------------
// The point nearest to the rays through the origin along (u1, v1, 1) and through c2 = -R' t along R' (u2, v2, 1)
// (P = [R | t], column-major 3 x 4): the middle of their common perpendicular, which is what the normal equations of
// pm_forwintersect3.m:55-68 give for two rays.  Returns whether the depths X_z and (R X + t)_z both have the sign of
// front and the rays are not parallel (RO_PARALLAX2).
__host__ __device__ inline bool ro_intersect(const double *P, double u1, double v1, double u2, double v2, int front, double *X) {
    double d1[3] = {u1, v1, 1.0}, q[3] = {u2, v2, 1.0}, d2[3], c2[3];
    const double n1 = sqrt(d1[0] * d1[0] + d1[1] * d1[1] + 1.0);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        d1[i] /= n1;
        d2[i] = P[3 * i] * q[0] + P[3 * i + 1] * q[1] + P[3 * i + 2] * q[2];
        c2[i] = -(P[3 * i] * P[9] + P[3 * i + 1] * P[10] + P[3 * i + 2] * P[11]);
    }
    const double n2 = sqrt(d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) d2[i] /= n2;
    const double cx[3] = {d1[1] * d2[2] - d1[2] * d2[1], d1[2] * d2[0] - d1[0] * d2[2], d1[0] * d2[1] - d1[1] * d2[0]};
    const double s2 = cx[0] * cx[0] + cx[1] * cx[1] + cx[2] * cx[2];
    const double c = d1[0] * d2[0] + d1[1] * d2[1] + d1[2] * d2[2];
    const double r1 = d1[0] * c2[0] + d1[1] * c2[1] + d1[2] * c2[2], r2 = d2[0] * c2[0] + d2[1] * c2[1] + d2[2] * c2[2];
    const double al1 = (r1 - c * r2) / s2, al2 = (c * r1 - r2) / s2;
#pragma unroll
    for (int i = 0; i < 3; ++i) X[i] = 0.5 * (al1 * d1[i] + c2[i] + al2 * d2[i]);
    const double z2 = P[2] * X[0] + P[5] * X[1] + P[8] * X[2] + P[11];
    const bool ok = s2 > RO_PARALLAX2 && (X[2] - X[2] == 0) && (z2 - z2 == 0);
    return ok && (front > 0 ? (X[2] > 0 && z2 > 0) : (X[2] < 0 && z2 < 0));
}

#if defined(__HIPCC__)

// Sample s: with idx, its five correspondences idx[5 s + i] of x1, x2 (2 doubles each, the third coordinate 1); without,
// the correspondences set_start[s] .. set_start[s + 1] of Q1, Q2 (3 doubles each).  E [90 s + 9 k], n_sol [s].
__global__ __launch_bounds__(RO_WG) void k_essmat5(int64_t n_sets, const int64_t *__restrict__ set_start, const double *__restrict__ Q1,
                                                   const double *__restrict__ Q2, const int64_t *__restrict__ idx,
                                                   double *__restrict__ E, int32_t *__restrict__ n_sol) {
    extern __shared__ double ro_lds[];                    // RO_WS * RO_WG doubles
    const int64_t s = (int64_t)blockIdx.x * RO_WG + threadIdx.x;
    if (s >= n_sets) return;                              // (no barrier in this kernel: a lane owns its workspace)
    const RoWs ws{ro_lds + threadIdx.x, RO_WG};
    for (int i = 0; i < 81; ++i) ws[i] = 0;
    const int64_t first = idx ? 0 : set_start[s], n = idx ? 5 : set_start[s + 1] - first;
    for (int64_t i = 0; i < n; ++i) {
        double q1[3], q2[3], w[9];
        if (idx) {
            const int64_t g = idx[5 * s + i];
            q1[0] = Q1[2 * g]; q1[1] = Q1[2 * g + 1]; q1[2] = 1.0; q2[0] = Q2[2 * g]; q2[1] = Q2[2 * g + 1]; q2[2] = 1.0;
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) { q1[k] = Q1[3 * (first + i) + k]; q2[k] = Q2[3 * (first + i) + k]; }
        }
        ro_design_row(q1, q2, w);
        ro_fold_row(ws, w);
    }
    double *out = E + 90 * s;
    n_sol[s] = ro_solve(ws, n < 9 ? (int)n : 9, [out](int k, const double *e) {
#pragma unroll
        for (int i = 0; i < 9; ++i) out[9 * k + i] = e[i];
    });
}

// The workgroup t of pair p = the last with tile_start[p] <= t scores the model slots 256 (t - tile_start[p]) + lane of
// the pair (slot = 10 local sample + solution) against all its correspondences; best[p] = max (count << 32 | ~slot).
__global__ __launch_bounds__(RO_SCORE_WG) void k_ro_score(int n_pairs, const int64_t *__restrict__ tile_start, const int64_t *__restrict__ pt_start,
                                                          const double *__restrict__ x1, const double *__restrict__ x2,
                                                          const int64_t *__restrict__ hyp_start, const double *__restrict__ E,
                                                          const int32_t *__restrict__ n_sol, const double *__restrict__ thr2,
                                                          unsigned long long *__restrict__ best) {
    __shared__ double sx[RO_SCORE_WG][4];
    __shared__ unsigned long long sk[RO_SCORE_WG / 64];
    int lo = 0, hi = n_pairs - 1;                         // uniform over the workgroup
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (tile_start[mid] <= (int64_t)blockIdx.x) lo = mid; else hi = mid - 1; }
    const int p = lo;
    const int64_t h0 = hyp_start[p], nh = hyp_start[p + 1] - h0, p0 = pt_start[p], np_ = pt_start[p + 1] - p0;
    const int64_t slot = ((int64_t)blockIdx.x - tile_start[p]) * RO_SCORE_WG + threadIdx.x;
    const int64_t smp = slot / 10;
    const int sol = (int)(slot - 10 * smp);
    const bool valid = smp < nh && sol < n_sol[h0 + (smp < nh ? smp : 0)];
    double e[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) e[i] = valid ? E[90 * (h0 + smp) + 9 * sol + i] : 0.0;
    const double t2 = thr2[p];
    uint32_t count = 0;
    for (int64_t c0 = 0; c0 < np_; c0 += RO_SCORE_WG) {
        const int64_t c = c0 + threadIdx.x;
        if (c < np_) {
            sx[threadIdx.x][0] = x1[2 * (p0 + c)]; sx[threadIdx.x][1] = x1[2 * (p0 + c) + 1];
            sx[threadIdx.x][2] = x2[2 * (p0 + c)]; sx[threadIdx.x][3] = x2[2 * (p0 + c) + 1];
        }
        __syncthreads();
        const int m = (int)(np_ - c0 < RO_SCORE_WG ? np_ - c0 : RO_SCORE_WG);
        if (valid)
            for (int j = 0; j < m; ++j) count += ro_inlier(e, sx[j][0], sx[j][1], sx[j][2], sx[j][3], t2) ? 1u : 0u;
        __syncthreads();
    }
    unsigned long long key = (valid && count > 0) ? (((unsigned long long)count << 32) | (0xFFFFFFFFull - (unsigned long long)slot)) : 0ull;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(key, off, 64); key = o > key ? o : key; }
    if ((threadIdx.x & 63) == 0) sk[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < RO_SCORE_WG / 64; ++w) key = sk[w] > key ? sk[w] : key;
        if (key) atomicMax(best + p, key);
    }
}

// Pair p: Ew [9 p] the winning E (NaN without one), win [3 p]: the inlier count, the sample, the solution (0, -1, -1)
__global__ __launch_bounds__(64) void k_ro_winner(int n_pairs, const int64_t *__restrict__ hyp_start, const double *__restrict__ E,
                                                  const unsigned long long *__restrict__ best, double *__restrict__ Ew,
                                                  int32_t *__restrict__ win) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n_pairs) return;
    const unsigned long long key = best[p];
    if (!key) {
        for (int i = 0; i < 9; ++i) Ew[9 * (int64_t)p + i] = __builtin_nan("");
        win[3 * p] = 0; win[3 * p + 1] = -1; win[3 * p + 2] = -1;
        return;
    }
    const int64_t slot = (int64_t)(0xFFFFFFFFull - (key & 0xFFFFFFFFull)), smp = slot / 10;
    const int sol = (int)(slot - 10 * smp);
    for (int i = 0; i < 9; ++i) Ew[9 * (int64_t)p + i] = E[90 * (hyp_start[p] + smp) + 9 * sol + i];
    win[3 * p] = (int32_t)(key >> 32); win[3 * p + 1] = (int32_t)smp; win[3 * p + 2] = sol;
}

// Correspondence g of pair p (the last with pt_start[p] <= g).  P4 [48 p + 12 c]: the four candidates of the pair.
// sel == nullptr: cnt [4 p + c] += in front under candidate c.  Otherwise candidate sel[p] (< 0: the pair has no
// model): X [3 g], in_front [g], inlier [g] under Ew [9 p].
__global__ __launch_bounds__(256) void k_ro_cams(int n_pairs, const int64_t *__restrict__ pt_start, const double *__restrict__ x1,
                                                 const double *__restrict__ x2, const double *__restrict__ P4,
                                                 const int32_t *__restrict__ sel, const double *__restrict__ Ew,
                                                 const double *__restrict__ thr2, int front, int32_t *__restrict__ cnt,
                                                 double *__restrict__ X, uint8_t *__restrict__ in_front, uint8_t *__restrict__ inlier) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= pt_start[n_pairs]) return;
    int lo = 0, hi = n_pairs - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (pt_start[mid] <= g) lo = mid; else hi = mid - 1; }
    const int p = lo;
    const double u1 = x1[2 * g], v1 = x1[2 * g + 1], u2 = x2[2 * g], v2 = x2[2 * g + 1];
    double Xg[3];
    if (!sel) {
        if (!(P4[48 * (int64_t)p] == P4[48 * (int64_t)p])) return;          // no model
        for (int c = 0; c < 4; ++c)
            if (ro_intersect(P4 + 48 * (int64_t)p + 12 * c, u1, v1, u2, v2, front, Xg)) atomicAdd(cnt + 4 * p + c, 1);
        return;
    }
    const int c = sel[p];
    bool fr = false, in = false;
    Xg[0] = Xg[1] = Xg[2] = __builtin_nan("");
    if (c >= 0) {
        double e[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) e[i] = Ew[9 * (int64_t)p + i];
        fr = ro_intersect(P4 + 48 * (int64_t)p + 12 * c, u1, v1, u2, v2, front, Xg);
        in = ro_inlier(e, u1, v1, u2, v2, thr2[p]);
    }
    X[3 * g] = Xg[0]; X[3 * g + 1] = Xg[1]; X[3 * g + 2] = Xg[2];
    in_front[g] = fr ? 1 : 0; inlier[g] = in ? 1 : 0;
}

#endif  // __HIPCC__

}  // namespace dbat
