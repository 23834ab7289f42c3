// Network transforms (dbat_hip_rigidalign, dbat_hip_multixform): the best similarity between two point sets
// (misc/rigidalign.m:27-61, Soderkvist and Wedin 1993) and a homogeneous transformation applied to every object point
// and every camera station (photogrammetry/pm_multixform.m:11-40).
//
//   k_align_centroid   pass 1 over the n columns of X and Y (3 x n, column-major; use[i] == 0 drops column i, whatever
//                      it holds): per workgroup the number of used columns and the sums of their x and y
//   k_align_cross      pass 2: with the centroids xm, ym of pass 1 (read from device memory: no host round trip between
//                      the passes), per workgroup C = sum (y - ym)(x - xm)' and sum |x - xm|^2.  Centred first, as
//                      rigidalign.m:36-43: products of coordinates of 1e6 m would lose every digit that matters.
//                      (rigidalign.m:54 takes tr(A'A) of an n x n matrix; the sum of squares is the same number.)
//   k_align_resid      pass 3, once the host has R, alpha: alpha R (x - xm) - (y - ym) = alpha R x + d - y per used
//                      column (NaN for the others), every residual rounded once (error-free sums and products), per
//                      workgroup the sum of their squares
//   k_align_finish     the second, small launch of every pass: one workgroup sums the workgroup partials
//   k_xform_points     A x + d per object point
//   k_xform_cams       per camera: centre A c + d, rotation M' R' (M' from cam_rotation, R = A / alpha), Euler angles
//
// Every sum is a tree of fixed shape: a thread's columns in ascending order, the wave by butterfly, the four waves of a
// workgroup in LDS, the workgroups (at most AL_MAXG, their number a function of n alone) in the finishing launch.  No
// floating-point atomics: two calls on the same input give the same bits.
//
// The host side (al_svd3, al_rotation, al_similarity) is plain C++ and needs no device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "model.hpp"

namespace dbat {

constexpr int AL_WG = 256;          // threads of a workgroup of every kernel here
constexpr int AL_MAXG = 1024;       // workgroups of a reduction pass at most: k_align_finish sums four partials per thread
constexpr int AL_PER_THREAD = 4;    // columns per thread below which the grid shrinks instead

// A (column-major), R = A / alpha (column-major) and d of T = [A d; 0 0 0 1]
struct XformPar { double A[9]; double R[9]; double d[3]; };
// alpha R (column-major; aR + aRl is the exact product of alpha and R) and the two centroids: the residual pass
struct AlignPar { double aR[9]; double aRl[9]; double xm[3]; double ym[3]; };

inline int64_t al_grid(int64_t n) {
    const int64_t g = (n + (int64_t)AL_WG * AL_PER_THREAD - 1) / ((int64_t)AL_WG * AL_PER_THREAD);
    return g < 1 ? 1 : (g > AL_MAXG ? AL_MAXG : g);
}

// ---- host: 3 x 3 singular value decomposition and the rotation of rigidalign.m:46-49 ----------------------------

// C = U diag(s) V' (all column-major) by one-sided Jacobi rotations of the columns of C (Hestenes): s descending, the
// columns of U that belong to s > 0 are unit vectors to rounding, a zero singular value leaves a zero column in U.
inline void al_svd3(const double *C, double *U, double *s, double *V) {
    double G[9], W[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int i = 0; i < 9; ++i) G[i] = C[i];
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool moved = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double a = 0, b = 0, c = 0;
                for (int i = 0; i < 3; ++i) { a += G[3 * p + i] * G[3 * p + i]; b += G[3 * q + i] * G[3 * q + i]; c += G[3 * p + i] * G[3 * q + i]; }
                // converged: the columns are orthogonal to rounding (sqrt(a) sqrt(b): a b may overflow)
                if (!(std::fabs(c) > 2.220446049250313e-16 * (std::sqrt(a) * std::sqrt(b)))) continue;
                moved = true;
                const double zeta = (b - a) / (2 * c);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1 + zeta * zeta));
                const double cs = 1 / std::sqrt(1 + t * t), sn = cs * t;
                for (int i = 0; i < 3; ++i) {
                    const double gp = G[3 * p + i], gq = G[3 * q + i];
                    G[3 * p + i] = cs * gp - sn * gq; G[3 * q + i] = sn * gp + cs * gq;
                    const double wp = W[3 * p + i], wq = W[3 * q + i];
                    W[3 * p + i] = cs * wp - sn * wq; W[3 * q + i] = sn * wp + cs * wq;
                }
            }
        if (!moved) break;
    }
    double nrm[3];
    int ord[3] = {0, 1, 2};
    for (int j = 0; j < 3; ++j) nrm[j] = std::sqrt(G[3 * j] * G[3 * j] + G[3 * j + 1] * G[3 * j + 1] + G[3 * j + 2] * G[3 * j + 2]);
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2 - i; ++j)
            if (nrm[ord[j]] < nrm[ord[j + 1]]) { const int t = ord[j]; ord[j] = ord[j + 1]; ord[j + 1] = t; }
    for (int j = 0; j < 3; ++j) {
        const int k = ord[j];
        s[j] = nrm[k];
        for (int i = 0; i < 3; ++i) { U[3 * j + i] = nrm[k] > 0 ? G[3 * k + i] / nrm[k] : 0.0; V[3 * j + i] = W[3 * k + i]; }
    }
}

inline double al_det3(const double *M) {       // column-major
    return M[0] * (M[4] * M[8] - M[7] * M[5]) - M[3] * (M[1] * M[8] - M[7] * M[2]) + M[6] * (M[1] * M[5] - M[4] * M[2]);
}

// R = P diag(1, 1, det(P Q')) Q' (rigidalign.m:49) from C = P S Q'.  The third column of P enters only through
// p3 det(P): with p3 = +-(p1 x p2) that is (p1 x p2) whatever the sign, so R = [p1, p2, p1 x p2] diag(1, 1, det Q) Q'
// -- which also holds where the third singular value is zero and p3 is not defined (three points; a planar set).
// Returns the singular values in s.
inline void al_rotation(const double *C, double *R, double *s) {
    double U[9], V[9];
    al_svd3(C, U, s, V);
    // p2 orthogonal to p1 to rounding (Gram-Schmidt: the Jacobi columns are orthogonal to about one unit already)
    const double dot = U[0] * U[3] + U[1] * U[4] + U[2] * U[5];
    double n2 = 0;
    for (int i = 0; i < 3; ++i) { U[3 + i] -= dot * U[i]; n2 += U[3 + i] * U[3 + i]; }
    n2 = std::sqrt(n2);
    for (int i = 0; i < 3; ++i) U[3 + i] = n2 > 0 ? U[3 + i] / n2 : 0.0;
    U[6] = U[1] * U[5] - U[2] * U[4]; U[7] = U[2] * U[3] - U[0] * U[5]; U[8] = U[0] * U[4] - U[1] * U[3];
    const double sg = al_det3(V) < 0 ? -1.0 : 1.0;
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) R[3 * j + i] = U[i] * V[j] + U[3 + i] * V[3 + j] + sg * U[6 + i] * V[6 + j];
}

// What is wrong with T (4 x 4, column-major) as a similarity, or nullptr; par: A, R = A / alpha, d
inline const char *al_similarity(const double *T, XformPar &par, double &alpha) {
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(T[i])) return "T is not finite";
    if (T[3] != 0 || T[7] != 0 || T[11] != 0 || T[15] != 1) return "the last row of T is not [0 0 0 1]";
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) par.A[3 * j + i] = T[4 * j + i];
    for (int i = 0; i < 3; ++i) par.d[i] = T[12 + i];
    const double det = al_det3(par.A);
    if (!(det > 0)) return "T(1:3,1:3) is not a scaled proper rotation: its determinant is not positive";
    alpha = std::cbrt(det);
    for (int i = 0; i < 9; ++i) par.R[i] = par.A[i] / alpha;
    double worst = 0;
    for (int i = 0; i < 3; ++i) {                    // || R'R - I ||_inf: the largest row sum
        double row = 0;
        for (int j = 0; j < 3; ++j)
            row += std::fabs(par.R[3 * i] * par.R[3 * j] + par.R[3 * i + 1] * par.R[3 * j + 1] + par.R[3 * i + 2] * par.R[3 * j + 2] - (i == j ? 1.0 : 0.0));
        worst = row > worst ? row : worst;
    }
    if (!(worst <= 1e-9)) return "T(1:3,1:3) is not a scale times a proper rotation (|| A'A / alpha^2 - I ||_inf > 1e-9)";
    return nullptr;
}

#if defined(__HIPCC__)

// v[k] <- the sum over the workgroup, valid in thread 0: butterfly in the wave, the four waves in LDS
template <int K>
__device__ __forceinline__ void al_block_sum(double (&v)[K], double (*s)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) s[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = (s[0][k] + s[1][k]) + (s[2][k] + s[3][k]);
}

// part[7 * workgroup + .]: used columns, sum of x (3), sum of y (3)
__global__ __launch_bounds__(AL_WG) void k_align_centroid(int64_t n, const double *__restrict__ X, const double *__restrict__ Y,
                                                          const uint8_t *__restrict__ use, double *__restrict__ part) {
    __shared__ double s[4][7];
    double v[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int64_t i = (int64_t)blockIdx.x * AL_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * AL_WG) {
        if (use && !use[i]) continue;
        v[0] += 1.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) { v[1 + k] += X[3 * i + k]; v[4 + k] += Y[3 * i + k]; }
    }
    al_block_sum<7>(v, s);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < 7; ++k) part[7 * (int64_t)blockIdx.x + k] = v[k];
}

// cen: what k_align_finish<7, true> left -- the count, xm, ym.  part[10 * workgroup + .]: C (column-major: C[3 j + i] =
// sum (y - ym)_i (x - xm)_j), sum |x - xm|^2
__global__ __launch_bounds__(AL_WG) void k_align_cross(int64_t n, const double *__restrict__ X, const double *__restrict__ Y,
                                                       const uint8_t *__restrict__ use, const double *__restrict__ cen,
                                                       double *__restrict__ part) {
    __shared__ double s[4][10];
    double v[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const double xm[3] = {cen[1], cen[2], cen[3]}, ym[3] = {cen[4], cen[5], cen[6]};
    for (int64_t i = (int64_t)blockIdx.x * AL_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * AL_WG) {
        if (use && !use[i]) continue;
        double a[3], b[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { a[k] = X[3 * i + k] - xm[k]; b[k] = Y[3 * i + k] - ym[k]; }
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int k = 0; k < 3; ++k) v[3 * j + k] = __builtin_fma(b[k], a[j], v[3 * j + k]);
        v[9] = __builtin_fma(a[0], a[0], __builtin_fma(a[1], a[1], __builtin_fma(a[2], a[2], v[9])));
    }
    al_block_sum<10>(v, s);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < 10; ++k) part[10 * (int64_t)blockIdx.x + k] = v[k];
}

// s + e = a + b exactly (Knuth); a * b = p + e exactly (one FMA)
__device__ __forceinline__ double al_two_sum(double a, double b, double &e) {
    const double s = a + b, bb = s - a;
    e = (a - (s - bb)) + (b - bb);
    return s;
}

// resid (null: not wanted) [3 n]: alpha R (x - xm) - (y - ym), NaN for a column that is not used; part[workgroup]: the
// sum of squares.  A residual of a millimetre is the difference of terms of the size of the network, and the rms is
// wanted to a few units of ITS last place: alpha R (two words), the centred coordinates, the three products and their
// sum are carried exactly (error-free sums and FMA products, the errors collected in a second word), so that a
// residual is rounded once.  The pass is bound by its loads; the extra arithmetic is not seen.
__global__ __launch_bounds__(AL_WG) void k_align_resid(int64_t n, const double *__restrict__ X, const double *__restrict__ Y,
                                                       const uint8_t *__restrict__ use, AlignPar p, double *__restrict__ resid,
                                                       double *__restrict__ part) {
    __shared__ double s[4][1];
    double v[1] = {0};
    for (int64_t i = (int64_t)blockIdx.x * AL_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * AL_WG) {
        if (use && !use[i]) {
            if (resid) { resid[3 * i] = __builtin_nan(""); resid[3 * i + 1] = __builtin_nan(""); resid[3 * i + 2] = __builtin_nan(""); }
            continue;
        }
        double ah[3], al[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) ah[j] = al_two_sum(X[3 * i + j], -p.xm[j], al[j]);
        double r[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double bl, e;
            const double bh = al_two_sum(Y[3 * i + k], -p.ym[k], bl);
            double hi = -bh, lo = -bl;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double m = p.aR[3 * j + k], ph = m * ah[j];
                lo += __builtin_fma(m, ah[j], -ph) + (m * al[j] + p.aRl[3 * j + k] * ah[j]);
                hi = al_two_sum(hi, ph, e);
                lo += e;
            }
            r[k] = hi + lo;
        }
        v[0] = __builtin_fma(r[0], r[0], __builtin_fma(r[1], r[1], __builtin_fma(r[2], r[2], v[0])));
        if (resid) { resid[3 * i] = r[0]; resid[3 * i + 1] = r[1]; resid[3 * i + 2] = r[2]; }
    }
    al_block_sum<1>(v, s);
    if (threadIdx.x == 0) part[blockIdx.x] = v[0];
}

// One workgroup: out[k] = the sum over the G <= AL_MAXG workgroups of part[K g + k], every thread its partials in
// ascending order.  MEANS (K = 7): out[1 .. 6] divided by out[0], the centroids.
template <int K, bool MEANS>
__global__ __launch_bounds__(AL_WG) void k_align_finish(int G, const double *__restrict__ part, double *__restrict__ out) {
    __shared__ double s[4][K];
    double v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = 0;
    for (int g = threadIdx.x; g < G; g += AL_WG)
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] += part[K * (int64_t)g + k];
    al_block_sum<K>(v, s);
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = (MEANS && k > 0) ? v[k] / v[0] : v[k];
}

__global__ __launch_bounds__(AL_WG) void k_xform_points(int64_t n, double *__restrict__ OP, XformPar p) {
    const int64_t i = (int64_t)blockIdx.x * AL_WG + threadIdx.x;
    if (i >= n) return;
    // a NaN coordinate makes the whole column NaN, as euclidean(T * homogeneous(OP)) does (0 * NaN = NaN)
    const double x = OP[3 * i], y = OP[3 * i + 1], z = OP[3 * i + 2];
#pragma unroll
    for (int k = 0; k < 3; ++k) OP[3 * i + k] = __builtin_fma(p.A[k], x, __builtin_fma(p.A[3 + k], y, __builtin_fma(p.A[6 + k], z, p.d[k])));
}

// Camera i: rows 0 .. 5 of column i of EO (eo_rows >= 6 rows per column; the others are not touched).  A row that is
// not finite: the column stays as it is and fail[i] = 1 (pm_multixform.m:27-34).  The camera matrix M' [I, -c] times
// inv(T) is M' R' / alpha [I, -(A c + d)]: the centre is A c + d, and the rotation -- with the scale divided out, which
// pm_multixform.m:37 does not do -- N = M' R'.  Angles (derotmat3d.m:17-19: omega = atan2(-N32, N33), phi = asin(N31),
// kappa = atan2(-N21, N11)) in a form that equals them for a rotation matrix and keeps its accuracy towards
// |phi| = pi/2, where N32, N33, N21, N11 all vanish: phi = atan2(N31, hypot(N32, N33)), and kappa from the second row
// of R1(omega)' N' = R2(phi) R3(kappa), [sin kappa, cos kappa, 0], with the omega just found.
__global__ __launch_bounds__(AL_WG) void k_xform_cams(int64_t n, int eo_rows, double *__restrict__ EO, XformPar p,
                                                      uint8_t *__restrict__ fail) {
    const int64_t i = (int64_t)blockIdx.x * AL_WG + threadIdx.x;
    if (i >= n) return;
    double *e = EO + (int64_t)eo_rows * i;
    double c[3], ang[3];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) { c[k] = e[k]; ang[k] = e[3 + k]; ok = ok && (c[k] - c[k] == 0) && (ang[k] - ang[k] == 0); }
    if (fail) fail[i] = ok ? 0 : 1;
    if (!ok) return;
    double Mt[9], sk, ck, N[9];
    cam_rotation(ang, Mt, sk, ck);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int j = 0; j < 3; ++j)          // N(r, j) = sum_k M'(r, k) R(j, k)
            N[3 * r + j] = __builtin_fma(Mt[3 * r], p.R[j], __builtin_fma(Mt[3 * r + 1], p.R[3 + j], Mt[3 * r + 2] * p.R[6 + j]));
    const double om = atan2(-N[7], N[8]);
    const double ph = atan2(N[6], hypot(N[7], N[8]));
    const double so = sin(om), co = cos(om);
    const double ka = atan2(co * N[1] + so * N[2], co * N[4] + so * N[5]);
#pragma unroll
    for (int k = 0; k < 3; ++k) e[k] = __builtin_fma(p.A[k], c[0], __builtin_fma(p.A[3 + k], c[1], __builtin_fma(p.A[6 + k], c[2], p.d[k])));
    e[3] = om; e[4] = ph; e[5] = ka;
}

#endif  // __HIPCC__

}  // namespace dbat
