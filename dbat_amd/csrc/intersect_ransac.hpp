// Robust forward intersection (dbat_hip_intersect_ransac, host side: intersect_host.hpp): a RANSAC over pairs of image
// rays, scored by inlier count, for many object points in one launch.  One wave of 64 lanes per point, four points per
// workgroup of 256 lanes.  A lane takes one sample -- two rays of the point -- and intersects them: the middle of their
// common perpendicular, what pm_forwintersect3.m:55-68 gives for two rays (ro_intersect of relorient.hpp has the formula
// for the pair [I | 0], [R | t]).  It keeps the point in registers and scores it against every ray of the object point.
// More than 64 samples run in rounds of 64.  A point that brings no samples has all its pairs i < j enumerated here, in
// lexicographic order: sample k = i (2 r - i - 1) / 2 + (j - i - 1) of r rays.  The reference has no counterpart.
//
// Scoring: a ray counts for a hypothesis if it may be used, the point lies in front of its camera (the third row of
// P [X; 1] is negative: the cameras look along -z) and e0^2 + e1^2 <= thr2 of its camera, the residual evaluated by
// rr_resid2 (resect_ransac.hpp) as the resection scores.  In the scoring loop the ray and its camera matrix are the same
// for every lane of the wave: they come from global memory by wave-uniform loads, there is no LDS tile and no barrier.
// Counts are integers, and the winner is one integer maximum over the packed key ir_key: the larger count, then the lower
// sample.  No floating-point value decides anything but the comparisons with thr2 and the parallax cut, and there are no
// atomics: two calls give the same bits, and a point gives the same bits alone and in a batch.
//
// Every loop is bounded: rounds by the point's samples, the scoring and the decoding of a pair by its rays.
#pragma once
#include "resect_ransac.hpp"

namespace dbat {

constexpr int IR_WG = 256;                  // lanes of a workgroup
constexpr int IR_WAVE = 64;                 // lanes of a point, and samples of a round
constexpr int IR_POINTS = IR_WG / IR_WAVE;  // points of a workgroup
constexpr int IR_MAX_EXHAUSTIVE = 64;       // rays up to which a point's pairs are enumerated here (2016 pairs)
constexpr int IR_MIN_INLIERS = 2;           // what every sample gets from itself
constexpr double IR_PARALLAX2 = 1e-24;      // |d1 x d2|^2 of unit directions below which two rays are parallel
// count (< 2^29) above the complement of the sample (< 2^31): the maximum is the larger count, then the lower sample.
// 0: nothing.
constexpr int IR_KEY_SHIFT = 32;
__host__ __device__ constexpr unsigned long long ir_key(long long count, long long sample) {
    return ((unsigned long long)count << IR_KEY_SHIFT) | (((1ULL << IR_KEY_SHIFT) - 1ULL) - (unsigned long long)sample);
}

#if defined(__HIPCC__)

// The projection centre -R' t and the unit direction R' (x0, x1, 1) of a ray under P (column-major 3 x 4).
__device__ __forceinline__ void ir_ray(const double *P, double x0, double x1, double *c, double *d) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        c[i] = -(P[3 * i] * P[9] + P[3 * i + 1] * P[10] + P[3 * i + 2] * P[11]);
        d[i] = P[3 * i] * x0 + P[3 * i + 1] * x1 + P[3 * i + 2];
    }
    rs_unit(d);
}

// The middle of the common perpendicular of the rays (c1, d1), (c2, d2), d unit; s2 = |d1 x d2|^2.
__device__ __forceinline__ void ir_midpoint(const double *c1, const double *d1, const double *c2, const double *d2, double *X, double &s2) {
    const double cx[3] = {d1[1] * d2[2] - d1[2] * d2[1], d1[2] * d2[0] - d1[0] * d2[2], d1[0] * d2[1] - d1[1] * d2[0]};
    s2 = cx[0] * cx[0] + cx[1] * cx[1] + cx[2] * cx[2];
    const double b[3] = {c2[0] - c1[0], c2[1] - c1[1], c2[2] - c1[2]};
    const double c = d1[0] * d2[0] + d1[1] * d2[1] + d1[2] * d2[2];
    const double r1 = d1[0] * b[0] + d1[1] * b[1] + d1[2] * b[2], r2 = d2[0] * b[0] + d2[1] * b[1] + d2[2] * b[2];
    const double al1 = (r1 - c * r2) / s2, al2 = (c * r1 - r2) / s2;
#pragma unroll
    for (int i = 0; i < 3; ++i) X[i] = c1[i] + 0.5 * ((al1 * d1[i] + b[i]) + al2 * d2[i]);
}

// Wave w of workgroup b handles point p = 4 b + w: rays ray_start[p] .. ray_start[p + 1] of cam, xn (2 doubles), use (may
// be null: all), samples smp_start[p] .. smp_start[p + 1] of smp (two indices local to the point's rays; smp_start may
// be null, and a point without samples has its pairs enumerated).  P [12 cam], thr2 [cam], par2 = max(sin^2 min_angle,
// IR_PARALLAX2).  X [3 p], stats [4 p] (count, sample, hypotheses scored, usable rays), inlier [g], ssq [p].
__global__ __launch_bounds__(IR_WG) void k_intersect_ransac(int n_points, const int64_t *__restrict__ ray_start,
                                                            const int32_t *__restrict__ cam, const double *__restrict__ xn,
                                                            const double *__restrict__ P, const uint8_t *__restrict__ use,
                                                            const int64_t *__restrict__ smp_start, const int32_t *__restrict__ smp,
                                                            const double *__restrict__ thr2, double par2, double *__restrict__ X,
                                                            int32_t *__restrict__ stats, uint8_t *__restrict__ inlier,
                                                            double *__restrict__ ssq) {
    const int lane = threadIdx.x & (IR_WAVE - 1);
    const int p = __builtin_amdgcn_readfirstlane((int)blockIdx.x * IR_POINTS + (int)(threadIdx.x >> 6));      // the wave's
    if (p >= n_points) return;
    const int64_t g0 = ray_start[p];
    const int nr = (int)(ray_start[p + 1] - g0);
    const int64_t h0 = smp_start ? smp_start[p] : 0;
    const int64_t nlist = smp_start ? smp_start[p + 1] - h0 : 0;
    const bool listed = nlist > 0;
    const int64_t ns = listed ? nlist : (nr <= IR_MAX_EXHAUSTIVE ? (int64_t)nr * (nr - 1) / 2 : 0);
    unsigned long long best = 0ULL;          // the lane's best key over its rounds, and that point
    double bX[3] = {0.0, 0.0, 0.0};
    int scored = 0;
    for (int64_t k0 = 0; k0 < ns; k0 += IR_WAVE) {          // uniform
        const int64_t k = k0 + lane;
        bool valid = false;
        double Xh[3] = {0.0, 0.0, 0.0};
        if (k < ns) {
            int i, j;
            if (listed) { i = smp[2 * (h0 + k)]; j = smp[2 * (h0 + k) + 1]; }
            else {                                          // row i of the pairs holds nr - 1 - i of them
                int rest = (int)k;
                i = 0;
                while (i < nr - 2 && rest >= nr - 1 - i) { rest -= nr - 1 - i; ++i; }
                j = i + 1 + rest;
            }
            const int64_t a = g0 + i, b = g0 + j;
            if (!use || (use[a] && use[b])) {
                double Pa[12], Pb[12], c1[3], d1[3], c2[3], d2[3], s2;
                const double *pa = P + 12 * (int64_t)cam[a], *pb = P + 12 * (int64_t)cam[b];
#pragma unroll
                for (int q = 0; q < 12; ++q) { Pa[q] = pa[q]; Pb[q] = pb[q]; }
                ir_ray(Pa, xn[2 * a], xn[2 * a + 1], c1, d1);
                ir_ray(Pb, xn[2 * b], xn[2 * b + 1], c2, d2);
                ir_midpoint(c1, d1, c2, d2, Xh, s2);
                valid = s2 >= par2 && (Xh[0] - Xh[0] == 0.0) && (Xh[1] - Xh[1] == 0.0) && (Xh[2] - Xh[2] == 0.0);
            }
        }
        scored += valid ? 1 : 0;
        int cnt = 0;
        if (valid)
            for (int q = 0; q < nr; ++q) {                  // the ray and its camera: the same in every lane
                const int64_t g = g0 + q;
                if (use && !use[g]) continue;
                const int c = cam[g];
                const double *Pq = P + 12 * (int64_t)c;
                bool fr;
                const double e = rr_resid2(Pq, Xh, xn[2 * g], xn[2 * g + 1], fr);
                cnt += (fr && e <= thr2[c]) ? 1 : 0;
            }
        if (valid && cnt >= IR_MIN_INLIERS) {
            const unsigned long long key = ir_key(cnt, k);
            if (key > best) { best = key; bX[0] = Xh[0]; bX[1] = Xh[1]; bX[2] = Xh[2]; }
        }
    }
    // ---- the winner: the maximum key of the wave, in every lane ----------------------------------------------------------
    unsigned long long win = best;
    int total_scored = scored;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(win, off, IR_WAVE);
        win = o > win ? o : win;
        total_scored += __shfl_xor(total_scored, off, IR_WAVE);
    }
    const bool won = win != 0ULL;
    const unsigned long long owner = __ballot(won && best == win);         // keys are unique: one lane
    const int src = won ? __ffsll((unsigned long long)owner) - 1 : 0;
    double Xw[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) Xw[i] = __shfl(bX[i], src, IR_WAVE);
    // ---- the inliers of the winner, the sum of their squared residuals, the usable rays ----------------------------------
    double acc = 0.0;
    int usable = 0;
    for (int q = lane; q < nr; q += IR_WAVE) {
        const int64_t g = g0 + q;
        const bool u = !use || use[g];
        bool in = false;
        if (won && u) {
            const int c = cam[g];
            bool fr;
            const double e = rr_resid2(P + 12 * (int64_t)c, Xw, xn[2 * g], xn[2 * g + 1], fr);
            in = fr && e <= thr2[c];
            if (in) acc += e;
        }
        usable += u ? 1 : 0;
        inlier[g] = in ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { acc += __shfl_xor(acc, off, IR_WAVE); usable += __shfl_xor(usable, off, IR_WAVE); }
    if (lane == 0) {
        const double nan = __builtin_nan("");
        const unsigned long long low = ((1ULL << IR_KEY_SHIFT) - 1ULL) - (win & ((1ULL << IR_KEY_SHIFT) - 1ULL));
#pragma unroll
        for (int i = 0; i < 3; ++i) X[3 * (int64_t)p + i] = won ? Xw[i] : nan;
        stats[4 * (int64_t)p] = won ? (int32_t)(win >> IR_KEY_SHIFT) : 0;
        stats[4 * (int64_t)p + 1] = won ? (int32_t)low : -1;
        stats[4 * (int64_t)p + 2] = total_scored;
        stats[4 * (int64_t)p + 3] = usable;
        ssq[p] = acc;
    }
}

#endif  // __HIPCC__

}  // namespace dbat
