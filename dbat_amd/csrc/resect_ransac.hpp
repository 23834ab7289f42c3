// Robust spatial resection (dbat_hip_resect_ransac, host side: poseadjust_host.hpp): a RANSAC over triples of control
// points, scored by inlier count, for many cameras in one launch.  One workgroup of 256 lanes per camera.  A lane solves
// one sample with rs_poses_3pt (resect.hpp: Grunert's quartic, up to four poses), keeps the poses in registers and scores
// them against every point of the camera; the points pass through LDS in tiles of RR_TILE.  More than 256 samples run in
// rounds of 256.  The reference has no counterpart: resect.m tries the largest triangles and keeps the smallest rms.
//
// Scoring: a point counts for a pose if it may be used, lies in front (the third row of P [X; 1] is negative: the
// cameras look along -z) and e0^2 + e1^2 <= thr2, the residuals evaluated with rs_dot2 / rs_resid as k_resect does.
// Counts are integers, and the winner is one integer maximum over the packed key rr_key: the larger count, then the
// lower sample, then the lower root.  No floating-point value decides anything but the residual's comparison with thr2,
// and there are no atomics: two calls give the same bits, and a camera gives the same bits alone and in a batch.
//
// Every loop is bounded: rounds by the camera's samples, tiles by its points, rs_roots by its 200 iterations.  Every
// barrier sits in control flow that is uniform over the workgroup (the trip counts come from pt_start and smp_start).
#pragma once
#include "resect.hpp"

namespace dbat {

constexpr int RR_WG = 256;                  // lanes of a workgroup, and samples of a round
constexpr int RR_TILE = 256;                // points of an LDS tile
constexpr int RR_MIN_INLIERS = 4;           // three is what every sample gets from itself
// count (< 2^29) above the complement of 4 sample + root (< 2^33): the maximum is the larger count, then the lower
// sample, then the lower root.  0: nothing.
constexpr int RR_KEY_SHIFT = 34;
__host__ __device__ constexpr unsigned long long rr_key(long long count, long long sample, int root) {
    return ((unsigned long long)count << RR_KEY_SHIFT) | (((1ULL << RR_KEY_SHIFT) - 1ULL) - (unsigned long long)(4 * sample + root));
}

#if defined(__HIPCC__)

// The squared residual of the point Q, xn under the pose P (column-major 3 x 4) and whether the point is in front.
__device__ __forceinline__ double rr_resid2(const double *P, const double *Q, double x0, double x1, bool &front) {
    double h0, h0l, h1, h1l, h2, h2l;
    rs_dot2(P[0], P[3], P[6], P[9], Q, h0, h0l);
    rs_dot2(P[1], P[4], P[7], P[10], Q, h1, h1l);
    rs_dot2(P[2], P[5], P[8], P[11], Q, h2, h2l);
    const double e0 = rs_resid(h0, h0l, h2, h2l, x0), e1 = rs_resid(h1, h1l, h2, h2l, x1);
    front = h2 < 0.0;
    return e0 * e0 + e1 * e1;
}

struct RrState {
    double X[3 * RR_TILE], x[2 * RR_TILE];  // a tile of points
    uint8_t u[RR_TILE];                     // and whether each may be used
    unsigned long long key[RR_WG / 64];     // wave partials
    long long scored[RR_WG / 64];
    double ssq[RR_WG / 64];
    double P[12];                           // the winner
};

// Workgroup c handles camera c: points pt_start[c] .. pt_start[c + 1] of X (3 doubles), xn (2), use (may be null: all),
// samples smp_start[c] .. smp_start[c + 1] of smp (three indices local to the camera's range).  Pout [12 c],
// stats [4 c] (count, sample, root, poses scored), inlier [g], ssq [c].
__global__ __launch_bounds__(RR_WG) void k_resect_ransac(const int64_t *__restrict__ pt_start, const double *__restrict__ X,
                                                         const double *__restrict__ xn, const uint8_t *__restrict__ use,
                                                         const int64_t *__restrict__ smp_start, const int32_t *__restrict__ smp,
                                                         const double *__restrict__ thr2, double *__restrict__ Pout,
                                                         int32_t *__restrict__ stats, uint8_t *__restrict__ inlier,
                                                         double *__restrict__ ssq) {
    __shared__ RrState s;
    const int c = blockIdx.x, tid = threadIdx.x;
    const int64_t g0 = pt_start[c], npt = pt_start[c + 1] - g0;
    const int64_t h0 = smp_start[c], ns = smp_start[c + 1] - h0;
    const double t2 = thr2[c];
    unsigned long long best = 0ULL;          // the lane's best key over its rounds, and that pose
    double bestP[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) bestP[i] = 0.0;
    long long scored = 0;
    for (int64_t r0 = 0; r0 < ns; r0 += RR_WG) {           // uniform
        const int64_t smpl = r0 + tid;
        double P0[12], P1[12], P2[12], P3[12];
        int np_ = 0;
        bool v0 = false, v1 = false, v2 = false, v3 = false;
        if (smpl < ns) {
            const int32_t *tri = smp + 3 * (h0 + smpl);
            bool ok = true;
            double Xt[3][3], d[3][3], PP[4][12];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int64_t q = g0 + tri[i];
                ok = ok && (!use || use[q]);
#pragma unroll
                for (int r = 0; r < 3; ++r) Xt[i][r] = X[3 * q + r];
                d[i][0] = xn[2 * q]; d[i][1] = xn[2 * q + 1]; d[i][2] = 1.0;
                rs_unit(d[i]);
            }
            if (ok) np_ = rs_poses_3pt(Xt, d, true, PP);
            // into registers, with whether every entry is finite: a pose of collinear points is not scored
            bool f0 = true, f1 = true, f2 = true, f3 = true;
#pragma unroll
            for (int i = 0; i < 12; ++i) {
                P0[i] = np_ > 0 ? PP[0][i] : 0.0; f0 = f0 && (P0[i] - P0[i] == 0.0);
                P1[i] = np_ > 1 ? PP[1][i] : 0.0; f1 = f1 && (P1[i] - P1[i] == 0.0);
                P2[i] = np_ > 2 ? PP[2][i] : 0.0; f2 = f2 && (P2[i] - P2[i] == 0.0);
                P3[i] = np_ > 3 ? PP[3][i] : 0.0; f3 = f3 && (P3[i] - P3[i] == 0.0);
            }
            v0 = np_ > 0 && f0; v1 = np_ > 1 && f1; v2 = np_ > 2 && f2; v3 = np_ > 3 && f3;
            scored += (v0 ? 1 : 0) + (v1 ? 1 : 0) + (v2 ? 1 : 0) + (v3 ? 1 : 0);
        }
        int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
        for (int64_t b0 = 0; b0 < npt; b0 += RR_TILE) {      // uniform
            __syncthreads();
            const int64_t i = b0 + tid;
            if (i < npt) {
                const int64_t g = g0 + i;
                s.X[3 * tid] = X[3 * g]; s.X[3 * tid + 1] = X[3 * g + 1]; s.X[3 * tid + 2] = X[3 * g + 2];
                s.x[2 * tid] = xn[2 * g]; s.x[2 * tid + 1] = xn[2 * g + 1];
                s.u[tid] = (!use || use[g]) ? 1 : 0;
            }
            __syncthreads();
            const int m = (int)(npt - b0 < RR_TILE ? npt - b0 : RR_TILE);
            if (v0 || v1 || v2 || v3)
                for (int k = 0; k < m; ++k) {
                    if (!s.u[k]) continue;
                    const double Q[3] = {s.X[3 * k], s.X[3 * k + 1], s.X[3 * k + 2]};
                    const double x0 = s.x[2 * k], x1 = s.x[2 * k + 1];
                    bool fr;
                    double e;
                    if (v0) { e = rr_resid2(P0, Q, x0, x1, fr); c0 += (fr && e <= t2) ? 1 : 0; }
                    if (v1) { e = rr_resid2(P1, Q, x0, x1, fr); c1 += (fr && e <= t2) ? 1 : 0; }
                    if (v2) { e = rr_resid2(P2, Q, x0, x1, fr); c2 += (fr && e <= t2) ? 1 : 0; }
                    if (v3) { e = rr_resid2(P3, Q, x0, x1, fr); c3 += (fr && e <= t2) ? 1 : 0; }
                }
        }
        // the lane's best so far: ascending roots, a later one only if its key is larger
        if (v0 && c0 >= RR_MIN_INLIERS) { const unsigned long long k = rr_key(c0, smpl, 0); if (k > best) { best = k;
#pragma unroll
            for (int i = 0; i < 12; ++i) bestP[i] = P0[i]; } }
        if (v1 && c1 >= RR_MIN_INLIERS) { const unsigned long long k = rr_key(c1, smpl, 1); if (k > best) { best = k;
#pragma unroll
            for (int i = 0; i < 12; ++i) bestP[i] = P1[i]; } }
        if (v2 && c2 >= RR_MIN_INLIERS) { const unsigned long long k = rr_key(c2, smpl, 2); if (k > best) { best = k;
#pragma unroll
            for (int i = 0; i < 12; ++i) bestP[i] = P2[i]; } }
        if (v3 && c3 >= RR_MIN_INLIERS) { const unsigned long long k = rr_key(c3, smpl, 3); if (k > best) { best = k;
#pragma unroll
            for (int i = 0; i < 12; ++i) bestP[i] = P3[i]; } }
    }
    // ---- the winner: the maximum key of the workgroup -----------------------------------------------------------------
    unsigned long long wk = best;
    long long ws = scored;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(wk, off, 64);
        wk = o > wk ? o : wk;
        ws += __shfl_down(ws, off, 64);
    }
    __syncthreads();
    if ((tid & 63) == 0) { s.key[tid >> 6] = wk; s.scored[tid >> 6] = ws; }
    __syncthreads();
    unsigned long long win = s.key[0];
#pragma unroll
    for (int wv = 1; wv < RR_WG / 64; ++wv) win = s.key[wv] > win ? s.key[wv] : win;
    const long long total_scored = ((s.scored[0] + s.scored[1]) + s.scored[2]) + s.scored[3];
    if (win != 0ULL && best == win)                       // keys are unique: one lane
#pragma unroll
        for (int i = 0; i < 12; ++i) s.P[i] = bestP[i];
    __syncthreads();
    // ---- the inliers of the winner and the sum of their squared residuals ---------------------------------------------
    double P[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) P[i] = win != 0ULL ? s.P[i] : 0.0;
    double acc = 0.0;
    for (int64_t i = tid; i < npt; i += RR_WG) {
        const int64_t g = g0 + i;
        bool in = false;
        if (win != 0ULL && (!use || use[g])) {
            const double Q[3] = {X[3 * g], X[3 * g + 1], X[3 * g + 2]};
            bool fr;
            const double e = rr_resid2(P, Q, xn[2 * g], xn[2 * g + 1], fr);
            in = fr && e <= t2;
            if (in) acc += e;
        }
        inlier[g] = in ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((tid & 63) == 0) s.ssq[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        const double nan = __builtin_nan("");
        const unsigned long long low = ((1ULL << RR_KEY_SHIFT) - 1ULL) - (win & ((1ULL << RR_KEY_SHIFT) - 1ULL));
#pragma unroll
        for (int i = 0; i < 12; ++i) Pout[12 * (int64_t)c + i] = win != 0ULL ? P[i] : nan;
        stats[4 * (int64_t)c] = win != 0ULL ? (int32_t)(win >> RR_KEY_SHIFT) : 0;
        stats[4 * (int64_t)c + 1] = win != 0ULL ? (int32_t)(low >> 2) : -1;
        stats[4 * (int64_t)c + 2] = win != 0ULL ? (int32_t)(low & 3ULL) : -1;
        stats[4 * (int64_t)c + 3] = (int32_t)total_scored;
        ssq[c] = ((s.ssq[0] + s.ssq[1]) + s.ssq[2]) + s.ssq[3];
    }
}

#endif  // __HIPCC__

}  // namespace dbat
