// Point depths and the chirality veto (dbat_hip_point_depths, dbat_hip_set_chirality): the depth of every object point
// with respect to every camera that sees it, d_k = -M'_(3,:) (Q_pt(k) - q0_cam(k)) for IP column k -- M' the
// world-to-camera rotation of the camera record (model.hpp: cam_rotation), q0 its centre.  The camera looks along its
// negative z axis (obs_eval: lhs = -f X / X_3), so a point in front has d > 0.  This is -ptdepth(P, X) of
// photogrammetry/pm_multidepth.m:19-37 with P = K M' [I, -q0]: det(K M') = f^2 > 0 and the third row of K M' is the
// third row of M', of norm 1.
//
//   k_depth_cm      one workgroup per chunk of the camera-major copy (one image per chunk: the third row of M' and the
//                   centre are wave-uniform and come from the camera record once per workgroup; point indices coalesced).
//                   Per observation the depth; per workgroup the number of observations with !(d > thr) -- a NaN depth
//                   counts as behind --, the smallest depth and the smallest IP column that attains it.  Across
//                   workgroups integer atomics only: atomicAdd of the count, atomicMin of the order-preserving key of
//                   the smallest depth (depth_key), per image and over all.  FULL: the depths scattered to IP-column
//                   order, the minima per image and the (key, column) of every chunk for the argmin.
//   k_depth_finish  one workgroup: the smallest column among the chunks whose key equals the overall minimum, and the
//                   three results -- count, smallest depth, its column -- to the host's mailbox.
// No floating-point atomics and no sums of floating-point values: every call gives the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "model.hpp"
#include "step_layout.hpp"

namespace dbat {

constexpr unsigned long long DEPTH_KEY_NONE = ~0ull;    // no depth (or only NaN): above the key of every number

// d = -M'_(3,:) (Q - q0); -0 is returned as +0 (one key per value)
DBAT_HD double cam_depth(const double m[3], const double c[3], double q0, double q1, double q2) {
    const double d0 = q0 - c[0], d1 = q1 - c[1], d2 = q2 - c[2];
    return 0.0 - __builtin_fma(m[0], d0, __builtin_fma(m[1], d1, m[2] * d2));
}

// unsigned keys that order like the doubles they come from (negative: all bits flipped, others: the sign bit set -- the
// usual radix-sort key; robust.hpp orders the bit patterns of non-negative values directly); NaN: DEPTH_KEY_NONE
DBAT_HD unsigned long long depth_key(double d) {
    if (d != d) return DEPTH_KEY_NONE;
    union { double f; unsigned long long u; } v;
    v.f = d;
    return (v.u >> 63) ? ~v.u : v.u | (1ull << 63);
}
DBAT_HD double depth_from_key(unsigned long long k) {
    if (k == DEPTH_KEY_NONE) return __builtin_nan("");
    union { double f; unsigned long long u; } v;
    v.u = (k >> 63) ? k & ~(1ull << 63) : ~k;
    return v.f;
}

#if defined(__HIPCC__)

constexpr long long DEPTH_NO_COL = 0x7fffffffffffffffll;

// (key, col) <- the smaller key; equal keys: the smaller column
__device__ __forceinline__ void depth_take(unsigned long long &key, long long &col, unsigned long long k2, long long c2) {
    const bool t = k2 < key || (k2 == key && c2 < col);
    key = t ? k2 : key; col = t ? c2 : col;
}

// red[0]: observations with !(d > thr) (zero on entry), red[1]: smallest key (DEPTH_KEY_NONE on entry).  FULL:
// img_min[image] likewise, chunk_key / chunk_col[chunk] the smallest key of the chunk and the smallest IP column with
// it, depth_out (null: not wanted) in IP-column order through cm_col, the IP column of every camera-major slot.
template <bool FULL>
__global__ __launch_bounds__(256) void k_depth_cm(const double *__restrict__ z, int64_t NS, const CamRec *__restrict__ cams,
                                                  const int32_t *__restrict__ cm_pt, const int32_t *__restrict__ chunk_cam,
                                                  const int64_t *__restrict__ chunk_start, const int64_t *__restrict__ cm_col, double thr,
                                                  double *__restrict__ depth_out, unsigned long long *__restrict__ red,
                                                  unsigned long long *__restrict__ img_min, unsigned long long *__restrict__ chunk_key,
                                                  long long *__restrict__ chunk_col) {
    __shared__ unsigned long long s_key[4];
    __shared__ long long s_col[4];
    __shared__ unsigned s_cnt[4];
    const int cam = chunk_cam[blockIdx.x];
    const CamRec &C = cams[cam];
    const double m[3] = {C.Mt[6], C.Mt[7], C.Mt[8]}, c[3] = {C.c[0], C.c[1], C.c[2]};
    const int64_t q0 = chunk_start[blockIdx.x], q1 = chunk_start[blockIdx.x + 1];
    unsigned cnt = 0;
    unsigned long long key = DEPTH_KEY_NONE;
    long long col = DEPTH_NO_COL;
    // a chunk holds at most 2048 observations, eight per thread; four at a time: their point indices (and columns) are
    // requested together, then the four gathers of the object points (k_residual_cm: bound by these latencies)
    for (int64_t qb = q0 + threadIdx.x; qb < q1; qb += 4 * 256) {
        int pt[4]; long long cl[4]; double Q[4][3];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t q = qb + 256 * u;
            const bool on = q < q1;
            pt[u] = on ? cm_pt[q] : -1;
            cl[u] = (FULL && on) ? cm_col[q] : DEPTH_NO_COL;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double *p = z + NS + 3 * (int64_t)(pt[u] < 0 ? 0 : pt[u]);
            Q[u][0] = p[0]; Q[u][1] = p[1]; Q[u][2] = p[2];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (pt[u] < 0) continue;
            const double d = cam_depth(m, c, Q[u][0], Q[u][1], Q[u][2]);
            cnt += !(d > thr) ? 1u : 0u;
            depth_take(key, col, depth_key(d), cl[u]);
            if (FULL && depth_out) depth_out[cl[u]] = d;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        cnt += __shfl_xor(cnt, off, 64);
        const unsigned long long k2 = __shfl_xor(key, off, 64);
        const long long c2 = __shfl_xor(col, off, 64);
        depth_take(key, col, k2, c2);
    }
    if ((threadIdx.x & 63) == 0) { s_key[threadIdx.x >> 6] = key; s_col[threadIdx.x >> 6] = col; s_cnt[threadIdx.x >> 6] = cnt; }
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int w = 1; w < 4; ++w) { cnt += s_cnt[w]; depth_take(key, col, s_key[w], s_col[w]); }
    if (cnt) atomicAdd(red, (unsigned long long)cnt);
    if (key != DEPTH_KEY_NONE) atomicMin(red + 1, key);
    if (FULL) {
        if (key != DEPTH_KEY_NONE) atomicMin(img_min + cam, key);
        chunk_key[blockIdx.x] = key; chunk_col[blockIdx.x] = col;
    }
}

__device__ __forceinline__ void mailbox_done(double *mailbox, unsigned long long seq);      // (kernels.hpp)

// mailbox[slot ..] (slot: MB_DEPTH, laid out as MB_DEPTH_BEHIND / _MIN / _ARGMIN) = {count (as an integer's bit pattern),
// smallest depth (NaN: none), its smallest IP column (bit pattern; -1: none, and where FULL is off)}, then the host's ticket
template <bool FULL>
__global__ __launch_bounds__(256) void k_depth_finish(int64_t nchunks, const unsigned long long *__restrict__ red,
                                                      const unsigned long long *__restrict__ chunk_key, const long long *__restrict__ chunk_col,
                                                      double *__restrict__ mailbox, int slot, unsigned long long seq) {
    __shared__ long long s_col[4];
    const unsigned long long gmin = red[1];
    long long col = DEPTH_NO_COL;
    if (FULL && gmin != DEPTH_KEY_NONE) {
        for (int64_t b = threadIdx.x; b < nchunks; b += 256)
            if (chunk_key[b] == gmin && chunk_col[b] < col) col = chunk_col[b];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { const long long c2 = __shfl_xor(col, off, 64); col = c2 < col ? c2 : col; }
        if ((threadIdx.x & 63) == 0) s_col[threadIdx.x >> 6] = col;
        __syncthreads();
        if (threadIdx.x == 0)
            for (int w = 1; w < 4; ++w) col = s_col[w] < col ? s_col[w] : col;
    }
    if (threadIdx.x != 0) return;
    mailbox[slot + (MB_DEPTH_BEHIND - MB_DEPTH)] = __longlong_as_double((long long)red[0]);
    mailbox[slot + (MB_DEPTH_MIN - MB_DEPTH)] = depth_from_key(gmin);
    mailbox[slot + (MB_DEPTH_ARGMIN - MB_DEPTH)] = __longlong_as_double(col == DEPTH_NO_COL ? -1ll : col);
    mailbox_done(mailbox, seq);
}

#endif  // __HIPCC__

}  // namespace dbat
