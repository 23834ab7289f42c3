// Ray intersection angles (dbat_hip_ray_angles): for every object point the largest angle between two of its rays
// (photogrammetry/angles.m:26-46), for every image the largest angle between two of its rays (camangles.m:26-46).
//
// For k rays with unit directions n_j the angle is max acos(|clip(n_i . n_j)|) = acos(min_{i<j} |n_i . n_j|): the
// kernels reduce the MINIMUM of |n_i . n_j| and take one acos per point or image (angle_from_min); 0 for one ray,
// NaN for none.
//
//   k_angles_pt_light     tiled points (at most Plan::CMAX <= 21 rays): eight lanes per point; the group gathers the
//                         camera centres, normalises once into LDS and loops over the pairs
//   k_angles_pt_heavy     the plan's heavy / giant points (everything after the tiled batches): a workgroup per
//                         point, its directions in LDS
//   k_angles_cam_dirs     the unit directions of every image, component-major (x | y | z, each padded to a multiple
//                         of 16 with copies of the image's first direction: the products of a copy are products of a
//                         real pair or 1, so padding never lowers the minimum)
//   k_angles_cam_pairs    one workgroup per (image, run of ANG_RUN 16-direction tiles I); its four waves walk the
//                         tiles J >= I: one v_mfma_f64_16x16x4_f64 per 256 pairs (K = 3 padded to 4 by a zero), every
//                         lane folds min |acc| over its four accumulator values; wave / workgroup min, then ONE
//                         unsigned atomic min per workgroup on the bit pattern (non-negative doubles order as
//                         unsigned integers).  The lower triangle of tile pairs is never formed; the diagonal tile
//                         holds i = j, whose |cos| = 1 never lowers a minimum over k >= 2 rays.
//   k_angles_cam_finish   acos of the minima
// All arithmetic is f64; no atomics on floating-point values, so two runs give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>

#include "model.hpp"

namespace dbat {

constexpr int ANG_LIGHT_KMAX = 21;     // rays of a tiled point at most (plan.hpp: CMAX <= 21)
constexpr int ANG_LIGHT_LANES = 8;     // lanes per tiled point
constexpr int ANG_LIGHT_PTS = 256 / ANG_LIGHT_LANES;
constexpr int ANG_RUN = 8;             // 16-direction tiles I of one workgroup of k_angles_cam_pairs
constexpr int ANG_HEAVY_KMAX = 6656;   // rays of a heavy point at most: 3 doubles each in 156 KiB of LDS

// 1/sqrt(x): an estimate and two Newton steps y <- y + y/2 (1 - x y^2) (v_rsq_f64 is good to about 2^-23).  The host
// starts from 1.0 / sqrt(x), where the steps only correct the rounding.
DBAT_HD double rsqrt_refined(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    double y = __builtin_amdgcn_rsq(x);
#else
    double y = 1.0 / std::sqrt(x);
#endif
    const double e1 = __builtin_fma(-x * y, y, 1.0);
    y = __builtin_fma(0.5 * y, e1, y);
    const double e2 = __builtin_fma(-x * y, y, 1.0);
    return __builtin_fma(0.5 * y, e2, y);
}

// n = (q - c) / ||q - c||
DBAT_HD void unit_dir(const double *q, const double *c, double &n0, double &n1, double &n2) {
    const double d0 = q[0] - c[0], d1 = q[1] - c[1], d2 = q[2] - c[2];
    const double rs = rsqrt_refined(__builtin_fma(d0, d0, __builtin_fma(d1, d1, d2 * d2)));
    n0 = d0 * rs; n1 = d1 * rs; n2 = d2 * rs;
}

DBAT_HD double abs_dot(double a0, double a1, double a2, double b0, double b1, double b2) {
    return fabs(__builtin_fma(a0, b0, __builtin_fma(a1, b1, a2 * b2)));
}

// k rays whose smallest |cos| is m (+Inf: no pair gave a number)
DBAT_HD double angle_from_min(int64_t k, double m) {
    if (k <= 0) return __builtin_nan("");
    if (k == 1) return 0.0;
    if (!(m <= 2.0)) return __builtin_nan("");
    return acos(m < 1.0 ? m : 1.0);
}

#if defined(__HIPCC__)

__device__ __forceinline__ double ang_wave_min(double m) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmin(m, __shfl_xor(m, off, 64));
    return m;
}

// min over the 256 threads of a workgroup (valid in thread 0); s: four doubles of LDS
__device__ __forceinline__ double ang_block_min(double m, double *s) {
    m = ang_wave_min(m);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = m;
    __syncthreads();
    return fmin(fmin(s[0], s[1]), fmin(s[2], s[3]));
}

// points [0, npts) of the processing order, all with at most ANG_LIGHT_KMAX rays: out[rank] = angle
__global__ __launch_bounds__(256) void k_angles_pt_light(const double *__restrict__ z, int64_t NS, const CamRec *__restrict__ cams,
                                                         const int32_t *__restrict__ o_cam, const int64_t *__restrict__ pt_pos,
                                                         int32_t npts, double *__restrict__ out) {
    __shared__ double dir[ANG_LIGHT_PTS][ANG_LIGHT_KMAX * 3];
    const int g = threadIdx.x / ANG_LIGHT_LANES, l = threadIdx.x % ANG_LIGHT_LANES;
    const int64_t r = (int64_t)blockIdx.x * ANG_LIGHT_PTS + g;
    const bool live = r < npts;
    int64_t o0 = 0;
    int k = 0;
    if (live) { o0 = pt_pos[r]; k = (int)(pt_pos[r + 1] - o0); }
    const int ks = k < ANG_LIGHT_KMAX ? k : ANG_LIGHT_KMAX;      // (the host has checked k: never clipped)
    if (ks > 0) {
        const double *q = z + NS + 3 * r;
        for (int j = l; j < ks; j += ANG_LIGHT_LANES) {
            double n0, n1, n2;
            unit_dir(q, cams[o_cam[o0 + j]].c, n0, n1, n2);
            dir[g][3 * j] = n0; dir[g][3 * j + 1] = n1; dir[g][3 * j + 2] = n2;
        }
    }
    __syncthreads();
    double m = INFINITY;
    for (int i = l; i < ks; i += ANG_LIGHT_LANES) {
        const double a0 = dir[g][3 * i], a1 = dir[g][3 * i + 1], a2 = dir[g][3 * i + 2];
        for (int j = i + 1; j < ks; ++j) m = fmin(m, abs_dot(a0, a1, a2, dir[g][3 * j], dir[g][3 * j + 1], dir[g][3 * j + 2]));
    }
#pragma unroll
    for (int off = ANG_LIGHT_LANES / 2; off > 0; off >>= 1) m = fmin(m, __shfl_xor(m, off, ANG_LIGHT_LANES));
    if (live && l == 0) out[r] = angle_from_min(k, m);
}

// point p0 + blockIdx.x of the processing order, any number of rays up to kcap (the doubles of dynamic LDS / 3)
__global__ __launch_bounds__(256) void k_angles_pt_heavy(const double *__restrict__ z, int64_t NS, const CamRec *__restrict__ cams,
                                                         const int32_t *__restrict__ o_cam, const int64_t *__restrict__ pt_pos,
                                                         int32_t p0, int32_t kcap, double *__restrict__ out) {
    extern __shared__ double hdir[];
    __shared__ double red[4];
    const int64_t r = (int64_t)p0 + blockIdx.x;
    const int64_t o0 = pt_pos[r];
    const int k = (int)(pt_pos[r + 1] - o0);
    const int ks = k < kcap ? k : kcap;                          // (the host has checked k: never clipped)
    const double *q = z + NS + 3 * r;
    for (int j = threadIdx.x; j < ks; j += 256) {
        double n0, n1, n2;
        unit_dir(q, cams[o_cam[o0 + j]].c, n0, n1, n2);
        hdir[3 * j] = n0; hdir[3 * j + 1] = n1; hdir[3 * j + 2] = n2;
    }
    __syncthreads();
    double m = INFINITY;
    for (int i = 0; i + 1 < ks; ++i) {
        const double a0 = hdir[3 * i], a1 = hdir[3 * i + 1], a2 = hdir[3 * i + 2];
        for (int j = i + 1 + threadIdx.x; j < ks; j += 256) m = fmin(m, abs_dot(a0, a1, a2, hdir[3 * j], hdir[3 * j + 1], hdir[3 * j + 2]));
    }
    m = ang_block_min(m, red);
    if (threadIdx.x == 0) out[r] = angle_from_min(k, m);
}

// Where an image's observations are in the camera-major copy of the plan (tiled part, then the heavy / giant part):
// cam_src[4 c ..] = {first of the tiled part, their number, first of the rest, observations in all};
// cam_pad[c] = first padded slot of image c (16 per tile), cdir holds 3 doubles per slot, component-major per image.
__global__ __launch_bounds__(256) void k_angles_cam_dirs(const double *__restrict__ z, int64_t NS, const CamRec *__restrict__ cams, int nc,
                                                         const int32_t *__restrict__ cm_pt, const int64_t *__restrict__ cam_src,
                                                         const int64_t *__restrict__ cam_pad, double *__restrict__ cdir) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= cam_pad[nc]) return;
    int lo = 0, hi = nc;                                         // the image c with cam_pad[c] <= s < cam_pad[c + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cam_pad[mid] <= s) lo = mid; else hi = mid;
    }
    const int c = lo;
    const int64_t s0 = cam_pad[c], npad = cam_pad[c + 1] - s0;
    const int64_t *src = cam_src + 4 * (int64_t)c;
    int64_t i = s - s0;
    if (i >= src[3]) i = 0;                                      // padding: the first direction again
    const int64_t o = i < src[1] ? src[0] + i : src[2] + (i - src[1]);
    double n0, n1, n2;
    unit_dir(z + NS + 3 * (int64_t)cm_pt[o], cams[c].c, n0, n1, n2);
    double *dst = cdir + 3 * s0 + (s - s0);
    dst[0] = n0; dst[npad] = n1; dst[2 * npad] = n2;
}

__device__ __forceinline__ double ang_fold(double m, mfma_d4 acc) {
    return fmin(fmin(m, fmin(fabs(acc[0]), fabs(acc[1]))), fmin(fabs(acc[2]), fabs(acc[3])));
}

// work item b: image wi[2 b], tiles I = wi[2 b + 1] .. + ANG_RUN - 1 against every tile J >= I
__global__ __launch_bounds__(256) void k_angles_cam_pairs(const double *__restrict__ cdir, const int64_t *__restrict__ cam_pad,
                                                          const int32_t *__restrict__ wi, unsigned long long *__restrict__ cam_min) {
    __shared__ double red[4];
    const int c = wi[2 * blockIdx.x], I0 = wi[2 * blockIdx.x + 1];
    const int64_t s0 = cam_pad[c];
    const int64_t npad = cam_pad[c + 1] - s0;
    const int T = (int)(npad >> 4);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = lane & 15, kk = lane >> 4;                   // operand layout of heavy.hpp: lane = (k-column kk, row)
    const double *col = cdir + 3 * s0 + (kk < 3 ? kk : 0) * npad + row;
    const int nI = T - I0 < ANG_RUN ? T - I0 : ANG_RUN;
    double a[ANG_RUN];
#pragma unroll
    for (int q = 0; q < ANG_RUN; ++q) a[q] = (q < nI && kk < 3) ? col[16 * (I0 + q)] : 0.0;
    double m = INFINITY;
    const mfma_d4 zero = {0, 0, 0, 0};
    for (int J = I0 + wave; J < T; J += 4) {
        const double bv = kk < 3 ? col[16 * (int64_t)J] : 0.0;
        const int qn = J - I0 + 1 < nI ? J - I0 + 1 : nI;        // tiles I <= J of this run
        if (qn == ANG_RUN) {
            mfma_d4 acc[ANG_RUN];
#pragma unroll
            for (int q = 0; q < ANG_RUN; ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], bv, zero, 0, 0, 0);
#pragma unroll
            for (int q = 0; q < ANG_RUN; ++q) m = ang_fold(m, acc[q]);
        } else {
#pragma unroll
            for (int q = 0; q < ANG_RUN; ++q)
                if (q < qn) m = ang_fold(m, __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], bv, zero, 0, 0, 0));
        }
    }
    m = ang_block_min(m, red);
    if (threadIdx.x == 0 && m <= 2.0) atomicMin(cam_min + c, (unsigned long long)__double_as_longlong(m));
}

__global__ __launch_bounds__(256) void k_angles_cam_finish(int nc, const int64_t *__restrict__ cam_src,
                                                           const unsigned long long *__restrict__ cam_min, double *__restrict__ out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= nc) return;
    out[c] = angle_from_min(cam_src[4 * (int64_t)c + 3], __longlong_as_double((long long)cam_min[c]));   // (never lowered: all ones, a NaN)
}

#endif  // __HIPCC__

}  // namespace dbat
