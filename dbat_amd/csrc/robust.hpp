// Robust reweighting of the image observations (iteratively reweighted least squares, dbat_hip_solve_robust).
//
// Per owned observation k (processing order) at the parameters of the last residual pass:
//   s_k   = ||(w_u v_u, w_v v_v)||, w the BASE weights (1 / sigma_mm of the plan), v the unweighted residual
//   scale = 1 ('apriori') or median(s) / sqrt(2 ln 2) ('mad'; exact median, all ranks' observations)
//   u_k   = s_k / scale, omega_k = Huber (u <= k ? 1 : k / u) or Cauchy 1 / (1 + (u/k)^2)
//   both rows of the observation then carry base * sqrt(omega_k) (o_w, and its slot-major / camera-major copies).
// The median is a radix select over the IEEE bit patterns of s (s >= 0: they order like uint64): six passes of
// 11/11/11/11/10/10 bits from the top; every pass histograms, per workgroup in LDS, the digit of the values whose
// higher bits equal the prefix chosen so far, merges with one global atomic per non-empty bin, and one workgroup
// picks the bucket of each of the two middle order statistics (equal for an odd count).  A sharded handle sums the
// histograms over the ranks between the two kernels: the select is collective and every rank picks the same bucket.
#pragma once

#include <cstdint>

#include "../../include/dbat_hip.h"

namespace dbat {

constexpr double ROBUST_MAD_C = 1.1774100225154747;     // sqrt(2 ln 2): the median of a chi_2-distributed norm
constexpr int RSEL_BINS = 2048;
constexpr int RSEL_PASSES = 6;
constexpr int RSEL_SHIFT[RSEL_PASSES] = {53, 42, 31, 20, 10, 0};
constexpr int RSEL_BITS[RSEL_PASSES] = {11, 11, 11, 11, 10, 10};

__device__ __forceinline__ double robust_omega(double s, double scale, int loss, double k) {
    const double u = s / scale;
    if (loss == DBAT_HIP_LOSS_HUBER) return u <= k ? 1.0 : k / u;
    const double t = u / k;
    return 1.0 / (1.0 + t * t);
}

// base weights of a plan with uniform weights per camera, spread over its observations (promotion)
__global__ __launch_bounds__(256) void k_robust_base(int64_t nobs, const int32_t *__restrict__ o_cam,
                                                     const double *__restrict__ cam_w, double *__restrict__ base) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nobs; k += (int64_t)gridDim.x * blockDim.x) {
        const int c = o_cam[k];
        base[2 * k] = cam_w[2 * c]; base[2 * k + 1] = cam_w[2 * c + 1];
    }
}

__global__ __launch_bounds__(256) void k_robust_fill(int64_t n, double v, double *__restrict__ out) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) out[k] = v;
}

// s_k from the unweighted residual rows that k_residual left in reference row order; optionally s in IP order
// (base == nullptr: a handle with uniform weights that was never promoted -- the camera's weights)
__global__ __launch_bounds__(256) void k_robust_norm(int64_t nobs, const int64_t *__restrict__ o_row, const double *__restrict__ r_unw,
                                                     const double *__restrict__ base, const int32_t *__restrict__ o_cam,
                                                     const double *__restrict__ cam_w, uint64_t *__restrict__ s_bits,
                                                     double *__restrict__ s_ip) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nobs; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = o_row[k];
        const double *w = base ? base + 2 * k : cam_w + 2 * o_cam[k];
        const double a = w[0] * r_unw[2 * row], b = w[1] * r_unw[2 * row + 1];
        const double s = __builtin_sqrt(a * a + b * b);
        s_bits[k] = (uint64_t)__double_as_longlong(s);
        if (s_ip) s_ip[row] = s;
    }
}

// One pass of the select: the digit histograms of the two targets (state[0], state[1]: their prefixes; one histogram
// when they are equal) over the values that match the prefix above the digit.
__global__ __launch_bounds__(256) void k_rsel_hist(int64_t n, const uint64_t *__restrict__ s_bits, const uint64_t *__restrict__ state,
                                                   int shift, int nbits, unsigned *__restrict__ hist) {
    __shared__ unsigned h[2 * RSEL_BINS];
    for (int i = threadIdx.x; i < 2 * RSEL_BINS; i += blockDim.x) h[i] = 0;
    __syncthreads();
    const uint64_t p0 = state[0], p1 = state[1];
    const bool two = p0 != p1;
    const uint64_t hi = shift + nbits >= 64 ? 0ull : ~0ull << (shift + nbits);
    const uint64_t dm = (1ull << nbits) - 1;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t v = s_bits[k];
        const int dg = (int)((v >> shift) & dm);
        if ((v & hi) == p0) atomicAdd(&h[dg], 1u);
        if (two && (v & hi) == p1) atomicAdd(&h[RSEL_BINS + dg], 1u);
    }
    __syncthreads();
    const int nb = two ? 2 * RSEL_BINS : RSEL_BINS;
    for (int i = threadIdx.x; i < nb; i += blockDim.x)
        if (h[i]) atomicAdd(&hist[i], h[i]);
}

// sharded handle: the counts as doubles for the all-reduce (exact below 2^53); the integer histogram is cleared
__global__ __launch_bounds__(256) void k_rsel_to_f64(unsigned *__restrict__ hist, double *__restrict__ out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 2 * RSEL_BINS; i += gridDim.x * blockDim.x) {
        out[i] = (double)hist[i];
        hist[i] = 0;
    }
}

// One workgroup of 256: for each target, the bucket that holds its remaining rank (state[2 + t]); the prefix grows by
// the bucket's digit, the rank loses the counts below it.  The integer histogram is cleared for the next pass.
template <bool F64>
__global__ __launch_bounds__(256) void k_rsel_pick(unsigned *__restrict__ hist, const double *__restrict__ hist_f, uint64_t *__restrict__ state,
                                                   int shift) {
    __shared__ uint64_t part[256];
    __shared__ uint64_t res[4];
    const int tid = threadIdx.x;
    const uint64_t p0 = state[0], p1 = state[1], rk0 = state[2], rk1 = state[3];
    const bool two = p0 != p1;
    if (tid == 0) { res[0] = p0; res[1] = p1; res[2] = rk0; res[3] = rk1; }
    constexpr int PER = RSEL_BINS / 256;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const uint64_t pt = t ? p1 : p0, rkt = t ? rk1 : rk0;
        const int src = two ? t : 0;
        uint64_t c[PER], sum = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int b = src * RSEL_BINS + tid * PER + j;
            c[j] = F64 ? (uint64_t)hist_f[b] : (uint64_t)hist[b];
            sum += c[j];
        }
        __syncthreads();
        part[tid] = sum;
        __syncthreads();
        if (tid == 0) {
            uint64_t run = 0;
            for (int i = 0; i < 256; ++i) { const uint64_t v = part[i]; part[i] = run; run += v; }
        }
        __syncthreads();
        uint64_t below = part[tid];
#pragma unroll
        for (int j = 0; j < PER; ++j) {              // (no early exit: c[] stays in registers)
            if (rkt >= below && rkt < below + c[j]) {
                res[t] = pt | ((uint64_t)(tid * PER + j) << shift);
                res[2 + t] = rkt - below;
            }
            below += c[j];
        }
    }
    __syncthreads();
    if (tid < 4) state[tid] = res[tid];
    if (!F64)
        for (int i = tid; i < 2 * RSEL_BINS; i += 256) hist[i] = 0;
}

// out[o_row[k]] = v[k]: a per-observation vector in IP order (this rank's entries)
__global__ __launch_bounds__(256) void k_scatter_rows1(int64_t nobs, const int64_t *__restrict__ o_row, const double *__restrict__ v,
                                                       double *__restrict__ out) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nobs; k += (int64_t)gridDim.x * blockDim.x) out[o_row[k]] = v[k];
}

// omega' of every owned observation and max |omega' - omega| (wave reduction, one atomic max on the bit pattern per
// wave); optionally omega' in IP order.  Nothing is applied.  (omega == nullptr: the factors of a fresh handle, all 1)
__global__ __launch_bounds__(256) void k_robust_weight(int64_t nobs, const uint64_t *__restrict__ s_bits, double scale, int loss,
                                                       double kk, const double *__restrict__ omega, const int64_t *__restrict__ o_row,
                                                       double *__restrict__ omega_ip, unsigned long long *__restrict__ maxchg) {
    double m = 0.0;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nobs; k += (int64_t)gridDim.x * blockDim.x) {
        const double w = robust_omega(__longlong_as_double((long long)s_bits[k]), scale, loss, kk);
        m = fmax(m, fabs(w - (omega ? omega[k] : 1.0)));
        if (omega_ip) omega_ip[o_row[k]] = w;
    }
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0 && m > 0.0) atomicMax(maxchg, (unsigned long long)__double_as_longlong(m));
}

// The weights of every owned observation from omega: base * sqrt(omega) into o_w and its slot-major (sg_map, -1: no
// slot) and camera-major (cm_map) copies.  FROM_S: omega is recomputed from s first (what k_robust_weight gave) and
// stored.
template <bool FROM_S>
__global__ __launch_bounds__(256) void k_robust_apply(int64_t nobs, const uint64_t *__restrict__ s_bits, double scale, int loss, double kk,
                                                      double *__restrict__ omega, const double *__restrict__ base, double *__restrict__ o_w,
                                                      const int32_t *__restrict__ sg_map, double *__restrict__ sg_w,
                                                      const int32_t *__restrict__ cm_map, double *__restrict__ cm_w) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nobs; k += (int64_t)gridDim.x * blockDim.x) {
        double w;
        if constexpr (FROM_S) {
            w = robust_omega(__longlong_as_double((long long)s_bits[k]), scale, loss, kk);
            omega[k] = w;
        } else {
            w = omega[k];
        }
        const double f = __builtin_sqrt(w);
        const double w0 = base[2 * k] * f, w1 = base[2 * k + 1] * f;
        o_w[2 * k] = w0; o_w[2 * k + 1] = w1;
        if (sg_map) {
            const int32_t q = sg_map[k];
            if (q >= 0) { sg_w[2 * (int64_t)q] = w0; sg_w[2 * (int64_t)q + 1] = w1; }
        }
        const int64_t q = cm_map[k];
        cm_w[2 * q] = w0; cm_w[2 * q + 1] = w1;
    }
}

}  // namespace dbat
