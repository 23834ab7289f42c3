// Posterior covariance blocks and reliability (dbat_hip_posterior_cov, dbat_hip_redundancy): kernels that read inv(S)
// and the point blocks of a linearisation at z.  No LM step launches any of them; the host side is cov_host.hpp.
//
//   k_cov_cam                   CEO, CIO: blocks of inv(S)
//   k_cov_points, k_cov_giant   COP per point; HAT: Qvv = I - H_t of every image point instead
//   k_hat_cam_blocks            inv(S)[cols_c, cols_c] of every camera, staged for the HAT kernels
//   k_hat_prior                 redundancy numbers of the prior rows
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace dbat {

// ------------------------------------------------------- posterior cov ---
// bundle_cov.m: blocks of C = s0^2 inv(J'J).  With the points eliminated,
//   inv(J'J)[cams, cams] = inv(S)                         (CEO, CIO)
//   inv(J'J)[p, p]       = V_p^-1 + Y_p' inv(S) Y_p,  Y_p = W_p V_p^-1  (COP)
// inv(S) comes in one of two forms (SinvView):
//   dense   the lower triangle of inv(S), column-major with leading dimension ld (rocsolver_dpotri on the in-place factor:
//           several ranks, shared EO blocks, or a caller who wants the whole inverse);
//   tiles   the entries of inv(S) ON THE PATTERN OF THE FACTOR only -- compact 64 x 64 tiles in the nested-dissection order
//           of the dataflow Cholesky, from the selected inversion of chol_df.hpp (DataflowChol::selected_inverse).  Everything
//           the covariance blocks need lies on that pattern: the cameras' own blocks, the IO block, and the blocks of camera
//           pairs that see a common object point.
struct SinvView {
    const double *dense = nullptr; int64_t ld = 0;
    const double *tiles = nullptr; const int64_t *toff = nullptr; const int *perm = nullptr; int nT = 0;
};
__device__ __forceinline__ double sym_at(const SinvView &V, int64_t /*unused*/, int r, int c) {
    if (V.dense) return r >= c ? V.dense[(int64_t)c * V.ld + r] : V.dense[(int64_t)r * V.ld + c];
    const int pr = V.perm[r], pc = V.perm[c];
    const int i = max(pr, pc), j = min(pr, pc);
    const int64_t off = V.toff[(int64_t)(i >> 6) * V.nT + (j >> 6)];
    return off < 0 ? 0.0 : V.tiles[off + (int64_t)(j & 63) * 64 + (i & 63)];      // (diagonal tiles hold both triangles)
}

// CEO: 6x6 block per image (zero rows/columns for fixed elements); CIO: the
// nIOu x nIOu block of the IO unknowns.
__global__ void k_cov_cam(DevProblem d, const SinvView Sinv, double s02, double *__restrict__ CEO,
                          double *__restrict__ CIO) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t nE = 36 * (int64_t)d.nc, nI = (int64_t)d.nIOu * d.nIOu;
    if (i < nE) {
        if (!CEO) return;
        const int c = (int)(i / 36), e = (int)(i % 36), a = e % 6, b = e / 6;
        const int ra = d.cam_col[(int64_t)c * MAXCOL + a], rb = d.cam_col[(int64_t)c * MAXCOL + b];   // (shared elements: the leader's)
        CEO[i] = (d.z_est[ra] && d.z_est[rb]) ? s02 * sym_at(Sinv, d.ldS, ra, rb) : 0.0;
    } else if (i < nE + nI) {
        if (!CIO) return;
        const int64_t q = i - nE;
        const int a = (int)(q % d.nIOu), b = (int)(q / d.nIOu);
        CIO[q] = s02 * sym_at(Sinv, d.ldS, 6 * d.nc + a, 6 * d.nc + b);
    }
}

// Reliability (dbat_hip_redundancy): the hat-matrix block H_t = J_t inv(J'J) J_t' of every image point, J_t = [E_t | B_t]
// its weighted rows.  With C = inv(J'J), C_cc = inv(S)[cols_t, cols_t], C_cp = -R (R_a = sum_j inv(S)[col_a, cols_j] Y_j,
// the rows k_cov_points forms anyway) and C_pp = V^-1 + Y' inv(S) Y (COP unscaled):
//   H_t = E C_cc E' - E R B' - B R' E' + B C_pp B'
// The k_cov_points / k_cov_giant of HAT = true form it in a third phase, once the segment head has C_pp.
struct HatOut {
    const double *Ccc = nullptr;    // [nc][ncolmax^2] inv(S)[cols_c, cols_c] of every camera (k_hat_cam_blocks)
    double *qvv = nullptr;          // [3 * nIP] Qvv = I - H_t per image point, CALLER's order (o_row): r_u, q_uv, r_v
    double *dCz = nullptr;          // [NZ] diag C of the point unknowns (z order), for the prior rows; zero where no point
    double *gscr = nullptr;         // [giant observations][9] k_cov_giant<HAT>: E C_cc E' - E R B' - B R' E' and B
};

// inv(S)[cols_c, cols_c] of every camera, ncol_c x ncol_c row-major at stride ncolmax^2: the E C_cc E' term then reads
// one contiguous block instead of ncol^2 lookups through the permutation and the tile table
__global__ void k_hat_cam_blocks(DevProblem d, const CamRec *__restrict__ cams, const SinvView Sinv,
                                 double *__restrict__ Ccc) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int n2 = d.ncolmax * d.ncolmax;
    if (i >= (int64_t)d.nc * n2) return;
    const int c = (int)(i / n2), e = (int)(i % n2);
    const CamRec &C = cams[c];
    const int a = e / C.ncol, b = e % C.ncol;
    if (a >= C.ncol) return;
    Ccc[i] = sym_at(Sinv, d.ldS, C.col[a], C.col[b]);
}

// h = w_p C(p, p) of every prior row (the row order of dbat_hip_final_residuals), as r = 1 - h.  A point unknown
// whose diagonal is still zero has no observation: its prior alone determines it (h = 1).
__global__ void k_hat_prior(DevProblem d, const SinvView Sinv, const int64_t *__restrict__ prior_z, int64_t nprior,
                            const double *__restrict__ dCz, double *__restrict__ rp) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= nprior) return;
    const int64_t zi = prior_z[i];
    double h = 0.0;
    if (d.z_est[zi]) {
        const double c = zi < d.NS ? sym_at(Sinv, d.ldS, (int)zi, (int)zi) : dCz[zi];
        h = (zi >= d.NS && c == 0.0) ? 1.0 : d.z_prw[zi] * c;
    }
    rp[i] = 1.0 - h;
}

// E_t C_cc E_t' (2 x 2: h00 h01 h11) from the camera's staged block
template <int NCX>
__device__ __forceinline__ void hat_ece(const double *__restrict__ cc, int ncol, const double (&E)[2][NCX],
                                        double &h00, double &h01, double &h11) {
#pragma unroll
    for (int a = 0; a < NCX; ++a)
        if (a < ncol) {
            double t0 = 0, t1 = 0;
#pragma unroll
            for (int b = 0; b < NCX; ++b)
                if (b < ncol) { const double cv = cc[a * ncol + b]; t0 += cv * E[0][b]; t1 += cv * E[1][b]; }
            h00 += E[0][a] * t0; h01 += E[0][a] * t1; h11 += E[1][a] * t1;
        }
}
// the cross terms -E R B' - B R' E' (er = E R, 2 x 3)
__device__ __forceinline__ void hat_cross(const double (&er)[6], const double (&B)[2][3], double &h00, double &h01,
                                          double &h11) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        h00 -= 2.0 * er[k] * B[0][k];
        h01 -= er[k] * B[1][k] + B[0][k] * er[3 + k];
        h11 -= 2.0 * er[3 + k] * B[1][k];
    }
}
// + B C_pp B' (C_pp symmetric: xx xy xz yy yz zz), and Qvv = I - H to the caller's row
__device__ __forceinline__ void hat_finish(const double *cp, const double (&B)[2][3], double h00, double h01,
                                           double h11, double *__restrict__ q) {
    double cb0[3], cb1[3];
    const double M[3][3] = {{cp[0], cp[1], cp[2]}, {cp[1], cp[3], cp[4]}, {cp[2], cp[4], cp[5]}};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        cb0[k] = M[k][0] * B[0][0] + M[k][1] * B[0][1] + M[k][2] * B[0][2];
        cb1[k] = M[k][0] * B[1][0] + M[k][1] * B[1][1] + M[k][2] * B[1][2];
    }
    h00 += B[0][0] * cb0[0] + B[0][1] * cb0[1] + B[0][2] * cb0[2];
    h01 += B[0][0] * cb1[0] + B[0][1] * cb1[1] + B[0][2] * cb1[2];
    h11 += B[1][0] * cb1[0] + B[1][1] * cb1[1] + B[1][2] * cb1[2];
    q[0] = 1.0 - h00; q[1] = -h01; q[2] = 1.0 - h11;
}

// COP for the points of one batch (same layout as k_build: lane t <-> observation).  HAT: Qvv of every observation
// instead (HatOut above); COP is not written.
template <int MODEL, bool WITH_IO, bool HAT = false>
__global__ __launch_bounds__(256) void k_cov_points(DevProblem d, const double *__restrict__ z,
                                                    const CamRec *__restrict__ cams,
                                                    const double *__restrict__ Vinv,
                                                    const SinvView Sinv, double s02,
                                                    double *__restrict__ COP, const HatOut hat = HatOut{}) {
    constexpr int NCX = WITH_IO ? MAXCOL : 6;
    extern __shared__ double smem[];
    const int BT = blockDim.x;
    const int strideW = d.ncolmax * 3;
    double *Yl = smem;                               // [BT][strideW]  Y = W V^-1
    double *red = Yl + (size_t)BT * strideW;         // [BT][6]
    const int t = threadIdx.x;
    const int64_t o0 = d.batch_start[blockIdx.x];
    const int nobs = (int)(d.batch_start[blockIdx.x + 1] - o0);
    const bool active = t < nobs;
    const int64_t o = o0 + t;
    int pt = 0, seg_start = 0, seg_len = 0, ncol = 6;
    const CamRec *C = cams;
    double vi[6] = {0, 0, 0, 0, 0, 0};
    double E[2][NCX], B[2][3];                       // (HAT: kept for the third phase)
    if (active) {
        pt = d.o_pt[o];
        const uint32_t sg = d.o_seg[o];
        seg_start = sg & 0xFFFF; seg_len = sg >> 16;
        C = cams + d.o_cam[o];
        ncol = WITH_IO ? C->ncol : 6;
        double r[2];
        eval_obs_cols<MODEL, WITH_IO>(d, *C, z, o, pt, r, E, B);
        point_block_inverse(Vinv + 6 * (int64_t)pt, vi);
        double *yl = Yl + (size_t)t * strideW;
#pragma unroll
        for (int a = 0; a < NCX; ++a)
            if (a < ncol) {
                const double w0 = E[0][a] * B[0][0] + E[1][a] * B[1][0];
                const double w1 = E[0][a] * B[0][1] + E[1][a] * B[1][1];
                const double w2 = E[0][a] * B[0][2] + E[1][a] * B[1][2];
                yl[3 * a] = w0 * vi[0] + w1 * vi[1] + w2 * vi[2];
                yl[3 * a + 1] = w0 * vi[1] + w1 * vi[3] + w2 * vi[4];
                yl[3 * a + 2] = w0 * vi[2] + w1 * vi[4] + w2 * vi[5];
            }
    }
    __syncthreads();
    double h00 = 0, h01 = 0, h11 = 0;                // (HAT) E C_cc E' - E R B' - B R' E'
    if (active) {
        // c = Y_i' (sum_j Sinv[cols_i, cols_j] Y_j), symmetric part xx xy xz yy yz zz
        double c6[6] = {0, 0, 0, 0, 0, 0};
        double er[6] = {0, 0, 0, 0, 0, 0};           // (HAT) E R
        const double *yi = Yl + (size_t)t * strideW;
        for (int a = 0; a < ncol; ++a) {
            const int ra = C->col[a];
            double r0 = 0, r1 = 0, r2 = 0;
            for (int jj = seg_start; jj < seg_start + seg_len; ++jj) {
                const CamRec *Cj = cams + d.o_cam[o0 + jj];
                const int ncj = WITH_IO ? Cj->ncol : 6;
                const double *yj = Yl + (size_t)jj * strideW;
                for (int b = 0; b < ncj; ++b) {
                    const double sv = sym_at(Sinv, d.ldS, ra, Cj->col[b]);
                    r0 += sv * yj[3 * b]; r1 += sv * yj[3 * b + 1]; r2 += sv * yj[3 * b + 2];
                }
            }
            const double y0 = yi[3 * a], y1 = yi[3 * a + 1], y2 = yi[3 * a + 2];
            c6[0] += y0 * r0; c6[1] += 0.5 * (y0 * r1 + y1 * r0); c6[2] += 0.5 * (y0 * r2 + y2 * r0);
            c6[3] += y1 * r1; c6[4] += 0.5 * (y1 * r2 + y2 * r1); c6[5] += y2 * r2;
            if constexpr (HAT) {                     // column a of E by selects: no dynamic register index
                double ea0 = 0, ea1 = 0;
#pragma unroll
                for (int q = 0; q < NCX; ++q) if (q == a) { ea0 = E[0][q]; ea1 = E[1][q]; }
                er[0] += ea0 * r0; er[1] += ea0 * r1; er[2] += ea0 * r2;
                er[3] += ea1 * r0; er[4] += ea1 * r1; er[5] += ea1 * r2;
            }
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) red[6 * t + q] = c6[q];
        if constexpr (HAT) {
            hat_ece<NCX>(hat.Ccc + (int64_t)d.o_cam[o] * d.ncolmax * d.ncolmax, ncol, E, h00, h01, h11);
            hat_cross(er, B, h00, h01, h11);
        }
    }
    __syncthreads();
    if (active && t == seg_start) {
        double c6[6] = {vi[0], vi[1], vi[2], vi[3], vi[4], vi[5]};
        for (int j = 0; j < seg_len; ++j)
#pragma unroll
            for (int q = 0; q < 6; ++q) c6[q] += red[6 * (t + j) + q];
        const int64_t zp = d.NS + 3 * (int64_t)pt;
        const bool e0 = d.z_est[zp], e1 = d.z_est[zp + 1], e2 = d.z_est[zp + 2];
        if constexpr (HAT) {                         // C_pp to the segment through the head's slot (read it all above)
#pragma unroll
            for (int q = 0; q < 6; ++q) red[6 * t + q] = c6[q];
            hat.dCz[zp] = e0 ? c6[0] : 0.0; hat.dCz[zp + 1] = e1 ? c6[3] : 0.0; hat.dCz[zp + 2] = e2 ? c6[5] : 0.0;
        } else {
            double *out = COP + 9 * (int64_t)pt;
            out[0] = e0 ? s02 * c6[0] : 0.0;
            out[1] = out[3] = (e0 && e1) ? s02 * c6[1] : 0.0;
            out[2] = out[6] = (e0 && e2) ? s02 * c6[2] : 0.0;
            out[4] = e1 ? s02 * c6[3] : 0.0;
            out[5] = out[7] = (e1 && e2) ? s02 * c6[4] : 0.0;
            out[8] = e2 ? s02 * c6[5] : 0.0;
        }
    }
    if constexpr (HAT) {
        __syncthreads();
        if (active) hat_finish(red + 6 * seg_start, B, h00, h01, h11, hat.qvv + 3 * d.o_row[o]);
    }
}

// COP of a giant point: one workgroup per point, Y in the W scratch.  HAT: Qvv of its observations instead (a thread
// holds several: the terms of phase two wait in hat.gscr for C_pp).
template <int MODEL, bool WITH_IO, bool HAT = false>
__global__ __launch_bounds__(256) void k_cov_giant(DevProblem d, const double *__restrict__ z,
                                                   const CamRec *__restrict__ cams,
                                                   const double *__restrict__ Vinv, const SinvView Sinv,
                                                   double s02, double *__restrict__ COP, const HatOut hat = HatOut{}) {
    constexpr int NCX = WITH_IO ? MAXCOL : 6;
    __shared__ double sh[6 * 4];
    __shared__ double cpp[HAT ? 6 : 1];
    const int t = threadIdx.x, BT = blockDim.x;
    const int64_t o0 = d.giant_start[blockIdx.x], o1 = d.giant_start[blockIdx.x + 1];
    const int k = (int)(o1 - o0);
    const int strideW = d.ncolmax * 3;
    double *Yg = d.giant_W + (o0 - d.giant_start[0]) * strideW;
    const int pt = d.o_pt[o0];
    double vi[6];
    point_block_inverse(Vinv + 6 * (int64_t)pt, vi);
    for (int i = t; i < k; i += BT) {
        const int64_t o = o0 + i;
        const CamRec &C = cams[d.o_cam[o]];
        const int ncol = WITH_IO ? C.ncol : 6;
        double r[2], E[2][NCX], B[2][3];
        eval_obs_cols<MODEL, WITH_IO>(d, C, z, o, pt, r, E, B);
        double *yl = Yg + (size_t)i * strideW;
        for (int a = 0; a < NCX; ++a) {
            if (a >= ncol) break;
            double ea0 = 0, ea1 = 0;
#pragma unroll
            for (int q = 0; q < NCX; ++q) if (q == a) { ea0 = E[0][q]; ea1 = E[1][q]; }
            const double w0 = ea0 * B[0][0] + ea1 * B[1][0];
            const double w1 = ea0 * B[0][1] + ea1 * B[1][1];
            const double w2 = ea0 * B[0][2] + ea1 * B[1][2];
            yl[3 * a] = w0 * vi[0] + w1 * vi[1] + w2 * vi[2];
            yl[3 * a + 1] = w0 * vi[1] + w1 * vi[3] + w2 * vi[4];
            yl[3 * a + 2] = w0 * vi[2] + w1 * vi[4] + w2 * vi[5];
        }
    }
    __threadfence_block();
    __syncthreads();
    double c6[6] = {0, 0, 0, 0, 0, 0};
    for (int i = t; i < k; i += BT) {
        const CamRec &Ci = cams[d.o_cam[o0 + i]];
        const int nci = WITH_IO ? Ci.ncol : 6;
        const double *yi = Yg + (size_t)i * strideW;
        double E[2][NCX], B[2][3], er[6] = {0, 0, 0, 0, 0, 0};     // (HAT: the observation's rows again, E R)
        if constexpr (HAT) { double r[2]; eval_obs_cols<MODEL, WITH_IO>(d, Ci, z, o0 + i, pt, r, E, B); }
        for (int a = 0; a < nci; ++a) {
            const int ra = Ci.col[a];
            double r0 = 0, r1 = 0, r2 = 0;
            for (int j = 0; j < k; ++j) {
                const CamRec &Cj = cams[d.o_cam[o0 + j]];
                const int ncj = WITH_IO ? Cj.ncol : 6;
                const double *yj = Yg + (size_t)j * strideW;
                for (int b = 0; b < ncj; ++b) {
                    const double sv = sym_at(Sinv, d.ldS, ra, Cj.col[b]);
                    r0 += sv * yj[3 * b]; r1 += sv * yj[3 * b + 1]; r2 += sv * yj[3 * b + 2];
                }
            }
            const double y0 = yi[3 * a], y1 = yi[3 * a + 1], y2 = yi[3 * a + 2];
            c6[0] += y0 * r0; c6[1] += 0.5 * (y0 * r1 + y1 * r0); c6[2] += 0.5 * (y0 * r2 + y2 * r0);
            c6[3] += y1 * r1; c6[4] += 0.5 * (y1 * r2 + y2 * r1); c6[5] += y2 * r2;
            if constexpr (HAT) {
                double ea0 = 0, ea1 = 0;
#pragma unroll
                for (int q = 0; q < NCX; ++q) if (q == a) { ea0 = E[0][q]; ea1 = E[1][q]; }
                er[0] += ea0 * r0; er[1] += ea0 * r1; er[2] += ea0 * r2;
                er[3] += ea1 * r0; er[4] += ea1 * r1; er[5] += ea1 * r2;
            }
        }
        if constexpr (HAT) {
            double h00 = 0, h01 = 0, h11 = 0;
            hat_ece<NCX>(hat.Ccc + (int64_t)d.o_cam[o0 + i] * d.ncolmax * d.ncolmax, nci, E, h00, h01, h11);
            hat_cross(er, B, h00, h01, h11);
            double *g = hat.gscr + (o0 + i - d.giant_start[0]) * 9;
            g[0] = h00; g[1] = h01; g[2] = h11;
#pragma unroll
            for (int q = 0; q < 3; ++q) { g[3 + q] = B[0][q]; g[6 + q] = B[1][q]; }
        }
    }
    block_sum<6>(c6, sh);
    if (t == 0) {
#pragma unroll
        for (int q = 0; q < 6; ++q) c6[q] += vi[q];
        const int64_t zp = d.NS + 3 * (int64_t)pt;
        const bool e0 = d.z_est[zp], e1 = d.z_est[zp + 1], e2 = d.z_est[zp + 2];
        if constexpr (HAT) {
#pragma unroll
            for (int q = 0; q < 6; ++q) cpp[q] = c6[q];
            hat.dCz[zp] = e0 ? c6[0] : 0.0; hat.dCz[zp + 1] = e1 ? c6[3] : 0.0; hat.dCz[zp + 2] = e2 ? c6[5] : 0.0;
        } else {
            double *out = COP + 9 * (int64_t)pt;
            out[0] = e0 ? s02 * c6[0] : 0.0;
            out[1] = out[3] = (e0 && e1) ? s02 * c6[1] : 0.0;
            out[2] = out[6] = (e0 && e2) ? s02 * c6[2] : 0.0;
            out[4] = e1 ? s02 * c6[3] : 0.0;
            out[5] = out[7] = (e1 && e2) ? s02 * c6[4] : 0.0;
            out[8] = e2 ? s02 * c6[5] : 0.0;
        }
    }
    if constexpr (HAT) {
        __syncthreads();
        for (int i = t; i < k; i += BT) {            // (the thread's own observations of phase two: own scratch rows)
            const double *g = hat.gscr + (o0 + i - d.giant_start[0]) * 9;
            const double B[2][3] = {{g[3], g[4], g[5]}, {g[6], g[7], g[8]}};
            hat_finish(cpp, B, g[0], g[1], g[2], hat.qvv + 3 * d.o_row[o0 + i]);
        }
    }
}

}  // namespace dbat
