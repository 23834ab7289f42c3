// Image coverage and marking-residual statistics (dbat_hip_coverage, dbat_hip_residual_stats): the numbers behind the
// report's "Photo point coverage" and "Point Marking Residuals" blocks (photogrammetry/coverage.m:113-185,
// file/bundle_result_file.m:630-672) without the dense points x images table.
//
// Both work on the image points in IP column order: IP is image-major, so image c owns the columns
// [ip_start[c], ip_start[c + 1]).  The measured pixel coordinates are kept in that order (ip_uv, scattered once from the
// point-major copy: the camera-major copy holds corrected coordinates when the interior orientation is fixed).
//
//   k_qual_ip_uv      ip_uv[o_row[o]] = measured (u, v) of observation o
//   k_qual_hull       one workgroup per image: exact min / max, the largest radial distance to the principal point, the
//                     convex hull and its area.  The eight extreme points (+-u, +-v, +-u+-v) span an octagon; a point
//                     strictly inside it (by more than any rounding of the test) is no hull vertex and is dropped
//                     (Akl-Toussaint).  The survivors are sorted by (u, v, column) with a bitonic network and a monotone
//                     scan (Andrew) builds the lower and the upper chain: every candidate is pushed once per chain and
//                     popped at most once, so the scan ends after at most 4 m steps whatever the orientation tests say.
//                     At most QUAL_HULL_CAP survivors are sorted in LDS; more are sorted as indices in global memory by
//                     the same workgroup with the same code, the chain's stack in global memory as well.
//                     LIMITATION: the chain scan and the shoelace sum run on ONE thread of the workgroup, about 4 m
//                     dependent steps for m survivors.  In LDS (m <= QUAL_HULL_CAP) that is short beside the sort; on
//                     the global path every step is a dependent global read, and the network re-reads (u, v) through
//                     the indices.  That path is correct and bounded but has been timed only on circles of 4097 and
//                     8193 points: an image with 10^5 or more boundary candidates serialises on that one lane.
//   k_qual_hull_pack  the vertex lists, packed (hull_start) as IP columns
//   k_qual_cam_res    one workgroup per image: e^2 of every image point (pixels), their sum in a fixed order, the largest
//   k_qual_pt_light   a thread per tiled point: sum of e^2 over its observations in the plan's point-major order
//   k_qual_pt_heavy   a wave per heavy / giant point
//   k_qual_total      the sum over the images and the overall maximum
// All arithmetic is f64, every sum has a fixed order, no atomics on floating-point values: two runs give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>

#include "model.hpp"

namespace dbat {

constexpr int QUAL_HULL_CAP = 4096;    // candidates of one image sorted in LDS: (u, v, column, stack) = 24 bytes each
constexpr int QUAL_THREADS = 1024;
constexpr int32_t QUAL_PAD = 0x7fffffff;   // padding of the sort network: sorts last

// twice the signed area of the triangle (a, b, c): > 0 for a left turn
DBAT_HD double qual_cross(double au, double av, double bu, double bv, double cu, double cv) {
    return __builtin_fma(bu - au, cv - av, -((bv - av) * (cu - au)));
}

// radial distance of pixel (u, v) to the principal point, mm (coverage.m:133-156: PP \ (S \ [u; v; 1]))
DBAT_HD double qual_radius(double u, double v, double pxu, double pxv, double ppx, double ppy) {
    const double x = u * pxu - ppx, y = -v * pxv - ppy;
    return sqrt(__builtin_fma(x, x, y * y));
}

// the value direction k of the octagon maximises: W, SW, S, SE, E, NE, N, NW (counter-clockwise)
DBAT_HD double qual_dir(int k, double u, double v) {
    switch (k) {
    case 0: return -u;
    case 1: return -u - v;
    case 2: return -v;
    case 3: return u - v;
    case 4: return u;
    case 5: return u + v;
    case 6: return v;
    default: return v - u;
    }
}

// The octagon of the extreme points: its distinct consecutive vertices (nv of them) and the margin of the test.
struct QualOct {
    double u[8], v[8];
    double tol;
    int nv;
};

// eu, ev: the eight extreme points in the order of qual_dir; W x H: the bounding box
DBAT_HD void qual_oct_build(const double *eu, const double *ev, double W, double H, QualOct &o) {
    o.nv = 0;
    for (int k = 0; k < 8; ++k) {
        if (o.nv > 0 && eu[k] == o.u[o.nv - 1] && ev[k] == o.v[o.nv - 1]) continue;
        o.u[o.nv] = eu[k]; o.v[o.nv] = ev[k]; ++o.nv;
    }
    if (o.nv > 1 && o.u[o.nv - 1] == o.u[0] && o.v[o.nv - 1] == o.v[0]) --o.nv;
    // the rounding of one test is below 4 eps W H (differences of coordinates inside the box, one product pair)
    o.tol = 0x1p-44 * W * H;
}

// strictly inside the octagon by more than the margin: not a vertex of the hull
DBAT_HD bool qual_oct_inside(const QualOct &o, double u, double v) {
    if (o.nv < 3) return false;
    for (int k = 0; k < o.nv; ++k) {
        const int k1 = k + 1 < o.nv ? k + 1 : 0;
        if (!(qual_cross(o.u[k], o.v[k], o.u[k1], o.v[k1], u, v) > o.tol)) return false;
    }
    return true;
}

// Candidates by index into the image's (u, v) pairs: idx[k] = column of the image (QUAL_PAD: padding)
struct QualIdxPts {
    const double *uv;
    int32_t *idx;
    DBAT_HD double u(int k) const { return idx[k] == QUAL_PAD ? INFINITY : uv[2 * (int64_t)idx[k]]; }
    DBAT_HD double v(int k) const { return idx[k] == QUAL_PAD ? INFINITY : uv[2 * (int64_t)idx[k] + 1]; }
    DBAT_HD int32_t id(int k) const { return idx[k]; }
    DBAT_HD void swap(int a, int b) const { const int32_t t = idx[a]; idx[a] = idx[b]; idx[b] = t; }
};

// Candidates with their coordinates beside them (LDS)
struct QualValPts {
    double *pu, *pv;
    int32_t *idx;
    DBAT_HD double u(int k) const { return pu[k]; }
    DBAT_HD double v(int k) const { return pv[k]; }
    DBAT_HD int32_t id(int k) const { return idx[k]; }
    DBAT_HD void swap(int a, int b) const {
        const double tu = pu[a], tv = pv[a]; const int32_t t = idx[a];
        pu[a] = pu[b]; pv[a] = pv[b]; idx[a] = idx[b];
        pu[b] = tu; pv[b] = tv; idx[b] = t;
    }
};

// (u, v, column) of candidate a before that of candidate b: a strict total order (columns are distinct)
template <class A>
DBAT_HD bool qual_less(const A &p, int a, int b) {
    const double ua = p.u(a), ub = p.u(b);
    if (ua != ub) return ua < ub;
    const double va = p.v(a), vb = p.v(b);
    if (va != vb) return va < vb;
    return p.id(a) < p.id(b);
}

// Monotone chain over m candidates sorted by qual_less.  stk (m + 1 entries) receives the positions of the hull's
// vertices: counter-clockwise from the lowest (u, v), strictly extreme points only, of equal points the lowest column;
// fewer than three distinct points: those points.  Returns their number.  Bounded: every position is pushed once per
// chain and every pop removes a push.
template <class A>
DBAT_HD int qual_hull_chain(const A &p, int m, int32_t *stk) {
    if (m <= 0) return 0;
    int k = 0, last = 0;
    for (int i = 0; i < m; ++i) {
        if (i > 0 && p.u(i) == p.u(i - 1) && p.v(i) == p.v(i - 1)) continue;     // a copy of the point before it
        while (k >= 2 && !(qual_cross(p.u(stk[k - 2]), p.v(stk[k - 2]), p.u(stk[k - 1]), p.v(stk[k - 1]), p.u(i), p.v(i)) > 0)) --k;
        stk[k++] = i;
        last = i;
    }
    if (k == 1) return 1;
    const int t = k + 1;
    for (int i = last - 1; i >= 0; --i) {
        if (i > 0 && p.u(i) == p.u(i - 1) && p.v(i) == p.v(i - 1)) continue;
        while (k >= t && !(qual_cross(p.u(stk[k - 2]), p.v(stk[k - 2]), p.u(stk[k - 1]), p.v(stk[k - 1]), p.u(i), p.v(i)) > 0)) --k;
        stk[k++] = i;
    }
    return k - 1;                                                                // (the last one is the first again)
}

// Shoelace sum over the h vertices, coordinates relative to (lu, lv): px^2, 0 for fewer than three vertices
template <class A>
DBAT_HD double qual_hull_area(const A &p, const int32_t *stk, int h, double lu, double lv) {
    if (h < 3) return 0.0;
    double s = 0.0;
    for (int j = 0; j < h; ++j) {
        const int a = stk[j], b = stk[j + 1 < h ? j + 1 : 0];
        const double xa = p.u(a) - lu, ya = p.v(a) - lv, xb = p.u(b) - lu, yb = p.v(b) - lv;
        s += __builtin_fma(xa, yb, -(xb * ya));
    }
    return 0.5 * s;
}

#if defined(__HIPCC__)

__global__ __launch_bounds__(256) void k_qual_ip_uv(int64_t nobs, const int64_t *__restrict__ o_row, const double *__restrict__ o_uv,
                                                    double *__restrict__ ip_uv) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= nobs) return;
    const int64_t i = o_row[o];
    ip_uv[2 * i] = o_uv[2 * o]; ip_uv[2 * i + 1] = o_uv[2 * o + 1];
}

// (value, index) with the largest value over the workgroup, ties to the lowest index; every thread receives it.
// sv / si: one entry per wave.  (Order-independent: a maximum with a total tie rule.)
__device__ __forceinline__ void qual_block_argmax(double &val, int32_t &idx, double *sv, int32_t *si) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(val, off, 64);
        const int32_t oi = __shfl_xor(idx, off, 64);
        if (oi >= 0 && (idx < 0 || ov > val || (ov == val && oi < idx))) { val = ov; idx = oi; }
    }
    const int nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = val; si[threadIdx.x >> 6] = idx; }
    __syncthreads();
    val = sv[0]; idx = si[0];
    for (int w = 1; w < nw; ++w) {
        const double ov = sv[w];
        const int32_t oi = si[w];
        if (oi >= 0 && (idx < 0 || ov > val || (ov == val && oi < idx))) { val = ov; idx = oi; }
    }
}

__device__ __forceinline__ int qual_block_sum_int(int v, int32_t *si) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    const int nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) si[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
    for (int w = 0; w < nw; ++w) s += si[w];
    return s;
}

// ascending bitonic network over m2 (a power of two) candidates
template <class A>
__device__ __forceinline__ void qual_bitonic(const A &p, int m2) {
    for (int k = 2; k <= m2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < m2; t += blockDim.x) {
                const int x = t ^ j;
                if (x > t) {
                    const bool up = (t & k) == 0;
                    if (qual_less(p, x, t) == up) p.swap(t, x);
                }
            }
            __syncthreads();
        }
}

// Image c = blockIdx.x: columns [ip_start[c], ip_start[c + 1]).  Dynamic LDS: QUAL_HULL_CAP (u, v, column) and
// QUAL_HULL_CAP + 1 stack entries.  big_idx + big_off[c]: the image's index scratch of the global path (a power of
// two >= its points; only images with more than QUAL_HULL_CAP points have one).  hull_tmp + ip_start[c] + c: the
// image's vertex list (columns of the image), hull_n[c] their number.
__global__ __launch_bounds__(QUAL_THREADS) void k_qual_hull(const int64_t *__restrict__ ip_start, const double *__restrict__ ip_uv,
                                                            const double *__restrict__ px, const double *__restrict__ io_val, int nIOrows,
                                                            int32_t *__restrict__ big_idx, const int64_t *__restrict__ big_off,
                                                            double *__restrict__ lo, double *__restrict__ hi, double *__restrict__ rad_max,
                                                            int64_t *__restrict__ rad_ip, double *__restrict__ hull_area,
                                                            int32_t *__restrict__ hull_tmp, int32_t *__restrict__ hull_n) {
    extern __shared__ double qual_lds[];
    __shared__ double sv[QUAL_THREADS / 64];
    __shared__ int32_t si[QUAL_THREADS / 64];
    __shared__ QualOct oct;
    __shared__ double ext_u[8], ext_v[8];
    __shared__ int32_t fill, hcount;
    double *su = qual_lds, *sw = su + QUAL_HULL_CAP;
    int32_t *sid = reinterpret_cast<int32_t *>(sw + QUAL_HULL_CAP), *sstk = sid + QUAL_HULL_CAP;
    const int c = blockIdx.x;
    const int64_t i0 = ip_start[c];
    const int n = (int)(ip_start[c + 1] - i0);
    const double *uv = ip_uv + 2 * i0;
    int32_t *out = hull_tmp + i0 + c;
    if (n == 0) {
        if (threadIdx.x == 0) {
            const double nan = __builtin_nan("");
            lo[2 * c] = lo[2 * c + 1] = hi[2 * c] = hi[2 * c + 1] = nan;
            rad_max[c] = nan; rad_ip[c] = -1; hull_area[c] = 0.0; hull_n[c] = 0;
        }
        return;
    }
    // ---- the eight extreme points and the largest radius
    const double pxu = px[2 * c], pxv = px[2 * c + 1];
    const double ppx = io_val[(int64_t)c * nIOrows + 1], ppy = io_val[(int64_t)c * nIOrows + 2];
    double ev[9];
    int32_t ei[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) { ev[k] = -INFINITY; ei[k] = -1; }
    for (int i = threadIdx.x; i < n; i += QUAL_THREADS) {
        const double u = uv[2 * (int64_t)i], v = uv[2 * (int64_t)i + 1];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const double f = k < 8 ? qual_dir(k, u, v) : qual_radius(u, v, pxu, pxv, ppx, ppy);
            if (ei[k] < 0 || f > ev[k]) { ev[k] = f; ei[k] = i; }            // (ascending i: ties keep the lowest)
        }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) qual_block_argmax(ev[k], ei[k], sv, si);
    if (threadIdx.x < 8) {
        int32_t e = ei[0];                                                   // (every thread holds all nine)
#pragma unroll
        for (int k = 1; k < 8; ++k) if ((int)threadIdx.x == k) e = ei[k];
        ext_u[threadIdx.x] = uv[2 * (int64_t)e]; ext_v[threadIdx.x] = uv[2 * (int64_t)e + 1];
    }
    __syncthreads();
    const double lu = ext_u[0], hu = ext_u[4], lv = ext_v[2], hv = ext_v[6];
    if (threadIdx.x == 0) {
        lo[2 * c] = lu; lo[2 * c + 1] = lv; hi[2 * c] = hu; hi[2 * c + 1] = hv;
        rad_max[c] = ev[8]; rad_ip[c] = i0 + ei[8];
        qual_oct_build(ext_u, ext_v, hu - lu, hv - lv, oct);
        fill = 0;
    }
    __syncthreads();
    // ---- the candidates: everything not strictly inside the octagon
    int mine = 0;
    for (int i = threadIdx.x; i < n; i += QUAL_THREADS)
        if (!qual_oct_inside(oct, uv[2 * (int64_t)i], uv[2 * (int64_t)i + 1])) ++mine;
    const int ns = qual_block_sum_int(mine, si);
    int m2 = 1;
    while (m2 < ns) m2 <<= 1;
    const bool big = ns > QUAL_HULL_CAP;                                     // (then n > QUAL_HULL_CAP: the image has its scratch)
    int32_t *gidx = big ? big_idx + big_off[c] : sid;
    // (the slots are handed out by an integer counter: the order of arrival does not matter, the sort's order is total)
    for (int i = threadIdx.x; i < n; i += QUAL_THREADS) {
        const double u = uv[2 * (int64_t)i], v = uv[2 * (int64_t)i + 1];
        if (qual_oct_inside(oct, u, v)) continue;
        const int slot = atomicAdd(&fill, 1);
        gidx[slot] = i;
        if (!big) { su[slot] = u; sw[slot] = v; }
    }
    for (int t = ns + threadIdx.x; t < m2; t += QUAL_THREADS) {
        gidx[t] = QUAL_PAD;
        if (!big) { su[t] = INFINITY; sw[t] = INFINITY; }
    }
    __syncthreads();
    int h;
    if (!big) {
        const QualValPts p{su, sw, sid};
        qual_bitonic(p, m2);
        if (threadIdx.x == 0) {
            h = qual_hull_chain(p, ns, sstk);
            hull_area[c] = qual_hull_area(p, sstk, h, lu, lv);
            hull_n[c] = h; hcount = h;
        }
        __syncthreads();
        h = hcount;
        for (int j = threadIdx.x; j < h; j += QUAL_THREADS) out[j] = sid[sstk[j]];
    } else {
        const QualIdxPts p{uv, gidx};
        qual_bitonic(p, m2);
        if (threadIdx.x == 0) {
            h = qual_hull_chain(p, ns, out);                                 // (n + 1 entries: the stack never holds more than ns + 1)
            hull_area[c] = qual_hull_area(p, out, h, lu, lv);
            hull_n[c] = h; hcount = h;
        }
        __syncthreads();
        h = hcount;
        for (int j = threadIdx.x; j < h; j += QUAL_THREADS) { const int32_t pos = out[j]; out[j] = gidx[pos]; }
    }
}

__global__ __launch_bounds__(256) void k_qual_hull_pack(const int64_t *__restrict__ ip_start, const int32_t *__restrict__ hull_tmp,
                                                        const int64_t *__restrict__ hull_start, int64_t *__restrict__ hull_ip) {
    const int c = blockIdx.x;
    const int64_t i0 = ip_start[c], h0 = hull_start[c];
    const int h = (int)(hull_start[c + 1] - h0);
    const int32_t *src = hull_tmp + i0 + c;
    for (int j = threadIdx.x; j < h; j += 256) hull_ip[h0 + j] = i0 + src[j];
}

// sum over the 256 threads in a fixed order (valid in every thread); s: 4 doubles
__device__ __forceinline__ double qual_block_sum(double v, double *s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    return (s[0] + s[1]) + (s[2] + s[3]);
}

// image c = blockIdx.x: e2[i] = |r_i / pxSize|^2 of its columns (r: mm, two rows per column), their sum, the largest
__global__ __launch_bounds__(256) void k_qual_cam_res(const int64_t *__restrict__ ip_start, const double *__restrict__ r,
                                                      const double *__restrict__ px, double *__restrict__ e2,
                                                      double *__restrict__ cam_ss, double *__restrict__ cam_max, int64_t *__restrict__ cam_max_ip) {
    __shared__ double sv[4];
    __shared__ int32_t si[4];
    const int c = blockIdx.x;
    const int64_t i0 = ip_start[c];
    const int n = (int)(ip_start[c + 1] - i0);
    const double iu = px[2 * c], iv = px[2 * c + 1];
    double s = 0.0, mx = -INFINITY;
    int32_t mi = -1;
    for (int i = threadIdx.x; i < n; i += 256) {
        const double a = r[2 * (i0 + i)] / iu, b = r[2 * (i0 + i) + 1] / iv;
        const double e = __builtin_fma(a, a, b * b);
        e2[i0 + i] = e;
        s += e;
        if (mi < 0 || e > mx) { mx = e; mi = i; }
    }
    s = qual_block_sum(s, sv);
    qual_block_argmax(mx, mi, sv, si);
    if (threadIdx.x == 0) { cam_ss[c] = s; cam_max[c] = mx; cam_max_ip[c] = mi < 0 ? -1 : i0 + mi; }
}

// points [0, npts) of the processing order (tiled: few rays each): out[rank] = sum of e2 over the point's observations
__global__ __launch_bounds__(256) void k_qual_pt_light(const int64_t *__restrict__ pt_pos, const int64_t *__restrict__ o_row,
                                                       const double *__restrict__ e2, int32_t npts, double *__restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= npts) return;
    double s = 0.0;
    for (int64_t o = pt_pos[r]; o < pt_pos[r + 1]; ++o) s += e2[o_row[o]];
    out[r] = s;
}

// point p0 + blockIdx.x of the processing order, any number of rays: one wave, lane-strided partial sums, shuffle tree
__global__ __launch_bounds__(64) void k_qual_pt_heavy(const int64_t *__restrict__ pt_pos, const int64_t *__restrict__ o_row,
                                                      const double *__restrict__ e2, int32_t p0, double *__restrict__ out) {
    const int64_t r = (int64_t)p0 + blockIdx.x;
    double s = 0.0;
    for (int64_t o = pt_pos[r] + threadIdx.x; o < pt_pos[r + 1]; o += 64) s += e2[o_row[o]];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (threadIdx.x == 0) out[r] = s;
}

// one workgroup: tot[0] = sum of cam_ss, tot[1] = the largest e (not squared), *max_ip its column (-1: no image point)
__global__ __launch_bounds__(256) void k_qual_total(int nc, const double *__restrict__ cam_ss, const double *__restrict__ cam_max,
                                                    const int64_t *__restrict__ cam_max_ip, double *__restrict__ tot, int64_t *__restrict__ max_ip) {
    __shared__ double sv[4];
    __shared__ int32_t si[4];
    double s = 0.0, mx = -INFINITY;
    int32_t mc = -1;
    for (int c = threadIdx.x; c < nc; c += 256) {
        s += cam_ss[c];
        if (cam_max_ip[c] >= 0 && (mc < 0 || cam_max[c] > mx)) { mx = cam_max[c]; mc = c; }   // (columns ascend with the image)
    }
    s = qual_block_sum(s, sv);
    qual_block_argmax(mx, mc, sv, si);
    if (threadIdx.x == 0) {
        tot[0] = s;
        tot[1] = mc < 0 ? __builtin_nan("") : sqrt(mx);
        *max_ip = mc < 0 ? -1 : cam_max_ip[mc];
    }
}

#endif  // __HIPCC__

}  // namespace dbat
