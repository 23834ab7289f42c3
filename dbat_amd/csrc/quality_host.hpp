// Host side of the image coverage and the marking-residual statistics (kernels: quality.hpp): plan, drivers, C entry
// points.  Included by dbat_core.hip after Core and analysis_host.hpp.
#pragma once

namespace dbat {
// Built by the first call and kept, as the angles' plan: the columns of every image (IP is image-major), the measured
// pixel coordinates in IP order (the observations are structure: dbat_hip_set_values never changes them; the principal
// point is read from io_fixed, which it does change), the index scratch of the images with over QUAL_HULL_CAP points.
struct QualPlan {
    std::vector<int64_t> ip_start;                       // [nc + 1]
    DevBuf<int64_t> d_ip_start, big_off, rad_ip, hull_start, hull_ip, cam_max_ip, max_ip;
    DevBuf<int32_t> big_idx, hull_tmp, hull_n;
    DevBuf<double> ip_uv, lo, hi, rad_max, hull_area, r, e2, cam_ss, cam_max, op_ss, tot;
    EventTimer<1> cov_timer, res_timer;                  // last dbat_hip_coverage, last dbat_hip_residual_stats (kernels only)
    explicit QualPlan(Core &c) {
        const Plan &P = c.P;
        const int64_t no = c.nobs;
        const int nc = P.nc;
        ip_start.assign((size_t)nc + 1, 0);
        for (int64_t o = 0; o < no; ++o) ++ip_start[(size_t)P.o_cam[o] + 1];
        for (int i = 0; i < nc; ++i) ip_start[(size_t)i + 1] += ip_start[i];
        for (int64_t o = 0; o < no; ++o)
            if (P.o_row[o] < ip_start[P.o_cam[o]] || P.o_row[o] >= ip_start[(size_t)P.o_cam[o] + 1])
                throw UsageError{"network quality: the image points are not image-major (the columns of an image must be contiguous, images ascending)"};
        std::vector<int64_t> boff((size_t)nc, 0);
        int64_t nbig = 0;
        for (int i = 0; i < nc; ++i) {
            const int64_t n = ip_start[(size_t)i + 1] - ip_start[i];
            if (n >= ((int64_t)1 << 30)) throw UsageError{"network quality: an image with more than 2^30 points"};
            boff[i] = nbig;
            if (n > QUAL_HULL_CAP) { int64_t m2 = 1; while (m2 < n) m2 <<= 1; nbig += m2; }
        }
        d_ip_start.upload(ip_start); big_off.upload(boff); big_idx.alloc((size_t)std::max<int64_t>(nbig, 1));
        const size_t nc1 = (size_t)std::max(nc, 1), no1 = (size_t)std::max<int64_t>(no, 1);
        ip_uv.alloc(2 * no1);
        hull_tmp.alloc(no1 + nc1); hull_n.alloc(nc1); hull_start.alloc(nc1 + 1); hull_ip.alloc(no1);
        lo.alloc(2 * nc1); hi.alloc(2 * nc1); rad_max.alloc(nc1); rad_ip.alloc(nc1); hull_area.alloc(nc1);
        r.alloc(2 * no1); e2.alloc(no1); cam_ss.alloc(nc1); cam_max.alloc(nc1); cam_max_ip.alloc(nc1);
        op_ss.alloc((size_t)std::max<int64_t>(P.np, 1)); tot.alloc(2); max_ip.alloc(1);
        if (no > 0) c.launch<k_qual_ip_uv>(dim3((unsigned)cdiv(no, 256)), dim3(256), 0, no, c.o_row.p, c.o_uv.p, ip_uv.p);
    }
};
static const char *const QUAL_ONE_RANK = "an image's points are spread over the shards";
static constexpr size_t qual_hull_lds = ((size_t)QUAL_HULL_CAP * 20 + ((size_t)QUAL_HULL_CAP + 1) * 4 + 7) / 8 * 8;

static void coverage(Core &c, QualPlan &qual, double *hlo, double *hhi, double *hrad, int64_t *hrad_ip, double *harea, int64_t *hstart, int64_t *hip_) {
    const int nc = c.P.nc;
    qual.cov_timer.start(c.stream);
    if (nc > 0)
        c.launch<k_qual_hull>(dim3((unsigned)nc), dim3(QUAL_THREADS), qual_hull_lds, qual.d_ip_start.p, qual.ip_uv.p, c.px.p, c.io_fixed.p, c.P.nIOrows,
                              qual.big_idx.p, qual.big_off.p, qual.lo.p, qual.hi.p, qual.rad_max.p, qual.rad_ip.p, qual.hull_area.p,
                              qual.hull_tmp.p, qual.hull_n.p);
    qual.cov_timer.lap(c.stream);
    if (hlo) HIPCHK(hipMemcpyAsync(hlo, qual.lo.p, (size_t)2 * nc * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    if (hhi) HIPCHK(hipMemcpyAsync(hhi, qual.hi.p, (size_t)2 * nc * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    if (hrad) HIPCHK(hipMemcpyAsync(hrad, qual.rad_max.p, (size_t)nc * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    if (hrad_ip) HIPCHK(hipMemcpyAsync(hrad_ip, qual.rad_ip.p, (size_t)nc * sizeof(int64_t), hipMemcpyDeviceToHost, c.stream));
    if (harea) HIPCHK(hipMemcpyAsync(harea, qual.hull_area.p, (size_t)nc * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    std::vector<int32_t> hn((size_t)nc);
    std::vector<int64_t> hs((size_t)nc + 1, 0);
    if (hstart || hip_) HIPCHK(hipMemcpyAsync(hn.data(), qual.hull_n.p, (size_t)nc * sizeof(int32_t), hipMemcpyDeviceToHost, c.stream));
    c.sync();
    qual.cov_timer.read();
    if (!hstart && !hip_) return;
    for (int i = 0; i < nc; ++i) hs[(size_t)i + 1] = hs[i] + hn[i];
    if (hstart) std::copy(hs.begin(), hs.end(), hstart);
    if (!hip_ || hs[nc] == 0) return;
    HIPCHK(hipMemcpyAsync(qual.hull_start.p, hs.data(), ((size_t)nc + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c.stream));
    c.launch<k_qual_hull_pack>(dim3((unsigned)nc), dim3(256), 0, qual.d_ip_start.p, qual.hull_tmp.p, qual.hull_start.p, qual.hull_ip.p);
    HIPCHK(hipMemcpyAsync(hip_, qual.hull_ip.p, (size_t)hs[nc] * sizeof(int64_t), hipMemcpyDeviceToHost, c.stream));
    c.sync();
}

static void residual_stats(Core &c, const PointIndex &ix, QualPlan &qual, int64_t *hcam_n, double *hcam_ss, int64_t *hop_n, double *hop_ss, double *htot,
                           double *hmax, int64_t *hmax_ip) {
    const Plan &P = c.P;
    const int nc = P.nc;
    if (hcam_n) for (int i = 0; i < nc; ++i) hcam_n[i] = qual.ip_start[(size_t)i + 1] - qual.ip_start[i];
    if (hop_n) std::copy(ix.count.begin(), ix.count.end(), hop_n);
    if (!hcam_ss && !hop_ss && !htot && !hmax && !hmax_ip) return;
    const double *zz = c.zt.p;                           // the statistics are taken at zt
    c.prep_cams(zz, c.cams_f.p);
    qual.res_timer.start(c.stream);
    if (c.nobs > 0)
        c.with_model([&](auto M) { with_value<false, true>(c.uv_pre, [&](auto PRE) {
            c.launch<k_residual<M, PRE>>(dim3(c.grid_obs), dim3(256), 0, c.d, zz, c.cams_f.p, c.rpart.p, (double *)nullptr, qual.r.p);
        }); });
    if (nc > 0)
        c.launch<k_qual_cam_res>(dim3((unsigned)nc), dim3(256), 0, qual.d_ip_start.p, qual.r.p, c.px.p, qual.e2.p, qual.cam_ss.p, qual.cam_max.p, qual.cam_max_ip.p);
    if (hop_ss) {
        if (ix.hp0 > 0) c.launch<k_qual_pt_light>(dim3((unsigned)cdiv(ix.hp0, 256)), dim3(256), 0, ix.d_pos.p, c.o_row.p, qual.e2.p, ix.hp0, qual.op_ss.p);
        if (ix.hp1 > ix.hp0) c.launch<k_qual_pt_heavy>(dim3((unsigned)(ix.hp1 - ix.hp0)), dim3(64), 0, ix.d_pos.p, c.o_row.p, qual.e2.p, ix.hp0, qual.op_ss.p);
    }
    c.launch<k_qual_total>(dim3(1), dim3(256), 0, nc, qual.cam_ss.p, qual.cam_max.p, qual.cam_max_ip.p, qual.tot.p, qual.max_ip.p);
    qual.res_timer.lap(c.stream);
    std::vector<double> tmp;
    double tot[2] = {0, 0};
    int64_t mip = -1;
    if (hcam_ss) HIPCHK(hipMemcpyAsync(hcam_ss, qual.cam_ss.p, (size_t)nc * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    if (hop_ss && ix.hp1 > 0) {
        tmp.resize((size_t)ix.hp1);
        HIPCHK(hipMemcpyAsync(tmp.data(), qual.op_ss.p, (size_t)ix.hp1 * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    }
    HIPCHK(hipMemcpyAsync(tot, qual.tot.p, 2 * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipMemcpyAsync(&mip, qual.max_ip.p, sizeof(int64_t), hipMemcpyDeviceToHost, c.stream));
    c.sync();
    if (hop_ss) scatter_points(c, tmp, ix.hp1, 0.0, hop_ss);
    if (htot) *htot = tot[0];
    if (hmax) *hmax = tot[1];
    if (hmax_ip) *hmax_ip = mip;
    qual.res_timer.read();
}
}  // namespace dbat

extern "C" {
int dbat_hip_coverage(dbat_hip_handle *h, double *lo, double *hi, double *rad_max, int64_t *rad_ip, double *hull_area, int64_t *hull_start, int64_t *hull_ip) {
    API_TRY
    if (!h) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    Core &c = *h->core;
    if (!one_rank(c, "coverage", QUAL_ONE_RANK)) return DBAT_HIP_EINVAL;
    DeviceGuard dev_guard(c.device);
    coverage(c, built_once(h->qual, c), lo, hi, rad_max, rad_ip, hull_area, hull_start, hull_ip);
    return DBAT_HIP_OK;
    API_CATCH
}

int dbat_hip_residual_stats(dbat_hip_handle *h, const double *x, int64_t *cam_n, double *cam_ss, int64_t *op_n, double *op_ss,
                            double *total_ss, double *max_e, int64_t *max_ip) {
    API_TRY
    if (!h || !x) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    Core &c = *h->core;
    if (!one_rank(c, "residual statistics", QUAL_ONE_RANK)) return DBAT_HIP_EINVAL;
    DeviceGuard dev_guard(c.device);
    if (cam_ss || op_ss || total_ss || max_e || max_ip) c.x_to_z(x, c.zt.p);
    QualPlan &qual = built_once(h->qual, c);
    residual_stats(c, built_once(h->pts, c), qual, cam_n, cam_ss, op_n, op_ss, total_ss, max_e, max_ip);
    return DBAT_HIP_OK;
    API_CATCH
}

int32_t dbat_hip_quality_hull_cap(void) { return QUAL_HULL_CAP; }

/* Debug / measurement: milliseconds of the kernels of the last dbat_hip_coverage (ms[0]) and of the last
 * dbat_hip_residual_stats (ms[1], the residual pass included) on the handle's stream (device events). */
int dbat_hip_debug_quality_ms(dbat_hip_handle *h, double *ms) {
    if (!h || !ms || !h->qual) { g_err = "no coverage or residual statistics computed on this handle"; return DBAT_HIP_EINVAL; }
    ms[0] = h->qual->cov_timer.ms[0]; ms[1] = h->qual->res_timer.ms[0];
    return DBAT_HIP_OK;
}

/* Host only, one thread (include/dbat_hip.h): the code of the kernel (octagon filter, order, chain scan, shoelace sum
 * of quality.hpp), std::sort in place of the network. */
int dbat_hip_debug_coverage_host(const dbat_hip_problem *prob, double *lo, double *hi, double *rad_max, int64_t *rad_ip,
                                 double *hull_area, int64_t *hull_start, int64_t *hull_ip) {
    API_TRY
    if (!prob) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    if (prob->abi_version != DBAT_HIP_ABI_VERSION) { g_err = "ABI version mismatch"; return DBAT_HIP_EINVAL; }
    const int64_t nc = prob->n_images, no = prob->n_obs;
    if (nc < 0 || no < 0 || (no > 0 && (!prob->ip_cam || !prob->ip_val)) || (nc > 0 && (!prob->IO_val || !prob->px_size))) {
        g_err = "bad problem"; return DBAT_HIP_EINVAL;
    }
    const int R = 5 + prob->nK + prob->nP;
    std::vector<int64_t> start((size_t)nc + 1, 0);
    for (int64_t o = 0; o < no; ++o) {
        if (prob->ip_cam[o] < 0 || prob->ip_cam[o] >= nc || (o > 0 && prob->ip_cam[o] < prob->ip_cam[o - 1])) {
            g_err = "IP.cam out of range or not image-major"; return DBAT_HIP_EINVAL;
        }
        ++start[(size_t)prob->ip_cam[o] + 1];
    }
    for (int64_t c = 0; c < nc; ++c) start[c + 1] += start[c];
    const double nan = std::nan("");
    std::vector<int32_t> idx, stk;
    int64_t nh = 0;
    if (hull_start) hull_start[0] = 0;
    for (int64_t c = 0; c < nc; ++c) {
        const int64_t i0 = start[c];
        const int n = (int)(start[c + 1] - i0);
        const double *uv = prob->ip_val + 2 * i0;
        double l[2] = {nan, nan}, hh[2] = {nan, nan}, rm = nan, area = 0.0;
        int64_t ri = -1;
        int h = 0;
        if (n > 0) {
            double ev[9];
            int ei[9];
            for (int k = 0; k < 9; ++k) { ev[k] = -INFINITY; ei[k] = -1; }
            for (int i = 0; i < n; ++i)
                for (int k = 0; k < 9; ++k) {
                    const double f = k < 8 ? qual_dir(k, uv[2 * i], uv[2 * i + 1])
                                           : qual_radius(uv[2 * i], uv[2 * i + 1], prob->px_size[2 * c], prob->px_size[2 * c + 1],
                                                         prob->IO_val[c * R + 1], prob->IO_val[c * R + 2]);
                    if (ei[k] < 0 || f > ev[k]) { ev[k] = f; ei[k] = i; }
                }
            double eu[8], evv[8];
            for (int k = 0; k < 8; ++k) { eu[k] = uv[2 * ei[k]]; evv[k] = uv[2 * ei[k] + 1]; }
            l[0] = eu[0]; hh[0] = eu[4]; l[1] = evv[2]; hh[1] = evv[6];
            rm = ev[8]; ri = i0 + ei[8];
            QualOct oct;
            qual_oct_build(eu, evv, hh[0] - l[0], hh[1] - l[1], oct);
            idx.clear();
            for (int i = 0; i < n; ++i) if (!qual_oct_inside(oct, uv[2 * i], uv[2 * i + 1])) idx.push_back(i);
            const int ns = (int)idx.size();
            const QualIdxPts p{uv, idx.data()};
            std::sort(idx.begin(), idx.end(), [&](int32_t a, int32_t b) {        // the order of qual_less
                if (uv[2 * a] != uv[2 * b]) return uv[2 * a] < uv[2 * b];
                if (uv[2 * a + 1] != uv[2 * b + 1]) return uv[2 * a + 1] < uv[2 * b + 1];
                return a < b;
            });
            stk.assign((size_t)ns + 1, 0);
            h = qual_hull_chain(p, ns, stk.data());
            area = qual_hull_area(p, stk.data(), h, l[0], l[1]);
            if (hull_ip) for (int j = 0; j < h; ++j) hull_ip[nh + j] = i0 + idx[stk[j]];
        }
        nh += h;
        if (lo) { lo[2 * c] = l[0]; lo[2 * c + 1] = l[1]; }
        if (hi) { hi[2 * c] = hh[0]; hi[2 * c + 1] = hh[1]; }
        if (rad_max) rad_max[c] = rm;
        if (rad_ip) rad_ip[c] = ri;
        if (hull_area) hull_area[c] = area;
        if (hull_start) hull_start[c + 1] = nh;
    }
    return DBAT_HIP_OK;
    API_CATCH
}
}  // extern "C"
