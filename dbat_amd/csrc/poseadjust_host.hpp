// Host side of the robust resection (kernels: resect_ransac.hpp, poseadjust.hpp): the C entry points
// dbat_hip_resect_ransac and dbat_hip_poseadjust.  Included by dbat_core.hip after Core; the calls take no handle and no
// plan.
#pragma once

namespace dbat {
// k_resect_ransac [0] and k_poseadjust [1] of the last call of each on this thread
using ResectRobustClock = KernelClock<struct ResectRobustFamily, 2>;

// The checks both entry points share, before any device call: the ranges, and that every point that may be used is finite.
static void rr_check_points(const char *who, int32_t n_images, const int64_t *pt_start, const double *X, const double *xn,
                            const uint8_t *use) {
    check_ranges(who, "pt_start", n_images, pt_start, (int64_t)1 << 29, "more than 2^29 points in one camera");
    const int64_t total = pt_start[n_images];
    if (total > 0 && (!X || !xn)) throw UsageError{"null argument"};
    check_used_points(who, total, use, X, xn);
}
}  // namespace dbat

extern "C" {
int dbat_hip_resect_ransac(int32_t device, int32_t n_images, const int64_t *pt_start, const double *X, const double *xn,
                           const uint8_t *use, const int64_t *smp_start, const int32_t *smp, const double *thr2, double *P,
                           int32_t *stats, uint8_t *inlier, double *ssq) {
    API_TRY
    if (n_images < 0 || !pt_start || !smp_start || !P || !stats || !ssq || (n_images > 0 && !thr2)) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    rr_check_points("resect_ransac", n_images, pt_start, X, xn, use);
    const int64_t total = pt_start[n_images];
    if (total > 0 && !inlier) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    check_ranges_start("resect_ransac", smp_start);
    for (int32_t c = 0; c < n_images; ++c) {              // camera by camera: its samples, then its threshold
        check_range("resect_ransac", "smp_start", smp_start, c, (int64_t)1 << 31, "more than 2^31 samples in one camera");
        if (!(thr2[c] > 0) || !std::isfinite(thr2[c])) refuse("resect_ransac", "thr2 of camera " + std::to_string(c) + " is not positive and finite");
    }
    const int64_t nsmp = smp_start[n_images];
    if (nsmp > 0 && !smp) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    for (int32_t c = 0; c < n_images; ++c) {
        const int64_t npt = pt_start[c + 1] - pt_start[c];
        for (int64_t h = smp_start[c]; h < smp_start[c + 1]; ++h) {       // any index outside comes before any that repeats
            const int32_t *t = smp + 3 * h;
            if (t[0] < 0 || t[1] < 0 || t[2] < 0 || t[0] >= npt || t[1] >= npt || t[2] >= npt)
                refuse("resect_ransac", "sample " + std::to_string(h) + " has an index outside the camera's points");
            if (t[0] == t[1] || t[0] == t[2] || t[1] == t[2]) refuse("resect_ransac", "sample " + std::to_string(h) + " repeats an index");
        }
    }
    BatchDevice dev(device);
    if (n_images == 0) return DBAT_HIP_OK;
    DevBuf<int64_t> dps, dss;
    DevBuf<double> dX, dx, dt, dP, dq;
    DevBuf<uint8_t> duse, din;
    DevBuf<int32_t> dsm, dst;
    dps.upload(pt_start, (size_t)n_images + 1); dss.upload(smp_start, (size_t)n_images + 1);
    dX.upload(X, (size_t)3 * total); dx.upload(xn, (size_t)2 * total); dsm.upload(smp, (size_t)3 * nsmp);
    if (use) duse.upload(use, (size_t)total);
    dt.upload(thr2, (size_t)n_images);
    dP.alloc((size_t)12 * n_images); dst.alloc((size_t)4 * n_images); dq.alloc((size_t)n_images); din.alloc((size_t)total);
    EventTimer<1> ev;
    ResectRobustClock::start(ev, dev.st);
    launch<k_resect_ransac>(dim3((unsigned)n_images), dim3(RR_WG), 0, dev.st, (const int64_t *)dps.p, (const double *)dX.p, (const double *)dx.p,
                            (const uint8_t *)(use ? duse.p : nullptr), (const int64_t *)dss.p, (const int32_t *)dsm.p, (const double *)dt.p,
                            dP.p, dst.p, din.p, dq.p);
    ev.lap(dev.st);
    dP.download(P); dst.download(stats); dq.download(ssq); din.download(inlier);
    ResectRobustClock::ms[0] = ev.read();
    return DBAT_HIP_OK;
    API_CATCH
}

int dbat_hip_poseadjust(int32_t device, int32_t n_images, const int64_t *pt_start, const double *X, const double *xn,
                        const uint8_t *use, const double *w, const dbat_hip_pair_options *opt, double *P, uint8_t *used,
                        double *dstat, int32_t *istat, double *Q, double *res) {
    API_TRY
    if (n_images < 0 || !pt_start || !opt || !P || !dstat || !istat || !Q) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    check_pair_options("poseadjust", opt);
    if (!(opt->min_angle == 0)) { g_err = "poseadjust: min_angle must be 0"; return DBAT_HIP_EINVAL; }
    rr_check_points("poseadjust", n_images, pt_start, X, xn, use);
    const int64_t total = pt_start[n_images];
    if (total > 0 && !used) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    check_weights("poseadjust", "point", total, w);
    for (int32_t p = 0; p < n_images; ++p) check_pose("poseadjust", "P", "camera", p, P + 12 * (size_t)p);
    BatchDevice dev(device);
    if (n_images == 0) return DBAT_HIP_OK;
    DevBuf<int64_t> dps;
    DevBuf<double> dX, dx, dw, dP, dds, dQ, dres;
    DevBuf<uint8_t> duse, dused;
    DevBuf<int32_t> dis;
    const size_t tot1 = (size_t)total;                    // may be 0: every camera then ends with code 4
    dps.upload(pt_start, (size_t)n_images + 1);
    dX.upload(X, 3 * tot1); dx.upload(xn, 2 * tot1);
    if (w) dw.upload(w, 2 * tot1);
    if (use) duse.upload(use, tot1);
    dP.upload(P, (size_t)12 * n_images); dused.alloc(tot1);
    dds.alloc((size_t)4 * n_images); dis.alloc((size_t)4 * n_images); dQ.alloc((size_t)36 * n_images);
    if (res && total > 0) dres.alloc(2 * tot1);
    EventTimer<1> ev;
    ResectRobustClock::start(ev, dev.st);
    launch<k_poseadjust>(dim3((unsigned)n_images), dim3(PO_WAVE), 0, dev.st, (const int64_t *)dps.p, (const double *)dX.p, (const double *)dx.p,
                         (const uint8_t *)(use ? duse.p : nullptr), (const double *)(w ? dw.p : nullptr), (int)opt->max_iter,
                         opt->conv_tol * opt->conv_tol, dP.p, dused.p, dds.p, dis.p, dQ.p, (double *)dres.p);
    ev.lap(dev.st);
    // a camera of fewer than three used points returns P as given: the kernel does not write it
    dP.download(P); dis.download(istat); dds.download(dstat); dQ.download(Q);
    dused.download(used); dres.download(res);             // (empty without points; dres without res)
    ResectRobustClock::ms[1] = ev.read();
    return DBAT_HIP_OK;
    API_CATCH
}

/* Debug / measurement: dbat_hip_debug_resect_robust_timing(1) makes dbat_hip_resect_ransac and dbat_hip_poseadjust on this
 * thread bracket their kernels with device events (off by default: a product call creates none);
 * dbat_hip_debug_resect_robust_ms then gives the milliseconds of the last k_resect_ransac [0] and k_poseadjust [1]. */
int dbat_hip_debug_resect_robust_timing(int32_t on) { return ResectRobustClock::set(on); }
int dbat_hip_debug_resect_robust_ms(double *ms) { return ResectRobustClock::get(ms); }
}  // extern "C"
