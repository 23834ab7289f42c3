// Host side of the robust resection (kernels: resect_ransac.hpp, poseadjust.hpp): the C entry points
// dbat_hip_resect_ransac and dbat_hip_poseadjust.  Included by dbat_core.hip after Core; the calls take no handle and no
// plan.
#pragma once

namespace dbat {
// device events around k_resect_ransac [0] and k_poseadjust [1] of the last call of each on this thread; 0: not launched
static thread_local double g_resect_robust_ms[2] = {0, 0};
static thread_local bool g_resect_robust_timing = false;  // dbat_hip_debug_resect_robust_timing: off, no event is created

// The checks both entry points share, before any device call: the ranges, and that every point that may be used is finite.
static int rr_check_points(const char *who, int32_t n_images, const int64_t *pt_start, const double *X, const double *xn,
                           const uint8_t *use) {
    const std::string w = who;
    if (pt_start[0] != 0) { g_err = w + ": ranges must start at 0"; return DBAT_HIP_EINVAL; }
    for (int32_t c = 0; c < n_images; ++c) {
        if (pt_start[c + 1] < pt_start[c]) { g_err = w + ": the ranges of pt_start must ascend"; return DBAT_HIP_EINVAL; }
        if (pt_start[c + 1] - pt_start[c] >= (int64_t)1 << 29) { g_err = w + ": more than 2^29 points in one camera"; return DBAT_HIP_EINVAL; }
    }
    const int64_t total = pt_start[n_images];
    if (total > 0 && (!X || !xn)) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    for (int64_t g = 0; g < total; ++g)
        if ((!use || use[g]) && !(std::isfinite(X[3 * g]) && std::isfinite(X[3 * g + 1]) && std::isfinite(X[3 * g + 2]) &&
                                  std::isfinite(xn[2 * g]) && std::isfinite(xn[2 * g + 1]))) {
            g_err = w + ": point " + std::to_string(g) + " is to be used and is not finite"; return DBAT_HIP_EINVAL;
        }
    return DBAT_HIP_OK;
}
}  // namespace dbat

extern "C" {
int dbat_hip_resect_ransac(int32_t device, int32_t n_images, const int64_t *pt_start, const double *X, const double *xn,
                           const uint8_t *use, const int64_t *smp_start, const int32_t *smp, const double *thr2, double *P,
                           int32_t *stats, uint8_t *inlier, double *ssq) {
    API_TRY
    if (n_images < 0 || !pt_start || !smp_start || !P || !stats || !ssq || (n_images > 0 && !thr2)) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    if (int rc = rr_check_points("resect_ransac", n_images, pt_start, X, xn, use)) return rc;
    const int64_t total = pt_start[n_images];
    if (total > 0 && !inlier) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    if (smp_start[0] != 0) { g_err = "resect_ransac: ranges must start at 0"; return DBAT_HIP_EINVAL; }
    for (int32_t c = 0; c < n_images; ++c) {
        if (smp_start[c + 1] < smp_start[c]) { g_err = "resect_ransac: the ranges of smp_start must ascend"; return DBAT_HIP_EINVAL; }
        if (smp_start[c + 1] - smp_start[c] >= (int64_t)1 << 31) { g_err = "resect_ransac: more than 2^31 samples in one camera"; return DBAT_HIP_EINVAL; }
        if (!(thr2[c] > 0) || !std::isfinite(thr2[c])) { g_err = "resect_ransac: thr2 of camera " + std::to_string(c) + " is not positive and finite"; return DBAT_HIP_EINVAL; }
    }
    const int64_t nsmp = smp_start[n_images];
    if (nsmp > 0 && !smp) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    for (int32_t c = 0; c < n_images; ++c) {
        const int64_t npt = pt_start[c + 1] - pt_start[c];
        for (int64_t h = smp_start[c]; h < smp_start[c + 1]; ++h) {
            const int32_t *t = smp + 3 * h;
            if (t[0] < 0 || t[1] < 0 || t[2] < 0 || t[0] >= npt || t[1] >= npt || t[2] >= npt) {
                g_err = "resect_ransac: sample " + std::to_string(h) + " has an index outside the camera's points"; return DBAT_HIP_EINVAL;
            }
            if (t[0] == t[1] || t[0] == t[2] || t[1] == t[2]) { g_err = "resect_ransac: sample " + std::to_string(h) + " repeats an index"; return DBAT_HIP_EINVAL; }
        }
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_err = "no HIP device: the dbat_hip core has no CPU path"; return DBAT_HIP_EDEVICE; }
    if (device < 0 || device >= ndev) { g_err = "bad device index"; return DBAT_HIP_EINVAL; }
    if (n_images == 0) return DBAT_HIP_OK;
    DeviceGuard dev_guard(device);
    const hipStream_t st = nullptr;
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
    if (g_resect_robust_timing) ev.start(st);
    launch<k_resect_ransac>(dim3((unsigned)n_images), dim3(RR_WG), 0, st, (const int64_t *)dps.p, (const double *)dX.p, (const double *)dx.p,
                            (const uint8_t *)(use ? duse.p : nullptr), (const int64_t *)dss.p, (const int32_t *)dsm.p, (const double *)dt.p,
                            dP.p, dst.p, din.p, dq.p);
    ev.lap(st);
    HIPCHK(hipMemcpy(P, dP.p, (size_t)12 * n_images * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(stats, dst.p, (size_t)4 * n_images * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ssq, dq.p, (size_t)n_images * sizeof(double), hipMemcpyDeviceToHost));
    if (total > 0) HIPCHK(hipMemcpy(inlier, din.p, (size_t)total, hipMemcpyDeviceToHost));
    g_resect_robust_ms[0] = ev.read();
    return DBAT_HIP_OK;
    API_CATCH
}

int dbat_hip_poseadjust(int32_t device, int32_t n_images, const int64_t *pt_start, const double *X, const double *xn,
                        const uint8_t *use, const double *w, const dbat_hip_pair_options *opt, double *P, uint8_t *used,
                        double *dstat, int32_t *istat, double *Q, double *res) {
    API_TRY
    if (n_images < 0 || !pt_start || !opt || !P || !dstat || !istat || !Q) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    if (opt->max_iter < 1 || opt->max_iter > 200) { g_err = "poseadjust: max_iter must be 1 .. 200"; return DBAT_HIP_EINVAL; }
    if (!(opt->conv_tol > 0) || !std::isfinite(opt->conv_tol)) { g_err = "poseadjust: conv_tol must be positive"; return DBAT_HIP_EINVAL; }
    if (!(opt->min_angle == 0)) { g_err = "poseadjust: min_angle must be 0"; return DBAT_HIP_EINVAL; }
    if (int rc = rr_check_points("poseadjust", n_images, pt_start, X, xn, use)) return rc;
    const int64_t total = pt_start[n_images];
    if (total > 0 && !used) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    if (w)
        for (int64_t i = 0; i < 2 * total; ++i)
            if (!std::isfinite(w[i]) || !(w[i] > 0)) { g_err = "poseadjust: weight of point " + std::to_string(i / 2) + " is not positive and finite"; return DBAT_HIP_EINVAL; }
    for (int32_t p = 0; p < n_images; ++p) {
        const double *Pp = P + 12 * (size_t)p;
        for (int i = 0; i < 12; ++i)
            if (!std::isfinite(Pp[i])) { g_err = "poseadjust: P of camera " + std::to_string(p) + " is not finite"; return DBAT_HIP_EINVAL; }
        double dev = 0;
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b)
                dev = std::max(dev, std::fabs(Pp[3 * a] * Pp[3 * b] + Pp[3 * a + 1] * Pp[3 * b + 1] + Pp[3 * a + 2] * Pp[3 * b + 2] - (a == b ? 1.0 : 0.0)));
        if (dev > 1e-6 || al_det3(Pp) < 0) { g_err = "poseadjust: R of camera " + std::to_string(p) + " is not a rotation"; return DBAT_HIP_EINVAL; }
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_err = "no HIP device: the dbat_hip core has no CPU path"; return DBAT_HIP_EDEVICE; }
    if (device < 0 || device >= ndev) { g_err = "bad device index"; return DBAT_HIP_EINVAL; }
    if (n_images == 0) return DBAT_HIP_OK;
    DeviceGuard dev_guard(device);
    const hipStream_t st = nullptr;
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
    if (g_resect_robust_timing) ev.start(st);
    launch<k_poseadjust>(dim3((unsigned)n_images), dim3(PO_WAVE), 0, st, (const int64_t *)dps.p, (const double *)dX.p, (const double *)dx.p,
                         (const uint8_t *)(use ? duse.p : nullptr), (const double *)(w ? dw.p : nullptr), (int)opt->max_iter,
                         opt->conv_tol * opt->conv_tol, dP.p, dused.p, dds.p, dis.p, dQ.p, (double *)dres.p);
    ev.lap(st);
    // a camera of fewer than three used points returns P as given: the kernel does not write it
    HIPCHK(hipMemcpy(P, dP.p, (size_t)12 * n_images * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(istat, dis.p, (size_t)4 * n_images * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(dstat, dds.p, (size_t)4 * n_images * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(Q, dQ.p, (size_t)36 * n_images * sizeof(double), hipMemcpyDeviceToHost));
    if (total > 0) {
        HIPCHK(hipMemcpy(used, dused.p, (size_t)total, hipMemcpyDeviceToHost));
        if (res) HIPCHK(hipMemcpy(res, dres.p, (size_t)2 * total * sizeof(double), hipMemcpyDeviceToHost));
    }
    g_resect_robust_ms[1] = ev.read();
    return DBAT_HIP_OK;
    API_CATCH
}

/* Debug / measurement: dbat_hip_debug_resect_robust_timing(1) makes dbat_hip_resect_ransac and dbat_hip_poseadjust on this
 * thread bracket their kernels with device events (off by default: a product call creates none);
 * dbat_hip_debug_resect_robust_ms then gives the milliseconds of the last k_resect_ransac [0] and k_poseadjust [1]. */
int dbat_hip_debug_resect_robust_timing(int32_t on) { g_resect_robust_timing = on != 0; return DBAT_HIP_OK; }
int dbat_hip_debug_resect_robust_ms(double *ms) {
    if (!ms) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    ms[0] = g_resect_robust_ms[0]; ms[1] = g_resect_robust_ms[1];
    return DBAT_HIP_OK;
}
}  // extern "C"
