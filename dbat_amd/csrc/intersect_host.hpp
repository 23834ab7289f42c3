// Host side of the robust forward intersection (kernels: intersect_ransac.hpp, pointadjust.hpp): the C entry points
// dbat_hip_intersect_ransac and dbat_hip_pointadjust.  Included by dbat_core.hip after Core; the calls take no handle and
// no plan.
#pragma once

namespace dbat {
// k_intersect_ransac [0] and k_pointadjust [1] of the last call of each on this thread
using IntersectClock = KernelClock<struct IntersectFamily, 2>;

// The checks both entry points share, before any device call and after the null arguments, the counts and the ranges:
// the camera of every ray, and that every ray that may be used is finite.
static void ir_check_rays(const char *who, int32_t n_points, const int64_t *ray_start, const int32_t *cam, const double *xn,
                          int32_t n_cams, const uint8_t *use) {
    const int64_t total = ray_start[n_points];
    for (int64_t g = 0; g < total; ++g)
        if (cam[g] < 0 || cam[g] >= n_cams) refuse(who, "cam of ray " + std::to_string(g) + " is outside the cameras");
    for (int64_t g = 0; g < total; ++g)
        if ((!use || use[g]) && !(std::isfinite(xn[2 * g]) && std::isfinite(xn[2 * g + 1])))
            refuse(who, "xn of ray " + std::to_string(g) + " is to be used and is not finite");
}
static void ir_check_ray_cap(const char *who, int32_t n_points, const int64_t *ray_start) {
    for (int32_t p = 0; p < n_points; ++p)
        if (ray_start[p + 1] - ray_start[p] >= ((int64_t)1 << 29)) refuse(who, "more than 2^29 rays in one point (ray_start)");
}
}  // namespace dbat

extern "C" {
int dbat_hip_intersect_ransac(int32_t device, int32_t n_points, const int64_t *ray_start, const int32_t *cam, const double *xn,
                              int32_t n_cams, const double *P, const uint8_t *use, const int64_t *smp_start, const int32_t *smp,
                              const double *thr2, double min_angle, double *X, int32_t *stats, uint8_t *inlier, double *ssq) {
    API_TRY
    const char *who = "intersect_ransac";
    // the null arguments first: those that are needed only where there are rays or samples read the two totals, which
    // takes a count that is not negative
    const int64_t total = ray_start && n_points >= 0 ? ray_start[n_points] : 0;
    const int64_t nsmp = smp_start && n_points >= 0 ? smp_start[n_points] : 0;
    if (!ray_start || (n_points > 0 && (!X || !stats || !ssq)) || (n_cams > 0 && (!P || !thr2)) ||
        (total > 0 && (!cam || !xn || !inlier)) || (nsmp > 0 && !smp)) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    if (n_points < 0 || n_cams < 0) { g_err = "intersect_ransac: n_points and n_cams must not be negative"; return DBAT_HIP_EINVAL; }
    check_ranges(who, "ray_start", n_points, ray_start);
    if (smp_start) check_ranges(who, "smp_start", n_points, smp_start);
    ir_check_rays(who, n_points, ray_start, cam, xn, n_cams, use);
    for (int32_t c = 0; c < n_cams; ++c) check_pose(who, "P", "camera", c, P + 12 * (size_t)c);
    for (int32_t c = 0; c < n_cams; ++c)
        if (!(thr2[c] > 0) || !std::isfinite(thr2[c])) refuse(who, "thr2 of camera " + std::to_string(c) + " is not positive and finite");
    if (!(min_angle >= 0 && min_angle < 1.5707963267948966)) refuse(who, "min_angle must be in [0, pi/2)");
    for (int32_t p = 0; smp_start && p < n_points; ++p) {
        const int64_t nr = ray_start[p + 1] - ray_start[p];
        for (int64_t h = smp_start[p]; h < smp_start[p + 1]; ++h) {       // any index outside comes before any that repeats
            const int32_t *t = smp + 2 * h;
            if (t[0] < 0 || t[1] < 0 || t[0] >= nr || t[1] >= nr) refuse(who, "sample " + std::to_string(h) + " has an index outside the point's rays");
            if (t[0] == t[1]) refuse(who, "sample " + std::to_string(h) + " repeats an index");
        }
    }
    for (int32_t p = 0; p < n_points; ++p)
        if ((!smp_start || smp_start[p + 1] == smp_start[p]) && ray_start[p + 1] - ray_start[p] > IR_MAX_EXHAUSTIVE)
            refuse(who, "point " + std::to_string(p) + " has more than " + std::to_string(IR_MAX_EXHAUSTIVE) + " rays and no samples (smp_start)");
    ir_check_ray_cap(who, n_points, ray_start);
    for (int32_t p = 0; smp_start && p < n_points; ++p)
        if (smp_start[p + 1] - smp_start[p] >= ((int64_t)1 << 31)) refuse(who, "more than 2^31 samples in one point (smp_start)");
    BatchDevice dev(device);
    if (n_points == 0) return DBAT_HIP_OK;
    DevBuf<int64_t> drs, dss;
    DevBuf<double> dx, dP, dt, dX, dq;
    DevBuf<uint8_t> duse, din;
    DevBuf<int32_t> dcam, dsm, dst;
    drs.upload(ray_start, (size_t)n_points + 1);
    if (smp_start) dss.upload(smp_start, (size_t)n_points + 1);
    dcam.upload(cam, (size_t)total); dx.upload(xn, (size_t)2 * total); dsm.upload(smp, (size_t)2 * nsmp);
    dP.upload(P, (size_t)12 * n_cams); dt.upload(thr2, (size_t)n_cams);
    if (use) duse.upload(use, (size_t)total);
    dX.alloc((size_t)3 * n_points); dst.alloc((size_t)4 * n_points); dq.alloc((size_t)n_points); din.alloc((size_t)total);
    const double sn = std::sin(min_angle), par2 = std::max(sn * sn, IR_PARALLAX2);
    EventTimer<1> ev;
    IntersectClock::start(ev, dev.st);
    launch<k_intersect_ransac>(dim3((unsigned)cdiv(n_points, IR_POINTS)), dim3(IR_WG), 0, dev.st, (int)n_points, (const int64_t *)drs.p,
                               (const int32_t *)dcam.p, (const double *)dx.p, (const double *)dP.p, (const uint8_t *)(use ? duse.p : nullptr),
                               (const int64_t *)(smp_start ? dss.p : nullptr), (const int32_t *)dsm.p, (const double *)dt.p, par2,
                               dX.p, dst.p, din.p, dq.p);
    ev.lap(dev.st);
    dX.download(X); dst.download(stats); dq.download(ssq); din.download(inlier);
    IntersectClock::ms[0] = ev.read();
    return DBAT_HIP_OK;
    API_CATCH
}

int dbat_hip_pointadjust(int32_t device, int32_t n_points, const int64_t *ray_start, const int32_t *cam, const double *xn,
                         int32_t n_cams, const double *P, const uint8_t *use, const double *w,
                         const dbat_hip_pair_options *opt, double *X, uint8_t *used, double *dstat, int32_t *istat,
                         double *Q, double *res) {
    API_TRY
    const char *who = "pointadjust";
    const int64_t total = ray_start && n_points >= 0 ? ray_start[n_points] : 0;       // (as in dbat_hip_intersect_ransac)
    if (!ray_start || !opt || (n_points > 0 && (!X || !dstat || !istat || !Q)) || (n_cams > 0 && !P) ||
        (total > 0 && (!cam || !xn || !used))) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    if (n_points < 0 || n_cams < 0) { g_err = "pointadjust: n_points and n_cams must not be negative"; return DBAT_HIP_EINVAL; }
    check_pair_options(who, opt);
    if (!(opt->min_angle == 0)) { g_err = "pointadjust: min_angle must be 0"; return DBAT_HIP_EINVAL; }
    check_ranges(who, "ray_start", n_points, ray_start);
    ir_check_rays(who, n_points, ray_start, cam, xn, n_cams, use);
    ir_check_ray_cap(who, n_points, ray_start);
    for (int32_t p = 0; p < n_points; ++p) {              // the start of a point that has a ray to use
        bool any = false;
        for (int64_t g = ray_start[p]; g < ray_start[p + 1] && !any; ++g) any = !use || use[g];
        if (any && !(std::isfinite(X[3 * (size_t)p]) && std::isfinite(X[3 * (size_t)p + 1]) && std::isfinite(X[3 * (size_t)p + 2])))
            refuse(who, "X of point " + std::to_string(p) + " has a ray to use and is not finite");
    }
    check_weights(who, "ray", total, w);
    for (int32_t c = 0; c < n_cams; ++c) check_pose(who, "P", "camera", c, P + 12 * (size_t)c);
    BatchDevice dev(device);
    if (n_points == 0) return DBAT_HIP_OK;
    DevBuf<int64_t> drs;
    DevBuf<double> dx, dw, dP, dX, dds, dQ, dres;
    DevBuf<uint8_t> duse, dused;
    DevBuf<int32_t> dcam, dis;
    const size_t tot1 = (size_t)total;                    // may be 0: every point then ends with code 4
    drs.upload(ray_start, (size_t)n_points + 1);
    dcam.upload(cam, tot1); dx.upload(xn, 2 * tot1);
    if (w) dw.upload(w, 2 * tot1);
    if (use) duse.upload(use, tot1);
    dP.upload(P, (size_t)12 * n_cams); dX.upload(X, (size_t)3 * n_points); dused.alloc(tot1);
    dds.alloc((size_t)4 * n_points); dis.alloc((size_t)4 * n_points); dQ.alloc((size_t)9 * n_points);
    if (res && total > 0) dres.alloc(2 * tot1);
    EventTimer<1> ev;
    IntersectClock::start(ev, dev.st);
    launch<k_pointadjust>(dim3((unsigned)cdiv(n_points, IA_POINTS)), dim3(IA_WG), 0, dev.st, (int)n_points, (const int64_t *)drs.p,
                          (const int32_t *)dcam.p, (const double *)dx.p, (const double *)dP.p, (const uint8_t *)(use ? duse.p : nullptr),
                          (const double *)(w ? dw.p : nullptr), (int)opt->max_iter, opt->conv_tol * opt->conv_tol, dX.p, dused.p,
                          dds.p, dis.p, dQ.p, (double *)dres.p);
    ev.lap(dev.st);
    // a point of fewer than two used rays returns X as given: the kernel does not write it
    dX.download(X); dis.download(istat); dds.download(dstat); dQ.download(Q);
    dused.download(used); dres.download(res);             // (empty without rays; dres without res)
    IntersectClock::ms[1] = ev.read();
    return DBAT_HIP_OK;
    API_CATCH
}

/* Debug / measurement: dbat_hip_debug_intersect_robust_timing(1) makes dbat_hip_intersect_ransac and dbat_hip_pointadjust on
 * this thread bracket their kernels with device events (off by default: a product call creates none);
 * dbat_hip_debug_intersect_robust_ms then gives the milliseconds of the last k_intersect_ransac [0] and k_pointadjust [1]. */
int dbat_hip_debug_intersect_robust_timing(int32_t on) { return IntersectClock::set(on); }
int dbat_hip_debug_intersect_robust_ms(double *ms) { return IntersectClock::get(ms); }
}  // extern "C"
