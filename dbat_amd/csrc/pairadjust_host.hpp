// Host side of the least-squares relative orientation (kernel: pairadjust.hpp): the C entry point dbat_hip_pairadjust.
// Included by dbat_core.hip after Core; the call takes no handle and no plan.
#pragma once

namespace dbat {
using PairadjustClock = KernelClock<struct PairadjustFamily, 1>;    // k_pairadjust of the last call on this thread
}  // namespace dbat

extern "C" {
int dbat_hip_default_pair_options(dbat_hip_pair_options *opt) {
    if (!opt) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    opt->max_iter = 20; opt->conv_tol = 1e-6; opt->min_angle = 0.0;
    return DBAT_HIP_OK;
}

int dbat_hip_pairadjust(int32_t device, int32_t n_pairs, const int64_t *pt_start, const double *x1, const double *x2,
                        const uint8_t *use, const double *w1, const double *w2, int32_t front_dir,
                        const dbat_hip_pair_options *opt, double *P2, double *X, uint8_t *used, double *dstat, int32_t *istat,
                        double *Q, double *res) {
    API_TRY
    if (n_pairs < 0 || !pt_start || !opt || !P2 || !dstat || !istat || !Q) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    if (front_dir != 1 && front_dir != -1) { g_err = "pairadjust: front_dir must be +1 or -1"; return DBAT_HIP_EINVAL; }
    check_pair_options("pairadjust", opt);
    if (!(opt->min_angle >= 0 && opt->min_angle < 1.5707963267948966)) { g_err = "pairadjust: min_angle must lie in [0, pi/2)"; return DBAT_HIP_EINVAL; }
    check_ranges("pairadjust", "pt_start", n_pairs, pt_start);       // (no cap on the points of a pair, where poseadjust has 2^29)
    const int64_t total = pt_start[n_pairs];
    if (total > 0 && (!x1 || !x2 || !X || !used)) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    check_columns("pairadjust", "correspondence", 2, total, x1, x2, w1, w2);
    check_used_points("pairadjust", total, use, X);
    for (int32_t p = 0; p < n_pairs; ++p) {
        const double *P = P2 + 12 * (size_t)p;
        check_pose("pairadjust", "P2", "pair", p, P);
        if (P[9] == 0 && P[10] == 0 && P[11] == 0) { g_err = "pairadjust: t of pair " + std::to_string(p) + " is zero"; return DBAT_HIP_EINVAL; }
    }
    BatchDevice dev(device);
    if (n_pairs == 0) return DBAT_HIP_OK;
    // t comes at unit length: the gauge of camsfrome
    std::vector<double> Pn(P2, P2 + 12 * (size_t)n_pairs);
    for (int32_t p = 0; p < n_pairs; ++p) {
        double *t = Pn.data() + 12 * (size_t)p + 9;
        const double m = std::max(std::fabs(t[0]), std::max(std::fabs(t[1]), std::fabs(t[2])));
        const double a = t[0] / m, b = t[1] / m, c = t[2] / m, n = std::sqrt(a * a + b * b + c * c);
        t[0] = a / n; t[1] = b / n; t[2] = c / n;
    }
    const double s = std::sin(opt->min_angle);
    DevBuf<int64_t> dps;
    DevBuf<double> dx1, dx2, dw1, dw2, dP, dX, dXt, dds, dQ, dres;
    DevBuf<uint8_t> duse, dused;
    DevBuf<int32_t> dis;
    const size_t tot1 = (size_t)total;                    // may be 0: every pair then ends with code 4
    dps.upload(pt_start, (size_t)n_pairs + 1);
    dx1.upload(x1, 2 * tot1); dx2.upload(x2, 2 * tot1);
    if (w1) dw1.upload(w1, 2 * tot1);
    if (w2) dw2.upload(w2, 2 * tot1);
    if (use) duse.upload(use, tot1);
    dP.upload(Pn); dX.upload(X, 3 * tot1); dXt.alloc(3 * tot1); dused.alloc(tot1);
    dds.alloc((size_t)4 * n_pairs); dis.alloc((size_t)4 * n_pairs); dQ.alloc((size_t)36 * n_pairs);
    if (res && total > 0) { dres.alloc(4 * tot1); HIPCHK(hipMemsetAsync(dres.p, 0, 4 * tot1 * sizeof(double), dev.st)); }
    EventTimer<1> ev;
    PairadjustClock::start(ev, dev.st);
    launch<k_pairadjust>(dim3((unsigned)n_pairs), dim3(PA_WG), 0, dev.st, (const int64_t *)dps.p, (const double *)dx1.p, (const double *)dx2.p,
                         (const uint8_t *)(use ? duse.p : nullptr), (const double *)(w1 ? dw1.p : nullptr),
                         (const double *)(w2 ? dw2.p : nullptr), (int)front_dir, (int)opt->max_iter, opt->conv_tol * opt->conv_tol, s * s,
                         dP.p, dX.p, dXt.p, dused.p, dds.p, dis.p, dQ.p, (double *)dres.p);
    ev.lap(dev.st);
    // a pair of fewer than five used correspondences returns P2 as given: the bits of the caller's, not the unit-length copy
    std::vector<double> Pout((size_t)12 * n_pairs);
    dP.download(Pout.data()); dis.download(istat); dds.download(dstat); dQ.download(Q);
    for (int32_t p = 0; p < n_pairs; ++p)
        if (istat[4 * (size_t)p] != PA_TOO_FEW) std::copy(Pout.begin() + 12 * (size_t)p, Pout.begin() + 12 * (size_t)(p + 1), P2 + 12 * (size_t)p);
    dX.download(X); dused.download(used); dres.download(res);     // (empty without points; dres without res)
    PairadjustClock::ms[0] = ev.read();
    return DBAT_HIP_OK;
    API_CATCH
}

/* Debug / measurement: dbat_hip_debug_pairadjust_timing(1) makes dbat_hip_pairadjust on this thread bracket its kernel with
 * device events (off by default: a product call creates none); dbat_hip_debug_pairadjust_ms then gives the milliseconds
 * of the last call's k_pairadjust. */
int dbat_hip_debug_pairadjust_timing(int32_t on) { return PairadjustClock::set(on); }
int dbat_hip_debug_pairadjust_ms(double *ms) { return PairadjustClock::get(ms); }
}  // extern "C"
