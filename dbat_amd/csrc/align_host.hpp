// Host side of the network transforms (kernels: align.hpp): helpers and C entry points of dbat_hip_rigidalign /
// dbat_hip_multixform.  Included by dbat_core.hip after Core; these calls take no handle.
#pragma once

namespace dbat {
// the kernels of the last call on this thread: [0] centroids [1] cross products [2] residuals (dbat_hip_rigidalign),
// [3] points [4] cameras (dbat_hip_multixform), each pass with its finishing launch
using AlignClock = KernelClock<struct AlignFamily, 5>;

static const char *const ALIGN_COLLINEAR = "rigidalign: the used points are collinear or coincide (second singular value of the "
                                           "cross-product matrix <= 1e-12 of the first): the rotation is not defined";
}  // namespace dbat

extern "C" {
int dbat_hip_rigidalign(int32_t device, int64_t n, const double *X, const double *Y, const uint8_t *use, int32_t scale, double *T, double *stats, double *resid) {
    API_TRY
    if (n < 0 || !T || !stats || (n > 0 && (!X || !Y))) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    // Everything that can be refused is refused here, before any device call.  The collinearity test needs the
    // cross-product matrix: the host pass that looks at every used coordinate anyway also sums it, with the first used
    // column as the origin of both sets.  The matrix the result comes from is the device's.
    int64_t m = 0;
    double x0[3] = {0, 0, 0}, y0[3] = {0, 0, 0}, Sx[3] = {0, 0, 0}, Sy[3] = {0, 0, 0}, Cxy[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t i = 0; i < n; ++i) {
        if (use && !use[i]) continue;
        const double *x = X + 3 * i, *y = Y + 3 * i;
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(x[k]) || !std::isfinite(y[k])) { g_err = "rigidalign: used column " + std::to_string(i) + " is not finite"; return DBAT_HIP_EINVAL; }
        if (m++ == 0) for (int k = 0; k < 3; ++k) { x0[k] = x[k]; y0[k] = y[k]; }
        double a[3], b[3];
        for (int k = 0; k < 3; ++k) { a[k] = x[k] - x0[k]; b[k] = y[k] - y0[k]; Sx[k] += a[k]; Sy[k] += b[k]; }
        for (int j = 0; j < 3; ++j) for (int k = 0; k < 3; ++k) Cxy[3 * j + k] += b[k] * a[j];
    }
    if (m < 3) { g_err = "rigidalign: fewer than three used columns"; return DBAT_HIP_EINVAL; }
    {
        double U[9], V[9], s[3];
        for (int j = 0; j < 3; ++j) for (int k = 0; k < 3; ++k) Cxy[3 * j + k] -= Sy[k] * Sx[j] / (double)m;
        al_svd3(Cxy, U, s, V);
        if (!(s[1] > 1e-12 * s[0])) { g_err = ALIGN_COLLINEAR; return DBAT_HIP_EINVAL; }
    }
    BatchDevice dev(device);                          // (no early return for n == 0: fewer than three columns were refused)
    const int G = (int)al_grid(n);
    DevBuf<double> dX, dY, part, out, dres;
    DevBuf<uint8_t> duse;
    dX.upload(X, (size_t)3 * n); dY.upload(Y, (size_t)3 * n);
    if (use) duse.upload(use, (size_t)n);
    part.alloc((size_t)10 * G); out.alloc(18);
    EventTimer<2> e01;
    EventTimer<1> e2;
    AlignClock::start(e01, dev.st);
    launch<k_align_centroid>(dim3(G), dim3(AL_WG), 0, dev.st, n, dX.p, dY.p, duse.p, part.p);
    launch<k_align_finish<7, true>>(dim3(1), dim3(AL_WG), 0, dev.st, G, part.p, out.p);
    e01.lap(dev.st);
    launch<k_align_cross>(dim3(G), dim3(AL_WG), 0, dev.st, n, dX.p, dY.p, duse.p, out.p, part.p);
    launch<k_align_finish<10, false>>(dim3(1), dim3(AL_WG), 0, dev.st, G, part.p, out.p + 7);
    e01.lap(dev.st);
    double h[18];
    HIPCHK(hipMemcpy(h, out.p, 17 * sizeof(double), hipMemcpyDeviceToHost));
    double *const ms = AlignClock::ms;
    ms[0] = e01.read(); ms[1] = e01.ms[1]; ms[2] = ms[3] = ms[4] = 0;
    // rigidalign.m:46-61
    AlignPar ap;
    double R[9], s[3];
    al_rotation(h + 7, R, s);
    if (!(s[1] > 1e-12 * s[0])) { g_err = ALIGN_COLLINEAR; return DBAT_HIP_EINVAL; }
    double alpha = 1.0;
    if (scale) {
        double gamma = 0;                           // tr((R A)' B) = sum R_ij C_ij
        for (int i = 0; i < 9; ++i) gamma += R[i] * h[7 + i];
        alpha = gamma / h[16];
    }
    double d[3];
    for (int k = 0; k < 3; ++k) { ap.xm[k] = h[1 + k]; ap.ym[k] = h[4 + k]; }
    for (int i = 0; i < 9; ++i) { ap.aR[i] = alpha * R[i]; ap.aRl[i] = std::fma(alpha, R[i], -ap.aR[i]); }
    for (int k = 0; k < 3; ++k) d[k] = ap.ym[k] - (ap.aR[k] * ap.xm[0] + ap.aR[3 + k] * ap.xm[1] + ap.aR[6 + k] * ap.xm[2]);
    if (resid) dres.alloc((size_t)3 * n);
    AlignClock::start(e2, dev.st);
    launch<k_align_resid>(dim3(G), dim3(AL_WG), 0, dev.st, n, dX.p, dY.p, duse.p, ap, dres.p, part.p);
    launch<k_align_finish<1, false>>(dim3(1), dim3(AL_WG), 0, dev.st, G, part.p, out.p + 17);
    e2.lap(dev.st);
    HIPCHK(hipMemcpy(h + 17, out.p + 17, sizeof(double), hipMemcpyDeviceToHost));
    dres.download(resid);                            // (empty without resid)
    ms[2] = e2.read();
    for (int j = 0; j < 3; ++j) {
        for (int i = 0; i < 3; ++i) T[4 * j + i] = ap.aR[3 * j + i];
        T[4 * j + 3] = 0; T[12 + j] = d[j];
    }
    T[15] = 1;
    stats[0] = alpha; stats[1] = std::sqrt(h[17] / h[0]); stats[2] = h[0]; stats[3] = s[1] / s[0];
    return DBAT_HIP_OK;
    API_CATCH
}

int dbat_hip_multixform(int32_t device, const double *T, int64_t n_images, int32_t eo_rows, double *EO, int64_t n_points, double *OP, uint8_t *fail) {
    API_TRY
    if (!T || n_images < 0 || n_points < 0 || (n_images > 0 && !EO) || (n_points > 0 && !OP)) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    if (eo_rows < 6) { g_err = "multixform: EO needs at least six rows"; return DBAT_HIP_EINVAL; }
    XformPar par;
    double alpha = 1.0;
    if (const char *e = al_similarity(T, par, alpha)) { g_err = std::string("multixform: ") + e; return DBAT_HIP_EINVAL; }
    BatchDevice dev(device);
    std::fill(AlignClock::ms, AlignClock::ms + 5, 0.0);
    if (n_points > 0) {
        DevBuf<double> dOP;
        dOP.upload(OP, (size_t)3 * n_points);
        EventTimer<1> ev;
        AlignClock::start(ev, dev.st);
        launch<k_xform_points>(dim3((unsigned)cdiv(n_points, AL_WG)), dim3(AL_WG), 0, dev.st, n_points, dOP.p, par);
        ev.lap(dev.st);
        dOP.download(OP);
        AlignClock::ms[3] = ev.read();
    }
    if (n_images > 0) {
        DevBuf<double> dEO;
        DevBuf<uint8_t> dfail;
        dEO.upload(EO, (size_t)eo_rows * n_images);
        dfail.alloc((size_t)n_images);
        EventTimer<1> ev;
        AlignClock::start(ev, dev.st);
        launch<k_xform_cams>(dim3((unsigned)cdiv(n_images, AL_WG)), dim3(AL_WG), 0, dev.st, n_images, (int)eo_rows, dEO.p, par, dfail.p);
        ev.lap(dev.st);
        dEO.download(EO);
        if (fail) dfail.download(fail);
        AlignClock::ms[4] = ev.read();
    }
    return DBAT_HIP_OK;
    API_CATCH
}

/* Debug / measurement: dbat_hip_debug_align_timing(1) makes dbat_hip_rigidalign / dbat_hip_multixform on this thread
 * bracket their kernels with device events (off by default: a product call creates none); dbat_hip_debug_align_ms then
 * gives the milliseconds of the last call: ms[0] centroids, ms[1] cross products, ms[2] residuals, ms[3] points, ms[4]
 * cameras; each pass with its finishing launch; 0 for what the last call did not launch or did not time. */
int dbat_hip_debug_align_timing(int32_t on) { return AlignClock::set(on); }
int dbat_hip_debug_align_ms(double *ms) { return AlignClock::get(ms); }
}  // extern "C"
