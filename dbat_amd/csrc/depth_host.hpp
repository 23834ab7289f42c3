// Host side of the point depths and the chirality veto at zt (kernels: depth.hpp), included by dbat_core.hip after Core,
// analysis_host.hpp and robust_host.hpp (cm_slots).  The state (Core::dep, the veto's switch and counters) stays with Core: the loops consult it.
#pragma once

namespace dbat {
static const char *const DEPTH_ONE_RANK = "the counts and minima of the shards are not combined";
// What the kernels need beyond the plan's uploads -- the IP column of every slot of the camera-major copy, the scratch
// of the reductions, the depths in IP-column order -- is built by the first call (or by dbat_hip_set_chirality) and
// kept: no allocation per call, none inside a damping loop.  The camera records are cams_f, the ones eval_f /
// eval_f_step leave at the point they evaluated.
static void depth_plan(Core &c) {
    Core::DepthPlan &dep = c.dep;
    if (dep.ready) return;
    const Plan &P = c.P;
    std::vector<int64_t> col((size_t)std::max<int64_t>(c.nobs, 1), 0);
    const std::vector<int32_t> cmm = cm_slots(c);        // (robust_host.hpp)
    for (int64_t o = 0; o < c.nobs; ++o) col[(size_t)cmm[o]] = P.o_row[o];
    dep.cm_col.upload(col);
    dep.chunk_col.alloc((size_t)std::max<int64_t>(c.n_cm_chunks_all, 1));
    dep.red.alloc((size_t)(2 + std::max(P.nc, 1) + std::max<int64_t>(c.n_cm_chunks_all, 1)));
    dep.depth.alloc((size_t)std::max<int64_t>(P.no, 1));
    dep.img_host.resize((size_t)std::max(P.nc, 1));
    dep.ready = true;
}

// the depth kernels at zz with the camera records cams_f; FULL: depths, per-image minima and the argmin as well.
// Results: the mailbox (MB_DEPTH .., step_layout.hpp) once the stream has run (ticket mb_seq).
template <bool FULL>
static void depth_enqueue(Core &c, const double *zz, double thr, bool want_depth) {
    Core::DepthPlan &dep = c.dep;
    const Plan &P = c.P;
    HIPCHK(hipMemsetAsync(dep.red.p, 0, sizeof(unsigned long long), c.stream));
    HIPCHK(hipMemsetAsync(dep.red.p + 1, 0xFF, (size_t)(FULL ? 1 + P.nc : 1) * sizeof(unsigned long long), c.stream));
    unsigned long long *img = dep.red.p + 2, *ckey = dep.red.p + 2 + std::max(P.nc, 1);
    if (c.n_cm_chunks_all > 0)
        c.launch<k_depth_cm<FULL>>(dim3((unsigned)c.n_cm_chunks_all), dim3(256), 0, zz, (int64_t)P.NS, (const CamRec *)c.cams_f.p, (const int32_t *)c.cm_pt.p,
                                   (const int32_t *)c.cm_chunk_cam.p, (const int64_t *)c.cm_chunk_start.p, (const int64_t *)dep.cm_col.p, thr,
                                   want_depth ? dep.depth.p : (double *)nullptr, dep.red.p, img, ckey, dep.chunk_col.p);
    c.launch<k_depth_finish<FULL>>(dim3(1), dim3(256), 0, c.n_cm_chunks_all, (const unsigned long long *)dep.red.p, (const unsigned long long *)ckey,
                                   (const long long *)dep.chunk_col.p, c.mailbox, MB_DEPTH, ++c.mb_seq);
}
static int64_t mailbox_int(const double *slot) { int64_t v; memcpy(&v, slot, sizeof v); return v; }

static void point_depths(Core &c, double thr, double *hdepth, double *himg, int64_t &n_behind, double &min_depth, int64_t &argmin) {
    Core::DepthPlan &dep = c.dep;
    const Plan &P = c.P;
    depth_plan(c);
    c.prep_cams(c.zt.p, c.cams_f.p);
    dep.timer.start(c.stream);
    depth_enqueue<true>(c, c.zt.p, thr, hdepth != nullptr);
    dep.timer.lap(c.stream);
    if (hdepth && P.no > 0) HIPCHK(hipMemcpyAsync(hdepth, dep.depth.p, (size_t)P.no * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    if (himg && P.nc > 0)
        HIPCHK(hipMemcpyAsync(dep.img_host.data(), dep.red.p + 2, (size_t)P.nc * sizeof(unsigned long long), hipMemcpyDeviceToHost, c.stream));
    c.sync();                                            // (not armed: the copies behind the ticket are waited for too)
    if (himg) for (int i = 0; i < P.nc; ++i) himg[i] = depth_from_key(dep.img_host[i]);
    n_behind = mailbox_int(c.mailbox + MB_DEPTH_BEHIND); min_depth = c.mailbox[MB_DEPTH_MIN]; argmin = mailbox_int(c.mailbox + MB_DEPTH_ARGMIN);
    dep.timer.read();
}

bool Core::chirality_veto() {                            // right after eval_f_step: cams_f are the trial point's records
    stage(3);
    depth_enqueue<false>(*this, zt.p, chir_thr, false);
    mb_armed = true;
    sync();
    const int64_t nb = mailbox_int(mailbox + MB_DEPTH_BEHIND);
    ++veto_tested;
    if (nb == 0) return false;
    ++veto_rejected; veto_n_behind = nb; veto_min_depth = mailbox[MB_DEPTH_MIN];
    return true;
}
}  // namespace dbat

extern "C" {
int dbat_hip_point_depths(dbat_hip_handle *h, const double *x, double thr, double *depth_out, double *img_min_out, dbat_hip_depth_stats *stats_out) {
    API_TRY
    if (!h || !x || !stats_out) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    if (thr != thr) { g_err = "point depths: the threshold is NaN"; return DBAT_HIP_EINVAL; }
    Core &c = *h->core;
    if (!one_rank(c, "point depths", DEPTH_ONE_RANK)) return DBAT_HIP_EUNSUPPORTED;
    DeviceGuard dev_guard(c.device);
    c.x_to_z(x, c.zt.p);
    point_depths(c, thr, depth_out, img_min_out, stats_out->n_behind, stats_out->min_depth, stats_out->argmin_column);
    return DBAT_HIP_OK;
    API_CATCH
}

int dbat_hip_set_chirality(dbat_hip_handle *h, int32_t on, double min_depth) {
    API_TRY
    if (!h) { g_err = "null handle"; return DBAT_HIP_EINVAL; }
    if (!std::isfinite(min_depth)) { g_err = "chirality veto: min_depth must be finite"; return DBAT_HIP_EINVAL; }
    Core &c = *h->core;
    if (on && !one_rank(c, "chirality veto", DEPTH_ONE_RANK)) return DBAT_HIP_EUNSUPPORTED;
    DeviceGuard dev_guard(c.device);
    if (on) depth_plan(c);
    c.chirality = on != 0; c.chir_thr = min_depth;
    return DBAT_HIP_OK;
    API_CATCH
}

int dbat_hip_chirality_stats(const dbat_hip_handle *h, dbat_hip_veto_stats *out) {
    if (!h || !out) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    const Core &c = *h->core;
    out->tested = c.veto_tested; out->rejected = c.veto_rejected; out->n_behind = c.veto_n_behind; out->min_depth = c.veto_min_depth;
    return DBAT_HIP_OK;
}

/* Debug / measurement: the veto's own pass (the reset of its two words, k_depth_cm<false>, k_depth_finish<false>) at x,
 * reps times back to back between two device events: ms[0] = milliseconds per pass, ms[1] = the count it found. */
int dbat_hip_debug_chirality_pass_ms(dbat_hip_handle *h, const double *x, int32_t reps, double *ms) {
    API_TRY
    if (!h || !x || !ms || reps < 1) { g_err = "bad argument"; return DBAT_HIP_EINVAL; }
    Core &c = *h->core;
    if (!one_rank(c, "chirality veto", DEPTH_ONE_RANK)) return DBAT_HIP_EUNSUPPORTED;
    DeviceGuard dev_guard(c.device);
    depth_plan(c);
    c.x_to_z(x, c.zt.p);
    c.prep_cams(c.zt.p, c.cams_f.p);
    EventTimer<1> timer;                                 // (its own: dbat_hip_debug_point_depths_ms keeps the last dbat_hip_point_depths)
    timer.start(c.stream);
    for (int i = 0; i < reps; ++i) depth_enqueue<false>(c, c.zt.p, c.chir_thr, false);
    timer.lap(c.stream);
    c.sync();
    ms[0] = (float)timer.read() / reps; ms[1] = (double)mailbox_int(c.mailbox + MB_DEPTH_BEHIND);
    return DBAT_HIP_OK;
    API_CATCH
}

/* Debug / measurement: milliseconds of the kernels of the last dbat_hip_point_depths on the handle's stream (device
 * events: the reset of the scratch, k_depth_cm, k_depth_finish). */
int dbat_hip_debug_point_depths_ms(dbat_hip_handle *h, double *ms) {
    if (!h || !ms || !h->core->dep.ready) { g_err = "no point depths computed on this handle"; return DBAT_HIP_EINVAL; }
    ms[0] = h->core->dep.timer.ms[0];
    return DBAT_HIP_OK;
}
}  // extern "C"
