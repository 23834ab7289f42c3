// Host side of the robust reweighting (kernels: robust.hpp), included by dbat_core.hip after Core, solve_once and the
// handle.  The engine knows nothing of it: its kernels read the weights Core holds (o_w, sg_w, cm_w), and
// Core::obs_weights() switches those between the plan's and one pair per observation.  What the reweighting itself
// needs is RobustState, which the handle owns from the first robust call on and robust_reset() gives up again: a
// handle that never sees such a call allocates none of it.
#pragma once

namespace dbat {
// camera-major slot of every owned observation (processing order): the plan's stable counting sort by camera, tiled
// part first
static std::vector<int32_t> cm_slots(const Core &c) {
    const Plan &P = c.P;
    std::vector<int32_t> cmm((size_t)c.nobs);
    const int64_t ntiled = P.nb_tiled > 0 ? P.batch_start[P.nb_tiled] : 0;
    std::vector<int64_t> cnt((size_t)P.nc + 1);
    for (int part = 0; part < 2; ++part) {
        const int64_t lo = part ? ntiled : 0, hi = part ? c.nobs : ntiled;
        std::fill(cnt.begin(), cnt.end(), 0);
        for (int64_t o = lo; o < hi; ++o) ++cnt[P.o_cam[o] + 1];
        for (int cam = 0; cam < P.nc; ++cam) cnt[cam + 1] += cnt[cam];
        for (int64_t o = lo; o < hi; ++o) cmm[o] = (int32_t)(lo + cnt[P.o_cam[o]]++);
    }
    return cmm;
}

// robust_scratch() allocates what an evaluation needs (rs_bits ... rsel_red); robust_promote() gives every owned
// observation its own weights (o_w = o_w_base * sqrt(omega)) and keeps the maps from processing order to the
// slot-major (sg_map, -1: no slot) and camera-major (cm_map) copies.
struct RobustState {
    bool robust_on = false;             // promoted: the engine's weights are o_w_base * sqrt(omega)
    DevBuf<double> o_w_base, omega, rsel_hist_f, rsel_red, robust_r;
    DevBuf<uint64_t> rs_bits, rsel_state;
    DevBuf<int32_t> sg_map, cm_map;
    DevBuf<unsigned> rsel_hist;
    DevBuf<unsigned long long> rmax;
};

static unsigned robust_grid(const Core &c) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(c.nobs, 256), 4096)); }
static void robust_scratch(Core &c, RobustState &r) {             // what an evaluation needs (dbat_hip_robust_weights does not promote)
    if (r.rs_bits.p || r.rsel_state.p) return;
    r.rs_bits.alloc((size_t)std::max<int64_t>(c.nobs, 1));
    r.robust_r.alloc((size_t)2 * std::max<int64_t>(c.P.no, 1));
    r.rsel_hist.alloc(2 * RSEL_BINS); r.rsel_hist_f.alloc(2 * RSEL_BINS);
    HIPCHK(hipMemset(r.rsel_hist.p, 0, 2 * RSEL_BINS * sizeof(unsigned)));
    r.rsel_state.alloc(4); r.rmax.alloc(1); r.rsel_red.alloc((size_t)c.P.nranks);
}
static void robust_apply_omega(Core &c, RobustState &r) {         // o_w, sg_w, cm_w from omega
    if (c.nobs > 0)
        c.launch<k_robust_apply<false>>(dim3(robust_grid(c)), dim3(256), 0, c.nobs, (const uint64_t *)nullptr, 1.0, 0, 1.0, r.omega.p, (const double *)r.o_w_base.p, c.o_w.p,
                                        (const int32_t *)(c.route == Core::TileRoute::sig ? r.sg_map.p : nullptr), c.sg_w.p, (const int32_t *)r.cm_map.p, c.cm_w.p);
    c.s_valid = false;
}
static void robust_set_ones(Core &c, RobustState &r) {
    if (c.nobs > 0) c.launch<k_robust_fill>(dim3(robust_grid(c)), dim3(256), 0, c.nobs, 1.0, r.omega.p);
    robust_apply_omega(c, r);
}
static void robust_promote(Core &c, RobustState &r) {
    if (r.robust_on) return;
    const Plan &P = c.P;
    const int64_t nobs = c.nobs;
    if (nobs >= ((int64_t)1 << 31) / 2) throw UsageError{"robust weights: more than 2^30 observations on one rank"};
    robust_scratch(c, r);
    r.o_w_base.alloc((size_t)2 * std::max<int64_t>(nobs, 1));
    c.obs_weights(true);
    if (P.uniform_w) {
        if (nobs > 0) c.launch<k_robust_base>(dim3(robust_grid(c)), dim3(256), 0, nobs, (const int32_t *)c.o_cam.p, (const double *)c.cam_w.p, r.o_w_base.p);
    } else if (nobs > 0) {
        HIPCHK(hipMemcpyAsync(r.o_w_base.p, c.o_w.p, (size_t)2 * nobs * sizeof(double), hipMemcpyDeviceToDevice, c.stream));
    }
    r.cm_map.upload(cm_slots(c));
    if (c.route == Core::TileRoute::sig) {   // slot-major slot: group g, slot j, point i at obs0_g + j*m_g + i (plan.hpp, signature groups)
        std::vector<int32_t> sgm((size_t)nobs, -1);
        for (size_t q = 0; q < P.sg_chunk.size() / 8; ++q) {
            const int32_t *ch = &P.sg_chunk[8 * q];
            const int64_t npts = ch[1], k = ch[2], m = ch[4], i0 = ch[5], g0 = ch[6];
            for (int64_t i = i0; i < i0 + npts; ++i)
                for (int64_t j = 0; j < k; ++j) sgm[g0 + i * k + j] = (int32_t)(g0 + j * m + i);
        }
        r.sg_map.upload(sgm);
    }
    r.omega.alloc((size_t)std::max<int64_t>(nobs, 1));
    r.robust_on = true;
    robust_set_ones(c, r);
}
// back to the fresh handle: the plan's weights in the engine, no state of the reweighting
static void robust_reset(dbat_hip_handle &h) {
    if (h.rob && h.rob->robust_on) h.core->obs_weights(false);
    h.rob.reset();
}
// max of one double over the ranks (the all-reduce sums: every rank contributes its own slot)
static double max_over_ranks(Core &c, RobustState &r, double v) {
    if (!c.multi()) return v;
    std::vector<double> h((size_t)c.P.nranks, 0.0);
    h[c.P.rank] = v;
    HIPCHK(hipMemcpyAsync(r.rsel_red.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, c.stream));
    c.do_allreduce(r.rsel_red.p, c.P.nranks);
    HIPCHK(hipMemcpyAsync(h.data(), r.rsel_red.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipStreamSynchronize(c.stream));
    return *std::max_element(h.begin(), h.end());
}
// exact median of s over all ranks' observations: radix select of the two middle order statistics
static double robust_median(Core &c, RobustState &r) {
    const int64_t nobs = c.nobs;
    const uint64_t total = (uint64_t)c.P.no;
    uint64_t st[4] = {0, 0, (total - 1) / 2, total / 2};
    HIPCHK(hipMemcpyAsync(r.rsel_state.p, st, sizeof st, hipMemcpyHostToDevice, c.stream));
    const unsigned gh = (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(nobs, 4096), 1024));
    for (int pass = 0; pass < RSEL_PASSES; ++pass) {
        if (nobs > 0) c.launch<k_rsel_hist>(dim3(gh), dim3(256), 0, nobs, (const uint64_t *)r.rs_bits.p, (const uint64_t *)r.rsel_state.p, RSEL_SHIFT[pass], RSEL_BITS[pass], r.rsel_hist.p);
        if (c.multi()) {
            c.launch<k_rsel_to_f64>(dim3(16), dim3(256), 0, r.rsel_hist.p, r.rsel_hist_f.p);
            c.do_allreduce(r.rsel_hist_f.p, 2 * RSEL_BINS);
            c.launch<k_rsel_pick<true>>(dim3(1), dim3(256), 0, r.rsel_hist.p, (const double *)r.rsel_hist_f.p, r.rsel_state.p, RSEL_SHIFT[pass]);
        } else {
            c.launch<k_rsel_pick<false>>(dim3(1), dim3(256), 0, r.rsel_hist.p, (const double *)nullptr, r.rsel_state.p, RSEL_SHIFT[pass]);
        }
    }
    HIPCHK(hipMemcpyAsync(st, r.rsel_state.p, sizeof st, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipStreamSynchronize(c.stream));
    double a, b;
    memcpy(&a, &st[0], 8); memcpy(&b, &st[1], 8);
    return (a + b) / 2.0;
}
// First half of an evaluation: s of every owned observation at zz into rs_bits.  s_ip (device, [no], zero outside this
// rank's observations): optional.
static void robust_norms(Core &c, RobustState &r, const double *zz, double *s_ip) {
    const Plan &P = c.P;
    const int64_t nobs = c.nobs;
    HIPCHK(hipMemsetAsync(r.robust_r.p, 0, (size_t)2 * P.no * sizeof(double), c.stream));
    c.eval_f(zz, nullptr, r.robust_r.p);
    if (nobs > 0)
        c.launch<k_robust_norm>(dim3(robust_grid(c)), dim3(256), 0, nobs, (const int64_t *)c.o_row.p, (const double *)r.robust_r.p,
                                (const double *)(r.robust_on ? r.o_w_base.p : (P.uniform_w ? nullptr : c.o_w.p)), (const int32_t *)c.o_cam.p, (const double *)c.cam_w.p, r.rs_bits.p, s_ip);
}
// Second half (collective), from the bit patterns in rs_bits: the median of s over all ranks (NaN with the a-priori
// scale, which selects nothing), the scale, omega' and max |omega' - omega| over all ranks.  omega_ip as s_ip above.
static void robust_from_bits(Core &c, RobustState &r, const dbat_hip_robust_options &ro, double *omega_ip, double &median, double &scale, double &maxchg) {
    const Plan &P = c.P;
    const int64_t nobs = c.nobs;
    scale = 1.0;
    median = std::nan("");
    if (ro.scale == DBAT_HIP_SCALE_MAD && P.no > 0) {
        median = robust_median(c, r);
        scale = median / ROBUST_MAD_C;
        if (scale == 0.0) scale = 1.0;
    }
    HIPCHK(hipMemsetAsync(r.rmax.p, 0, sizeof(unsigned long long), c.stream));
    if (nobs > 0)
        c.launch<k_robust_weight>(dim3(robust_grid(c)), dim3(256), 0, nobs, (const uint64_t *)r.rs_bits.p, scale, (int)ro.loss, ro.k,
                                  (const double *)(r.robust_on ? r.omega.p : nullptr), (const int64_t *)c.o_row.p, omega_ip, r.rmax.p);
    unsigned long long mb = 0;
    HIPCHK(hipMemcpyAsync(&mb, r.rmax.p, sizeof mb, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipStreamSynchronize(c.stream));
    memcpy(&maxchg, &mb, 8);
    maxchg = max_over_ranks(c, r, maxchg);
}
// One evaluation at zz (collective): both halves.
static void robust_eval(Core &c, RobustState &r, const double *zz, const dbat_hip_robust_options &ro, double *s_ip, double *omega_ip, double &scale, double &maxchg) {
    robust_scratch(c, r);
    robust_norms(c, r, zz, s_ip);
    double median;
    robust_from_bits(c, r, ro, omega_ip, median, scale, maxchg);
}
// apply the omega' of the last evaluation (same scale and loss)
static void robust_apply_eval(Core &c, RobustState &r, const dbat_hip_robust_options &ro, double scale) {
    robust_promote(c, r);
    if (c.nobs > 0)
        c.launch<k_robust_apply<true>>(dim3(robust_grid(c)), dim3(256), 0, c.nobs, (const uint64_t *)r.rs_bits.p, scale, (int)ro.loss, ro.k, r.omega.p,
                                       (const double *)r.o_w_base.p, c.o_w.p, (const int32_t *)(c.route == Core::TileRoute::sig ? r.sg_map.p : nullptr), c.sg_w.p,
                                       (const int32_t *)r.cm_map.p, c.cm_w.p);
    c.s_valid = false;
}
// omega in IP order on every rank (1 everywhere on a handle that was not promoted)
static void robust_omega_ip(Core &c, const RobustState &r, double *host) {
    const Plan &P = c.P;
    if (!r.robust_on) { std::fill(host, host + P.no, 1.0); return; }
    DevBuf<double> t;
    t.alloc((size_t)std::max<int64_t>(P.no, 1));
    HIPCHK(hipMemsetAsync(t.p, 0, (size_t)P.no * sizeof(double), c.stream));
    if (c.nobs > 0) c.launch<k_scatter_rows1>(dim3(robust_grid(c)), dim3(256), 0, c.nobs, (const int64_t *)c.o_row.p, (const double *)r.omega.p, t.p);
    if (c.multi()) c.do_allreduce(t.p, P.no);
    HIPCHK(hipMemcpyAsync(host, t.p, (size_t)P.no * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipStreamSynchronize(c.stream));
}

static const char *robust_args_error(const dbat_hip_robust_options *ro) {
    if (!ro) return "null argument";
    if (ro->loss != DBAT_HIP_LOSS_HUBER && ro->loss != DBAT_HIP_LOSS_CAUCHY) return "robust: unknown loss";
    if (!(ro->k > 0) || !std::isfinite(ro->k)) return "robust: k must be positive and finite";
    if (ro->scale != DBAT_HIP_SCALE_APRIORI && ro->scale != DBAT_HIP_SCALE_MAD) return "robust: unknown scale";
    if (ro->max_outer < 1 || ro->max_outer >= DBAT_HIP_ROBUST_MAX_OUTER) return "robust: max_outer out of range";
    if (!(ro->weight_tol >= 0) || !std::isfinite(ro->weight_tol)) return "robust: weight_tol must be finite and >= 0";
    return nullptr;
}
}  // namespace dbat

extern "C" {
int dbat_hip_default_robust_options(int32_t loss, dbat_hip_robust_options *ropt) {
    if (!ropt || (loss != DBAT_HIP_LOSS_HUBER && loss != DBAT_HIP_LOSS_CAUCHY)) { g_err = "bad loss"; return DBAT_HIP_EINVAL; }
    ropt->loss = loss;
    ropt->k = loss == DBAT_HIP_LOSS_HUBER ? 1.5 : 2.385;
    ropt->scale = DBAT_HIP_SCALE_APRIORI;
    ropt->max_outer = 10;
    ropt->weight_tol = 1e-3;
    return DBAT_HIP_OK;
}

int dbat_hip_robust_weights(dbat_hip_handle *h, const double *x, const dbat_hip_robust_options *ropt,
                            double *omega, double *s_norm, double *scale) {
    API_TRY
    if (!h || !x || !omega) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    if (const char *e = robust_args_error(ropt)) { g_err = e; return DBAT_HIP_EINVAL; }
    Core &c = *h->core;
    const Plan &P = c.P;
    DeviceGuard dev_guard(c.device);
    RobustState &r = built_once(h->rob);
    c.x_to_z(x, c.zt.p);
    DevBuf<double> om, sn;
    om.alloc((size_t)std::max<int64_t>(P.no, 1));
    HIPCHK(hipMemsetAsync(om.p, 0, (size_t)P.no * sizeof(double), c.stream));
    if (s_norm) {
        sn.alloc((size_t)std::max<int64_t>(P.no, 1));
        HIPCHK(hipMemsetAsync(sn.p, 0, (size_t)P.no * sizeof(double), c.stream));
    }
    double sc = 1.0, chg = 0.0;
    robust_eval(c, r, c.zt.p, *ropt, sn.p, om.p, sc, chg);
    if (c.multi()) {
        c.do_allreduce(om.p, P.no);
        if (s_norm) c.do_allreduce(sn.p, P.no);
    }
    HIPCHK(hipMemcpyAsync(omega, om.p, (size_t)P.no * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    if (s_norm) HIPCHK(hipMemcpyAsync(s_norm, sn.p, (size_t)P.no * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipStreamSynchronize(c.stream));
    if (scale) *scale = sc;
    return DBAT_HIP_OK;
    API_CATCH
}

int dbat_hip_set_obs_weights(dbat_hip_handle *h, const double *omega) {
    API_TRY
    if (!h) { g_err = "null handle"; return DBAT_HIP_EINVAL; }
    Core &c = *h->core;
    const Plan &P = c.P;
    DeviceGuard dev_guard(c.device);
    if (!omega) { robust_reset(*h); return DBAT_HIP_OK; }
    for (int64_t i = 0; i < P.no; ++i)
        if (!(omega[i] > 0.0 && omega[i] <= 1.0)) {
            g_err = "dbat_hip_set_obs_weights: omega[" + std::to_string(i) + "] is not in (0, 1]";
            return DBAT_HIP_EINVAL;
        }
    RobustState &r = built_once(h->rob);
    robust_promote(c, r);
    if (c.nobs > 0) {           // processing order of this rank's observations
        std::vector<double> om((size_t)c.nobs);
        for (int64_t k = 0; k < c.nobs; ++k) om[k] = omega[P.o_row[k]];
        HIPCHK(hipMemcpy(r.omega.p, om.data(), om.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    robust_apply_omega(c, r);
    HIPCHK(hipStreamSynchronize(c.stream));
    return DBAT_HIP_OK;
    API_CATCH
}

int dbat_hip_solve_robust(dbat_hip_handle *h, const dbat_hip_options *opt, const dbat_hip_robust_options *ropt,
                          double *x, dbat_hip_result *result, double *res, double *damp, double *aux, double *trace,
                          dbat_hip_robust_result *rr, double *omega_out) {
    API_TRY
    int rc;
    if (const char *e = solve_args_error(h, opt, x, result, trace, rc)) { g_err = e; return rc; }
    if (!rr) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    if (const char *e = robust_args_error(ropt)) { g_err = e; return DBAT_HIP_EINVAL; }
    Core &c = *h->core;
    if (c.chirality) { g_err = "robust solve: the chirality veto (dbat_hip_set_chirality) is not combined with the reweighting loop"; return DBAT_HIP_EUNSUPPORTED; }
    DeviceGuard dev_guard(c.device);
    RobustState &r = built_once(h->rob);
    memset(rr, 0, sizeof *rr);
    auto t0 = std::chrono::steady_clock::now();
    auto rw_clock = [&]() {
        const auto now = std::chrono::steady_clock::now();
        rr->reweight_s += std::chrono::duration<double>(now - t0).count();
    };
    robust_promote(c, r);
    robust_set_ones(c, r);
    HIPCHK(hipStreamSynchronize(c.stream));
    rw_clock();
    solve_once(c, opt, x, result, res, damp, aux, trace);
    rr->inner_iters[0] = result->iters;
    rr->outer = 1;
    for (int t = 1; t <= ropt->max_outer && result->code == 0; ++t) {
        t0 = std::chrono::steady_clock::now();
        c.x_to_z(x, c.zt.p);
        double sc = 1.0, chg = 0.0;
        robust_eval(c, r, c.zt.p, *ropt, nullptr, nullptr, sc, chg);
        rr->scale[t - 1] = sc;
        rr->max_change = chg;
        if (chg <= ropt->weight_tol) { rr->converged = 1; rw_clock(); break; }
        robust_apply_eval(c, r, *ropt, sc);
        HIPCHK(hipStreamSynchronize(c.stream));
        rw_clock();
        solve_once(c, opt, x, result, res, damp, aux, trace);
        rr->inner_iters[rr->outer++] = result->iters;
    }
    if (omega_out) robust_omega_ip(c, r, omega_out);
    return DBAT_HIP_OK;
    API_CATCH
}

/* Debug / tests: the second half of a reweighting evaluation (select, scale, weights, largest change) on the caller's
 * s instead of the residuals' (include/dbat_hip.h).  The host only places the bit patterns of this rank's observations
 * in rs_bits, in processing order; everything after that is the code of a solve. */
int dbat_hip_debug_robust_from_s(dbat_hip_handle *h, const double *s_ip, const dbat_hip_robust_options *ropt,
                                 double *omega_ip, double *median, double *scale, double *max_change, uint8_t *owned) {
    API_TRY
    if (!h || !s_ip || !scale || !max_change) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    if (const char *e = robust_args_error(ropt)) { g_err = e; return DBAT_HIP_EINVAL; }
    Core &c = *h->core;
    const Plan &P = c.P;
    for (int64_t i = 0; i < P.no; ++i)
        if (!std::isfinite(s_ip[i]) || std::signbit(s_ip[i])) {
            g_err = "dbat_hip_debug_robust_from_s: s_ip[" + std::to_string(i) + "] is not finite with the sign bit clear";
            return DBAT_HIP_EINVAL;
        }
    DeviceGuard dev_guard(c.device);
    RobustState &r = built_once(h->rob);
    robust_scratch(c, r);
    if (c.nobs > 0) {           // processing order of this rank's observations
        std::vector<uint64_t> bits((size_t)c.nobs);
        for (int64_t k = 0; k < c.nobs; ++k) memcpy(&bits[k], &s_ip[P.o_row[k]], 8);
        HIPCHK(hipMemcpy(r.rs_bits.p, bits.data(), bits.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    DevBuf<double> om;
    if (omega_ip) {
        om.alloc((size_t)std::max<int64_t>(P.no, 1));
        HIPCHK(hipMemsetAsync(om.p, 0, (size_t)P.no * sizeof(double), c.stream));
    }
    double med = 0.0, sc = 1.0, chg = 0.0;
    robust_from_bits(c, r, *ropt, om.p, med, sc, chg);
    if (omega_ip) {
        if (c.multi()) c.do_allreduce(om.p, P.no);
        HIPCHK(hipMemcpyAsync(omega_ip, om.p, (size_t)P.no * sizeof(double), hipMemcpyDeviceToHost, c.stream));
        HIPCHK(hipStreamSynchronize(c.stream));
    }
    if (median) *median = med;
    *scale = sc; *max_change = chg;
    if (owned) {
        std::fill(owned, owned + P.no, (uint8_t)0);
        for (int64_t k = 0; k < c.nobs; ++k) owned[P.o_row[k]] = 1;
    }
    return DBAT_HIP_OK;
    API_CATCH
}
}  // extern "C"
