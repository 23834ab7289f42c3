// What a caller can take out of a handle beside the solution: residuals, Jacobian blocks (all, sampled, or as a CSC
// matrix), the gradient, the column norms and J v.  Included by dbat_core.hip after Core and the handle.  The damping
// loops reach export_residuals and jtimes_rows through term_fun and keep_Jp (a caller-supplied termFun only).
#pragma once

namespace dbat {
static void export_residuals(Core &c, const double *zdev, double *r_unw, double *r_wgt, double *f) {
    // image rows via k_residual (reference row order), prior rows on the host
    DevBuf<double> tmp;
    double *dev_unw = nullptr;
    if (r_unw || r_wgt) { tmp.alloc(2 * std::max<int64_t>(c.P.no, 1)); dev_unw = tmp.p; HIPCHK(hipMemsetAsync(dev_unw, 0, 2 * c.P.no * 8, c.stream)); }
    const double ff = c.eval_f(zdev, nullptr, dev_unw);
    if (f) *f = ff;
    if (!(r_unw || r_wgt)) return;
    const Plan &P = c.P;
    // a sharded handle computes the rows of its own observations; the sum over the ranks
    // (zeros elsewhere) gives every rank the whole vector.  Weighted rows on the device
    // as well, so that the weights of the other shards' observations are not needed here.
    DevBuf<double> tmpw;
    if (r_wgt) {
        tmpw.alloc(2 * std::max<int64_t>(P.no, 1));
        HIPCHK(hipMemsetAsync(tmpw.p, 0, 2 * P.no * 8, c.stream));
        if (c.nobs > 0)
            c.launch<k_weight_rows>(dim3((unsigned)cdiv(c.nobs, 256)), dim3(256), 0, c.d, dev_unw, tmpw.p);
    }
    if (c.multi()) {
        c.do_allreduce(dev_unw, 2 * P.no);
        if (r_wgt) c.do_allreduce(tmpw.p, 2 * P.no);
    }
    const double *zfull = c.gathered(zdev);
    std::vector<double> zh(P.NZ);
    if (r_unw) HIPCHK(hipMemcpyAsync(r_unw, dev_unw, 2 * P.no * 8, hipMemcpyDeviceToHost, c.stream));
    if (r_wgt) HIPCHK(hipMemcpyAsync(r_wgt, tmpw.p, 2 * P.no * 8, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipMemcpyAsync(zh.data(), zfull, P.NZ * 8, hipMemcpyDeviceToHost, c.stream));
    c.sync();
    int64_t row = 2 * P.no;
    for (int64_t zi : P.prior_z) {
        const double e = zh[zi] - P.z_prv[zi];
        if (r_unw) r_unw[row] = e;
        if (r_wgt) r_wgt[row] = e * std::sqrt(P.z_prw[zi]);
        ++row;
    }
}

// J v (v in z layout on the device) as host rows: image rows in the reference's order, then the prior rows -- at the
// linearisation the handle holds (zlin)
static void jtimes_rows(Core &c, const double *v_dev, double *Jv) {
    const Plan &P = c.P;
    if (!c.cams_at_lin) { c.prep_cams(c.zlin.p); c.cams_at_lin = true; }
    DevBuf<double> out;
    out.alloc(2 * std::max<int64_t>(P.no, 1));
    if (c.nobs > 0) {
        c.with_model([&](auto M) { with_value<6, 14, 15, MAXCOL>(c.tile_ncx, [&](auto NCX) {
            c.launch<k_jtimes_vec<M, NCX>>(dim3((unsigned)cdiv(c.nobs, 256)), dim3(256), 0, c.d, c.zlin.p, c.cams.p, v_dev, out.p);
        }); });
    }
    std::vector<double> vz(P.NZ);
    HIPCHK(hipMemcpyAsync(Jv, out.p, 2 * P.no * 8, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipMemcpyAsync(vz.data(), v_dev, P.NZ * 8, hipMemcpyDeviceToHost, c.stream));
    c.sync();
    int64_t row = 2 * P.no;                                  // prior rows: selection rows of I, weighted (prior_obs.m:45-72)
    for (int64_t zi : P.prior_z) Jv[row++] = vz[zi] * std::sqrt(P.z_prw[zi]);
}
}  // namespace dbat

extern "C" {
int dbat_hip_residual(dbat_hip_handle *h, const double *x, double *r_unweighted, double *f) {
    API_TRY
    if (!h || !x) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    Core &c = *h->core;
    DeviceGuard dev_guard(c.device);
    c.x_to_z(x, c.zt.p);
    export_residuals(c, c.zt.p, r_unweighted, nullptr, f);
    return DBAT_HIP_OK;
    API_CATCH
}

int dbat_hip_final_residuals(dbat_hip_handle *h, double *r_unweighted, double *r_weighted) {
    API_TRY
    if (!h || !h->core->have_lin) { g_err = "no linearisation"; return DBAT_HIP_EINVAL; }
    Core &c = *h->core;
    DeviceGuard dev_guard(c.device);
    export_residuals(c, c.zlin.p, r_unweighted, r_weighted, nullptr);
    return DBAT_HIP_OK;
    API_CATCH
}

int dbat_hip_jacobian_blocks(dbat_hip_handle *h, const double *x, double *JEO, double *JOP, double *JIO) {
    API_TRY
    if (!h || !x) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    Core &c = *h->core;
    DeviceGuard dev_guard(c.device);
    const Plan &P = c.P;
    c.x_to_z(x, c.zt.p);
    c.prep_cams(c.zt.p);
    DevBuf<double> a, b, cc;
    const int64_t no = std::max<int64_t>(P.no, 1);
    if (JEO) { a.alloc(12 * no); HIPCHK(hipMemsetAsync(a.p, 0, 12 * no * 8, c.stream)); }
    if (JOP) { b.alloc(6 * no); HIPCHK(hipMemsetAsync(b.p, 0, 6 * no * 8, c.stream)); }
    if (JIO) { cc.alloc(2 * (int64_t)P.nIOrows * no); HIPCHK(hipMemsetAsync(cc.p, 0, 2 * (int64_t)P.nIOrows * no * 8, c.stream)); }
    if (c.nobs > 0) c.jac_blocks(c.zt.p, a.p, b.p, cc.p);
    if (JEO) HIPCHK(hipMemcpyAsync(JEO, a.p, 12 * P.no * 8, hipMemcpyDeviceToHost, c.stream));
    if (JOP) HIPCHK(hipMemcpyAsync(JOP, b.p, 6 * P.no * 8, hipMemcpyDeviceToHost, c.stream));
    if (JIO) HIPCHK(hipMemcpyAsync(JIO, cc.p, 2 * (int64_t)P.nIOrows * P.no * 8, hipMemcpyDeviceToHost, c.stream));
    c.sync();
    return DBAT_HIP_OK;
    API_CATCH
}

int dbat_hip_jacobian_sample(dbat_hip_handle *h, const double *x, int64_t n, const int64_t *ip_col, double *res,
                             double *JEO, double *JOP, double *JIO) {
    API_TRY
    if (!h || !x || n < 0 || (n > 0 && (!ip_col || !res || !JEO || !JOP || !JIO))) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    Core &c = *h->core;
    const Plan &P = c.P;
    if (P.nranks > 1) { g_err = "dbat_hip_jacobian_sample: one-rank handles only"; return DBAT_HIP_EUNSUPPORTED; }
    if (n == 0) return DBAT_HIP_OK;
    // IP column -> position in processing order, for the requested columns only
    std::vector<int64_t> pos((size_t)n, -1);
    {
        std::vector<std::pair<int64_t, int64_t>> want((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            if (ip_col[i] < 0 || ip_col[i] >= P.no) { g_err = "IP column out of range"; return DBAT_HIP_EINVAL; }
            want[i] = {ip_col[i], i};
        }
        std::sort(want.begin(), want.end());
        const int64_t nobs = (int64_t)P.o_row.size();
        for (int64_t o = 0; o < nobs; ++o) {
            auto it = std::lower_bound(want.begin(), want.end(), std::make_pair(P.o_row[o], (int64_t)-1));
            for (; it != want.end() && it->first == P.o_row[o]; ++it) pos[it->second] = o;
        }
        // (a one-rank plan holds every IP column; the kernel indexes the observation arrays with these positions)
        for (int64_t i = 0; i < n; ++i)
            if (pos[i] < 0) { g_err = "dbat_hip_jacobian_sample: IP column " + std::to_string(ip_col[i]) + " is not in this handle's plan"; return DBAT_HIP_EINVAL; }
    }
    DeviceGuard dev_guard(c.device);
    c.x_to_z(x, c.zt.p);
    c.prep_cams(c.zt.p);
    DevBuf<int64_t> dpos;
    dpos.upload(pos);
    const int R = P.nIOrows;
    DevBuf<double> dr, a, b, cc;
    dr.alloc(2 * n); a.alloc(12 * n); b.alloc(6 * n); cc.alloc(2 * (int64_t)R * n);
    c.with_model([&](auto M) {
        c.launch<k_jac_sample<M>>(dim3((unsigned)cdiv(n, 256)), dim3(256), 0, c.d, c.zt.p, c.cams.p, n, dpos.p, dr.p, a.p, b.p, cc.p);
    });
    HIPCHK(hipMemcpyAsync(res, dr.p, 2 * n * 8, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipMemcpyAsync(JEO, a.p, 12 * n * 8, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipMemcpyAsync(JOP, b.p, 6 * n * 8, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipMemcpyAsync(JIO, cc.p, 2 * (int64_t)R * n * 8, hipMemcpyDeviceToHost, c.stream));
    c.sync();
    return DBAT_HIP_OK;
    API_CATCH
}

int dbat_hip_jacobian_csc(dbat_hip_handle *h, const double *x, int32_t weighted, int64_t *nnz_out,
                          int64_t *colptr, int64_t *rowidx, double *val) {
    API_TRY
    if (!h || !x || !nnz_out) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    Core &c = *h->core;
    const Plan &P = c.P;
    if (P.nranks > 1) { g_err = "dbat_hip_jacobian_csc: one-rank handles only"; return DBAT_HIP_EUNSUPPORTED; }
    std::vector<int64_t> z2x((size_t)P.NZ, -1);
    for (int64_t i = 0; i < P.n; ++i) z2x[P.x2z[i]] = i;
    // columns of one observation: EO (6), IO (the camera's estimated IO columns), OP (3); -1 = no unknown
    const int R = P.nIOrows;
    auto cols_of = [&](int64_t o, int64_t *eo, int64_t *io, int *iorow, int &nio, int64_t *op) {
        const int cam = P.o_cam[o];
        for (int k = 0; k < 6; ++k) { const int32_t zc = P.cam_col[(size_t)cam * MAXCOL + k]; eo[k] = (P.cam_eo_est[cam] >> k) & 1u ? z2x[zc] : -1; }
        nio = P.cam_ncol[cam] - 6;
        for (int q = 0; q < nio; ++q) { io[q] = z2x[P.cam_col[(size_t)cam * MAXCOL + 6 + q]]; iorow[q] = P.cam_iorow[(size_t)cam * MAXIO + q]; }
        for (int k = 0; k < 3; ++k) op[k] = z2x[P.NS + 3 * (int64_t)P.o_pt[o] + k];
    };
    const int64_t nobs = (int64_t)P.o_cam.size();
    std::vector<int64_t> cnt((size_t)P.n + 1, 0);
    int64_t eo[6], io[MAXIO], op[3];
    int iorow[MAXIO], nio;
    for (int64_t o = 0; o < nobs; ++o) {
        cols_of(o, eo, io, iorow, nio, op);
        for (int k = 0; k < 6; ++k) if (eo[k] >= 0) cnt[eo[k] + 1] += 2;
        for (int q = 0; q < nio; ++q) if (io[q] >= 0) cnt[io[q] + 1] += 2;
        for (int k = 0; k < 3; ++k) if (op[k] >= 0) cnt[op[k] + 1] += 2;
    }
    for (int64_t zi : P.prior_z) cnt[z2x[zi] + 1] += 1;
    for (int64_t i = 0; i < P.n; ++i) cnt[i + 1] += cnt[i];
    *nnz_out = cnt[P.n];
    if (!colptr) return DBAT_HIP_OK;
    if (!rowidx || !val) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    DeviceGuard dev_guard(c.device);
    c.x_to_z(x, c.zt.p);
    c.prep_cams(c.zt.p);
    const int64_t no = std::max<int64_t>(P.no, 1);
    DevBuf<double> a, b, cc;
    a.alloc(12 * no); b.alloc(6 * no); cc.alloc(2 * (int64_t)R * no);
    if (c.nobs > 0) c.jac_blocks(c.zt.p, a.p, b.p, cc.p);
    std::vector<double> JEO((size_t)12 * no), JOP((size_t)6 * no), JIO((size_t)2 * R * no);
    HIPCHK(hipMemcpyAsync(JEO.data(), a.p, JEO.size() * 8, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipMemcpyAsync(JOP.data(), b.p, JOP.size() * 8, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipMemcpyAsync(JIO.data(), cc.p, JIO.size() * 8, hipMemcpyDeviceToHost, c.stream));
    c.sync();
    for (int64_t i = 0; i <= P.n; ++i) colptr[i] = cnt[i];
    std::vector<int64_t> fill(cnt.begin(), cnt.end() - 1);
    // observations in REFERENCE row order (ascending IP column), so that the rows of a column ascend
    std::vector<int64_t> by_row((size_t)nobs);
    for (int64_t o = 0; o < nobs; ++o) by_row[P.o_row[o]] = o;
    // reweighted observations (robust): the device's current weights, not the plan's
    std::vector<double> ow_dev;
    if (weighted && h->rob && h->rob->robust_on && nobs > 0) {
        ow_dev.resize((size_t)2 * nobs);
        HIPCHK(hipMemcpy(ow_dev.data(), c.o_w.p, ow_dev.size() * 8, hipMemcpyDeviceToHost));
    }
    const double *ow = ow_dev.empty() ? (P.uniform_w ? nullptr : P.o_w.data()) : ow_dev.data();
    for (int64_t k = 0; k < nobs; ++k) {
        const int64_t o = by_row[k];
        const int cam = P.o_cam[o];
        double w0 = 1.0, w1 = 1.0;
        if (weighted) { w0 = ow ? ow[2 * o] : P.cam_w[2 * cam]; w1 = ow ? ow[2 * o + 1] : P.cam_w[2 * cam + 1]; }
        cols_of(o, eo, io, iorow, nio, op);
        auto put = [&](int64_t col, double v0, double v1) {
            int64_t &f = fill[col];
            rowidx[f] = 2 * k; val[f] = v0 * w0; rowidx[f + 1] = 2 * k + 1; val[f + 1] = v1 * w1;
            f += 2;
        };
        for (int q = 0; q < 6; ++q) if (eo[q] >= 0) put(eo[q], JEO[12 * k + 2 * q], JEO[12 * k + 2 * q + 1]);
        for (int q = 0; q < nio; ++q) if (io[q] >= 0) put(io[q], JIO[2 * (int64_t)R * k + 2 * iorow[q]], JIO[2 * (int64_t)R * k + 2 * iorow[q] + 1]);
        for (int q = 0; q < 3; ++q) if (op[q] >= 0) put(op[q], JOP[6 * k + 2 * q], JOP[6 * k + 2 * q + 1]);
    }
    int64_t row = 2 * P.no;
    for (int64_t zi : P.prior_z) {                       // prior rows: selection rows of I (prior_obs.m:45-72)
        int64_t &f = fill[z2x[zi]];
        rowidx[f] = row++; val[f] = weighted ? std::sqrt(P.z_prw[zi]) : 1.0;
        ++f;
    }
    return DBAT_HIP_OK;
    API_CATCH
}

int dbat_hip_gradient(dbat_hip_handle *h, double *g) {
    API_TRY
    if (!h || !g || !h->core->have_lin) { g_err = "no linearisation"; return DBAT_HIP_EINVAL; }
    Core &c = *h->core;
    DeviceGuard dev_guard(c.device);
    c.ensure_build();                                 // (a linearisation the damping loop left to whoever needs it)
    c.gradient(c.vtmp.p);
    c.z_to_x(c.vtmp.p, g);
    return DBAT_HIP_OK;
    API_CATCH
}

int dbat_hip_colnorms(dbat_hip_handle *h, double *Jn) {
    API_TRY
    if (!h || !Jn || !h->core->have_lin) { g_err = "no linearisation"; return DBAT_HIP_EINVAL; }
    Core &c = *h->core;
    DeviceGuard dev_guard(c.device);
    c.ensure_build();                                 // (a linearisation the damping loop left to whoever needs it)
    c.colnorm2(c.vtmp.p);
    c.z_to_x(c.vtmp.p, Jn);
    for (int64_t i = 0; i < c.P.n; ++i) Jn[i] = std::sqrt(Jn[i]);
    return DBAT_HIP_OK;
    API_CATCH
}

int dbat_hip_jtimes_sqnorm(dbat_hip_handle *h, const double *v, double *sqnorm) {
    API_TRY
    if (!h || !v || !sqnorm || !h->core->have_lin) { g_err = "no linearisation"; return DBAT_HIP_EINVAL; }
    Core &c = *h->core;
    DeviceGuard dev_guard(c.device);
    c.ensure_build();                                 // (a linearisation the damping loop left to whoever needs it)
    HIPCHK(hipMemsetAsync(c.vtmp.p, 0, c.P.NZ * 8, c.stream));
    if (c.P.n) {
        HIPCHK(hipMemcpyAsync(c.xbuf.p, v, c.P.n * 8, hipMemcpyHostToDevice, c.stream));
        c.launch<k_scatter_x>(dim3((unsigned)cdiv(c.P.n, 256)), dim3(256), 0, c.P.n, c.x2z.p, c.xbuf.p, c.vtmp.p);
    }
    double a, b, vv;
    c.jtimes(c.vtmp.p, a, b, vv);
    *sqnorm = a;
    return DBAT_HIP_OK;
    API_CATCH
}

int dbat_hip_jtimes(dbat_hip_handle *h, const double *v, double *Jv) {
    API_TRY
    if (!h || !v || !Jv || !h->core->have_lin) { g_err = "no linearisation"; return DBAT_HIP_EINVAL; }
    Core &c = *h->core;
    const Plan &P = c.P;
    if (P.nranks > 1) { g_err = "dbat_hip_jtimes: one-rank handles only"; return DBAT_HIP_EUNSUPPORTED; }
    DeviceGuard dev_guard(c.device);
    c.ensure_build();                                 // (a linearisation the damping loop left to whoever needs it)
    HIPCHK(hipMemsetAsync(c.vtmp.p, 0, P.NZ * 8, c.stream));
    if (P.n) {
        HIPCHK(hipMemcpyAsync(c.xbuf.p, v, P.n * 8, hipMemcpyHostToDevice, c.stream));
        c.launch<k_scatter_x>(dim3((unsigned)cdiv(P.n, 256)), dim3(256), 0, P.n, c.x2z.p, c.xbuf.p, c.vtmp.p);
    }
    jtimes_rows(c, c.vtmp.p, Jv);
    return DBAT_HIP_OK;
    API_CATCH
}
}  // extern "C"
