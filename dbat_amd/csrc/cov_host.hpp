// Host side of the posterior covariance and the reliability numbers at z (kernels: cov.hpp), included by dbat_core.hip
// after Core.  Nothing in a solve uses it; it borrows the engine's build and factorisation and leaves the handle without
// a linearisation.
#pragma once

namespace dbat {
// The set-up shared by posterior_cov and redundancy: the unscaled, undamped reduced system at z (and V^-1 per
// point), factored, and inv(S).  On one rank, from the compact nested-dissection factor, only the entries the blocks
// need (selected inversion, chol_df.hpp) -- no dense inverse (C4: 7.2 GB and 9 TF of rocsolver_dpotri).  The dense
// inverse remains for several ranks, for problems without the compact factor (shared EO blocks, DBAT_HIP_ND_OFF)
// and for a caller who asks for it (want_dense).  Leaves the camera records at z.
static SinvView inverse_at_z(Core &c, bool want_dense) {
    const bool selinv = c.use_perm && !c.multi() && !want_dense && c.dfchol.selinv_supported() && !env_on("DBAT_HIP_COV_DENSE");
    c.replicate_next = !selinv;                  // (domain sharding: the whole system on every rank for this one)
    try { c.build(c.z.p, 0.0, 0); } catch (...) { c.replicate_next = false; throw; }   // unscaled, undamped reduced system + V^-1 per point
    c.replicate_next = false;
    c.s_valid = false;
    SinvView SV;
    int hinfo = 0;
    if (selinv) {
        c.factor_solve_enqueue();                // the compact factor (S itself is only read)
        HIPCHK(hipMemcpyAsync(&hinfo, c.info.p, sizeof(hinfo), hipMemcpyDeviceToHost, c.stream));
        c.sync();
        if (hinfo != 0) throw DeviceError{"posterior covariance: the reduced normal matrix is not positive definite"};
        if (!c.dfchol.selected_inverse(c.stream, c.linv.p)) throw DeviceError{"out of device memory (selected inverse)"};
        HIPCHK(hipGetLastError());
        SV.tiles = c.dfchol.d_ztiles; SV.toff = c.dfchol.d_toff; SV.perm = c.dfchol.d_perm; SV.nT = c.dfchol.nT;
    } else {
        c.chol_in_place = true;
        // the in-place factorisation stores whole 64 x 64 tiles, which straddle the column envelope that the
        // next build clears: from here on S must be cleared densely -- also when the factorisation fails
        c.s_dense_dirty = true;
        c.factor_solve_enqueue();                // L in the lower triangle of S
        c.chol_in_place = false;
        HIPCHK(hipMemcpyAsync(&hinfo, c.info.p, sizeof(hinfo), hipMemcpyDeviceToHost, c.stream));
        c.sync();
        if (hinfo != 0) throw DeviceError{"posterior covariance: the reduced normal matrix is not positive definite"};
        if (!c.blas) {   // (created on first use: rocblas_create_handle costs 0.1 s, and only the dense inverse needs it)
            if (rocblas_create_handle(&c.blas) != rocblas_status_success) throw DeviceError{"rocblas_create_handle failed"};
            rocblas_set_stream(c.blas, c.stream);
        }
        if (rocsolver_dpotri(c.blas, rocblas_fill_lower, (rocblas_int)c.P.NS, c.S, (rocblas_int)c.ldS, c.info.p) != rocblas_status_success)
            throw DeviceError{"rocsolver_dpotri failed"};
        SV.dense = c.S; SV.ld = c.ldS;
    }
    c.have_lin = false;
    c.prep_cams(c.z.p);
    return SV;
}

// ---- posterior covariance blocks at z (bundle_cov.m): s0^2 * blocks of inv(J'J)
static void posterior_cov(Core &c, double s0, double *hCEO, double *hCIO, double *hCOP, double *hSinv) {
    const Plan &P = c.P;
    const SinvView SV = inverse_at_z(c, hSinv != nullptr);
    const double s02 = s0 * s0;
    DevBuf<double> dCEO, dCIO, dCOP;
    std::vector<double> cop_tmp;
    if (hCEO) dCEO.alloc((size_t)36 * P.nc);
    if (hCIO && P.nIOu > 0) dCIO.alloc((size_t)P.nIOu * P.nIOu);
    if (hCEO || (hCIO && P.nIOu > 0)) {
        const int64_t tot = 36 * (int64_t)P.nc + (int64_t)P.nIOu * P.nIOu;
        c.launch<k_cov_cam>(dim3((unsigned)cdiv(tot, 256)), dim3(256), 0, c.d, SV, s02, dCEO.p, dCIO.p);
    }
    if (hCOP) {
        dCOP.alloc((size_t)9 * P.np);
        HIPCHK(hipMemsetAsync(dCOP.p, 0, (size_t)9 * P.np * sizeof(double), c.stream));
        c.with_model([&](auto M) { with_value<false, true>(P.with_io, [&](auto IO) {
            if (c.nb > 0) c.launch<k_cov_points<M, IO>>(dim3((unsigned)c.nb), dim3(P.BT), c.lds_cov, c.d, c.z.p, c.cams.p, c.Vinv.p, SV, s02, dCOP.p, HatOut{});
            if (c.ngiant > 0) c.launch<k_cov_giant<M, IO>>(dim3((unsigned)c.ngiant), dim3(c.giant_threads), 0, c.d, c.z.p, c.cams.p, c.Vinv.p, SV, s02, dCOP.p, HatOut{});
        }); });
        if (c.multi()) c.do_allreduce(dCOP.p, (int64_t)9 * P.np);   // blocks of the other shards' points
        cop_tmp.resize((size_t)9 * P.np);
        HIPCHK(hipMemcpyAsync(cop_tmp.data(), dCOP.p, (size_t)9 * P.np * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    }
    if (hCEO) HIPCHK(hipMemcpyAsync(hCEO, dCEO.p, (size_t)36 * P.nc * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    if (hCIO && P.nIOu > 0) HIPCHK(hipMemcpyAsync(hCIO, dCIO.p, (size_t)P.nIOu * P.nIOu * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    if (hSinv)                                   // full inv(S) (lower triangle valid), NS x NS column-major, not scaled by s0^2
        HIPCHK(hipMemcpy2DAsync(hSinv, (size_t)P.NS * sizeof(double), c.S, (size_t)c.ldS * sizeof(double),
                                (size_t)P.NS * sizeof(double), (size_t)P.NS, hipMemcpyDeviceToHost, c.stream));
    c.sync();
    if (hCOP)                                    // device blocks are in processing order
        for (int64_t p = 0; p < P.np; ++p)
            std::copy(cop_tmp.begin() + 9 * (int64_t)P.pt_rank[p], cop_tmp.begin() + 9 * (int64_t)P.pt_rank[p] + 9, hCOP + 9 * p);
}

// ---- reliability at z: Qvv = I - J inv(J'J) J' on the image rows (2 x 2 per image point, caller's order: r_u, q_uv,
// r_v) and the redundancy numbers r = 1 - w_p C(p, p) of the prior rows (dbat_hip_final_residuals' row order)
static void redundancy(Core &c, double *hqvv, double *hrp) {
    const Plan &P = c.P;
    const SinvView SV = inverse_at_z(c, false);
    const int64_t nprior = (int64_t)P.prior_z.size();
    DevBuf<double> qvv, dCz, Ccc, gscr, rp;
    DevBuf<int64_t> pz;
    qvv.alloc((size_t)3 * std::max<int64_t>(P.no, 1));
    dCz.alloc((size_t)P.NZ);
    Ccc.alloc((size_t)P.nc * P.ncolmax * P.ncolmax);
    HIPCHK(hipMemsetAsync(qvv.p, 0, (size_t)3 * P.no * sizeof(double), c.stream));
    HIPCHK(hipMemsetAsync(dCz.p, 0, (size_t)P.NZ * sizeof(double), c.stream));
    const int64_t nCcc = (int64_t)P.nc * P.ncolmax * P.ncolmax;
    if (nCcc > 0) c.launch<k_hat_cam_blocks>(dim3((unsigned)cdiv(nCcc, 256)), dim3(256), 0, c.d, c.cams.p, SV, Ccc.p);
    HatOut hat;
    hat.Ccc = Ccc.p; hat.qvv = qvv.p; hat.dCz = dCz.p;
    if (c.ngiant > 0) {
        gscr.alloc((size_t)(P.giant_start.back() - P.giant_start.front()) * 9);
        hat.gscr = gscr.p;
    }
    c.with_model([&](auto M) { with_value<false, true>(P.with_io, [&](auto IO) {
        if (c.nb > 0) c.launch<k_cov_points<M, IO, true>>(dim3((unsigned)c.nb), dim3(P.BT), c.lds_cov, c.d, c.z.p, c.cams.p, c.Vinv.p, SV, 1.0, (double *)nullptr, hat);
        if (c.ngiant > 0) c.launch<k_cov_giant<M, IO, true>>(dim3((unsigned)c.ngiant), dim3(c.giant_threads), 0, c.d, c.z.p, c.cams.p, c.Vinv.p, SV, 1.0, (double *)nullptr, hat);
    }); });
    if (c.multi()) {                             // the other shards' observations and points
        c.do_allreduce(qvv.p, 3 * P.no);
        c.do_allreduce(dCz.p + P.NS, P.NZ - P.NS);
    }
    if (nprior > 0) {
        rp.alloc((size_t)nprior);
        pz.alloc((size_t)nprior);
        HIPCHK(hipMemcpyAsync(pz.p, P.prior_z.data(), (size_t)nprior * sizeof(int64_t), hipMemcpyHostToDevice, c.stream));
        c.launch<k_hat_prior>(dim3((unsigned)cdiv(nprior, 256)), dim3(256), 0, c.d, SV, pz.p, nprior, dCz.p, rp.p);
        HIPCHK(hipMemcpyAsync(hrp, rp.p, (size_t)nprior * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    }
    HIPCHK(hipMemcpyAsync(hqvv, qvv.p, (size_t)3 * P.no * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    c.sync();
}
}  // namespace dbat

extern "C" {
int dbat_hip_posterior_cov(dbat_hip_handle *h, const double *x, double sigma0, double *CEO, double *CIO,
                           double *COP, double *Sinv) {
    API_TRY
    if (!h || !x) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    Core &c = *h->core;
    DeviceGuard dev_guard(c.device);
    c.x_to_z(x, c.z.p);
    posterior_cov(c, sigma0, CEO, CIO, COP, Sinv);
    return DBAT_HIP_OK;
    API_CATCH
}

int dbat_hip_redundancy(dbat_hip_handle *h, const double *x, double *qvv_ip, double *r_prior) {
    API_TRY
    if (!h || !x || !qvv_ip || (!r_prior && !h->core->P.prior_z.empty())) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    Core &c = *h->core;
    DeviceGuard dev_guard(c.device);
    c.x_to_z(x, c.z.p);
    redundancy(c, qvv_ip, r_prior);
    return DBAT_HIP_OK;
    API_CATCH
}
}  // extern "C"
