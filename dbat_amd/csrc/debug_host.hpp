// Debug entry points that need no handle and no device: the host plan and the host evaluation of the model, for the
// CPU unit tests.  Never used by the product path.  Included by dbat_core.hip (plan.hpp, heavy.hpp and model.hpp are
// all they read).
#pragma once

extern "C" {
/* Digest of the host plan (debug / CPU tests only: the plan must be identical bit for bit whatever the number of
 * threads that built it).  out[k] = FNV-1a hash of the k-th field of Plan in the order of plan_digest_names(). */
#define DBAT_PLAN_FIELDS(X)                                                                                           \
    X(x2z) X(io_src) X(io_fixed) X(z_est) X(z_prw) X(z_prv) X(z_mine) X(z0) X(prior_z) X(porder) X(pt_rank) X(o_cam)    \
    X(o_pt) X(o_uv) X(o_w) X(o_seg) X(o_row) X(batch_start) X(o_lc) X(o_pidx) X(tile_batch) X(tile_cam_start)           \
    X(tile_order) X(tile_cams) X(cm_pt) X(cm_uv) X(cm_w) X(cm_chunk_cam) X(cm_chunk_start) X(giant_start)               \
    X(tile_io_start) X(tile_iocols) X(tile_cam_io) X(tile_io_simple) X(sg_chunk) X(sg_tile_chunk0) X(sg_lc) X(sg_gcam)  \
    X(sg_uv) X(sg_w) X(cam_w) X(cam_ncol) X(cam_col) X(cam_iorow) X(cam_eo_est) X(px) X(cam_first) X(cam_adj)
int dbat_hip_debug_plan_digest(const dbat_hip_problem *prob, uint64_t *out, int32_t n_out, char *names, int32_t names_len) {
    API_TRY
    if (!prob || !out) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    Plan P;
    if (!build_plan(*prob, P, true)) { g_err = P.err; return DBAT_HIP_EINVAL; }
    auto fnv = [](const void *p, size_t n) {
        uint64_t h = 1469598103934665603ull;
        const unsigned char *b = (const unsigned char *)p;
        for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
        return h ^ (uint64_t)n;
    };
    std::vector<uint64_t> hs;
    std::string nm;
#define X(F) hs.push_back(fnv(P.F.data(), P.F.size() * sizeof(P.F[0]))); nm += #F ",";
    DBAT_PLAN_FIELDS(X)
#undef X
    hs.push_back(fnv(P.nd.order.data(), P.nd.order.size() * sizeof(int))); nm += "nd.order,";
    hs.push_back(fnv(P.nd.block_end.data(), P.nd.block_end.size() * sizeof(int))); nm += "nd.block_end,";
    hs.push_back(fnv(P.nd.cam_owner.data(), P.nd.cam_owner.size() * sizeof(int))); nm += "nd.cam_owner,";
    const int64_t sc[] = {P.n, P.m, P.NS, P.NZ, P.nIOu, P.pt_lo, P.pt_hi, P.CMAX, P.nb_tiled, P.n_cm_chunks_tiled, P.sg_kmax, P.sg_rows_max,
                          P.sg_ngroups, P.sg_npoints, P.sg_ok, P.sg_backsub_ok, P.BT, P.ncolmax, P.with_io, P.uniform_w, P.all_std8, P.max_k,
                          P.shared_eo, P.rank_ok, P.order_dims, P.mg_subtree, P.n_tiles_io_simple, P.n_prior[0], P.n_prior[1], P.n_prior[2]};
    hs.push_back(fnv(sc, sizeof(sc))); nm += "scalars";
    if ((int)hs.size() > n_out) { g_err = "digest buffer too small"; return DBAT_HIP_EINVAL; }
    for (size_t i = 0; i < hs.size(); ++i) out[i] = hs[i];
    for (int i = (int)hs.size(); i < n_out; ++i) out[i] = 0;
    if (names && names_len > 0) snprintf(names, (size_t)names_len, "%s", nm.c_str());
    return (int)hs.size();
    API_CATCH
}

/* Host only (debug / CPU unit tests; never used by the product path): the index structures of the heavy / giant points
 * (Plan::hv_*, csrc/heavy.hpp) checked against their definition.  Every row of Z that k_heavy_z would write gets a
 * pseudo-random value (a hash of its point, its row of the reduced system and its k-column) at the place the plan gives
 * it; the tasks of k_heavy_syrk are then replayed on the host (same operand places, same flush rules) and compared with
 * the plain sum over the points of z_p z_p' over ALL their rows.  out[8]: { 1 if the plan takes the path, untiled points,
 * row groups, tasks, k-steps, largest absolute difference, largest absolute entry, number of compared entries }. */
int dbat_hip_debug_heavy_plan_selftest(const dbat_hip_problem *prob, double *out) {
    API_TRY
    if (!prob || !out) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    Plan P;
    if (!build_plan(*prob, P, true)) { g_err = P.err; return DBAT_HIP_EINVAL; }
    for (int i = 0; i < 8; ++i) out[i] = 0.0;
    if (!P.hv_ok) return DBAT_HIP_OK;
    const int64_t NS = P.NS;
    if (NS > 4000) { g_err = "selftest: reduced system too large for the dense host check"; return DBAT_HIP_EINVAL; }
    auto val = [](int64_t pt, int64_t row, int c) {
        uint64_t h = (uint64_t)pt * 0x9E3779B97F4A7C15ull ^ (uint64_t)(row + 1) * 0xC2B2AE3D27D4EB4Full ^ (uint64_t)(c + 1) * 0x165667B19E3779F9ull;
        h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
        return (double)(int64_t)(h % 2001) / 1000.0 - 1.0;
    };
    std::vector<double> Zs((size_t)P.hv_z_doubles, 0.0);
    std::vector<double> ref((size_t)(NS + 1) * (NS + 1), 0.0), got((size_t)(NS + 1) * (NS + 1), 0.0);
    const int64_t ho0 = P.hv_obs0, ho1 = (int64_t)P.o_cam.size();
    // rows of every point: (row of the reduced system, values of the three k-columns)
    std::vector<int64_t> prow; std::vector<double> pval;
    int64_t o = ho0;
    while (o < ho1) {
        const int32_t pt = P.o_pt[o];
        const int32_t hp = pt - P.hv_pt0;
        prow.clear(); pval.clear();
        std::vector<int32_t> slot_row((size_t)(P.hv_pt_io0[hp + 1] - P.hv_pt_io0[hp]), -1);
        int64_t oe = o;
        for (; oe < ho1 && P.o_pt[oe] == pt; ++oe) {
            const int32_t c = P.o_cam[oe];
            const int32_t dst = P.hv_obs_dst[oe - ho0];
            const int ld = P.hv_obs_ld[oe - ho0];
            for (int a = 0; a < 6; ++a) {
                const int64_t row = P.cam_col[(size_t)c * MAXCOL + a];
                prow.push_back(row);
                for (int k = 0; k < 3; ++k) { const double v = val(pt, row, k); pval.push_back(v); Zs[(size_t)dst + (size_t)k * ld + a] = v; }
            }
            for (int q = 6; q < P.cam_ncol[c]; ++q) {
                const int sl = P.hv_obs_ioloc[(size_t)(oe - ho0) * Plan::HV_NIOC + (q - 6)];
                if (sl >= (int)slot_row.size()) { g_err = "selftest: IO slot out of range"; return DBAT_HIP_EINVAL; }
                const int32_t row = P.cam_col[(size_t)c * MAXCOL + q];
                if (slot_row[sl] >= 0 && slot_row[sl] != row) { g_err = "selftest: two IO columns in one slot"; return DBAT_HIP_EINVAL; }
                slot_row[sl] = row;
            }
        }
        for (size_t sl = 0; sl < slot_row.size(); ++sl) {
            if (slot_row[sl] < 0) { g_err = "selftest: IO slot without a column"; return DBAT_HIP_EINVAL; }
            const int gs = P.hv_pt_io0[hp] + (int)sl;
            if (P.hv_io_pt[gs] != hp) { g_err = "selftest: IO slot of another point"; return DBAT_HIP_EINVAL; }
            prow.push_back(slot_row[sl]);
            for (int k = 0; k < 3; ++k) { const double v = val(pt, slot_row[sl], k); pval.push_back(v); Zs[(size_t)P.hv_io_dst[gs] + (size_t)k * P.hv_io_ld[gs]] = v; }
        }
        prow.push_back(NS);
        for (int k = 0; k < 3; ++k) { const double v = val(pt, NS, k); pval.push_back(v); Zs[(size_t)P.hv_pt_y[2 * hp] + (size_t)k * P.hv_pt_y[2 * hp + 1]] = v; }
        for (size_t a = 0; a < prow.size(); ++a)
            for (size_t b = 0; b < prow.size(); ++b) {
                const int64_t ri = prow[a], rj = prow[b];
                if (ri < rj || (ri == NS && rj == NS)) continue;
                ref[(size_t)rj * (NS + 1) + ri] -= pval[3 * a] * pval[3 * b] + pval[3 * a + 1] * pval[3 * b + 1] + pval[3 * a + 2] * pval[3 * b + 2];
            }
        o = oe;
    }
    // the tasks, as k_heavy_syrk runs them
    int64_t nks_all = 0;
    for (int t = 0; t < P.hv_ntasks; ++t) {
        const int gi = P.hv_task[4 * t], gj = P.hv_task[4 * t + 1], ks0 = P.hv_task[4 * t + 2], nks = P.hv_task[4 * t + 3];
        const int nbi = P.hv_grp_nb[gi], nbj = P.hv_grp_nb[gj];
        nks_all += nks;
        std::vector<double> acc((size_t)48 * 48, 0.0);
        for (int ks = 0; ks < nks; ++ks)
            for (int kk = 0; kk < 4; ++kk) {
                const int32_t *op = P.hv_ops.data() + ((size_t)(ks0 + ks) * 4 + kk) * 2;
                if ((op[0] < 0) != (op[1] < 0)) { g_err = "selftest: half an operand"; return DBAT_HIP_EINVAL; }
                if (op[0] < 0) continue;
                for (int i = 0; i < 16 * nbi; ++i)
                    for (int j = 0; j < 16 * nbj; ++j) acc[(size_t)i * 48 + j] += Zs[(size_t)op[0] + i] * Zs[(size_t)op[1] + j];
            }
        for (int i = 0; i < 16 * nbi; ++i)
            for (int j = 0; j < 16 * nbj; ++j) {
                if (gi == gj && i < j) continue;
                const int32_t ri = P.hv_grp_row[(size_t)gi * 48 + i], cj = P.hv_grp_row[(size_t)gj * 48 + j];
                if (ri < 0 || cj < 0 || cj == NS) continue;
                if (ri < cj) { g_err = "selftest: rows of the groups are not ascending"; return DBAT_HIP_EINVAL; }
                got[(size_t)cj * (NS + 1) + ri] -= acc[(size_t)i * 48 + j];
            }
    }
    double dmax = 0, vmax = 0; int64_t ncmp = 0;
    for (size_t i = 0; i < ref.size(); ++i) {
        dmax = std::max(dmax, std::fabs(ref[i] - got[i])); vmax = std::max(vmax, std::fabs(ref[i]));
        ncmp += ref[i] != 0.0;
    }
    out[0] = 1; out[1] = P.hv_npts; out[2] = P.hv_ngroups; out[3] = P.hv_ntasks; out[4] = (double)nks_all;
    out[5] = dmax; out[6] = vmax; out[7] = (double)ncmp;
    return DBAT_HIP_OK;
    API_CATCH
}

/* Host only (debug / CPU unit tests): the sizes of the batches of the plan.  out[16]: for the tiled batches {most points
 * of one batch, most observations of one batch, batches closed by Plan::PMAX rather than by BT, most batches of one
 * tile}, the same four for the batches after the tiles (heavy points; every batch when nothing is tiled; the last
 * entry 0), then {BT, Plan::PMAX, the plan's cap of batches per tile, tiled batches, untiled batches}, zeros. */
int dbat_hip_debug_batch_stats(const dbat_hip_problem *prob, int64_t *out) {
    API_TRY
    if (!prob || !out) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    Plan P;
    if (!build_plan(*prob, P, true)) { g_err = P.err; return DBAT_HIP_EINVAL; }
    for (int i = 0; i < 16; ++i) out[i] = 0;
    const int64_t nb = (int64_t)P.batch_start.size() - 1;
    for (int64_t b = 0; b < nb; ++b) {
        const int64_t o0 = P.batch_start[b], o1 = P.batch_start[b + 1];
        if (o1 <= o0) continue;
        int64_t *st = out + (b < P.nb_tiled ? 0 : 4);
        st[0] = std::max<int64_t>(st[0], (int64_t)P.o_pidx[o1 - 1] + 1);
        st[1] = std::max<int64_t>(st[1], o1 - o0);
    }
    out[2] = P.nb_pcap[0]; out[6] = P.nb_pcap[1];
    for (size_t t = 0; P.nb_tiled > 0 && t + 1 < P.tile_batch.size(); ++t)
        out[3] = std::max<int64_t>(out[3], P.tile_batch[t + 1] - P.tile_batch[t]);
    out[8] = P.BT; out[9] = Plan::PMAX; out[10] = P.tile_bmax; out[11] = P.nb_tiled; out[12] = nb - P.nb_tiled;
    return DBAT_HIP_OK;
    API_CATCH
}

/* Host only (debug / CPU unit tests): the nested dissection with the separators of `mode` (nd.hpp: 0, 1, 2) and with the
 * ones the model chooses (whatever DBAT_HIP_ND_SEP says), each laid out in tiles and scored on the host.  out[24], twelve
 * numbers for the requested mode and twelve for the choice: { cameras, blocks, tile columns, tiles, longest chain (depth
 * of the elimination tree in tile columns), tile products (without the right-hand-side row), modelled time (us), the mode,
 * nd_check (0: a permutation whose co-visible cameras always lie on one root path of the block tree), longest run of
 * consecutive columns, model (0: list schedule, 1: chain / products estimate), 0 }. */
int dbat_hip_debug_nd_stats(const dbat_hip_problem *prob, int32_t mode, double *out) {
    API_TRY
    if (!prob || !out || mode < 0 || mode > 2) { g_err = "null argument or mode not 0, 1, 2"; return DBAT_HIP_EINVAL; }
    Plan P;
    if (!build_plan(*prob, P, false)) { g_err = P.err; return DBAT_HIP_EINVAL; }
    const bool nd_off = env_on("DBAT_HIP_ND_OFF");
    const int nparts = P.mg_subtree ? P.nranks : 1;
    auto put = [&](const NdTree &T, NdScore sc, int m, double *o) {
        if (sc.mode != m) df_score_order(P.nc, P.nIOu, P.cam_adj.data(), P.cam_adj_words, T, sc);
        const double v[12] = {(double)sc.cams, (double)sc.blocks, (double)sc.tile_cols, (double)sc.tiles, (double)sc.chain, (double)sc.products,
                              sc.model_us, (double)m, (double)nd_check(P.nc, P.cam_adj.data(), P.cam_adj_words, T), (double)sc.run, (double)sc.model, 0.0};
        std::copy(v, v + 12, o);
    };
    NdTree T;
    nd_build(P.nc, P.cam_adj.data(), P.cam_adj_words, P.nd_xyz.data(), P.nd_weight.data(), nparts, P.nd_leaf, nd_off, mode, T);
    put(T, NdScore(), mode, out);
    NdScore sc[3];
    const int chosen = nd_select(P.nc, P.nIOu, P.cam_adj.data(), P.cam_adj_words, P.nd_xyz.data(), P.nd_weight.data(), nparts, P.nd_leaf, nd_off,
                                 -1, true, T, sc);
    put(T, sc[chosen], chosen, out + 12);
    return DBAT_HIP_OK;
    API_CATCH
}

/* Host only (debug / CPU unit tests): the schedule of the factorisation in the compact layout on one rank, as the
 * handle would build it for this problem (the plan's dissection, DBAT_HIP_DF_SUMS / DBAT_HIP_DF_MERGE honoured) -- see
 * include/dbat_hip.h. */
int dbat_hip_debug_df_schedule(const dbat_hip_problem *prob, int64_t *hdr, double *cand_us, int32_t *jobs, int64_t jobs_cap,
                               int32_t *plist, int64_t plist_cap, uint64_t *rowbits, int64_t rowbits_cap) {
    API_TRY
    if (!prob || !hdr || !cand_us) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    Plan P;
    if (!build_plan(*prob, P, false)) { g_err = P.err; return DBAT_HIP_EINVAL; }
    if (P.shared_eo || P.nd.nparts > 1) { g_err = "df_schedule: the compact layout on one rank only"; return DBAT_HIP_EINVAL; }
    DataflowChol D;
    DataflowChol::Symbolic Y;
    D.symbolic_permuted(P.nc, P.nIOu, P.cam_adj.data(), P.cam_adj_words, P.nd, Y);
    DataflowChol::Sched H;
    D.schedule_host(Y.rb, Y.col_owner, 0, H);
    int64_t nlisted = 0;
    for (const DfJob &j : D.h_tasks) nlisted += (j.mode & DF_LISTED) != 0;
    const int64_t h[16] = {D.nT, D.W, D.ntasks, (int64_t)D.h_plist.size(), D.cand_taken, D.nparts, D.n_products, D.use_chain ? 1 : 0,
                           D.nchain, nlisted, DF_LISTED, (int64_t)Y.rb.size(), 0, 0, 0, 0};
    std::copy(h, h + 16, hdr);
    std::copy(D.cand_us, D.cand_us + 4, cand_us);
    if (jobs) {
        if (jobs_cap < (int64_t)D.h_tasks.size() * 8) { g_err = "df_schedule: task buffer too small"; return DBAT_HIP_EINVAL; }
        static_assert(sizeof(DfJob) == 8 * sizeof(int32_t), "DfJob is eight ints");
        if (!D.h_tasks.empty()) memcpy(jobs, D.h_tasks.data(), D.h_tasks.size() * sizeof(DfJob));
    }
    if (plist) {
        if (plist_cap < (int64_t)D.h_plist.size()) { g_err = "df_schedule: list buffer too small"; return DBAT_HIP_EINVAL; }
        std::copy(D.h_plist.begin(), D.h_plist.end(), plist);
    }
    if (rowbits) {
        if (rowbits_cap < (int64_t)Y.rb.size()) { g_err = "df_schedule: pattern buffer too small"; return DBAT_HIP_EINVAL; }
        std::copy(Y.rb.begin(), Y.rb.end(), rowbits);
    }
    return DBAT_HIP_OK;
    API_CATCH
}

/* Host evaluation of the per-observation model (debug / CPU unit tests of
 * model.hpp only; never used by the product path). */
int dbat_hip_debug_model_eval_host(int32_t model, int32_t nK, int32_t nP, const double *EO6, const double *IO,
                                   double px_size, const double *Q3, const double *uv, double *r2,
                                   double *A12, double *B6, double *C /* 2 x nIOrows */) {
    if (model < 2 || model > 5 || nK < 0 || nK > MAXK || nP < 0 || nP > MAXP) { g_err = "bad model"; return DBAT_HIP_EINVAL; }
    CamRec c{};
    c.c[0] = EO6[0]; c.c[1] = EO6[1]; c.c[2] = EO6[2];
    cam_rotation(EO6 + 3, c.Mt, c.sk, c.ck);
    c.f = IO[0]; c.pp[0] = IO[1]; c.pp[1] = IO[2]; c.b[0] = IO[3]; c.b[1] = IO[4];
    for (int k = 0; k < nK; ++k) c.K[k] = IO[5 + k];
    for (int k = 0; k < nP; ++k) c.P[k] = IO[5 + nK + k];
    c.sz = px_size;
    double r[2], A[2][6], B[2][3], Cf[2][MAXIO];
    switch (model) {
        case 2: obs_eval<2, true, true>(c, nK, nP, Q3, uv[0], uv[1], r, A, B, Cf); break;
        case 3: obs_eval<3, true, true>(c, nK, nP, Q3, uv[0], uv[1], r, A, B, Cf); break;
        case 4: obs_eval<4, true, true>(c, nK, nP, Q3, uv[0], uv[1], r, A, B, Cf); break;
        default: obs_eval<5, true, true>(c, nK, nP, Q3, uv[0], uv[1], r, A, B, Cf); break;
    }
    r2[0] = r[0]; r2[1] = r[1];
    for (int k = 0; k < 6; ++k) { A12[2 * k] = A[0][k]; A12[2 * k + 1] = A[1][k]; }
    for (int k = 0; k < 3; ++k) { B6[2 * k] = B[0][k]; B6[2 * k + 1] = B[1][k]; }
    for (int k = 0; k < 5 + nK + nP; ++k) { C[2 * k] = Cf[0][k]; C[2 * k + 1] = Cf[1][k]; }
    return DBAT_HIP_OK;
}
}  // extern "C"
