// Host side of the relative orientation (kernels: relorient.hpp): C entry points of dbat_hip_essmat5 /
// dbat_hip_relorient.  Included by dbat_core.hip after Core; these calls take no handle.
#pragma once

namespace dbat {
// the kernels of the last call on this thread: [0] k_essmat5 [1] k_ro_score with k_ro_winner [2] the two passes of k_ro_cams
using RelorientClock = KernelClock<struct RelorientFamily, 3>;

static void ro_launch_essmat5(hipStream_t st, int64_t n_sets, const int64_t *set_start, const double *Q1, const double *Q2,
                              const int64_t *idx, double *E, int32_t *n_sol) {
    static const size_t lds = (size_t)RO_WS * RO_WG * sizeof(double);    // over 64 KiB: the kernel opts in
    HIPCHK(hipFuncSetAttribute((const void *)k_essmat5, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    launch<k_essmat5>(dim3((unsigned)cdiv(n_sets, RO_WG)), dim3(RO_WG), lds, st, n_sets, set_start, Q1, Q2, idx, E, n_sol);
}

// The four [R | +-u3] of camsfrome.m:16-33 for the winner e (e[a + 3 b]: camsfrome's E, xp' E x = 0, row-major), each
// 3 x 4 column-major, into P4[48].  The SVD by the Jacobi rotations of al_svd3; where the third singular value is zero
// al_svd3 leaves a zero column in U, and u3 = u1 x u2 is the det(U) > 0 choice of camsfrome.m:17-19 in either case.
static void ro_candidates(const double *e, double *P4) {
    double Ecm[9], U[9], V[9], s[3];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) Ecm[3 * c + r] = e[3 * r + c];
    al_svd3(Ecm, U, s, V);
    U[6] = U[1] * U[5] - U[2] * U[4]; U[7] = U[2] * U[3] - U[0] * U[5]; U[8] = U[0] * U[4] - U[1] * U[3];
    if (al_det3(V) < 0) for (int i = 0; i < 3; ++i) V[6 + i] = -V[6 + i];
    // U W V' = [u2, -u1, u3] V' (k = 0) and U W' V' = [-u2, u1, u3] V' (k = 1)
    for (int k = 0; k < 2; ++k) {
        const double sg = k == 0 ? -1.0 : 1.0;
        double R[9];
        for (int c = 0; c < 3; ++c)
            for (int r = 0; r < 3; ++r) R[3 * c + r] = sg * (U[r] * V[3 + c] - U[3 + r] * V[c]) + U[6 + r] * V[6 + c];
        for (int j = 0; j < 2; ++j) {
            double *P = P4 + 12 * (2 * k + j);
            for (int i = 0; i < 9; ++i) P[i] = R[i];
            for (int i = 0; i < 3; ++i) P[9 + i] = (j == 0 ? 1.0 : -1.0) * U[6 + i];
        }
    }
}
}  // namespace dbat

extern "C" {
int dbat_hip_essmat5(int32_t device, int32_t n_sets, const int64_t *set_start, const double *Q1, const double *Q2, double *E, int32_t *n_sol) {
    API_TRY
    if (n_sets < 0 || !set_start || !E || !n_sol) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    check_ranges_start("essmat5", set_start);
    for (int32_t s = 0; s < n_sets; ++s)
        if (set_start[s + 1] - set_start[s] < 5) refuse("essmat5", "set " + std::to_string(s) + " has fewer than five correspondences");
    const int64_t total = set_start[n_sets];
    if (total > 0 && (!Q1 || !Q2)) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    check_columns("essmat5", "correspondence", 3, total, Q1, Q2);
    BatchDevice dev(device);
    if (n_sets == 0) return DBAT_HIP_OK;
    DevBuf<int64_t> dss;
    DevBuf<double> dQ1, dQ2, dE;
    DevBuf<int32_t> dn;
    dss.upload(set_start, (size_t)n_sets + 1); dQ1.upload(Q1, (size_t)3 * total); dQ2.upload(Q2, (size_t)3 * total);
    dE.alloc((size_t)90 * n_sets); dn.alloc((size_t)n_sets);
    HIPCHK(hipMemsetAsync(dE.p, 0, (size_t)90 * n_sets * sizeof(double), dev.st));      // the slots past n_sol: zero
    EventTimer<1> ev;
    RelorientClock::start(ev, dev.st);
    ro_launch_essmat5(dev.st, n_sets, dss.p, dQ1.p, dQ2.p, nullptr, dE.p, dn.p);
    ev.lap(dev.st);
    dE.download(E); dn.download(n_sol);
    RelorientClock::ms[0] = ev.read(); RelorientClock::ms[1] = RelorientClock::ms[2] = 0;
    return DBAT_HIP_OK;
    API_CATCH
}

int dbat_hip_relorient(int32_t device, int32_t n_pairs, const int64_t *pt_start, const double *x1, const double *x2,
                       const int64_t *hyp_start, const int32_t *samples, const double *thr2, int32_t front_dir,
                       double *E, double *P2, int32_t *stats, uint8_t *inlier, uint8_t *in_front, double *X) {
    API_TRY
    const bool given = hyp_start == nullptr;          // E holds one model per pair: no samples, no scoring
    const std::vector<int64_t> no_hyp((size_t)(n_pairs > 0 ? n_pairs : 0) + 1, 0);
    if (given) hyp_start = no_hyp.data();
    if (n_pairs < 0 || !pt_start || !thr2 || !E || !P2 || !stats || !inlier || !in_front || !X) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    if (front_dir != 1 && front_dir != -1) { g_err = "relorient: front_dir must be +1 or -1"; return DBAT_HIP_EINVAL; }
    check_ranges_start("relorient", pt_start); check_ranges_start("relorient", hyp_start);
    for (int32_t p = 0; p < n_pairs; ++p) {            // (worded for the pairs: inline)
        const int64_t np_ = pt_start[p + 1] - pt_start[p], nh = hyp_start[p + 1] - hyp_start[p];
        if (np_ < 5) { g_err = "relorient: pair " + std::to_string(p) + " has fewer than five correspondences"; return DBAT_HIP_EINVAL; }
        if (nh < 0 || nh > 100000000) { g_err = "relorient: the sample ranges must ascend (at most 1e8 samples per pair)"; return DBAT_HIP_EINVAL; }
        if (np_ > 2147483647) { g_err = "relorient: more correspondences in a pair than a sample index can address"; return DBAT_HIP_EINVAL; }
        if (!(thr2[p] > 0) || !std::isfinite(thr2[p])) { g_err = "relorient: thr2 must be positive"; return DBAT_HIP_EINVAL; }
    }
    const int64_t total = pt_start[n_pairs], S = hyp_start[n_pairs];
    if (given)
        for (int64_t i = 0; i < 9 * (int64_t)n_pairs; ++i)
            if (!std::isfinite(E[i])) { g_err = "relorient: a given E is not finite"; return DBAT_HIP_EINVAL; }
    if ((total > 0 && (!x1 || !x2)) || (S > 0 && !samples)) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    check_columns("relorient", "correspondence", 2, total, x1, x2);
    std::vector<int64_t> gidx((size_t)5 * S);
    // (the sample checks of the three calls differ in order and wording, and this one runs over 5e5 samples: inline)
    for (int32_t p = 0; p < n_pairs; ++p) {
        const int64_t np_ = pt_start[p + 1] - pt_start[p];
        for (int64_t h = hyp_start[p]; h < hyp_start[p + 1]; ++h)
            for (int i = 0; i < 5; ++i) {
                const int32_t q = samples[5 * h + i];
                if (q < 0 || q >= np_) refuse("relorient", "sample index outside the pair's correspondences");
                for (int j = 0; j < i; ++j)
                    if (samples[5 * h + j] == q) refuse("relorient", "a sample repeats an index");
                gidx[(size_t)5 * h + i] = pt_start[p] + q;
            }
    }
    BatchDevice dev(device);
    if (n_pairs == 0) return DBAT_HIP_OK;
    std::vector<int64_t> tile_start((size_t)n_pairs + 1, 0);
    for (int32_t p = 0; p < n_pairs; ++p) tile_start[p + 1] = tile_start[p] + cdiv(10 * (hyp_start[p + 1] - hyp_start[p]), RO_SCORE_WG);
    const int64_t n_tiles = tile_start[n_pairs];
    if (n_tiles > 2147483647) { g_err = "relorient: too many samples for one call"; return DBAT_HIP_EINVAL; }
    DevBuf<int64_t> dps, dhs, dts, didx;
    DevBuf<double> dx1, dx2, dthr, dE, dEw, dP4, dX;
    DevBuf<int32_t> dn, dwin, dcnt, dsel;
    DevBuf<unsigned long long> dbest;
    DevBuf<uint8_t> dfr, din;
    dps.upload(pt_start, (size_t)n_pairs + 1); dhs.upload(hyp_start, (size_t)n_pairs + 1); dts.upload(tile_start); didx.upload(gidx);
    dx1.upload(x1, (size_t)2 * total); dx2.upload(x2, (size_t)2 * total); dthr.upload(thr2, (size_t)n_pairs);
    dE.alloc((size_t)90 * S); dn.alloc((size_t)S); dbest.alloc((size_t)n_pairs); dEw.alloc((size_t)9 * n_pairs); dwin.alloc((size_t)3 * n_pairs);
    dP4.alloc((size_t)48 * n_pairs); dcnt.alloc((size_t)4 * n_pairs); dsel.alloc((size_t)n_pairs);
    dX.alloc((size_t)3 * total); dfr.alloc((size_t)total); din.alloc((size_t)total);
    HIPCHK(hipMemsetAsync(dbest.p, 0, (size_t)n_pairs * sizeof(unsigned long long), dev.st));
    HIPCHK(hipMemsetAsync(dcnt.p, 0, (size_t)4 * n_pairs * sizeof(int32_t), dev.st));
    EventTimer<2> e01;
    EventTimer<1> e2;
    RelorientClock::start(e01, dev.st);
    if (S > 0) ro_launch_essmat5(dev.st, S, nullptr, dx1.p, dx2.p, didx.p, dE.p, dn.p);
    e01.lap(dev.st);
    if (n_tiles > 0) launch<k_ro_score>(dim3((unsigned)n_tiles), dim3(RO_SCORE_WG), 0, dev.st, (int)n_pairs, dts.p, dps.p, dx1.p, dx2.p, dhs.p, dE.p, dn.p, dthr.p, dbest.p);
    if (!given) launch<k_ro_winner>(dim3((unsigned)cdiv(n_pairs, 64)), dim3(64), 0, dev.st, (int)n_pairs, dhs.p, dE.p, dbest.p, dEw.p, dwin.p);
    e01.lap(dev.st);
    std::vector<int32_t> win((size_t)3 * n_pairs, 0), nsol((size_t)S), cnt((size_t)4 * n_pairs), sel((size_t)n_pairs);
    std::vector<double> P4((size_t)48 * n_pairs);
    if (given) HIPCHK(hipMemcpy(dEw.p, E, (size_t)9 * n_pairs * sizeof(double), hipMemcpyHostToDevice));   // sample 0, solution 0
    else { dEw.download(E); dwin.download(win.data()); }
    dn.download(nsol.data());                         // (empty without samples)
    double *const ms = RelorientClock::ms;
    ms[0] = e01.read(); ms[1] = e01.ms[1];
    const double nan = std::nan("");
    for (int32_t p = 0; p < n_pairs; ++p) {
        if (win[3 * p + 1] >= 0) ro_candidates(E + 9 * (size_t)p, P4.data() + 48 * (size_t)p);
        else for (int i = 0; i < 48; ++i) P4[48 * (size_t)p + i] = nan;
    }
    HIPCHK(hipMemcpy(dP4.p, P4.data(), P4.size() * sizeof(double), hipMemcpyHostToDevice));
    const dim3 cgrid((unsigned)cdiv(total, 256));
    RelorientClock::start(e2, dev.st);
    launch<k_ro_cams>(cgrid, dim3(256), 0, dev.st, (int)n_pairs, dps.p, dx1.p, dx2.p, dP4.p, (const int32_t *)nullptr, dEw.p, dthr.p, (int)front_dir, dcnt.p, dX.p, dfr.p, din.p);
    dcnt.download(cnt.data());
    for (int32_t p = 0; p < n_pairs; ++p) {
        int32_t *s = stats + 8 * (size_t)p;
        int64_t models = 0;
        for (int64_t h = hyp_start[p]; h < hyp_start[p + 1]; ++h) models += nsol[h];
        s[0] = win[3 * p]; s[1] = win[3 * p + 1]; s[2] = win[3 * p + 2]; s[3] = (int32_t)std::min<int64_t>(models, 2147483647);
        int ord[4] = {0, 1, 2, 3};                   // camsfrome.m:55: a stable sort, the first of equal counts wins
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3 - i; ++j)
                if (cnt[4 * p + ord[j]] < cnt[4 * p + ord[j + 1]]) { const int t = ord[j]; ord[j] = ord[j + 1]; ord[j + 1] = t; }
        for (int i = 0; i < 4; ++i) s[4 + i] = cnt[4 * p + ord[i]];
        sel[p] = win[3 * p + 1] >= 0 ? ord[0] : -1;
        for (int i = 0; i < 12; ++i) P2[12 * (size_t)p + i] = sel[p] >= 0 ? P4[48 * (size_t)p + 12 * sel[p] + i] : nan;
    }
    HIPCHK(hipMemcpy(dsel.p, sel.data(), sel.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    launch<k_ro_cams>(cgrid, dim3(256), 0, dev.st, (int)n_pairs, dps.p, dx1.p, dx2.p, dP4.p, (const int32_t *)dsel.p, dEw.p, dthr.p, (int)front_dir, dcnt.p, dX.p, dfr.p, din.p);
    e2.lap(dev.st);
    dX.download(X); dfr.download(in_front); din.download(inlier);
    ms[2] = e2.read();
    if (given)                                        // the count of a given model: that of its mask
        for (int32_t p = 0; p < n_pairs; ++p) {
            int32_t c = 0;
            for (int64_t g = pt_start[p]; g < pt_start[p + 1]; ++g) c += inlier[g];
            stats[8 * (size_t)p] = c; stats[8 * (size_t)p + 3] = 1;
        }
    return DBAT_HIP_OK;
    API_CATCH
}

/* Debug / measurement: dbat_hip_debug_relorient_timing(1) makes dbat_hip_essmat5 / dbat_hip_relorient on this thread
 * bracket their kernels with device events (off by default); dbat_hip_debug_relorient_ms then gives the milliseconds
 * of the last call: ms[0] the solver, ms[1] scoring and winner, ms[2] the two decomposition passes (with the small
 * copies between them). */
int dbat_hip_debug_relorient_timing(int32_t on) { return RelorientClock::set(on); }
int dbat_hip_debug_relorient_ms(double *ms) { return RelorientClock::get(ms); }
}  // extern "C"
