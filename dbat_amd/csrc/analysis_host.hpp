// What the host sides of the network analyses share (angles_host.hpp, depth_host.hpp, quality_host.hpp).  Included by
// dbat_core.hip after Core; nothing here is on the LM step's path.
#pragma once

namespace dbat {
// The analyses look at the whole problem.  why: what a shard lacks, the clause in brackets of the message.
static bool one_rank(const Core &c, const char *what, const char *why) {
    if (c.P.nranks <= 1) return true;
    g_err = std::string(what) + ": this handle is one shard of " + std::to_string(c.P.nranks) + " (" + why + "; use a handle of the whole problem)";
    return false;
}

// The state of an analysis is built by its first call and kept with the handle; a constructor that throws leaves none.
template <class T, class... A>
static T &built_once(std::unique_ptr<T> &slot, A &&...a) {
    if (!slot) slot = std::make_unique<T>(std::forward<A>(a)...);
    return *slot;
}

// Where every point's observations start (processing order: the observations are sorted by point) and how the plan
// classified the points: the tiled ones [0, hp0) take a lane-group kernel, everything after the tiled batches (heavy
// and giant points; every point where nothing is tiled) [hp0, hp1) a workgroup each, the unobserved ones come last.
struct PointIndex {
    int32_t hp0 = 0, hp1 = 0;
    std::vector<int64_t> pos, count;                     // [np + 1] processing order; observations per point, caller's order
    DevBuf<int64_t> d_pos;
    explicit PointIndex(const Core &c) : pos((size_t)c.P.np + 1, 0), count((size_t)c.P.np, 0) {
        const Plan &P = c.P;
        for (int64_t o = 0; o < c.nobs; ++o) ++pos[(size_t)P.o_pt[o] + 1];
        for (int64_t r = 0; r < P.np; ++r) count[P.porder[r]] = pos[r + 1];
        for (int64_t r = 0; r < P.np; ++r) pos[r + 1] += pos[r];
        const int64_t ho0 = P.batch_start[std::min<int64_t>(P.nb_tiled, c.nb)];
        hp1 = c.nobs > 0 ? P.o_pt[c.nobs - 1] + 1 : 0;
        hp0 = ho0 < c.nobs ? P.o_pt[ho0] : hp1;
        d_pos.upload(pos);
    }
};

// a per-point result of the device (processing order, its first n entries computed) in the caller's order
static void scatter_points(const Core &c, const std::vector<double> &dev, int64_t n, double fill, double *out) {
    for (int64_t r = 0; r < c.P.np; ++r) out[c.P.porder[r]] = r < n ? dev[r] : fill;
}
}  // namespace dbat
