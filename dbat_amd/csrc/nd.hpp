// Nested dissection of the camera co-visibility graph (host only).
//
// One ordering serves two purposes:
//   * the elimination order of the reduced camera system in the dataflow Cholesky
//     (chol_df.hpp): independent parts of the camera network factor concurrently, only the
//     separators form a dependent chain;
//   * multi-GPU: the first levels of the same tree cut the network into one DOMAIN per rank
//     and a few TOP separators.  A separator is the set of cameras of one half that see a
//     camera of the other half, so an object point never sees interior cameras of two
//     domains (two such cameras would be co-visible and one of them in the separator):
//     every point belongs to the one domain whose interior cameras it sees, its block of
//     the reduced system touches only that domain's rows and the top separators' rows, and
//     a rank can build AND factor its domain without a word from the others.  Only the
//     Schur complement on the top separators is summed over the ranks.
//
// The cuts BETWEEN the ranks take that one-sided boundary layer (the lower half's cameras that
// see the upper half), at a position that balances the observations.  INSIDE a rank's domain
// the separators are what the dependent chain of the factorisation is made of, and the
// boundary layer is not the smallest set that separates the halves.  There (sep_mode):
//   0  the lower half's boundary at the median (the rule of the rank cuts);
//   1  at the median, the best of: the lower boundary, the upper boundary, and the minimum
//      vertex cover of the bipartite graph between the two boundaries (Koenig's theorem: from
//      a maximum matching; no smaller set of cameras separates the halves at that cut);
//   2  the same three at five positions around the median (0, +-2.5 %, +-5 % of the part).
// The best candidate has the fewest 64-row tiles of separator rows, then the fewest cameras,
// then the most even parts; ties go to the earlier candidate (median first, lower boundary
// first), so mode 1 and 2 fall back to the separator of mode 0 wherever nothing is smaller.
// Which mode a problem gets is decided by the model of the factorisation (nd_select below): a
// shorter chain of tile columns is not always a shorter factorisation -- a cover takes cameras
// from both halves, the two parts then end at the same time, and the separator's first column
// waits for both (profiles/nd_separators.md; chol_df.hpp cuts the sums of such columns).
// Everything here is serial and works on sorted camera lists: the order does not depend on
// the number of threads of the plan.
//
// No counterpart in the reference (MATLAB's `\` orders and factors J'J internally,
// gauss_newton_armijo.m:172); the closest structure is the permuted block factor
// [OP; EO; IO] of bundle_cov.m:82-99.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <functional>
#include <vector>

namespace dbat {

struct NdTree {
    int nparts = 1;
    std::vector<int> order;         // position -> camera
    std::vector<int> block_end;     // order.size() after every block (leaf or separator), in elimination order
    std::vector<int> block_owner;   // per block: the rank whose domain it belongs to, -1: a top separator
    std::vector<uint8_t> block_sep; // per block: a separator -- it directly follows the last block of the part it was cut from
    std::vector<int> block_first;   // per block: the first block of the part it closes (a leaf: itself) -- blocks
                                    // block_first[b] .. b are the subtree of b, all of them eliminated before it
    std::vector<int> cam_owner;     // per camera: rank, -1: top separator
    int n_top_cams = 0;
};

// Minimum vertex cover of the bipartite graph between L and R (both ascending by camera; every camera of L sees one of
// R and the reverse), by augmenting paths in ascending camera order.  inL / inR: the cameras of the cover.
inline void nd_min_cover(const std::vector<int> &L, const std::vector<int> &R, const uint64_t *adj, int adj_words,
                         std::vector<int> &ridx /* nc entries, all -1 on entry and on return */,
                         std::vector<uint8_t> &inL, std::vector<uint8_t> &inR) {
    const int nl = (int)L.size(), nr = (int)R.size();
    for (int r = 0; r < nr; ++r) ridx[R[r]] = r;
    std::vector<int> ptr(nl + 1, 0), nb;                // neighbours of every camera of L in R, ascending
    for (int l = 0; l < nl; ++l) {
        const uint64_t *row = adj + (size_t)L[l] * adj_words;
        for (int w = 0; w < adj_words; ++w) {
            uint64_t m = row[w];
            while (m) {
                const int b = 64 * w + __builtin_ctzll(m);
                m &= m - 1;
                if (ridx[b] >= 0) nb.push_back(ridx[b]);
            }
        }
        ptr[l + 1] = (int)nb.size();
    }
    for (int r = 0; r < nr; ++r) ridx[R[r]] = -1;
    std::vector<int> matchL(nl, -1), matchR(nr, -1), seen(nr, -1), it(nl, 0), via(nl, -1), stack;
    for (int l0 = 0; l0 < nl; ++l0) {                   // Kuhn's algorithm, the search kept on an explicit stack
        stack.assign(1, l0); it[l0] = ptr[l0];
        while (!stack.empty()) {
            const int l = stack.back();
            if (it[l] == ptr[l + 1]) { stack.pop_back(); continue; }
            const int r = nb[it[l]++];
            if (seen[r] == l0) continue;
            seen[r] = l0; via[l] = r;
            if (matchR[r] < 0) {                        // augment: every camera on the stack takes the one of R it went through
                for (int lq : stack) { matchL[lq] = via[lq]; matchR[via[lq]] = lq; }
                break;
            }
            it[matchR[r]] = ptr[matchR[r]];
            stack.push_back(matchR[r]);
        }
    }
    // Koenig: Z = what alternating paths reach from the unmatched cameras of L; cover = (L \ Z) + (R & Z)
    std::vector<uint8_t> zl(nl, 0), zr(nr, 0);
    stack.clear();
    for (int l = 0; l < nl; ++l) if (matchL[l] < 0) { zl[l] = 1; stack.push_back(l); }
    while (!stack.empty()) {
        const int l = stack.back(); stack.pop_back();
        for (int q = ptr[l]; q < ptr[l + 1]; ++q) {
            const int r = nb[q];
            if (zr[r]) continue;
            zr[r] = 1;
            const int l2 = matchR[r];
            if (l2 >= 0 && !zl[l2]) { zl[l2] = 1; stack.push_back(l2); }
        }
    }
    inL.assign(nl, 0); inR.assign(nr, 0);
    for (int l = 0; l < nl; ++l) inL[l] = !zl[l];
    for (int r = 0; r < nr; ++r) inR[r] = zr[r];
}

// adj: symmetric co-visibility bitsets (adj_words 64-bit words per camera); xyz: 3 coordinates per
// camera (projection centres) for the geometric bisection; weight (may be null): observations per
// camera, balances the domains; nparts: ranks; leaf: cameras of a block that is not cut further;
// sep_mode: the separators inside a rank's domain (0, 1, 2: the header comment).
inline void nd_build(int nc, const uint64_t *adj, int adj_words, const double *xyz, const double *weight,
                     int nparts, int leaf, bool nd_off, int sep_mode, NdTree &T) {
    T = NdTree();
    T.nparts = std::max(1, nparts);
    T.order.reserve(nc);
    T.cam_owner.assign(nc, 0);
    auto emit = [&](std::vector<int> &cams, int owner, bool sep = false, int first = -1) {
        std::sort(cams.begin(), cams.end());
        for (int c : cams) { T.order.push_back(c); T.cam_owner[c] = owner; if (owner < 0) ++T.n_top_cams; }
        if (!cams.empty()) {
            T.block_first.push_back(first >= 0 ? first : (int)T.block_end.size());
            T.block_end.push_back((int)T.order.size()); T.block_owner.push_back(owner); T.block_sep.push_back(sep ? 1 : 0);
        }
    };
    std::vector<uint64_t> maskA((size_t)adj_words), maskB((size_t)adj_words);
    std::vector<int> ridx((size_t)nc, -1);
    // part0 .. part0+np-1: the ranks this set of cameras is divided among
    std::function<void(std::vector<int> &, int, int)> nd = [&](std::vector<int> &cams, int part0, int np) {
        if (cams.empty()) return;
        if (np == 1 && (int)cams.size() <= leaf) { emit(cams, part0); return; }
        double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
        for (int c : cams) for (int d = 0; d < 3; ++d) { lo[d] = std::min(lo[d], xyz[3 * c + d]); hi[d] = std::max(hi[d], xyz[3 * c + d]); }
        int ax = 0;
        for (int d = 1; d < 3; ++d) if (hi[d] - lo[d] > hi[ax] - lo[ax]) ax = d;
        std::vector<int> s(cams);
        std::stable_sort(s.begin(), s.end(), [&](int a, int b) { return xyz[3 * a + ax] < xyz[3 * b + ax]; });
        size_t half = s.size() / 2;
        const int npa = np / 2, npb = np - npa;
        std::vector<int> A, B, Sep, A2, B2;
        // the cameras of `from` (part of s) that see a camera of the set `mask`: touch; the others: rest
        auto boundary = [&](const int *from, size_t n, const std::vector<uint64_t> &mask, std::vector<int> &touch, std::vector<int> &rest) {
            touch.clear(); rest.clear();
            for (size_t q = 0; q < n; ++q) {
                const uint64_t *row = adj + (size_t)from[q] * adj_words;
                uint64_t any = 0;
                for (int w = 0; w < adj_words && !any; ++w) any = row[w] & mask[w];
                (any ? touch : rest).push_back(from[q]);
            }
        };
        auto set_masks = [&](size_t h) {
            std::fill(maskA.begin(), maskA.end(), 0); std::fill(maskB.begin(), maskB.end(), 0);
            for (size_t q = 0; q < h; ++q) maskA[s[q] >> 6] |= 1ull << (s[q] & 63);
            for (size_t q = h; q < s.size(); ++q) maskB[s[q] >> 6] |= 1ull << (s[q] & 63);
        };
        auto cut = [&](size_t h) {                      // lower part A = s[0, h), separator = the cameras of A that see B
            set_masks(h);
            B.assign(s.begin() + h, s.end()); B2 = B;
            boundary(s.data(), h, maskB, Sep, A2);
        };
        if (np > 1) {
            // The cut between the ranks.  The separator comes out of the lower part, so the cut is moved until
            // what REMAINS of it carries npa / np of the two interiors' weight (observations): bisection on the
            // position (the interior of A grows with it).
            auto wsum = [&](const std::vector<int> &v) { double t = 0; for (int c : v) t += weight ? weight[c] : 1.0; return t; };
            size_t lo = 1, hi = s.size() - 1;
            half = std::min(std::max<size_t>(s.size() * npa / np, lo), hi);
            for (int it = 0; it < 16 && lo < hi; ++it) {
                cut(half);
                const double wa = wsum(A2) / npa, wb = wsum(B) / npb;
                if (wa < wb) lo = half + 1; else hi = half;
                const size_t next = (lo + hi) / 2;
                if (next == half) break;
                half = next;
            }
            half = std::min(std::max<size_t>(half, 1), s.size() - 1);
        }
        cut(half);
        if (np == 1 && sep_mode > 0) {
            // Candidates inside a domain: positions x {lower boundary, upper boundary, minimum cover}.  Key: tiles of
            // separator rows, cameras, imbalance of the parts; the first of equals stays.
            const long n = (long)s.size();
            const long slide[5] = {0, -(n / 40), n / 40, -(n / 20), n / 20};
            const int npos = sep_mode >= 2 ? 5 : 1;
            long best_key[3] = {0, 0, 0};
            bool have = false;
            std::vector<int> bA, bB, bS, La, Lb, Ia, Ib, cS, cA, cB;
            std::vector<uint8_t> inL, inR;
            auto offer = [&](const std::vector<int> &Sc, const std::vector<int> &Ac, const std::vector<int> &Bc) {
                const long key[3] = {(6 * (long)Sc.size() + 63) / 64, (long)Sc.size(), std::labs((long)Ac.size() - (long)Bc.size())};
                if (have && !std::lexicographical_compare(key, key + 3, best_key, best_key + 3)) return;
                have = true; std::copy(key, key + 3, best_key);
                bS = Sc; bA = Ac; bB = Bc;
            };
            for (int p = 0; p < npos; ++p) {
                const long h = (long)half + slide[p];
                if (h < 1 || h > n - 1 || (p > 0 && slide[p] == 0)) continue;
                set_masks((size_t)h);
                boundary(s.data(), (size_t)h, maskB, La, Ia);                   // lower boundary, lower interior
                boundary(s.data() + h, (size_t)(n - h), maskA, Lb, Ib);         // upper boundary, upper interior
                cA.assign(s.begin(), s.begin() + h); cB.assign(s.begin() + h, s.end());
                offer(La, Ia, cB);
                offer(Lb, cA, Ib);
                if (La.empty()) continue;                                       // (no camera sees across: nothing to cover)
                std::sort(La.begin(), La.end()); std::sort(Lb.begin(), Lb.end());
                nd_min_cover(La, Lb, adj, adj_words, ridx, inL, inR);
                cS.clear(); cA = Ia; cB = Ib;
                for (size_t q = 0; q < La.size(); ++q) (inL[q] ? cS : cA).push_back(La[q]);
                for (size_t q = 0; q < Lb.size(); ++q) (inR[q] ? cS : cB).push_back(Lb[q]);
                offer(cS, cA, cB);
            }
            Sep.swap(bS); A2.swap(bA); B2.swap(bB);
        }
        if (Sep.size() * 2 >= cams.size() || A2.empty()) {     // no useful separator: one dense block
            emit(cams, np > 1 ? -1 : part0);                   // (between ranks: the whole set is shared)
            return;
        }
        const int first = (int)T.block_end.size();
        nd(A2, part0, np > 1 ? npa : 1);
        nd(B2, np > 1 ? part0 + npa : part0, np > 1 ? npb : 1);
        emit(Sep, np > 1 ? -1 : part0, true, first);
    };
    std::vector<int> all(nc);
    for (int c = 0; c < nc; ++c) all[c] = c;
    if (nd_off) emit(all, T.nparts > 1 ? -1 : 0);
    else nd(all, 0, T.nparts);
}

// Independent check of a tree against the graph: the order is a permutation, the subtrees nest, and two co-visible
// cameras always lie on one root path of the block tree (the earlier one's block inside the subtree of the later one's)
// -- no camera of one part sees a camera of the other, at every cut.  0: valid; 1: not a permutation; 2: subtrees do not
// nest; 3: a co-visible pair across a cut.
inline int nd_check(int nc, const uint64_t *adj, int adj_words, const NdTree &T) {
    const int nb = (int)T.block_end.size();
    if ((int)T.order.size() != nc || (int)T.block_first.size() != nb || (nb ? T.block_end[nb - 1] : 0) != nc) return 1;
    std::vector<int> blk((size_t)nc, -1);
    for (int b = 0, q = 0; b < nb; ++b) {
        if (T.block_end[b] <= q) return 1;
        for (; q < T.block_end[b]; ++q) {
            const int c = T.order[q];
            if (c < 0 || c >= nc || blk[c] >= 0) return 1;
            blk[c] = b;
        }
    }
    for (int b = 0; b < nb; ++b) {
        const int f = T.block_first[b];
        if (f < 0 || f > b) return 2;
        for (int d = f; d < b; ++d) if (T.block_first[d] < f) return 2;
    }
    for (int a = 0; a < nc; ++a)
        for (int w = 0; w < adj_words; ++w) {
            uint64_t m = adj[(size_t)a * adj_words + w];
            while (m) {
                const int b = 64 * w + __builtin_ctzll(m);
                m &= m - 1;
                if (b >= nc || blk[b] <= blk[a]) continue;
                if (T.block_first[blk[b]] > blk[a]) return 3;
            }
        }
    return 0;
}

// ---- which separators: whole orders as candidates, scored by the model of the factorisation.
// What one candidate comes to once it is laid out in tiles (chol_df.hpp: symbolic_permuted): chain = the longest
// dependent chain of tile columns (depth of the elimination tree), run = the longest run of columns one workgroup of the
// chain role walks, products without the right-hand-side row, model_us = the list-schedule simulation that also picks
// the task order (model 0), or, for very large patterns, max(chain x 17 us, products x 2.6 us / workgroups) (model 1).
struct NdScore {
    int mode = -1, cams = 0, blocks = 0, tile_cols = 0, tiles = 0, chain = 0, run = 0, model = 0, valid = -1;
    long long products = 0;
    double model_us = 0.0;
};
// The scorer is the library's (dbat_core.hip registers the one of chol_df.hpp, device code and all); a program that
// includes the host plan alone has none, and then the order is that of mode 0 unless DBAT_HIP_ND_SEP names another.
using NdScoreFn = void (*)(int nc, int nio, const uint64_t *adj, int adj_words, const NdTree &T, NdScore &sc);
inline NdScoreFn &nd_score_hook() { static NdScoreFn f = nullptr; return f; }

// forced: 0, 1, 2 = that mode; otherwise the candidate with the smallest modelled time -- where it beats mode 0 by more
// than 1 % of the modelled time and its chain is no longer; mode 0 otherwise.  sc[3] (may be null): the candidates that
// were scored (mode < 0: not scored).  Several ranks: every rank scores the whole pattern as one task list, so all of
// them take the same order.  Returns the mode of T.
inline int nd_select(int nc, int nio, const uint64_t *adj, int adj_words, const double *xyz, const double *weight,
                     int nparts, int leaf, bool nd_off, int forced, bool score_forced, NdTree &T, NdScore *sc) {
    NdScore local[3];
    if (!sc) sc = local;
    for (int m = 0; m < 3; ++m) sc[m] = NdScore();
    const NdScoreFn score = nd_score_hook();
    auto run = [&](int m, NdTree &t) {
        nd_build(nc, adj, adj_words, xyz, weight, nparts, leaf, nd_off, m, t);
        if (score && (score_forced || forced < 0 || forced > 2)) { score(nc, nio, adj, adj_words, t, sc[m]); sc[m].mode = m; }
    };
    if ((forced >= 0 && forced <= 2) || !score || nd_off) {
        const int m = forced >= 0 && forced <= 2 ? forced : 0;
        run(m, T);
        return m;
    }
    NdTree cand[3];
    int best = 0;
    for (int m = 0; m < 3; ++m) {
        nd_build(nc, adj, adj_words, xyz, weight, nparts, leaf, nd_off, m, cand[m]);
        int same = -1;
        for (int q = 0; q < m && same < 0; ++q) if (cand[q].order == cand[m].order && cand[q].block_end == cand[m].block_end) same = q;
        if (same >= 0) { sc[m] = sc[same]; sc[m].mode = m; continue; }    // (nothing smaller than the separators of an earlier mode anywhere)
        score(nc, nio, adj, adj_words, cand[m], sc[m]); sc[m].mode = m;
        if (m > 0 && sc[m].chain <= sc[0].chain && sc[m].model_us < 0.99 * sc[0].model_us && sc[m].model_us < sc[best].model_us) best = m;
    }
    T = std::move(cand[best]);
    return best;
}

}  // namespace dbat
