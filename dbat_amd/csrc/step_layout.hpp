// The host protocol of a Levenberg-Marquardt step: the slots of the three small buffers through which the step's
// kernels and the host loops (dbat_core.hip) talk to each other.  One definition for both sides; DESIGN.md
// ("Step protocol") has the table of who writes and who reads each slot.
#pragma once

namespace dbat {

// ---- scal: the step's sums on the device (what an all-reduce carries over the ranks).  On one rank the kernel that
// ends a phase mirrors them into the mailbox at the same index.
constexpr int SCAL_OBJECTIVE = 0;        // after an objective value: r'r of the image rows + the prior rows
constexpr int SCAL_JPJP = 0;             // after a solve / J v: ||Jp||^2 and r'Jp of the image rows ...
constexpr int SCAL_RJP = 1;
constexpr int SCAL_JPJP_PRIOR = 4;       // ... and the prior rows' shares of both
constexpr int SCAL_RJP_PRIOR = 5;
constexpr int SCAL_PP = 6;               // p'p over the owned entries
constexpr int SCAL_FAILED = 7;           // > 0: the factorisation failed on some rank
constexpr int SCAL_SUMS = 8;             // the sums above (2, 3: zero)
constexpr int SCAL_RANK0 = 8;            // behind them, per rank: {min, max} pivot of its point blocks, of its part of the reduced system
constexpr int SCAL_PER_RANK = 4;
constexpr int scal_size(int nranks) { return 16 + SCAL_PER_RANK * nranks; }

// ---- the pinned mailbox (doubles): what the host reads without a copy of its own
constexpr int MB_SIZE = 64;
constexpr int MB_SCAL = 0, MB_SCAL_N = 32;           // the mirror of scal; on several ranks the landing place of its copy
constexpr int MB_OBJECTIVE = MB_SCAL + SCAL_OBJECTIVE;
constexpr int MB_JPJP = MB_SCAL + SCAL_JPJP, MB_RJP = MB_SCAL + SCAL_RJP;
constexpr int MB_JPJP_PRIOR = MB_SCAL + SCAL_JPJP_PRIOR, MB_RJP_PRIOR = MB_SCAL + SCAL_RJP_PRIOR;
constexpr int MB_PP = MB_SCAL + SCAL_PP;
constexpr int MB_LIN = 32, MB_LIN_N = 3;             // sums of a linearisation:
constexpr int MB_LIN_RR = MB_LIN;                    //   r'r (image + prior rows) at the linearisation point
constexpr int MB_LIN_TRACE_PT = MB_LIN + 1;          //   squared column norms of the point columns
constexpr int MB_LIN_TRACE_CAM = MB_LIN + 2;         //   ... of the estimated camera / IO columns
constexpr int MB_PIVOTS = 40, MB_PIVOTS_N = 4;       // pivot extremes {min, max} of the point blocks, of the reduced system (bit patterns)
constexpr int MB_INFO = 44;                          // info of the factorisation (an integer's bit pattern)
constexpr int MB_PIVOT_RESET = 48;                   // host-written: what the pivot extremes start from (MB_PIVOTS_N values)
constexpr int MB_DEPTH = 52, MB_DEPTH_N = 3;         // depth.hpp (k_depth_finish is handed MB_DEPTH):
constexpr int MB_DEPTH_BEHIND = MB_DEPTH;            //   observations behind their camera (an integer's bit pattern)
constexpr int MB_DEPTH_MIN = MB_DEPTH + 1;           //   the smallest depth
constexpr int MB_DEPTH_ARGMIN = MB_DEPTH + 2;        //   ... and its column (an integer's bit pattern)
constexpr int MB_DET_TIMEOUTS = 60;                  // deterministic mode: copy of the counter CTR_SIG_TIMEOUTS
constexpr int MB_TICKET = 63;                        // ticket of the host's current wait (mailbox_done)

constexpr bool mb_ranges_ok() {
    const int r[][2] = {{MB_SCAL, MB_SCAL_N}, {MB_LIN, MB_LIN_N}, {MB_PIVOTS, MB_PIVOTS_N}, {MB_INFO, 1}, {MB_PIVOT_RESET, MB_PIVOTS_N},
                        {MB_DEPTH, MB_DEPTH_N}, {MB_DET_TIMEOUTS, 1}, {MB_TICKET, 1}};
    const int n = sizeof(r) / sizeof(r[0]);
    for (int i = 0; i < n; ++i) {
        if (r[i][0] < 0 || r[i][1] < 1 || r[i][0] + r[i][1] > MB_SIZE) return false;
        for (int j = i + 1; j < n; ++j)
            if (r[i][0] < r[j][0] + r[j][1] && r[j][0] < r[i][0] + r[i][1]) return false;
    }
    return true;
}
static_assert(mb_ranges_ok(), "mailbox ranges overlap or leave the mailbox");
static_assert(SCAL_SUMS <= MB_SCAL_N && SCAL_RANK0 >= SCAL_SUMS, "the sums are mirrored into the mailbox; the ranks' slots follow them");

// ---- gctr: tickets of the in-kernel grid sums (each zero between launches) and the signature kernel's counters
constexpr int CTR_SIZE = 16;
constexpr int CTR_OBJECTIVE = 1;         // k_residual_cm's own tail, or k_prior_sq
constexpr int CTR_BUILD_TAIL = 2;        // k_build_tail
constexpr int CTR_FINISH = 3;            // k_finish
constexpr int CTR_PRIOR_JV = 4;          // k_prior_jv (a solve's tail, and J v)
constexpr int CTR_SIG_TICKET = 5;        // k_build_sig: the next tile
constexpr int CTR_TRACE_TAIL = 6;        // k_trace_tail
constexpr int CTR_SIG_TIMEOUTS = 7;      // k_build_sig, deterministic mode: chunks that gave up waiting for their turn

constexpr bool ctr_distinct() {
    const int c[] = {CTR_OBJECTIVE, CTR_BUILD_TAIL, CTR_FINISH, CTR_PRIOR_JV, CTR_SIG_TICKET, CTR_TRACE_TAIL, CTR_SIG_TIMEOUTS};
    const int n = sizeof(c) / sizeof(c[0]);
    for (int i = 0; i < n; ++i) {
        if (c[i] < 0 || c[i] >= CTR_SIZE) return false;
        for (int j = i + 1; j < n; ++j) if (c[i] == c[j]) return false;
    }
    return true;
}
static_assert(ctr_distinct(), "two users of one ticket counter");
// k_build_sig is handed its ticket and finds its time-out counter from there
static_assert(CTR_SIG_TIMEOUTS - CTR_SIG_TICKET == 2, "sig.hpp: the time-out counter sits two behind the tile ticket");

}  // namespace dbat
