// What the calls that take a device index instead of a handle share (dbat_hip_resect, _rigidalign, _multixform, _essmat5,
// _relorient, _pairadjust, _resect_ransac, _poseadjust): device scope, argument checks, kernel clock.  Included by
// dbat_core.hip before initial_host.hpp.  A new call of this family checks its arguments in the order the caller is to see
// the refusals (a check throws UsageError: DBAT_HIP_EINVAL with the message, by API_CATCH), opens a BatchDevice, works on
// its stream and copies the results back with DevBuf::download; kernels it wants timed get a KernelClock.
#pragma once

namespace dbat {

// The device of a handle-less call, current while this lives, and the stream the call works on.  Without a device, or
// with an index that names none, there is no scope: the constructor throws what API_CATCH reports.
// (It stands where the device test stood, so the device is made current before a call's return for n == 0 -- in
// dbat_hip_resect before its range checks -- where the calls used to set it after: one hipSetDevice and its restore more
// for an empty or refused call on another device than the current one.)
struct BatchDevice {
    DeviceGuard guard;
    static constexpr hipStream_t st = nullptr;
    explicit BatchDevice(int32_t device) : guard(checked(device)) {}
    static int checked(int32_t device) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) throw DeviceError{"no HIP device: the dbat_hip core has no CPU path"};
        if (device < 0 || device >= ndev) throw UsageError{"bad device index"};
        return device;
    }
};

// Device events around the N kernel spans of a family of calls, per thread: whether the calls record them (off: no event
// is created) and the milliseconds of the last call (0: not launched or not timed).  A family names its clock by a tag
// (using AlignClock = KernelClock<struct AlignFamily, 5>); set() and get() are its dbat_hip_debug_*_timing / _ms.
template <class Family, int N>
struct KernelClock {
    static inline thread_local bool on = false;
    static inline thread_local double ms[N] = {};
    template <int M>
    static void start(EventTimer<M> &ev, hipStream_t st) { if (on) ev.start(st); }
    static int set(int32_t v) { on = v != 0; return DBAT_HIP_OK; }
    static int get(double *out) {
        if (!out) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
        std::copy(ms, ms + N, out);
        return DBAT_HIP_OK;
    }
};

[[noreturn]] static void refuse(const char *who, const std::string &what) { throw UsageError{std::string(who) + ": " + what}; }

// The ranges start[c] .. start[c + 1] of the n items of a batch (`name`: the argument) start at 0, and no item ends before
// it begins or, with a cap, holds cap or more (`over`: what to say then).  A call that checks more per item takes the parts.
static void check_ranges_start(const char *who, const int64_t *start) { if (start[0] != 0) refuse(who, "ranges must start at 0"); }
static void check_range(const char *who, const char *name, const int64_t *start, int32_t c, int64_t cap = 0, const char *over = nullptr) {
    if (start[c + 1] < start[c]) refuse(who, std::string("the ranges of ") + name + " must ascend");
    if (cap > 0 && start[c + 1] - start[c] >= cap) refuse(who, over);
}
static void check_ranges(const char *who, const char *name, int32_t n, const int64_t *start, int64_t cap = 0, const char *over = nullptr) {
    check_ranges_start(who, start);
    for (int32_t c = 0; c < n; ++c) check_range(who, name, start, c, cap, over);
}

// max_iter and conv_tol of the options (min_angle: every call has a rule of its own)
static void check_pair_options(const char *who, const dbat_hip_pair_options *opt) {
    if (opt->max_iter < 1 || opt->max_iter > 200) refuse(who, "max_iter must be 1 .. 200");
    if (!(opt->conv_tol > 0) || !std::isfinite(opt->conv_tol)) refuse(who, "conv_tol must be positive");
}

// The rows-by-total arrays a and b are finite and the weights w1, w2 of their elements, where given, positive and finite:
// element by element, coordinates before weights; `noun` is what a column is called.
static bool weight_ok(double w) { return std::isfinite(w) && w > 0; }
static void check_columns(const char *who, const char *noun, int rows, int64_t total, const double *a, const double *b,
                          const double *w1 = nullptr, const double *w2 = nullptr) {
    for (int64_t i = 0; i < rows * total; ++i) {
        if (!std::isfinite(a[i]) || !std::isfinite(b[i])) refuse(who, std::string(noun) + " " + std::to_string(i / rows) + " is not finite");
        if ((w1 && !weight_ok(w1[i])) || (w2 && !weight_ok(w2[i]))) refuse(who, std::string("weight of ") + noun + " " + std::to_string(i / rows) + " is not positive and finite");
    }
}
static void check_weights(const char *who, const char *noun, int64_t total, const double *w) {      // 2-by-total, or null
    for (int64_t i = 0; w && i < 2 * total; ++i)
        if (!weight_ok(w[i])) refuse(who, std::string("weight of ") + noun + " " + std::to_string(i / 2) + " is not positive and finite");
}

// every point that may be used is finite: X (3-by-total) and, where given, xn (2-by-total)
static void check_used_points(const char *who, int64_t total, const uint8_t *use, const double *X, const double *xn = nullptr) {
    for (int64_t g = 0; g < total; ++g)
        if ((!use || use[g]) && !(std::isfinite(X[3 * g]) && std::isfinite(X[3 * g + 1]) && std::isfinite(X[3 * g + 2]) &&
                                  (!xn || (std::isfinite(xn[2 * g]) && std::isfinite(xn[2 * g + 1])))))
            refuse(who, "point " + std::to_string(g) + " is to be used and is not finite");
}

// P (3 x 4, column-major: `name` of `item` i) is finite and starts with a rotation
static void check_pose(const char *who, const char *name, const char *item, int64_t i, const double *P) {
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(P[k])) refuse(who, std::string(name) + " of " + item + " " + std::to_string(i) + " is not finite");
    double dev = 0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b)
            dev = std::max(dev, std::fabs(P[3 * a] * P[3 * b] + P[3 * a + 1] * P[3 * b + 1] + P[3 * a + 2] * P[3 * b + 2] - (a == b ? 1.0 : 0.0)));
    if (dev > 1e-6 || al_det3(P) < 0) refuse(who, std::string("R of ") + item + " " + std::to_string(i) + " is not a rotation");
}

}  // namespace dbat
