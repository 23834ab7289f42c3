// Initial values: forward intersection of the object points from a handle's rays, and spatial resection of single
// images, which takes no handle (kernels: kernels.hpp k_forwintersect*, resect.hpp).  Included by dbat_core.hip after
// Core and the handle.  The relative orientation of image pairs is relorient_host.hpp.
#pragma once

extern "C" {
int dbat_hip_forwintersect(dbat_hip_handle *h, const double *x, const uint8_t *skip, double *OP) {
    API_TRY
    if (!h || !x || !OP) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    Core &c = *h->core;
    DeviceGuard dev_guard(c.device);
    const Plan &P = c.P;
    c.x_to_z(x, c.zt.p);                              // IO / EO of the rays
    c.prep_cams(c.zt.p);
    // [3 np] the points, [np] whether a point has any observation: a shard knows that of its own points only, so
    // the flags ride in the sum with the coordinates
    DevBuf<double> dOP;
    dOP.alloc((size_t)4 * std::max(P.np, 1));
    HIPCHK(hipMemsetAsync(dOP.p, 0, (size_t)3 * P.np * sizeof(double), c.stream));
    std::vector<double> seen((size_t)P.np, 0.0);      // points without any observation: NaN (pm_multiforwintersect.m:41)
    for (int32_t r : P.o_pt) seen[r] = 1.0;
    if (P.np > 0) HIPCHK(hipMemcpyAsync(dOP.p + (size_t)3 * P.np, seen.data(), (size_t)P.np * sizeof(double), hipMemcpyHostToDevice, c.stream));
    if (c.nb > 0) c.launch<k_forwintersect>(dim3((unsigned)c.nb), dim3(P.BT), (size_t)P.BT * 9 * sizeof(double), c.d, c.cams.p, dOP.p);
    if (c.ngiant > 0) c.launch<k_forwintersect_giant>(dim3((unsigned)c.ngiant), dim3(256), 0, c.d, c.cams.p, dOP.p);
    if (c.multi()) c.do_allreduce(dOP.p, (int64_t)4 * P.np);             // every point is computed by its owner
    std::vector<double> tmp((size_t)4 * P.np);
    HIPCHK(hipMemcpyAsync(tmp.data(), dOP.p, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    c.sync();
    const double nan = std::nan("");
    for (int64_t p = 0; p < P.np; ++p) {
        if (skip && skip[p]) continue;                // keeps the caller's value (forwintersect.m:32-36)
        const int64_t r = P.pt_rank[p];
        const bool has_rays = tmp[(size_t)3 * P.np + r] > 0;
        for (int k = 0; k < 3; ++k) OP[3 * p + k] = has_rays ? tmp[3 * r + k] : nan;
    }
    return DBAT_HIP_OK;
    API_CATCH
}

int dbat_hip_resect(int32_t device, int32_t n_images, const int64_t *pt_start, const double *X, const double *xn,
                    const int64_t *tri_start, const int32_t *tri, double *P, double *rms) {
    API_TRY
    if (n_images < 0 || !pt_start || !tri_start || !P || !rms) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    // (the oldest of the family: the device before the ranges, no prefix in the messages, a triangle may repeat an index)
    BatchDevice dev(device);
    if (n_images == 0) return DBAT_HIP_OK;
    if (pt_start[0] != 0 || tri_start[0] != 0) { g_err = "ranges must start at 0"; return DBAT_HIP_EINVAL; }
    for (int c = 0; c < n_images; ++c)
        if (pt_start[c + 1] < pt_start[c] || tri_start[c + 1] < tri_start[c]) { g_err = "ranges must ascend"; return DBAT_HIP_EINVAL; }
    const int64_t npt = pt_start[n_images], ntri = tri_start[n_images];
    if ((npt > 0 && (!X || !xn)) || (ntri > 0 && !tri)) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    for (int c = 0; c < n_images; ++c)
        for (int64_t t = 3 * tri_start[c]; t < 3 * tri_start[c + 1]; ++t)
            if (tri[t] < 0 || tri[t] >= pt_start[c + 1] - pt_start[c]) { g_err = "triangle index outside the camera's points"; return DBAT_HIP_EINVAL; }
    DevBuf<int64_t> dps, dts;
    DevBuf<double> dX, dx, dP, dr;
    DevBuf<int32_t> dtri;
    dps.upload(pt_start, (size_t)n_images + 1); dts.upload(tri_start, (size_t)n_images + 1);
    dX.upload(X, (size_t)3 * npt); dx.upload(xn, (size_t)2 * npt); dtri.upload(tri, (size_t)3 * ntri);
    dP.alloc((size_t)12 * n_images); dr.alloc((size_t)n_images);
    launch<k_resect>(dim3((unsigned)n_images), dim3(64), 0, dev.st, n_images, dps.p, dX.p, dx.p, dts.p, dtri.p, 1, dP.p, dr.p);
    dP.download(P); dr.download(rms);
    return DBAT_HIP_OK;
    API_CATCH
}
}  // extern "C"
