// Host side of the ray intersection angles at zt (kernels: angles.hpp): plan, driver, C entry points.  Included by
// dbat_core.hip after Core and analysis_host.hpp.
#pragma once

namespace dbat {
// What the kernels need beyond the plan's uploads and the point index -- where every image's observations are in the
// camera-major copy, the work items of the pair kernel, the scratch array of unit directions -- is built by the first
// call and kept; a handle that never asks for angles has none of it.
struct AnglePlan {
    int32_t heavy_kmax = 0;
    int64_t n_items = 0, n_slots = 0, n_mfma = 0;
    std::vector<int32_t> cam_rays;                       // per image
    DevBuf<int64_t> cam_src, cam_pad;
    DevBuf<int32_t> items;
    DevBuf<double> cdir, op_out, cam_out;
    DevBuf<unsigned long long> cam_min;
    EventTimer<3> timer;                                 // last call: point kernels, directions of the images, pair kernel + finish
    AnglePlan(const Core &c, const PointIndex &ix) {
        const Plan &P = c.P;
        for (int64_t r = 0; r < ix.hp0; ++r)
            if (ix.pos[r + 1] - ix.pos[r] > ANG_LIGHT_KMAX) throw DeviceError{"internal: a tiled point with more rays than the angle kernel holds"};
        for (int64_t r = ix.hp0; r < ix.hp1; ++r) heavy_kmax = (int32_t)std::max<int64_t>(heavy_kmax, ix.pos[r + 1] - ix.pos[r]);
        if (heavy_kmax > ANG_HEAVY_KMAX)
            throw UsageError{"ray angles: an object point with " + std::to_string(heavy_kmax) + " rays (at most " + std::to_string(ANG_HEAVY_KMAX) + ")"};
        // images: their ranges in the two parts of the camera-major copy, 16-direction tiles, work items
        std::vector<int64_t> src((size_t)4 * P.nc, 0), pad((size_t)P.nc + 1, 0);
        for (int64_t q = 0; q < c.n_cm_chunks_all; ++q) {
            const int cam = P.cm_chunk_cam[q];
            const int64_t len = P.cm_chunk_start[q + 1] - P.cm_chunk_start[q];
            int64_t *sc = src.data() + 4 * (size_t)cam;      // {first tiled, tiled, first of the rest, all}
            if (q < c.n_cm_chunks) {
                if (sc[1] == 0) sc[0] = P.cm_chunk_start[q];
                sc[1] += len;
            } else if (sc[3] == sc[1]) sc[2] = P.cm_chunk_start[q];   // (the chunks of the tiled part all come first)
            sc[3] += len;
        }
        cam_rays.assign((size_t)P.nc, 0);
        std::vector<int32_t> it;
        for (int cam = 0; cam < P.nc; ++cam) {
            const int64_t n = src[4 * (size_t)cam + 3];
            if (n >= ((int64_t)1 << 31) - 16) throw UsageError{"ray angles: an image with more than 2^31 points"};
            cam_rays[cam] = (int32_t)n;
            const int64_t T = (n + 15) / 16;
            pad[(size_t)cam + 1] = pad[cam] + 16 * T;
            if (n >= 2) {
                for (int64_t I0 = 0; I0 < T; I0 += ANG_RUN) { it.push_back(cam); it.push_back((int32_t)I0); }
                n_mfma += T * (T + 1) / 2;
            }
        }
        n_items = (int64_t)it.size() / 2; n_slots = pad[P.nc];
        cam_src.upload(src); cam_pad.upload(pad); items.upload(it);
        cdir.alloc((size_t)3 * std::max<int64_t>(n_slots, 1));
        op_out.alloc((size_t)std::max<int64_t>(P.np, 1)); cam_out.alloc((size_t)std::max(P.nc, 1)); cam_min.alloc((size_t)std::max(P.nc, 1));
    }
};

static void ray_angles(Core &c, const PointIndex &ix, AnglePlan &ang, double *hop, double *hcam, int32_t *hop_rays, int32_t *hcam_rays) {
    const Plan &P = c.P;
    if (hop_rays) std::copy(ix.count.begin(), ix.count.end(), hop_rays);
    if (hcam_rays) std::copy(ang.cam_rays.begin(), ang.cam_rays.end(), hcam_rays);
    if (!hop && !hcam) return;
    c.prep_cams(c.zt.p);
    const double *zz = c.zt.p;
    ang.timer.start(c.stream);
    if (hop) {
        if (ix.hp0 > 0)
            c.launch<k_angles_pt_light>(dim3((unsigned)cdiv(ix.hp0, ANG_LIGHT_PTS)), dim3(256), 0, zz, (int64_t)P.NS, c.cams.p, c.o_cam.p, ix.d_pos.p, ix.hp0, ang.op_out.p);
        if (ix.hp1 > ix.hp0)
            c.launch<k_angles_pt_heavy>(dim3((unsigned)(ix.hp1 - ix.hp0)), dim3(256), (size_t)3 * ang.heavy_kmax * sizeof(double), zz, (int64_t)P.NS, c.cams.p,
                                        c.o_cam.p, ix.d_pos.p, ix.hp0, ang.heavy_kmax, ang.op_out.p);
    }
    ang.timer.lap(c.stream);
    if (hcam) {
        HIPCHK(hipMemsetAsync(ang.cam_min.p, 0xFF, (size_t)P.nc * sizeof(unsigned long long), c.stream));
        if (ang.n_slots > 0)
            c.launch<k_angles_cam_dirs>(dim3((unsigned)cdiv(ang.n_slots, 256)), dim3(256), 0, zz, (int64_t)P.NS, c.cams.p, P.nc, c.cm_pt.p, ang.cam_src.p, ang.cam_pad.p, ang.cdir.p);
    }
    ang.timer.lap(c.stream);
    if (hcam) {
        if (ang.n_items > 0)
            c.launch<k_angles_cam_pairs>(dim3((unsigned)ang.n_items), dim3(256), 0, ang.cdir.p, ang.cam_pad.p, ang.items.p, ang.cam_min.p);
        c.launch<k_angles_cam_finish>(dim3((unsigned)cdiv(P.nc, 256)), dim3(256), 0, P.nc, ang.cam_src.p, ang.cam_min.p, ang.cam_out.p);
    }
    ang.timer.lap(c.stream);
    std::vector<double> tmp;
    if (hop && ix.hp1 > 0) {
        tmp.resize((size_t)ix.hp1);
        HIPCHK(hipMemcpyAsync(tmp.data(), ang.op_out.p, (size_t)ix.hp1 * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    }
    if (hcam) HIPCHK(hipMemcpyAsync(hcam, ang.cam_out.p, (size_t)P.nc * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    c.sync();
    if (hop) scatter_points(c, tmp, ix.hp1, std::nan(""), hop);
    ang.timer.read();
}
}  // namespace dbat

extern "C" {
int dbat_hip_ray_angles(dbat_hip_handle *h, const double *x, double *op_angle, double *cam_angle, int32_t *op_rays, int32_t *cam_rays) {
    API_TRY
    if (!h || !x) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    Core &c = *h->core;
    if (!one_rank(c, "ray angles", "the pairs of rays across shards are not formed")) return DBAT_HIP_EINVAL;
    DeviceGuard dev_guard(c.device);
    if (op_angle || cam_angle) c.x_to_z(x, c.zt.p);
    const PointIndex &ix = built_once(h->pts, c);
    ray_angles(c, ix, built_once(h->ang, c, ix), op_angle, cam_angle, op_rays, cam_rays);
    return DBAT_HIP_OK;
    API_CATCH
}

/* Debug / measurement: milliseconds of the last dbat_hip_ray_angles on the handle's stream (device events): ms[0] the
 * point kernels, ms[1] the unit directions of the images, ms[2] the pair kernel and the final acos; info[0] the
 * v_mfma_f64_16x16x4_f64 instructions (256 pairs each) of one launch of the pair kernel, info[1] its workgroups. */
int dbat_hip_debug_ray_angles_ms(dbat_hip_handle *h, double *ms, int64_t *info) {
    if (!h || !ms || !info || !h->ang) { g_err = "no ray angles computed on this handle"; return DBAT_HIP_EINVAL; }
    for (int i = 0; i < 3; ++i) ms[i] = h->ang->timer.ms[i];
    info[0] = h->ang->n_mfma; info[1] = h->ang->n_items;
    return DBAT_HIP_OK;
}

/* Host only, one thread (include/dbat_hip.h): angles.m:26-46, camangles.m:26-46 with the arithmetic of the kernels
 * (unit_dir, abs_dot, angle_from_min). */
int dbat_hip_debug_ray_angles_host(const dbat_hip_problem *prob, double *op_angle, double *cam_angle) {
    API_TRY
    if (!prob) { g_err = "null argument"; return DBAT_HIP_EINVAL; }
    if (prob->abi_version != DBAT_HIP_ABI_VERSION) { g_err = "ABI version mismatch"; return DBAT_HIP_EINVAL; }
    const int64_t nc = prob->n_images, np = prob->n_points, no = prob->n_obs;
    if (nc < 0 || np < 0 || no < 0 || (no > 0 && (!prob->ip_cam || !prob->ip_pt)) || (nc > 0 && !prob->EO_val) || (np > 0 && !prob->OP_val)) {
        g_err = "bad problem"; return DBAT_HIP_EINVAL;
    }
    for (int64_t o = 0; o < no; ++o)
        if (prob->ip_cam[o] < 0 || prob->ip_cam[o] >= nc || prob->ip_pt[o] < 0 || prob->ip_pt[o] >= np) { g_err = "IP index out of range"; return DBAT_HIP_EINVAL; }
    // side 0: the rays of every point (apex = the point, ends = camera centres); side 1: of every image
    for (int side = 0; side < 2; ++side) {
        double *out = side == 0 ? op_angle : cam_angle;
        if (!out) continue;
        const int64_t n = side == 0 ? np : nc;
        const int32_t *own = side == 0 ? prob->ip_pt : prob->ip_cam, *other = side == 0 ? prob->ip_cam : prob->ip_pt;
        std::vector<int64_t> start((size_t)n + 1, 0);
        for (int64_t o = 0; o < no; ++o) ++start[(size_t)own[o] + 1];
        for (int64_t i = 0; i < n; ++i) start[i + 1] += start[i];
        std::vector<int32_t> lst((size_t)no);
        {
            std::vector<int64_t> fill(start.begin(), start.end() - 1);
            for (int64_t o = 0; o < no; ++o) lst[(size_t)fill[own[o]]++] = other[o];
        }
        std::vector<double> dir;
        for (int64_t i = 0; i < n; ++i) {
            const int64_t k = start[i + 1] - start[i];
            dir.resize((size_t)3 * k);
            for (int64_t j = 0; j < k; ++j) {
                const int32_t e = lst[(size_t)(start[i] + j)];
                const double *q = side == 0 ? prob->OP_val + 3 * i : prob->OP_val + 3 * (int64_t)e;
                const double *cc = side == 0 ? prob->EO_val + 6 * (int64_t)e : prob->EO_val + 6 * i;
                unit_dir(q, cc, dir[3 * j], dir[3 * j + 1], dir[3 * j + 2]);
            }
            double m = INFINITY;
            for (int64_t a = 0; a < k; ++a)
                for (int64_t b = a + 1; b < k; ++b)
                    m = std::fmin(m, abs_dot(dir[3 * a], dir[3 * a + 1], dir[3 * a + 2], dir[3 * b], dir[3 * b + 1], dir[3 * b + 2]));
            out[i] = angle_from_min(k, m);
        }
    }
    return DBAT_HIP_OK;
    API_CATCH
}
}  // extern "C"
