// capi_fuse.cpp -- the Fuse entry points of include/xfeat_hip.h: the level thresholds that stand for MapPoint::PredictScale, the
// per-point arithmetic on the host (fuse_math.h, the kernel's own lines), the device form and the host-pointer form (host_stage.h).
#include "host_stage.h"
#include "window_layout.h"
#include "fuse_math.h"
#include <math.h>
#include <string.h>

// MapPoint::PredictScale before the clamp (MapPoint.cc:522), float overloads: what the thresholds are bisected against
static float scale_level_expr(float ratio, float log_sf) { return ceilf(logf(ratio) / log_sf); }

// the checks every entry with a scale table shares, and the tables as the kernels take them (also capi_loop.cpp)
bool fuse_levels(const float* scale_factors, const float* ratio_max, int nlevels, FuseLevels* L) {
    if (nlevels < 1 || nlevels > XFH_FUSE_MAX_LEVELS || !scale_factors || (nlevels > 1 && !ratio_max)) return false;
    memset(L, 0, sizeof *L);
    L->nlevels = nlevels;
    for (int l = 0; l < nlevels; ++l) L->scale_factors[l] = scale_factors[l];
    for (int l = 0; l < nlevels - 1; ++l) L->ratio_max[l] = ratio_max[l];
    return true;
}

// what xfh_fuse_search_device and xfh_fuse_search check alike before anything is staged or launched (the pointers are theirs to check);
// fills the kernel's level tables
static bool fuse_args_ok(int nq, int nt, const xfh_camera* cam, const xfh_grid_bounds* bounds, float th, const float* scale_factors, const float* ratio_max,
                         int nlevels, int flags, FuseLevels* L) {
    if (nq < 1 || nq > (1 << 20) || nt < 1 || nt > XFH_GRID_MAX_N || !cam || !bounds || !isfinite(th) || (flags & ~XFH_FUSE_CHI2)) return false;
    return fuse_levels(scale_factors, ratio_max, nlevels, L);
}

extern "C" {

// ratio_max[l] = the largest finite float with ceilf(logf(ratio) / logf(scale_factor)) <= l.  Positive finite floats are ordered like
// their bit patterns, and the expression does not decrease with the ratio as long as the host's logf is monotone: bisection over
// the patterns 0x00000001 (the least denormal: the expression is negative) .. 0x7f7fffff (FLT_MAX).
int xfh_scale_level_thresholds(float scale_factor, int nlevels, float* ratio_max) {
    if (nlevels < 1 || nlevels > XFH_FUSE_MAX_LEVELS || !isfinite(scale_factor) || !(scale_factor > 1.0f) || (nlevels > 1 && !ratio_max)) return XFH_ERR_INVALID_ARG;
    const float log_sf = logf(scale_factor);
    if (!(log_sf > 0.0f)) return XFH_ERR_INVALID_ARG;
    for (int l = 0; l < nlevels - 1; ++l) {
        uint32_t lo = 0x00000001u, hi = 0x7f7fffffu;                   // invariant: the expression at lo is <= l
        float f;
        memcpy(&f, &hi, 4);
        if (!(scale_level_expr(f, log_sf) <= (float)l)) {
            while (hi - lo > 1) {                                      // ... and at hi it is > l
                const uint32_t mid = lo + (hi - lo) / 2;
                memcpy(&f, &mid, 4);
                if (scale_level_expr(f, log_sf) <= (float)l) lo = mid; else hi = mid;
            }
        } else lo = hi;
        memcpy(&ratio_max[l], &lo, 4);
    }
    return XFH_OK;
}

int xfh_fuse_project(const float* Tcw, const float* Ow, const xfh_camera* cam, const xfh_grid_bounds* bounds, float th, const float* scale_factors,
                     const float* ratio_max, int nlevels, const float* xyz, const float* normals, const float* distances, int n,
                     float* uvr, float* ur, int* level, uint8_t* status) {
    FuseLevels L;
    if (!Tcw || !Ow || !cam || !bounds || n < 0 || !fuse_levels(scale_factors, ratio_max, nlevels, &L)) return XFH_ERR_INVALID_ARG;
    if (n > 0 && (!xyz || !normals || !distances || !uvr || !ur || !level || !status)) return XFH_ERR_INVALID_ARG;
    for (int i = 0; i < n; ++i)
        status[i] = (uint8_t)xfh_fuse_point(Tcw, Ow, *cam, *bounds, th, L, xyz + 3 * (size_t)i, normals + 3 * (size_t)i, distances + 3 * (size_t)i,
                                            &uvr[3 * (size_t)i], &uvr[3 * (size_t)i + 1], &ur[i], &uvr[3 * (size_t)i + 2], &level[i]);
    return XFH_OK;
}

int xfh_fuse_search_device(xfh_ctx* c, int B, int nq, size_t query_stride, const float* d_pts, const float* d_normals, const float* d_dist,
                           const float* d_qdesc, const uint8_t* d_qflags, const float* d_Tcw, const float* d_Ow, const xfh_camera* cam,
                           const xfh_grid_bounds* bounds, float th, const float* scale_factors, const float* ratio_max, int nlevels, const void* d_grids,
                           const float* d_targets, size_t target_stride, int nt, const float* d_uright, int flags, int init_dist, int th_low,
                           uint8_t* d_status, int* d_best_idx, int* d_best_dist, int* d_n_window, int* d_n_tested, int* d_level, float* d_proj_out,
                           int* d_n_fused) {
    FuseArgs a = {};
    if (!c || B < 1 || B > 65535 || (query_stride != 0 && query_stride != (size_t)nq)) return XFH_ERR_INVALID_ARG;
    if (!fuse_args_ok(nq, nt, cam, bounds, th, scale_factors, ratio_max, nlevels, flags, &a.lv)) return XFH_ERR_INVALID_ARG;
    if (!d_pts || !d_normals || !d_dist || !d_qdesc || !d_qflags || !d_Tcw || !d_Ow || !d_grids || !d_targets || !d_status || !d_best_idx || !d_best_dist ||
        !d_n_window || !d_n_tested || !d_level || !d_n_fused) return XFH_ERR_INVALID_ARG;
    if (misaligned(15, d_qdesc, d_targets, d_grids, target_stride) ||
        misaligned(3, d_pts, d_normals, d_dist, d_Tcw, d_Ow, d_uright, d_best_idx, d_best_dist, d_n_window, d_n_tested, d_level, d_proj_out, d_n_fused))
        return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    a.nq = nq; a.nt = nt; a.flags = flags; a.init_dist = init_dist; a.th_low = th_low; a.th = th; a.query_stride = query_stride;
    a.pts = d_pts; a.normals = d_normals; a.dist = d_dist; a.qdesc = d_qdesc; a.qflags = d_qflags; a.Tcw = d_Tcw; a.Ow = d_Ow;
    a.cam = *cam; a.bounds = *bounds;
    a.grids = (const char*)d_grids; a.grid_stride = xfh_grid_bytes(nt); a.targets = (const char*)d_targets; a.target_stride = target_stride; a.uright = d_uright;
    a.status = d_status; a.best_idx = d_best_idx; a.best_dist = d_best_dist; a.n_window = d_n_window; a.n_tested = d_n_tested; a.level = d_level;
    a.proj_out = d_proj_out; a.n_fused = d_n_fused;
    HIPCK(c, launch_fuse_search(c, a, B));
    return XFH_OK;
}

int xfh_fuse_search(xfh_ctx* c, int nq, const float* pts, const float* normals, const float* dist, const float* qdesc, const uint8_t* qflags,
                    const float* Tcw, const float* Ow, const xfh_camera* cam, const xfh_grid_bounds* bounds, float th, const float* scale_factors,
                    const float* ratio_max, int nlevels, const xfh_keypoint* kps, const float* targets, int nt, const float* uright, int flags,
                    int init_dist, int th_low, uint8_t* status, int* best_idx, int* best_dist, int* n_window, int* n_tested, int* level,
                    float* proj_out, int* n_fused) {
    GridGeom g;
    FuseLevels lv;
    if (!c || !fuse_args_ok(nq, nt, cam, bounds, th, scale_factors, ratio_max, nlevels, flags, &lv) || !grid_geom(bounds, &g)) return XFH_ERR_INVALID_ARG;
    if (!pts || !normals || !dist || !qdesc || !qflags || !Tcw || !Ow || !kps || !targets || !status || !best_idx || !best_dist || !n_window || !n_tested ||
        !level || !n_fused) return XFH_ERR_INVALID_ARG;
    HostStage s{c};
    auto dq = s.in<float>(qdesc, (size_t)nq * 256), dp = s.in<float>(pts, (size_t)nq * 12), dn = s.in<float>(normals, (size_t)nq * 12);
    auto dd = s.in<float>(dist, (size_t)nq * 12);
    auto dfl = s.in<uint8_t>(qflags, (size_t)nq);
    auto dT = s.in<float>(Tcw, 48), dO = s.in<float>(Ow, 12);
    auto dt = s.in<float>(targets, (size_t)nt * 256);
    auto dk = s.in<xfh_keypoint>(kps, (size_t)nt * sizeof(xfh_keypoint));
    auto dur = s.in_opt<float>(uright, (size_t)nt * 4);
    auto dg = s.tmp<char>(xfh_grid_bytes(nt));
    int* const out[5] = {best_idx, best_dist, n_window, n_tested, level};
    HostStage::Dev<int> o[5];
    for (int k = 0; k < 5; ++k) o[k] = s.out<int>(out[k], (size_t)nq * 4);
    auto dst = s.out<uint8_t>(status, (size_t)nq);
    auto dpo = s.out_opt<float>(proj_out, (size_t)nq * 12);
    auto dnf = s.out<int>(n_fused, 4);
    if (const int rc = s.upload(); rc != XFH_OK) return rc;
    HIPCK(c, launch_grid_build(c, dk, 0, nullptr, 0, dg, 0, nt, 1, g, 0));
    const int rc = xfh_fuse_search_device(c, 1, nq, 0, dp, dn, dd, dq, dfl, dT, dO, cam, bounds, th, scale_factors, ratio_max, nlevels, dg, dt, 0, nt, dur,
                                          flags, init_dist, th_low, dst, o[0], o[1], o[2], o[3], o[4], dpo, dnf);
    if (rc != XFH_OK) return rc;                                              // (a HIP error: every argument check has passed above)
    return s.download();
}

}  // extern "C"
