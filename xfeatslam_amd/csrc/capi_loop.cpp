// capi_loop.cpp -- the entry points of include/xfeat_hip.h that LoopClosing and Tracking::Relocalization call: the Sim3 and relocalisation
// forms of SearchByProjection (xfh_map_project, xfh_map_projection_search*) and SearchBySim3 (xfh_sim3_project, xfh_sim3_search*): the
// per-point arithmetic on the host (mapproj_math.h / sim3_math.h, the kernels' own lines), the device forms and the host-pointer forms
// (host_stage.h).
#include "host_stage.h"
#include "window_layout.h"
#include "mapproj_math.h"
#include "sim3_math.h"
#include <limits.h>
#include <math.h>
#include <string.h>

// what xfh_sim3_search_device and xfh_sim3_search check alike before anything is staged or launched; fills the kernel's level tables
static bool sim3_args_ok(const xfh_sim3_side* s1, const xfh_sim3_side* s2, const xfh_camera* cam, const xfh_grid_bounds* bounds, float th,
                         const float* scale_factors, const float* ratio_max, int nlevels, FuseLevels* L) {
    if (!s1 || !s2 || !cam || !bounds || !isfinite(th)) return false;
    if (s1->n < 1 || s1->n > XFH_GRID_MAX_N || s2->n < 1 || s2->n > XFH_GRID_MAX_N) return false;
    return fuse_levels(scale_factors, ratio_max, nlevels, L);
}
// the pointers both forms need of a side (grid / kps are the forms' own to check)
static bool sim3_side_null(const xfh_sim3_side* s) {
    return !s->desc || !s->points || !s->dist || !s->mp_desc || !s->flags || !s->Tw || !s->status || !s->match || !s->best_dist || !s->n_window ||
           !s->n_tested || !s->level;
}
static bool sim3_side_misaligned(const xfh_sim3_side* s) {
    return misaligned(15, s->grid, s->desc, s->desc_stride_bytes, s->mp_desc) ||
           misaligned(3, s->points, s->dist, s->Tw, s->match, s->best_dist, s->n_window, s->n_tested, s->level, s->proj_out_or_null);
}
static Sim3Side sim3_side(const xfh_sim3_side* s, bool shared) {
    Sim3Side k;
    k.n = s->n; k.stride = shared ? 0 : 1;
    k.grids = (const char*)s->grid; k.grid_stride = xfh_grid_bytes(s->n); k.desc = (const char*)s->desc; k.desc_stride = s->desc_stride_bytes;
    k.X = s->points; k.dist = s->dist; k.mpdesc = s->mp_desc; k.flags = s->flags; k.Tw = s->Tw;
    k.status = s->status; k.match = s->match; k.best_dist = s->best_dist; k.n_window = s->n_window; k.n_tested = s->n_tested; k.level = s->level;
    k.proj_out = s->proj_out_or_null;
    return k;
}

#define XFH_MAPPROJ_FORM_BITS (XFH_MAPPROJ_CULL_BEHIND | XFH_MAPPROJ_CHECK_ANGLE | XFH_MAPPROJ_PROJECT_INVZ | XFH_MAPPROJ_BOUNDS_CLOSED)
// what xfh_map_projection_search_device and xfh_map_projection_search check alike before anything is staged or launched (the pointers are
// theirs to check); fills the kernel's level tables
static bool mapproj_args_ok(int form, int nq, int nt, const xfh_camera* cam, const xfh_grid_bounds* bounds, float th, const float* scale_factors,
                            const float* ratio_max, int nlevels, float accept_max, FuseLevels* L) {
    if (nq < 1 || nq > XFH_GRID_MAX_N || nt < 1 || nt > XFH_GRID_MAX_N || !cam || !bounds || (form & ~XFH_MAPPROJ_FORM_BITS)) return false;
    if (!isfinite(th) || !isfinite(accept_max) || accept_max < 0.0f) return false;
    return fuse_levels(scale_factors, ratio_max, nlevels, L);
}
// the workspace: B problems of projection_layout.h, then the resolver's second-best distances [B][nq], which are no output here
static size_t mapproj_ws_second(int nq, int nt, int B) { return proj_ws_layout(nq, nt).bytes * (size_t)B; }

extern "C" {

int xfh_map_project(const float* Tcw, const float* Ow, const xfh_camera* cam, const xfh_grid_bounds* bounds, float th, const float* scale_factors,
                    const float* ratio_max, int nlevels, int form, const float* xyz, const float* normals, const float* distances, int n,
                    float* uvr, int* level, uint8_t* status) {
    FuseLevels L;
    if (!Tcw || !Ow || !cam || !bounds || n < 0 || (form & ~XFH_MAPPROJ_FORM_BITS) || !fuse_levels(scale_factors, ratio_max, nlevels, &L)) return XFH_ERR_INVALID_ARG;
    if (n > 0 && (!xyz || !normals || !distances || !uvr || !level || !status)) return XFH_ERR_INVALID_ARG;
    for (int i = 0; i < n; ++i)
        status[i] = (uint8_t)xfh_mapproj_point(Tcw, Ow, *cam, *bounds, th, L, form, xyz + 3 * (size_t)i, normals + 3 * (size_t)i, distances + 3 * (size_t)i,
                                               &uvr[3 * (size_t)i], &uvr[3 * (size_t)i + 1], &uvr[3 * (size_t)i + 2], &level[i]);
    return XFH_OK;
}

size_t xfh_map_projection_search_workspace_bytes(int nq, int nt, int B) {
    if (nq < 1 || nq > XFH_GRID_MAX_N || nt < 1 || nt > XFH_GRID_MAX_N || B < 1 || B > 65535) return 0;
    return mapproj_ws_second(nq, nt, B) + (((size_t)B * nq * sizeof(int) + 255) & ~(size_t)255);
}

int xfh_map_projection_search_device(xfh_ctx* c, int form, int B, int nq, const float* d_pts, const float* d_normals, const float* d_dist, const float* d_qdesc,
                                     const uint8_t* d_qflags, const float* d_Tcw, const float* d_Ow, const xfh_camera* cam, const xfh_grid_bounds* bounds,
                                     float th, const float* scale_factors, const float* ratio_max, int nlevels, const void* d_grids, const float* d_targets,
                                     size_t target_stride, int target_shared, int nt, const uint8_t* d_taken, int init_dist, float accept_max, void* d_ws,
                                     uint8_t* d_status, int* d_match_idx, int* d_best_dist, int* d_n_window, int* d_n_tested, int* d_level, float* d_proj_out,
                                     int* d_assigned, int* d_n_matches) {
    MapProjArgs m = {};
    if (!c || B < 1 || B > 65535 || target_shared < 0 || target_shared > 1) return XFH_ERR_INVALID_ARG;
    if (!mapproj_args_ok(form, nq, nt, cam, bounds, th, scale_factors, ratio_max, nlevels, accept_max, &m.lv)) return XFH_ERR_INVALID_ARG;
    if (!d_pts || !d_normals || !d_dist || !d_qdesc || !d_qflags || !d_Tcw || !d_Ow || !d_grids || !d_targets || !d_ws || !d_status || !d_match_idx ||
        !d_best_dist || !d_n_window || !d_n_tested || !d_level || !d_assigned || !d_n_matches) return XFH_ERR_INVALID_ARG;
    if (misaligned(15, d_qdesc, d_targets, d_grids, d_ws, target_shared ? (size_t)0 : target_stride) ||
        misaligned(3, d_pts, d_normals, d_dist, d_Tcw, d_Ow, d_match_idx, d_best_dist, d_n_window, d_n_tested, d_level, d_proj_out, d_assigned, d_n_matches))
        return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    ProjArgs& a = m.p;
    a.mode = XFH_PROJ_GIVEN; a.nq = nq; a.nt = nt; a.radius = 0.0f;
    a.pts = d_pts; a.Tcw = d_Tcw; a.cam = *cam; a.bounds = *bounds; a.qdesc = d_qdesc; a.qflags = d_qflags;
    a.grids = (const char*)d_grids; a.grid_stride = target_shared ? 0 : xfh_grid_bytes(nt);
    a.targets = (const char*)d_targets; a.target_stride = target_shared ? 0 : target_stride; a.skip = d_taken;
    a.init_dist = init_dist; a.nn_ratio = 0.0f;
    // (float)best <= accept_max for an integer best is best <= floorf(accept_max); past the int range every best passes
    const float fl = floorf(accept_max);
    a.th_high = fl >= 2147483648.0f ? INT_MAX : (int)fl;
    a.ws = (char*)d_ws; a.ws_stride = proj_ws_layout(nq, nt).bytes;
    a.status = d_status; a.match_idx = d_match_idx; a.best_dist = d_best_dist; a.second_dist = (int*)((char*)d_ws + mapproj_ws_second(nq, nt, B));
    a.n_candidates = d_n_tested; a.proj_out = d_proj_out; a.assigned = d_assigned; a.n_matches = d_n_matches;
    a.status_base = XFH_MAPPROJ_NO_CANDIDATES - XFH_PROJ_NO_CANDIDATES; a.flags_or = XFH_PROJ_FLAG_CLAIMS;
    m.normals = d_normals; m.dist = d_dist; m.Ow = d_Ow; m.th = th; m.form = form; m.n_window = d_n_window; m.level = d_level;
    HIPCK(c, launch_map_projection_search(c, m, B));
    return XFH_OK;
}

int xfh_map_projection_search(xfh_ctx* c, int form, int nq, const float* pts, const float* normals, const float* dist, const float* qdesc,
                              const uint8_t* qflags, const float* Tcw, const float* Ow, const xfh_camera* cam, const xfh_grid_bounds* bounds, float th,
                              const float* scale_factors, const float* ratio_max, int nlevels, const xfh_keypoint* kps, const float* targets, int nt,
                              const uint8_t* taken, int init_dist, float accept_max, uint8_t* status, int* match_idx, int* best_dist, int* n_window,
                              int* n_tested, int* level, float* proj_out, int* assigned, int* n_matches) {
    GridGeom g;
    FuseLevels lv;
    if (!c || !mapproj_args_ok(form, nq, nt, cam, bounds, th, scale_factors, ratio_max, nlevels, accept_max, &lv) || !grid_geom(bounds, &g)) return XFH_ERR_INVALID_ARG;
    if (!pts || !normals || !dist || !qdesc || !qflags || !Tcw || !Ow || !kps || !targets || !status || !match_idx || !best_dist || !n_window || !n_tested ||
        !level || !assigned || !n_matches) return XFH_ERR_INVALID_ARG;
    HostStage s{c};
    auto dq = s.in<float>(qdesc, (size_t)nq * 256), dp = s.in<float>(pts, (size_t)nq * 12), dn = s.in<float>(normals, (size_t)nq * 12);
    auto dd = s.in<float>(dist, (size_t)nq * 12);
    auto dfl = s.in<uint8_t>(qflags, (size_t)nq);
    auto dT = s.in<float>(Tcw, 48), dO = s.in<float>(Ow, 12);
    auto dt = s.in<float>(targets, (size_t)nt * 256);
    auto dk = s.in<xfh_keypoint>(kps, (size_t)nt * sizeof(xfh_keypoint));
    auto dtk = s.in_opt<uint8_t>(taken, (size_t)nt);
    auto dg = s.tmp<char>(xfh_grid_bytes(nt)), dws = s.tmp<char>(xfh_map_projection_search_workspace_bytes(nq, nt, 1));
    int* const out[5] = {match_idx, best_dist, n_window, n_tested, level};
    HostStage::Dev<int> o[5];
    for (int k = 0; k < 5; ++k) o[k] = s.out<int>(out[k], (size_t)nq * 4);
    auto dst = s.out<uint8_t>(status, (size_t)nq);
    auto dpo = s.out_opt<float>(proj_out, (size_t)nq * 12);
    auto das = s.out<int>(assigned, (size_t)nt * 4), dnm = s.out<int>(n_matches, 4);
    if (const int rc = s.upload(); rc != XFH_OK) return rc;
    HIPCK(c, launch_grid_build(c, dk, 0, nullptr, 0, dg, 0, nt, 1, g, 0));
    const int rc = xfh_map_projection_search_device(c, form, 1, nq, dp, dn, dd, dq, dfl, dT, dO, cam, bounds, th, scale_factors, ratio_max, nlevels, dg, dt, 0, 0, nt,
                                                    dtk, init_dist, accept_max, dws, dst, o[0], o[1], o[2], o[3], o[4], dpo, das, dnm);
    if (rc != XFH_OK) return rc;                                              // (a HIP error: every argument check has passed above)
    return s.download();
}

int xfh_sim3_project(const float* Tqw, const float* M, const xfh_camera* cam, const xfh_grid_bounds* bounds, float th, const float* scale_factors,
                     const float* ratio_max, int nlevels, const float* xyz, const float* distances, int n, float* uvr, int* level, uint8_t* status) {
    FuseLevels L;
    if (!Tqw || !M || !cam || !bounds || n < 0 || !fuse_levels(scale_factors, ratio_max, nlevels, &L)) return XFH_ERR_INVALID_ARG;
    if (n > 0 && (!xyz || !distances || !uvr || !level || !status)) return XFH_ERR_INVALID_ARG;
    for (int i = 0; i < n; ++i)
        status[i] = (uint8_t)xfh_sim3_point(Tqw, M, *cam, *bounds, th, L, xyz + 3 * (size_t)i, distances + 3 * (size_t)i, &uvr[3 * (size_t)i],
                                            &uvr[3 * (size_t)i + 1], &uvr[3 * (size_t)i + 2], &level[i]);
    return XFH_OK;
}

int xfh_sim3_search_device(xfh_ctx* c, int B, int side1_shared, const xfh_sim3_side* s1, const xfh_sim3_side* s2, const float* d_M21, const float* d_M12,
                           const xfh_camera* cam, const xfh_grid_bounds* bounds, float th, const float* scale_factors, const float* ratio_max, int nlevels,
                           int th_high, int* d_match12, int* d_n_found) {
    Sim3Args a = {};
    if (!c || B < 1 || B > 65535 || side1_shared < 0 || side1_shared > 1) return XFH_ERR_INVALID_ARG;
    if (!sim3_args_ok(s1, s2, cam, bounds, th, scale_factors, ratio_max, nlevels, &a.lv)) return XFH_ERR_INVALID_ARG;
    if (sim3_side_null(s1) || sim3_side_null(s2) || !s1->grid || !s2->grid || !d_M21 || !d_M12 || !d_match12 || !d_n_found) return XFH_ERR_INVALID_ARG;
    if (sim3_side_misaligned(s1) || sim3_side_misaligned(s2) || misaligned(3, d_M21, d_M12, d_match12, d_n_found)) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    a.s[0] = sim3_side(s1, side1_shared != 0); a.s[1] = sim3_side(s2, false);
    a.M21 = d_M21; a.M12 = d_M12; a.cam = *cam; a.bounds = *bounds; a.th = th; a.th_high = th_high; a.nb1 = (s1->n + 3) / 4;
    a.match12 = d_match12; a.n_found = d_n_found;
    HIPCK(c, launch_sim3_search(c, a, B));
    return XFH_OK;
}

int xfh_sim3_search(xfh_ctx* c, const xfh_sim3_side* s1, const xfh_sim3_side* s2, const float* M21, const float* M12, const xfh_camera* cam,
                    const xfh_grid_bounds* bounds, float th, const float* scale_factors, const float* ratio_max, int nlevels, int th_high,
                    int* match12, int* n_found) {
    GridGeom g;
    FuseLevels lv;
    if (!c || !sim3_args_ok(s1, s2, cam, bounds, th, scale_factors, ratio_max, nlevels, &lv) || !grid_geom(bounds, &g)) return XFH_ERR_INVALID_ARG;
    if (sim3_side_null(s1) || sim3_side_null(s2) || !s1->kps || !s2->kps || !M21 || !M12 || !match12 || !n_found) return XFH_ERR_INVALID_ARG;
    HostStage st{c};
    const xfh_sim3_side* hs[2] = {s1, s2};
    xfh_sim3_side ds[2];
    HostStage::Dev<xfh_keypoint> dk[2]; HostStage::Dev<char> dg[2]; HostStage::Dev<float> dd[2], dp[2], dr[2], dm[2], dT[2], dpo[2];
    HostStage::Dev<uint8_t> dfl[2], dst[2];
    HostStage::Dev<int> o[2][5];
    for (int s = 0; s < 2; ++s) {
        const xfh_sim3_side* h = hs[s];
        const size_t n = (size_t)h->n;
        dk[s] = st.in<xfh_keypoint>(h->kps, n * sizeof(xfh_keypoint)); dg[s] = st.tmp<char>(xfh_grid_bytes(h->n));
        dd[s] = st.in<float>(h->desc, n * 256); dp[s] = st.in<float>(h->points, n * 12); dr[s] = st.in<float>(h->dist, n * 12);
        dm[s] = st.in<float>(h->mp_desc, n * 256); dfl[s] = st.in<uint8_t>(h->flags, n); dT[s] = st.in<float>(h->Tw, 48);
        int* const out[5] = {h->match, h->best_dist, h->n_window, h->n_tested, h->level};
        for (int k = 0; k < 5; ++k) o[s][k] = st.out<int>(out[k], n * 4);
        dst[s] = st.out<uint8_t>(h->status, n); dpo[s] = st.out_opt<float>(h->proj_out_or_null, n * 12);
    }
    auto d21 = st.in<float>(M21, 48), d12 = st.in<float>(M12, 48);
    auto dm12 = st.out<int>(match12, (size_t)s1->n * 4), dnf = st.out<int>(n_found, 4);
    if (const int rc = st.upload(); rc != XFH_OK) return rc;
    for (int s = 0; s < 2; ++s) {
        HIPCK(c, launch_grid_build(c, dk[s], 0, nullptr, 0, dg[s], 0, hs[s]->n, 1, g, 0));
        ds[s] = xfh_sim3_side{hs[s]->n, (char*)dg[s], nullptr, dd[s], 0, dp[s], dr[s], dm[s], dfl[s], dT[s], dst[s], o[s][0], o[s][1], o[s][2], o[s][3],
                              o[s][4], dpo[s]};
    }
    const int rc = xfh_sim3_search_device(c, 1, 0, &ds[0], &ds[1], d21, d12, cam, bounds, th, scale_factors, ratio_max, nlevels, th_high, dm12, dnf);
    if (rc != XFH_OK) return rc;                                              // (a HIP error: every argument check has passed above)
    return st.download();
}

}  // extern "C"
