// capi_init.cpp -- the entry points of include/xfeat_hip.h that Tracking::MonocularInitialization calls: SearchForInitialization with the
// reference's retraction order (xfh_init_accept, xfh_init_search*): the acceptance line on the host (init_math.h, the kernels' own line), the
// device form and the host-pointer form (host_stage.h).
#include "host_stage.h"
#include "window_layout.h"
#include "init_math.h"
#include <math.h>
#include <vector>

// what xfh_init_search_device and xfh_init_search check alike before anything is staged or launched (the pointers are theirs to check)
static bool init_args_ok(int nq, int nt, float window, int th_low, float nn_ratio) {
    if (nq < 1 || nq > XFH_GRID_MAX_N || nt < 1 || nt > XFH_GRID_MAX_N) return false;
    return isfinite(window) && isfinite(nn_ratio) && nn_ratio >= 0.0f && th_low >= 0;
}

extern "C" {

int xfh_init_accept(int best, int second, int th_low, float nn_ratio) { return xfh_init_accept_line(best, second, th_low, nn_ratio) ? 1 : 0; }

int xfh_init_list_entries(void) { return XFH_INIT_K; }

size_t xfh_init_search_workspace_bytes(int nq, int nt, int B) {
    if (nq < 1 || nq > XFH_GRID_MAX_N || nt < 1 || nt > XFH_GRID_MAX_N || B < 1 || B > 65535) return 0;
    return init_ws_layout(nq, nt).bytes * (size_t)B;
}

int xfh_init_search_device(xfh_ctx* c, int B, int nq, const float* d_qdesc, const float* d_prev, const uint8_t* d_qflags, float window, const void* d_grids,
                           const float* d_targets, size_t target_stride, const float* d_target_xy, int nt, int th_low, float nn_ratio, void* d_ws,
                           uint8_t* d_status, int* d_claim_idx, int* d_matches12, int* d_best_dist, int* d_second_dist, int* d_n_window, int* d_n_tested,
                           int* d_matches21, int* d_matched_distance, int* d_n_matches, float* d_prev_out) {
    if (!c || B < 1 || B > 65535 || !init_args_ok(nq, nt, window, th_low, nn_ratio)) return XFH_ERR_INVALID_ARG;
    if ((d_target_xy != nullptr) != (d_prev_out != nullptr)) return XFH_ERR_INVALID_ARG;
    if (!d_qdesc || !d_prev || !d_grids || !d_targets || !d_ws || !d_status || !d_claim_idx || !d_matches12 || !d_best_dist || !d_second_dist || !d_n_window ||
        !d_n_tested || !d_matches21 || !d_matched_distance || !d_n_matches) return XFH_ERR_INVALID_ARG;
    if (misaligned(15, d_qdesc, d_targets, d_grids, d_ws, target_stride) ||
        misaligned(3, d_prev, d_target_xy, d_claim_idx, d_matches12, d_best_dist, d_second_dist, d_n_window, d_n_tested, d_matches21, d_matched_distance,
                   d_n_matches, d_prev_out)) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    InitArgs a = {};
    a.nq = nq; a.nt = nt; a.window = window; a.qdesc = d_qdesc; a.prev = d_prev; a.qflags = d_qflags;
    a.grids = (const char*)d_grids; a.grid_stride = xfh_grid_bytes(nt); a.targets = (const char*)d_targets; a.target_stride = target_stride;
    a.target_xy = d_target_xy; a.th_low = th_low; a.nn_ratio = nn_ratio;
    a.ws = (char*)d_ws; a.ws_stride = init_ws_layout(nq, nt).bytes;
    a.status = d_status; a.claim_idx = d_claim_idx; a.matches12 = d_matches12; a.best_dist = d_best_dist; a.second_dist = d_second_dist;
    a.n_window = d_n_window; a.n_tested = d_n_tested; a.matches21 = d_matches21; a.matched_distance = d_matched_distance; a.n_matches = d_n_matches;
    a.prev_out = d_prev_out;
    HIPCK(c, launch_init_search(c, a, B));
    return XFH_OK;
}

int xfh_init_search(xfh_ctx* c, int nq, const float* qdesc, const float* prev, const uint8_t* qflags, float window, const xfh_keypoint* kps,
                    const xfh_grid_bounds* bounds, const float* targets, int nt, int th_low, float nn_ratio, uint8_t* status, int* claim_idx, int* matches12,
                    int* best_dist, int* second_dist, int* n_window, int* n_tested, int* matches21, int* matched_distance, int* n_matches, float* prev_out) {
    GridGeom g;
    if (!c || !grid_geom(bounds, &g) || !init_args_ok(nq, nt, window, th_low, nn_ratio)) return XFH_ERR_INVALID_ARG;
    if (!qdesc || !prev || !kps || !targets || !status || !claim_idx || !matches12 || !best_dist || !second_dist || !n_window || !n_tested || !matches21 ||
        !matched_distance || !n_matches) return XFH_ERR_INVALID_ARG;
    std::vector<float> xy;                                                    // mvKeysUn[k].pt of the targets: what prev_out takes (:945)
    if (prev_out) { xy.resize((size_t)nt * 2); for (int k = 0; k < nt; ++k) { xy[2 * (size_t)k] = kps[k].x; xy[2 * (size_t)k + 1] = kps[k].y; } }
    HostStage s{c};
    auto dq = s.in<float>(qdesc, (size_t)nq * 256), dp = s.in<float>(prev, (size_t)nq * 8);
    auto dfl = s.in_opt<uint8_t>(qflags, (size_t)nq);
    auto dt = s.in<float>(targets, (size_t)nt * 256);
    auto dk = s.in<xfh_keypoint>(kps, (size_t)nt * sizeof(xfh_keypoint));
    auto dxy = s.in_opt<float>(prev_out ? xy.data() : nullptr, (size_t)nt * 8);
    auto dg = s.tmp<char>(xfh_grid_bytes(nt)), dws = s.tmp<char>(init_ws_layout(nq, nt).bytes);
    int* const out[6] = {claim_idx, matches12, best_dist, second_dist, n_window, n_tested};
    HostStage::Dev<int> o[6];
    for (int k = 0; k < 6; ++k) o[k] = s.out<int>(out[k], (size_t)nq * 4);
    auto dst = s.out<uint8_t>(status, (size_t)nq);
    auto d21 = s.out<int>(matches21, (size_t)nt * 4), dmd = s.out<int>(matched_distance, (size_t)nt * 4), dnm = s.out<int>(n_matches, 4);
    auto dpo = s.out_opt<float>(prev_out, (size_t)nq * 8);
    if (const int rc = s.upload(); rc != XFH_OK) return rc;
    HIPCK(c, launch_grid_build(c, dk, 0, nullptr, 0, dg, 0, nt, 1, g, 0));
    const int rc = xfh_init_search_device(c, 1, nq, dq, dp, dfl, window, dg, dt, 0, dxy, nt, th_low, nn_ratio, dws, dst, o[0], o[1], o[2], o[3], o[4], o[5], d21,
                                          dmd, dnm, dpo);
    if (rc != XFH_OK) return rc;                                              // (a HIP error: every argument check has passed above)
    return s.download();
}

}  // extern "C"
