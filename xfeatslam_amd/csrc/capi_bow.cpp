// capi_bow.cpp -- the SearchByBoW entry points of include/xfeat_hip.h: the acceptance line on the host (bow_math.h, the kernel's own
// line), the workspace size, the device form and the host-pointer form (host_stage.h).
#include "host_stage.h"
#include "nodes_layout.h"
#include "bow_math.h"
#include <math.h>
#include <vector>

// what xfh_bow_search_device and xfh_bow_search check alike before anything is staged or launched (the pointers are theirs to check)
static bool bow_args_ok(int B, int n1, int n2, int shared, int flags, int init_dist, int th_low, float nn_ratio) {
    return B >= 1 && B <= 65535 && n1 >= 1 && n1 <= XFH_GRID_MAX_N && n2 >= 1 && n2 <= XFH_GRID_MAX_N && shared >= 0 && shared <= 2 &&
           !(flags & ~XFH_BOW_STRICT_LOW) && init_dist >= 0 && th_low >= 0 && isfinite(nn_ratio) && nn_ratio >= 0.0f;
}

extern "C" {

int xfh_bow_accept(int best_idx, int best, int second, int th_low, float nn_ratio, int flags) {
    return xfh_bow_accept_line(best_idx, best, second, th_low, nn_ratio, flags) ? 1 : 0;
}

size_t xfh_bow_search_workspace_bytes(int n1, int n2, int B) {
    if (B < 1 || B > 65535 || n1 < 1 || n1 > XFH_GRID_MAX_N || n2 < 1 || n2 > XFH_GRID_MAX_N) return 0;
    return bow_ws_layout(n1, B).bytes;
}

int xfh_bow_search_device(xfh_ctx* c, int B, int n1, int n2, int shared, int flags, int init_dist, int th_low, float nn_ratio, const void* d_nodes1,
                          const uint8_t* d_active1, const float* d_desc1, size_t desc1_stride_bytes, const void* d_nodes2, const uint8_t* d_eligible2,
                          const float* d_desc2, size_t desc2_stride_bytes, void* d_workspace, uint8_t* d_status, int* d_match12, int* d_best_dist,
                          int* d_second_dist, int* d_n_candidates, int* d_assigned2, int* d_n_matches) {
    if (!c || !bow_args_ok(B, n1, n2, shared, flags, init_dist, th_low, nn_ratio)) return XFH_ERR_INVALID_ARG;
    if (!d_nodes1 || !d_active1 || !d_desc1 || !d_nodes2 || !d_desc2 || !d_workspace || !d_status || !d_match12 || !d_best_dist || !d_second_dist ||
        !d_n_candidates || !d_assigned2 || !d_n_matches) return XFH_ERR_INVALID_ARG;
    if (misaligned(15, d_desc1, d_desc2, d_nodes1, d_nodes2, desc1_stride_bytes, desc2_stride_bytes, d_workspace) ||
        misaligned(3, d_match12, d_best_dist, d_second_dist, d_n_candidates, d_assigned2, d_n_matches)) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    const bool sh1 = shared == 1, sh2 = shared == 2;
    BowArgs a = {};
    a.flags = flags; a.init_dist = init_dist; a.th_low = th_low; a.nn_ratio = nn_ratio;
    a.s1 = BowSide{n1, sh1 ? 0 : (size_t)n1, sh1 ? 0 : nodes_bytes(n1), sh1 ? 0 : desc1_stride_bytes, (const char*)d_nodes1, d_active1, (const char*)d_desc1};
    a.s2 = BowSide{n2, sh2 ? 0 : (size_t)n2, sh2 ? 0 : nodes_bytes(n2), sh2 ? 0 : desc2_stride_bytes, (const char*)d_nodes2, d_eligible2, (const char*)d_desc2};
    a.ws = (char*)d_workspace;
    a.status = d_status; a.match12 = d_match12; a.best_dist = d_best_dist; a.second_dist = d_second_dist; a.n_candidates = d_n_candidates;
    a.assigned2 = d_assigned2; a.n_matches = d_n_matches;
    HIPCK(c, launch_bow_search(c, a, B));
    return XFH_OK;
}

int xfh_bow_search(xfh_ctx* c, int n1, int n2, int flags, int init_dist, int th_low, float nn_ratio, const uint32_t* node_of1, const uint8_t* active1,
                   const float* desc1, const uint32_t* node_of2, const uint8_t* eligible2, const float* desc2, uint8_t* status, int* match12, int* best_dist,
                   int* second_dist, int* n_candidates, int* assigned2, int* n_matches) {
    if (!c || !bow_args_ok(1, n1, n2, 0, flags, init_dist, th_low, nn_ratio)) return XFH_ERR_INVALID_ARG;
    if (!node_of1 || !active1 || !desc1 || !node_of2 || !desc2 || !status || !match12 || !best_dist || !second_dist || !n_candidates || !assigned2 || !n_matches)
        return XFH_ERR_INVALID_ARG;
    std::vector<char> b1(nodes_bytes(n1)), b2(nodes_bytes(n2));        // (alive until download()'s stream synchronise)
    if (xfh_nodes_pack(node_of1, n1, b1.data(), nullptr) != XFH_OK || xfh_nodes_pack(node_of2, n2, b2.data(), nullptr) != XFH_OK) return XFH_ERR_INVALID_ARG;
    HostStage s{c};
    auto dn1 = s.in<char>(b1.data(), b1.size()), dn2 = s.in<char>(b2.data(), b2.size());
    auto da1 = s.in<uint8_t>(active1, (size_t)n1);
    auto de2 = s.in_opt<uint8_t>(eligible2, (size_t)n2);
    auto dd1 = s.in<float>(desc1, (size_t)n1 * 256), dd2 = s.in<float>(desc2, (size_t)n2 * 256);
    auto dws = s.tmp<char>(bow_ws_layout(n1, 1).bytes);
    int* const out[4] = {match12, best_dist, second_dist, n_candidates};
    HostStage::Dev<int> o[4];
    for (int k = 0; k < 4; ++k) o[k] = s.out<int>(out[k], (size_t)n1 * 4);
    auto das = s.out<int>(assigned2, (size_t)n2 * 4);
    auto dst = s.out<uint8_t>(status, (size_t)n1);
    auto dnm = s.out<int>(n_matches, 4);
    if (const int rc = s.upload(); rc != XFH_OK) return rc;
    const int rc = xfh_bow_search_device(c, 1, n1, n2, 0, flags, init_dist, th_low, nn_ratio, dn1, da1, dd1, 0, dn2, de2, dd2, 0, dws, dst, o[0], o[1], o[2], o[3],
                                         das, dnm);
    if (rc != XFH_OK) return rc;                                              // (a HIP error: every argument check has passed above)
    return s.download();
}

}  // extern "C"
