// capi_triangulation.cpp -- the SearchForTriangulation entry points of include/xfeat_hip.h: the node index of a feature vector (host
// writer and reader of the blob of nodes_layout.h), the per-pair gates on the host (tri_math.h, the kernel's own lines), the device form
// and the host-pointer form (host_stage.h).
#include "host_stage.h"
#include "nodes_layout.h"
#include "tri_math.h"
#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>

// what xfh_triangulation_search_device and xfh_triangulation_search check alike before anything is staged or launched (the pointers are
// theirs to check)
static bool tri_args_ok(int B, int n1, int n2, int flags, float epipole_r2, float unc) {
    return B >= 1 && B <= 65535 && n1 >= 1 && n1 <= XFH_GRID_MAX_N && n2 >= 1 && n2 <= XFH_GRID_MAX_N &&
           !(flags & ~(XFH_TRI_ONLY_STEREO | XFH_TRI_COARSE)) && isfinite(epipole_r2) && isfinite(unc);
}

extern "C" {

size_t xfh_nodes_bytes(int n) { return n < 0 ? 0 : nodes_bytes(n); }

int xfh_nodes_pack(const uint32_t* node_of, int n, void* blob, int* n_nodes) {
    if (!node_of || !blob || n < 1 || n > XFH_GRID_MAX_N) return XFH_ERR_INVALID_ARG;
    std::vector<u64> keys;                                             // node << 32 | index: ascending = FeatureVector order
    keys.reserve(n);
    for (int i = 0; i < n; ++i) if (node_of[i] != XFH_NODE_NONE) keys.push_back(((u64)node_of[i] << 32) | (u64)(unsigned)i);
    std::sort(keys.begin(), keys.end());
    char* p = (char*)blob;
    memset(p, 0, nodes_bytes(n));
    uint32_t* ids = (uint32_t*)(p + nodes_ids_off(n));
    int32_t* ns = (int32_t*)(p + nodes_start_off(n));
    int32_t* items = (int32_t*)(p + nodes_items_off(n));
    int nn = 0;
    for (size_t k = 0; k < keys.size(); ++k) {
        const uint32_t id = (uint32_t)(keys[k] >> 32);
        if (k == 0 || id != ids[nn - 1]) { ids[nn] = id; ns[nn] = (int32_t)k; ++nn; }
        items[k] = (int32_t)(keys[k] & 0xFFFFFFFFull);
    }
    ns[nn] = (int32_t)keys.size();
    memcpy(p + nodes_of_off(n), node_of, (size_t)n * 4);
    NodesHeader h;
    memset(&h, 0, sizeof h);
    h.magic = XFH_NODES_MAGIC; h.n = n; h.n_nodes = nn; h.n_items = (int32_t)keys.size();
    memcpy(p, &h, sizeof h);
    if (n_nodes) *n_nodes = nn;
    return XFH_OK;
}

// host, stateless: a node blob -> node_ids[n] (the first *n_nodes are meaningful, the rest 0), node_start[n + 1] (entries past
// *n_nodes repeat the item count), items[n] (-1 past the item count).  Everything the blob claims is checked before it is used.
int xfh_nodes_unpack(const void* blob, size_t nbytes, int n, uint32_t* node_ids, int* node_start, int* items, int* n_nodes) {
    if (!blob || n < 1 || n > XFH_GRID_MAX_N || !node_ids || !node_start || !items || !n_nodes) return XFH_ERR_INVALID_ARG;
    if (nbytes < nodes_bytes(n)) return XFH_ERR_INVALID_ARG;                               // truncated
    NodesHeader h;
    memcpy(&h, blob, sizeof h);
    if (h.magic != XFH_NODES_MAGIC || h.n != n || h.n_nodes < 0 || h.n_nodes > n || h.n_items < h.n_nodes || h.n_items > n) return XFH_ERR_INVALID_ARG;
    const char* p = (const char*)blob;
    std::vector<uint32_t> ids(h.n_nodes), of(n);
    std::vector<int32_t> ns(h.n_nodes + 1), it(h.n_items);
    if (h.n_nodes) memcpy(ids.data(), p + nodes_ids_off(n), ids.size() * 4);
    memcpy(ns.data(), p + nodes_start_off(n), ns.size() * 4);
    if (h.n_items) memcpy(it.data(), p + nodes_items_off(n), it.size() * 4);
    memcpy(of.data(), p + nodes_of_off(n), of.size() * 4);
    if (ns[0] != 0 || ns[h.n_nodes] != h.n_items) return XFH_ERR_INVALID_ARG;
    int in_nodes = 0;
    for (int i = 0; i < n; ++i) in_nodes += of[i] != XFH_NODE_NONE ? 1 : 0;
    if (in_nodes != h.n_items) return XFH_ERR_INVALID_ARG;
    for (int k = 0; k < h.n_nodes; ++k) {
        if (ids[k] == XFH_NODE_NONE || (k > 0 && ids[k] <= ids[k - 1]) || ns[k + 1] <= ns[k] || ns[k + 1] > h.n_items) return XFH_ERR_INVALID_ARG;
        for (int q = ns[k]; q < ns[k + 1]; ++q)
            if (it[q] < 0 || it[q] >= n || of[it[q]] != ids[k] || (q > ns[k] && it[q] <= it[q - 1])) return XFH_ERR_INVALID_ARG;
    }
    for (int k = 0; k < n; ++k) { node_ids[k] = k < h.n_nodes ? ids[k] : 0; items[k] = k < h.n_items ? it[k] : -1; }
    for (int k = 0; k <= n; ++k) node_start[k] = k <= h.n_nodes ? ns[k] : h.n_items;
    *n_nodes = h.n_nodes;
    return XFH_OK;
}

int xfh_epipolar_gate(const float* F12, const float* ep, float epipole_r2, float unc, int flags, float x1, float y1, int stereo1, const float* xy2,
                      const float* uright2, int n, uint8_t* pass) {
    if (!F12 || !ep || n < 0 || (flags & ~(XFH_TRI_ONLY_STEREO | XFH_TRI_COARSE)) || (n > 0 && (!xy2 || !pass))) return XFH_ERR_INVALID_ARG;
    const TriLine l = xfh_tri_line(F12, x1, y1);
    const bool inactive = (flags & XFH_TRI_ONLY_STEREO) && !stereo1;                       // (:1166-1168: the query itself is skipped)
    for (int k = 0; k < n; ++k)
        pass[k] = inactive ? (uint8_t)XFH_TRI_GATE_SKIPPED
                           : (uint8_t)xfh_tri_member(l, ep[0], ep[1], epipole_r2, unc, flags, stereo1 != 0, xy2[2 * (size_t)k], xy2[2 * (size_t)k + 1],
                                                     uright2 ? uright2[k] : -1.0f);
    return XFH_OK;
}

int xfh_triangulation_search_device(xfh_ctx* c, int B, int n1, int n2, int side1_shared, int flags, int th_low, float epipole_r2, float unc,
                                    const void* d_nodes1, const float* d_xy1, const float* d_uright1, const uint8_t* d_has1, const float* d_desc1,
                                    size_t desc1_stride_bytes, const void* d_nodes2, const float* d_xy2, const float* d_uright2, const uint8_t* d_has2,
                                    const float* d_desc2, size_t desc2_stride_bytes, const float* d_F12, const float* d_ep, uint8_t* d_status,
                                    int* d_match12, int* d_best_dist, int* d_n_candidates, int* d_n_geom, int* d_n_matches) {
    if (!c || !tri_args_ok(B, n1, n2, flags, epipole_r2, unc) || (side1_shared != 0 && side1_shared != 1)) return XFH_ERR_INVALID_ARG;
    if (!d_nodes1 || !d_xy1 || !d_has1 || !d_desc1 || !d_nodes2 || !d_xy2 || !d_has2 || !d_desc2 || !d_F12 || !d_ep || !d_status || !d_match12 ||
        !d_best_dist || !d_n_candidates || !d_n_geom || !d_n_matches) return XFH_ERR_INVALID_ARG;
    if (misaligned(15, d_desc1, d_desc2, d_nodes1, d_nodes2, desc1_stride_bytes, desc2_stride_bytes) ||
        misaligned(3, d_xy1, d_xy2, d_uright1, d_uright2, d_F12, d_ep, d_match12, d_best_dist, d_n_candidates, d_n_geom, d_n_matches))
        return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    TriArgs a = {};
    a.flags = flags; a.th_low = th_low; a.epipole_r2 = epipole_r2; a.unc = unc;
    a.s1 = TriSide{n1, side1_shared ? 0 : (size_t)n1, side1_shared ? 0 : nodes_bytes(n1), side1_shared ? 0 : desc1_stride_bytes, (const char*)d_nodes1, d_xy1,
                   d_uright1, d_has1, (const char*)d_desc1};
    a.s2 = TriSide{n2, (size_t)n2, nodes_bytes(n2), desc2_stride_bytes, (const char*)d_nodes2, d_xy2, d_uright2, d_has2, (const char*)d_desc2};
    a.F12 = d_F12; a.ep = d_ep;
    a.status = d_status; a.match12 = d_match12; a.best_dist = d_best_dist; a.n_candidates = d_n_candidates; a.n_geom = d_n_geom; a.n_matches = d_n_matches;
    HIPCK(c, launch_triangulation_search(c, a, B));
    return XFH_OK;
}

int xfh_triangulation_search(xfh_ctx* c, int n1, int n2, int flags, int th_low, float epipole_r2, float unc, const uint32_t* node_of1, const float* xy1,
                             const float* uright1, const uint8_t* has1, const float* desc1, const uint32_t* node_of2, const float* xy2, const float* uright2,
                             const uint8_t* has2, const float* desc2, const float* F12, const float* ep, uint8_t* status, int* match12, int* best_dist,
                             int* n_candidates, int* n_geom, int* n_matches) {
    if (!c || !tri_args_ok(1, n1, n2, flags, epipole_r2, unc)) return XFH_ERR_INVALID_ARG;
    if (!node_of1 || !xy1 || !has1 || !desc1 || !node_of2 || !xy2 || !has2 || !desc2 || !F12 || !ep || !status || !match12 || !best_dist || !n_candidates ||
        !n_geom || !n_matches) return XFH_ERR_INVALID_ARG;
    std::vector<char> b1(nodes_bytes(n1)), b2(nodes_bytes(n2));        // (alive until download()'s stream synchronise)
    if (xfh_nodes_pack(node_of1, n1, b1.data(), nullptr) != XFH_OK || xfh_nodes_pack(node_of2, n2, b2.data(), nullptr) != XFH_OK) return XFH_ERR_INVALID_ARG;
    HostStage s{c};
    auto dn1 = s.in<char>(b1.data(), b1.size()), dn2 = s.in<char>(b2.data(), b2.size());
    auto dx1 = s.in<float>(xy1, (size_t)n1 * 8), dx2 = s.in<float>(xy2, (size_t)n2 * 8);
    auto du1 = s.in_opt<float>(uright1, (size_t)n1 * 4), du2 = s.in_opt<float>(uright2, (size_t)n2 * 4);
    auto dh1 = s.in<uint8_t>(has1, (size_t)n1), dh2 = s.in<uint8_t>(has2, (size_t)n2);
    auto dd1 = s.in<float>(desc1, (size_t)n1 * 256), dd2 = s.in<float>(desc2, (size_t)n2 * 256);
    auto dF = s.in<float>(F12, 36), de = s.in<float>(ep, 8);
    int* const out[4] = {match12, best_dist, n_candidates, n_geom};
    HostStage::Dev<int> o[4];
    for (int k = 0; k < 4; ++k) o[k] = s.out<int>(out[k], (size_t)n1 * 4);
    auto dst = s.out<uint8_t>(status, (size_t)n1);
    auto dnm = s.out<int>(n_matches, 4);
    if (const int rc = s.upload(); rc != XFH_OK) return rc;
    const int rc = xfh_triangulation_search_device(c, 1, n1, n2, 1, flags, th_low, epipole_r2, unc, dn1, dx1, du1, dh1, dd1, 0, dn2, dx2, du2, dh2, dd2, 0, dF, de,
                                                   dst, o[0], o[1], o[2], o[3], dnm);
    if (rc != XFH_OK) return rc;                                              // (a HIP error: every argument check has passed above)
    return s.download();
}

}  // extern "C"
