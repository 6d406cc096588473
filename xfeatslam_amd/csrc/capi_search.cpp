// capi_search.cpp -- the matcher and search entry points of include/xfeat_hip.h: mutual nearest neighbours, distance tables, the CSR forms,
// frame grid, windowed search, frame finish, SearchByProjection.  Each device form checks its arguments and launches; each host-pointer form
// stages its arrays through the ctx' one arena (host_stage.h) around the same launch.
#include "host_stage.h"
#include "window_layout.h"
#include "frame_math.h"
#include "projection_layout.h"
#include <math.h>
#include <string.h>

// Many pairs in one call (ORBmatcher::match once per frame pair in the reference, ORBmatcher.cc:358-372; its consumers meet one frame with
// several partners): one persistent GEMM launch over the tiles of all pairs + one post launch (kernels_match.hip: launch_mnn_batch).
int gather_pairs(xfh_ctx* c, int n_pairs, const void* const* image1, const int* n1, const void* const* image2, const int* n2,
                 int* const* idx1, int* const* idx2, float* const* dist, int* n_matches, bool need_out, std::vector<XfhMatchPair>& v) {
    if (!c || n_pairs < 0 || (n_pairs > 0 && (!image1 || !n1 || !image2 || !n2))) return XFH_ERR_INVALID_ARG;
    if (need_out && n_pairs > 0 && (!idx1 || !idx2 || !dist || !n_matches)) return XFH_ERR_INVALID_ARG;
    v.resize((size_t)n_pairs);
    for (int p = 0; p < n_pairs; ++p) {
        if (n1[p] < 0 || n2[p] < 0) return XFH_ERR_INVALID_ARG;
        if ((n1[p] > 0 && !image1[p]) || (n2[p] > 0 && !image2[p])) return XFH_ERR_INVALID_ARG;
        if (misaligned(15, image1[p], image2[p])) return XFH_ERR_INVALID_ARG;
        if (need_out && n1[p] > 0 && n2[p] > 0 && (!idx1[p] || !idx2[p] || !dist[p])) return XFH_ERR_INVALID_ARG;
        v[p] = XfhMatchPair{(const float*)image1[p], n1[p], (const float*)image2[p], n2[p], need_out ? idx1[p] : nullptr, need_out ? idx2[p] : nullptr,
                            need_out ? dist[p] : nullptr, need_out ? n_matches + p : nullptr};
    }
    return XFH_OK;
}
// CSR input of the host forms: offsets[0..n] non-negative and non-decreasing, every index in [0, limit), lists and rows present unless all
// lists are empty; *longest = the longest list
static bool csr_ok(const int* offsets, int n, const int* indices, const float* rows, int limit, int* longest) {
    if (offsets[n] < 0 || (offsets[n] > 0 && (!indices || !rows))) return false;
    for (int i = 0; i < n; ++i) {
        if (offsets[i] < 0 || offsets[i] > offsets[i + 1]) return false;
        if (longest && offsets[i + 1] - offsets[i] > *longest) *longest = offsets[i + 1] - offsets[i];
    }
    for (int p = 0; p < offsets[n]; ++p) if (indices[p] < 0 || indices[p] >= limit) return false;
    return true;
}

// the pieces of xfh_match_mnn, declared in one place for the call itself and for the reservation xfh_create makes.  Output block: n at
// int 0, idx1 / idx2 / dist from byte 256 on, nm = min(n1, n2) entries each.
struct MnnStage { HostStage::Dev<float> d1, d2; HostStage::Dev<int> o; size_t ob; };
static MnnStage mnn_declare(HostStage& s, const float* d1, int n1, const float* d2, int n2) {
    const size_t ob = (size_t)(n1 < n2 ? n1 : n2) * 12 + 256;
    return {s.in<float>(d1, (size_t)n1 * 256), s.in<float>(d2, (size_t)n2 * 256), s.tmp<int>(ob), ob};     // (a braced list is evaluated left to right)
}
size_t match_mnn_stage_bytes(int n1, int n2) { HostStage s{nullptr}; mnn_declare(s, nullptr, n1, nullptr, n2); return HostStage::layout(s.pc, s.n); }

extern "C" {

// ------------------------------------------------------------------------- matching
int xfh_descriptor_distance(const float* a, const float* b) {
    double s = 0.0;
    for (int k = 0; k < 64; ++k) { const double d = (double)(a[k] - b[k]); s = fma(d, d, s); }      // the device kernels' expression (k_dist_i32)
    const float nd = (float)s;
    return (int)(nd * 512);
}

int xfh_match_mnn_device(xfh_ctx* c, const float* d1, int n1, const float* d2, int n2, float min_cossim,
                         int* idx1, int* idx2, float* dist, int* n_matches) {
    if (!c || n1 < 0 || n2 < 0 || !n_matches) return XFH_ERR_INVALID_ARG;
    if ((n1 > 0 && !d1) || (n2 > 0 && !d2)) return XFH_ERR_INVALID_ARG;
    if (n1 > 0 && n2 > 0 && (!idx1 || !idx2 || !dist)) return XFH_ERR_INVALID_ARG;
    if (misaligned(15, d1, d2)) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    XfhRange range("xfh:match_mnn_device");
    HIPCK(c, launch_mnn(c, d1, n1, d2, n2, min_cossim, idx1, idx2, dist, n_matches));
    return XFH_OK;
}

size_t xfh_match_image_bytes(int n) { return n <= 0 ? 0 : (size_t)((n + 255) / 256) * 256 * 64 * sizeof(float); }

int xfh_match_prepare_device(xfh_ctx* c, const float* d, int n, void* image) {
    if (!c || n < 0) return XFH_ERR_INVALID_ARG;
    if (n == 0) return XFH_OK;
    if (!d || !image || misaligned(15, d, image)) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, launch_match_prepare(c, d, n, (float*)image));
    return XFH_OK;
}

int xfh_match_mnn_prepared_device(xfh_ctx* c, const void* image1, int n1, const void* image2, int n2, float min_cossim,
                                  int* idx1, int* idx2, float* dist, int* n_matches) {
    if (!c || n1 < 0 || n2 < 0 || !n_matches) return XFH_ERR_INVALID_ARG;
    if ((n1 > 0 && !image1) || (n2 > 0 && !image2)) return XFH_ERR_INVALID_ARG;
    if (n1 > 0 && n2 > 0 && (!idx1 || !idx2 || !dist)) return XFH_ERR_INVALID_ARG;
    if (misaligned(15, image1, image2)) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    XfhRange range("xfh:match_mnn_prepared_device");
    HIPCK(c, launch_mnn_prepared(c, (const float*)image1, n1, (const float*)image2, n2, min_cossim, idx1, idx2, dist, n_matches));
    return XFH_OK;
}

int xfh_match_mnn_prepared_batch_device(xfh_ctx* c, int n_pairs, const void* const* image1, const int* n1, const void* const* image2, const int* n2,
                                        float min_cossim, int* const* idx1, int* const* idx2, float* const* dist, int* n_matches) {
    std::vector<XfhMatchPair> v;
    const int rc = gather_pairs(c, n_pairs, image1, n1, image2, n2, idx1, idx2, dist, n_matches, true, v);
    if (rc != XFH_OK) return rc;
    if (n_pairs == 0) return XFH_OK;
    HIPCK(c, hipSetDevice(c->cfg.device));
    XfhRange range("xfh:match_mnn_prepared_batch_device");
    HIPCK(c, launch_mnn_batch(c, v.data(), n_pairs, min_cossim));
    return XFH_OK;
}

// n_valid-aware form: the two sets are the nfeatures slots of two extraction records whose prepared images came
// out of xfh_extract_batch_device_images; pairs that touch a padding slot are not reported (the reference's match() would report
// them: zero rows have similarity 0 with everything, ORBmatcher.cc:358-372).  Otherwise xfh_match_mnn_prepared_device.
int xfh_match_records_device(xfh_ctx* c, const void* d_record1, const void* image1, const void* d_record2, const void* image2, float min_cossim,
                             int* idx1, int* idx2, float* dist, int* n_matches) {
    if (!c || !d_record1 || !d_record2 || !image1 || !image2 || !idx1 || !idx2 || !dist || !n_matches) return XFH_ERR_INVALID_ARG;
    if (misaligned(15, image1, image2)) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    const int nf = c->cfg.nfeatures;
    HIPCK(c, launch_mnn_prepared(c, (const float*)image1, nf, (const float*)image2, nf, min_cossim, idx1, idx2, dist, n_matches,
                                 (const int*)d_record1, (const int*)d_record2));
    return XFH_OK;
}

int xfh_match_mnn(xfh_ctx* c, const float* d1, int n1, const float* d2, int n2, float min_cossim,
                  int* idx1, int* idx2, float* dist, int* n_matches) {
    if (!c || n1 < 0 || n2 < 0 || !n_matches) return XFH_ERR_INVALID_ARG;
    if (n1 == 0 || n2 == 0) { *n_matches = 0; return XFH_OK; }
    if (!d1 || !d2 || !idx1 || !idx2 || !dist) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));                                   // (for the pinned mirror; the other forms leave it to upload())
    XfhRange range("xfh:match_mnn");
    MatchWs& w = c->mws;
    HostStage s{c};
    const int nm = n1 < n2 ? n1 : n2;
    const MnnStage m = mnn_declare(s, d1, n1, d2, n2);                       // fits the reservation of xfh_create up to nfeatures x nfeatures
    if (w.cap_hout < m.ob) {
        if (w.h_out) { hipHostFree(w.h_out); w.h_out = nullptr; w.cap_hout = 0; }
        HIPCK(c, hipHostMalloc((void**)&w.h_out, m.ob, hipHostMallocDefault));
        w.cap_hout = m.ob;
    }
    if (const int rc = s.upload(); rc != XFH_OK) return rc;
    int* o = m.o;
    HIPCK(c, launch_mnn(c, m.d1, n1, m.d2, n2, min_cossim, o + 64, o + 64 + nm, (float*)(o + 64 + 2 * (size_t)nm), o));
    // one asynchronous copy of the whole output block into pinned memory (<= 48 KB at 4096 rows), then one wait
    HIPCK(c, hipMemcpyAsync(w.h_out, o, m.ob, hipMemcpyDeviceToHost, c->stream));
    if (const int rc = s.download(); rc != XFH_OK) return rc;
    const int n = w.h_out[0];
    if (n < 0 || n > nm) { c->hip_err = "k_mnn_post: collector timed out"; return XFH_ERR_HIP; }
    memcpy(idx1, w.h_out + 64, (size_t)n * 4);
    memcpy(idx2, w.h_out + 64 + nm, (size_t)n * 4);
    memcpy(dist, w.h_out + 64 + 2 * (size_t)nm, (size_t)n * 4);
    *n_matches = n;
    return XFH_OK;
}

int xfh_distance_i32_device(xfh_ctx* c, const float* d1, int n1, const float* d2, int n2, int32_t* out) {
    if (!c || n1 < 0 || n2 < 0) return XFH_ERR_INVALID_ARG;
    if (n1 > 0 && n2 > 0 && (!d1 || !d2 || !out)) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, launch_dist_i32(c, d1, n1, d2, n2, out));
    return XFH_OK;
}

int xfh_distance_i32(xfh_ctx* c, const float* d1, int n1, const float* d2, int n2, int32_t* out) {
    if (!c || n1 < 0 || n2 < 0) return XFH_ERR_INVALID_ARG;
    if (n1 == 0 || n2 == 0) return XFH_OK;
    if (!d1 || !d2 || !out) return XFH_ERR_INVALID_ARG;
    HostStage s{c};
    auto dd1 = s.in<float>(d1, (size_t)n1 * 256), dd2 = s.in<float>(d2, (size_t)n2 * 256);
    auto tab = s.out<int32_t>(out, (size_t)n1 * n2 * 4);
    if (const int rc = s.upload(); rc != XFH_OK) return rc;
    HIPCK(c, launch_dist_i32(c, dd1, n1, dd2, n2, tab));
    return s.download();
}

int xfh_best2_csr_device(xfh_ctx* c, const float* q, int nq, const float* tg, int nt, const int* offsets, const int* indices, int init_dist,
                         int* best_idx, int* best_dist, int* second_idx, int* second_dist) {
    if (!c || nq < 0 || nt < 0) return XFH_ERR_INVALID_ARG;
    if (nq == 0) return XFH_OK;
    if (!q || !offsets || !indices || !tg || !best_idx || !best_dist || !second_idx || !second_dist) return XFH_ERR_INVALID_ARG;
    if (misaligned(15, q, tg)) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, launch_best2(c, q, nq, tg, offsets, indices, init_dist, best_idx, best_dist, second_idx, second_dist));
    return XFH_OK;
}

int xfh_best2_csr(xfh_ctx* c, const float* q, int nq, const float* tg, int nt, const int* offsets, const int* indices, int init_dist,
                  int* best_idx, int* best_dist, int* second_idx, int* second_dist) {
    if (!c || nq < 0 || nt < 0) return XFH_ERR_INVALID_ARG;
    if (nq == 0) return XFH_OK;
    if (!q || !offsets || !best_idx || !best_dist || !second_idx || !second_dist) return XFH_ERR_INVALID_ARG;
    if (!csr_ok(offsets, nq, indices, tg, nt, nullptr)) return XFH_ERR_INVALID_ARG;
    HostStage s{c};
    auto dq = s.in<float>(q, (size_t)nq * 256), dt = s.in<float>(tg, (size_t)nt * 256);
    auto doff = s.in<int>(offsets, (size_t)(nq + 1) * 4), dind = s.in<int>(indices, (size_t)offsets[nq] * 4);
    auto o0 = s.out<int>(best_idx, (size_t)nq * 4), o1 = s.out<int>(best_dist, (size_t)nq * 4), o2 = s.out<int>(second_idx, (size_t)nq * 4), o3 = s.out<int>(second_dist, (size_t)nq * 4);
    if (const int rc = s.upload(); rc != XFH_OK) return rc;
    HIPCK(c, launch_best2(c, dq, nq, dt, doff, dind, init_dist, o0, o1, o2, o3));
    return s.download();
}

// ---- frame grid + windowed search (window_search.hip.h, window_layout.h) -----------------------------------
size_t xfh_grid_bytes(int n) { return n < 0 ? 0 : (size_t)XFH_GRID_ITEMS_OFF + (size_t)n * sizeof(GridItem); }

int xfh_grid_build_device(xfh_ctx* c, const xfh_keypoint* d_kps, int n, const void* d_record, const xfh_grid_bounds* bounds, int flags, void* d_grid) {
    GridGeom g;
    if (!c || n < 0 || n > XFH_GRID_MAX_N || !d_grid || (n > 0 && !d_kps) || (flags & ~XFH_GRID_SKIP_PADDING)) return XFH_ERR_INVALID_ARG;
    if ((flags & XFH_GRID_SKIP_PADDING) && !d_record) return XFH_ERR_INVALID_ARG;          // which slots are padding is the record header's knowledge
    if (misaligned(15, d_grid) || misaligned(3, d_kps, d_record) || !grid_geom(bounds, &g)) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, launch_grid_build(c, d_kps, 0, d_record, 0, d_grid, 0, n, 1, g, flags));
    return XFH_OK;
}

int xfh_grid_build_records_device(xfh_ctx* c, const void* d_records, int B, const xfh_grid_bounds* bounds, int flags, void* d_grids) {
    GridGeom g;
    if (!c || B < 0 || (flags & ~XFH_GRID_SKIP_PADDING) || !grid_geom(bounds, &g)) return XFH_ERR_INVALID_ARG;
    if (B == 0) return XFH_OK;
    const int nf = c->cfg.nfeatures;
    if (!d_records || !d_grids || nf > XFH_GRID_MAX_N || misaligned(15, d_grids) || misaligned(3, d_records)) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    const size_t rb = xfh_record_bytes(nf);
    HIPCK(c, launch_grid_build(c, (const char*)d_records + xfh_record_kps_offset(), rb, d_records, rb, d_grids, xfh_grid_bytes(nf), nf, B, g, flags));
    return XFH_OK;
}

// host, stateless: a grid blob copied out of device memory -> cell_start[64 * 48 + 1] (cell = ix * 48 + iy), items[n] (slot numbers
// in cell order; the first *n_binned are meaningful, the rest -1).  Everything the blob claims is checked before it is used.
int xfh_grid_unpack(const void* blob, size_t nbytes, int n, int* cell_start, int* items, int* n_binned) {
    if (!blob || n < 0 || !cell_start || (n > 0 && !items)) return XFH_ERR_INVALID_ARG;
    if (nbytes < xfh_grid_bytes(n)) return XFH_ERR_INVALID_ARG;                            // truncated
    GridHeader h;
    memcpy(&h, blob, sizeof h);
    if (h.magic != XFH_GRID_MAGIC || h.n != n || h.n_binned < 0 || h.n_binned > n) return XFH_ERR_INVALID_ARG;
    const char* p = (const char*)blob;
    std::vector<int> cs(XFH_GRID_CELLS + 1);
    memcpy(cs.data(), p + XFH_GRID_CS_OFF, cs.size() * sizeof(int));
    if (cs[0] != 0 || cs[XFH_GRID_CELLS] != h.n_binned) return XFH_ERR_INVALID_ARG;
    for (int k = 0; k < XFH_GRID_CELLS; ++k) if (cs[k] > cs[k + 1]) return XFH_ERR_INVALID_ARG;      // (with the two ends: every entry in [0, n_binned])
    for (int k = 0; k < h.n_binned; ++k) {
        GridItem it;
        memcpy(&it, p + XFH_GRID_ITEMS_OFF + (size_t)k * sizeof it, sizeof it);
        if (it.index < 0 || it.index >= n) return XFH_ERR_INVALID_ARG;
    }
    memcpy(cell_start, cs.data(), cs.size() * sizeof(int));
    for (int k = 0; k < n; ++k) {
        GridItem it;
        memcpy(&it, p + XFH_GRID_ITEMS_OFF + (size_t)k * sizeof it, sizeof it);
        items[k] = k < h.n_binned ? it.index : -1;
    }
    if (n_binned) *n_binned = h.n_binned;
    return XFH_OK;
}

int xfh_search_window_device(xfh_ctx* c, const float* q, const float* uvr, int nq, const void* d_grid, const float* tg, int nt,
                             const uint8_t* skip, const float* uright, const float* ur_query, int init_dist,
                             int* best_idx, int* best_dist, int* second_idx, int* second_dist, int* n_candidates) {
    if (!c || nq < 0 || nt < 0 || nt > XFH_GRID_MAX_N) return XFH_ERR_INVALID_ARG;
    if ((uright != nullptr) != (ur_query != nullptr)) return XFH_ERR_INVALID_ARG;
    if (nq == 0) return XFH_OK;
    if (!q || !uvr || !d_grid || (nt > 0 && !tg) || !best_idx || !best_dist || !second_idx || !second_dist || !n_candidates) return XFH_ERR_INVALID_ARG;
    if (misaligned(15, q, tg, d_grid) || misaligned(3, uvr, uright, ur_query)) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, launch_search_window(c, q, uvr, nq, d_grid, tg, nt, skip, uright, ur_query, init_dist, best_idx, best_dist, second_idx, second_dist, n_candidates));
    return XFH_OK;
}

int xfh_search_window(xfh_ctx* c, const float* q, const float* uvr, int nq, const xfh_keypoint* kps, const xfh_grid_bounds* bounds,
                      const float* tg, int nt, const uint8_t* skip, const float* uright, const float* ur_query, int init_dist,
                      int* best_idx, int* best_dist, int* second_idx, int* second_dist, int* n_candidates) {
    GridGeom g;
    if (!c || nq < 0 || nt < 0 || nt > XFH_GRID_MAX_N || !grid_geom(bounds, &g)) return XFH_ERR_INVALID_ARG;
    if ((uright != nullptr) != (ur_query != nullptr)) return XFH_ERR_INVALID_ARG;
    if (nq == 0) return XFH_OK;
    if (!q || !uvr || (nt > 0 && (!tg || !kps)) || !best_idx || !best_dist || !second_idx || !second_dist || !n_candidates) return XFH_ERR_INVALID_ARG;
    HostStage s{c};
    auto dq = s.in<float>(q, (size_t)nq * 256), du = s.in<float>(uvr, (size_t)nq * 12);
    auto dt = s.in<float>(tg, (size_t)nt * 256);
    auto dk = s.in<xfh_keypoint>(kps, (size_t)nt * sizeof(xfh_keypoint));
    auto dsk = s.in_opt<uint8_t>(skip, (size_t)nt);
    auto dur = s.in_opt<float>(uright, (size_t)nt * 4), duq = s.in_opt<float>(ur_query, (size_t)nq * 4);
    auto dg = s.tmp<char>(xfh_grid_bytes(nt));
    int* const out[5] = {best_idx, best_dist, second_idx, second_dist, n_candidates};
    HostStage::Dev<int> o[5];
    for (int k = 0; k < 5; ++k) o[k] = s.out<int>(out[k], (size_t)nq * 4);
    if (const int rc = s.upload(); rc != XFH_OK) return rc;
    HIPCK(c, launch_grid_build(c, dk, 0, nullptr, 0, dg, 0, nt, 1, g, 0));
    HIPCK(c, launch_search_window(c, dq, du, nq, dg, dt, nt, dsk, dur, duq, init_dist, o[0], o[1], o[2], o[3], o[4]));
    return s.download();
}

// ---- finishing an RGB-D frame: undistort, depth / right coordinate, grid of the undistorted keypoints (frame_math.h, frame_finish.hip.h) ----
int xfh_undistort_points(const xfh_camera* cam, const float* xy, int n, float* xy_un) {
    if (!cam || n < 0 || (n > 0 && (!xy || !xy_un))) return XFH_ERR_INVALID_ARG;
    for (int i = 0; i < n; ++i) xfh_undistort_point(*cam, xy[2 * i], xy[2 * i + 1], &xy_un[2 * i], &xy_un[2 * i + 1]);
    return XFH_OK;
}

// Frame::ComputeImageBounds (Frame.cc:975-1002)
int xfh_camera_bounds(const xfh_camera* cam, xfh_grid_bounds* out) {
    if (!cam || !out || cam->width <= 0 || cam->height <= 0) return XFH_ERR_INVALID_ARG;
    const float w = (float)cam->width, h = (float)cam->height;
    if (cam->k1 == 0.0f) { out->min_x = 0.0f; out->min_y = 0.0f; out->max_x = w; out->max_y = h; return XFH_OK; }
    const float in[8] = {0.0f, 0.0f, w, 0.0f, 0.0f, h, w, h};
    float p[8];
    for (int i = 0; i < 4; ++i) xfh_undistort_point(*cam, in[2 * i], in[2 * i + 1], &p[2 * i], &p[2 * i + 1]);
    // std::min / std::max as the reference calls them (a NaN in the second operand is not taken)
    out->min_x = p[4] < p[0] ? p[4] : p[0]; out->max_x = p[2] < p[6] ? p[6] : p[2];
    out->min_y = p[3] < p[1] ? p[3] : p[1]; out->max_y = p[5] < p[7] ? p[7] : p[5];
    return XFH_OK;
}

// the checks the two finish calls share: camera size, depth type / pitch / alignment
static bool finish_depth_ok(const xfh_camera* cam, const void* depth, int depth_type, size_t pitch) {
    if (!cam || cam->width <= 0 || cam->height <= 0) return false;
    if (depth_type != XFH_DEPTH_NONE && depth_type != XFH_DEPTH_F32 && depth_type != XFH_DEPTH_U16) return false;
    if (depth_type == XFH_DEPTH_NONE || !depth) return true;                               // no image: -1 everywhere, pitch unused
    const size_t es = depth_type == XFH_DEPTH_F32 ? 4 : 2;
    return pitch >= (size_t)cam->width * es && pitch % es == 0 && !misaligned(es - 1, depth);
}

int xfh_frame_finish_records_device(xfh_ctx* c, const void* d_records, int B, const xfh_camera* cam, const void* d_depth, int depth_type, size_t depth_pitch,
                                    float depth_scale, const xfh_grid_bounds* bounds, int flags, float* d_xy_un, float* d_uright, float* d_depth_out, void* d_grids) {
    if (!c || B < 1 || B > c->cfg.max_batch || (flags & ~XFH_GRID_SKIP_PADDING) || !finish_depth_ok(cam, d_depth, depth_type, depth_pitch)) return XFH_ERR_INVALID_ARG;
    GridGeom g = {};
    if (d_grids && !grid_geom(bounds, &g)) return XFH_ERR_INVALID_ARG;
    const int nf = c->cfg.nfeatures;
    if (!d_records || !d_xy_un || !d_uright || !d_depth_out || (d_grids && nf > XFH_GRID_MAX_N)) return XFH_ERR_INVALID_ARG;
    if (misaligned(15, d_grids) || misaligned(3, d_records, d_xy_un, d_uright, d_depth_out)) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    const size_t rb = xfh_record_bytes(nf);
    HIPCK(c, launch_frame_finish(c, (const char*)d_records + xfh_record_kps_offset(), rb, d_records, rb, *cam, d_depth, depth_type, depth_pitch, depth_scale,
                                 d_xy_un, d_uright, d_depth_out, d_grids, xfh_grid_bytes(nf), nf, B, g, flags));
    return XFH_OK;
}

int xfh_frame_finish(xfh_ctx* c, const xfh_keypoint* kps, int n, const xfh_camera* cam, const void* depth_img, int depth_type, size_t depth_pitch,
                     float depth_scale, float* xy_un, float* uright, float* depth) {
    if (!c || n < 0 || !finish_depth_ok(cam, depth_img, depth_type, depth_pitch)) return XFH_ERR_INVALID_ARG;
    if (n == 0) return XFH_OK;
    if (depth_type == XFH_DEPTH_NONE) depth_img = nullptr;
    if (!kps || !xy_un || !uright || !depth) return XFH_ERR_INVALID_ARG;
    HostStage s{c};
    auto dk = s.in<xfh_keypoint>(kps, (size_t)n * sizeof(xfh_keypoint));
    auto dimg = s.in_opt<char>(depth_img, (size_t)cam->height * depth_pitch);
    auto dxy = s.out<float>(xy_un, (size_t)n * 8), dur = s.out<float>(uright, (size_t)n * 4), ddz = s.out<float>(depth, (size_t)n * 4);
    if (const int rc = s.upload(); rc != XFH_OK) return rc;
    GridGeom g = {};
    HIPCK(c, launch_frame_finish(c, dk, 0, nullptr, 0, *cam, dimg, depth_type, depth_pitch, depth_scale, dxy, dur, ddz, nullptr, 0, n, 1, g, 0));
    return s.download();
}

// ---- SearchByProjection with the reference's claim order (projection_math.h, projection_search.hip.h) ---------------------------------
int xfh_project_points(const float* Tcw, const xfh_camera* cam, const xfh_grid_bounds* bounds, const float* xyz, int n, float radius,
                       float* uvr, float* ur, uint8_t* status) {
    if (!Tcw || !cam || !bounds || n < 0 || (n > 0 && (!xyz || !uvr || !ur || !status))) return XFH_ERR_INVALID_ARG;
    for (int i = 0; i < n; ++i) {
        status[i] = (uint8_t)xfh_project_point(Tcw, *cam, *bounds, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], &uvr[3 * i], &uvr[3 * i + 1], &ur[i]);
        uvr[3 * i + 2] = radius;
    }
    return XFH_OK;
}

size_t xfh_search_projection_workspace_bytes(int nq, int nt, int B) {
    if (nq < 0 || nt < 0 || B < 0) return 0;
    return proj_ws_layout(nq, nt).bytes * (size_t)B;
}

// the checks the two search calls share (everything that does not depend on where the pointers live)
static bool proj_args_ok(int mode, int nq, int nt, const float* ur_query, const float* Tcw, const xfh_camera* cam, const xfh_grid_bounds* bounds,
                         float radius, const float* uright, float nn_ratio) {
    if (nq < 1 || nq > XFH_GRID_MAX_N || nt < 1 || nt > XFH_GRID_MAX_N) return false;
    if (mode != XFH_PROJ_POINTS && mode != XFH_PROJ_GIVEN) return false;
    if (mode == XFH_PROJ_GIVEN && (ur_query != nullptr) != (uright != nullptr)) return false;
    if (mode == XFH_PROJ_POINTS && (!Tcw || !cam || !bounds)) return false;
    return isfinite(radius) && isfinite(nn_ratio) && nn_ratio >= 0.0f;
}

int xfh_search_projection_device(xfh_ctx* c, int mode, int B, int nq, const float* d_pts, const float* d_ur_query, const float* d_Tcw,
                                 const xfh_camera* cam, const xfh_grid_bounds* bounds, float radius, const float* d_qdesc, const uint8_t* d_qflags,
                                 const void* d_grids, const float* d_targets, size_t target_stride, int nt, const uint8_t* d_skip, const float* d_uright,
                                 int init_dist, int th_high, float nn_ratio, void* d_ws, uint8_t* d_status, int* d_match_idx, int* d_best_dist,
                                 int* d_second_dist, int* d_n_candidates, float* d_proj_out, int* d_assigned, int* d_n_matches) {
    if (!c || B < 1 || !proj_args_ok(mode, nq, nt, d_ur_query, d_Tcw, cam, bounds, radius, d_uright, nn_ratio)) return XFH_ERR_INVALID_ARG;
    if (!d_pts || !d_qdesc || !d_qflags || !d_grids || !d_targets || !d_ws || !d_status || !d_match_idx || !d_best_dist || !d_second_dist ||
        !d_n_candidates || !d_assigned || !d_n_matches) return XFH_ERR_INVALID_ARG;
    if (misaligned(15, d_qdesc, d_targets, d_grids, d_ws, target_stride) ||
        misaligned(3, d_pts, d_ur_query, d_Tcw, d_uright, d_match_idx, d_best_dist, d_second_dist, d_n_candidates, d_proj_out, d_assigned, d_n_matches))
        return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    ProjArgs a = {};
    a.mode = mode; a.nq = nq; a.nt = nt; a.radius = radius;
    a.pts = d_pts; a.ur_query = mode == XFH_PROJ_GIVEN ? d_ur_query : nullptr; a.Tcw = d_Tcw;
    if (cam) a.cam = *cam;
    if (bounds) a.bounds = *bounds;
    a.qdesc = d_qdesc; a.qflags = d_qflags; a.grids = (const char*)d_grids; a.grid_stride = xfh_grid_bytes(nt);
    a.targets = (const char*)d_targets; a.target_stride = target_stride; a.skip = d_skip; a.uright = d_uright;
    a.init_dist = init_dist; a.th_high = th_high; a.nn_ratio = nn_ratio;
    a.ws = (char*)d_ws; a.ws_stride = proj_ws_layout(nq, nt).bytes;
    a.status = d_status; a.match_idx = d_match_idx; a.best_dist = d_best_dist; a.second_dist = d_second_dist; a.n_candidates = d_n_candidates;
    a.proj_out = d_proj_out; a.assigned = d_assigned; a.n_matches = d_n_matches;
    HIPCK(c, launch_search_projection(c, a, B));
    return XFH_OK;
}

int xfh_search_projection(xfh_ctx* c, int mode, int nq, const float* pts, const float* ur_query, const float* Tcw, const xfh_camera* cam,
                          const xfh_grid_bounds* bounds, float radius, const float* qdesc, const uint8_t* qflags, const xfh_keypoint* kps,
                          const float* targets, int nt, const uint8_t* skip, const float* uright, int init_dist, int th_high, float nn_ratio,
                          uint8_t* status, int* match_idx, int* best_dist, int* second_dist, int* n_candidates, float* proj_out, int* assigned, int* n_matches) {
    GridGeom g;
    if (!c || !grid_geom(bounds, &g) || !proj_args_ok(mode, nq, nt, ur_query, Tcw, cam, bounds, radius, uright, nn_ratio)) return XFH_ERR_INVALID_ARG;
    if (!pts || !qdesc || !qflags || !kps || !targets || !status || !match_idx || !best_dist || !second_dist || !n_candidates || !assigned || !n_matches)
        return XFH_ERR_INVALID_ARG;
    HostStage s{c};
    auto dq = s.in<float>(qdesc, (size_t)nq * 256), dp = s.in<float>(pts, (size_t)nq * 12);
    auto dfl = s.in<uint8_t>(qflags, (size_t)nq);
    auto dt = s.in<float>(targets, (size_t)nt * 256);
    auto dk = s.in<xfh_keypoint>(kps, (size_t)nt * sizeof(xfh_keypoint));
    auto dT = s.in_opt<float>(Tcw, 48), duq = s.in_opt<float>(ur_query, (size_t)nq * 4), dur = s.in_opt<float>(uright, (size_t)nt * 4);
    auto dsk = s.in_opt<uint8_t>(skip, (size_t)nt);
    auto dg = s.tmp<char>(xfh_grid_bytes(nt)), dws = s.tmp<char>(proj_ws_layout(nq, nt).bytes);
    int* const out[4] = {match_idx, best_dist, second_dist, n_candidates};
    HostStage::Dev<int> o[4];
    for (int k = 0; k < 4; ++k) o[k] = s.out<int>(out[k], (size_t)nq * 4);
    auto dst = s.out<uint8_t>(status, (size_t)nq);
    auto dpo = s.out_opt<float>(proj_out, (size_t)nq * 12);
    auto das = s.out<int>(assigned, (size_t)nt * 4), dnm = s.out<int>(n_matches, 4);
    if (const int rc = s.upload(); rc != XFH_OK) return rc;
    HIPCK(c, launch_grid_build(c, dk, 0, nullptr, 0, dg, 0, nt, 1, g, 0));
    const int rc = xfh_search_projection_device(c, mode, 1, nq, dp, duq, dT, cam, bounds, radius, dq, dfl, dg, dt, 0, nt, dsk, dur, init_dist, th_high, nn_ratio,
                                                dws, dst, o[0], o[1], o[2], o[3], dpo, das, dnm);
    if (rc != XFH_OK) return rc;                                              // that entry's checks apply here too
    return s.download();
}

int xfh_distinctive_csr_device(xfh_ctx* c, const float* table, int n_rows, const int* offsets, const int* indices, int n_groups,
                               int max_group, int* best_pos, int* best_median) {
    if (!c || n_rows < 0 || n_groups < 0 || max_group < 0 || max_group > XFH_MAX_GROUP) return XFH_ERR_INVALID_ARG;
    if (n_groups == 0) return XFH_OK;
    if (!offsets || !best_pos || !best_median || (max_group > 0 && (!table || !indices))) return XFH_ERR_INVALID_ARG;
    if (misaligned(15, table)) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, launch_distinctive(c, table, offsets, indices, n_groups, max_group, best_pos, best_median));
    return XFH_OK;
}

int xfh_distinctive_csr(xfh_ctx* c, const float* table, int n_rows, const int* offsets, const int* indices, int n_groups,
                        int* best_pos, int* best_median) {
    if (!c || n_rows < 0 || n_groups < 0) return XFH_ERR_INVALID_ARG;
    if (n_groups == 0) return XFH_OK;
    if (!offsets || !best_pos || !best_median) return XFH_ERR_INVALID_ARG;
    int max_group = 0;
    if (!csr_ok(offsets, n_groups, indices, table, n_rows, &max_group) || max_group > XFH_MAX_GROUP) return XFH_ERR_INVALID_ARG;
    HostStage s{c};
    auto dt = s.in<float>(table, (size_t)n_rows * 256);
    auto doff = s.in<int>(offsets, (size_t)(n_groups + 1) * 4), dind = s.in<int>(indices, (size_t)offsets[n_groups] * 4);
    auto o0 = s.out<int>(best_pos, (size_t)n_groups * 4), o1 = s.out<int>(best_median, (size_t)n_groups * 4);
    if (const int rc = s.upload(); rc != XFH_OK) return rc;
    HIPCK(c, launch_distinctive(c, dt, doff, dind, n_groups, max_group, o0, o1));
    return s.download();
}

}  // extern "C"
