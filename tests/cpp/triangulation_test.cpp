// triangulation_test.cpp -- XFmatcher::searchForTriangulation (include/xfeat/ORBmatcher_xfeat.h), host and device forms, against the C ABI
// (xfh_triangulation_search) on one scene: three dumps that must be identical.
// usage: triangulation_test in.bin out.bin
// in.bin : int32 n1, n2, flags (bit0 bOnlyStereo, bit1 bCoarse), 0; xfh_camera (64 B, k1 = 0); float F12[9], ep[2]; then for KF1 and for KF2:
//          keypoints[n * 28 B]; descriptors[n * 64 f32]; uright[n f32]; has[n u8]; node_of[n u32]; depth image f32 [height][width]
// out.bin: three times (C ABI, host form, device form): int32 nmatches, npairs, pairs[npairs][2], status[n1] (widened), match12[n1], best_dist[n1],
//          n_candidates[n1], n_geom[n1]
#define XFEAT_NO_OPENCV 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "xfeat/XFextractor.h"
#include "xfeat/ORBmatcher_xfeat.h"

using namespace ORB_SLAM3;

template <class T> static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

struct KF {
    int n = 0;
    std::vector<XFgrid::KeyPoint> keys;
    XFmatcher::Mat desc;
    std::vector<float> xy, uright, depth;
    std::vector<unsigned char> has;
    std::vector<uint32_t> node_of;
    bool read(FILE* f, int count, const xfh_camera& cam) {
        n = count; keys.resize(n); desc = XFmatcher::Mat(n, 64, 4); uright.resize(n); has.resize(n); node_of.resize(n); depth.resize((size_t)cam.width * cam.height);
        if (!rd(f, keys.data(), n) || !rd(f, desc.ptr<float>(0), (size_t)n * 64) || !rd(f, uright.data(), n) || !rd(f, has.data(), n) || !rd(f, node_of.data(), n) ||
            !rd(f, depth.data(), depth.size())) return false;
        xy.resize(2 * (size_t)n);
        for (int i = 0; i < n; ++i) { xy[2 * i] = keys[i].pt.x; xy[2 * i + 1] = keys[i].pt.y; }
        return true;
    }
};

static void dump(FILE* o, int nmatches, const std::vector<std::pair<size_t, size_t>>& pairs, const std::vector<unsigned char>& status, const std::vector<int>& m,
                 const std::vector<int>& best, const std::vector<int>& nc, const std::vector<int>& ng) {
    const int np = (int)pairs.size();
    fwrite(&nmatches, 4, 1, o); fwrite(&np, 4, 1, o);
    for (const auto& pr : pairs) { const int v[2] = {(int)pr.first, (int)pr.second}; fwrite(v, 4, 2, o); }
    for (unsigned char s : status) { const int v = s; fwrite(&v, 4, 1, o); }
    fwrite(m.data(), 4, m.size(), o); fwrite(best.data(), 4, best.size(), o); fwrite(nc.data(), 4, nc.size(), o); fwrite(ng.data(), 4, ng.size(), o);
}

// the keyframe as the RGB-D pipeline leaves it in device memory: a record (keypoints + descriptor block) finished by XFgrid::buildFromRecord,
// the node blob and the has-a-map-point bytes
struct DeviceKF {
    xfh_ctx* ctx = nullptr; void *rec = nullptr, *nodes = nullptr, *has = nullptr;
    XFgrid* grid = nullptr;
    bool make(const KF& k, const xfh_camera& cam, const xfh_grid_bounds& b) {
        xfh_config cfg; xfh_config_default(&cfg);
        cfg.nfeatures = k.n; cfg.max_height = 32; cfg.max_width = 32;
        if (xfh_create(&cfg, &ctx) != XFH_OK) return false;
        std::vector<unsigned char> r(xfh_record_bytes(k.n), 0);
        int* rh = (int*)r.data(); rh[0] = k.n; rh[1] = k.n;
        memcpy(r.data() + xfh_record_kps_offset(), k.keys.data(), (size_t)k.n * 28);
        memcpy(r.data() + xfh_record_desc_offset(k.n), k.desc.ptr<float>(0), (size_t)k.n * 256);
        std::vector<unsigned char> blob(xfh_nodes_bytes(k.n));
        if (xfh_nodes_pack(k.node_of.data(), k.n, blob.data(), nullptr) != XFH_OK) return false;
        if (xfh_dev_alloc(&rec, r.size()) || xfh_dev_alloc(&nodes, blob.size()) || xfh_dev_alloc(&has, (size_t)k.n + 16)) return false;
        if (xfh_memcpy_h2d(rec, r.data(), r.size()) || xfh_memcpy_h2d(nodes, blob.data(), blob.size()) || xfh_memcpy_h2d(has, k.has.data(), (size_t)k.n)) return false;
        grid = new XFgrid(ctx);
        grid->buildFromRecord(rec, k.n, cam, b, k.depth.data(), XFH_DEPTH_F32, (size_t)cam.width * 4, 1.0f);
        const std::vector<float>& ur = grid->uRight();                           // (waits for the build: the search runs on another ctx' stream)
        return ur == k.uright && grid->keysUn() == k.xy;
    }
    const float* desc(int n) const { return (const float*)((const char*)rec + xfh_record_desc_offset(n)); }
    void free() { delete grid; xfh_dev_free(rec); xfh_dev_free(nodes); xfh_dev_free(has); xfh_destroy(ctx); }
};

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    int hdr[4]; xfh_camera cam; float F12[9], ep[2];
    if (!f || !rd(f, hdr, 4) || !rd(f, &cam, 1) || !rd(f, F12, 9) || !rd(f, ep, 2)) return 2;
    const int n1 = hdr[0], n2 = hdr[1];
    const bool only_stereo = hdr[2] & 1, coarse = hdr[2] & 2;
    KF k1, k2;
    if (!k1.read(f, n1, cam) || !k2.read(f, n2, cam)) return 2;
    fclose(f);
    try {
        xfh_grid_bounds b;
        if (xfh_camera_bounds(&cam, &b) != XFH_OK) return 4;
        DeviceKF d1, d2;
        if (!d1.make(k1, cam, b) || !d2.make(k2, cam, b)) { fprintf(stderr, "device keyframes differ from the host's\n"); return 4; }
        xfh_ctx* ctx = d2.ctx;
        FILE* o = fopen(argv[2], "wb");
        std::vector<std::pair<size_t, size_t>> pairs;
        // the C ABI, host pointers
        std::vector<unsigned char> status(n1);
        std::vector<int> m(n1), best(n1), nc(n1), ng(n1);
        int nm = -1;
        if (xfh_triangulation_search(ctx, n1, n2, hdr[2], XFmatcher::TH_LOW, 100.0f, 1.0f, k1.node_of.data(), k1.xy.data(), k1.uright.data(), k1.has.data(),
                                     k1.desc.ptr<float>(0), k2.node_of.data(), k2.xy.data(), k2.uright.data(), k2.has.data(), k2.desc.ptr<float>(0), F12, ep,
                                     status.data(), m.data(), best.data(), nc.data(), ng.data(), &nm) != XFH_OK) return 4;
        for (int i = 0; i < n1; ++i) if (m[i] >= 0) pairs.push_back(std::make_pair((size_t)i, (size_t)m[i]));
        dump(o, nm, pairs, status, m, best, nc, ng);
        // the wrapper, host vectors
        XFmatcher matcher(ctx, 0.6f, false);
        pairs.assign(3, std::make_pair((size_t)9, (size_t)9));                   // (stale content must go)
        const int na = matcher.searchForTriangulation(k1.desc, k1.xy, &k1.uright, k1.has, k1.node_of, k2.desc, k2.xy, &k2.uright, k2.has, k2.node_of, F12, ep, pairs,
                                                      only_stereo, coarse);
        dump(o, na, pairs, matcher.lastTriangulationStatus(), matcher.lastTriangulationMatches(), matcher.lastTriangulationBestDist(),
             matcher.lastTriangulationCandidates(), matcher.lastTriangulationGeom());
        // the wrapper, device-resident keyframes
        pairs.assign(1, std::make_pair((size_t)7, (size_t)7));
        const int nb = matcher.searchForTriangulation(*d1.grid, d1.desc(n1), d1.nodes, (const unsigned char*)d1.has, *d2.grid, d2.desc(n2), d2.nodes,
                                                      (const unsigned char*)d2.has, F12, ep, pairs, only_stereo, coarse);
        dump(o, nb, pairs, matcher.lastTriangulationStatus(), matcher.lastTriangulationMatches(), matcher.lastTriangulationBestDist(),
             matcher.lastTriangulationCandidates(), matcher.lastTriangulationGeom());
        fclose(o);
        d1.free(); d2.free();
    } catch (const std::exception& e) { fprintf(stderr, "%s\n", e.what()); return 5; }
    return 0;
}
