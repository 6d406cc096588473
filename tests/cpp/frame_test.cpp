// frame_test.cpp -- XFgrid::buildFromRecord(record, n, camera, bounds, depth) (include/xfeat/ORBmatcher_xfeat.h) the way the RGB-D
// Frame constructor and SearchByProjection(Frame, Frame) would use it: finish a record that is in device memory, read mvKeysUn /
// mvuRight / mvDepth back, ask featuresInArea on the undistorted grid, and hand the object's uright to searchWindow.
// usage: frame_test in.bin out.bin
// in.bin : int32 nq, nt, init, depth_type (0 none, 1 f32, 2 u16); xfh_camera (64 B); float depth_scale; keypoints[nt * 28 B];
//          targets[nt * 64 f32]; queries[nq * 64 f32]; uvr[nq * 3 f32]; ur_query[nq f32]; depth image [height][width] of the type
// out.bin: float bounds[4]; xy_un[nt * 2]; uright[nt]; depth[nt]; 5 x int32[nq] of searchWindow with the object's uright; per query
//          int32 count + int32 indices of featuresInArea; then uright[nt], depth[nt] of a second build WITHOUT a depth image on the
//          same object (all -1)
#define XFEAT_NO_OPENCV 1
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "xfeat/XFextractor.h"
#include "xfeat/ORBmatcher_xfeat.h"

using namespace ORB_SLAM3;

template <class T> static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    int hdr[4]; xfh_camera cam; float scale = 1.f;
    if (!f || !rd(f, hdr, 4) || !rd(f, &cam, 1) || !rd(f, &scale, 1)) return 2;
    const int nq = hdr[0], nt = hdr[1], init = hdr[2], dtype = hdr[3];
    std::vector<XFgrid::KeyPoint> keys(nt);
    XFmatcher::Mat tg(nt, 64, 4), q(nq, 64, 4);
    std::vector<float> uvr(3 * (size_t)nq), urq(nq);
    const size_t es = dtype == XFH_DEPTH_F32 ? 4 : 2, pitch = (size_t)cam.width * es;
    std::vector<unsigned char> img(dtype ? pitch * cam.height : 0);
    if (!rd(f, keys.data(), nt) || !rd(f, tg.ptr<float>(0), (size_t)nt * 64) || !rd(f, q.ptr<float>(0), (size_t)nq * 64) || !rd(f, uvr.data(), uvr.size()) ||
        !rd(f, urq.data(), nq) || !rd(f, img.data(), img.size())) return 2;
    fclose(f);
    xfh_config cfg; xfh_config_default(&cfg);
    cfg.nfeatures = nt; cfg.max_height = 32; cfg.max_width = 32;
    xfh_ctx* ctx = nullptr;
    if (xfh_create(&cfg, &ctx) != XFH_OK) return 3;
    try {
        // a record holding the keypoints, in device memory: header n_valid = nt, mono_index = nt
        std::vector<unsigned char> rec(xfh_record_bytes(nt), 0);
        int* rh = (int*)rec.data(); rh[0] = nt; rh[1] = nt;
        memcpy(rec.data() + xfh_record_kps_offset(), keys.data(), (size_t)nt * 28);
        void* d_rec = nullptr;
        if (xfh_dev_alloc(&d_rec, rec.size()) != XFH_OK || xfh_memcpy_h2d(d_rec, rec.data(), rec.size()) != XFH_OK) return 4;
        xfh_grid_bounds b;
        if (xfh_camera_bounds(&cam, &b) != XFH_OK) return 4;                       // ComputeImageBounds, once per calibration
        XFgrid grid(ctx);
        grid.buildFromRecord(d_rec, nt, cam, b, dtype ? img.data() : nullptr, dtype, pitch, scale);
        FILE* o = fopen(argv[2], "wb");
        fwrite(&b, sizeof b, 1, o);
        const std::vector<float> xy = grid.keysUn(), ur = grid.uRight(), dz = grid.depth();
        fwrite(xy.data(), 4, xy.size(), o); fwrite(ur.data(), 4, ur.size(), o); fwrite(dz.data(), 4, dz.size(), o);
        XFmatcher matcher(ctx);
        std::vector<int> r[5];
        matcher.searchWindow(q, uvr, grid, tg, r[0], r[1], r[2], r[3], r[4], init, nullptr, &ur, &urq);
        for (auto& v : r) fwrite(v.data(), 4, v.size(), o);
        for (int i = 0; i < nq; ++i) {
            const std::vector<size_t> v = grid.featuresInArea(uvr[3 * i], uvr[3 * i + 1], uvr[3 * i + 2]);
            const int cnt = (int)v.size();
            fwrite(&cnt, 4, 1, o);
            for (size_t k : v) { const int x = (int)k; fwrite(&x, 4, 1, o); }
        }
        grid.buildFromRecord(d_rec, nt, cam, b);                                   // the monocular constructor on the same object
        fwrite(grid.uRight().data(), 4, nt, o); fwrite(grid.depth().data(), 4, nt, o);
        // a grid built without a camera has no side arrays
        grid.buildFromRecord(d_rec, nt, b);
        bool threw = false;
        try { grid.keysUn(); } catch (const std::exception&) { threw = true; }
        fclose(o);
        xfh_dev_free(d_rec);
        if (!threw) { fprintf(stderr, "keysUn() of a grid without a camera did not throw\n"); return 6; }
    } catch (const std::exception& e) { fprintf(stderr, "%s\n", e.what()); return 5; }
    xfh_destroy(ctx);
    return 0;
}
