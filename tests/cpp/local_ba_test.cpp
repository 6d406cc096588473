// local_ba_test.cpp -- ORB_SLAM3::XFoptimizer::LocalBundleAdjustment (include/xfeat/Optimizer_xfeat.h) on a scene the Python side writes out.
// usage: local_ba_test in.bin out.bin
// in.bin : int32 nK, nP, nE, pose_rows, point_rows, iterations; float cam[5] (fx fy cx cy bf), inv_sigma2; float pose_table[pose_rows][12],
//          point_table[point_rows][3]; int32 kf_row[nK]; uint8 kf_fixed[nK]; int32 point_row[nP], edge_begin[nP + 1], edge_kf[nE]; float edge_obs[nE][3]
// out.bin: int32 status; float Tcw[nK][12], points[nP][3]; uint8 erase[nE]; float chi2[nE]; int32 header[10]; double final_chi2; then both tables as the
//          call left them (write_back); then the same again from a second call on the same object, on fresh tables (it reuses its buffer)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "xfeat/Optimizer_xfeat.h"

template <class T> static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T> static T* up(const std::vector<T>& v) {
    void* d = nullptr;
    if (xfh_dev_alloc(&d, v.size() * sizeof(T) + 16) != XFH_OK || xfh_memcpy_h2d(d, v.data(), v.size() * sizeof(T)) != XFH_OK) exit(3);
    return (T*)d;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    int h[6]; float cf[6];
    if (!f || !rd(f, h, 6) || !rd(f, cf, 6)) return 2;
    const int nK = h[0], nP = h[1], nE = h[2];
    std::vector<float> poses((size_t)h[3] * 12), points((size_t)h[4] * 3);
    ORB_SLAM3::XFoptimizer::LocalBAInput in;
    in.kfRow.resize(nK); in.kfFixed.resize(nK); in.pointRow.resize(nP); in.edgeBegin.resize(nP + 1); in.edgeKF.resize(nE); in.edgeObs.resize((size_t)nE * 3);
    if (!rd(f, poses.data(), poses.size()) || !rd(f, points.data(), points.size()) || !rd(f, in.kfRow.data(), in.kfRow.size()) || !rd(f, in.kfFixed.data(), in.kfFixed.size()) ||
        !rd(f, in.pointRow.data(), in.pointRow.size()) || !rd(f, in.edgeBegin.data(), in.edgeBegin.size()) || !rd(f, in.edgeKF.data(), in.edgeKF.size()) ||
        !rd(f, in.edgeObs.data(), in.edgeObs.size())) return 2;
    fclose(f);
    try {
        xfh_config cfg; xfh_config_default(&cfg);
        cfg.nfeatures = 1; cfg.max_height = 32; cfg.max_width = 32;
        xfh_ctx* ctx = nullptr;
        if (xfh_create(&cfg, &ctx) != XFH_OK) return 4;
        xfh_camera cam; memset(&cam, 0, sizeof cam);
        cam.fx = cf[0]; cam.fy = cf[1]; cam.cx = cf[2]; cam.cy = cf[3]; cam.bf = cf[4]; cam.width = 640; cam.height = 480;
        FILE* o = fopen(argv[2], "wb");
        {
            ORB_SLAM3::XFoptimizer opt(ctx);
            for (int rep = 0; rep < 2; ++rep) {
                in.d_poseTable = up(poses); in.poseRows = h[3]; in.d_pointTable = up(points); in.pointRows = h[4];
                const int status = opt.LocalBundleAdjustment(in, cam, cf[5], h[5], true);
                std::vector<float> T, X, c2; std::vector<unsigned char> er;
                opt.localPoses(T); opt.localPoints(X); opt.eraseFlags(er); opt.edgeChi2(c2);
                if (!opt.deviceTcw() || !opt.devicePoints() || !opt.deviceErase() || status != opt.lbaHeader[0]) return 6;
                std::vector<float> tp(poses.size()), tx(points.size());
                if (xfh_memcpy_d2h(tp.data(), in.d_poseTable, tp.size() * 4) != XFH_OK || xfh_memcpy_d2h(tx.data(), in.d_pointTable, tx.size() * 4) != XFH_OK) return 5;
                fwrite(&status, 4, 1, o); fwrite(T.data(), 4, T.size(), o); fwrite(X.data(), 4, X.size(), o); fwrite(er.data(), 1, er.size(), o); fwrite(c2.data(), 4, c2.size(), o);
                fwrite(opt.lbaHeader, 4, XFH_LBA_HEADER_INTS, o); fwrite(&opt.lbaFinalChi2, 8, 1, o); fwrite(tp.data(), 4, tp.size(), o); fwrite(tx.data(), 4, tx.size(), o);
                xfh_dev_free(in.d_poseTable); xfh_dev_free(in.d_pointTable);
            }
            bool threw = false;                                            // what does not fit is refused: more free keyframes than XFH_LBA_MAX_FREE
            ORB_SLAM3::XFoptimizer::LocalBAInput big = in;
            big.kfRow.assign(XFH_LBA_MAX_FREE + 2, 0); big.kfFixed.assign(XFH_LBA_MAX_FREE + 2, 0); big.kfFixed[0] = 1;
            big.d_poseTable = up(poses); big.d_pointTable = up(points);
            try { opt.LocalBundleAdjustment(big, cam); } catch (const std::exception&) { threw = true; }
            if (!threw) return 7;
        }
        fclose(o);
        xfh_destroy(ctx);
    } catch (const std::exception& e) { fprintf(stderr, "%s\n", e.what()); return 5; }
    return 0;
}
