// essential_graph_test.cpp -- ORB_SLAM3::XFoptimizer::OptimizeEssentialGraph (include/xfeat/Optimizer_xfeat.h) on a scene the Python side writes out.
// usage: essential_graph_test in.bin out.bin
// in.bin : int32 nV, nE, nP, nS, pose_rows, point_rows, fix_scale, iterations; float pose_table[pose_rows][12], point_table[point_rows][3]; int32 kf_row[nV];
//          uint8 kf_fixed[nV]; int32 corrected_index[nV], noncorrected_index[nV]; double sim3[nS][8]; int32 edge_i[nE], edge_j[nE], edge_kind[nE],
//          point_row[nP], point_ref[nP]
// out.bin: int32 status; double sim3[nV][8]; float Tcw[nV][12], points[nP][3], chi2[nE]; int32 header[9]; double final_chi2; then both tables as the call
//          left them (write_back); then the same again from a second call on the same object, on fresh tables (it reuses its buffer)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "xfeat/Optimizer_xfeat.h"

template <class T> static bool rd(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }
template <class T> static T* up(const std::vector<T>& v) {
    void* d = nullptr;
    if (xfh_dev_alloc(&d, v.size() * sizeof(T) + 16) != XFH_OK || xfh_memcpy_h2d(d, v.data(), v.size() * sizeof(T)) != XFH_OK) exit(3);
    return (T*)d;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    std::vector<int> h;
    if (!f || !rd(f, h, 8)) return 2;
    const int nV = h[0], nE = h[1], nP = h[2], nS = h[3];
    std::vector<float> poses, points;
    ORB_SLAM3::XFoptimizer::EssentialGraphInput in;
    if (!rd(f, poses, (size_t)h[4] * 12) || !rd(f, points, (size_t)h[5] * 3) || !rd(f, in.kfRow, nV) || !rd(f, in.kfFixed, nV) || !rd(f, in.correctedIndex, nV) ||
        !rd(f, in.nonCorrectedIndex, nV) || !rd(f, in.sim3, (size_t)nS * 8) || !rd(f, in.edgeI, nE) || !rd(f, in.edgeJ, nE) || !rd(f, in.edgeKind, nE) ||
        !rd(f, in.pointRow, nP) || !rd(f, in.pointRef, nP)) return 2;
    fclose(f);
    try {
        xfh_config cfg; xfh_config_default(&cfg);
        cfg.nfeatures = 1; cfg.max_height = 32; cfg.max_width = 32;
        xfh_ctx* ctx = nullptr;
        if (xfh_create(&cfg, &ctx) != XFH_OK) return 4;
        FILE* o = fopen(argv[2], "wb");
        {
            ORB_SLAM3::XFoptimizer opt(ctx);
            for (int rep = 0; rep < 2; ++rep) {
                in.d_poseTable = up(poses); in.poseRows = h[4]; in.d_pointTable = up(points); in.pointRows = h[5];
                const int status = opt.OptimizeEssentialGraph(in, h[6] != 0, true, h[7]);
                std::vector<double> S; std::vector<float> T, X, c2;
                opt.egSim3(S); opt.egPoses(T); opt.egMapPoints(X); opt.egEdgeChi2(c2);
                if (!opt.deviceEgTcw() || !opt.deviceEgPoints() || status != opt.egHeader[0] || opt.deviceTcw()) return 6;   // LocalBundleAdjustment's getters are not touched
                std::vector<float> tp(poses.size()), tx(points.size());
                if (xfh_memcpy_d2h(tp.data(), in.d_poseTable, tp.size() * 4) != XFH_OK || xfh_memcpy_d2h(tx.data(), in.d_pointTable, tx.size() * 4) != XFH_OK) return 5;
                fwrite(&status, 4, 1, o); fwrite(S.data(), 8, S.size(), o); fwrite(T.data(), 4, T.size(), o); fwrite(X.data(), 4, X.size(), o); fwrite(c2.data(), 4, c2.size(), o);
                fwrite(opt.egHeader, 4, XFH_EG_HEADER_INTS, o); fwrite(&opt.egFinalChi2, 8, 1, o); fwrite(tp.data(), 4, tp.size(), o); fwrite(tx.data(), 4, tx.size(), o);
                xfh_dev_free(in.d_poseTable); xfh_dev_free(in.d_pointTable);
            }
            bool threw = false;                                            // what does not fit is refused: more free keyframes than XFH_EG_MAX_FREE
            ORB_SLAM3::XFoptimizer::EssentialGraphInput big = in;
            big.kfRow.assign(XFH_EG_MAX_FREE + 2, 0); big.kfFixed.assign(XFH_EG_MAX_FREE + 2, 0); big.kfFixed[0] = 1;
            big.correctedIndex.assign(XFH_EG_MAX_FREE + 2, -1); big.nonCorrectedIndex.assign(XFH_EG_MAX_FREE + 2, -1);
            big.d_poseTable = up(poses); big.d_pointTable = up(points);
            try { opt.OptimizeEssentialGraph(big, false); } catch (const std::exception&) { threw = true; }
            if (!threw) return 7;
        }
        fclose(o);
        xfh_destroy(ctx);
    } catch (const std::exception& e) { fprintf(stderr, "%s\n", e.what()); return 5; }
    return 0;
}
