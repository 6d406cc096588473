/*
 * Optimizer_xfeat.h -- the motion-only pose refinement of ORB_SLAM3::Optimizer on a frame whose arrays are in device memory.
 *
 * ORB_SLAM3::XFoptimizer::PoseOptimization is Optimizer::PoseOptimization(Frame*) (reference src/Optimizer.cc:814-1114, the conventional
 * camera with a Pinhole model) as one call of xfh_pose_optimize_device: the frame's undistorted keypoints and right coordinates as
 * xfh_frame_finish_records_device (or XFgrid::buildFromRecord) left them, the assignment a search wrote (assigned[k] = index of the map point
 * of keypoint k, or anything outside [0, nq) for none), the world points the search projected, and the pose.  It returns the reference's int
 * (nInitialCorrespondences - nBad) and leaves the new pose and the mvbOutlier flags in device memory, where the next search reads them; the
 * pose also comes back to the host, as pFrame->SetPose would want it.  This is not a graph optimiser: one SE3 vertex, unary edges, nothing else
 * (include/xfeat_hip.h has the contract line by line).  XFoptimizer::OptimizeSim3 is Optimizer::OptimizeSim3 (:2100-2381) in the same way: one
 * Sim3 vertex, two projection edges per correspondence, as one call of xfh_sim3_optimize_device between the two Sim3 projection searches of loop
 * detection.  XFoptimizer::LocalBundleAdjustment is Optimizer::LocalBundleAdjustment (:1188-1460, the graph, optimize(10) and vToErase) as one call of
 * xfh_local_ba_device on the map's device tables.  XFoptimizer::OptimizeEssentialGraph is Optimizer::OptimizeEssentialGraph (:1532-1779, the Sim3 pose graph
 * of loop closing, optimize(20), the recovered poses and the corrected points) as one call of xfh_essential_graph_device on the same tables.  Header only;
 * needs nothing but xfeat_hip.h.
 */
#ifndef XFEAT_OPTIMIZER_XFEAT_H
#define XFEAT_OPTIMIZER_XFEAT_H

#include "../xfeat_hip.h"

#include <stdexcept>
#include <string>
#include <vector>

namespace ORB_SLAM3 {

class XFoptimizer {
public:
    explicit XFoptimizer(xfh_ctx* c) : ctx(c) {}
    ~XFoptimizer() { if (d_buf) xfh_dev_free(d_buf); if (d_s3) xfh_dev_free(d_s3); if (d_lba) xfh_dev_free(d_lba); if (d_eg) xfh_dev_free(d_eg); }
    XFoptimizer(const XFoptimizer&) = delete;
    XFoptimizer& operator=(const XFoptimizer&) = delete;

    // Tcw: the frame's pose, row-major 3x4 [R|t]; replaced by the optimised pose.  d_keysUn [nt][2], d_uRight [nt] (nullptr: a monocular frame),
    // d_assigned [nt], d_points [nq][3]: device memory.  invSigma2 = mvInvLevelSigma2[0] (every XFeat keypoint has octave 0).  Blocks until the
    // pose and the counts are on the host; the flags stay on the device (deviceOutliers()) and are copied only when asked for (outliers()).
    int PoseOptimization(float Tcw[12], const xfh_camera& cam, int nt, const float* d_keysUn, const float* d_uRight, const int* d_assigned, int nq,
                         const float* d_points, float invSigma2 = 1.0f) {
        const size_t ws = xfh_pose_optimize_workspace_bytes(nt, 1);
        if (ws == 0 || nq < 1) throw std::runtime_error("XFoptimizer::PoseOptimization: sizes out of range");
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t bw = al(ws), bo = al((size_t)nt), bc = al((size_t)nt * 4);
        const size_t need = bw + 256 + bo + bc + 256;
        if (need > bytes) {
            if (d_buf) { xfh_synchronize(ctx); xfh_dev_free(d_buf); d_buf = nullptr; bytes = 0; }
            if (xfh_dev_alloc(&d_buf, need) != XFH_OK) throw std::runtime_error("XFoptimizer::PoseOptimization: out of device memory");
            bytes = need;
        }
        char* p = (char*)d_buf;
        void* dws = p; p += bw;
        d_pose = (float*)p; p += 256;
        d_outlier = (unsigned char*)p; p += bo;
        d_chi2 = (float*)p; p += bc;
        int* dh = (int*)p; double* dfc = (double*)(p + 64);
        n = nt;
        int rc = xfh_synchronize(ctx);                       // (the copy below is synchronous: nothing queued earlier may still read the buffer)
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(d_pose, Tcw, 48);
        if (rc == XFH_OK) rc = xfh_pose_optimize_device(ctx, 1, nt, nq, d_pose, &cam, d_keysUn, d_uRight, d_assigned, d_points, invSigma2, dws, d_pose, d_outlier,
                                                        d_chi2, dh, dfc);
        if (rc == XFH_OK) rc = xfh_synchronize(ctx);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(Tcw, d_pose, 48);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(header, dh, 32);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(&finalChi2, dfc, 8);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFoptimizer::PoseOptimization: ") + xfh_strerror(rc));
        return header[2];
    }

    // of the last call.  The pose and the flags in device memory: what the next xfh_search_projection_device takes as d_Tcw, and mvbOutlier.
    const float* devicePose() const { return d_pose; }
    const unsigned char* deviceOutliers() const { return d_outlier; }
    void outliers(std::vector<unsigned char>& mvbOutlier) const {
        mvbOutlier.assign((size_t)n, 0);
        if (n > 0 && xfh_memcpy_d2h(mvbOutlier.data(), d_outlier, (size_t)n) != XFH_OK) throw std::runtime_error("XFoptimizer::outliers: download failed");
    }
    void chi2(std::vector<float>& out) const {
        out.assign((size_t)n, 0.0f);
        if (n > 0 && xfh_memcpy_d2h(out.data(), d_chi2, (size_t)n * 4) != XFH_OK) throw std::runtime_error("XFoptimizer::chi2: download failed");
    }
    // ---- Optimizer::OptimizeSim3 (reference src/Optimizer.cc:2100-2381) as LoopClosing calls it between its two Sim3 projection searches: one call of
    // xfh_sim3_optimize_device.  The arrays of both keyframes are in device memory as the calls around it leave them (include/xfeat_hip.h, the
    // OptimizeSim3 section, names them one by one); d_Tmw, the pose of pMostBoWMatchesKF, may be nullptr (then no composed pose is written).
    struct Sim3Input {
        int n1, M1, nq, n2;
        const float* d_T1w; const float* d_keysUn1; const int* d_point1; const float* d_points1;
        const int* d_assigned; const float* d_points2; const unsigned char* d_flags2; const int* d_index2; const float* d_keysUn2; const float* d_T2w;
        const float* d_Tmw;
    };
    // S12: g2oS12 as 13 floats (R row-major 9, t 3, s), replaced by the optimised similarity.  Returns the reference's int (nIn, or 0 when fewer
    // than 10 correspondences survive the first classification).  vpMatches1 with its NULLs (deviceMatches()), the composed pose and camera centre
    // for the next search (deviceScw(), deviceOw()) and the similarity (deviceS12()) stay on the device.  Blocks until S12 and the counts are on the host.
    int OptimizeSim3(const Sim3Input& in, float S12[13], const xfh_camera& cam1, const xfh_camera& cam2, float th2, bool bFixScale, bool bAllPoints,
                     float invSigma2_1 = 1.0f, float invSigma2_2 = 1.0f) {
        const size_t ws = xfh_sim3_optimize_workspace_bytes(in.n1, 1);
        if (ws == 0) throw std::runtime_error("XFoptimizer::OptimizeSim3: sizes out of range");
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t N = (size_t)in.n1, bw = al(ws), ba = al(N * 4), bs = al(N), bc = al(N * 8);
        const size_t need = bw + ba + bs + bc + 5 * 256;
        if (need > s3_bytes) {
            if (d_s3) { xfh_synchronize(ctx); xfh_dev_free(d_s3); d_s3 = nullptr; s3_bytes = 0; }
            if (xfh_dev_alloc(&d_s3, need) != XFH_OK) throw std::runtime_error("XFoptimizer::OptimizeSim3: out of device memory");
            s3_bytes = need;
        }
        char* p = (char*)d_s3;
        void* dws = p; p += bw;
        d_matches = (int*)p; p += ba;
        d_status = (unsigned char*)p; p += bs;
        d_chi2_pairs = (float*)p; p += bc;
        d_S12 = (float*)p; p += 256;
        d_Scw = in.d_Tmw ? (float*)p : nullptr; d_Ow = in.d_Tmw ? (float*)(p + 64) : nullptr; p += 256;     // no composed pose without d_Tmw
        double* dst = (double*)p; double* dfc = (double*)(p + 64); p += 256;
        int* dh = (int*)p;
        n_pairs = in.n1;
        int rc = xfh_synchronize(ctx);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(d_S12, S12, XFH_SIM3_OPT_S12_FLOATS * 4);
        if (rc == XFH_OK) rc = xfh_sim3_optimize_device(ctx, 1, in.n1, in.M1, in.nq, in.n2, 0, in.d_T1w, in.d_keysUn1, in.d_point1, in.d_points1, in.d_assigned,
                                                        in.d_points2, in.d_flags2, in.d_index2, in.d_keysUn2, in.d_T2w, d_S12, XFH_SIM3_OPT_S12_FLOATS, in.d_Tmw,
                                                        &cam1, &cam2, th2, bFixScale ? 1 : 0, bAllPoints ? 1 : 0, invSigma2_1, invSigma2_2, dws, d_matches, d_status,
                                                        d_chi2_pairs, dst, d_S12, XFH_SIM3_OPT_S12_FLOATS, d_Scw, d_Ow,
                                                        dh, dfc);
        if (rc == XFH_OK) rc = xfh_synchronize(ctx);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(S12, d_S12, XFH_SIM3_OPT_S12_FLOATS * 4);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(sim3State, dst, 64);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(sim3Header, dh, XFH_SIM3_OPT_HEADER_INTS * 4);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(&sim3FinalChi2, dfc, 8);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFoptimizer::OptimizeSim3: ") + xfh_strerror(rc));
        return sim3Header[6];
    }
    // of the last OptimizeSim3: vpMatches1 (d_assigned with -1 where the match was removed), the composed [R | t / s] and camera centre the fine
    // xfh_map_projection_search_device takes (both nullptr when the call had no d_Tmw: nothing was composed), the similarity; the pair status and the
    // two chi2 per keypoint on request
    const int* deviceMatches() const { return d_matches; }
    const float* deviceScw() const { return d_Scw; }
    const float* deviceOw() const { return d_Ow; }
    const float* deviceS12() const { return d_S12; }
    void matches(std::vector<int>& out) const {
        out.assign((size_t)n_pairs, -1);
        if (n_pairs > 0 && xfh_memcpy_d2h(out.data(), d_matches, (size_t)n_pairs * 4) != XFH_OK) throw std::runtime_error("XFoptimizer::matches: download failed");
    }
    void pairStatus(std::vector<unsigned char>& out) const {
        out.assign((size_t)n_pairs, 0);
        if (n_pairs > 0 && xfh_memcpy_d2h(out.data(), d_status, (size_t)n_pairs) != XFH_OK) throw std::runtime_error("XFoptimizer::pairStatus: download failed");
    }
    void pairChi2(std::vector<float>& out) const {
        out.assign((size_t)n_pairs * 2, 0.0f);
        if (n_pairs > 0 && xfh_memcpy_d2h(out.data(), d_chi2_pairs, (size_t)n_pairs * 8) != XFH_OK) throw std::runtime_error("XFoptimizer::pairChi2: download failed");
    }
    // n_corr, n_in_kf2, n_out_kf2, n_bad, n_bad_out_kf2, n_more, the return value, classifications run, iterations, trials, rejected, failures, zeros
    int sim3Header[XFH_SIM3_OPT_HEADER_INTS] = {};
    double sim3State[8] = {};                                // quaternion (x, y, z, w), t, s of g2oS12 on return
    double sim3FinalChi2 = 0.0;

    // ---- Optimizer::LocalBundleAdjustment (reference src/Optimizer.cc:1116-1498) as LocalMapping::Run calls it: the host keeps :1118-1186 (the three lists)
    // and hands the problem over as indices into the map's two device tables; :1188-1460 is one call of xfh_local_ba_device.  The host-side vectors are
    // copied to the device here (they are small: indices and observations); the tables are refined in place (write_back).
    struct LocalBAInput {
        float* d_poseTable; int poseRows;                       // [poseRows][12] row-major [R|t]
        float* d_pointTable; int pointRows;                     // [pointRows][3]
        std::vector<int> kfRow;                                 // lLocalKeyFrames, then lFixedCameras: the row of each in the pose table
        std::vector<unsigned char> kfFixed;                     // 1 for lFixedCameras and for the initial keyframe (mnId == GetInitKFid())
        std::vector<int> pointRow;                              // lLocalMapPoints: the row of each in the point table
        std::vector<int> edgeBegin;                             // [points + 1]: the edges of point p are edgeBegin[p] .. edgeBegin[p + 1] - 1, in the
        std::vector<int> edgeKF;                                // order of :1296 (observations of !isBad() keyframes of this map with leftIndex != -1);
        std::vector<float> edgeObs;                             // index into kfRow; (kpUn.pt.x, kpUn.pt.y, mvuRight[leftIndex]) per edge
    };
    // Returns the status (XFH_LBA_OK, _ABORTED, _NOTHING_FREE).  Blocks until the header is on the host; the refined poses, points and the vToErase flags
    // stay on the device (deviceTcw(), devicePoints(), deviceErase()) and come to the host on request.  After the call the host re-checks
    // pMP->isBad() (:1422), erases the flagged observations, and calls SetPose / SetWorldPos / UpdateNormalAndDepth with the downloaded values.
    int LocalBundleAdjustment(const LocalBAInput& in, const xfh_camera& cam, float invSigma2 = 1.0f, int iterations = 10, bool writeBack = true) {
        const int nK = (int)in.kfRow.size(), nP = (int)in.pointRow.size(), nE = (int)in.edgeKF.size();
        int nFree = 0;
        for (unsigned char f : in.kfFixed) nFree += f ? 0 : 1;
        const size_t ws = xfh_local_ba_workspace_bytes(nK, nP, nE, nFree);
        if (ws == 0 || in.kfFixed.size() != (size_t)nK || in.edgeBegin.size() != (size_t)nP + 1 || in.edgeObs.size() != (size_t)nE * 3)
            throw std::runtime_error("XFoptimizer::LocalBundleAdjustment: sizes out of range (more than XFH_LBA_MAX_FREE free keyframes?)");
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t K = (size_t)nK, P = (size_t)nP, E = (size_t)nE;
        const size_t sz[] = {al(ws), al(K * 4), al(K), al(P * 4), al((P + 1) * 4), al(E * 4), al(E * 12), al(K * 48), al(P * 12), al(E), al(E * 4), 256, 256};
        size_t need = 0;
        for (size_t v : sz) need += v;
        if (need > lba_bytes) {
            if (d_lba) { xfh_synchronize(ctx); xfh_dev_free(d_lba); d_lba = nullptr; lba_bytes = 0; }
            if (xfh_dev_alloc(&d_lba, need) != XFH_OK) throw std::runtime_error("XFoptimizer::LocalBundleAdjustment: out of device memory");
            lba_bytes = need;
        }
        char* q[13];
        q[0] = (char*)d_lba;
        for (int i = 1; i < 13; ++i) q[i] = q[i - 1] + sz[i - 1];
        d_lbaTcw = (float*)q[7]; d_lbaPoints = (float*)q[8]; d_lbaErase = (unsigned char*)q[9]; d_lbaChi2 = (float*)q[10];
        lbaKF = nK; lbaPoints = nP; lbaEdges = nE;
        int rc = xfh_synchronize(ctx);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(q[1], in.kfRow.data(), K * 4);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(q[2], in.kfFixed.data(), K);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(q[3], in.pointRow.data(), P * 4);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(q[4], in.edgeBegin.data(), (P + 1) * 4);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(q[5], in.edgeKF.data(), E * 4);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(q[6], in.edgeObs.data(), E * 12);
        if (rc == XFH_OK) rc = xfh_local_ba_device(ctx, nK, nFree, nP, nE, in.d_poseTable, in.poseRows, in.d_pointTable, in.pointRows, (const int*)q[1],
                                                   (const unsigned char*)q[2], (const int*)q[3], (const int*)q[4], (const int*)q[5], (const float*)q[6], &cam, invSigma2,
                                                   iterations, writeBack ? 1 : 0, q[0], d_lbaTcw, d_lbaPoints, d_lbaErase, d_lbaChi2, (int*)q[11], (double*)q[12]);
        if (rc == XFH_OK) rc = xfh_synchronize(ctx);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(lbaHeader, q[11], XFH_LBA_HEADER_INTS * 4);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(&lbaFinalChi2, q[12], 8);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFoptimizer::LocalBundleAdjustment: ") + xfh_strerror(rc));
        return lbaHeader[0];
    }
    // of the last LocalBundleAdjustment: the refined poses [keyframes][12] (a fixed keyframe's: its input), points [points][3], the vToErase flag and
    // the chi2 of every edge, in device memory; and copies on request
    const float* deviceTcw() const { return d_lbaTcw; }
    const float* devicePoints() const { return d_lbaPoints; }
    const unsigned char* deviceErase() const { return d_lbaErase; }
    void localPoses(std::vector<float>& out) const { lbaGet(out, d_lbaTcw, (size_t)lbaKF * 12); }
    void localPoints(std::vector<float>& out) const { lbaGet(out, d_lbaPoints, (size_t)lbaPoints * 3); }
    void eraseFlags(std::vector<unsigned char>& out) const { lbaGet(out, d_lbaErase, (size_t)lbaEdges); }
    void edgeChi2(std::vector<float>& out) const { lbaGet(out, d_lbaChi2, (size_t)lbaEdges); }
    // status, free keyframes, fixed keyframes with an edge, mono edges, stereo edges, iterations, trials, rejected trials, factorisation failures, edges to erase
    int lbaHeader[XFH_LBA_HEADER_INTS] = {};
    double lbaFinalChi2 = 0.0;

    // ---- Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:1501-1783) as LoopClosing::CorrectLoop calls it: the host keeps the walk over the map
    // (:1532-1706: which keyframes, which edges pass minFeat / sInsertedEdges / hasChild, nIDr of every point) and hands the problem over as indices into
    // the map's two device tables; the optimisation and the recovery (:1708-1779) are one call of xfh_essential_graph_device.  The host-side vectors are
    // copied to the device here; the tables are corrected in place (write_back).
    struct EssentialGraphInput {
        float* d_poseTable; int poseRows;                       // [poseRows][12] row-major [R|t]
        float* d_pointTable; int pointRows;                     // [pointRows][3]
        std::vector<int> kfRow;                                 // vpKFs without the bad ones: the row of each in the pose table
        std::vector<unsigned char> kfFixed;                     // 1 for mnId == pMap->GetInitKFid()
        std::vector<int> correctedIndex, nonCorrectedIndex;     // per keyframe: its entry of CorrectedSim3 / NonCorrectedSim3 in sim3, or -1
        std::vector<double> sim3;                               // [entries][8]: (qx, qy, qz, qw, tx, ty, tz, s) of a g2o::Sim3
        std::vector<int> edgeI, edgeJ, edgeKind;                // vertex 0, vertex 1 (indices into kfRow) and the kind (0: a loop connection of :1577-1605,
                                                                // 1: a spanning-tree, loop or covisibility edge of :1608-1706) in the reference's creation order
        std::vector<int> pointRow, pointRef;                    // vpMPs without the bad ones: the row of each in the point table and the vertex of nIDr
    };
    // Returns the status (XFH_EG_OK, _NOTHING_FREE, _FREE_MISMATCH, _NO_EDGES).  SYNCHRONOUS, as xfh_essential_graph_device is: when it returns the header is
    // on the host and the corrected poses and points are in device memory (deviceEgTcw(), deviceEgPoints()) and, with writeBack, in the tables.  After the call
    // the host walks vpKFs and vpMPs once: SetPose(egPoses()), SetWorldPos(egMapPoints()) + UpdateNormalAndDepth, then pMap->IncreaseChangeIndex().
    int OptimizeEssentialGraph(const EssentialGraphInput& in, bool bFixScale, bool writeBack = true, int iterations = XFH_EG_MAX_ITERATIONS) {
        const int nV = (int)in.kfRow.size(), nE = (int)in.edgeI.size(), nP = (int)in.pointRow.size(), nS = (int)(in.sim3.size() / 8);
        int nFree = 0;
        for (unsigned char f : in.kfFixed) nFree += f ? 0 : 1;
        const size_t ws = xfh_essential_graph_workspace_bytes(nV, nE, nFree);
        if (ws == 0 || nP < 1 || nS < 1 || in.sim3.size() != (size_t)nS * 8 || in.kfFixed.size() != (size_t)nV || in.correctedIndex.size() != (size_t)nV ||
            in.nonCorrectedIndex.size() != (size_t)nV || in.edgeJ.size() != (size_t)nE || in.edgeKind.size() != (size_t)nE || in.pointRef.size() != (size_t)nP)
            throw std::runtime_error("XFoptimizer::OptimizeEssentialGraph: sizes out of range (more than XFH_EG_MAX_FREE free keyframes?)");
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t V = (size_t)nV, P = (size_t)nP, E = (size_t)nE;
        const size_t sz[] = {al(ws), al(V * 4), al(V), al(V * 4), al(V * 4), al((size_t)nS * 64), al(E * 4), al(E * 4), al(E * 4), al(P * 4), al(P * 4),
                             al(V * 64), al(V * 48), al(P * 12), al(E * 4), 256, 256};
        const int NQ = (int)(sizeof(sz) / sizeof(sz[0]));
        size_t need = 0;
        for (size_t v : sz) need += v;
        if (need > eg_bytes) {
            if (d_eg) { xfh_synchronize(ctx); xfh_dev_free(d_eg); d_eg = nullptr; eg_bytes = 0; }
            if (xfh_dev_alloc(&d_eg, need) != XFH_OK) throw std::runtime_error("XFoptimizer::OptimizeEssentialGraph: out of device memory");
            eg_bytes = need;
        }
        char* q[17];
        q[0] = (char*)d_eg;
        for (int i = 1; i < NQ; ++i) q[i] = q[i - 1] + sz[i - 1];
        d_egSim3 = (double*)q[11];
        d_egTcw = (float*)q[12]; d_egPoints = (float*)q[13]; d_egChi2 = (float*)q[14];
        egKF = nV; egPoints = nP; egEdges = nE;
        int rc = xfh_synchronize(ctx);
        const void* src[] = {in.kfRow.data(), in.kfFixed.data(), in.correctedIndex.data(), in.nonCorrectedIndex.data(), in.sim3.data(), in.edgeI.data(),
                             in.edgeJ.data(), in.edgeKind.data(), in.pointRow.data(), in.pointRef.data()};
        const size_t bytes_of[] = {V * 4, V, V * 4, V * 4, (size_t)nS * 64, E * 4, E * 4, E * 4, P * 4, P * 4};
        for (int i = 0; i < 10 && rc == XFH_OK; ++i) rc = xfh_memcpy_h2d(q[1 + i], src[i], bytes_of[i]);
        if (rc == XFH_OK) rc = xfh_essential_graph_device(ctx, nV, nFree, nE, nP, nS, in.d_poseTable, in.poseRows, in.d_pointTable, in.pointRows, (const int*)q[1],
                                                          (const unsigned char*)q[2], (const int*)q[3], (const int*)q[4], (const double*)q[5], (const int*)q[6],
                                                          (const int*)q[7], (const int*)q[8], (const int*)q[9], (const int*)q[10], bFixScale ? 1 : 0, iterations,
                                                          writeBack ? 1 : 0, q[0], d_egSim3, d_egTcw, d_egPoints, d_egChi2, (int*)q[15], (double*)q[16]);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(egHeader, q[15], XFH_EG_HEADER_INTS * 4);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(&egFinalChi2, q[16], 8);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFoptimizer::OptimizeEssentialGraph: ") + xfh_strerror(rc));
        return egHeader[0];
    }
    // of the last OptimizeEssentialGraph, in device memory: the corrected poses [keyframes][12] = [R | t / s] and points [points][3]; and copies on request:
    // egPoses(), egMapPoints(), egSim3() (the estimates [keyframes][8]) and egEdgeChi2().  LocalBundleAdjustment's getters keep speaking of LocalBundleAdjustment.
    const float* deviceEgTcw() const { return d_egTcw; }
    const float* deviceEgPoints() const { return d_egPoints; }
    void egPoses(std::vector<float>& out) const { lbaGet(out, d_egTcw, (size_t)egKF * 12); }
    void egMapPoints(std::vector<float>& out) const { lbaGet(out, d_egPoints, (size_t)egPoints * 3); }
    void egSim3(std::vector<double>& out) const { lbaGet(out, d_egSim3, (size_t)egKF * 8); }
    void egEdgeChi2(std::vector<float>& out) const { lbaGet(out, d_egChi2, (size_t)egEdges); }
    // status, free keyframes, valid edges, loop-connection edges, iterations, trials, rejected trials, factorisation failures, corrected points
    int egHeader[XFH_EG_HEADER_INTS] = {};
    double egFinalChi2 = 0.0;

    int nInitialCorrespondences() const { return header[0]; }
    int nBad() const { return header[1]; }
    // n_initial, n_bad, the return value, rounds run, Levenberg iterations, trials, rejected trials, factorisation failures
    int header[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double finalChi2 = 0.0;

private:
    xfh_ctx* ctx;
    void* d_buf = nullptr; size_t bytes = 0;
    float* d_pose = nullptr; unsigned char* d_outlier = nullptr; float* d_chi2 = nullptr;
    int n = 0;
    void* d_s3 = nullptr; size_t s3_bytes = 0;                       // OptimizeSim3's own buffer
    int* d_matches = nullptr; unsigned char* d_status = nullptr; float* d_chi2_pairs = nullptr; float* d_S12 = nullptr; float* d_Scw = nullptr; float* d_Ow = nullptr;
    int n_pairs = 0;
    void* d_lba = nullptr; size_t lba_bytes = 0;                     // LocalBundleAdjustment's own buffer
    float* d_lbaTcw = nullptr; float* d_lbaPoints = nullptr; unsigned char* d_lbaErase = nullptr; float* d_lbaChi2 = nullptr;
    int lbaKF = 0, lbaPoints = 0, lbaEdges = 0;
    void* d_eg = nullptr; size_t eg_bytes = 0;                       // OptimizeEssentialGraph's own buffer
    double* d_egSim3 = nullptr; float* d_egTcw = nullptr; float* d_egPoints = nullptr; float* d_egChi2 = nullptr;
    int egKF = 0, egPoints = 0, egEdges = 0;
    template <class T> void lbaGet(std::vector<T>& out, const T* d, size_t count) const {
        out.assign(count, T());
        if (count > 0 && xfh_memcpy_d2h(out.data(), d, count * sizeof(T)) != XFH_OK) throw std::runtime_error("XFoptimizer: download failed");
    }
};

}  // namespace ORB_SLAM3

#endif /* XFEAT_OPTIMIZER_XFEAT_H */
