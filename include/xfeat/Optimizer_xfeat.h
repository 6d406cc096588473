/*
 * Optimizer_xfeat.h -- the motion-only pose refinement of ORB_SLAM3::Optimizer on a frame whose arrays are in device memory.
 *
 * ORB_SLAM3::XFoptimizer::PoseOptimization is Optimizer::PoseOptimization(Frame*) (reference src/Optimizer.cc:814-1114, the conventional
 * camera with a Pinhole model) as one call of xfh_pose_optimize_device: the frame's undistorted keypoints and right coordinates as
 * xfh_frame_finish_records_device (or XFgrid::buildFromRecord) left them, the assignment a search wrote (assigned[k] = index of the map point
 * of keypoint k, or anything outside [0, nq) for none), the world points the search projected, and the pose.  It returns the reference's int
 * (nInitialCorrespondences - nBad) and leaves the new pose and the mvbOutlier flags in device memory, where the next search reads them; the
 * pose also comes back to the host, as pFrame->SetPose would want it.  This is not a graph optimiser: one SE3 vertex, unary edges, nothing else
 * (include/xfeat_hip.h has the contract line by line).  Header only; needs nothing but xfeat_hip.h.
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
    ~XFoptimizer() { if (d_buf) xfh_dev_free(d_buf); }
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
};

}  // namespace ORB_SLAM3

#endif /* XFEAT_OPTIMIZER_XFEAT_H */
