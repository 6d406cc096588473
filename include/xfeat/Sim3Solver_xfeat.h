/*
 * Sim3Solver_xfeat.h -- ORB_SLAM3::Sim3Solver under the iterate(20) loop of LoopClosing::DetectCommonRegionsFromBoW on arrays in device memory.
 *
 * ORB_SLAM3::XFsim3Solver::solve is `Sim3Solver solver(mpCurrentKF, pMostBoWMatchesKF, vpMatchedPoints, bFixedScale, vpKeyFrameMatchedMP);
 * solver.SetRansacParameters(0.99, nBoWInliers, 300); while(!bConverge && !bNoMore) solver.iterate(20, ..)` (reference src/LoopClosing.cc:698-710,
 * src/Sim3Solver.cc, the Pinhole camera) as one call of xfh_sim3_solve_device: map points are rows of one table of world positions, the current
 * keyframe's and the matched points are row indices per keypoint (the second as xfh_sim3_merge_matches_device leaves them).  It returns
 * bConverge; the similarity and the inlier flags come back to the host as :712-749 want them, and the composed pose gScm * gSmw stays on the
 * device (deviceTcw() / deviceOw()) in the layout xfh_map_projection_search_device takes.
 *
 * The reference draws its minimal sets with rand().  The library holds no generator: setDraws() takes maxIterations x 3 raw draws and RAND_MAX;
 * drawWithStdRand() fills them from the process's rand() in the order the reference consumes them.  The reference stops drawing when it
 * converges: consumed() says how many iterations (three draws each) it would have used.
 *
 * include/xfeat_hip.h has the contract line by line, the stated deviations included (an exactly zero rotation gives the identity here and NaN
 * in the reference).  Header only; needs nothing but xfeat_hip.h.
 */
#ifndef XFEAT_SIM3SOLVER_XFEAT_H
#define XFEAT_SIM3SOLVER_XFEAT_H

#include "../xfeat_hip.h"

#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

namespace ORB_SLAM3 {

class XFsim3Solver {
public:
    // sigma2: mvLevelSigma2[0] of the two keyframes (every XFeat keypoint has octave 0)
    XFsim3Solver(xfh_ctx* c, const xfh_camera& k1, const xfh_camera& k2, int maxIterations = 300, float sigma2_1 = 1.0f, float sigma2_2 = 1.0f)
        : ctx(c), cam1(k1), cam2(k2), mMaxIterations(maxIterations) {
        if (maxIterations < 1 || maxIterations > XFH_SIM3_SOLVE_MAX_ITERS) throw std::runtime_error("XFsim3Solver: iterations out of range");
        mMaxErr1 = (float)(size_t)(9.210 * sigma2_1); mMaxErr2 = (float)(size_t)(9.210 * sigma2_2);      // the reference's std::vector<size_t> truncates
    }
    ~XFsim3Solver() { if (d_buf) xfh_dev_free(d_buf); if (d_draws) xfh_dev_free(d_draws); if (d_in) xfh_dev_free(d_in); }
    XFsim3Solver(const XFsim3Solver&) = delete;
    XFsim3Solver& operator=(const XFsim3Solver&) = delete;

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
        mProb = probability; mMinInliers = minInliers; mMaxIts = maxIterations; tableN = -1;
    }
    // maxIterations x 3 raw values of the caller's generator and its largest value
    void setDraws(const int* draws, int randMax) {
        const size_t nb = (size_t)mMaxIterations * 12;
        if (!d_draws && xfh_dev_alloc(&d_draws, nb) != XFH_OK) throw std::runtime_error("XFsim3Solver::setDraws: out of device memory");
        int rc = xfh_synchronize(ctx);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(d_draws, draws, nb);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFsim3Solver::setDraws: ") + xfh_strerror(rc));
        mRandMax = randMax;
    }
    void drawWithStdRand() {
        std::vector<int> d((size_t)mMaxIterations * 3);
        for (int& v : d) v = rand();
        setDraws(d.data(), RAND_MAX);
    }

    // d_points [M][3], d_point1 [n1], d_matched [n1], d_T1w [12], d_T2w [12]: device memory; d_numMatches: the merge's count on the device, or null.
    // Blocks until the header, the similarity and the flags are on the host.
    bool solve(int n1, int M, const float* d_points, const int* d_point1, const int* d_matched, const float* d_T1w, const float* d_T2w, bool bFixScale,
               const int* d_numMatches = nullptr, int minMatches = 0) {
        if (!d_draws) drawWithStdRand();
        const size_t ws = xfh_sim3_solve_workspace_bytes(n1, M, 1);
        if (ws == 0) throw std::runtime_error("XFsim3Solver::solve: sizes out of range");
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t N = (size_t)n1, need = al(ws) + 4 * 256 + al(N) + al((N + 1) * 4);
        if (need > bytes) {
            if (d_buf) { xfh_synchronize(ctx); xfh_dev_free(d_buf); d_buf = nullptr; bytes = 0; }
            if (xfh_dev_alloc(&d_buf, need) != XFH_OK) throw std::runtime_error("XFsim3Solver::solve: out of device memory");
            bytes = need; tableN = -1;
        }
        char* p = (char*)d_buf;
        void* dws = p; p += al(ws);
        int* dh = (int*)p; p += 256;
        float* df = (float*)p; p += 256;
        d_Tcw = (float*)p; p += 256;
        d_Ow = (float*)p; p += 256;
        unsigned char* di = (unsigned char*)p; p += al(N);
        int* dt = (int*)p;
        int rc = XFH_OK;
        if (tableN != n1) {                                                  // the iteration count per N: host libm, as the reference evaluates it
            std::vector<int> table(N + 1);
            rc = xfh_sim3_solve_iterations_table(mProb, mMinInliers, mMaxIts, n1, table.data());
            if (rc == XFH_OK) rc = xfh_synchronize(ctx);
            if (rc == XFH_OK) rc = xfh_memcpy_h2d(dt, table.data(), (N + 1) * 4);
            tableN = n1;
        }
        if (rc == XFH_OK) rc = xfh_sim3_solve_device(ctx, 1, n1, M, d_points, d_point1, d_matched, d_T1w, 0, d_T2w, &cam1, &cam2, mMaxErr1, mMaxErr2, bFixScale ? 1 : 0,
                                                     mMinInliers, minMatches, d_numMatches, dt, mMaxIterations, (const int*)d_draws, 0, mRandMax, dws, dh, df, di,
                                                     d_Tcw, d_Ow);
        if (rc == XFH_OK) rc = xfh_synchronize(ctx);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(header, dh, sizeof header);
        for (float& v : floats) v = 0.0f;
        for (float& v : Tcw) v = 0.0f;
        for (float& v : Ow) v = 0.0f;
        std::vector<unsigned char> f(N, 0);
        if (rc == XFH_OK && header[1] != XFH_SIM3_SOLVE_TOO_FEW) {           // (with too few correspondences only the header is written)
            rc = xfh_memcpy_d2h(floats, df, sizeof floats);
            if (rc == XFH_OK) rc = xfh_memcpy_d2h(f.data(), di, N);
        }
        const bool ok = rc == XFH_OK && header[1] == XFH_SIM3_SOLVE_CONVERGED;
        if (ok) {                                                            // (the pose is written only when the problem converged)
            rc = xfh_memcpy_d2h(Tcw, d_Tcw, sizeof Tcw);
            if (rc == XFH_OK) rc = xfh_memcpy_d2h(Ow, d_Ow, sizeof Ow);
        }
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFsim3Solver::solve: ") + xfh_strerror(rc));
        vbInliers.assign(f.begin(), f.end());
        poseValid = ok;
        return ok;
    }

    // the same from host containers: points as x, y, z triples, T1w / T2w row-major [R|t].  The arrays are staged in a device buffer this object owns.
    bool solve(const std::vector<float>& vPoints, const std::vector<int>& vPoint1, const std::vector<int>& vMatched, const float* T1w, const float* T2w,
               bool bFixScale) {
        const size_t n1 = vPoint1.size(), M = vPoints.size() / 3;
        if (n1 == 0 || M == 0 || vMatched.size() != n1 || vPoints.size() != 3 * M) throw std::runtime_error("XFsim3Solver::solve: container sizes disagree");
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t need = al(M * 12) + 2 * al(n1 * 4) + 2 * 256;
        if (need > in_bytes) {
            if (d_in) { xfh_synchronize(ctx); xfh_dev_free(d_in); d_in = nullptr; in_bytes = 0; }
            if (xfh_dev_alloc(&d_in, need) != XFH_OK) throw std::runtime_error("XFsim3Solver::solve: out of device memory");
            in_bytes = need;
        }
        char* p = (char*)d_in;
        float* dp = (float*)p; p += al(M * 12);
        int* d1 = (int*)p; p += al(n1 * 4);
        int* dm = (int*)p; p += al(n1 * 4);
        float* dT1 = (float*)p; p += 256;
        float* dT2 = (float*)p;
        int rc = xfh_synchronize(ctx);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dp, vPoints.data(), M * 12);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(d1, vPoint1.data(), n1 * 4);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dm, vMatched.data(), n1 * 4);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dT1, T1w, 48);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dT2, T2w, 48);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFsim3Solver::solve: ") + xfh_strerror(rc));
        return solve((int)n1, (int)M, dp, d1, dm, dT1, dT2, bFixScale);
    }

    // of the last call: the winner's similarity, or the best iteration's when it did not converge (zeros with too few correspondences)
    const float* T12() const { return floats; }                             // row-major 3x4 [sR|t]
    const float* GetEstimatedRotation() const { return floats + 12; }       // row-major 3x3
    const float* GetEstimatedTranslation() const { return floats + 21; }
    float GetEstimatedScale() const { return floats[24]; }
    const std::vector<bool>& inliers() const { return vbInliers; }          // [n1], vbInliers of iterate(): all false unless the call converged
    int nInliers() const { return header[4]; }
    int status() const { return header[1]; }
    int nCorrespondences() const { return header[0]; }
    int iterations() const { return header[2]; }
    int consumed() const { return header[7]; }
    // Scw = S12 o T2w for ORBmatcher::SearchByProjection(pKF, Scw, ..): d_Tcw [12] / d_Ow [3] of xfh_map_projection_search_device; null unless converged
    const float* deviceTcw() const { return poseValid ? d_Tcw : nullptr; }
    const float* deviceOw() const { return poseValid ? d_Ow : nullptr; }
    int header[XFH_SIM3_SOLVE_HEADER_INTS] = {};
    float floats[XFH_SIM3_SOLVE_FLOATS] = {};
    float Tcw[12] = {}, Ow[3] = {};                                         // the composed pose on the host (zeros unless converged)
    std::vector<bool> vbInliers;

private:
    xfh_ctx* ctx;
    xfh_camera cam1, cam2;
    int mMaxIterations; int mRandMax = RAND_MAX;
    float mMaxErr1, mMaxErr2;
    double mProb = 0.99; int mMinInliers = 6, mMaxIts = 300;                // Sim3Solver.h's defaults
    void* d_buf = nullptr; size_t bytes = 0;
    void* d_draws = nullptr;
    void* d_in = nullptr; size_t in_bytes = 0;
    float *d_Tcw = nullptr, *d_Ow = nullptr;
    int tableN = -1; bool poseValid = false;
};

}  // namespace ORB_SLAM3

#endif /* XFEAT_SIM3SOLVER_XFEAT_H */
