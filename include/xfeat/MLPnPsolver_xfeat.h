/*
 * MLPnPsolver_xfeat.h -- ORB_SLAM3::MLPnPsolver under the iterate(5) calls of Tracking::Relocalization on arrays in device memory.
 *
 * ORB_SLAM3::XFmlpnpSolver is `MLPnPsolver* pSolver = new MLPnPsolver(mCurrentFrame, vvpMapPointMatches[i]); pSolver->SetRansacParameters(0.99, 10, 300,
 * 6, 0.5, 5.991); ... pSolver->iterate(5, bNoMore, vbInliers, nInliers, eigTcw)` (reference src/Tracking.cc:3715-3742, src/MLPnPsolver.cpp, the Pinhole
 * camera) on top of xfh_mlpnp_solve_device: setProblem() binds what the constructor reads -- the frame's undistorted keypoints, row i of the BoW
 * search's assigned2 output and the candidate's point block, all in device memory --, iterate() is one call of the library, fresh the first time
 * and resumed afterwards (the solver's state between two calls is one number, the iterations consumed so far).  It returns what the reference's bool
 * means, with one stated deviation: Refine's re-solved pose is stored and reported, where the reference as written reports the calling iteration's;
 * the inlier flags and the pose come back to the host as :3744-3771 want them, and deviceTcw() / deviceAssigned() are the pose and
 * mCurrentFrame.mvpMapPoints after :3762-3771 in the layout xfh_pose_optimize_device takes, so PoseOptimization can follow without a host step.
 *
 * The reference draws its minimal sets with rand().  The library holds no generator: setDraws() takes maxIterations x 6 raw draws and RAND_MAX;
 * drawWithStdRand() fills them from the process's rand() in the order the reference consumes them.  consumed() says how many iterations (six
 * draws each) the reference would have used so far.
 *
 * include/xfeat_hip.h has the contract line by line, the stated deviations included.  Header only; needs nothing but xfeat_hip.h.
 */
#ifndef XFEAT_MLPNPSOLVER_XFEAT_H
#define XFEAT_MLPNPSOLVER_XFEAT_H

#include "../xfeat_hip.h"

#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

namespace ORB_SLAM3 {

class XFmlpnpSolver {
public:
    // maxIterations: how many iterations the draws hold (>= the maxIterations of SetRansacParameters); sigma2: mvLevelSigma2[0]
    XFmlpnpSolver(xfh_ctx* c, const xfh_camera& k, int maxIterations = 300, float sigma2 = 1.0f) : ctx(c), cam(k), mMaxIterations(maxIterations), mSigma2(sigma2) {
        if (maxIterations < 1 || maxIterations > XFH_MLPNP_MAX_ITERS) throw std::runtime_error("XFmlpnpSolver: iterations out of range");
        mMaxErr = mSigma2 * 5.991f;
    }
    ~XFmlpnpSolver() { if (d_buf) xfh_dev_free(d_buf); if (d_draws) xfh_dev_free(d_draws); if (d_in) xfh_dev_free(d_in); }
    XFmlpnpSolver(const XFmlpnpSolver&) = delete;
    XFmlpnpSolver& operator=(const XFmlpnpSolver&) = delete;

    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 6, float epsilon = 0.4f, float th2 = 5.991f) {
        if (minSet != 6) throw std::runtime_error("XFmlpnpSolver: minSet must be 6");
        mProb = probability; mMinInliers = minInliers; mMaxIts = maxIterations; mEps = epsilon; mMaxErr = mSigma2 * th2; tableN = -1;
    }
    // maxIterations x 6 raw values of the caller's generator and its largest value
    void setDraws(const int* draws, int randMax) {
        const size_t nb = (size_t)mMaxIterations * 24;
        if (!d_draws && xfh_dev_alloc(&d_draws, nb) != XFH_OK) throw std::runtime_error("XFmlpnpSolver::setDraws: out of device memory");
        int rc = xfh_synchronize(ctx);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(d_draws, draws, nb);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFmlpnpSolver::setDraws: ") + xfh_strerror(rc));
        mRandMax = randMax;
    }
    void drawWithStdRand() {
        std::vector<int> d((size_t)mMaxIterations * 6);
        for (int& v : d) v = rand();
        setDraws(d.data(), RAND_MAX);
    }

    // what the reference's constructor reads, in device memory: d_xy_un [n][2] (mvKeysUn), d_assigned [n] (keypoint -> index into the point block, as
    // the BoW search's assigned2 row), d_points [nq][3], d_pointValid [nq] bytes or null, the BoW search's match count on the device or null.
    // The next iterate() starts at iteration 0.
    void setProblem(int n, int nq, const float* d_xy_un, const int* d_assigned, const float* d_points, const unsigned char* d_pointValid = nullptr,
                    const int* d_nMatches = nullptr, int minMatches = 0) {
        pn = n; pnq = nq; pxy = d_xy_un; passigned = d_assigned; ppoints = d_points; pvalid = d_pointValid; pnm = d_nMatches; pmin = minMatches; mConsumed = 0;
        poseValid = false;
    }
    // the same from host containers: keypoints as x, y pairs, points as x, y, z triples; staged in a device buffer this object owns.  nMatches >= 0: the
    // BoW search's match count, gated against minMatches (nmatches < 15, Tracking.cc:3708)
    void setProblem(const std::vector<float>& vKeysUn, const std::vector<int>& vAssigned, const std::vector<float>& vPoints,
                    const std::vector<unsigned char>* vPointValid = nullptr, int nMatches = -1, int minMatches = 0) {
        const size_t n = vAssigned.size(), nq = vPoints.size() / 3;
        if (n == 0 || nq == 0 || vKeysUn.size() != 2 * n || vPoints.size() != 3 * nq || (vPointValid && vPointValid->size() != nq))
            throw std::runtime_error("XFmlpnpSolver::setProblem: container sizes disagree");
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t need = al(n * 8) + al(n * 4) + al(nq * 12) + al(nq) + 256;
        if (need > in_bytes) {
            if (d_in) { xfh_synchronize(ctx); xfh_dev_free(d_in); d_in = nullptr; in_bytes = 0; }
            if (xfh_dev_alloc(&d_in, need) != XFH_OK) throw std::runtime_error("XFmlpnpSolver::setProblem: out of device memory");
            in_bytes = need;
        }
        char* p = (char*)d_in;
        float* dxy = (float*)p; p += al(n * 8);
        int* da = (int*)p; p += al(n * 4);
        float* dp = (float*)p; p += al(nq * 12);
        unsigned char* dv = (unsigned char*)p; p += al(nq);
        int* dnm = (int*)p;
        int rc = xfh_synchronize(ctx);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dxy, vKeysUn.data(), n * 8);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(da, vAssigned.data(), n * 4);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dp, vPoints.data(), nq * 12);
        if (rc == XFH_OK && vPointValid) rc = xfh_memcpy_h2d(dv, vPointValid->data(), nq);
        if (rc == XFH_OK && nMatches >= 0) rc = xfh_memcpy_h2d(dnm, &nMatches, 4);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFmlpnpSolver::setProblem: ") + xfh_strerror(rc));
        setProblem((int)n, (int)nq, dxy, da, dp, vPointValid ? dv : nullptr, nMatches >= 0 ? dnm : nullptr, minMatches);
    }

    // iterate(nIterations, ..) of the reference on the bound problem: fresh after setProblem(), resumed otherwise.  Tcw: row-major [R|t], written
    // when the call returns true.  Blocks until the header, the flags and the pose are on the host.
    bool iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliersOut, int& nInliersOut, float* TcwOut) {
        if (pn <= 0) throw std::runtime_error("XFmlpnpSolver::iterate: no problem bound");
        if (!d_draws) drawWithStdRand();
        const size_t ws = xfh_mlpnp_workspace_bytes(pn, pnq, 1, mMaxIterations);
        if (ws == 0) throw std::runtime_error("XFmlpnpSolver::iterate: sizes out of range");
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t N = (size_t)pn, need = al(ws) + 3 * 256 + al(N) + al(N * 4) + 2 * al((N + 1) * 4);
        if (need > bytes) {
            if (d_buf) { xfh_synchronize(ctx); xfh_dev_free(d_buf); d_buf = nullptr; bytes = 0; }
            if (xfh_dev_alloc(&d_buf, need) != XFH_OK) throw std::runtime_error("XFmlpnpSolver::iterate: out of device memory");
            bytes = need; tableN = -1;
        }
        char* p = (char*)d_buf;
        void* dws = p; p += al(ws);
        int* dh = (int*)p; p += 256;
        d_Tcw = (float*)p; p += 256;
        int* dstart = (int*)p; p += 256;
        unsigned char* di = (unsigned char*)p; p += al(N);
        d_assignedOut = (int*)p; p += al(N * 4);
        int* dti = (int*)p; p += al((N + 1) * 4);
        int* dtm = (int*)p;
        int rc = xfh_synchronize(ctx);
        if (rc == XFH_OK && tableN != pn) {                                   // SetRansacParameters per N: host libm, as the reference evaluates it
            std::vector<int> ti(N + 1), tm(N + 1);
            rc = xfh_mlpnp_iterations_table(mProb, mMinInliers, mMaxIts, 6, mEps, pn, ti.data(), tm.data());
            if (rc == XFH_OK) rc = xfh_memcpy_h2d(dti, ti.data(), (N + 1) * 4);
            if (rc == XFH_OK) rc = xfh_memcpy_h2d(dtm, tm.data(), (N + 1) * 4);
            tableN = pn;
        }
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dstart, &mConsumed, 4);
        if (rc == XFH_OK) rc = xfh_mlpnp_solve_device(ctx, 1, pn, pnq, pxy, passigned, ppoints, pvalid, &cam, mMaxErr, pmin, pnm, dti, dtm, nIterations, dstart,
                                                      mMaxIterations, (const int*)d_draws, 0, mRandMax, dws, dh, d_Tcw, di, d_assignedOut);
        if (rc == XFH_OK) rc = xfh_synchronize(ctx);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(header, dh, sizeof header);
        std::vector<unsigned char> f(N, 0);
        const bool ran = rc == XFH_OK && header[1] != XFH_MLPNP_TOO_FEW;       // (with too few correspondences only the header is written)
        const bool ok = ran && header[1] != XFH_MLPNP_NONE;
        if (ran) rc = xfh_memcpy_d2h(f.data(), di, N);
        for (float& v : Tcw) v = 0.0f;
        if (ok && rc == XFH_OK) rc = xfh_memcpy_d2h(Tcw, d_Tcw, sizeof Tcw);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFmlpnpSolver::iterate: ") + xfh_strerror(rc));
        if (ran) mConsumed = header[8];
        vbInliers.assign(f.begin(), f.end());
        poseValid = ok; assignedValid = true;
        bNoMore = header[1] != XFH_MLPNP_REFINED;
        vbInliersOut = ok ? vbInliers : std::vector<bool>();
        nInliersOut = ok ? header[5] : 0;
        if (ok && TcwOut) for (int k = 0; k < 12; ++k) TcwOut[k] = Tcw[k];
        return ok;
    }

    // of the last iterate()
    int status() const { return header[1]; }
    int nCorrespondences() const { return header[0]; }
    int iterations() const { return header[2]; }
    int minInliers() const { return header[3]; }
    int consumed() const { return mConsumed; }                              // iterations used so far: the next call starts there
    // [R|t] [12] and mvpMapPoints [n] (the assigned index where the keypoint is an inlier, -1 elsewhere) for xfh_pose_optimize_device; null unless the
    // call returned true (deviceAssigned: never null after a call, all -1 when it found nothing or had too few correspondences)
    const float* deviceTcw() const { return poseValid ? d_Tcw : nullptr; }
    const int* deviceAssigned() const { return assignedValid ? d_assignedOut : nullptr; }
    // (plain results of the last iterate(), public for reading as in the other XF classes; writing them changes nothing the solver uses)
    int header[XFH_MLPNP_HEADER_INTS] = {};
    float Tcw[12] = {};
    std::vector<bool> vbInliers;                                            // [n], by keypoint

private:
    xfh_ctx* ctx;
    xfh_camera cam;
    int mMaxIterations; float mSigma2; int mRandMax = RAND_MAX;
    double mProb = 0.99; int mMinInliers = 8, mMaxIts = 300; float mEps = 0.4f, mMaxErr = 5.991f;      // MLPnPsolver.h's defaults
    int pn = 0, pnq = 0, pmin = 0, mConsumed = 0;
    const float *pxy = nullptr, *ppoints = nullptr; const int *passigned = nullptr, *pnm = nullptr; const unsigned char* pvalid = nullptr;
    void* d_buf = nullptr; size_t bytes = 0;
    void* d_draws = nullptr;
    void* d_in = nullptr; size_t in_bytes = 0;
    float* d_Tcw = nullptr; int* d_assignedOut = nullptr;
    int tableN = -1; bool poseValid = false, assignedValid = false;
};

}  // namespace ORB_SLAM3

#endif /* XFEAT_MLPNPSOLVER_XFEAT_H */
