/*
 * TwoViewReconstruction_xfeat.h -- ORB_SLAM3::TwoViewReconstruction::Reconstruct on two frames whose arrays are in device memory.
 *
 * ORB_SLAM3::XFtwoView::Reconstruct is mpCamera->ReconstructWithTwoViews of Tracking::MonocularInitialization (reference src/Tracking.cc:2531,
 * src/TwoViewReconstruction.cc, the Pinhole camera) as one call of xfh_two_view_device: the undistorted keypoints of the reference and the
 * current frame as xfh_frame_finish_records_device (or XFgrid::deviceKeysUn()) left them and vnMatches12 as XFmatcher::searchForInitialization's
 * device overload left it.  It returns the reference's bool; T21, the points and the flags come back to the host as the caller of :2533-2560
 * wants them, and the match list with the untriangulated entries cleared stays on the device (deviceMatches()) for what follows.
 *
 * The reference draws its minimal sets with rand() after srand(0).  The library holds no generator: setDraws() takes iterations x 8 raw draws
 * and RAND_MAX; drawWithStdRand() fills them from the process's rand() in the order the reference consumes them (seed it as the reference does
 * to get the reference's sets).  The draws are kept and used by every call until replaced: the reference, which seeds once per process and
 * draws for every attempt, is followed by calling drawWithStdRand() before each Reconstruct.
 *
 * include/xfeat_hip.h has the contract line by line, the stated deviations included (on the H path this class, unlike the reference, fills
 * vP3D).  Header only; needs nothing but xfeat_hip.h.
 */
#ifndef XFEAT_TWOVIEWRECONSTRUCTION_XFEAT_H
#define XFEAT_TWOVIEWRECONSTRUCTION_XFEAT_H

#include "../xfeat_hip.h"

#include <cmath>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

namespace ORB_SLAM3 {

class XFtwoView {
public:
    XFtwoView(xfh_ctx* c, const xfh_camera& k, float sigma = 1.0f, int iterations = 200) : ctx(c), cam(k), mSigma(sigma), mMaxIterations(iterations) {
        if (iterations < 1 || iterations > XFH_TWO_VIEW_MAX_ITERS) throw std::runtime_error("XFtwoView: iterations out of range");
    }
    ~XFtwoView() { if (d_buf) xfh_dev_free(d_buf); if (d_draws) xfh_dev_free(d_draws); if (d_in) xfh_dev_free(d_in); }
    XFtwoView(const XFtwoView&) = delete;
    XFtwoView& operator=(const XFtwoView&) = delete;

    // iterations x 8 raw values of the caller's generator and its largest value
    void setDraws(const int* draws, int randMax) {
        const size_t nb = (size_t)mMaxIterations * 32;
        if (!d_draws && xfh_dev_alloc(&d_draws, nb) != XFH_OK) throw std::runtime_error("XFtwoView::setDraws: out of device memory");
        int rc = xfh_synchronize(ctx);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(d_draws, draws, nb);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFtwoView::setDraws: ") + xfh_strerror(rc));
        mRandMax = randMax;
    }
    void drawWithStdRand() {
        std::vector<int> d((size_t)mMaxIterations * 8);
        for (int& v : d) v = rand();
        setDraws(d.data(), RAND_MAX);
    }

    // d_keysUn1 [n1][2], d_keysUn2 [n2][2], d_matches12 [n1]: device memory.  Blocks until the header, T21, the points and the flags are on the host.
    bool Reconstruct(int n1, const float* d_keysUn1, int n2, const float* d_keysUn2, const int* d_matches12, float minParallax = 1.0f,
                     int minTriangulated = 50) {
        if (!d_draws) drawWithStdRand();
        const size_t ws = xfh_two_view_workspace_bytes(n1, n2, mMaxIterations, 1);
        if (ws == 0) throw std::runtime_error("XFtwoView::Reconstruct: sizes out of range");
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t N = (size_t)n1, need = al(ws) + 512 + 3 * al(N) + al(N * 12) + al(N * 4);
        if (need > bytes) {
            if (d_buf) { xfh_synchronize(ctx); xfh_dev_free(d_buf); d_buf = nullptr; bytes = 0; }
            if (xfh_dev_alloc(&d_buf, need) != XFH_OK) throw std::runtime_error("XFtwoView::Reconstruct: out of device memory");
            bytes = need;
        }
        char* p = (char*)d_buf;
        void* dws = p; p += al(ws);
        int* dh = (int*)p; p += 256;
        float* df = (float*)p; p += 256;
        unsigned char* dih = (unsigned char*)p; p += al(N);
        unsigned char* dif = (unsigned char*)p; p += al(N);
        d_tri = (unsigned char*)p; p += al(N);
        d_p3d = (float*)p; p += al(N * 12);
        d_matches = (int*)p;
        n = n1;
        const double mpc = std::cos((double)minParallax * 3.14159265358979323846 / 180.0);
        int rc = xfh_two_view_device(ctx, 1, n1, n2, d_keysUn1, d_keysUn2, d_matches12, &cam, mSigma, mMaxIterations, (const int*)d_draws, 0, mRandMax, mpc,
                                     minTriangulated, dws, dh, df, dih, dif, d_tri, d_p3d, d_matches);
        if (rc == XFH_OK) rc = xfh_synchronize(ctx);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(header, dh, sizeof header);
        const bool ok = rc == XFH_OK && header[1] >= XFH_TWO_VIEW_OK_H;
        for (float& v : floats) v = 0.0f;
        vP3D.assign(N * 3, 0.0f);
        std::vector<unsigned char> t(N, 0);
        if (rc == XFH_OK && header[1] != XFH_TWO_VIEW_TOO_FEW) {             // (with fewer than eight matches only the header is written)
            rc = xfh_memcpy_d2h(floats, df, sizeof floats);
            if (rc == XFH_OK) rc = xfh_memcpy_d2h(vP3D.data(), d_p3d, N * 12);
            if (rc == XFH_OK) rc = xfh_memcpy_d2h(t.data(), d_tri, N);
        }
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFtwoView::Reconstruct: ") + xfh_strerror(rc));
        vbTriangulated.assign(t.begin(), t.end());
        matchesValid = header[1] != XFH_TWO_VIEW_TOO_FEW;
        return ok;
    }

    // the same from host containers: keys as x, y pairs.  The arrays are staged in a device buffer this object owns.
    bool Reconstruct(const std::vector<float>& vKeysUn1, const std::vector<float>& vKeysUn2, const std::vector<int>& vMatches12, float minParallax = 1.0f,
                     int minTriangulated = 50) {
        const size_t n1 = vMatches12.size(), n2 = vKeysUn2.size() / 2;
        if (n1 == 0 || n2 == 0 || vKeysUn1.size() != 2 * n1) throw std::runtime_error("XFtwoView::Reconstruct: container sizes disagree");
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t need = al(n1 * 8) + al(n2 * 8) + al(n1 * 4);
        if (need > in_bytes) {
            if (d_in) { xfh_synchronize(ctx); xfh_dev_free(d_in); d_in = nullptr; in_bytes = 0; }
            if (xfh_dev_alloc(&d_in, need) != XFH_OK) throw std::runtime_error("XFtwoView::Reconstruct: out of device memory");
            in_bytes = need;
        }
        char* p = (char*)d_in;
        float* d1 = (float*)p; float* d2 = (float*)(p + al(n1 * 8)); int* dm = (int*)(p + al(n1 * 8) + al(n2 * 8));
        int rc = xfh_synchronize(ctx);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(d1, vKeysUn1.data(), n1 * 8);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(d2, vKeysUn2.data(), n2 * 8);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dm, vMatches12.data(), n1 * 4);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFtwoView::Reconstruct: ") + xfh_strerror(rc));
        return Reconstruct((int)n1, d1, (int)n2, d2, dm, minParallax, minTriangulated);
    }

    // of the last call
    const float* T21() const { return floats + 21; }                        // row-major 3x4 [R|t]; zeros unless the call returned true
    std::vector<float> vP3D;                                                // [n1][3], indexed like mvIniP3D
    std::vector<bool> vbTriangulated;                                       // [n1]
    int header[XFH_TWO_VIEW_HEADER_INTS] = {};                              // N, status, model, winners, nGood[8], chosen, inlier counts, ... (xfeat_hip.h)
    float floats[XFH_TWO_VIEW_FLOATS] = {};                                 // SH, SF, RH, H21, F21, T21, the cosines
    int status() const { return header[1]; }
    float SH() const { return floats[0]; }
    float SF() const { return floats[1]; }
    float RH() const { return floats[2]; }
    // the reference's parallax of motion hypothesis h: acos(cos) * 180 / pi, converted on the host
    // (NaN for an h outside 0 .. 7, such as the -1 the header holds for the chosen hypothesis after a call that returned false)
    float parallaxDegrees(int h) const {
        if (h < 0 || h > 7) return std::nanf("");
        return (float)(std::acos((double)floats[33 + h]) * 180.0 / 3.14159265358979323846);
    }
    const std::vector<float>& P3D() const { return vP3D; }
    const std::vector<bool>& Triangulated() const { return vbTriangulated; }
    const int* Header() const { return header; }
    int chosenHypothesis() const { return header[13]; }
    // mvIniMatches after Tracking.cc:2533-2540 (matched but untriangulated entries are -1 when the call returned true), in device memory and copied
    const int* deviceMatches() const { return matchesValid ? d_matches : nullptr; }
    const float* deviceP3D() const { return d_p3d; }
    const unsigned char* deviceTriangulated() const { return d_tri; }
    void matches(std::vector<int>& mvIniMatches) const {
        if (!matchesValid) throw std::runtime_error("XFtwoView::matches: the last call had fewer than eight matches and wrote none");
        mvIniMatches.assign((size_t)n, -1);
        if (n > 0 && xfh_memcpy_d2h(mvIniMatches.data(), d_matches, (size_t)n * 4) != XFH_OK) throw std::runtime_error("XFtwoView::matches: download failed");
    }

private:
    xfh_ctx* ctx;
    xfh_camera cam;
    float mSigma; int mMaxIterations; int mRandMax = RAND_MAX;
    void* d_buf = nullptr; size_t bytes = 0;
    void* d_draws = nullptr;
    void* d_in = nullptr; size_t in_bytes = 0;
    unsigned char* d_tri = nullptr; float* d_p3d = nullptr; int* d_matches = nullptr;
    int n = 0; bool matchesValid = false;
};

}  // namespace ORB_SLAM3

#endif /* XFEAT_TWOVIEWRECONSTRUCTION_XFEAT_H */
