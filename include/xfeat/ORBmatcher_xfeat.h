/*
 * ORBmatcher_xfeat.h -- the XFeat half of the reference's ORB_SLAM3::ORBmatcher
 * (include/ORBmatcher.h:43,77) on top of include/xfeat_hip.h.
 *
 *   static int DescriptorDistance(const cv::Mat& a, const cv::Mat& b)   -- ORBmatcher.cc:2242-2250
 *   void match(cv::Mat d1, cv::Mat d2, std::vector<cv::DMatch>& out)    -- declared :77, the
 *        definition is commented out in the reference (ORBmatcher.cc:340-405); this supplies it.
 *   TH_LOW / TH_HIGH                                                    -- ORBmatcher.cc:34-35
 *   XFgrid / XFmatcher::searchWindow: Frame::AssignFeaturesToGrid + GetFeaturesInArea (Frame.cc:569-599, 850-916) and the
 *        loop of SearchByProjection (ORBmatcher.cc:1925-1955) on the GPU: a frame grid in device memory and one fused
 *        window -> candidates -> best two call for all queries; XFgrid::buildFromRecord(record, n, camera, bounds, depth) is the rest
 *        of the RGB-D Frame constructor (UndistortKeyPoints, ComputeStereoFromRGBD, the grid on mvKeysUn; Frame.cc:311-374)
 *   XFmatcher::searchByProjection: the whole of ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono) (ORBmatcher.cc:1861-2047)
 *        and of the SearchLocalPoints form (:42-141): projection, cull, windowed best two and the reference's claim order in one call
 *   XFmatcher::fuse / searchForTriangulation: the two matchers of LocalMapping, ORBmatcher::Fuse (ORBmatcher.cc:1333-1640) up to the map
 *        bookkeeping and ORBmatcher::SearchForTriangulation (:1092-1331) over the nodes of the DBoW2 feature vectors, each as one call
 *   XFmatcher::triangulate: the loop body of LocalMapping::CreateNewMapPoints (LocalMapping.cc:481-710) behind searchForTriangulation for all
 *        neighbours at once: the new map points with their normals and distance bounds, the first accepted neighbour owning a keypoint
 *   XFmatcher::searchByProjection(Sim3Form / RelocForm, ...) / searchBySim3: the matchers of LoopClosing and Tracking::Relocalization, the Sim3
 *        forms of SearchByProjection (ORBmatcher.cc:612-717, :719-831), the relocalisation form (:2074-2195) and SearchBySim3 (:1642-1859), each
 *        as one call.  The caller keeps what needs Sophus or the map: the decomposition of Scw into Tcw = [R | t/s] and Ow (:621-622), S12 and its
 *        inverse as 3x4 [s*R | t], vbAlreadyMatched (:1662-1675, folded into the flag bytes) and the pointer writes behind the matches
 *   XFmatcher::searchForInitialization: ORBmatcher::SearchForInitialization (ORBmatcher.cc:833-948), the matcher of
 *        Tracking::MonocularInitialization, with the reference's retraction order as one call; vbPrevMatched travels as (x, y) floats and is
 *        updated in place
 *   XFvocabulary: the DBoW2 vocabulary as a blob in device memory and Frame::ComputeBoW / KeyFrame::ComputeBoW on it (TemplatedVocabulary::transform):
 *        mBowVec, mFeatVec and, without a host step, the node blob searchByBoW / searchForTriangulation read in their device forms
 *   best2 / distinctive: the batched inner loops of SearchBy* (ORBmatcher.cc:75-119) and of
 *        MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:329-403)
 *
 * Drop the two member definitions into src/ORBmatcher.cc or use this
 * class directly.  Without OpenCV the cvlite mirrors of XFextractor.h are used.
 */
#ifndef XFEAT_ORBMATCHER_XFEAT_H
#define XFEAT_ORBMATCHER_XFEAT_H

#include "XFextractor.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>

namespace xfeat {
#if !XFEAT_HAVE_OPENCV
namespace cvlite {
struct DMatch {
    int queryIdx = -1, trainIdx = -1, imgIdx = -1; float distance = 3.402823466e+38f;
    DMatch() = default;
    DMatch(int q, int t, float d) : queryIdx(q), trainIdx(t), distance(d) {}
};
}  // namespace cvlite
#endif
}  // namespace xfeat

namespace ORB_SLAM3 {

// The frame grid of one frame in device memory (xfh_grid_build_device; Frame::AssignFeaturesToGrid, Frame.cc:569-599): owns the
// blob.  build() uploads a host keypoint vector (all slots are binned, padding included, as the reference does);
// buildFromRecord() takes the keypoints straight from an extraction record that is already in device memory (flags:
// XFH_GRID_SKIP_PADDING leaves the padding slots out).  featuresInArea() is Frame::GetFeaturesInArea (Frame.cc:850-916) on a host
// copy of the grid, for callers that still want the index list; XFmatcher::searchWindow never needs it.
class XFgrid {
public:
    using KeyPoint = xfeat::cvx::KeyPoint;
    explicit XFgrid(xfh_ctx* shared_ctx) : ctx(shared_ctx) {}
    ~XFgrid() { if (d_grid) xfh_dev_free(d_grid); if (d_kps) xfh_dev_free(d_kps); if (d_side) xfh_dev_free(d_side); if (d_img) xfh_dev_free(d_img); }
    XFgrid(const XFgrid&) = delete;
    XFgrid& operator=(const XFgrid&) = delete;

    void build(const std::vector<KeyPoint>& keys, const xfh_grid_bounds& bounds) {
        static_assert(sizeof(KeyPoint) == sizeof(xfh_keypoint), "KeyPoint must mirror xfh_keypoint");
        const int count = (int)keys.size();
        reserve(count, true);
        if (count > 0 && xfh_memcpy_h2d(d_kps, keys.data(), (size_t)count * sizeof(xfh_keypoint)) != XFH_OK) throw std::runtime_error("XFgrid::build: upload failed");
        finish(xfh_grid_build_device(ctx, (const xfh_keypoint*)d_kps, count, nullptr, &bounds, 0, d_grid), count, bounds);
        host_x.resize(count); host_y.resize(count);
        for (int i = 0; i < count; ++i) { host_x[i] = keys[i].pt.x; host_y[i] = keys[i].pt.y; }
        side_n = -1; side_host = false;
    }
    // d_record: one record of `nfeatures` slots in device memory (xfh_extract_batch_device)
    void buildFromRecord(const void* d_record, int nfeatures, const xfh_grid_bounds& bounds, int flags = 0) {
        reserve(nfeatures, false);
        finish(xfh_grid_build_device(ctx, (const xfh_keypoint*)((const char*)d_record + xfh_record_kps_offset()), nfeatures, d_record, &bounds, flags, d_grid),
               nfeatures, bounds);
        host_x.clear(); host_y.clear(); side_n = -1; side_host = false;
    }
    // The RGB-D Frame constructor between ExtractXF and the first search (Frame.cc:311-374) for a camera WITH distortion, one launch
    // (xfh_frame_finish_records_device): UndistortKeyPoints -> keysUn(), ComputeStereoFromRGBD -> uRight() / depth(), and
    // AssignFeaturesToGrid on the undistorted keypoints with `bounds` (xfh_camera_bounds(&cam, &bounds), once per calibration).
    // d_record: one record of the ctx' nfeatures slots in device memory.  depth: the HOST depth image (cam.height rows, depth_pitch
    // bytes apart; XFH_DEPTH_F32 metres or XFH_DEPTH_U16 raw values times depth_scale = 1.0f / DepthMapFactor), uploaded into a
    // buffer of the object; nullptr / XFH_DEPTH_NONE = the monocular constructor (uRight = depth = -1).  The three arrays live in
    // device memory owned by the object (deviceKeysUn / deviceURight / deviceDepth: what xfh_search_window_device takes); the host
    // getters download them at the first call after a build.
    void buildFromRecord(const void* d_record, int nfeatures, const xfh_camera& cam, const xfh_grid_bounds& bounds, const void* depth = nullptr,
                         int depth_type = XFH_DEPTH_NONE, size_t depth_pitch = 0, float depth_scale = 1.0f, int flags = 0) {
        reserve(nfeatures, false);
        const size_t sb = (size_t)(nfeatures > 0 ? nfeatures : 1) * 16;
        if (sb > side_cap) {
            if (d_side) xfh_dev_free(d_side);
            d_side = nullptr; side_cap = 0;
            if (xfh_dev_alloc(&d_side, sb) != XFH_OK) throw std::runtime_error("XFgrid: out of device memory");
            side_cap = sb;
        }
        const void* dimg = nullptr;
        if (depth && depth_type != XFH_DEPTH_NONE) {
            if (cam.height <= 0 || depth_pitch == 0) throw std::runtime_error("XFgrid::buildFromRecord: depth image without a size");
            const size_t ib = (size_t)cam.height * depth_pitch;
            if (ib > img_cap) {
                if (d_img) xfh_dev_free(d_img);
                d_img = nullptr; img_cap = 0;
                if (xfh_dev_alloc(&d_img, ib) != XFH_OK) throw std::runtime_error("XFgrid: out of device memory");
                img_cap = ib;
            }
            // (the copy is synchronous: an earlier launch that read the buffer is ordered before it only after a host wait)
            if (xfh_synchronize(ctx) != XFH_OK || xfh_memcpy_h2d(d_img, depth, ib) != XFH_OK) throw std::runtime_error("XFgrid::buildFromRecord: upload failed");
            dimg = d_img;
        }
        side_n = nfeatures;
        finish(xfh_frame_finish_records_device(ctx, d_record, 1, &cam, dimg, dimg ? depth_type : XFH_DEPTH_NONE, depth_pitch, depth_scale, &bounds, flags,
                                               deviceKeysUn(), deviceURight(), deviceDepth(), d_grid),
               nfeatures, bounds);
        host_x.clear(); host_y.clear(); side_host = false;
    }
    const void* device() const { return d_grid; }
    // the coordinates the grid was built from as (x, y) pairs, on the host (a keypoint the grid dropped reads 0, 0 when the grid came from a record)
    void keysXY(std::vector<float>& xy) {
        unpack();
        xy.resize(2 * (size_t)(n > 0 ? n : 0));
        for (int i = 0; i < n; ++i) { xy[2 * (size_t)i] = host_x[i]; xy[2 * (size_t)i + 1] = host_y[i]; }
    }
    int size() const { return n; }
    // device arrays of the last buildFromRecord(.., cam, ..): xy_un[n][2], uright[n], depth[n] (nullptr before it)
    float* deviceKeysUn() const { return (float*)d_side; }
    float* deviceURight() const { return d_side ? (float*)d_side + 2 * (size_t)side_n : nullptr; }
    float* deviceDepth() const { return d_side ? (float*)d_side + 3 * (size_t)side_n : nullptr; }
    // host copies: mvKeysUn as (x, y) pairs, mvuRight, mvDepth
    const std::vector<float>& keysUn() { fetch_side(); return h_xy; }
    const std::vector<float>& uRight() { fetch_side(); return h_ur; }
    const std::vector<float>& depth() { fetch_side(); return h_dz; }

    // Frame::GetFeaturesInArea on the host copy (downloaded and unpacked at the first call after a build): indices in the
    // reference's visiting order
    std::vector<size_t> featuresInArea(float u, float v, float r) {
        std::vector<size_t> out;
        if (!d_grid) return out;
        unpack();
        if (!(std::isfinite(u) && std::isfinite(v) && std::isfinite(r))) return out;
        const float inv_w = (float)XFH_GRID_COLS / (b.max_x - b.min_x), inv_h = (float)XFH_GRID_ROWS / (b.max_y - b.min_y);
        auto sat = [](float f, int hi) { return (int)std::fmin(std::fmax(f, -1.0f), (float)hi); };
        const int c0x = std::max(0, sat(std::floor((u - b.min_x - r) * inv_w), XFH_GRID_COLS));
        if (c0x >= XFH_GRID_COLS) return out;
        const int c1x = std::min(XFH_GRID_COLS - 1, sat(std::ceil((u - b.min_x + r) * inv_w), XFH_GRID_COLS));
        if (c1x < 0) return out;
        const int c0y = std::max(0, sat(std::floor((v - b.min_y - r) * inv_h), XFH_GRID_ROWS));
        if (c0y >= XFH_GRID_ROWS) return out;
        const int c1y = std::min(XFH_GRID_ROWS - 1, sat(std::ceil((v - b.min_y + r) * inv_h), XFH_GRID_ROWS));
        if (c1y < 0) return out;
        for (int ix = c0x; ix <= c1x; ++ix)
            for (int p = cell_start[ix * XFH_GRID_ROWS + c0y]; c1y >= c0y && p < cell_start[ix * XFH_GRID_ROWS + c1y + 1]; ++p) {
                const int k = items[p];
                if (std::fabs(host_x[k] - u) < r && std::fabs(host_y[k] - v) < r) out.push_back((size_t)k);
            }
        return out;
    }

private:
    void reserve(int count, bool with_kps) {
        const size_t gb = xfh_grid_bytes(count), kb = (size_t)(count > 0 ? count : 1) * sizeof(xfh_keypoint);
        if (gb > grid_cap) {
            if (d_grid) xfh_dev_free(d_grid);
            d_grid = nullptr; grid_cap = 0;
            if (xfh_dev_alloc(&d_grid, gb) != XFH_OK) throw std::runtime_error("XFgrid: out of device memory");
            grid_cap = gb;
        }
        if (with_kps && kb > kps_cap) {
            if (d_kps) xfh_dev_free(d_kps);
            d_kps = nullptr; kps_cap = 0;
            if (xfh_dev_alloc(&d_kps, kb) != XFH_OK) throw std::runtime_error("XFgrid: out of device memory");
            kps_cap = kb;
        }
    }
    void finish(int rc, int count, const xfh_grid_bounds& bounds) {
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFgrid: ") + xfh_strerror(rc));
        n = count; b = bounds; unpacked = false;
    }
    void unpack() {
        if (unpacked) return;
        std::vector<unsigned char> blob(xfh_grid_bytes(n));
        int rc = xfh_synchronize(ctx);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(blob.data(), d_grid, blob.size());
        cell_start.assign(XFH_GRID_COLS * XFH_GRID_ROWS + 1, 0); items.assign(n > 0 ? n : 1, -1);
        int nb = 0;
        if (rc == XFH_OK) rc = xfh_grid_unpack(blob.data(), blob.size(), n, cell_start.data(), items.data(), &nb);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFgrid::featuresInArea: ") + xfh_strerror(rc));
        if (host_x.empty() && n > 0) {                      // built from a record: the coordinates travel in the blob's items (slot, x, y, pad)
            host_x.assign(n, 0.f); host_y.assign(n, 0.f);
            for (int p = 0; p < nb; ++p) {
                float xy[2];
                memcpy(xy, blob.data() + (blob.size() - (size_t)n * 16) + (size_t)p * 16 + 4, 8);
                host_x[items[p]] = xy[0]; host_y[items[p]] = xy[1];
            }
        }
        unpacked = true;
    }
    void fetch_side() {
        if (side_host) return;
        if (!d_side || side_n != n) throw std::runtime_error("XFgrid: the grid was not built with a camera");
        h_xy.assign(2 * (size_t)n, 0.f); h_ur.assign(n, 0.f); h_dz.assign(n, 0.f);
        int rc = xfh_synchronize(ctx);
        if (rc == XFH_OK && n > 0) rc = xfh_memcpy_d2h(h_xy.data(), deviceKeysUn(), (size_t)n * 8);
        if (rc == XFH_OK && n > 0) rc = xfh_memcpy_d2h(h_ur.data(), deviceURight(), (size_t)n * 4);
        if (rc == XFH_OK && n > 0) rc = xfh_memcpy_d2h(h_dz.data(), deviceDepth(), (size_t)n * 4);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFgrid: ") + xfh_strerror(rc));
        side_host = true;
    }
    xfh_ctx* ctx;
    void* d_side = nullptr; size_t side_cap = 0; int side_n = 0;      // xy_un, uright, depth of buildFromRecord(.., cam, ..)
    void* d_img = nullptr; size_t img_cap = 0;                        // its depth image
    bool side_host = false;
    std::vector<float> h_xy, h_ur, h_dz;
    void* d_grid = nullptr; size_t grid_cap = 0;
    void* d_kps = nullptr; size_t kps_cap = 0;
    int n = 0;
    xfh_grid_bounds b = {0.f, 0.f, 1.f, 1.f};
    bool unpacked = false;
    std::vector<int> cell_start, items;
    std::vector<float> host_x, host_y;
};

// What XFmatcher::triangulate reads of a keyframe.  keysUn = mvKeysUn as (x, y) pairs, keys = mvKeys[i].pt likewise (nullptr: the camera has no
// distortion, keysUn is read), uright = mvuRight and depth = mvDepth (both nullptr: a monocular keyframe), Tcw = GetPose() row-major 3x4, Ow =
// GetCameraCenter().  Host form: pointers to host arrays of n (2n) floats; device form: device pointers, and for the neighbours of one call the
// arrays of all B keyframes one behind the other (Tcw [B][12], Ow [B][3]).
struct XFtriKeyFrame { const float* keysUn; const float* keys; const float* uright; const float* depth; const float* Tcw; const float* Ow; };
// One new map point of LocalMapping::CreateNewMapPoints: the caller runs :694-709 on it (new MapPoint(x3D, ..), AddObservation(KF1, idx1),
// AddObservation(neighbour's keyframe, idx2), AddMapPoint on both).  normal / minDistance / maxDistance are what UpdateNormalAndDepth would store;
// fuseDistances is the triple xfh_fuse_search_device reads (0.8f * min, 1.2f * max, max).
struct XFnewMapPoint { int idx1, neighbour, idx2; float x3D[3], normal[3], minDistance, maxDistance, fuseDistances[3]; bool stereo; };

class XFmatcher {
public:
    using Mat = xfeat::cvx::Mat;
    using DMatch = xfeat::cvx::DMatch;

    static constexpr int TH_HIGH = 1000;   // ORBmatcher.cc:34, USE_ORB unset
    static constexpr int TH_LOW = 100;     // ORBmatcher.cc:35

    explicit XFmatcher(xfh_ctx* shared_ctx, float nnratio = 0.6f, bool checkOri = true)
        : mfNNratio(nnratio), mbCheckOrientation(checkOri), ctx(shared_ctx) {}

    // stateless and thread-safe like the reference's static member
    static int DescriptorDistance(const Mat& a, const Mat& b) {
        return xfh_descriptor_distance(a.template ptr<float>(0), b.template ptr<float>(0));
    }

    // mutual-nearest-neighbour cosine matching on the GPU
    void match(const Mat& _frame1_desc, const Mat& _frame2_desc, std::vector<DMatch>& _matches, float min_cossim = -1.f) {
        const int n1 = _frame1_desc.rows, n2 = _frame2_desc.rows;
        _matches.clear();
        if (n1 == 0 || n2 == 0) return;
        const int nm = n1 < n2 ? n1 : n2;
        i1.resize(nm); i2.resize(nm); d.resize(nm);
        int n = 0;
        const int rc = xfh_match_mnn(ctx, _frame1_desc.template ptr<float>(0), n1, _frame2_desc.template ptr<float>(0), n2,
                                     min_cossim, i1.data(), i2.data(), d.data(), &n);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFmatcher::match: ") + xfh_strerror(rc));
        _matches.reserve(n);
        for (int k = 0; k < n; ++k) _matches.emplace_back(DMatch(i1[k], i2[k], d[k]));   // :401
    }

    // The same match on two PREPARED images in device memory (XFextractor::extractBatchDevice with d_images, or
    // xfh_match_prepare_device): the tracker's frame-to-frame match without a normalisation pass, two kernel launches.  n1 / n2 =
    // rows the images were made from (nfeatures for images written by the extraction).  Blocks until the result is on the host.
    void matchPrepared(const void* d_image1, int n1, const void* d_image2, int n2, std::vector<DMatch>& _matches, float min_cossim = -1.f) {
        _matches.clear();
        if (n1 <= 0 || n2 <= 0) return;
        const int nm = n1 < n2 ? n1 : n2;
        const size_t bytes = (size_t)nm * 12 + 16;
        if (bytes > d_out_bytes) {
            if (d_out) xfh_dev_free(d_out);
            d_out = nullptr; d_out_bytes = 0;
            if (xfh_dev_alloc(&d_out, bytes) != XFH_OK) throw std::runtime_error("XFmatcher::matchPrepared: out of device memory");
            d_out_bytes = bytes;
        }
        char* o = (char*)d_out;
        int rc = xfh_match_mnn_prepared_device(ctx, d_image1, n1, d_image2, n2, min_cossim, (int*)o, (int*)(o + 4 * (size_t)nm), (float*)(o + 8 * (size_t)nm),
                                               (int*)(o + 12 * (size_t)nm));
        if (rc == XFH_OK) rc = xfh_synchronize(ctx);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFmatcher::matchPrepared: ") + xfh_strerror(rc));
        int n = 0;
        xfh_memcpy_d2h(&n, o + 12 * (size_t)nm, 4);
        if (n < 0 || n > nm) throw std::runtime_error("XFmatcher::matchPrepared: the device reported a collector time-out (n_matches < 0)");
        i1.resize(nm); i2.resize(nm); d.resize(nm);
        if (n > 0) { xfh_memcpy_d2h(i1.data(), o, 4 * (size_t)n); xfh_memcpy_d2h(i2.data(), o + 4 * (size_t)nm, 4 * (size_t)n); xfh_memcpy_d2h(d.data(), o + 8 * (size_t)nm, 4 * (size_t)n); }
        _matches.reserve(n);
        for (int k = 0; k < n; ++k) _matches.emplace_back(DMatch(i1[k], i2[k], d[k]));
    }
    // One frame against several partners in ONE call (the tracker's frame against previous frame / key frames / loop candidates; the reference
    // calls match() once per pair, ORBmatcher.cc:358-372): xfh_match_mnn_prepared_batch_device -- one persistent GEMM launch over the tiles of
    // all pairs + one launch for the mutual check and the output.  _matches[p] = what matchPrepared(d_image1, n1, d_images2[p], n2[p]) gives.
    void matchPreparedMany(const void* d_image1, int n1, const std::vector<const void*>& d_images2, const std::vector<int>& n2,
                           std::vector<std::vector<DMatch>>& _matches, float min_cossim = -1.f) {
        const int P = (int)d_images2.size();
        _matches.assign(P, std::vector<DMatch>());
        if (P == 0 || n1 <= 0) return;
        std::vector<size_t> off(P + 1, 0);
        std::vector<int> nm(P);
        for (int p = 0; p < P; ++p) { nm[p] = n2[p] <= 0 ? 1 : (n1 < n2[p] ? n1 : n2[p]); off[p + 1] = off[p] + (((size_t)nm[p] * 12 + 63) & ~(size_t)63); }
        const size_t bytes = off[P] + (size_t)P * 4 + 64;
        if (bytes > d_out_bytes) {
            if (d_out) xfh_dev_free(d_out);
            d_out = nullptr; d_out_bytes = 0;
            if (xfh_dev_alloc(&d_out, bytes) != XFH_OK) throw std::runtime_error("XFmatcher::matchPreparedMany: out of device memory");
            d_out_bytes = bytes;
        }
        char* o = (char*)d_out;
        std::vector<const void*> a1(P, d_image1);
        std::vector<int> vn1(P, n1);
        std::vector<int*> p1(P), p2(P); std::vector<float*> pd(P);
        for (int p = 0; p < P; ++p) { p1[p] = (int*)(o + off[p]); p2[p] = (int*)(o + off[p] + 4 * (size_t)nm[p]); pd[p] = (float*)(o + off[p] + 8 * (size_t)nm[p]); }
        int* d_cnt = (int*)(o + off[P]);
        int rc = xfh_match_mnn_prepared_batch_device(ctx, P, a1.data(), vn1.data(), d_images2.data(), n2.data(), min_cossim, p1.data(), p2.data(), pd.data(), d_cnt);
        if (rc == XFH_OK) rc = xfh_synchronize(ctx);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFmatcher::matchPreparedMany: ") + xfh_strerror(rc));
        std::vector<int> cnt(P, 0);
        xfh_memcpy_d2h(cnt.data(), d_cnt, (size_t)P * 4);
        for (int p = 0; p < P; ++p) {
            const int n = cnt[p];
            if (n < 0 || n > nm[p]) throw std::runtime_error("XFmatcher::matchPreparedMany: the device reported a collector time-out (n_matches < 0)");
            i1.resize(n); i2.resize(n); d.resize(n);
            if (n > 0) { xfh_memcpy_d2h(i1.data(), p1[p], 4 * (size_t)n); xfh_memcpy_d2h(i2.data(), p2[p], 4 * (size_t)n); xfh_memcpy_d2h(d.data(), pd[p], 4 * (size_t)n); }
            _matches[p].reserve(n);
            for (int k = 0; k < n; ++k) _matches[p].emplace_back(DMatch(i1[k], i2[k], d[k]));
        }
    }
    ~XFmatcher() { if (d_out) xfh_dev_free(d_out); if (d_proj) xfh_dev_free(d_proj); if (d_triang) xfh_dev_free(d_triang); }
    XFmatcher(const XFmatcher&) = delete;
    XFmatcher& operator=(const XFmatcher&) = delete;

    // Guided matching: the inner loop of SearchByProjection / SearchByBoW / SearchForTriangulation / Fuse
    // (ORBmatcher.cc:75-119): best and second-best DescriptorDistance over per-query candidate lists
    // (CSR: offsets[nq+1], indices[]) with the reference's initial value 256 for both.
    void best2(const Mat& queries, const Mat& targets, const std::vector<int>& offsets, const std::vector<int>& indices,
               std::vector<int>& bestIdx, std::vector<int>& bestDist, std::vector<int>& secondIdx, std::vector<int>& secondDist,
               int initDist = 256) {
        const int nq = queries.rows;
        bestIdx.assign(nq, -1); bestDist.assign(nq, initDist); secondIdx.assign(nq, -1); secondDist.assign(nq, initDist);
        if (nq == 0) return;
        const int rc = xfh_best2_csr(ctx, queries.template ptr<float>(0), nq, targets.template ptr<float>(0), targets.rows,
                                     offsets.data(), indices.data(), initDist, bestIdx.data(), bestDist.data(), secondIdx.data(), secondDist.data());
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFmatcher::best2: ") + xfh_strerror(rc));
    }

    // The windowed search of SearchByProjection (ORBmatcher.cc:1925-1955 / :82-119) for ALL queries in one call: query q is row q
    // of `queries` at (u, v, r) = uvr[3q .. 3q + 2]; its candidates are the keypoints of `grid` inside the window
    // (Frame::GetFeaturesInArea), minus those with skip[k] != 0 ("already has a map point with observations", :1931-1933) and, when
    // uright / urQuery are given, minus those with uright[k] > 0 && |urQuery[q] - uright[k]| > r (:1935-1941); best / second best
    // DescriptorDistance in visiting order as best2().  nCandidates[q] = candidates that were compared (`if (vIndices2.empty()) continue`).
    // `targets`: the descriptor rows of the grid's frame (rows == grid.size()).  Blocks until the result is on the host.
    void searchWindow(const Mat& queries, const std::vector<float>& uvr, const XFgrid& grid, const Mat& targets,
                      std::vector<int>& bestIdx, std::vector<int>& bestDist, std::vector<int>& secondIdx, std::vector<int>& secondDist,
                      std::vector<int>& nCandidates, int initDist = 256, const std::vector<unsigned char>* skip = nullptr,
                      const std::vector<float>* uright = nullptr, const std::vector<float>* urQuery = nullptr) {
        const int nq = queries.rows, nt = targets.rows;
        bestIdx.assign(nq, -1); bestDist.assign(nq, initDist); secondIdx.assign(nq, -1); secondDist.assign(nq, initDist); nCandidates.assign(nq, 0);
        if (nq == 0) return;
        if ((int)uvr.size() != 3 * nq || nt != grid.size() || (skip && (int)skip->size() != nt) || (uright && (int)uright->size() != nt) ||
            (urQuery && (int)urQuery->size() != nq) || ((uright != nullptr) != (urQuery != nullptr)))
            throw std::runtime_error("XFmatcher::searchWindow: sizes do not fit");
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t bq = al((size_t)nq * 256), bu = al((size_t)nq * 12), bt = al((size_t)nt * 256 + 16), bs = al((size_t)nt + 16), bf = al((size_t)nt * 4 + 16), bn = al((size_t)nq * 4);
        const size_t bytes = bq + bu + bt + bs + bf + 6 * bn;
        if (bytes > d_out_bytes) {
            if (d_out) xfh_dev_free(d_out);
            d_out = nullptr; d_out_bytes = 0;
            if (xfh_dev_alloc(&d_out, bytes) != XFH_OK) throw std::runtime_error("XFmatcher::searchWindow: out of device memory");
            d_out_bytes = bytes;
        }
        char* p = (char*)d_out;
        float* dq = (float*)p; p += bq; float* du = (float*)p; p += bu; float* dt = (float*)p; p += bt; unsigned char* ds = (unsigned char*)p; p += bs;
        float* dr = (float*)p; p += bf; float* dz = (float*)p; p += bn;
        int* o[5];
        for (int k = 0; k < 5; ++k) { o[k] = (int*)p; p += bn; }
        int rc = xfh_memcpy_h2d(dq, queries.template ptr<float>(0), (size_t)nq * 256);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(du, uvr.data(), (size_t)nq * 12);
        if (rc == XFH_OK && nt > 0) rc = xfh_memcpy_h2d(dt, targets.template ptr<float>(0), (size_t)nt * 256);
        if (rc == XFH_OK && skip && nt > 0) rc = xfh_memcpy_h2d(ds, skip->data(), (size_t)nt);
        if (rc == XFH_OK && uright && nt > 0) rc = xfh_memcpy_h2d(dr, uright->data(), (size_t)nt * 4);
        if (rc == XFH_OK && urQuery) rc = xfh_memcpy_h2d(dz, urQuery->data(), (size_t)nq * 4);
        if (rc == XFH_OK) rc = xfh_search_window_device(ctx, dq, du, nq, grid.device(), dt, nt, skip ? ds : nullptr, uright ? dr : nullptr, urQuery ? dz : nullptr,
                                                        initDist, o[0], o[1], o[2], o[3], o[4]);
        if (rc == XFH_OK) rc = xfh_synchronize(ctx);
        int* out[5] = {bestIdx.data(), bestDist.data(), secondIdx.data(), secondDist.data(), nCandidates.data()};
        for (int k = 0; k < 5 && rc == XFH_OK; ++k) rc = xfh_memcpy_d2h(out[k], o[k], (size_t)nq * 4);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFmatcher::searchWindow: ") + xfh_strerror(rc));
    }

    // ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono) (ORBmatcher.cc:1861-2047) as ONE call
    // (xfh_search_projection_device): query q is row q of `queries` (the map point's descriptor) with world position
    // worldPoints[3q .. 3q + 2] and flags[q] (XFH_PROJ_FLAG_ACTIVE: pMP != NULL && !mvbOutlier; XFH_PROJ_FLAG_CLAIMS:
    // pMP->Observations() > 0); Tcw is the row-major 3x4 [R|t] of CurrentFrame.GetPose(); `grid` / `targets` are the current frame's
    // grid and descriptor rows; skip / uright as in searchWindow (skip: entries of mvpMapPoints that were set BEFORE the call).
    // The queries are processed in index order with the reference's claim rule: matchOfQuery[q] = the keypoint query q wrote
    // (mvpMapPoints[bestIdx2] = pMP, :1957) or -1, assignedQuery[k] = the query that holds mvpMapPoints[k] after the loop or -1 (the
    // last writer wins), and the return value is nmatches.  nnRatio > 0 selects the SearchLocalPoints acceptance rule (:122-127).
    // status / bestDist / secondDist / nCandidates of the last call stay readable in lastStatus() etc.  Blocks until the result is
    // on the host.
    int searchByProjection(const Mat& queries, const std::vector<float>& worldPoints, const std::vector<unsigned char>& flags, const float* Tcw,
                           const xfh_camera& cam, const xfh_grid_bounds& bounds, float th, const XFgrid& grid, const Mat& targets,
                           std::vector<int>& matchOfQuery, std::vector<int>& assignedQuery, const std::vector<unsigned char>* skip = nullptr,
                           const std::vector<float>* uright = nullptr, int initDist = 256, float nnRatio = 0.f, int thHigh = TH_HIGH) {
        const int nq = queries.rows, nt = targets.rows;
        matchOfQuery.assign(nq, -1); assignedQuery.assign(nt, -1);
        if (nq == 0 || nt == 0) return 0;
        if ((int)worldPoints.size() != 3 * nq || (int)flags.size() != nq || nt != grid.size() || (skip && (int)skip->size() != nt) ||
            (uright && (int)uright->size() != nt) || !Tcw)
            throw std::runtime_error("XFmatcher::searchByProjection: sizes do not fit");
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t bq = al((size_t)nq * 256), bp = al((size_t)nq * 12), bfl = al((size_t)nq), bT = 256, bt = al((size_t)nt * 256), bs = al((size_t)nt), bf = al((size_t)nt * 4);
        reserve(d_out, d_out_bytes, bq + bp + bfl + bT + bt + bs + bf, "XFmatcher::searchByProjection");
        char* p = (char*)d_out;
        float* dq = (float*)p; p += bq; float* dp = (float*)p; p += bp; unsigned char* dfl = (unsigned char*)p; p += bfl; float* dT = (float*)p; p += bT;
        float* dt = (float*)p; p += bt; unsigned char* ds = (unsigned char*)p; p += bs; float* dr = (float*)p;
        int rc = xfh_synchronize(ctx);                       // (the copies below are synchronous: nothing queued earlier may still read the buffer)
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dq, queries.template ptr<float>(0), (size_t)nq * 256);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dp, worldPoints.data(), (size_t)nq * 12);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dfl, flags.data(), (size_t)nq);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dT, Tcw, 48);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dt, targets.template ptr<float>(0), (size_t)nt * 256);
        if (rc == XFH_OK && skip) rc = xfh_memcpy_h2d(ds, skip->data(), (size_t)nt);
        if (rc == XFH_OK && uright) rc = xfh_memcpy_h2d(dr, uright->data(), (size_t)nt * 4);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFmatcher::searchByProjection: ") + xfh_strerror(rc));
        return searchByProjection(XFH_PROJ_POINTS, nq, dp, nullptr, dT, &cam, &bounds, th, dq, dfl, grid, dt, skip ? ds : nullptr, uright ? dr : nullptr,
                                  matchOfQuery, assignedQuery, initDist, nnRatio, thHigh);
    }
    // The same on DEVICE pointers and an XFgrid (a frame finished with XFgrid::buildFromRecord: d_targets = the record's descriptor block,
    // d_uright = grid.deviceURight()).  mode XFH_PROJ_POINTS: d_points_or_uvr = world points [nq][3], d_Tcw = 12 floats in device memory;
    // mode XFH_PROJ_GIVEN (the SearchLocalPoints form): d_points_or_uvr = (u, v, r) per query from the caller's isInFrustum, d_ur_query
    // with d_uright or neither, nnRatio = mfNNratio.  Only the results travel to the host.
    int searchByProjection(int mode, int nq, const float* d_points_or_uvr, const float* d_ur_query, const float* d_Tcw, const xfh_camera* cam,
                           const xfh_grid_bounds* bounds, float radius, const float* d_queries, const unsigned char* d_flags, const XFgrid& grid,
                           const float* d_targets, const unsigned char* d_skip, const float* d_uright, std::vector<int>& matchOfQuery,
                           std::vector<int>& assignedQuery, int initDist = 256, float nnRatio = 0.f, int thHigh = TH_HIGH) {
        const int nt = grid.size();
        matchOfQuery.assign(nq > 0 ? nq : 0, -1); assignedQuery.assign(nt > 0 ? nt : 0, -1);
        if (nq <= 0 || nt <= 0) return 0;
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t bw = al(xfh_search_projection_workspace_bytes(nq, nt, 1)), bn = al((size_t)nq * 4), ba = al((size_t)nt * 4), bs = al((size_t)nq);
        reserve(d_proj, d_proj_bytes, bw + 4 * bn + ba + bs + 256, "XFmatcher::searchByProjection");
        char* p = (char*)d_proj;
        void* dws = p; p += bw;
        int* o[4];
        for (int k = 0; k < 4; ++k) { o[k] = (int*)p; p += bn; }
        int* das = (int*)p; p += ba; unsigned char* dst = (unsigned char*)p; p += bs; int* dnm = (int*)p;
        int rc = xfh_search_projection_device(ctx, mode, 1, nq, d_points_or_uvr, d_ur_query, d_Tcw, cam, bounds, radius, d_queries, d_flags, grid.device(),
                                              d_targets, 0, nt, d_skip, d_uright, initDist, thHigh, nnRatio, dws, dst, o[0], o[1], o[2], o[3], nullptr, das, dnm);
        if (rc == XFH_OK) rc = xfh_synchronize(ctx);
        projStatus.assign(nq, 0); projBest.assign(nq, 0); projSecond.assign(nq, 0); projCandidates.assign(nq, 0);
        int nmatches = 0;
        int* out[4] = {matchOfQuery.data(), projBest.data(), projSecond.data(), projCandidates.data()};
        for (int k = 0; k < 4 && rc == XFH_OK; ++k) rc = xfh_memcpy_d2h(out[k], o[k], (size_t)nq * 4);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(projStatus.data(), dst, (size_t)nq);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(assignedQuery.data(), das, (size_t)nt * 4);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(&nmatches, dnm, 4);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFmatcher::searchByProjection: ") + xfh_strerror(rc));
        return nmatches;
    }
    // per query, of the last searchByProjection: XFH_PROJ_* status, best / second DescriptorDistance, survivors after the claim skip
    const std::vector<unsigned char>& lastStatus() const { return projStatus; }
    const std::vector<int>& lastBestDist() const { return projBest; }
    const std::vector<int>& lastSecondDist() const { return projSecond; }
    const std::vector<int>& lastCandidates() const { return projCandidates; }

    // The search of ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th) (ORBmatcher.cc:1333-1523; sim3 = true: the form of :1525-1640
    // with Tcw = [R | t/s] and Ow from the caller's decomposition of Scw, :1534-1535 -- no chi-square gates, bestDist starts at INT_MAX) as
    // ONE call (xfh_fuse_search_device).  Query q is map point q: row q of `queries`, world position worldPoints[3q ..], normal
    // normals[3q ..], distances[3q ..] = (GetMinDistanceInvariance(), GetMaxDistanceInvariance(), mfMaxDistance) and flags[q] bit0 =
    // `pMP && !pMP->isBad() && !pMP->IsInKeyFrame(pKF)`.  `grid` / `targets` / uright are the keyframe's (mvKeysUn grid, mDescriptors,
    // mvuRight; uright = nullptr: a monocular keyframe); scaleFactors = mvScaleFactors.  bestIdx[q] is the keypoint the reference's loop
    // would look at when lastFuseStatus()[q] == XFH_FUSE_FUSED; the return value is nFused.  The bookkeeping (:1497-1516 resp.
    // :1622-1636) is the caller's, over q in order.  Blocks until the result is on the host.
    int fuse(const Mat& queries, const std::vector<float>& worldPoints, const std::vector<float>& normals, const std::vector<float>& distances,
             const std::vector<unsigned char>& flags, const float* Tcw, const float* Ow, const xfh_camera& cam, const xfh_grid_bounds& bounds, float th,
             const std::vector<float>& scaleFactors, const XFgrid& grid, const Mat& targets, std::vector<int>& bestIdx,
             const std::vector<float>* uright = nullptr, bool sim3 = false) {
        const int nq = queries.rows, nt = targets.rows;
        bestIdx.assign(nq, -1);
        if (nq == 0 || nt == 0) return 0;
        if ((int)worldPoints.size() != 3 * nq || (int)normals.size() != 3 * nq || (int)distances.size() != 3 * nq || (int)flags.size() != nq || nt != grid.size() ||
            (uright && (int)uright->size() != nt) || !Tcw || !Ow)
            throw std::runtime_error("XFmatcher::fuse: sizes do not fit");
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t bq = al((size_t)nq * 256), bp = al((size_t)nq * 12), bfl = al((size_t)nq), bT = 256, bt = al((size_t)nt * 256), bf = al((size_t)nt * 4);
        reserve(d_out, d_out_bytes, bq + 3 * bp + bfl + 2 * bT + bt + bf, "XFmatcher::fuse");
        char* p = (char*)d_out;
        float* dq = (float*)p; p += bq; float* dp = (float*)p; p += bp; float* dn = (float*)p; p += bp; float* dd = (float*)p; p += bp;
        unsigned char* dfl = (unsigned char*)p; p += bfl; float* dT = (float*)p; p += bT; float* dO = (float*)p; p += bT; float* dt = (float*)p; p += bt; float* dr = (float*)p;
        int rc = xfh_synchronize(ctx);                       // (the copies below are synchronous: nothing queued earlier may still read the buffer)
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dq, queries.template ptr<float>(0), (size_t)nq * 256);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dp, worldPoints.data(), (size_t)nq * 12);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dn, normals.data(), (size_t)nq * 12);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dd, distances.data(), (size_t)nq * 12);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dfl, flags.data(), (size_t)nq);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dT, Tcw, 48);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dO, Ow, 12);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dt, targets.template ptr<float>(0), (size_t)nt * 256);
        if (rc == XFH_OK && uright) rc = xfh_memcpy_h2d(dr, uright->data(), (size_t)nt * 4);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFmatcher::fuse: ") + xfh_strerror(rc));
        return fuse(nq, dp, dn, dd, dq, dfl, dT, dO, cam, bounds, th, scaleFactors, grid, dt, uright ? dr : nullptr, bestIdx, sim3);
    }
    // The same on DEVICE pointers and an XFgrid (a keyframe finished with XFgrid::buildFromRecord: d_targets = the record's descriptor
    // block, d_uright = grid.deviceURight()).  Only the results travel to the host.
    int fuse(int nq, const float* d_points, const float* d_normals, const float* d_distances, const float* d_queries, const unsigned char* d_flags,
             const float* d_Tcw, const float* d_Ow, const xfh_camera& cam, const xfh_grid_bounds& bounds, float th, const std::vector<float>& scaleFactors,
             const XFgrid& grid, const float* d_targets, const float* d_uright, std::vector<int>& bestIdx, bool sim3 = false) {
        const int nt = grid.size(), nl = (int)scaleFactors.size();
        bestIdx.assign(nq > 0 ? nq : 0, -1);
        if (nq <= 0 || nt <= 0) return 0;
        levelTable(scaleFactors, "XFmatcher::fuse");
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t bn = al((size_t)nq * 4), bs = al((size_t)nq);
        reserve(d_proj, d_proj_bytes, 5 * bn + bs + 256, "XFmatcher::fuse");
        char* p = (char*)d_proj;
        int* o[5];
        for (int k = 0; k < 5; ++k) { o[k] = (int*)p; p += bn; }
        unsigned char* dst = (unsigned char*)p; p += bs; int* dnf = (int*)p;
        int rc = xfh_fuse_search_device(ctx, 1, nq, 0, d_points, d_normals, d_distances, d_queries, d_flags, d_Tcw, d_Ow, &cam, &bounds, th, scaleFactors.data(),
                                        fuseRatioMax.data(), nl, grid.device(), d_targets, 0, nt, d_uright, sim3 ? 0 : XFH_FUSE_CHI2, sim3 ? 0x7fffffff : 256, TH_LOW,
                                        dst, o[0], o[1], o[2], o[3], o[4], nullptr, dnf);
        if (rc == XFH_OK) rc = xfh_synchronize(ctx);
        fuseStatus.assign(nq, 0); fuseBest.assign(nq, 0); fuseWindow.assign(nq, 0); fuseTested.assign(nq, 0); fuseLevel.assign(nq, 0);
        int nfused = 0;
        int* out[5] = {bestIdx.data(), fuseBest.data(), fuseWindow.data(), fuseTested.data(), fuseLevel.data()};
        for (int k = 0; k < 5 && rc == XFH_OK; ++k) rc = xfh_memcpy_d2h(out[k], o[k], (size_t)nq * 4);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(fuseStatus.data(), dst, (size_t)nq);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(&nfused, dnf, 4);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFmatcher::fuse: ") + xfh_strerror(rc));
        return nfused;
    }
    // per query, of the last fuse: XFH_FUSE_* status, best DescriptorDistance, window members, candidates compared, predicted level
    const std::vector<unsigned char>& lastFuseStatus() const { return fuseStatus; }
    const std::vector<int>& lastFuseBestDist() const { return fuseBest; }
    const std::vector<int>& lastFuseWindow() const { return fuseWindow; }
    const std::vector<int>& lastFuseTested() const { return fuseTested; }
    const std::vector<int>& lastFuseLevel() const { return fuseLevel; }

    // The map-point forms of SearchByProjection, which claim keypoints in query order (xfh_map_projection_search_device), each as ONE call.
    //   Sim3Form{ratioHamming, withKeyFrames}: ORBmatcher::SearchByProjection(KeyFrame*, Sim3f& Scw, vpPoints, vpMatched, th, ratioHamming)
    //       (ORBmatcher.cc:612-717; withKeyFrames: the form of :719-831 with vpPointsKFs / vpMatchedKF), called from LoopClosing.  Tcw = [R | t/s]
    //       and Ow come from the caller's decomposition of Scw (:621-622).
    //   RelocForm{ORBdist}: ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame*, sAlreadyFound, th, ORBdist) (:2074-2195), called from
    //       Tracking::Relocalization: the candidate keyframe's map points in keypoint order; Tcw / Ow are the frame's pose and camera centre
    //       (:2078-2079).  normals are not read by this form.  mbCheckOrientation stays without effect: every XFeat angle is -1.
    // Query q is map point q of the reference's loop: row q of `queries` (pMP->GetDescriptor()), worldPoints / normals / distances as in fuse(),
    // flags[q] bit0 = `!pMP->isBad() && !spAlreadyFound.count(pMP)` (with `pMP &&` in the relocalisation form).  `grid` / `targets` are the
    // keyframe's resp. the current frame's; taken[k] != 0 where vpMatched[k] resp. mvpMapPoints[k] is set before the call (nullptr: none).
    // matchOfQuery[q] = the keypoint query q claimed or -1; assignedQuery[k] = the query that claimed keypoint k or -1 -- the caller writes
    // vpMatched[k] = vpPoints[assignedQuery[k]] (and vpMatchedKF[k] = vpPointsKFs[assignedQuery[k]]) resp. mvpMapPoints[k]; the return value is
    // nmatches.  Blocks until the result is on the host.
    struct Sim3Form { float ratioHamming = 1.0f; bool withKeyFrames = false; };
    struct RelocForm { int ORBdist = TH_LOW; };
    int searchByProjection(const Sim3Form& form, const Mat& queries, const std::vector<float>& worldPoints, const std::vector<float>& normals,
                           const std::vector<float>& distances, const std::vector<unsigned char>& flags, const float* Tcw, const float* Ow, const xfh_camera& cam,
                           const xfh_grid_bounds& bounds, float th, const std::vector<float>& scaleFactors, const XFgrid& grid, const Mat& targets,
                           std::vector<int>& matchOfQuery, std::vector<int>& assignedQuery, const std::vector<unsigned char>* taken = nullptr) {
        return mapProjectionHost(form.withKeyFrames ? XFH_MAPPROJ_FORM_SIM3_KF : XFH_MAPPROJ_FORM_SIM3, (float)TH_LOW * form.ratioHamming, queries, worldPoints, normals,
                                 distances, flags, Tcw, Ow, cam, bounds, th, scaleFactors, grid, targets, matchOfQuery, assignedQuery, taken);
    }
    int searchByProjection(const RelocForm& form, const Mat& queries, const std::vector<float>& worldPoints, const std::vector<float>& normals,
                           const std::vector<float>& distances, const std::vector<unsigned char>& flags, const float* Tcw, const float* Ow, const xfh_camera& cam,
                           const xfh_grid_bounds& bounds, float th, const std::vector<float>& scaleFactors, const XFgrid& grid, const Mat& targets,
                           std::vector<int>& matchOfQuery, std::vector<int>& assignedQuery, const std::vector<unsigned char>* taken = nullptr) {
        return mapProjectionHost(XFH_MAPPROJ_FORM_RELOC, (float)form.ORBdist, queries, worldPoints, normals, distances, flags, Tcw, Ow, cam, bounds, th, scaleFactors,
                                 grid, targets, matchOfQuery, assignedQuery, taken);
    }
    // The same on DEVICE pointers and an XFgrid (a frame or keyframe finished with XFgrid::buildFromRecord: d_targets = the record's descriptor
    // block).  Only the results travel to the host.
    int searchByProjection(const Sim3Form& form, int nq, const float* d_points, const float* d_normals, const float* d_distances, const float* d_queries,
                           const unsigned char* d_flags, const float* d_Tcw, const float* d_Ow, const xfh_camera& cam, const xfh_grid_bounds& bounds, float th,
                           const std::vector<float>& scaleFactors, const XFgrid& grid, const float* d_targets, const unsigned char* d_taken,
                           std::vector<int>& matchOfQuery, std::vector<int>& assignedQuery) {
        return mapProjection(form.withKeyFrames ? XFH_MAPPROJ_FORM_SIM3_KF : XFH_MAPPROJ_FORM_SIM3, (float)TH_LOW * form.ratioHamming, nq, d_points, d_normals, d_distances,
                             d_queries, d_flags, d_Tcw, d_Ow, cam, bounds, th, scaleFactors, grid, d_targets, d_taken, matchOfQuery, assignedQuery);
    }
    int searchByProjection(const RelocForm& form, int nq, const float* d_points, const float* d_normals, const float* d_distances, const float* d_queries,
                           const unsigned char* d_flags, const float* d_Tcw, const float* d_Ow, const xfh_camera& cam, const xfh_grid_bounds& bounds, float th,
                           const std::vector<float>& scaleFactors, const XFgrid& grid, const float* d_targets, const unsigned char* d_taken,
                           std::vector<int>& matchOfQuery, std::vector<int>& assignedQuery) {
        return mapProjection(XFH_MAPPROJ_FORM_RELOC, (float)form.ORBdist, nq, d_points, d_normals, d_distances, d_queries, d_flags, d_Tcw, d_Ow, cam, bounds, th,
                             scaleFactors, grid, d_targets, d_taken, matchOfQuery, assignedQuery);
    }
    // per query, of the last map-point searchByProjection: XFH_MAPPROJ_* status, best DescriptorDistance, window members, candidates compared
    // when the query's turn came, predicted level
    const std::vector<unsigned char>& lastMapProjectionStatus() const { return mapStatus; }
    const std::vector<int>& lastMapProjectionBestDist() const { return mapBest; }
    const std::vector<int>& lastMapProjectionWindow() const { return mapWindow; }
    const std::vector<int>& lastMapProjectionTested() const { return mapTested; }
    const std::vector<int>& lastMapProjectionLevel() const { return mapLevel; }

    // ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, S12, th) (ORBmatcher.cc:1642-1859; no call site in the reference's LoopClosing.cc) as ONE call
    // (xfh_sim3_search): the map points of
    // each keyframe projected into the other through S21 / S12 and searched, then the agreement step.  Per keyframe: keysUn = mvKeysUn, desc =
    // mDescriptors, and per keypoint i the map point it holds: points[3i ..] = GetWorldPos(), distances[3i ..] = (GetMinDistanceInvariance(),
    // GetMaxDistanceInvariance(), mfMaxDistance), row i of mpDesc = pMP->GetDescriptor(), flags[i] bit0 = `pMP && !vbAlreadyMatched[i] &&
    // !pMP->isBad()` with vbAlreadyMatched as :1662-1675 compute it; Tw = the keyframe's pose (row-major 3x4).  M21 / M12 = the row-major 3x4
    // [s*R | t] of S12.inverse() and S12 (the caller's Sophus).  cam: pKF1's intrinsics serve both directions (:1644-1647).
    // match12[i1] = the keypoint of keyframe 2 or -1: the caller writes vpMatches12[i1] = vpMapPoints2[match12[i1]] (:1852); the return value is
    // nFound.  Blocks until the result is on the host.
    struct Sim3KeyFrame {
        const std::vector<XFgrid::KeyPoint>* keysUn; const Mat* desc; const std::vector<float>* points; const std::vector<float>* distances; const Mat* mpDesc;
        const std::vector<unsigned char>* flags; const float* Tw;
    };
    int searchBySim3(const Sim3KeyFrame& kf1, const Sim3KeyFrame& kf2, const float* M21, const float* M12, const xfh_camera& cam, const xfh_grid_bounds& bounds,
                     float th, const std::vector<float>& scaleFactors, std::vector<int>& match12) {
        const Sim3KeyFrame* kf[2] = {&kf1, &kf2};
        xfh_sim3_side side[2];
        int n[2];
        for (int s = 0; s < 2; ++s) {
            const Sim3KeyFrame& k = *kf[s];
            if (!k.keysUn || !k.desc || !k.points || !k.distances || !k.mpDesc || !k.flags || !k.Tw) throw std::runtime_error("XFmatcher::searchBySim3: a keyframe is incomplete");
            n[s] = (int)k.keysUn->size();
            if (k.desc->rows != n[s] || k.mpDesc->rows != n[s] || (int)k.points->size() != 3 * n[s] || (int)k.distances->size() != 3 * n[s] || (int)k.flags->size() != n[s])
                throw std::runtime_error("XFmatcher::searchBySim3: sizes do not fit");
            sim3Reset(s, n[s]);
        }
        match12.assign(n[0], -1);
        if (n[0] == 0 || n[1] == 0) return 0;
        if (!M21 || !M12) throw std::runtime_error("XFmatcher::searchBySim3: sizes do not fit");
        levelTable(scaleFactors, "XFmatcher::searchBySim3");
        for (int s = 0; s < 2; ++s) {
            const Sim3KeyFrame& k = *kf[s];
            side[s] = xfh_sim3_side{n[s], nullptr, (const xfh_keypoint*)k.keysUn->data(), k.desc->template ptr<float>(0), 0, k.points->data(), k.distances->data(),
                                    k.mpDesc->template ptr<float>(0), k.flags->data(), k.Tw, sim3Status[s].data(), sim3Match[s].data(), sim3Best[s].data(),
                                    sim3Window[s].data(), sim3Tested[s].data(), sim3Level[s].data(), nullptr};
        }
        int nfound = 0;
        const int rc = xfh_sim3_search(ctx, &side[0], &side[1], M21, M12, &cam, &bounds, th, scaleFactors.data(), fuseRatioMax.data(), (int)scaleFactors.size(), TH_HIGH,
                                       match12.data(), &nfound);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFmatcher::searchBySim3: ") + xfh_strerror(rc));
        return nfound;
    }
    // The same on two keyframes that live in device memory: their XFgrids (built from mvKeysUn), the records' descriptor blocks and the map-point
    // arrays, poses and M21 / M12 as device pointers.  Only the results travel back.
    struct Sim3KeyFrameDevice {
        const XFgrid* grid; const float* d_desc; const float* d_points; const float* d_distances; const float* d_mpDesc; const unsigned char* d_flags; const float* d_Tw;
    };
    int searchBySim3(const Sim3KeyFrameDevice& kf1, const Sim3KeyFrameDevice& kf2, const float* d_M21, const float* d_M12, const xfh_camera& cam,
                     const xfh_grid_bounds& bounds, float th, const std::vector<float>& scaleFactors, std::vector<int>& match12) {
        const Sim3KeyFrameDevice* kf[2] = {&kf1, &kf2};
        if (!kf1.grid || !kf2.grid) throw std::runtime_error("XFmatcher::searchBySim3: a keyframe is incomplete");
        const int n[2] = {kf1.grid->size(), kf2.grid->size()};
        for (int s = 0; s < 2; ++s) sim3Reset(s, n[s] > 0 ? n[s] : 0);
        match12.assign(n[0] > 0 ? n[0] : 0, -1);
        if (n[0] <= 0 || n[1] <= 0) return 0;
        levelTable(scaleFactors, "XFmatcher::searchBySim3");
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        size_t total = al((size_t)n[0] * 4) + 256;
        for (int s = 0; s < 2; ++s) total += 5 * al((size_t)n[s] * 4) + al((size_t)n[s]);
        reserve(d_proj, d_proj_bytes, total, "XFmatcher::searchBySim3");
        char* p = (char*)d_proj;
        int* o[2][5]; unsigned char* dst[2];
        xfh_sim3_side side[2];
        for (int s = 0; s < 2; ++s) {
            for (int k = 0; k < 5; ++k) { o[s][k] = (int*)p; p += al((size_t)n[s] * 4); }
            dst[s] = (unsigned char*)p; p += al((size_t)n[s]);
            side[s] = xfh_sim3_side{n[s], kf[s]->grid->device(), nullptr, kf[s]->d_desc, 0, kf[s]->d_points, kf[s]->d_distances, kf[s]->d_mpDesc, kf[s]->d_flags, kf[s]->d_Tw,
                                    dst[s], o[s][0], o[s][1], o[s][2], o[s][3], o[s][4], nullptr};
        }
        int* dm12 = (int*)p; p += al((size_t)n[0] * 4); int* dnf = (int*)p;
        int rc = xfh_sim3_search_device(ctx, 1, 0, &side[0], &side[1], d_M21, d_M12, &cam, &bounds, th, scaleFactors.data(), fuseRatioMax.data(), (int)scaleFactors.size(),
                                        TH_HIGH, dm12, dnf);
        if (rc == XFH_OK) rc = xfh_synchronize(ctx);
        int nfound = 0;
        for (int s = 0; s < 2; ++s) {
            int* out[5] = {sim3Match[s].data(), sim3Best[s].data(), sim3Window[s].data(), sim3Tested[s].data(), sim3Level[s].data()};
            for (int k = 0; k < 5 && rc == XFH_OK; ++k) rc = xfh_memcpy_d2h(out[k], o[s][k], (size_t)n[s] * 4);
            if (rc == XFH_OK) rc = xfh_memcpy_d2h(sim3Status[s].data(), dst[s], (size_t)n[s]);
        }
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(match12.data(), dm12, (size_t)n[0] * 4);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(&nfound, dnf, 4);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFmatcher::searchBySim3: ") + xfh_strerror(rc));
        return nfound;
    }
    // per keypoint of keyframe `side` (1 or 2), of the last searchBySim3: XFH_SIM3_* status, vnMatch1 / vnMatch2, best DescriptorDistance, window
    // members, candidates compared, predicted level
    const std::vector<unsigned char>& lastSim3Status(int side) const { return sim3Status[side == 2]; }
    const std::vector<int>& lastSim3Matches(int side) const { return sim3Match[side == 2]; }
    const std::vector<int>& lastSim3BestDist(int side) const { return sim3Best[side == 2]; }
    const std::vector<int>& lastSim3Window(int side) const { return sim3Window[side == 2]; }
    const std::vector<int>& lastSim3Tested(int side) const { return sim3Tested[side == 2]; }
    const std::vector<int>& lastSim3Level(int side) const { return sim3Level[side == 2]; }

    // ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (ORBmatcher.cc:833-948) as ONE call (xfh_init_search_device)
    // with the reference's retraction order: a later query that is strictly closer takes a keypoint away from an earlier one, whose match is
    // then gone for good.  `queries` = F1.mDescriptors, vbPrevMatched = the window centres as (x, y) pairs, updated in place as :943-945 do;
    // `grid` / `targets` = F2's grid (on mvKeysUn) and F2.mDescriptors; flags: bit0 clear leaves a query out (nullptr: all take part, the
    // reference).  mfNNratio and TH_LOW are the matcher's; the level test and the rotation histogram remove nothing (every XFeat keypoint has
    // octave 0 and angle -1).  The return value is nmatches.  Blocks until the result is on the host.
    int searchForInitialization(const Mat& queries, std::vector<float>& vbPrevMatched, XFgrid& grid, const Mat& targets, std::vector<int>& vnMatches12,
                                int windowSize = 10, const std::vector<unsigned char>* flags = nullptr) {
        const int nq = queries.rows, nt = targets.rows;
        if (nq == 0 || nt == 0) { initReset(nq, nt, vnMatches12); return 0; }
        if ((int)vbPrevMatched.size() != 2 * nq || nt != grid.size() || (flags && (int)flags->size() != nq))
            throw std::runtime_error("XFmatcher::searchForInitialization: sizes do not fit");
        std::vector<float> xy;
        grid.keysXY(xy);
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t bq = al((size_t)nq * 256), bp = al((size_t)nq * 8), bfl = al((size_t)nq), bt = al((size_t)nt * 256), bx = al((size_t)nt * 8);
        reserve(d_out, d_out_bytes, bq + bp + bfl + bt + bx, "XFmatcher::searchForInitialization");
        char* p = (char*)d_out;
        float* dq = (float*)p; p += bq; float* dp = (float*)p; p += bp; unsigned char* dfl = (unsigned char*)p; p += bfl; float* dt = (float*)p; p += bt;
        float* dx = (float*)p;
        int rc = xfh_synchronize(ctx);                       // (the copies below are synchronous: nothing queued earlier may still read the buffer)
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dq, queries.template ptr<float>(0), (size_t)nq * 256);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dp, vbPrevMatched.data(), (size_t)nq * 8);
        if (rc == XFH_OK && flags) rc = xfh_memcpy_h2d(dfl, flags->data(), (size_t)nq);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dt, targets.template ptr<float>(0), (size_t)nt * 256);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dx, xy.data(), (size_t)nt * 8);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFmatcher::searchForInitialization: ") + xfh_strerror(rc));
        const int nmatches = searchForInitialization(nq, dq, dp, flags ? dfl : nullptr, grid, dt, dx, vnMatches12, windowSize);
        if (xfh_memcpy_d2h(vbPrevMatched.data(), dp, (size_t)nq * 8) != XFH_OK) throw std::runtime_error("XFmatcher::searchForInitialization: download failed");
        return nmatches;
    }
    // The same on DEVICE pointers and an XFgrid (F2 finished with XFgrid::buildFromRecord(record, n, camera, ..): d_targets = the record's
    // descriptor block, d_targetXY = grid.deviceKeysUn()).  d_prevMatched [nq][2] is updated in place; with d_targetXY = nullptr it is left
    // as it is.  Only the results travel to the host.
    int searchForInitialization(int nq, const float* d_queries, float* d_prevMatched, const unsigned char* d_flags, const XFgrid& grid, const float* d_targets,
                                const float* d_targetXY, std::vector<int>& vnMatches12, int windowSize = 10) {
        const int nt = grid.size();
        initReset(nq > 0 ? nq : 0, nt > 0 ? nt : 0, vnMatches12);
        if (nq <= 0 || nt <= 0) return 0;
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t bw = al(xfh_init_search_workspace_bytes(nq, nt, 1)), bn = al((size_t)nq * 4), ba = al((size_t)nt * 4), bs = al((size_t)nq);
        if (bw == 0) throw std::runtime_error("XFmatcher::searchForInitialization: sizes out of range");
        reserve(d_proj, d_proj_bytes, bw + 6 * bn + 2 * ba + bs + 256, "XFmatcher::searchForInitialization");
        char* p = (char*)d_proj;
        void* dws = p; p += bw;
        int* o[6];
        for (int k = 0; k < 6; ++k) { o[k] = (int*)p; p += bn; }
        int* d21 = (int*)p; p += ba; int* dmd = (int*)p; p += ba; unsigned char* dst = (unsigned char*)p; p += bs; int* dnm = (int*)p;
        int rc = xfh_init_search_device(ctx, 1, nq, d_queries, d_prevMatched, d_flags, (float)windowSize, grid.device(), d_targets, 0, d_targetXY, nt, TH_LOW,
                                        mfNNratio, dws, dst, o[0], o[1], o[2], o[3], o[4], o[5], d21, dmd, dnm, d_targetXY ? d_prevMatched : nullptr);
        if (rc == XFH_OK) rc = xfh_synchronize(ctx);
        int nmatches = 0;
        int* out[6] = {initClaim.data(), vnMatches12.data(), initBest.data(), initSecond.data(), initWindow.data(), initTested.data()};
        for (int k = 0; k < 6 && rc == XFH_OK; ++k) rc = xfh_memcpy_d2h(out[k], o[k], (size_t)nq * 4);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(initStatus.data(), dst, (size_t)nq);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(initMatches21.data(), d21, (size_t)nt * 4);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(initMatchedDistance.data(), dmd, (size_t)nt * 4);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(&nmatches, dnm, 4);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFmatcher::searchForInitialization: ") + xfh_strerror(rc));
        return nmatches;
    }
    // of the last searchForInitialization.  Per query of F1: XFH_INIT_* status, the keypoint it wrote when its turn came (-1: none; a retracted
    // query keeps it), best / second DescriptorDistance (INT_MAX: none), window members, members compared when its turn came.  Per keypoint of
    // F2: vnMatches21 and vMatchedDistance
    const std::vector<unsigned char>& lastInitStatus() const { return initStatus; }
    const std::vector<int>& lastInitClaim() const { return initClaim; }
    const std::vector<int>& lastInitBestDist() const { return initBest; }
    const std::vector<int>& lastInitSecondDist() const { return initSecond; }
    const std::vector<int>& lastInitWindow() const { return initWindow; }
    const std::vector<int>& lastInitTested() const { return initTested; }
    const std::vector<int>& lastInitMatches21() const { return initMatches21; }
    const std::vector<int>& lastInitMatchedDistance() const { return initMatchedDistance; }

    // ORBmatcher::SearchForTriangulation(pKF1, pKF2, vMatchedPairs, bOnlyStereo, bCoarse) (ORBmatcher.cc:1092-1331; mbCheckOrientation = false as
    // LocalMapping builds the matcher, no second camera) as ONE call (xfh_triangulation_search): every keypoint of KF1 without a map point
    // against the keypoints of KF2 without one that share its vocabulary node, under the epipole radius and the epipolar test.  Per keyframe:
    // desc = mDescriptors, keysUn = mvKeysUn as (x, y) pairs, uright = mvuRight (nullptr: monocular), has[i] != 0 where GetMapPoint(i) is set,
    // nodeOf[i] = the NodeId of keypoint i in mFeatVec (XFH_NODE_NONE: in none).  F12 (row-major, the matrix of Pinhole.cpp:112) and ep (the
    // epipole of :1105) are the caller's, computed once per pair.  scaleFactor0 / levelSigma2_0 = mvScaleFactors[0] / mvLevelSigma2[0] of KF2.
    // vMatchedPairs comes back in ascending idx1 (:1320-1328); the return value is nmatches.  Blocks until the result is on the host.
    int searchForTriangulation(const Mat& desc1, const std::vector<float>& keysUn1, const std::vector<float>* uright1, const std::vector<unsigned char>& has1,
                               const std::vector<uint32_t>& nodeOf1, const Mat& desc2, const std::vector<float>& keysUn2, const std::vector<float>* uright2,
                               const std::vector<unsigned char>& has2, const std::vector<uint32_t>& nodeOf2, const float* F12, const float* ep,
                               std::vector<std::pair<size_t, size_t>>& vMatchedPairs, bool bOnlyStereo = false, bool bCoarse = false, float scaleFactor0 = 1.f,
                               float levelSigma2_0 = 1.f) {
        const int n1 = desc1.rows, n2 = desc2.rows;
        vMatchedPairs.clear();
        triStatus.assign(n1, 0); triMatch.assign(n1, -1); triBest.assign(n1, TH_LOW); triCandidates.assign(n1, 0); triGeom.assign(n1, 0);
        if (n1 == 0 || n2 == 0) return 0;
        if ((int)keysUn1.size() != 2 * n1 || (int)has1.size() != n1 || (int)nodeOf1.size() != n1 || (uright1 && (int)uright1->size() != n1) ||
            (int)keysUn2.size() != 2 * n2 || (int)has2.size() != n2 || (int)nodeOf2.size() != n2 || (uright2 && (int)uright2->size() != n2) || !F12 || !ep)
            throw std::runtime_error("XFmatcher::searchForTriangulation: sizes do not fit");
        int nmatches = 0;
        const int rc = xfh_triangulation_search(ctx, n1, n2, (bOnlyStereo ? XFH_TRI_ONLY_STEREO : 0) | (bCoarse ? XFH_TRI_COARSE : 0), TH_LOW, 100 * scaleFactor0,
                                                levelSigma2_0, nodeOf1.data(), keysUn1.data(), uright1 ? uright1->data() : nullptr, has1.data(),
                                                desc1.template ptr<float>(0), nodeOf2.data(), keysUn2.data(), uright2 ? uright2->data() : nullptr, has2.data(),
                                                desc2.template ptr<float>(0), F12, ep, triStatus.data(), triMatch.data(), triBest.data(), triCandidates.data(),
                                                triGeom.data(), &nmatches);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFmatcher::searchForTriangulation: ") + xfh_strerror(rc));
        return triPairs(vMatchedPairs, nmatches);
    }
    // The same on two keyframes that live in device memory: XFgrids finished with XFgrid::buildFromRecord(record, n, camera, ..) (their
    // deviceKeysUn() / deviceURight() are mvKeysUn / mvuRight), the records' descriptor blocks, and per keyframe a node blob (xfh_nodes_pack,
    // uploaded by the caller) and the has-a-map-point bytes in device memory.  F12 and ep are host arrays.  Only the results travel back.
    int searchForTriangulation(const XFgrid& grid1, const float* d_desc1, const void* d_nodes1, const unsigned char* d_has1, const XFgrid& grid2,
                               const float* d_desc2, const void* d_nodes2, const unsigned char* d_has2, const float* F12, const float* ep,
                               std::vector<std::pair<size_t, size_t>>& vMatchedPairs, bool bOnlyStereo = false, bool bCoarse = false, float scaleFactor0 = 1.f,
                               float levelSigma2_0 = 1.f) {
        const int n1 = grid1.size(), n2 = grid2.size();
        vMatchedPairs.clear();
        triStatus.assign(n1 > 0 ? n1 : 0, 0); triMatch.assign(triStatus.size(), -1); triBest.assign(triStatus.size(), TH_LOW);
        triCandidates.assign(triStatus.size(), 0); triGeom.assign(triStatus.size(), 0);
        if (n1 <= 0 || n2 <= 0) return 0;
        if (!grid1.deviceKeysUn() || !grid2.deviceKeysUn() || !F12 || !ep) throw std::runtime_error("XFmatcher::searchForTriangulation: the grids were not built with a camera");
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t bn = al((size_t)n1 * 4), bs = al((size_t)n1);
        reserve(d_proj, d_proj_bytes, 4 * bn + bs + 3 * 256, "XFmatcher::searchForTriangulation");
        char* p = (char*)d_proj;
        int* o[4];
        for (int k = 0; k < 4; ++k) { o[k] = (int*)p; p += bn; }
        unsigned char* dst = (unsigned char*)p; p += bs; int* dnm = (int*)p; p += 256; float* dF = (float*)p; p += 256; float* de = (float*)p;
        int rc = xfh_synchronize(ctx);                       // (the copies below are synchronous: nothing queued earlier may still read the buffer)
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dF, F12, 36);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(de, ep, 8);
        if (rc == XFH_OK)
            rc = xfh_triangulation_search_device(ctx, 1, n1, n2, 1, (bOnlyStereo ? XFH_TRI_ONLY_STEREO : 0) | (bCoarse ? XFH_TRI_COARSE : 0), TH_LOW, 100 * scaleFactor0,
                                                 levelSigma2_0, d_nodes1, grid1.deviceKeysUn(), grid1.deviceURight(), d_has1, d_desc1, 0, d_nodes2, grid2.deviceKeysUn(),
                                                 grid2.deviceURight(), d_has2, d_desc2, 0, dF, de, dst, o[0], o[1], o[2], o[3], dnm);
        if (rc == XFH_OK) rc = xfh_synchronize(ctx);
        int nmatches = 0;
        int* out[4] = {triMatch.data(), triBest.data(), triCandidates.data(), triGeom.data()};
        for (int k = 0; k < 4 && rc == XFH_OK; ++k) rc = xfh_memcpy_d2h(out[k], o[k], (size_t)n1 * 4);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(triStatus.data(), dst, (size_t)n1);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(&nmatches, dnm, 4);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFmatcher::searchForTriangulation: ") + xfh_strerror(rc));
        return triPairs(vMatchedPairs, nmatches);
    }
    // per keypoint of KF1, of the last searchForTriangulation: XFH_TRI_* status, vMatches12, best DescriptorDistance, the members of KF2's node that
    // were candidates, and those of them that passed the geometry
    const std::vector<unsigned char>& lastTriangulationStatus() const { return triStatus; }
    const std::vector<int>& lastTriangulationMatches() const { return triMatch; }
    const std::vector<int>& lastTriangulationBestDist() const { return triBest; }
    const std::vector<int>& lastTriangulationCandidates() const { return triCandidates; }
    const std::vector<int>& lastTriangulationGeom() const { return triGeom; }

    // The loop body of LocalMapping::CreateNewMapPoints (LocalMapping.cc:481-710) for ALL neighbours of the new keyframe in one call
    // (xfh_triangulate_device with XFH_TRIANG_CLAIM): parallax, triangulation or stereo unprojection, cheirality, reprojection and scale gates, and
    // the reference's rule that the first neighbour that creates a point at a keypoint of KF1 keeps it.  match12 [B][n1] is what the batched
    // searchForTriangulation (xfh_triangulation_search_device, side1_shared = 1) wrote.  levelSigma2_0 = mvLevelSigma2[0], scaleFactor = mfScaleFactor,
    // scaleFactorLast = mvScaleFactors[nLevels - 1], thFarPoints = mThFarPoints (<= 0: mbFarPoints off).  The list comes back in the reference's
    // creation order (neighbour ascending, then idx1).  The device form reads everything where the searches left it and only the list travels back;
    // the points, normals and distance triples also stay on the device for fuse (deviceNewPoints() / deviceNewNormals() / deviceNewDistances()).
    // ComputeDistinctiveDescriptors of a new point is the caller's: with two observations either row is a legal outcome, KF1's is recommended.
    int triangulate(const xfh_camera& cam, int B, int n1, int n2, const XFtriKeyFrame& d_kf1, const XFtriKeyFrame& d_neighbours, const int* d_match12,
                    std::vector<XFnewMapPoint>& vNew, float levelSigma2_0 = 1.f, float scaleFactor = 1.2f, float scaleFactorLast = 1.f, float thFarPoints = 0.f,
                    bool bInertial = false) {
        vNew.clear();
        triangHeader.assign(B > 0 ? (size_t)B * 8 : 0, 0);
        if (B <= 0 || n1 <= 0 || n2 <= 0) return 0;
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t P = (size_t)B * n1, bst = al(P), bx = al(P * 12), bh = al((size_t)B * 32), bi = al((size_t)n1 * 4), bf = al((size_t)n1 * 12);
        reserve(d_triang, d_triang_bytes, 2 * bst + bx + bh + 4 * bi + 3 * bf + 256, "XFmatcher::triangulate");
        char* p = (char*)d_triang;
        unsigned char* dst = (unsigned char*)p; p += bst; unsigned char* dkd = (unsigned char*)p; p += bst; float* dxyz = (float*)p; p += bx; int* dh = (int*)p; p += bh;
        int* di[4];
        for (int k = 0; k < 4; ++k) { di[k] = (int*)p; p += bi; }
        d_new[0] = (float*)p; p += bf; d_new[1] = (float*)p; p += bf; d_new[2] = (float*)p; p += bf; int* dn = (int*)p;
        int rc = xfh_triangulate_device(ctx, B, n1, n2, 1, XFH_TRIANG_CLAIM | (bInertial ? XFH_TRIANG_INERTIAL : 0), &cam, levelSigma2_0, 1.5f * scaleFactor, scaleFactorLast,
                                        thFarPoints, d_kf1.keysUn, d_kf1.keys, d_kf1.uright, d_kf1.depth, d_kf1.Tcw, d_kf1.Ow, d_neighbours.keysUn, d_neighbours.keys,
                                        d_neighbours.uright, d_neighbours.depth, d_neighbours.Tcw, d_neighbours.Ow, d_match12, dst, dkd, dxyz, dh, di[0], di[1], di[2],
                                        di[3], d_new[0], d_new[1], d_new[2], dn);
        if (rc == XFH_OK) rc = xfh_synchronize(ctx);
        int nNew = 0;
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(&nNew, dn, 4);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(triangHeader.data(), dh, (size_t)B * 32);
        std::vector<int> idx[3];
        std::vector<float> f[3];
        std::vector<unsigned char> kind(P);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(kind.data(), dkd, P);
        for (int k = 0; k < 3 && rc == XFH_OK && nNew > 0; ++k) {
            idx[k].resize(nNew); f[k].resize((size_t)nNew * 3);
            rc = xfh_memcpy_d2h(idx[k].data(), di[k + 1], (size_t)nNew * 4);
            if (rc == XFH_OK) rc = xfh_memcpy_d2h(f[k].data(), d_new[k], (size_t)nNew * 12);
        }
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFmatcher::triangulate: ") + xfh_strerror(rc));
        vNew.resize(nNew);
        for (int j = 0; j < nNew; ++j) {
            XFnewMapPoint& q = vNew[j];
            q.idx1 = idx[0][j]; q.neighbour = idx[1][j]; q.idx2 = idx[2][j];
            for (int k = 0; k < 3; ++k) { q.x3D[k] = f[0][3 * j + k]; q.normal[k] = f[1][3 * j + k]; q.fuseDistances[k] = f[2][3 * j + k]; }
            q.maxDistance = q.fuseDistances[2]; q.minDistance = q.maxDistance / scaleFactorLast;
            q.stereo = kind[(size_t)q.neighbour * n1 + q.idx1] != 0;
        }
        nTriangNew = nNew;
        return nNew;
    }
    // The same on host containers: kf1 and each of the B neighbours (all with n2 keypoints) as host arrays, match12 [B][n1] on the host.
    int triangulate(const xfh_camera& cam, int n1, int n2, const XFtriKeyFrame& kf1, const std::vector<XFtriKeyFrame>& neighbours, const std::vector<int>& match12,
                    std::vector<XFnewMapPoint>& vNew, float levelSigma2_0 = 1.f, float scaleFactor = 1.2f, float scaleFactorLast = 1.f, float thFarPoints = 0.f,
                    bool bInertial = false) {
        const int B = (int)neighbours.size();
        vNew.clear();
        if (B == 0 || n1 <= 0 || n2 <= 0) return 0;
        if ((int)match12.size() != B * n1 || !kf1.keysUn || !kf1.Tcw || !kf1.Ow) throw std::runtime_error("XFmatcher::triangulate: sizes do not fit");
        const bool raw = neighbours[0].keys != nullptr, st = neighbours[0].uright != nullptr;
        std::vector<float> xy((size_t)B * n2 * 2), xr(raw ? xy.size() : 0), ur(st ? (size_t)B * n2 : 0), z(ur.size()), T((size_t)B * 12), O((size_t)B * 3);
        for (int b = 0; b < B; ++b) {
            const XFtriKeyFrame& k = neighbours[b];
            if (!k.keysUn || !k.Tcw || !k.Ow || (k.keys != nullptr) != raw || (k.uright != nullptr) != st || (st && !k.depth))
                throw std::runtime_error("XFmatcher::triangulate: the neighbours must name the same arrays");
            std::copy(k.keysUn, k.keysUn + 2 * n2, xy.begin() + (size_t)b * n2 * 2);
            if (raw) std::copy(k.keys, k.keys + 2 * n2, xr.begin() + (size_t)b * n2 * 2);
            if (st) { std::copy(k.uright, k.uright + n2, ur.begin() + (size_t)b * n2); std::copy(k.depth, k.depth + n2, z.begin() + (size_t)b * n2); }
            std::copy(k.Tcw, k.Tcw + 12, T.begin() + (size_t)b * 12); std::copy(k.Ow, k.Ow + 3, O.begin() + (size_t)b * 3);
        }
        const size_t P = (size_t)B * n1;
        std::vector<unsigned char> status(P), kind(P);
        std::vector<float> xyz(P * 3), nx((size_t)n1 * 3), nn((size_t)n1 * 3), nd((size_t)n1 * 3);
        std::vector<int> winner(n1), i1v(n1), bv(n1), i2v(n1);
        triangHeader.assign((size_t)B * 8, 0);
        int nNew = 0;
        const int rc = xfh_triangulate(ctx, B, n1, n2, XFH_TRIANG_CLAIM | (bInertial ? XFH_TRIANG_INERTIAL : 0), &cam, levelSigma2_0, 1.5f * scaleFactor, scaleFactorLast,
                                       thFarPoints, kf1.keysUn, kf1.keys, kf1.uright, kf1.depth, kf1.Tcw, kf1.Ow, xy.data(), raw ? xr.data() : nullptr, st ? ur.data() : nullptr,
                                       st ? z.data() : nullptr, T.data(), O.data(), match12.data(), status.data(), kind.data(), xyz.data(), triangHeader.data(), winner.data(),
                                       i1v.data(), bv.data(), i2v.data(), nx.data(), nn.data(), nd.data(), &nNew);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFmatcher::triangulate: ") + xfh_strerror(rc));
        vNew.resize(nNew);
        for (int j = 0; j < nNew; ++j) {
            XFnewMapPoint& q = vNew[j];
            q.idx1 = i1v[j]; q.neighbour = bv[j]; q.idx2 = i2v[j];
            for (int k = 0; k < 3; ++k) { q.x3D[k] = nx[3 * j + k]; q.normal[k] = nn[3 * j + k]; q.fuseDistances[k] = nd[3 * j + k]; }
            q.maxDistance = q.fuseDistances[2]; q.minDistance = q.maxDistance / scaleFactorLast;
            q.stereo = kind[(size_t)q.neighbour * n1 + q.idx1] != 0;
        }
        nTriangNew = nNew;
        return nNew;
    }
    // of the last triangulate: per neighbour the eight counts of xfh_triangulate_device (matched, triangulation attempts, stereo attempts, accepted, new,
    // new stereo (countStereo), superseded, 0); and of its device form the new points in device memory, nTriangNew rows each, as fuse takes them
    const std::vector<int>& lastTriangulateHeader() const { return triangHeader; }
    const float* deviceNewPoints() const { return d_new[0]; }
    const float* deviceNewNormals() const { return d_new[1]; }
    const float* deviceNewDistances() const { return d_new[2]; }
    int lastTriangulateCount() const { return nTriangNew; }

    // ORBmatcher::SearchByBoW, both overloads (ORBmatcher.cc:408-610 and :950-1090; no second camera; the rotation histogram removes nothing
    // because every XFeat angle is -1, so mbCheckOrientation stays without effect) as ONE call (xfh_bow_search).  Side 1 is the keyframe whose
    // map points are matched: desc1 = mDescriptors, nodeOf1[i] = the NodeId of keypoint i in mFeatVec (XFH_NODE_NONE: in none), active1[i] != 0
    // where its map point i exists and is not bad.  Side 2 is the frame (keyframeForm = false: eligible2 is not read and may be empty,
    // `bestDist1 <= TH_LOW`) or the second keyframe (keyframeForm = true: eligible2[k] != 0 where ITS map point k exists and is not bad,
    // `bestDist1 < TH_LOW`).  mfNNratio is the matcher's.  matchOfQuery[i] = the keypoint of side 2 matched to keypoint i of side 1 or -1
    // (vpMatches12 by index), assignedQuery[k] = the keypoint of side 1 that claimed keypoint k of side 2 or -1 (vpMapPointMatches[k] =
    // vpMapPointsKF[assignedQuery[k]]); the return value is nmatches.  Blocks until the result is on the host.
    int searchByBoW(const Mat& desc1, const std::vector<uint32_t>& nodeOf1, const std::vector<unsigned char>& active1, const Mat& desc2,
                    const std::vector<uint32_t>& nodeOf2, const std::vector<unsigned char>& eligible2, bool keyframeForm, std::vector<int>& matchOfQuery,
                    std::vector<int>& assignedQuery) {
        const int n1 = desc1.rows, n2 = desc2.rows;
        bowReset(n1, n2, matchOfQuery, assignedQuery);
        if (n1 == 0 || n2 == 0) return 0;
        if ((int)nodeOf1.size() != n1 || (int)active1.size() != n1 || (int)nodeOf2.size() != n2 || (keyframeForm && (int)eligible2.size() != n2))
            throw std::runtime_error("XFmatcher::searchByBoW: sizes do not fit");
        int nmatches = 0;
        const int rc = xfh_bow_search(ctx, n1, n2, keyframeForm ? XFH_BOW_STRICT_LOW : 0, 256, TH_LOW, mfNNratio, nodeOf1.data(), active1.data(),
                                      desc1.template ptr<float>(0), nodeOf2.data(), keyframeForm ? eligible2.data() : nullptr, desc2.template ptr<float>(0),
                                      bowStatus.data(), matchOfQuery.data(), bowBest.data(), bowSecond.data(), bowCandidates.data(), assignedQuery.data(), &nmatches);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFmatcher::searchByBoW: ") + xfh_strerror(rc));
        return nmatches;
    }
    // The same on two sides that live in device memory: the descriptor blocks of two records, per side a node blob (xfh_nodes_pack, uploaded by
    // the caller) and the flag bytes (d_eligible2 is not read when keyframeForm is false).  Only the results travel back.
    int searchByBoW(int n1, const float* d_desc1, const void* d_nodes1, const unsigned char* d_active1, int n2, const float* d_desc2, const void* d_nodes2,
                    const unsigned char* d_eligible2, bool keyframeForm, std::vector<int>& matchOfQuery, std::vector<int>& assignedQuery) {
        bowReset(n1 > 0 ? n1 : 0, n2 > 0 ? n2 : 0, matchOfQuery, assignedQuery);
        if (n1 <= 0 || n2 <= 0) return 0;
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t b1 = al((size_t)n1 * 4), b2 = al((size_t)n2 * 4), bs = al((size_t)n1), wsb = al(xfh_bow_search_workspace_bytes(n1, n2, 1));
        if (wsb == 0) throw std::runtime_error("XFmatcher::searchByBoW: sizes out of range");
        reserve(d_proj, d_proj_bytes, wsb + 4 * b1 + b2 + bs + 256, "XFmatcher::searchByBoW");
        char* p = (char*)d_proj;
        void* ws = p; p += wsb;
        int* o[4];
        for (int k = 0; k < 4; ++k) { o[k] = (int*)p; p += b1; }
        int* das = (int*)p; p += b2; unsigned char* dst = (unsigned char*)p; p += bs; int* dnm = (int*)p;
        int rc = xfh_bow_search_device(ctx, 1, n1, n2, 0, keyframeForm ? XFH_BOW_STRICT_LOW : 0, 256, TH_LOW, mfNNratio, d_nodes1, d_active1, d_desc1, 0, d_nodes2,
                                       keyframeForm ? d_eligible2 : nullptr, d_desc2, 0, ws, dst, o[0], o[1], o[2], o[3], das, dnm);
        if (rc == XFH_OK) rc = xfh_synchronize(ctx);
        int nmatches = 0;
        int* out[4] = {matchOfQuery.data(), bowBest.data(), bowSecond.data(), bowCandidates.data()};
        for (int k = 0; k < 4 && rc == XFH_OK; ++k) rc = xfh_memcpy_d2h(out[k], o[k], (size_t)n1 * 4);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(assignedQuery.data(), das, (size_t)n2 * 4);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(bowStatus.data(), dst, (size_t)n1);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(&nmatches, dnm, 4);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFmatcher::searchByBoW: ") + xfh_strerror(rc));
        return nmatches;
    }
    // per keypoint of side 1, of the last searchByBoW: XFH_BOW_* status, best and second-best DescriptorDistance (256 where there is none) and
    // the members of side 2's node that were candidates when the query's turn came
    const std::vector<unsigned char>& lastBoWStatus() const { return bowStatus; }
    const std::vector<int>& lastBoWBestDist() const { return bowBest; }
    const std::vector<int>& lastBoWSecondDist() const { return bowSecond; }
    const std::vector<int>& lastBoWCandidates() const { return bowCandidates; }

    // MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:329-403), batched over map points: group g observes the
    // rows indices[offsets[g] .. offsets[g+1]) of `table`; bestPos[g] = position in the group of the descriptor with
    // the least median DescriptorDistance to the others (-1 for an empty group), bestMedian[g] = that median.
    void distinctive(const Mat& table, const std::vector<int>& offsets, const std::vector<int>& indices,
                     std::vector<int>& bestPos, std::vector<int>& bestMedian) {
        const int ng = offsets.empty() ? 0 : (int)offsets.size() - 1;
        bestPos.assign(ng, -1); bestMedian.assign(ng, 0x7fffffff);
        if (ng == 0) return;
        const int rc = xfh_distinctive_csr(ctx, table.template ptr<float>(0), table.rows, offsets.data(), indices.data(), ng,
                                           bestPos.data(), bestMedian.data());
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFmatcher::distinctive: ") + xfh_strerror(rc));
    }

protected:
    // the level thresholds of this pyramid (xfh_scale_level_thresholds), computed once per pyramid
    void levelTable(const std::vector<float>& scaleFactors, const char* who) {
        const int nl = (int)scaleFactors.size();
        if (nl < 1 || nl > XFH_FUSE_MAX_LEVELS) throw std::runtime_error(std::string(who) + ": 1 .. XFH_FUSE_MAX_LEVELS scale factors");
        if (fuseRatioMax.size() + 1 != (size_t)nl || fuseScale != (nl > 1 ? scaleFactors[1] : 0.f)) {
            fuseRatioMax.assign(nl - 1, 0.f);
            if (nl > 1 && xfh_scale_level_thresholds(scaleFactors[1], nl, fuseRatioMax.data()) != XFH_OK) throw std::runtime_error(std::string(who) + ": scale factor must be > 1");
            fuseScale = nl > 1 ? scaleFactors[1] : 0.f;
        }
    }
    int triPairs(std::vector<std::pair<size_t, size_t>>& vMatchedPairs, int nmatches) const {          // :1320-1328
        vMatchedPairs.reserve(nmatches > 0 ? nmatches : 0);
        for (size_t i = 0; i < triMatch.size(); ++i) if (triMatch[i] >= 0) vMatchedPairs.push_back(std::make_pair(i, (size_t)triMatch[i]));
        return nmatches;
    }
    void sim3Reset(int s, int n) {
        sim3Status[s].assign(n, 0); sim3Match[s].assign(n, -1); sim3Best[s].assign(n, 0x7fffffff); sim3Window[s].assign(n, 0); sim3Tested[s].assign(n, 0);
        sim3Level[s].assign(n, -1);
    }
    int mapProjectionHost(int form, float acceptMax, const Mat& queries, const std::vector<float>& worldPoints, const std::vector<float>& normals,
                          const std::vector<float>& distances, const std::vector<unsigned char>& flags, const float* Tcw, const float* Ow, const xfh_camera& cam,
                          const xfh_grid_bounds& bounds, float th, const std::vector<float>& scaleFactors, const XFgrid& grid, const Mat& targets,
                          std::vector<int>& matchOfQuery, std::vector<int>& assignedQuery, const std::vector<unsigned char>* taken) {
        const int nq = queries.rows, nt = targets.rows;
        matchOfQuery.assign(nq, -1); assignedQuery.assign(nt, -1);
        if (nq == 0 || nt == 0) return 0;
        if ((int)worldPoints.size() != 3 * nq || (int)normals.size() != 3 * nq || (int)distances.size() != 3 * nq || (int)flags.size() != nq || nt != grid.size() ||
            (taken && (int)taken->size() != nt) || !Tcw || !Ow)
            throw std::runtime_error("XFmatcher::searchByProjection: sizes do not fit");
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t bq = al((size_t)nq * 256), bp = al((size_t)nq * 12), bfl = al((size_t)nq), bT = 256, bt = al((size_t)nt * 256), bk = al((size_t)nt);
        reserve(d_out, d_out_bytes, bq + 3 * bp + bfl + 2 * bT + bt + bk, "XFmatcher::searchByProjection");
        char* p = (char*)d_out;
        float* dq = (float*)p; p += bq; float* dp = (float*)p; p += bp; float* dn = (float*)p; p += bp; float* dd = (float*)p; p += bp;
        unsigned char* dfl = (unsigned char*)p; p += bfl; float* dT = (float*)p; p += bT; float* dO = (float*)p; p += bT; float* dt = (float*)p; p += bt;
        unsigned char* dk = (unsigned char*)p;
        int rc = xfh_synchronize(ctx);                       // (the copies below are synchronous: nothing queued earlier may still read the buffer)
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dq, queries.template ptr<float>(0), (size_t)nq * 256);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dp, worldPoints.data(), (size_t)nq * 12);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dn, normals.data(), (size_t)nq * 12);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dd, distances.data(), (size_t)nq * 12);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dfl, flags.data(), (size_t)nq);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dT, Tcw, 48);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dO, Ow, 12);
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(dt, targets.template ptr<float>(0), (size_t)nt * 256);
        if (rc == XFH_OK && taken) rc = xfh_memcpy_h2d(dk, taken->data(), (size_t)nt);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFmatcher::searchByProjection: ") + xfh_strerror(rc));
        return mapProjection(form, acceptMax, nq, dp, dn, dd, dq, dfl, dT, dO, cam, bounds, th, scaleFactors, grid, dt, taken ? dk : nullptr, matchOfQuery, assignedQuery);
    }
    int mapProjection(int form, float acceptMax, int nq, const float* d_points, const float* d_normals, const float* d_distances, const float* d_queries,
                      const unsigned char* d_flags, const float* d_Tcw, const float* d_Ow, const xfh_camera& cam, const xfh_grid_bounds& bounds, float th,
                      const std::vector<float>& scaleFactors, const XFgrid& grid, const float* d_targets, const unsigned char* d_taken, std::vector<int>& matchOfQuery,
                      std::vector<int>& assignedQuery) {
        const int nt = grid.size();
        matchOfQuery.assign(nq > 0 ? nq : 0, -1); assignedQuery.assign(nt > 0 ? nt : 0, -1);
        mapStatus.assign(matchOfQuery.size(), 0); mapBest.assign(matchOfQuery.size(), 256); mapWindow.assign(matchOfQuery.size(), 0);
        mapTested.assign(matchOfQuery.size(), 0); mapLevel.assign(matchOfQuery.size(), -1);
        if (nq <= 0 || nt <= 0) return 0;
        levelTable(scaleFactors, "XFmatcher::searchByProjection");
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t bw = al(xfh_map_projection_search_workspace_bytes(nq, nt, 1)), bn = al((size_t)nq * 4), ba = al((size_t)nt * 4), bs = al((size_t)nq);
        if (bw == 0) throw std::runtime_error("XFmatcher::searchByProjection: sizes out of range");
        reserve(d_proj, d_proj_bytes, bw + 5 * bn + ba + bs + 256, "XFmatcher::searchByProjection");
        char* p = (char*)d_proj;
        void* dws = p; p += bw;
        int* o[5];
        for (int k = 0; k < 5; ++k) { o[k] = (int*)p; p += bn; }
        int* das = (int*)p; p += ba; unsigned char* dst = (unsigned char*)p; p += bs; int* dnm = (int*)p;
        int rc = xfh_map_projection_search_device(ctx, form, 1, nq, d_points, d_normals, d_distances, d_queries, d_flags, d_Tcw, d_Ow, &cam, &bounds, th,
                                                  scaleFactors.data(), fuseRatioMax.data(), (int)scaleFactors.size(), grid.device(), d_targets, 0, 0, nt, d_taken, 256,
                                                  acceptMax, dws, dst, o[0], o[1], o[2], o[3], o[4], nullptr, das, dnm);
        if (rc == XFH_OK) rc = xfh_synchronize(ctx);
        int nmatches = 0;
        int* out[5] = {matchOfQuery.data(), mapBest.data(), mapWindow.data(), mapTested.data(), mapLevel.data()};
        for (int k = 0; k < 5 && rc == XFH_OK; ++k) rc = xfh_memcpy_d2h(out[k], o[k], (size_t)nq * 4);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(mapStatus.data(), dst, (size_t)nq);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(assignedQuery.data(), das, (size_t)nt * 4);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(&nmatches, dnm, 4);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFmatcher::searchByProjection: ") + xfh_strerror(rc));
        return nmatches;
    }
    void initReset(int nq, int nt, std::vector<int>& vnMatches12) {
        vnMatches12.assign(nq, -1);
        initStatus.assign(nq, 0); initClaim.assign(nq, -1); initBest.assign(nq, 0x7fffffff); initSecond.assign(nq, 0x7fffffff); initWindow.assign(nq, 0);
        initTested.assign(nq, 0); initMatches21.assign(nt, -1); initMatchedDistance.assign(nt, 0x7fffffff);
    }
    void bowReset(int n1, int n2, std::vector<int>& matchOfQuery, std::vector<int>& assignedQuery) {
        matchOfQuery.assign(n1, -1); assignedQuery.assign(n2, -1);
        bowStatus.assign(n1, 0); bowBest.assign(n1, 256); bowSecond.assign(n1, 256); bowCandidates.assign(n1, 0);
    }
    static void reserve(void*& buf, size_t& cap, size_t bytes, const char* who) {
        if (bytes <= cap) return;
        if (buf) xfh_dev_free(buf);
        buf = nullptr; cap = 0;
        if (xfh_dev_alloc(&buf, bytes) != XFH_OK) throw std::runtime_error(std::string(who) + ": out of device memory");
        cap = bytes;
    }
    float mfNNratio;
    bool mbCheckOrientation;
    xfh_ctx* ctx;
    std::vector<int> i1, i2;
    std::vector<float> d;
    void* d_out = nullptr; size_t d_out_bytes = 0;          // device result buffer of matchPrepared
    void* d_proj = nullptr; size_t d_proj_bytes = 0;        // workspace and results of searchByProjection
    std::vector<unsigned char> projStatus;
    std::vector<int> projBest, projSecond, projCandidates;
    std::vector<unsigned char> fuseStatus;                  // results of fuse, and the level thresholds of the pyramid it was last called with
    std::vector<int> fuseBest, fuseWindow, fuseTested, fuseLevel;
    std::vector<float> fuseRatioMax; float fuseScale = 0.f;
    std::vector<unsigned char> mapStatus;                   // results of the map-point searchByProjection forms
    std::vector<int> mapBest, mapWindow, mapTested, mapLevel;
    std::vector<unsigned char> sim3Status[2];               // results of searchBySim3, per side
    std::vector<int> sim3Match[2], sim3Best[2], sim3Window[2], sim3Tested[2], sim3Level[2];
    std::vector<unsigned char> triStatus;                   // results of searchForTriangulation
    std::vector<int> triMatch, triBest, triCandidates, triGeom;
    void* d_triang = nullptr; size_t d_triang_bytes = 0;    // outputs of triangulate (device form)
    float* d_new[3] = {nullptr, nullptr, nullptr};
    std::vector<int> triangHeader; int nTriangNew = 0;
    std::vector<unsigned char> bowStatus;                   // results of searchByBoW
    std::vector<int> bowBest, bowSecond, bowCandidates;
    std::vector<unsigned char> initStatus;                  // results of searchForInitialization
    std::vector<int> initClaim, initBest, initSecond, initWindow, initTested, initMatches21, initMatchedDistance;
};

// The DBoW2 vocabulary in device memory and Frame::ComputeBoW / KeyFrame::ComputeBoW on it (xfh_vocab_pack, xfh_bow_transform_device;
// TemplatedVocabulary::transform, thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1194, for ORBvoc's TF_IDF / L1_NORM).  The constructor takes
// m_nodes flattened in node-id order (INTEGRATION.md has the loop) and uploads the blob once; the object owns it and the outputs of the last
// transform().  transform(d_desc, n) runs every one of the n rows of a descriptor block that is already in device memory (a record's) down
// the tree: deviceNodes() is then the node blob XFmatcher::searchByBoW / searchForTriangulation take in their device forms, with no host step
// between; bowVec() is mBowVec (word id, value) in ascending word id and nodeOf()[i] the NodeId of keypoint i in mFeatVec (XFH_NODE_NONE: a
// stopped feature, in no node).  Blocks until bowVec() and nodeOf() are on the host.
class XFvocabulary {
public:
    using Mat = xfeat::cvx::Mat;
    XFvocabulary(xfh_ctx* shared_ctx, int L, const std::vector<uint32_t>& parent, const std::vector<uint32_t>& wordId, const std::vector<double>& weight,
                 const std::vector<unsigned char>& desc32) : ctx(shared_ctx) {
        const size_t n = parent.size();
        if (n > 0x7fffffffu || wordId.size() != n || weight.size() != n || desc32.size() != 32 * n) throw std::runtime_error("XFvocabulary: sizes do not fit");
        vocabBytes = xfh_vocab_bytes((int)n);
        std::vector<unsigned char> blob(vocabBytes ? vocabBytes : 1);
        int rc = xfh_vocab_pack((int)n, L, parent.data(), wordId.data(), weight.data(), desc32.data(), blob.data(), &maxChildren_, &depth_);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFvocabulary: ") + xfh_strerror(rc));
        if (xfh_dev_alloc(&d_vocab, vocabBytes) != XFH_OK) throw std::runtime_error("XFvocabulary: out of device memory");
        rc = xfh_memcpy_h2d(d_vocab, blob.data(), vocabBytes);
        if (rc != XFH_OK) { xfh_dev_free(d_vocab); throw std::runtime_error(std::string("XFvocabulary: ") + xfh_strerror(rc)); }
        nodes_ = (int)n; levels_ = L;
    }
    ~XFvocabulary() { if (d_vocab) xfh_dev_free(d_vocab); if (d_out) xfh_dev_free(d_out); if (d_rows) xfh_dev_free(d_rows); }
    XFvocabulary(const XFvocabulary&) = delete;
    XFvocabulary& operator=(const XFvocabulary&) = delete;

    int size() const { return nodes_; }
    int levels() const { return levels_; }
    int maxChildren() const { return maxChildren_; }
    int depth() const { return depth_; }
    const void* device() const { return d_vocab; }
    size_t deviceBytes() const { return vocabBytes; }

    // n rows of 64 floats at d_desc (device memory, 16-byte aligned); returns the number of words of the BowVector
    int transform(const float* d_desc, int n, int levelsup = 4) {
        bow.clear(); nodeOf_.clear(); n_ = 0;
        if (n <= 0) return 0;
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t b4 = al((size_t)n * 4), b8 = al((size_t)n * 8), bn = al(xfh_nodes_bytes(n)), bw = al(xfh_bow_transform_workspace_bytes(n, 1));
        if (bw == 0) throw std::runtime_error("XFvocabulary::transform: sizes out of range");
        const size_t need = bw + 3 * b4 + 2 * b8 + bn + 256;
        if (need > outBytes) {
            if (d_out) xfh_dev_free(d_out);
            d_out = nullptr; outBytes = 0;
            if (xfh_dev_alloc(&d_out, need) != XFH_OK) throw std::runtime_error("XFvocabulary::transform: out of device memory");
            outBytes = need;
        }
        char* p = (char*)d_out;
        void* ws = p; p += bw;
        uint32_t* dword = (uint32_t*)p; p += b4; uint32_t* dno = (uint32_t*)p; p += b4; uint32_t* dids = (uint32_t*)p; p += b4;
        double* dwt = (double*)p; p += b8; double* dvals = (double*)p; p += b8;
        d_nodes = p; p += bn;
        int* dnw = (int*)p;
        int rc = xfh_bow_transform_device(ctx, 1, n, levelsup, XFH_BOWT_TF_IDF_L1, d_vocab, vocabBytes, d_desc, 0, ws, dword, dno, dwt, d_nodes, dids, dvals, dnw);
        if (rc == XFH_OK) rc = xfh_synchronize(ctx);
        int nw = 0;
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(&nw, dnw, 4);
        nodeOf_.resize(n);
        std::vector<uint32_t> ids(nw > 0 ? nw : 0); std::vector<double> vals(ids.size());
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(nodeOf_.data(), dno, (size_t)n * 4);
        if (rc == XFH_OK && nw > 0) rc = xfh_memcpy_d2h(ids.data(), dids, ids.size() * 4);
        if (rc == XFH_OK && nw > 0) rc = xfh_memcpy_d2h(vals.data(), dvals, vals.size() * 8);
        if (rc != XFH_OK) { nodeOf_.clear(); throw std::runtime_error(std::string("XFvocabulary::transform: ") + xfh_strerror(rc)); }
        bow.reserve(ids.size());
        for (size_t k = 0; k < ids.size(); ++k) bow.push_back(std::make_pair(ids[k], vals[k]));
        n_ = n;
        return nw;
    }
    // the same on host rows (mDescriptors: CV_32F, 64 columns, continuous): uploads them first
    int transform(const Mat& descriptors, int levelsup = 4) {
        const int n = descriptors.rows;
        if (n <= 0) { bow.clear(); nodeOf_.clear(); n_ = 0; return 0; }
        const size_t bytes = (size_t)n * 256;
        if (bytes > rowBytes) {
            if (d_rows) xfh_dev_free(d_rows);
            d_rows = nullptr; rowBytes = 0;
            if (xfh_dev_alloc(&d_rows, bytes) != XFH_OK) throw std::runtime_error("XFvocabulary::transform: out of device memory");
            rowBytes = bytes;
        }
        int rc = xfh_synchronize(ctx);                       // (the copy below is synchronous: nothing queued earlier may still read the buffer)
        if (rc == XFH_OK) rc = xfh_memcpy_h2d(d_rows, descriptors.template ptr<float>(0), bytes);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFvocabulary::transform: ") + xfh_strerror(rc));
        return transform((const float*)d_rows, n, levelsup);
    }
    // of the last transform(): mBowVec, mFeatVec flattened, and the node blob in device memory (valid until the next transform())
    const std::vector<std::pair<uint32_t, double>>& bowVec() const { return bow; }
    const std::vector<uint32_t>& nodeOf() const { return nodeOf_; }
    const void* deviceNodes() const { return n_ > 0 ? d_nodes : nullptr; }
    int rows() const { return n_; }

private:
    xfh_ctx* ctx;
    void* d_vocab = nullptr; size_t vocabBytes = 0;
    void* d_out = nullptr; size_t outBytes = 0;
    void* d_rows = nullptr; size_t rowBytes = 0;
    void* d_nodes = nullptr;
    int nodes_ = 0, levels_ = 0, maxChildren_ = 0, depth_ = 0, n_ = 0;
    std::vector<std::pair<uint32_t, double>> bow;
    std::vector<uint32_t> nodeOf_;
};

// KeyFrameDatabase without the inverted file (reference include/KeyFrameDatabase.h; DetectRelocalizationCandidates, src/KeyFrameDatabase.cc:733-845,
// and DetectNBestCandidates, :604-730, with L1Scoring::score): the BowVectors of the keyframes live in device arrays, one SLOT per keyframe, and a
// query scans them (xfh_bowdb_query_device).  A slot is the caller's handle for a keyframe: the caller keeps the KeyFrame pointers (slot ->
// KeyFrame*), erases a keyframe before it turns bad, and owns the maps.  add() takes mBowVec and the slots of GetBestCovisibilityKeyFrames(nn);
// deviceIds / deviceVals / deviceWords(slot) let xfh_bow_transform_device write a keyframe straight into its slot (stride == the transform's
// n), after which stamp(slot) puts it at the end of the insertion order.  The two persistent scores (mRelocScore, mPlaceRecognitionScore) are
// two device arrays of the database, zero at the start.  The candidate functions block until the answer is on the host; the sequence before the
// map tests and the caps is kept in candSlot / candAcc, the scored list in listSlot / listAcc / listBest, the header in nListed ... bestAcc.
class XFkeyframeDatabase {
public:
    typedef std::vector<std::pair<uint32_t, double>> BowVec;
    XFkeyframeDatabase(xfh_ctx* shared_ctx, int nSlots, int stride, int nNeighbours = 10) : ctx(shared_ctx), n(nSlots), st(stride), nn(nNeighbours) {
        const size_t wsb = xfh_bowdb_query_workspace_bytes(n, 1);
        if (wsb == 0 || st < 1 || st > XFH_GRID_MAX_N || nn < 0 || nn > XFH_BOWDB_MAX_NEIGHBOURS) throw std::runtime_error("XFkeyframeDatabase: sizes out of range");
        const size_t N = (size_t)n, S = (size_t)st, K = (size_t)(nn > 0 ? nn : 1);
        const size_t sizes[] = {N * S * 4, N * S * 8, N * 4, N * 4, N * K * 4, N * 4, N * 4, S * 4, S * 8, 4, N, wsb,
                                N * 4, N * 8, N, XFH_BOWDB_HEADER_INTS * 4, 4, N * 4, N * 4, N * 4, N * 4, N * 4};
        size_t off[sizeof sizes / sizeof *sizes], total = 0;
        for (size_t i = 0; i < sizeof sizes / sizeof *sizes; ++i) { off[i] = total; total += (sizes[i] + 255) & ~(size_t)255; }
        if (xfh_dev_alloc(&d_all, total) != XFH_OK) throw std::runtime_error("XFkeyframeDatabase: out of device memory");
        std::vector<unsigned char> zero(total, 0);
        memset(zero.data() + off[4], 0xFF, sizes[4]);                   // neighbours: -1
        if (xfh_memcpy_h2d(d_all, zero.data(), total) != XFH_OK) { xfh_dev_free(d_all); d_all = nullptr; throw std::runtime_error("XFkeyframeDatabase: upload failed"); }
        char* p = (char*)d_all;
        d_ids = (uint32_t*)(p + off[0]); d_vals = (double*)(p + off[1]); d_nw = (int*)(p + off[2]); d_seq = (uint32_t*)(p + off[3]); d_neigh = (int32_t*)(p + off[4]);
        d_state[0] = (float*)(p + off[5]); d_state[1] = (float*)(p + off[6]);
        d_qi = (uint32_t*)(p + off[7]); d_qv = (double*)(p + off[8]); d_qn = (int*)(p + off[9]); d_ex = (uint8_t*)(p + off[10]); d_ws = p + off[11];
        d_common = (int32_t*)(p + off[12]); d_score = (double*)(p + off[13]); d_status = (uint8_t*)(p + off[14]); d_header = (int32_t*)(p + off[15]);
        d_best = (float*)(p + off[16]); d_ls = (int32_t*)(p + off[17]); d_la = (float*)(p + off[18]); d_lb = (int32_t*)(p + off[19]);
        d_cs = (int32_t*)(p + off[20]); d_ca = (float*)(p + off[21]);
    }
    ~XFkeyframeDatabase() { if (d_all) xfh_dev_free(d_all); }
    XFkeyframeDatabase(const XFkeyframeDatabase&) = delete;
    XFkeyframeDatabase& operator=(const XFkeyframeDatabase&) = delete;

    int slots() const { return n; }
    int stride() const { return st; }
    uint32_t* deviceIds(int slot) const { return d_ids + (size_t)slot * st; }
    double* deviceVals(int slot) const { return d_vals + (size_t)slot * st; }
    int* deviceWords(int slot) const { return d_nw + slot; }

    // KeyFrameDatabase::add(pKF): mBowVec (ascending word id) into a slot, at the end of the insertion order
    void add(int slot, const BowVec& bow, const std::vector<int>& neighbours = std::vector<int>()) {
        if (slot < 0 || slot >= n || bow.size() > (size_t)st) throw std::runtime_error("XFkeyframeDatabase::add: out of range");
        std::vector<uint32_t> ids(bow.size()); std::vector<double> vals(bow.size());
        for (size_t k = 0; k < bow.size(); ++k) { ids[k] = bow[k].first; vals[k] = bow[k].second; }
        const int nw = (int)bow.size();
        sync();
        if (nw > 0) { put(deviceIds(slot), ids.data(), ids.size() * 4); put(deviceVals(slot), vals.data(), vals.size() * 8); }
        put(deviceWords(slot), &nw, 4);
        stamp(slot);
        setNeighbours(slot, neighbours);
    }
    // the slot's place in the insertion order: now the last
    void stamp(int slot) { const uint32_t s = nextSeq++; sync(); put(d_seq + slot, &s, 4); }
    // the slots of GetBestCovisibilityKeyFrames(nn) in its order (an entry outside 0 .. slots-1 means none)
    void setNeighbours(int slot, const std::vector<int>& neighbours) {
        if (slot < 0 || slot >= n) throw std::runtime_error("XFkeyframeDatabase::setNeighbours: out of range");
        if (nn == 0) return;
        std::vector<int32_t> ng(nn, -1);
        for (size_t k = 0; k < neighbours.size() && k < (size_t)nn; ++k) ng[k] = neighbours[k];
        sync();
        put(d_neigh + (size_t)slot * nn, ng.data(), (size_t)nn * 4);
    }
    // KeyFrameDatabase::erase(pKF)
    void erase(int slot) {
        if (slot < 0 || slot >= n) throw std::runtime_error("XFkeyframeDatabase::erase: out of range");
        const int zero = 0;
        sync();
        put(deviceWords(slot), &zero, 4);
    }

    // one query; fills the members below.  exclude: the slots of the connected keyframes (and of the query keyframe itself)
    void query(int form, const BowVec& bow, const std::vector<int>& exclude = std::vector<int>()) {
        if (bow.size() > (size_t)st) throw std::runtime_error("XFkeyframeDatabase::query: the vector does not fit the stride");
        std::vector<uint32_t> ids(bow.size()); std::vector<double> vals(bow.size());
        for (size_t k = 0; k < bow.size(); ++k) { ids[k] = bow[k].first; vals[k] = bow[k].second; }
        std::vector<uint8_t> ex(n, 0);
        for (int s : exclude) if (s >= 0 && s < n) ex[s] = 1;
        const int nw = (int)bow.size();
        sync();
        if (nw > 0) { put(d_qi, ids.data(), ids.size() * 4); put(d_qv, vals.data(), vals.size() * 8); }
        put(d_qn, &nw, 4); put(d_ex, ex.data(), ex.size());
        int rc = xfh_bowdb_query_device(ctx, 1, n, form, d_qi, d_qv, d_qn, st, d_ids, d_vals, d_nw, st, d_seq, nn > 0 ? d_neigh : nullptr, nn, d_ex,
                                        d_state[form == XFH_BOWDB_FORM_NBEST ? 1 : 0], d_ws, d_common, d_score, d_status, d_header, d_best, d_ls, d_la, d_lb, d_cs, d_ca);
        if (rc == XFH_OK) rc = xfh_synchronize(ctx);
        int32_t h[XFH_BOWDB_HEADER_INTS] = {};
        common.resize(n); score.resize(n); status.resize(n); listSlot.resize(n); listAcc.resize(n); listBest.resize(n); candSlot.resize(n); candAcc.resize(n);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(h, d_header, sizeof h);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(&bestAcc, d_best, 4);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(common.data(), d_common, (size_t)n * 4);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(score.data(), d_score, (size_t)n * 8);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(status.data(), d_status, (size_t)n);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(listSlot.data(), d_ls, (size_t)n * 4);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(listAcc.data(), d_la, (size_t)n * 4);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(listBest.data(), d_lb, (size_t)n * 4);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(candSlot.data(), d_cs, (size_t)n * 4);
        if (rc == XFH_OK) rc = xfh_memcpy_d2h(candAcc.data(), d_ca, (size_t)n * 4);
        if (rc != XFH_OK) throw std::runtime_error(std::string("XFkeyframeDatabase::query: ") + xfh_strerror(rc));
        nListed = h[0]; maxCommon = h[1]; minCommon = h[2]; nScored = h[3]; nCandidates = h[4];
    }

    // DetectRelocalizationCandidates(F, pMap): the candidate slots in the reference's order.  mapOfSlot[s] is compared with map
    // (`if (pKFi->GetMap() != pMap) continue;`, :834); an empty mapOfSlot keeps every candidate
    std::vector<int> DetectRelocalizationCandidates(const BowVec& bow, const std::vector<int>& mapOfSlot = std::vector<int>(), int map = 0) {
        query(XFH_BOWDB_FORM_RELOC, bow);
        std::vector<int> out;
        for (int k = 0; k < nCandidates; ++k) {
            const int s = candSlot[k];
            if (mapOfSlot.empty() || mapOfSlot[s] == map) out.push_back(s);
        }
        return out;
    }
    // DetectNBestCandidates(pKF, vpLoopCand, vpMergeCand, nNumCandidates): connected = the slots of pKF->GetConnectedKeyFrames() (and of pKF itself
    // when it is in the database), queryMap = pKF->GetMap(), badMaps = the maps with IsBad()
    void DetectNBestCandidates(const BowVec& bow, const std::vector<int>& connected, std::vector<int>& vpLoopCand, std::vector<int>& vpMergeCand, int nNumCandidates,
                               const std::vector<int>& mapOfSlot, int queryMap, const std::vector<int>& badMaps = std::vector<int>()) {
        query(XFH_BOWDB_FORM_NBEST, bow, connected);
        vpLoopCand.clear(); vpMergeCand.clear();
        for (int k = 0; k < nCandidates && ((int)vpLoopCand.size() < nNumCandidates || (int)vpMergeCand.size() < nNumCandidates); ++k) {
            const int s = candSlot[k], m = mapOfSlot[s];
            bool bad = false;
            for (int b : badMaps) bad = bad || b == m;
            if (m == queryMap && (int)vpLoopCand.size() < nNumCandidates) vpLoopCand.push_back(s);
            else if (m != queryMap && (int)vpMergeCand.size() < nNumCandidates && !bad) vpMergeCand.push_back(s);
        }
    }

    // of the last query
    int nListed = 0, maxCommon = 0, minCommon = 0, nScored = 0, nCandidates = 0;
    float bestAcc = 0.f;
    std::vector<int32_t> common, listSlot, listBest, candSlot;
    std::vector<double> score;
    std::vector<uint8_t> status;
    std::vector<float> listAcc, candAcc;

private:
    void sync() { if (xfh_synchronize(ctx) != XFH_OK) throw std::runtime_error("XFkeyframeDatabase: the stream failed"); }   // (the copies are synchronous: nothing queued may still read)
    static void put(void* dst, const void* src, size_t bytes) { if (xfh_memcpy_h2d(dst, src, bytes) != XFH_OK) throw std::runtime_error("XFkeyframeDatabase: upload failed"); }
    xfh_ctx* ctx;
    int n, st, nn;
    uint32_t nextSeq = 0;
    void* d_all = nullptr;
    uint32_t* d_ids = nullptr; double* d_vals = nullptr; int* d_nw = nullptr; uint32_t* d_seq = nullptr; int32_t* d_neigh = nullptr;
    float* d_state[2] = {nullptr, nullptr};
    uint32_t* d_qi = nullptr; double* d_qv = nullptr; int* d_qn = nullptr; uint8_t* d_ex = nullptr; void* d_ws = nullptr;
    int32_t* d_common = nullptr; double* d_score = nullptr; uint8_t* d_status = nullptr; int32_t* d_header = nullptr; float* d_best = nullptr;
    int32_t* d_ls = nullptr; float* d_la = nullptr; int32_t* d_lb = nullptr; int32_t* d_cs = nullptr; float* d_ca = nullptr;
};

}  // namespace ORB_SLAM3
#endif
