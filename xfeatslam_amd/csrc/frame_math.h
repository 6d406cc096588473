// frame_math.h -- the per-keypoint arithmetic of the reference's RGB-D Frame constructor (src/Frame.cc:311-374), written ONCE for the
// host entry points (xfh_undistort_points, xfh_camera_bounds; capi_search.cpp) and the kernel (frame_finish.hip.h).
//
//   Frame::UndistortKeyPoints     :940-973   cv::undistortPoints(src, dst, K, dist, Mat(), P = K), restated from OpenCV's documented
//                                            algorithm (the library does not link OpenCV): five fixed-point iterations of the inverse
//                                            of the radial-tangential model (the default TermCriteria is COUNT 5: no epsilon exit),
//                                            everything in float64, the result rounded to fp32 once per coordinate
//   Frame::ComputeStereoFromRGBD  :1177-1198 d = imDepth(v, u) at the RAW keypoint; mvDepth = d, mvuRight = kpU.x - mbf / d when d > 0,
//                                            else both -1
//
// The library is built with -ffp-contract=off: every line below is the IEEE operation sequence it spells, on both sides.
#pragma once
#include <stdint.h>
#include "../../include/xfeat_hip.h"
#include "hd.h"

// (u, v) -> (u', v').  k1 == 0 copies the point whatever the other coefficients are (Frame.cc:942).
XFH_HD void xfh_undistort_point(const xfh_camera& cam, float u, float v, float* uo, float* vo) {
    if (cam.k1 == 0.0f) { *uo = u; *vo = v; return; }
    const double fx = (double)cam.fx, fy = (double)cam.fy, cx = (double)cam.cx, cy = (double)cam.cy;
    const double k1 = (double)cam.k1, k2 = (double)cam.k2, p1 = (double)cam.p1, p2 = (double)cam.p2, k3 = (double)cam.k3;
    const double x0 = ((double)u - cx) / fx, y0 = ((double)v - cy) / fy;
    double x = x0, y = y0;
    for (int it = 0; it < 5; ++it) {
        const double r2 = x * x + y * y;
        const double icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2);
        if (icdist < 0.0) { x = x0; y = y0; break; }
        const double dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
        const double dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
        x = (x0 - dx) * icdist; y = (y0 - dy) * icdist;
    }
    *uo = (float)(x * fx + cx); *vo = (float)(y * fy + cy);
}

// imDepth.at<float>(v, u) of frame `img` (rows `pitch` bytes apart) at the RAW keypoint; raw uint16 becomes (float)raw * scale, one fp32
// rounding (convertTo with the reference's 1.0f / DepthMapFactor, Tracking.cc:577-581, :1548).  (int) truncates, so (-1, 0) reads
// column / row 0 like the reference; where the reference would read outside the image the sample is 0 and nothing is read: the
// test is made on the floats, so a non-finite or huge coordinate never reaches the conversion.
XFH_HD float xfh_depth_sample(const void* img, int depth_type, size_t pitch, float scale, int width, int height, float u, float v) {
    if (!(u > -1.0f && u < (float)width && v > -1.0f && v < (float)height)) return 0.0f;
    const int iu = (int)u, iv = (int)v;
    const char* row = (const char*)img + (size_t)iv * pitch;
    if (depth_type == XFH_DEPTH_U16) return (float)((const uint16_t*)row)[iu] * scale;
    return ((const float*)row)[iu];
}

// mvDepth / mvuRight of one keypoint from its depth sample and its UNDISTORTED u (a NaN depth fails d > 0)
XFH_HD void xfh_stereo_from_depth(float d, float u_un, float bf, float* depth, float* uright) {
    if (d > 0.0f) { *depth = d; *uright = u_un - bf / d; }
    else { *depth = -1.0f; *uright = -1.0f; }
}
