// asan_frame_test.cpp -- the host side of the frame-finish entry points, linked against the sanitizer build of libxfeat_hip
// (make -C xfeatslam_amd/csrc asan): xfh_undistort_points and xfh_camera_bounds on hostile coordinates and coefficients, and the
// argument checks of the device calls that return before any HIP call.  AddressSanitizer / UBSan abort on any finding, so exit
// code 0 = clean.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "xfeat_hip.h"
#include "xfeat_hip_bench.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "asan_frame_test: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

static xfh_camera tum1() {
    xfh_camera c;
    memset(&c, 0, sizeof c);
    c.fx = 517.306408f; c.fy = 516.469215f; c.cx = 318.643040f; c.cy = 255.313989f;
    c.k1 = 0.262383f; c.k2 = -0.953104f; c.p1 = -0.005358f; c.p2 = 0.002628f; c.k3 = 1.163314f; c.bf = 40.0f;
    c.width = 640; c.height = 480;
    return c;
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float bad[] = {nan, inf, -inf, 1e30f, -1e30f, 0.0f, -0.0f, 3.4e38f, 1e-45f};
    const int nb = (int)(sizeof bad / sizeof bad[0]);
    CHECK(strcmp(xfh_kernel_name(XFH_K_FRAME_FINISH), "k_frame_finish") == 0 && XFH_K_FRAME_FINISH == 15);
    xfh_camera cam = tum1();
    // exactly-sized buffers: any access past n pairs is a finding
    for (int n : {0, 1, 7}) {
        std::vector<float> in(2 * n, 100.0f), out(2 * n, -7.0f);
        CHECK(xfh_undistort_points(&cam, n ? in.data() : nullptr, n, n ? out.data() : nullptr) == XFH_OK);
        for (int k = 0; k < 2 * n; ++k) CHECK(std::isfinite(out[k]) && std::fabs(out[k] - 100.0f) < 30.0f);
    }
    CHECK(xfh_undistort_points(nullptr, nullptr, 0, nullptr) == XFH_ERR_INVALID_ARG);
    float one[2] = {1.0f, 2.0f}, res[2];
    CHECK(xfh_undistort_points(&cam, one, -1, res) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_undistort_points(&cam, nullptr, 1, res) == XFH_ERR_INVALID_ARG && xfh_undistort_points(&cam, one, 1, nullptr) == XFH_ERR_INVALID_ARG);
    // hostile coordinates, every pair of them
    std::vector<float> in, out;
    for (int a = 0; a < nb; ++a) for (int b = 0; b < nb; ++b) { in.push_back(bad[a]); in.push_back(bad[b]); }
    out.assign(in.size(), 0.0f);
    CHECK(xfh_undistort_points(&cam, in.data(), (int)in.size() / 2, out.data()) == XFH_OK);
    // hostile coefficients and intrinsics, one field at a time (zero focal length included), on ordinary and hostile points
    xfh_grid_bounds gb;
    float* fields[] = {&cam.fx, &cam.fy, &cam.cx, &cam.cy, &cam.k1, &cam.k2, &cam.p1, &cam.p2, &cam.k3, &cam.bf};
    for (float* f : fields)
        for (int a = 0; a < nb; ++a) {
            cam = tum1();
            *f = bad[a];
            CHECK(xfh_undistort_points(&cam, in.data(), (int)in.size() / 2, out.data()) == XFH_OK);
            CHECK(xfh_camera_bounds(&cam, &gb) == XFH_OK);
        }
    // k1 == 0: the input bits, whatever the other coefficients are; bounds (0, 0, cols, rows)
    cam = tum1(); cam.k1 = 0.0f;
    CHECK(xfh_undistort_points(&cam, in.data(), (int)in.size() / 2, out.data()) == XFH_OK && memcmp(in.data(), out.data(), in.size() * 4) == 0);
    CHECK(xfh_camera_bounds(&cam, &gb) == XFH_OK && gb.min_x == 0.0f && gb.min_y == 0.0f && gb.max_x == 640.0f && gb.max_y == 480.0f);
    cam = tum1();
    CHECK(xfh_camera_bounds(&cam, &gb) == XFH_OK && gb.min_x > 10.0f && gb.min_x < 11.0f && gb.max_y > 473.0f && gb.max_y < 474.0f);
    CHECK(xfh_camera_bounds(nullptr, &gb) == XFH_ERR_INVALID_ARG && xfh_camera_bounds(&cam, nullptr) == XFH_ERR_INVALID_ARG);
    cam.width = 0; CHECK(xfh_camera_bounds(&cam, &gb) == XFH_ERR_INVALID_ARG);
    cam = tum1(); cam.height = -3; CHECK(xfh_camera_bounds(&cam, &gb) == XFH_ERR_INVALID_ARG);
    // the device calls refuse a NULL ctx before anything touches HIP
    cam = tum1();
    float buf[16];
    CHECK(xfh_frame_finish_records_device(nullptr, buf, 1, &cam, nullptr, XFH_DEPTH_NONE, 0, 1.0f, &gb, 0, buf, buf, buf, nullptr) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_frame_finish(nullptr, nullptr, 0, &cam, nullptr, XFH_DEPTH_NONE, 0, 1.0f, buf, buf, buf) == XFH_ERR_INVALID_ARG);
    printf("asan_frame_test ok\n");
    return 0;
}
