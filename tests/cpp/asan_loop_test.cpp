// asan_loop_test.cpp -- the host side of the loop-closing / relocalisation entry points under AddressSanitizer + UBSan, linked against the
// sanitizer build of libxfeat_hip (make -C xfeatslam_amd/csrc asan): xfh_map_project and xfh_sim3_project on heap buffers of EXACTLY the
// documented sizes (a byte too far is a finding) over ordinary and hostile values, against the lines of mapproj_math.h / sim3_math.h
// compiled here, and the argument checks of the search calls that return before any HIP call (a NULL ctx).  Exit code 0 = clean.
// Host code only: nothing here runs on a GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "xfeat_hip.h"
#include "mapproj_math.h"
#include "sim3_math.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "asan_loop_test: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

template <typename T> struct Exact {                         // exactly n elements on the heap: the redzone starts behind the last one
    T* p; size_t n;
    explicit Exact(size_t count) : p((T*)malloc(count ? count * sizeof(T) : 1)), n(count) {}
    ~Exact() { free(p); }
    Exact(const Exact&) = delete;
};

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float special[10] = {nan, inf, -inf, 0.0f, -0.0f, 1e38f, -1e38f, 1e-40f, 3.4e38f, 1e30f};
    unsigned seed = 99;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 8) / 16777216.0f; };
    xfh_camera cam; memset(&cam, 0, sizeof cam);
    cam.fx = 517.3f; cam.fy = 516.5f; cam.cx = 318.6f; cam.cy = 255.3f; cam.bf = 40.0f; cam.width = 640; cam.height = 480;
    const xfh_grid_bounds b = {0.0f, 0.0f, 640.0f, 480.0f};
    float sf[XFH_FUSE_MAX_LEVELS], rmax[XFH_FUSE_MAX_LEVELS];
    long long sum = 0;
    for (int nl : {1, 2, 8, XFH_FUSE_MAX_LEVELS}) {
        sf[0] = 1.0f;
        for (int l = 1; l < nl; ++l) sf[l] = sf[l - 1] * 1.2f;
        CHECK(xfh_scale_level_thresholds(1.2f, nl, nl > 1 ? rmax : nullptr) == XFH_OK);
        FuseLevels L; memset(&L, 0, sizeof L);
        L.nlevels = nl;
        for (int l = 0; l < nl; ++l) L.scale_factors[l] = sf[l];
        for (int l = 0; l + 1 < nl; ++l) L.ratio_max[l] = rmax[l];
        for (int n : {0, 1, 7, 1000}) {
            Exact<float> xyz(3 * (size_t)n), nr(3 * (size_t)n), dd(3 * (size_t)n), uvr(3 * (size_t)n), T(12), M(12), Ow(3), sfe(nl), rme(nl > 1 ? nl - 1 : 0);
            Exact<int> lv(n); Exact<uint8_t> st(n);
            memcpy(sfe.p, sf, nl * sizeof(float)); memcpy(rme.p, rmax, (nl > 1 ? nl - 1 : 0) * sizeof(float));
            for (int round = 0; round < 3; ++round) {
                for (int i = 0; i < 3 * n; ++i) { xyz.p[i] = rnd() * 6 - 2; nr.p[i] = rnd() * 2 - 1; dd.p[i] = rnd() * 5; }
                if (round) for (int i = 0; i < 3 * n; i += 5) (i % 3 == 0 ? xyz : i % 3 == 1 ? nr : dd).p[i] = special[(i / 5) % 10];
                const float eye[12] = {1, 0, 0, 0.01f, 0, 1, 0, -0.02f, 0, 0, 1, 0.03f};
                memcpy(T.p, eye, sizeof eye); memcpy(M.p, eye, sizeof eye);
                M.p[0] = M.p[5] = M.p[10] = 1.03f;
                Ow.p[0] = -0.01f; Ow.p[1] = 0.02f; Ow.p[2] = -0.03f;
                if (round == 2) { T.p[5] = nan; T.p[11] = inf; M.p[2] = -inf; Ow.p[1] = 1e38f; }
                for (int form = 0; form < 16; ++form) {
                    CHECK(xfh_map_project(T.p, Ow.p, &cam, &b, 7.0f, sfe.p, rme.p, nl, form, xyz.p, nr.p, dd.p, n, uvr.p, lv.p, st.p) == XFH_OK);
                    for (int i = 0; i < n; ++i) {
                        float u, v, r; int level;
                        const int s = xfh_mapproj_point(T.p, Ow.p, cam, b, 7.0f, L, form, xyz.p + 3 * i, nr.p + 3 * i, dd.p + 3 * i, &u, &v, &r, &level);
                        CHECK(s == st.p[i] && level == lv.p[i] && memcmp(&u, uvr.p + 3 * i, 4) == 0 && memcmp(&v, uvr.p + 3 * i + 1, 4) == 0 && memcmp(&r, uvr.p + 3 * i + 2, 4) == 0);
                        CHECK(level >= -1 && level < nl && (s == XFH_MAPPROJ_VISIBLE) == (level >= 0));
                        sum += s;
                    }
                }
                CHECK(xfh_sim3_project(T.p, M.p, &cam, &b, 7.0f, sfe.p, rme.p, nl, xyz.p, dd.p, n, uvr.p, lv.p, st.p) == XFH_OK);
                for (int i = 0; i < n; ++i) {
                    float u, v, r; int level;
                    const int s = xfh_sim3_point(T.p, M.p, cam, b, 7.0f, L, xyz.p + 3 * i, dd.p + 3 * i, &u, &v, &r, &level);
                    CHECK(s == st.p[i] && level == lv.p[i] && memcmp(&u, uvr.p + 3 * i, 4) == 0 && memcmp(&v, uvr.p + 3 * i + 1, 4) == 0 && memcmp(&r, uvr.p + 3 * i + 2, 4) == 0);
                    CHECK(s != XFH_FUSE_BAD_ANGLE && level >= -1 && level < nl && (s == XFH_SIM3_VISIBLE) == (level >= 0));
                    sum += s;
                }
            }
        }
    }
    // the argument checks of the stateless functions
    float f12[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, p3[3] = {0, 0, 1}, o3[3]; int l1; uint8_t s1;
    sf[0] = 1.0f; sf[1] = 1.2f;
    CHECK(xfh_map_project(f12, p3, &cam, &b, 3.0f, sf, rmax, 2, XFH_MAPPROJ_FORM_SIM3, p3, p3, p3, 1, o3, &l1, &s1) == XFH_OK && s1 == XFH_MAPPROJ_VISIBLE);
    CHECK(xfh_map_project(nullptr, p3, &cam, &b, 3.0f, sf, rmax, 2, 3, p3, p3, p3, 1, o3, &l1, &s1) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_map_project(f12, p3, &cam, &b, 3.0f, sf, rmax, 2, 16, p3, p3, p3, 1, o3, &l1, &s1) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_map_project(f12, p3, &cam, &b, 3.0f, sf, rmax, 17, 3, p3, p3, p3, 1, o3, &l1, &s1) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_map_project(f12, p3, &cam, &b, 3.0f, sf, nullptr, 2, 3, p3, p3, p3, 1, o3, &l1, &s1) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_map_project(f12, p3, &cam, &b, 3.0f, sf, rmax, 2, 3, p3, nullptr, p3, 1, o3, &l1, &s1) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_map_project(f12, p3, &cam, &b, 3.0f, sf, rmax, 2, 3, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == XFH_OK);
    CHECK(xfh_sim3_project(f12, f12, &cam, &b, 3.0f, sf, rmax, 2, p3, p3, 1, o3, &l1, &s1) == XFH_OK);
    CHECK(xfh_sim3_project(f12, nullptr, &cam, &b, 3.0f, sf, rmax, 2, p3, p3, 1, o3, &l1, &s1) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_sim3_project(f12, f12, nullptr, &b, 3.0f, sf, rmax, 2, p3, p3, 1, o3, &l1, &s1) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_sim3_project(f12, f12, &cam, &b, 3.0f, sf, rmax, 0, p3, p3, 1, o3, &l1, &s1) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_sim3_project(f12, f12, &cam, &b, 3.0f, sf, rmax, 2, p3, p3, -1, o3, &l1, &s1) == XFH_ERR_INVALID_ARG);
    // the workspace size, and the search calls with a NULL ctx: refused before any HIP call
    CHECK(xfh_map_projection_search_workspace_bytes(0, 1, 1) == 0 && xfh_map_projection_search_workspace_bytes(1, 1, 0) == 0);
    CHECK(xfh_map_projection_search_workspace_bytes(1, XFH_GRID_MAX_N + 1, 1) == 0 && xfh_map_projection_search_workspace_bytes(1, 1, 65536) == 0);
    CHECK(xfh_map_projection_search_workspace_bytes(1000, 1000, 3) % 256 == 0 &&
          xfh_map_projection_search_workspace_bytes(1000, 1000, 3) >= xfh_search_projection_workspace_bytes(1000, 1000, 3) + 3 * 1000 * sizeof(int));
    float row[64] = {0}; uint8_t fl[4] = {1, 1, 1, 1}; int o[4]; xfh_keypoint kp[1]; memset(kp, 0, sizeof kp);
    CHECK(xfh_map_projection_search_device(nullptr, 3, 1, 1, p3, p3, p3, row, fl, f12, p3, &cam, &b, 3.0f, sf, rmax, 2, row, row, 0, 0, 1, nullptr, 256, 100.0f, row, fl,
                                           o, o, o, o, o, nullptr, o, o) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_map_projection_search(nullptr, 3, 1, p3, p3, p3, row, fl, f12, p3, &cam, &b, 3.0f, sf, rmax, 2, kp, row, 1, nullptr, 256, 100.0f, fl, o, o, o, o, o, nullptr,
                                    o, o) == XFH_ERR_INVALID_ARG);
    xfh_sim3_side side; memset(&side, 0, sizeof side);
    side.n = 1; side.grid = row; side.kps = kp; side.desc = row; side.points = p3; side.dist = p3; side.mp_desc = row; side.flags = fl; side.Tw = f12;
    side.status = fl; side.match = o; side.best_dist = o; side.n_window = o; side.n_tested = o; side.level = o;
    CHECK(xfh_sim3_search_device(nullptr, 1, 0, &side, &side, f12, f12, &cam, &b, 3.0f, sf, rmax, 2, 1000, o, o) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_sim3_search(nullptr, &side, &side, f12, f12, &cam, &b, 3.0f, sf, rmax, 2, 1000, o, o) == XFH_ERR_INVALID_ARG);
    printf("asan_loop_test ok (%lld)\n", sum);
    return 0;
}
