// asan_init_test.cpp -- the host side of the monocular-initialisation entry points under AddressSanitizer + UBSan, linked against the
// sanitizer build of libxfeat_hip (make -C xfeatslam_amd/csrc asan): xfh_init_accept against the line of init_math.h compiled here over
// every boundary and over random and extreme operands (INT_MAX and INT_MIN converted to float, NaN / Inf ratios), the layout helper against
// the workspace size the library reports, and the argument checks of the search calls that return before any HIP call (a NULL ctx).
// Exit code 0 = clean.  Host code only: nothing here runs on a GPU.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>
#include "xfeat_hip.h"
#include "xfeat_hip_bench.h"
#include "init_math.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "asan_init_test: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // the boundaries, answers written out
    CHECK(xfh_init_accept(100, INT_MAX, 100, 0.9f) == 1);                 // best == th_low
    CHECK(xfh_init_accept(101, INT_MAX, 100, 0.9f) == 0);                 // th_low + 1
    CHECK(xfh_init_accept(0, INT_MAX, 100, 0.9f) == 1);                   // no second candidate
    CHECK(xfh_init_accept(0, 0, 100, 0.9f) == 0);                         // 0 < 0 is false
    CHECK(xfh_init_accept(45, 100, 100, 0.5f) == 1 && xfh_init_accept(50, 100, 100, 0.5f) == 0 && xfh_init_accept(51, 100, 100, 0.5f) == 0);   // best == second * ratio exactly
    CHECK(xfh_init_accept(INT_MAX, INT_MAX, INT_MAX, 2.0f) == 0);         // "none" never accepts
    CHECK(xfh_init_accept(5, 10, 100, nan) == 0 && xfh_init_accept(5, 10, 100, inf) == 1 && xfh_init_accept(5, 0, 100, inf) == 0);
    const int ints[10] = {0, 1, 99, 100, 101, 1000, INT_MAX, INT_MAX - 1, -1, INT_MIN};
    const float ratios[8] = {0.0f, 0.6f, 0.9f, 1.0f, 2.0f, inf, nan, 1e-30f};
    long long sum = 0;
    for (int b : ints) for (int s : ints) for (int t : ints) for (float r : ratios) {
        const int got = xfh_init_accept(b, s, t, r);
        CHECK(got == (xfh_init_accept_line(b, s, t, r) ? 1 : 0));
        sum += got;
    }
    unsigned seed = 7;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return seed; };
    for (int i = 0; i < 100000; ++i) {
        const int b = (int)(rnd() % 300), s = (int)(rnd() % 300), t = (int)(rnd() % 200);
        const float r = (float)(rnd() % 1000) / 1000.0f;
        CHECK(xfh_init_accept(b, s, t, r) == ((b <= t && (float)b < (float)s * r) ? 1 : 0));
    }
    // the layout helper against the library
    CHECK(xfh_init_list_entries() == XFH_INIT_K);
    for (int nq : {1, 7, 1000, XFH_GRID_MAX_N}) for (int nt : {1, 9, 4096, XFH_GRID_MAX_N}) for (int B : {1, 3, 65535}) {
        const InitWs w = init_ws_layout(nq, nt);
        CHECK(xfh_init_search_workspace_bytes(nq, nt, B) == w.bytes * (size_t)B && w.bytes % 256 == 0 && w.next + (size_t)nq * 4 <= w.bytes);
        CHECK(w.centre >= 16 && w.ldist >= w.centre + (size_t)nq * 16 && w.head >= w.dist + (size_t)nq * 4 && w.next >= w.head + (size_t)nt * 4);
    }
    for (int bad : {0, -1, XFH_GRID_MAX_N + 1}) {
        CHECK(xfh_init_search_workspace_bytes(bad, 8, 1) == 0 && xfh_init_search_workspace_bytes(8, bad, 1) == 0);
    }
    CHECK(xfh_init_search_workspace_bytes(8, 8, 0) == 0 && xfh_init_search_workspace_bytes(8, 8, 65536) == 0 && xfh_init_search_workspace_bytes(8, 8, -1) == 0);
    // the argument checks that return before any HIP call
    float* f = (float*)malloc(64 * 64 * sizeof(float)); int* ip = (int*)malloc(64 * sizeof(int)); uint8_t* u8 = (uint8_t*)malloc(64);
    xfh_keypoint* kp = (xfh_keypoint*)calloc(8, sizeof(xfh_keypoint));
    const xfh_grid_bounds gb = {0.0f, 0.0f, 640.0f, 480.0f};
    CHECK(xfh_init_search_device(nullptr, 1, 8, f, f, nullptr, 100.0f, f, f, 0, nullptr, 8, 100, 0.9f, f, u8, ip, ip, ip, ip, ip, ip, ip, ip, ip, nullptr) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_init_search(nullptr, 8, f, f, nullptr, 100.0f, kp, &gb, f, 8, 100, 0.9f, u8, ip, ip, ip, ip, ip, ip, ip, ip, ip, nullptr) == XFH_ERR_INVALID_ARG);
    CHECK(strcmp(xfh_kernel_name(XFH_K_INIT_CANDIDATES), "k_init_candidates") == 0 && strcmp(xfh_kernel_name(XFH_K_INIT_FINAL), "k_init_final") == 0 &&
          XFH_K_INIT_CANDIDATES == 27 && strcmp(xfh_kernel_name(26), "?") == 0);
    free(f); free(ip); free(u8); free(kp);
    printf("asan_init_test ok (%lld accepted)\n", sum);
    return 0;
}
