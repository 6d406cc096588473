// asan_nodes_test.cpp -- the host side of the SearchForTriangulation entry points, linked against the sanitizer build of libxfeat_hip
// (make -C xfeatslam_amd/csrc asan): xfh_nodes_pack, xfh_nodes_unpack on well-formed, truncated and inconsistent blobs, xfh_epipolar_gate
// on hostile floats, and the argument checks that return before any HIP call.  AddressSanitizer / UBSan abort on any finding, so exit
// code 0 = clean.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "xfeat_hip.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "asan_nodes_test: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

int main() {
    const uint32_t ids[6] = {0u, 1u, (1u << 21) + 9u, (1u << 31) + 3u, 0xFFFFFFFEu, XFH_NODE_NONE};
    unsigned seed = 12345;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    for (int n : {1, 2, 3, 4, 5, 63, 64, 65, 301, 515, 4096, XFH_GRID_MAX_N}) {
        std::vector<uint32_t> no(n);
        for (int i = 0; i < n; ++i) no[i] = ids[rnd() % 6];
        const size_t nb = xfh_nodes_bytes(n);
        CHECK(nb % 16 == 0 && nb >= 64 + 16 * ((size_t)n + 1));
        // heap buffers of EXACTLY the documented sizes: a byte too far is a finding
        std::vector<unsigned char> blob(nb, 0xA5), again(nb, 0x5A);
        int nn = -1, nn2 = -1;
        CHECK(xfh_nodes_pack(no.data(), n, blob.data(), &nn) == XFH_OK && xfh_nodes_pack(no.data(), n, again.data(), nullptr) == XFH_OK);
        CHECK(memcmp(blob.data(), again.data(), nb) == 0 && nn >= 0 && nn <= 5);
        std::vector<uint32_t> nid(n);
        std::vector<int> ns(n + 1), items(n);
        CHECK(xfh_nodes_unpack(blob.data(), nb, n, nid.data(), ns.data(), items.data(), &nn2) == XFH_OK && nn2 == nn);
        CHECK(ns[0] == 0);
        for (int k = 0; k < nn; ++k) {
            CHECK(ns[k + 1] > ns[k] && (k == 0 || nid[k] > nid[k - 1]));
            for (int q = ns[k]; q < ns[k + 1]; ++q) CHECK(items[q] >= 0 && items[q] < n && no[items[q]] == nid[k] && (q == ns[k] || items[q] > items[q - 1]));
        }
        // truncated: every prefix length of a small blob, some of a large one (the copy has exactly that many bytes)
        for (size_t len = 0; len < nb; len += (nb > 4096 ? nb / 37 + 1 : 1)) {
            std::vector<unsigned char> cut(blob.begin(), blob.begin() + len);
            CHECK(xfh_nodes_unpack(cut.data(), len, n, nid.data(), ns.data(), items.data(), &nn2) == XFH_ERR_INVALID_ARG);
        }
        // inconsistent: one int of the blob replaced by an out-of-range value, at many places; the call must return (either status) and never read outside
        const int vals[6] = {-1, n, n + 1, 1 << 30, (int)0x80000000u, 0x7fffffff};
        const size_t words = nb / 4;
        for (size_t w = 0; w < words; w += (words > 2048 ? words / 251 + 1 : 1))
            for (int v : vals) {
                std::vector<unsigned char> bad(blob);
                memcpy(bad.data() + 4 * w, &v, 4);
                const int rc = xfh_nodes_unpack(bad.data(), nb, n, nid.data(), ns.data(), items.data(), &nn2);
                CHECK(rc == XFH_OK || rc == XFH_ERR_INVALID_ARG);
                if (w == 0) CHECK(rc == XFH_ERR_INVALID_ARG);                              // the magic
            }
        CHECK(xfh_nodes_unpack(blob.data(), nb, n + 1, nid.data(), ns.data(), items.data(), &nn2) == XFH_ERR_INVALID_ARG);
    }
    std::vector<unsigned char> b(xfh_nodes_bytes(4));
    uint32_t four[4] = {1, 2, 3, 4};
    CHECK(xfh_nodes_pack(nullptr, 4, b.data(), nullptr) == XFH_ERR_INVALID_ARG && xfh_nodes_pack(four, 4, nullptr, nullptr) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_nodes_pack(four, 0, b.data(), nullptr) == XFH_ERR_INVALID_ARG && xfh_nodes_pack(four, XFH_GRID_MAX_N + 1, b.data(), nullptr) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_nodes_unpack(nullptr, 64, 4, nullptr, nullptr, nullptr, nullptr) == XFH_ERR_INVALID_ARG && xfh_nodes_bytes(-3) == 0);

    // the gates on hostile floats: every combination of special values in F12, the epipole, the coordinates and uright
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float sp[8] = {nan, inf, -inf, 1e30f, -1e30f, 0.0f, 3.4e38f, 1e-40f};
    const int n = 37;
    std::vector<float> xy(2 * n), ur(n);
    std::vector<uint8_t> pass(n);
    for (int t = 0; t < 512; ++t) {
        float Fm[9], ep[2];
        for (int k = 0; k < 9; ++k) Fm[k] = (rnd() % 3 == 0) ? sp[rnd() % 8] : (float)(rnd() % 1000) * 1e-6f;
        for (int k = 0; k < 2; ++k) ep[k] = (rnd() % 3 == 0) ? sp[rnd() % 8] : (float)(rnd() % 640);
        for (int k = 0; k < 2 * n; ++k) xy[k] = (rnd() % 5 == 0) ? sp[rnd() % 8] : (float)(rnd() % 640);
        for (int k = 0; k < n; ++k) ur[k] = (rnd() % 4 == 0) ? sp[rnd() % 8] : (rnd() % 2 ? -1.0f : (float)(rnd() % 640));
        const int flags = t & 3;
        CHECK(xfh_epipolar_gate(Fm, ep, 100.0f, 1.0f, flags, sp[t % 8], 240.0f, t & 4, xy.data(), (t & 8) ? ur.data() : nullptr, n, pass.data()) == XFH_OK);
        for (int k = 0; k < n; ++k) CHECK(pass[k] <= XFH_TRI_GATE_PASSED);
        if ((flags & XFH_TRI_ONLY_STEREO) && !(t & 8)) for (int k = 0; k < n; ++k) CHECK(pass[k] == XFH_TRI_GATE_SKIPPED);
    }
    float Fz[9] = {0}, e0[2] = {0, 0};
    CHECK(xfh_epipolar_gate(nullptr, e0, 100.f, 1.f, 0, 0.f, 0.f, 0, xy.data(), nullptr, n, pass.data()) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_epipolar_gate(Fz, e0, 100.f, 1.f, 4, 0.f, 0.f, 0, xy.data(), nullptr, n, pass.data()) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_epipolar_gate(Fz, e0, 100.f, 1.f, 0, 0.f, 0.f, 0, nullptr, nullptr, 0, nullptr) == XFH_OK);
    // argument checks of the device and host forms that return before any HIP call
    const void* p = Fz;
    CHECK(xfh_triangulation_search_device(nullptr, 1, 1, 1, 1, 0, 100, 100.f, 1.f, p, Fz, nullptr, pass.data(), Fz, 0, p, Fz, nullptr, pass.data(), Fz, 0, Fz, e0,
                                          pass.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_triangulation_search(nullptr, 1, 1, 0, 100, 100.f, 1.f, four, Fz, nullptr, pass.data(), Fz, four, Fz, nullptr, pass.data(), Fz, Fz, e0, pass.data(),
                                   nullptr, nullptr, nullptr, nullptr, nullptr) == XFH_ERR_INVALID_ARG);
    printf("asan_nodes_test ok\n");
    return 0;
}
