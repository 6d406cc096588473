// asan_bow_test.cpp -- the host side of the SearchByBoW entry points under AddressSanitizer + UBSan: nodes_clamp.h, the very lines the
// kernels of bow_search.hip.h and k_triangulation_search (triangulation_search.hip.h, which walks side 2's blob as k_bow_candidates does)
// read node blobs through, walked the way the kernels walk them over well-formed and hostile blobs that live in
// heap buffers of EXACTLY xfh_nodes_bytes(n) bytes (a byte too far is a finding); xfh_bow_accept and the argument checks that return
// before any HIP call, linked against the sanitizer build of libxfeat_hip (make -C xfeatslam_amd/csrc asan).  Exit code 0 = clean.
// The hostile blobs are those of tests/test_gpu_bow.py::test_hostile_blobs: the items of a node replaced by out-of-range values, a
// node_start far out of range or negative, n_nodes far out of range, negative or n + 1 -- and beyond those every word of the blob replaced
// in turn, and blobs of random words.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "xfeat_hip.h"
#include "nodes_clamp.h"
#include "bow_math.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "asan_bow_test: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

// what k_bow_candidates does with side 2's blob for every query, and k_bow_resolve with both: -> false if an index left its range
static bool walk(const char* b1, int n1, const char* b2, int n2, long long* sum) {
    const int nn1 = nodes_count(b1, n1), nn2 = nodes_count(b2, n2);
    if (nn1 < 0 || nn1 > n1 || nn2 < 0 || nn2 > n2) return false;
    for (int i = 0; i < n1; ++i) {
        const int slot = nodes_find(b2, n2, nn2, nodes_node_of(b1, n1, i));
        if (slot < -1 || slot >= nn2) return false;
        if (slot < 0) continue;
        const NodeRange r = nodes_range(b2, n2, slot);
        if (r.start < 0 || r.len < 0 || r.start + r.len > n2) return false;
        for (int p = 0; p < r.len; ++p) {
            const int idx = nodes_item(b2, n2, r.start + p);
            if (idx < -1 || idx >= n2) return false;
            *sum += idx;
        }
    }
    for (int w = 0; w < nn1; ++w) {
        const int slot = nodes_find(b2, n2, nn2, nodes_id(b1, n1, w));
        if (slot < -1 || slot >= nn2) return false;
        const NodeRange r = nodes_range(b1, n1, w);
        if (r.start < 0 || r.len < 0 || r.start + r.len > n1) return false;
        for (int t = 0; t < r.len; ++t) {
            const int i = nodes_item(b1, n1, r.start + t);
            if (i < -1 || i >= n1) return false;
            *sum += i;
        }
    }
    return true;
}

int main() {
    const uint32_t ids[6] = {0u, 1u, (1u << 21) + 9u, (1u << 31) + 3u, 0xFFFFFFFEu, XFH_NODE_NONE};
    unsigned seed = 4321;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    long long sum = 0;
    for (int n : {1, 2, 3, 5, 63, 64, 65, 390, 515, 4096, XFH_GRID_MAX_N}) {
        std::vector<uint32_t> no(n);
        for (int i = 0; i < n; ++i) no[i] = ids[rnd() % 6];
        const size_t nb = xfh_nodes_bytes(n);
        std::vector<unsigned char> good(nb);
        CHECK(xfh_nodes_pack(no.data(), n, good.data(), nullptr) == XFH_OK);
        auto run = [&](const std::vector<unsigned char>& blob) {
            char* exact = (char*)aligned_alloc(16, nb);                                   // exactly nb bytes: the redzone starts behind the last one
            memcpy(exact, blob.data(), nb);
            const bool ok = walk(exact, n, exact, n, &sum);
            free(exact);
            return ok;
        };
        // a well-formed blob: every member the walk reaches is in the query's node
        {
            char* exact = (char*)aligned_alloc(16, nb);
            memcpy(exact, good.data(), nb);
            const int nn = nodes_count(exact, n);
            for (int i = 0; i < n; ++i) {
                const int slot = nodes_find(exact, n, nn, no[i]);
                CHECK((slot >= 0) == (no[i] != XFH_NODE_NONE));
                if (slot < 0) continue;
                const NodeRange r = nodes_range(exact, n, slot);
                bool self = false;
                for (int p = 0; p < r.len; ++p) { const int k = nodes_item(exact, n, r.start + p); CHECK(k >= 0 && no[k] == no[i]); self |= k == i; }
                CHECK(self);
            }
            free(exact);
        }
        CHECK(run(good));
        const size_t cap = ((size_t)n + 4) & ~(size_t)3, NS = 16 + cap, IT = 16 + 2 * cap;  // int32 offsets of node_start and items
        const int nn = ((const int*)good.data())[2];
        const int vals[6] = {n, -1, 1 << 30, (int)0x80000000u, n + 5, 0x7fffffff};
        // the items of every node in turn; the last node_start; a negative node_start; n_nodes
        for (int k = 0; k < nn; ++k) {
            std::vector<unsigned char> bad(good);
            int* w = (int*)bad.data();
            for (int q = w[NS + k], j = 0; q < w[NS + k + 1]; ++q, ++j) w[IT + q] = vals[j % 6];
            CHECK(run(bad));
        }
        for (int v : {1 << 30, -7, n + 1, 0}) {
            std::vector<unsigned char> bad(good);
            ((int*)bad.data())[NS + nn] = v;
            CHECK(run(bad));
            bad = good; ((int*)bad.data())[NS + (nn > 1 ? 1 : 0)] = v;
            CHECK(run(bad));
        }
        for (int v : {1 << 30, -5, n + 1, (int)0x80000000u, 0x7fffffff}) {
            std::vector<unsigned char> bad(good);
            ((int*)bad.data())[2] = v;
            CHECK(run(bad));
        }
        // every word in turn (a stride for the large blobs), and blobs of random words
        const size_t words = nb / 4;
        for (size_t wd = 0; wd < words; wd += (words > 2048 ? words / 199 + 1 : 1))
            for (int v : vals) {
                std::vector<unsigned char> bad(good);
                memcpy(bad.data() + 4 * wd, &v, 4);
                CHECK(run(bad));
            }
        for (int t = 0; t < (n > 1000 ? 3 : 40); ++t) {
            std::vector<unsigned char> bad(nb);
            for (size_t wd = 0; wd < words; ++wd) { const unsigned v = (rnd() % 3 == 0) ? rnd() % (2 * (unsigned)n + 2) : (rnd() << 8) ^ rnd(); memcpy(bad.data() + 4 * wd, &v, 4); }
            CHECK(run(bad));
        }
    }

    // xfh_bow_accept: the line of bow_math.h, on the boundaries and on hostile values (no overflow, no invalid conversion)
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const int iv[9] = {0, 1, 99, 100, 101, 255, 256, 0x7fffffff, (int)0x80000000u};
    const float rv[9] = {0.0f, 0.6f, 0.7f, 0.75f, 0.9f, 1.5f, 3.4e38f, inf, nan};
    int accepted = 0;
    for (int bi : {-1, 0, 7}) for (int b : iv) for (int s : iv) for (int th : iv) for (float r : rv) for (int fl : {0, 1}) {
        const int a = xfh_bow_accept(bi, b, s, th, r, fl);
        CHECK(a == 0 || a == 1);
        CHECK(a == (xfh_bow_accept_line(bi, b, s, th, r, fl) ? 1 : 0));
        if (bi < 0 || (fl ? b >= th : b > th)) CHECK(a == 0);
        accepted += a;
    }
    CHECK(accepted > 0);
    CHECK(xfh_bow_accept(0, 100, 256, 100, 0.6f, 0) == 1 && xfh_bow_accept(0, 100, 256, 100, 0.6f, XFH_BOW_STRICT_LOW) == 0);
    CHECK(xfh_bow_accept(0, 30, 30, 100, 0.9f, 0) == 0 && xfh_bow_accept(0, 30, 30, 100, 1.5f, 0) == 1 && xfh_bow_accept(0, 0, 0, 100, 1.5f, 0) == 0);
    // the workspace size and the argument checks of the device and host forms that return before any HIP call
    CHECK(xfh_bow_search_workspace_bytes(0, 1, 1) == 0 && xfh_bow_search_workspace_bytes(1, 1, 0) == 0 && xfh_bow_search_workspace_bytes(1, XFH_GRID_MAX_N + 1, 1) == 0);
    CHECK(xfh_bow_search_workspace_bytes(390, 515, 3) == bow_ws_layout(390, 3).bytes && bow_ws_layout(390, 3).bytes % 256 == 0);
    float row[64] = {0};
    uint8_t fl[4] = {1, 1, 1, 1};
    uint32_t four[4] = {1, 2, 3, 4};
    int o[4];
    CHECK(xfh_bow_search_device(nullptr, 1, 1, 1, 0, 0, 256, 100, 0.6f, row, fl, row, 0, row, nullptr, row, 0, row, fl, o, o, o, o, o, o) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_bow_search(nullptr, 1, 1, 0, 256, 100, 0.6f, four, fl, row, four, nullptr, row, fl, o, o, o, o, o, o) == XFH_ERR_INVALID_ARG);
    printf("asan_bow_test ok (%lld)\n", sum);
    return 0;
}
