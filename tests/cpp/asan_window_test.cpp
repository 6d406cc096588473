// asan_window_test.cpp -- the host side of the frame-grid entry points, linked against the sanitizer build of libxfeat_hip
// (make -C xfeatslam_amd/csrc asan): xfh_grid_unpack on well-formed, truncated and inconsistent blobs, xfh_grid_bytes, and the
// argument checks that return before any HIP call.  AddressSanitizer / UBSan abort on any finding, so exit code 0 = clean.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "xfeat_hip.h"
#include "xfeat_hip_bench.h"
#include "grid_blob.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "asan_window_test: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

static const int CELLS = XFH_GRID_COLS * XFH_GRID_ROWS;
static const size_t CS_OFF = XFH_GRID_CS_OFF, ITEMS_OFF = XFH_GRID_ITEMS_OFF;

int main() {
    CHECK(xfh_grid_bytes(0) == ITEMS_OFF && xfh_grid_bytes(-1) == 0 && xfh_grid_bytes(XFH_GRID_MAX_N) == ITEMS_OFF + 16 * (size_t)XFH_GRID_MAX_N);
    CHECK(strcmp(xfh_kernel_name(XFH_K_GRID_BUILD), "k_grid_build") == 0 && strcmp(xfh_kernel_name(XFH_K_SEARCH_WINDOW), "k_search_window") == 0);
    // a well-formed blob of n = 8 slots: slots 5, 2 in cell 0, slot 7 in cell 49, slot 0 in the last cell; 4 slots not binned
    const int n = GRID_BLOB_N;
    std::vector<unsigned char> blob = example_grid_blob();
    CHECK(blob.size() == xfh_grid_bytes(n));
    std::vector<int> ocs(CELLS + 1), oit(n);
    int nb = -1;
    CHECK(xfh_grid_unpack(blob.data(), blob.size(), n, ocs.data(), oit.data(), &nb) == XFH_OK && nb == 4);
    CHECK(ocs[0] == 0 && ocs[1] == 2 && ocs[50] == 3 && ocs[CELLS] == 4 && oit[0] == 2 && oit[3] == 0 && oit[4] == -1);
    CHECK(xfh_grid_unpack(blob.data(), blob.size(), n, ocs.data(), oit.data(), nullptr) == XFH_OK);
    // truncated: every shorter length is refused without reading past it (the copies below are exactly that long)
    for (size_t len : {(size_t)0, (size_t)1, (size_t)63, (size_t)64, ITEMS_OFF - 1, ITEMS_OFF, blob.size() - 1}) {
        std::vector<unsigned char> t(blob.begin(), blob.begin() + len);
        CHECK(xfh_grid_unpack(t.data() ? t.data() : blob.data(), len, n, ocs.data(), oit.data(), &nb) == XFH_ERR_INVALID_ARG);
    }
    CHECK(xfh_grid_unpack(nullptr, blob.size(), n, ocs.data(), oit.data(), &nb) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_grid_unpack(blob.data(), blob.size(), n, nullptr, oit.data(), &nb) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_grid_unpack(blob.data(), blob.size(), n, ocs.data(), nullptr, &nb) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_grid_unpack(blob.data(), blob.size(), -1, ocs.data(), oit.data(), &nb) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_grid_unpack(blob.data(), blob.size(), n - 1, ocs.data(), oit.data(), &nb) == XFH_ERR_INVALID_ARG);      // header n differs
    // inconsistent contents
    struct Patch { size_t off; int val; };
    const Patch patches[] = {{0, 0}, {4, 1 << 30}, {8, n + 1}, {8, -1}, {CS_OFF, 1}, {CS_OFF + 4 * 10, 1 << 30}, {CS_OFF + 4 * 10, -(1 << 30)}, {CS_OFF + 4 * 60, 2},
                             {CS_OFF + 4 * (size_t)CELLS, 3}, {ITEMS_OFF, n}, {ITEMS_OFF + 16, -1}, {ITEMS_OFF + 48, 1 << 30}};
    for (const Patch& p : patches) {
        std::vector<unsigned char> bad(blob);
        memcpy(bad.data() + p.off, &p.val, 4);
        CHECK(xfh_grid_unpack(bad.data(), bad.size(), n, ocs.data(), oit.data(), &nb) == XFH_ERR_INVALID_ARG);
    }
    // a blob that claims far more than it holds
    { std::vector<unsigned char> bad(blob); int big = 1 << 28; memcpy(bad.data() + 4, &big, 4); memcpy(bad.data() + 8, &big, 4);
      CHECK(xfh_grid_unpack(bad.data(), bad.size(), big, ocs.data(), oit.data(), &nb) == XFH_ERR_INVALID_ARG); }
    // argument checks that come before any HIP call
    xfh_grid_bounds gb = {0.f, 0.f, 640.f, 480.f};
    int dummy[16] = {0};
    CHECK(xfh_grid_build_device(nullptr, (const xfh_keypoint*)dummy, 1, nullptr, &gb, 0, dummy) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_grid_build_records_device(nullptr, dummy, 1, &gb, 0, dummy) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_search_window_device(nullptr, (float*)dummy, (float*)dummy, 1, dummy, (float*)dummy, 1, nullptr, nullptr, nullptr, 256, dummy, dummy, dummy, dummy, dummy) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_search_window(nullptr, (float*)dummy, (float*)dummy, 1, (const xfh_keypoint*)dummy, &gb, (float*)dummy, 1, nullptr, nullptr, nullptr, 256, dummy, dummy, dummy, dummy, dummy) == XFH_ERR_INVALID_ARG);
    printf("asan_window_test ok\n");
    return 0;
}
