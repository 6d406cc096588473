// search_common_test.cpp -- the lane-local pieces of xfeatslam_amd/csrc/search_common.hip.h (the XFH_HD functions every search kernel runs)
// against the obvious form, on the host, under AddressSanitizer + UBSan: klist_insert<K> against sorting the stream, top2_insert / top2_merge
// against sorting the union, descriptor_distance against xfh_descriptor_distance of the sanitizer build of libxfeat_hip
// (make -C xfeatslam_amd/csrc asan).  Exit code 0 = clean.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>
#include "xfeat_hip.h"
#include "search_common.hip.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "search_common_test: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

static u64 rng_state = 0x9E3779B97F4A7C15ull;
static u64 rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

// keys of a walk: few distinct distances, so that many keys share one, and the position in the stream (keys are distinct)
static std::vector<u64> stream(int len, int ndist) {
    std::vector<u64> s(len);
    for (int i = 0; i < len; ++i) s[i] = key_pack((int)(rnd() % ndist), (unsigned)i);
    for (int i = len - 1; i > 0; --i) std::swap(s[i], s[rnd() % (i + 1)]);         // any arrival order
    return s;
}

template <int K>
static int klist_case(int len, int ndist) {
    const std::vector<u64> s = stream(len, ndist);
    u64 lk[K];
    for (int j = 0; j < K; ++j) lk[j] = XFH_KEY_NONE;
    for (u64 k : s) klist_insert(lk, k);
    std::vector<u64> want(s);
    std::sort(want.begin(), want.end());
    want.resize(K, XFH_KEY_NONE);
    for (int j = 0; j < K; ++j) CHECK(lk[j] == want[j]);
    // the same stream with a value beside every key (what k_proj_candidates keeps): the keys end up as before and every value is its key's
    u64 lk2[K]; int ls[K];
    for (int j = 0; j < K; ++j) { lk2[j] = XFH_KEY_NONE; ls[j] = -1; }
    for (u64 k : s) klist_insert(lk2, k, ls, key_pos(k) ^ 0x5a5a);
    for (int j = 0; j < K; ++j) CHECK(lk2[j] == want[j] && ls[j] == (want[j] == XFH_KEY_NONE ? -1 : (key_pos(want[j]) ^ 0x5a5a)));
    return 0;
}
template <int K>
static int klist_all() {
    const int lens[] = {0, 1, K - 1, K, K + 1, 200};
    for (int len : lens)
        for (int ndist : {1, 3, 1000})
            for (int rep = 0; rep < 20; ++rep)
                if (klist_case<K>(len, ndist)) return 1;
    return 0;
}

static int top2_all() {
    const u64 NONE = XFH_KEY_NONE;
    for (int rep = 0; rep < 20000; ++rep) {
        // two ascending pairs from a small alphabet: duplicated distances, equal keys and sentinels on either side all occur
        u64 v[4];
        for (u64& x : v) { const u64 r = rnd() % 8; x = r >= 6 ? NONE : key_pack((int)(r % 3), (unsigned)(rnd() % 3)); }
        u64 b = std::min(v[0], v[1]), s = std::max(v[0], v[1]);
        const u64 ob = std::min(v[2], v[3]), os = std::max(v[2], v[3]);
        top2_merge(b, s, ob, os);
        std::sort(v, v + 4);
        CHECK(b == v[0] && s == v[1]);
        // the same four as a stream, from any starting point
        u64 ib = NONE, is = NONE;
        for (int i = 0; i < 4; ++i) top2_insert(ib, is, v[(i + rep) % 4]);
        CHECK(ib == v[0] && is == v[1]);
    }
    for (int len : {0, 1, 2, 3, 200}) {
        const std::vector<u64> st = stream(len, 3);
        u64 b = NONE, s = NONE;
        for (u64 k : st) top2_insert(b, s, k);
        std::vector<u64> want(st);
        std::sort(want.begin(), want.end());
        want.resize(2, NONE);
        CHECK(b == want[0] && s == want[1]);
    }
    return 0;
}

static int distance_all() {
    alignas(16) float a[64], b[64];
    for (int rep = 0; rep < 2000; ++rep) {
        const float scale = rep % 3 == 0 ? 1.0f : (rep % 3 == 1 ? 0.125f : 40.0f);   // unit rows, near rows, rows far apart (distances up to ~10^8, below 2^31)
        for (int k = 0; k < 64; ++k) {
            a[k] = scale * ((float)(rnd() % 20001) - 10000.0f) / 80000.0f;
            b[k] = rep % 7 == 0 ? a[k] : scale * ((float)(rnd() % 20001) - 10000.0f) / 80000.0f;
        }
        const int want = xfh_descriptor_distance(a, b);
        CHECK(descriptor_distance<false>(a, (const f32x4*)b) == want);
        CHECK(descriptor_distance<true>(a, (const f32x4*)b) == want);              // SAT leaves every distance the conversion can hold alone
    }
    // rows whose squared norm the conversion cannot hold: NaN, Inf, and exactly 2^31 / 512 = 4194304 (2048^2).  The non-SAT form converts
    // such a value to int, which only the device defines, so the host asks the SAT form alone; just below the edge both forms agree.
    for (int k = 0; k < 64; ++k) { a[k] = 0.0f; b[k] = 0.0f; }
    a[5] = std::numeric_limits<float>::quiet_NaN();
    CHECK(descriptor_distance<true>(a, (const f32x4*)b) == INT_MAX && descriptor_distance<true>(b, (const f32x4*)a) == INT_MAX);
    a[5] = std::numeric_limits<float>::infinity();
    CHECK(descriptor_distance<true>(a, (const f32x4*)b) == INT_MAX && descriptor_distance<true>(b, (const f32x4*)a) == INT_MAX);
    a[5] = 2048.0f;
    CHECK(descriptor_distance<true>(a, (const f32x4*)b) == INT_MAX);
    a[5] = std::nextafterf(2048.0f, 0.0f);
    const int edge = xfh_descriptor_distance(a, b);
    CHECK(edge > 0 && edge < INT_MAX && descriptor_distance<true>(a, (const f32x4*)b) == edge && descriptor_distance<false>(a, (const f32x4*)b) == edge);
    return 0;
}

int main() {
    CHECK(key_dist(key_pack(0x7fffffff, 0xFFFFFFFFu)) == 0x7fffffff && key_pos(key_pack(7, 123u)) == 123 && key_pack(1, 0u) > key_pack(0, 0xFFFFFFFFu));
    if (klist_all<2>() || klist_all<4>() || klist_all<8>() || klist_all<16>()) return 1;
    if (top2_all()) return 1;
    if (distance_all()) return 1;
    printf("search_common_test ok\n");
    return 0;
}
