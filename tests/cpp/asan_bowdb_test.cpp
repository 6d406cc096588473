// asan_bowdb_test.cpp -- the host side of the keyframe database entry points under AddressSanitizer + UBSan: bowdb_math.h, the very lines
// k_bowdb_score and k_bowdb_select (bowdb_query.hip.h) run per lane, over well-formed and hostile BowVectors that live in heap buffers of
// EXACTLY their size (an entry too far is a finding, a search that does not end is a hang), xfh_bow_score on good and refused input and the
// argument checks that return before any HIP call, linked against the sanitizer build of libxfeat_hip (make -C xfeatslam_amd/csrc asan).
// Exit code 0 = clean.
// Hostile: n_words far beyond the stride and below zero (clamped before use), ids descending, ids all equal, ids random, NaN and Inf values.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "xfeat_hip.h"
#include "xfeat_hip_bench.h"
#include "bowdb_math.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "asan_bowdb_test: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

static unsigned g_seed = 24680;
static unsigned rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

struct Vec {                                                            // heap buffers of exactly n entries
    uint32_t* ids; double* vals; int n;
    explicit Vec(int n_) : ids((uint32_t*)malloc(n_ ? 4 * (size_t)n_ : 1)), vals((double*)malloc(n_ ? 8 * (size_t)n_ : 1)), n(n_) {}
    ~Vec() { free(ids); free(vals); }
    void ascending(uint32_t universe) {
        uint32_t id = rnd() % 3;
        for (int i = 0; i < n; ++i) { ids[i] = id; id += 1 + rnd() % (universe / (n + 1) + 1); vals[i] = (1 + rnd() % 1000) / 4096.0 / (n + 1); }
    }
};

// L1Scoring::score as the reference writes it: two cursors, lower_bound hops
static double naive(const Vec& a, const Vec& b, int* common, uint32_t* first) {
    int i = 0, j = 0;
    double s = 0;
    *common = 0; *first = 0xFFFFFFFFu;
    while (i != a.n && j != b.n) {
        if (a.ids[i] == b.ids[j]) {
            s += fabs(a.vals[i] - b.vals[j]) - fabs(a.vals[i]) - fabs(b.vals[j]);
            if ((*common)++ == 0) *first = a.ids[i];
            ++i; ++j;
        } else if (a.ids[i] < b.ids[j]) { while (i != a.n && a.ids[i] < b.ids[j]) ++i; }
        else { while (j != b.n && b.ids[j] < a.ids[i]) ++j; }
    }
    return -s / 2.0;
}

static bool same_bits(double a, double b) { return memcmp(&a, &b, 8) == 0; }

int main() {
    // ---- well-formed vectors: the kernel's lines against the reference's walk, bit for bit
    long long total = 0;
    for (int t = 0; t < 400; ++t) {
        Vec a((int)(rnd() % 300)), b((int)(rnd() % 300));
        a.ascending(600); b.ascending(600);
        double s = 0; int c = 0; uint32_t f = 0, wf = 0; int wc = 0;
        CHECK(xfh_bow_score(a.ids, a.vals, a.n, b.ids, b.vals, b.n, &s, &c, &f) == XFH_OK);
        const double w = naive(a, b, &wc, &wf);
        CHECK(same_bits(s, w) && c == wc && f == wf);
        total += c;
    }
    CHECK(total > 2000);
    {   // nothing shared: -0.0; an empty side; identical vectors
        Vec a(5), b(0);
        a.ascending(50);
        double s = 1; int c = 1; uint32_t f = 0;
        CHECK(xfh_bow_score(a.ids, a.vals, a.n, nullptr, nullptr, 0, &s, &c, &f) == XFH_OK && same_bits(s, -0.0) && c == 0 && f == 0xFFFFFFFFu);
        CHECK(xfh_bow_score(nullptr, nullptr, 0, a.ids, a.vals, a.n, &s, &c, &f) == XFH_OK && same_bits(s, -0.0) && c == 0);
        CHECK(xfh_bow_score(a.ids, a.vals, a.n, a.ids, a.vals, a.n, &s, &c, &f) == XFH_OK && c == 5 && f == a.ids[0] && s > 0);
    }
    // ---- hostile: the word count is clamped before use, the search ends and stays inside whatever the ids hold
    CHECK(bowdb_clamp_n(1 << 30, 7) == 7 && bowdb_clamp_n(-5, 7) == 0 && bowdb_clamp_n(8, 7) == 7 && bowdb_clamp_n(3, 7) == 3 &&
          bowdb_clamp_n(std::numeric_limits<int>::min(), 1) == 0 && bowdb_clamp_n(std::numeric_limits<int>::max(), 16384) == 16384);
    for (int t = 0; t < 300; ++t) {
        const int stride = 1 + (int)(rnd() % 130);
        Vec a(stride), b(stride);
        const int mode = t % 4;
        for (int i = 0; i < stride; ++i) {
            a.ids[i] = mode == 0 ? (uint32_t)(stride - i) : mode == 1 ? 7u : mode == 2 ? rnd() % 16 : 0xFFFFFFFFu - (uint32_t)i;
            b.ids[i] = mode == 3 ? rnd() : (uint32_t)(rnd() % 16);
            a.vals[i] = i % 5 == 0 ? std::numeric_limits<double>::quiet_NaN() : (i % 7 == 0 ? std::numeric_limits<double>::infinity() : -1.5 * i);
            b.vals[i] = (double)rnd();
        }
        const int claims[] = {stride + 1, 1 << 30, -1, stride, std::numeric_limits<int>::max()};
        for (int claim : claims) {
            const int n1 = bowdb_clamp_n(claim, stride), n2 = bowdb_clamp_n(claim, stride);
            double s = 0; int c = -1; uint32_t f = 0;
            bowdb_score_host(a.ids, a.vals, n1, b.ids, b.vals, n2, &s, &c, &f);
            CHECK(c >= 0 && c <= n2);
            for (int i = 0; i < n2; ++i) { const int p = bowdb_lower_bound(a.ids, n1, b.ids[i]); CHECK(p >= 0 && p <= n1); }
        }
    }
    // ---- the threshold and the descending key
    CHECK(bowdb_min_common(0) == 0 && bowdb_min_common(1) == 0 && bowdb_min_common(4) == 3 && bowdb_min_common(5) == 4 && bowdb_min_common(6) == 4 &&
          bowdb_min_common(10) == 8 && bowdb_min_common(16384) == 13107);
    const float fl[] = {std::numeric_limits<float>::infinity(), 3.5f, 1.0f, 1e-30f, 0.0f, -1e-30f, -2.0f, -std::numeric_limits<float>::infinity()};
    for (size_t i = 0; i + 1 < sizeof fl / sizeof *fl; ++i) CHECK(bowdb_desc_key(fl[i]) < bowdb_desc_key(fl[i + 1]));
    CHECK(bowdb_desc_key(0.0f) == bowdb_desc_key(-0.0f));
    CHECK(same_bits(bowdb_finish(0.0), -0.0) && same_bits(bowdb_term(0.25, 0.5), -0.5));
    // ---- refusals that return before any HIP call
    {
        uint32_t id[2] = {1, 2}; double v[2] = {0.5, 0.5}; double s; int c; uint32_t f;
        CHECK(xfh_bow_score(id, v, -1, id, v, 2, &s, &c, &f) == XFH_ERR_INVALID_ARG && xfh_bow_score(id, v, 2, id, v, -1, &s, &c, &f) == XFH_ERR_INVALID_ARG);
        CHECK(xfh_bow_score(nullptr, v, 2, id, v, 2, &s, &c, &f) == XFH_ERR_INVALID_ARG && xfh_bow_score(id, v, 2, id, nullptr, 2, &s, &c, &f) == XFH_ERR_INVALID_ARG);
        CHECK(xfh_bow_score(id, v, 2, id, v, 2, nullptr, &c, &f) == XFH_ERR_INVALID_ARG && xfh_bow_score(id, v, 2, id, v, 2, &s, nullptr, &f) == XFH_ERR_INVALID_ARG &&
              xfh_bow_score(id, v, 2, id, v, 2, &s, &c, nullptr) == XFH_ERR_INVALID_ARG);
        CHECK(xfh_bowdb_query_workspace_bytes(0, 1) == 0 && xfh_bowdb_query_workspace_bytes(XFH_BOWDB_MAX_SLOTS + 1, 1) == 0 &&
              xfh_bowdb_query_workspace_bytes(5, 0) == 0 && xfh_bowdb_query_workspace_bytes(5, 65536) == 0 &&
              xfh_bowdb_query_workspace_bytes(300, 3) % 256 == 0 && xfh_bowdb_query_workspace_bytes(300, 3) >= 3 * 300 * 4);
        alignas(16) char p[64] = {};
        CHECK(xfh_bowdb_query_device(nullptr, 1, 1, XFH_BOWDB_FORM_RELOC, (uint32_t*)p, (double*)p, (int*)p, 1, (uint32_t*)p, (double*)p, (int*)p, 1, nullptr, nullptr,
                                     0, nullptr, (float*)p, p, (int32_t*)p, (double*)p, (uint8_t*)p, (int32_t*)p, (float*)p, (int32_t*)p, (float*)p, (int32_t*)p,
                                     (int32_t*)p, (float*)p) == XFH_ERR_INVALID_ARG);
        CHECK(strcmp(xfh_kernel_name(XFH_K_BOWDB_SCORE), "k_bowdb_score") == 0 && strcmp(xfh_kernel_name(XFH_K_BOWDB_SELECT), "k_bowdb_select") == 0 &&
              XFH_K_BOWDB_SCORE == 33 && XFH_K_VOCAB_FINISH == 32);
    }
    printf("asan_bowdb_test: ok (%lld shared words)\n", total);
    return 0;
}
