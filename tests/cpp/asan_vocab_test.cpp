// asan_vocab_test.cpp -- the host side of the vocabulary entry points under AddressSanitizer + UBSan: vocab_math.h, the very lines
// k_vocab_descend (vocab_transform.hip.h) goes down a vocabulary blob through, run over well-formed, truncated and hostile blobs that live in
// heap buffers of EXACTLY their byte count (a byte too far is a finding, a walk that does not end is a hang), xfh_vocab_pack / _unpack on
// good and refused input, and the argument checks that return before any HIP call, linked against the sanitizer build of libxfeat_hip
// (make -C xfeatslam_amd/csrc asan).  Exit code 0 = clean.
// Hostile: every index field of every slot set to 0xFFFFFFFF, to the slot itself (a self-reference), to n and to n - 1; the header's node
// count and L at their extremes; every word of the blob replaced in turn; blobs of random words.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "xfeat_hip.h"
#include "vocab_math.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "asan_vocab_test: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

static unsigned g_seed = 97531;
static unsigned rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

struct Voc {
    int L = 3;
    std::vector<uint32_t> parent, word;
    std::vector<double> weight;
    std::vector<uint8_t> desc;
    int add(uint32_t p) {
        parent.push_back(p); word.push_back((uint32_t)parent.size()); weight.push_back(0.25 + (rnd() % 1000) / 128.0);
        for (int k = 0; k < 32; ++k) desc.push_back((uint8_t)rnd());
        return (int)parent.size() - 1;
    }
    int n() const { return (int)parent.size(); }
};

// the obvious descent on the arrays themselves: children = the nodes that name the parent, ascending id
static void naive(const Voc& v, const uint8_t* row, int levelsup, uint32_t* word, uint32_t* node, double* weight) {
    const int nid_level = v.L - levelsup;
    bool have = nid_level <= 0;
    uint32_t nid = 0, cur = 0;
    for (int level = 1;; ++level) {
        int best = -1, bd = 1 << 30;
        for (int i = 1; i < v.n(); ++i) {
            if (v.parent[i] != cur) continue;
            int d = 0;
            for (int k = 0; k < 32; ++k) d += __builtin_popcount((unsigned)(v.desc[(size_t)i * 32 + k] ^ row[k]));
            if (d < bd) { bd = d; best = i; }
        }
        if (best < 0) break;
        cur = (uint32_t)best;
        if (level == nid_level) { nid = cur; have = true; }
    }
    *word = v.word[cur]; *weight = v.weight[cur]; *node = have ? nid : cur;
}

static int run_rows(const void* blob, size_t nb, const std::vector<uint8_t>& rows, long long* sum) {
    for (size_t r = 0; r + 32 <= rows.size(); r += 32)
        for (int lu : {0, 1, 4, 40}) {
            uint32_t w = 0, nd = 0; double wt = 0;
            const int rc = xfh_vocab_descend(blob, nb, lu, rows.data() + r, &w, &nd, &wt);
            if (rc != XFH_OK && rc != XFH_ERR_INVALID_ARG) return 1;
            *sum += w + nd;
        }
    return 0;
}

int main() {
    long long sum = 0;
    std::vector<Voc> vocs(3);
    {   // regular k = 3, L = 3
        Voc& v = vocs[0]; v.add(0); v.parent[0] = 0;
        for (int i = 0; i < 39; ++i) v.add((uint32_t)(i / 3));
    }
    {   // a node with 25 children, leaves at several levels, a zero-descriptor last child of the root
        Voc& v = vocs[1]; v.add(0);
        for (int i = 0; i < 5; ++i) v.add(0);
        for (int i = 0; i < 25; ++i) v.add(2);
        for (int i = 0; i < 7; ++i) v.add(8);
        for (int i = 0; i < 3; ++i) v.add(33);
        const int ph = v.add(0);
        memset(&v.desc[(size_t)ph * 32], 0, 32); v.weight[ph] = 0.0; v.word[ph] = 0;
        v.weight[9] = std::numeric_limits<double>::quiet_NaN(); v.weight[10] = -2.0;
    }
    {   // a chain of depth 32 beside a bush
        Voc& v = vocs[2]; v.L = 10; v.add(0);
        int x = v.add(0);
        for (int i = 0; i < 4; ++i) v.add(0);
        for (int i = 0; i < 31; ++i) x = v.add((uint32_t)x);
    }
    for (const Voc& v : vocs) {
        const int n = v.n();
        const size_t nb = xfh_vocab_bytes(n);
        CHECK(nb == vocab_bytes((size_t)n) && nb % 32 == 0 && vocab_fit(nb) == (size_t)n && vocab_fit(nb - 1) == (size_t)n - 1);
        unsigned char* good = (unsigned char*)malloc(nb);
        int mc = -1, dp = -1;
        CHECK(xfh_vocab_pack(n, v.L, v.parent.data(), v.word.data(), v.weight.data(), v.desc.data(), good, &mc, &dp) == XFH_OK);
        CHECK(mc >= 1 && mc <= XFH_VOCAB_MAX_CHILDREN && dp >= 1 && dp <= XFH_VOCAB_MAX_DEPTH);
        {   // deterministic, and the round trip
            std::vector<unsigned char> again(nb, 0xEE);
            CHECK(xfh_vocab_pack(n, v.L, v.parent.data(), v.word.data(), v.weight.data(), v.desc.data(), again.data(), nullptr, nullptr) == XFH_OK);
            CHECK(memcmp(again.data(), good, nb) == 0);
            std::vector<uint32_t> pa(n), wi(n); std::vector<double> wt(n); std::vector<uint8_t> de((size_t)n * 32);
            int L = 0, mc2 = 0, dp2 = 0;
            CHECK(xfh_vocab_unpack(good, nb, n, &L, pa.data(), wi.data(), wt.data(), de.data(), &mc2, &dp2) == XFH_OK);
            CHECK(L == v.L && mc2 == mc && dp2 == dp && pa[0] == 0);
            for (int i = 1; i < n; ++i)
                CHECK(pa[i] == v.parent[i] && wi[i] == v.word[i] && memcmp(&wt[i], &v.weight[i], 8) == 0 && memcmp(&de[(size_t)i * 32], &v.desc[(size_t)i * 32], 32) == 0);
            CHECK(xfh_vocab_unpack(good, nb - 1, n, &L, pa.data(), wi.data(), wt.data(), de.data(), nullptr, nullptr) == XFH_ERR_INVALID_ARG);
        }
        // rows: random, zero, every node's descriptor
        std::vector<uint8_t> rows;
        for (int r = 0; r < 40 * 32; ++r) rows.push_back((uint8_t)rnd());
        rows.insert(rows.end(), 32, 0);
        rows.insert(rows.end(), v.desc.begin(), v.desc.end());
        for (size_t r = 0; r + 32 <= rows.size(); r += 32)
            for (int lu : {0, 1, 2, 4, v.L, v.L + 1}) {
                uint32_t w0, n0, w1, n1, w2, n2; double t0, t1, t2;
                naive(v, rows.data() + r, lu, &w0, &n0, &t0);
                CHECK(xfh_vocab_descend(good, nb, lu, rows.data() + r, &w1, &n1, &t1) == XFH_OK);
                VocabView view;
                CHECK(vocab_open(good, nb, &view) && view.n == (uint32_t)n && view.L == v.L);
                uint32_t q[8];
                memcpy(q, rows.data() + r, 32);
                vocab_descend_row(view, lu, q, &w2, &n2, &t2);
                CHECK(w0 == w1 && n0 == n1 && memcmp(&t0, &t1, 8) == 0 && w0 == w2 && n0 == n2 && memcmp(&t0, &t2, 8) == 0);
            }
        rows.resize(12 * 32);
        // truncated: a buffer of exactly nt bytes
        for (size_t nt = 0; nt < nb; nt += (nt < 200 ? 1 : 37)) {
            unsigned char* cut = (unsigned char*)malloc(nt ? nt : 1);
            memcpy(cut, good, nt);
            CHECK(run_rows(cut, nt, rows, &sum) == 0);
            free(cut);
        }
        auto run = [&](const std::vector<unsigned char>& blob) {
            unsigned char* exact = (unsigned char*)malloc(nb);                              // exactly nb bytes: the redzone starts behind the last one
            memcpy(exact, blob.data(), nb);
            const int rc = run_rows(exact, nb, rows, &sum);
            free(exact);
            return rc == 0;
        };
        const std::vector<unsigned char> base(good, good + nb);
        // every index field of every slot
        for (int s = 0; s < n; ++s)
            for (int field = 0; field < 2; ++field)
                for (uint32_t val : {0xFFFFFFFFu, (uint32_t)s, (uint32_t)n, (uint32_t)n - 1u, 0u, 0x80000000u}) {
                    std::vector<unsigned char> bad(base);
                    memcpy(bad.data() + vocab_slot_off(n) + 16 * (size_t)s + 4 * field, &val, 4);
                    if (field == 0) { const uint32_t many = 0xFFFFFFFFu; memcpy(bad.data() + vocab_slot_off(n) + 16 * (size_t)s + 4, &many, 4); }
                    CHECK(run(bad));
                }
        {   // every slot names itself as its only child
            std::vector<unsigned char> bad(base);
            for (int s = 0; s < n; ++s) { const uint32_t e[2] = {(uint32_t)s, 1u}; memcpy(bad.data() + vocab_slot_off(n) + 16 * (size_t)s, e, 8); }
            CHECK(run(bad));
        }
        for (int word = 1; word <= 2; ++word)                                              // the header's node count and L
            for (uint32_t val : {0u, 1u, 0xFFFFFFFFu, 0x7FFFFFFFu, 0x80000000u, (uint32_t)n + 1u, (uint32_t)n - 1u}) {
                std::vector<unsigned char> bad(base);
                memcpy(bad.data() + 4 * word, &val, 4);
                CHECK(run(bad));
            }
        const size_t words = nb / 4;
        for (size_t wd = 0; wd < words; wd += (words > 1024 ? 7 : 1))
            for (uint32_t val : {0xFFFFFFFFu, (uint32_t)n, 0x40000000u}) {
                std::vector<unsigned char> bad(base);
                memcpy(bad.data() + 4 * wd, &val, 4);
                CHECK(run(bad));
            }
        for (int t = 0; t < 40; ++t) {
            std::vector<unsigned char> bad(nb);
            for (size_t wd = 0; wd < words; ++wd) { const unsigned val = (rnd() % 3 == 0) ? rnd() % (2 * (unsigned)n + 2) : (rnd() << 8) ^ rnd(); memcpy(bad.data() + 4 * wd, &val, 4); }
            CHECK(run(bad));
        }
        free(good);
    }

    // xfh_vocab_pack: every class of refusal
    {
        const Voc& v = vocs[0];
        const int n = v.n();
        std::vector<unsigned char> blob(xfh_vocab_bytes(n));
        auto pack = [&](int nn, int L, const std::vector<uint32_t>& pa) {
            return xfh_vocab_pack(nn, L, pa.data(), v.word.data(), v.weight.data(), v.desc.data(), blob.data(), nullptr, nullptr);
        };
        CHECK(pack(n, 3, v.parent) == XFH_OK);
        CHECK(pack(1, 3, v.parent) == XFH_ERR_INVALID_ARG && pack(0, 3, v.parent) == XFH_ERR_INVALID_ARG && pack(-4, 3, v.parent) == XFH_ERR_INVALID_ARG);
        CHECK(pack(n, 0, v.parent) == XFH_ERR_INVALID_ARG && pack(n, 11, v.parent) == XFH_ERR_INVALID_ARG && pack(n, 10, v.parent) == XFH_OK && pack(n, 1, v.parent) == XFH_OK);
        std::vector<uint32_t> pa(v.parent);
        pa[5] = 5; CHECK(pack(n, 3, pa) == XFH_ERR_INVALID_ARG);                           // parent[i] == i
        pa[5] = 6; CHECK(pack(n, 3, pa) == XFH_ERR_INVALID_ARG);                           // parent[i] > i
        pa[5] = 0xFFFFFFFFu; CHECK(pack(n, 3, pa) == XFH_ERR_INVALID_ARG);
        pa = v.parent; pa[1] = 1; CHECK(pack(n, 3, pa) == XFH_ERR_INVALID_ARG);             // (the only way to a root without children is parent[1] != 0)
        pa.assign(n, 0); CHECK(pack(34, 3, pa) == XFH_ERR_INVALID_ARG && pack(33, 3, pa) == XFH_OK);   // 33 resp. 32 children of the root
        for (int i = 1; i < n; ++i) pa[i] = (uint32_t)i - 1u;                               // a chain: depth n - 1
        CHECK(pack(34, 3, pa) == XFH_ERR_INVALID_ARG && pack(33, 3, pa) == XFH_OK);
        CHECK(xfh_vocab_pack(n, 3, nullptr, v.word.data(), v.weight.data(), v.desc.data(), blob.data(), nullptr, nullptr) == XFH_ERR_INVALID_ARG);
        CHECK(xfh_vocab_pack(n, 3, v.parent.data(), v.word.data(), v.weight.data(), v.desc.data(), nullptr, nullptr, nullptr) == XFH_ERR_INVALID_ARG);
        CHECK(xfh_vocab_bytes(0) == 0 && xfh_vocab_bytes(-1) == 0 && xfh_vocab_bytes(2) == vocab_bytes(2));
    }
    // the workspace size and the argument checks of the device and host forms that return before any HIP call
    CHECK(xfh_bow_transform_workspace_bytes(0, 1) == 0 && xfh_bow_transform_workspace_bytes(1, 0) == 0 && xfh_bow_transform_workspace_bytes(XFH_GRID_MAX_N + 1, 1) == 0);
    CHECK(xfh_bow_transform_workspace_bytes(257, 3) >= 3 * 257 * 8 && xfh_bow_transform_workspace_bytes(257, 3) % 256 == 0);
    alignas(16) float row[64] = {0};
    uint32_t u[4]; double d[4]; int o[4];
    CHECK(xfh_bow_transform_device(nullptr, 1, 1, 4, 0, row, 4096, row, 0, row, u, u, d, row, u, d, o) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_bow_transform(nullptr, 1, 4, 0, row, 4096, row, u, u, d, row, u, d, o) == XFH_ERR_INVALID_ARG);
    uint32_t w; double wt;
    CHECK(xfh_vocab_descend(nullptr, 100, 4, row, &w, &w, &wt) == XFH_ERR_INVALID_ARG && xfh_vocab_descend(row, 256, -1, row, &w, &w, &wt) == XFH_ERR_INVALID_ARG);
    printf("asan_vocab_test ok (%lld)\n", sum);
    return 0;
}
