// bow_test.cpp -- XFmatcher::searchByBoW (include/xfeat/ORBmatcher_xfeat.h), host and device forms, against the C ABI (xfh_bow_search) on one
// scene: three dumps that must be identical.
// usage: bow_test in.bin out.bin
// in.bin : int32 n1, n2, keyframe form (0 / 1), 0; float nn_ratio; then for side 1 and for side 2: descriptors[n * 64 f32]; node_of[n u32];
//          flags[n u8] (active1 resp. eligible2)
// out.bin: three times (C ABI, host form, device form): int32 nmatches, status[n1] (widened), match12[n1], best_dist[n1], second_dist[n1],
//          n_candidates[n1], assigned2[n2]
#define XFEAT_NO_OPENCV 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "xfeat/XFextractor.h"
#include "xfeat/ORBmatcher_xfeat.h"

using namespace ORB_SLAM3;

template <class T> static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

struct Side {
    int n = 0;
    XFmatcher::Mat desc;
    std::vector<uint32_t> node_of;
    std::vector<unsigned char> flag;
    bool read(FILE* f, int count) {
        n = count; desc = XFmatcher::Mat(n, 64, 4); node_of.resize(n); flag.resize(n);
        return rd(f, desc.ptr<float>(0), (size_t)n * 64) && rd(f, node_of.data(), n) && rd(f, flag.data(), n);
    }
};

static void dump(FILE* o, int nmatches, const std::vector<unsigned char>& status, const std::vector<int>& m, const std::vector<int>& best,
                 const std::vector<int>& second, const std::vector<int>& nc, const std::vector<int>& as2) {
    fwrite(&nmatches, 4, 1, o);
    for (unsigned char s : status) { const int v = s; fwrite(&v, 4, 1, o); }
    fwrite(m.data(), 4, m.size(), o); fwrite(best.data(), 4, best.size(), o); fwrite(second.data(), 4, second.size(), o); fwrite(nc.data(), 4, nc.size(), o);
    fwrite(as2.data(), 4, as2.size(), o);
}

// the side as the pipeline leaves it in device memory: a record's descriptor block, the node blob and the flag bytes
struct DeviceSide {
    void *rec = nullptr, *nodes = nullptr, *flag = nullptr;
    int n = 0;
    bool make(const Side& k) {
        n = k.n;
        std::vector<unsigned char> r(xfh_record_bytes(k.n), 0);
        memcpy(r.data() + xfh_record_desc_offset(k.n), k.desc.ptr<float>(0), (size_t)k.n * 256);
        std::vector<unsigned char> blob(xfh_nodes_bytes(k.n));
        if (xfh_nodes_pack(k.node_of.data(), k.n, blob.data(), nullptr) != XFH_OK) return false;
        if (xfh_dev_alloc(&rec, r.size()) || xfh_dev_alloc(&nodes, blob.size()) || xfh_dev_alloc(&flag, (size_t)k.n + 16)) return false;
        return !(xfh_memcpy_h2d(rec, r.data(), r.size()) || xfh_memcpy_h2d(nodes, blob.data(), blob.size()) || xfh_memcpy_h2d(flag, k.flag.data(), (size_t)k.n));
    }
    const float* desc() const { return (const float*)((const char*)rec + xfh_record_desc_offset(n)); }
    void free() { xfh_dev_free(rec); xfh_dev_free(nodes); xfh_dev_free(flag); }
};

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    int hdr[4]; float ratio;
    if (!f || !rd(f, hdr, 4) || !rd(f, &ratio, 1)) return 2;
    const int n1 = hdr[0], n2 = hdr[1];
    const bool keyframe = hdr[2] != 0;
    Side s1, s2;
    if (!s1.read(f, n1) || !s2.read(f, n2)) return 2;
    fclose(f);
    try {
        xfh_config cfg; xfh_config_default(&cfg);
        cfg.nfeatures = 1; cfg.max_height = 32; cfg.max_width = 32;
        xfh_ctx* ctx = nullptr;
        if (xfh_create(&cfg, &ctx) != XFH_OK) return 4;
        DeviceSide d1, d2;
        if (!d1.make(s1) || !d2.make(s2)) return 4;
        FILE* o = fopen(argv[2], "wb");
        // the C ABI, host pointers
        std::vector<unsigned char> status(n1);
        std::vector<int> m(n1), best(n1), second(n1), nc(n1), as2(n2);
        int nm = -1;
        if (xfh_bow_search(ctx, n1, n2, keyframe ? XFH_BOW_STRICT_LOW : 0, 256, XFmatcher::TH_LOW, ratio, s1.node_of.data(), s1.flag.data(), s1.desc.ptr<float>(0),
                           s2.node_of.data(), keyframe ? s2.flag.data() : nullptr, s2.desc.ptr<float>(0), status.data(), m.data(), best.data(), second.data(), nc.data(),
                           as2.data(), &nm) != XFH_OK) return 4;
        dump(o, nm, status, m, best, second, nc, as2);
        // the wrapper, host vectors
        XFmatcher matcher(ctx, ratio, true);
        std::vector<int> mq(3, 9), aq(5, 9);                                     // (stale content must go)
        const int na = matcher.searchByBoW(s1.desc, s1.node_of, s1.flag, s2.desc, s2.node_of, s2.flag, keyframe, mq, aq);
        dump(o, na, matcher.lastBoWStatus(), mq, matcher.lastBoWBestDist(), matcher.lastBoWSecondDist(), matcher.lastBoWCandidates(), aq);
        // the wrapper, device-resident sides
        mq.assign(1, 7); aq.assign(1, 7);
        const int nb = matcher.searchByBoW(n1, d1.desc(), d1.nodes, (const unsigned char*)d1.flag, n2, d2.desc(), d2.nodes, (const unsigned char*)d2.flag, keyframe, mq, aq);
        dump(o, nb, matcher.lastBoWStatus(), mq, matcher.lastBoWBestDist(), matcher.lastBoWSecondDist(), matcher.lastBoWCandidates(), aq);
        fclose(o);
        d1.free(); d2.free();
        xfh_destroy(ctx);
    } catch (const std::exception& e) { fprintf(stderr, "%s\n", e.what()); return 5; }
    return 0;
}
