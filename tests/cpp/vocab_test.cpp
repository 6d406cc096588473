// vocab_test.cpp -- XFvocabulary (include/xfeat/ORBmatcher_xfeat.h): the Mat overload and the form on rows that live in a record in device
// memory, against the C ABI (xfh_vocab_pack + xfh_bow_transform) on one vocabulary and one frame: three dumps that must be identical.
// usage: vocab_test in.bin out.bin
// in.bin : int32 n_nodes, L, n, levelsup; parent[n_nodes u32]; word_id[n_nodes u32]; weight[n_nodes f64]; desc[n_nodes * 32 u8]; rows[n * 64 f32]
// out.bin: three times (C ABI, Mat overload, device rows): int32 n_words; node_of[n u32]; bow ids[n u32] (0xFFFFFFFF past n_words);
//          bow values[n f64] (0 past n_words); the node blob [xfh_nodes_bytes(n) bytes]
#define XFEAT_NO_OPENCV 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "xfeat/XFextractor.h"
#include "xfeat/ORBmatcher_xfeat.h"

using namespace ORB_SLAM3;

template <class T> static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

static void dump(FILE* o, int n, int nw, const std::vector<uint32_t>& nodeOf, const std::vector<std::pair<uint32_t, double>>& bow, const std::vector<unsigned char>& nodes) {
    std::vector<uint32_t> ids(n, 0xFFFFFFFFu); std::vector<double> vals(n, 0.0);
    for (size_t k = 0; k < bow.size() && k < (size_t)n; ++k) { ids[k] = bow[k].first; vals[k] = bow[k].second; }
    fwrite(&nw, 4, 1, o); fwrite(nodeOf.data(), 4, n, o); fwrite(ids.data(), 4, n, o); fwrite(vals.data(), 8, n, o); fwrite(nodes.data(), 1, nodes.size(), o);
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    int hdr[4];
    if (!f || !rd(f, hdr, 4)) return 2;
    const int nn = hdr[0], L = hdr[1], n = hdr[2], levelsup = hdr[3];
    std::vector<uint32_t> parent(nn), word(nn);
    std::vector<double> weight(nn);
    std::vector<unsigned char> desc((size_t)nn * 32);
    XFvocabulary::Mat rows(n, 64, 4);
    if (!rd(f, parent.data(), nn) || !rd(f, word.data(), nn) || !rd(f, weight.data(), nn) || !rd(f, desc.data(), desc.size()) || !rd(f, rows.ptr<float>(0), (size_t)n * 64)) return 2;
    fclose(f);
    try {
        xfh_config cfg; xfh_config_default(&cfg);
        cfg.nfeatures = 1; cfg.max_height = 32; cfg.max_width = 32;
        xfh_ctx* ctx = nullptr;
        if (xfh_create(&cfg, &ctx) != XFH_OK) return 4;
        FILE* o = fopen(argv[2], "wb");
        const size_t nb = xfh_nodes_bytes(n);
        // the C ABI, host pointers
        {
            std::vector<unsigned char> blob(xfh_vocab_bytes(nn)), nodes(nb);
            if (xfh_vocab_pack(nn, L, parent.data(), word.data(), weight.data(), desc.data(), blob.data(), nullptr, nullptr) != XFH_OK) return 4;
            std::vector<uint32_t> w(n), no(n), ids(n);
            std::vector<double> wt(n), vals(n);
            int nw = -1;
            if (xfh_bow_transform(ctx, n, levelsup, XFH_BOWT_TF_IDF_L1, blob.data(), blob.size(), rows.ptr<float>(0), w.data(), no.data(), wt.data(), nodes.data(), ids.data(),
                                  vals.data(), &nw) != XFH_OK) return 4;
            std::vector<std::pair<uint32_t, double>> bow;
            for (int k = 0; k < nw; ++k) bow.push_back(std::make_pair(ids[k], vals[k]));
            dump(o, n, nw, no, bow, nodes);
        }
        XFvocabulary voc(ctx, L, parent, word, weight, desc);
        if (voc.size() != nn || voc.levels() != L) return 5;
        std::vector<unsigned char> nodes(nb, 0xEE);
        // the wrapper, host rows
        int nw = voc.transform(rows, levelsup);
        if (voc.rows() != n || xfh_memcpy_d2h(nodes.data(), voc.deviceNodes(), nb) != XFH_OK) return 4;
        dump(o, n, nw, voc.nodeOf(), voc.bowVec(), nodes);
        // the wrapper, rows as the pipeline leaves them in device memory: the descriptor block of a record
        std::vector<unsigned char> rec(xfh_record_bytes(n), 0);
        memcpy(rec.data() + xfh_record_desc_offset(n), rows.ptr<float>(0), (size_t)n * 256);
        void* d_rec = nullptr;
        if (xfh_dev_alloc(&d_rec, rec.size()) != XFH_OK || xfh_memcpy_h2d(d_rec, rec.data(), rec.size()) != XFH_OK) return 4;
        nodes.assign(nb, 0xEE);
        nw = voc.transform((const float*)((const char*)d_rec + xfh_record_desc_offset(n)), n, levelsup);
        if (xfh_memcpy_d2h(nodes.data(), voc.deviceNodes(), nb) != XFH_OK) return 4;
        dump(o, n, nw, voc.nodeOf(), voc.bowVec(), nodes);
        fclose(o);
        xfh_dev_free(d_rec);
        // a refused vocabulary throws
        bool threw = false;
        try { std::vector<uint32_t> bad(parent); bad[1] = 1; XFvocabulary v2(ctx, L, bad, word, weight, desc); } catch (const std::exception&) { threw = true; }
        if (!threw) return 6;
        xfh_destroy(ctx);
    } catch (const std::exception& e) { fprintf(stderr, "%s\n", e.what()); return 5; }
    return 0;
}
