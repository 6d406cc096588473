// bowdb_test.cpp -- XFkeyframeDatabase (include/xfeat/ORBmatcher_xfeat.h) on a database and a list of queries the Python side writes out.
// usage: bowdb_test in.bin out.bin
// in.bin : int32 n_slots, stride, nn, n_add, n_queries; per add: int32 slot, n_words, ids[u32], vals[f64], int32 neigh[nn];
//          per query: int32 form, n_words, ids[u32], vals[f64], int32 n_exclude, exclude[i32]
// out.bin: per query: int32 n_listed, max_common, min_common, n_scored, n_candidates; float best_acc; common[n i32]; score[n f64]; status[n u8];
//          list_slot[n i32]; list_acc[n f32]; list_best[n i32]; cand_slot[n i32]; cand_acc[n f32]
// then the two candidate functions on the LAST query: int32 count + slots of DetectRelocalizationCandidates, of vpLoopCand and of vpMergeCand
// (nNumCandidates = 2, the map of slot s = s % 2, the query's map = 0)
#define XFEAT_NO_OPENCV 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "xfeat/XFextractor.h"
#include "xfeat/ORBmatcher_xfeat.h"

using namespace ORB_SLAM3;

template <class T> static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
static bool rd_bow(FILE* f, XFkeyframeDatabase::BowVec* bow) {
    int nw = 0;
    if (!rd(f, &nw, 1) || nw < 0) return false;
    std::vector<uint32_t> ids(nw); std::vector<double> vals(nw);
    if (!rd(f, ids.data(), nw) || !rd(f, vals.data(), nw)) return false;
    bow->clear();
    for (int k = 0; k < nw; ++k) bow->push_back(std::make_pair(ids[k], vals[k]));
    return true;
}
static void wr_slots(FILE* o, const std::vector<int>& v) { const int c = (int)v.size(); fwrite(&c, 4, 1, o); fwrite(v.data(), 4, v.size(), o); }

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    int hdr[5];
    if (!f || !rd(f, hdr, 5)) return 2;
    const int n = hdr[0], stride = hdr[1], nn = hdr[2], n_add = hdr[3], n_queries = hdr[4];
    try {
        xfh_config cfg; xfh_config_default(&cfg);
        cfg.nfeatures = 1; cfg.max_height = 32; cfg.max_width = 32;
        xfh_ctx* ctx = nullptr;
        if (xfh_create(&cfg, &ctx) != XFH_OK) return 4;
        {
            XFkeyframeDatabase db(ctx, n, stride, nn);
            if (db.slots() != n || db.stride() != stride) return 5;
            for (int a = 0; a < n_add; ++a) {
                int slot = 0;
                XFkeyframeDatabase::BowVec bow;
                std::vector<int> neigh(nn);
                if (!rd(f, &slot, 1) || !rd_bow(f, &bow) || !rd(f, neigh.data(), nn)) return 2;
                db.add(slot, bow, neigh);
            }
            FILE* o = fopen(argv[2], "wb");
            XFkeyframeDatabase::BowVec last;
            for (int q = 0; q < n_queries; ++q) {
                int form = 0, nex = 0;
                if (!rd(f, &form, 1) || !rd_bow(f, &last) || !rd(f, &nex, 1)) return 2;
                std::vector<int> ex(nex);
                if (!rd(f, ex.data(), nex)) return 2;
                db.query(form, last, ex);
                const int h[5] = {db.nListed, db.maxCommon, db.minCommon, db.nScored, db.nCandidates};
                fwrite(h, 4, 5, o); fwrite(&db.bestAcc, 4, 1, o);
                fwrite(db.common.data(), 4, n, o); fwrite(db.score.data(), 8, n, o); fwrite(db.status.data(), 1, n, o);
                fwrite(db.listSlot.data(), 4, n, o); fwrite(db.listAcc.data(), 4, n, o); fwrite(db.listBest.data(), 4, n, o);
                fwrite(db.candSlot.data(), 4, n, o); fwrite(db.candAcc.data(), 4, n, o);
            }
            std::vector<int> maps(n), loop, merge;
            for (int s = 0; s < n; ++s) maps[s] = s % 2;
            wr_slots(o, db.DetectRelocalizationCandidates(last, maps, 0));
            db.DetectNBestCandidates(last, std::vector<int>(), loop, merge, 2, maps, 0);
            wr_slots(o, loop); wr_slots(o, merge);
            fclose(o);
            // what does not fit is refused
            bool threw = false;
            try { XFkeyframeDatabase::BowVec big(stride + 1, std::make_pair(1u, 1.0)); db.add(0, big); } catch (const std::exception&) { threw = true; }
            if (!threw) return 6;
            threw = false;
            try { XFkeyframeDatabase bad(ctx, XFH_BOWDB_MAX_SLOTS + 1, 8); } catch (const std::exception&) { threw = true; }
            if (!threw) return 6;
        }
        fclose(f);
        xfh_destroy(ctx);
    } catch (const std::exception& e) { fprintf(stderr, "%s\n", e.what()); return 5; }
    return 0;
}
