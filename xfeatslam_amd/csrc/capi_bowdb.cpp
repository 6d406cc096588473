// capi_bowdb.cpp -- the keyframe database entry points of include/xfeat_hip.h: L1Scoring::score on the host (bowdb_math.h, the kernel's own
// lines), the workspace size, the device form of DetectRelocalizationCandidates / DetectNBestCandidates and the host-pointer form (host_stage.h).
#include "host_stage.h"
#include "bowdb_math.h"

static size_t query_ws_stride(int n_slots) { return ((size_t)n_slots * sizeof(uint32_t) + 255) & ~(size_t)255; }
// what xfh_bowdb_query_device and xfh_bowdb_query check alike before anything is staged or launched (the pointers are theirs to check)
static bool query_args_ok(int B, int n_slots, int form, int q_stride, int db_stride, int nn) {
    return B >= 1 && B <= 65535 && n_slots >= 1 && n_slots <= XFH_BOWDB_MAX_SLOTS && (form == XFH_BOWDB_FORM_RELOC || form == XFH_BOWDB_FORM_NBEST) &&
           q_stride >= 1 && q_stride <= XFH_GRID_MAX_N && db_stride >= 1 && db_stride <= XFH_GRID_MAX_N && nn >= 0 && nn <= XFH_BOWDB_MAX_NEIGHBOURS;
}

extern "C" {

int xfh_bow_score(const uint32_t* ids1, const double* vals1, int n1, const uint32_t* ids2, const double* vals2, int n2, double* score,
                  int* n_common, uint32_t* first_common) {
    if (n1 < 0 || n2 < 0 || !score || !n_common || !first_common) return XFH_ERR_INVALID_ARG;
    if ((n1 > 0 && (!ids1 || !vals1)) || (n2 > 0 && (!ids2 || !vals2))) return XFH_ERR_INVALID_ARG;
    bowdb_score_host(ids1, vals1, n1, ids2, vals2, n2, score, n_common, first_common);
    return XFH_OK;
}

size_t xfh_bowdb_query_workspace_bytes(int n_slots, int B) {
    if (B < 1 || B > 65535 || n_slots < 1 || n_slots > XFH_BOWDB_MAX_SLOTS) return 0;
    return (size_t)B * query_ws_stride(n_slots);
}

int xfh_bowdb_query_device(xfh_ctx* c, int B, int n_slots, int form, const uint32_t* d_q_ids, const double* d_q_vals, const int* d_q_n_words,
                           int q_stride, const uint32_t* d_db_ids, const double* d_db_vals, const int* d_db_n_words, int db_stride,
                           const uint32_t* d_seq, const int32_t* d_neigh, int nn, const uint8_t* d_exclude, float* d_state, void* d_workspace,
                           int32_t* d_common, double* d_score, uint8_t* d_status, int32_t* d_header, float* d_best_acc, int32_t* d_list_slot,
                           float* d_list_acc, int32_t* d_list_best, int32_t* d_cand_slot, float* d_cand_acc) {
    if (!c || !query_args_ok(B, n_slots, form, q_stride, db_stride, nn)) return XFH_ERR_INVALID_ARG;
    if (!d_q_ids || !d_q_vals || !d_q_n_words || !d_db_ids || !d_db_vals || !d_db_n_words || (nn > 0 && !d_neigh) || !d_state || !d_workspace ||
        !d_common || !d_score || !d_status || !d_header || !d_best_acc || !d_list_slot || !d_list_acc || !d_list_best || !d_cand_slot || !d_cand_acc)
        return XFH_ERR_INVALID_ARG;
    if (misaligned(15, d_workspace) || misaligned(7, d_q_vals, d_db_vals, d_score) ||
        misaligned(3, d_q_ids, d_q_n_words, d_db_ids, d_db_n_words, d_seq, d_neigh, d_state, d_common, d_header, d_best_acc, d_list_slot, d_list_acc,
                   d_list_best, d_cand_slot, d_cand_acc)) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    BowDbArgs a = {};
    a.n_slots = n_slots; a.form = form; a.nn = nn;
    a.q_ids = d_q_ids; a.q_vals = d_q_vals; a.q_n_words = d_q_n_words; a.q_stride = q_stride;
    a.db_ids = d_db_ids; a.db_vals = d_db_vals; a.db_n_words = d_db_n_words; a.db_stride = db_stride;
    a.seq = d_seq; a.neigh = d_neigh; a.exclude = d_exclude; a.state = d_state;
    a.first_common = (uint32_t*)d_workspace;                              // [B][n_slots], the problems back to back
    a.common = d_common; a.score = d_score; a.status = d_status; a.header = d_header; a.best_acc = d_best_acc;
    a.list_slot = d_list_slot; a.list_acc = d_list_acc; a.list_best = d_list_best; a.cand_slot = d_cand_slot; a.cand_acc = d_cand_acc;
    HIPCK(c, launch_bowdb_query(c, a, B));
    return XFH_OK;
}

int xfh_bowdb_query(xfh_ctx* c, int n_slots, int form, const uint32_t* q_ids, const double* q_vals, int q_n_words, const uint32_t* db_ids,
                    const double* db_vals, const int* db_n_words, int db_stride, const uint32_t* seq, const int32_t* neigh, int nn,
                    const uint8_t* exclude, float* state, int32_t* common, double* score, uint8_t* status, int32_t* header, float* best_acc,
                    int32_t* list_slot, float* list_acc, int32_t* list_best, int32_t* cand_slot, float* cand_acc) {
    const int q_stride = q_n_words < 1 ? 1 : q_n_words;                    // the query's arrays hold q_n_words entries
    if (!c || q_n_words < 0 || !query_args_ok(1, n_slots, form, q_stride, db_stride, nn)) return XFH_ERR_INVALID_ARG;
    if ((q_n_words > 0 && (!q_ids || !q_vals)) || !db_ids || !db_vals || !db_n_words || (nn > 0 && !neigh) || !state || !common || !score || !status ||
        !header || !best_acc || !list_slot || !list_acc || !list_best || !cand_slot || !cand_acc) return XFH_ERR_INVALID_ARG;
    const size_t ns = (size_t)n_slots;
    HostStage s{c};
    auto dqi = s.in<uint32_t>(q_ids, (size_t)q_n_words * 4);
    auto dqv = s.in<double>(q_vals, (size_t)q_n_words * 8);
    auto dqn = s.in<int>(&q_n_words, 4);
    auto ddi = s.in<uint32_t>(db_ids, ns * db_stride * 4);
    auto ddv = s.in<double>(db_vals, ns * db_stride * 8);
    auto ddn = s.in<int>(db_n_words, ns * 4);
    auto dsq = s.in_opt<uint32_t>(seq, ns * 4);
    auto dng = s.in_opt<int32_t>(nn > 0 ? neigh : nullptr, ns * nn * 4);
    auto dex = s.in_opt<uint8_t>(exclude, ns);
    auto dst = s.add<float>(ns * 4, state, state, false);                 // in/out
    auto dws = s.tmp<char>(query_ws_stride(n_slots));
    auto dcm = s.out<int32_t>(common, ns * 4), dls = s.out<int32_t>(list_slot, ns * 4), dlb = s.out<int32_t>(list_best, ns * 4),
         dcs = s.out<int32_t>(cand_slot, ns * 4), dhd = s.out<int32_t>(header, XFH_BOWDB_HEADER_INTS * 4);
    auto dsc = s.out<double>(score, ns * 8);
    auto dss = s.out<uint8_t>(status, ns);
    auto dla = s.out<float>(list_acc, ns * 4), dca = s.out<float>(cand_acc, ns * 4), dba = s.out<float>(best_acc, 4);
    if (const int rc = s.upload(); rc != XFH_OK) return rc;
    const int rc = xfh_bowdb_query_device(c, 1, n_slots, form, dqi, dqv, dqn, q_stride, ddi, ddv, ddn, db_stride, dsq, dng, nn, dex, dst, dws, dcm, dsc,
                                          dss, dhd, dba, dls, dla, dlb, dcs, dca);
    if (rc != XFH_OK) return rc;                                              // (a HIP error: every argument check has passed above)
    return s.download();
}

}  // extern "C"
