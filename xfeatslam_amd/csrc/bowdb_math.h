// bowdb_math.h -- the lane-local lines of the keyframe database query (KeyFrameDatabase::DetectRelocalizationCandidates / DetectNBestCandidates,
// src/KeyFrameDatabase.cc:604-845, and L1Scoring::score, thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) over BowVectors that may hold ANYTHING.
// Plain C++, host and device: k_bowdb_score / k_bowdb_select (bowdb_query.hip.h) deal the entries of a vector to 64 lanes and xfh_bow_score
// (capi_bowdb.cpp) walks them one after the other, both through the lines below, and tests/cpp/asan_bowdb_test.cpp runs these very lines under
// AddressSanitizer on heap buffers of exactly the vectors' size.
//
// A BowVector is two arrays in ascending word id, ids[n] and vals[n] (what xfh_bow_transform_device writes).  score(v1, v2) walks both maps and
// adds one term per SHARED id, in ascending id; its lower_bound hops skip only ids that are not shared.  Here every entry of v2 looks its id up in
// v1 (a binary search), which visits the shared ids in the same order.
//
// Bounds: a word count is clamped to [0, stride] before anything is indexed (bowdb_clamp_n); the binary search halves its range and ends after
// at most 32 steps whatever the ids hold, and never returns an index past n.  Ids that are not ascending give unspecified results only.
#pragma once
#include <math.h>
#include <stdint.h>
#include "hd.h"

#define XFH_BOWDB_NO_WORD 0xFFFFFFFFu                        // first_common of two vectors that share nothing

XFH_HD int bowdb_clamp_n(int n_words, int stride) { return n_words < 0 ? 0 : (n_words > stride ? stride : n_words); }

// std::lower_bound on ids[0 .. n): the first index whose id is >= id, n if none
XFH_HD int bowdb_lower_bound(const uint32_t* ids, int n, uint32_t id) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (ids[mid] < id) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// the position of id in ids[0 .. n), or -1
XFH_HD int bowdb_find(const uint32_t* ids, int n, uint32_t id) {
    const int p = bowdb_lower_bound(ids, n, id);
    return (p < n && ids[p] == id) ? p : -1;
}

// `fabs(vi - wi) - fabs(vi) - fabs(wi)` (ScoringObject.cpp:41): vi of v1 (the query), wi of v2
XFH_HD double bowdb_term(double vi, double wi) { return (fabs(vi - wi) - fabs(vi)) - fabs(wi); }
// `score = -score/2.0` (:65): -0.0 for a sum that is still 0.0
XFH_HD double bowdb_finish(double sum) { return -sum / 2.0; }

// `int minCommonWords = maxCommonWords*0.8f;` (KeyFrameDatabase.cc:648, :769)
XFH_HD int bowdb_min_common(int max_common) { return (int)((float)max_common * 0.8f); }

// an fp32 acc as a 32-bit key whose ASCENDING order is the DESCENDING order of the floats; -0.0 and 0.0 (equal under `a.first > b.first`) get one key
XFH_HD uint32_t bowdb_desc_key(float acc) {
    union { float f; uint32_t u; } c;
    c.f = acc;
    if (acc == 0.0f) c.u = 0u;
    const uint32_t asc = (c.u & 0x80000000u) ? ~c.u : (c.u | 0x80000000u);
    return ~asc;
}

// L1Scoring::score(v1, v2) with the number of shared ids and the least of them: the entries of v2 one after the other
XFH_HD void bowdb_score_host(const uint32_t* ids1, const double* vals1, int n1, const uint32_t* ids2, const double* vals2, int n2, double* score,
                             int* n_common, uint32_t* first_common) {
    double sum = 0.0;
    int common = 0;
    uint32_t first = XFH_BOWDB_NO_WORD;
    for (int e = 0; e < n2; ++e) {
        const int p = bowdb_find(ids1, n1, ids2[e]);
        if (p < 0) continue;
        if (common++ == 0) first = ids2[e];
        sum += bowdb_term(vals1[p], vals2[e]);
    }
    *score = bowdb_finish(sum); *n_common = common; *first_common = first;
}

// the arguments of the two kernels of bowdb_query.hip.h, filled by xfh_bowdb_query_device (capi_bowdb.cpp)
struct BowDbArgs {
    int n_slots, form, nn;
    const uint32_t* q_ids; const double* q_vals; const int* q_n_words; int q_stride;        // [B][q_stride], [B]
    const uint32_t* db_ids; const double* db_vals; const int* db_n_words; int db_stride;    // [n_slots][db_stride], [n_slots]
    const uint32_t* seq; const int32_t* neigh; const uint8_t* exclude;                      // [n_slots] or null, [n_slots][nn], [B][n_slots] or null
    float* state;                                                                           // [B][n_slots], in/out
    uint32_t* first_common;                                                                 // the workspace: [B][n_slots]
    int32_t* common; double* score; uint8_t* status;                                        // [B][n_slots]
    int32_t* header; float* best_acc;                                                       // [B][XFH_BOWDB_HEADER_INTS], [B]
    int32_t* list_slot; float* list_acc; int32_t* list_best;                                // [B][n_slots]
    int32_t* cand_slot; float* cand_acc;                                                    // [B][n_slots]
};
