// bow_math.h -- the acceptance test of ORBmatcher::SearchByBoW (src/ORBmatcher.cc:512-514 for the frame form, :1033-1036 for the keyframe
// form), written ONCE for the host entry point (xfh_bow_accept; capi_bow.cpp) and the kernel (bow_search.hip.h), the workspace layout of
// xfh_bow_search_device and the kernels' argument block.
//
//   accept = best_idx >= 0 && (STRICT_LOW ? best < th_low : best <= th_low) && (float)best < nn_ratio * (float)second
//
// The integer comparisons are exact; the one float expression is two int -> fp32 conversions, one fp32 multiply and one compare.  The
// library is built with -ffp-contract=off: the line below is the IEEE operation sequence it spells, on both sides.
#pragma once
#include "projection_math.h"

XFH_HD bool xfh_bow_accept_line(int best_idx, int best, int second, int th_low, float nn_ratio, int flags) {
    return best_idx >= 0 && ((flags & XFH_BOW_STRICT_LOW) ? best < th_low : best <= th_low) && (float)best < nn_ratio * (float)second;
}

// ---- workspace of xfh_bow_search_device -----------------------------------------------------------------------------------------------
//   int counters[B][4]     per problem: queries that needed a full re-search, queries resolved, nodes resolved, 0 (zeroed by a memset on
//                          the stream before the launches; tools and tests read them, the result does not depend on them)
//   per problem, `stride` bytes apart, written by k_bow_candidates and read by k_bow_resolve:
//     int slot[n1]         the slot of the query's node in side 2's id list, -1 for a query that is INACTIVE or NO_NODE
//     int ntot[n1]         members of that node that are statically eligible
//     int nlow[n1]         those of them with a distance < init_dist: the only ones that can ever become best or second
//     int ldist[n1][K], lpos[n1][K]   the K least of those, ascending by (distance, position in the node): min(nlow, K) entries are valid
#define XFH_BOW_K 4
struct BowWs { size_t slot, ntot, nlow, ldist, lpos, stride, first, bytes; };
XFH_HD BowWs bow_ws_layout(int n1, int B) {
    const size_t al = 255;
    const size_t col = ((size_t)n1 * 4 + al) & ~al, lst = ((size_t)n1 * 4 * XFH_BOW_K + al) & ~al;
    BowWs w;
    w.slot = 0; w.ntot = col; w.nlow = 2 * col; w.ldist = 3 * col; w.lpos = 3 * col + lst; w.stride = 3 * col + 2 * lst;
    w.first = ((size_t)B * 16 + al) & ~al;
    w.bytes = w.first + (size_t)B * w.stride;
    return w;
}

// one side of the kernels (device pointers; problem b's arrays start b * elem_stride bytes of flags, b * nodes_stride resp. b * desc_stride
// bytes into each; the shared side of a call has all three at 0)
struct BowSide {
    int n;
    size_t elem_stride, nodes_stride, desc_stride;
    const char* nodes;
    const uint8_t* flag;             // [.][n]: active1 resp. eligible2 (side 2: NULL = every keypoint is eligible)
    const char* desc;                // [n][64] floats per problem
};
struct BowArgs {
    int flags, init_dist, th_low;
    float nn_ratio;
    BowSide s1, s2;
    char* ws;
    uint8_t* status; int* match12; int* best_dist; int* second_dist; int* n_candidates;   // [B][n1]
    int* assigned2;                  // [B][n2], set to -1 on the stream before the launches
    int* n_matches;                  // [B], zeroed on the stream before the launches
};
