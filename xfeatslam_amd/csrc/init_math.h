// init_math.h -- the acceptance test of ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:887-889), written ONCE for the host entry
// point (xfh_init_accept; capi_init.cpp) and the kernels (init_search.hip.h), the workspace layout of xfh_init_search_device and the
// kernels' argument block.
//
//   accept = best != INT_MAX && best <= th_low && (float)best < (float)second * nn_ratio
//
// best == INT_MAX is "no member was tested" (bestIdx2 == -1); the reference relies on TH_LOW < INT_MAX for that.
//
// The integer comparison is exact; the float expression is two int -> fp32 conversions, one fp32 multiply and one compare, `second`
// first as the reference writes it.  second == INT_MAX (no second candidate) converts to 2^31.  The library is built with
// -ffp-contract=off: the line below is the IEEE operation sequence it spells, on both sides.
#pragma once
#include "projection_math.h"

XFH_HD bool xfh_init_accept_line(int best, int second, int th_low, float nn_ratio) {
    return best != 0x7fffffff && best <= th_low && (float)best < (float)second * nn_ratio;
}

// entries of a query's candidate list: its nearest window members ordered by (dist, visiting position).  The measurement behind it is
// profiles/init_search.md; a build with another value (-DXFH_INIT_K=n, 2 .. 16) is the same library with another list length.
#ifndef XFH_INIT_K
#define XFH_INIT_K 8
#endif
#define XFH_INIT_NONE 0x7fffffff                                       // INT_MAX: the reference's initial distances

// workspace of one problem: header (rounds, full re-searches, lists that ran out, K), centre[nq] (u, v, r, 0: the window of the query,
// copied so that prev_out may alias prev_matched), the K-lists, the window sizes, the re-search list, the resolver's state (claim, dist:
// what the query wrote when its turn came, -1 / INT_MAX for a query that did not accept), and the chains of the final state: head[nt]
// (an acceptor of the keypoint or -1) and next[nq] (the next acceptor of the same keypoint or -1)
struct InitWs { size_t centre, ldist, lidx, ntot, redo, claim, dist, head, next, bytes; };
XFH_HD InitWs init_ws_layout(int nq, int nt) {
    InitWs w;
    w.centre = 16;
    w.ldist = w.centre + (size_t)nq * 16;
    w.lidx = w.ldist + (size_t)nq * XFH_INIT_K * 4;
    w.ntot = w.lidx + (size_t)nq * XFH_INIT_K * 4;
    w.redo = w.ntot + (size_t)nq * 4;
    w.claim = w.redo + (size_t)nq * 4;
    w.dist = w.claim + (size_t)nq * 4;
    w.head = w.dist + (size_t)nq * 4;
    w.next = w.head + (size_t)nt * 4;
    w.bytes = (w.next + (size_t)nq * 4 + 255) & ~(size_t)255;
    return w;
}

struct InitArgs {
    int nq, nt;
    float window;
    const float* qdesc;              // [B][nq][64]
    const float* prev;               // [B][nq][2]
    const uint8_t* qflags;           // [B][nq] or NULL
    const char* grids; size_t grid_stride;
    const char* targets; size_t target_stride;
    const float* target_xy;          // [B][nt][2] or NULL (with prev_out)
    int th_low;
    float nn_ratio;
    char* ws; size_t ws_stride;
    uint8_t* status; int* claim_idx; int* matches12; int* best_dist; int* second_dist; int* n_window; int* n_tested;   // [B][nq]
    int* matches21; int* matched_distance;                                                                          // [B][nt]
    int* n_matches;                  // [B]
    float* prev_out;                 // [B][nq][2] or NULL; may be `prev`
};
