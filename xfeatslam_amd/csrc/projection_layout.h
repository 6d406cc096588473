// projection_layout.h -- the workspace layout and the kernel arguments of xfh_search_projection_device (plain C++: the kernels in
// projection_search.hip.h and the entry points in capi_search.cpp share it).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "projection_math.h"

// entries of a query's candidate list: its best candidates under the static filters, ordered by (dist, visiting position)
#define XFH_PROJ_K 4

// workspace of one problem: header (rounds, full re-searches, 0, 0), proj[nq] (u, v, ur, r), the K-lists, counts, the re-search list, claim_min[nt]
struct ProjWs { size_t proj, ldist, lidx, ntot, redo, claim, bytes; };
XFH_HD ProjWs proj_ws_layout(int nq, int nt) {
    ProjWs w;
    w.proj = 16;
    w.ldist = w.proj + (size_t)nq * 16;
    w.lidx = w.ldist + (size_t)nq * XFH_PROJ_K * 4;
    w.ntot = w.lidx + (size_t)nq * XFH_PROJ_K * 4;
    w.redo = w.ntot + (size_t)nq * 4;
    w.claim = w.redo + (size_t)nq * 4;
    w.bytes = (w.claim + (size_t)nt * 4 + 255) & ~(size_t)255;
    return w;
}

struct ProjArgs {
    int mode, nq, nt;
    float radius;
    const float* pts;                // [B][nq][3]: world points (POINTS) or (u, v, r) (GIVEN)
    const float* ur_query;           // [B][nq] or NULL (GIVEN)
    const float* Tcw;                // [B][12] (POINTS)
    xfh_camera cam; xfh_grid_bounds bounds;
    const float* qdesc;              // [B][nq][64]
    const uint8_t* qflags;           // [B][nq]
    const char* grids; size_t grid_stride;
    const char* targets; size_t target_stride;
    const uint8_t* skip;             // [B][nt] or NULL
    const float* uright;             // [B][nt] or NULL
    int init_dist, th_high;
    float nn_ratio;
    char* ws; size_t ws_stride;
    uint8_t* status; int* match_idx; int* best_dist; int* second_dist; int* n_candidates;
    float* proj_out;                 // [B][nq][3] or NULL
    int* assigned;                   // [B][nt]
    int* n_matches;                  // [B]
    // what xfh_map_projection_search_device sets (mapproj_search.hip.h); zero in xfh_search_projection_device, whose kernel instances do not read them
    int status_base;                 // added to XFH_PROJ_NO_CANDIDATES / REJECTED / MATCHED: 2 = the numbering of XFH_MAPPROJ_* (and of XFH_FUSE_*)
    int flags_or;                    // or-ed into every query's flag byte: 2 = every query claims
};

