// capi_internal.h -- what the entry-point files (capi.cpp, capi_search.cpp, capi_fuse.cpp, capi_triangulation.cpp, capi_bow.cpp, capi_vocab.cpp, capi_bowdb.cpp, capi_loop.cpp, capi_init.cpp, capi_poseopt.cpp, capi_triangulate.cpp, capi_twoview.cpp, capi_sim3solve.cpp, capi_mlpnp.cpp, capi_bench.cpp) share.
#pragma once
#include "ctx.h"
#include "window_layout.h"
#include <math.h>
#include <vector>
#define HIPCK(c, x) do { hipError_t _e = (x); if (_e != hipSuccess) { (c)->hip_err = std::string(#x) + ": " + hipGetErrorString(_e); return XFH_ERR_HIP; } } while (0)

// true when any of the pointers (or strides) has a bit of `mask` set: misaligned(15, a, b) = a or b is not 16-byte aligned; null passes
template <typename... P>
inline bool misaligned(uintptr_t mask, P... p) { return ((... | (uintptr_t)p) & mask) != 0; }
// the argument checks of the many-pairs calls -> the launcher's pair list (capi_search.cpp)
int gather_pairs(xfh_ctx* c, int n_pairs, const void* const* image1, const int* n1, const void* const* image2, const int* n2,
                 int* const* idx1, int* const* idx2, float* const* dist, int* n_matches, bool need_out, std::vector<XfhMatchPair>& v);
// bytes of the staging arena xfh_match_mnn needs for n1 x n2 rows: xfh_create reserves that for nfeatures x nfeatures (capi_search.cpp)
size_t match_mnn_stage_bytes(int n1, int n2);
// the caller's scale tables checked and copied into the kernels' argument form (capi_fuse.cpp)
struct FuseLevels;
bool fuse_levels(const float* scale_factors, const float* ratio_max, int nlevels, FuseLevels* L);
// the caller's grid bounds -> the kernels' geometry; false for bounds that are not finite or not ordered.
// mfGridElementWidthInv = FRAME_GRID_COLS / (mnMaxX - mnMinX), mfGridElementHeightInv likewise, in fp32 (Frame.cc:336-341)
inline bool grid_geom(const xfh_grid_bounds* b, GridGeom* g) {
    if (!b || !isfinite(b->min_x) || !isfinite(b->min_y) || !isfinite(b->max_x) || !isfinite(b->max_y)) return false;
    if (!(b->max_x > b->min_x) || !(b->max_y > b->min_y)) return false;
    g->min_x = b->min_x; g->min_y = b->min_y; g->max_x = b->max_x; g->max_y = b->max_y;
    g->inv_w = (float)XFH_GRID_COLS / (b->max_x - b->min_x);
    g->inv_h = (float)XFH_GRID_ROWS / (b->max_y - b->min_y);
    return isfinite(g->inv_w) && isfinite(g->inv_h) && g->inv_w > 0.0f && g->inv_h > 0.0f;
}
