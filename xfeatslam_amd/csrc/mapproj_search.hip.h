// mapproj_search.hip.h -- the Sim3 forms of ORBmatcher::SearchByProjection (src/ORBmatcher.cc:612-717, :719-831; LoopClosing) and the
// relocalisation form (:2074-2195; Tracking::Relocalization) as ONE device-resident call for B problems (xfh_map_projection_search_device;
// the contract is the sequential loop written out in include/xfeat_hip.h).
//
// The loop is xfh_search_projection_device's in GIVEN mode with skip = taken, every query claiming and no ratio test, plus the level
// rule, so there is no second claim resolver here:
//   k_mapproj_candidates  one wave per (problem, query), four per workgroup: the per-point arithmetic of mapproj_math.h on wave-uniform
//                      values (the query's row and inputs come through uniform loads as in k_fuse_search, and ALL stores sit at the
//                      kernel's end for the reason given there), then the window walk with the STATIC filter (taken) only.  It counts
//                      n_window before any filter, so the taken test sits in the walk's `extra` hook, not in its skip argument.  A query
//                      at level >= 2 walks without descriptors and leaves an EMPTY candidate list (every XFeat keypoint has octave 0),
//                      which is all k_proj_resolve needs to search nothing for it.  Writes status, level, n_window, proj and the
//                      workspace of projection_layout.h: (u, v, 0, r), the K-list, the number of static candidates.
//   k_proj_resolve<true> / k_proj_count<true>   projection_search.hip.h, the instances that read ProjArgs::status_base = 2 and ::flags_or = 2.  The acceptance
//                      (float)best <= accept_max reaches them as th_high = (int)floorf(accept_max) clamped to the int range: best is an
//                      integer below 2^24, so (float)best is exact and best <= floorf(accept_max) says the same.
//
// Bounds: as projection_search.hip.h.
#pragma once
#include "ctx.h"
#include "mapproj_math.h"
#include "search_common.hip.h"
#include "window_search.hip.h"
#include "projection_search.hip.h"                         // k_proj_resolve, k_proj_count

__global__ __launch_bounds__(256)
void k_mapproj_candidates(MapProjArgs m) {
    const ProjArgs& a = m.p;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int qi = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave), pb = blockIdx.y;
    if (qi >= a.nq) return;
    const size_t qg = (size_t)pb * a.nq + qi;                          // the query's place in the [B][nq] arrays
    const ProjWs L = proj_ws_layout(a.nq, a.nt);
    char* ws = a.ws + (size_t)pb * a.ws_stride;
    // every input of the query is read here, before the kernel's first store, from addresses that are uniform in the wave
    const float* __restrict__ qr = a.qdesc + qg * 64;
    int st = XFH_MAPPROJ_INACTIVE, level = -1;
    float u = 0.0f, v = 0.0f, r = 0.0f;
    if (a.qflags[qg] & XFH_MAPPROJ_FLAG_ACTIVE)
        st = xfh_mapproj_point(a.Tcw + (size_t)pb * 12, m.Ow + (size_t)pb * 3, a.cam, a.bounds, m.th, m.lv, m.form, a.pts + qg * 3, m.normals + qg * 3,
                               m.dist + qg * 3, &u, &v, &r, &level);
    st = __builtin_amdgcn_readfirstlane(st); level = __builtin_amdgcn_readfirstlane(level);      // (computed from uniform values: say so to the compiler)
    u64 lk[XFH_PROJ_K];                                                // the lane's K smallest keys, ascending, and their slots
    int ls[XFH_PROJ_K];
#pragma unroll
    for (int j = 0; j < XFH_PROJ_K; ++j) { lk[j] = XFH_KEY_NONE; ls[j] = -1; }
    int nwin = 0, nc = 0;
    if (st == XFH_MAPPROJ_VISIBLE) {                                   // (uniform) a culled query never touches the grid
        const char* __restrict__ grid = a.grids + (size_t)pb * a.grid_stride;
        const float* __restrict__ tg = (const float*)(a.targets + (size_t)pb * a.target_stride);
        const uint8_t* __restrict__ taken = a.skip ? a.skip + (size_t)pb * a.nt : nullptr;
        const WindowWalk w = window_open(grid, u, v, r, a.nt, lane);
        if (level <= 1) {                                              // (uniform) kpLevel = 0 lies in [level - 1, level]
            nc = window_walk<true>(w, grid, qr, u, v, r, tg, a.nt, nullptr, nullptr, 0.0f, lane,
                                   [&](int idx, float, float) { ++nwin; return !(taken && taken[idx] != 0); },
                                   [&](u64 key, int idx) { klist_insert(lk, key, ls, idx); });
        } else nwin = window_count(w, grid, u, v, r, a.nt, lane);
        nwin = wave_sum_i32(nwin);
    }
    // the stores of the kernel, behind every load
    proj_store_list(ws, L, qi, lk, ls);
    if (lane == 0) {
        a.status[qg] = (uint8_t)st;                                    // XFH_MAPPROJ_VISIBLE is XFH_MAPPROJ_NO_CANDIDATES until k_proj_resolve has found one
        a.match_idx[qg] = -1; a.best_dist[qg] = a.init_dist; a.second_dist[qg] = a.init_dist; a.n_candidates[qg] = 0;
        m.n_window[qg] = nwin; m.level[qg] = level;
        if (a.proj_out) { a.proj_out[qg * 3] = u; a.proj_out[qg * 3 + 1] = v; a.proj_out[qg * 3 + 2] = r; }
        float* pj = (float*)(ws + L.proj) + (size_t)qi * 4;
        pj[0] = u; pj[1] = v; pj[2] = 0.0f; pj[3] = r;
        ((int*)(ws + L.ntot))[qi] = nc;
    }
}

hipError_t launch_map_projection_search(xfh_ctx* c, const MapProjArgs& m, int B) {
    XFH_SET_LDS_ATTR_ONCE(c, k_proj_resolve<true>, XFH_GRID_MAX_N * sizeof(int));
    const ProjArgs& a = m.p;
    const dim3 per_query((a.nq + 3) / 4, B);
    launch_k(c, XFH_K_MAPPROJ_CANDIDATES, -1, k_mapproj_candidates, per_query, dim3(256), 0, m);
    launch_k(c, XFH_K_PROJ_RESOLVE, -1, k_proj_resolve<true>, dim3(B), dim3(XFH_PROJ_RESOLVE_THREADS), (size_t)a.nt * sizeof(int), a);
    launch_k(c, XFH_K_PROJ_COUNT, -1, k_proj_count<true>, per_query, dim3(256), 0, a);
    return hipGetLastError();
}
