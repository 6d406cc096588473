// fuse_search.hip.h -- ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th) (src/ORBmatcher.cc:1333-1523) and the Sim3 form
// Fuse(KeyFrame*, Sim3f&, ...) (:1525-1640) up to the sequential bookkeeping, for B keyframes per launch (xfh_fuse_search_device; the
// contract is written out in include/xfeat_hip.h).
//
//   k_fuse_search   one wave per (problem, query), four per workgroup.  The wave evaluates the per-point arithmetic of fuse_math.h on
//                   wave-uniform values, and a culled query goes through a uniform branch round everything that touches the grid.
//                   The query's descriptor row comes through the scalar cache once, before the walk, as in k_search_window (four
//                   16-dword scalar loads; the walk's loop holds the 16 vector loads of the target row and none of the query), and
//                   so do the point, normal, distances, pose and camera centre; the flag byte is one vector load (gfx950 has no
//                   scalar byte load, and a dword around it could leave the caller's buffer).  The compiler may only do that for
//                   memory the kernel has not written: FuseArgs' pointers carry no noalias guarantee, so ALL stores of the kernel
//                   sit at its end, behind the last load -- keep them there.
//                   A query that reaches the search opens the window of window_search.hip.h with its own radius
//                   th * scale_factors[level] and walks it once: the chi-square gate sits in the walk's `extra` hook, where the item's
//                   coordinates are in registers already, and every lane counts the window members it was dealt (n_window) before
//                   the gate.  A query at level >= 2 walks without descriptors: every XFeat keypoint has octave 0, so the level window
//                   kpLevel < nPredictedLevel - 1 (:1454) rejects each member, and only n_window is wanted.
//
// Fuse has no claim order and no second best: there is nothing between the queries, so nothing is resolved afterwards and the call
// needs no workspace.  With query_stride = 0 the B problems read the same points and descriptor rows (LocalMapping::SearchInNeighbors:
// one keyframe's map points against every neighbour); the rows are then served from L2, which is the intent.
//
// Bounds: slot numbers come from the blob and are checked against nt in window_walk before uright or a target row is indexed with
// them; a non-finite (u, v, r) opens no window; level is a count of at most nlevels - 1 <= 15 comparisons.  Nothing is read through a float.
#pragma once
#include "ctx.h"
#include "fuse_math.h"
#include "search_common.hip.h"
#include "window_search.hip.h"

__global__ __launch_bounds__(256)
void k_fuse_search(FuseArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int qi = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave), pb = blockIdx.y;
    if (qi >= a.nq) return;
    const size_t qs = (size_t)pb * a.query_stride + qi;                // where the query's inputs are
    const size_t qg = (size_t)pb * a.nq + qi;                          // its place in the [B][nq] outputs
    // every input of the query is read here, before the kernel's first store, from addresses that are uniform in the wave
    const float* __restrict__ qr = a.qdesc + qs * 64;
    int st = XFH_FUSE_INACTIVE, level = -1;
    float u = 0.0f, v = 0.0f, ur = 0.0f, r = 0.0f;
    if (a.qflags[qs] & XFH_FUSE_FLAG_ACTIVE)
        st = xfh_fuse_point(a.Tcw + (size_t)pb * 12, a.Ow + (size_t)pb * 3, a.cam, a.bounds, a.th, a.lv, a.pts + qs * 3, a.normals + qs * 3, a.dist + qs * 3,
                            &u, &v, &ur, &r, &level);
    st = __builtin_amdgcn_readfirstlane(st); level = __builtin_amdgcn_readfirstlane(level);      // (computed from uniform values: say so to the compiler)
    int nwin = 0, ntest = 0, bi = -1, bd = a.init_dist;
    if (st == XFH_FUSE_VISIBLE) {                                      // (uniform) a culled query never touches the grid
        const char* __restrict__ grid = a.grids + (size_t)pb * a.grid_stride;
        const float* __restrict__ tg = (const float*)(a.targets + (size_t)pb * a.target_stride);
        const float* __restrict__ uright = a.uright ? a.uright + (size_t)pb * a.nt : nullptr;
        const bool chi2 = (a.flags & XFH_FUSE_CHI2) != 0;
        const WindowWalk w = window_open(grid, u, v, r, a.nt, lane);
        if (level <= 1) {                                              // (uniform) kpLevel = 0 lies in [level - 1, level] (:1454)
            u64 b = XFH_KEY_NONE, s2 = XFH_KEY_NONE;
            ntest = window_walk<true>(w, grid, qr, u, v, r, tg, a.nt, nullptr, nullptr, 0.0f, lane,
                                      [&](int idx, float xk, float yk) {
                                          ++nwin;
                                          return !(chi2 && xfh_fuse_chi2_skips(u, v, ur, xk, yk, uright ? uright[idx] : -1.0f));
                                      },
                                      [&](u64 key, int) { top2_insert(b, s2, key); });
            int si, sd;
            window_best2(w, grid, b, s2, a.init_dist, bi, bd, si, sd);
        } else nwin = window_count(w, grid, u, v, r, a.nt, lane);
        nwin = wave_sum_i32(nwin);
        const bool fused = bi >= 0 && bd <= a.th_low;
        st = nwin == 0 ? XFH_FUSE_NO_CANDIDATES : (fused ? XFH_FUSE_FUSED : XFH_FUSE_REJECTED);
    }
    // the only stores of the kernel, behind every load: nothing the wave reads can have been written by it
    if (lane == 0) {
        a.status[qg] = (uint8_t)st; a.best_idx[qg] = bi; a.best_dist[qg] = bd; a.n_window[qg] = nwin; a.n_tested[qg] = ntest; a.level[qg] = level;
        if (a.proj_out) { a.proj_out[qg * 3] = u; a.proj_out[qg * 3 + 1] = v; a.proj_out[qg * 3 + 2] = ur; }
        if (st == XFH_FUSE_FUSED) atomicAdd(&a.n_fused[pb], 1);
    }
}

hipError_t launch_fuse_search(xfh_ctx* c, const FuseArgs& a, int B) {
    hipError_t e = hipMemsetAsync(a.n_fused, 0, (size_t)B * sizeof(int), c->stream);
    if (e != hipSuccess) return e;
    launch_k(c, XFH_K_FUSE_SEARCH, -1, k_fuse_search, dim3((a.nq + 3) / 4, B), dim3(256), 0, a);
    return hipGetLastError();
}
