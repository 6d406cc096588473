// sim3_search.hip.h -- ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, S12, th) (src/ORBmatcher.cc:1642-1859) up to vpMatches12, for B
// keyframe pairs per call (xfh_sim3_search_device; the contract is written out in include/xfeat_hip.h).
//
//   k_sim3_search   one wave per (problem, direction, query), four per workgroup; the first nb1 workgroups of a problem run direction
//                   1->2 (side 1's map points into keyframe 2, :1681-1758), the others 2->1 (:1761-1838).  It is k_fuse_search with the
//                   arithmetic of sim3_math.h: the query's inputs and its map point's descriptor row come through uniform loads before
//                   the walk, a culled query goes through a uniform branch round everything that touches the grid, a query at level
//                   >= 2 walks without descriptors (every XFeat keypoint has octave 0, :1740), and ALL stores sit at the kernel's
//                   end, behind the last load (fuse_search.hip.h says why).  No claim, no second best, no workspace.
//   k_sim3_agree    the agreement step (:1840-1856): match12[i1] = idx2 iff match1[i1] == idx2 >= 0 && match2[idx2] == i1; n_found.
//
// With Sim3Side::stride = 0 for side 1 the B problems read the same current keyframe (LoopClosing: one keyframe against several
// candidates); its rows and grid are then served from L2.
//
// Bounds: as k_fuse_search -- slot numbers come from the blob and are checked against the target side's n in window_walk; a non-finite
// (u, v, r) opens no window; k_sim3_agree checks match1 against n2 before it indexes match2 with it.
#pragma once
#include <limits.h>
#include "ctx.h"
#include "sim3_math.h"
#include "search_common.hip.h"
#include "window_search.hip.h"

__global__ __launch_bounds__(256)
void k_sim3_search(Sim3Args a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int dir = (int)blockIdx.x >= a.nb1 ? 1 : 0, pb = blockIdx.y;                  // (uniform) 0: queries of side 1 search keyframe 2
    const Sim3Side& Q = a.s[dir];
    const Sim3Side& G = a.s[dir ^ 1];
    const int qi = __builtin_amdgcn_readfirstlane(((int)blockIdx.x - (dir ? a.nb1 : 0)) * 4 + wave);
    if (qi >= Q.n) return;
    const size_t qp = (size_t)pb * Q.stride, gp = (size_t)pb * G.stride;                // the problem whose inputs are read
    const size_t qs = qp * Q.n + qi;                                   // where the query's inputs are
    const size_t qg = (size_t)pb * Q.n + qi;                           // its place in the [B][n] outputs
    // every input of the query is read here, before the kernel's first store, from addresses that are uniform in the wave
    const float* __restrict__ qr = Q.mpdesc + qs * 64;
    int st = XFH_SIM3_INACTIVE, level = -1;
    float u = 0.0f, v = 0.0f, r = 0.0f;
    if (Q.flags[qs] & XFH_SIM3_FLAG_ACTIVE)
        st = xfh_sim3_point(Q.Tw + qp * 12, (dir ? a.M12 : a.M21) + (size_t)pb * 12, a.cam, a.bounds, a.th, a.lv, Q.X + qs * 3, Q.dist + qs * 3, &u, &v, &r, &level);
    st = __builtin_amdgcn_readfirstlane(st); level = __builtin_amdgcn_readfirstlane(level);      // (computed from uniform values: say so to the compiler)
    int nwin = 0, ntest = 0, bi = -1, bd = INT_MAX;
    if (st == XFH_SIM3_VISIBLE) {                                      // (uniform) a culled query never touches the grid
        const char* __restrict__ grid = G.grids + gp * G.grid_stride;
        const float* __restrict__ tg = (const float*)(G.desc + gp * G.desc_stride);
        const WindowWalk w = window_open(grid, u, v, r, G.n, lane);
        if (level <= 1) {                                              // (uniform) kp.octave = 0 lies in [level - 1, level] (:1740)
            u64 b = XFH_KEY_NONE, s2 = XFH_KEY_NONE;
            ntest = window_walk<true>(w, grid, qr, u, v, r, tg, G.n, nullptr, nullptr, 0.0f, lane,
                                      [&](int, float, float) { ++nwin; return true; },
                                      [&](u64 key, int) { top2_insert(b, s2, key); });
            int si, sd;
            window_best2(w, grid, b, s2, INT_MAX, bi, bd, si, sd);
        } else nwin = window_count(w, grid, u, v, r, G.n, lane);
        nwin = wave_sum_i32(nwin);
        const bool found = bi >= 0 && bd <= a.th_high;
        st = nwin == 0 ? XFH_SIM3_NO_CANDIDATES : (found ? XFH_SIM3_FOUND : XFH_SIM3_REJECTED);
    }
    // the only stores of the kernel, behind every load: nothing the wave reads can have been written by it
    if (lane == 0) {
        Q.status[qg] = (uint8_t)st; Q.match[qg] = st == XFH_SIM3_FOUND ? bi : -1; Q.best_dist[qg] = bd; Q.n_window[qg] = nwin; Q.n_tested[qg] = ntest;
        Q.level[qg] = level;
        if (Q.proj_out) { Q.proj_out[qg * 3] = u; Q.proj_out[qg * 3 + 1] = v; Q.proj_out[qg * 3 + 2] = r; }
    }
}

__global__ __launch_bounds__(256)
void k_sim3_agree(const int* __restrict__ match1, const int* __restrict__ match2, int n1, int n2, int* __restrict__ match12, int* __restrict__ n_found) {
    const int i1 = blockIdx.x * 256 + threadIdx.x, pb = blockIdx.y;
    bool ok = false;
    if (i1 < n1) {
        const int idx2 = match1[(size_t)pb * n1 + i1];
        ok = idx2 >= 0 && idx2 < n2 && match2[(size_t)pb * n2 + idx2] == i1;
        match12[(size_t)pb * n1 + i1] = ok ? idx2 : -1;
    }
    const int cnt = __popcll(__ballot(ok));
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&n_found[pb], cnt);
}

hipError_t launch_sim3_search(xfh_ctx* c, const Sim3Args& a, int B) {
    hipError_t e = hipMemsetAsync(a.n_found, 0, (size_t)B * sizeof(int), c->stream);
    if (e != hipSuccess) return e;
    const int n1 = a.s[0].n, n2 = a.s[1].n;
    launch_k(c, XFH_K_SIM3_SEARCH, -1, k_sim3_search, dim3(a.nb1 + (n2 + 3) / 4, B), dim3(256), 0, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    launch_k(c, XFH_K_SIM3_AGREE, -1, k_sim3_agree, dim3((n1 + 255) / 256, B), dim3(256), 0, (const int*)a.s[0].match, (const int*)a.s[1].match, n1, n2,
             a.match12, a.n_found);
    return hipGetLastError();
}
