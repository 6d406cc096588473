// projection_search.hip.h -- ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono) (src/ORBmatcher.cc:1861-2047) and the
// SearchLocalPoints form (:42-141) as ONE device-resident call: projection, cull, windowed best / second best, and the reference's
// claim order (xfh_search_projection_device; the contract is the sequential loop written out in include/xfeat_hip.h).
//
// The claim rule makes the loop sequential: CurrentFrame.mvpMapPoints is all NULL before the call (Tracking.cc:2914), so every entry
// the candidate test (:1932-1934) sees was written by an earlier iteration (:1957): query q depends on queries < q only.  With
// claim_min[k] = min{ j : match[j] == k and j claims } (a statically skipped k: -1), query q skips k iff claim_min[k] < q; the rounds that
// settle this, why they end at the sequential answer and what the worst case costs: resolve_rounds.hip.h.
//
//   k_proj_candidates  many workgroups, one wave per query: flags, projection (projection_math.h) or the caller's (u, v, r), cull,
//                      then the window walk of window_search.hip.h with the STATIC filters only.  Writes status and proj, and
//                      into the workspace the query's XFH_PROJ_K best candidates ordered by (dist, visiting position) -- the
//                      order in which the reference's strict '<' would pick them -- and the number of static candidates.
//   k_proj_resolve     one workgroup per problem, claim_min of the nt keypoints in LDS (64 KB at 16384; LDS atomics, no global
//                      atomics, no other workgroup to wait for).  A round: rebuild claim_min from the matches, then one THREAD per
//                      query reads its K-list: best = first unclaimed entry, second = the next.  A query whose list was truncated
//                      and holds fewer than two unclaimed entries goes on a list, and the WAVES of the workgroup then re-search
//                      those in full with the claim test inside the walk.  The round count is data dependent and decided here: the
//                      host reads nothing back.  At the end: match_idx, distances, status, assigned (largest matched q per
//                      keypoint = last writer) and n_matches, and the final claim_min to the workspace.
//   k_proj_count       many workgroups, one wave per query: n_candidates = survivors of the walk with the FINAL claim_min (no
//                      descriptor is read).
// k_proj_resolve and k_proj_count also serve xfh_map_projection_search_device behind its own front kernel (mapproj_search.hip.h), which
// fills the same workspace; ProjArgs::status_base and ::flags_or are what differs.  Both are 0 here, and the kernels are templates on
// whether they read the two fields at all: the <false> instances this file launches are the code they were before the fields existed.
//
// Bounds: slot numbers come from the blob and are checked against nt in the walk (window_walk) before anything is indexed with them;
// list entries are such slot numbers; point coordinates and poses are only ever used as floats; a non-finite (u, v, r) opens no
// window.  Nothing is read through a float.
#pragma once
#include "ctx.h"
#include "projection_math.h"
#include "projection_layout.h"
#include "search_common.hip.h"
#include "resolve_rounds.hip.h"
#include "window_search.hip.h"

#define XFH_PROJ_RESOLVE_THREADS 1024

// the wave's K smallest (dist, slot), ascending, into the query's list in the workspace: the owner of each writes it
__device__ __forceinline__ void proj_store_list(char* ws, const ProjWs& L, int qi, u64 (&lk)[XFH_PROJ_K], int (&ls)[XFH_PROJ_K]) {
    int* ld = (int*)(ws + L.ldist) + (size_t)qi * XFH_PROJ_K;
    int* li = (int*)(ws + L.lidx) + (size_t)qi * XFH_PROJ_K;
    for (int j = 0; j < XFH_PROJ_K; ++j) {
        int slot;
        const u64 m = klist_head(lk);
        if (m == XFH_KEY_NONE) break;                                  // (uniform)
        if (klist_drop(lk, m, ls, &slot)) { ld[j] = key_dist(m); li[j] = slot; }
    }
}

__global__ __launch_bounds__(256)
void k_proj_candidates(ProjArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int qi = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave), pb = blockIdx.y;
    if (qi >= a.nq) return;
    const size_t qg = (size_t)pb * a.nq + qi;                          // the query's place in the [B][nq] arrays
    const ProjWs L = proj_ws_layout(a.nq, a.nt);
    char* ws = a.ws + (size_t)pb * a.ws_stride;
    int st = XFH_PROJ_INACTIVE;
    float u = 0.0f, v = 0.0f, ur = 0.0f, r = a.radius;
    if (a.qflags[qg] & 1) {
        const float* p = a.pts + qg * 3;
        if (a.mode == XFH_PROJ_POINTS) st = xfh_project_point(a.Tcw + (size_t)pb * 12, a.cam, a.bounds, p[0], p[1], p[2], &u, &v, &ur);
        else { u = p[0]; v = p[1]; r = p[2]; ur = a.ur_query ? a.ur_query[qg] : 0.0f; st = XFH_PROJ_VISIBLE; }
    }
    if (lane == 0) {
        a.status[qg] = (uint8_t)st;                                    // XFH_PROJ_VISIBLE is XFH_PROJ_NO_CANDIDATES until k_proj_resolve has found one
        a.match_idx[qg] = -1; a.best_dist[qg] = a.init_dist; a.second_dist[qg] = a.init_dist; a.n_candidates[qg] = 0;
        if (a.proj_out) { a.proj_out[qg * 3] = u; a.proj_out[qg * 3 + 1] = v; a.proj_out[qg * 3 + 2] = ur; }
        float* pj = (float*)(ws + L.proj) + (size_t)qi * 4;
        pj[0] = u; pj[1] = v; pj[2] = ur; pj[3] = r;
    }
    int* ntot = (int*)(ws + L.ntot);
    if (st != XFH_PROJ_VISIBLE) { if (lane == 0) ntot[qi] = 0; return; }          // (uniform)
    const char* grid = a.grids + (size_t)pb * a.grid_stride;
    const float* tg = (const float*)(a.targets + (size_t)pb * a.target_stride);
    const WindowWalk w = window_open(grid, u, v, r, a.nt, lane);
    u64 lk[XFH_PROJ_K];                                                // the lane's K smallest keys, ascending, and their slots
    int ls[XFH_PROJ_K];
#pragma unroll
    for (int j = 0; j < XFH_PROJ_K; ++j) { lk[j] = XFH_KEY_NONE; ls[j] = -1; }
    const int nc = window_walk<true>(w, grid, a.qdesc + qg * 64, u, v, r, tg, a.nt, a.skip ? a.skip + (size_t)pb * a.nt : nullptr,
                                     a.uright ? a.uright + (size_t)pb * a.nt : nullptr, ur, lane, [](int, float, float) { return true; },
                                     [&](u64 key, int idx) { klist_insert(lk, key, ls, idx); });
    proj_store_list(ws, L, qi, lk, ls);
    if (lane == 0) ntot[qi] = nc;
}

// accept / reject of one query from its best two (include/xfeat_hip.h), the outputs, and the round's "smallest query that moved"
__device__ __forceinline__ void proj_finish(const ProjArgs& a, int sbase, size_t qg, int q, int bi, int bd, int si, int sd, bool survivors, int* changed_lo) {
    const bool accept = bi >= 0 && bd <= a.th_high && !(a.nn_ratio > 0.0f && si >= 0 && (float)bd > a.nn_ratio * (float)sd);
    const int m = accept ? bi : -1;
    if (a.match_idx[qg] != m) { a.match_idx[qg] = m; atomicMin(changed_lo, q); }
    a.best_dist[qg] = bd; a.second_dist[qg] = sd;
    a.status[qg] = (uint8_t)((accept ? XFH_PROJ_MATCHED : (survivors ? XFH_PROJ_REJECTED : XFH_PROJ_NO_CANDIDATES)) + sbase);
}

template <bool MAPPROJ>
__global__ __launch_bounds__(XFH_PROJ_RESOLVE_THREADS)
void k_proj_resolve(ProjArgs a) {
    const int sbase = MAPPROJ ? a.status_base : 0, flags_or = MAPPROJ ? a.flags_or : 0;
    extern __shared__ int claim[];                                     // nt entries: claim_min, at the end the assignment
    __shared__ int s_changed_lo, s_defer_lo, s_nredo, s_nwalk, s_nmatch;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, pb = blockIdx.x;
    const int nq = a.nq, nt = a.nt;
    const ProjWs L = proj_ws_layout(nq, nt);
    char* ws = a.ws + (size_t)pb * a.ws_stride;
    const float* proj = (const float*)(ws + L.proj);
    const int* ld = (const int*)(ws + L.ldist);
    const int* li = (const int*)(ws + L.lidx);
    const int* ntot = (const int*)(ws + L.ntot);
    int* redo = (int*)(ws + L.redo);
    const size_t q0 = (size_t)pb * nq;
    const uint8_t* skip = a.skip ? a.skip + (size_t)pb * nt : nullptr;
    const uint8_t* qflags = a.qflags + q0;
    const char* grid = a.grids + (size_t)pb * a.grid_stride;
    const float* tg = (const float*)(a.targets + (size_t)pb * a.target_stride);
    const float* uright = a.uright ? a.uright + (size_t)pb * nt : nullptr;
    int lo = 0, rounds = 0;
    if (tid == 0) s_nwalk = 0;                                         // (the first barrier of the loop publishes it)
    for (;;) {
        // claim_min of the matches so far (match_idx is global memory written by this workgroup only; the barriers order it)
        for (int k = tid; k < nt; k += XFH_PROJ_RESOLVE_THREADS) claim[k] = (skip && skip[k]) ? -1 : 0x7fffffff;
        if (tid == 0) { s_changed_lo = XFH_RESOLVE_NONE; s_defer_lo = XFH_RESOLVE_NONE; s_nredo = 0; }
        __syncthreads();
        for (int q = tid; q < nq; q += XFH_PROJ_RESOLVE_THREADS) {
            const int m = a.match_idx[q0 + q];
            if (m >= 0 && ((qflags[q] | flags_or) & 2)) atomicMin(&claim[m], q);
        }
        __syncthreads();
        // one thread per query: the K-list against claim_min
        for (int q = lo + tid; q < nq; q += XFH_PROJ_RESOLVE_THREADS) {
            if (a.status[q0 + q] < XFH_PROJ_NO_CANDIDATES + sbase) continue;
            const int n = ntot[q], len = n < XFH_PROJ_K ? n : XFH_PROJ_K;
            int found = 0, bi = -1, bd = a.init_dist, si = -1, sd = a.init_dist;
            bool settled = false;                                      // nothing past the list can change best / second
            for (int j = 0; j < len && !settled; ++j) {
                const int idx = li[(size_t)q * XFH_PROJ_K + j];
                if (claim[idx] < q) continue;
                const int d = ld[(size_t)q * XFH_PROJ_K + j];
                ++found;
                if (d >= a.init_dist) settled = true;                  // ascending: every later survivor is >= init_dist too
                else if (found == 1) { bi = idx; bd = d; }
                else { si = idx; sd = d; settled = true; }
            }
            if (n > XFH_PROJ_K && !settled) redo[atomicAdd(&s_nredo, 1)] = q;
            else proj_finish(a, sbase, q0 + q, q, bi, bd, si, sd, found > 0, &s_changed_lo);
        }
        __syncthreads();
        // one wave per truncated query: the full walk with the claim test inside
        const int nredo = s_nredo;
        const int cut = XFH_RESOLVE_CUT(lo, nq, nredo);
        for (int i = wave; i < nredo; i += XFH_PROJ_RESOLVE_THREADS / 64) {
            const int q = __builtin_amdgcn_readfirstlane(redo[i]);
            if (q >= cut) { if (lane == 0) atomicMin(&s_defer_lo, q); continue; }     // (uniform) postponed (resolve_rounds.hip.h)
            if (lane == 0) atomicAdd(&s_nwalk, 1);
            const float u = proj[(size_t)q * 4], v = proj[(size_t)q * 4 + 1], ur = proj[(size_t)q * 4 + 2], r = proj[(size_t)q * 4 + 3];
            const WindowWalk w = window_open(grid, u, v, r, nt, lane);
            u64 b = XFH_KEY_NONE, s2 = XFH_KEY_NONE;
            const int nc = window_walk<true>(w, grid, a.qdesc + (q0 + q) * 64, u, v, r, tg, nt, skip, uright, ur, lane,
                                             [&](int idx, float, float) { return claim[idx] >= q; },
                                             [&](u64 key, int) { top2_insert(b, s2, key); });
            int bi, bd, si, sd;
            window_best2(w, grid, b, s2, a.init_dist, bi, bd, si, sd);
            if (lane == 0) proj_finish(a, sbase, q0 + q, q, bi, bd, si, sd, nc > 0, &s_changed_lo);
        }
        __syncthreads();
        const int c = s_changed_lo, d = s_defer_lo;
        ++rounds;
        __syncthreads();                                               // everyone has read the round's result before it is reset
        if (c == XFH_RESOLVE_NONE && d == XFH_RESOLVE_NONE) break;
        lo = XFH_RESOLVE_NEXT_LO(c, d);
    }
    // claim_min is the one of the final matches: for k_proj_count
    int* wclaim = (int*)(ws + L.claim);
    for (int k = tid; k < nt; k += XFH_PROJ_RESOLVE_THREADS) wclaim[k] = claim[k];
    if (tid == 0) { s_nmatch = 0; ((int*)ws)[0] = rounds; ((int*)ws)[1] = s_nwalk; ((int*)ws)[2] = 0; ((int*)ws)[3] = 0; }
    __syncthreads();
    // assigned[k] = the LAST query that wrote mvpMapPoints[k] (:1957) = the largest matched q; n_matches counts every accepting query
    for (int k = tid; k < nt; k += XFH_PROJ_RESOLVE_THREADS) claim[k] = -1;
    __syncthreads();
    int mine = 0;
    for (int q = tid; q < nq; q += XFH_PROJ_RESOLVE_THREADS) {
        const int m = a.match_idx[q0 + q];
        if (m >= 0) { atomicMax(&claim[m], q); ++mine; }
    }
    if (mine) atomicAdd(&s_nmatch, mine);
    __syncthreads();
    for (int k = tid; k < nt; k += XFH_PROJ_RESOLVE_THREADS) a.assigned[(size_t)pb * nt + k] = claim[k];
    if (tid == 0) a.n_matches[pb] = s_nmatch;
}

template <bool MAPPROJ>
__global__ __launch_bounds__(256)
void k_proj_count(ProjArgs a) {
    const int sbase = MAPPROJ ? a.status_base : 0;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int qi = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave), pb = blockIdx.y;
    if (qi >= a.nq) return;
    const size_t qg = (size_t)pb * a.nq + qi;
    const ProjWs L = proj_ws_layout(a.nq, a.nt);
    const char* ws = a.ws + (size_t)pb * a.ws_stride;
    if (a.status[qg] < XFH_PROJ_NO_CANDIDATES + sbase || ((const int*)(ws + L.ntot))[qi] == 0) return;       // n_candidates is 0 already
    const float* pj = (const float*)(ws + L.proj) + (size_t)qi * 4;
    const int* wclaim = (const int*)(ws + L.claim);
    const char* grid = a.grids + (size_t)pb * a.grid_stride;
    const WindowWalk w = window_open(grid, pj[0], pj[1], pj[3], a.nt, lane);
    const int nc = window_walk<false>(w, grid, nullptr, pj[0], pj[1], pj[3], nullptr, a.nt, a.skip ? a.skip + (size_t)pb * a.nt : nullptr,
                                      a.uright ? a.uright + (size_t)pb * a.nt : nullptr, pj[2], lane,
                                      [&](int idx, float, float) { return wclaim[idx] >= qi; }, [](u64, int) {});
    if (lane == 0) a.n_candidates[qg] = nc;
}

hipError_t launch_search_projection(xfh_ctx* c, const ProjArgs& a, int B) {
    XFH_SET_LDS_ATTR_ONCE(c, k_proj_resolve<false>, XFH_GRID_MAX_N * sizeof(int));
    const dim3 per_query((a.nq + 3) / 4, B);
    launch_k(c, XFH_K_PROJ_CANDIDATES, -1, k_proj_candidates, per_query, dim3(256), 0, a);
    launch_k(c, XFH_K_PROJ_RESOLVE, -1, k_proj_resolve<false>, dim3(B), dim3(XFH_PROJ_RESOLVE_THREADS), (size_t)a.nt * sizeof(int), a);
    launch_k(c, XFH_K_PROJ_COUNT, -1, k_proj_count<false>, per_query, dim3(256), 0, a);
    return hipGetLastError();
}
