// init_search.hip.h -- ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:833-948) as ONE device-resident call
// (xfh_init_search_device; the contract is the sequential loop written out in include/xfeat_hip.h).
//
// The retraction rule makes the loop sequential, but not through a claim: a keypoint is never taken.  vMatchedDistance[k] is the distance
// of the last query that accepted k, it only ever decreases (an acceptor got past `vMatchedDistance[k] <= dist`, :872, so it is strictly
// closer than the one before), and a retracted query never searches again.  So when query q's turn comes, member (k, d) is skipped iff
//       d == INT_MAX  (the initial vMatchedDistance blocks it)  or  some accepting j < q with claim[j] == k has dist[j] <= d,
// where (claim[j], dist[j]) is what j wrote when ITS turn came -- whether j was retracted later does not matter.  That is a triangular
// system like the claim rule of projection_search.hip.h, settled by the same rounds (resolve_rounds.hip.h).  What differs is the per-keypoint state: not one
// integer but the SET of (acceptor, distance) pairs, kept here as a chain through the queries -- head[nt] + next[nq] -- and the skip test
// is an order-free "exists" over the chain of k, so the order in which the chain was linked does not matter.
//
//   k_init_candidates  many workgroups, one wave per query: flags, the window walk of window_search.hip.h with no filter.  Writes n_window,
//                      the copy of the window centre, and into the workspace the query's XFH_INIT_K nearest members ordered by (dist,
//                      visiting position) -- the order in which the reference's strict '<' would pick them -- and their total number.
//   k_init_resolve     one workgroup per problem, head[nt] and next[nq] in LDS (128 KB at 16384 x 16384: the > 64 KB attribute), no global
//                      atomics, no other workgroup to wait for.  A round: snapshot the distances and relink the chains from the claims
//                      (LDS exchanges), then one THREAD per query reads its K-list: best = first unblocked entry, second = the next.  Only
//                      (accepts?, keypoint, distance) of a query is state, so a list is settled as soon as that is known: two unblocked
//                      entries, or one whose distance is already above th_low, or a last entry above th_low, or one unblocked entry that passes the
//                      ratio test against the last entry (a lower bound of the true second best).  A truncated list that is not
//                      settled goes on a list, and the WAVES of the workgroup re-search those in full with the test inside the walk, under
//                      the budget and postponement rule of resolve_rounds.hip.h (see "Cost of the worst case" there).  The round
//                      count is decided here: the host reads nothing back.  At the end: matches21 (the LARGEST acceptor of a keypoint =
//                      the last writer), matched_distance (its distance), n_matches (keypoints with an acceptor: every acceptor but the
//                      last of a keypoint was retracted), and the final chains to the workspace.
//   k_init_final       many workgroups, one wave per query: the full walk against the FINAL chains, which is the query's turn in the
//                      sequential loop: n_tested, best / second, status, claim_idx; matches12 = claim_idx iff the query is the last
//                      acceptor of its keypoint; prev_out.  It reads the window centre from the workspace copy, so prev_out may be
//                      prev_matched.
// Truncation: most near members of a late query are held by earlier queries at a smaller distance, but with the three settling rules above a
// list rarely runs out before the query's state is known (profiles/init_search.md has the counts for three list lengths).
//
// Bounds: slot numbers come from the blob and are checked against nt in the walk (window_walk) before anything is indexed with them; list
// entries are such slot numbers; chain entries are query numbers < nq written by the resolver itself; coordinates are only ever used as
// floats; a non-finite centre opens no window.  A distance that is not below 2^31 / 512 as a float (Inf or NaN rows) is INT_MAX: such a
// member is always blocked, as in the reference (INT_MAX <= INT_MAX).
//
// Cost of the worst case: thousands of acceptors on one keypoint make every test of that keypoint a walk over a chain of thousands; thousands of
// queries on one spot: resolve_rounds.hip.h.
#pragma once
#include "ctx.h"
#include "init_math.h"
#include "search_common.hip.h"
#include "resolve_rounds.hip.h"
#include "window_search.hip.h"

#define XFH_INIT_RESOLVE_THREADS 1024
static_assert(XFH_INIT_K >= 2 && XFH_INIT_K <= 16, "the per-lane list lives in registers");

__global__ __launch_bounds__(256)
void k_init_candidates(InitArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int qi = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave), pb = blockIdx.y;
    if (qi >= a.nq) return;
    const size_t qg = (size_t)pb * a.nq + qi;
    const InitWs L = init_ws_layout(a.nq, a.nt);
    char* ws = a.ws + (size_t)pb * a.ws_stride;
    const bool active = !a.qflags || (a.qflags[qg] & 1);
    const float u = a.prev[qg * 2], v = a.prev[qg * 2 + 1], r = a.window;
    int* ntot = (int*)(ws + L.ntot);
    if (lane == 0) {
        float* ce = (float*)(ws + L.centre) + (size_t)qi * 4;
        ce[0] = u; ce[1] = v; ce[2] = r; ce[3] = 0.0f;
        ((int*)(ws + L.claim))[qi] = -1; ((int*)(ws + L.dist))[qi] = XFH_INIT_NONE;
    }
    if (!active) { if (lane == 0) { ntot[qi] = 0; a.n_window[qg] = 0; } return; }      // (uniform)
    const char* grid = a.grids + (size_t)pb * a.grid_stride;
    const float* tg = (const float*)(a.targets + (size_t)pb * a.target_stride);
    const WindowWalk w = window_open(grid, u, v, r, a.nt, lane);
    u64 lk[XFH_INIT_K];                                                // the lane's K smallest keys, ascending
#pragma unroll
    for (int j = 0; j < XFH_INIT_K; ++j) lk[j] = XFH_KEY_NONE;
    int mine = 0;                                                      // members that can ever be unblocked (dist < INT_MAX)
    const int nw = window_walk<true, true>(w, grid, a.qdesc + qg * 64, u, v, r, tg, a.nt, nullptr, nullptr, 0.0f, lane, [](int, float, float) { return true; },
                                           [&](u64 key, int) {
                                               if (key_dist(key) == XFH_INIT_NONE) return;
                                               ++mine;
                                               klist_insert(lk, key);
                                           });
    mine = wave_sum_i32(mine);
    // the wave's K smallest, ascending, with the slot at each one's position
    int* ld = (int*)(ws + L.ldist) + (size_t)qi * XFH_INIT_K;
    int* li = (int*)(ws + L.lidx) + (size_t)qi * XFH_INIT_K;
    for (int j = 0; j < XFH_INIT_K; ++j) {
        const u64 m = klist_head(lk);
        if (m == XFH_KEY_NONE) break;                                  // (uniform)
        const int slot = window_slot(w, grid, key_pos(m));             // (uniform: every lane names the same item)
        if (lane == 0) { ld[j] = key_dist(m); li[j] = slot; }
        klist_drop(lk, m);
    }
    if (lane == 0) { ntot[qi] = mine; a.n_window[qg] = nw; }
}

// some acceptor j < q of keypoint k at a distance <= d (the chain of k; dist: the distances the chain was linked with)
__device__ __forceinline__ bool init_blocked(const int* head, const int* next, const int* __restrict__ dist, int k, int d, int q) {
    for (int j = head[k]; j >= 0; j = next[j])
        if (j < q && dist[j] <= d) return true;
    return false;
}

// the query's new state against the one it had, and the round's "smallest query that moved"
__device__ __forceinline__ void init_finish(int* wclaim, int* wdist, int q, bool accept, int bi, int bd, int* changed_lo) {
    const int c = accept ? bi : -1, d = accept ? bd : XFH_INIT_NONE;
    if (wclaim[q] != c || wdist[q] != d) { wclaim[q] = c; wdist[q] = d; atomicMin(changed_lo, q); }
}

__global__ __launch_bounds__(XFH_INIT_RESOLVE_THREADS)
void k_init_resolve(InitArgs a) {
    extern __shared__ int chain[];                                     // head[nt], next[nq]
    __shared__ int s_changed_lo, s_defer_lo, s_nredo, s_nwalk, s_nout, s_nmatch;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, pb = blockIdx.x;
    const int nq = a.nq, nt = a.nt;
    int* head = chain;
    int* next = chain + nt;
    const InitWs L = init_ws_layout(nq, nt);
    char* ws = a.ws + (size_t)pb * a.ws_stride;
    const float* centre = (const float*)(ws + L.centre);
    const int* ld = (const int*)(ws + L.ldist);
    const int* li = (const int*)(ws + L.lidx);
    const int* ntot = (const int*)(ws + L.ntot);
    int* redo = (int*)(ws + L.redo);
    int* wclaim = (int*)(ws + L.claim);
    int* wdist = (int*)(ws + L.dist);
    int* snap = (int*)(ws + L.next);                                   // the round's copy of the distances (the final `next` is written after the loop)
    const size_t q0 = (size_t)pb * nq;
    const char* grid = a.grids + (size_t)pb * a.grid_stride;
    const float* tg = (const float*)(a.targets + (size_t)pb * a.target_stride);
    int lo = 0, rounds = 0;
    if (tid == 0) { s_nwalk = 0; s_nout = 0; }                         // (the first barrier of the loop publishes them)
    for (;;) {
        // the chains of the state so far (claim / dist are global memory written by this workgroup only; the barriers order it)
        for (int k = tid; k < nt; k += XFH_INIT_RESOLVE_THREADS) head[k] = -1;
        if (tid == 0) { s_changed_lo = XFH_RESOLVE_NONE; s_defer_lo = XFH_RESOLVE_NONE; s_nredo = 0; }
        __syncthreads();
        for (int q = tid; q < nq; q += XFH_INIT_RESOLVE_THREADS) {
            const int c = wclaim[q];
            snap[q] = wdist[q];
            if (c >= 0) next[q] = atomicExch(&head[c], q);
        }
        __syncthreads();
        // one thread per query: the K-list against the chains
        for (int q = lo + tid; q < nq; q += XFH_INIT_RESOLVE_THREADS) {
            const int n = ntot[q];
            if (n == 0) continue;                                      // inactive, an empty window, or no member under INT_MAX: never accepts
            const int len = n < XFH_INIT_K ? n : XFH_INIT_K;
            int found = 0, bi = -1, bd = XFH_INIT_NONE, sd = XFH_INIT_NONE, last = 0;
            bool settled = false;
            for (int j = 0; j < len && !settled; ++j) {
                const int idx = li[(size_t)q * XFH_INIT_K + j], d = ld[(size_t)q * XFH_INIT_K + j];
                last = d;
                if (init_blocked(head, next, snap, idx, d, q)) continue;
                ++found;
                if (found == 1) { bi = idx; bd = d; settled = d > a.th_low; }     // ascending: nothing at or under th_low is left
                else { sd = d; settled = true; }
            }
            if (!settled && found == 0 && last > a.th_low) settled = true;                  // whatever is unblocked past the list is above th_low
            // the true second is >= the list's last entry and the test only gets easier with a larger second (nn_ratio >= 0)
            if (!settled && found == 1 && xfh_init_accept_line(bd, last, a.th_low, a.nn_ratio)) { sd = last; settled = true; }
            if (n > XFH_INIT_K && !settled) redo[atomicAdd(&s_nredo, 1)] = q;
            else init_finish(wclaim, wdist, q, xfh_init_accept_line(bd, sd, a.th_low, a.nn_ratio), bi, bd, &s_changed_lo);
        }
        __syncthreads();
        // one wave per unsettled query: the full walk with the test inside
        const int nredo = s_nredo;
        const int cut = XFH_RESOLVE_CUT(lo, nq, nredo);
        if (tid == 0) s_nout += nredo;
        for (int i = wave; i < nredo; i += XFH_INIT_RESOLVE_THREADS / 64) {
            const int q = __builtin_amdgcn_readfirstlane(redo[i]);
            if (q >= cut) { if (lane == 0) atomicMin(&s_defer_lo, q); continue; }     // (uniform) postponed
            if (lane == 0) atomicAdd(&s_nwalk, 1);
            const float u = centre[(size_t)q * 4], v = centre[(size_t)q * 4 + 1], r = centre[(size_t)q * 4 + 2];
            const WindowWalk w = window_open(grid, u, v, r, nt, lane);
            u64 b = XFH_KEY_NONE, s2 = XFH_KEY_NONE;
            window_walk<true, true>(w, grid, a.qdesc + (q0 + q) * 64, u, v, r, tg, nt, nullptr, nullptr, 0.0f, lane, [](int, float, float) { return true; },
                                    [&](u64 key, int idx) {
                                        const int d = key_dist(key);
                                        if (d != XFH_INIT_NONE && !init_blocked(head, next, snap, idx, d, q)) top2_insert(b, s2, key);
                                    });
            int bi, bd, si, sd;
            window_best2(w, grid, b, s2, XFH_INIT_NONE, bi, bd, si, sd);
            if (lane == 0) init_finish(wclaim, wdist, q, xfh_init_accept_line(bd, sd, a.th_low, a.nn_ratio), bi, bd, &s_changed_lo);
        }
        __syncthreads();
        const int c = s_changed_lo, d = s_defer_lo;
        ++rounds;
        __syncthreads();                                               // everyone has read the round's result before it is reset
        if (c == XFH_RESOLVE_NONE && d == XFH_RESOLVE_NONE) break;
        lo = XFH_RESOLVE_NEXT_LO(c, d);
    }
    // the last round changed nothing: the chains in LDS are those of the final state.  For k_init_final: head, next; and per keypoint the
    // last acceptor (the largest), its distance, and the number of keypoints that have one
    int* whead = (int*)(ws + L.head);
    int* wnext = (int*)(ws + L.next);
    if (tid == 0) { s_nmatch = 0; ((int*)ws)[0] = rounds; ((int*)ws)[1] = s_nwalk; ((int*)ws)[2] = s_nout; ((int*)ws)[3] = XFH_INIT_K; }
    __syncthreads();                                                   // (also: nobody reads snap any more)
    for (int q = tid; q < nq; q += XFH_INIT_RESOLVE_THREADS) wnext[q] = wclaim[q] >= 0 ? next[q] : -1;
    int mine = 0;
    for (int k = tid; k < nt; k += XFH_INIT_RESOLVE_THREADS) {
        int m = -1;
        for (int j = head[k]; j >= 0; j = next[j]) m = j > m ? j : m;
        whead[k] = head[k];
        a.matches21[(size_t)pb * nt + k] = m;
        a.matched_distance[(size_t)pb * nt + k] = m >= 0 ? wdist[m] : XFH_INIT_NONE;
        mine += m >= 0;
    }
    if (mine) atomicAdd(&s_nmatch, mine);
    __syncthreads();
    if (tid == 0) a.n_matches[pb] = s_nmatch;
}

__global__ __launch_bounds__(256)
void k_init_final(InitArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int qi = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave), pb = blockIdx.y;
    if (qi >= a.nq) return;
    const size_t qg = (size_t)pb * a.nq + qi;
    const InitWs L = init_ws_layout(a.nq, a.nt);
    const char* ws = a.ws + (size_t)pb * a.ws_stride;
    const float* ce = (const float*)(ws + L.centre) + (size_t)qi * 4;
    const float u = ce[0], v = ce[1], r = ce[2];
    const bool active = !a.qflags || (a.qflags[qg] & 1);
    const int nw = a.n_window[qg];
    int st = active ? XFH_INIT_NO_CANDIDATES : XFH_INIT_INACTIVE, bi = -1, bd = XFH_INIT_NONE, sd = XFH_INIT_NONE, ntst = 0, m12 = -1;
    if (active && nw > 0) {                                            // (uniform)
        const int* head = (const int*)(ws + L.head);
        const int* next = (const int*)(ws + L.next);
        const int* dist = (const int*)(ws + L.dist);
        const char* grid = a.grids + (size_t)pb * a.grid_stride;
        const float* tg = (const float*)(a.targets + (size_t)pb * a.target_stride);
        const WindowWalk w = window_open(grid, u, v, r, a.nt, lane);
        u64 b = XFH_KEY_NONE, s2 = XFH_KEY_NONE;
        window_walk<true, true>(w, grid, a.qdesc + qg * 64, u, v, r, tg, a.nt, nullptr, nullptr, 0.0f, lane, [](int, float, float) { return true; },
                                [&](u64 key, int idx) {
                                    const int d = key_dist(key);
                                    if (d != XFH_INIT_NONE && !init_blocked(head, next, dist, idx, d, qi)) { ++ntst; top2_insert(b, s2, key); }
                                });
        ntst = wave_sum_i32(ntst);
        int si;
        window_best2(w, grid, b, s2, XFH_INIT_NONE, bi, bd, si, sd);
        const bool accept = xfh_init_accept_line(bd, sd, a.th_low, a.nn_ratio);
        st = accept ? XFH_INIT_MATCHED : XFH_INIT_REJECTED;
        if (!accept) bi = -1;
        else if (a.matches21[(size_t)pb * a.nt + bi] == qi) m12 = bi;
    }
    if (lane == 0) {
        a.status[qg] = (uint8_t)st; a.claim_idx[qg] = bi; a.matches12[qg] = m12; a.best_dist[qg] = bd; a.second_dist[qg] = sd; a.n_tested[qg] = ntst;
        if (a.prev_out) {
            float x = u, y = v;
            if (m12 >= 0) { const float* t = a.target_xy + ((size_t)pb * a.nt + m12) * 2; x = t[0]; y = t[1]; }
            a.prev_out[qg * 2] = x; a.prev_out[qg * 2 + 1] = y;
        }
    }
}

hipError_t launch_init_search(xfh_ctx* c, const InitArgs& a, int B) {
    XFH_SET_LDS_ATTR_ONCE(c, k_init_resolve, 2 * XFH_GRID_MAX_N * sizeof(int));
    const dim3 per_query((a.nq + 3) / 4, B);
    launch_k(c, XFH_K_INIT_CANDIDATES, -1, k_init_candidates, per_query, dim3(256), 0, a);
    launch_k(c, XFH_K_INIT_RESOLVE, -1, k_init_resolve, dim3(B), dim3(XFH_INIT_RESOLVE_THREADS), ((size_t)a.nt + a.nq) * sizeof(int), a);
    launch_k(c, XFH_K_INIT_FINAL, -1, k_init_final, per_query, dim3(256), 0, a);
    return hipGetLastError();
}
