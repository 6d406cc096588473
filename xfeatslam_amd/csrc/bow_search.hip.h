// bow_search.hip.h -- ORBmatcher::SearchByBoW, the frame form (src/ORBmatcher.cc:408-610) and the keyframe form (:950-1090), for B
// problems per call (xfh_bow_search_device; the contract is the sequential loop written out in include/xfeat_hip.h).
//
// The claim (vpMapPointMatches[realIdxF] resp. vbMatched2) makes the reference's loop sequential, but only inside a node: a keypoint is in
// exactly one node, so a claim made while node A is walked can be seen by later queries of node A only.  Nodes are independent, inside a
// node the queries are resolved in stored order, and claims only ever REMOVE targets.
//
//   k_bow_candidates  one wave per (problem, keypoint of side 1), four per workgroup, as k_triangulation_search: the flag byte and node id
//                   from wave-uniform addresses, the node looked up in side 2's id list (nodes_clamp.h), its members dealt to the lanes 64 at a
//                   time in stored order, the STATIC filter only (eligible2), DescriptorDistance with the query row through the scalar cache.
//                   Each lane keeps its XFH_BOW_K least keys dist << 32 | position: the reference updates on a strict '<', so among equal
//                   distances the member visited FIRST wins and ascending key is the order in which it would pick them.  The wave's K least
//                   go to the workspace with the node's slot, the static candidate count and the count of candidates below init_dist (only
//                   those can become best or second).  INACTIVE and NO_NODE are final here; every output gets its "none" value.
//   k_bow_resolve   one wave per (problem, node of side 1), four per workgroup.  The claimed set of side 2's node is a bitmap over the
//                   POSITIONS in that node, 2 KB of LDS per wave (XFH_GRID_MAX_N bits), touched by this wave only: no atomics, no other
//                   wave to wait for, and a claim in one node can never serialise another.  The queries of the node are taken in stored
//                   order, wave-uniformly: best = the first unclaimed list entry, second = the next, n_candidates = the static count minus
//                   the claims made so far, then the acceptance line of bow_math.h; an accepted query sets its bit.  A query whose list was
//                   truncated (more than K candidates below init_dist) and holds fewer than two unclaimed entries is searched again in
//                   full by the wave, 64 members at a time, with the claim test inside the walk.  Every iteration count is read from the
//                   blobs on the device; the host reads nothing back.
//
// The claim state lives in LDS, and the lists in memory this kernel never writes: nothing it reads through a possibly scalar path is
// written by it (see the note in triangulation_search.hip.h).  Plain stores only.
//
// Bounds: blobs are read through nodes_clamp.h only (counts and ranges clamped to [0, n], items checked against n).  k_bow_resolve trusts a
// workspace entry only after it has compared the query's recorded slot with the slot it resolves, so a side-1 blob whose items disagree with
// its node_of makes queries be left as the candidate pass wrote them, and a list position is checked against the node's length before
// it indexes the bitmap.  With such blobs two waves may write the outputs of one query or one assigned2 entry: any of the values, in bounds.
//
// Cost.  Candidate pass: every (query, member of its node) pair pays one distance, spread over n1 waves.  Resolve: a step without a
// re-search reads the query's workspace entries and a few LDS words -- a chain of dependent loads, about 1.3 us measured
// (profiles/bow_search.md) --, so a node of m1 queries costs m1 short sequential steps on one wave while the other nodes run beside it.  The lists are sized for the usual scene, where few queries find their nearest targets taken.  Worst case: ONE node holds
// every keypoint of both sides and every query's nearest targets are the same few rows.  Then the call is n1 sequential steps on one wave,
// and each step past the K-th walks all n2 members again (n2 / 64 distances per lane): n1 = n2 = XFH_GRID_MAX_N is 16384 steps of 256
// distance rounds -- about a second on one SIMD, exact and terminating, and nothing more.  The workspace counter says how many queries of a
// call took that path.
#pragma once
#include "ctx.h"
#include "bow_math.h"
#include "nodes_clamp.h"
#include "search_common.hip.h"

// The members of side 2's node `r`, dealt to the lanes 64 at a time in stored order, for k_bow_candidates and the re-search of k_bow_resolve: the
// eligibility test (a keypoint of side 2, eligible2), the claimed bitmap over the positions when there is one, DescriptorDistance, and visit(key) for
// every member below init_dist (one at or above it can never pass `d < best` nor `d < second`).  Returns how many THIS LANE found eligible and unclaimed.
template <typename Visit>
__device__ __forceinline__ int bow_walk(const char* nb2, int n2, const NodeRange r, const uint8_t* el, const char* tg, const float* qr, int init_dist,
                                        const unsigned* claimed, int lane, Visit visit) {
    int n = 0;
    for (int p0 = 0; p0 < r.len; p0 += 64) {
        const int p = p0 + lane;
        if (p >= r.len) continue;
        const int idx = nodes_item(nb2, n2, r.start + p);
        if (idx < 0 || (el && el[idx] == 0) || (claimed && ((claimed[p >> 5] >> (p & 31)) & 1u))) continue;
        ++n;
        const int dist = descriptor_distance(qr, (const f32x4*)(tg + (size_t)idx * 256));
        if (dist < 0 || dist >= init_dist) continue;
        visit(key_pack(dist, (unsigned)p));
    }
    return n;
}

__global__ __launch_bounds__(256)
void k_bow_candidates(BowArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int qi = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave), pb = blockIdx.y;
    const int n1 = a.s1.n, n2 = a.s2.n;
    if (qi >= n1) return;
    const size_t qg = (size_t)pb * n1 + qi;                            // the query's place in the [B][n1] outputs
    const char* __restrict__ nb1 = a.s1.nodes + (size_t)pb * a.s1.nodes_stride;
    const char* __restrict__ nb2 = a.s2.nodes + (size_t)pb * a.s2.nodes_stride;
    const float* __restrict__ qr = (const float*)(a.s1.desc + (size_t)pb * a.s1.desc_stride) + (size_t)qi * 64;
    const uint32_t node = nodes_node_of(nb1, n1, qi);
    const int active = __builtin_amdgcn_readfirstlane(a.s1.flag[(size_t)pb * a.s1.elem_stride + qi] != 0 ? 1 : 0);
    u64 lk[XFH_BOW_K];                                                 // the lane's K least keys, ascending
#pragma unroll
    for (int j = 0; j < XFH_BOW_K; ++j) lk[j] = XFH_KEY_NONE;
    int st = XFH_BOW_INACTIVE, slot = -1, ntot = 0, nlow = 0;
    if (active) {                                                      // (uniform)
        st = XFH_BOW_NO_NODE;
        slot = nodes_find(nb2, n2, nodes_count(nb2, n2), node);
        if (slot >= 0) {
            st = XFH_BOW_NO_CANDIDATES;                                // until k_bow_resolve has looked
            const NodeRange r = nodes_range(nb2, n2, slot);
            const uint8_t* __restrict__ el = a.s2.flag ? a.s2.flag + (size_t)pb * a.s2.elem_stride : nullptr;
            const char* __restrict__ tg = a.s2.desc + (size_t)pb * a.s2.desc_stride;
            ntot = bow_walk(nb2, n2, r, el, tg, qr, a.init_dist, nullptr, lane, [&](u64 key) { ++nlow; klist_insert(lk, key); });
            ntot = wave_sum_i32(ntot); nlow = wave_sum_i32(nlow);
        }
    }
    const BowWs L = bow_ws_layout(n1, 1);
    char* ws = a.ws + bow_ws_layout(n1, (int)gridDim.y).first + (size_t)pb * L.stride;
    // the wave's K least, ascending
    int* ld = (int*)(ws + L.ldist) + (size_t)qi * XFH_BOW_K;
    int* lp = (int*)(ws + L.lpos) + (size_t)qi * XFH_BOW_K;
    for (int j = 0; j < XFH_BOW_K; ++j) {
        const u64 m = klist_head(lk);
        if (m == XFH_KEY_NONE) break;                                  // (uniform)
        if (lane == 0) { ld[j] = key_dist(m); lp[j] = key_pos(m); }
        klist_drop(lk, m);
    }
    if (lane == 0) {
        ((int*)(ws + L.slot))[qi] = slot; ((int*)(ws + L.ntot))[qi] = ntot; ((int*)(ws + L.nlow))[qi] = nlow;
        a.status[qg] = (uint8_t)st; a.match12[qg] = -1; a.best_dist[qg] = a.init_dist; a.second_dist[qg] = a.init_dist; a.n_candidates[qg] = 0;
    }
}

__global__ __launch_bounds__(256)
void k_bow_resolve(BowArgs a) {
    __shared__ unsigned s_claim[4][XFH_GRID_MAX_N / 32];               // per wave: bit p = member p of side 2's node is claimed
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int w1 = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave), pb = blockIdx.y;
    const int n1 = a.s1.n, n2 = a.s2.n;
    if (w1 >= n1) return;
    const char* nb1 = a.s1.nodes + (size_t)pb * a.s1.nodes_stride;
    const char* nb2 = a.s2.nodes + (size_t)pb * a.s2.nodes_stride;
    if (w1 >= nodes_count(nb1, n1)) return;                            // (uniform: this wave has no node)
    const int slot2 = nodes_find(nb2, n2, nodes_count(nb2, n2), nodes_id(nb1, n1, w1));
    if (slot2 < 0) return;                                             // side 2 lacks the node: its queries are NO_NODE already
    const NodeRange r1 = nodes_range(nb1, n1, w1), r2 = nodes_range(nb2, n2, slot2);
    const BowWs L = bow_ws_layout(n1, 1);
    char* ws0 = a.ws;
    const char* ws = a.ws + bow_ws_layout(n1, (int)gridDim.y).first + (size_t)pb * L.stride;
    const int* wslot = (const int*)(ws + L.slot);
    const int* wtot = (const int*)(ws + L.ntot);
    const int* wlow = (const int*)(ws + L.nlow);
    const int* ld = (const int*)(ws + L.ldist);
    const int* lp = (const int*)(ws + L.lpos);
    const uint8_t* el = a.s2.flag ? a.s2.flag + (size_t)pb * a.s2.elem_stride : nullptr;
    const char* tg = a.s2.desc + (size_t)pb * a.s2.desc_stride;
    const char* q1 = a.s1.desc + (size_t)pb * a.s1.desc_stride;
    unsigned* claim = s_claim[wave];
    for (int w = lane; w < (r2.len + 31) / 32; w += 64) claim[w] = 0u;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    int nclaimed = 0, nmatch = 0, nsearch = 0, nsteps = 0;
    for (int t = 0; t < r1.len; ++t) {                                 // the queries of the node in stored order; everything is uniform
        const int i = nodes_item(nb1, n1, r1.start + t);
        if (i < 0 || wslot[i] != slot2) continue;                      // not a keypoint, inactive, or the blob's items contradict its node_of
        ++nsteps;
        const int ntot = wtot[i], nlow = wlow[i], len = nlow < XFH_BOW_K ? nlow : XFH_BOW_K;
        int found = 0, bp = -1, bd = a.init_dist, sd = a.init_dist;
        for (int j = 0; j < len && found < 2; ++j) {
            const int p = lp[(size_t)i * XFH_BOW_K + j];
            if ((unsigned)p >= (unsigned)r2.len || ((claim[p >> 5] >> (p & 31)) & 1u)) continue;
            const int d = ld[(size_t)i * XFH_BOW_K + j];
            if (++found == 1) { bp = p; bd = d; } else sd = d;
        }
        if (nlow > XFH_BOW_K && found < 2) {                           // the truncated list ran out: the full walk with the claim test inside
            ++nsearch;
            u64 b = XFH_KEY_NONE, s2 = XFH_KEY_NONE;
            bow_walk(nb2, n2, r2, el, tg, (const float*)q1 + (size_t)i * 64, a.init_dist, claim, lane, [&](u64 key) { top2_insert(b, s2, key); });
            wave_top2(b, s2);
            bp = -1; bd = a.init_dist; sd = a.init_dist;
            if (b != XFH_KEY_NONE) { bp = key_pos(b); bd = key_dist(b); }                       // (bp < r2.len: the position the key was made of)
            if (s2 != XFH_KEY_NONE) sd = key_dist(s2);
        }
        const int bi = bp >= 0 ? nodes_item(nb2, n2, r2.start + bp) : -1;
        const int ncand = ntot > nclaimed ? ntot - nclaimed : 0;       // every claim of the node took one statically eligible member away
        const bool accept = xfh_bow_accept_line(bi, bd, sd, a.th_low, a.nn_ratio, a.flags);
        if (lane == 0) {
            const size_t qg = (size_t)pb * n1 + i;
            a.status[qg] = (uint8_t)(accept ? XFH_BOW_MATCHED : (ncand == 0 ? XFH_BOW_NO_CANDIDATES : XFH_BOW_REJECTED));
            a.match12[qg] = accept ? bi : -1; a.best_dist[qg] = bd; a.second_dist[qg] = sd; a.n_candidates[qg] = ncand;
            if (accept) a.assigned2[(size_t)pb * n2 + bi] = i;
        }
        if (accept) {                                                  // (uniform) every lane stores the same word: each reads back its own store
            claim[bp >> 5] |= 1u << (bp & 31);
            ++nclaimed; ++nmatch;
        }
    }
    if (lane == 0) {
        if (nmatch) atomicAdd(&a.n_matches[pb], nmatch);
        int* cnt = (int*)ws0 + (size_t)pb * 4;
        if (nsearch) atomicAdd(&cnt[0], nsearch);
        if (nsteps) atomicAdd(&cnt[1], nsteps);
        atomicAdd(&cnt[2], 1);
    }
}

hipError_t launch_bow_search(xfh_ctx* c, const BowArgs& a, int B) {
    hipError_t e = hipMemsetAsync(a.n_matches, 0, (size_t)B * sizeof(int), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(a.assigned2, 0xFF, (size_t)B * a.s2.n * sizeof(int), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(a.ws, 0, bow_ws_layout(a.s1.n, B).first, c->stream);
    if (e != hipSuccess) return e;
    const dim3 grid((a.s1.n + 3) / 4, B);
    launch_k(c, XFH_K_BOW_CANDIDATES, -1, k_bow_candidates, grid, dim3(256), 0, a);
    launch_k(c, XFH_K_BOW_RESOLVE, -1, k_bow_resolve, grid, dim3(256), 0, a);
    return hipGetLastError();
}
