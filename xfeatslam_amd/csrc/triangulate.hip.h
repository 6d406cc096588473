// triangulate.hip.h -- the triangulation half of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:481-710) for B neighbours of one keyframe
// (included by kernels_match.hip).  The contract is in include/xfeat_hip.h; the arithmetic is triangulate_math.h, the host's own lines.
//
//   k_triangulate_pairs   one lane per (problem b, keypoint i of KF1): the match of the search, the whole per-pair rule, status / kind / xyz.  Lanes
//                         do not talk to each other: no LDS, no atomics.  The fp64 null vector keeps U and V (32 doubles) in registers: the pair
//                         loop of the Jacobi sweep is unrolled with compile-time indices, so nothing goes to scratch.
//   k_triangulate_winner  XFH_TRIANG_CLAIM only, one lane per keypoint i: the least b whose pair (b, i) is ACCEPTED, or -1.  A minimum over b found by
//                         walking b upwards: no atomics, nothing depends on timing.
//   k_triangulate_finish  one workgroup per problem b: the header counts in a fixed fold, the pairs a lower neighbour owns rewritten to SUPERSEDED,
//                         and the compact list in creation order.  Problem b's first entry sits behind the winners of all b' < b, which the
//                         workgroup counts itself from winner[]; inside b the entries are placed by an ordered scan over i (ballot + popcount
//                         inside a wave, the four wave totals in order), never by an atomic counter.  Workgroup 0 also writes n_new and the
//                         -1 / 0 tail.  Two runs give identical bytes.
#pragma once
#include "triangulate_math.h"
#include "block_common.hip.h"

#define XFH_TRIANG_THREADS 256

__global__ __launch_bounds__(XFH_TRIANG_THREADS)
void k_triangulate_pairs(TriangArgs a) {
    const int i = blockIdx.x * XFH_TRIANG_THREADS + threadIdx.x, b = blockIdx.y, n1 = a.s1.n;
    if (i >= n1) return;
    const size_t kg = (size_t)b * n1 + i;
    const int m = a.match12[kg];
    TriangPair r;
    r.status = TRIANG_NO_MATCH; r.kind = 0; r.x3D[0] = r.x3D[1] = r.x3D[2] = 0.0f;
    if (m >= 0 && m < a.s2.n) {                                            // anything else is "no match": nothing is indexed with it
        const TriangObs o1 = triang_obs(a.s1, b, i), o2 = triang_obs(a.s2, b, m);
        triang_pair(a.p, o1, o2, &r);
    }
    a.status[kg] = (unsigned char)r.status; a.kind[kg] = (unsigned char)r.kind;
    a.xyz[3 * kg] = r.x3D[0]; a.xyz[3 * kg + 1] = r.x3D[1]; a.xyz[3 * kg + 2] = r.x3D[2];
}

__global__ __launch_bounds__(XFH_TRIANG_THREADS)
void k_triangulate_winner(TriangArgs a) {
    const int i = blockIdx.x * XFH_TRIANG_THREADS + threadIdx.x, n1 = a.s1.n;
    if (i >= n1) return;
    int w = -1;
    for (int b = 0; b < a.B; ++b)
        if (a.status[(size_t)b * n1 + i] == TRIANG_ACCEPTED) { w = b; break; }
    a.winner[i] = w;
}

__global__ __launch_bounds__(XFH_TRIANG_THREADS)
void k_triangulate_finish(TriangArgs a) {
    __shared__ int s_cnt[XFH_TRIANG_THREADS / 64][9];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x, n1 = a.s1.n;
    int cnt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};                              // the seven header counts, winners of b' < b, winners of all b
    for (int i = tid; i < n1; i += XFH_TRIANG_THREADS) {
        const size_t kg = (size_t)b * n1 + i;
        const int st = a.status[kg], kd = a.kind[kg];
        const int w = a.claim ? a.winner[i] : (st == TRIANG_ACCEPTED ? b : -1);
        const bool matched = st != TRIANG_NO_MATCH, mine = w == b, earlier = w >= 0 && w < b;
        cnt[TRIANG_H_MATCHED] += matched;
        cnt[TRIANG_H_TRI_ATTEMPTS] += matched && st != TRIANG_LOW_PARALLAX && kd == 0;
        cnt[TRIANG_H_STEREO_ATTEMPTS] += kd != 0;
        cnt[TRIANG_H_ACCEPTED] += st == TRIANG_ACCEPTED;
        cnt[TRIANG_H_NEW] += mine;
        cnt[TRIANG_H_NEW_STEREO] += mine && kd != 0;
        cnt[TRIANG_H_SUPERSEDED] += matched && earlier;
        cnt[7] += earlier; cnt[8] += w >= 0;
        if (matched && earlier) a.status[kg] = TRIANG_SUPERSEDED;          // (own element only; k_triangulate_winner has finished)
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) { const int s = wave_sum_i32(cnt[k]); if (lane == 0) s_cnt[wave][k] = s; }
    __syncthreads();
    int tot[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) tot[k] = ((s_cnt[0][k] + s_cnt[1][k]) + s_cnt[2][k]) + s_cnt[3][k];
    if (tid < 8) a.header[(size_t)b * 8 + tid] = tid < 7 ? tot[tid] : 0;
    if (!a.claim) return;
    __syncthreads();                                                       // s_cnt is free again
    int base = tot[7];
    const float* Ow1 = a.s1.Ow + (a.s1.per_b ? (size_t)b * 3 : 0);
    const float* Ow2 = a.s2.Ow + (size_t)b * 3;
    for (int i0 = 0; i0 < n1; i0 += XFH_TRIANG_THREADS) {
        const int i = i0 + tid;
        const bool mine = i < n1 && a.winner[i] == b;
        const int pos = block_compact_step(mine, s_cnt[0], base);         // < n1: one entry per keypoint of KF1 at most; the four ints lie in row 0
        if (mine) {
            const size_t kg = (size_t)b * n1 + i;
            const float X[3] = {a.xyz[3 * kg], a.xyz[3 * kg + 1], a.xyz[3 * kg + 2]};
            float nrm[3], dst[3];
            triang_normal_depth(X, Ow1, Ow2, a.p.scale_last, nrm, dst);
            a.new_idx1[pos] = i; a.new_b[pos] = b; a.new_idx2[pos] = a.match12[kg];
#pragma unroll
            for (int k = 0; k < 3; ++k) { a.new_xyz[3 * pos + k] = X[k]; a.new_normal[3 * pos + k] = nrm[k]; a.new_dist[3 * pos + k] = dst[k]; }
        }
        __syncthreads();                                                   // s_cnt is free for the next step
    }
    if (b == 0) {
        const int n_new = tot[8];
        if (tid == 0) a.n_new[0] = n_new;
        for (int pos = n_new + tid; pos < n1; pos += XFH_TRIANG_THREADS) {
            a.new_idx1[pos] = -1; a.new_b[pos] = -1; a.new_idx2[pos] = -1;
#pragma unroll
            for (int k = 0; k < 3; ++k) { a.new_xyz[3 * pos + k] = 0.0f; a.new_normal[3 * pos + k] = 0.0f; a.new_dist[3 * pos + k] = 0.0f; }
        }
    }
}

hipError_t launch_triangulate(xfh_ctx* c, const TriangArgs& a) {
    const int n1 = a.s1.n, gx = (n1 + XFH_TRIANG_THREADS - 1) / XFH_TRIANG_THREADS;
    launch_k(c, XFH_K_TRIANGULATE_PAIRS, -1, k_triangulate_pairs, dim3(gx, a.B), dim3(XFH_TRIANG_THREADS), 0, a);
    if (a.claim) launch_k(c, XFH_K_TRIANGULATE_WINNER, -1, k_triangulate_winner, dim3(gx), dim3(XFH_TRIANG_THREADS), 0, a);
    launch_k(c, XFH_K_TRIANGULATE_FINISH, -1, k_triangulate_finish, dim3(a.B), dim3(XFH_TRIANG_THREADS), 0, a);
    return hipGetLastError();
}
