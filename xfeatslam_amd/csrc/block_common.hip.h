// block_common.hip.h -- what a 256-lane workgroup (four waves) does in every device-side geometry solver (triangulate / twoview / sim3solve /
// mlpnp .hip.h), written once on top of the wave primitives of search_common.hip.h: the ordered compaction step, the integer sum, the tree fold
// of geo_tree_fold with a barrier between its steps, and one wave counting a predicate.  No atomics: two runs give identical bytes.
#pragma once
#include "search_common.hip.h"
#include "geom_common.h"

// One step of an ordered compaction: of 256 consecutive items, one per lane, those with `pred` go to consecutive output positions in lane order (ballot +
// popcount inside a wave, the four wave totals in order, never an atomic counter).  Returns this lane's position (meaningful where pred holds) and advances
// `base`, every lane's running count, by the step's total.  s4 must be free on entry (a barrier of the caller's since its last read) and is read until the caller's next barrier.
__device__ __forceinline__ int block_compact_step(bool pred, int* s4, int& base) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(pred);
    if (lane == 0) s4[wave] = __popcll(bal);
    __syncthreads();
    int before = 0;
    for (int wv = 0; wv < wave; ++wv) before += s4[wv];
    const int pos = base + before + __popcll(bal & ((1ull << lane) - 1ull));
    base += ((s4[0] + s4[1]) + s4[2]) + s4[3];
    return pos;
}

// the sum of one int per lane over the workgroup, on every lane (its two barriers also publish the workgroup's earlier global writes)
__device__ __forceinline__ int block_sum_i32(int* s4, int mine) {
    const int v = wave_sum_i32(mine);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((s4[0] + s4[1]) + s4[2]) + s4[3];
}

// K sums at once in the order of geo_tree_fold: lane l's partial sums mine[k] go to s[k * 256 + l], then s[l] += s[l + h] for h = 128, 64, .. 1;
// every lane receives out[k] = s[k * 256].  s: K * GEO_LANES scalars of LDS.
template <class T, int K>
__device__ __forceinline__ void block_tree_fold(T* s, const T* mine, T* out) {
    const int tid = threadIdx.x;
    __syncthreads();                                                       // s is free
#pragma unroll
    for (int k = 0; k < K; ++k) s[k * GEO_LANES + tid] = mine[k];
    __syncthreads();
    for (int h = GEO_LANES / 2; h >= 1; h >>= 1) {
        if (tid < h) {
#pragma unroll
            for (int k = 0; k < K; ++k) s[k * GEO_LANES + tid] = s[k * GEO_LANES + tid] + s[k * GEO_LANES + tid + h];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = s[k * GEO_LANES];
}

// how many of the items 0 .. N - 1 satisfy in(k), counted by ONE wave (64 items per pass, ballot + popcount); every lane returns the count
template <class F>
__device__ __forceinline__ int wave_count(int N, F in) {
    const int lane = threadIdx.x & 63;
    int count = 0;
    for (int k0 = 0; k0 < N; k0 += 64) {
        const int k = k0 + lane;
        count += __popcll(__ballot(k < N && in(k)));
    }
    return count;
}
