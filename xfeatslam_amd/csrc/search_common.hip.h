// search_common.hip.h -- what a wave does in every device-side ORBmatcher search (k_best2_csr and the *_search.hip.h kernels), written once: the
// keys, DescriptorDistance, a lane's two / K smallest keys with their wave-wide merges, the wave minimum and sums (integer, and fp64 for the two optimisers), one lane's double for all.  The lane-local pieces are plain
// C++ (XFH_HD): tests/cpp/search_common_test.cpp runs these very lines on the host against the obvious form.
#pragma once
#include <math.h>
#include "hd.h"

#define XFH_KEY_NONE (~0ull)                                            // larger than every key: an empty entry

// dist << 32 | position: ascending key = ascending distance and, inside a distance, visiting order -- the order of the reference's strict '<'
XFH_HD u64 key_pack(int dist, unsigned pos) { return ((u64)(unsigned)dist << 32) | (u64)pos; }
XFH_HD int key_dist(u64 key) { return (int)(key >> 32); }
XFH_HD int key_pos(u64 key) { return (int)(key & 0xFFFFFFFFull); }

// ORBmatcher::DescriptorDistance, the numerics contract of every integer distance the searches report: ONE fp64 fma chain over the 64 fp32
// differences in element order (-ffp-contract=off), rounded to fp32, times 512, truncated.  qr: the wave-uniform query row, tr: this lane's row.
// SAT: a squared norm that is Inf, NaN or >= 2^31 / 512 is INT_MAX (init_search.hip.h)
template <bool SAT = false>
XFH_HD int descriptor_distance(const float* qr, const f32x4* tr) {
    double acc = 0.0;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        const f32x4 tv = tr[g];
#pragma unroll
        for (int e = 0; e < 4; ++e) { const double df = (double)(qr[g * 4 + e] - tv[e]); acc = fma(df, df, acc); }
    }
    const float nd = (float)acc;
    if (SAT && !(nd < 4194304.0f)) return 0x7fffffff;
    return (int)(nd * 512.0f);
}

// one key into a lane's two smallest: if (key < b) { s2 = b; b = key; } else if (key < s2) s2 = key; -- written as minima so that the pair
// stays in registers when it is captured by reference
XFH_HD void top2_insert(u64& b, u64& s2, u64 key) {
    const u64 hi = key < b ? b : key;
    b = key < b ? key : b; s2 = hi < s2 ? hi : s2;
}
// the two smallest of (b, s) and (ob, os), each pair ascending
XFH_HD void top2_merge(u64& b, u64& s, u64 ob, u64 os) {
    const u64 lo = b < ob ? b : ob, hi = b < ob ? ob : b;
    const u64 ms = s < os ? s : os;
    b = lo; s = hi < ms ? hi : ms;
}
// one key into a lane's K smallest, ascending: a bubble through the sorted list -- every entry keeps the smaller and passes on the larger.
// ls (or nullptr): a value per entry that moves with its key
template <int K>
XFH_HD void klist_insert(u64 (&lk)[K], u64 key, int* ls = nullptr, int slot = -1) {
    u64 x = key;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const bool in = x < lk[j];
        const u64 lo = in ? x : lk[j], hi = in ? lk[j] : x;
        lk[j] = lo; x = hi;
        if (ls) { const int sl = in ? slot : ls[j], sh = in ? ls[j] : slot; ls[j] = sl; slot = sh; }
    }
}

#if defined(__HIPCC__)
__device__ __forceinline__ u64 wave_min_u64(u64 x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const u64 o = __shfl_xor(x, m); x = o < x ? o : x; }
    return x;
}
__device__ __forceinline__ int wave_sum_i32(int x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
    return x;
}
// a + b is commutative, so after the xor butterfly every lane holds the same bits
__device__ __forceinline__ double wave_sum_f64(double x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
    return x;
}
// every lane gets lane l's double; l is the same on all lanes
__device__ __forceinline__ double wave_readlane_f64(double x, int l) {
    const int sl = __builtin_amdgcn_readfirstlane(l);
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), sl), __builtin_amdgcn_readlane(__double2loint(x), sl));
}
// every lane gets the two smallest keys of the wave's 64 pairs
__device__ __forceinline__ void wave_top2(u64& b, u64& s2) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const u64 ob = __shfl_xor(b, m), os = __shfl_xor(s2, m);
        top2_merge(b, s2, ob, os);
    }
}
// Popping the wave's next smallest key in two steps, so that a caller can use the key between them (k_init_candidates looks the item up first):
// klist_head is the smallest head of all lanes (uniform; keys are distinct), XFH_KEY_NONE when all lists are empty; klist_drop shifts its owner's
// list and returns true on that lane, with *slot the value the key had beside it
template <int K>
__device__ __forceinline__ u64 klist_head(const u64 (&lk)[K]) { return wave_min_u64(lk[0]); }
template <int K>
__device__ __forceinline__ bool klist_drop(u64 (&lk)[K], u64 m, int* ls = nullptr, int* slot = nullptr) {
    const bool own = lk[0] == m;
    if (own) {
        if (ls) *slot = ls[0];
#pragma unroll
        for (int t = 0; t + 1 < K; ++t) { lk[t] = lk[t + 1]; if (ls) ls[t] = ls[t + 1]; }
        lk[K - 1] = XFH_KEY_NONE;
    }
    return own;
}
#endif
