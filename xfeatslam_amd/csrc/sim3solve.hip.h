// sim3solve.hip.h -- Sim3Solver (src/Sim3Solver.cc) under the iterate(20) loop of LoopClosing::DetectCommonRegionsFromBoW for B candidates per call,
// and the merge of the per-covisible BoW match lists in front of it (included by kernels_match.hip).  The contract is in include/xfeat_hip.h; the
// arithmetic is sim3solve_math.h, the host's own lines.  The solver is four launches, whatever the data:
//
//   k_sim3solve_prepare  one workgroup per problem: the compact correspondence list in i1 order (ordered scan: ballot + popcount inside a wave, the
//                        four wave totals in order, never an atomic counter) with X1, X2 and their projections, N, and the iteration count read
//                        from the caller's table and clamped (0 = TOO_FEW: the later kernels leave at once).
//   k_sim3solve_fit      one lane per (problem, iteration): the minimal set from the raw draws, Horn's closed form with the fp64 4 x 4 Jacobi in
//                        registers (the pair loops are unrolled, so every index is a constant).  All B x its hypotheses share one grid.
//   k_sim3solve_count    one wave per (problem, iteration): CheckInliers over the N correspondences, ballot + popcount.  Only the count is written:
//                        no iterations x N mask reaches HBM.
//   k_sim3solve_decide   one workgroup per problem: the first iteration above min_inliers and the last of the largest counts (integer min / max
//                        in LDS), the header, the reported hypothesis, the winner's flags recomputed per slot, the composition.
// The merge is three launches: the owner table set to INT_MAX, an integer atomicMin of j * n1 + k per entry, then one lane per slot.  The minimum
// and the owner count (an integer atomicAdd per workgroup) do not depend on the order of arrival: two runs give identical bytes.
#pragma once
#include "sim3solve_math.h"
#include "block_common.hip.h"

#define XFH_S3_THREADS 256
#define XFH_S3_FIT_LANES 64

struct S3Ws { int *cm, *sel, *cnt; float *X1, *X2, *P1, *P2, *hyp; };
__device__ __forceinline__ S3Ws s3_ws(const S3Args& a, int b) {
    const S3Layout L = s3_layout(a.n1);
    unsigned char* p = a.ws + (size_t)b * L.per_problem;
    S3Ws w;
    w.cm = (int*)(p + L.cm); w.sel = (int*)(p + L.sel); w.cnt = (int*)(p + L.cnt); w.X1 = (float*)(p + L.X1); w.X2 = (float*)(p + L.X2);
    w.P1 = (float*)(p + L.P1); w.P2 = (float*)(p + L.P2); w.hyp = (float*)(p + L.hyp);
    return w;
}

__global__ __launch_bounds__(XFH_S3_THREADS)
void k_sim3solve_prepare(S3Args a) {
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x, b = blockIdx.x, n1 = a.n1;
    const S3Ws w = s3_ws(a, b);
    int base = 0;
    for (int i0 = 0; i0 < n1; i0 += XFH_S3_THREADS) {
        const int i = i0 + tid;
        float X1[3], X2[3], p1[2], p2[2];
        const bool ok = i < n1 && s3_corr(a, b, i, X1, X2, p1, p2);
        __syncthreads();                                                   // s_cnt is free
        const size_t pos = (size_t)block_compact_step(ok, s_cnt, base);    // pos < n1
        if (ok) {
            w.cm[pos] = i;
            for (int c = 0; c < 3; ++c) { w.X1[3 * pos + c] = X1[c]; w.X2[3 * pos + c] = X2[c]; }
            w.P1[2 * pos] = p1[0]; w.P1[2 * pos + 1] = p1[1]; w.P2[2 * pos] = p2[0]; w.P2[2 * pos + 1] = p2[1];
        }
    }
    if (tid == 0) {
        const int N = base;                                                // N <= n1: inside the table of n1 + 1 entries
        const bool few = N < 3 || N < a.min_inliers || (a.num_matches && *a.num_matches < a.min_matches);
        w.sel[0] = N; w.sel[1] = few ? 0 : geo_clamp_its(a.iters_of_N[N], a.max_iters);
    }
}

__global__ __launch_bounds__(XFH_S3_FIT_LANES)
void k_sim3solve_fit(S3Args a) {
    const int it = blockIdx.x * XFH_S3_FIT_LANES + threadIdx.x, b = blockIdx.y;
    const S3Ws w = s3_ws(a, b);
    const int N = w.sel[0], its = w.sel[1];
    if (it >= its) return;                                                 // (no barrier below; its <= max_iters, so the draws are inside the caller's list)
    int set[3];
    geo_set<3>(a.draws + (size_t)b * a.draws_stride + 3 * (size_t)it, a.rand_max, N, set);
    float p1[9], p2[9], h[S3_HYP];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) { p1[3 * j + c] = w.X1[3 * (size_t)set[j] + c]; p2[3 * j + c] = w.X2[3 * (size_t)set[j] + c]; }
    s3_horn(p1, p2, a.fix_scale != 0, h);
    float* dst = w.hyp + (size_t)it * S3_HYP;
#pragma unroll
    for (int k = 0; k < S3_HYP; ++k) dst[k] = h[k];
}

__global__ __launch_bounds__(XFH_S3_THREADS)
void k_sim3solve_count(S3Args a) {
    const int lane = threadIdx.x & 63, it = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    const S3Ws w = s3_ws(a, b);
    const int N = w.sel[0], its = w.sel[1];
    if (it >= its) return;                                                 // (the whole wave; no barrier below)
    float T12[12], T21[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) { T12[k] = w.hyp[(size_t)it * S3_HYP + S3_F_T12 + k]; T21[k] = w.hyp[(size_t)it * S3_HYP + S3_F_T21 + k]; }
    const int count = wave_count(N, [&](int k) {
        float err[2];
        return s3_check(T12, T21, a.cam1, a.cam2, w.X1 + 3 * (size_t)k, w.X2 + 3 * (size_t)k, w.P1 + 2 * (size_t)k, w.P2 + 2 * (size_t)k, a.max_err1, a.max_err2, err) != 0;
    });
    if (lane == 0) w.cnt[it] = count;
}

__global__ __launch_bounds__(XFH_S3_THREADS)
void k_sim3solve_decide(S3Args a) {
    __shared__ int s_first, s_key;
    const int tid = threadIdx.x, b = blockIdx.x, n1 = a.n1;
    const S3Ws w = s3_ws(a, b);
    const int N = w.sel[0], its = w.sel[1];
    int* hdr = a.header + (size_t)b * S3_HEADER_INTS;
    if (its == 0) {                                                        // TOO_FEW: the header and nothing else
        if (tid == 0) s3_too_few_header(hdr, N);
        return;
    }
    if (tid == 0) { s_first = INT_MAX; s_key = -1; }
    __syncthreads();
    int first = INT_MAX, key = -1;
    for (int k = tid; k < its; k += XFH_S3_THREADS) {
        const int c = w.cnt[k];
        if (c > a.min_inliers && k < first) first = k;
        const int kk = s3_best_key(c, k);
        key = kk > key ? kk : key;
    }
    atomicMin(&s_first, first); atomicMax(&s_key, key);                    // LDS, integers: order-free
    __syncthreads();
    const int winner = s_first == INT_MAX ? -1 : s_first;
    const int best = winner >= 0 ? winner : s_key % S3_MAX_ITERS;
    const float* h = w.hyp + (size_t)best * S3_HYP;
    float T12[12], T21[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) { T12[k] = h[S3_F_T12 + k]; T21[k] = h[S3_F_T21 + k]; }
    for (int i = tid; i < n1; i += XFH_S3_THREADS) {
        int in = 0;
        float X1[3], X2[3], p1[2], p2[2], err[2];
        if (winner >= 0 && s3_corr(a, b, i, X1, X2, p1, p2)) in = s3_check(T12, T21, a.cam1, a.cam2, X1, X2, p1, p2, a.max_err1, a.max_err2, err);
        a.inliers[(size_t)b * n1 + i] = (unsigned char)in;
    }
    if (tid < S3_FLOATS) a.fout[(size_t)b * S3_FLOATS + tid] = tid < S3_F_T21 ? h[tid] : 0.0f;
    if (tid != 0) return;
    if (winner >= 0) {
        float hh[S3_F_T21], Tcw[12], Ow[3];
        for (int k = 0; k < S3_F_T21; ++k) hh[k] = h[k];
        s3_compose(hh, a.T2w + (size_t)b * 12, Tcw, Ow);
        for (int k = 0; k < 12; ++k) a.Tcw[(size_t)b * 12 + k] = Tcw[k];
        for (int k = 0; k < 3; ++k) a.Ow[(size_t)b * 3 + k] = Ow[k];
    }
    for (int k = S3_H_CONSUMED + 1; k < S3_HEADER_INTS; ++k) hdr[k] = 0;
    hdr[S3_H_N] = N; hdr[S3_H_STATUS] = winner >= 0 ? S3_CONVERGED : S3_NO_MORE; hdr[S3_H_ITS] = its; hdr[S3_H_WINNER] = winner;
    hdr[S3_H_NINL] = winner >= 0 ? w.cnt[winner] : 0; hdr[S3_H_BEST] = best; hdr[S3_H_BEST_COUNT] = w.cnt[best]; hdr[S3_H_CONSUMED] = winner >= 0 ? winner + 1 : its;
}

hipError_t launch_sim3_solve(xfh_ctx* c, const S3Args& a) {
    launch_k(c, XFH_K_SIM3SOLVE_PREPARE, -1, k_sim3solve_prepare, dim3(a.B), dim3(XFH_S3_THREADS), 0, a);
    launch_k(c, XFH_K_SIM3SOLVE_FIT, -1, k_sim3solve_fit, dim3((a.max_iters + XFH_S3_FIT_LANES - 1) / XFH_S3_FIT_LANES, a.B), dim3(XFH_S3_FIT_LANES), 0, a);
    launch_k(c, XFH_K_SIM3SOLVE_COUNT, -1, k_sim3solve_count, dim3((a.max_iters + 3) / 4, a.B), dim3(XFH_S3_THREADS), 0, a);
    launch_k(c, XFH_K_SIM3SOLVE_DECIDE, -1, k_sim3solve_decide, dim3(a.B), dim3(XFH_S3_THREADS), 0, a);
    return hipGetLastError();
}

// ---- the merge -----------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(XFH_S3_THREADS)
void k_sim3merge_init(S3MergeArgs a) {
    const int i = blockIdx.x * XFH_S3_THREADS + threadIdx.x;
    if (i < a.M) a.owner[i] = INT_MAX;
    if (i == 0) *a.num = 0;
}
__global__ __launch_bounds__(XFH_S3_THREADS)
void k_sim3merge_claim(S3MergeArgs a) {
    const int k = blockIdx.x * XFH_S3_THREADS + threadIdx.x, j = blockIdx.y;
    if (k >= a.n1) return;
    const int r = s3_merge_row(a.match12, a.point2, a.n1, a.n2, a.M, j, k);
    if (r >= 0) atomicMin(a.owner + r, j * a.n1 + k);
}
__global__ __launch_bounds__(XFH_S3_THREADS)
void k_sim3merge_select(S3MergeArgs a) {
    const int k = blockIdx.x * XFH_S3_THREADS + threadIdx.x;
    int owners = 0;
    if (k < a.n1) {
        int m, kf;
        owners = s3_merge_slot(a.match12, a.point2, a.owner, a.J, a.n1, a.n2, a.M, k, &m, &kf);
        a.matched[k] = m; a.matched_kf[k] = kf;
    }
    owners = wave_sum_i32(owners);
    if ((threadIdx.x & 63) == 0 && owners) atomicAdd(a.num, owners);
}

hipError_t launch_sim3_merge(xfh_ctx* c, const S3MergeArgs& a) {
    const int mb = (a.M + XFH_S3_THREADS - 1) / XFH_S3_THREADS, kb = (a.n1 + XFH_S3_THREADS - 1) / XFH_S3_THREADS;
    launch_k(c, XFH_K_SIM3SOLVE_MERGE, -1, k_sim3merge_init, dim3(mb), dim3(XFH_S3_THREADS), 0, a);
    launch_k(c, XFH_K_SIM3SOLVE_MERGE, -1, k_sim3merge_claim, dim3(kb, a.J), dim3(XFH_S3_THREADS), 0, a);
    launch_k(c, XFH_K_SIM3SOLVE_MERGE, -1, k_sim3merge_select, dim3(kb), dim3(XFH_S3_THREADS), 0, a);
    return hipGetLastError();
}
