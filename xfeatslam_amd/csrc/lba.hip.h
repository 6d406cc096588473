// lba.hip.h -- the kernels of xfh_local_ba_device (included by kernels_lba.hip): Optimizer::LocalBundleAdjustment as a FIXED schedule of launches on the
// ctx stream.  The contract is in include/xfeat_hip.h; the arithmetic, and each step as a function of one work item, is lba_math.h.
//
// The schedule (launch_local_ba): four plan launches, then for each of the max_iterations iterations BUILD (k_lba_linearize<true>, k_lba_point_build,
// k_lba_begin) and ten times TRIAL (k_lba_schur, k_lba_solve, k_lba_update, k_lba_linearize<false>, k_lba_decide), then k_lba_finish and
// k_lba_header: 4 + max_iterations * 53 + 2 launches, 536 for optimize(10).  The host never learns how the optimisation went: every kernel reads the
// control block (LbaCtl, first in the workspace) and returns at once unless its step is the one the machine wants (act) in the iteration it was
// launched for (iter).  A kernel hands data to a LATER kernel of the stream only, never to a running workgroup: no grid barrier, no flag, no spin.
//
// The work is spread by keyframe (one workgroup of 256 lanes per keyframe: errors, Jacobians, the edge records, the fold of Hpp, bp and the robust
// chi2), by point (one lane per point: Hll, bl, the back-substitution) and by pair of free keyframes (one workgroup per block of S on or above the
// diagonal).  The LDL^T of S and the two substitutions run in ONE workgroup of 1024 lanes on S in the workspace: 768 x 768 doubles are 4.5 MiB, 29
// times the 160 KiB of LDS a CU has, and a column's hand-off between workgroups would need the grid barrier the schedule does without.
// Every fold is block_fold below: the xor butterfly inside a wave, the four waves in order on lane 0.  No floating-point atomic anywhere: two runs
// give identical bytes.  The only atomic is the integer count of erase flags.
#pragma once
#include "lba_math.h"
#include "search_common.hip.h"

// the N sums of a workgroup of 256: out[n] on lane 0 (every lane must call; ends behind a barrier)
template <int N>
__device__ __forceinline__ void lba_block_fold(const double* acc, double (*s_red)[N], double* out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int n = 0; n < N; ++n) { const double s = wave_sum_f64(acc[n]); if (lane == 0) s_red[wave][n] = s; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int n = 0; n < N; ++n) out[n] = ((s_red[0][n] + s_red[1][n]) + s_red[2][n]) + s_red[3][n];
    }
}
#define LBA_WS(a) lba_ws((a).ws, (a).nK, (a).nP, (a).nE, (a).n_free)

// ---- the plan ------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(XFH_LBA_THREADS) void k_lba_plan_edges(LbaArgs a) {
    const LbaWs w = LBA_WS(a);
    const int t = blockIdx.x * XFH_LBA_THREADS + threadIdx.x;
    if (t < a.nE) w.edge_pt[t] = lba_edge_plan(a, t);
    if (t < a.nK) lba_kf_init(a, w, t);
}
// blocks 0 .. nK - 1: one wave per keyframe counts its edges; the blocks behind them: one lane per point
__global__ __launch_bounds__(64) void k_lba_plan_count(LbaArgs a) {
    const LbaWs w = LBA_WS(a);
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= a.nK) {
        const int p = ((int)blockIdx.x - a.nK) * 64 + lane;
        if (p < a.nP) lba_point_init(a, w, p);
        return;
    }
    const int k = blockIdx.x;
    int n = 0, s = 0;
    for (int e = lane; e < a.nE; e += 64)
        if (w.edge_pt[e] >= 0 && a.edge_kf[e] == k) { ++n; s += lba_stereo(a, e) ? 1 : 0; }
    n = wave_sum_i32(n); s = wave_sum_i32(s);
    if (lane == 0) { w.kf_cnt[k] = n; w.kf_stereo[k] = s; w.kf_mono[k] = n - s; }
}
__global__ __launch_bounds__(64) void k_lba_plan_scan(LbaArgs a) {
    if (threadIdx.x == 0) lba_plan_scan(a, LBA_WS(a));
}
// the keyframe-major index: keyframe k's edges in ascending edge order (one wave; a chunk of 64 edges per step, placed by the ballot's prefix)
__global__ __launch_bounds__(64) void k_lba_plan_fill(LbaArgs a) {
    const LbaWs w = LBA_WS(a);
    const int k = blockIdx.x, lane = threadIdx.x;
    int base = w.kf_begin[k];
    const int end = base + w.kf_cnt[k];
    for (int e0 = 0; e0 < a.nE; e0 += 64) {
        const int e = e0 + lane;
        const bool mine = e < a.nE && w.edge_pt[e] >= 0 && a.edge_kf[e] == k;
        const u64 m = __ballot(mine);
        const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
        if (mine && pos < end) w.kf_edges[pos] = e;
        base += __popcll(m);
    }
}

// ---- BUILD ---------------------------------------------------------------------------------------------------------------------------------------------
// BUILD = true: computeActiveErrors + linearizeOplus + the pose side of buildSystem at the estimate; false: computeActiveErrors at the trial estimate
template <bool BUILD>
__global__ __launch_bounds__(XFH_LBA_THREADS) void k_lba_linearize(LbaArgs a, int it) {
    const LbaWs w = LBA_WS(a);
    const LbaCtl& c = *w.ctl;
    if (c.act != (BUILD ? LBA_BUILD : LBA_TRIAL) || c.iter != it) return;
    constexpr int N = BUILD ? XFH_POSE_NSUM : 1;
    __shared__ double s_red[XFH_LBA_THREADS / 64][N];
    const int k = blockIdx.x;
    double acc[XFH_POSE_NSUM];
#pragma unroll
    for (int n = 0; n < XFH_POSE_NSUM; ++n) acc[n] = 0.0;
    lba_kf_lane(a, w, k, threadIdx.x, BUILD ? c.cur : 1 - c.cur, BUILD, acc);
    if constexpr (BUILD) {
        double out[XFH_POSE_NSUM];
        lba_block_fold<N>(acc, s_red, out);
        if (threadIdx.x == 0)
            for (int n = 0; n < XFH_POSE_NSUM; ++n) w.kf_sum[(size_t)XFH_POSE_NSUM * k + n] = out[n];
    } else {
        double out[1];
        lba_block_fold<1>(acc + 27, s_red, out);
        if (threadIdx.x == 0) w.kf_chi[k] = out[0];
    }
}
__global__ __launch_bounds__(XFH_LBA_THREADS) void k_lba_point_build(LbaArgs a, int it) {
    const LbaWs w = LBA_WS(a);
    if (w.ctl->act != LBA_BUILD || w.ctl->iter != it) return;
    const int p = blockIdx.x * XFH_LBA_THREADS + threadIdx.x;
    if (p < a.nP) lba_point_build(a, w, p);
}
// the 256-lane fold of count terms: lane l adds the terms l, l + 256, ...
template <class Term>
__device__ __forceinline__ double lba_fold_terms(int count, Term term, double (*s_red)[1]) {
    double s = 0.0, out[1] = {0.0};
    for (int j = threadIdx.x; j < count; j += XFH_LBA_THREADS) s += term(j);
    lba_block_fold<1>(&s, s_red, out);
    __syncthreads();                                                          // s_red is free again
    return out[0];
}
// currentChi and, in iteration 0, computeLambdaInit: one workgroup
__global__ __launch_bounds__(XFH_LBA_THREADS) void k_lba_begin(LbaArgs a, int it) {
    const LbaWs w = LBA_WS(a);
    LbaCtl& c = *w.ctl;
    if (c.act != LBA_BUILD || c.iter != it) return;
    __shared__ double s_red[XFH_LBA_THREADS / 64][1], s_m[XFH_LBA_THREADS];
    __shared__ int s_nan[XFH_LBA_THREADS];
    const int tid = threadIdx.x;
    const double chi = lba_fold_terms(a.nK, [&](int k) { return w.kf_sum[(size_t)XFH_POSE_NSUM * k + 27]; }, s_red);
    const int T = 6 * a.n_free + 3 * a.nP, chunk = (T + XFH_LBA_THREADS - 1) / XFH_LBA_THREADS;
    double m = 0.0;
    int nan = 0;
    for (int j = tid * chunk; j < T && j < (tid + 1) * chunk; ++j) lba_max_step(lba_diag_entry(a, w, j), &m, &nan);
    s_m[tid] = m; s_nan[tid] = nan;
    __syncthreads();
    if (tid == 0) {
        m = 0.0; nan = 0;
        for (int l = 0; l < XFH_LBA_THREADS; ++l) lba_max_join(s_m[l], s_nan[l], &m, &nan);
        lba_lm_after_build(c, chi, m);
    }
}

// ---- TRIAL ---------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(XFH_LBA_THREADS) void k_lba_schur(LbaArgs a, int it) {
    const LbaWs w = LBA_WS(a);
    if (w.ctl->act != LBA_TRIAL || w.ctl->iter != it) return;
    __shared__ double s_red[XFH_LBA_THREADS / 64][42];
    int i = 0, r = blockIdx.x;
    for (int s = 0; s < XFH_LBA_MAX_FREE_KF && r >= a.n_free - i; ++s) { r -= a.n_free - i; ++i; }
    const int j = i + r;
    if (i >= a.n_free || j >= a.n_free) return;
    double acc[42], out[42];
#pragma unroll
    for (int n = 0; n < 42; ++n) acc[n] = 0.0;
    lba_schur_lane(a, w, i, j, threadIdx.x, acc);
    lba_block_fold<42>(acc, s_red, out);
    if (threadIdx.x == 0) lba_schur_store(a, w, i, j, out);
}
// the operations of lba_ldlt_solve_host over one workgroup: a column of L, a barrier, the rank-1 update of the trailing lower triangle, a barrier; the
// substitutions one column per barrier, lane i owning unknown i (n <= 768 < 1024)
__global__ __launch_bounds__(XFH_LBA_SOLVE_THREADS) void k_lba_solve(LbaArgs a, int it) {
    const LbaWs w = LBA_WS(a);
    LbaCtl& c = *w.ctl;
    if (c.act != LBA_TRIAL || c.iter != it) return;
    __shared__ double col[6 * XFH_LBA_MAX_FREE_KF], yv[6 * XFH_LBA_MAX_FREE_KF];
    const int n = 6 * a.n_free, tid = threadIdx.x;
    const size_t N = (size_t)n;
    double* S = w.S;
    bool ok = true;
    for (int k = 0; k < n; ++k) {
        const double dk = S[k * N + k];                                      // the same word on every lane: the loop ends for all of them together
        if (!(dk > 0.0)) { ok = false; break; }
        for (int i = k + 1 + tid; i < n; i += XFH_LBA_SOLVE_THREADS) { const double l = S[i * N + k] / dk; S[i * N + k] = l; col[i] = l; }
        __syncthreads();
        for (int i = k + 1 + (tid >> 5); i < n; i += XFH_LBA_SOLVE_THREADS / 32)      // 32 rows at a time, 32 consecutive entries of a row per half wave
            for (int j = k + 1 + (tid & 31); j <= i; j += 32) S[i * N + j] = S[i * N + j] - col[i] * col[j] * dk;
        __syncthreads();
    }
    if (ok) {
        if (tid < n) yv[tid] = w.bS[tid];
        __syncthreads();
        for (int k = 0; k < n; ++k) {
            const double yk = yv[k];
            if (tid > k && tid < n) yv[tid] = yv[tid] - S[tid * N + k] * yk;
            __syncthreads();
        }
        if (tid < n) yv[tid] = yv[tid] / S[tid * N + tid];
        __syncthreads();
        for (int k = n - 1; k >= 0; --k) {
            const double xk = yv[k];
            if (tid < k) yv[tid] = yv[tid] - S[k * N + tid] * xk;
            __syncthreads();
        }
        if (tid < n) w.xp[tid] = yv[tid];
    }
    if (tid == 0) c.solved = ok ? 1 : 0;
}
__global__ __launch_bounds__(XFH_LBA_THREADS) void k_lba_update(LbaArgs a, int it) {
    const LbaWs w = LBA_WS(a);
    if (w.ctl->act != LBA_TRIAL || w.ctl->iter != it) return;
    const int t = blockIdx.x * XFH_LBA_THREADS + threadIdx.x;
    if (t < a.nP) lba_point_update(a, w, t);
    else if (t - a.nP < a.nK) lba_kf_update(a, w, t - a.nP);
}
__global__ __launch_bounds__(XFH_LBA_THREADS) void k_lba_decide(LbaArgs a, int it) {
    const LbaWs w = LBA_WS(a);
    LbaCtl& c = *w.ctl;
    if (c.act != LBA_TRIAL || c.iter != it) return;
    __shared__ double s_red[XFH_LBA_THREADS / 64][1];
    const double chi = lba_fold_terms(a.nK, [&](int k) { return w.kf_chi[k]; }, s_red);
    const double scale = lba_fold_terms(6 * a.n_free + a.nP, [&](int j) { return lba_scale_term(a, w, j); }, s_red);
    if (threadIdx.x == 0) lba_lm_after_trial(c, chi, scale);
}

// ---- the outputs ---------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(XFH_LBA_THREADS) void k_lba_finish(LbaArgs a) {
    const LbaWs w = LBA_WS(a);
    const int t = blockIdx.x * XFH_LBA_THREADS + threadIdx.x;
    if (t < a.nK) lba_finish_kf(a, w, t);
    if (t < a.nP) lba_finish_point(a, w, t);
    int n = t < a.nE ? lba_finish_edge(a, w, t) : 0;
    n = wave_sum_i32(n);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&w.ctl->n_erase, n);
}
__global__ __launch_bounds__(64) void k_lba_header(LbaArgs a) {
    if (threadIdx.x == 0) lba_finish_header(a, LBA_WS(a));
}

hipError_t launch_local_ba(xfh_ctx* c, const LbaArgs& a) {
    const int T = XFH_LBA_THREADS;
    const int items = a.nE > a.nP ? (a.nE > a.nK ? a.nE : a.nK) : (a.nP > a.nK ? a.nP : a.nK);
    const dim3 g_items((items + T - 1) / T), g_points((a.nP + T - 1) / T), g_update((a.nP + a.nK + T - 1) / T), g_kf(a.nK);
    const int pairs = a.n_free * (a.n_free + 1) / 2;
    launch_k(c, XFH_K_LBA_PLAN, -1, k_lba_plan_edges, g_items, dim3(T), 0, a);
    launch_k(c, XFH_K_LBA_PLAN, -1, k_lba_plan_count, dim3(a.nK + (a.nP + 63) / 64), dim3(64), 0, a);
    launch_k(c, XFH_K_LBA_PLAN, -1, k_lba_plan_scan, dim3(1), dim3(64), 0, a);
    launch_k(c, XFH_K_LBA_PLAN, -1, k_lba_plan_fill, g_kf, dim3(64), 0, a);
    for (int it = 0; it < a.max_it; ++it) {
        launch_k(c, XFH_K_LBA_LINEARIZE, -1, k_lba_linearize<true>, g_kf, dim3(T), 0, a, it);
        launch_k(c, XFH_K_LBA_POINT_BUILD, -1, k_lba_point_build, g_points, dim3(T), 0, a, it);
        launch_k(c, XFH_K_LBA_BEGIN, -1, k_lba_begin, dim3(1), dim3(T), 0, a, it);
        for (int q = 0; q < GEO_LM_MAX_TRIALS; ++q) {
            if (pairs > 0) {
                launch_k(c, XFH_K_LBA_SCHUR, -1, k_lba_schur, dim3(pairs), dim3(T), 0, a, it);
                launch_k(c, XFH_K_LBA_SOLVE, -1, k_lba_solve, dim3(1), dim3(XFH_LBA_SOLVE_THREADS), 0, a, it);
            }
            launch_k(c, XFH_K_LBA_UPDATE, -1, k_lba_update, g_update, dim3(T), 0, a, it);
            launch_k(c, XFH_K_LBA_EVALUATE, -1, k_lba_linearize<false>, g_kf, dim3(T), 0, a, it);
            launch_k(c, XFH_K_LBA_DECIDE, -1, k_lba_decide, dim3(1), dim3(T), 0, a, it);
        }
    }
    launch_k(c, XFH_K_LBA_FINISH, -1, k_lba_finish, g_items, dim3(T), 0, a);
    launch_k(c, XFH_K_LBA_FINISH, -1, k_lba_header, dim3(1), dim3(64), 0, a);
    return hipGetLastError();
}
// xfh_debug_lba_solve: the schedule's k_lba_solve once, as the TRIAL step of iteration 0, on a workspace whose control block, S, b_S and x the caller made
hipError_t launch_lba_solve_alone(xfh_ctx* c, const LbaArgs& a) {
    launch_k(c, XFH_K_LBA_SOLVE, -1, k_lba_solve, dim3(1), dim3(XFH_LBA_SOLVE_THREADS), 0, a, 0);
    return hipGetLastError();
}
