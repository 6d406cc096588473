// mlpnp.hip.h -- MLPnPsolver (src/MLPnPsolver.cpp) under the iterate(chunk) calls of Tracking::Relocalization for B candidates per call (included by
// kernels_mlpnp.hip).  The contract is in include/xfeat_hip.h; the arithmetic is mlpnp_math.h, the host's own lines.  Six launches, whatever the data:
//
//   k_mlpnp_prepare  one workgroup per problem: the compact correspondence list in keypoint order (ordered scan: ballot + popcount inside a wave, the
//                    four wave totals in order, never an atomic counter) with point, keypoint position, bearing vector and null-space basis; N, the
//                    iteration count and min_inliers_eff from the caller's tables, the end of the loop (its == 0 = TOO_FEW: the later kernels leave).
//   k_mlpnp_fit      one lane per (problem, iteration), 16 lanes per workgroup: the minimal set from the raw draws and computePose on its six points.
//                    A^T A (12 x 12) and V of the fp64 Jacobi live in LDS, element k of lane l at [k][l]: no run-time index reaches a register array
//                    of that size.  All B x end hypotheses share one grid.
//   k_mlpnp_count    one wave per (problem, iteration): CheckInliers over the N correspondences, ballot + popcount.  Only the count is written.
//   k_mlpnp_records  one lane per problem: the prefix maxima of the counts (the distinct bests) and where each is first consulted.
//   k_mlpnp_refine   one workgroup per (problem, record): the record's flags recomputed (a 64-bit mask per lane: lane l owns the correspondences l,
//                    l + 256, ..), computePose on them with every sum folded over the 256 lanes in LDS, 13 sums per pass, then its inlier count.
//   k_mlpnp_decide   one workgroup per problem: the winner among the records, the header, the pose, the flags and d_assigned_out per keypoint.
// No global atomics, no waiting between workgroups; every loop is bounded (Jacobi sweeps <= 30, Gauss-Newton rounds <= 5).
#pragma once
#include "mlpnp_math.h"
#include "block_common.hip.h"

#define XFH_ML_THREADS GEO_LANES
#define XFH_ML_FIT_LANES 16

__global__ __launch_bounds__(XFH_ML_THREADS)
void k_mlpnp_prepare(MlArgs a) {
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x, b = blockIdx.x, n = a.n;
    const MlWs w = ml_ws(a, b);
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += XFH_ML_THREADS) {
        const int i = i0 + tid;
        float pt[3];
        const bool ok = i < n && ml_corr_of(a, b, i, pt);
        __syncthreads();                                                   // s_cnt is free
        const size_t c = (size_t)block_compact_step(ok, s_cnt, base);      // c < n
        if (ok) {
            w.cm[c] = i;
            for (int k = 0; k < 3; ++k) w.pt[3 * c + k] = pt[k];
            const float x = a.xy_un[2 * (size_t)i], y = a.xy_un[2 * (size_t)i + 1];
            w.xy[2 * c] = x; w.xy[2 * c + 1] = y;
            float f[3];
            ml_bearing(a.cam, x, y, f);
            double rs[6];
            const double fd[3] = {(double)f[0], (double)f[1], (double)f[2]};
            ml_nullspace(fd, rs);
            for (int k = 0; k < 3; ++k) w.f[3 * c + k] = f[k];
            for (int k = 0; k < 6; ++k) w.rs[6 * c + k] = rs[k];
        }
    }
    if (tid == 0) ml_select(a, b, base, w.sel);                            // base <= n
}

__global__ __launch_bounds__(XFH_ML_FIT_LANES)
void k_mlpnp_fit(MlArgs a) {
    __shared__ double s_m[288 * XFH_ML_FIT_LANES];
    const int tid = threadIdx.x, it = blockIdx.x * XFH_ML_FIT_LANES + tid, b = blockIdx.y;
    const MlWs w = ml_ws(a, b);
    if (it >= w.sel[ML_S_END]) return;                                     // (no barrier below; end <= max_iters, so the draws are inside the caller's list)
    const GeoMat U{s_m + tid, XFH_ML_FIT_LANES}, V{s_m + 144 * XFH_ML_FIT_LANES + tid, XFH_ML_FIT_LANES};
    double h[ML_HYP];
    ml_fit_iteration(a, b, w, it, U, V, h);
    double* dst = w.hyp + (size_t)it * ML_HYP;
#pragma unroll
    for (int k = 0; k < ML_HYP; ++k) dst[k] = h[k];
}

__global__ __launch_bounds__(XFH_ML_THREADS)
void k_mlpnp_count(MlArgs a) {
    const int lane = threadIdx.x & 63, it = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    const MlWs w = ml_ws(a, b);
    const int N = w.sel[ML_S_N];
    if (it >= w.sel[ML_S_END]) return;                                     // (the whole wave; no barrier below)
    double Rt[12];
    ml_hyp_Rt(w.hyp + (size_t)it * ML_HYP, Rt);
    const int count = wave_count(N, [&](int k) { float e; return ml_check(Rt, a.cam, w.pt + 3 * (size_t)k, w.xy + 2 * (size_t)k, a.max_err, &e) != 0; });
    if (lane == 0) w.cnt[it] = count;
}

__global__ __launch_bounds__(64)
void k_mlpnp_records(MlArgs a) {
    const int b = blockIdx.x;
    const MlWs w = ml_ws(a, b);
    if (threadIdx.x != 0 || w.sel[ML_S_ITS] == 0) return;
    ml_scan(w.cnt, w.sel[ML_S_END], w.sel[ML_S_K0], w.sel[ML_S_MIN], w.rec_it, w.rec_use, w.sel);       // at most end <= max_iters records
}

// the flagged correspondences of one record, the sums folded by the workgroup (MlHostFold's adds, lane by lane)
struct MlBlock {
    const MlWs& w; int N; unsigned long long mask; double* s_fold; const int* s_first;
    __device__ __forceinline__ void corr(int c, double* fo, double* po, double* r, double* s) const {
        for (int k = 0; k < 3; ++k) { fo[k] = (double)w.f[3 * (size_t)c + k]; po[k] = (double)w.pt[3 * (size_t)c + k]; r[k] = w.rs[6 * (size_t)c + k]; s[k] = w.rs[6 * (size_t)c + 3 + k]; }
    }
    __device__ __forceinline__ int first(int j) const { return s_first[j]; }
    __device__ __forceinline__ bool leader() const { return threadIdx.x == 0; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    template <int K, class F> __device__ __forceinline__ void sum(F term, double* out) const {
        const int tid = threadIdx.x;
        double part[K], t[K];
#pragma unroll
        for (int k = 0; k < K; ++k) part[k] = 0.0;
        for (int j = 0, c = tid; c < N; ++j, c += XFH_ML_THREADS)
            if ((mask >> j) & 1ull) {
                term(c, t);
#pragma unroll
                for (int k = 0; k < K; ++k) part[k] = part[k] + t[k];
            }
        block_tree_fold<double, K>(s_fold, part, out);
    }
};

__global__ __launch_bounds__(XFH_ML_THREADS)
void k_mlpnp_refine(MlArgs a) {
    __shared__ double s_fold[ML_CHUNK * XFH_ML_THREADS];
    __shared__ double s_m[288];
    __shared__ MlShared s_sh;
    __shared__ int s_first[6], s_cnt[4];
    const int tid = threadIdx.x, r = blockIdx.x, b = blockIdx.y;
    const MlWs w = ml_ws(a, b);
    if (w.sel[ML_S_ITS] == 0 || r >= w.sel[ML_S_NREC]) return;             // (the whole workgroup)
    double* rec = w.rec + (size_t)r * ML_HYP;
    if (w.rec_use[r] < 0) {                                                 // never consulted at k >= k0
        if (tid < ML_HYP) rec[tid] = 0.0;
        return;
    }
    const int N = w.sel[ML_S_N];                                           // N <= XFH_GRID_MAX_N = 64 * 256: one bit per owned correspondence
    double Rt[12];
    ml_hyp_Rt(w.hyp + (size_t)w.rec_it[r] * ML_HYP, Rt);
    unsigned long long mask = 0ull;
    int base = 0;
    for (int j = 0, c0 = 0; c0 < N; ++j, c0 += XFH_ML_THREADS) {
        const int c = c0 + tid;
        float e;
        const bool in = c < N && ml_check(Rt, a.cam, w.pt + 3 * (size_t)c, w.xy + 2 * (size_t)c, a.max_err, &e);
        if (in) mask |= 1ull << j;
        __syncthreads();                                                   // s_cnt is free
        const int pos = block_compact_step(in, s_cnt, base);
        if (in && pos < 6) s_first[pos] = c;
    }
    __syncthreads();
    if (base < 6) {                                                         // (cannot happen: a record's count is >= min_inliers_eff >= 6; the whole workgroup)
        if (tid < ML_HYP) rec[tid] = 0.0;
        return;
    }
    MlBlock cx{w, N, mask, s_fold, s_first};
    double Rr[12]; int planar;
    ml_compute_pose(cx, GeoMat{s_m, 1}, GeoMat{s_m + 144, 1}, &s_sh, Rr, &planar);
    int count = 0;
    for (int c = tid; c < N; c += XFH_ML_THREADS) { float e; count += ml_check(Rr, a.cam, w.pt + 3 * (size_t)c, w.xy + 2 * (size_t)c, a.max_err, &e); }
    count = block_sum_i32(s_cnt, count);
    if (tid != 0) return;
    for (int rr = 0; rr < 3; ++rr) { for (int cc = 0; cc < 3; ++cc) rec[ML_P_R + 3 * rr + cc] = Rr[4 * rr + cc]; rec[ML_P_T + rr] = Rr[4 * rr + 3]; }
    rec[ML_P_PLANAR] = (double)planar; rec[ML_P_COUNT] = (double)count; rec[14] = 0.0; rec[15] = 0.0;
}

__global__ __launch_bounds__(XFH_ML_THREADS)
void k_mlpnp_decide(MlArgs a) {
    const int tid = threadIdx.x, b = blockIdx.x, n = a.n;
    const MlWs w = ml_ws(a, b);
    int* hdr = a.header + (size_t)b * ML_HEADER_INTS;
    if (w.sel[ML_S_ITS] == 0) {                                            // TOO_FEW: the header, and no match for the optimiser behind
        if (tid == 0) ml_too_few_header(hdr, w.sel[ML_S_N]);
        for (int i = tid; i < n; i += XFH_ML_THREADS) a.assigned_out[(size_t)b * n + i] = -1;
        return;
    }
    int h[ML_HEADER_INTS];
    const double* rep = ml_decide(w, h);                                   // every lane: the same few reads
    if (tid < ML_HEADER_INTS) {
#pragma unroll
        for (int k = 0; k < ML_HEADER_INTS; ++k) if (k == tid) hdr[k] = h[k];
    }
    double Rt[12];
    if (rep) {
        ml_hyp_Rt(rep, Rt);
        if (tid < 12) {
#pragma unroll
            for (int k = 0; k < 12; ++k) if (k == tid) a.Tcw[(size_t)b * 12 + k] = (float)Rt[k];
        }
    }
    for (int i = tid; i < n; i += XFH_ML_THREADS) {
        int in = 0;
        float pt[3], e;
        if (rep && ml_corr_of(a, b, i, pt)) {
            const float xy[2] = {a.xy_un[2 * (size_t)i], a.xy_un[2 * (size_t)i + 1]};
            in = ml_check(Rt, a.cam, pt, xy, a.max_err, &e);
        }
        const size_t o = (size_t)b * n + i;
        a.inliers[o] = (unsigned char)in;
        a.assigned_out[o] = in ? a.assigned[o] : -1;
    }
}

hipError_t launch_mlpnp_solve(xfh_ctx* c, const MlArgs& a) {
    launch_k(c, XFH_K_MLPNP_PREPARE, -1, k_mlpnp_prepare, dim3(a.B), dim3(XFH_ML_THREADS), 0, a);
    launch_k(c, XFH_K_MLPNP_FIT, -1, k_mlpnp_fit, dim3((a.max_iters + XFH_ML_FIT_LANES - 1) / XFH_ML_FIT_LANES, a.B), dim3(XFH_ML_FIT_LANES), 0, a);
    launch_k(c, XFH_K_MLPNP_COUNT, -1, k_mlpnp_count, dim3((a.max_iters + 3) / 4, a.B), dim3(XFH_ML_THREADS), 0, a);
    launch_k(c, XFH_K_MLPNP_RECORDS, -1, k_mlpnp_records, dim3(a.B), dim3(64), 0, a);
    launch_k(c, XFH_K_MLPNP_REFINE, -1, k_mlpnp_refine, dim3(a.max_iters, a.B), dim3(XFH_ML_THREADS), 0, a);
    launch_k(c, XFH_K_MLPNP_DECIDE, -1, k_mlpnp_decide, dim3(a.B), dim3(XFH_ML_THREADS), 0, a);
    return hipGetLastError();
}
