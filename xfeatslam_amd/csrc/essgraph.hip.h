// essgraph.hip.h -- the kernels of xfh_essential_graph_device (included by kernels_essgraph.hip): Optimizer::OptimizeEssentialGraph as launches on the ctx
// stream around a control record (EgCtl, first in the workspace).  The contract is in include/xfeat_hip.h; the arithmetic, and each step as a function of
// one work item, is essgraph_math.h.
//
// Control.  Unlike xfh_local_ba_device this call keeps no fixed idle schedule: a factorisation is 2 x ceil(7 n_free / 64) launches, so ten trial slots per
// iteration would be tens of thousands of idle launches.  The host queues the plan, then one step at a time -- BUILD (k_eg_sims, k_eg_edges<true>,
// k_eg_vertices<true>, k_eg_begin) followed by its first TRIAL, or a TRIAL alone (the fill of S, the factorisation, the substitutions, k_eg_update,
// k_eg_sims, k_eg_edges<false>, k_eg_vertices<false>, k_eg_decide) -- and reads the control record back after every trial: at most 200 reads.  Every
// kernel still checks the record first, so a step queued behind a call that ended in the plan does nothing.  A kernel hands data to a LATER kernel of the
// stream only, never to a running workgroup: no grid barrier, no flag, no spin; every loop has a bound that does not depend on the data.
//
// The blocked LDL^T (k_eg_ldlt_diag, k_eg_ldlt_panel, k_eg_subst): left-looking over block columns of XFH_EG_TILE = 64.  For block column J one workgroup
// brings the diagonal tile up to date -- A[i][j] -= (L[i][k] * L[j][k]) * d[k] for every earlier column k in ASCENDING order, 64 x 32 slices of the two
// tiles of L staged through LDS, a 4 x 4 patch of the tile in each lane's registers -- and eliminates its 64 columns in order; then one workgroup per
// tile below brings its tile up to date the same way and finishes it against the factored diagonal tile.  Every entry therefore receives exactly the
// terms of the column form (lba_ldlt_solve_host), each as two rounded products and one rounded subtraction, in the same order, and is divided by its pivot
// last: the same bits.  Plain fp64 multiplies and subtractions (the library is built without contraction); the fp64 MFMA sums in an order of its own and
// is not used.  A pivot that is not > 0 clears the flag every later kernel of the factorisation reads first.
#pragma once
#include "essgraph_math.h"
#include "search_common.hip.h"

#define EG_WS(a) eg_ws((a).ws, (a).nV, (a).nE, (a).n_free)
#define XFH_EG_SUBST_THREADS 512
#define EG_KC 32                          /* columns of L per LDS slice */
#define EG_LD 66                          /* row stride of a slice in LDS: 64 + 2 keeps the 4-entry reads on 16 bytes and spreads the transposed writes */

// the system the factorisation works on: the lower triangle of S [n][n] (row stride n), b, x, the flag
struct EgSolve { double* S; const double* b; double* x; int* ok; int n; };

template <int N>
__device__ __forceinline__ void eg_block_fold(const double* acc, double (*s_red)[N], double* out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int n = 0; n < N; ++n) { const double s = wave_sum_f64(acc[n]); if (lane == 0) s_red[wave][n] = s; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int n = 0; n < N; ++n) out[n] = ((s_red[0][n] + s_red[1][n]) + s_red[2][n]) + s_red[3][n];
    }
}
template <class Term>
__device__ __forceinline__ double eg_fold_terms(int count, Term term, double (*s_red)[1]) {
    double s = 0.0, out[1] = {0.0};
    for (int j = threadIdx.x; j < count; j += XFH_EG_THREADS) s += term(j);
    eg_block_fold<1>(&s, s_red, out);
    __syncthreads();
    return out[0];
}

// ---- the plan ------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(XFH_EG_THREADS) void k_eg_plan_init(EgArgs a) {
    const EgWs w = EG_WS(a);
    const int t = blockIdx.x * XFH_EG_THREADS + threadIdx.x;
    if (t < a.nV) eg_vertex_init(a, w, t);
    if (t < a.nE) w.edge_ok[t] = eg_edge_plan(a, t);
}
// blocks 0 .. nV - 1: one wave per vertex counts its edges; the blocks behind them: one lane per edge forms the measurement (vScw and Smw are there)
__global__ __launch_bounds__(64) void k_eg_plan_count(EgArgs a) {
    const EgWs w = EG_WS(a);
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= a.nV) {
        const int e = ((int)blockIdx.x - a.nV) * 64 + lane;
        if (e < a.nE) eg_edge_meas(a, w, e);
        return;
    }
    const int v = blockIdx.x;
    int n = 0, n0 = 0, l0 = 0;
    for (int e = lane; e < a.nE; e += 64) { const int bits = eg_count_bits(a, w, e, v); n += bits & 1; n0 += (bits >> 1) & 1; l0 += (bits >> 2) & 1; }
    n = wave_sum_i32(n); n0 = wave_sum_i32(n0); l0 = wave_sum_i32(l0);
    if (lane == 0) { w.v_cnt[v] = n; w.v_lead[v] = n0; w.v_loop[v] = l0; }
}
__global__ __launch_bounds__(64) void k_eg_plan_scan(EgArgs a) {
    if (threadIdx.x == 0) eg_plan_scan(a, EG_WS(a));
}
__global__ __launch_bounds__(64) void k_eg_plan_fill(EgArgs a) {
    const EgWs w = EG_WS(a);
    const int v = blockIdx.x, lane = threadIdx.x;
    int base = w.v_begin[v];
    const int end = base + w.v_cnt[v];
    for (int e0 = 0; e0 < a.nE; e0 += 64) {
        const int e = e0 + lane;
        const bool mine = e < a.nE && eg_incident(a, w, e, v);
        const u64 m = __ballot(mine);
        const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
        if (mine && pos < end) w.v_edges[pos] = e;
        base += __popcll(m);
    }
}

// ---- BUILD and the evaluation of a trial ---------------------------------------------------------------------------------------------------------------
// one lane per (vertex, piece): BUILD = true all 15 pieces at the estimate, false the inverse alone at the trial estimate
template <bool BUILD>
__global__ __launch_bounds__(XFH_EG_THREADS) void k_eg_sims(EgArgs a) {
    const EgWs w = EG_WS(a);
    const EgCtl& c = *w.ctl;
    if (c.act != (BUILD ? EG_BUILD : EG_TRIAL)) return;
    const int t = blockIdx.x * XFH_EG_THREADS + threadIdx.x;
    if constexpr (BUILD) { if (t < 15 * a.nV) eg_sims_piece(a, w, t / 15, t % 15, c.cur); }
    else { if (t < a.nV) eg_sims_piece(a, w, t, 14, 1 - c.cur); }
}
template <bool BUILD>
__global__ __launch_bounds__(XFH_EG_THREADS) void k_eg_edges(EgArgs a) {
    const EgWs w = EG_WS(a);
    const EgCtl& c = *w.ctl;
    if (c.act != (BUILD ? EG_BUILD : EG_TRIAL)) return;
    const int e = blockIdx.x * XFH_EG_THREADS + threadIdx.x;
    if (e < a.nE) eg_edge_step(a, w, e, BUILD ? c.cur : 1 - c.cur, BUILD);
}
template <bool BUILD>
__global__ __launch_bounds__(XFH_EG_THREADS) void k_eg_vertices(EgArgs a) {
    const EgWs w = EG_WS(a);
    if (w.ctl->act != (BUILD ? EG_BUILD : EG_TRIAL)) return;
    constexpr int N = BUILD ? XFH_EG_NSUM : 1;
    __shared__ double s_red[XFH_EG_THREADS / 64][N];
    const int v = blockIdx.x;
    double acc[XFH_EG_NSUM];
#pragma unroll
    for (int n = 0; n < XFH_EG_NSUM; ++n) acc[n] = 0.0;
    eg_vertex_lane(a, w, v, threadIdx.x, BUILD, acc);
    if constexpr (BUILD) {
        double out[XFH_EG_NSUM];
        eg_block_fold<N>(acc, s_red, out);
        if (threadIdx.x == 0)
            for (int n = 0; n < XFH_EG_NSUM; ++n) w.v_sum[(size_t)XFH_EG_NSUM * v + n] = out[n];
    } else {
        double out[1];
        eg_block_fold<1>(acc + 35, s_red, out);
        if (threadIdx.x == 0) w.v_chi[v] = out[0];
    }
}
__global__ __launch_bounds__(XFH_EG_THREADS) void k_eg_begin(EgArgs a) {
    const EgWs w = EG_WS(a);
    EgCtl& c = *w.ctl;
    if (c.act != EG_BUILD) return;
    __shared__ double s_red[XFH_EG_THREADS / 64][1];
    const double chi = eg_fold_terms(a.nV, [&](int v) { return w.v_sum[(size_t)XFH_EG_NSUM * v + 35]; }, s_red);
    if (threadIdx.x == 0) eg_lm_after_build(c, chi);
}

// ---- TRIAL: the system ---------------------------------------------------------------------------------------------------------------------------------
// S is zero (a memset in front); one lane per free vertex (its diagonal block, b) and per edge (the off-diagonal block of its pair); lane 0 raises the flag
__global__ __launch_bounds__(XFH_EG_THREADS) void k_eg_fill(EgArgs a) {
    const EgWs w = EG_WS(a);
    EgCtl& c = *w.ctl;
    const int t = blockIdx.x * XFH_EG_THREADS + threadIdx.x;
    if (c.act != EG_TRIAL) { if (t == 0) c.solved = 0; return; }
    if (t < a.n_free) eg_diag_store(a, w, t);
    if (t < a.nE) eg_pair_store(a, w, t);
    if (t == 0) c.solved = 1;
}

// ---- the blocked LDL^T -----------------------------------------------------------------------------------------------------------------------------------
// C (the lane's 4 x 4 patch of tile (I, J): rows I 64 + 4 ty + a, columns J 64 + 4 tx + b) -= (L[i][k] * L[j][k]) * d[k] for k = 0 .. 64 J - 1 ascending.
// sA / sB: the slices of tile (I, K) and (J, K), transposed to [k][row]; sd: d of the slice.  Rows at or beyond n read as 0 and are never stored.
__device__ __forceinline__ void eg_tile_update(const EgSolve& s, int I, int J, double (*C)[4], double* sA, double* sB, double* sd) {
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const size_t N = (size_t)s.n;
    for (int k0 = 0; k0 < J * XFH_EG_TILE; k0 += EG_KC) {
        __syncthreads();                                                     // the slice before is read
        for (int m = tid; m < XFH_EG_TILE * EG_KC; m += XFH_EG_THREADS) {
            const int r = m / EG_KC, kk = m % EG_KC, ri = I * XFH_EG_TILE + r, rj = J * XFH_EG_TILE + r;
            sA[kk * EG_LD + r] = ri < s.n ? s.S[ri * N + k0 + kk] : 0.0;
            if (I != J) sB[kk * EG_LD + r] = rj < s.n ? s.S[rj * N + k0 + kk] : 0.0;
        }
        if (tid < EG_KC) sd[tid] = s.S[(size_t)(k0 + tid) * N + k0 + tid];
        __syncthreads();
        const double* pB = I != J ? sB : sA;
#pragma unroll 4
        for (int kk = 0; kk < EG_KC; ++kk) {
            const double dk = sd[kk];
            double av[4], bv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { av[q] = sA[kk * EG_LD + 4 * ty + q]; bv[q] = pB[kk * EG_LD + 4 * tx + q]; }
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) C[p][q] = C[p][q] - av[p] * bv[q] * dk;
        }
    }
    __syncthreads();
}
__device__ __forceinline__ void eg_tile_load(const EgSolve& s, int I, int J, double (*C)[4]) {
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = I * XFH_EG_TILE + 4 * ty + p, j = J * XFH_EG_TILE + 4 * tx + q;
            C[p][q] = (i < s.n && j <= i) ? s.S[(size_t)i * s.n + j] : 0.0;
        }
}
// the diagonal tile of block column J: brought up to date, then its columns eliminated in order.  Column k travels through LDS (two buffers in turn, one
// barrier per column): every lane divides the entries it needs by the pivot itself, which gives the bits the owner stores.
__global__ __launch_bounds__(XFH_EG_THREADS) void k_eg_ldlt_diag(EgSolve s, int J) {
    if (*s.ok == 0) return;
    __shared__ double sm[2 * EG_KC * EG_LD], sd[EG_KC], col[2][XFH_EG_TILE];
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15, base = J * XFH_EG_TILE;
    const int kmax = s.n - base < XFH_EG_TILE ? s.n - base : XFH_EG_TILE;
    double C[4][4];
    eg_tile_load(s, J, J, C);
    eg_tile_update(s, J, J, C, sm, sm + EG_KC * EG_LD, sd);
    bool ok = true;
#pragma unroll
    for (int k = 0; k < XFH_EG_TILE; ++k) {
        if (!ok || k >= kmax) continue;                                      // the same on every lane: the barrier below is reached by all or by none
        double* cb = col[k & 1];
        if (tx == k / 4) {
#pragma unroll
            for (int p = 0; p < 4; ++p) cb[4 * ty + p] = C[p][k % 4];
        }
        __syncthreads();
        const double dk = cb[k];
        if (!(dk > 0.0)) { ok = false; continue; }                           // the same word on every lane
        double li[4], lj[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { li[q] = cb[4 * ty + q] / dk; lj[q] = cb[4 * tx + q] / dk; }
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = 4 * ty + p, j = 4 * tx + q;
                if (j > k && j <= i) C[p][q] = C[p][q] - li[p] * lj[q] * dk;
                if (j == k && i > k) C[p][q] = li[p];
            }
    }
    if (!ok) { if (tid == 0) *s.ok = 0; return; }
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = base + 4 * ty + p, j = base + 4 * tx + q;
            if (i < s.n && j <= i) s.S[(size_t)i * s.n + j] = C[p][q];
        }
}
// tile (J + 1 + blockIdx.x, J): brought up to date, then finished against the factored diagonal tile: for k in order L[i][k] = A[i][k] / d[k] and
// A[i][j] -= (L[i][k] * L[j][k]) * d[k] for the later columns j of the tile.  sm holds the diagonal tile transposed, [k][j], d on its diagonal.
__global__ __launch_bounds__(XFH_EG_THREADS) void k_eg_ldlt_panel(EgSolve s, int J) {
    if (*s.ok == 0) return;
    __shared__ double sm[2 * EG_KC * EG_LD], sd[EG_KC], col[2][XFH_EG_TILE];
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15, base = J * XFH_EG_TILE, I = J + 1 + blockIdx.x;
    double C[4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = I * XFH_EG_TILE + 4 * ty + p;
            C[p][q] = i < s.n ? s.S[(size_t)i * s.n + base + 4 * tx + q] : 0.0;
        }
    eg_tile_update(s, I, J, C, sm, sm + EG_KC * EG_LD, sd);
    for (int m = tid; m < XFH_EG_TILE * XFH_EG_TILE; m += XFH_EG_THREADS) {
        const int j = m / XFH_EG_TILE, k = m % XFH_EG_TILE;
        sm[k * XFH_EG_TILE + j] = k <= j ? s.S[(size_t)(base + j) * s.n + base + k] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < XFH_EG_TILE; ++k) {
        double* cb = col[k & 1];
        const double dk = sm[k * XFH_EG_TILE + k];
        if (tx == k / 4) {
#pragma unroll
            for (int p = 0; p < 4; ++p) { const double l = C[p][k % 4] / dk; C[p][k % 4] = l; cb[4 * ty + p] = l; }
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (4 * tx + q > k) C[p][q] = C[p][q] - cb[4 * ty + p] * sm[k * XFH_EG_TILE + 4 * tx + q] * dk;
    }
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = I * XFH_EG_TILE + 4 * ty + p;
            if (i < s.n) s.S[(size_t)i * s.n + base + 4 * tx + q] = C[p][q];
        }
}
// the substitutions in ONE workgroup, by block column: forward in ascending column order, the division by d, backward in DESCENDING column order -- the
// orders of lba_ldlt_solve_host.  The unknowns live in x (written only here, and only when the factorisation held).  Inside a diagonal tile wave 0 works
// alone: lane r holds row (forward) or column (backward) r of the tile in registers and the 64 steps pass the finished unknown by a lane read.
__global__ __launch_bounds__(XFH_EG_SUBST_THREADS) void k_eg_subst(EgSolve s) {
    if (*s.ok == 0) return;
    const int tid = threadIdx.x, n = s.n, nb = (n + XFH_EG_TILE - 1) / XFH_EG_TILE;
    const size_t N = (size_t)n;
    double* y = s.x;
    for (int i = tid; i < n; i += XFH_EG_SUBST_THREADS) y[i] = s.b[i];
    __syncthreads();
    for (int K = 0; K < nb; ++K) {
        const int base = K * XFH_EG_TILE, kmax = n - base < XFH_EG_TILE ? n - base : XFH_EG_TILE;
        if (tid < 64) {
            const int i = base + tid;
            double L[XFH_EG_TILE], v = i < n ? y[i] : 0.0;
#pragma unroll
            for (int kk = 0; kk < XFH_EG_TILE; ++kk) L[kk] = (i < n && kk < tid) ? s.S[i * N + base + kk] : 0.0;
#pragma unroll
            for (int kk = 0; kk < XFH_EG_TILE; ++kk) {
                const double yk = wave_readlane_f64(v, kk);
                if (tid > kk) v = v - L[kk] * yk;
            }
            if (i < n) y[i] = v;
        }
        __syncthreads();
        for (int i = base + XFH_EG_TILE + tid; i < n; i += XFH_EG_SUBST_THREADS) {
            double v = y[i];
            for (int kk = 0; kk < kmax; ++kk) v = v - s.S[i * N + base + kk] * y[base + kk];
            y[i] = v;
        }
        __syncthreads();
    }
    for (int i = tid; i < n; i += XFH_EG_SUBST_THREADS) y[i] = y[i] / s.S[i * N + i];
    __syncthreads();
    for (int K = nb - 1; K >= 0; --K) {
        const int base = K * XFH_EG_TILE, kmax = n - base < XFH_EG_TILE ? n - base : XFH_EG_TILE;
        if (tid < 64) {
            const int i = base + tid;
            double L[XFH_EG_TILE], v = i < n ? y[i] : 0.0;
#pragma unroll
            for (int kk = 0; kk < XFH_EG_TILE; ++kk) L[kk] = (kk > tid && kk < kmax) ? s.S[(size_t)(base + kk) * N + i] : 0.0;
#pragma unroll
            for (int kk = XFH_EG_TILE - 1; kk >= 0; --kk) {
                const double xk = wave_readlane_f64(v, kk);
                if (tid < kk && kk < kmax) v = v - L[kk] * xk;
            }
            if (i < n) y[i] = v;
        }
        __syncthreads();
        for (int i = tid; i < base; i += XFH_EG_SUBST_THREADS) {
            double v = y[i];
            for (int kk = kmax - 1; kk >= 0; --kk) v = v - s.S[(size_t)(base + kk) * N + i] * y[base + kk];
            y[i] = v;
        }
        __syncthreads();
    }
}

// ---- TRIAL: the update and the decision ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(XFH_EG_THREADS) void k_eg_update(EgArgs a) {
    const EgWs w = EG_WS(a);
    if (w.ctl->act != EG_TRIAL) return;
    const int v = blockIdx.x * XFH_EG_THREADS + threadIdx.x;
    if (v < a.nV) eg_vertex_update(a, w, v);
}
__global__ __launch_bounds__(XFH_EG_THREADS) void k_eg_decide(EgArgs a) {
    const EgWs w = EG_WS(a);
    EgCtl& c = *w.ctl;
    if (c.act != EG_TRIAL) return;
    __shared__ double s_red[XFH_EG_THREADS / 64][1];
    const double chi = eg_fold_terms(a.nV, [&](int v) { return w.v_chi[v]; }, s_red);
    const double scale = eg_fold_terms(7 * a.n_free, [&](int j) { return eg_scale_term(w, j); }, s_red);
    if (threadIdx.x == 0) eg_lm_after_trial(c, chi, scale);
}

// ---- the outputs ---------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(XFH_EG_THREADS) void k_eg_finish(EgArgs a) {
    const EgWs w = EG_WS(a);
    const int t = blockIdx.x * XFH_EG_THREADS + threadIdx.x;
    if (t < a.nV) eg_finish_vertex(a, w, t);
    if (t < a.nE) eg_finish_edge(a, w, t);
    int n = t < a.nP ? eg_finish_point(a, w, t) : 0;
    n = wave_sum_i32(n);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&w.ctl->n_points, n);
}
__global__ __launch_bounds__(64) void k_eg_header(EgArgs a) {
    if (threadIdx.x == 0) eg_finish_header(a, EG_WS(a));
}

// ---- the launches ----------------------------------------------------------------------------------------------------------------------------------------
static void eg_launch_solve(xfh_ctx* c, const EgSolve& s) {
    const int nb = (s.n + XFH_EG_TILE - 1) / XFH_EG_TILE;
    for (int J = 0; J < nb; ++J) {
        launch_k(c, XFH_K_EG_FACTOR, -1, k_eg_ldlt_diag, dim3(1), dim3(XFH_EG_THREADS), 0, s, J);
        if (J + 1 < nb) launch_k(c, XFH_K_EG_FACTOR, -1, k_eg_ldlt_panel, dim3(nb - J - 1), dim3(XFH_EG_THREADS), 0, s, J);
    }
    launch_k(c, XFH_K_EG_SUBST, -1, k_eg_subst, dim3(1), dim3(XFH_EG_SUBST_THREADS), 0, s);
}
hipError_t launch_eg_plan(xfh_ctx* c, const EgArgs& a) {
    const int T = XFH_EG_THREADS, items = a.nE > a.nV ? a.nE : a.nV;
    launch_k(c, XFH_K_EG_PLAN, -1, k_eg_plan_init, dim3((items + T - 1) / T), dim3(T), 0, a);
    launch_k(c, XFH_K_EG_PLAN, -1, k_eg_plan_count, dim3(a.nV + (a.nE + 63) / 64), dim3(64), 0, a);
    launch_k(c, XFH_K_EG_PLAN, -1, k_eg_plan_scan, dim3(1), dim3(64), 0, a);
    launch_k(c, XFH_K_EG_PLAN, -1, k_eg_plan_fill, dim3(a.nV), dim3(64), 0, a);
    return hipGetLastError();
}
hipError_t launch_eg_build(xfh_ctx* c, const EgArgs& a) {
    const int T = XFH_EG_THREADS;
    launch_k(c, XFH_K_EG_LINEARIZE, -1, k_eg_sims<true>, dim3((15 * a.nV + T - 1) / T), dim3(T), 0, a);
    launch_k(c, XFH_K_EG_LINEARIZE, -1, k_eg_edges<true>, dim3((a.nE + T - 1) / T), dim3(T), 0, a);
    launch_k(c, XFH_K_EG_LINEARIZE, -1, k_eg_vertices<true>, dim3(a.nV), dim3(T), 0, a);
    launch_k(c, XFH_K_EG_LINEARIZE, -1, k_eg_begin, dim3(1), dim3(T), 0, a);
    return hipGetLastError();
}
hipError_t launch_eg_trial(xfh_ctx* c, const EgArgs& a) {
    const int T = XFH_EG_THREADS, n = 7 * a.n_free, items = a.nE > a.n_free ? a.nE : a.n_free;
    const EgWs w = EG_WS(a);
    if (hipError_t e = hipMemsetAsync(w.S, 0, (size_t)n * n * sizeof(double), c->stream); e != hipSuccess) return e;
    launch_k(c, XFH_K_EG_FILL, -1, k_eg_fill, dim3((items + T - 1) / T), dim3(T), 0, a);
    eg_launch_solve(c, EgSolve{w.S, w.b, w.x, &w.ctl->solved, n});
    launch_k(c, XFH_K_EG_EVALUATE, -1, k_eg_update, dim3((a.nV + T - 1) / T), dim3(T), 0, a);
    launch_k(c, XFH_K_EG_EVALUATE, -1, k_eg_sims<false>, dim3((a.nV + T - 1) / T), dim3(T), 0, a);
    launch_k(c, XFH_K_EG_EVALUATE, -1, k_eg_edges<false>, dim3((a.nE + T - 1) / T), dim3(T), 0, a);
    launch_k(c, XFH_K_EG_EVALUATE, -1, k_eg_vertices<false>, dim3(a.nV), dim3(T), 0, a);
    launch_k(c, XFH_K_EG_EVALUATE, -1, k_eg_decide, dim3(1), dim3(T), 0, a);
    return hipGetLastError();
}
hipError_t launch_eg_finish(xfh_ctx* c, const EgArgs& a) {
    const int T = XFH_EG_THREADS;
    const int items = a.nE > a.nP ? (a.nE > a.nV ? a.nE : a.nV) : (a.nP > a.nV ? a.nP : a.nV);
    launch_k(c, XFH_K_EG_FINISH, -1, k_eg_finish, dim3((items + T - 1) / T), dim3(T), 0, a);
    launch_k(c, XFH_K_EG_FINISH, -1, k_eg_header, dim3(1), dim3(64), 0, a);
    return hipGetLastError();
}
// xfh_debug_eg_solve: the factorisation and the substitutions alone on a caller's system
hipError_t launch_eg_solve_alone(xfh_ctx* c, double* S, const double* b, double* x, int* ok, int n) {
    eg_launch_solve(c, EgSolve{S, b, x, ok, n});
    return hipGetLastError();
}
