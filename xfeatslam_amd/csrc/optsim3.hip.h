// optsim3.hip.h -- k_sim3_optimize: Optimizer::OptimizeSim3 (src/Optimizer.cc:2100-2381) for B problems in ONE launch, one workgroup of 256 lanes per
// problem (included by kernels_match.hip).  The contract is in include/xfeat_hip.h; the arithmetic is optsim3_math.h.
//
// Lane l owns the keypoints l, l + 256, ...  For n1 <= 1024 they are EPT = 4 slots, a template parameter, so that the slot loop unrolls and a pair's
// two camera-frame points, its two observations, its state word and the two chi2 its last computeActiveErrors left stay in registers through both
// rounds.  For larger n1 (EPT = 0) the state word and the two chi2 live in the caller's workspace and the points and observations are computed
// again in every pass (float arithmetic on the same inputs: the same bits).  No instance uses scratch.  The workgroup runs the state machine of
// geom_common.h (Os3LM of optsim3_math.h): lane 0 holds it in LDS and names the next pass (BUILD / TRIAL / CLASSIFY); lanes 0 .. 14 then write the similarities of the pass
// into LDS -- the estimate's inverse, and for BUILD the 14 perturbed similarities of the numeric Jacobian with their inverses, once per
// linearisation -- and every lane runs the pass over its slots, adding its shares of H, b and the robust chi2 in slot order, e12 before e21.  The
// fold is k_pose_optimize's: the xor butterfly 32, 16, .. 1 inside a wave, then waves 0 .. 3 in order on lane 0.  Nothing depends on timing, so two
// runs give identical bytes.  At most XFH_OS3_MAX_PASSES passes, whatever the data.
#pragma once
#include "optsim3_math.h"
#include "search_common.hip.h"

template <int EPT>
__global__ __launch_bounds__(XFH_OS3_THREADS)
void k_sim3_optimize(Os3Args a) {
    __shared__ Os3LM S;
    __shared__ Os3Sims sims;
    __shared__ double s_red[XFH_OS3_THREADS / 64][XFH_OS3_NSUM];
    __shared__ int s_cnt[XFH_OS3_THREADS / 64], s_act;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, pb = blockIdx.x;
    constexpr int NS = EPT > 0 ? EPT : 1;
    Os3Pair P[NS];
    double l12[NS], l21[NS];
    int st[NS];
    double* ws_last = (double*)(a.ws + (size_t)pb * a.ws_stride);          // (EPT == 0 only)
    int* ws_st = (int*)(a.ws + (size_t)pb * a.ws_stride + os3_ws_last_bytes(a.n1));
    int mine = 0;                                                          // pairs | pairs not in KF2 << 16
    if constexpr (EPT > 0) {
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            const int k = tid + j * XFH_OS3_THREADS;
            st[j] = 0; l12[j] = 0.0; l21[j] = 0.0;
            P[j] = Os3Pair{};
            if (k < a.n1) st[j] = os3_pair_load(a, pb, k, &P[j]);
            mine += st[j] ? ((st[j] & OS3_IN_KF2) ? 1 : 65537) : 0;
        }
    } else {
        for (int k = tid; k < a.n1; k += XFH_OS3_THREADS) {
            const int s = os3_pair_load(a, pb, k, &P[0]);
            ws_st[k] = s; ws_last[2 * k] = 0.0; ws_last[2 * k + 1] = 0.0;
            mine += s ? ((s & OS3_IN_KF2) ? 1 : 65537) : 0;
        }
    }
    mine = wave_sum_i32(mine);
    if (lane == 0) s_cnt[wave] = mine;
    __syncthreads();
    if (tid == 0) {
        const int n = ((s_cnt[0] + s_cnt[1]) + s_cnt[2]) + s_cnt[3];
        Os3Sim in;
        os3_from_floats(a.S12 + (size_t)pb * a.S12_stride, &in);
        s_act = os3_lm_begin(S, in, a.fix_scale, n & 0xFFFF, n >> 16);
    }

    for (int pass = 0; pass <= XFH_OS3_MAX_PASSES; ++pass) {
        __syncthreads();                                                   // lane 0's action and estimate are in LDS; s_red and s_cnt are free again
        const int act = s_act;
        if (act == GEO_LM_DONE) break;
        if (tid < 15 && (tid == 14 || act == GEO_LM_BUILD)) {
            const Os3Sim E = S.est;
            os3_sims_piece(E, a.fix_scale, tid, &sims);
        }
        const bool robust = os3_lm_robust(S), final = os3_lm_final(S);
        __syncthreads();
        double acc[XFH_OS3_NSUM];
#pragma unroll
        for (int n = 0; n < XFH_OS3_NSUM; ++n) acc[n] = 0.0;
        int bad = 0;
        if constexpr (EPT > 0) {
#pragma unroll
            for (int j = 0; j < EPT; ++j)
                if (st[j] & OS3_EDGE) os3_pair_pass(act, robust, final, sims, a, P[j], st[j], l12[j], l21[j], acc, bad);
        } else {
            for (int k = tid; k < a.n1; k += XFH_OS3_THREADS) {            // each lane reads and writes its own slots only
                int s = ws_st[k];
                if (!(s & OS3_EDGE)) continue;
                double c12 = ws_last[2 * k], c21 = ws_last[2 * k + 1];
                os3_pair_load(a, pb, k, &P[0]);
                os3_pair_pass(act, robust, final, sims, a, P[0], s, c12, c21, acc, bad);
                ws_st[k] = s; ws_last[2 * k] = c12; ws_last[2 * k + 1] = c21;
            }
        }
        if (act == GEO_LM_BUILD) {
#pragma unroll
            for (int n = 0; n < XFH_OS3_NSUM; ++n) { const double s = wave_sum_f64(acc[n]); if (lane == 0) s_red[wave][n] = s; }
        } else if (act == GEO_LM_TRIAL) {
            const double s = wave_sum_f64(acc[35]);
            if (lane == 0) s_red[wave][35] = s;
        } else {
            bad = wave_sum_i32(bad);
            if (lane == 0) s_cnt[wave] = bad;
        }
        __syncthreads();
        if (tid == 0) {
            if (act == GEO_LM_BUILD) {
                double sums[XFH_OS3_NSUM];
#pragma unroll
                for (int n = 0; n < XFH_OS3_NSUM; ++n) sums[n] = ((s_red[0][n] + s_red[1][n]) + s_red[2][n]) + s_red[3][n];
                s_act = geo_lm_after_build(S, sums);
            } else if (act == GEO_LM_TRIAL) {
                s_act = geo_lm_after_trial(S, ((s_red[0][35] + s_red[1][35]) + s_red[2][35]) + s_red[3][35]);
            } else {
                s_act = os3_lm_after_classify(S, ((s_cnt[0] + s_cnt[1]) + s_cnt[2]) + s_cnt[3]);
            }
        }
    }
    // every lane's own keypoints: assigned is read before assigned_out is written, so the two may be one array
    if constexpr (EPT > 0) {
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            const int k = tid + j * XFH_OS3_THREADS;
            if (k < a.n1) os3_pair_store(a, pb, k, st[j], l12[j], l21[j]);
        }
    } else {
        for (int k = tid; k < a.n1; k += XFH_OS3_THREADS) os3_pair_store(a, pb, k, ws_st[k], ws_last[2 * k], ws_last[2 * k + 1]);
    }
    if (tid == 0) os3_finish(a, pb, S);
}

hipError_t launch_sim3_optimize(xfh_ctx* c, const Os3Args& a, int B) {
    if (a.n1 <= 4 * XFH_OS3_THREADS) launch_k(c, XFH_K_SIM3_OPTIMIZE, -1, k_sim3_optimize<4>, dim3(B), dim3(XFH_OS3_THREADS), 0, a);
    else launch_k(c, XFH_K_SIM3_OPTIMIZE, -1, k_sim3_optimize<0>, dim3(B), dim3(XFH_OS3_THREADS), 0, a);
    return hipGetLastError();
}
