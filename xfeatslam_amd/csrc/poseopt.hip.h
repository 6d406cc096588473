// poseopt.hip.h -- k_pose_optimize: Optimizer::PoseOptimization (src/Optimizer.cc:814-1114, conventional camera) for B frames in ONE launch, one
// workgroup of 256 lanes per problem (included by kernels_match.hip).  The contract is in include/xfeat_hip.h; the arithmetic is poseopt_math.h.
//
// Lane l owns the keypoints l, l + 256, ...  For nt <= 4096 they are EPT slots, a template parameter (4 or 16), so that the slot loop unrolls and an
// edge's world point, observation, state and the chi2 its last computeActiveErrors left stay in registers through all four rounds.  For larger nt
// (EPT = 0) that state does not fit the register file: the state word and the chi2 live in the caller's workspace and the point and the observation
// are read again in every pass.  No instance uses scratch.  The workgroup runs the state machine of geom_common.h (PoseLM of poseopt_math.h): lane 0 holds it in LDS and names
// the next pass (BUILD / TRIAL / CLASSIFY) and its pose, every lane reads both after a barrier, runs the pass over its slots and adds its shares of
// H, b and the robust chi2 in slot order.  The fold is fixed: the xor butterfly 32, 16, .. 1 inside a wave (a + b is commutative, so all lanes hold
// the same bits), then waves 0 .. 3 in order on lane 0.  Nothing depends on timing, so two runs give identical bytes.  At most
// XFH_POSE_MAX_PASSES passes, whatever the data.
#pragma once
#include "poseopt_math.h"
#include "search_common.hip.h"

#define XFH_POSE_THREADS 256
#define XFH_POSE_MAX_PASSES (XFH_POSE_ROUNDS * (XFH_POSE_ITERATIONS * (1 + GEO_LM_MAX_TRIALS) + 1))
enum { POSE_EDGE = 1, POSE_STEREO = 2, POSE_OUTLIER = 4 };

// keypoint k of problem pb: has it an edge, and of which kind; the point and the observation when it has
__device__ __forceinline__ int pose_slot_load(const PoseArgs& a, int pb, int k, float* X, float* ob) {
    const size_t kg = (size_t)pb * a.nt + k;
    const int q = a.assigned[kg];
    if (q < 0 || q >= a.nq) return 0;
    const float ur = a.uright ? a.uright[kg] : -1.0f;
    const float* p = a.points + ((size_t)pb * a.nq + q) * 3;
    X[0] = p[0]; X[1] = p[1]; X[2] = p[2];
    ob[0] = a.xy_un[kg * 2]; ob[1] = a.xy_un[kg * 2 + 1]; ob[2] = ur;
    return POSE_EDGE | (ur < 0.0f ? 0 : POSE_STEREO);                      // `if (pFrame->mvuRight[i] < 0)` mono, else stereo
}

// one edge in one pass: st = its state word, last = the chi2 of _error as the last computeActiveErrors left it
__device__ __forceinline__ void pose_slot_pass(int act, const PosePose& P, bool robust, const PoseArgs& a, size_t kg, int& st, double& last, const float* X,
                                               const float* ob, double (&acc)[XFH_POSE_NSUM], int& bad) {
    const bool stereo = (st & POSE_STEREO) != 0, out = (st & POSE_OUTLIER) != 0;
    if (act != GEO_LM_CLASSIFY && out) return;                             // level 1: not in _activeEdges
    const double Xd[3] = {(double)X[0], (double)X[1], (double)X[2]}, od[3] = {(double)ob[0], (double)ob[1], (double)ob[2]};
    double pc[3], e[3];
    if (act == GEO_LM_CLASSIFY) {
        // an outlier's error is computed afresh at the round's estimate (:1021-1024); an inlier's is what computeActiveErrors left
        const double c = out ? pose_edge_error(P, a.cam, Xd, od, stereo, a.w, pc, e) : last;
        const float cf = (float)c;
        const bool o = cf > (stereo ? XFH_POSE_CHI2_STEREO : XFH_POSE_CHI2_MONO);
        st = (st & ~POSE_OUTLIER) | (o ? POSE_OUTLIER : 0);
        bad += o ? 1 : 0;
        a.outlier[kg] = o ? 1 : 0; a.chi2[kg] = cf;
        return;
    }
    const double c = pose_edge_error(P, a.cam, Xd, od, stereo, a.w, pc, e);
    last = c;
    double r0 = c, r1 = 1.0;
    if (robust) pose_huber(c, pose_delta(stereo), &r0, &r1);
    acc[27] += r0;
    if (act == GEO_LM_BUILD) {
        double J[18];
        pose_edge_jacobian(a.cam, pc, stereo, J);
        pose_accumulate(acc, J, e, stereo, a.w, r1);
    }
}

template <int EPT>
__global__ __launch_bounds__(XFH_POSE_THREADS)
void k_pose_optimize(PoseArgs a) {
    __shared__ PoseLM S;
    __shared__ double s_red[XFH_POSE_THREADS / 64][XFH_POSE_NSUM];
    __shared__ int s_cnt[XFH_POSE_THREADS / 64], s_act;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, pb = blockIdx.x;
    const size_t k0 = (size_t)pb * a.nt;
    constexpr int NS = EPT > 0 ? EPT : 1;
    float X[NS][3], ob[NS][3];
    double last[NS];
    int st[NS];
    double* ws_last = (double*)(a.ws + (size_t)pb * a.ws_stride);          // (EPT == 0 only)
    int* ws_st = (int*)(a.ws + (size_t)pb * a.ws_stride + pose_ws_last_bytes(a.nt));
    int mine = 0;
    if constexpr (EPT > 0) {
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            const int k = tid + j * XFH_POSE_THREADS;
            st[j] = 0; last[j] = 0.0;
            X[j][0] = X[j][1] = X[j][2] = ob[j][0] = ob[j][1] = ob[j][2] = 0.0f;
            if (k < a.nt) {
                st[j] = pose_slot_load(a, pb, k, X[j], ob[j]);
                mine += st[j] ? 1 : 0;
                a.outlier[k0 + k] = 0; a.chi2[k0 + k] = 0.0f;
            }
        }
    } else {
        for (int k = tid; k < a.nt; k += XFH_POSE_THREADS) {
            const int s = pose_slot_load(a, pb, k, X[0], ob[0]);
            ws_st[k] = s; ws_last[k] = 0.0;
            mine += s ? 1 : 0;
            a.outlier[k0 + k] = 0; a.chi2[k0 + k] = 0.0f;
        }
    }
    mine = wave_sum_i32(mine);
    if (lane == 0) s_cnt[wave] = mine;
    __syncthreads();
    const int n_initial = ((s_cnt[0] + s_cnt[1]) + s_cnt[2]) + s_cnt[3];
    if (n_initial < 3) {                                                   // `if (nInitialCorrespondences < 3) return 0`: the pose is not touched
        if (tid < 12) a.Tcw_out[(size_t)pb * 12 + tid] = a.Tcw[(size_t)pb * 12 + tid];
        if (tid < 8) a.header[(size_t)pb * 8 + tid] = tid == XFH_POSE_H_INITIAL ? n_initial : 0;
        if (tid == 0) a.final_chi2[pb] = 0.0;
        return;
    }
    if (tid == 0) {
        PosePose in;
        pose_from_tcw(a.Tcw + (size_t)pb * 12, &in);
        s_act = pose_lm_begin(S, in, n_initial);
    }

    for (int pass = 0; pass <= XFH_POSE_MAX_PASSES; ++pass) {
        __syncthreads();                                                   // lane 0's action and pose are in LDS; s_red and s_cnt are free again
        const int act = s_act;
        if (act == GEO_LM_DONE) break;
        const PosePose P = S.est;
        const bool robust = pose_lm_robust(S);
        double acc[XFH_POSE_NSUM];
#pragma unroll
        for (int n = 0; n < XFH_POSE_NSUM; ++n) acc[n] = 0.0;
        int bad = 0;
        if constexpr (EPT > 0) {
#pragma unroll
            for (int j = 0; j < EPT; ++j)
                if (st[j] & POSE_EDGE) pose_slot_pass(act, P, robust, a, k0 + tid + j * XFH_POSE_THREADS, st[j], last[j], X[j], ob[j], acc, bad);
        } else {
            for (int k = tid; k < a.nt; k += XFH_POSE_THREADS) {           // each lane reads and writes its own slots only
                int s = ws_st[k];
                if (!(s & POSE_EDGE)) continue;
                double l = ws_last[k];
                pose_slot_load(a, pb, k, X[0], ob[0]);
                pose_slot_pass(act, P, robust, a, k0 + k, s, l, X[0], ob[0], acc, bad);
                ws_st[k] = s; ws_last[k] = l;
            }
        }
        if (act == GEO_LM_BUILD) {
#pragma unroll
            for (int n = 0; n < XFH_POSE_NSUM; ++n) { const double s = wave_sum_f64(acc[n]); if (lane == 0) s_red[wave][n] = s; }
        } else if (act == GEO_LM_TRIAL) {
            const double s = wave_sum_f64(acc[27]);
            if (lane == 0) s_red[wave][27] = s;
        } else {
            bad = wave_sum_i32(bad);
            if (lane == 0) s_cnt[wave] = bad;
        }
        __syncthreads();
        if (tid == 0) {
            if (act == GEO_LM_BUILD) {
                double sums[XFH_POSE_NSUM];
#pragma unroll
                for (int n = 0; n < XFH_POSE_NSUM; ++n) sums[n] = ((s_red[0][n] + s_red[1][n]) + s_red[2][n]) + s_red[3][n];
                s_act = geo_lm_after_build(S, sums);
            } else if (act == GEO_LM_TRIAL) {
                s_act = geo_lm_after_trial(S, ((s_red[0][27] + s_red[1][27]) + s_red[2][27]) + s_red[3][27]);
            } else {
                s_act = pose_lm_after_classify(S, ((s_cnt[0] + s_cnt[1]) + s_cnt[2]) + s_cnt[3]);
            }
        }
    }
    if (tid == 0) {
        pose_to_tcw(S.est, a.Tcw_out + (size_t)pb * 12);
#pragma unroll
        for (int n = 0; n < 8; ++n) a.header[(size_t)pb * 8 + n] = S.hdr[n];
        a.final_chi2[pb] = S.currentChi;
    }
}

hipError_t launch_pose_optimize(xfh_ctx* c, const PoseArgs& a, int B) {
    if (a.nt <= 4 * XFH_POSE_THREADS) launch_k(c, XFH_K_POSE_OPTIMIZE, -1, k_pose_optimize<4>, dim3(B), dim3(XFH_POSE_THREADS), 0, a);
    else if (a.nt <= 16 * XFH_POSE_THREADS) launch_k(c, XFH_K_POSE_OPTIMIZE, -1, k_pose_optimize<16>, dim3(B), dim3(XFH_POSE_THREADS), 0, a);
    else launch_k(c, XFH_K_POSE_OPTIMIZE, -1, k_pose_optimize<0>, dim3(B), dim3(XFH_POSE_THREADS), 0, a);
    return hipGetLastError();
}
