// twoview.hip.h -- TwoViewReconstruction::Reconstruct (src/TwoViewReconstruction.cc) for B problems per call (included by kernels_match.hip).
// The contract is in include/xfeat_hip.h; the arithmetic is twoview_math.h, the host's own lines.  Six launches, whatever the data:
//
//   k_twoview_prepare  one workgroup per problem: the compact match list in idx1 order (ordered scan: ballot + popcount inside a wave, the four
//                      wave totals in order, never an atomic counter), N, and Normalize of both frames (two passes each, the rule's 256-lane sums).
//   k_twoview_fit      one lane per (problem, model, iteration): the minimal set from the raw draws, the 16 x 9 or 8 x 9 fp64 Jacobi and, for F, the
//                      rank-2 projection, composed with the normalisations.  U and V (225 doubles) of a lane live in LDS, element k of lane l at
//                      [k][l]: runtime column indices without scratch, and the 32 lanes of a workgroup hit 32 different banks.
//   k_twoview_score    one workgroup per (problem, model, iteration): the score of the hypothesis over the N matches in the rule's 256-lane sum.
//                      Only the score is written: no iterations x N mask reaches HBM.
//   k_twoview_select   one workgroup per problem: the two argmaxes (one lane each), the inlier flags of the two winners recomputed, SH / SF / RH,
//                      the model and its motion hypotheses (one lane; its 3 x 3 Jacobi in LDS).
//   k_twoview_check_rt one workgroup per (problem, motion hypothesis): CheckRT of every inlier pair, nGood, and the cosine at sorted index
//                      min(50, nGood - 1) by a radix select over the float keys (32 counting passes; only the value matters, so ties are harmless).
//   k_twoview_final    one workgroup per problem: the decision (tv_decide, the same integers on every lane) and the outputs.
// No global atomics, no waiting between workgroups; every float sum has the order of geo_tree_fold.  Two runs give identical bytes.
#pragma once
#include "twoview_math.h"
#include "block_common.hip.h"

#define XFH_TV_THREADS GEO_LANES
#define XFH_TV_FIT_LANES 32

struct TvWs {
    int *cm1, *cm2, *sel, *ngood;
    float *nrm, *hyp, *score, *motion, *cosk, *cosv, *p3d;
    unsigned char* verdict;
};
__device__ __forceinline__ TvWs tv_ws(const TvArgs& a, int b) {
    const TvLayout L = tv_layout(a.n1, a.iters);
    unsigned char* p = a.ws + (size_t)b * L.per_problem;
    TvWs w;
    w.cm1 = (int*)(p + L.cm1); w.cm2 = (int*)(p + L.cm2); w.nrm = (float*)(p + L.nrm); w.sel = (int*)(p + L.sel); w.hyp = (float*)(p + L.hyp);
    w.score = (float*)(p + L.score); w.motion = (float*)(p + L.motion); w.ngood = (int*)(p + L.ngood); w.cosk = (float*)(p + L.cosk);
    w.verdict = p + L.verdict; w.cosv = (float*)(p + L.cosv); w.p3d = (float*)(p + L.p3d);
    return w;
}
// one float sum of the rule: the fold of geo_tree_fold by 256 lanes, on every lane
__device__ __forceinline__ float tv_block_fold(float* s, float mine) {
    float out;
    block_tree_fold<float, 1>(s, &mine, &out);
    return out;
}

__global__ __launch_bounds__(XFH_TV_THREADS)
void k_twoview_prepare(TvArgs a) {
    __shared__ float s_f[GEO_LANES];
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x, b = blockIdx.x, n1 = a.n1, n2 = a.n2;
    const TvWs w = tv_ws(a, b);
    const int* m12 = a.match12 + (size_t)b * n1;
    int base = 0;
    for (int i0 = 0; i0 < n1; i0 += XFH_TV_THREADS) {
        const int i = i0 + tid;
        const int m = i < n1 ? m12[i] : -1;
        const bool ok = i < n1 && tv_match_ok(m, n2);
        __syncthreads();                                                   // s_cnt is free
        const int pos = block_compact_step(ok, s_cnt, base);
        if (ok) { w.cm1[pos] = i; w.cm2[pos] = m; }                        // pos < n1
    }
    if (tid == 0) w.sel[TV_S_N] = base;
    for (int f = 0; f < 2; ++f) {
        const int n = f ? n2 : n1;
        const float* xy = f ? a.xy2 + (size_t)b * n2 * 2 : a.xy1 + (size_t)b * n1 * 2;
        float mean[2], inv[2];
        for (int d = 0; d < 2; ++d) {
            float acc = 0.0f;
            for (int i = tid; i < n; i += GEO_LANES) acc = acc + xy[2 * (size_t)i + d];
            mean[d] = tv_mean(tv_block_fold(s_f, acc), n);
            acc = 0.0f;
            for (int i = tid; i < n; i += GEO_LANES) acc = acc + fabsf(xy[2 * (size_t)i + d] - mean[d]);
            inv[d] = tv_inv_dev(tv_block_fold(s_f, acc), n);
        }
        if (tid == 0) { w.nrm[4 * f] = mean[0]; w.nrm[4 * f + 1] = mean[1]; w.nrm[4 * f + 2] = inv[0]; w.nrm[4 * f + 3] = inv[1]; }
    }
}

__global__ __launch_bounds__(XFH_TV_FIT_LANES)
void k_twoview_fit(TvArgs a) {
    __shared__ double s_m[225 * XFH_TV_FIT_LANES];
    const int tid = threadIdx.x, it = blockIdx.x * XFH_TV_FIT_LANES + tid, model = blockIdx.y ? TV_MODEL_F : TV_MODEL_H, b = blockIdx.z;
    const TvWs w = tv_ws(a, b);
    const int N = w.sel[TV_S_N];
    if (it >= a.iters || N < 8) return;                                    // (no barrier below)
    int set[8];
    geo_set<TV_MIN_SET>(a.draws + (size_t)b * a.draws_stride + (size_t)it * 8, a.rand_max, N, set);
    float p1[16], p2[16];
    const float* xy1 = a.xy1 + (size_t)b * a.n1 * 2;
    const float* xy2 = a.xy2 + (size_t)b * a.n2 * 2;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int i1 = w.cm1[set[j]], i2 = w.cm2[set[j]];
        tv_normalized(w.nrm, xy1[2 * (size_t)i1], xy1[2 * (size_t)i1 + 1], p1 + 2 * j);
        tv_normalized(w.nrm + 4, xy2[2 * (size_t)i2], xy2[2 * (size_t)i2 + 1], p2 + 2 * j);
    }
    const GeoMat U{s_m + tid, XFH_TV_FIT_LANES}, V{s_m + 144 * XFH_TV_FIT_LANES + tid, XFH_TV_FIT_LANES};
    float M[9], out[18];
    if (model == TV_MODEL_H) { tv_fit_h(p1, p2, U, V, M); tv_compose_h(M, w.nrm, w.nrm + 4, out); }
    else { tv_fit_f(p1, p2, U, V, M); tv_compose_f(M, w.nrm, w.nrm + 4, out); }
    float* dst = w.hyp + ((size_t)(model - 1) * a.iters + it) * 18;
#pragma unroll
    for (int k = 0; k < 18; ++k) dst[k] = out[k];
}

__global__ __launch_bounds__(XFH_TV_THREADS)
void k_twoview_score(TvArgs a) {
    __shared__ float s_f[GEO_LANES];
    __shared__ float s_M[18];
    const int tid = threadIdx.x, it = blockIdx.x, model = blockIdx.y ? TV_MODEL_F : TV_MODEL_H, b = blockIdx.z;
    const TvWs w = tv_ws(a, b);
    const int N = w.sel[TV_S_N];
    if (N < 8) return;                                                     // (the whole workgroup)
    if (tid < 18) s_M[tid] = w.hyp[((size_t)(model - 1) * a.iters + it) * 18 + tid];
    __syncthreads();
    float M[18];
#pragma unroll
    for (int k = 0; k < 18; ++k) M[k] = s_M[k];
    const float* xy1 = a.xy1 + (size_t)b * a.n1 * 2;
    const float* xy2 = a.xy2 + (size_t)b * a.n2 * 2;
    const float inv_s2 = tv_inv_sigma2(a.sigma);
    float acc = 0.0f;
    for (int k = tid; k < N; k += GEO_LANES) {
        const int i1 = w.cm1[k], i2 = w.cm2[k];
        float chi[2]; int in;
        acc = acc + tv_score(model, M, inv_s2, xy1[2 * (size_t)i1], xy1[2 * (size_t)i1 + 1], xy2[2 * (size_t)i2], xy2[2 * (size_t)i2 + 1], chi, &in);
    }
    const float s = tv_block_fold(s_f, acc);
    if (tid == 0) w.score[(size_t)(model - 1) * a.iters + it] = s;
}

__global__ __launch_bounds__(XFH_TV_THREADS)
void k_twoview_select(TvArgs a) {
    __shared__ int s_win[2];
    __shared__ float s_best[2];
    __shared__ int s_cnt[4];
    __shared__ double s_m[18];
    const int tid = threadIdx.x, b = blockIdx.x, n1 = a.n1;
    const TvWs w = tv_ws(a, b);
    const int N = w.sel[TV_S_N];
    int* hdr = a.header + (size_t)b * TV_HEADER_INTS;
    if (N < 8) {                                                           // TOO_FEW: the header and nothing else
        if (tid < TV_HEADER_INTS) hdr[tid] = tid == TV_H_N ? N : (tid == TV_H_STATUS ? TV_TOO_FEW : (tid == TV_H_WIN_H || tid == TV_H_WIN_F || tid == TV_H_CHOSEN ? -1 : 0));
        return;
    }
    if (tid == 0 || tid == 64) {
        const int m = tid ? 1 : 0;
        float best;
        s_win[m] = tv_argmax(w.score + (size_t)m * a.iters, a.iters, &best);
        s_best[m] = best;
    }
    __syncthreads();
    const int winH = s_win[0], winF = s_win[1];
    const float SH = s_best[0], SF = s_best[1];
    float MH[18], MF[9];
#pragma unroll
    for (int k = 0; k < 18; ++k) MH[k] = winH >= 0 ? w.hyp[(size_t)winH * 18 + k] : 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) MF[k] = winF >= 0 ? w.hyp[((size_t)a.iters + winF) * 18 + k] : 0.0f;
    const float* xy1 = a.xy1 + (size_t)b * n1 * 2;
    const float* xy2 = a.xy2 + (size_t)b * a.n2 * 2;
    const int* m12 = a.match12 + (size_t)b * n1;
    const float inv_s2 = tv_inv_sigma2(a.sigma);
    int cH = 0, cF = 0;
    for (int i = tid; i < n1; i += XFH_TV_THREADS) {
        const int m = m12[i];
        int inH = 0, inF = 0;
        if (tv_match_ok(m, a.n2)) {
            float chi[2];
            const float u1 = xy1[2 * (size_t)i], v1 = xy1[2 * (size_t)i + 1], u2 = xy2[2 * (size_t)m], v2 = xy2[2 * (size_t)m + 1];
            if (winH >= 0) tv_score_h(MH, inv_s2, u1, v1, u2, v2, chi, &inH);
            if (winF >= 0) tv_score_f(MF, inv_s2, u1, v1, u2, v2, chi, &inF);
        }
        a.inl_h[(size_t)b * n1 + i] = (unsigned char)inH; a.inl_f[(size_t)b * n1 + i] = (unsigned char)inF;
        cH += inH; cF += inF;
    }
    cH = block_sum_i32(s_cnt, cH);
    cF = block_sum_i32(s_cnt, cF);
    if (tid != 0) return;
    float* fo = a.fout + (size_t)b * TV_FLOATS;
    for (int k = 0; k < TV_FLOATS; ++k) fo[k] = 0.0f;
    fo[TV_F_SH] = SH; fo[TV_F_SF] = SF;
    for (int k = 0; k < 9; ++k) { fo[TV_F_H21 + k] = MH[k]; fo[TV_F_F21 + k] = MF[k]; }
    int model = TV_MODEL_NONE, nhyp = 0, hdeg = 0;
    if (SH + SF != 0.0f) {
        const float RH = SH / (SH + SF);
        fo[TV_F_RH] = RH;
        model = (double)RH > 0.50 ? TV_MODEL_H : TV_MODEL_F;
        const GeoMat U{s_m, 1}, V{s_m + 9, 1};
        if (model == TV_MODEL_H) { hdeg = !tv_motions_h(MH, a.cam, U, V, w.motion); nhyp = hdeg ? 0 : 8; }
        else { tv_motions_f(MF, a.cam, U, V, w.motion); nhyp = 4; }
    }
    w.sel[TV_S_WIN_H] = winH; w.sel[TV_S_WIN_F] = winF; w.sel[TV_S_MODEL] = model; w.sel[TV_S_NINL] = model == TV_MODEL_H ? cH : cF;
    w.sel[TV_S_HDEG] = hdeg; w.sel[TV_S_NHYP] = nhyp;
    hdr[TV_H_INL_H] = cH; hdr[TV_H_INL_F] = cF;
}

__global__ __launch_bounds__(XFH_TV_THREADS)
void k_twoview_check_rt(TvArgs a) {
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x, h = blockIdx.x, b = blockIdx.y, n1 = a.n1;
    const TvWs w = tv_ws(a, b);
    if (w.sel[TV_S_N] < 8) return;
    if (h >= w.sel[TV_S_NHYP]) {                                           // (uniform)
        if (tid == 0) { w.ngood[h] = 0; w.cosk[h] = 1.0f; }
        return;
    }
    float Rt[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) Rt[k] = w.motion[h * 12 + k];
    const unsigned char* inl = (w.sel[TV_S_MODEL] == TV_MODEL_H ? a.inl_h : a.inl_f) + (size_t)b * n1;
    const float* xy1 = a.xy1 + (size_t)b * n1 * 2;
    const float* xy2 = a.xy2 + (size_t)b * a.n2 * 2;
    const int* m12 = a.match12 + (size_t)b * n1;
    const float th2 = tv_th2(a.sigma);
    unsigned char* verdict = w.verdict + (size_t)h * n1;
    float* cosv = w.cosv + (size_t)h * n1;
    float* p3d = w.p3d + (size_t)h * n1 * 3;
    int cnt = 0;
    for (int i = tid; i < n1; i += XFH_TV_THREADS) {
        int v = 0; float c = 0.0f, p[3] = {0.0f, 0.0f, 0.0f};
        if (inl[i]) {                                                      // set only where match12[i] is inside 0 .. n2 - 1
            const int m = m12[i];
            v = tv_check_rt_pair(a.cam, Rt, th2, xy1[2 * (size_t)i], xy1[2 * (size_t)i + 1], xy2[2 * (size_t)m], xy2[2 * (size_t)m + 1], &c, p);
        }
        verdict[i] = (unsigned char)v; cosv[i] = c;
        p3d[3 * (size_t)i] = p[0]; p3d[3 * (size_t)i + 1] = p[1]; p3d[3 * (size_t)i + 2] = p[2];
        cnt += v != 0;
    }
    const int nGood = block_sum_i32(s_cnt, cnt);                        // (its barriers also publish verdict / cosv to the workgroup)
    float ck = 1.0f;
    if (nGood > 0) {
        int k = nGood - 1 < 50 ? nGood - 1 : 50;
        uint32_t prefix = 0, mask = 0;
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t bb = 1u << bit;
            int c0 = 0;
            for (int i = tid; i < n1; i += XFH_TV_THREADS) {
                const uint32_t key = tv_float_key(cosv[i]);
                c0 += verdict[i] != 0 && (key & mask) == prefix && !(key & bb);
            }
            c0 = block_sum_i32(s_cnt, c0);
            if (k >= c0) { k -= c0; prefix |= bb; }
            mask |= bb;
        }
        ck = tv_key_float(prefix);
    }
    if (tid == 0) { w.ngood[h] = nGood; w.cosk[h] = ck; }
}

__global__ __launch_bounds__(XFH_TV_THREADS)
void k_twoview_final(TvArgs a) {
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x, b = blockIdx.x, n1 = a.n1;
    const TvWs w = tv_ws(a, b);
    const int N = w.sel[TV_S_N];
    if (N < 8) return;
    const int model = w.sel[TV_S_MODEL];
    int nGood[8]; float cosk[8];
#pragma unroll
    for (int h = 0; h < 8; ++h) { nGood[h] = w.ngood[h]; cosk[h] = w.cosk[h]; }
    int chosen = -1;
    const int status = model == TV_MODEL_NONE ? TV_BOTH_ZERO
                                              : tv_decide(model, w.sel[TV_S_HDEG] != 0, nGood, cosk, w.sel[TV_S_NINL], a.min_parallax_cos, a.min_tri, &chosen);
    const int* m12 = a.match12 + (size_t)b * n1;
    int ntri = 0;
    for (int i = tid; i < n1; i += XFH_TV_THREADS) {
        const size_t kg = (size_t)b * n1 + i;
        const int m = m12[i];
        int v = 0; float p[3] = {0.0f, 0.0f, 0.0f};
        if (chosen >= 0) {
            v = w.verdict[(size_t)chosen * n1 + i];
            if (v) { const float* q = w.p3d + ((size_t)chosen * n1 + i) * 3; p[0] = q[0]; p[1] = q[1]; p[2] = q[2]; }
        }
        a.tri[kg] = (unsigned char)(v == 2);
        a.p3d[3 * kg] = p[0]; a.p3d[3 * kg + 1] = p[1]; a.p3d[3 * kg + 2] = p[2];
        a.matches_out[kg] = chosen >= 0 && tv_match_ok(m, a.n2) && v != 2 ? -1 : m;
        ntri += v == 2;
    }
    ntri = block_sum_i32(s_cnt, ntri);
    if (tid != 0) return;
    int* hdr = a.header + (size_t)b * TV_HEADER_INTS;
    float* fo = a.fout + (size_t)b * TV_FLOATS;
    hdr[TV_H_N] = N; hdr[TV_H_STATUS] = status; hdr[TV_H_MODEL] = model; hdr[TV_H_WIN_H] = w.sel[TV_S_WIN_H]; hdr[TV_H_WIN_F] = w.sel[TV_S_WIN_F];
    for (int h = 0; h < 8; ++h) { hdr[TV_H_NGOOD + h] = nGood[h]; fo[TV_F_COS + h] = cosk[h]; }
    hdr[TV_H_CHOSEN] = chosen; hdr[TV_H_NTRI] = ntri; hdr[TV_H_NHYP] = w.sel[TV_S_NHYP]; hdr[TV_H_NMATCHES] = chosen >= 0 ? ntri : N;
    for (int k = TV_H_NMATCHES + 1; k < TV_HEADER_INTS; ++k) hdr[k] = 0;
    if (chosen >= 0) for (int k = 0; k < 12; ++k) fo[TV_F_T21 + k] = w.motion[chosen * 12 + k];
}

hipError_t launch_two_view(xfh_ctx* c, const TvArgs& a) {
    const int fit_blocks = (a.iters + XFH_TV_FIT_LANES - 1) / XFH_TV_FIT_LANES;
    launch_k(c, XFH_K_TWOVIEW_PREPARE, -1, k_twoview_prepare, dim3(a.B), dim3(XFH_TV_THREADS), 0, a);
    launch_k(c, XFH_K_TWOVIEW_FIT, -1, k_twoview_fit, dim3(fit_blocks, 2, a.B), dim3(XFH_TV_FIT_LANES), 0, a);
    launch_k(c, XFH_K_TWOVIEW_SCORE, -1, k_twoview_score, dim3(a.iters, 2, a.B), dim3(XFH_TV_THREADS), 0, a);
    launch_k(c, XFH_K_TWOVIEW_SELECT, -1, k_twoview_select, dim3(a.B), dim3(XFH_TV_THREADS), 0, a);
    launch_k(c, XFH_K_TWOVIEW_CHECK_RT, -1, k_twoview_check_rt, dim3(8, a.B), dim3(XFH_TV_THREADS), 0, a);
    launch_k(c, XFH_K_TWOVIEW_FINAL, -1, k_twoview_final, dim3(a.B), dim3(XFH_TV_THREADS), 0, a);
    return hipGetLastError();
}
