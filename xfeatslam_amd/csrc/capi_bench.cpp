// capi_bench.cpp -- implementation of include/xfeat_hip_bench.h: the measurement and debugging entry points (nothing a SLAM consumer calls),
// and the kernel-timing hook of launch_k (ctx.h).
#include "capi_internal.h"
#include "mnn_seg_plan.h"
#include <stdlib.h>

// `call` queued `warmup` times, then `iters` times between two events on the ctx stream -> microseconds per call
template <typename F>
static int time_calls(xfh_ctx* c, int warmup, int iters, double* us_per_call, F call) {
    hipEvent_t e0, e1;
    HIPCK(c, hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { hipEventDestroy(e0); return XFH_ERR_HIP; }
    hipError_t e = hipSuccess;
    for (int i = 0; i < warmup && e == hipSuccess; ++i) e = call();
    if (e == hipSuccess) e = hipEventRecord(e0, c->stream);
    for (int i = 0; i < iters && e == hipSuccess; ++i) e = call();
    if (e == hipSuccess) e = hipEventRecord(e1, c->stream);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    hipEventDestroy(e0); hipEventDestroy(e1);
    *us_per_call = (double)ms * 1e3 / iters;
    HIPCK(c, e);
    return XFH_OK;
}

extern "C" {

int xfh_bench_mnn_gemm(xfh_ctx* c, const void* image1, int n1, const void* image2, int n2, int iters, double* us_per_launch) {
    if (!c || !image1 || !image2 || n1 < 1 || n2 < 1 || iters < 1 || !us_per_launch) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, bench_mnn_gemm(c, (const float*)image1, n1, (const float*)image2, n2, iters, us_per_launch));
    return XFH_OK;
}
static int bench_match(xfh_ctx* c, bool prepared, const void* a1, int n1, const void* a2, int n2, float min_cossim,
                       int* idx1, int* idx2, float* dist, int* n_matches, int iters, double* us_per_call) {
    if (!c || !a1 || !a2 || n1 < 1 || n2 < 1 || iters < 1 || !us_per_call || !idx1 || !idx2 || !dist || !n_matches) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    return time_calls(c, 200, iters, us_per_call, [&]() {                   // the clocks settle over a few hundred of these ~30 us calls
        return prepared ? launch_mnn_prepared(c, (const float*)a1, n1, (const float*)a2, n2, min_cossim, idx1, idx2, dist, n_matches)
                        : launch_mnn(c, (const float*)a1, n1, (const float*)a2, n2, min_cossim, idx1, idx2, dist, n_matches);
    });
}
int xfh_bench_match_prepared(xfh_ctx* c, const void* image1, int n1, const void* image2, int n2, float min_cossim,
                             int* idx1, int* idx2, float* dist, int* n_matches, int iters, double* us_per_call) {
    return bench_match(c, true, image1, n1, image2, n2, min_cossim, idx1, idx2, dist, n_matches, iters, us_per_call);
}
int xfh_bench_match_raw(xfh_ctx* c, const float* d1, int n1, const float* d2, int n2, float min_cossim,
                        int* idx1, int* idx2, float* dist, int* n_matches, int iters, double* us_per_call) {
    return bench_match(c, false, d1, n1, d2, n2, min_cossim, idx1, idx2, dist, n_matches, iters, us_per_call);
}
int xfh_debug_match_plan(int n_pairs, const int* n1, const int* n2, int num_cu, int* tiles, int* workgroups, int* tile0, int* planes_max, int* wg_lo, unsigned long long* keys) {
    if (n_pairs < 1 || n_pairs > MNN_MAX_JOBS || !n1 || !n2 || num_cu < 1 || !tiles || !workgroups || !tile0 || !planes_max || !wg_lo || !keys) return XFH_ERR_INVALID_ARG;
    MnnPairIn in[MNN_MAX_JOBS];
    for (int p = 0; p < n_pairs; ++p) { if (n1[p] < 1 || n2[p] < 1) return XFH_ERR_INVALID_ARG; in[p] = MnnPairIn{nullptr, n1[p], nullptr, n2[p]}; }
    MnnBatch jb;
    *keys = (unsigned long long)mnn_seg_plan(in, n_pairs, num_cu, nullptr, &jb);
    *tiles = jb.T; *workgroups = jb.G;
    for (int p = 0; p < n_pairs; ++p) { tile0[p] = jb.job[p].tile0; planes_max[p] = mnn_seg_planes_max(jb.job[p].P2, jb.T, jb.G); }
    for (int w = 0; w <= jb.G; ++w) wg_lo[w] = mnn_seg_lo(w, jb.T, jb.G);
    return XFH_OK;
}
int xfh_bench_mnn_gemm_batch(xfh_ctx* c, int n_pairs, const void* const* image1, const int* n1, const void* const* image2, const int* n2, int iters, double* us_per_launch,
                             double* sclk_mhz) {
    std::vector<XfhMatchPair> v;
    const int rc = gather_pairs(c, n_pairs, image1, n1, image2, n2, nullptr, nullptr, nullptr, nullptr, false, v);
    if (rc != XFH_OK) return rc;
    if (n_pairs < 1 || iters < 1 || !us_per_launch) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, bench_mnn_gemm_batch(c, v.data(), n_pairs, iters, us_per_launch, sclk_mhz));
    return XFH_OK;
}
int xfh_bench_match_batch(xfh_ctx* c, int n_pairs, const void* const* image1, const int* n1, const void* const* image2, const int* n2, float min_cossim,
                          int* const* idx1, int* const* idx2, float* const* dist, int* n_matches, int iters, double* us_per_call) {
    std::vector<XfhMatchPair> v;
    const int rc = gather_pairs(c, n_pairs, image1, n1, image2, n2, idx1, idx2, dist, n_matches, true, v);
    if (rc != XFH_OK) return rc;
    if (n_pairs < 1 || iters < 1 || !us_per_call) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    return time_calls(c, 50, iters, us_per_call, [&]() { return launch_mnn_batch(c, v.data(), n_pairs, min_cossim); });
}
int xfh_timing_enable(xfh_ctx* c, int kernel_id, unsigned layer_mask) {
    if (!c || kernel_id < 0 || kernel_id >= XFH_K_COUNT) return XFH_ERR_INVALID_ARG;
    KTimer& t = c->timer;
    if (kernel_id != XFH_K_NONE && !t.ev) {
        t.ev = (hipEvent_t*)calloc(2 * KTimer::MAXEV, sizeof(hipEvent_t));
        for (int i = 0; i < 2 * KTimer::MAXEV; ++i) HIPCK(c, hipEventCreate(&t.ev[i]));
    }
    t.kernel_id = kernel_id; t.layer_mask = layer_mask; t.nev = 0; t.launches = 0; t.dropped = 0;
    return XFH_OK;
}
int xfh_timing_read(xfh_ctx* c, int* launches, double* total_ms) {
    if (!c) return XFH_ERR_INVALID_ARG;
    KTimer& t = c->timer;
    HIPCK(c, hipStreamSynchronize(c->stream));
    double tot = 0.0;
    for (int i = 0; i < t.nev; ++i) {
        float ms = 0.f;
        HIPCK(c, hipEventElapsedTime(&ms, t.ev[2 * i], t.ev[2 * i + 1]));
        tot += ms;
    }
    if (launches) *launches = t.nev;
    if (total_ms) *total_ms = tot;
    const bool overflow = t.dropped > 0;
    t.nev = 0; t.dropped = 0;
    return overflow ? XFH_ERR_BATCH_TOO_LARGE : XFH_OK;       // more than 4096 matching launches since xfh_timing_enable: the sums cover the first 4096 only
}

// ------------------------------------------------------------------------- debug tensors
int xfh_debug_tensor(xfh_ctx* c, int id, int frame, float* out, size_t cap, size_t* count_out) {
    if (!c || frame < 0 || frame >= c->B || !count_out) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipStreamSynchronize(c->stream));
    const size_t xs = (size_t)c->Hmax * c->Wmax;
    const int H = c->H, W = c->W, h8 = H / 8, w8 = W / 8, h4 = H / 4, w4 = W / 4;
    const float* src = nullptr; size_t n = 0;
    if (!was_written(c, id)) return XFH_ERR_INVALID_ARG;          // block1.0's map, or a tensor the last call's regime did not write
    switch (id) {
        case XFH_T_X: src = c->X + frame * xs; n = (size_t)H * W; break;
        case XFH_T_XSTAT: src = c->xstat + frame * 2; n = 2; break;
        case XFH_T_SKIP_POOL: src = c->skip_pool + frame * (xs / 16); n = (size_t)h4 * w4; break;
        case XFH_T_FEATS: src = c->feats + frame * c->raw_stride[17]; n = (size_t)h8 * w8 * 64; break;
        case XFH_T_H1: src = c->H1 + frame * (xs / 64); n = (size_t)h8 * w8; break;
        case XFH_T_K1H: src = c->K1h + frame * xs; n = (size_t)H * W; break;
        case XFH_T_M1N: {
            // the normalised map is never written on the GPU: k_desc divides the pixels a sample touches by their stored norm.  This is that
            // quotient for every pixel, formed on the host (IEEE fp32 division) from the two tensors the GPU does hold.
            n = (size_t)h8 * w8 * 64;
            *count_out = n;
            if (!out) return XFH_OK;
            if (cap < n) return XFH_ERR_INVALID_ARG;
            std::vector<float> nrm((size_t)h8 * w8);
            HIPCK(c, hipMemcpy(out, c->feats + frame * c->raw_stride[17], n * sizeof(float), hipMemcpyDeviceToHost));
            HIPCK(c, hipMemcpy(nrm.data(), c->feat_nrm + frame * (xs / 64), nrm.size() * sizeof(float), hipMemcpyDeviceToHost));
            for (size_t p = 0; p < nrm.size(); ++p)
                for (int ch = 0; ch < 64; ++ch) out[p * 64 + ch] = out[p * 64 + ch] / nrm[p];
            return XFH_OK;
        }
        default:
            if (id >= XFH_T_RAW0 && id < XFH_T_RAW0 + XFH_NUM_LAYERS) {
                const int i = id - XFH_T_RAW0;
                if (!c->raw[i]) return XFH_ERR_INVALID_ARG;
                src = c->raw[i] + frame * c->raw_stride[i]; n = (size_t)c->lh[i] * c->lw[i] * XFH_LAYERS[i].cout;
            } else if (id >= XFH_T_STAT0 && id < XFH_T_STAT0 + XFH_NUM_LAYERS) {
                const int i = id - XFH_T_STAT0;
                src = c->stat[i] + (size_t)frame * 2 * XFH_LAYERS[i].cout; n = 2 * (size_t)XFH_LAYERS[i].cout;
            } else if (id == XFH_T_SEL) {
                int N = 0;
                HIPCK(c, hipMemcpy(&N, c->sel_n + frame, sizeof(int), hipMemcpyDeviceToHost));
                *count_out = (size_t)N * 3;
                if (!out || cap < (size_t)N * 3) return out ? XFH_ERR_INVALID_ARG : XFH_OK;
                std::vector<u64> keys((size_t)N);
                if (N > 0) HIPCK(c, hipMemcpy(keys.data(), c->sel_key + (size_t)frame * c->cfg.nfeatures, (size_t)N * 8, hipMemcpyDeviceToHost));
                for (int i = 0; i < N; ++i) {
                    const unsigned idx = (unsigned)(keys[i] & 0xFFFFFFFFull);
                    out[i * 3 + 0] = (float)(idx % (unsigned)W); out[i * 3 + 1] = (float)(idx / (unsigned)W);
                    out[i * 3 + 2] = ord2f(~(unsigned)(keys[i] >> 32));
                }
                return XFH_OK;
            } else return XFH_ERR_INVALID_ARG;
    }
    *count_out = n;
    if (!out) return XFH_OK;
    if (cap < n) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipMemcpy(out, src, n * sizeof(float), hipMemcpyDeviceToHost));
    return XFH_OK;
}

}  // extern "C"

bool ktimer_slot(xfh_ctx* c, int kernel_id, int layer, hipEvent_t* e0, hipEvent_t* e1) {
    KTimer& t = c->timer;
    if (t.kernel_id == XFH_K_NONE || t.kernel_id != kernel_id) return false;
    if (t.layer_mask != 0 && layer >= 0 && !((t.layer_mask >> layer) & 1u)) return false;
    if (!t.ev) return false;
    if (t.nev >= KTimer::MAXEV) { ++t.dropped; return false; }      // reported by xfh_timing_read: never silently
    *e0 = t.ev[2 * t.nev]; *e1 = t.ev[2 * t.nev + 1];
    ++t.nev;
    return true;
}
