// bowdb_query.hip.h -- KeyFrameDatabase::DetectRelocalizationCandidates / DetectNBestCandidates (src/KeyFrameDatabase.cc:733-845, :604-730) with
// L1Scoring::score (thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68), B queries against ONE database per call (xfh_bowdb_query_device; the contract
// is written out in include/xfeat_hip.h).  The database is plain arrays of BowVectors, one per slot; there is no inverted file: every query scans
// every slot.
//
//   k_bowdb_score   one wave per (query, slot), 16 slots of one query per workgroup, which stages the query's ids in LDS (ids only: 16384 * 4 B =
//                   64 KB at the largest stride; a value is fetched on a hit).  The lanes take the slot's entries 64 at a time, coalesced, and
//                   binary-search the query ids (bowdb_math.h).  A ballot gives the hits: its popcount adds to `common`, its first bit of the
//                   first chunk that has one names first_common.  The double terms are added to ONE accumulator in lane order -- the set bits of
//                   the ballot are walked with a readlane -- chunk after chunk: the reference's left-to-right sum over ascending word id.  (A tree
//                   or butterfly reduction gives other bits.)  Writes common, score and, into the workspace, first_common per (query, slot).
//   k_bowdb_select  one workgroup of 1024 threads per query.  max_common by an LDS atomic, min_common, the status of every slot, state = (float)
//                   score for the SCORED ones, a barrier (a neighbour that is BELOW_MIN is read with its old value).  With d_seq the slots are
//                   ranked by (seq, slot) with one sort; then the scored slots are sorted by first_common << 32 | rank << 16 | slot -- the list
//                   order of lKFsSharingWords -- with the bitonic sort of vocab_transform.hip.h.  acc and pBestKF per list entry in parallel,
//                   best_acc by an LDS atomic on the bits of the non-negative floats.  RELOC keeps acc > 0.75f * best_acc in list order; NBEST
//                   sorts by (descending acc, list rank), which is list::sort's stable order.  The dedupe by pBestKF is an atomicMin of the
//                   position per best slot, among the kept entries only; the survivors are compacted in order by ballot and prefix sum.
//
// Plain stores only.  k_bowdb_select reads what k_bowdb_score wrote across the kernel boundary; inside it the barriers order the workgroup's
// own global stores (status, state) before its loads, as in k_vocab_finish.  LDS atomics are integer min / max / add: order free.
#pragma once
#include "ctx.h"
#include "bowdb_math.h"
#include "search_common.hip.h"
#include "vocab_transform.hip.h"                                       // vocab_sort, vocab_count_items

#define XFH_BOWDB_SCORE_THREADS 1024
#define XFH_BOWDB_SELECT_THREADS XFH_VOCAB_FINISH_THREADS              // vocab_sort strides by it
#define XFH_BOWDB_SELECT_TAIL 256                                      // bytes of LDS behind the arrays: the wave counts and the scalars
#define XFH_BOWDB_SELECT_MIN_P 64                                      // keeps every carve offset a multiple of 16
// LDS of k_bowdb_select per key: u64 key, float acc, int first (uint16 seq rank before), uint16 best
#define XFH_BOWDB_SELECT_LDS(P) ((size_t)(P) * 18 + XFH_BOWDB_SELECT_TAIL)

__global__ __launch_bounds__(XFH_BOWDB_SCORE_THREADS)
void k_bowdb_score(BowDbArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t bq[];      // the query's ids
    const int tid = threadIdx.x, lane = tid & 63, pb = blockIdx.y;
    const int nq = bowdb_clamp_n(a.q_n_words[pb], a.q_stride);
    const uint32_t* qi = a.q_ids + (size_t)pb * a.q_stride;
    for (int k = tid; k < nq; k += XFH_BOWDB_SCORE_THREADS) bq[k] = qi[k];
    __syncthreads();
    const int s = __builtin_amdgcn_readfirstlane(blockIdx.x * (XFH_BOWDB_SCORE_THREADS / 64) + (tid >> 6));
    if (s >= a.n_slots) return;
    const int nk = bowdb_clamp_n(a.db_n_words[s], a.db_stride);
    const uint32_t* ids = a.db_ids + (size_t)s * a.db_stride;
    const double* dv = a.db_vals + (size_t)s * a.db_stride;
    const double* qv = a.q_vals + (size_t)pb * a.q_stride;
    double sum = 0.0;
    int common = 0;
    uint32_t first = XFH_BOWDB_NO_WORD;
    for (int c0 = 0; c0 < nk; c0 += 64) {                              // (uniform)
        const int e = c0 + lane;
        uint32_t id = 0;
        int p = -1;
        if (e < nk) { id = ids[e]; p = bowdb_find(bq, nq, id); }
        u64 hits = __ballot(p >= 0);
        if (hits == 0) continue;
        const double t = p >= 0 ? bowdb_term(qv[p], dv[e]) : 0.0;
        if (common == 0) first = (uint32_t)__builtin_amdgcn_readlane((int)id, __builtin_amdgcn_readfirstlane(__builtin_ctzll(hits)));
        common += __popcll(hits);
        while (hits) {                                                 // `score += ...` in ascending word id
            sum += wave_readlane_f64(t, __builtin_ctzll(hits));
            hits &= hits - 1;
        }
    }
    if (lane == 0) {
        const size_t g = (size_t)pb * a.n_slots + s;
        a.common[g] = common; a.score[g] = bowdb_finish(sum); a.first_common[g] = first;
    }
}

// positions p < n with keep(p), in order: emit(p, k) with k the number of kept positions before p.  Returns their count.  wsum: 16 ints of LDS.
// Every thread of the workgroup calls it; ends with a barrier.
template <typename Keep, typename Emit>
__device__ __forceinline__ int bowdb_compact(int n, int* wsum, Keep keep, Emit emit) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0;
    for (int p0 = 0; p0 < n; p0 += XFH_BOWDB_SELECT_THREADS) {        // (uniform)
        const int p = p0 + tid;
        const bool kp = p < n && keep(p);
        const u64 bal = __ballot(kp);
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int pre = 0, tot = 0;
        for (int x = 0; x < XFH_BOWDB_SELECT_THREADS / 64; ++x) { const int cnt = wsum[x]; pre += x < wave ? cnt : 0; tot += cnt; }
        if (kp) emit(p, base + pre + __popcll(bal & ((1ull << lane) - 1ull)));
        base += tot;
        __syncthreads();
    }
    return base;
}

__global__ __launch_bounds__(XFH_BOWDB_SELECT_THREADS)
void k_bowdb_select(BowDbArgs a) {
    extern __shared__ __attribute__((aligned(16))) u64 bkeys[];        // P keys, P acc, P first, P best, then XFH_BOWDB_SELECT_TAIL bytes
    const int tid = threadIdx.x, pb = blockIdx.x, n = a.n_slots;
    int P = XFH_BOWDB_SELECT_MIN_P;
    while (P < n) P <<= 1;
    float* s_acc = (float*)(bkeys + P);
    int* s_first = (int*)(s_acc + P);
    uint16_t* s_rank = (uint16_t*)s_first;                             // the seq rank of a slot: done with before s_first is filled
    uint16_t* s_best = (uint16_t*)(s_first + P);
    int* wsum = (int*)(s_best + P);                                    // [16]
    int* s_sc = wsum + 16;                                             // n_listed, max_common, n_scored, the bits of best_acc
    const size_t off = (size_t)pb * n;
    const int32_t* common = a.common + off;
    const double* score = a.score + off;
    const uint8_t* excl = a.exclude ? a.exclude + off : nullptr;
    uint8_t* status = a.status + off;
    float* state = a.state + off;

    // ---- lKFsSharingWords as a set: the occupied slots that share a word and are not excluded; maxCommonWords over them
    if (tid < 4) s_sc[tid] = 0;
    __syncthreads();
    for (int s = tid; s < n; s += XFH_BOWDB_SELECT_THREADS)
        if (bowdb_clamp_n(a.db_n_words[s], a.db_stride) > 0 && common[s] > 0 && !(excl && excl[s])) { atomicAdd(&s_sc[0], 1); atomicMax(&s_sc[1], common[s]); }
    __syncthreads();
    const int n_listed = s_sc[0], max_common = s_sc[1], min_common = bowdb_min_common(max_common);

    // ---- status; the persistent score of the slots that are scored (`pKFi->mRelocScore=si`), of no other
    for (int s = tid; s < P; s += XFH_BOWDB_SELECT_THREADS) {
        if (s < n) {
            const int cm = common[s];
            const uint8_t st = bowdb_clamp_n(a.db_n_words[s], a.db_stride) <= 0 ? XFH_BOWDB_EMPTY : cm <= 0 ? XFH_BOWDB_NOT_SHARING
                             : (excl && excl[s]) ? XFH_BOWDB_EXCLUDED : cm > min_common ? XFH_BOWDB_SCORED : XFH_BOWDB_BELOW_MIN;
            status[s] = st;
            if (st == XFH_BOWDB_SCORED) state[s] = (float)score[s];
        }
        if (a.seq) bkeys[s] = s < n ? (((u64)a.seq[s] << 32) | (u64)(unsigned)s) : XFH_KEY_NONE;
    }
    if (a.seq) {                                                       // the insertion order of the slots: rank by (seq, slot)
        vocab_sort(bkeys, P);
        for (int k = tid; k < n; k += XFH_BOWDB_SELECT_THREADS) s_rank[(int)(bkeys[k] & 0xFFFFull)] = (uint16_t)k;
    }
    __syncthreads();

    // ---- lScoreAndMatch in list order: (first shared word, insertion order)
    for (int s = tid; s < P; s += XFH_BOWDB_SELECT_THREADS) {
        const bool in = s < n && status[s] == XFH_BOWDB_SCORED;
        const u64 rank = a.seq ? (u64)s_rank[s < n ? s : 0] : (u64)(unsigned)s;
        bkeys[s] = in ? (((u64)a.first_common[off + s] << 32) | (rank << 16) | (u64)(unsigned)s) : XFH_KEY_NONE;
    }
    vocab_sort(bkeys, P);
    const int ns = vocab_count_items(bkeys, P, &s_sc[2]);

    // ---- the accumulation over the covisibility neighbours (:675-700, :796-821): every LISTED neighbour counts, with the state it has now
    for (int r = tid; r < n; r += XFH_BOWDB_SELECT_THREADS) {
        int slot = -1, best = -1;
        float acc = 0.0f;
        if (r < ns) {
            slot = (int)(bkeys[r] & 0xFFFFull);
            float best_score = (float)score[slot];
            acc = best_score; best = slot;
            for (int j = 0; j < a.nn; ++j) {
                const int nb = a.neigh[(size_t)slot * a.nn + j];
                if (nb < 0 || nb >= n) continue;
                const uint8_t st = status[nb];
                if (st != XFH_BOWDB_SCORED && st != XFH_BOWDB_BELOW_MIN) continue;            // `mnRelocQuery != F->mnId`
                const float v = state[nb];
                acc += v;
                if (v > best_score) { best = nb; best_score = v; }
            }
            s_acc[r] = acc; s_best[r] = (uint16_t)best;
            if (acc > 0.0f) atomicMax(&s_sc[3], __float_as_int(acc));   // `if(accScore>bestAccScore)` from 0: the bits of floats > 0 order as ints
        }
        a.list_slot[off + r] = slot; a.list_acc[off + r] = acc; a.list_best[off + r] = best;
        s_first[r] = 0x7fffffff;
    }
    __syncthreads();
    const float best_acc = __int_as_float(s_sc[3]);

    // ---- the tail of the form; the dedupe keeps the first entry of a pBestKF among the entries that are in
    int nc;
    if (a.form == XFH_BOWDB_FORM_RELOC) {
        const float min_retain = 0.75f * best_acc;
        for (int r = tid; r < ns; r += XFH_BOWDB_SELECT_THREADS)
            if (s_acc[r] > min_retain) atomicMin(&s_first[s_best[r]], r);
        __syncthreads();
        nc = bowdb_compact(ns, wsum, [&](int r) { return s_acc[r] > min_retain && s_first[s_best[r]] == r; },
                           [&](int r, int k) { a.cand_slot[off + k] = (int)s_best[r]; a.cand_acc[off + k] = s_acc[r]; });
    } else {
        for (int k = tid; k < P; k += XFH_BOWDB_SELECT_THREADS)       // `lAccScoreAndMatch.sort(compFirst)`: stable, acc descending
            bkeys[k] = k < ns ? (((u64)bowdb_desc_key(s_acc[k]) << 32) | (u64)(unsigned)k) : XFH_KEY_NONE;
        vocab_sort(bkeys, P);
        for (int p = tid; p < ns; p += XFH_BOWDB_SELECT_THREADS) atomicMin(&s_first[s_best[(int)(bkeys[p] & 0xFFFFull)]], p);
        __syncthreads();
        nc = bowdb_compact(ns, wsum, [&](int p) { return s_first[s_best[(int)(bkeys[p] & 0xFFFFull)]] == p; },
                           [&](int p, int k) { const int r = (int)(bkeys[p] & 0xFFFFull); a.cand_slot[off + k] = (int)s_best[r]; a.cand_acc[off + k] = s_acc[r]; });
    }
    for (int k = nc + tid; k < n; k += XFH_BOWDB_SELECT_THREADS) { a.cand_slot[off + k] = -1; a.cand_acc[off + k] = 0.0f; }
    if (tid == 0) {
        int32_t* h = a.header + (size_t)pb * XFH_BOWDB_HEADER_INTS;
        h[0] = n_listed; h[1] = max_common; h[2] = min_common; h[3] = ns; h[4] = nc; h[5] = 0; h[6] = 0; h[7] = 0;
        a.best_acc[pb] = best_acc;
    }
}

hipError_t launch_bowdb_query(xfh_ctx* c, const BowDbArgs& a, int B) {
    XFH_SET_LDS_ATTR_ONCE(c, k_bowdb_score, (size_t)XFH_GRID_MAX_N * sizeof(uint32_t));
    XFH_SET_LDS_ATTR_ONCE(c, k_bowdb_select, XFH_BOWDB_SELECT_LDS(XFH_BOWDB_MAX_SLOTS));
    int P = XFH_BOWDB_SELECT_MIN_P;
    while (P < a.n_slots) P <<= 1;
    const int per = XFH_BOWDB_SCORE_THREADS / 64;
    launch_k(c, XFH_K_BOWDB_SCORE, -1, k_bowdb_score, dim3((a.n_slots + per - 1) / per, B), dim3(XFH_BOWDB_SCORE_THREADS), (size_t)a.q_stride * sizeof(uint32_t), a);
    launch_k(c, XFH_K_BOWDB_SELECT, -1, k_bowdb_select, dim3(B), dim3(XFH_BOWDB_SELECT_THREADS), XFH_BOWDB_SELECT_LDS(P), a);
    return hipGetLastError();
}
