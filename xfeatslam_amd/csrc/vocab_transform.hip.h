// vocab_transform.hip.h -- TemplatedVocabulary::transform(features, v, fv, levelsup) (thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1194) for
// the TF_IDF / L1_NORM vocabulary of ORB-SLAM3, B frames of n rows per call (xfh_bow_transform_device; the contract is written out in
// include/xfeat_hip.h).  Every row of the descriptor block goes through the vocabulary, zero padding rows included, as the reference hands
// every row of mDescriptors to DBoW2.
//
//   k_vocab_descend  16 lanes per feature, 4 features per wave, 16 per workgroup.  The feature's 8 words stay in registers.  Per level a lane
//                   loads the 32 descriptor bytes of its child as two 16-byte loads -- the children of a node are consecutive rows of the
//                   blob, so a group reads one 320-byte run at k = 10 -- and, beside them, the child's own slot entry, so that the winner's
//                   child range arrives with its distance and a level costs ONE dependent memory round trip.  8 popcounts, a 16-lane minimum
//                   of d << 8 | child position (the first child with the strictly least distance, vocab_math.h), the winner's entry by four
//                   shuffles.  More than 16 children take a second pass of the same lanes.  The loop is uniform across the wave: a group that
//                   has reached its leaf idles until the deepest of the four has.  The kernel is latency bound (L dependent gathers from a
//                   table that does not fit L2 at ORBvoc's size) and small: 4096 * B / 4 waves; it keeps few registers so that all of them
//                   are resident.  Writes word, weight and node_of (XFH_NODE_NONE for a stopped feature) per feature.
//   k_vocab_finish   two workgroups of 1024 threads per frame, one for the node blob and one for the BowVector.  64-bit keys node_id << 32 | index
//                   resp. word << 32 | index of the features
//                   that are not stopped are sorted in LDS (bitonic; a node id of a 1.1 M-node vocabulary and a 14-bit index do not fit the
//                   32-bit keys of the grid sort; 16384 keys are 128 KB, the large-LDS opt-in k_init_resolve uses).  Runs of equal ids are
//                   ranked with a ballot and a prefix over the 16 waves.  From the node keys the node blob is written field by field as
//                   xfh_nodes_pack writes it (capi_triangulation.cpp): zeroed, header, ids, node_start, items, node_of.  From the word keys
//                   the BowVector: the thread on the head of a run adds the weights of the run's features in index order, ONE double add per
//                   feature (BowVector::addWeight in feature order), then ONE thread sums the values in ascending word id (normalize(L1))
//                   and all divide.  Both are sequential by definition: at most n <= 16384 dependent double adds each, on one lane, from LDS
//                   resp. from the weights the first kernel wrote.
//
// Plain stores only; the only memory one kernel reads after another wrote it crosses a kernel boundary, and inside k_vocab_finish the
// barriers order the workgroup's own global stores (the raw values in the workspace) before its loads, as in k_init_resolve.
#pragma once
#include "ctx.h"
#include "vocab_math.h"
#include "nodes_layout.h"
#include "search_common.hip.h"

#define XFH_VOCAB_FINISH_THREADS 1024
#define XFH_VOCAB_FINISH_TAIL 256                                      // bytes of LDS behind the keys: the wave counts and the scalars

__global__ __launch_bounds__(256)
void k_vocab_descend(VocabArgs a) {
    const int lane = threadIdx.x & 63, sub = lane & 15;
    const int i = blockIdx.x * 16 + (threadIdx.x >> 4), pb = blockIdx.y;
    VocabView v;
    if (!vocab_open(a.vocab, a.vocab_bytes, &v)) return;              // (uniform; the entry point refuses such a size)
    const bool live = i < a.n;
    const int row = live ? i : a.n - 1;                               // an idle group walks the last row: the loop below is uniform
    uint32_t q[8];
    const char* qr = a.desc + (size_t)pb * a.desc_stride + (size_t)row * 256;
    vocab_load16(qr, q); vocab_load16(qr + 16, q + 4);
    VocabWalk w = vocab_walk_begin(v.L, a.levelsup);
    VocabSlot e = vocab_slot(v, 0);
    for (int steps = 0;; ++steps) {
        vocab_walk_enter(w, e);
        const bool stop = vocab_walk_stops(e, steps);                  // (uniform in the group of 16)
        if (__all(stop)) break;
        uint32_t key = XFH_VOCAB_KEY_NONE;
        VocabSlot ce = e;                                              // the entry of this lane's best child
        if (!stop)
            for (uint32_t c = sub; c < e.nch; c += 16) {
                const uint32_t k = vocab_child_key(v, e.first, c, q);
                const VocabSlot s = vocab_slot(v, e.first + c);
                if (k < key) { key = k; ce = s; }
            }
        uint32_t best = key;
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) { const uint32_t o = __shfl_xor(best, m); best = o < best ? o : best; }
        const int src = (lane & 48) | (int)(best & 15u);               // the lane that holds the winner (position c sits on lane c & 15)
        VocabSlot ne;
        ne.first = __shfl(ce.first, src); ne.nch = __shfl(ce.nch, src); ne.node_id = __shfl(ce.node_id, src); ne.word_id = __shfl(ce.word_id, src);
        if (!stop) { vocab_walk_take(w, e, best); e = ne; }
    }
    if (live && sub == 0) {
        const size_t g = (size_t)pb * a.n + i;
        const double wt = vocab_weight(v, w.slot);
        a.word[g] = e.word_id; a.weight[g] = wt;
        a.node_of[g] = vocab_stopped(wt) ? XFH_NODE_NONE : vocab_walk_node(w, e);
    }
}

// ascending bitonic sort of P (a power of two) keys in LDS by the whole workgroup; ends with a barrier.  Pair t of a stage is (i, i + j) with
// i = t with a zero bit inserted at j: for j <= 32 the 64 pairs of a wave lie in ONE block of 128 consecutive keys, the same block for
// every such j, so the stages j = 32 .. 1 of a merge need no workgroup barrier between them -- the LDS serves the instructions of a wave in
// order, and the wave-scope fences keep the compiler from moving a load above the stores of the stage before.
__device__ __forceinline__ void vocab_sort(u64* s, int P) {
    const int tid = threadIdx.x;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += XFH_VOCAB_FINISH_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const u64 x = s[i], y = s[i + j];
                if ((x > y) == ((i & k) == 0)) { s[i] = y; s[i + j] = x; }
            }
            if (j > 32 || j == 1) __syncthreads();
            else {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
        }
}

// The first `nit` sorted keys in rounds of 1024 positions: emit(k, rank, head) for every position k, where head says that the upper word of
// key k differs from that of key k - 1 and rank counts the heads before k (a head's rank = the index of its run).  Returns the number of
// runs.  wsum: 16 ints of LDS.  Every thread of the workgroup calls it; ends with a barrier.
template <typename Emit>
__device__ __forceinline__ int vocab_runs(const u64* key, int nit, int* wsum, Emit emit) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0;
    for (int k0 = 0; k0 < nit; k0 += XFH_VOCAB_FINISH_THREADS) {     // (uniform)
        const int k = k0 + tid;
        const bool head = k < nit && (k == 0 || (uint32_t)(key[k] >> 32) != (uint32_t)(key[k - 1] >> 32));
        const u64 bal = __ballot(head);
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int pre = 0, tot = 0;
        for (int x = 0; x < XFH_VOCAB_FINISH_THREADS / 64; ++x) { const int cnt = wsum[x]; pre += x < wave ? cnt : 0; tot += cnt; }
        if (k < nit) emit(k, base + pre + __popcll(bal & ((1ull << lane) - 1ull)), head);
        base += tot;
        __syncthreads();
    }
    return base;
}

// the number of keys below XFH_KEY_NONE in P sorted keys (they come first); ends with a barrier
__device__ __forceinline__ int vocab_count_items(const u64* key, int P, int* out) {
    if (threadIdx.x == 0) *out = 0;
    __syncthreads();
    for (int k = threadIdx.x; k < P; k += XFH_VOCAB_FINISH_THREADS)
        if (key[k] != XFH_KEY_NONE && (k + 1 == P || key[k + 1] == XFH_KEY_NONE)) *out = k + 1;
    __syncthreads();
    return *out;
}

__global__ __launch_bounds__(XFH_VOCAB_FINISH_THREADS)
void k_vocab_finish(VocabArgs a) {
    extern __shared__ __attribute__((aligned(16))) u64 vkeys[];        // P keys, then XFH_VOCAB_FINISH_TAIL bytes
    const int tid = threadIdx.x, pb = blockIdx.x, n = a.n;
    const bool words = blockIdx.y != 0;                                // two workgroups per frame: the node blob, the BowVector
    int P = 1;
    while (P < n) P <<= 1;
    int* wsum = (int*)(vkeys + P);                                     // [16]
    int* s_cnt = wsum + 16;
    double* s_norm = (double*)(wsum + 32);
    const uint32_t* node_of = a.node_of + (size_t)pb * n;
    const uint32_t* id_of = words ? a.word + (size_t)pb * n : node_of;
    char* blob = a.nodes + (size_t)pb * nodes_bytes(n);
    if (!words)                                                        // (the barriers of the sort order the zeroing before the stores below)
        for (size_t q = tid; q < nodes_bytes(n) / 16; q += XFH_VOCAB_FINISH_THREADS) ((uint4*)blob)[q] = make_uint4(0u, 0u, 0u, 0u);
    for (int k = tid; k < P; k += XFH_VOCAB_FINISH_THREADS)
        vkeys[k] = (k < n && node_of[k] != XFH_NODE_NONE) ? (((u64)id_of[k] << 32) | (u64)(unsigned)k) : XFH_KEY_NONE;
    vocab_sort(vkeys, P);
    const int nit = vocab_count_items(vkeys, P, s_cnt);

    if (!words) {
        // ---- the node blob: what xfh_nodes_pack(node_of) writes
        uint32_t* ids = (uint32_t*)(blob + nodes_ids_off(n));
        int32_t* ns = (int32_t*)(blob + nodes_start_off(n));
        int32_t* items = (int32_t*)(blob + nodes_items_off(n));
        uint32_t* of = (uint32_t*)(blob + nodes_of_off(n));
        const int nn = vocab_runs(vkeys, nit, wsum, [&](int k, int rank, bool head) {
            items[k] = (int32_t)(vkeys[k] & 0xFFFFFFFFull);
            if (head) { ids[rank] = (uint32_t)(vkeys[k] >> 32); ns[rank] = k; }
        });
        for (int k = tid; k < n; k += XFH_VOCAB_FINISH_THREADS) of[k] = node_of[k];
        if (tid == 0) {
            ns[nn] = nit;
            NodesHeader* h = (NodesHeader*)blob;
            h->magic = XFH_NODES_MAGIC; h->n = n; h->n_nodes = nn; h->n_items = nit;
        }
        return;
    }

    // ---- the BowVector: distinct words ascending, addWeight in feature order, normalize(L1)
    const double* weight = a.weight + (size_t)pb * n;
    uint32_t* bow_ids = a.bow_ids + (size_t)pb * n;
    double* bow_vals = a.bow_vals + (size_t)pb * n;
    double* raw = (double*)(a.ws + (size_t)pb * a.ws_stride);
    const int nw = vocab_runs(vkeys, nit, wsum, [&](int k, int rank, bool head) {
        if (!head) return;
        const uint32_t id = (uint32_t)(vkeys[k] >> 32);
        double val = weight[(int)(vkeys[k] & 0xFFFFFFFFull)];         // `insert(vit, value_type(id, v))`, then `vit->second += v` per feature
        for (int j = k + 1; j < nit && (uint32_t)(vkeys[j] >> 32) == id; ++j) val += weight[(int)(vkeys[j] & 0xFFFFFFFFull)];
        bow_ids[rank] = id; raw[rank] = val;
    });
    double* vals = (double*)vkeys;                                     // the keys are done with (vocab_runs ended with a barrier)
    for (int r = tid; r < nw; r += XFH_VOCAB_FINISH_THREADS) vals[r] = raw[r];
    __syncthreads();
    if (tid == 0) {
        double norm = 0.0;
        for (int r = 0; r < nw; ++r) norm += fabs(vals[r]);            // BowVector::normalize(L1): left to right over ascending word id
        *s_norm = norm;
        a.n_words[pb] = nw;
    }
    __syncthreads();
    const double norm = *s_norm;
    for (int r = tid; r < n; r += XFH_VOCAB_FINISH_THREADS) {
        if (r < nw) bow_vals[r] = norm > 0.0 ? vals[r] / norm : vals[r];
        else { bow_ids[r] = 0xFFFFFFFFu; bow_vals[r] = 0.0; }
    }
}

hipError_t launch_bow_transform(xfh_ctx* c, const VocabArgs& a, int B) {
    XFH_SET_LDS_ATTR_ONCE(c, k_vocab_finish, (size_t)XFH_GRID_MAX_N * sizeof(u64) + XFH_VOCAB_FINISH_TAIL);
    int P = 1;
    while (P < a.n) P <<= 1;
    launch_k(c, XFH_K_VOCAB_DESCEND, -1, k_vocab_descend, dim3((a.n + 15) / 16, B), dim3(256), 0, a);
    launch_k(c, XFH_K_VOCAB_FINISH, -1, k_vocab_finish, dim3(B, 2), dim3(XFH_VOCAB_FINISH_THREADS), (size_t)P * sizeof(u64) + XFH_VOCAB_FINISH_TAIL, a);
    return hipGetLastError();
}
