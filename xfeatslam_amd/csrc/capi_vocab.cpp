// capi_vocab.cpp -- the vocabulary entry points of include/xfeat_hip.h: the host writer and reader of the vocabulary blob (vocab_layout.h),
// the descent of one feature on the host (vocab_math.h, the kernel's own lines), the workspace size, the device form of
// TemplatedVocabulary::transform and the host-pointer form (host_stage.h).
#include "host_stage.h"
#include "nodes_layout.h"
#include "vocab_math.h"
#include <string.h>
#include <vector>

static size_t transform_ws_stride(int n) { return ((size_t)n * sizeof(double) + 255) & ~(size_t)255; }
// what xfh_bow_transform_device and xfh_bow_transform check alike before anything is staged or launched (the pointers are theirs to check)
static bool transform_args_ok(int B, int n, int levelsup, int flags, size_t vocab_bytes) {
    return B >= 1 && B <= 65535 && n >= 1 && n <= XFH_GRID_MAX_N && levelsup >= 0 && flags == XFH_BOWT_TF_IDF_L1 && vocab_bytes >= ::vocab_bytes(2);
}

extern "C" {

size_t xfh_vocab_bytes(int n_nodes) { return n_nodes < 1 ? 0 : vocab_bytes((size_t)n_nodes); }

int xfh_vocab_pack(int n_nodes, int L, const uint32_t* parent, const uint32_t* word_id, const double* weight, const uint8_t* desc, void* blob,
                   int* max_children, int* depth) {
    if (n_nodes < 2 || L < 1 || L > 10 || !parent || !word_id || !weight || !desc || !blob) return XFH_ERR_INVALID_ARG;
    const size_t n = (size_t)n_nodes;
    std::vector<uint32_t> cnt(n, 0), start(n + 1, 0), child(n), order(n), level(n, 0), slot_of(n);
    for (size_t i = 1; i < n; ++i) {
        if (parent[i] >= i) return XFH_ERR_INVALID_ARG;                 // (the reference would index past m_nodes)
        if (++cnt[parent[i]] > XFH_VOCAB_MAX_CHILDREN) return XFH_ERR_INVALID_ARG;
    }
    if (cnt[0] == 0) return XFH_ERR_INVALID_ARG;                        // a root without children: transform() would read children[0] of none
    for (size_t i = 0; i < n; ++i) start[i + 1] = start[i] + cnt[i];
    {
        std::vector<uint32_t> fill(start.begin(), start.end() - 1);
        for (size_t i = 1; i < n; ++i) child[fill[parent[i]]++] = (uint32_t)i;    // ascending id inside a parent: the push_back order
    }
    // breadth first: slot 0 is the root, the children of a slot are the next free slots in child order
    size_t next = 1;
    uint32_t maxc = 0, deep = 0;
    order[0] = 0; slot_of[0] = 0;
    for (size_t s = 0; s < n; ++s) {
        const uint32_t node = order[s];
        maxc = cnt[node] > maxc ? cnt[node] : maxc;
        for (uint32_t q = start[node]; q < start[node + 1]; ++q) {
            const uint32_t c = child[q];
            level[c] = level[node] + 1; deep = level[c] > deep ? level[c] : deep;
            slot_of[c] = (uint32_t)next; order[next++] = c;
        }
    }
    if (deep > XFH_VOCAB_MAX_DEPTH) return XFH_ERR_INVALID_ARG;
    char* p = (char*)blob;
    memset(p, 0, vocab_bytes(n));
    VocabHeader h;
    memset(&h, 0, sizeof h);
    h.magic = XFH_VOCAB_MAGIC; h.n_nodes = n_nodes; h.L = L; h.max_children = (int32_t)maxc; h.depth = (int32_t)deep;
    memcpy(p, &h, sizeof h);
    for (size_t s = 0; s < n; ++s) {
        const uint32_t node = order[s];
        VocabSlot e;
        e.nch = cnt[node]; e.first = e.nch ? slot_of[child[start[node]]] : 0u; e.node_id = node; e.word_id = word_id[node];
        memcpy(p + vocab_slot_off(n) + 16 * s, &e, 16);
        if (s > 0) {                                                    // (the root's weight and descriptor are never read: stored as zero)
            memcpy(p + vocab_weight_off(n) + 8 * s, &weight[node], 8);
            memcpy(p + vocab_desc_off(n) + XFH_VOCAB_ROW * s, desc + XFH_VOCAB_ROW * (size_t)node, XFH_VOCAB_ROW);
        }
    }
    if (max_children) *max_children = (int)maxc;
    if (depth) *depth = (int)deep;
    return XFH_OK;
}

// host, stateless: a vocabulary blob -> the arrays it was packed from, in node-id order (parent[0] = 0, weight[0] = 0 and a zero row for the
// root).  Everything the blob claims is checked before it is used.
int xfh_vocab_unpack(const void* blob, size_t nbytes, int n_nodes, int* L, uint32_t* parent, uint32_t* word_id, double* weight, uint8_t* desc,
                     int* max_children, int* depth) {
    if (!blob || n_nodes < 2 || !L || !parent || !word_id || !weight || !desc) return XFH_ERR_INVALID_ARG;
    const size_t n = (size_t)n_nodes;
    if (nbytes < vocab_bytes(n)) return XFH_ERR_INVALID_ARG;            // truncated
    VocabHeader h;
    memcpy(&h, blob, sizeof h);
    if (h.magic != XFH_VOCAB_MAGIC || h.n_nodes != n_nodes || h.L < 1 || h.L > 10) return XFH_ERR_INVALID_ARG;
    const char* p = (const char*)blob;
    std::vector<VocabSlot> e(n);
    memcpy(e.data(), p + vocab_slot_off(n), 16 * n);
    std::vector<uint8_t> seen(n, 0);
    std::vector<uint32_t> level(n, 0);
    size_t next = 1;
    uint32_t maxc = 0, deep = 0;
    if (e[0].node_id != 0 || e[0].nch == 0) return XFH_ERR_INVALID_ARG;
    for (size_t s = 0; s < n; ++s) {
        if (e[s].node_id >= n || seen[e[s].node_id]) return XFH_ERR_INVALID_ARG;           // the ids are a permutation
        seen[e[s].node_id] = 1;
        if (e[s].nch == 0) { if (e[s].first != 0) return XFH_ERR_INVALID_ARG; continue; }
        if (e[s].nch > XFH_VOCAB_MAX_CHILDREN || e[s].first != next || e[s].nch > n - next) return XFH_ERR_INVALID_ARG;   // breadth first, no gaps
        for (size_t c = next; c < next + e[s].nch; ++c) {
            if (e[c].node_id <= e[s].node_id || e[c].node_id >= n || (c > next && e[c].node_id <= e[c - 1].node_id)) return XFH_ERR_INVALID_ARG;
            level[c] = level[s] + 1; deep = level[c] > deep ? level[c] : deep;
            parent[e[c].node_id] = e[s].node_id;
        }
        maxc = e[s].nch > maxc ? e[s].nch : maxc;
        next += e[s].nch;
    }
    if (next != n || deep > XFH_VOCAB_MAX_DEPTH) return XFH_ERR_INVALID_ARG;
    parent[0] = 0;
    for (size_t s = 0; s < n; ++s) {
        const uint32_t node = e[s].node_id;
        word_id[node] = e[s].word_id;
        memcpy(&weight[node], p + vocab_weight_off(n) + 8 * s, 8);
        memcpy(desc + XFH_VOCAB_ROW * (size_t)node, p + vocab_desc_off(n) + XFH_VOCAB_ROW * s, XFH_VOCAB_ROW);
    }
    *L = h.L;
    if (max_children) *max_children = (int)maxc;
    if (depth) *depth = (int)deep;
    return XFH_OK;
}

int xfh_vocab_descend(const void* blob, size_t nbytes, int levelsup, const void* row32, uint32_t* word_id, uint32_t* node_id, double* weight) {
    if (!blob || !row32 || !word_id || !node_id || !weight || levelsup < 0) return XFH_ERR_INVALID_ARG;
    VocabView v;
    if (!vocab_open(blob, nbytes, &v)) return XFH_ERR_INVALID_ARG;      // not even one node fits nbytes
    uint32_t q[8];
    memcpy(q, row32, 32);                                               // the bits of the first 8 floats; never read as floats
    vocab_descend_row(v, levelsup, q, word_id, node_id, weight);
    return XFH_OK;
}

size_t xfh_bow_transform_workspace_bytes(int n, int B) {
    if (B < 1 || B > 65535 || n < 1 || n > XFH_GRID_MAX_N) return 0;
    return (size_t)B * transform_ws_stride(n);
}

int xfh_bow_transform_device(xfh_ctx* c, int B, int n, int levelsup, int flags, const void* d_vocab, size_t vocab_nbytes, const float* d_desc,
                             size_t desc_stride_bytes, void* d_workspace, uint32_t* d_word, uint32_t* d_node_of, double* d_weight, void* d_nodes,
                             uint32_t* d_bow_ids, double* d_bow_vals, int* d_n_words) {
    if (!c || !transform_args_ok(B, n, levelsup, flags, vocab_nbytes)) return XFH_ERR_INVALID_ARG;
    if (!d_vocab || !d_desc || !d_workspace || !d_word || !d_node_of || !d_weight || !d_nodes || !d_bow_ids || !d_bow_vals || !d_n_words)
        return XFH_ERR_INVALID_ARG;
    if (misaligned(15, d_vocab, d_desc, desc_stride_bytes, d_workspace, d_nodes) || misaligned(7, d_weight, d_bow_vals) ||
        misaligned(3, d_word, d_node_of, d_bow_ids, d_n_words)) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    VocabArgs a = {};
    a.vocab = (const char*)d_vocab; a.vocab_bytes = vocab_nbytes; a.n = n; a.levelsup = levelsup;
    a.desc = (const char*)d_desc; a.desc_stride = desc_stride_bytes;
    a.ws = (char*)d_workspace; a.ws_stride = transform_ws_stride(n);
    a.word = d_word; a.node_of = d_node_of; a.weight = d_weight; a.nodes = (char*)d_nodes;
    a.bow_ids = d_bow_ids; a.bow_vals = d_bow_vals; a.n_words = d_n_words;
    HIPCK(c, launch_bow_transform(c, a, B));
    return XFH_OK;
}

int xfh_bow_transform(xfh_ctx* c, int n, int levelsup, int flags, const void* vocab, size_t vocab_nbytes, const float* desc, uint32_t* word,
                      uint32_t* node_of, double* weight, void* nodes, uint32_t* bow_ids, double* bow_vals, int* n_words) {
    if (!c || !transform_args_ok(1, n, levelsup, flags, vocab_nbytes)) return XFH_ERR_INVALID_ARG;
    if (!vocab || !desc || !word || !node_of || !weight || !nodes || !bow_ids || !bow_vals || !n_words) return XFH_ERR_INVALID_ARG;
    HostStage s{c};
    auto dv = s.in<char>(vocab, vocab_nbytes);
    auto dd = s.in<float>(desc, (size_t)n * 256);
    auto dws = s.tmp<char>(transform_ws_stride(n));
    auto dw = s.out<uint32_t>(word, (size_t)n * 4), dno = s.out<uint32_t>(node_of, (size_t)n * 4), dbi = s.out<uint32_t>(bow_ids, (size_t)n * 4);
    auto dwt = s.out<double>(weight, (size_t)n * 8), dbv = s.out<double>(bow_vals, (size_t)n * 8);
    auto dn = s.out<char>(nodes, nodes_bytes(n));
    auto dnw = s.out<int>(n_words, 4);
    if (const int rc = s.upload(); rc != XFH_OK) return rc;
    const int rc = xfh_bow_transform_device(c, 1, n, levelsup, flags, dv, vocab_nbytes, dd, 0, dws, dw, dno, dwt, dn, dbi, dbv, dnw);
    if (rc != XFH_OK) return rc;                                              // (a HIP error: every argument check has passed above)
    return s.download();
}

}  // extern "C"
