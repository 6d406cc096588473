// vocab_math.h -- TemplatedVocabulary::transform(feature, word_id, weight, nid, levelsup) (thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1218-1259)
// over a vocabulary blob (vocab_layout.h) that may hold ANYTHING.  Plain C++, host and device: k_vocab_descend (vocab_transform.hip.h) deals the
// children of a node to 16 lanes and xfh_vocab_descend (capi_vocab.cpp) walks them one after the other, both through the lines below, and
// tests/cpp/asan_vocab_test.cpp runs these very lines under AddressSanitizer on heap buffers of exactly the blob's size.
//
// The feature is 8 uint32: the bit patterns of the first 8 floats of an XFeat row, which DBoW2 reads as a 256-bit ORB descriptor (SURVEY.md Q8;
// FORB::distance, FORB.cpp:81-101, popcounts the XOR of the first 8 int32 of the row).  The floats are never touched as floats.
//
// Descent: from the root, level by level, to the FIRST child with the strictly least distance (`d < best_d` over the children in order =
// the least key d << 8 | position), until a node without children.  nid_level = L - levelsup; the node id is 0 when nid_level <= 0, the
// path's node at level nid_level when the path is that long, otherwise the leaf (the reference leaves *nid uninitialised in that case,
// TemplatedVocabulary.h:1150-1155, 1251: a documented deviation).
//
// Bounds: the node count a blob claims is clamped to what fits its byte count (vocab_open); a slot's first child is clamped to [0, n - 1] and
// its child count to min(XFH_VOCAB_MAX_CHILDREN, n - first) before either indexes anything (vocab_slot); a walk takes at most
// XFH_VOCAB_MAX_DEPTH steps.  So a hostile blob can neither leave the buffer nor loop forever; what it yields is unspecified.
#pragma once
#include "../../include/xfeat_hip.h"                         // XFH_VOCAB_MAX_CHILDREN, XFH_VOCAB_MAX_DEPTH
#include "vocab_layout.h"
#include <string.h>

#define XFH_VOCAB_KEY_NONE 0xFFFFFFFFu                       // larger than every child key

struct VocabView { const char* blob; uint32_t n; int L; };  // n >= 1 nodes readable, L clamped to [0, XFH_VOCAB_MAX_DEPTH]

// 16 bytes of the blob as four words (on the device one 16-byte load: every array of a 16-byte aligned blob starts on 16 bytes)
XFH_HD void vocab_load16(const char* p, uint32_t w[4]) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 v = *(const u32x4*)p;
    w[0] = v[0]; w[1] = v[1]; w[2] = v[2]; w[3] = v[3];
#else
    memcpy(w, p, 16);
#endif
}

// false: the buffer cannot hold one node
XFH_HD bool vocab_open(const void* blob, size_t nbytes, VocabView* v) {
    const size_t fit = vocab_fit(nbytes);
    if (fit < 1) return false;
    uint32_t h[4];
    vocab_load16((const char*)blob, h);                      // magic, n_nodes, L, max_children
    const int32_t n = (int32_t)h[1], L = (int32_t)h[2];
    v->blob = (const char*)blob;
    v->n = n < 1 ? 1u : ((size_t)n > fit ? (uint32_t)fit : (uint32_t)n);
    v->L = L < 0 ? 0 : (L > XFH_VOCAB_MAX_DEPTH ? XFH_VOCAB_MAX_DEPTH : L);
    return true;
}

// slot s < v.n, its child range clamped: first <= n - 1, first + nch <= n, nch <= XFH_VOCAB_MAX_CHILDREN
XFH_HD VocabSlot vocab_slot(const VocabView& v, uint32_t s) {
    uint32_t w[4];
    vocab_load16(v.blob + vocab_slot_off(v.n) + 16 * (size_t)s, w);
    VocabSlot e;
    e.first = w[0] < v.n ? w[0] : v.n - 1;
    const uint32_t room = v.n - e.first, cap = room < XFH_VOCAB_MAX_CHILDREN ? room : XFH_VOCAB_MAX_CHILDREN;
    e.nch = w[1] < cap ? w[1] : cap;
    e.node_id = w[2]; e.word_id = w[3];
    return e;
}

XFH_HD double vocab_weight(const VocabView& v, uint32_t s) {
    const char* p = v.blob + vocab_weight_off(v.n) + 8 * (size_t)s;
#if defined(__HIP_DEVICE_COMPILE__)
    return *(const double*)p;
#else
    double w;
    memcpy(&w, p, 8);
    return w;
#endif
}

// child c < e.nch of a slot whose children start at `first`: d << 8 | c, d = FORB::distance(feature, the child's descriptor)
XFH_HD uint32_t vocab_child_key(const VocabView& v, uint32_t first, uint32_t c, const uint32_t q[8]) {
    const char* row = v.blob + vocab_desc_off(v.n) + XFH_VOCAB_ROW * (size_t)(first + c);
    uint32_t a[4], b[4];
    vocab_load16(row, a); vocab_load16(row + 16, b);
    uint32_t d = 0;
    for (int k = 0; k < 4; ++k) d += (uint32_t)__builtin_popcount(a[k] ^ q[k]) + (uint32_t)__builtin_popcount(b[k] ^ q[4 + k]);
    return (d << 8) | c;
}

// the bookkeeping of one walk: where it stands, and the node id at nid_level once the path has reached it
struct VocabWalk { uint32_t slot, nid; int level, nid_level; bool have; };

XFH_HD VocabWalk vocab_walk_begin(int L, int levelsup) {
    VocabWalk w;
    w.slot = 0; w.nid = 0; w.level = 0;
    w.nid_level = L - (levelsup < 0 ? 0 : (levelsup > 2 * XFH_VOCAB_MAX_DEPTH ? 2 * XFH_VOCAB_MAX_DEPTH : levelsup));
    w.have = w.nid_level <= 0;                                // `if(nid_level <= 0 && nid != NULL) *nid = 0; // root` (:1228)
    return w;
}
// the walk stands on slot entry e (:1250-1251)
XFH_HD void vocab_walk_enter(VocabWalk& w, const VocabSlot& e) {
    if (w.level > 0 && w.level == w.nid_level) { w.nid = e.node_id; w.have = true; }
}
// ... and goes on to the child the least key names
XFH_HD void vocab_walk_take(VocabWalk& w, const VocabSlot& e, uint32_t key) { w.slot = e.first + (key & 0xFFu); ++w.level; }
XFH_HD bool vocab_walk_stops(const VocabSlot& e, int steps) { return e.nch == 0 || steps >= XFH_VOCAB_MAX_DEPTH; }
XFH_HD uint32_t vocab_walk_node(const VocabWalk& w, const VocabSlot& leaf) { return w.have ? w.nid : leaf.node_id; }
// `if(w > 0) // not stopped` (:1152): a weight of 0, below 0 or NaN stops the feature
XFH_HD bool vocab_stopped(double weight) { return !(weight > 0.0); }

// one feature, the children one after the other
XFH_HD void vocab_descend_row(const VocabView& v, int levelsup, const uint32_t q[8], uint32_t* word, uint32_t* node, double* weight) {
    VocabWalk w = vocab_walk_begin(v.L, levelsup);
    VocabSlot e = vocab_slot(v, 0);
    for (int steps = 0;; ++steps) {
        vocab_walk_enter(w, e);
        if (vocab_walk_stops(e, steps)) break;
        uint32_t key = XFH_VOCAB_KEY_NONE;
        for (uint32_t c = 0; c < e.nch; ++c) { const uint32_t k = vocab_child_key(v, e.first, c, q); key = k < key ? k : key; }
        vocab_walk_take(w, e, key);
        e = vocab_slot(v, w.slot);
    }
    *word = e.word_id; *node = vocab_walk_node(w, e); *weight = vocab_weight(v, w.slot);
}

// the arguments of the two kernels of vocab_transform.hip.h, filled by xfh_bow_transform_device (capi_vocab.cpp)
struct VocabArgs {
    const char* vocab; size_t vocab_bytes;
    int n, levelsup;
    const char* desc; size_t desc_stride;
    char* ws; size_t ws_stride;                                        // per frame: double raw[n], the values before normalisation
    uint32_t* word; uint32_t* node_of; double* weight;                 // [B][n]
    char* nodes;                                                       // [B] blobs of nodes_bytes(n)
    uint32_t* bow_ids; double* bow_vals; int* n_words;                 // [B][n], [B][n], [B]
};
