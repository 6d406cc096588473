// nodes_clamp.h -- reading a node blob (nodes_layout.h) that may hold ANYTHING: every count, range and item is clamped or checked here
// before a caller indexes with it.  Plain C++, host and device: the kernels of bow_search.hip.h and triangulation_search.hip.h read blobs through these functions only,
// and tests/cpp/asan_bow_test.cpp runs the very same lines under AddressSanitizer on heap buffers of exactly xfh_nodes_bytes(n) bytes.
//
// Every array of the blob has nodes_cap(n) >= n + 1 entries, so with the number of nodes clamped to [0, n], both ends of a range to [0, n]
// and a position < n nothing below reads outside the blob, whatever it holds.  A blob is 16-byte aligned (the entry points check).
#pragma once
#include "../../include/xfeat_hip.h"                         // XFH_NODE_NONE
#include "nodes_layout.h"

struct NodeRange { int start, len; };                       // items[start .. start + len), inside [0, n]

XFH_HD int nodes_clamp_i(int v, int n) { return v < 0 ? 0 : (v > n ? n : v); }
// the number of nodes the blob claims, clamped to [0, n]
XFH_HD int nodes_count(const char* blob, int n) { return nodes_clamp_i(((const NodesHeader*)blob)->n_nodes, n); }
// the id of node `slot`, 0 <= slot < nodes_count
XFH_HD uint32_t nodes_id(const char* blob, int n, int slot) { return ((const uint32_t*)(blob + nodes_ids_off(n)))[slot]; }
// the slot whose id is `node` among the first nn (= nodes_count) ids, or -1: lower_bound, as the reference walks its maps.  An id list
// that is not ascending makes the search miss, never leave the list.
XFH_HD int nodes_find(const char* blob, int n, int nn, uint32_t node) {
    if (node == XFH_NODE_NONE) return -1;
    const uint32_t* ids = (const uint32_t*)(blob + nodes_ids_off(n));
    int lo = 0, hi = nn;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ids[mid] < node) lo = mid + 1; else hi = mid;
    }
    return (lo < nn && ids[lo] == node) ? lo : -1;
}
// the items of node `slot`, 0 <= slot < nodes_count: both ends clamped to [0, n], an inverted range is empty
XFH_HD NodeRange nodes_range(const char* blob, int n, int slot) {
    const int32_t* ns = (const int32_t*)(blob + nodes_start_off(n));
    const int s = nodes_clamp_i(ns[slot], n), e = nodes_clamp_i(ns[slot + 1], n);
    NodeRange r;
    r.start = s; r.len = e > s ? e - s : 0;
    return r;
}
// items[pos], 0 <= pos < n: the keypoint index, or -1 when it is not one of the n keypoints
XFH_HD int nodes_item(const char* blob, int n, int pos) {
    const int idx = ((const int32_t*)(blob + nodes_items_off(n)))[pos];
    return (idx >= 0 && idx < n) ? idx : -1;
}
// node_of[i], 0 <= i < n
XFH_HD uint32_t nodes_node_of(const char* blob, int n, int i) { return ((const uint32_t*)(blob + nodes_of_off(n)))[i]; }
