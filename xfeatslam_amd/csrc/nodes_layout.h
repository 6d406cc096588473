// nodes_layout.h -- the node-index blob of xfh_nodes_pack / xfh_triangulation_search_device (plain C++: the kernel in
// triangulation_search.hip.h and the host writer / reader in capi_triangulation.cpp share it).
//
// A DBoW2 feature vector (FeatureVector = map<NodeId, vector<unsigned>>: TemplatedVocabulary::transform visits the features in
// ascending index and addFeature push_backs) is "node id ascending, keypoint index ascending inside a node": a function of node_of[i],
// the NodeId of keypoint i.  One blob per keyframe, xfh_nodes_bytes(n) bytes, self-contained, with cap = (n + 4) & ~3 entries per array:
//   NodesHeader            64 bytes: magic, n, n_nodes, n_items
//   uint32 node_ids[cap]   the n_nodes distinct ids, ascending
//   int32  node_start[cap] n_nodes + 1 entries: node k owns items[node_start[k] .. node_start[k + 1])
//   int32  items[cap]      n_items keypoint indices: nodes in id order, ascending index inside a node
//   uint32 node_of[cap]    the caller's array (XFH_NODE_NONE: the keypoint is in no node and in no item)
// Unused entries are zero: packing the same input twice gives identical bytes.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "hd.h"

#define XFH_NODES_MAGIC 0x314e4658                          // "XFN1"
#define XFH_NODES_HDR 64

struct NodesHeader { int32_t magic, n, n_nodes, n_items; int32_t pad[12]; };
static_assert(sizeof(NodesHeader) == XFH_NODES_HDR, "nodes header is 64 bytes");

XFH_HD size_t nodes_cap(int n) { return ((size_t)n + 4) & ~(size_t)3; }                   // >= n + 1, a multiple of 4: every array starts on 16 bytes
XFH_HD size_t nodes_ids_off(int) { return XFH_NODES_HDR; }
XFH_HD size_t nodes_start_off(int n) { return XFH_NODES_HDR + 4 * nodes_cap(n); }
XFH_HD size_t nodes_items_off(int n) { return XFH_NODES_HDR + 8 * nodes_cap(n); }
XFH_HD size_t nodes_of_off(int n) { return XFH_NODES_HDR + 12 * nodes_cap(n); }
XFH_HD size_t nodes_bytes(int n) { return XFH_NODES_HDR + 16 * nodes_cap(n); }
