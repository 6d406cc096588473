// vocab_layout.h -- the vocabulary blob of xfh_vocab_pack / xfh_bow_transform_device (plain C++: the kernels in vocab_transform.hip.h, the
// descent in vocab_math.h and the host writer / reader in capi_vocab.cpp share it).
//
// A DBoW2 vocabulary is m_nodes in node-id order: parent, word id, weight and the 32 descriptor bytes (FORB::L) of every node; node 0 is the
// root.  CONTRACT: the children of a node are the nodes that name it as parent, in ascending id -- the order in which loadFromTextFile
// push_backs them (TemplatedVocabulary.h:1385-1392) and the order in which transform() walks them.  A node is a leaf iff it has no children
// (isLeaf()), whatever its word id.
//
// The blob reorders the nodes into SLOTS, breadth first: slot 0 is the root and the children of a slot are consecutive slots in child order,
// so the descriptors of one node's children are one contiguous run of 32-byte rows.  n = the number of nodes:
//   VocabHeader            64 bytes: magic, n_nodes, L, max_children, depth
//   VocabSlot  slot[n]     16 bytes each: first_child_slot, n_children, node_id, word_id
//   double     weight[n]   by slot
//   (padding to a multiple of 32 bytes)
//   uint8      desc[n][32] by slot: row s is the descriptor of slot s (the root's row is zero)
// Unused bytes are zero: packing the same input twice gives identical bytes.  Every offset is a function of n alone, and vocab_bytes is
// monotone in n: a reader that clamps the n a blob claims to vocab_fit(nbytes) stays inside nbytes whatever the blob holds.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "hd.h"

#define XFH_VOCAB_MAGIC 0x31564658                          // "XFV1"
#define XFH_VOCAB_HDR 64
#define XFH_VOCAB_ROW 32                                    // FORB::L: descriptor bytes of a node

struct VocabHeader { int32_t magic, n_nodes, L, max_children, depth; int32_t pad[11]; };
static_assert(sizeof(VocabHeader) == XFH_VOCAB_HDR, "vocabulary header is 64 bytes");
struct VocabSlot { uint32_t first, nch, node_id, word_id; };
static_assert(sizeof(VocabSlot) == 16, "a vocabulary slot is 16 bytes");

XFH_HD size_t vocab_slot_off(size_t) { return XFH_VOCAB_HDR; }
XFH_HD size_t vocab_weight_off(size_t n) { return XFH_VOCAB_HDR + 16 * n; }
XFH_HD size_t vocab_desc_off(size_t n) { return (XFH_VOCAB_HDR + 24 * n + 31) & ~(size_t)31; }
XFH_HD size_t vocab_bytes(size_t n) { return vocab_desc_off(n) + XFH_VOCAB_ROW * n; }
// the largest n with vocab_bytes(n) <= nbytes (0: not even a header)
XFH_HD size_t vocab_fit(size_t nbytes) {
    if (nbytes < XFH_VOCAB_HDR) return 0;
    size_t n = (nbytes - XFH_VOCAB_HDR) / 56;               // 56 bytes per node plus at most 24 of padding: at most one too many
    while (n > 0 && vocab_bytes(n) > nbytes) --n;
    return n;
}
