// triangulation_search.hip.h -- ORBmatcher::SearchForTriangulation(KeyFrame*, KeyFrame*, vMatchedPairs, bOnlyStereo, bCoarse)
// (src/ORBmatcher.cc:1092-1331) up to vMatches12, for B keyframe pairs per launch (xfh_triangulation_search_device; the contract is
// written out in include/xfeat_hip.h).
//
//   k_triangulation_search   one wave per (problem, keypoint of KF1), four per workgroup.  The wave reads the query's flag byte, node id,
//                   coordinates and right coordinate, the pair's F12 and epipole from wave-uniform addresses and evaluates the epipolar
//                   line of tri_math.h once; the query's descriptor row comes through the scalar cache as in k_fuse_search.  The node
//                   is looked up in KF2's ascending id list by a wave-uniform binary search (nodes_clamp.h), and the node's members are dealt to the
//                   lanes 64 at a time in stored order: map-point flag, stereo gate, epipole radius and epipolar distance first
//                   (xfh_tri_member, the host's own lines), DescriptorDistance only for the survivors.  Each lane keeps ONE key
//                   dist << 32 | ~position: the reference lowers bestDist on `dist <= bestDist` (:1202 is `continue` on strictly greater),
//                   so among equal distances the member visited LAST wins -- the smallest key is the smallest distance and, inside it,
//                   the largest position; a butterfly minimum merges the lanes.  This is the opposite tie rule of k_best2_csr.
//                   The compiler may use the scalar cache only for memory the kernel has not written: TriArgs' pointers carry no
//                   noalias guarantee, so ALL stores of the kernel sit at its end, behind the last load -- keep them there.
//
// There is no order between the queries: vbMatched2 is never written in this function (:1134, :1189), so two keypoints of KF1 may name
// the same keypoint of KF2, nothing is resolved afterwards and the call needs no workspace.  With a shared side 1 the B problems read
// the same KF1 arrays (LocalMapping::CreateNewMapPoints: the new keyframe against every neighbour); its rows are then served from L2.
//
// Bounds: both blobs are read through nodes_clamp.h only -- n_nodes and both ends of a node's range are clamped to [0, n2] before they
// index anything (every array of the blob has more than n2 entries), an item is checked against n2 before has, xy, uright or a
// descriptor row is indexed with it -- and nothing is read through a float.
#pragma once
#include "ctx.h"
#include "tri_math.h"
#include "nodes_layout.h"
#include "nodes_clamp.h"
#include "search_common.hip.h"

__global__ __launch_bounds__(256)
void k_triangulation_search(TriArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int qi = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave), pb = blockIdx.y;
    const int n1 = a.s1.n, n2 = a.s2.n;
    if (qi >= n1) return;
    const size_t e1 = (size_t)pb * a.s1.elem_stride, e2 = (size_t)pb * a.s2.elem_stride;
    const size_t qg = (size_t)pb * n1 + qi;                            // the query's place in the [B][n1] outputs
    // every input of the query is read here, before the kernel's first store, from addresses that are uniform in the wave
    const char* __restrict__ nb1 = a.s1.nodes + (size_t)pb * a.s1.nodes_stride;
    const char* __restrict__ nb2 = a.s2.nodes + (size_t)pb * a.s2.nodes_stride;
    const float* __restrict__ qr = (const float*)(a.s1.desc + (size_t)pb * a.s1.desc_stride) + (size_t)qi * 64;
    const float* __restrict__ F = a.F12 + (size_t)pb * 9;
    const uint32_t node = nodes_node_of(nb1, n1, qi);
    const float x1 = a.s1.xy[(e1 + qi) * 2], y1 = a.s1.xy[(e1 + qi) * 2 + 1];
    const float ur1 = a.s1.uright ? a.s1.uright[e1 + qi] : -1.0f;
    const float ex = a.ep[(size_t)pb * 2], ey = a.ep[(size_t)pb * 2 + 1];
    const bool stereo1 = ur1 >= 0.0f;
    const TriLine l = xfh_tri_line(F, x1, y1);
    int active = a.s1.has[e1 + qi] == 0 && !((a.flags & XFH_TRI_ONLY_STEREO) && !stereo1);
    active = __builtin_amdgcn_readfirstlane(active);
    int st = XFH_TRI_INACTIVE, ncand = 0, ngeom = 0, bi = -1, bd = a.th_low;
    if (active) {                                                      // (uniform)
        st = XFH_TRI_NO_NODE;
        const int slot = nodes_find(nb2, n2, nodes_count(nb2, n2), node);                       // (uniform)
        if (slot >= 0) {
            const NodeRange nr = nodes_range(nb2, n2, slot);
            const float* __restrict__ xy2 = a.s2.xy + e2 * 2;
            const float* __restrict__ ur2 = a.s2.uright ? a.s2.uright + e2 : nullptr;
            const uint8_t* __restrict__ has2 = a.s2.has + e2;
            const char* __restrict__ tg = a.s2.desc + (size_t)pb * a.s2.desc_stride;
            u64 best = XFH_KEY_NONE;
            for (int p0 = 0; p0 < nr.len; p0 += 64) {
                const int p = p0 + lane;
                const int idx = p < nr.len ? nodes_item(nb2, n2, nr.start + p) : -1;
                int g = XFH_TRI_GATE_SKIPPED;
                if (idx >= 0 && has2[idx] == 0)                                                    // :1189
                    g = xfh_tri_member(l, ex, ey, a.epipole_r2, a.unc, a.flags, stereo1, xy2[(size_t)idx * 2], xy2[(size_t)idx * 2 + 1], ur2 ? ur2[idx] : -1.0f);
                ncand += g >= XFH_TRI_GATE_REJECTED ? 1 : 0; ngeom += g == XFH_TRI_GATE_PASSED ? 1 : 0;
                if (g == XFH_TRI_GATE_PASSED) {
                    const u64 key = key_pack(descriptor_distance(qr, (const f32x4*)(tg + (size_t)idx * 256)), 0xFFFFFFFFu - (unsigned)p);
                    best = key < best ? key : best;
                }
            }
            best = wave_min_u64(best);
            ncand = wave_sum_i32(ncand); ngeom = wave_sum_i32(ngeom);
            if (best != XFH_KEY_NONE && key_dist(best) <= a.th_low) {
                const int p = (int)(0xFFFFFFFFu - (unsigned)key_pos(best));                    // < nr.len: the position the key was made of
                bd = key_dist(best); bi = nodes_item(nb2, n2, nr.start + p);
            }
            st = bi >= 0 ? XFH_TRI_MATCHED : (ncand == 0 ? XFH_TRI_NO_CANDIDATES : XFH_TRI_REJECTED);
        }
    }
    // the only stores of the kernel, behind every load: nothing the wave reads can have been written by it
    if (lane == 0) {
        a.status[qg] = (uint8_t)st; a.match12[qg] = bi; a.best_dist[qg] = bd; a.n_candidates[qg] = ncand; a.n_geom[qg] = ngeom;
        if (st == XFH_TRI_MATCHED) atomicAdd(&a.n_matches[pb], 1);
    }
}

hipError_t launch_triangulation_search(xfh_ctx* c, const TriArgs& a, int B) {
    hipError_t e = hipMemsetAsync(a.n_matches, 0, (size_t)B * sizeof(int), c->stream);
    if (e != hipSuccess) return e;
    launch_k(c, XFH_K_TRIANGULATION_SEARCH, -1, k_triangulation_search, dim3((a.s1.n + 3) / 4, B), dim3(256), 0, a);
    return hipGetLastError();
}
