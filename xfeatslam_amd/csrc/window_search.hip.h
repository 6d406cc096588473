// window_search.hip.h -- the frame grid in device memory and the windowed best / second-best search.
//
//   k_grid_build    : Frame::AssignFeaturesToGrid (src/Frame.cc:569-599) with Frame::PosInGrid (:918-929) for B frames per launch,
//                     one workgroup per frame, into the blob of window_layout.h.
//   k_search_window : Frame::GetFeaturesInArea (:850-916) fused with the best / second-best loop of ORBmatcher::SearchByProjection
//                     (src/ORBmatcher.cc:1925-1955, :82-119): one wave per query, no candidate list is ever materialised.
//
// Everything here is integer-exact against the reference's fp32 expressions (the library is built with -ffp-contract=off, so
// (x - min_x) * inv_w is a subtraction and a multiplication as written).
#pragma once
#include "ctx.h"
#include "window_layout.h"
#include "search_common.hip.h"

// ---- k_grid_build ---------------------------------------------------------------------------------------------------------
// Every slot gets the key (cell << 20 | slot) -- slots that PosInGrid drops (:925) or that the caller leaves out get the largest
// key -- and the keys are sorted in LDS (bitonic, like k_select's candidate keys): ascending key = cell order, and inside a cell
// ascending slot number, which is the reference's push_back order.  A sort costs the same whatever the distribution is: in the
// faithful mode every padding slot is a default cv::KeyPoint() at (0, 0) and lands in cell (0, 0) (N = mvKeys.size(), Frame.cc:318),
// hundreds of them, so anything that orders a cell's members by one thread serialises on that cell.  cell_start falls out of the
// sorted keys (position p opens every cell in (cell(p - 1), cell(p)]), no histogram is needed.  The result is a pure function
// of the input: two builds give identical bytes.
#define XFH_GRID_DROPPED 0xFFFFFFFFu
#define XFH_GRID_BUILD_THREADS 1024
// valid slots of a record: [0, mono_index) and [n - (n_valid - mono_index), n) (xfh_match_records_device); all of them otherwise
__device__ __forceinline__ void grid_valid_slots(const char* hdr, size_t hdr_stride, int f, int n, int flags, int& lo_end, int& hi_beg) {
    lo_end = n; hi_beg = n;
    if (hdr && (flags & XFH_GRID_SKIP_PADDING)) {
        const int* h = (const int*)(hdr + (size_t)f * hdr_stride);
        int nv = h[0], mono = h[1];
        nv = nv < 0 ? 0 : (nv > n ? n : nv); mono = mono < 0 ? 0 : (mono > nv ? nv : mono);
        lo_end = mono; hi_beg = n - (nv - mono);
    }
}
// the key of slot i at (x, y): cell << 20 | slot, or XFH_GRID_DROPPED when PosInGrid drops it
__device__ __forceinline__ unsigned grid_key(float x, float y, int i, const GridGeom& g) {
    const float fx = roundf((x - g.min_x) * g.inv_w);                  // posX = round((kp.pt.x - mnMinX) * mfGridElementWidthInv), :920
    const float fy = roundf((y - g.min_y) * g.inv_h);
    // posX < 0 || posX >= FRAME_GRID_COLS || ... -> not binned (:925); decided on the float, so a non-finite or huge value never reaches the conversion
    if (fx >= 0.0f && fx < (float)XFH_GRID_COLS && fy >= 0.0f && fy < (float)XFH_GRID_ROWS)
        return ((unsigned)((int)fx * XFH_GRID_ROWS + (int)fy) << 20) | (unsigned)i;
    return XFH_GRID_DROPPED;
}
// bitonic network over the P keys in LDS (all XFH_GRID_BUILD_THREADS threads; the caller has put a barrier behind the keys).
// Steps with a partner distance j >= 64 cross waves and end in a workgroup barrier; for j <= 32 the 64 pairs of a
// wave (t = 64 w .. 64 w + 63) touch exactly the keys [128 w, 128 w + 128) at every such j, so the steps j = 32 .. 1 of a stage run
// inside the wave, ordered by a wave-level fence only (27 workgroup barriers instead of 78 at 4096 slots).
__device__ __forceinline__ void grid_sort(unsigned* gkeys, int P, int tid) {
    auto exchange = [&](int t, int j, int k) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const unsigned a = gkeys[i], b = gkeys[l];
        if ((a > b) == ((i & k) == 0)) { gkeys[i] = b; gkeys[l] = a; }
    };
    for (int k = 2; k <= P; k <<= 1) {
        int j = k >> 1;
        for (; j >= 64; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += XFH_GRID_BUILD_THREADS) exchange(t, j, k);
            __syncthreads();
        }
        for (int t = tid; t < (P >> 1); t += XFH_GRID_BUILD_THREADS)
            for (int jj = j; jj > 0; jj >>= 1) {
                exchange(t, jj, k);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        __syncthreads();
    }
}
// the blob of one frame from its sorted keys; xy[2 * slot], xy[2 * slot + 1] (stride_floats apart per slot) are the coordinates the keys were made of
__device__ __forceinline__ void grid_emit(char* grid, const unsigned* gkeys, const float* xy, int stride_floats, int n, int P, const GridGeom& g, int flags, int tid) {
    int* cs = (int*)(grid + XFH_GRID_CS_OFF);
    GridItem* items = (GridItem*)(grid + XFH_GRID_ITEMS_OFF);
    GridHeader* gh = (GridHeader*)grid;
    for (int p = tid; p <= P; p += XFH_GRID_BUILD_THREADS) {
        const unsigned key = p < P ? gkeys[p] : XFH_GRID_DROPPED;
        const int cell = (int)(key >> 20), prev = p > 0 ? (int)(gkeys[p - 1] >> 20) : -1;
        const int last = cell < XFH_GRID_CELLS ? cell : XFH_GRID_CELLS;
        for (int c = prev + 1; c <= last; ++c) cs[c] = p;                     // (a dropped predecessor has cell 4095: no iteration)
        if (prev < XFH_GRID_CELLS && last == XFH_GRID_CELLS) gh->n_binned = p; // exactly one p: the first key past the binned ones
        if (p < n) {
            GridItem it = {-1, 0.0f, 0.0f, 0};
            if (cell < XFH_GRID_CELLS) {
                const int idx = (int)(key & 0xFFFFFu);
                it.index = idx; it.x = xy[(size_t)idx * stride_floats]; it.y = xy[(size_t)idx * stride_floats + 1];
            }
            items[p] = it;
        }
    }
    if (tid == 0) {
        gh->magic = XFH_GRID_MAGIC; gh->n = n; gh->flags = flags;
        gh->min_x = g.min_x; gh->min_y = g.min_y; gh->max_x = g.max_x; gh->max_y = g.max_y; gh->inv_w = g.inv_w; gh->inv_h = g.inv_h;
        for (int k = 0; k < 6; ++k) gh->pad[k] = 0;
    }
    for (int c = XFH_GRID_CELLS + 1 + tid; c < XFH_GRID_CS_SLOTS; c += XFH_GRID_BUILD_THREADS) cs[c] = 0;
}

__global__ __launch_bounds__(XFH_GRID_BUILD_THREADS)
void k_grid_build(const char* __restrict__ kps, size_t kps_stride, const char* __restrict__ hdr, size_t hdr_stride,
                  char* __restrict__ grids, size_t grid_stride, int n, int P, GridGeom g, int flags) {
    extern __shared__ unsigned gkeys[];                    // P keys, P = power of two >= max(n, 2)
    const int f = blockIdx.x, tid = threadIdx.x;
    const xfh_keypoint* kp = (const xfh_keypoint*)(kps + (size_t)f * kps_stride);
    int lo_end, hi_beg;
    grid_valid_slots(hdr, hdr_stride, f, n, flags, lo_end, hi_beg);
    for (int i = tid; i < P; i += XFH_GRID_BUILD_THREADS) {
        unsigned key = XFH_GRID_DROPPED;
        if (i < n && (i < lo_end || i >= hi_beg)) key = grid_key(kp[i].x, kp[i].y, i, g);
        gkeys[i] = key;
    }
    __syncthreads();
    grid_sort(gkeys, P, tid);
    grid_emit(grids + (size_t)f * grid_stride, gkeys, (const float*)kp, (int)(sizeof(xfh_keypoint) / sizeof(float)), n, P, g, flags, tid);
}

hipError_t launch_grid_build(xfh_ctx* c, const void* kps, size_t kps_stride, const void* hdr, size_t hdr_stride, void* grids, size_t grid_stride,
                             int n, int B, const GridGeom& g, int flags) {
    if (B <= 0) return hipSuccess;
    int P = 2;
    while (P < n) P <<= 1;
    launch_k(c, XFH_K_GRID_BUILD, -1, k_grid_build, dim3(B), dim3(XFH_GRID_BUILD_THREADS), (size_t)P * sizeof(unsigned), (const char*)kps, kps_stride,
             (const char*)hdr, hdr_stride, (char*)grids, grid_stride, n, P, g, flags);
    return hipGetLastError();
}

// ---- k_search_window ------------------------------------------------------------------------------------------------------
// One wave per query, four per workgroup, the query row through the scalar cache, (dist << 32 | position) keys and the butterfly
// merge of search_common.hip.h, as k_best2_csr; the candidate list is replaced by the grid walk.  With cell = ix * 48 + iy the cells c0y .. c1y of column
// ix are ONE contiguous range of items, so the reference's visiting order (ix outer, iy inner, cell order inside, :884-911) is
// the concatenation of at most 64 ranges: lane c takes column c0x + c, a wave scan of the range lengths gives every column its
// first position, and position p of the walk is item adj[col(p)] + p.  Lanes are dealt positions of that walk (all members of
// the visited cells), test |x - u| < r && |y - v| < r (:907, strict), the skip mask (ORBmatcher.cc:1931-1933) and the
// right-coordinate check (:1935-1941), and only survivors compute DescriptorDistance.  The key keeps the position in the walk
// (filtering preserves order), so "first visited wins a tie" is the smallest key -- NOT the lowest slot number.
// Octaves: every XFeat keypoint has octave 0 and every level window the reference passes contains 0, so bCheckLevels (:880,
// :896-903) never rejects; it is not part of the interface.
// Out-of-contract floats: a query with a non-finite u, v or r has no candidates; the cell bounds are clamped as floats before the
// conversion to int; every range is clamped to [0, nt] and every slot number is checked against nt, so no load leaves the blob
// or the target rows whatever the query holds.
// The walk is written once, as device functions, for k_search_window and the kernels of projection_search.hip.h:
//   window_open   the cell bounds of (u, v, r), lane = column: its range of items and its first position in the walk
//   window_walk   deals the positions to the lanes, applies the window test and the static filters plus the caller's `extra(slot, x, y)`
//                 (x, y: the item's coordinates),
//                 and calls visit(key, slot) for every survivor with key = dist << 32 | position (DIST = false: no descriptor is
//                 read and the key's distance is 0; SAT = true: a distance the conversion cannot hold is INT_MAX); returns the number of
//                 survivors of the whole wave
//   window_count  the walk without descriptors: the window members this lane was dealt
//   window_slot   the slot number at a position of the walk
//   window_best2  the wave's two smallest keys (wave_top2) under the reference's initial values (k_best2_csr's rule), and their slots
struct WindowWalk { int ncols, first, adj, T; };            // first / adj: of this lane's column; item = adj + position

__device__ __forceinline__ WindowWalk window_open(const char* __restrict__ grid, float u, float v, float r, int nt, int lane) {
    const GridHeader* gh = (const GridHeader*)grid;
    const int* cs = (const int*)(grid + XFH_GRID_CS_OFF);
    const float min_x = gh->min_x, min_y = gh->min_y, inv_w = gh->inv_w, inv_h = gh->inv_h;
    int c0x = 0, c1x = -1, c0y = 0, c1y = -1;
    if (__builtin_isfinite(u) && __builtin_isfinite(v) && __builtin_isfinite(r)) {
        // nMinCellX = max(0, (int)floor((x - mnMinX - factorX) * mfGridElementWidthInv)) ... (:858-880); fminf / fmaxf also swallow a NaN
        const float fx0 = fminf(fmaxf(floorf((u - min_x - r) * inv_w), -1.0f), (float)XFH_GRID_COLS);
        const float fx1 = fminf(fmaxf(ceilf((u - min_x + r) * inv_w), -1.0f), (float)XFH_GRID_COLS);
        const float fy0 = fminf(fmaxf(floorf((v - min_y - r) * inv_h), -1.0f), (float)XFH_GRID_ROWS);
        const float fy1 = fminf(fmaxf(ceilf((v - min_y + r) * inv_h), -1.0f), (float)XFH_GRID_ROWS);
        const int a0 = (int)fx0 < 0 ? 0 : (int)fx0, a1 = (int)fx1 > XFH_GRID_COLS - 1 ? XFH_GRID_COLS - 1 : (int)fx1;
        const int b0 = (int)fy0 < 0 ? 0 : (int)fy0, b1 = (int)fy1 > XFH_GRID_ROWS - 1 ? XFH_GRID_ROWS - 1 : (int)fy1;
        if (a0 < XFH_GRID_COLS && a1 >= 0 && b0 < XFH_GRID_ROWS && b1 >= 0) { c0x = a0; c1x = a1; c0y = b0; c1y = b1; }   // else: the early returns
    }
    WindowWalk w;
    w.ncols = (c1x >= c0x && c1y >= c0y) ? c1x - c0x + 1 : 0;
    // lane = column: its range of items, and an inclusive scan of the lengths
    int beg = 0, len = 0;
    if (lane < w.ncols) {
        const int col = (c0x + lane) * XFH_GRID_ROWS;
        int s = cs[col + c0y], e = cs[col + c1y + 1];
        s = s < 0 ? 0 : (s > nt ? nt : s); e = e < 0 ? 0 : (e > nt ? nt : e);
        beg = s; len = e > s ? e - s : 0;
    }
    int inc = len;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(inc, d); if (lane >= d) inc += t; }
    w.first = inc - len; w.adj = beg - w.first;            // column's first position in the walk; item = adj + position
    w.T = __builtin_amdgcn_readlane(inc, 63);
    return w;
}

// the last column whose first position is <= p holds p (empty columns repeat a value)
__device__ __forceinline__ int window_base(const WindowWalk& w, int p) {
    int a = 0;
    for (int c = 0; c < w.ncols; ++c) {
        const int fc = __builtin_amdgcn_readlane(w.first, c), ac = __builtin_amdgcn_readlane(w.adj, c);
        a = p >= fc ? ac : a;
    }
    return a;
}
__device__ __forceinline__ int window_slot(const WindowWalk& w, const char* __restrict__ grid, int p) {
    return ((const GridItem*)(grid + XFH_GRID_ITEMS_OFF))[window_base(w, p) + p].index;
}

template <bool DIST, bool SAT = false, typename Extra, typename Visit>
__device__ __forceinline__ int window_walk(const WindowWalk& w, const char* __restrict__ grid, const float* __restrict__ qr, float u, float v, float r,
                                           const float* __restrict__ tg, int nt, const uint8_t* __restrict__ skip, const float* __restrict__ uright,
                                           float urq, int lane, Extra extra, Visit visit) {
    const GridItem* items = (const GridItem*)(grid + XFH_GRID_ITEMS_OFF);
    int ncand = 0;
    for (int p0 = 0; p0 < w.T; p0 += 64) {
        const int p = p0 + lane;
        const int a = window_base(w, p);
        bool pass = false;
        int idx = 0;
        if (p < w.T) {
            const GridItem it = items[a + p];
            idx = it.index;
            pass = idx >= 0 && idx < nt && fabsf(it.x - u) < r && fabsf(it.y - v) < r;               // Frame.cc:904-908
            if (pass && skip) pass = skip[idx] == 0;                                                   // ORBmatcher.cc:1931-1933
            if (pass && uright) { const float ur = uright[idx]; if (ur > 0.0f && fabsf(urq - ur) > r) pass = false; }   // :1935-1941
            if (pass) pass = extra(idx, it.x, it.y);
        }
        ncand += __popcll(__ballot(pass));
        if (pass) {
            const int dist = DIST ? descriptor_distance<SAT>(qr, (const f32x4*)(tg + (size_t)idx * 64)) : 0;
            visit(key_pack(dist, (unsigned)p), idx);
        }
    }
    return ncand;
}

// the members of the window (u, v, r) THIS LANE was dealt, whatever else they are: no descriptor is read
__device__ __forceinline__ int window_count(const WindowWalk& w, const char* __restrict__ grid, float u, float v, float r, int nt, int lane) {
    int n = 0;
    window_walk<false>(w, grid, nullptr, u, v, r, nullptr, nt, nullptr, nullptr, 0.0f, lane, [&](int, float, float) { ++n; return false; }, [](u64, int) {});
    return n;
}

// every lane gets the merged pair of the wave; the reference's initial values: a candidate only counts if dist < init_dist (k_best2_csr)
__device__ __forceinline__ void window_best2(const WindowWalk& w, const char* __restrict__ grid, u64 b, u64 s2, int init_dist,
                                             int& bi, int& bd, int& si, int& sd) {
    wave_top2(b, s2);
    const bool hb = b != XFH_KEY_NONE && key_dist(b) < init_dist, hs = hb && s2 != XFH_KEY_NONE && key_dist(s2) < init_dist;
    const int wb = hb ? key_pos(b) : 0, ws = hs ? key_pos(s2) : 0;
    // the items of the two winning positions (window_base for both in one pass over the columns)
    int pb = 0, ps = 0;
    for (int c = 0; c < w.ncols; ++c) {
        const int fc = __builtin_amdgcn_readlane(w.first, c), ac = __builtin_amdgcn_readlane(w.adj, c);
        pb = wb >= fc ? ac : pb; ps = ws >= fc ? ac : ps;
    }
    const GridItem* items = (const GridItem*)(grid + XFH_GRID_ITEMS_OFF);
    bd = init_dist; bi = -1; sd = init_dist; si = -1;
    if (hb) { bd = key_dist(b); bi = items[pb + wb].index; }
    if (hs) { sd = key_dist(s2); si = items[ps + ws].index; }
}

__global__ __launch_bounds__(256)
void k_search_window(const float* __restrict__ q, const float* __restrict__ uvr, int nq, const char* __restrict__ grid,
                     const float* __restrict__ tg, int nt, const uint8_t* __restrict__ skip, const float* __restrict__ uright,
                     const float* __restrict__ ur_query, int init_dist, int* __restrict__ best_idx, int* __restrict__ best_dist,
                     int* __restrict__ second_idx, int* __restrict__ second_dist, int* __restrict__ n_candidates) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int qi = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave);
    if (qi >= nq) return;
    const float* qr = q + (size_t)qi * 64;
    const float u = uvr[(size_t)qi * 3], v = uvr[(size_t)qi * 3 + 1], r = uvr[(size_t)qi * 3 + 2];
    const float urq = ur_query ? ur_query[qi] : 0.0f;
    const WindowWalk w = window_open(grid, u, v, r, nt, lane);
    u64 b = XFH_KEY_NONE, s2 = XFH_KEY_NONE;
    const int ncand = window_walk<true>(w, grid, qr, u, v, r, tg, nt, skip, uright, urq, lane, [](int, float, float) { return true; },
                                        [&](u64 key, int) { top2_insert(b, s2, key); });
    int bi, bd, si, sd;
    window_best2(w, grid, b, s2, init_dist, bi, bd, si, sd);
    if (lane == 0) { best_idx[qi] = bi; best_dist[qi] = bd; second_idx[qi] = si; second_dist[qi] = sd; n_candidates[qi] = ncand; }
}

hipError_t launch_search_window(xfh_ctx* c, const float* q, const float* uvr, int nq, const void* grid, const float* tg, int nt,
                                const uint8_t* skip, const float* uright, const float* ur_query, int init_dist,
                                int* best_idx, int* best_dist, int* second_idx, int* second_dist, int* n_candidates) {
    if (nq <= 0) return hipSuccess;
    launch_k(c, XFH_K_SEARCH_WINDOW, -1, k_search_window, dim3((nq + 3) / 4), dim3(256), 0, q, uvr, nq, (const char*)grid, tg, nt, skip, uright, ur_query,
             init_dist, best_idx, best_dist, second_idx, second_dist, n_candidates);
    return hipGetLastError();
}
