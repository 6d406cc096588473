// window_layout.h -- the frame-grid blob of xfh_grid_build_device / xfh_search_window_device (plain C++: the kernels in
// window_search.hip.h and the host reader xfh_grid_unpack in capi_search.cpp share it).
//
// One blob per frame, xfh_grid_bytes(n) bytes, self-contained (the search kernel needs no pointer into the record):
//   GridHeader          64 bytes: magic, n, n_binned, flags, the bounds and the inverse cell sizes (Frame.cc:336-341)
//   int cell_start[]    XFH_GRID_CELLS + 1 entries (padded to 3088): cell = ix * 48 + iy -- the cells c0y..c1y of one column of
//                       Frame::GetFeaturesInArea's walk (Frame.cc:884-886, ix outer, iy inner) are one contiguous range of items
//   GridItem items[n]   in cell order, inside a cell in ascending slot order (push_back order, Frame.cc:585-597): slot number and
//                       the keypoint's coordinates, 16 bytes = one load per candidate.  Entries [n_binned, n) are {-1, 0, 0, 0}.
#pragma once
#include <stdint.h>
#include "../../include/xfeat_hip.h"

#define XFH_GRID_CELLS (XFH_GRID_COLS * XFH_GRID_ROWS)      // 3072
#define XFH_GRID_MAGIC 0x31474658                           // "XFG1"
#define XFH_GRID_CS_OFF 64
#define XFH_GRID_CS_SLOTS 3088                              // 3073 used
#define XFH_GRID_ITEMS_OFF (XFH_GRID_CS_OFF + XFH_GRID_CS_SLOTS * 4)   // 12416, a multiple of 64

struct GridHeader {
    int32_t magic, n, n_binned, flags;
    float min_x, min_y, max_x, max_y, inv_w, inv_h;
    int32_t pad[6];
};
static_assert(sizeof(GridHeader) == XFH_GRID_CS_OFF, "grid header is 64 bytes");
struct GridItem { int32_t index; float x, y; int32_t pad; };
static_assert(sizeof(GridItem) == 16, "one 16-byte load per candidate");

// kernel arguments of the geometry: the caller's bounds and 64 / (max_x - min_x), 48 / (max_y - min_y) in fp32
struct GridGeom { float min_x, min_y, max_x, max_y, inv_w, inv_h; };
