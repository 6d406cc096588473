// grid_blob.h -- one well-formed frame-grid blob written by hand, for the host-side tests that feed xfh_grid_unpack (asan_window_test.cpp,
// tsan_host_test.cpp).  The offsets and the magic are the library's own (xfeatslam_amd/csrc/window_layout.h), so a change of the layout
// is followed here without an edit.  No call into the library: the size is computed from the layout constants.
#pragma once
#include <vector>
#include "../../xfeatslam_amd/csrc/window_layout.h"

static const int GRID_BLOB_N = 8;            // slots of the example blob

// n = 8 slots: slots 2, 5 in cell 0, slot 7 in cell 49, slot 0 in the last cell; 4 slots not binned
inline std::vector<unsigned char> example_grid_blob() {
    std::vector<unsigned char> blob(XFH_GRID_ITEMS_OFF + sizeof(GridItem) * (size_t)GRID_BLOB_N, 0);
    GridHeader* h = (GridHeader*)blob.data();
    int* cs = (int*)(blob.data() + XFH_GRID_CS_OFF);
    GridItem* it = (GridItem*)(blob.data() + XFH_GRID_ITEMS_OFF);
    h->magic = XFH_GRID_MAGIC; h->n = GRID_BLOB_N; h->n_binned = 4;
    for (int c = 1; c <= XFH_GRID_CELLS; ++c) cs[c] = c <= 49 ? 2 : (c < XFH_GRID_CELLS ? 3 : 4);
    const int slots[GRID_BLOB_N] = {2, 5, 7, 0, -1, -1, -1, -1};
    for (int k = 0; k < GRID_BLOB_N; ++k) it[k].index = slots[k];
    return blob;
}
