// frame_finish.hip.h -- what the reference's RGB-D Frame constructor does between ExtractXF and the first search
// (src/Frame.cc:311-374), for B extraction records per launch, device resident.
//
//   k_frame_finish : Frame::UndistortKeyPoints (:940-973) + Frame::ComputeStereoFromRGBD (:1177-1198) + Frame::AssignFeaturesToGrid
//                    (:569-599) on mvKeysUn, one workgroup per frame.  It is k_grid_build (window_search.hip.h) with another key
//                    computation: the thread that is about to bin slot i undistorts it first (frame_math.h: float64, five
//                    iterations), stores xy_un / depth / uright of the slot, and makes the key of the UNDISTORTED point; sort and
//                    blob are k_grid_build's own code, and the items carry the undistorted coordinates, so xfh_grid_unpack and
//                    k_search_window take the blob as it is.  No launch is added to extract -> grid -> search.  Without a grid
//                    (d_grids = NULL) the same kernel runs as n / 256 small workgroups per frame and stops after the side arrays.
//
// All n slots are processed, padding at (0, 0) included (N = mvKeys.size(), Frame.cc:318): XFH_GRID_SKIP_PADDING only keeps a slot
// out of the grid, its side arrays are written like everyone's.  Bounds: slot numbers are < n by construction; the depth image is
// read only where xfh_depth_sample has found the pixel inside it; a non-finite undistorted coordinate fails grid_key's cell test
// and is not binned.  Nothing is read through a float.
#pragma once
#include "ctx.h"
#include "frame_math.h"
#include "window_search.hip.h"

struct FinishDepth {                // the depth images of the batch: frame f at base + f * frame_stride, rows `pitch` bytes apart
    const char* base; size_t frame_stride, pitch; int type; float scale;
};

__global__ __launch_bounds__(XFH_GRID_BUILD_THREADS)
void k_frame_finish(const char* __restrict__ kps, size_t kps_stride, const char* __restrict__ hdr, size_t hdr_stride, xfh_camera cam, FinishDepth dp,
                    float* xy_un, float* __restrict__ uright, float* __restrict__ depth, char* grids, size_t grid_stride,
                    int n, int P, GridGeom g, int flags) {
    extern __shared__ unsigned gkeys[];                    // P keys when a grid is built, nothing otherwise
    const int f = blockIdx.x, tid = threadIdx.x;
    const xfh_keypoint* kp = (const xfh_keypoint*)(kps + (size_t)f * kps_stride);
    float* xu = xy_un + (size_t)f * n * 2;
    float* ur = uright + (size_t)f * n;
    float* dz = depth + (size_t)f * n;
    const char* img = dp.type != XFH_DEPTH_NONE ? dp.base + (size_t)f * dp.frame_stride : nullptr;
    int lo_end, hi_beg;
    grid_valid_slots(hdr, hdr_stride, f, n, flags, lo_end, hi_beg);
    // with a grid: ONE workgroup per frame (gridDim.y = 1) fills all P keys; without: the slots are dealt to gridDim.y workgroups
    const int end = grids ? P : n;
    for (int i = blockIdx.y * blockDim.x + tid; i < end; i += gridDim.y * blockDim.x) {
        unsigned key = XFH_GRID_DROPPED;
        if (i < n) {
            const float u = kp[i].x, v = kp[i].y;
            float uu, vu, d = -1.0f, r = -1.0f;
            xfh_undistort_point(cam, u, v, &uu, &vu);
            if (img) xfh_stereo_from_depth(xfh_depth_sample(img, dp.type, dp.pitch, dp.scale, cam.width, cam.height, u, v), uu, cam.bf, &d, &r);
            xu[2 * i] = uu; xu[2 * i + 1] = vu; dz[i] = d; ur[i] = r;
            if (i < lo_end || i >= hi_beg) key = grid_key(uu, vu, i, g);
        }
        if (grids) gkeys[i] = key;
    }
    if (!grids) return;                                    // (uniform: side arrays only)
    // also orders this workgroup's xy_un stores before grid_emit reads them back: workgroup-scope release / acquire, which holds
    // because a workgroup lives on one CU -- the library must not be built with -mtgsplit (threadgroup split mode)
    __syncthreads();
    grid_sort(gkeys, P, tid);
    grid_emit(grids + (size_t)f * grid_stride, gkeys, xu, 2, n, P, g, flags, tid);
}

hipError_t launch_frame_finish(xfh_ctx* c, const void* kps, size_t kps_stride, const void* hdr, size_t hdr_stride, const xfh_camera& cam,
                               const void* d_depth, int depth_type, size_t depth_pitch, float depth_scale, float* xy_un, float* uright, float* depth,
                               void* grids, size_t grid_stride, int n, int B, const GridGeom& g, int flags) {
    if (B <= 0 || n <= 0) return hipSuccess;
    int P = 2;
    while (P < n) P <<= 1;
    FinishDepth dp = {(const char*)d_depth, (size_t)cam.height * depth_pitch, depth_pitch, d_depth ? depth_type : XFH_DEPTH_NONE, depth_scale};
    // side arrays only: nothing needs a per-frame workgroup, so a frame is spread over n / 256 workgroups (fp64 on as many CUs)
    const dim3 grid = grids ? dim3(B) : dim3(B, (n + 255) / 256), block = grids ? dim3(XFH_GRID_BUILD_THREADS) : dim3(256);
    launch_k(c, XFH_K_FRAME_FINISH, -1, k_frame_finish, grid, block, grids ? (size_t)P * sizeof(unsigned) : 0, (const char*)kps, kps_stride,
             (const char*)hdr, hdr_stride, cam, dp, xy_un, uright, depth, (char*)grids, grid_stride, n, P, g, flags);
    return hipGetLastError();
}
