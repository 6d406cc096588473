/*
 * xfeat_hip.h -- C ABI of libxfeat_hip.so: the MI355X (gfx950) XFeat feature-extraction
 * and descriptor-matching front end for xfeatSLAM.
 *
 * This is the drop-in boundary.  Each entry point names the reference interface it
 * replaces (paths relative to udaysankar01/xfeatSLAM).  Plain pointers and sizes only;
 * no C++ or torch types; nothing throws or aborts across this ABI -- every call returns
 * an xfh_status (0 = OK) except where noted.  A ctx is single-caller (one HIP stream per
 * ctx), exactly like the reference's XFextractor object (Tracking.h:265); create one ctx
 * per GPU for multi-GPU use.  xfh_descriptor_distance is stateless and thread-safe like
 * the static ORBmatcher::DescriptorDistance.
 *
 * Threads (each of the three points is tested; INTEGRATION.md section 4 names the tests):
 *   - several ctx may be driven from several host threads at the same time, one thread per
 *     ctx -- the way Tracking, LocalMapping and LoopClosing run beside each other
 *     (System.cc:197,214,233) -- also when all of them are inside the SAME entry point;
 *   - a ctx may be handed from one thread to another (System constructs the extractor on
 *     one thread, Tracking calls it from another): one caller at a time, not always the
 *     same thread.  Two threads inside ONE ctx at the same time are outside the contract;
 *   - pure host code, stateless, callable from any thread at any time, the first call of
 *     the process included: xfh_version, xfh_strerror, xfh_kernel_name, xfh_config_default,
 *     xfh_descriptor_distance, xfh_undistort_points, xfh_camera_bounds, xfh_project_points,
 *     xfh_scale_level_thresholds, xfh_fuse_project, xfh_epipolar_gate, xfh_bow_accept,
 *     xfh_nodes_pack, xfh_nodes_unpack, xfh_grid_unpack and the size / layout helpers
 *     (xfh_record_*, xfh_*_bytes, xfh_compact_bytes_max); xfh_create itself may run on
 *     several threads at once (without a device each call returns XFH_ERR_NO_DEVICE).
 *     xfh_map_project, xfh_sim3_project and xfh_map_projection_search_workspace_bytes are stateless in the same way (a loop over
 *     one pure function, no static data); they are not part of the ThreadSanitizer run.  So are xfh_init_accept,
 *     xfh_init_list_entries and xfh_init_search_workspace_bytes, and xfh_vocab_bytes, xfh_vocab_pack, xfh_vocab_unpack, xfh_vocab_descend
 *     and xfh_bow_transform_workspace_bytes, and xfh_bow_score and xfh_bowdb_query_workspace_bytes, and xfh_sim3_solve_host,
 *     xfh_sim3_merge_matches_host, xfh_sim3_solve_iterations[_table], xfh_sim3_solve_set / _horn / _check and xfh_sim3_solve_workspace_bytes.
 *
 * The C++ wrappers that restore the reference's class surface on top of this ABI are
 * include/xfeat/XFextractor.h and include/xfeat/ORBmatcher_xfeat.h; INTEGRATION.md shows
 * the edits a maintainer makes in the reference tree.
 */
#ifndef XFEAT_HIP_H
#define XFEAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct xfh_ctx xfh_ctx;

typedef enum {
    XFH_OK = 0,
    XFH_ERR_INVALID_ARG = 1,
    XFH_ERR_EMPTY_IMAGE = 2,      /* reference returns -1 (XFextractor.cc:253-254)            */
    XFH_ERR_BAD_SIZE = 3,         /* image smaller than 32x32 or larger than the ctx maximum  */
    XFH_ERR_NO_WEIGHTS = 4,       /* extract called before xfh_load_weights                   */
    XFH_ERR_BAD_WEIGHTS = 5,      /* blob magic / tensor table / shapes wrong                 */
    XFH_ERR_HIP = 6,              /* a HIP runtime call failed; see xfh_last_hip_error        */
    XFH_ERR_NO_DEVICE = 7,        /* device ordinal absent or not gfx950: the library never falls back */
    XFH_ERR_OUT_OF_MEMORY = 8,
    XFH_ERR_BATCH_TOO_LARGE = 9,
    XFH_ERR_IO = 10,
    XFH_ERR_COMM = 11             /* RCCL missing or a collective failed; see xfh_last_hip_error */
} xfh_status;

/* mirrors cv::KeyPoint field for field (28 bytes): pt.x, pt.y, size, angle, response,
 * octave, class_id.  Written keypoints are KeyPoint(x, y, 1, -1, score) and unwritten
 * slots are the default cv::KeyPoint() -- XFextractor.cc:312,329 */
typedef struct {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} xfh_keypoint;

/* BatchNorm behaviour.  BATCH_STATS (default) reproduces the reference: the module is never put in
 * eval(), so every BasicLayer normalises with the statistics of the current frame;
 * statistics are always per frame, also in batched calls.  RUNNING_STATS is the upstream-XFeat
 * eval() behaviour: the running_mean / running_var buffers of the weight file are used instead (the
 * blob must carry them, otherwise xfh_load_weights returns XFH_ERR_BAD_WEIGHTS); the InstanceNorm of
 * the input image is per frame in all modes.
 * RUNNING_FOLDED is the same eval() network with every BatchNorm folded into the preceding convolution when the weights
 * are loaded (W' = W * rstd, b' = -mean * rstd, ReLU in the epilogue): no statistics are computed or applied at run time.
 * Folding re-rounds the weights, so this mode equals RUNNING_STATS to ~1e-6, not bit for bit. */
enum { XFH_BN_BATCH_STATS = 0, XFH_BN_RUNNING_STATS = 1, XFH_BN_RUNNING_FOLDED = 2 };

typedef struct {
    int32_t device;        /* HIP device ordinal                                              */
    int32_t max_height;    /* largest input image accepted (before the /32 resize)            */
    int32_t max_width;
    int32_t nfeatures;     /* rows of every output (XFextractor ctor arg, Tracking.cc:597)    */
    int32_t max_batch;     /* frames per xfh_extract_batch* call                              */
    int32_t bn_mode;       /* XFH_BN_*                                                        */
    float nms_threshold;   /* 0.05 in the reference (XFextractor.cc:277)                      */
    int32_t flags;         /* XFH_FLAG_*; 0 = the reference's behaviour                        */
    int32_t reserved[7];
} xfh_config;

/* flags.  XFH_FLAG_RESCALE_KEYPOINTS: report keypoints in INPUT-image coordinates, x * (W/W32), y * (H/H32) in fp32
 * as upstream XFeat does.  The reference multiplies by a Long-typed factor, i.e. by 1 (XFextractor.cc:304-305,
 * SURVEY.md Q2): for inputs whose sides are not multiples of 32 its keypoints stay in the resized frame. */
#define XFH_FLAG_RESCALE_KEYPOINTS 1
/* XFH_FLAG_SERIAL_BRANCH: run the keypoint-head branch on the ctx stream instead of the ctx's second stream (same results;
 * no two kernels overlap, so a profiler's per-launch durations are the kernels' own: profiles/r02_roofline_table.md). */
#define XFH_FLAG_SERIAL_BRANCH 2

/* fills the defaults: device 0, 480x640, nfeatures 4096, max_batch 1, threshold 0.05 */
void xfh_config_default(xfh_config* cfg);

/* XFextractor::XFextractor (XFextractor.cc:75-149) minus the host-only scale tables,
 * which live in the C++ wrapper.  Allocates all device memory up front. */
int xfh_create(const xfh_config* cfg, xfh_ctx** out);
int xfh_destroy(xfh_ctx* ctx);

/* Weight loading (replaces InputArchive::load_from + model->load, XFextractor.cc:133-137).
 * blob format: xfeatslam_amd/weights.py ("XFHWGT01" + tensor table + fp32 OIHW data). */
int xfh_load_weights(xfh_ctx* ctx, const void* blob, size_t nbytes);
int xfh_load_weights_file(xfh_ctx* ctx, const char* path);

/* ---- extraction: XFextractor::operator() (XFextractor.cc:250-356) -------------------
 * gray: H x W CV_8UC1 in host memory, stride_bytes between rows (the reference assumes a
 * dense Mat, :166).  lap_x0/lap_x1 = vLappingArea (Frame.cc:311 passes {0,0}, :495
 * {0,1000}).  kps_out: nfeatures records, desc_out: nfeatures x 64 floats row-major; both
 * fully written (padding = default KeyPoint / zero rows).  *mono_index is operator()'s
 * return value, *n_valid the number of keypoints with score > 0 that were written. */
int xfh_extract(xfh_ctx* ctx, const uint8_t* gray, int H, int W, int stride_bytes, int lap_x0, int lap_x1,
                xfh_keypoint* kps_out, float* desc_out, int* n_valid, int* mono_index);

/* Split form of xfh_extract: submit copies the image into a pinned staging buffer of the ctx and
 * enqueues H2D and the kernels, which write the record straight into pinned host memory, then returns; collect waits
 * for the oldest submission and unpacks it (only the valid rows are copied, the padding is filled on the host).  Up to
 * XFH_MAX_INFLIGHT submissions may be outstanding per ctx (a further submit returns XFH_ERR_INVALID_ARG until one is
 * collected), so frame t+1 can be uploaded and computed while the caller still copies out / tracks frame t; or submit the
 * right image of a stereo pair on a second ctx. */
#define XFH_MAX_INFLIGHT 2
int xfh_extract_submit(xfh_ctx* ctx, const uint8_t* gray, int H, int W, int stride_bytes, int lap_x0, int lap_x1);
int xfh_extract_collect(xfh_ctx* ctx, xfh_keypoint* kps_out, float* desc_out, int* n_valid, int* mono_index);

/* the upstream name of the same call (README.md:9, xfeat_cpp `detectAndCompute`) */
int xfh_detect_and_compute(xfh_ctx* ctx, const uint8_t* gray, int H, int W, int stride_bytes,
                           int lap_x0, int lap_x1, xfh_keypoint* kps_out, float* desc_out,
                           int* n_valid, int* mono_index);

/* One output record per frame, device or host resident, fixed size (the reference output
 * is already padded to nfeatures rows -- SURVEY.md Q3):
 *   int32 n_valid, mono_index, n_candidates, reserved;
 *   xfh_keypoint kps[nfeatures];  float desc[nfeatures*64];                              */
size_t xfh_record_bytes(int nfeatures);
size_t xfh_record_kps_offset(void);
size_t xfh_record_desc_offset(int nfeatures);

/* B dense frames [B][H][W] u8 in HOST memory -> B records in HOST memory: the batched form of operator()'s contract (host image
 * in, host keypoints / descriptors out, XFextractor.cc:250-356; SURVEY.md 8d "host-visible").  B is NOT limited by cfg.max_batch:
 * the call is cut into sub-batches of cfg.max_batch frames.  One sub-batch (B <= cfg.max_batch) runs on the ctx itself, in order on its stream.
 * More go into one queue that up to xfh_pipeline_lanes (default 6) internal lanes drain: a lane = a child ctx (own activations and HIP streams,
 * the ctx' weights, built at the first call that needs it) + a copy stream + a host THREAD of the library that drives one sub-batch at a time --
 * copy in, kernels, copy out, each waited for on the host -- so that no copy command ever sits in a stream in front of a kernel and no stream
 * waits for a copy on the GPU; the lanes overlap each other (NOTES.md 6: 0.97-0.98 of the device-resident rate, 0.74-0.85 with in-order streams).
 * Cost: every lane is a full child ctx -- activations for cfg.max_batch frames (about 29 MB per VGA frame, i.e. 1.9 GB per lane at max_batch 64) --
 * plus one host thread; they are built at the first submit that spans more than one sub-batch (min(sub-batches, lanes) of them), and that submit is
 * where XFH_ERR_OUT_OF_MEMORY surfaces if the device cannot hold them.  xfh_pipeline_lanes(ctx, n) bounds the number before that call.
 * gray / records_out should be pinned (xfh_host_alloc, or the caller's own buffers through xfh_host_register): pageable
 * memory works, but the runtime then stages every copy and the stages serialise.
 *   xfh_extract_batch_submit  returns when everything is queued; both buffers must stay untouched until the batch is complete.
 *                             Up to XFH_MAX_BATCHES_INFLIGHT submits may be outstanding (one more: XFH_ERR_INVALID_ARG); their
 *                             sub-batches simply queue up on the lanes, so a consumer that double-buffers records_out keeps
 *                             the GPU busy across calls: submit(t + 1); wait() -> batch t is complete; ...
 *   xfh_extract_batch_wait    the OLDEST outstanding submit is complete in its records_out (XFH_ERR_INVALID_ARG if none is)
 *   xfh_extract_batch_drain   every submit so far is complete
 *   xfh_extract_batch         = submit + drain.
 *                             A submit that FAILS has waited for whatever part of it was already queued: nothing of it is in flight when
 *                             the error comes back, and the buffers are the caller's again.
 * These calls and the single-frame ring (xfh_extract_submit) share the ctx' first frame buffer (a one-sub-batch submit runs on the ctx itself): a
 * batch call while a single-frame submission is outstanding returns XFH_ERR_INVALID_ARG, and so does xfh_extract (it would collect the OLDER
 * submission's result).  The other direction needs no guard: xfh_extract_submit while batches are outstanding queues on the ctx' own stream BEHIND a
 * one-sub-batch submit (same stream, in order), and the lanes of larger submits have buffers of their own.  The ctx stays single-caller: the worker
 * threads touch the lanes only, never the ctx' own buffers or streams. */
#define XFH_MAX_BATCHES_INFLIGHT 8
int xfh_extract_batch(xfh_ctx* ctx, const uint8_t* gray, int B, int H, int W, int lap_x0, int lap_x1,
                      void* records_out);
int xfh_extract_batch_submit(xfh_ctx* ctx, const uint8_t* gray, int B, int H, int W, int lap_x0, int lap_x1,
                             void* records_out);
int xfh_extract_batch_wait(xfh_ctx* ctx);
int xfh_extract_batch_drain(xfh_ctx* ctx);
int xfh_pipeline_lanes(xfh_ctx* ctx, int lanes);      /* 1 .. 8 (default 6); sub-batches in flight side by side, one worker thread each */
/* pinned host memory for the calls above (hipHostMalloc / hipHostRegister behind the ABI, for host languages without a HIP binding) */
int xfh_host_alloc(void** p, size_t nbytes);
int xfh_host_free(void* p);
int xfh_host_register(void* p, size_t nbytes);
int xfh_host_unregister(void* p);
/* same with DEVICE pointers (frames resident in HBM, records stay in HBM for the matcher or
 * an RCCL all-gather); asynchronous on the ctx stream -- call xfh_synchronize to wait. */
int xfh_extract_batch_device(xfh_ctx* ctx, const uint8_t* d_gray, int B, int H, int W, int lap_x0,
                             int lap_x1, void* d_records_out);
/* the same, and each frame's descriptor block is also written as the matcher's PREPARED IMAGE (see xfh_match_prepare_device):
 * d_images_out holds B images of xfh_match_image_bytes(nfeatures) bytes, image b = what xfh_match_prepare_device makes of the
 * nfeatures descriptor rows of record b, bit for bit (padding slots are rows of zeros).  The frame-to-frame match of the tracker
 * (frame t against t-1) is then xfh_match_mnn_prepared_device on two of these images with n1 = n2 = nfeatures: two launches, no
 * normalisation pass over descriptors that k_desc has only just written. */
int xfh_extract_batch_device_images(xfh_ctx* ctx, const uint8_t* d_gray, int B, int H, int W, int lap_x0,
                                    int lap_x1, void* d_records_out, void* d_images_out);

/* ---- matching ----------------------------------------------------------------------
 * ORBmatcher::match (declared ORBmatcher.h:77; its definition is commented out at
 * ORBmatcher.cc:340-405; these are the semantics of that code with float descriptors):
 * rows L2-normalised, cosine similarity, mutual nearest neighbours, first maximum wins
 * ties, matches in ascending idx1 order, dist = sqrt(2 (1 - cos)).  min_cossim <= 0
 * disables the gate as the reference does (:361).  idx1/idx2/dist need min(n1,n2) slots.
 * Descriptors must be finite.  Rows holding NaN or Inf are outside the contract: the calls still return (a bounded wait, never a
 * hang) and the pairs among finite rows that do not compete with a poisoned row are unaffected, but which partner a poisoned row
 * gets -- the reference's torch::max would propagate the NaN -- is unspecified (the match GEMM is built with -fno-honor-nans).
 * The extraction never produces such rows. */
int xfh_match_mnn(xfh_ctx* ctx, const float* d1, int n1, const float* d2, int n2, float min_cossim,
                  int* idx1, int* idx2, float* dist, int* n_matches);
/* device-resident variant: d1/d2 device pointers (e.g. the desc block of two records),
 * outputs device pointers; *d_n_matches is one int in device memory.  Asynchronous. */
int xfh_match_mnn_device(xfh_ctx* ctx, const float* d_d1, int n1, const float* d_d2, int n2,
                         float min_cossim, int* d_idx1, int* d_idx2, float* d_dist, int* d_n_matches);

/* Prepared descriptor sets (device-resident hand-off).  A tracker matches every frame against several
 * others (previous frame, key frames, loop candidates): xfh_match_prepare_device normalises the n x 64 rows once
 * (F::normalize, ORBmatcher.cc:358-359) and stores them as the "panel image" the GEMM kernel reads
 * (xfh_match_image_bytes(n) bytes of device memory owned by the caller); xfh_match_mnn_prepared_device then runs
 * ORBmatcher::match on two images with the same results as xfh_match_mnn_device on the rows they were made from,
 * in two kernel launches instead of three.  Device pointers, asynchronous on the ctx stream. */
size_t xfh_match_image_bytes(int n);
int xfh_match_prepare_device(xfh_ctx* ctx, const float* d_desc, int n, void* d_image);
int xfh_match_mnn_prepared_device(xfh_ctx* ctx, const void* d_image1, int n1, const void* d_image2, int n2,
                                  float min_cossim, int* d_idx1, int* d_idx2, float* d_dist, int* d_n_matches);

/* Many pairs in one call.  The reference's consumers meet one frame with several partners -- the previous frame, key frames, loop
 * candidates: one ORBmatcher::match per frame pair (ORBmatcher.cc:358-372 per call; SURVEY.md 8e "for many frame pairs, shard pairs") --
 * and one 4096 x 4096 pair is exactly one tile per CU, so a call per pair pays its launch ramp, staging wait and epilogue latency with
 * nothing to overlap them.  This entry runs the similarity GEMM of ALL pairs as one persistent launch (equal shares of the tiles of all
 * pairs per workgroup, the next tile's panel arriving while the current one is multiplied) and the mutual check / output of all
 * pairs as a second one.  Pair p: prepared images d_image1[p] (n1[p] rows) and d_image2[p] (n2[p] rows) -- the same image may appear
 * in any number of pairs, on either side -- match list to d_idx1[p] / d_idx2[p] / d_dist[p] (min(n1[p], n2[p]) slots each) and its
 * length to d_n_matches[p]; results are those of xfh_match_mnn_prepared_device pair by pair, bit for bit.  The pointer and size arrays
 * are HOST arrays (read before the call returns); everything they point to is device memory.  Asynchronous on the ctx stream. */
int xfh_match_mnn_prepared_batch_device(xfh_ctx* ctx, int n_pairs, const void* const* d_image1, const int* n1, const void* const* d_image2, const int* n2,
                                        float min_cossim, int* const* d_idx1, int* const* d_idx2, float* const* d_dist, int* d_n_matches);

/* n_valid-aware match of two extraction records (option).  ORBmatcher::match treats the zero rows that pad a record
 * like descriptors (they have similarity 0 with everything and can end up in mutual pairs); here every pair that touches a padding
 * slot is dropped.  d_record1/2: records of this ctx' nfeatures (only their headers are read: valid slots are [0, mono_index) and
 * [nfeatures - (n_valid - mono_index), nfeatures)); d_image1/2: their prepared images (xfh_extract_batch_device_images).  Indices
 * are slot numbers; everything else as xfh_match_mnn_prepared_device. */
int xfh_match_records_device(xfh_ctx* ctx, const void* d_record1, const void* d_image1, const void* d_record2, const void* d_image2,
                             float min_cossim, int* d_idx1, int* d_idx2, float* d_dist, int* d_n_matches);

/* ORBmatcher::DescriptorDistance (ORBmatcher.cc:2242-2250), XFeat branch:
 * (int)(float(cv::norm(a, b, NORM_L2SQR)) * 512).  Scalar host version, stateless. */
int xfh_descriptor_distance(const float* a, const float* b);
/* dense n1 x n2 table of the same integer metric, computed on the GPU (host pointers) */
int xfh_distance_i32(xfh_ctx* ctx, const float* d1, int n1, const float* d2, int n2, int32_t* out);
int xfh_distance_i32_device(xfh_ctx* ctx, const float* d_d1, int n1, const float* d_d2, int n2, int32_t* d_out);

/* Guided ("windowed") matching, the inner loop of ORBmatcher::SearchByProjection / SearchByBoW /
 * SearchForTriangulation / Fuse (ORBmatcher.cc:82-119, 1928-1953, 450-500, ...): for query q the
 * candidates are indices[offsets[q] .. offsets[q+1]) into the target descriptors, visited in that
 * order with
 *     dist = DescriptorDistance(query_q, target_idx);
 *     if (dist < best)        { second = best; best = dist; best_idx = idx; }
 *     else if (dist < second) { second = dist; }
 * starting from best = second = init_dist (the reference keeps ORB's 256) and
 * best_idx = -1.  second_idx is the candidate that holds `second` at the end (the reference keeps
 * its pyramid level, always 0 for XFeat).  The map-state filters of the reference (already-matched
 * map points, stereo consistency) are applied by the caller when it builds the candidate lists.
 * All pointers host memory (the _device variant: device memory, asynchronous). */
int xfh_best2_csr(xfh_ctx* ctx, const float* queries, int nq, const float* targets, int nt,
                  const int* offsets, const int* indices, int init_dist,
                  int* best_idx, int* best_dist, int* second_idx, int* second_dist);
int xfh_best2_csr_device(xfh_ctx* ctx, const float* d_queries, int nq, const float* d_targets, int nt,
                         const int* d_offsets, const int* d_indices, int init_dist,
                         int* d_best_idx, int* d_best_dist, int* d_second_idx, int* d_second_dist);

/* ---- frame grid + windowed search, device resident ------------------------------------------------------
 * What the tracker runs every frame is not the dense match but the WINDOWED search: ORBmatcher::SearchByProjection(Frame, Frame)
 * (ORBmatcher.cc:1861-1960, from TrackWithMotionModel), SearchByProjection(Frame, vector<MapPoint*>) (:42-130, SearchLocalPoints)
 * and the relocalisation variants project a point to (u, v), ask Frame::GetFeaturesInArea(u, v, r) (Frame.cc:850-916) for the
 * keypoints inside the window through the 64 x 48 grid that Frame::AssignFeaturesToGrid (:569-599) built, and run the best /
 * second-best DescriptorDistance loop over them.  These calls keep all of it on the GPU: a grid per frame in device memory, built
 * straight from extraction records, and one fused kernel "window -> candidates -> best two" per batch of queries.
 *
 * Grid (Frame.cc:569-599, PosInGrid :918-929, bounds and inverse cell sizes :336-341, :985-1001): the caller gives the bounds
 * (0, 0, cols, rows for an undistorted camera; with distortion the grid is built from the UNDISTORTED keypoints with mnMinX .. mnMaxY:
 * xfh_frame_finish_records_device and xfh_camera_bounds below);
 * inv_w = 64.0f / (max_x - min_x), inv_h = 48.0f / (max_y - min_y) in fp32.  Keypoint i goes to cell
 * (round((x - min_x) * inv_w), round((y - min_y) * inv_h)), round = roundf (half away from zero), and is NOT binned when a
 * coordinate is < 0, >= 64 resp. >= 48: the reference rounds (it does not floor), so the right-most / bottom half cell of the
 * image is lost; that is reproduced.  Inside a cell keypoints keep ascending slot order (push_back order).
 * flags = 0 is the reference: all n slots are binned, padding included -- padding slots are default cv::KeyPoint() at (0, 0) and
 * all land in cell (0, 0) (N = mvKeys.size(), Frame.cc:318).  With XFH_GRID_SKIP_PADDING and a record header, slots outside
 * [0, mono_index) U [n - (n_valid - mono_index), n) are left out (the valid slots of xfh_match_records_device); the flag without
 * a record is XFH_ERR_INVALID_ARG.
 *
 * The grid is an opaque, self-contained blob of xfh_grid_bytes(n) bytes in device memory owned by the caller (16-byte aligned):
 * bounds, inverse cell sizes, cell_start, and per item slot number, x, y in cell order.  Two builds of the same input give
 * identical bytes.  n <= XFH_GRID_MAX_N.
 *   xfh_grid_build_device          one grid from n keypoints in device memory (d_record: the record they belong to, or NULL)
 *   xfh_grid_build_records_device  B grids (grid b at d_grids + b * xfh_grid_bytes(nfeatures)) from B extraction records of this
 *                                  ctx, ONE launch
 *   xfh_grid_unpack                host, stateless: a blob copied out of device memory (nbytes of it) -> cell_start[64 * 48 + 1]
 *                                  (cell = ix * 48 + iy), items[n] (slot numbers in cell order, -1 past *n_binned).  A truncated or
 *                                  inconsistent blob is XFH_ERR_INVALID_ARG, never an out-of-bounds access.
 *
 * Search, per query q with (u, v, r) = d_uvr[3q .. 3q + 2] and descriptor row q of d_queries (GetFeaturesInArea + the loop of
 * ORBmatcher.cc:1925-1955 / :82-119):
 *   c0x = max(0, (int)floorf((u - min_x - r) * inv_w)), no candidates if >= 64; c1x = min(63, (int)ceilf((u - min_x + r) * inv_w)),
 *   none if < 0; the same for y with 48 rows; cells ix = c0x .. c1x (outer), iy = c0y .. c1y (inner), a cell's keypoints in stored
 *   order; keypoint k is a candidate when fabsf(x_k - u) < r && fabsf(y_k - v) < r (strict);
 *   d_skip (optional, one byte per target, non-zero = skip): "already has a map point with observations" (:1931-1933).  A static
 *   mask is exact only for entries that were set BEFORE the loop: inside SearchByProjection the test also sees what earlier
 *   iterations of the same loop wrote (:1957, :128) -- that order is xfh_search_projection_device below; d_uright + d_ur_query (optional, both or neither): a candidate with uright[k] > 0 is skipped when
 *   fabsf(ur_query[q] - uright[k]) > r (:1935-1941);
 *   over the survivors in visiting order the rule and the result contract of xfh_best2_csr (best = second = init_dist, strict '<',
 *   exact DescriptorDistance), indices = keypoint slot numbers.  A tie goes to the candidate visited FIRST, which is not the lowest
 *   slot number.  n_candidates[q] = candidates that passed the window and the optional filters (`if (vIndices.empty()) continue`).
 * Octave windows (minLevel / maxLevel) are not part of the interface: every XFeat keypoint has octave 0 and every level window the
 * reference passes contains 0.  Where the reference is undefined -- (int) of a non-finite or huge float -- a query whose u, v or r is
 * not finite has no candidates, and cell bounds saturate before the conversion; the kernel reads nothing outside the grid and the
 * nt target rows whatever floats it is given.  d_targets / d_skip / d_uright are indexed by slot number: nt = the n of the grid.
 * The _device calls take device pointers only and are asynchronous on the ctx stream: no host synchronisation, no allocation.
 * xfh_search_window is the convenience form for host pointers (like xfh_best2_csr): stages the inputs, builds the grid of the nt
 * keypoints (flags 0), searches and copies the five result arrays back. */
#define XFH_GRID_COLS 64              /* FRAME_GRID_COLS, include/Frame.h:48 */
#define XFH_GRID_ROWS 48              /* FRAME_GRID_ROWS, include/Frame.h:47 */
#define XFH_GRID_SKIP_PADDING 1
#define XFH_GRID_MAX_N 16384          /* keypoint slots per grid (the build sorts one frame's keys in the LDS of one workgroup) */
typedef struct { float min_x, min_y, max_x, max_y; } xfh_grid_bounds;
size_t xfh_grid_bytes(int n);
int xfh_grid_build_device(xfh_ctx* ctx, const xfh_keypoint* d_kps, int n, const void* d_record_or_null, const xfh_grid_bounds* bounds,
                          int flags, void* d_grid);
int xfh_grid_build_records_device(xfh_ctx* ctx, const void* d_records, int B, const xfh_grid_bounds* bounds, int flags, void* d_grids);
int xfh_grid_unpack(const void* host_copy_of_grid, size_t nbytes, int n, int* cell_start, int* items, int* n_binned);
int xfh_search_window_device(xfh_ctx* ctx, const float* d_queries, const float* d_uvr, int nq, const void* d_grid, const float* d_targets, int nt,
                             const uint8_t* d_skip_or_null, const float* d_uright_or_null, const float* d_ur_query_or_null, int init_dist,
                             int* d_best_idx, int* d_best_dist, int* d_second_idx, int* d_second_dist, int* d_n_candidates);
int xfh_search_window(xfh_ctx* ctx, const float* queries, const float* uvr, int nq, const xfh_keypoint* kps, const xfh_grid_bounds* bounds,
                      const float* targets, int nt, const uint8_t* skip_or_null, const float* uright_or_null, const float* ur_query_or_null,
                      int init_dist, int* best_idx, int* best_dist, int* second_idx, int* second_dist, int* n_candidates);

/* ---- finishing an RGB-D frame on the device: undistort, depth, grid of mvKeysUn ------------------------------------------------
 * Between ExtractXF and AssignFeaturesToGrid the reference's RGB-D constructor (src/Frame.cc:311-374) runs UndistortKeyPoints
 * (:940-973), ComputeStereoFromRGBD (:1177-1198) and, once per calibration, ComputeImageBounds (:975-1002); the grid, GetFeaturesInArea
 * and SearchByProjection then work on mvKeysUn and mvuRight.  These calls are that stage, so that extract -> finish -> grid -> search
 * stays in device memory for a camera WITH distortion (the reference's examples/RGB-D/TUM1.yaml has five non-zero coefficients).
 *
 * Undistort: cv::undistortPoints(src, dst, K, dist, Mat(), P = K) restated from its documented algorithm (this library does not link
 * OpenCV), per point in float64, in this operation order:
 *     x0 = (u - cx) / fx; y0 = (v - cy) / fy; x = x0; y = y0
 *     5 times (the default TermCriteria is COUNT 5, there is no epsilon exit):
 *         r2 = x*x + y*y;  icdist = 1 / (1 + ((k3*r2 + k2)*r2 + k1)*r2);  if (icdist < 0) { x = x0; y = y0; stop }
 *         dx = 2*p1*x*y + p2*(r2 + 2*x*x);  dy = p1*(r2 + 2*y*y) + 2*p2*x*y;  x = (x0 - dx)*icdist;  y = (y0 - dy)*icdist
 *     u' = (float)(x*fx + cx); v' = (float)(y*fy + cy)
 * k1 == 0 copies the points unchanged whatever the other coefficients are (Frame.cc:942), and the same test selects the bounds
 * (0, 0, width, height) (:977).  Otherwise the bounds come from the undistorted corners p0 = (0, 0), p1 = (width, 0), p2 = (0, height),
 * p3 = (width, height): min_x = min(p0.x, p2.x), max_x = max(p1.x, p3.x), min_y = min(p0.y, p1.y), max_y = max(p2.y, p3.y).
 * All n slots are processed, padding slots at (0, 0) included, as the reference does (N = mvKeys.size()).
 *
 * Depth: the image is fp32 metres (XFH_DEPTH_F32) or raw uint16 (XFH_DEPTH_U16) with the multiplier depth_scale (the reference's
 * 1.0f / DepthMapFactor, Tracking.cc:577-581): d = (float)raw * depth_scale, one fp32 rounding.  Rows are depth_pitch_bytes apart (a
 * multiple of the element size).  It is sampled at ((int)v, (int)u) of the RAW keypoint; depth = d and uright = u' - bf / d (fp32) when
 * d > 0, otherwise both are -1 (a NaN depth fails d > 0).  Where the reference would read outside the image the sample is 0 and nothing
 * is read.  XFH_DEPTH_NONE writes -1 to both arrays: the monocular constructor.  A NULL image with XFH_DEPTH_F32 / XFH_DEPTH_U16 is accepted
 * and treated as XFH_DEPTH_NONE; depth_pitch_bytes and depth_scale are ignored whenever there is no image.
 *
 *   xfh_undistort_points / xfh_camera_bounds   host, stateless, thread-safe: n (u, v) pairs -> n (u', v') pairs; mnMinX .. mnMaxY
 *   xfh_frame_finish_records_device   B records of this ctx in ONE launch: per frame b xy_un[n][2] at d_xy_un + b * 2 * nfeatures floats,
 *                                     the outputs d_uright / d_depth at + b * nfeatures floats (plain fp32 arrays: d_uright plugs into
 *                                     xfh_search_window_device), INPUT depth image b at d_depth_or_null + b * height * depth_pitch_bytes, and -- unless
 *                                     d_grids is NULL -- the grid blob of the UNDISTORTED coordinates with the caller's bounds at
 *                                     d_grids + b * xfh_grid_bytes(nfeatures), in the format of xfh_grid_build_records_device (for k1 == 0
 *                                     the same bytes).  XFH_GRID_SKIP_PADDING keeps padding slots out of the grid only; their side
 *                                     arrays are written like everyone's.  Device pointers, asynchronous on the ctx stream, no allocation.
 *   xfh_frame_finish                  host-pointer convenience form for one frame's n keypoints (side arrays only)
 * XFH_ERR_INVALID_ARG before anything is launched: B outside 1 .. max_batch, nfeatures > XFH_GRID_MAX_N with a grid requested, a pitch
 * smaller than a row or not a multiple of the element size, width or height <= 0, an unknown depth type, bounds as for
 * xfh_grid_build_device, misaligned pointers (16 bytes for the grids, the element size otherwise).  Coefficients, keypoints and
 * depth values may be anything, NaN and Inf included: a non-finite undistorted coordinate is not binned, and no load leaves the
 * records, the depth images or the blob. */
typedef struct {
    float fx, fy, cx, cy, k1, k2, p1, p2, k3, bf;
    int32_t width, height;
    int32_t reserved[4];
} xfh_camera;
enum { XFH_DEPTH_NONE = 0, XFH_DEPTH_F32 = 1, XFH_DEPTH_U16 = 2 };
int xfh_undistort_points(const xfh_camera* cam, const float* xy, int n, float* xy_un);
int xfh_camera_bounds(const xfh_camera* cam, xfh_grid_bounds* out);
int xfh_frame_finish_records_device(xfh_ctx* ctx, const void* d_records, int B, const xfh_camera* cam, const void* d_depth_or_null, int depth_type,
                                    size_t depth_pitch_bytes, float depth_scale, const xfh_grid_bounds* bounds, int grid_flags,
                                    float* d_xy_un, float* d_uright, float* d_depth, void* d_grids_or_null);
int xfh_frame_finish(xfh_ctx* ctx, const xfh_keypoint* kps, int n, const xfh_camera* cam, const void* depth_or_null, int depth_type,
                     size_t depth_pitch_bytes, float depth_scale, float* xy_un, float* uright, float* depth);

/* ---- SearchByProjection with the reference's claim order, device resident ------------------------------------------------------
 * ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono) (src/ORBmatcher.cc:1861-2047, called from
 * Tracking.cc:2914-2932) and the SearchLocalPoints form SearchByProjection(Frame&, vector<MapPoint*>&, ...) (:42-141) as one call: world
 * points and a pose (or the caller's projections) in, the reference's mvpMapPoints assignment and nmatches out, everything in device
 * memory.  The candidate test `CurrentFrame.mvpMapPoints[i2] && ->Observations() > 0` (:1932-1934, :87-89) cannot be evaluated
 * beforehand: Tracking.cc:2914 fills mvpMapPoints with NULL just before the call, so every entry the test sees was written by an
 * earlier iteration of the same loop (:1957, :128).  The loop is sequential and greedy; a query whose map point has observations
 * claims its keypoint and later queries skip it; a query whose map point has none (the temporal points of UpdateLastFrame) does not
 * claim and a later query may overwrite its assignment; nmatches counts both.  The contract is that sequential loop.  Each problem b
 * has one current-frame grid with its nt target descriptors and nq queries:
 *
 *   claimed[k] = d_skip ? d_skip[k] != 0 : 0        for k in [0, nt)
 *   assigned[k] = -1;  n_matches = 0
 *   for q = 0 .. nq-1, in this order:
 *     flags[q] bit0 clear                          -> status INACTIVE  (pMP == NULL or mvbOutlier, :1883-1885)
 *     -- projection, mode XFH_PROJ_POINTS (fp32, no contraction, exactly this order)
 *     xc = ((T[0]*X + T[1]*Y) + T[2]*Z) + T[3]     (T = row-major 3x4 [R|t] of Tcw; yc, zc likewise from rows 1, 2)
 *     invz = (float)(1.0 / (double)zc);            invz < 0 -> status BEHIND           (:1893-1896)
 *     u = fx*xc/zc + cx;  v = fy*yc/zc + cy        (multiply, divide, add: Pinhole.cpp:45-46)
 *     u < min_x || u > max_x || v < min_y || v > max_y -> status OUT_OF_BOUNDS          (:1900-1903, a NaN passes as in the reference)
 *     ur = u - bf*invz;  r = radius (one float per call: th * mvScaleFactors[0] = th)
 *     -- mode XFH_PROJ_GIVEN: (u, v, r) = d_uvr[3q..], ur = d_ur_query[q]; no culls (the caller's isInFrustum did them)
 *     window + candidate filters exactly as xfh_search_window_device documents them (strict |dx| < r, |dy| < r; the uright filter
 *     only when d_uright is given; a non-finite u, v or r has no candidates), with ONE addition: a candidate k with claimed[k] is
 *     skipped.                                      no survivors -> status NO_CANDIDATES (:1920 / :73)
 *     best / second over the survivors in visiting order, the rule of xfh_best2_csr (init_dist, strict '<')
 *     accept = best_idx >= 0 && best <= th_high && !(nn_ratio > 0 && second_idx >= 0 && (float)best > nn_ratio * (float)second)
 *              (nn_ratio = 0: the Frame-Frame form :1955;  > 0: :122-127 with bestLevel == bestLevel2 == 0 whenever a second exists,
 *               and bestLevel2 == -1 -- accepted without the ratio -- when it does not.  best_idx < 0, no survivor under init_dist:
 *               the reference goes on to index mvpMapPoints with -1, which is undefined; here the query is rejected)
 *     !accept -> status REJECTED;   accept -> status MATCHED, assigned[best_idx] = q, ++n_matches,
 *                and if flags[q] bit1 ("the map point has Observations() > 0"): claimed[best_idx] = 1
 *
 * Outputs, all exact and all in device memory.  Per query: status (XFH_PROJ_*), match_idx (-1 unless MATCHED), best_dist,
 * second_dist (init_dist where there is none), n_candidates (survivors AFTER the claim skip; 0 for a query that never reached the
 * search), and optionally d_proj_out[q] = (u, v, ur) ((0, 0, 0) for INACTIVE and BEHIND; GIVEN: the caller's values, ur = 0 without
 * d_ur_query).  Per keypoint: assigned[k] = the query that holds mvpMapPoints[k] after the loop, -1 for none: the last writer wins,
 * as at :1957.  n_matches[b]: one int per problem, counting accepting queries, not distinct keypoints, as the reference does.
 *
 * What of the reference function does not appear, and why.  The level windows of bForward / bBackward (:1913-1918) admit every XFeat
 * keypoint, because all have octave 0: Tlw is not an input.  The rotation histogram (:1960-1977, 2049 ff.) puts every match in bin 0,
 * because every XFeat keypoint has angle = -1: it removes nothing.  The Nleft != -1 branch is fisheye stereo, which SURVEY.md puts out
 * of scope.  The pose goes in as a 3x4 matrix with the stated operation order.  The reference applies Sophus::SE3f * Vector3f through
 * Eigen's quaternion path, which cannot be compiled or run here: bit equality with the reference's own x3Dc is NOT claimed, and
 * nobody has measured it.  Everything after x3Dc follows the reference's expressions.
 *
 *   xfh_project_points    host, stateless, thread-safe (like xfh_undistort_points): the projection arithmetic above for n points with
 *                         ONE pose.  uvr[i] = (u, v, radius), ur[i], status[i] = XFH_PROJ_BEHIND (u = v = ur = 0),
 *                         XFH_PROJ_OUT_OF_BOUNDS or XFH_PROJ_VISIBLE.  The same source line as the kernel (projection_math.h).
 *   xfh_search_projection_workspace_bytes(nq, nt, B)   bytes of d_workspace (16-byte aligned, owned by the caller, contents
 *                         irrelevant before the call), = B times the value for B = 1.  After the call the first two ints of problem
 *                         b's slice say how many rounds the claim resolution took and how many queries it searched a second time.
 *   xfh_search_projection_device   B problems with the same nq, nt, camera, bounds and thresholds.  Layouts: d_points_or_uvr [B][nq][3],
 *                         d_ur_query [B][nq], d_Tcw [B][12] in DEVICE memory, d_query_desc [B][nq][64], d_query_flags [B][nq] bytes,
 *                         grid b at d_grids + b * xfh_grid_bytes(nt), target rows of problem b at d_targets + b * target_stride_bytes
 *                         (xfh_record_bytes(nfeatures) lets d_targets point at the desc block of record 0 of a batch), d_skip and
 *                         d_uright [B][nt]; outputs d_status [B][nq] bytes, d_match_idx / d_best_dist / d_second_dist / d_n_candidates
 *                         [B][nq] ints, d_proj_out [B][nq][3] or NULL, d_assigned [B][nt] ints, d_n_matches [B] ints.  All pointers are
 *                         device pointers; asynchronous on the ctx stream, no host synchronisation, no allocation; the number of
 *                         resolution rounds depends on the data and is decided on the device (at most nq: one workgroup per problem
 *                         resolves the claims, so the cost grows with the depth of the claim chains -- measured figures in
 *                         profiles/search_projection.md; thousands of queries on ONE spot take seconds).  cam (fx, fy, cx, cy, bf
 *                         are read) and bounds are needed in POINTS mode only.  XFH_ERR_INVALID_ARG before any launch: B < 1, nq or
 *                         nt outside 1 .. XFH_GRID_MAX_N, an unknown mode, GIVEN mode with d_ur_query but no d_uright or the reverse,
 *                         POINTS mode without pose, camera or bounds, a NULL required pointer, misaligned pointers (16 bytes for
 *                         descriptors, targets, the stride, grids and the workspace, the element size otherwise), a non-finite
 *                         radius, nn_ratio < 0 or not finite.  Point coordinates, poses and descriptors may hold any value, NaN and
 *                         Inf included: no load leaves the buffers the caller named.
 *   xfh_search_projection host-pointer convenience form for ONE problem (like xfh_search_window): stages the inputs, builds the grid
 *                         of the nt keypoints with flags 0, runs the call and copies the results back.  Tcw is a host array here and `bounds` (always
 *                         needed) is also the grid's. */
enum { XFH_PROJ_POINTS = 0, XFH_PROJ_GIVEN = 1 };
enum { XFH_PROJ_INACTIVE = 0, XFH_PROJ_BEHIND = 1, XFH_PROJ_OUT_OF_BOUNDS = 2, XFH_PROJ_NO_CANDIDATES = 3, XFH_PROJ_REJECTED = 4, XFH_PROJ_MATCHED = 5,
       XFH_PROJ_VISIBLE = 3 /* xfh_project_points: the point reaches the search */ };
#define XFH_PROJ_FLAG_ACTIVE 1        /* d_query_flags bit0: pMP != NULL && !mvbOutlier */
#define XFH_PROJ_FLAG_CLAIMS 2        /* d_query_flags bit1: pMP->Observations() > 0 */
int xfh_project_points(const float* Tcw, const xfh_camera* cam, const xfh_grid_bounds* bounds, const float* xyz, int n, float radius,
                       float* uvr, float* ur, uint8_t* status);
size_t xfh_search_projection_workspace_bytes(int nq, int nt, int B);
int xfh_search_projection_device(xfh_ctx* ctx, int mode, int B, int nq, const float* d_points_or_uvr, const float* d_ur_query_or_null, const float* d_Tcw,
                                 const xfh_camera* cam, const xfh_grid_bounds* bounds, float radius, const float* d_query_desc,
                                 const uint8_t* d_query_flags, const void* d_grids, const float* d_targets, size_t target_stride_bytes, int nt,
                                 const uint8_t* d_skip_or_null, const float* d_uright_or_null, int init_dist, int th_high, float nn_ratio,
                                 void* d_workspace, uint8_t* d_status, int* d_match_idx, int* d_best_dist, int* d_second_dist, int* d_n_candidates,
                                 float* d_proj_out_or_null, int* d_assigned, int* d_n_matches);
int xfh_search_projection(xfh_ctx* ctx, int mode, int nq, const float* points_or_uvr, const float* ur_query_or_null, const float* Tcw,
                          const xfh_camera* cam, const xfh_grid_bounds* bounds, float radius, const float* query_desc, const uint8_t* query_flags,
                          const xfh_keypoint* kps, const float* targets, int nt, const uint8_t* skip_or_null,
                          const float* uright_or_null, int init_dist, int th_high, float nn_ratio, uint8_t* status, int* match_idx, int* best_dist,
                          int* second_dist, int* n_candidates, float* proj_out_or_null, int* assigned, int* n_matches);

/* ---- Fuse: map points projected into keyframes and searched, device resident -------------------------------------------------------
 * ORBmatcher::Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, th, bRight = false) (src/ORBmatcher.cc:1333-1523, the SE3 form,
 * called from LocalMapping::SearchInNeighbors, src/LocalMapping.cc:714 ff.) and Fuse(KeyFrame*, Sim3f& Scw, vpPoints, th, vpReplacePoint)
 * (:1525-1640, the Sim3 form of LoopClosing; the caller decomposes Scw into Tcw = [R | t/s] and Ow as :1534-1535 do) as one call for B
 * keyframes.  The search reads no map state: everything up to `bestDist <= TH_LOW` is a function of the query and the keyframe, and two
 * queries do not see each other.  Only the bookkeeping behind it (:1497-1516, :1622-1636: Replace / AddObservation / AddMapPoint /
 * vpReplacePoint) is sequential; it stays with the caller, who consumes best_idx[q] in query order.  There is no claim order and no
 * assigned[]: two queries may name the same keypoint, and the caller's loop resolves that as the reference's does.
 *
 * Problem b is one keyframe: pose Tcw[12] (row-major 3x4), camera centre Ow[3], its grid blob (built from mvKeysUn: the blob carries
 * every item's x, y, which is where the chi-square test reads the candidate's coordinates -- xy_un itself is not an input of the
 * device call), nt descriptor rows and uright[nt] (mvuRight; NULL = a monocular keyframe, every entry -1).  Query q is a map point:
 * world position X, normal Pn, dist = (min_distance, max_distance, predict_distance), a 64-D descriptor and a flag byte whose bit0
 * (XFH_FUSE_FLAG_ACTIVE) is `pMP && !pMP->isBad() && !pMP->IsInKeyFrame(pKF)` (:1366-1381) resp. `!pMP->isBad() &&
 * !spAlreadyFound.count(pMP)` (:1550).  min_distance / max_distance are GetMinDistanceInvariance() / GetMaxDistanceInvariance() (0.8f *
 * mfMinDistance, 1.2f * mfMaxDistance, MapPoint.cc:502-512); predict_distance is the UNSCALED mfMaxDistance that PredictScale divides
 * (MapPoint.cc:519).  They are separate inputs because 1.2f * x cannot be undone exactly; a caller without access to mfMaxDistance
 * passes max_distance twice and gets a ratio 1.2 times the reference's.
 * All arithmetic is fp32 in the order written unless stated otherwise (the library is built with -ffp-contract=off):
 *
 *   flags bit0 clear                                      -> INACTIVE
 *   xc = ((T[0]*X + T[1]*Y) + T[2]*Z) + T[3], yc / zc from rows 1 / 2          (as xfh_search_projection_device)
 *   zc < 0.0f                                             -> BEHIND          (:1387; zc == 0 and NaN go on)
 *   invz = 1.0f / zc                                      (a FLOAT division, :1393 -- not the double one of :1893)
 *   u = fx*xc/zc + cx;  v = fy*yc/zc + cy                 (Pinhole.cpp:45-46)
 *   !(u >= min_x && u < max_x && v >= min_y && v < max_y) -> OUT_OF_IMAGE    (KeyFrame::IsInImage, KeyFrame.cc:750-753: half-open, NaN is out)
 *   ur = u - bf*invz                                      (:1404)
 *   PO = X - Ow;  dist3D = sqrtf((PO.x*PO.x + PO.y*PO.y) + PO.z*PO.z)
 *   dist3D < min_distance || dist3D > max_distance        -> OUT_OF_RANGE    (:1412)
 *   dot = (PO.x*Pn.x + PO.y*Pn.y) + PO.z*Pn.z;  (double)dot < 0.5 * (double)dist3D -> BAD_ANGLE (:1420: more than 60 degrees)
 *   ratio = predict_distance / dist3D;  level = PredictScale(ratio), see below;  r = th * scale_factors[level]     (:1426-1429)
 *   window: exactly xfh_search_window_device's (KeyFrame::GetFeaturesInArea, KeyFrame.cc:704-748, is the expression sequence of
 *           Frame::GetFeaturesInArea), no skip mask and no uright filter;  n_window = its size;  n_window == 0 -> NO_CANDIDATES (:1433)
 *   per candidate k in visiting order (kpLevel = 0 for every XFeat keypoint, mvInvLevelSigma2[0] = 1.0f):
 *       level > 1                                         -> skipped         (:1454: kpLevel < nPredictedLevel - 1)
 *       with XFH_FUSE_CHI2 (the SE3 form):  ex = u - x_k;  ey = v - y_k
 *           uright[k] >= 0:  er = ur - uright[k];  e2 = (ex*ex + ey*ey) + er*er;  (double)e2 > 7.8  -> skipped   (:1457-1470)
 *           else          :                         e2 =  ex*ex + ey*ey;           (double)e2 > 5.99 -> skipped   (:1471-1481)
 *           (a NaN e2 is not skipped; a NaN uright[k] takes the monocular branch)
 *       dist = DescriptorDistance;  dist < best -> best = dist, best_idx = k   (strict: the candidate visited first wins a tie)
 *   best starts at init_dist (256 in the SE3 form, INT_MAX in the Sim3 form);  n_tested = candidates that reached DescriptorDistance
 *   best_idx >= 0 && best <= th_low -> FUSED, else REJECTED   (TH_LOW = 100, :1497 / :1622)
 *
 * PredictScale (MapPoint.cc:514-529) is ceil(log(ratio) / mfLogScaleFactor) through the float overloads of the host's libm
 * (mfLogScaleFactor = log(mfScaleFactor) in float, Frame.cc:113), clamped to [0, nlevels - 1].  A device logf is not that function to
 * the bit, and the level decides the radius (th or 1.2f * th) and whether there are candidates at all (level <= 1) -- so the device
 * computes no logarithm: xfh_scale_level_thresholds (host, stateless) finds, per level l < nlevels - 1, ratio_max[l] = the largest finite
 * float for which the HOST expression ceilf(logf(ratio) / logf(scale_factor)) is <= l, by bisection over the float's bit pattern, which
 * relies on the host's logf being monotone (glibc's is).  The kernel gets ratio_max and scale_factors (mvScaleFactors, the caller's) by
 * value and computes level = #{ l : ratio > ratio_max[l] }.  That also settles the inputs for which the reference's (int) conversion is
 * undefined: a NaN ratio gives level 0, +Inf gives nlevels - 1, a ratio <= 0 gives level 0.  nlevels <= XFH_FUSE_MAX_LEVELS.
 *
 * Outputs, all exact, all in device memory.  Per query: status (XFH_FUSE_*), best_idx (-1 unless a candidate got under init_dist),
 * best_dist (init_dist where there is none), n_window, n_tested (both 0 for a culled query), level (-1 for a query culled before
 * PredictScale), and optionally proj[q] = (u, v, ur): zeros for INACTIVE and BEHIND, the computed values otherwise.  Per problem: n_fused.
 *
 *   xfh_scale_level_thresholds   host, stateless: ratio_max[nlevels - 1].  XFH_ERR_INVALID_ARG: nlevels outside 1 .. XFH_FUSE_MAX_LEVELS, a
 *                         scale_factor that is not finite or not > 1.
 *   xfh_fuse_project      host, stateless, thread-safe: the per-point arithmetic above for n points and ONE pose down to status
 *                         (BEHIND .. BAD_ANGLE or XFH_FUSE_VISIBLE), level and radius: uvr[i] = (u, v, r), r = 0 for a culled point.  The same
 *                         source lines as the kernel (fuse_math.h).
 *   xfh_fuse_search_device   B problems of nq queries with the same camera, bounds, th and thresholds.  Query arrays: d_points, d_normals,
 *                         d_distances [.][nq][3], d_query_desc [.][nq][64], d_query_flags [.][nq] bytes, problem b's block starting
 *                         query_problem_stride * b queries into each: the stride is nq (own queries per problem) or 0 (all B problems read
 *                         the SAME block: SearchInNeighbors, the current keyframe's points against every neighbour).  d_Tcw [B][12],
 *                         d_Ow [B][3]; grid b at d_grids + b * xfh_grid_bytes(nt), target rows of problem b at d_targets + b *
 *                         target_stride_bytes (as xfh_search_projection_device), d_uright [B][nt] or NULL: the grids and uright of
 *                         xfh_frame_finish_records_device plug in unchanged.  Outputs d_status [B][nq] bytes, d_best_idx / d_best_dist /
 *                         d_n_window / d_n_tested / d_level [B][nq] ints, d_proj_out [B][nq][3] or NULL, d_n_fused [B] ints.  flags:
 *                         XFH_FUSE_CHI2 or 0.  All pointers but cam, bounds, scale_factors and ratio_max are device pointers;
 *                         asynchronous on the ctx stream, no allocation, no workspace, ONE kernel launch (behind a 4 * B byte memset of
 *                         d_n_fused on the same stream).  nt in 1 .. XFH_GRID_MAX_N, nq in 1 .. 2^20 (nothing here sorts queries in LDS),
 *                         B in 1 .. 65535.  XFH_ERR_INVALID_ARG before anything is queued: those ranges, nlevels outside 1 ..
 *                         XFH_FUSE_MAX_LEVELS, a stride other than 0 or nq, a non-finite th, unknown flag bits, a NULL required pointer,
 *                         misaligned pointers (16 bytes for descriptors, targets, the target stride and grids, the element size
 *                         otherwise).  Points, normals, distances, poses, scale tables and descriptors may hold anything, NaN and Inf
 *                         included: no load leaves the buffers the caller named.
 *   xfh_fuse_search       host-pointer convenience form for ONE problem: stages the inputs, builds the grid of the nt keypoints (x, y =
 *                         the undistorted coordinates) with flags 0 and `bounds`, runs the call and copies the results back.
 *                         XFH_ERR_INVALID_ARG for the device form's classes of error (and bounds no grid can be built from) before
 *                         anything is staged or queued.
 * Out of scope: bRight / NLeft != -1 (fisheye stereo).  (The Sim3 SearchByProjection forms are
 * xfh_map_projection_search_device and SearchBySim3 is xfh_sim3_search_device, both below; the two functions that walk DBoW2 feature
 * vectors are xfh_triangulation_search_device and xfh_bow_search_device.) */
#define XFH_FUSE_MAX_LEVELS 16
#define XFH_FUSE_FLAG_ACTIVE 1        /* d_query_flags bit0 */
#define XFH_FUSE_CHI2 1               /* flags: the chi-square reprojection gates of the SE3 form */
enum { XFH_FUSE_INACTIVE = 0, XFH_FUSE_BEHIND = 1, XFH_FUSE_OUT_OF_IMAGE = 2, XFH_FUSE_OUT_OF_RANGE = 3, XFH_FUSE_BAD_ANGLE = 4,
       XFH_FUSE_NO_CANDIDATES = 5, XFH_FUSE_REJECTED = 6, XFH_FUSE_FUSED = 7,
       XFH_FUSE_VISIBLE = 5 /* xfh_fuse_project: the point reaches the search */ };
int xfh_scale_level_thresholds(float scale_factor, int nlevels, float* ratio_max /* [nlevels - 1] */);
int xfh_fuse_project(const float* Tcw, const float* Ow, const xfh_camera* cam, const xfh_grid_bounds* bounds, float th, const float* scale_factors,
                     const float* ratio_max, int nlevels, const float* xyz, const float* normals, const float* distances, int n,
                     float* uvr, float* ur, int* level, uint8_t* status);
int xfh_fuse_search_device(xfh_ctx* ctx, int B, int nq, size_t query_problem_stride, const float* d_points, const float* d_normals,
                           const float* d_distances, const float* d_query_desc, const uint8_t* d_query_flags, const float* d_Tcw, const float* d_Ow,
                           const xfh_camera* cam, const xfh_grid_bounds* bounds, float th, const float* scale_factors, const float* ratio_max, int nlevels,
                           const void* d_grids, const float* d_targets, size_t target_stride_bytes, int nt, const float* d_uright_or_null,
                           int flags, int init_dist, int th_low, uint8_t* d_status, int* d_best_idx, int* d_best_dist, int* d_n_window, int* d_n_tested,
                           int* d_level, float* d_proj_out_or_null, int* d_n_fused);
int xfh_fuse_search(xfh_ctx* ctx, int nq, const float* points, const float* normals, const float* distances, const float* query_desc,
                    const uint8_t* query_flags, const float* Tcw, const float* Ow, const xfh_camera* cam, const xfh_grid_bounds* bounds, float th,
                    const float* scale_factors, const float* ratio_max, int nlevels, const xfh_keypoint* kps, const float* targets, int nt,
                    const float* uright_or_null, int flags, int init_dist, int th_low, uint8_t* status, int* best_idx, int* best_dist, int* n_window,
                    int* n_tested, int* level, float* proj_out_or_null, int* n_fused);

/* ---- SearchForTriangulation over feature-vector nodes, device resident ---------------------------------------------------------------
 * ORBmatcher::SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, vMatchedPairs, bOnlyStereo, bCoarse) (src/ORBmatcher.cc:1092-1331,
 * called once per covisible neighbour from LocalMapping::CreateNewMapPoints, src/LocalMapping.cc:434-466) up to vMatches12, as one call
 * for B keyframe pairs.  Every keypoint of KF1 without a map point is compared with the keypoints of KF2 without a map point that share
 * its vocabulary node, under an epipolar test.  vbMatched2 is created at :1134 and read at :1189 but never written in this function
 * (the write exists only in SearchByBoW, :1038): two keypoints of KF1 never see each other, there is no claim order, two of them may
 * name the same keypoint of KF2 as in the reference, and the call needs no workspace.
 *
 * Node index.  TemplatedVocabulary::transform visits the features in ascending index and FeatureVector::addFeature push_backs, so
 * mFeatVec is "node id ascending, keypoint index ascending inside a node": a function of node_of[i], the NodeId of keypoint i
 * (XFH_NODE_NONE: keypoint i is in no node; every other uint32 is a valid id).  node_of comes either from the caller's own DBoW2 (mFeatVec
 * flattened on the host) or, without a host step, from xfh_bow_transform_device below, which writes the blob itself.
 *   xfh_nodes_bytes / xfh_nodes_pack   host, stateless: node_of[n] -> an opaque, self-contained blob of xfh_nodes_bytes(n) bytes (a multiple
 *                         of 16): a header, the distinct node ids ascending, node_start, the items (keypoint indices, nodes in id order,
 *                         ascending inside a node) and a copy of node_of.  The caller uploads it with xfh_memcpy_h2d (16-byte aligned); one
 *                         blob serves a keyframe on either side.  Packing the same input twice gives identical bytes; padding is zeroed.
 *                         n in 1 .. XFH_GRID_MAX_N.
 *   xfh_nodes_unpack      the test and debug inverse: node_ids[n] (the first *n_nodes meaningful), node_start[n + 1], items[n] (-1 past the
 *                         item count).  A truncated or inconsistent blob is XFH_ERR_INVALID_ARG, never an out-of-bounds access.
 *
 * Problem b is the pair (KF1, KF2_b).  With side1_shared = 1 all B problems read the SAME side-1 arrays (CreateNewMapPoints: the new
 * keyframe against every neighbour; its rows are then served from L2, and desc1_stride_bytes is ignored); with 0 problem b reads its own.
 * Per side and problem: the node blob (b * xfh_nodes_bytes(n) bytes in), xy[n][2] (mvKeysUn, the layout of xfh_frame_finish_records_device's
 * xy_un), uright[n] (mvuRight; NULL = a monocular keyframe, every entry -1), has[n] bytes (non-zero: GetMapPoint(idx) != NULL) -- these
 * three b * n elements in -- and descriptor rows b * desc_stride_bytes in (xfh_record_bytes(nfeatures) lets d_desc point at the desc block
 * of record 0 of a batch).  Per problem: F12[9] row-major, the matrix of Pinhole.cpp:112 (K1^-T [t12]x R12 K2^-1), and ep[2], the epipole
 * of :1105 -- both computed once per pair by the caller with its own Eigen (the reference recomputes the identical F12 per candidate).
 * Scalars: th_low (TH_LOW = 100), epipole_r2 = 100 * mvScaleFactors[0] (:1215), unc = mvLevelSigma2[0] (:1257): every XFeat keypoint has
 * octave 0.  flags: XFH_TRI_ONLY_STEREO = bOnlyStereo, XFH_TRI_COARSE = bCoarse.
 * All arithmetic is fp32 in the order written unless stated otherwise (the library is built with -ffp-contract=off).  For keypoint i of KF1:
 *
 *   has1[i] != 0                                          -> INACTIVE        (:1159)
 *   stereo1 = uright1[i] >= 0 (NULL or NaN: false);  ONLY_STEREO && !stereo1 -> INACTIVE   (:1164-1168)
 *   node = node_of1[i];  node == XFH_NODE_NONE or absent from KF2's node ids -> NO_NODE
 *   a = (x1*F[0] + y1*F[3]) + F[6];  b = (x1*F[1] + y1*F[4]) + F[7];  c = (x1*F[2] + y1*F[5]) + F[8];  den = a*a + b*b   (Pinhole.cpp:115-121)
 *   per member k of KF2's node, in stored (ascending index) order:
 *       has2[k] != 0                                      -> skipped         (:1189)
 *       stereo2 = uright2[k] >= 0;  ONLY_STEREO && !stereo2 -> skipped       (:1192-1196)
 *       -- n_candidates counts the members that got here
 *       !stereo1 && !stereo2:  dx = ep[0] - x2;  dy = ep[1] - y2;  dx*dx + dy*dy < epipole_r2 -> skipped   (:1211-1219)
 *       without XFH_TRI_COARSE:  num = (a*x2 + b*y2) + c;  den == 0 -> skipped;  dsqr = (num*num) / den;
 *                                !((double)dsqr < 3.84 * (double)unc) -> skipped   (a NaN dsqr is skipped; Pinhole.cpp:119-128)
 *       -- n_geom counts the members that got here
 *       dist = DescriptorDistance(row i of KF1, row k of KF2);  dist <= th_low && dist <= best -> best = dist, best_idx = k
 *   best starts at th_low;  best_idx >= 0 -> MATCHED, else n_candidates == 0 -> NO_CANDIDATES, else REJECTED
 *
 * The reference tests `dist>TH_LOW || dist>bestDist` (:1202, continue on strictly greater) BEFORE the geometry and lowers bestDist only for
 * a candidate that passes everything: the result is the least dist over the members that pass every gate with dist <= th_low, and among
 * equal distances the member visited LAST wins -- the opposite of xfh_best2_csr's rule.  The gates are pure, so their order changes
 * neither the result nor the two counts; the kernel applies the geometry first and computes distances only for the n_geom survivors.
 * Outputs, all exact, all in device memory.  Per (problem, i): status (XFH_TRI_*), match12 (vMatches12: idx2 or -1), best_dist (th_low
 * where there is none), n_candidates, n_geom (both 0 for a query that never reached a node).  Per problem: n_matches (nmatches).  The
 * caller builds vMatchedPairs from match12 in ascending i (:1320-1328).
 *
 *   xfh_epipolar_gate     host, stateless, thread-safe: the gates above for ONE keypoint (x1, y1, stereo1) of KF1 against n keypoints of KF2
 *                         that have no map point: pass[k] = XFH_TRI_GATE_SKIPPED (the stereo-only gate; every k when ONLY_STEREO && !stereo1),
 *                         XFH_TRI_GATE_REJECTED (a candidate the epipole or epipolar test drops) or XFH_TRI_GATE_PASSED (it reaches
 *                         DescriptorDistance).  The same source lines as the kernel (tri_math.h).
 *   xfh_triangulation_search_device   B problems with the same n1, n2, flags and scalars.  d_F12 [B][9], d_ep [B][2]; outputs d_status [B][n1]
 *                         bytes, d_match12 / d_best_dist / d_n_candidates / d_n_geom [B][n1] ints, d_n_matches [B] ints.  All pointers are
 *                         device pointers; asynchronous on the ctx stream, no allocation, no workspace, ONE kernel launch (behind a 4 * B
 *                         byte memset of d_n_matches on the same stream).  XFH_ERR_INVALID_ARG before anything is queued: n1 or n2
 *                         outside 1 .. XFH_GRID_MAX_N, B outside 1 .. 65535, side1_shared other than 0 or 1, unknown flag bits, a non-finite
 *                         epipole_r2 or unc, a NULL required pointer, misaligned pointers (16 bytes for descriptor rows, their strides and
 *                         the blobs, the element size otherwise).  Blobs, F12, ep, coordinates and uright may hold anything, NaN and Inf
 *                         included: every count and range read from a blob is clamped and every item is checked against n2 before it
 *                         indexes anything, so no load leaves the buffers the caller named.  The distance of a row that holds a NaN is
 *                         not defined.
 *   xfh_triangulation_search   host-pointer convenience form for ONE problem: packs both node blobs, stages the inputs, runs the call and
 *                         copies the results back.  XFH_ERR_INVALID_ARG for the device form's classes of error before anything is staged
 *                         or queued.
 * Out of scope: mbCheckOrientation and the rotation histogram (:1272-1318; the only caller builds ORBmatcher(0.6f, false),
 * LocalMapping.cc:412); fisheye stereo (mpCamera2, NLeft != -1, the four T12 variants of :1221-1255); KannalaBrandt8::epipolarConstrain;
 * computing F12 or the epipole; and computing the feature vector (DBoW2).  The triangulation of the matched pairs is
 * xfh_triangulate_device; with B > 1 its claim is what makes the batched search equal the per-neighbour reference.  (SearchByBoW, which has a real claim
 * order and a ratio test, is xfh_bow_search_device below.) */
#define XFH_NODE_NONE 0xFFFFFFFFu     /* node_of: the keypoint is in no node of the feature vector */
#define XFH_TRI_ONLY_STEREO 1         /* flags: bOnlyStereo */
#define XFH_TRI_COARSE 2              /* flags: bCoarse */
enum { XFH_TRI_INACTIVE = 0, XFH_TRI_NO_NODE = 1, XFH_TRI_NO_CANDIDATES = 2, XFH_TRI_REJECTED = 3, XFH_TRI_MATCHED = 4 };
enum { XFH_TRI_GATE_SKIPPED = 0, XFH_TRI_GATE_REJECTED = 1, XFH_TRI_GATE_PASSED = 2 };
size_t xfh_nodes_bytes(int n);
int xfh_nodes_pack(const uint32_t* node_of, int n, void* blob /* xfh_nodes_bytes(n) */, int* n_nodes_or_null);
int xfh_nodes_unpack(const void* blob, size_t nbytes, int n, uint32_t* node_ids /* [n] */, int* node_start /* [n + 1] */, int* items /* [n] */, int* n_nodes);
int xfh_epipolar_gate(const float* F12, const float* ep, float epipole_r2, float unc, int flags, float x1, float y1, int stereo1, const float* xy2,
                      const float* uright2_or_null, int n, uint8_t* pass);
int xfh_triangulation_search_device(xfh_ctx* ctx, int B, int n1, int n2, int side1_shared, int flags, int th_low, float epipole_r2, float unc,
                                    const void* d_nodes1, const float* d_xy1, const float* d_uright1_or_null, const uint8_t* d_has1, const float* d_desc1,
                                    size_t desc1_stride_bytes, const void* d_nodes2, const float* d_xy2, const float* d_uright2_or_null,
                                    const uint8_t* d_has2, const float* d_desc2, size_t desc2_stride_bytes, const float* d_F12, const float* d_ep,
                                    uint8_t* d_status, int* d_match12, int* d_best_dist, int* d_n_candidates, int* d_n_geom, int* d_n_matches);
int xfh_triangulation_search(xfh_ctx* ctx, int n1, int n2, int flags, int th_low, float epipole_r2, float unc, const uint32_t* node_of1, const float* xy1,
                             const float* uright1_or_null, const uint8_t* has1, const float* desc1, const uint32_t* node_of2, const float* xy2,
                             const float* uright2_or_null, const uint8_t* has2, const float* desc2, const float* F12, const float* ep, uint8_t* status,
                             int* match12, int* best_dist, int* n_candidates, int* n_geom, int* n_matches);

/* ---- SearchByBoW over feature-vector nodes, device resident ------------------------------------------------------------------------------
 * ORBmatcher::SearchByBoW, both overloads (src/ORBmatcher.cc): the frame form SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) (:408-610;
 * Tracking::TrackReferenceKeyFrame, Tracking.cc:2759, and once per candidate keyframe from Tracking::Relocalization, Tracking.cc:3697) and
 * the keyframe form SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12) (:950-1090; LoopClosing.cc:662, the current keyframe against each
 * covisible keyframe of a candidate), as one call for B problems.  Side 1 holds the queries (the keyframe whose map points are matched),
 * side 2 the targets.  Both overloads walk the two feature vectors with the two-iterator / lower_bound loop, keep best and second best
 * with the strict `<` / `else if <` update from 256, and let an accepted query CLAIM its target (vpMapPointMatches[realIdxF] is tested at
 * :463 and written at :516 -- the vector is all NULL at :412, so only an earlier iteration of this call can have set it; vbMatched2 at :1011
 * and :1038).  The claim makes the loop sequential, but only inside a node: a keypoint is in exactly one node (node_of[i] is a function of
 * i), so a claim made while node A is walked is seen by later queries of node A only; nodes are independent, in any order, and inside a
 * node the queries are resolved in stored (ascending index) order.  Node blobs: xfh_nodes_pack above.
 *
 * Per problem, the contract is this loop.  All integer comparisons are exact; the one float expression is fp32 in the order written (the
 * library is built with -ffp-contract=off):
 *
 *   claimed[k] = 0 for all k
 *   for every node id present on both sides; for the members i of side 1's node in stored order:
 *       active1[i] == 0                              -> INACTIVE
 *       best = second = init_dist; best_idx = -1; n_candidates = 0
 *       for the members k of side 2's node in stored order:
 *           eligible2 && eligible2[k] == 0 -> skip;  claimed[k] -> skip;  ++n_candidates
 *           d = DescriptorDistance(row i, row k)
 *           d < best ? (second = best, best = d, best_idx = k) : (d < second ? second = d : nothing)
 *       accept = best_idx >= 0 && (STRICT_LOW ? best < th_low : best <= th_low) && (float)best < nn_ratio * (float)second
 *       accept -> MATCHED, match12[i] = best_idx, assigned2[best_idx] = i, claimed[best_idx] = 1, ++n_matches
 *       else   -> n_candidates == 0 ? NO_CANDIDATES : REJECTED
 *
 * An active query whose node is XFH_NODE_NONE or absent from side 2 is NO_NODE; an inactive query is INACTIVE whatever its node.  Among
 * equal distances the member visited FIRST wins -- the opposite of the triangulation rule.  match12 is -1 unless MATCHED, best_dist and
 * second_dist are init_dist where there is none, assigned2[k] is -1 for an unclaimed keypoint.
 * The frame form is flags = 0, eligible2 = NULL, active1[i] = "pKF's map point i exists and is not bad" (:445), th_low = TH_LOW = 100
 * (`bestDist1 <= TH_LOW`, :512), init_dist = 256, nn_ratio = mfNNratio; match12 / assigned2 are vpMapPointMatches seen from either side.
 * The keyframe form is XFH_BOW_STRICT_LOW (`bestDist1 < TH_LOW`, :1033) with eligible2[k] = the same predicate on side 2 (:1009-1015);
 * match12 is vpMatches12 by index.  The rotation histogram (:523-538 and :589-607, and its counterpart in the keyframe form) puts every match in bin 0, because every
 * XFeat keypoint has angle -1 (the argument of the projection contract above): it removes nothing, and mbCheckOrientation stays without
 * effect.
 *
 *   xfh_bow_accept        host, stateless, thread-safe: the `accept` line, 1 or 0.  The same source line as the kernel (bow_math.h).
 *   xfh_bow_search_workspace_bytes   bytes of d_workspace for B problems (0 for sizes the call would refuse); n2 does not enter today.
 *   xfh_bow_search_device   B problems with the same n1, n2, flags and scalars.  shared = 0: problem b reads its own two sides; 1: all
 *                         problems read side 1 (blob, active1, rows) of problem 0 (LoopClosing: the current keyframe against its
 *                         covisibles); 2: the same for side 2 (Relocalization: the candidates against one frame); the stride of the
 *                         shared side's rows is ignored.  Per side and problem: the node blob (b * xfh_nodes_bytes(n) bytes in), the flag
 *                         bytes (b * n in; d_eligible2 may be NULL) and descriptor rows b * desc_stride_bytes in.  Outputs are always
 *                         d_status [B][n1] bytes, d_match12 / d_best_dist / d_second_dist / d_n_candidates [B][n1] ints, d_assigned2
 *                         [B][n2] ints, d_n_matches [B] ints.  All pointers are device pointers; asynchronous on the ctx stream, no
 *                         allocation, no host synchronisation: three memsets (n_matches, assigned2, the workspace counters) and two
 *                         kernel launches; every data-dependent iteration count is decided on the device.  The first int[4] per problem
 *                         of the workspace are counters (queries that needed a full re-search, queries resolved, nodes resolved, 0).
 *                         XFH_ERR_INVALID_ARG before anything is queued: n1 or n2 outside 1 .. XFH_GRID_MAX_N, B outside 1 .. 65535,
 *                         shared outside 0 .. 2, unknown flag bits, nn_ratio negative or not finite, th_low < 0, init_dist < 0, a NULL
 *                         required pointer, misaligned pointers (16 bytes for descriptor rows, their strides, the blobs and the
 *                         workspace, 4 for the int outputs).  Blobs may hold anything: every count, range and item read from one is
 *                         clamped or checked before it indexes anything, so no access leaves the buffers the caller named; the results
 *                         of the nodes such a blob misdescribes are unspecified, those of the others are the loop's.  The distance of a
 *                         row that holds a NaN is not defined.
 *   xfh_bow_search        host-pointer convenience form for ONE problem: packs both node blobs, stages the inputs and the workspace, runs
 *                         the call and copies the results back.  XFH_ERR_INVALID_ARG for the device form's classes of error before
 *                         anything is staged or queued.
 * Out of scope: the Nleft != -1 branches (fisheye stereo); computing the BoW or feature vector (xfh_bow_transform_device below);
 * (SearchForInitialization is xfh_init_search_device, the relocalisation and Sim3 SearchByProjection forms are
 * xfh_map_projection_search_device, SearchBySim3 is xfh_sim3_search_device, all below); the PnP and Sim3 solvers that consume the matches. */
#define XFH_BOW_STRICT_LOW 1          /* flags: accept on best < th_low (the keyframe form) instead of best <= th_low */
enum { XFH_BOW_INACTIVE = 0, XFH_BOW_NO_NODE = 1, XFH_BOW_NO_CANDIDATES = 2, XFH_BOW_REJECTED = 3, XFH_BOW_MATCHED = 4 };
int xfh_bow_accept(int best_idx, int best, int second, int th_low, float nn_ratio, int flags);
size_t xfh_bow_search_workspace_bytes(int n1, int n2, int B);
int xfh_bow_search_device(xfh_ctx* ctx, int B, int n1, int n2, int shared, int flags, int init_dist, int th_low, float nn_ratio, const void* d_nodes1,
                          const uint8_t* d_active1, const float* d_desc1, size_t desc1_stride_bytes, const void* d_nodes2,
                          const uint8_t* d_eligible2_or_null, const float* d_desc2, size_t desc2_stride_bytes, void* d_workspace, uint8_t* d_status,
                          int* d_match12, int* d_best_dist, int* d_second_dist, int* d_n_candidates, int* d_assigned2, int* d_n_matches);
int xfh_bow_search(xfh_ctx* ctx, int n1, int n2, int flags, int init_dist, int th_low, float nn_ratio, const uint32_t* node_of1, const uint8_t* active1,
                   const float* desc1, const uint32_t* node_of2, const uint8_t* eligible2_or_null, const float* desc2, uint8_t* status, int* match12,
                   int* best_dist, int* second_dist, int* n_candidates, int* assigned2, int* n_matches);

/* ---- The vocabulary transform: BowVector and node blobs, device resident -------------------------------------------------------------------
 * TemplatedVocabulary::transform(features, v, fv, levelsup) of DBoW2 (thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1194; Frame::ComputeBoW
 * and KeyFrame::ComputeBoW: Tracking.cc:2750, :3661, :2563-2564, LocalMapping.cc:307) for B frames of n rows per call, for the weighting and
 * norm ORBvoc.txt's header `10 6 0 0` selects: TF_IDF, L1_NORM.  It removes the last host round trip between xfh_extract_batch_device and
 * xfh_bow_search_device / xfh_triangulation_search_device: the node blob those two read is written on the device.
 *
 * DBoW2 treats an XFeat row as a 256-bit ORB descriptor: FORB::distance (FORB.cpp:81-101) popcounts the XOR of the first 8
 * int32 of the row, i.e. of the bit patterns of its first 8 floats.  The library reads those 32 bytes as 8 uint32 and never as floats: NaN
 * and Inf patterns are just bits.  Everything here is integers and IEEE doubles in a fixed order, so every output is exact.
 *
 * The vocabulary.  The caller keeps its DBoW2 vocabulary (KeyFrameDatabase needs it) and flattens m_nodes, in node-id order, into parent[],
 * word_id[], weight[] and desc[][32] (FORB::L); INTEGRATION.md has the loop.  Node 0 is the root; its parent, descriptor and weight are
 * ignored.  CONTRACT: the children of a node are the nodes that name it as parent, in ascending id -- loadFromTextFile's push_back order
 * (TemplatedVocabulary.h:1385-1392).  A node is a leaf iff it has no children (isLeaf()), whatever its word_id and whatever the text file's
 * leaf flag said: loadFromTextFile's `while(!f.eof())` loop turns a trailing newline into one extra node under the root with a zero
 * descriptor, weight 0, word_id 0 and no children; it is accepted, and a feature that lands on it is stopped like any w <= 0.
 *   xfh_vocab_bytes / xfh_vocab_pack   host, stateless: the arrays -> an opaque, self-contained blob of xfh_vocab_bytes(n_nodes) bytes
 *                         (0 for n_nodes < 1).  The nodes are reordered into slots so that the children of a node are one contiguous,
 *                         32-byte aligned run of descriptors in child order; per slot {first_child_slot, n_children, node_id, word_id} and,
 *                         in an array apart, weight.  Padding is zeroed: two packs of the same input give identical bytes.  The caller uploads
 *                         it once with xfh_memcpy_h2d (16-byte aligned).  XFH_ERR_INVALID_ARG: n_nodes < 2, parent[i] >= i for an i >= 1 (the
 *                         reference would index past m_nodes), a root without children, more than XFH_VOCAB_MAX_CHILDREN children of one
 *                         node, a tree deeper than XFH_VOCAB_MAX_DEPTH, L outside 1 .. 10 (the loader's own range), a NULL array.
 *   xfh_vocab_unpack      the test and debug inverse, in node-id order (parent[0] = 0; the root's weight and row come back as zero).  A
 *                         truncated or inconsistent blob is XFH_ERR_INVALID_ARG, never an out-of-bounds access.
 *   xfh_vocab_descend     host, stateless, thread-safe: transform(feature, word_id, weight, nid, levelsup) (:1218-1259) for ONE row, the same
 *                         source lines as the kernel (vocab_math.h).  row32: 32 bytes.  Start at the root; at each level d(child) is the
 *                         popcount of the XOR over the 8 words and the first child with the least d wins (strict `<` over the children in
 *                         order); stop at a node without children.  *word_id and *weight are that leaf's.  nid_level = L - levelsup:
 *                         *node_id is 0 when nid_level <= 0, the path's node at level nid_level when the path is that long, otherwise the
 *                         leaf -- a documented deviation: the reference leaves nid uninitialised there (:1150-1155, :1251).  levelsup < 0 is
 *                         XFH_ERR_INVALID_ARG.  Hostile blobs: the node count is clamped to what nbytes holds, every slot index and child
 *                         count is clamped before it indexes anything, and the loop runs at most XFH_VOCAB_MAX_DEPTH levels, so such a
 *                         blob can neither leave the buffer nor loop forever; results for a blob xfh_vocab_pack did not write are
 *                         unspecified.
 *
 * Per frame, over ALL n rows in index order (zero padding rows included: the reference hands every row of mDescriptors to DBoW2):
 *   word[i], weight[i] = the leaf's (also when stopped);  node_of[i] = the node id above, or XFH_NODE_NONE when !(weight[i] > 0) (a NaN
 *   weight stops the feature too) -- `if(w > 0)` (:1152)
 *   nodes     byte for byte what xfh_nodes_pack(node_of) writes: FeatureVector::addFeature in feature order
 *   BowVector the distinct words of the features that are not stopped, ascending;  val(word) = ((w + w') + w'') ..., ONE double add per
 *             feature in index order (BowVector::addWeight; the iterated sum is not count * w in general);  norm = the left-to-right double
 *             sum of |val| over ascending word id, from 0.0;  val /= norm when norm > 0 (BowVector::normalize(L1));  bow_ids / bow_vals hold
 *             them in that order, unused entries are id 0xFFFFFFFF, value 0;  n_words is the count
 *
 *   xfh_bow_transform_workspace_bytes   bytes of d_workspace for B frames of n rows (0 for sizes the call would refuse).
 *   xfh_bow_transform_device   flags = XFH_BOWT_TF_IDF_L1.  d_vocab: the uploaded blob, vocab_bytes its size.  Frame b reads its rows b *
 *                         desc_stride_bytes in (xfh_record_bytes(nfeatures) lets d_desc point at the desc block of record 0 of a batch) and
 *                         writes d_word / d_node_of / d_bow_ids [B][n] uint32, d_weight / d_bow_vals [B][n] doubles, d_nodes [B] blobs of
 *                         xfh_nodes_bytes(n) bytes (ready for xfh_bow_search_device and xfh_triangulation_search_device), d_n_words [B]
 *                         ints.  All pointers are device pointers; asynchronous on the ctx stream, no allocation, no host
 *                         synchronisation, two kernel launches; two runs give identical bytes.  XFH_ERR_INVALID_ARG before anything is
 *                         queued: n outside 1 .. XFH_GRID_MAX_N, B outside 1 .. 65535, levelsup < 0, any other flags (the other
 *                         weightings and norms), vocab_bytes < xfh_vocab_bytes(2), a NULL pointer, misaligned pointers (16 bytes for the
 *                         vocabulary, the rows and their stride, the workspace and d_nodes, 8 for the doubles, 4 for the rest).  The
 *                         vocabulary blob may hold anything (see xfh_vocab_descend).
 *   xfh_bow_transform     host-pointer convenience form for ONE frame: stages the vocabulary blob (all of it, per call: a test and
 *                         debugging form), the rows and the workspace, runs the call and copies the results back.
 * Out of scope: the yml and binary vocabulary loaders (and the text loader: the caller has DBoW2's);
 * vocabulary creation; the other weightings and norms; skipping padding rows.  (KeyFrameDatabase and L1Scoring::score: the next section.) */
#define XFH_VOCAB_MAX_CHILDREN 32     /* children of one vocabulary node (ORBvoc: k = 10) */
#define XFH_VOCAB_MAX_DEPTH 32        /* levels below the root (ORBvoc: L = 6) */
#define XFH_BOWT_TF_IDF_L1 0          /* flags: WeightingType TF_IDF, ScoringType L1_NORM */
size_t xfh_vocab_bytes(int n_nodes);
int xfh_vocab_pack(int n_nodes, int L, const uint32_t* parent, const uint32_t* word_id, const double* weight, const uint8_t* desc /* [n_nodes][32] */,
                   void* blob /* xfh_vocab_bytes(n_nodes) */, int* max_children_or_null, int* depth_or_null);
int xfh_vocab_unpack(const void* blob, size_t nbytes, int n_nodes, int* L, uint32_t* parent, uint32_t* word_id, double* weight,
                     uint8_t* desc /* [n_nodes][32] */, int* max_children_or_null, int* depth_or_null);
int xfh_vocab_descend(const void* blob, size_t nbytes, int levelsup, const void* row32, uint32_t* word_id, uint32_t* node_id, double* weight);
size_t xfh_bow_transform_workspace_bytes(int n, int B);
int xfh_bow_transform_device(xfh_ctx* ctx, int B, int n, int levelsup, int flags, const void* d_vocab, size_t vocab_bytes, const float* d_desc,
                             size_t desc_stride_bytes, void* d_workspace, uint32_t* d_word, uint32_t* d_node_of, double* d_weight, void* d_nodes,
                             uint32_t* d_bow_ids, double* d_bow_vals, int* d_n_words);
int xfh_bow_transform(xfh_ctx* ctx, int n, int levelsup, int flags, const void* vocab, size_t vocab_bytes, const float* desc, uint32_t* word,
                      uint32_t* node_of, double* weight, void* nodes /* xfh_nodes_bytes(n) */, uint32_t* bow_ids, double* bow_vals, int* n_words);

/* ---- KeyFrameDatabase query: shared words, L1 score, candidates, device resident ---------------------------------------------------------
 * The two database functions the reference calls (src/KeyFrameDatabase.cc), with L1Scoring::score (thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68):
 *   DetectRelocalizationCandidates(Frame*, Map*)                              :733-845    Tracking.cc:3665 (Relocalization)         XFH_BOWDB_FORM_RELOC
 *   DetectNBestCandidates(KeyFrame*, vpLoopCand, vpMergeCand, nNumCandidates) :604-730    LoopClosing.cc:491 (every keyframe)       XFH_BOWDB_FORM_NBEST
 * They are pure functions of the query BowVector, the database BowVectors, the insertion order of the keyframes, each keyframe's first
 * covisibility neighbours, a connected-keyframe set and ONE persistent float per keyframe (mRelocScore resp. mPlaceRecognitionScore).
 * Everything is integers, IEEE doubles and fp32 adds in a fixed order, so every output is exact.
 *
 * The database is plain device arrays in the layout xfh_bow_transform_device writes: d_db_ids [n_slots][db_stride] uint32 ascending,
 * d_db_vals [n_slots][db_stride] doubles, d_db_n_words [n_slots] ints.  A slot with n_words <= 0 is empty (erase = write 0); entries past
 * n_words are never read.  With db_stride == n, xfh_bow_transform_device called with d_bow_ids + slot * n, d_bow_vals + slot * n and
 * d_n_words + slot writes a keyframe straight into its slot.  There is no database object, no inverted file and no `add` entry point: a
 * query scans every slot.  PRECONDITION: a bad keyframe is erased before the query (the reference's `if(pKFi->isBad()) continue;` at :712
 * does not advance its iterator and would spin forever; it is not modelled).
 *
 * What one query computes, per problem b, with v1 = the query and slot s = keyframe s:
 *   common[s]   = |ids(v1) AND ids(s)| (mnRelocWords / mnPlaceRecognitionWords of a listed keyframe: mvInvertedFile[w] holds a keyframe at
 *                 most once), 0 for an empty slot
 *   score[s]    = L1Scoring::score(v1, s): sum = 0.0; for the shared ids in ASCENDING id: sum += (fabs(vi - wi) - fabs(vi)) - fabs(wi), vi of
 *                 v1, wi of s; score = -sum / 2.0.  -0.0 where nothing is shared.  Computed for every slot.
 *   first[s]    = the least shared id (internal: the workspace)
 *   status[s]   = XFH_BOWDB_EMPTY        n_words <= 0
 *                 XFH_BOWDB_NOT_SHARING  common == 0 (also when the slot is excluded)
 *                 XFH_BOWDB_EXCLUDED     d_exclude[b][s] != 0: spConnectedKF (:626), and the query keyframe itself when it is in the database
 *                 XFH_BOWDB_BELOW_MIN / XFH_BOWDB_SCORED   the LISTED slots (lKFsSharingWords), see below
 *   max_common  = max of common over the listed slots; min_common = (int)((float)max_common * 0.8f); a listed slot is SCORED iff
 *                 common > min_common (strictly), otherwise BELOW_MIN
 *   state[s]    = (float)score[s] for the SCORED slots ONLY (`pKFi->mRelocScore=si`); every other entry keeps its value
 *   the list    = the SCORED slots ordered by (first[s], seq[s], s): the order in which the walk over the inverted file lists them (the
 *                 query's words ascending, inside a word the order of the `add` calls).  For list entry r with slot s, si = (float)score[s]:
 *                   acc = si; best = s; best_score = si;
 *                   for j in 0 .. nn-1: t = neigh[s][j]; skip when t < 0, t >= n_slots or t is not LISTED;
 *                       acc += state[t];                                   (fp32, in neighbour order)
 *                       if (state[t] > best_score) { best = t; best_score = state[t]; }
 *                 state[t] is read AFTER the writes above: a neighbour that is BELOW_MIN contributes the value an EARLIER query left in
 *                 d_state, as mRelocScore / mPlaceRecognitionScore do in the reference.  The caller owns d_state and zero-fills it once
 *                 (the KeyFrame constructors initialise mPlaceRecognitionScore(0) and leave mRelocScore uninitialised).
 *                 list_slot / list_acc / list_best [r] = s / acc / best, -1 / 0 / -1 past n_scored
 *   best_acc    = 0; over the list: if (acc > best_acc) best_acc = acc
 *   candidates  RELOC: the list entries with acc > 0.75f * best_acc, in list order;
 *               NBEST: all list entries, stable-sorted by acc descending (list::sort with a.first > b.first);
 *               then, in that order, an entry is dropped when an EARLIER entry of the sequence has the same best (spAlreadyAddedKF).
 *               cand_slot / cand_acc [k] = best / acc of the k-th survivor, -1 / 0 past n_candidates.
 *   header      d_header[b][XFH_BOWDB_HEADER_INTS] = n_listed, max_common, min_common, n_scored, n_candidates, 0, 0, 0;  d_best_acc[b]
 * The map tests (GetMap(), IsBad()) and the nNumCandidates caps select from cand_slot without changing it; they stay with the caller, as
 * do the KeyFrame pointers.
 *
 *   xfh_bow_score         host, stateless, thread-safe: L1Scoring::score on two ascending id arrays through the kernel's own source lines
 *                         (bowdb_math.h); *n_common and *first_common (0xFFFFFFFF when nothing is shared) as above.  n1 or n2 < 0, or a
 *                         NULL pointer (an array may be NULL when its count is 0): XFH_ERR_INVALID_ARG.
 *   xfh_bowdb_query_workspace_bytes   bytes of d_workspace for B queries against n_slots slots (0 for sizes the call would refuse).
 *   xfh_bowdb_query_device   B queries against ONE database.  Queries in the transform's layout: d_q_ids / d_q_vals [B][q_stride], d_q_n_words
 *                         [B].  Shared: the database; d_seq [n_slots] uint32 insertion sequence, or NULL (= the slot index; a reused slot
 *                         needs it; equal values order by slot); d_neigh [n_slots][nn] int32, the first nn entries of
 *                         GetBestCovisibilityKeyFrames in its order, an entry < 0 or >= n_slots means none (NULL allowed when nn == 0).  Per
 *                         problem: d_exclude [B][n_slots] bytes or NULL; d_state [B][n_slots] floats, in/out; outputs d_common (int32),
 *                         d_score (double), d_status (bytes), d_list_slot / d_list_best / d_cand_slot (int32), d_list_acc / d_cand_acc
 *                         (float), all [B][n_slots]; d_header, d_best_acc.  All pointers are device pointers; asynchronous on the ctx
 *                         stream, no allocation, no host synchronisation, two kernel launches; two runs from the same inputs give identical
 *                         bytes.  XFH_ERR_INVALID_ARG before anything is queued: n_slots outside 1 .. XFH_BOWDB_MAX_SLOTS, B outside 1 ..
 *                         65535, a stride < 1 or > XFH_GRID_MAX_N, nn outside 0 .. XFH_BOWDB_MAX_NEIGHBOURS, an unknown form, a NULL
 *                         required pointer, misaligned pointers (8 bytes for doubles, 4 for 32-bit entries, 16 for the workspace).
 *                         Hostile input: every n_words is clamped to [0, stride] before use and neighbour entries are range-checked before
 *                         they index; ids that are not ascending give unspecified results but no out-of-bounds access and no endless
 *                         loop; NaN values give unspecified ordering.
 *   xfh_bowdb_query       host-pointer convenience form for ONE query: stages everything, runs the call and copies state and the outputs back.
 * Design note: the dense scan reads the whole database per query where the host's inverted file touches only the shared postings.  Whether
 * the scan wins at a given database size has NOT been measured against the host walk; profiles/bow_database.md has the kernel times alone.
 * Out of scope: the inverted file itself, the map tests and caps, DetectCandidates / DetectLoopCandidates / DetectBestCandidates (never called). */
#define XFH_BOWDB_MAX_SLOTS 8192       /* keyframe slots per database (the select kernel sorts one query's list in the LDS of one workgroup) */
#define XFH_BOWDB_MAX_NEIGHBOURS 16    /* covisibility neighbours per keyframe (the reference asks for 10) */
#define XFH_BOWDB_HEADER_INTS 8
#define XFH_BOWDB_FORM_RELOC 0         /* DetectRelocalizationCandidates */
#define XFH_BOWDB_FORM_NBEST 1         /* DetectNBestCandidates */
#define XFH_BOWDB_EMPTY 0
#define XFH_BOWDB_NOT_SHARING 1
#define XFH_BOWDB_EXCLUDED 2
#define XFH_BOWDB_BELOW_MIN 3
#define XFH_BOWDB_SCORED 4
int xfh_bow_score(const uint32_t* ids1, const double* vals1, int n1, const uint32_t* ids2, const double* vals2, int n2, double* score,
                  int* n_common, uint32_t* first_common);
size_t xfh_bowdb_query_workspace_bytes(int n_slots, int B);
int xfh_bowdb_query_device(xfh_ctx* ctx, int B, int n_slots, int form, const uint32_t* d_q_ids, const double* d_q_vals, const int* d_q_n_words,
                           int q_stride, const uint32_t* d_db_ids, const double* d_db_vals, const int* d_db_n_words, int db_stride,
                           const uint32_t* d_seq_or_null, const int32_t* d_neigh, int nn, const uint8_t* d_exclude_or_null, float* d_state,
                           void* d_workspace, int32_t* d_common, double* d_score, uint8_t* d_status, int32_t* d_header, float* d_best_acc,
                           int32_t* d_list_slot, float* d_list_acc, int32_t* d_list_best, int32_t* d_cand_slot, float* d_cand_acc);
int xfh_bowdb_query(xfh_ctx* ctx, int n_slots, int form, const uint32_t* q_ids, const double* q_vals, int q_n_words, const uint32_t* db_ids,
                    const double* db_vals, const int* db_n_words, int db_stride, const uint32_t* seq_or_null, const int32_t* neigh, int nn,
                    const uint8_t* exclude_or_null, float* state, int32_t* common, double* score, uint8_t* status, int32_t* header,
                    float* best_acc, int32_t* list_slot, float* list_acc, int32_t* list_best, int32_t* cand_slot, float* cand_acc);

/* ---- SearchByProjection of map points with a claim: the Sim3 forms and the relocalisation form, device resident -----------------------
 * Three reference functions as one call (src/ORBmatcher.cc):
 *   SearchByProjection(KeyFrame*, Sim3f& Scw, vpPoints, vpMatched, th, ratioHamming)                              :612-717    LoopClosing.cc:777, :964
 *   SearchByProjection(KeyFrame*, Sim3f& Scw, vpPoints, vpPointsKFs, vpMatched, vpMatchedKF, th, ratioHamming)    :719-831    LoopClosing.cc:755
 *   SearchByProjection(Frame& CurrentFrame, KeyFrame*, sAlreadyFound, th, ORBdist)                                :2074-2195  Tracking.cc:3785, :3799 (Relocalization)
 * Unlike Fuse they CLAIM: an accepted query writes vpMatched[idx] (:710, :823) resp. CurrentFrame.mvpMapPoints[i2] (:2153), and a later
 * query skips that keypoint (:689, :802, :2137).  The loop is therefore sequential in the query order; the library resolves it on the
 * device with the resolver of xfh_search_projection_device and gives the sequential answer.
 *
 * Problem b is one target frame / keyframe: nt keypoints, their grid blob, their descriptor rows, pose Tcw[12] (row-major 3x4) and camera
 * centre Ow[3] -- the caller decomposes Scw into Tcw = [R | t/s] and Ow as :621-622 do, resp. takes both from the frame pose
 * (:2078-2079) -- and taken[nt], nonzero where vpMatched[idx] != NULL resp. mvpMapPoints[i2] != NULL at entry (NULL: none).  Query q is a
 * map point in the reference's iteration order: world position X, normal Pn, dist = (min_distance, max_distance, predict_distance), a
 * 64-D descriptor and a flag byte -- exactly the query arrays of xfh_fuse_search_device; bit0 (XFH_MAPPROJ_FLAG_ACTIVE) is `!pMP->isBad()
 * && !spAlreadyFound.count(pMP)` (:636, :744) resp. `pMP && !pMP->isBad() && !sAlreadyFound.count(pMP)` (:2093-2095).  The loop, fp32 in
 * the order written (the library is built with -ffp-contract=off):
 *
 *   taken[k] = d_taken ? d_taken[k] != 0 : 0;  assigned[k] = -1;  n_matches = 0
 *   for q = 0 .. nq-1, in this order:
 *     flags[q] bit0 clear                                 -> INACTIVE
 *     xc, yc, zc = Tcw * X                                (each row as ((m0*x + m1*y) + m2*z) + m3, as Fuse)
 *     form & XFH_MAPPROJ_CULL_BEHIND and zc < 0.0f        -> BEHIND          (:646 / :754; the relocalisation form has no such test)
 *     form & XFH_MAPPROJ_PROJECT_INVZ:  invz = 1.0f / zc;  x = xc*invz;  y = yc*invz;  u = fx*x + cx;  v = fy*y + cy      (:758-763)
 *     otherwise (Pinhole::project):     u = fx*xc/zc + cx;  v = fy*yc/zc + cy                                             (:650, :2101)
 *     form & XFH_MAPPROJ_BOUNDS_CLOSED: u < min_x || u > max_x || v < min_y || v > max_y -> OUT_OF_IMAGE   (a NaN passes, :2103-2106)
 *     otherwise (IsInImage): !(u >= min_x && u < max_x && v >= min_y && v < max_y)       -> OUT_OF_IMAGE   (half-open, a NaN is out)
 *     PO = X - Ow;  dist3D = sqrtf((PO.x*PO.x + PO.y*PO.y) + PO.z*PO.z);  dist3D < min || dist3D > max     -> OUT_OF_RANGE
 *     form & XFH_MAPPROJ_CHECK_ANGLE and (double)((PO.x*Pn.x + PO.y*Pn.y) + PO.z*Pn.z) < 0.5 * (double)dist3D -> BAD_ANGLE  (:668 / :781)
 *     level = #{ l : predict_distance / dist3D > ratio_max[l] } (xfh_scale_level_thresholds, as Fuse);  r = th * scale_factors[level]
 *     n_window = members of the window (exactly xfh_search_window_device's window, before any filter)
 *     per member k in visiting order:  taken[k] -> skipped;  level > 1 -> skipped (every XFeat keypoint has octave 0: :694, :807, and the
 *         level window of Frame::GetFeaturesInArea at :2124);  ++n_tested;
 *         d = DescriptorDistance;  d < best -> best = d, best_idx = k              (best starts at init_dist, 256 in all three forms)
 *     accept = best_idx >= 0 && (float)best <= accept_max
 *     accept -> MATCHED, match_idx[q] = best_idx, assigned[best_idx] = q, taken[best_idx] = 1, ++n_matches
 *     else   -> n_tested == 0 ? NO_CANDIDATES : REJECTED
 *
 * accept_max is ONE float the caller computes as the reference does: (float)TH_LOW * ratioHamming (int times float, :708 / :821) for the
 * Sim3 forms, (float)ORBdist (:2151) for the relocalisation form.  The forms are flag sets: XFH_MAPPROJ_FORM_SIM3 (:612),
 * XFH_MAPPROJ_FORM_SIM3_KF (:719) and XFH_MAPPROJ_FORM_RELOC (:2074); any combination of the four bits is valid.
 * Where the reference's observable result does not depend on a distinction it is not modelled: the reference leaves a query whose window
 * is empty (:678) before the loop and one whose members are all skipped after it, with the same outcome, and here both are NO_CANDIDATES;
 * in the relocalisation form at level > 1 the reference's vIndices2 is empty already, here n_window still counts the members, and the
 * outcome (no match) is the same.  vpMatchedKF of :824 is vpPointsKFs[assigned[k]]: caller bookkeeping, as are the pointer writes.  The
 * rotation histogram of :2156-2192 removes nothing: every XFeat keypoint has angle -1, so rot = 0 for every match and all land in one bin.
 *
 * Outputs, all exact, all in device memory.  Per query: status (XFH_MAPPROJ_*, numbered like XFH_FUSE_*), match_idx (-1 unless MATCHED),
 * best_dist (init_dist where no candidate got under it), n_window, n_tested (counted when the query's turn came, i.e. after the claims of
 * the queries before it), level (-1 for a query culled before PredictScale), optionally proj[q] = (u, v, r): zeros for INACTIVE and
 * BEHIND, r = 0 for every culled query.  Per keypoint: assigned[k] = the query that claimed it or -1; every match claims, so a keypoint
 * is assigned at most once.  Per problem: n_matches.
 *
 *   xfh_map_project       host, stateless, thread-safe: the per-point arithmetic above for n points and ONE pose down to status (BEHIND ..
 *                         BAD_ANGLE or XFH_MAPPROJ_VISIBLE), level and radius: uvr[i] = (u, v, r).  The same source lines as the kernel
 *                         (mapproj_math.h).
 *   xfh_map_projection_search_workspace_bytes   bytes of d_workspace for B problems (0 for sizes the call would refuse).
 *   xfh_map_projection_search_device   B problems with the same nq, nt, camera, bounds, th, form and thresholds.  d_points, d_normals,
 *                         d_distances [B][nq][3], d_query_desc [B][nq][64], d_query_flags [B][nq] bytes, d_Tcw [B][12], d_Ow [B][3],
 *                         d_taken [B][nt] bytes or NULL: all per problem.  target_shared = 0: grid b at d_grids + b * xfh_grid_bytes(nt),
 *                         target rows of problem b at d_targets + b * target_stride_bytes, as xfh_fuse_search_device.  target_shared = 1:
 *                         every problem reads the grid and the rows of problem 0 and the stride is ignored -- LoopClosing's shape (several
 *                         hypotheses Scw with their own vpPoints against the one current keyframe) and Relocalization's (several candidate
 *                         keyframes against the one current frame); taken stays per problem.  Outputs d_status [B][nq] bytes, d_match_idx /
 *                         d_best_dist / d_n_window / d_n_tested / d_level [B][nq] ints, d_proj_out [B][nq][3] or NULL, d_assigned [B][nt]
 *                         ints, d_n_matches [B] ints.  The first four ints of problem b's part of the workspace (which starts b *
 *                         xfh_search_projection_workspace_bytes(nq, nt, 1) bytes in) hold afterwards: rounds of the resolver, queries it searched again in full, 0, 0.  All pointers but cam, bounds,
 *                         scale_factors and ratio_max are device pointers; asynchronous on the ctx stream, no allocation, no host
 *                         synchronisation, THREE kernel launches; the data-dependent round count is decided on the device.  nq, nt in 1 ..
 *                         XFH_GRID_MAX_N, B in 1 .. 65535.  XFH_ERR_INVALID_ARG before anything is queued: those ranges, nlevels outside 1 ..
 *                         XFH_FUSE_MAX_LEVELS, unknown form bits, target_shared outside 0 .. 1, a non-finite th or accept_max, accept_max <
 *                         0, a NULL required pointer, misaligned pointers (16 bytes for descriptors, targets, the target stride, grids and the
 *                         workspace, the element size otherwise).  Points, normals, distances, poses, camera centres and descriptors may
 *                         hold anything, NaN and Inf included: no load leaves the buffers the caller named.  Many queries piled on one spot
 *                         cost what xfh_search_projection_device says of that case: exact and terminating, but seconds.
 *   xfh_map_projection_search   host-pointer convenience form for ONE problem: stages the inputs and the workspace, builds the grid of the
 *                         nt keypoints (x, y = the undistorted coordinates) with flags 0 and `bounds`, runs the call and copies the results
 *                         back.  XFH_ERR_INVALID_ARG for the device form's classes of error (and bounds no grid can be built from) before
 *                         anything is staged or queued.
 * Out of scope: fisheye
 * stereo; the PnP and Sim3 solvers that consume the matches. */
#define XFH_MAPPROJ_FLAG_ACTIVE 1     /* d_query_flags bit0 */
#define XFH_MAPPROJ_CULL_BEHIND 1     /* form bits */
#define XFH_MAPPROJ_CHECK_ANGLE 2
#define XFH_MAPPROJ_PROJECT_INVZ 4
#define XFH_MAPPROJ_BOUNDS_CLOSED 8
#define XFH_MAPPROJ_FORM_SIM3 (XFH_MAPPROJ_CULL_BEHIND | XFH_MAPPROJ_CHECK_ANGLE)
#define XFH_MAPPROJ_FORM_SIM3_KF (XFH_MAPPROJ_CULL_BEHIND | XFH_MAPPROJ_CHECK_ANGLE | XFH_MAPPROJ_PROJECT_INVZ)
#define XFH_MAPPROJ_FORM_RELOC XFH_MAPPROJ_BOUNDS_CLOSED
enum { XFH_MAPPROJ_INACTIVE = 0, XFH_MAPPROJ_BEHIND = 1, XFH_MAPPROJ_OUT_OF_IMAGE = 2, XFH_MAPPROJ_OUT_OF_RANGE = 3, XFH_MAPPROJ_BAD_ANGLE = 4,
       XFH_MAPPROJ_NO_CANDIDATES = 5, XFH_MAPPROJ_REJECTED = 6, XFH_MAPPROJ_MATCHED = 7,
       XFH_MAPPROJ_VISIBLE = 5 /* xfh_map_project: the point reaches the search */ };
int xfh_map_project(const float* Tcw, const float* Ow, const xfh_camera* cam, const xfh_grid_bounds* bounds, float th, const float* scale_factors,
                    const float* ratio_max, int nlevels, int form, const float* xyz, const float* normals, const float* distances, int n,
                    float* uvr, int* level, uint8_t* status);
size_t xfh_map_projection_search_workspace_bytes(int nq, int nt, int B);
int xfh_map_projection_search_device(xfh_ctx* ctx, int form, int B, int nq, const float* d_points, const float* d_normals, const float* d_distances,
                                     const float* d_query_desc, const uint8_t* d_query_flags, const float* d_Tcw, const float* d_Ow,
                                     const xfh_camera* cam, const xfh_grid_bounds* bounds, float th, const float* scale_factors, const float* ratio_max,
                                     int nlevels, const void* d_grids, const float* d_targets, size_t target_stride_bytes, int target_shared, int nt,
                                     const uint8_t* d_taken_or_null, int init_dist, float accept_max, void* d_workspace, uint8_t* d_status,
                                     int* d_match_idx, int* d_best_dist, int* d_n_window, int* d_n_tested, int* d_level, float* d_proj_out_or_null,
                                     int* d_assigned, int* d_n_matches);
int xfh_map_projection_search(xfh_ctx* ctx, int form, int nq, const float* points, const float* normals, const float* distances,
                              const float* query_desc, const uint8_t* query_flags, const float* Tcw, const float* Ow, const xfh_camera* cam,
                              const xfh_grid_bounds* bounds, float th, const float* scale_factors, const float* ratio_max, int nlevels,
                              const xfh_keypoint* kps, const float* targets, int nt, const uint8_t* taken_or_null, int init_dist, float accept_max,
                              uint8_t* status, int* match_idx, int* best_dist, int* n_window, int* n_tested, int* level, float* proj_out_or_null,
                              int* assigned, int* n_matches);

/* ---- SearchBySim3: two keyframes' map points projected into each other and searched, device resident ---------------------------------
 * ORBmatcher::SearchBySim3(KeyFrame* pKF1, KeyFrame* pKF2, vpMatches12, const Sim3f& S12, th) (src/ORBmatcher.cc:1642-1859; the reference's own
 * LoopClosing.cc no longer calls it, a caller that refines S12 against a candidate keyframe does) up to vpMatches12, as one call for B keyframe pairs.  Both directions
 * read no map state and no query sees another -- there is no claim -- so the whole function is two independent searches and the
 * agreement step behind them (:1840-1856).  What stays with the caller: S12 and its inverse (its own Sophus), vbAlreadyMatched1 / 2 as
 * :1662-1675 compute them (folded into the flag bytes), and the pointer write vpMatches12[i1] = vpMapPoints2[match12[i1]] (:1852).
 *
 * Problem b is a keyframe pair.  Side s (1 or 2) is xfh_sim3_side: n keypoints, their grid blob (built from mvKeysUn), the keyframe's
 * descriptor rows desc[n][64] (mDescriptors), and per keypoint i the map point it holds (vpMapPoints_s[i]): world position points[i],
 * dist[i] = (min_distance, max_distance, predict_distance) as in Fuse above, the map point's OWN descriptor mp_desc[i][64]
 * (pMP->GetDescriptor(), :1730 -- not the keyframe's row i) and a flag byte whose bit0 (XFH_SIM3_FLAG_ACTIVE) is `pMP &&
 * !vbAlreadyMatched_s[i] && !pMP->isBad()` (:1685-1689, :1765-1769); the arrays of a keypoint without a map point may hold anything.
 * Tw[12] is the side's pose (row-major 3x4).  Per problem: M21[12] and M12[12], the row-major 3x4 [s*R | t] of S12.inverse() and S12,
 * so that M * p is the Sim3 applied to p.  Bit equality with Sophus' Sim3 * Vector3 is not claimed, as for every pose product in this
 * header.  ONE camera and ONE bounds struct serve both directions: the reference uses pKF1's intrinsics for both (:1644-1647).
 * All arithmetic is fp32 in the order written unless stated otherwise (the library is built with -ffp-contract=off).
 * Direction 1->2, for i1 in any order (2->1 is the mirror image with T2w, M12 and side 1's grid and rows):
 *
 *   flags1[i1] bit0 clear                                 -> INACTIVE
 *   p1 = T1w * X;  p2 = M21 * p1                          (each row as ((m0*x + m1*y) + m2*z) + m3, as Fuse)
 *   p2.z < 0.0f                                           -> BEHIND          (:1696; +-0 and NaN go on)
 *   invz = (float)(1.0 / (double)p2.z)                    (a DOUBLE division rounded once, :1699)
 *   x = p2.x*invz;  y = p2.y*invz;  u = fx*x + cx;  v = fy*y + cy            (:1700-1704)
 *   !(u >= min_x && u < max_x && v >= min_y && v < max_y) -> OUT_OF_IMAGE    (KeyFrame::IsInImage: half-open, NaN is out)
 *   dist3D = sqrtf((p2.x*p2.x + p2.y*p2.y) + p2.z*p2.z)   (the norm of the CAMERA-frame point, :1712 -- not |X - Ow| as in Fuse)
 *   dist3D < min_distance || dist3D > max_distance        -> OUT_OF_RANGE    (:1715)
 *   level = #{ l : predict_distance / dist3D > ratio_max[l] } (xfh_scale_level_thresholds, as Fuse);  r = th * scale_factors[level]
 *   window: exactly xfh_search_window_device's, no skip mask and no uright filter;  n_window = its size;  0 -> NO_CANDIDATES (:1726)
 *   per member k in visiting order:  level > 1 -> skipped (every XFeat keypoint has octave 0, :1740);  ++n_tested;
 *       dist = DescriptorDistance(mp_desc1[i1], desc2[k]);  dist < best -> best = dist, best_idx = k     (best starts at INT_MAX)
 *   best_idx >= 0 && best <= th_high -> FOUND, match1[i1] = best_idx;  else REJECTED, match1[i1] = -1   (TH_HIGH, :1754)
 *
 * Agreement (:1840-1856): match12[i1] = idx2 iff match1[i1] == idx2 >= 0 && match2[idx2] == i1, else -1; n_found[b] counts them.  There
 * is no viewing-angle test and no rotation histogram in SearchBySim3.
 *
 * Outputs, all exact, all in device memory.  Per side and keypoint: status (XFH_SIM3_*, numbered like XFH_FUSE_* without BAD_ANGLE),
 * match, best_dist (INT_MAX where no candidate was tested; the best of a REJECTED query otherwise), n_window, n_tested (both 0 for a
 * culled query), level (-1 for a query culled before PredictScale) and optionally proj[i] = (u, v, r): zeros for INACTIVE and BEHIND,
 * r = 0 for every culled query.  Per problem: match12[n1] and n_found.
 *
 *   xfh_sim3_project      host, stateless, thread-safe: the per-point arithmetic above for n points, ONE pose Tqw and ONE M down to
 *                         status (BEHIND .. OUT_OF_RANGE or XFH_SIM3_VISIBLE), level and radius: uvr[i] = (u, v, r).  The same source
 *                         lines as the kernel (sim3_math.h).
 *   xfh_sim3_search_device   B pairs with the same n1, n2, camera, bounds, th, th_high and scale tables.  Of a side it reads n, grid
 *                         (problem b's blob at grid + b * xfh_grid_bytes(n)), desc (problem b's rows desc_stride_bytes * b in), points /
 *                         dist [B][n][3], mp_desc [B][n][64], flags [B][n] bytes, Tw [B][12], and writes status [B][n] bytes, match /
 *                         best_dist / n_window / n_tested / level [B][n] ints and proj_out [B][n][3] (or NULL); kps is not read.
 *                         d_M21 / d_M12 [B][12], d_match12 [B][n1], d_n_found [B].  side1_shared = 1: every problem reads the INPUTS of
 *                         side 1 (grid, desc, points, dist, mp_desc, flags, Tw) of problem 0 and side1->desc_stride_bytes is ignored --
 *                         LoopClosing's shape, the current keyframe against several candidates; the outputs stay [B][n1].  All pointers
 *                         inside the sides and d_M21, d_M12, d_match12, d_n_found are device pointers; the side structs themselves, cam,
 *                         bounds and the scale tables are host memory, read before the call returns.  Asynchronous on the ctx stream, no
 *                         allocation, no workspace, TWO kernel launches (behind a 4 * B byte memset of d_n_found on the same stream).
 *                         n1, n2 in 1 .. XFH_GRID_MAX_N, B in 1 .. 65535.  XFH_ERR_INVALID_ARG before anything is queued: those ranges,
 *                         nlevels outside 1 .. XFH_FUSE_MAX_LEVELS, a non-finite th, side1_shared outside 0 .. 1, a NULL required pointer,
 *                         misaligned pointers (16 bytes for desc, mp_desc, the desc strides and grids, the element size otherwise).
 *                         Points, distances, poses, M21 / M12, scale tables and descriptors may hold anything, NaN and Inf included: no
 *                         load leaves the buffers the caller named.
 *   xfh_sim3_search       host-pointer convenience form for ONE pair: every pointer of the sides is host memory, kps holds the side's n
 *                         keypoints (x, y = the undistorted coordinates) instead of a grid, and desc_stride_bytes is ignored.  It stages the
 *                         inputs, builds both grids with flags 0 and `bounds`, runs the call and copies the results back.
 *                         XFH_ERR_INVALID_ARG for the device form's classes of error (and bounds no grid can be built from) before
 *                         anything is staged or queued.
 * Out of scope: fisheye stereo; the Sim3 solver that produces S12 and consumes the matches. */
#define XFH_SIM3_FLAG_ACTIVE 1        /* flags bit0 */
enum { XFH_SIM3_INACTIVE = 0, XFH_SIM3_BEHIND = 1, XFH_SIM3_OUT_OF_IMAGE = 2, XFH_SIM3_OUT_OF_RANGE = 3,
       XFH_SIM3_NO_CANDIDATES = 5, XFH_SIM3_REJECTED = 6, XFH_SIM3_FOUND = 7,
       XFH_SIM3_VISIBLE = 5 /* xfh_sim3_project: the point reaches the search */ };
typedef struct xfh_sim3_side {
    int n;                            /* keypoints of the keyframe */
    const void* grid;                 /* device form: the grid blobs */
    const xfh_keypoint* kps;          /* host form: the n keypoints the grid is built from */
    const float* desc;                /* keyframe descriptor rows */
    size_t desc_stride_bytes;         /* device form: from one problem's rows to the next one's */
    const float* points;              /* world position of the map point of keypoint i */
    const float* dist;                /* (min_distance, max_distance, predict_distance) */
    const float* mp_desc;             /* the map point's own descriptor */
    const uint8_t* flags;
    const float* Tw;
    uint8_t* status; int* match; int* best_dist; int* n_window; int* n_tested; int* level;
    float* proj_out_or_null;
} xfh_sim3_side;
int xfh_sim3_project(const float* Tqw, const float* M, const xfh_camera* cam, const xfh_grid_bounds* bounds, float th, const float* scale_factors,
                     const float* ratio_max, int nlevels, const float* xyz, const float* distances, int n, float* uvr, int* level, uint8_t* status);
int xfh_sim3_search_device(xfh_ctx* ctx, int B, int side1_shared, const xfh_sim3_side* side1, const xfh_sim3_side* side2, const float* d_M21,
                           const float* d_M12, const xfh_camera* cam, const xfh_grid_bounds* bounds, float th, const float* scale_factors,
                           const float* ratio_max, int nlevels, int th_high, int* d_match12, int* d_n_found);
int xfh_sim3_search(xfh_ctx* ctx, const xfh_sim3_side* side1, const xfh_sim3_side* side2, const float* M21, const float* M12, const xfh_camera* cam,
                    const xfh_grid_bounds* bounds, float th, const float* scale_factors, const float* ratio_max, int nlevels, int th_high,
                    int* match12, int* n_found);

/* ---- SearchForInitialization with the reference's retraction order, device resident ----------------------------------------------------
 * ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (src/ORBmatcher.cc:833-948), the first matcher of a
 * monocular session: Tracking::MonocularInitialization calls it on every frame until the map initialises (Tracking.cc:2518-2519:
 * ORBmatcher(0.9, true), windowSize = 100) and carries mvbPrevMatched from call to call.  Unlike every other matcher here a keypoint of
 * F2 is never "taken": a later query may take it away from an earlier one if it is strictly closer (vMatchedDistance, :872), and the
 * earlier query's match is then RETRACTED (:891-895) without a second try.  The loop is sequential in the query order; the library
 * resolves it on the device and gives the sequential answer.
 *
 * Problem b is one pair (initial frame F1, current frame F2): nq query keypoints of F1 with their descriptor rows and prev_matched[nq][2]
 * (the window centres, vbPrevMatched); F2's grid blob, its nt descriptor rows and optionally its undistorted coordinates target_xy[nt][2]
 * (mvKeysUn[k].pt).  The loop; all integer comparisons are exact, the one float expression is fp32 in the order written (the library is
 * built with -ffp-contract=off):
 *
 *   matched_distance[k] = INT_MAX; matches21[k] = -1 for k in [0, nt); matches12[q] = -1; n_matches = 0
 *   for q = 0 .. nq-1, in this order:
 *     query_flags given and bit0 clear                    -> INACTIVE   (the caller's `level1 > 0`, :850, or slots it wants left out; NULL =
 *                                                                        all active, which is the reference: padding slots included)
 *     (u, v) = prev_matched[q];  r = window (one float per call, (float)windowSize)
 *     n_window = members of the window, exactly xfh_search_window_device's window; a non-finite u or v has none
 *     n_window == 0                                       -> NO_CANDIDATES  (:855)
 *     best = second = INT_MAX; best_idx = -1; n_tested = 0
 *     per member k in visiting order:  d = DescriptorDistance(q, k)
 *         matched_distance[k] <= d -> skipped             (:872, '<=': an equal distance is blocked)
 *         ++n_tested;  d < best ? (second = best, best = d, best_idx = k) : (d < second ? second = d : nothing)     (xfh_best2_csr's rule:
 *                                                          strict '<', the first visited wins a tie)
 *     accept = best_idx >= 0 && best <= th_low && (float)best < (float)second * nn_ratio      (:887-889; second == INT_MAX when there is none)
 *     !accept -> REJECTED
 *     accept  -> MATCHED: if matches21[best_idx] >= 0 { matches12[matches21[best_idx]] = -1; --n_matches }           (:891-895, the retraction)
 *                claim_idx[q] = matches12[q] = best_idx;  matches21[best_idx] = q;  matched_distance[best_idx] = best;  ++n_matches
 *   after the loop:  prev_out[q] = matches12[q] >= 0 ? target_xy[matches12[q]] : prev_matched[q]                      (:943-945)
 *
 * DescriptorDistance here is xfh_descriptor_distance where the fp32 squared norm is below 2^31 / 512, and INT_MAX otherwise (Inf, NaN):
 * such a member is always skipped (INT_MAX <= INT_MAX), so rows may hold anything.  The level window (level1, level1) = (0, 0) of :853
 * admits every XFeat keypoint, and the rotation histogram (:901-940) removes nothing: every XFeat keypoint has octave 0 and angle -1 (the
 * argument of the projection contract above), so rot = 0 for every match, all land in bin 0, and mbCheckOrientation stays without effect.
 * A retracted query keeps status MATCHED and its claim_idx: both say what the query did when its turn came; matches12 is the final
 * vnMatches12.
 *
 * Outputs, all exact, all in device memory.  Per query: status (XFH_INIT_*), claim_idx (what q wrote when its turn came, -1 otherwise),
 * matches12 (the final vnMatches12, i.e. after retractions), best_dist, second_dist (INT_MAX where there is none), n_window (0 for an
 * inactive query) and n_tested (counted when q's turn came).  Per keypoint: matches21 and matched_distance (INT_MAX where unmatched).
 * Per problem: n_matches.  prev_out and target_xy are given together or both NULL; prev_out may be the same pointer as prev_matched (the
 * reference's in-place update): the window centres are copied into the workspace before anything is written.
 *
 * How it is made parallel.  A retracted query never searches again and matched_distance[k] only ever decreases, so when q's turn comes a
 * member (k, d) is skipped iff d == INT_MAX or some accepting query j < q with claim_idx[j] == k has best_dist[j] <= d.  That is a
 * triangular system like the claim rule: re-evaluating all queries against the previous round's (claim_idx, best_dist) reaches the
 * sequential answer as its only fixed point, every query up to the smallest one that moved is final, so there are at most nq rounds.
 * After the fixed point matches21[k] is the largest accepting q on k, matches12[q] = claim_idx[q] iff q is that one, and n_matches is the
 * number of keypoints with an acceptor.  Three kernels: per query the nearest xfh_init_list_entries() members of its window; the resolver
 * (one workgroup per problem, the acceptors of every keypoint chained in LDS, no global atomics, no waiting between workgroups, the round
 * count decided on the device); and every query's turn against the final chains.  A query whose list runs out before its state is known
 * is searched again in full inside the resolver, under the budget of xfh_search_projection_device.  The worst cases -- thousands of
 * acceptors on one keypoint, thousands of queries on one spot -- cost what that call says of its worst case: exact and terminating, but
 * seconds.
 *
 *   xfh_init_accept       host, stateless, thread-safe: the `accept` line for best_idx >= 0 (best == INT_MAX stands for "none": 0), 1 or 0.
 *                         The same source line as the kernels (init_math.h).
 *   xfh_init_list_entries   the length K of the per-query lists this build was made with (tests and tools ask; nothing depends on it).
 *   xfh_init_search_workspace_bytes   bytes of d_workspace for B problems (0 for sizes the call would refuse).
 *   xfh_init_search_device   B problems with the same nq, nt, window and thresholds.  d_query_desc [B][nq][64], d_prev_matched [B][nq][2],
 *                         d_query_flags [B][nq] bytes or NULL; grid b at d_grids + b * xfh_grid_bytes(nt), target rows of problem b at
 *                         d_targets + b * target_stride_bytes (0: one frame for all), d_target_xy [B][nt][2] or NULL: the layout of
 *                         xfh_search_projection_device.  Outputs d_status [B][nq] bytes, d_claim_idx / d_matches12 / d_best_dist /
 *                         d_second_dist / d_n_window / d_n_tested [B][nq] ints, d_matches21 / d_matched_distance [B][nt] ints, d_n_matches
 *                         [B] ints, d_prev_out [B][nq][2] or NULL.  The first four ints of problem b's part of the workspace (which
 *                         starts b * xfh_init_search_workspace_bytes(nq, nt, 1) bytes in) hold afterwards: rounds of the resolver,
 *                         queries it searched again in full, lists that ran out (summed over the rounds), K.  All pointers are device
 *                         pointers; asynchronous on the ctx stream, no allocation, no host synchronisation, THREE kernel launches.  nq, nt
 *                         in 1 .. XFH_GRID_MAX_N, B in 1 .. 65535.  XFH_ERR_INVALID_ARG before anything is queued: those ranges, a
 *                         non-finite window, nn_ratio negative or not finite, th_low < 0, target_xy without prev_out or the reverse, a
 *                         NULL required pointer, misaligned pointers (16 bytes for descriptors, targets, the target stride, grids and the
 *                         workspace, 4 otherwise).  Descriptors and coordinates may hold anything, NaN and Inf included: no load leaves
 *                         the buffers the caller named, and no index outside [0, nt) is ever reported.
 *   xfh_init_search       host-pointer convenience form for ONE problem: stages the inputs and the workspace, builds the grid of the nt
 *                         keypoints (x, y = the undistorted coordinates, which are also target_xy) with flags 0 and `bounds`, runs the
 *                         call and copies the results back; prev_out may be NULL or prev_matched itself.  XFH_ERR_INVALID_ARG for the
 *                         device form's classes of error (and bounds no grid can be built from) before anything is staged or queued. */
#define XFH_INIT_FLAG_ACTIVE 1        /* d_query_flags bit0 */
enum { XFH_INIT_INACTIVE = 0, XFH_INIT_NO_CANDIDATES = 1, XFH_INIT_REJECTED = 2, XFH_INIT_MATCHED = 3 };
int xfh_init_accept(int best, int second, int th_low, float nn_ratio);
int xfh_init_list_entries(void);
size_t xfh_init_search_workspace_bytes(int nq, int nt, int B);
int xfh_init_search_device(xfh_ctx* ctx, int B, int nq, const float* d_query_desc, const float* d_prev_matched, const uint8_t* d_query_flags_or_null,
                           float window, const void* d_grids, const float* d_targets, size_t target_stride_bytes, const float* d_target_xy_or_null, int nt,
                           int th_low, float nn_ratio, void* d_workspace, uint8_t* d_status, int* d_claim_idx, int* d_matches12, int* d_best_dist,
                           int* d_second_dist, int* d_n_window, int* d_n_tested, int* d_matches21, int* d_matched_distance, int* d_n_matches,
                           float* d_prev_out_or_null);
int xfh_init_search(xfh_ctx* ctx, int nq, const float* query_desc, const float* prev_matched, const uint8_t* query_flags_or_null, float window,
                    const xfh_keypoint* kps, const xfh_grid_bounds* bounds, const float* targets, int nt, int th_low, float nn_ratio, uint8_t* status,
                    int* claim_idx, int* matches12, int* best_dist, int* second_dist, int* n_window, int* n_tested, int* matches21,
                    int* matched_distance, int* n_matches, float* prev_out_or_null);

/* ---- PoseOptimization: the motion-only pose refinement behind every tracking search, device resident ------------------------------------
 * Optimizer::PoseOptimization(Frame*) (src/Optimizer.cc:814-1114), the conventional-camera branch (!pFrame->mpCamera2) with a Pinhole camera.  This
 * is not a graph optimiser: it is the one fixed problem that function sets up -- one SE3 vertex, unary reprojection edges, Levenberg on a dense
 * 6x6 system -- for B frames per call.  It reads what the searches leave in device memory (assigned[k], the world points, the xy_un / uright of
 * xfh_frame_finish_records_device) and writes what the next search reads (Tcw for XFH_PROJ_POINTS, the outlier flags for the query flags).
 *
 * Edges.  Keypoint k of problem b has an edge iff assigned[k] is in [0, nq); its map point is points[assigned[k]] (float -> double), its
 *   measurement xy_un[k] (and uright[k]).  The edge is mono (EdgeSE3ProjectXYZOnlyPose, 2 rows, threshold 5.991f, Huber delta (float)sqrt(5.991))
 *   when d_uright is NULL or uright[k] < 0, otherwise stereo (EdgeStereoSE3ProjectXYZOnlyPose, 3 rows, 7.815f, (float)sqrt(7.815)); a NaN uright
 *   is stereo, as `mvuRight[i] < 0` decides.  Information = inv_sigma2 * I: every XFeat keypoint has octave 0, so mvInvLevelSigma2[octave] is one
 *   float per call.  n_initial = number of edges.  n_initial < 3: the call returns 0 for that problem, Tcw_out = the 12 input floats, every flag 0 (:996).
 * Pose.  State = SE3Quat: unit quaternion (x, y, z, w) + translation, doubles.  Tcw is the library's row-major 3x4 float [R|t]; R is converted by
 *   Eigen's matrix-to-quaternion rule written out in poseopt_math.h (trace > 0: the trace branch, else the largest diagonal entry, a later index
 *   winning only when strictly larger), then normalizeRotation (w < 0 flips, divide by the norm).  An update u = (omega, upsilon) is applied as
 *   SE3Quat::exp(u) * estimate: Rodrigues with the theta < 1e-5 branch R = V = I + Omega + Omega^2, the matrix-to-quaternion rule again, the
 *   quaternion product, normalizeRotation.  Tcw_out = (float) of [toRotationMatrix | t] of the final estimate.  Bit equality with the
 *   reference's own Sophus / Eigen quaternion path is NOT claimed (summation orders inside Eigen, libm's sin / cos); the decisions below are.
 * Edge arithmetic.  pc = q * X + t.  Mono: e = obs - (fx*x/z + cx, fy*y/z + cy) (Pinhole::project, double); J = -projectJac(pc) * SE3deriv.
 *   Stereo: invz = (float)(1.0 / z) as the reference's cam_project has it, e = obs - (x*invz*fx + cx, y*invz*fy + cy, u - bf*invz); J as
 *   types_six_dof_expmap.cpp:375-404 (there invz is a double).  chi2 = sum_r e_r * (inv_sigma2 * e_r).  Huber (robust_kernel_impl.cpp:78):
 *   chi2 <= delta^2 -> rho = (chi2, 1), else (2 sqrt(chi2) delta - delta^2, delta / sqrt(chi2)).  An edge adds A^T (rho[1] w) A to H and subtracts
 *   rho[1] A^T (w e) from b (base_unary_edge.hpp:43-72; robustInformation = rho[1] * information, the second-order term is commented out there).
 * Rounds.  Four rounds of optimize(10).  EVERY round starts from the INPUT pose (:1008-1009 reads pFrame->GetPose(), which is not written before
 *   :1111) and uses the level-0 edges only: those not flagged by the previous round.  A round without a level-0 edge runs no iteration.  After a
 *   round every edge is classified: an edge flagged by the previous round computes its error afresh at the round's final estimate; an unflagged edge
 *   reads _error as the last computeActiveErrors() left it -- when the last Levenberg trial of the round was rejected and popped, that is the
 *   error at the REJECTED estimate, not at the restored one.  flag = (float)chi2 > 5.991f (7.815f stereo); flagged edges go to level 1, the others
 *   back to level 0.  The Huber kernel is removed after the third round.  n_initial < 10: one round only (:1102 counts all edges).
 * Levenberg (optimization_algorithm_levenberg.cpp:61-194).  Per iteration: errors, currentChi = iniChi = the robust chi2 sum, H and b.  Iteration 0
 *   of a round: lambda = 1e-5 * max_j |H_jj| (std::max(fabs(H_jj), m): a NaN diagonal replaces m and is replaced by the next one), ni = 2.  Up to 10
 *   trials: solve (H + lambda I) x = b, estimate <- exp(x) * estimate, tempChi = the robust chi2 sum there, DBL_MAX when the factorisation
 *   failed; rho = (currentChi - tempChi) / (sum_j x_j (lambda x_j + b_j) + 1e-3); rho > 0 and tempChi finite: lambda *= max(1/3, min(1 - (2 rho
 *   - 1)^3, 2/3)), ni = 2, currentChi = tempChi; otherwise lambda *= ni, ni *= 2 and the estimate is restored.  Another trial while rho < 0.  The
 *   round ends when 10 trials ran or rho == 0, or at the third iteration in a row with (iniChi - currentChi) * 1e3 < iniChi, or after 10
 *   iterations.  NaN: every comparison above is false for a NaN, so a NaN rho ends the trials with the estimate restored and the iteration counts
 *   as progress; at most 4 x 10 x 10 trials run whatever the data.  The factorisation is an unpivoted LDL^T that fails at the first pivot that is
 *   not > 0 (Eigen's pivoting LDLT with isPositive() in the reference; no bit claim); after a failure x keeps the previous solve's values (zero
 *   before the first), which the reference leaves uninitialised.
 * Sums.  H, b and the chi2 sums are folded in a fixed order that is part of the contract of the _device call only in that it is FIXED: lane l of
 *   256 adds its keypoints l, l + 256, ... in that order, 64 lanes fold by the xor butterfly 32, 16, .. 1, the four partial sums are added in
 *   order.  Two runs on the same input give identical bytes, and a problem's result does not depend on B or on its neighbours.
 *
 *   xfh_pose_from_tcw / _to_tcw / _oplus / _solve / xfh_pose_edge
 *                         host, stateless, thread-safe, no ctx: the kernel's own source lines.  pose7 = (qx, qy, qz, qw, tx, ty, tz).
 *                         xfh_pose_solve: H21 = the upper triangle row by row; returns 1, or 0 (x untouched) when a pivot is not > 0.
 *                         xfh_pose_edge: one edge at one pose -> error[3], chi2, jacobian[18] (3x6 row-major; a mono edge (uright < 0) has a
 *                         zero third row and error[2] = 0) and rho[1] of its Huber kernel (1 when robust == 0); any output may be NULL.
 *   xfh_pose_optimize_workspace_bytes
 *                         bytes of d_workspace for B problems of nt keypoints (0 for arguments the call would refuse).  For nt <= 4096 the kernel
 *                         keeps every edge in registers and does not touch it; for larger nt an edge's state word and stored chi2 live there.
 *   xfh_pose_optimize_device
 *                         B problems, ONE launch, one workgroup each, asynchronous on the ctx stream: no host synchronisation, no allocation.
 *                         d_Tcw [B][12], d_xy_un [B][nt][2], d_uright_or_null [B][nt], d_assigned [B][nt], d_points [B][nq][3] in;
 *                         d_Tcw_out [B][12] (may be d_Tcw), d_outlier [B][nt] bytes (mvbOutlier; 0 where there is no edge), d_chi2 [B][nt]
 *                         floats (the chi2 each edge's LAST classification read; 0 where there is no edge), d_header [B][8] ints: n_initial,
 *                         n_bad, the reference's return value n_initial - n_bad of the last round that ran (0 when refused at < 3), rounds
 *                         run, Levenberg iterations, trials, rejected trials, factorisation failures; d_final_chi2 [B] doubles: currentChi
 *                         of the last iteration that ran (0 if none).  cam (host memory): fx, fy, cx, cy, bf are read.
 *                         XFH_ERR_INVALID_ARG before any launch: B < 1 (or > 65535), nt or nq outside 1 .. XFH_GRID_MAX_N, a NULL required
 *                         pointer, a misaligned pointer (16 bytes for the workspace, 8 for d_final_chi2, 4 for floats and ints), an
 *                         inv_sigma2 that is not finite or not > 0.  Points, poses, observations and camera values may be anything, NaN and
 *                         Inf included: the call terminates, and no load or store leaves the buffers the caller named.
 *   xfh_pose_optimize     host-pointer convenience form for ONE problem: stages the arrays, runs the call, copies the results back. */
int xfh_pose_from_tcw(const float* Tcw, double* pose7);
int xfh_pose_to_tcw(const double* pose7, float* Tcw);
int xfh_pose_oplus(const double* pose7, const double* update6, double* pose7_out);
int xfh_pose_solve(const double* H21, double lambda, const double* b6, double* x6);
int xfh_pose_edge(const double* pose7, const xfh_camera* cam, const float* point3, const float* xy, float uright, float inv_sigma2, int robust,
                  double* error3, double* chi2, double* jacobian18, double* rho1);
size_t xfh_pose_optimize_workspace_bytes(int nt, int B);
int xfh_pose_optimize_device(xfh_ctx* ctx, int B, int nt, int nq, const float* d_Tcw, const xfh_camera* cam, const float* d_xy_un,
                             const float* d_uright_or_null, const int* d_assigned, const float* d_points, float inv_sigma2, void* d_workspace,
                             float* d_Tcw_out, uint8_t* d_outlier, float* d_chi2, int* d_header, double* d_final_chi2);
int xfh_pose_optimize(xfh_ctx* ctx, int nt, int nq, const float* Tcw, const xfh_camera* cam, const float* xy_un, const float* uright_or_null,
                      const int* assigned, const float* points, float inv_sigma2, float* Tcw_out, uint8_t* outlier, float* chi2, int* header,
                      double* final_chi2);

/* ---- CreateNewMapPoints: triangulation of the matched pairs of a new keyframe, device resident ---------------------------------------------
 * The loop body of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:481-710) behind SearchForTriangulation, for B neighbours of one keyframe
 * per call, conventional Pinhole keyframes (mpCamera2 == NULL, NLeft == -1): the ray-parallax test, the choice between two-view triangulation and
 * KeyFrame::UnprojectStereo, GeometricTools::Triangulate, the cheirality test, the two reprojection gates, the scale-consistency test and
 * MapPoint::UpdateNormalAndDepth of the fresh point.  It reads the match12[B][n1] that xfh_triangulation_search_device left in device memory and
 * writes the points, normals and distance triples that xfh_fuse_search_device takes as d_points / d_normals / d_distances.
 *
 * The claim.  The reference searches one neighbour at a time, and a keypoint of KF1 that received a map point at neighbour b' is skipped as a query
 * at every b > b' (ORBmatcher.cc:1156-1159).  The batched search sees one has1 snapshot, so the same idx1 may come back matched at several
 * neighbours.  The search is pure per query and has2 of neighbour b does not depend on the neighbours before it, so the reference's answer is: the
 * LOWEST b whose pair (b, i) passes every gate below owns keypoint i, and the pairs of i at every later b never happened.  With XFH_TRIANG_CLAIM
 * (side1_shared = 1 required) the call decides exactly that: winner[i], the later matched pairs of i marked SUPERSEDED, and the new points as a
 * compact list in the reference's creation order, b ascending, then idx1 ascending.
 *
 * Problem b is the pair (KF1, KF2_b).  Per side and problem: xy [n][2] (mvKeysUn: xy_un of xfh_frame_finish_records_device), xy_raw [n][2]
 * (mvKeys[i].pt, which KeyFrame::UnprojectStereo reads, KeyFrame.cc:760-761; NULL = use xy), uright [n] (mvuRight; NULL = a monocular keyframe),
 * depth [n] (mvDepth; required when uright is given, not read otherwise), Tcw [12] row-major [R|t], Ow [3] (GetCameraCenter()).  With
 * side1_shared = 1 every problem reads side 1 at offset 0; with 0 problem b reads its own block.  cam (host memory, one for both sides): fx, fy,
 * cx, cy, bf are read; invfx = 1.0f / fx, invfy = 1.0f / fy, mb = bf / fx in float, as Frame computes them.  Scalars: sigma2 = mvLevelSigma2[0]
 * (every XFeat keypoint has octave 0, so ratioOctave == 1.0f), ratio_factor = 1.5f * mfScaleFactor, scale_last = mvScaleFactors[nLevels - 1],
 * far_th = mThFarPoints (<= 0: mbFarPoints is off).  flags: XFH_TRIANG_INERTIAL (the literal 0.9996 instead of 0.9998), XFH_TRIANG_CLAIM.
 *
 * The rule for keypoint i of KF1 at problem b.  All arithmetic is fp32 in the order written unless marked (the library is built with
 * -ffp-contract=off); dot(a, b) = (a0*b0 + a1*b1) + a2*b2 everywhere.
 *   m = match12[b][i];  m outside 0 .. n2 - 1                                   -> NO_MATCH
 *   stereo1 = uright1[i] >= 0, stereo2 = uright2[m] >= 0 (NULL or NaN: false)                                              (:492, :501)
 *   1. Rays.  xn = ((x - cx) / fx, (y - cy) / fy, 1) from xy (Pinhole.cpp:61-64); ray = Rwc * xn with Rwc = Rcw^T:
 *        ray[k] = (R[0][k]*xn[0] + R[1][k]*xn[1]) + R[2][k]*1;  norm = sqrtf(dot(ray, ray));  cosRays = dot(ray1, ray2) / (norm1 * norm2)      (:558-563)
 *      Eigen's unrolled 3-term reductions may associate differently: bit equality with the reference's own cosParallaxRays is not claimed (as
 *      for x3Dc in SearchByProjection); the decisions are.
 *   2. Stereo cosines (:565-576, including the `else if`).  cos1 = cos2 = cosRays + 1;  stereo1: cos1 = C(depth1[i]);  else stereo2: cos2 =
 *      C(depth2[m]) -- when both are stereo only cos1 is computed.  cosStereo = cos2 < cos1 ? cos2 : cos1.  The reference computes
 *      cosf(2 * atan2f(mb / 2, depth)), and device libm and glibc differ in the last bits; the rule is the identity
 *        C(z) = (float)(((double)z*z - h*h) / ((double)z*z + h*h)),  h = (double)(mb / 2.0f)                  -- in double, rounded once
 *      A stated deviation: at most about 2e-7 from the reference's float (two sub-ulp libm calls and one doubling); tests bound it by 1e-6.
 *   3. Branch (:582-604).  cosRays < cosStereo && cosRays > 0 && (stereo1 || stereo2 || (double)cosRays < 0.9998 (0.9996 with
 *      XFH_TRIANG_INERTIAL))  -> two-view triangulation, kind 0;  else stereo1 && cos1 < cos2 -> UnprojectStereo from KF1, kind 1;  else stereo2 &&
 *      cos2 < cos1 -> from KF2, kind 2;  else                                   -> LOW_PARALLAX
 *      UnprojectStereo (KeyFrame.cc:755-772): z = depth; !(z > 0)               -> STEREO_NO_DEPTH
 *        x = (u - cx) * z * invfx, y = (v - cy) * z * invfy from the RAW key;  x3D[k] = ((R[0][k]*x + R[1][k]*y) + R[2][k]*z) + Ow[k]
 *   4. GeometricTools::Triangulate (GeometricTools.cc:47-66).  The rows of the 4x4 A in fp32 exactly as written: A[0] = xn1[0] * T1[2] - T1[0],
 *      A[1] = xn1[1] * T1[2] - T1[1], A[2] = xn2[0] * T2[2] - T2[0], A[3] = xn2[1] * T2[2] - T2[1] (T[r] = row r of Tcw, 4 floats).  Then the right
 *      singular vector of the smallest singular value of A IN FP64: one-sided (Hestenes) Jacobi on the columns of U = (double)A with V = I
 *      accumulated, cyclic pair order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); for a pair (p, q): alpha = |U_p|^2, beta = |U_q|^2, gamma = U_p . U_q
 *      (four terms, left to right); rotate iff fabs(gamma) > 1e-15 * sqrt(alpha * beta) with zeta = (beta - alpha) / (2 gamma), t = sign(zeta) /
 *      (fabs(zeta) + sqrt(1 + zeta^2)) (sign(0) = +1), c = 1 / sqrt(1 + t^2), s = c t, (U_p, U_q) <- (c U_p - s U_q, s U_p + c U_q), V likewise.
 *      Stop after the first sweep that rotates nothing, at most 30 sweeps.  x3Dh = the column of V whose column of U has the least squared
 *      norm (the first on a tie), rounded to float.  x3Dh[3] == 0                -> DEGENERATE;  x3D = x3Dh[0..2] / x3Dh[3] in float.
 *      The reference's Eigen::JacobiSVD<Matrix4f> cannot be reproduced bit for bit; the same iteration in fp32 is 10-50x farther from the exact
 *      null vector than an fp32 LAPACK SVD, worst at low parallax, while in fp64 and rounded once it equals the fp64 SVD to within one float
 *      step.  The rule therefore returns the answer Eigen approximates, not an imitation of its rounding.  A stated deviation.
 *   5. Gates (:612-691), comparisons literally as written; a NaN behaves as in the reference (it passes `z <= 0` and every `>` gate).
 *      z1 = dot(R1[2], x3D) + t1[2];  z1 <= 0 -> BEHIND1;   z2 likewise         -> BEHIND2
 *      per view, x = dot(R[0], x3D) + t[0], y = dot(R[1], x3D) + t[1];  mono: u = fx*x/z + cx, v = fy*y/z + cy (Pinhole.cpp:30-33), ex = u - kp.x,
 *      ey = v - kp.y, (double)(ex*ex + ey*ey) > 5.991 * (double)sigma2 -> REPROJ1 / REPROJ2;  stereo: invz = (float)(1.0 / (double)z), u =
 *      fx*x*invz + cx, u_r = u - bf*invz, v = fy*y*invz + cy, er = u_r - uright, (double)(ex*ex + ey*ey + er*er) > 7.8 * (double)sigma2 likewise
 *      dist1 = sqrtf(dot(x3D - Ow1, x3D - Ow1)), dist2 likewise;  dist1 == 0 || dist2 == 0 -> ZERO_DIST
 *      far_th > 0 && (dist1 >= far_th || dist2 >= far_th)                       -> FAR
 *      ratioDist = dist2 / dist1;  ratioDist * ratio_factor < 1.0f || ratioDist > 1.0f * ratio_factor -> SCALE;  everything else -> ACCEPTED
 *   6. UpdateNormalAndDepth of the fresh point with its two observations (MapPoint.cc:426-494): n1 = x3D - Ow1, n2 = x3D - Ow2,
 *      normal[k] = ((0 + n1[k] / |n1|) + n2[k] / |n2|) / 2 (a two-term sum from zero does not depend on the std::map's pointer order),
 *      mfMax = |n1| * 1.0f, mfMin = mfMax / scale_last, dist[3] = (0.8f * mfMin, 1.2f * mfMax, mfMax).
 * Outputs, all in device memory; the integers are exact.  Per (b, i): status (XFH_TRIANG_*), kind (0 two-view, 1 stereo of KF1, 2 stereo of KF2:
 * bPointStereo = kind != 0; 0 for NO_MATCH and LOW_PARALLAX), xyz[3] (zeros unless a 3-D point was formed).  Per problem an eight-int header:
 * matched pairs, triangulation attempts, stereo attempts (countStereoAttempt), accepted pairs -- these four of the snapshot, before the claim --
 * new points after the claim, new stereo points (countStereo), superseded pairs, 0.  With XFH_TRIANG_CLAIM: winner[n1] (b or -1); status[b][i]
 * = SUPERSEDED for every matched pair with b > winner[i] >= 0 (its kind and xyz stay those of the snapshot evaluation); the compact list
 * new_idx1 / new_b / new_idx2 [n1], new_xyz / new_normal / new_dist [n1][3] with n_new entries and -1 / 0 behind them; n_new.  Without it the
 * claim outputs are not touched (they may be NULL) and header[4], [5] count the accepted pairs.  The caller runs :694-709 (new MapPoint,
 * AddObservation, AddMapPoint) over the list in order.  Two runs on the same input give identical bytes.
 *
 *   xfh_triangulate_pair  host, stateless, thread-safe, no ctx: the whole rule for ONE pair from the header the kernels compile (triangulate_math.h)
 *                         -> status, kind, x3D[3], and for an ACCEPTED pair normal[3], dist[3] (zeros otherwise); x3Dh_or_null[4]: the fp64 null
 *                         vector before rounding (zeros unless step 4 ran).  flags: XFH_TRIANG_INERTIAL only.
 *   xfh_triangulate_device   B problems with the same n1, n2.  d_match12 [B][n1]; d_status, d_kind [B][n1] bytes, d_xyz [B][n1][3], d_header
 *                         [B][8].  All arrays are device pointers; asynchronous on the ctx stream, no allocation, no workspace, no atomics: one
 *                         launch for the pairs, one for winner[] (with the claim), one for the headers and the list.  XFH_ERR_INVALID_ARG
 *                         before anything is queued: n1 or n2 outside 1 .. XFH_GRID_MAX_N, B outside 1 .. 65535, side1_shared other than 0 or 1,
 *                         unknown flag bits, XFH_TRIANG_CLAIM without a shared side 1, a NULL required pointer (depth beside a given uright; the
 *                         claim outputs with the claim), a pointer that is not 4-byte aligned, a non-finite scalar.  Coordinates, depths, poses
 *                         and camera values may hold anything, NaN and Inf included; a match12 entry outside 0 .. n2 - 1 is -1: no load or store
 *                         leaves the buffers the caller named, and the call terminates (at most 30 sweeps per pair).
 *   xfh_triangulate       host-pointer convenience form for one call with a shared side 1: stages the arrays, runs the call, copies the results back.
 * Out of scope: a second camera (mpCamera2, NLeft != -1, the four pose variants of :505-555) and KannalaBrandt8; per-keypoint octaves (sigma2 and
 * ratioOctave are per call); the baseline test of :443-460 and CheckNewKeyFrames() (the caller passes the neighbours it wants); creating the
 * MapPoint objects and their observations; MapPoint::ComputeDistinctiveDescriptors of a new point (with two observations both medians are 0 and
 * the reference keeps whichever keyframe pointer sorts first: either row is a legal outcome, KF1's is recommended). */
#define XFH_TRIANG_INERTIAL 1         /* flags: mbInertial (0.9996) */
#define XFH_TRIANG_CLAIM 2            /* flags: the first accepted neighbour owns a keypoint of KF1; needs side1_shared = 1 */
enum { XFH_TRIANG_NO_MATCH = 0, XFH_TRIANG_LOW_PARALLAX = 1, XFH_TRIANG_STEREO_NO_DEPTH = 2, XFH_TRIANG_DEGENERATE = 3, XFH_TRIANG_BEHIND1 = 4,
       XFH_TRIANG_BEHIND2 = 5, XFH_TRIANG_REPROJ1 = 6, XFH_TRIANG_REPROJ2 = 7, XFH_TRIANG_ZERO_DIST = 8, XFH_TRIANG_FAR = 9, XFH_TRIANG_SCALE = 10,
       XFH_TRIANG_ACCEPTED = 11, XFH_TRIANG_SUPERSEDED = 12 };
int xfh_triangulate_pair(const xfh_camera* cam, int flags, float sigma2, float ratio_factor, float scale_last, float far_th, const float* xy1,
                         const float* xy_raw1_or_null, float uright1, float depth1, const float* Tcw1, const float* Ow1, const float* xy2,
                         const float* xy_raw2_or_null, float uright2, float depth2, const float* Tcw2, const float* Ow2, int* status, int* kind,
                         float* x3D, float* normal, float* dist, double* x3Dh_or_null);
int xfh_triangulate_device(xfh_ctx* ctx, int B, int n1, int n2, int side1_shared, int flags, const xfh_camera* cam, float sigma2, float ratio_factor,
                           float scale_last, float far_th, const float* d_xy1, const float* d_xy_raw1_or_null, const float* d_uright1_or_null,
                           const float* d_depth1_or_null, const float* d_Tcw1, const float* d_Ow1, const float* d_xy2, const float* d_xy_raw2_or_null,
                           const float* d_uright2_or_null, const float* d_depth2_or_null, const float* d_Tcw2, const float* d_Ow2, const int* d_match12,
                           uint8_t* d_status, uint8_t* d_kind, float* d_xyz, int* d_header, int* d_winner, int* d_new_idx1, int* d_new_b,
                           int* d_new_idx2, float* d_new_xyz, float* d_new_normal, float* d_new_dist, int* d_n_new);
int xfh_triangulate(xfh_ctx* ctx, int B, int n1, int n2, int flags, const xfh_camera* cam, float sigma2, float ratio_factor, float scale_last, float far_th,
                    const float* xy1, const float* xy_raw1_or_null, const float* uright1_or_null, const float* depth1_or_null, const float* Tcw1,
                    const float* Ow1, const float* xy2, const float* xy_raw2_or_null, const float* uright2_or_null, const float* depth2_or_null,
                    const float* Tcw2, const float* Ow2, const int* match12, uint8_t* status, uint8_t* kind, float* xyz, int* header, int* winner,
                    int* new_idx1, int* new_b, int* new_idx2, float* new_xyz, float* new_normal, float* new_dist, int* n_new);

/* ---- TwoViewReconstruction::Reconstruct (src/TwoViewReconstruction.cc), the second half of Tracking::MonocularInitialization -----------------
 * (src/Tracking.cc:2531, mpCamera->ReconstructWithTwoViews for the Pinhole camera), for B problems per call, on the arrays that
 * xfh_init_search_device leaves in device memory: d_xy1 [B][n1][2] and d_xy2 [B][n2][2] are the undistorted keypoints (mvKeysUn) of the
 * reference and the current frame, d_matches12 [B][n1] is vnMatches12 (an entry outside 0 .. n2 - 1 is "no match").  The rule, written once in
 * xfeatslam_amd/csrc/twoview_math.h and compiled for the kernels and for the host entry points below; fp32 in the order written unless a double
 * is named:
 *   1. The compact match list (:50-66) in idx1 order; N matches.  N < 8 -> status TOO_FEW: the reference's set generation is undefined there; the
 *      header is written (N, status, -1 for the winners and the chosen hypothesis, 0 elsewhere) and NOTHING else.
 *   2. The minimal sets (:78-98) from the CALLER's raw draws: d_draws holds iters x 8 values of the caller's rand() (after its SeedRandOnce(0),
 *      in the order the reference consumes them) and rand_max its RAND_MAX; problem b reads d_draws + b * draws_problem_stride (ints; 0 = all
 *      problems share one list).  Draw j of an iteration indexes the shrinking vAvailableIndices of size d = N - j at int(((double)draw /
 *      ((double)rand_max + 1.0)) * d), followed by the swap-remove; only the at most eight overwritten positions are tracked.  This reproduces
 *      mvSets for any N without a host round trip for N, and the library holds no generator.  A draw outside 0 .. rand_max is clamped into
 *      0 .. d - 1.
 *   3. Normalize (:737-784) over ALL keypoints of a frame, as in the reference: mean = sum / n, s = (float)(1.0 / (double)(sum |x - mean| / n)),
 *      normalised point ((x - meanX) * sX, (y - meanY) * sY).  A stated deviation: every float sum of the rule (these four per frame, and the score
 *      sums of step 5) is not sequential but has ONE fixed parallel order, whatever the grid or B: 256 lanes, lane l adds the terms l, l + 256, ...
 *      in order to 0.0f; the 256 partial sums fold s[l] += s[l + h] for h = 128, 64, .. 1.
 *   4. ComputeH21 / ComputeF21 (:232-308) per iteration.  The rows of the 16 x 9 / 8 x 9 A in fp32 as the reference writes them.  Every
 *      Eigen::JacobiSVD<float> of the rule (16 x 9, 8 x 9, 3 x 3) is the one-sided Jacobi of xfh_triangulate_device's step 4 IN FP64 (same
 *      rotation -- the two share its code --, cyclic pairs p < q in lexicographic order, column dot products over the rows in order starting from
 *      row 0's product, stop after the first sweep that rotates nothing, at most 30 sweeps), rounded to float once.  A stated deviation, for the
 *      reason given there.  Null vector = V's column whose column of U has the least squared norm, the first on a tie.  For a full 3 x 3 SVD the
 *      columns are ordered by squared norm descending (stable), w_i = sqrt |a_i|^2, u_i = a_i / w_i with a_i the columns of A V.  The rank-2
 *      projection of F is a_i0 v_i0^T + a_i1 v_i1^T in double over the two largest columns.  For the rank-2 E of DecomposeE the third column of U
 *      cannot come from a_2 / w_2 (0 / 0 up to rounding): it is the cross product u_0 x u_1 in double.
 *      H21i = T2inv Hn T1 and F21i = T2^T Fn T1 with the triangular T written out: M = X T1: M[r][0] = X[r][0] sX, M[r][1] = X[r][1] sY, M[r][2] =
 *      (X[r][0] tx + X[r][1] ty) + X[r][2], tx = -meanX sX;  T2inv = [1/sX 0 meanX; 0 1/sY meanY; 0 0 1] analytically (the reference inverts T2
 *      numerically);  H12i = the cofactor inverse of H21i times 1.0f / det, det = (a(ei - fh) - b(di - fg)) + c(dh - eg).
 *   5. CheckHomography / CheckFundamental (:310-473) per (iteration, match), as written with each three-term dot product (x*a + y*b) + c,
 *      w = (float)(1.0 / (double)den), invSigmaSquare = (float)(1.0 / (double)(sigma * sigma)), th 5.991f (H), 3.841f with score threshold 5.991f
 *      (F).  A match's share = (chi1 > th ? 0 : th - chi1) + (chi2 > th ? 0 : th - chi2), summed over the matches in the order of step 3 (the
 *      reference adds the two halves to the running sum one after the other).  The argmax with the strict >: the first iteration with the
 *      highest score wins; a score that is not > 0 -- zero, or the NaN of a rank-deficient fit -- never wins.  Only the scores are stored; the
 *      inlier flags of the two winners are recomputed.
 *   6. SH + SF == 0 -> BOTH_ZERO.  RH = SH / (SH + SF); (double)RH > 0.50 -> ReconstructH, else ReconstructF.
 *   7. ReconstructF (:475-569): E = K^T (F K) with K's zeros not multiplied; DecomposeE from the SVD of step 4: t = u_2 / |u_2|, R1 = U W V^T =
 *      (u_1 v_0^T - u_0 v_1^T) + u_2 v_2^T, R2 = (u_0 v_1^T - u_1 v_0^T) + u_2 v_2^T, each negated when its float determinant is < 0; hypotheses
 *      0 .. 3 = (R1, t) (R2, t) (R1, -t) (R2, -t).  ReconstructH (:571-734): A = K^-1 (H K) with K^-1 = [1/fx 0 -cx/fx; 0 1/fy -cy/fy; 0 0 1]
 *      written out, the SVD, s = det U * det V, (double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001 -> H_DEGENERATE (an H that is a
 *      similarity to five digits: a pair without motion or a pure zoom, which F fits as well as H, so SH and SF tie and RH is 0.5 up to the
 *      rounding of the two sums: whether such a pair ends here or on the F path is decided by rounding, in the reference as here), and the eight
 *      Faugeras hypotheses in the reference's order, R = s * ((X V^T)) with X = U Rp, t = U tp normalised.  The sign and pairing ambiguities of an
 *      SVD permute the hypotheses against Eigen's: the SET is the contract, the index reported is that of this rule.
 *   8. CheckRT (:786-901) per (hypothesis, inlier of the chosen model): P1 = K [I|0], P2 = K [R|t], the 4 x 4 A and the fp64 null vector of
 *      xfh_triangulate_device's step 4, p = h[0..2] / h[3] in float; a non-finite p is skipped; O2 = -R^T t; cosParallax as written; the two
 *      depth tests with (double)cos < 0.99998; invZ = (float)(1.0 / (double)z); squared errors against th2 = (float)(4.0 * (double)(sigma *
 *      sigma)).  A pair that passes is counted (nGood, its cosine, its point) and is good (vbGood) when (double)cos < 0.99998.  The cosine at
 *      sorted index min(50, nGood - 1) is selected by value over the floats' order keys; 1.0f with nGood = 0.  Parallax, a stated deviation: the
 *      reference converts with acos(..) * 180 / CV_PI and compares degrees; the device compares the cosine with the double min_parallax_cos =
 *      cos(minParallax * pi / 180) the caller passes (F: (double)cos < min_parallax_cos; H, whose test is >=: (double)cos <= min_parallax_cos)
 *      and reports the cosine.
 *   9. The decision.  F: maxGood, nMinGood = max((int)(0.9 * (double)N_inliers), min_triangulated), nsimilar over (double)nGood > 0.7 *
 *      (double)maxGood; maxGood < nMinGood || nsimilar > 1 -> F_NO_WINNER; the first hypothesis with nGood == maxGood: enough parallax ->
 *      OK_F, else LOW_PARALLAX.  H: best / second best with the strict >; (double)second < 0.75 * (double)best && best > min_triangulated &&
 *      (double)best > 0.9 * (double)N_inliers, else H_GATES; then the parallax test, else LOW_PARALLAX; -> OK_H.
 * Outputs per problem.  d_header [B][24] ints: N, status (XFH_TWO_VIEW_*), model (0 none, 1 H, 2 F), winning iteration of H, of F (-1: none),
 * nGood[8], the chosen hypothesis (-1), inliers of the winning H, of the winning F, triangulated count, number of hypotheses, n_matches_out
 * (triangulated count on success, N otherwise), five zeros.  d_floats [B][48]: SH, SF, RH, H21[9], F21[9], T21[12] row-major [R|t] (zeros
 * unless the call succeeded), the cosine at the parallax index of the eight hypotheses (1.0f where none), zeros.  Per keypoint of frame 1,
 * indexed by idx1 (a keypoint has at most one match): d_inlier_h, d_inlier_f, d_triangulated [B][n1] bytes, d_p3d [B][n1][3] (the winning
 * hypothesis' point for every counted pair, zeros elsewhere), d_matches_out [B][n1] = matches12 with the entries that were matched but not
 * triangulated set to -1 on success (Tracking.cc:2533-2540) and unchanged otherwise.  On the H path the reference returns true without
 * assigning vP3D (:725-731); this call writes the winning hypothesis' points on both paths.
 *
 *   xfh_two_view_workspace_bytes  bytes of d_workspace for such a call; 0 for sizes the call refuses.
 *   xfh_two_view_device   everything in device memory; asynchronous on the ctx stream, no allocation, no host synchronisation, no global
 *                         atomics; SIX launches whatever the data.  XFH_ERR_INVALID_ARG before anything is queued: B outside 1 .. 65535, n1 or
 *                         n2 outside 1 .. XFH_GRID_MAX_N, iters outside 1 .. 4096, sigma not finite and > 0, rand_max < 1, min_parallax_cos not
 *                         finite, min_triangulated < 0, a stride that is neither 0 nor >= iters * 8 with B > 1, a NULL pointer, a pointer that is
 *                         not 4-byte (d_workspace: 16-byte) aligned.  Coordinates and camera values may hold anything, NaN and Inf included, and
 *                         matches and draws any int: no load or store leaves the buffers, and every loop is bounded.
 *   xfh_two_view          host-pointer form for one problem through the ctx staging arena.
 *   xfh_two_view_host     the whole rule on ONE host thread over host pointers (workspace included): no ctx, no GPU; what the sanitizer
 *                         program and the CPU tests run.  Stateless and thread-safe, as are the four below, each one piece of the rule:
 *   xfh_two_view_set      the set of one iteration from its eight draws and N >= 8
 *   xfh_two_view_fit      Hn or Fn[9] (step 4, before the composition) of eight NORMALISED point pairs [8][2]
 *   xfh_two_view_score    chi2[2], the inlier flag and the share of the score of one match under M = H21 followed by H12 (18 floats) or F21 (9)
 *   xfh_two_view_check_rt CheckRT's verdict for one pair under T21 [R|t]: 0 not counted, 1 counted, 2 counted and good; its cosine and point
 * Out of scope: KannalaBrandt8::ReconstructWithTwoViews. */
enum { XFH_TWO_VIEW_TOO_FEW = 0, XFH_TWO_VIEW_BOTH_ZERO = 1, XFH_TWO_VIEW_H_DEGENERATE = 2, XFH_TWO_VIEW_F_NO_WINNER = 3, XFH_TWO_VIEW_H_GATES = 4,
       XFH_TWO_VIEW_LOW_PARALLAX = 5, XFH_TWO_VIEW_OK_H = 6, XFH_TWO_VIEW_OK_F = 7 };
#define XFH_TWO_VIEW_MODEL_H 1
#define XFH_TWO_VIEW_MODEL_F 2
#define XFH_TWO_VIEW_HEADER_INTS 24
#define XFH_TWO_VIEW_FLOATS 48
#define XFH_TWO_VIEW_MAX_ITERS 4096
size_t xfh_two_view_workspace_bytes(int n1, int n2, int iters, int B);
int xfh_two_view_device(xfh_ctx* ctx, int B, int n1, int n2, const float* d_xy1, const float* d_xy2, const int* d_matches12, const xfh_camera* cam,
                        float sigma, int iters, const int* d_draws, size_t draws_problem_stride, int rand_max, double min_parallax_cos,
                        int min_triangulated, void* d_workspace, int* d_header, float* d_floats, uint8_t* d_inlier_h, uint8_t* d_inlier_f,
                        uint8_t* d_triangulated, float* d_p3d, int* d_matches_out);
int xfh_two_view(xfh_ctx* ctx, int n1, int n2, const float* xy1, const float* xy2, const int* matches12, const xfh_camera* cam, float sigma, int iters,
                 const int* draws, int rand_max, double min_parallax_cos, int min_triangulated, int* header, float* floats, uint8_t* inlier_h,
                 uint8_t* inlier_f, uint8_t* triangulated, float* p3d, int* matches_out);
int xfh_two_view_host(int B, int n1, int n2, const float* xy1, const float* xy2, const int* matches12, const xfh_camera* cam, float sigma, int iters,
                      const int* draws, size_t draws_problem_stride, int rand_max, double min_parallax_cos, int min_triangulated, void* workspace,
                      int* header, float* floats, uint8_t* inlier_h, uint8_t* inlier_f, uint8_t* triangulated, float* p3d, int* matches_out);
int xfh_two_view_set(const int* draws8, int rand_max, int N, int* set8);
int xfh_two_view_fit(int model, const float* xy1n, const float* xy2n, float* M);
int xfh_two_view_score(int model, const float* M, float sigma, const float* xy1, const float* xy2, float* chi2, int* inlier, float* term);
int xfh_two_view_check_rt(const xfh_camera* cam, const float* T21, float sigma, const float* xy1, const float* xy2, int* verdict, float* cos_parallax,
                          float* p3d);

/* ---- Sim3Solver (src/Sim3Solver.cc) as LoopClosing::DetectCommonRegionsFromBoW drives it (src/LoopClosing.cc:645-755) ---------------------------
 * The two steps between xfh_bow_search_device (shared = 1, the current keyframe against the J covisibles of a candidate) and the first
 * xfh_map_projection_search_device: the merge of the per-covisible match lists (:670-687) and the RANSAC over 3-point sets with Horn's closed
 * form (:698-710), with the composition gScm * gSmw (:746-749) so that nothing is read back between the calls.  B problems per call, each one
 * candidate keyframe against the current keyframe.  Map points are rows of ONE table d_points [M][3] of world positions; d_point1 [n1] is the
 * row of the current keyframe's map point at keypoint i1 (negative: no map point, a bad one, or GetIndexInKeyFrame < 0, :78-91), d_matched
 * [B][n1] the row of vpMatched12[i1] (negative: NULL, bad, or not indexed in its keyframe); an entry outside 0 .. M - 1 is "none".  d_T1w [12]
 * and d_T2w [B][12] are the row-major [R|t] of the two keyframes' poses (T1w_problem_stride in floats; 0 = all problems share one), cam1 / cam2
 * the two cameras, of which only the Pinhole project is used: fx * x / z + cx.  max_err1 / max_err2: the reference stores 9.210 * sigma2 in a
 * std::vector<size_t>, so the value is truncated (9 at level 0, and every XFeat keypoint has octave 0): pass
 * (float)(size_t)(9.210 * mvLevelSigma2[0]).  The rule, written once in xfeatslam_amd/csrc/sim3solve_math.h and compiled for the kernels and
 * for the host entry points below; fp32 in the order written unless a double is named:
 *   1. The compact list (:71-115) in i1 order over the slots where both rows are valid; N entries.  X1 = R1w p + t1w, X2 likewise, each row
 *      ((a*x + b*y) + c*z) + t; mvP1im1 = project(X1) under cam1, mvP2im2 = project(X2) under cam2.
 *   2. Too few: N < min_inliers (the reference's bNoMore at :225-229), N < 3 (the set generation is undefined there), or the merge's count
 *      *d_num_matches_or_null < min_matches (nBoWMatches at LoopClosing.cc:691) -> status TOO_FEW.  It does not depend on the draws.  The header
 *      is written (N, status, 0 iterations, -1 for the winner and the best, zeros) and NOTHING else.
 *   3. The iteration count (:123-147) needs host libm and must equal the reference's value exactly, so the caller passes a table: its =
 *      d_iters_of_N[N] (n1 + 1 entries, xfh_sim3_solve_iterations_table), clamped into 1 .. max_iters; max_iters (1 .. 4096) is the number of
 *      iterations d_draws holds.  xfh_sim3_solve_iterations is ceil(log(1 - p) / log(1 - pow((float)min_inliers / N, 3))) as the reference
 *      evaluates it, then max(1, min(nIterations, max_its)); 1 for N == min_inliers; max_its where the double is not finite or does not fit an
 *      int (the reference's cast is undefined there).
 *   4. The minimal set (:245-259) from the CALLER's raw draws, as xfh_two_view_device takes them: iteration k reads draws 3k .. 3k + 2 of
 *      d_draws + b * draws_problem_stride; draw j indexes the shrinking vector of size d = N - j at int(((double)draw / ((double)rand_max + 1.0))
 *      * d) (thirdparty/DBoW2/DUtils/Random.cpp:47-50), followed by the swap-remove; only the at most three overwritten positions are tracked.
 *      A draw outside 0 .. rand_max is clamped into 0 .. d - 1.
 *   5. ComputeSim3 (:311-412).  Centroids ((p0 + p1) + p2) / 3.0f; M = Pr2 Pr1^T, each entry the sum over the three points in order; the ten
 *      entries of the symmetric 4 x 4 N as the reference writes them, float expressions left to right assigned to doubles.  The eigenvector of
 *      the largest eigenvalue, a stated deviation of the same kind and for the same reason as the fp64 Jacobi of xfh_triangulate_device's step
 *      4: the reference runs the general Eigen::EigenSolver<Matrix4f>; the rule is a cyclic two-sided Jacobi IN FP64: pairs p < q in
 *      lexicographic order, a pair rotates iff |a_pq| > 1e-15 |N|_F, theta = (a_qq - a_pp) / (2 a_pq), t = sgn(theta) / (|theta| + sqrt(1 +
 *      theta^2)), c = 1 / sqrt(1 + t^2), s = c t, a_pp -= t a_pq, a_qq += t a_pq; stop after the first sweep that rotates nothing, at most 30
 *      sweeps; the first of equal eigenvalues wins, as maxCoeff does.  The rotation, a stated deviation: the reference goes quaternion -> atan2
 *      -> angle-axis -> Sophus::SO3f::exp; the rule builds R directly from the unit quaternion in double and rounds once.  Both are invariant
 *      to the eigenvector's sign.  This removes the reference's 0 / 0 for an exactly zero rotation (vec.norm() == 0: the reference's T is NaN
 *      with no inliers); the rule yields the identity.  Scale = nom / den in double over the nine products (double)Pr1 * (double)P3 resp. P3 *
 *      P3 in column-major order, P3 = R Pr2 in float; 1.0f with fix_scale.  sR = s R; t12 = O1 - sR O2; T12 = [sR|t12]; T21 = [(float)(1.0 /
 *      (double)s) R^T | -sRinv t12].
 *   6. CheckInliers (:415-439) per (iteration, correspondence): err1 = |mvP1im1 - project1(T12 X2)|^2, err2 = |project2(T21 X1) - mvP2im2|^2,
 *      inlier iff err1 < max_err1 && err2 < max_err2; a NaN never passes.  The count is an integer: no summation order enters.
 *   7. The decision of `while(!bConverge && !bNoMore) iterate(20, ..)` (:240-293), order-free.  Converged: the winner is the first iteration k <
 *      its with inliers_k > min_inliers (every earlier best is <= min_inliers < inliers_k, so the >= test holds there).  Otherwise NO_MORE, and
 *      the best is the last iteration whose count is >= every earlier count (the reference reads nothing from it, but GetEstimated* would
 *      return it).  tests/test_sim3solve_ref.py proves the equivalence against a literal transcription with the chunks of 20.
 *   8. The composition for the next search (LoopClosing.cc:746-749, ORBmatcher.cc:621-622), in double from the floats: R = R12 R2w, t = s (R12
 *      t2w) + t12; d_Tcw = [R | t / s], d_Ow = -R^T (t / s), each rounded to float once: exactly what xfh_map_projection_search_device takes as
 *      d_Tcw / d_Ow.  The reference passes through g2o's quaternion here; bit equality with that round trip is not claimed.
 * Outputs per problem.  d_header [B][16] ints: N, status (XFH_SIM3_SOLVE_*), the effective number of iterations, the winning iteration (-1),
 * nInliers, the best iteration, the best count, the iterations consumed (winner + 1, or all: a caller that emulates one global rand() stream
 * knows from it how many draws the reference would have used), zeros.  d_floats [B][32]: T12 [12], R12 [9], t12 [3], s12 of the winner, or of
 * the best iteration when there is none, zeros.  d_inliers [B][n1] bytes indexed by i1 (vbInliers, :277-279): all zero unless the problem
 * converged.  d_Tcw [B][12], d_Ow [B][3]: written only when the problem converged.
 *
 * The merge (LoopClosing.cc:670-687): d_match12 [J][n1] is the output of xfh_bow_search_device with covisible j as problem j, d_point2 [J][n2]
 * the row of covisible j's map point at its keypoint (negative: none or bad).  The reference's loop, j ascending and k ascending: the first
 * appearance of a map point inserts it into the set and writes slot k; a later covisible can overwrite slot k with a different new point.
 * Order-free: entry (j, k) OWNS its point when no lexicographically earlier entry has the same row; slot k takes the owner entry with the
 * largest j; numBoWMatches is the number of owners.  Outputs d_matched [n1] (the row, or -1: the form the solver reads), d_matched_kf [n1] (j or
 * -1), *d_num_matches.  An owner table of M ints in the workspace and an integer atomicMin of j * n1 + k: deterministic.
 *
 *   xfh_sim3_solve_workspace_bytes  bytes of d_workspace for the solver with B problems, which also hold the merge's owner table; 0 for sizes
 *                         the calls refuse.
 *   xfh_sim3_solve_device everything in device memory; asynchronous on the ctx stream, no allocation, no host synchronisation; FOUR launches
 *                         whatever the data.  XFH_ERR_INVALID_ARG before anything is queued: B outside 1 .. 65535, n1 outside 1 ..
 *                         XFH_GRID_MAX_N, M outside 1 .. 2^24, min_inliers < 0, max_iters outside 1 .. XFH_SIM3_SOLVE_MAX_ITERS, thresholds that
 *                         are not finite, rand_max < 1, a stride that is neither 0 nor a whole problem (3 * max_iters draws, 12 floats) with B >
 *                         1, a NULL pointer (but d_num_matches_or_null), a pointer that is not 4-byte (d_workspace: 16-byte) aligned.  Points,
 *                         poses and cameras may hold anything, NaN and Inf included, and d_point1, d_matched, d_draws and d_iters_of_N any int: no
 *                         load or store leaves the buffers, and every loop is bounded.
 *   xfh_sim3_solve        host-pointer form for one problem through the ctx staging arena.
 *   xfh_sim3_solve_host   the whole rule on ONE host thread over host pointers (workspace included): no ctx, no GPU.  Stateless and
 *                         thread-safe, as are the ones below, each one piece of the rule:
 *   xfh_sim3_solve_iterations / _iterations_table   step 3
 *   xfh_sim3_solve_set    the three indices of one iteration from its three draws and N >= 3
 *   xfh_sim3_solve_horn   step 5 of two point triples (point j at [3j .. 3j + 3)) -> hyp [40]: T12 [12], R [9], t [3], s, T21 [12], zeros
 *   xfh_sim3_solve_check  step 6 of one correspondence (X1, X2 in their camera frames) -> err [2] and the flag
 *   xfh_sim3_merge_matches_device / xfh_sim3_merge_matches / xfh_sim3_merge_matches_host   the merge: three launches; J in 1 .. 65535, n1, n2 in
 *                         1 .. XFH_GRID_MAX_N; the host form takes M ints of workspace.
 * Optimizer::OptimizeSim3 behind this call is xfh_sim3_optimize_device below.  Out of scope: the KannalaBrandt8 project; per-keypoint octaves other than 0; the 4-argument iterate / find as
 * separate entry points (the same rule gives them: find() is iterate(mRansacMaxIts), one chunk, and the chunk length does not enter the rule;
 * the 4-argument iterate differs from the 5-argument one only in what it returns without convergence). */
enum { XFH_SIM3_SOLVE_TOO_FEW = 0, XFH_SIM3_SOLVE_NO_MORE = 1, XFH_SIM3_SOLVE_CONVERGED = 2 };
#define XFH_SIM3_SOLVE_HEADER_INTS 16
#define XFH_SIM3_SOLVE_FLOATS 32
#define XFH_SIM3_SOLVE_HYP_FLOATS 40
#define XFH_SIM3_SOLVE_MAX_ITERS 4096
size_t xfh_sim3_solve_workspace_bytes(int n1, int M, int B);
int xfh_sim3_solve_device(xfh_ctx* ctx, int B, int n1, int M, const float* d_points, const int* d_point1, const int* d_matched, const float* d_T1w,
                          size_t T1w_problem_stride, const float* d_T2w, const xfh_camera* cam1, const xfh_camera* cam2, float max_err1, float max_err2,
                          int fix_scale, int min_inliers, int min_matches, const int* d_num_matches_or_null, const int* d_iters_of_N, int max_iters,
                          const int* d_draws, size_t draws_problem_stride, int rand_max, void* d_workspace, int* d_header, float* d_floats,
                          uint8_t* d_inliers, float* d_Tcw, float* d_Ow);
int xfh_sim3_solve(xfh_ctx* ctx, int n1, int M, const float* points, const int* point1, const int* matched, const float* T1w, const float* T2w,
                   const xfh_camera* cam1, const xfh_camera* cam2, float max_err1, float max_err2, int fix_scale, int min_inliers, const int* iters_of_N,
                   int max_iters, const int* draws, int rand_max, int* header, float* floats, uint8_t* inliers, float* Tcw, float* Ow);
int xfh_sim3_solve_host(int B, int n1, int M, const float* points, const int* point1, const int* matched, const float* T1w, size_t T1w_problem_stride,
                        const float* T2w, const xfh_camera* cam1, const xfh_camera* cam2, float max_err1, float max_err2, int fix_scale, int min_inliers,
                        int min_matches, const int* num_matches_or_null, const int* iters_of_N, int max_iters, const int* draws, size_t draws_problem_stride,
                        int rand_max, void* workspace, int* header, float* floats, uint8_t* inliers, float* Tcw, float* Ow);
int xfh_sim3_solve_iterations(double prob, int min_inliers, int max_its, int N);
int xfh_sim3_solve_iterations_table(double prob, int min_inliers, int max_its, int n1, int* iters_of_N /* n1 + 1 */);
int xfh_sim3_solve_set(const int* draws3, int rand_max, int N, int* set3);
int xfh_sim3_solve_horn(const float* P1, const float* P2, int fix_scale, float* hyp /* XFH_SIM3_SOLVE_HYP_FLOATS */);
int xfh_sim3_solve_check(const float* T12, const float* T21, const xfh_camera* cam1, const xfh_camera* cam2, const float* X1, const float* X2, float max_err1,
                         float max_err2, float* err, int* inlier);
int xfh_sim3_merge_matches_device(xfh_ctx* ctx, int J, int n1, int n2, int M, const int* d_match12, const int* d_point2, void* d_workspace, int* d_matched,
                                  int* d_matched_kf, int* d_num_matches);
int xfh_sim3_merge_matches(xfh_ctx* ctx, int J, int n1, int n2, int M, const int* match12, const int* point2, int* matched, int* matched_kf, int* num_matches);
int xfh_sim3_merge_matches_host(int J, int n1, int n2, int M, const int* match12, const int* point2, void* workspace, int* matched, int* matched_kf,
                                int* num_matches);

/* ---- OptimizeSim3: the similarity refinement between the two Sim3 projection searches of loop detection, device resident --------------------
 * Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale, mAcumHessian, bAllPoints) (src/Optimizer.cc:2100-2381) as
 * LoopClosing::DetectCommonRegionsFromBoW (src/LoopClosing.cc:767) and DetectAndReffineSim3FromLastKF (:556) call it, Pinhole cameras.  Not a graph
 * optimiser: the one fixed problem that function sets up -- one Sim3 vertex of 7 unknowns, two mono edges per correspondence, fixed points,
 * Levenberg on a dense 7x7 system -- for B problems per call.  It reads what xfh_sim3_solve_device (d_floats + 12 with stride
 * XFH_SIM3_SOLVE_FLOATS is d_S12) and the coarse xfh_map_projection_search_device (d_assigned) leave in device memory, and writes what the fine
 * xfh_map_projection_search_device reads (d_Tcw, d_Ow).  The rule is written once in xfeatslam_amd/csrc/optsim3_math.h and compiled for the
 * kernel, the host form and the piece functions below; IEEE double in the order written there unless a float is named.
 *
 * Side 1 is the current keyframe: d_T1w [12] row-major [R|t], d_xy_un1 [n1][2] (mvKeysUn), d_point1 [n1] = the row of the keyframe's own map point
 *   in d_points1 [M1][3] (world positions); an entry outside 0 .. M1 - 1 is NULL or isBad(), which both leave the loop without an edge (:2183-2227;
 *   only counters nobody reads tell them apart).  With side1_shared = 1 every problem reads problem 0's arrays, with 0 its own block.
 * Side 2, per problem: d_assigned [B][n1] = exactly the d_assigned of the coarse search, assigned[i] = q the row of vpMatches1[i] in d_points2
 *   [B][nq][3], anything outside 0 .. nq - 1 is NULL; d_flags2 [B][nq] bytes, bit 0 = !pMP2->isBad() (the search's XFH_MAPPROJ_FLAG_ACTIVE array
 *   can be passed as it is); d_index2 [B][nq] ints = get<0>(GetIndexInKeyFrame(pKF2)), negative = not in KF2 (STATED: an index >= n2, which the
 *   reference cannot produce, is "not in KF2" too); d_xy_un2 [B][n2][2]; d_T2w [B][12].
 * d_S12 + b * S12_problem_stride: 13 floats, R row-major 9, t 3, s.  d_Tmw_or_null [B][12]: the pose of pMostBoWMatchesKF for the composed output.
 * Host scalars: cam1, cam2 (fx, fy, cx, cy are read), th2, fix_scale, all_points, inv_sigma2_1, inv_sigma2_2 (mvInvLevelSigma2[octave]: every
 *   XFeat keypoint has octave 0, and the cv::KeyPoint(Point2f, mnTrackScaleLevel) of :2280 passes the level as the SIZE, so its octave is 0 too).
 *
 * Edges (:2167-2304).  Keypoint i has the edge pair iff assigned[i] is valid, bit 0 of its flag byte is set, point1[i] is valid, index2 >= 0 ||
 *   all_points, and !(P3D2c.z < 0) (a NaN z passes, as there).  P3D1c = R1w X1 + t1w and P3D2c = R2w X2 + t2w in FLOAT, each row ((a*x + b*y) +
 *   c*z) + t (no bit claim against Eigen's product), then widened.  e12 (EdgeSim3ProjectXYZ): error = obs1 - project1(S12.map(P3D2c)), obs1 =
 *   xy_un1[i].  e21 (EdgeInverseSim3ProjectXYZ): error = obs2 - project2(S12.inverse().map(P3D1c)); obs2 = xy_un2[index2] when the point is in
 *   KF2, otherwise the NORMALISED coordinates the reference writes at :2275-2279 (invz = 1 / z, x * invz, y * invz in float) -- not pixels,
 *   although the edge projects to pixels; such a pair normally leaves in the first classification, and that behaviour is kept, not repaired.
 *   project = f * x / z + c in double (Pinhole.cpp:35-41).  Information = inv_sigma2 * I, chi2 = e0 * (w * e0) + e1 * (w * e1), Huber delta =
 *   (float)sqrt(th2) (:2157).  n_corr = the number of pairs; n_in_kf2 / n_out_kf2 split them by index2.
 * State (thirdparty/g2o/g2o/types/sim3.h).  Quaternion (x, y, z, w), t, s, doubles.  The quaternion comes from R by the matrix-to-quaternion rule
 *   of the PoseOptimization section and is NOT normalised afterwards (Sim3(R, t, s) does not, neither does operator*).  map(X) = s * (r * X) + t,
 *   r * X by Eigen's quaternion-vector formula; inverse() = (r*, r* * ((-1 / s) * t), 1 / s).  An update u = (omega, upsilon, sigma) is applied as
 *   Sim3(u) * estimate (OptimizableTypes.h:158-167) with u[6] = 0 first under fix_scale; Sim3(u) is the exponential of sim3.h:70-142 with all four
 *   branches of (|sigma| < 1e-5, theta < 1e-5), through the matrix-to-quaternion rule again.  No bit claim against Eigen / libm.
 * Jacobian.  The reference defines no linearizeOplus for these edges (OptimizableTypes.h:192, 213), so g2o differentiates numerically
 *   (base_binary_edge.hpp:130-205): column d = (e(exp(+delta e_d) (+) est) - e(exp(-delta e_d) (+) est)) * (1 / (2 delta)), delta = 1e-9; the
 *   points are fixed, so only the 2 x 7 block of the Sim3 vertex exists.  The rule IS that central difference: its rounding noise, about 1e-7
 *   relative in an entry, is part of the path the reference takes.  The 14 perturbed similarities and their 14 inverses are the same for every
 *   edge and are computed once per linearisation.  With fix_scale column 6 is exactly zero and H_66 is lambda alone.
 * System and Levenberg (:2306-2380).  An edge adds B^T (rho[1] w) B to H and subtracts rho[1] B^T (w e) from b (base_binary_edge.hpp:56-120).
 *   The Levenberg loop is the one the PoseOptimization section describes -- lambda init, trial loop, rho, stop rules, the unpivoted LDL^T that
 *   fails at a pivot that is not > 0, x kept after a failure, the NaN behaviour -- with 7 unknowns.
 *   Round 1: optimize(5), all pairs, Huber; it runs whenever n_corr >= 1.  Classification 1: a pair is bad iff chi2_12 > (double)th2 || chi2_21 >
 *   (double)th2, each chi2 read from _error as the last computeActiveErrors() left it -- after a rejected last trial the error at the REJECTED
 *   estimate.  n_bad, n_bad_out_kf2 (bad pairs not in KF2); the survivors lose their kernel.  n_more = n_bad > 0 ? 10 : 5.  n_corr - n_bad < 10:
 *   the function returns 0, the estimate stays the INPUT (the reference returns before :2378) and the bad matches are already removed.
 *   Round 2: optimize(n_more) CONTINUES from round 1's estimate, survivors only, no kernel, lambda afresh.  Final classification: fresh errors at
 *   the final estimate, the same test; a failing pair loses its match, the others count into n_in, the return value.  mAcumHessian is zeroed at
 *   :2356 and never filled: not an output.  At most (5 + 10) x 10 trials run whatever the data.
 * Sums.  The upper triangle of H (28), b (7) and the robust chi2 are folded as in xfh_pose_optimize_device: lane l of 256 adds its keypoints l,
 *   l + 256, .. in that order, e12 before e21; 64 lanes fold by the xor butterfly 32 .. 1; the four waves in order.  Two runs give identical
 *   bytes, and a problem's result does not depend on B or on its neighbours.
 *
 *   xfh_sim3_state_from / _to   13 floats <-> state8 = (qx, qy, qz, qw, tx, ty, tz, s); host, stateless, thread-safe, no ctx, the kernel's own
 *                         lines, as are:  xfh_sim3_oplus (update7, fix_scale), xfh_sim3_map, xfh_sim3_inverse_map (inverse() then map),
 *                         xfh_sim3_solve7 (H28 = the upper triangle row by row; 1, or 0 with x untouched when a pivot is not > 0),
 *                         xfh_sim3_edge: one pair (its two camera-frame points and observations) at one state -> error4 (e12, e21), chi2_2,
 *                         jacobian28 (the 2 x 7 numeric Jacobian of e12 row-major, then e21's) and rho[1] of each Huber kernel (1 when robust
 *                         == 0); any output may be NULL.
 *   xfh_sim3_optimize_workspace_bytes   bytes of d_workspace for B problems of n1 keypoints (0 for arguments the call would refuse).  For n1 <=
 *                         1024 the kernel keeps every pair in registers and does not touch it.
 *   xfh_sim3_optimize_device   B problems, ONE launch, one workgroup each, asynchronous on the ctx stream: no host synchronisation, no allocation.
 *                         Outputs, every one always written: d_assigned_out [B][n1] = the input with -1 where vpMatches1 was set NULL (may be
 *                         d_assigned); d_pair_status [B][n1] bytes XFH_SIM3_OPT_NO_EDGE / _BAD_FIRST / _BAD_FINAL / _INLIER (INLIER = the pair
 *                         kept its match: after the early return that is every survivor of classification 1); d_chi2 [B][n1][2] floats, the
 *                         two values the pair's last classification read, 0 without an edge; d_state [B][8] doubles, the estimate g2oS12 holds
 *                         on return; d_S12_out + b * S12_out_problem_stride, 13 floats in the input layout, the matrix taken from the
 *                         quaternion (may be d_S12 when the strides agree); d_Tcw [B][12], d_Ow [B][3], written (and required) only with d_Tmw:
 *                         gScw = gS12 * Sim3(Rmw, tmw, 1), Tcw = [R | t / s], Ow = -R^T (t / s) in double, rounded once
 *                         (LoopClosing.cc:771-773, ORBmatcher.cc:621-622); d_header [B][XFH_SIM3_OPT_HEADER_INTS] ints: n_corr, n_in_kf2,
 *                         n_out_kf2, n_bad, n_bad_out_kf2, n_more, the return value, classifications run (1 or 2), Levenberg iterations,
 *                         trials, rejected trials, factorisation failures, zeros; d_final_chi2 [B] doubles, currentChi of the last iteration
 *                         that ran (0 if none).
 *                         XFH_ERR_INVALID_ARG before any launch: B outside 1 .. 65535; n1, M1, nq or n2 outside 1 .. XFH_GRID_MAX_N; a NULL
 *                         required pointer; a misaligned pointer (16 bytes for the workspace, 8 for d_state and d_final_chi2, 4 for floats
 *                         and ints); th2 or an inv_sigma2 that is not finite or not > 0; side1_shared, fix_scale or all_points outside 0 .. 1;
 *                         a stride below 13 floats.  Every array may hold anything, NaN, Inf and any int included: no load or store leaves the
 *                         named buffers, and the call terminates.
 *   xfh_sim3_optimize     host-pointer form for ONE problem through the ctx staging arena (S12 and S12_out are 13 floats).
 *   xfh_sim3_optimize_host   the whole rule on ONE host thread over host pointers (workspace included): no ctx, no GPU.
 * Out of scope: KannalaBrandt8, octaves other than 0, OptimizeEssentialGraph and the other graph optimisers. */
enum { XFH_SIM3_OPT_NO_EDGE = 0, XFH_SIM3_OPT_BAD_FIRST = 1, XFH_SIM3_OPT_BAD_FINAL = 2, XFH_SIM3_OPT_INLIER = 3 };
#define XFH_SIM3_OPT_HEADER_INTS 16
#define XFH_SIM3_OPT_S12_FLOATS 13
int xfh_sim3_state_from(const float* S13, double* state8);
int xfh_sim3_state_to(const double* state8, float* S13);
int xfh_sim3_oplus(const double* state8, const double* update7, int fix_scale, double* state8_out);
int xfh_sim3_map(const double* state8, const double* point3, double* out3);
int xfh_sim3_inverse_map(const double* state8, const double* point3, double* out3);
int xfh_sim3_solve7(const double* H28, double lambda, const double* b7, double* x7);
int xfh_sim3_edge(const double* state8, const xfh_camera* cam1, const xfh_camera* cam2, const float* P3D1c, const float* P3D2c, const float* obs1, const float* obs2,
                  float inv_sigma2_1, float inv_sigma2_2, float th2, int fix_scale, int robust, double* error4, double* chi2_2, double* jacobian28, double* rho1_2);
size_t xfh_sim3_optimize_workspace_bytes(int n1, int B);
int xfh_sim3_optimize_device(xfh_ctx* ctx, int B, int n1, int M1, int nq, int n2, int side1_shared, const float* d_T1w, const float* d_xy_un1, const int* d_point1,
                             const float* d_points1, const int* d_assigned, const float* d_points2, const uint8_t* d_flags2, const int* d_index2,
                             const float* d_xy_un2, const float* d_T2w, const float* d_S12, size_t S12_problem_stride, const float* d_Tmw_or_null,
                             const xfh_camera* cam1, const xfh_camera* cam2, float th2, int fix_scale, int all_points, float inv_sigma2_1, float inv_sigma2_2,
                             void* d_workspace, int* d_assigned_out, uint8_t* d_pair_status, float* d_chi2, double* d_state, float* d_S12_out,
                             size_t S12_out_problem_stride, float* d_Tcw, float* d_Ow, int* d_header, double* d_final_chi2);
int xfh_sim3_optimize(xfh_ctx* ctx, int n1, int M1, int nq, int n2, const float* T1w, const float* xy_un1, const int* point1, const float* points1,
                      const int* assigned, const float* points2, const uint8_t* flags2, const int* index2, const float* xy_un2, const float* T2w, const float* S12,
                      const float* Tmw_or_null, const xfh_camera* cam1, const xfh_camera* cam2, float th2, int fix_scale, int all_points, float inv_sigma2_1,
                      float inv_sigma2_2, int* assigned_out, uint8_t* pair_status, float* chi2, double* state, float* S12_out, float* Tcw, float* Ow, int* header,
                      double* final_chi2);
int xfh_sim3_optimize_host(int B, int n1, int M1, int nq, int n2, int side1_shared, const float* T1w, const float* xy_un1, const int* point1, const float* points1,
                           const int* assigned, const float* points2, const uint8_t* flags2, const int* index2, const float* xy_un2, const float* T2w,
                           const float* S12, size_t S12_problem_stride, const float* Tmw_or_null, const xfh_camera* cam1, const xfh_camera* cam2, float th2,
                           int fix_scale, int all_points, float inv_sigma2_1, float inv_sigma2_2, void* workspace, int* assigned_out, uint8_t* pair_status,
                           float* chi2, double* state, float* S12_out, size_t S12_out_problem_stride, float* Tcw, float* Ow, int* header, double* final_chi2);

/* ---- LocalBundleAdjustment: the Schur-complement Levenberg behind the triangulate -> fuse chain of LocalMapping, device resident ----------------------
 * Optimizer::LocalBundleAdjustment (src/Optimizer.cc:1116-1498) from the graph to vToErase (:1188-1460): optimize(10) of OptimizationAlgorithmLevenberg over
 * BlockSolver_6_3 with the Schur complement, then the three loops that fill vToErase.  Conventional Pinhole keyframes, mono and stereo (RGB-D)
 * observations, octave 0, ONE problem per call.  The host keeps :1118-1186 (the three lists) and hands the problem over as indices into two device
 * tables: d_pose_table [pose_rows][12] row-major [R|t] floats and d_point_table [point_rows][3], the map as the tracker's device calls read it.
 *
 * Problem.  nK keyframes d_kf_row [nK] (rows of the pose table); d_kf_fixed [nK] bytes, non-zero for lFixedCameras and for the initial keyframe
 *   inside lLocalKeyFrames (:1220, :1237); n_free = the number of zero bytes, which the host knows and the call needs to size S (a device count
 *   that differs gives status FREE_MISMATCH).  nP points d_point_row [nP].  nE edges in the order the reference creates them, point by point
 *   (:1282-1403): the CSR d_edge_begin [nP + 1], d_edge_kf [nE] (index into the nK keyframes), d_edge_obs [nE][3] = (kpUn.pt.x, kpUn.pt.y,
 *   mvuRight).  ur < 0 is a mono edge (EdgeSE3ProjectXYZ, delta (float)sqrt(5.991)), anything else -- a NaN too -- a stereo edge
 *   (EdgeStereoSE3ProjectXYZ, the FLOAT invz of cam_project in the error and the double one in the Jacobian, delta (float)sqrt(7.815)).
 *   Information = inv_sigma2 * I.  An edge is NO edge (inactive, erase 0, chi2 0) when its keyframe index is outside [0, nK), when the CSR names no
 *   point for it (the first p with edge_begin[p + 1] > e, found in 32 fixed steps, must have edge_begin[p] <= e), or when its keyframe's or its point's
 *   row is outside its table.  A keyframe whose row is outside the table counts as fixed and its Tcw_out is 12 zeros; such a point's points_out is
 *   3 zeros; neither is written back.  A point without an edge is not a vertex: points_out = its input.
 * Statuses, header[0].  OK; ABORTED: no keyframe with d_kf_fixed set has an edge (:1182); NOTHING_FREE: no free keyframe (a STATED DEVIATION: g2o
 *   with zero poses under Schur is not modelled); FREE_MISMATCH.  In the last three every output equals its input, flags and chi2 are 0, final_chi2 0.
 * Edge arithmetic.  The SE3 state, exp(u) * estimate, the error and the pose Jacobian are xfh_pose_optimize_device's.  The point Jacobian is
 *   -projectJac(pc) * R (mono, OptimizableTypes.cpp:139-152) or types_six_dof_expmap.cpp:242-252 (stereo), R = toRotationMatrix of the pose.  An edge
 *   adds A_l^T (rho1 w) A_l to its point's block Hll, -rho1 A_l^T (w e) to bl, and -- when its keyframe is free -- A_p^T (rho1 w) A_p to Hpp, -rho1
 *   A_p^T (w e) to bp and W = A_p^T (rho1 w) A_l to the 6 x 3 cross block; each entry is summed over the edge's rows first.  A fixed keyframe
 *   contributes to its points only.
 * Per iteration.  Errors and the robust chi2 sum at the estimate, the blocks above.  Iteration 0: lambda = 1e-5 * max |diagonal| over the free
 *   keyframes in index order, then the points in index order, with the NaN rule of xfh_pose_optimize_device; ni = 2.
 * Per trial.  lambda goes on both diagonals.  Dinv_p = the closed-form cofactor inverse of Hll_p + lambda I (a singular block makes what it makes).
 *   S = Hpp + lambda I - sum W Dinv W^T, b_S = b_p - sum (W Dinv) b_l.  The pose step: a dense unpivoted LDL^T of S in fp64 that fails at the first pivot
 *   not > 0 (a STATED DEVIATION, as in the two existing optimisers, here standing in for SimplicialLDLT with an AMD ordering).  The point steps by
 *   back-substitution x_l = Dinv (b_l - sum W^T x_p).  After a failed factorisation x (poses and points) keeps its previous values (zero before the first),
 *   the update is applied all the same and tempChi = DBL_MAX.  The pivots of S alone decide, as the matrix alone does in LinearSolverEigen::solve: an
 *   infinite observation gives chi2 = e0 (w e0) + e1 (w e1) = Inf and rho1 = delta / sqrt(Inf) = 0, so H stays finite while b = 0 * Inf is NaN; no
 *   pivot fails, x is NaN and the trial is rejected on a NaN rho.  (A STATED DEVIATION: the reference's chi2 is a dense information * error product,
 *   whose 0 * Inf makes chi2, rho1 and H NaN for the same edge.)  computeScale runs over ALL unknowns, landmarks included.  rho, lambda, ni, the ten-trial
 *   limit, rho == 0 and the three-bad-iterations stop are exactly xfh_pose_optimize_device's Levenberg paragraph; at most max_iterations x 10 trials.
 * Classification.  erase = chi2 > 5.991 (7.815 stereo; doubles, as e->chi2() is compared there) || !isDepthPositive().  chi2 reads _error as the last
 *   computeActiveErrors() left it: after a rejected last trial that is the error at the REJECTED estimate (the stale-error rule of the two existing
 *   optimisers); the depth is computed afresh at the final (restored) estimate.  The host re-checks pMP->isBad() (:1422) when it reads the flags.
 * Summation orders (part of the contract only in being FIXED; tests/ref_local_ba.py mirrors them):
 *   - a point's Hll and bl: its edges' shares added to 0 in edge order (g2o's own order); the back-substitution subtracts edge by edge in edge order,
 *     rows 0 .. 5 of W in turn;
 *   - a keyframe's Hpp, bp and robust chi2: the 256-lane fold of xfh_pose_optimize_device over the keyframe's edges in edge order (lane l adds the
 *     edges l, l + 256, ..; the xor butterfly 32 .. 1 in each wave of 64; the four waves in order);
 *   - a block (i, j), i <= j, of sum W Dinv W^T and b_S: the same fold over keyframe i's edges; an edge's term is (W_e Dinv_p) W_e'^T summed over the
 *     edges e' of the same point at keyframe j in edge order (one, in a proper graph);
 *   - the chi2 of the whole graph: the same fold over the nK keyframe sums; computeScale: the same fold over the 6 n_free pose terms followed by one
 *     term per point (its three terms added to 0);
 *   - the LDL^T: every entry receives its terms in ascending column order; forward substitution ascending, back-substitution DESCENDING.
 *   No floating-point atomic: two runs give identical bytes.  No bit claim against the reference: its order inside a point follows
 *   std::map<KeyFrame*, ..>, pointer values.
 * Out of scope: mpCamera2 / EdgeSE3ProjectXYZToBody, the inertial and merge forms, pbStopFlag in mid-optimisation (the host looks at it once before
 *   the call, :1406).
 *
 *   xfh_lba_edge          host, stateless: one binary edge at pose7 = (qx, qy, qz, qw, tx, ty, tz) and point3 -> error[3], chi2, the pose Jacobian [3][6], the
 *                         point Jacobian [3][3] (third rows zero and error[2] = 0 for a mono edge, obs3[2] < 0) and rho[1]; any output may be NULL.
 *   xfh_lba_point_block   (H6 + lambda I)^-1, H6 = the upper triangle row by row -> Dinv9 row-major.
 *   xfh_lba_solve         the LDL^T above on the lower triangle of S [n][n] (overwritten by L and d) -> 1 and x, or 0 with x untouched; n <= 768.
 *   xfh_local_ba_workspace_bytes   bytes of d_workspace (0 for arguments the call would refuse).
 *   xfh_local_ba_device   asynchronous on the ctx stream: nothing is read back, nothing is allocated.  A fixed schedule of 4 + 53 max_iterations + 2
 *                         launches (536 for optimize(10)) around a control block in the workspace; each kernel returns at once when its step is not
 *                         wanted.  No graph capture, no cooperative launch, no grid barrier; every loop has a bound that does not depend on the data.
 *                         Outputs: d_Tcw_out [nK][12] (a fixed keyframe's: its input bits), d_points_out [nP][3], d_erase [nE] bytes, d_chi2 [nE] floats,
 *                         d_header [10] ints: status, free keyframes, fixed keyframes that have an edge, mono edges, stereo edges, iterations, trials,
 *                         rejected trials, factorisation failures, edges to erase; d_final_chi2: currentChi of the last iteration.  write_back = 1 also
 *                         scatters Tcw_out of the free keyframes and points_out of the points with an edge into the two tables in place.
 *                         XFH_ERR_INVALID_ARG before any launch: n_free > XFH_LBA_MAX_FREE (or < 0, or > nK); nK, nP or nE < 1 (or nK > 65535, nP > 2^22,
 *                         nE > 2^24); pose_rows or point_rows < 1; max_iterations outside 1 .. 10; write_back outside 0 .. 1; a NULL pointer; a misaligned
 *                         pointer (16 bytes for the workspace, 8 for d_final_chi2, 4 for floats and ints); an inv_sigma2 that is not finite or not > 0.
 *                         Points, poses, observations, indices and the CSR may hold anything, NaN and Inf included: the call terminates and no load or
 *                         store leaves the buffers the caller named.
 *   xfh_local_ba          host-pointer form through the ctx staging arena (the tables are copied back when write_back is set).
 *   xfh_local_ba_host     the whole rule on ONE host thread over host pointers (workspace included): the kernels' own lines, no ctx, no GPU. */
#define XFH_LBA_MAX_FREE 128
#define XFH_LBA_MAX_ITERATIONS 10
#define XFH_LBA_HEADER_INTS 10
enum { XFH_LBA_OK = 0, XFH_LBA_ABORTED = 1, XFH_LBA_NOTHING_FREE = 2, XFH_LBA_FREE_MISMATCH = 3 };
int xfh_lba_edge(const double* pose7, const double* point3, const xfh_camera* cam, const float* obs3, float inv_sigma2, double* error3, double* chi2,
                 double* jacobian_pose18, double* jacobian_point9, double* rho1);
int xfh_lba_point_block(const double* H6, double lambda, double* Dinv9);
int xfh_lba_solve(int n, double* S, const double* b, double* x);
size_t xfh_local_ba_workspace_bytes(int nK, int nP, int nE, int n_free);
int xfh_local_ba_device(xfh_ctx* ctx, int nK, int n_free, int nP, int nE, float* d_pose_table, int pose_rows, float* d_point_table, int point_rows,
                        const int* d_kf_row, const uint8_t* d_kf_fixed, const int* d_point_row, const int* d_edge_begin, const int* d_edge_kf,
                        const float* d_edge_obs, const xfh_camera* cam, float inv_sigma2, int max_iterations, int write_back, void* d_workspace, float* d_Tcw_out,
                        float* d_points_out, uint8_t* d_erase, float* d_chi2, int* d_header, double* d_final_chi2);
int xfh_local_ba(xfh_ctx* ctx, int nK, int n_free, int nP, int nE, float* pose_table, int pose_rows, float* point_table, int point_rows, const int* kf_row,
                 const uint8_t* kf_fixed, const int* point_row, const int* edge_begin, const int* edge_kf, const float* edge_obs, const xfh_camera* cam,
                 float inv_sigma2, int max_iterations, int write_back, float* Tcw_out, float* points_out, uint8_t* erase, float* chi2, int* header,
                 double* final_chi2);
int xfh_local_ba_host(int nK, int n_free, int nP, int nE, float* pose_table, int pose_rows, float* point_table, int point_rows, const int* kf_row,
                      const uint8_t* kf_fixed, const int* point_row, const int* edge_begin, const int* edge_kf, const float* edge_obs, const xfh_camera* cam,
                      float inv_sigma2, int max_iterations, int write_back, void* workspace, float* Tcw_out, float* points_out, uint8_t* erase, float* chi2,
                      int* header, double* final_chi2);

/* ---- OptimizeEssentialGraph: the Sim3 pose graph behind the Sim3 Fuse of LoopClosing, on a blocked LDL^T, device resident --------------------------------
 * Optimizer::OptimizeEssentialGraph(Map*, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale) (src/Optimizer.cc:1501-1783) from
 * the vertices to the corrected points (:1532-1779): optimize(20) of OptimizationAlgorithmLevenberg over BlockSolver_7_3 with setUserLambdaInit(1e-16), no
 * Schur complement (nothing is marginalised), no robust kernel, the information matrix the identity.  ONE problem per call.  The host keeps the walk over
 * the map -- everything that needs KeyFrame* / MapPoint* -- and hands the problem over as indices into the two device tables the tracker's calls read:
 * d_pose_table [pose_rows][12] row-major [R|t] floats and d_point_table [point_rows][3].
 *
 * Vertices.  nV vertices in the order of vpKFs with bad keyframes left out: d_kf_row [nV] (rows of the pose table); d_kf_fixed [nV] bytes, non-zero for
 *   mnId == GetInitKFid(); n_free = the number of zero bytes, which the host knows and the call needs to size H (a device count that differs gives status
 *   FREE_MISMATCH).  d_corrected_index [nV] and d_noncorrected_index [nV] index d_sim3 [nS][8] doubles (qx, qy, qz, qw, tx, ty, tz, s), the entries of
 *   CorrectedSim3 / NonCorrectedSim3 as CorrectLoop computed them; anything outside [0, nS) -- -1 by convention -- means "not in that map".
 *   vScw[v] = the corrected entry, or else (Quaterniond(R), t, 1.0) of the pose-table row with R and t widened to double (:1551-1554); Smw[v] = the
 *   non-corrected entry, or else vScw[v] (:1616-1621, :1632-1637).  The estimate starts at vScw[v].  A STATED DEVIATION: the reference takes
 *   Tcw.unit_quaternion() of a Sophus SE3f; here the quaternion comes from the float rotation matrix by Eigen's Quaterniond(Matrix3d) branches, as
 *   xfh_sim3_optimize_device forms its states.  A vertex whose row is outside the table and that has no corrected entry starts at the identity; it has no
 *   edge and its row is never written.
 * Edges.  nE edges in the reference's creation order -- per keyframe first all loop-connection edges (:1577-1605), then the spanning-tree edge, the loop
 *   edges and the covisibility edges (:1608-1706): d_edge_i [nE] (vertex 0), d_edge_j [nE] (vertex 1), d_edge_kind [nE].  Kind 0 is a loop connection, Sji =
 *   vScw[j] * vScw[i]^-1; every other kind a normal edge, Sji = Smw[j] * Smw[i]^-1.  The minFeat / sInsertedEdges / hasChild filters are the host's.  An edge
 *   is NO edge (chi2 0) when an index is outside [0, nV), when both indices are the same, or when a vertex's row is outside the pose table.
 * Points.  d_point_row [nP] (rows of the point table), d_point_ref [nP] the vertex of nIDr (:1759-1768).  A reference outside [0, nV) leaves points_out the
 *   input; a row outside the table gives 3 zeros; neither is written back.
 * Edge arithmetic.  EdgeSim3::computeError (types_seven_dof_expmap.h:106-114): error = ((C * v1) * v2^-1).log(), C the measurement.  Sim3::log follows
 *   sim3.h:148-229 branch for branch: the eps = 1e-5 tests on sigma and d, deltaR, and W.lu().solve(t) as a partial-pivot LU of the 3 x 3 in a fixed order
 *   (column by column the row with the largest |entry|, a later row only when strictly larger).  chi2 = e . e, the seven terms added in index order.  The
 *   Jacobians are g2o's numeric ones (base_binary_edge.hpp:56-205): delta 1e-9, central differences through oplusImpl, as xfh_sim3_optimize_device states
 *   them; with fix_scale the update's seventh entry is zeroed, so column 6 of both Jacobians is exactly 0.  A fixed vertex has no Jacobian and no block.
 * System.  H [7 n_free][7 n_free] with the free vertices in vertex order, b [7 n_free].  An edge adds Ji^T Ji and Jj^T Jj to its vertices' diagonal blocks,
 *   Ji^T Jj to the block of the pair, -Ji^T e and -Jj^T e to b; every entry of an edge's term is summed over the 7 rows first, in row order.
 *   Summation orders (part of the contract only in being FIXED; tests/ref_essential_graph.py mirrors them): a vertex's diagonal block, its b and its share
 *   of chi2 (the edges whose vertex 0 it is) take its edges in edge order through the 256-lane fold of xfh_pose_optimize_device (lane l adds the edges l,
 *   l + 256, ..; the xor butterfly 32 .. 1 in each wave of 64; the four waves in order); an off-diagonal block takes the edges between that pair added to
 *   0 in edge order; the chi2 of the graph is the same fold over the nV vertex shares, computeScale the same fold over the 7 n_free terms.  No
 *   floating-point atomic: two runs give identical bytes.
 * Levenberg.  Exactly the paragraph of xfh_pose_optimize_device / xfh_local_ba_device with these particulars: lambda at iteration 0 is 1e-16, the user
 *   value, not 1e-5 max|diag|; computeScale runs over all 7 n_free unknowns; at most max_iterations <= XFH_EG_MAX_ITERATIONS iterations of at most 10
 *   trials; after a failed factorisation x keeps its previous values (zero before the first), the update is applied all the same and tempChi = DBL_MAX;
 *   chi2 [nE] reads _error as the last computeActiveErrors() left it (the stale-error rule).
 * Solve.  The dense unpivoted fp64 LDL^T of xfh_lba_solve for any n <= 7 XFH_EG_MAX_FREE: it fails at the first pivot not > 0; every entry receives its terms
 *   (L_ik * L_jk) * d_k in ascending k, each as two rounded products and one rounded subtraction; forward substitution ascending, back-substitution
 *   DESCENDING.  On the device a left-looking blocked form over the whole GPU with those bits (xfeatslam_amd/csrc/essgraph.hip.h).  It stands in for
 *   LinearSolverEigen (SimplicialLDLT with an AMD ordering): a STATED DEVIATION, as in the three existing optimisers.
 * Recovery.  Sim3_out [nV][8] doubles: the estimates.  Tcw_out [nV][12] floats = [R | t / s], R from the normalised quaternion in double, rounded once
 *   (:1747); a fixed vertex's row is its vScw recovered the same way.  points_out[p] = Swr_corrected.map(vScw[ref].map(P)) in double, rounded once
 *   (:1771-1776).  write_back = 1 scatters both into the tables (rows inside the tables only; not under FREE_MISMATCH).  UpdateNormalAndDepth and
 *   IncreaseChangeIndex stay with the host.
 * Statuses, header[0].  OK; NOTHING_FREE; FREE_MISMATCH; NO_EDGES: no valid edge.  In the last three nothing is optimised: the outputs are the recovery of
 *   the inputs, chi2 is 0, final_chi2 0.
 * Limit.  XFH_EG_MAX_FREE = 192 free vertices: a system of 1344 x 1344 doubles, 14 MB of workspace, the largest size at which the call has been run and
 *   measured (profiles/essential_graph.md) and its factorisation checked by bits against the column form.  The kernels have no bound of their own below 1024 free vertices (7168 x 7168, 411 MB), for which
 *   the limit was designed; it is raised when a run at that size is on record.  More is refused with XFH_ERR_INVALID_ARG before any
 *   launch and stays on the host's g2o: a capacity limit, not a speed claim.
 * Out of scope: the merge form (:1785), OptimizeEssentialGraph4DoF, the inertial edges (:1709-1725).
 *
 *   xfh_sim3_log          host, stateless: Sim3::log of sim8 = (qx, qy, qz, qw, tx, ty, tz, s) -> (omega, upsilon, sigma).
 *   xfh_eg_edge           host, stateless: one edge with measurement meas8 at the estimates Si8, Sj8 -> error [7], chi2, the Jacobians [7][7] row-major of
 *                         vertex 0 and vertex 1 (zeros where free_i / free_j is 0); any output may be NULL.
 *   xfh_eg_solve          the LDL^T above on the lower triangle of S [n][n] (overwritten by L and d) -> 1 and x, or 0 with x untouched; n <= 1344.  The bits
 *                         of xfh_lba_solve where both take n.
 *   xfh_essential_graph_workspace_bytes   bytes of d_workspace (0 for arguments the call would refuse).
 *   xfh_essential_graph_device   SYNCHRONOUS: this call does not follow the fixed idle schedule of xfh_local_ba_device.  A factorisation is 2 x
 *                         ceil(7 n_free / 64) launches, so the host launches one step at a time and reads a small control record back after every trial: at
 *                         most max_iterations x 10 reads (200), about 21 in a converging run.  It is called once per loop closure from the LoopClosing
 *                         thread; when it returns every output is written.  A HIP error at any read ends the loop and is returned.  No graph capture, no
 *                         cooperative launch, no grid barrier; every loop has a bound that does not depend on the data.
 *                         Outputs: d_Sim3_out [nV][8], d_Tcw_out [nV][12], d_points_out [nP][3], d_chi2 [nE] floats, d_header [9] ints: status, free
 *                         vertices, valid edges, kind-0 edges, iterations, trials, rejected trials, factorisation failures, corrected points;
 *                         d_final_chi2: currentChi of the last iteration.
 *                         XFH_ERR_INVALID_ARG before any launch: n_free > XFH_EG_MAX_FREE (or < 0, or > nV); nV, nE, nP or nS < 1 (or nV > 65535,
 *                         nE > 2^20, nP > 2^22, nS > 2^17); pose_rows or point_rows < 1; max_iterations outside 1 .. 20; write_back or fix_scale outside
 *                         0 .. 1; a NULL pointer; a misaligned pointer (16 bytes for the workspace, 8 for doubles, 4 for floats and ints).  Poses, points,
 *                         similarities and indices may hold anything, NaN and Inf included: the call terminates and no load or store leaves the buffers
 *                         the caller named.
 *   xfh_essential_graph   host-pointer form through the ctx staging arena (the tables are copied back when write_back is set).
 *   xfh_essential_graph_host   the whole rule on ONE host thread over host pointers (workspace included): the kernels' own lines, no ctx, no GPU. */
#define XFH_EG_MAX_FREE 192
#define XFH_EG_MAX_ITERATIONS 20
#define XFH_EG_HEADER_INTS 9
enum { XFH_EG_OK = 0, XFH_EG_NOTHING_FREE = 1, XFH_EG_FREE_MISMATCH = 2, XFH_EG_NO_EDGES = 3 };
int xfh_sim3_log(const double* sim8, double* log7);
int xfh_eg_edge(const double* meas8, const double* Si8, const double* Sj8, int free_i, int free_j, int fix_scale, double* error7, double* chi2,
                double* jacobian_i49, double* jacobian_j49);
int xfh_eg_solve(int n, double* S, const double* b, double* x);
size_t xfh_essential_graph_workspace_bytes(int nV, int nE, int n_free);
int xfh_essential_graph_device(xfh_ctx* ctx, int nV, int n_free, int nE, int nP, int nS, float* d_pose_table, int pose_rows, float* d_point_table,
                               int point_rows, const int* d_kf_row, const uint8_t* d_kf_fixed, const int* d_corrected_index, const int* d_noncorrected_index,
                               const double* d_sim3, const int* d_edge_i, const int* d_edge_j, const int* d_edge_kind, const int* d_point_row,
                               const int* d_point_ref, int fix_scale, int max_iterations, int write_back, void* d_workspace, double* d_Sim3_out, float* d_Tcw_out,
                               float* d_points_out, float* d_chi2, int* d_header, double* d_final_chi2);
int xfh_essential_graph(xfh_ctx* ctx, int nV, int n_free, int nE, int nP, int nS, float* pose_table, int pose_rows, float* point_table, int point_rows,
                        const int* kf_row, const uint8_t* kf_fixed, const int* corrected_index, const int* noncorrected_index, const double* sim3, const int* edge_i,
                        const int* edge_j, const int* edge_kind, const int* point_row, const int* point_ref, int fix_scale, int max_iterations, int write_back,
                        double* Sim3_out, float* Tcw_out, float* points_out, float* chi2, int* header, double* final_chi2);
int xfh_essential_graph_host(int nV, int n_free, int nE, int nP, int nS, float* pose_table, int pose_rows, float* point_table, int point_rows, const int* kf_row,
                             const uint8_t* kf_fixed, const int* corrected_index, const int* noncorrected_index, const double* sim3, const int* edge_i,
                             const int* edge_j, const int* edge_kind, const int* point_row, const int* point_ref, int fix_scale, int max_iterations, int write_back,
                             void* workspace, double* Sim3_out, float* Tcw_out, float* points_out, float* chi2, int* header, double* final_chi2);

/* ---- MLPnPsolver (src/MLPnPsolver.cpp) as Tracking::Relocalization drives it (src/Tracking.cc:3678-3773) ------------------------------------------
 * The step between xfh_bow_search_device (shared = 2: the current frame against the B relocalisation candidates) and xfh_pose_optimize_device:
 * the PnP RANSAC over 6-point sets.  B problems per call, one candidate keyframe each; inputs as xfh_pose_optimize_device takes them: d_xy_un
 * [n][2] (mvKeysUn, shared by all problems), d_assigned [B][n] (row b of the BoW search's d_assigned2: keypoint -> index into problem b's point
 * block; anything outside 0 .. nq - 1 is "none"), d_points [B][nq][3] world positions, d_point_valid_or_null [B][nq] bytes (pMP && !pMP->isBad();
 * NULL = all valid), cam (only the Pinhole model: fx, fy, cx, cy).  max_err = mvLevelSigma2[0] * th2 evaluated in float by the caller (every
 * XFeat keypoint has octave 0).  The rule, written once in xfeatslam_amd/csrc/mlpnp_math.h and compiled for the kernels and for the host entry
 * points below; IEEE double in the order written unless a float is named (the library is built without contraction):
 *   1. Correspondences (:55-97).  The compact list in keypoint order over the keypoints with a valid point (ordered scan, no atomic counter);
 *      N entries.  Bearing vector ((x - cx) / fx, (y - cy) / fy, 1) in float, then widened; it is NOT normalised (cv_br /= cv_br.z is a no-op,
 *      the reference's comment at :77 notwithstanding).  The point stays float and is widened where a double is needed.
 *   2. Parameters (:225-260).  min_inliers_eff = max((int)(N * eps), min_inliers, min_set) and the iteration count need the reference's float
 *      arithmetic and host libm, so the caller passes two tables of n + 1 entries filled by xfh_mlpnp_iterations_table: for each N the
 *      reference's lines :237-255 as written (int nMinInliers = N * eps in float; the float epsilon update; ceil(log(1 - p) / log(1 - pow(eps,
 *      3))); max(1, min(nIterations, max_its)); max_its where the double is not finite or does not fit an int).  min_set is 6 and nothing else.
 *      The count read from the table is clamped into 1 .. max_iters, the number of iterations d_draws holds (1 .. XFH_MLPNP_MAX_ITERS).
 *   3. Too few: N < min_inliers_eff (:106), N < 6 (the set generation is undefined there) or d_n_matches_or_null[b] < min_matches (nmatches <
 *      15, Tracking.cc:3708) -> status TOO_FEW.  The header is written (N, status, -1 for the winner and the best, zeros), d_assigned_out is set
 *      to -1 (the optimiser behind this call must not see another problem's matches) and NOTHING else.
 *   4. The loop of iterate(chunk, ..) (:100-223): `while (mnIterations < its || nCurrent < chunk)`.  A call that starts at iteration k0 =
 *      d_start_iter_or_null[b] (NULL or negative: 0) runs the iterations k0 .. end - 1, end = min(max(its, k0 + chunk), max_iters), unless it
 *      returns earlier.  Iteration k reads the draws 6k .. 6k + 5 of d_draws + b * draws_problem_stride whether or not it qualifies: draw j
 *      indexes the shrinking vector of size N - j as step 4 of xfh_sim3_solve_device has it, six draws instead of three.
 *   5. computePose (:356-658) on the 6 points of a set, or on the flagged inliers (Refine); m points, point i with bearing f_i, basis r_i, s_i:
 *      (a) null-space basis: n = sqrt((x*x + y*y) + 1), sg = x >= 0 ? n : -n, v = (x + sg, y, 1), vv = (v0*v0 + v1*v1) + v2*v2, r = e_2 -
 *          (2 v1 / vv) v, s = e_3 - (2 v2 / vv) v: columns 2 and 3 of the Householder reflection that maps f onto -sg e_1.  STATED DEVIATION: the
 *          reference takes JacobiSVD<.., HouseholderQRPreconditioner> of the 1 x 3 matrix.  A^T A, J^T J and J^T r do not depend on the choice of
 *          basis in exact arithmetic; only the stop test max |J dx| < 1e-5 does.
 *      (b) planar test: S = sum p p^T (uncentred, as the reference has it; six sums).  rank(S) by a full-pivot Householder QR: at step k the
 *          entry of largest magnitude of the remaining corner is swapped to (k, k) (the first in row-major order among equals); the loop ends
 *          when that magnitude is <= 3 DBL_EPSILON times the first step's; the pivot is sqrt(sum of squares of column k from row k down); the
 *          reflector is applied to the remaining columns; a pivot counts when it is > 3 DBL_EPSILON times the largest pivot.  rank == 2: the
 *          eigenvectors of S in increasing eigenvalue order from the Jacobi of (d) (STATED DEVIATION from SelfAdjointEigenSolver), as the rows of
 *          eigenRot; the design matrix uses eigenRot p and has 9 columns (r12 r13 r22 r23 r32 r33 t1 t2 t3), otherwise 12 (r11 .. r33 t1 t2 t3).
 *      (c) A^T A is accumulated directly, entry (i, j), i <= j: the sum over the points of a_i a_j + b_i b_j, where a / b are the point's two
 *          rows of the design matrix (basis vector r / s).  Sums over the 6 points of a set start at 0.0 and add in index order.  Sums over the
 *          inliers of a Refine are the 256-lane fold of xfh_two_view_device: lane l adds the terms of the inlier correspondences l, l + 256, ..
 *          (correspondence index, non-inliers skipped) to 0.0, then s[l] += s[l + h] for h = 128 .. 1.  Every sum of (b) and (g) likewise.
 *      (d) the eigenvector of the smallest eigenvalue of A^T A: one-sided cyclic Jacobi in fp64 on the columns (pairs p < q in lexicographic
 *          order, the rotation of xfh_triangulate_device's step 4, at most 30 sweeps); the column of least norm, the LAST among equals, as
 *          matrixV().col(colsA - 1) does.  STATED DEVIATION from JacobiSVD<MatrixXd>.  Everything after it is invariant to the vector's sign.
 *      (e) non-planar: scale = 1 / cbrt(|n0 n1 n2|) of the column norms (STATED DEVIATION: the reference writes pow(x, 1.0 / 3.0)); the nearest
 *          rotation U V^T = (u0 v0^T + u1 v1^T) + u2 v2^T from the same Jacobi on the 3 x 3 (columns by norm, descending, u = column / norm),
 *          negated when det < 0; tout = R (scale t); the two candidates [R | +-tout] are inverted as rigid motions (R^T, -R^T t: STATED DEVIATION
 *          from the general Matrix4d::inverse()) and the one with the smaller sum of 1 - v.f over the FIRST six points wins (error[0] <
 *          error[1], else the second); R = R^T.  Planar: :532-593 as written, four candidates, the first minimum wins.
 *      (f) rot2rodrigues (acos, sin) and rodrigues2rot (sin, cos) as written.
 *      (g) mlpnp_gn (:694-758), at most 5 rounds.  Residuals r = (r_i . u, s_i . u), u = (R X + T) / |R X + T|.  STATED DEVIATION: the reference's
 *          machine-generated Jacobian is replaced by the same derivative in closed form: g = (n - (n . u) u) / |v|, J[3..5] = g, J[0..2] = -P^T
 *          ((R^T g) x X) with P = (w w^T + (R^T - I)[w]x) / |w|^2; like the reference's it is 0 / 0 at w = 0.  J^T J (21 entries) and J^T r by
 *          the sums of (c); the 6 x 6 system by the unpivoted LDL^T of xfh_pose_optimize_device (STATED DEVIATION from the pivoted Eigen::LDLT; a
 *          pivot that is not > 0 ends the rounds without an update).  Then :744 (any |dx| > 5, or all |dx| > 1: end without update), :748 (stop
 *          after the update when every |J dx| < 1e-5; a NaN is not below) and x -= dx.
 *   6. CheckInliers (:262-293): xc = (float)(((R00 * (double)X + R01 * Y) + R02 * Z) + t0), likewise yc, zc; Pinhole::project in float; there is
 *      NO depth test (a point behind the camera can be an inlier, as in the reference); inlier iff error2 < max_err; a NaN never passes.
 *   7. The decision, order-free.  k ascending from 0; the state (best_count, best_iteration) is carried through the iterations < k0 too, without
 *      returning there.  An iteration qualifies when count_k >= min_inliers_eff and becomes the new best when count_k > best_count.  At every
 *      qualifying k >= k0, Refine (:295-353) runs on the CURRENT best's flags: step 5 on those inliers, step 6, success iff refined_count >
 *      min_inliers_eff.  Refine depends only on the best's flags, so it is evaluated once per distinct best; the winner is the first
 *      qualifying k >= k0 whose best refines.  REFINED: the refined pose and flags.  BEST: the loop ran out and best_count >= min_inliers_eff:
 *      the best iteration's pose and flags.  NONE otherwise.  The pose is [R|t] rounded to float once.
 *      STATED DEVIATION, and the one that changes results beyond last bits: the reference's Refine() as written (:325-334) calls computePose(..,
 *      result) and then CheckInliers(), but never copies `result` into mRi / mti, which only iterate() writes (:152-164).  So the reference counts
 *      and reports the pose of the ITERATION THAT CALLED Refine: it returns at the first qualifying k whose own count_k > min_inliers_eff, with
 *      iteration k's pose and flags, and the re-solve on the best's inliers is discarded.  The rule stores the re-solved pose, as the function's
 *      name, its members (mRefinedTcw, mvbRefinedInliers) and the caller (Tracking.cc:3744-3773) intend: REFINED reports another pose, and can
 *      report other flags, another nInliers, another winning iteration and another consumed count than the reference as written does
 *      (tests/test_mlpnp_forms.py pins both: the rule equals the literal form with that one copy added, and the literal form as written equals
 *      the prediction above made from the rule's own iterations; profiles/mlpnp.md has how often they differ).
 *      Resuming is stateless: mnBestInliers and mvbBestInliers are changed only by the loop, never by Refine, so a second iterate(chunk) on the
 *      same solver is the SAME call with d_start_iter[b] = the previous header's consumed count.
 * Outputs per problem.  d_header [B][16] ints: N, status (XFH_MLPNP_*), its, min_inliers_eff, the winning iteration (-1), nInliers, the best
 * iteration (-1), the best count, the iterations consumed (winner + 1, or end), the number of Refine evaluations the sequential loop would have
 * made on distinct bests, the planar flag of the reported solve, zeros.  d_Tcw [B][12]: written for REFINED and BEST only.  d_inliers [B][n]
 * bytes by keypoint (vbInliers), d_assigned_out [B][n]: d_assigned where the keypoint is an inlier, -1 elsewhere (mCurrentFrame.mvpMapPoints
 * after Tracking.cc:3762-3771: what xfh_pose_optimize_device takes with d_Tcw beside it); both all 0 / all -1 for NONE; for TOO_FEW d_assigned_out is all -1 and d_inliers untouched.
 *
 *   xfh_mlpnp_workspace_bytes  bytes of d_workspace; 0 for sizes the calls refuse.
 *   xfh_mlpnp_solve_device  everything in device memory; asynchronous on the ctx stream, no allocation, no host synchronisation, no global
 *                         atomics; SIX launches whatever the data (the Refine launch is max_iters x B workgroups, one per possible distinct
 *                         best, of which all but the few that exist leave at once: keep max_iters at the draws the caller really holds).  XFH_ERR_INVALID_ARG before anything is queued: B outside 1 .. 65535, n
 *                         outside 1 .. XFH_GRID_MAX_N, nq outside 1 .. 2^24, max_iters outside 1 .. XFH_MLPNP_MAX_ITERS, chunk < 0, max_err not
 *                         finite, rand_max < 1, a draw stride that is neither 0 nor >= 6 * max_iters with B > 1, a NULL pointer (but the
 *                         _or_null ones), a pointer that is not 4-byte (d_workspace: 16-byte) aligned.  Points, keypoints and the camera may
 *                         hold anything, NaN and Inf included, and d_assigned, d_draws, d_start_iter and both tables any int: no load or store
 *                         leaves the buffers, and every loop is bounded (Jacobi sweeps <= 30, GN rounds <= 5).
 *   xfh_mlpnp_solve       host-pointer form for one problem through the ctx staging arena.
 *   xfh_mlpnp_solve_host  the whole rule on ONE host thread over host pointers (workspace included): no ctx, no GPU.  Stateless and
 *                         thread-safe, as are the ones below, each one piece of the rule:
 *   xfh_mlpnp_iterations_table  step 2 for N = 0 .. n
 *   xfh_mlpnp_set         the six indices of one iteration from its six draws and N >= 6
 *   xfh_mlpnp_nullspace   step 5 (a) of one bearing vector -> rs [6]: r then s
 *   xfh_mlpnp_compute_pose  step 5 of the points in use among m >= 6 correspondences (f [m][3], p [m][3] floats; use_or_null [m] bytes, NULL = all;
 *                         at least six in use) -> Rt [12] doubles, row-major [R|t], and the planar flag; fold = 0: the sums in index order (a
 *                         minimal set), 1: the 256-lane fold over the correspondence index (Refine)
 *   xfh_mlpnp_check       step 6 of one correspondence -> error2 and the flag
 * Out of scope: covariance input (use_cov; the reference never sets it); the KannalaBrandt8 model; octaves other than 0; min_set != 6. */
enum { XFH_MLPNP_TOO_FEW = 0, XFH_MLPNP_NONE = 1, XFH_MLPNP_BEST = 2, XFH_MLPNP_REFINED = 3 };
#define XFH_MLPNP_HEADER_INTS 16
#define XFH_MLPNP_MAX_ITERS 1024
size_t xfh_mlpnp_workspace_bytes(int n, int nq, int B, int max_iters);
int xfh_mlpnp_solve_device(xfh_ctx* ctx, int B, int n, int nq, const float* d_xy_un, const int* d_assigned, const float* d_points,
                           const uint8_t* d_point_valid_or_null, const xfh_camera* cam, float max_err, int min_matches, const int* d_n_matches_or_null,
                           const int* d_iters_of_N, const int* d_min_inliers_of_N, int chunk, const int* d_start_iter_or_null, int max_iters,
                           const int* d_draws, size_t draws_problem_stride, int rand_max, void* d_workspace, int* d_header, float* d_Tcw,
                           uint8_t* d_inliers, int* d_assigned_out);
int xfh_mlpnp_solve(xfh_ctx* ctx, int n, int nq, const float* xy_un, const int* assigned, const float* points, const uint8_t* point_valid_or_null,
                    const xfh_camera* cam, float max_err, const int* iters_of_N, const int* min_inliers_of_N, int chunk, int start_iter, int max_iters,
                    const int* draws, int rand_max, int* header, float* Tcw, uint8_t* inliers, int* assigned_out);
int xfh_mlpnp_solve_host(int B, int n, int nq, const float* xy_un, const int* assigned, const float* points, const uint8_t* point_valid_or_null,
                         const xfh_camera* cam, float max_err, int min_matches, const int* n_matches_or_null, const int* iters_of_N,
                         const int* min_inliers_of_N, int chunk, const int* start_iter_or_null, int max_iters, const int* draws,
                         size_t draws_problem_stride, int rand_max, void* workspace, int* header, float* Tcw, uint8_t* inliers, int* assigned_out);
int xfh_mlpnp_iterations_table(double prob, int min_inliers, int max_its, int min_set, float eps, int n, int* iters_of_N /* n + 1 */,
                               int* min_inliers_of_N /* n + 1 */);
int xfh_mlpnp_set(const int* draws6, int rand_max, int N, int* set6);
int xfh_mlpnp_nullspace(const double* f, double* rs);
int xfh_mlpnp_compute_pose(int m, const float* f, const float* p, const uint8_t* use_or_null, int fold, double* Rt, int* planar);
int xfh_mlpnp_check(const double* Rt, const xfh_camera* cam, const float* X, const float* xy, float max_err, float* error2, int* inlier);

/* MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:329-403), batched over map points: group g observes the
 * descriptor rows indices[offsets[g] .. offsets[g+1]) of `table` (n_rows x 64).  Pairwise DescriptorDistance inside
 * the group (diagonal 0), per row the median sorted[(N-1)/2], and the FIRST row with the least median wins:
 * best_pos[g] = its position inside the group, best_median[g] = that median; an empty group gives -1 / INT_MAX
 * (the reference returns without touching mDescriptor).  Groups may hold at most XFH_MAX_GROUP rows.
 * All pointers host memory (the _device variant: device memory, asynchronous, max_group = largest group size). */
#define XFH_MAX_GROUP 256
int xfh_distinctive_csr(xfh_ctx* ctx, const float* table, int n_rows, const int* offsets, const int* indices, int n_groups,
                        int* best_pos, int* best_median);
int xfh_distinctive_csr_device(xfh_ctx* ctx, const float* d_table, int n_rows, const int* d_offsets, const int* d_indices,
                               int n_groups, int max_group, int* d_best_pos, int* d_best_median);

/* ---- multi-GPU exchange (BASELINE.json configs[3]) ---------------------------------------------------
 * Frames are independent: frame i of a batch goes to rank i mod R (one process and one ctx per GPU, every rank holds the
 * weights) and the fixed-size records travel to the rank that runs the sequential SLAM state machine (the reference is
 * one process, src/System.cc:197-233) with RCCL over xGMI.  These calls wrap librccl directly (dlopen at
 * xfh_comm_create); no Python or torch is involved.  Rank 0 calls xfh_comm_unique_id and ships the 128 bytes to the
 * other ranks by any means (TCP, MPI, a file); then every rank calls xfh_comm_create.
 *   xfh_allgather_records   : ncclAllGather -- d_all receives world x B records, rank r's at offset r * B * record_bytes
 *   xfh_gather_records_root : ncclSend / ncclRecv -- only `root` receives (same layout); cheaper when one rank consumes
 *   xfh_gather_compact_root : only header + valid rows travel (a frame with n_valid of nfeatures rows sends n_valid * 284 B);
 *                             shard r lands at d_all + r * xfh_compact_bytes_max(nfeatures, B) with shard_bytes[r] bytes, and
 *                             xfh_unpack_compact restores a frame's padded form on the host.  Needs one host round trip for
 *                             the sizes (the only blocking call of the three).
 * All of them start when the ctx stream reaches the call (the records are complete) and run on the ctx's communication
 * stream, so the next extraction overlaps them; `gen` (0 / 1) names the record buffer generation the call reads:
 * xfh_comm_fence(ctx, gen) makes the ctx stream wait for the last collective on that generation before the buffer is
 * overwritten, xfh_comm_synchronize waits on the host. */
#define XFH_UNIQUE_ID_BYTES 128
int xfh_comm_unique_id(void* id_out /* XFH_UNIQUE_ID_BYTES */);
/* Which librccl the exchange runs on and what it is: "<file> (RCCL a.b.c; its HIP runtime x.y at <file>; libxfeat_hip's HIP runtime x.y at <file>)",
 * "" when none can be loaded.  Search order: $XFH_RCCL_LIB (explicit, no fallback), /opt/rocm/lib/librccl.so.1, librccl.so.1, librccl.so.
 * xfh_comm_create returns XFH_ERR_COMM when that RCCL is bound to another HIP runtime (file or major.minor) than this library. */
const char* xfh_comm_library(void);
int xfh_comm_create(xfh_ctx* ctx, const void* unique_id, int rank, int world);
int xfh_comm_destroy(xfh_ctx* ctx);
int xfh_comm_rank(xfh_ctx* ctx);
int xfh_comm_world(xfh_ctx* ctx);
int xfh_allgather_records(xfh_ctx* ctx, const void* d_records, int B, void* d_all, int gen);
int xfh_gather_records_root(xfh_ctx* ctx, const void* d_records, int B, void* d_all, int root, int gen);
size_t xfh_compact_bytes_max(int nfeatures, int B);
int xfh_gather_compact_root(xfh_ctx* ctx, const void* d_records, int B, void* d_all, size_t* shard_bytes /* [world], root only */, int root, int gen);
int xfh_unpack_compact(const void* shard, size_t nbytes, int frame, int nfeatures, xfh_keypoint* kps_out, float* desc_out, int* n_valid, int* mono_index);
int xfh_allgather_bytes(xfh_ctx* ctx, const void* d_send, size_t nbytes, void* d_recv, int gen);   /* e.g. timings, barriers */
int xfh_comm_fence(xfh_ctx* ctx, int gen);
/* Several ctx of one GPU feeding one communicator (sub-batches of a step, each extracted by its own ctx into one record buffer):
 * xfh_comm_wait_ctx makes the NEXT collective of `ctx` also wait for the work queued on `other` so far; xfh_comm_fence_ctx is
 * xfh_comm_fence for `other`'s stream.  Neither synchronises the host nor orders the two ctx streams against each other. */
int xfh_comm_wait_ctx(xfh_ctx* ctx, xfh_ctx* other);
int xfh_comm_fence_ctx(xfh_ctx* ctx, xfh_ctx* other, int gen);
int xfh_comm_synchronize(xfh_ctx* ctx);

/* ---- plumbing ----------------------------------------------------------------------- */
int xfh_synchronize(xfh_ctx* ctx);
/* run the ctx on an externally owned hipStream_t (e.g. torch's current stream); NULL
 * restores the ctx's own stream */
int xfh_set_stream(xfh_ctx* ctx, void* hip_stream);
const char* xfh_strerror(int status);
const char* xfh_last_hip_error(xfh_ctx* ctx);
/* "xfeat_hip 0.1 (gfx950); built with clang <x.y.z>, HIP <x.y.z>; runtime HIP <n>, driver <n>": the compiler the library was built with and the HIP runtime it
 * met in this process (the library carries hand-counted MFMA hazard padding; tests/test_gpu_hazard.py re-checks it with the GPU box's own compiler) */
const char* xfh_version(void);
int xfh_device_count(void);

/* device-memory helpers so that a host language without a HIP binding can keep inputs and
 * records resident in HBM (used by bench.py and the tests through ctypes) */
int xfh_dev_alloc(void** dptr, size_t nbytes);
int xfh_dev_free(void* dptr);
int xfh_memcpy_h2d(void* dst, const void* src, size_t nbytes);
int xfh_memcpy_d2h(void* dst, const void* src, size_t nbytes);

/* Measurement and debugging entry points (kernel timers, back-to-back timing loops, intermediate tensors, counter
 * calibration kernels) are declared in xfeat_hip_bench.h: they are exported by the same library but are not part of the
 * drop-in surface. */

#ifdef __cplusplus
}
#endif
#endif /* XFEAT_HIP_H */
