"""ctypes binding of libxfeat_hip.so (include/xfeat_hip.h).

The shared library is the product; this module only declares its C ABI for the Python
host-side mirror, the tests and bench.py.  It never falls back to a CPU implementation:
if the library is missing it raises, and every compute call fails loudly when no HIP
device is present (XFH_ERR_NO_DEVICE).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_DIR = os.path.dirname(os.path.abspath(__file__))
# XFEAT_HIP_LIB: another build of the same ABI (the harness only: tests/workers/knob_worker.py and tools/ load the debug build with the test knobs,
# libxfeat_hip_knobs.so, this way -- the library itself reads no such variable)
LIB_PATH = os.environ.get("XFEAT_HIP_LIB") or os.path.join(_DIR, "libxfeat_hip.so")
KNOBS_LIB_PATH = os.path.join(_DIR, "libxfeat_hip_knobs.so")

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
assert KP_DTYPE.itemsize == 28

OK = 0
STATUS = {0: "OK", 1: "INVALID_ARG", 2: "EMPTY_IMAGE", 3: "BAD_SIZE", 4: "NO_WEIGHTS", 5: "BAD_WEIGHTS",
          6: "HIP", 7: "NO_DEVICE", 8: "OUT_OF_MEMORY", 9: "BATCH_TOO_LARGE", 10: "IO", 11: "COMM"}
ERR_EMPTY_IMAGE = 2
ERR_NO_DEVICE = 7
ERR_COMM = 11

K = dict(NONE=0, MNN_GEMM=1, CONV_MFMA=2, CONV_DIRECT=3, NMS=4, SELECT=5, DESC=6, HEADS=7, DIST_I32=8, PREPROC=9, BEST2=10, DISTINCTIVE=11, MNN_GEMM_SEG=12, GRID_BUILD=13, SEARCH_WINDOW=14, FRAME_FINISH=15, PROJ_CANDIDATES=16, PROJ_RESOLVE=17, PROJ_COUNT=18, FUSE_SEARCH=19, TRIANGULATION_SEARCH=20, BOW_CANDIDATES=21, BOW_RESOLVE=22, MAPPROJ_CANDIDATES=23, SIM3_SEARCH=24, SIM3_AGREE=25, INIT_CANDIDATES=27, INIT_RESOLVE=28, INIT_FINAL=29, VOCAB_DESCEND=31, VOCAB_FINISH=32, BOWDB_SCORE=33, BOWDB_SELECT=34, POSE_OPTIMIZE=35, TRIANGULATE_PAIRS=36, TRIANGULATE_WINNER=37, TRIANGULATE_FINISH=38, TWOVIEW_PREPARE=39, TWOVIEW_FIT=40, TWOVIEW_SCORE=41, TWOVIEW_SELECT=42, TWOVIEW_CHECK_RT=43, TWOVIEW_FINAL=44, SIM3SOLVE_PREPARE=45, SIM3SOLVE_FIT=46, SIM3SOLVE_COUNT=47, SIM3SOLVE_DECIDE=48, SIM3SOLVE_MERGE=49, MLPNP_PREPARE=50, MLPNP_FIT=51, MLPNP_COUNT=52, MLPNP_RECORDS=53, MLPNP_REFINE=54, MLPNP_DECIDE=55, SIM3_OPTIMIZE=56, LBA_PLAN=57, LBA_LINEARIZE=58, LBA_POINT_BUILD=59, LBA_BEGIN=60, LBA_SCHUR=61, LBA_SOLVE=62, LBA_UPDATE=63, LBA_EVALUATE=64, LBA_DECIDE=65, LBA_FINISH=66, EG_PLAN=67, EG_LINEARIZE=68, EG_FILL=69, EG_FACTOR=70, EG_SUBST=71, EG_EVALUATE=72, EG_FINISH=73)
T = dict(X=0, XSTAT=1, SKIP_POOL=2, FEATS=6, M1N=7, H1=8, K1H=9, RAW0=16, STAT0=48, SEL=80)


class Config(C.Structure):
    _fields_ = [("device", C.c_int32), ("max_height", C.c_int32), ("max_width", C.c_int32),
                ("nfeatures", C.c_int32), ("max_batch", C.c_int32), ("bn_mode", C.c_int32),
                ("nms_threshold", C.c_float), ("flags", C.c_int32), ("reserved", C.c_int32 * 7)]


class GridBounds(C.Structure):
    """xfh_grid_bounds: mnMinX, mnMinY, mnMaxX, mnMaxY of the frame (0, 0, cols, rows for an undistorted camera)"""
    _fields_ = [("min_x", C.c_float), ("min_y", C.c_float), ("max_x", C.c_float), ("max_y", C.c_float)]


class Camera(C.Structure):
    """xfh_camera: pinhole intrinsics, the radial-tangential coefficients (k1, k2, p1, p2, k3), mbf and the image size"""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("k1", C.c_float), ("k2", C.c_float),
                ("p1", C.c_float), ("p2", C.c_float), ("k3", C.c_float), ("bf", C.c_float), ("width", C.c_int32), ("height", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class Sim3Side(C.Structure):
    """xfh_sim3_side: one keyframe of a SearchBySim3 pair (device pointers for xfh_sim3_search_device, host pointers for xfh_sim3_search)"""
    _fields_ = [("n", C.c_int), ("grid", C.c_void_p), ("kps", C.c_void_p), ("desc", C.c_void_p), ("desc_stride_bytes", C.c_size_t),
                ("points", C.c_void_p), ("dist", C.c_void_p), ("mp_desc", C.c_void_p), ("flags", C.c_void_p), ("Tw", C.c_void_p),
                ("status", C.c_void_p), ("match", C.c_void_p), ("best_dist", C.c_void_p), ("n_window", C.c_void_p), ("n_tested", C.c_void_p),
                ("level", C.c_void_p), ("proj_out", C.c_void_p)]


DEPTH_NONE, DEPTH_F32, DEPTH_U16 = 0, 1, 2
GRID_COLS, GRID_ROWS = 64, 48
GRID_SKIP_PADDING = 1
GRID_MAX_N = 16384
PROJ_POINTS, PROJ_GIVEN = 0, 1
PROJ_INACTIVE, PROJ_BEHIND, PROJ_OUT_OF_BOUNDS, PROJ_NO_CANDIDATES, PROJ_REJECTED, PROJ_MATCHED = range(6)
PROJ_VISIBLE = 3
PROJ_FLAG_ACTIVE, PROJ_FLAG_CLAIMS = 1, 2
FUSE_INACTIVE, FUSE_BEHIND, FUSE_OUT_OF_IMAGE, FUSE_OUT_OF_RANGE, FUSE_BAD_ANGLE, FUSE_NO_CANDIDATES, FUSE_REJECTED, FUSE_FUSED = range(8)
FUSE_VISIBLE = 5
FUSE_FLAG_ACTIVE = 1
FUSE_CHI2 = 1
FUSE_MAX_LEVELS = 16
NODE_NONE = 0xFFFFFFFF
TRI_ONLY_STEREO, TRI_COARSE = 1, 2
TRI_INACTIVE, TRI_NO_NODE, TRI_NO_CANDIDATES, TRI_REJECTED, TRI_MATCHED = range(5)
TRI_GATE_SKIPPED, TRI_GATE_REJECTED, TRI_GATE_PASSED = range(3)
BOW_STRICT_LOW = 1
VOCAB_MAX_CHILDREN, VOCAB_MAX_DEPTH = 32, 32
BOWT_TF_IDF_L1 = 0
BOWDB_MAX_SLOTS, BOWDB_MAX_NEIGHBOURS, BOWDB_HEADER_INTS = 8192, 16, 8
BOWDB_FORM_RELOC, BOWDB_FORM_NBEST = 0, 1
BOWDB_EMPTY, BOWDB_NOT_SHARING, BOWDB_EXCLUDED, BOWDB_BELOW_MIN, BOWDB_SCORED = range(5)
BOWDB_NO_WORD = 0xFFFFFFFF
BOW_INACTIVE, BOW_NO_NODE, BOW_NO_CANDIDATES, BOW_REJECTED, BOW_MATCHED = range(5)
MAPPROJ_INACTIVE, MAPPROJ_BEHIND, MAPPROJ_OUT_OF_IMAGE, MAPPROJ_OUT_OF_RANGE, MAPPROJ_BAD_ANGLE, MAPPROJ_NO_CANDIDATES, MAPPROJ_REJECTED, MAPPROJ_MATCHED = range(8)
MAPPROJ_VISIBLE = 5
MAPPROJ_FLAG_ACTIVE = 1
MAPPROJ_CULL_BEHIND, MAPPROJ_CHECK_ANGLE, MAPPROJ_PROJECT_INVZ, MAPPROJ_BOUNDS_CLOSED = 1, 2, 4, 8
MAPPROJ_FORM_SIM3, MAPPROJ_FORM_SIM3_KF, MAPPROJ_FORM_RELOC = 3, 7, 8
SIM3_INACTIVE, SIM3_BEHIND, SIM3_OUT_OF_IMAGE, SIM3_OUT_OF_RANGE = range(4)
SIM3_NO_CANDIDATES, SIM3_REJECTED, SIM3_FOUND = 5, 6, 7
SIM3_VISIBLE = 5
SIM3_FLAG_ACTIVE = 1
INIT_INACTIVE, INIT_NO_CANDIDATES, INIT_REJECTED, INIT_MATCHED = range(4)
INIT_FLAG_ACTIVE = 1
INIT_NONE = 0x7fffffff
TRIANG_INERTIAL, TRIANG_CLAIM = 1, 2
(TRIANG_NO_MATCH, TRIANG_LOW_PARALLAX, TRIANG_STEREO_NO_DEPTH, TRIANG_DEGENERATE, TRIANG_BEHIND1, TRIANG_BEHIND2, TRIANG_REPROJ1, TRIANG_REPROJ2,
 TRIANG_ZERO_DIST, TRIANG_FAR, TRIANG_SCALE, TRIANG_ACCEPTED, TRIANG_SUPERSEDED) = range(13)
(TWO_VIEW_TOO_FEW, TWO_VIEW_BOTH_ZERO, TWO_VIEW_H_DEGENERATE, TWO_VIEW_F_NO_WINNER, TWO_VIEW_H_GATES, TWO_VIEW_LOW_PARALLAX, TWO_VIEW_OK_H,
 TWO_VIEW_OK_F) = range(8)
TWO_VIEW_MODEL_H, TWO_VIEW_MODEL_F = 1, 2
TWO_VIEW_HEADER_INTS, TWO_VIEW_FLOATS, TWO_VIEW_MAX_ITERS = 24, 48, 4096
SIM3_SOLVE_TOO_FEW, SIM3_SOLVE_NO_MORE, SIM3_SOLVE_CONVERGED = range(3)
SIM3_SOLVE_HEADER_INTS, SIM3_SOLVE_FLOATS, SIM3_SOLVE_HYP_FLOATS, SIM3_SOLVE_MAX_ITERS = 16, 32, 40, 4096
MLPNP_TOO_FEW, MLPNP_NONE, MLPNP_BEST, MLPNP_REFINED = range(4)
MLPNP_HEADER_INTS, MLPNP_MAX_ITERS = 16, 1024
SIM3_OPT_NO_EDGE, SIM3_OPT_BAD_FIRST, SIM3_OPT_BAD_FINAL, SIM3_OPT_INLIER = range(4)
SIM3_OPT_HEADER_INTS, SIM3_OPT_S12_FLOATS = 16, 13

FLAG_RESCALE_KEYPOINTS = 1
FLAG_SERIAL_BRANCH = 2


# every symbol include/xfeat_hip.h declares: (name, restype, argtypes)
_vp, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
_pi = C.POINTER(C.c_int)
SYMBOLS = [
    ("xfh_config_default", None, [C.POINTER(Config)]),
    ("xfh_create", _i, [C.POINTER(Config), C.POINTER(_vp)]),
    ("xfh_destroy", _i, [_vp]),
    ("xfh_load_weights", _i, [_vp, _vp, _sz]),
    ("xfh_load_weights_file", _i, [_vp, C.c_char_p]),
    ("xfh_extract", _i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _pi, _pi]),
    ("xfh_extract_submit", _i, [_vp, _vp, _i, _i, _i, _i, _i]),
    ("xfh_extract_collect", _i, [_vp, _vp, _vp, _pi, _pi]),
    ("xfh_detect_and_compute", _i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _pi, _pi]),
    ("xfh_record_bytes", _sz, [_i]),
    ("xfh_record_kps_offset", _sz, []),
    ("xfh_record_desc_offset", _sz, [_i]),
    ("xfh_extract_batch", _i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    ("xfh_extract_batch_submit", _i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    ("xfh_extract_batch_wait", _i, [_vp]),
    ("xfh_extract_batch_drain", _i, [_vp]),
    ("xfh_pipeline_lanes", _i, [_vp, _i]),
    ("xfh_host_alloc", _i, [C.POINTER(_vp), _sz]),
    ("xfh_host_free", _i, [_vp]),
    ("xfh_host_register", _i, [_vp, _sz]),
    ("xfh_host_unregister", _i, [_vp]),
    ("xfh_extract_batch_device", _i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    ("xfh_extract_batch_device_images", _i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    ("xfh_match_mnn", _i, [_vp, _vp, _i, _vp, _i, _f, _vp, _vp, _vp, _pi]),
    ("xfh_match_mnn_device", _i, [_vp, _vp, _i, _vp, _i, _f, _vp, _vp, _vp, _vp]),
    ("xfh_match_image_bytes", _sz, [_i]),
    ("xfh_match_prepare_device", _i, [_vp, _vp, _i, _vp]),
    ("xfh_match_mnn_prepared_device", _i, [_vp, _vp, _i, _vp, _i, _f, _vp, _vp, _vp, _vp]),
    ("xfh_match_mnn_prepared_batch_device", _i, [_vp, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp]),
    ("xfh_match_records_device", _i, [_vp, _vp, _vp, _vp, _vp, C.c_float, _vp, _vp, _vp, _vp]),
    ("xfh_descriptor_distance", _i, [_vp, _vp]),
    ("xfh_distance_i32", _i, [_vp, _vp, _i, _vp, _i, _vp]),
    ("xfh_distance_i32_device", _i, [_vp, _vp, _i, _vp, _i, _vp]),
    ("xfh_best2_csr", _i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    ("xfh_best2_csr_device", _i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    ("xfh_grid_bytes", _sz, [_i]),
    ("xfh_grid_build_device", _i, [_vp, _vp, _i, _vp, C.POINTER(GridBounds), _i, _vp]),
    ("xfh_grid_build_records_device", _i, [_vp, _vp, _i, C.POINTER(GridBounds), _i, _vp]),
    ("xfh_grid_unpack", _i, [_vp, _sz, _i, _vp, _vp, _pi]),
    ("xfh_search_window_device", _i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    ("xfh_search_window", _i, [_vp, _vp, _vp, _i, _vp, C.POINTER(GridBounds), _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    ("xfh_undistort_points", _i, [C.POINTER(Camera), _vp, _i, _vp]),
    ("xfh_camera_bounds", _i, [C.POINTER(Camera), C.POINTER(GridBounds)]),
    ("xfh_frame_finish_records_device", _i, [_vp, _vp, _i, C.POINTER(Camera), _vp, _i, _sz, _f, C.POINTER(GridBounds), _i, _vp, _vp, _vp, _vp]),
    ("xfh_frame_finish", _i, [_vp, _vp, _i, C.POINTER(Camera), _vp, _i, _sz, _f, _vp, _vp, _vp]),
    ("xfh_project_points", _i, [_vp, C.POINTER(Camera), C.POINTER(GridBounds), _vp, _i, _f, _vp, _vp, _vp]),
    ("xfh_search_projection_workspace_bytes", _sz, [_i, _i, _i]),
    ("xfh_search_projection_device", _i, [_vp, _i, _i, _i, _vp, _vp, _vp, C.POINTER(Camera), C.POINTER(GridBounds), _f, _vp, _vp, _vp, _vp, _sz, _i, _vp, _vp,
                                          _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("xfh_search_projection", _i, [_vp, _i, _i, _vp, _vp, _vp, C.POINTER(Camera), C.POINTER(GridBounds), _f, _vp, _vp, _vp, _vp, _i, _vp, _vp,
                                   _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("xfh_scale_level_thresholds", _i, [_f, _i, _vp]),
    ("xfh_fuse_project", _i, [_vp, _vp, C.POINTER(Camera), C.POINTER(GridBounds), _f, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    ("xfh_fuse_search_device", _i, [_vp, _i, _i, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(Camera), C.POINTER(GridBounds), _f, _vp, _vp, _i,
                                    _vp, _vp, _sz, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("xfh_fuse_search", _i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(Camera), C.POINTER(GridBounds), _f, _vp, _vp, _i, _vp, _vp, _i,
                             _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("xfh_nodes_bytes", _sz, [_i]),
    ("xfh_nodes_pack", _i, [_vp, _i, _vp, _pi]),
    ("xfh_nodes_unpack", _i, [_vp, _sz, _i, _vp, _vp, _vp, _pi]),
    ("xfh_epipolar_gate", _i, [_vp, _vp, _f, _f, _i, _f, _f, _i, _vp, _vp, _i, _vp]),
    ("xfh_triangulation_search_device", _i, [_vp, _i, _i, _i, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp,
                                             _vp, _vp, _vp, _vp, _vp, _vp]),
    ("xfh_triangulation_search", _i, [_vp, _i, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("xfh_bow_accept", _i, [_i, _i, _i, _i, _f, _i]),
    ("xfh_bow_search_workspace_bytes", _sz, [_i, _i, _i]),
    ("xfh_bow_search_device", _i, [_vp, _i, _i, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("xfh_bow_search", _i, [_vp, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("xfh_vocab_bytes", _sz, [_i]),
    ("xfh_vocab_pack", _i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _pi, _pi]),
    ("xfh_vocab_unpack", _i, [_vp, _sz, _i, _pi, _vp, _vp, _vp, _vp, _pi, _pi]),
    ("xfh_vocab_descend", _i, [_vp, _sz, _i, _vp, _vp, _vp, _vp]),
    ("xfh_bow_transform_workspace_bytes", _sz, [_i, _i]),
    ("xfh_bow_transform_device", _i, [_vp, _i, _i, _i, _i, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("xfh_bow_transform", _i, [_vp, _i, _i, _i, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("xfh_bow_score", _i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    ("xfh_bowdb_query_workspace_bytes", _sz, [_i, _i]),
    ("xfh_bowdb_query_device", _i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                    _vp, _vp]),
    ("xfh_bowdb_query", _i, [_vp, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("xfh_map_project", _i, [_vp, _vp, C.POINTER(Camera), C.POINTER(GridBounds), _f, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    ("xfh_map_projection_search_workspace_bytes", _sz, [_i, _i, _i]),
    ("xfh_map_projection_search_device", _i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(Camera), C.POINTER(GridBounds), _f, _vp, _vp, _i,
                                              _vp, _vp, _sz, _i, _i, _vp, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("xfh_map_projection_search", _i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(Camera), C.POINTER(GridBounds), _f, _vp, _vp, _i, _vp, _vp, _i,
                                       _vp, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("xfh_sim3_project", _i, [_vp, _vp, C.POINTER(Camera), C.POINTER(GridBounds), _f, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    ("xfh_sim3_search_device", _i, [_vp, _i, _i, C.POINTER(Sim3Side), C.POINTER(Sim3Side), _vp, _vp, C.POINTER(Camera), C.POINTER(GridBounds), _f, _vp, _vp, _i,
                                    _i, _vp, _vp]),
    ("xfh_sim3_search", _i, [_vp, C.POINTER(Sim3Side), C.POINTER(Sim3Side), _vp, _vp, C.POINTER(Camera), C.POINTER(GridBounds), _f, _vp, _vp, _i, _i, _vp, _vp]),
    ("xfh_init_accept", _i, [_i, _i, _i, _f]),
    ("xfh_init_list_entries", _i, []),
    ("xfh_init_search_workspace_bytes", _sz, [_i, _i, _i]),
    ("xfh_init_search_device", _i, [_vp, _i, _i, _vp, _vp, _vp, _f, _vp, _vp, _sz, _vp, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("xfh_init_search", _i, [_vp, _i, _vp, _vp, _vp, _f, _vp, C.POINTER(GridBounds), _vp, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("xfh_pose_from_tcw", _i, [_vp, _vp]),
    ("xfh_pose_to_tcw", _i, [_vp, _vp]),
    ("xfh_pose_oplus", _i, [_vp, _vp, _vp]),
    ("xfh_pose_solve", _i, [_vp, C.c_double, _vp, _vp]),
    ("xfh_pose_edge", _i, [_vp, C.POINTER(Camera), _vp, _vp, _f, _f, _i, _vp, _vp, _vp, _vp]),
    ("xfh_pose_optimize_workspace_bytes", _sz, [_i, _i]),
    ("xfh_pose_optimize_device", _i, [_vp, _i, _i, _i, _vp, C.POINTER(Camera), _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("xfh_pose_optimize", _i, [_vp, _i, _i, _vp, C.POINTER(Camera), _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp]),
    ("xfh_triangulate_pair", _i, [C.POINTER(Camera), _i, _f, _f, _f, _f, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("xfh_triangulate_device", _i, [_vp, _i, _i, _i, _i, _i, C.POINTER(Camera), _f, _f, _f, _f] + [_vp] * 25),
    ("xfh_triangulate", _i, [_vp, _i, _i, _i, _i, C.POINTER(Camera), _f, _f, _f, _f] + [_vp] * 25),
    ("xfh_two_view_workspace_bytes", _sz, [_i, _i, _i, _i]),
    ("xfh_two_view_device", _i, [_vp, _i, _i, _i, _vp, _vp, _vp, C.POINTER(Camera), _f, _i, _vp, _sz, _i, C.c_double, _i] + [_vp] * 8),
    ("xfh_two_view", _i, [_vp, _i, _i, _vp, _vp, _vp, C.POINTER(Camera), _f, _i, _vp, _i, C.c_double, _i] + [_vp] * 7),
    ("xfh_two_view_host", _i, [_i, _i, _i, _vp, _vp, _vp, C.POINTER(Camera), _f, _i, _vp, _sz, _i, C.c_double, _i] + [_vp] * 8),
    ("xfh_two_view_set", _i, [_vp, _i, _i, _vp]),
    ("xfh_two_view_fit", _i, [_i, _vp, _vp, _vp]),
    ("xfh_two_view_score", _i, [_i, _vp, _f, _vp, _vp, _vp, _vp, _vp]),
    ("xfh_two_view_check_rt", _i, [C.POINTER(Camera), _vp, _f, _vp, _vp, _vp, _vp, _vp]),
    ("xfh_sim3_solve_workspace_bytes", _sz, [_i, _i, _i]),
    ("xfh_sim3_solve_device", _i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp, C.POINTER(Camera), C.POINTER(Camera), _f, _f, _i, _i, _i, _vp, _vp, _i, _vp, _sz, _i] + [_vp] * 6),
    ("xfh_sim3_solve", _i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, C.POINTER(Camera), C.POINTER(Camera), _f, _f, _i, _i, _vp, _i, _vp, _i] + [_vp] * 5),
    ("xfh_sim3_solve_host", _i, [_i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp, C.POINTER(Camera), C.POINTER(Camera), _f, _f, _i, _i, _i, _vp, _vp, _i, _vp, _sz, _i] + [_vp] * 6),
    ("xfh_sim3_solve_iterations", _i, [C.c_double, _i, _i, _i]),
    ("xfh_sim3_solve_iterations_table", _i, [C.c_double, _i, _i, _i, _vp]),
    ("xfh_sim3_solve_set", _i, [_vp, _i, _i, _vp]),
    ("xfh_sim3_solve_horn", _i, [_vp, _vp, _i, _vp]),
    ("xfh_sim3_solve_check", _i, [_vp, _vp, C.POINTER(Camera), C.POINTER(Camera), _vp, _vp, _f, _f, _vp, _vp]),
    ("xfh_mlpnp_workspace_bytes", _sz, [_i, _i, _i, _i]),
    ("xfh_mlpnp_solve_device", _i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, C.POINTER(Camera), _f, _i, _vp, _vp, _vp, _i, _vp, _i, _vp, _sz, _i] + [_vp] * 5),
    ("xfh_mlpnp_solve", _i, [_vp, _i, _i, _vp, _vp, _vp, _vp, C.POINTER(Camera), _f, _vp, _vp, _i, _i, _i, _vp, _i] + [_vp] * 4),
    ("xfh_mlpnp_solve_host", _i, [_i, _i, _i, _vp, _vp, _vp, _vp, C.POINTER(Camera), _f, _i, _vp, _vp, _vp, _i, _vp, _i, _vp, _sz, _i] + [_vp] * 5),
    ("xfh_mlpnp_iterations_table", _i, [C.c_double, _i, _i, _i, _f, _i, _vp, _vp]),
    ("xfh_mlpnp_set", _i, [_vp, _i, _i, _vp]),
    ("xfh_mlpnp_nullspace", _i, [_vp, _vp]),
    ("xfh_mlpnp_compute_pose", _i, [_i, _vp, _vp, _vp, _i, _vp, _vp]),
    ("xfh_mlpnp_check", _i, [_vp, C.POINTER(Camera), _vp, _vp, _f, _vp, _vp]),
    ("xfh_sim3_merge_matches_device", _i, [_vp, _i, _i, _i, _i] + [_vp] * 6),
    ("xfh_sim3_merge_matches", _i, [_vp, _i, _i, _i, _i] + [_vp] * 5),
    ("xfh_sim3_merge_matches_host", _i, [_i, _i, _i, _i] + [_vp] * 6),
    ("xfh_sim3_state_from", _i, [_vp, _vp]),
    ("xfh_sim3_state_to", _i, [_vp, _vp]),
    ("xfh_sim3_oplus", _i, [_vp, _vp, _i, _vp]),
    ("xfh_sim3_map", _i, [_vp, _vp, _vp]),
    ("xfh_sim3_inverse_map", _i, [_vp, _vp, _vp]),
    ("xfh_sim3_solve7", _i, [_vp, C.c_double, _vp, _vp]),
    ("xfh_sim3_edge", _i, [_vp, C.POINTER(Camera), C.POINTER(Camera), _vp, _vp, _vp, _vp, _f, _f, _f, _i, _i, _vp, _vp, _vp, _vp]),
    ("xfh_sim3_optimize_workspace_bytes", _sz, [_i, _i]),
    ("xfh_sim3_optimize_device", _i, [_vp] + [_i] * 6 + [_vp] * 11 + [_sz, _vp, C.POINTER(Camera), C.POINTER(Camera), _f, _i, _i, _f, _f] + [_vp] * 6 + [_sz] + [_vp] * 4),
    ("xfh_sim3_optimize", _i, [_vp] + [_i] * 4 + [_vp] * 12 + [C.POINTER(Camera), C.POINTER(Camera), _f, _i, _i, _f, _f] + [_vp] * 9),
    ("xfh_sim3_optimize_host", _i, [_i] * 6 + [_vp] * 11 + [_sz, _vp, C.POINTER(Camera), C.POINTER(Camera), _f, _i, _i, _f, _f] + [_vp] * 6 + [_sz] + [_vp] * 4),
    ("xfh_lba_edge", _i, [_vp, _vp, C.POINTER(Camera), _vp, _f] + [_vp] * 5),
    ("xfh_lba_point_block", _i, [_vp, C.c_double, _vp]),
    ("xfh_lba_solve", _i, [_i, _vp, _vp, _vp]),
    ("xfh_local_ba_workspace_bytes", _sz, [_i] * 4),
    ("xfh_local_ba_device", _i, [_vp] + [_i] * 4 + [_vp, _i, _vp, _i] + [_vp] * 6 + [C.POINTER(Camera), _f, _i, _i] + [_vp] * 7),
    ("xfh_local_ba", _i, [_vp] + [_i] * 4 + [_vp, _i, _vp, _i] + [_vp] * 6 + [C.POINTER(Camera), _f, _i, _i] + [_vp] * 6),
    ("xfh_local_ba_host", _i, [_i] * 4 + [_vp, _i, _vp, _i] + [_vp] * 6 + [C.POINTER(Camera), _f, _i, _i] + [_vp] * 7),
    ("xfh_sim3_log", _i, [_vp, _vp]),
    ("xfh_eg_edge", _i, [_vp, _vp, _vp, _i, _i, _i] + [_vp] * 4),
    ("xfh_eg_solve", _i, [_i, _vp, _vp, _vp]),
    ("xfh_essential_graph_workspace_bytes", _sz, [_i] * 3),
    ("xfh_essential_graph_device", _i, [_vp] + [_i] * 5 + [_vp, _i, _vp, _i] + [_vp] * 10 + [_i] * 3 + [_vp] * 7),
    ("xfh_essential_graph", _i, [_vp] + [_i] * 5 + [_vp, _i, _vp, _i] + [_vp] * 10 + [_i] * 3 + [_vp] * 6),
    ("xfh_essential_graph_host", _i, [_i] * 5 + [_vp, _i, _vp, _i] + [_vp] * 10 + [_i] * 3 + [_vp] * 7),
    ("xfh_distinctive_csr", _i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _vp]),
    ("xfh_distinctive_csr_device", _i, [_vp, _vp, _i, _vp, _vp, _i, _i, _vp, _vp]),
    ("xfh_comm_unique_id", _i, [_vp]),
    ("xfh_comm_library", C.c_char_p, []),
    ("xfh_comm_create", _i, [_vp, _vp, _i, _i]),
    ("xfh_comm_destroy", _i, [_vp]),
    ("xfh_comm_rank", _i, [_vp]),
    ("xfh_comm_world", _i, [_vp]),
    ("xfh_allgather_records", _i, [_vp, _vp, _i, _vp, _i]),
    ("xfh_gather_records_root", _i, [_vp, _vp, _i, _vp, _i, _i]),
    ("xfh_compact_bytes_max", _sz, [_i, _i]),
    ("xfh_gather_compact_root", _i, [_vp, _vp, _i, _vp, C.POINTER(_sz), _i, _i]),
    ("xfh_unpack_compact", _i, [_vp, _sz, _i, _i, _vp, _vp, _pi, _pi]),
    ("xfh_allgather_bytes", _i, [_vp, _vp, _sz, _vp, _i]),
    ("xfh_comm_fence", _i, [_vp, _i]),
    ("xfh_comm_wait_ctx", _i, [_vp, _vp]),
    ("xfh_comm_fence_ctx", _i, [_vp, _vp, _i]),
    ("xfh_comm_synchronize", _i, [_vp]),
    ("xfh_synchronize", _i, [_vp]),
    ("xfh_set_stream", _i, [_vp, _vp]),
    ("xfh_strerror", C.c_char_p, [_i]),
    ("xfh_last_hip_error", C.c_char_p, [_vp]),
    ("xfh_version", C.c_char_p, []),
    ("xfh_device_count", _i, []),
    ("xfh_dev_alloc", _i, [C.POINTER(_vp), _sz]),
    ("xfh_dev_free", _i, [_vp]),
    ("xfh_memcpy_h2d", _i, [_vp, _vp, _sz]),
    ("xfh_memcpy_d2h", _i, [_vp, _vp, _sz]),
    ("xfh_timing_enable", _i, [_vp, _i, C.c_uint]),
    ("xfh_timing_read", _i, [_vp, _pi, C.POINTER(C.c_double)]),
    ("xfh_bench_mnn_gemm", _i, [_vp, _vp, _i, _vp, _i, _i, C.POINTER(C.c_double)]),
    ("xfh_debug_match_plan", _i, [_i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("xfh_bench_sclk", _i, [_vp, _i, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("xfh_bench_mnn_gemm_batch", _i, [_vp, _i, _vp, _vp, _vp, _vp, _i, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("xfh_bench_match_batch", _i, [_vp, _i, _vp, _vp, _vp, _vp, C.c_float, _vp, _vp, _vp, _vp, _i, C.POINTER(C.c_double)]),
    ("xfh_bench_match_prepared", _i, [_vp, _vp, _i, _vp, _i, C.c_float, _vp, _vp, _vp, _vp, _i, C.POINTER(C.c_double)]),
    ("xfh_bench_match_raw", _i, [_vp, _vp, _i, _vp, _i, C.c_float, _vp, _vp, _vp, _vp, _i, C.POINTER(C.c_double)]),
    ("xfh_bench_calib", _i, [_vp, _i, _sz, _i]),
    ("xfh_kernel_name", C.c_char_p, [_i]),
    ("xfh_debug_tensor", _i, [_vp, _i, _i, _vp, _sz, C.POINTER(_sz)]),
    ("xfh_debug_select", _i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    ("xfh_debug_lba_solve", _i, [_vp, _i, _vp, _vp, _vp, _i, _vp]),
    ("xfh_debug_eg_solve", _i, [_vp, _i, _vp, _vp, _vp, _vp]),
]

_lib = None


def lib():
    """Load libxfeat_hip.so (raises if it has not been built: there is no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(hipcc --offload-arch=gfx950); this package has no CPU fallback")
        L = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(L, name)          # AttributeError if the ABI symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


class XfhError(RuntimeError):
    def __init__(self, status: int, detail: str = ""):
        self.status = status
        msg = lib().xfh_strerror(status).decode()
        super().__init__(f"xfeat_hip status {status} ({STATUS.get(status, '?')}: {msg}) {detail}")


def check(status: int, ctx=None):
    if status != OK:
        detail = ""
        if ctx is not None and status in (6, 11):
            detail = lib().xfh_last_hip_error(ctx).decode()
        raise XfhError(status, detail)


class HostBuffer:
    """pinned host allocation through the C ABI (xfh_host_alloc), viewed as a numpy array"""

    def __init__(self, nbytes: int):
        p = C.c_void_p()
        check(lib().xfh_host_alloc(C.byref(p), nbytes))
        self.ptr = p.value
        self.nbytes = nbytes
        self.array = np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(self.ptr))

    def free(self):
        if self.ptr:
            self.array = None
            lib().xfh_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceBuffer:
    """HBM allocation owned through the C ABI (no torch needed)."""

    def __init__(self, nbytes: int):
        p = C.c_void_p()
        check(lib().xfh_dev_alloc(C.byref(p), nbytes))
        self.ptr = p.value
        self.nbytes = nbytes

    def upload(self, arr: np.ndarray):
        a = np.ascontiguousarray(arr)
        assert a.nbytes <= self.nbytes
        check(lib().xfh_memcpy_h2d(self.ptr, a.ctypes.data, a.nbytes))
        return self

    def download(self, dtype, count: int, offset: int = 0) -> np.ndarray:
        out = np.empty(count, dtype)
        check(lib().xfh_memcpy_d2h(out.ctypes.data, self.ptr + offset, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            lib().xfh_dev_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
