"""Python mirror of the reference's `ORB_SLAM3::XFextractor` (include/XFextractor.h:32-67,
src/XFextractor.cc:75-356) on top of the C ABI in include/xfeat_hip.h.

Same constructor arguments, same `operator()` behaviour (exactly `nfeatures` output rows,
default keypoints / zero descriptor rows as padding, lapping-area placement, return value =
monoIndex, -1 for an empty image) and the same scale getters.  All compute happens in
libxfeat_hip.so on the GPU; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .capi import KP_DTYPE, Config, check, lib
from .layout import Layout

I32, U32, F32, F64, U8 = np.int32, np.uint32, np.float32, np.float64, np.uint8


def _ptr(a):
    """the address of a host array, None for an absent one"""
    return None if a is None else a.ctypes.data


def _opt(a, dt):
    """an optional input as a contiguous array of dt, None when absent"""
    return None if a is None else np.ascontiguousarray(a, dt)


def _names(table, per=None):
    """the names of a table's arrays in its order (per: only the int arrays shaped ("B", per), which the C calls take side by side)"""
    return tuple(name for name, dt, shape in table if per is None or (dt is I32 and shape == ("B", per)))


def _with_prior(out, prior):
    """the zeroed outputs of a host form with the arrays of prior (what the caller's buffers held before the call) put over them"""
    for k, v in (prior or {}).items():
        out[k] = np.ascontiguousarray(v, out[k].dtype).reshape(out[k].shape).copy()
    return out


class Context:
    """Owns one xfh_ctx (one per GPU)."""

    def __init__(self, nfeatures=4096, max_height=480, max_width=640, max_batch=1, device=0, nms_threshold=0.05, bn_mode=0, flags=0):
        cfg = Config()
        lib().xfh_config_default(C.byref(cfg))
        cfg.device, cfg.max_height, cfg.max_width = device, max_height, max_width
        cfg.nfeatures, cfg.max_batch, cfg.nms_threshold = nfeatures, max_batch, nms_threshold
        cfg.bn_mode = bn_mode          # 0 = batch statistics (the reference), 1 = running statistics (upstream eval()), 2 = the same folded into the weights
        cfg.flags = flags              # capi.FLAG_*; 0 = the reference's behaviour
        h = C.c_void_p()
        check(lib().xfh_create(C.byref(cfg), C.byref(h)))
        self.h = h
        self.device = device
        self.nfeatures = nfeatures
        self.max_batch = max_batch
        self.max_height, self.max_width = max_height, max_width
        self.rec_bytes = int(lib().xfh_record_bytes(nfeatures))
        self.kps_off = int(lib().xfh_record_kps_offset())
        self.desc_off = int(lib().xfh_record_desc_offset(nfeatures))

    def close(self):
        if getattr(self, "h", None):
            lib().xfh_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_weights(self, blob: bytes):
        check(lib().xfh_load_weights(self.h, blob, len(blob)), self.h)

    def synchronize(self):
        check(lib().xfh_synchronize(self.h), self.h)

    # -- records --------------------------------------------------------------------------
    def parse_records(self, raw: np.ndarray, B: int):
        """raw u8 [B*rec_bytes] -> list of (kps, desc, n_valid, mono_index, n_candidates)"""
        out = []
        nf = self.nfeatures
        for b in range(B):
            r = raw[b * self.rec_bytes:(b + 1) * self.rec_bytes]
            hdr = r[:16].view(np.int32)
            kps = r[self.kps_off:self.kps_off + 28 * nf].view(KP_DTYPE).copy()
            desc = r[self.desc_off:self.desc_off + 256 * nf].view(np.float32).reshape(nf, 64).copy()
            out.append((kps, desc, int(hdr[0]), int(hdr[1]), int(hdr[2])))
        return out

    def extract_batch(self, frames: np.ndarray, lapping=(0, 0)):
        frames = np.ascontiguousarray(frames, np.uint8)
        B, H, W = frames.shape
        raw = np.empty(B * self.rec_bytes, np.uint8)
        check(lib().xfh_extract_batch(self.h, frames.ctypes.data, B, H, W, int(lapping[0]), int(lapping[1]), raw.ctypes.data), self.h)
        return self.parse_records(raw, B)

    def debug_tensor(self, tid: int, frame: int = 0) -> np.ndarray:
        n = C.c_size_t(0)
        check(lib().xfh_debug_tensor(self.h, tid, frame, None, 0, C.byref(n)), self.h)
        out = np.empty(n.value, np.float32)
        if n.value:
            check(lib().xfh_debug_tensor(self.h, tid, frame, out.ctypes.data, n.value, C.byref(n)), self.h)
        return out

    # -- matching -------------------------------------------------------------------------
    def match_mnn(self, d1: np.ndarray, d2: np.ndarray, min_cossim: float = -1.0):
        d1 = np.ascontiguousarray(d1, np.float32); d2 = np.ascontiguousarray(d2, np.float32)
        n = max(1, min(len(d1), len(d2)))
        i1 = np.zeros(n, np.int32); i2 = np.zeros(n, np.int32); dist = np.zeros(n, np.float32)
        nm = C.c_int(0)
        check(lib().xfh_match_mnn(self.h, d1.ctypes.data, len(d1), d2.ctypes.data, len(d2), float(min_cossim),
                                  i1.ctypes.data, i2.ctypes.data, dist.ctypes.data, C.byref(nm)), self.h)
        k = nm.value
        return i1[:k].copy(), i2[:k].copy(), dist[:k].copy()

    def match_prepare(self, desc: np.ndarray):
        """xfh_match_prepare_device: upload n x 64 rows and build their panel image once -> (DeviceBuffer image, n)"""
        d = np.ascontiguousarray(desc, np.float32)
        n = len(d)
        raw = capi.DeviceBuffer(max(d.nbytes, 16)).upload(d)
        img = capi.DeviceBuffer(max(lib().xfh_match_image_bytes(n), 16))
        check(lib().xfh_match_prepare_device(self.h, raw.ptr, n, img.ptr), self.h)
        self.synchronize()
        raw.free()
        return img, n

    def match_mnn_prepared(self, p1, p2, min_cossim: float = -1.0):
        """xfh_match_mnn_prepared_device on two prepared sets (results identical to match_mnn on their rows)"""
        (img1, n1), (img2, n2) = p1, p2
        nm = max(1, min(n1, n2))
        out = capi.DeviceBuffer(nm * 12 + 64)
        check(lib().xfh_match_mnn_prepared_device(self.h, img1.ptr, n1, img2.ptr, n2, float(min_cossim),
                                                  out.ptr + 64, out.ptr + 64 + 4 * nm, out.ptr + 64 + 8 * nm, out.ptr), self.h)
        self.synchronize()
        k = int(out.download(np.int32, 1)[0])
        if k < 0 or k > nm:
            out.free()
            raise capi.XfhError(6, "k_mnn_post: collector timed out (n_matches < 0)")
        i1 = out.download(np.int32, nm, 64)[:k]; i2 = out.download(np.int32, nm, 64 + 4 * nm)[:k]; dist = out.download(np.float32, nm, 64 + 8 * nm)[:k]
        out.free()
        return i1, i2, dist

    @staticmethod
    def pair_tables(pairs):
        """host-side pointer / size arrays of a many-pairs call: pairs = [((img1, n1), (img2, n2)), ...] -> (p1, n1, p2, n2) ctypes arrays"""
        P = len(pairs)
        p1 = (C.c_void_p * P)(*[a[0].ptr for a, _ in pairs]); p2 = (C.c_void_p * P)(*[b[0].ptr for _, b in pairs])
        n1 = (C.c_int * P)(*[a[1] for a, _ in pairs]); n2 = (C.c_int * P)(*[b[1] for _, b in pairs])
        return p1, n1, p2, n2

    def match_mnn_prepared_batch(self, pairs, min_cossim: float = -1.0):
        """xfh_match_mnn_prepared_batch_device: ORBmatcher::match of every (prepared set, prepared set) pair in one persistent GEMM launch +
        one post launch -> [(idx1, idx2, dist), ...], pair by pair what match_mnn_prepared returns"""
        P = len(pairs)
        if P == 0:
            return []
        nm = [max(1, min(a[1], b[1])) for a, b in pairs]
        off = np.concatenate([[0], np.cumsum([(12 * k + 63) // 64 * 64 for k in nm])]).astype(np.int64)
        out = capi.DeviceBuffer(int(off[-1]) + 64); cnt = capi.DeviceBuffer(4 * P + 64)
        p1, n1, p2, n2 = self.pair_tables(pairs)
        i1 = (C.c_void_p * P)(*[out.ptr + int(off[p]) for p in range(P)])
        i2 = (C.c_void_p * P)(*[out.ptr + int(off[p]) + 4 * nm[p] for p in range(P)])
        ds = (C.c_void_p * P)(*[out.ptr + int(off[p]) + 8 * nm[p] for p in range(P)])
        check(lib().xfh_match_mnn_prepared_batch_device(self.h, P, p1, n1, p2, n2, float(min_cossim), i1, i2, ds, cnt.ptr), self.h)
        self.synchronize()
        ks = cnt.download(np.int32, P)
        res = []
        for p in range(P):
            k = int(ks[p])
            if k < 0 or k > nm[p]:
                out.free(); cnt.free()
                raise capi.XfhError(6, "k_mnn_post_batch: collector timed out (n_matches < 0)")
            res.append((out.download(np.int32, nm[p], int(off[p]))[:k], out.download(np.int32, nm[p], int(off[p]) + 4 * nm[p])[:k],
                        out.download(np.float32, nm[p], int(off[p]) + 8 * nm[p])[:k]))
        out.free(); cnt.free()
        return res

    def distance_i32(self, d1: np.ndarray, d2: np.ndarray) -> np.ndarray:
        d1 = np.ascontiguousarray(d1, np.float32); d2 = np.ascontiguousarray(d2, np.float32)
        out = np.zeros((len(d1), len(d2)), np.int32)
        check(lib().xfh_distance_i32(self.h, d1.ctypes.data, len(d1), d2.ctypes.data, len(d2), out.ctypes.data), self.h)
        return out

    def best2_csr(self, queries, targets, offsets, indices, init_dist: int = 256):
        """guided matching primitive: best / second-best (int)(512*d^2) over per-query candidate lists"""
        q = np.ascontiguousarray(queries, np.float32); tg = np.ascontiguousarray(targets, np.float32)
        off = np.ascontiguousarray(offsets, np.int32); ind = np.ascontiguousarray(indices, np.int32)
        nq = len(q)
        out = [np.zeros(max(nq, 1), np.int32) for _ in range(4)]
        check(lib().xfh_best2_csr(self.h, q.ctypes.data, nq, tg.ctypes.data, len(tg), off.ctypes.data, ind.ctypes.data, int(init_dist),
                                  *[o.ctypes.data for o in out]), self.h)
        return tuple(o[:nq] for o in out)

    # -- frame grid + windowed search (xfh_grid_* / xfh_search_window*) -------------------------
    @staticmethod
    def grid_bytes(n: int) -> int:
        return int(lib().xfh_grid_bytes(n))

    def grid_build_device(self, d_kps, n: int, bounds, flags: int = 0, d_record=None, d_grid=None):
        """xfh_grid_build_device on device pointers (ints); asynchronous.  -> DeviceBuffer holding the grid (d_grid if given)"""
        g = d_grid or capi.DeviceBuffer(self.grid_bytes(n))
        check(lib().xfh_grid_build_device(self.h, d_kps, n, d_record, C.byref(capi.GridBounds(*bounds)), flags, g.ptr), self.h)
        return g

    def grid_build(self, kps: np.ndarray, bounds, flags: int = 0, header=None):
        """Frame::AssignFeaturesToGrid on the GPU: keypoints (KP_DTYPE) -> DeviceBuffer with the grid blob.  header = (n_valid,
        mono_index) of the record the keypoints belong to (needed by GRID_SKIP_PADDING)."""
        k = np.ascontiguousarray(kps, KP_DTYPE)
        n = len(k)
        dk = capi.DeviceBuffer(max(k.nbytes, 16)).upload(k)
        dh = None
        if header is not None:
            dh = capi.DeviceBuffer(16).upload(np.array([header[0], header[1], 0, 0], np.int32))
        g = self.grid_build_device(dk.ptr, n, bounds, flags, dh.ptr if dh else None)
        self.synchronize()
        dk.free()
        if dh:
            dh.free()
        return g

    def grid_build_records(self, d_records, B: int, bounds, flags: int = 0, d_grids=None):
        """xfh_grid_build_records_device: B grids in one launch straight from B extraction records in device memory (pointer);
        asynchronous.  Grid b starts at byte b * grid_bytes(nfeatures) of the returned DeviceBuffer."""
        g = d_grids or capi.DeviceBuffer(max(B, 1) * self.grid_bytes(self.nfeatures))
        check(lib().xfh_grid_build_records_device(self.h, d_records, B, C.byref(capi.GridBounds(*bounds)), flags, g.ptr), self.h)
        return g

    @staticmethod
    def grid_unpack(blob: np.ndarray, n: int):
        """xfh_grid_unpack (host): a downloaded grid blob -> (cell_start[64 * 48 + 1], items[n_binned])"""
        b = np.ascontiguousarray(blob, np.uint8)
        cs = np.zeros(capi.GRID_COLS * capi.GRID_ROWS + 1, np.int32); items = np.zeros(max(n, 1), np.int32); nb = C.c_int(0)
        check(lib().xfh_grid_unpack(b.ctypes.data, b.nbytes, n, cs.ctypes.data, items.ctypes.data, C.byref(nb)))
        return cs, items[:nb.value].copy()

    def grid_download(self, grid, n: int, index: int = 0) -> np.ndarray:
        self.synchronize()
        nb = self.grid_bytes(n)
        return grid.download(np.uint8, nb, index * nb)

    def search_window_device(self, d_queries, d_uvr, nq: int, d_grid, d_targets, nt: int, d_out, init_dist: int = 256,
                             d_skip=None, d_uright=None, d_ur_query=None):
        """xfh_search_window_device on device pointers; d_out: pointer to 5 * nq ints (best_idx, best_dist, second_idx,
        second_dist, n_candidates, nq each); asynchronous"""
        o = [d_out + 4 * nq * k for k in range(5)]
        check(lib().xfh_search_window_device(self.h, d_queries, d_uvr, nq, d_grid, d_targets, nt, d_skip, d_uright, d_ur_query,
                                             int(init_dist), *o), self.h)

    def search_window(self, queries, uvr, kps, bounds, targets, init_dist: int = 256, skip=None, uright=None, ur_query=None):
        """GetFeaturesInArea + the best / second-best loop of SearchByProjection for every query (descriptor row, (u, v, r)) against
        the keypoints / descriptor rows of one frame -> (best_idx, best_dist, second_idx, second_dist, n_candidates)"""
        q = np.ascontiguousarray(queries, np.float32); w = np.ascontiguousarray(uvr, np.float32).reshape(-1, 3)
        k = np.ascontiguousarray(kps, KP_DTYPE); tg = np.ascontiguousarray(targets, np.float32)
        nq, nt = len(q), len(k)
        assert len(w) == nq and len(tg) == nt
        sk = _opt(skip, np.uint8)
        ur = _opt(uright, np.float32)
        uq = _opt(ur_query, np.float32)
        out = [np.zeros(max(nq, 1), np.int32) for _ in range(5)]
        check(lib().xfh_search_window(self.h, q.ctypes.data, w.ctypes.data, nq, k.ctypes.data, C.byref(capi.GridBounds(*bounds)), tg.ctypes.data, nt,
                                      _ptr(sk), _ptr(ur),
                                      _ptr(uq), int(init_dist), *[o.ctypes.data for o in out]), self.h)
        return tuple(o[:nq] for o in out)

    # -- finishing an RGB-D frame (xfh_undistort_points / xfh_camera_bounds / xfh_frame_finish*) ---------
    @staticmethod
    def undistort_points(cam, xy):
        """xfh_undistort_points (host): [n][2] fp32 pixel coordinates -> mvKeysUn coordinates, cv::undistortPoints with P = K"""
        a = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        out = np.empty_like(a)
        check(lib().xfh_undistort_points(C.byref(cam), a.ctypes.data, len(a), out.ctypes.data))
        return out

    @staticmethod
    def camera_bounds(cam):
        """xfh_camera_bounds (host): Frame::ComputeImageBounds -> (mnMinX, mnMinY, mnMaxX, mnMaxY)"""
        b = capi.GridBounds()
        check(lib().xfh_camera_bounds(C.byref(cam), C.byref(b)))
        return (b.min_x, b.min_y, b.max_x, b.max_y)

    def frame_finish_records(self, d_records, B: int, cam, bounds=None, flags: int = 0, d_depth=None, depth_type: int = capi.DEPTH_NONE,
                             depth_pitch: int = 0, depth_scale: float = 1.0, grid: bool = True, out=None):
        """xfh_frame_finish_records_device: UndistortKeyPoints + ComputeStereoFromRGBD + AssignFeaturesToGrid of B extraction records
        in device memory (pointer) in one launch; asynchronous.  d_depth: pointer to B depth images (fp32 metres or raw uint16 times
        depth_scale), rows depth_pitch bytes apart.  -> (xy_un, uright, depth, grids) DeviceBuffers (grids None when grid=False): frame b
        at 2 * b * nfeatures / b * nfeatures floats and b * grid_bytes(nfeatures) bytes.  out = the same tuple from an earlier call."""
        nf = self.nfeatures
        if out is None:
            out = (capi.DeviceBuffer(max(B, 1) * nf * 8), capi.DeviceBuffer(max(B, 1) * nf * 4), capi.DeviceBuffer(max(B, 1) * nf * 4),
                   capi.DeviceBuffer(max(B, 1) * self.grid_bytes(nf)) if grid else None)
        xy, ur, dz, g = out
        gb = C.byref(capi.GridBounds(*bounds)) if bounds is not None else None
        check(lib().xfh_frame_finish_records_device(self.h, d_records, B, C.byref(cam), d_depth, depth_type, depth_pitch, float(depth_scale), gb, flags,
                                                    xy.ptr, ur.ptr, dz.ptr, g.ptr if g else None), self.h)
        return out

    def frame_finish(self, kps, cam, depth=None, depth_scale: float = 1.0):
        """xfh_frame_finish (host pointers): keypoints (KP_DTYPE) and an optional [height][width] depth image (float32 metres, or
        uint16 times depth_scale) -> (xy_un[n][2], uright[n], depth[n])"""
        k = np.ascontiguousarray(kps, KP_DTYPE)
        n = len(k)
        xy = np.zeros((max(n, 1), 2), np.float32); ur = np.zeros(max(n, 1), np.float32); dz = np.zeros(max(n, 1), np.float32)
        img, dt, pitch = None, capi.DEPTH_NONE, 0
        if depth is not None:
            img = np.ascontiguousarray(depth)
            dt = {np.dtype(np.float32): capi.DEPTH_F32, np.dtype(np.uint16): capi.DEPTH_U16}[img.dtype]
            pitch = img.strides[0]
        check(lib().xfh_frame_finish(self.h, k.ctypes.data, n, C.byref(cam), _ptr(img), dt, pitch, float(depth_scale),
                                     xy.ctypes.data, ur.ctypes.data, dz.ctypes.data), self.h)
        return xy[:n], ur[:n], dz[:n]

    # -- SearchByProjection with the reference's claim order (xfh_project_points / xfh_search_projection*) -------
    @staticmethod
    def project_points(Tcw, cam, bounds, xyz, radius: float):
        """xfh_project_points (host): world points [n][3] through the row-major 3x4 pose -> (uvr[n][3], ur[n], status[n])"""
        T = np.ascontiguousarray(Tcw, np.float32).reshape(12); p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n = len(p)
        uvr = np.zeros((max(n, 1), 3), np.float32); ur = np.zeros(max(n, 1), np.float32); st = np.zeros(max(n, 1), np.uint8)
        check(lib().xfh_project_points(T.ctypes.data, C.byref(cam), C.byref(capi.GridBounds(*bounds)), p.ctypes.data, n, float(radius),
                                       uvr.ctypes.data, ur.ctypes.data, st.ctypes.data))
        return uvr[:n], ur[:n], st[:n]

    @staticmethod
    def search_projection_workspace_bytes(nq: int, nt: int, B: int = 1) -> int:
        return int(lib().xfh_search_projection_workspace_bytes(nq, nt, B))

    def search_projection_device(self, mode: int, B: int, nq: int, d_points, d_query_desc, d_query_flags, d_grids, d_targets, target_stride: int, nt: int,
                                 d_workspace, d_out, radius: float = 0.0, d_Tcw=None, cam=None, bounds=None, d_ur_query=None, d_skip=None, d_uright=None,
                                 init_dist: int = 256, th_high: int = 1000, nn_ratio: float = 0.0, d_proj_out=None, guard: int = 0):
        """xfh_search_projection_device on device pointers; asynchronous.  d_out: pointer to the outputs laid out as
        search_projection_layout(B, nq, nt, guard) says"""
        o = self.search_projection_layout(B, nq, nt, guard)
        check(lib().xfh_search_projection_device(self.h, mode, B, nq, d_points, d_ur_query, d_Tcw, C.byref(cam) if cam is not None else None,
                                                 C.byref(capi.GridBounds(*bounds)) if bounds is not None else None, float(radius), d_query_desc, d_query_flags,
                                                 d_grids, d_targets, target_stride, nt, d_skip, d_uright, int(init_dist), int(th_high), float(nn_ratio),
                                                 d_workspace, d_out + o["status"], d_out + o["match_idx"], d_out + o["best_dist"], d_out + o["second_dist"],
                                                 d_out + o["n_candidates"], d_proj_out, d_out + o["assigned"], d_out + o["n_matches"]), self.h)

    SEARCH_PROJECTION_TABLE = (("match_idx", I32, ("B", "nq")), ("best_dist", I32, ("B", "nq")), ("second_dist", I32, ("B", "nq")), ("n_candidates", I32, ("B", "nq")),
                               ("assigned", I32, ("B", "nt")), ("n_matches", I32, ("B",)), ("status", U8, ("B", "nq")))

    @staticmethod
    def search_projection_layout(B: int, nq: int, nt: int, guard: int = 0):
        """byte offsets of the outputs of search_projection_device inside one buffer (and its size under "bytes"); guard > 0 leaves
        at least that many bytes the call never writes before the first array and after every array (for tests that fill them)"""
        return Layout.of(Context.SEARCH_PROJECTION_TABLE, guard, B=B, nq=nq, nt=nt)

    def search_projection(self, mode: int, points, query_desc, query_flags, kps, bounds, targets, radius: float = 0.0, Tcw=None, cam=None,
                          ur_query=None, skip=None, uright=None, init_dist: int = 256, th_high: int = 1000, nn_ratio: float = 0.0):
        """xfh_search_projection (host pointers, one problem) -> dict(status, match_idx, best_dist, second_dist, n_candidates, proj, assigned, n_matches)"""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3); q = np.ascontiguousarray(query_desc, np.float32)
        fl = np.ascontiguousarray(query_flags, np.uint8); k = np.ascontiguousarray(kps, KP_DTYPE); tg = np.ascontiguousarray(targets, np.float32)
        nq, nt = len(p), len(k)
        assert len(q) == nq and len(fl) == nq and len(tg) == nt
        T = None if Tcw is None else np.ascontiguousarray(Tcw, np.float32).reshape(12)
        uq = _opt(ur_query, np.float32)
        sk = _opt(skip, np.uint8)
        ur = _opt(uright, np.float32)
        st = np.zeros(nq, np.uint8); oi = [np.zeros(nq, np.int32) for _ in range(4)]; proj = np.zeros((nq, 3), np.float32)
        asg = np.zeros(nt, np.int32); nm = np.zeros(1, np.int32)
        check(lib().xfh_search_projection(self.h, mode, nq, p.ctypes.data, _ptr(uq), _ptr(T), C.byref(cam) if cam is not None else None,
                                          C.byref(capi.GridBounds(*bounds)), float(radius), q.ctypes.data, fl.ctypes.data, k.ctypes.data, tg.ctypes.data, nt,
                                          _ptr(sk), _ptr(ur), int(init_dist), int(th_high), float(nn_ratio), st.ctypes.data, *[o.ctypes.data for o in oi],
                                          proj.ctypes.data, asg.ctypes.data, nm.ctypes.data), self.h)
        return dict(status=st, match_idx=oi[0], best_dist=oi[1], second_dist=oi[2], n_candidates=oi[3], proj=proj, assigned=asg, n_matches=int(nm[0]))

    def distinctive_csr(self, table, offsets, indices):
        """MapPoint::ComputeDistinctiveDescriptors over CSR groups of descriptor rows ->
        (position inside the group of the descriptor with the least median distance, that median)"""
        tb = np.ascontiguousarray(table, np.float32)
        off = np.ascontiguousarray(offsets, np.int32); ind = np.ascontiguousarray(indices, np.int32)
        ng = len(off) - 1
        pos = np.zeros(max(ng, 1), np.int32); med = np.zeros(max(ng, 1), np.int32)
        check(lib().xfh_distinctive_csr(self.h, tb.ctypes.data, len(tb), off.ctypes.data, ind.ctypes.data, ng, pos.ctypes.data, med.ctypes.data), self.h)
        return pos[:ng], med[:ng]

    # -- Fuse: map points into keyframes (xfh_scale_level_thresholds / xfh_fuse_project / xfh_fuse_search*) -------
    @staticmethod
    def scale_level_thresholds(scale_factor: float, nlevels: int) -> np.ndarray:
        """xfh_scale_level_thresholds (host): ratio_max[nlevels - 1], the table that stands for MapPoint::PredictScale on the device"""
        r = np.zeros(max(nlevels - 1, 1), np.float32)
        check(lib().xfh_scale_level_thresholds(float(scale_factor), int(nlevels), r.ctypes.data))
        return r[:max(nlevels - 1, 0)]

    @staticmethod
    def fuse_project(Tcw, Ow, cam, bounds, th: float, scale_factors, ratio_max, xyz, normals, distances):
        """xfh_fuse_project (host): the per-point arithmetic of ORBmatcher::Fuse for one pose -> (uvr[n][3], ur[n], level[n], status[n])"""
        T = np.ascontiguousarray(Tcw, np.float32).reshape(12); O = np.ascontiguousarray(Ow, np.float32).reshape(3)
        sf = np.ascontiguousarray(scale_factors, np.float32); rm = np.ascontiguousarray(ratio_max, np.float32)
        p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3); nr = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(distances, np.float32).reshape(-1, 3)
        n = len(p)
        assert len(nr) == n and len(d) == n and len(rm) >= len(sf) - 1
        uvr = np.zeros((max(n, 1), 3), np.float32); ur = np.zeros(max(n, 1), np.float32); lv = np.zeros(max(n, 1), np.int32); st = np.zeros(max(n, 1), np.uint8)
        check(lib().xfh_fuse_project(T.ctypes.data, O.ctypes.data, C.byref(cam), C.byref(capi.GridBounds(*bounds)), float(th), sf.ctypes.data, rm.ctypes.data,
                                     len(sf), p.ctypes.data, nr.ctypes.data, d.ctypes.data, n, uvr.ctypes.data, ur.ctypes.data, lv.ctypes.data, st.ctypes.data))
        return uvr[:n], ur[:n], lv[:n], st[:n]

    FUSE_TABLE = (("best_idx", I32, ("B", "nq")), ("best_dist", I32, ("B", "nq")), ("n_window", I32, ("B", "nq")), ("n_tested", I32, ("B", "nq")), ("level", I32, ("B", "nq")),
                  ("proj", F32, ("B", "nq", 3)), ("n_fused", I32, ("B",)), ("status", U8, ("B", "nq")))
    FUSE_OUT_INT = _names(FUSE_TABLE, "nq")

    @staticmethod
    def fuse_search_layout(B: int, nq: int, guard: int = 0):
        """byte offsets of the outputs of fuse_search_device inside one buffer (and its size under "bytes"); guard > 0 leaves at least
        that many bytes the call never writes before the first array and after every array (for tests that fill them)"""
        return Layout.of(Context.FUSE_TABLE, guard, B=B, nq=nq)

    def fuse_search_device(self, B: int, nq: int, query_stride: int, d_points, d_normals, d_distances, d_query_desc, d_query_flags, d_Tcw, d_Ow, cam, bounds,
                           th: float, scale_factors, ratio_max, d_grids, d_targets, target_stride: int, nt: int, d_out, d_uright=None, chi2: bool = True,
                           init_dist: int = 256, th_low: int = 100, proj: bool = True, guard: int = 0):
        """xfh_fuse_search_device on device pointers; asynchronous.  d_out: pointer to the outputs laid out as fuse_search_layout(B, nq,
        guard) says (proj = False: the proj block is left alone)"""
        o = self.fuse_search_layout(B, nq, guard)
        sf = np.ascontiguousarray(scale_factors, np.float32); rm = np.ascontiguousarray(ratio_max, np.float32)
        check(lib().xfh_fuse_search_device(self.h, B, nq, query_stride, d_points, d_normals, d_distances, d_query_desc, d_query_flags, d_Tcw, d_Ow, C.byref(cam),
                                           C.byref(capi.GridBounds(*bounds)), float(th), sf.ctypes.data, rm.ctypes.data, len(sf), d_grids, d_targets,
                                           target_stride, nt, d_uright, capi.FUSE_CHI2 if chi2 else 0, int(init_dist), int(th_low), d_out + o["status"],
                                           *[d_out + o[k] for k in self.FUSE_OUT_INT], d_out + o["proj"] if proj else None, d_out + o["n_fused"]), self.h)

    def fuse_search(self, points, normals, distances, query_desc, query_flags, Tcw, Ow, cam, bounds, th: float, scale_factors, ratio_max, kps, targets,
                    uright=None, chi2: bool = True, init_dist: int = 256, th_low: int = 100):
        """xfh_fuse_search (host pointers, one keyframe) -> dict(status, best_idx, best_dist, n_window, n_tested, level, proj, n_fused)"""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3); nr = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(distances, np.float32).reshape(-1, 3); q = np.ascontiguousarray(query_desc, np.float32)
        fl = np.ascontiguousarray(query_flags, np.uint8); k = np.ascontiguousarray(kps, KP_DTYPE); tg = np.ascontiguousarray(targets, np.float32)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(12); O = np.ascontiguousarray(Ow, np.float32).reshape(3)
        sf = np.ascontiguousarray(scale_factors, np.float32); rm = np.ascontiguousarray(ratio_max, np.float32)
        nq, nt = len(p), len(k)
        assert len(nr) == nq and len(d) == nq and len(q) == nq and len(fl) == nq and len(tg) == nt and len(rm) >= len(sf) - 1
        ur = _opt(uright, np.float32)
        st = np.zeros(nq, np.uint8); oi = [np.zeros(nq, np.int32) for _ in range(5)]; proj = np.zeros((nq, 3), np.float32); nf = np.zeros(1, np.int32)
        check(lib().xfh_fuse_search(self.h, nq, p.ctypes.data, nr.ctypes.data, d.ctypes.data, q.ctypes.data, fl.ctypes.data, T.ctypes.data, O.ctypes.data,
                                    C.byref(cam), C.byref(capi.GridBounds(*bounds)), float(th), sf.ctypes.data, rm.ctypes.data, len(sf), k.ctypes.data,
                                    tg.ctypes.data, nt, _ptr(ur), capi.FUSE_CHI2 if chi2 else 0, int(init_dist), int(th_low),
                                    st.ctypes.data, *[o.ctypes.data for o in oi], proj.ctypes.data, nf.ctypes.data), self.h)
        r = dict(zip(self.FUSE_OUT_INT, oi))
        r.update(status=st, proj=proj, n_fused=int(nf[0]))
        return r

    # -- SearchForTriangulation over feature-vector nodes (xfh_nodes_* / xfh_epipolar_gate / xfh_triangulation_search*) -------
    @staticmethod
    def nodes_bytes(n: int) -> int:
        return int(lib().xfh_nodes_bytes(n))

    @staticmethod
    def nodes_pack(node_of) -> np.ndarray:
        """xfh_nodes_pack (host): node_of[n] (uint32, capi.NODE_NONE = in no node) -> the node blob as bytes, ready for upload"""
        no = np.ascontiguousarray(node_of, np.uint32)
        n = len(no)
        blob = np.full(max(Context.nodes_bytes(n), 16), 0xA5, np.uint8)
        check(lib().xfh_nodes_pack(no.ctypes.data, n, blob.ctypes.data, None))
        return blob

    @staticmethod
    def nodes_unpack(blob: np.ndarray, n: int):
        """xfh_nodes_unpack (host): a node blob -> (node_ids[n_nodes], node_start[n_nodes + 1], items[n_items])"""
        b = np.ascontiguousarray(blob, np.uint8)
        ids = np.zeros(max(n, 1), np.uint32); ns = np.zeros(max(n, 1) + 1, np.int32); items = np.zeros(max(n, 1), np.int32); nn = C.c_int(0)
        check(lib().xfh_nodes_unpack(b.ctypes.data, b.nbytes, n, ids.ctypes.data, ns.ctypes.data, items.ctypes.data, C.byref(nn)))
        return ids[:nn.value].copy(), ns[:nn.value + 1].copy(), items[:ns[nn.value]].copy()

    @staticmethod
    def epipolar_gate(F12, ep, epipole_r2: float, unc: float, flags: int, x1: float, y1: float, stereo1: bool, xy2, uright2=None) -> np.ndarray:
        """xfh_epipolar_gate (host): the gates of SearchForTriangulation for one keypoint of KF1 against n of KF2 -> capi.TRI_GATE_* per keypoint"""
        Fm = np.ascontiguousarray(F12, np.float32).reshape(9); e = np.ascontiguousarray(ep, np.float32).reshape(2)
        xy = np.ascontiguousarray(xy2, np.float32).reshape(-1, 2)
        ur = _opt(uright2, np.float32)
        n = len(xy)
        assert ur is None or len(ur) == n
        out = np.zeros(max(n, 1), np.uint8)
        check(lib().xfh_epipolar_gate(Fm.ctypes.data, e.ctypes.data, float(epipole_r2), float(unc), int(flags), float(x1), float(y1), int(bool(stereo1)),
                                      xy.ctypes.data, _ptr(ur), n, out.ctypes.data))
        return out[:n]

    TRI_TABLE = (("match12", I32, ("B", "n1")), ("best_dist", I32, ("B", "n1")), ("n_candidates", I32, ("B", "n1")), ("n_geom", I32, ("B", "n1")), ("n_matches", I32, ("B",)),
                 ("status", U8, ("B", "n1")))
    TRI_OUT_INT = _names(TRI_TABLE, "n1")

    @staticmethod
    def triangulation_search_layout(B: int, n1: int, guard: int = 0):
        """byte offsets of the outputs of triangulation_search_device inside one buffer (and its size under "bytes"); guard as in
        fuse_search_layout"""
        return Layout.of(Context.TRI_TABLE, guard, B=B, n1=n1)

    def triangulation_search_device(self, B: int, n1: int, n2: int, side1_shared: bool, d_nodes1, d_xy1, d_uright1, d_has1, d_desc1, desc1_stride: int,
                                    d_nodes2, d_xy2, d_uright2, d_has2, d_desc2, desc2_stride: int, d_F12, d_ep, d_out, only_stereo: bool = False,
                                    coarse: bool = False, th_low: int = 100, epipole_r2: float = 100.0, unc: float = 1.0, guard: int = 0):
        """xfh_triangulation_search_device on device pointers; asynchronous.  d_out: pointer to the outputs laid out as
        triangulation_search_layout(B, n1, guard) says"""
        o = self.triangulation_search_layout(B, n1, guard)
        flags = (capi.TRI_ONLY_STEREO if only_stereo else 0) | (capi.TRI_COARSE if coarse else 0)
        check(lib().xfh_triangulation_search_device(self.h, B, n1, n2, 1 if side1_shared else 0, flags, int(th_low), float(epipole_r2), float(unc),
                                                    d_nodes1, d_xy1, d_uright1, d_has1, d_desc1, desc1_stride, d_nodes2, d_xy2, d_uright2, d_has2, d_desc2,
                                                    desc2_stride, d_F12, d_ep, d_out + o["status"], *[d_out + o[k] for k in self.TRI_OUT_INT],
                                                    d_out + o["n_matches"]), self.h)

    def triangulation_search(self, node_of1, xy1, has1, desc1, node_of2, xy2, has2, desc2, F12, ep, uright1=None, uright2=None, only_stereo: bool = False,
                             coarse: bool = False, th_low: int = 100, epipole_r2: float = 100.0, unc: float = 1.0):
        """xfh_triangulation_search (host pointers, one keyframe pair) -> dict(status, match12, best_dist, n_candidates, n_geom, n_matches)"""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        no1, no2 = np.ascontiguousarray(node_of1, np.uint32), np.ascontiguousarray(node_of2, np.uint32)
        x1, x2, d1, d2 = f32(xy1).reshape(-1, 2), f32(xy2).reshape(-1, 2), f32(desc1), f32(desc2)
        h1, h2 = np.ascontiguousarray(has1, np.uint8), np.ascontiguousarray(has2, np.uint8)
        Fm, e = f32(F12).reshape(9), f32(ep).reshape(2)
        n1, n2 = len(no1), len(no2)
        assert len(x1) == n1 and len(h1) == n1 and len(d1) == n1 and len(x2) == n2 and len(h2) == n2 and len(d2) == n2
        u1 = None if uright1 is None else f32(uright1); u2 = None if uright2 is None else f32(uright2)
        st = np.zeros(n1, np.uint8); oi = [np.zeros(n1, np.int32) for _ in range(4)]; nm = np.zeros(1, np.int32)
        flags = (capi.TRI_ONLY_STEREO if only_stereo else 0) | (capi.TRI_COARSE if coarse else 0)
        check(lib().xfh_triangulation_search(self.h, n1, n2, flags, int(th_low), float(epipole_r2), float(unc), no1.ctypes.data, x1.ctypes.data,
                                             _ptr(u1), h1.ctypes.data, d1.ctypes.data, no2.ctypes.data, x2.ctypes.data,
                                             _ptr(u2), h2.ctypes.data, d2.ctypes.data, Fm.ctypes.data, e.ctypes.data,
                                             st.ctypes.data, *[o.ctypes.data for o in oi], nm.ctypes.data), self.h)
        r = dict(zip(self.TRI_OUT_INT, oi))
        r.update(status=st, n_matches=int(nm[0]))
        return r

    # -- SearchByBoW over feature-vector nodes (xfh_bow_accept / xfh_bow_search*) ---------------------------------------------
    BOW_TABLE = (("match12", I32, ("B", "n1")), ("best_dist", I32, ("B", "n1")), ("second_dist", I32, ("B", "n1")), ("n_candidates", I32, ("B", "n1")),
                 ("assigned2", I32, ("B", "n2")), ("n_matches", I32, ("B",)), ("status", U8, ("B", "n1")))
    BOW_OUT_INT = _names(BOW_TABLE, "n1")

    @staticmethod
    def bow_accept(best_idx: int, best: int, second: int, th_low: int, nn_ratio: float, flags: int = 0) -> bool:
        """xfh_bow_accept (host): the acceptance line of SearchByBoW"""
        return bool(lib().xfh_bow_accept(int(best_idx), int(best), int(second), int(th_low), float(nn_ratio), int(flags)))

    @staticmethod
    def bow_search_workspace_bytes(n1: int, n2: int, B: int = 1) -> int:
        return int(lib().xfh_bow_search_workspace_bytes(n1, n2, B))

    @staticmethod
    def bow_search_layout(B: int, n1: int, n2: int, guard: int = 0):
        """byte offsets of the outputs of bow_search_device inside one buffer (and its size under "bytes"); guard as in fuse_search_layout.
        The workspace is a buffer of its own (bow_search_workspace_bytes)."""
        return Layout.of(Context.BOW_TABLE, guard, B=B, n1=n1, n2=n2)

    def bow_search_device(self, B: int, n1: int, n2: int, shared: int, d_nodes1, d_active1, d_desc1, desc1_stride: int, d_nodes2, d_eligible2, d_desc2,
                          desc2_stride: int, d_workspace, d_out, strict_low: bool = False, init_dist: int = 256, th_low: int = 100, nn_ratio: float = 0.6,
                          guard: int = 0):
        """xfh_bow_search_device on device pointers; asynchronous.  shared: 0 none, 1 side 1, 2 side 2.  d_out: pointer to the outputs laid
        out as bow_search_layout(B, n1, n2, guard) says"""
        o = self.bow_search_layout(B, n1, n2, guard)
        check(lib().xfh_bow_search_device(self.h, B, n1, n2, int(shared), capi.BOW_STRICT_LOW if strict_low else 0, int(init_dist), int(th_low), float(nn_ratio),
                                          d_nodes1, d_active1, d_desc1, desc1_stride, d_nodes2, d_eligible2, d_desc2, desc2_stride, d_workspace,
                                          d_out + o["status"], *[d_out + o[k] for k in self.BOW_OUT_INT], d_out + o["assigned2"], d_out + o["n_matches"]), self.h)

    def bow_search(self, node_of1, active1, desc1, node_of2, desc2, eligible2=None, strict_low: bool = False, init_dist: int = 256, th_low: int = 100,
                   nn_ratio: float = 0.6):
        """xfh_bow_search (host pointers, one problem) -> dict(status, match12, best_dist, second_dist, n_candidates, assigned2, n_matches)"""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        no1, no2 = np.ascontiguousarray(node_of1, np.uint32), np.ascontiguousarray(node_of2, np.uint32)
        d1, d2 = f32(desc1), f32(desc2)
        a1 = np.ascontiguousarray(active1, np.uint8)
        e2 = _opt(eligible2, np.uint8)
        n1, n2 = len(no1), len(no2)
        assert len(a1) == n1 and len(d1) == n1 and len(d2) == n2 and (e2 is None or len(e2) == n2)
        st = np.zeros(n1, np.uint8); oi = [np.zeros(n1, np.int32) for _ in range(4)]; as2 = np.zeros(n2, np.int32); nm = np.zeros(1, np.int32)
        check(lib().xfh_bow_search(self.h, n1, n2, capi.BOW_STRICT_LOW if strict_low else 0, int(init_dist), int(th_low), float(nn_ratio), no1.ctypes.data,
                                   a1.ctypes.data, d1.ctypes.data, no2.ctypes.data, _ptr(e2), d2.ctypes.data, st.ctypes.data,
                                   *[o.ctypes.data for o in oi], as2.ctypes.data, nm.ctypes.data), self.h)
        r = dict(zip(self.BOW_OUT_INT, oi))
        r.update(status=st, assigned2=as2, n_matches=int(nm[0]))
        return r

    # -- the vocabulary transform: BowVector and node blobs (xfh_vocab_* / xfh_bow_transform*) ------------------------------------------------
    @staticmethod
    def vocab_bytes(n_nodes: int) -> int:
        return int(lib().xfh_vocab_bytes(n_nodes))

    @staticmethod
    def vocab_pack(parent, word_id, weight, desc, L: int):
        """xfh_vocab_pack (host): m_nodes flattened in node-id order (parent[n], word_id[n], weight[n], desc[n][32] bytes; node 0 = the root)
        -> (the vocabulary blob as bytes, ready for upload, max_children, depth)"""
        pa, wi = np.ascontiguousarray(parent, np.uint32), np.ascontiguousarray(word_id, np.uint32)
        wt, de = np.ascontiguousarray(weight, np.float64), np.ascontiguousarray(desc, np.uint8)
        n = len(pa)
        assert len(wi) == n and len(wt) == n and de.shape == (n, 32)
        blob = np.full(max(Context.vocab_bytes(n), 16), 0xA5, np.uint8)
        mc, dp = C.c_int(0), C.c_int(0)
        check(lib().xfh_vocab_pack(n, int(L), pa.ctypes.data, wi.ctypes.data, wt.ctypes.data, de.ctypes.data, blob.ctypes.data, C.byref(mc), C.byref(dp)))
        return blob, mc.value, dp.value

    @staticmethod
    def vocab_unpack(blob: np.ndarray, n_nodes: int):
        """xfh_vocab_unpack (host): a vocabulary blob -> dict(L, parent, word_id, weight, desc, max_children, depth) in node-id order"""
        b = np.ascontiguousarray(blob, np.uint8)
        n = max(n_nodes, 1)
        pa, wi, wt, de = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.float64), np.zeros((n, 32), np.uint8)
        L, mc, dp = C.c_int(0), C.c_int(0), C.c_int(0)
        check(lib().xfh_vocab_unpack(b.ctypes.data, b.nbytes, n_nodes, C.byref(L), pa.ctypes.data, wi.ctypes.data, wt.ctypes.data, de.ctypes.data,
                                     C.byref(mc), C.byref(dp)))
        return dict(L=L.value, parent=pa, word_id=wi, weight=wt, desc=de, max_children=mc.value, depth=dp.value)

    @staticmethod
    def vocab_descend(blob: np.ndarray, rows, levelsup: int = 4):
        """xfh_vocab_descend (host) for every row (float32 [n][>= 8] or any array with >= 32 bytes per row) -> (word[n], node[n], weight[n])"""
        b = np.ascontiguousarray(blob, np.uint8)
        r = np.ascontiguousarray(rows)
        r = r.reshape(len(r), -1).view(np.uint8)
        n = len(r)
        first = np.ascontiguousarray(r[:, :32])
        word, node, wt = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.float64)
        L = lib()
        for i in range(n):
            check(L.xfh_vocab_descend(b.ctypes.data, b.nbytes, int(levelsup), first.ctypes.data + 32 * i, word.ctypes.data + 4 * i, node.ctypes.data + 4 * i,
                                      wt.ctypes.data + 8 * i))
        return word, node, wt

    @staticmethod
    def bow_transform_workspace_bytes(n: int, B: int = 1) -> int:
        return int(lib().xfh_bow_transform_workspace_bytes(n, B))

    BOW_TRANSFORM_TABLE = (("word", U32, ("B", "n")), ("node_of", U32, ("B", "n")), ("weight", F64, ("B", "n")), ("nodes", U8, ("B", "nodes_bytes")),
                           ("bow_ids", U32, ("B", "n")), ("bow_vals", F64, ("B", "n")), ("n_words", I32, ("B",)))

    @staticmethod
    def bow_transform_layout(B: int, n: int, guard: int = 0):
        """byte offsets of the outputs of bow_transform_device inside one buffer (and its size under "bytes"); guard as in fuse_search_layout.
        The workspace is a buffer of its own (bow_transform_workspace_bytes)."""
        return Layout.of(Context.BOW_TRANSFORM_TABLE, guard, B=B, n=n, nodes_bytes=Context.nodes_bytes(n))

    def bow_transform_device(self, B: int, n: int, d_vocab, vocab_bytes: int, d_desc, desc_stride: int, d_workspace, d_out, levelsup: int = 4, guard: int = 0):
        """xfh_bow_transform_device on device pointers; asynchronous.  d_out: pointer to the outputs laid out as bow_transform_layout(B, n,
        guard) says; d_out + layout["nodes"] then feeds bow_search_device / triangulation_search_device"""
        o = self.bow_transform_layout(B, n, guard)
        check(lib().xfh_bow_transform_device(self.h, B, n, int(levelsup), capi.BOWT_TF_IDF_L1, d_vocab, vocab_bytes, d_desc, desc_stride, d_workspace,
                                             d_out + o["word"], d_out + o["node_of"], d_out + o["weight"], d_out + o["nodes"], d_out + o["bow_ids"],
                                             d_out + o["bow_vals"], d_out + o["n_words"]), self.h)

    def bow_transform(self, vocab_blob, desc, levelsup: int = 4):
        """xfh_bow_transform (host pointers, one frame) -> dict(word, node_of, weight, nodes (the node blob as bytes), bow_ids, bow_vals
        (both cut to n_words), n_words)"""
        b = np.ascontiguousarray(vocab_blob, np.uint8)
        d = np.ascontiguousarray(desc, np.float32)
        n = len(d)
        assert d.shape == (n, 64)
        word, node_of, ids = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        wt, vals = np.zeros(n, np.float64), np.zeros(n, np.float64)
        nodes = np.zeros(self.nodes_bytes(n), np.uint8); nw = np.zeros(1, np.int32)
        check(lib().xfh_bow_transform(self.h, n, int(levelsup), capi.BOWT_TF_IDF_L1, b.ctypes.data, b.nbytes, d.ctypes.data, word.ctypes.data, node_of.ctypes.data,
                                      wt.ctypes.data, nodes.ctypes.data, ids.ctypes.data, vals.ctypes.data, nw.ctypes.data), self.h)
        k = int(nw[0])
        return dict(word=word, node_of=node_of, weight=wt, nodes=nodes, bow_ids=ids[:k].copy(), bow_vals=vals[:k].copy(), n_words=k)

    # -- the keyframe database query: shared words, L1 score, candidates (xfh_bow_score / xfh_bowdb_query*) -----------------------------------
    BOWDB_TABLE = (("common", I32, ("B", "n")), ("score", F64, ("B", "n")), ("status", U8, ("B", "n")), ("list_slot", I32, ("B", "n")), ("list_acc", F32, ("B", "n")),
                   ("list_best", I32, ("B", "n")), ("cand_slot", I32, ("B", "n")), ("cand_acc", F32, ("B", "n")), ("header", I32, ("B", capi.BOWDB_HEADER_INTS)),
                   ("best_acc", F32, ("B",)))
    BOWDB_OUT = tuple((name, dt) for name, dt, shape in BOWDB_TABLE if shape == ("B", "n"))
    BOWDB_HEADER = ("n_listed", "max_common", "min_common", "n_scored", "n_candidates")

    @staticmethod
    def bow_score(ids1, vals1, ids2, vals2):
        """xfh_bow_score (host): L1Scoring::score(v1, v2) on two BowVectors in ascending word id -> (score, n_common, first_common)"""
        i1, v1 = np.ascontiguousarray(ids1, np.uint32), np.ascontiguousarray(vals1, np.float64)
        i2, v2 = np.ascontiguousarray(ids2, np.uint32), np.ascontiguousarray(vals2, np.float64)
        assert len(i1) == len(v1) and len(i2) == len(v2)
        sc, nc, fc = C.c_double(0), C.c_int(0), C.c_uint32(0)
        check(lib().xfh_bow_score(i1.ctypes.data if len(i1) else None, v1.ctypes.data if len(i1) else None, len(i1), i2.ctypes.data if len(i2) else None,
                                  v2.ctypes.data if len(i2) else None, len(i2), C.byref(sc), C.byref(nc), C.byref(fc)))
        return sc.value, nc.value, fc.value

    @staticmethod
    def bowdb_query_workspace_bytes(n_slots: int, B: int = 1) -> int:
        return int(lib().xfh_bowdb_query_workspace_bytes(n_slots, B))

    @staticmethod
    def bowdb_query_layout(B: int, n_slots: int, guard: int = 0):
        """byte offsets of the outputs of bowdb_query_device inside one buffer (and its size under "bytes"); guard as in fuse_search_layout.
        The workspace and d_state are buffers of their own."""
        return Layout.of(Context.BOWDB_TABLE, guard, B=B, n=n_slots)

    @staticmethod
    def bowdb_query_parse(raw: np.ndarray, lay, B: int, n_slots: int):
        """the bytes of an output buffer of bowdb_query_device -> one dict per query (the arrays at full length, the header fields as ints)"""
        a = lay.parse(raw)
        assert a["common"].shape == (B, n_slots)
        res = []
        for b in range(B):
            o = {k: v[b] for k, v in a.items()}
            o.update({k: int(o["header"][i]) for i, k in enumerate(Context.BOWDB_HEADER)})
            res.append(o)
        return res

    def bowdb_query_device(self, B: int, n_slots: int, form: int, d_q_ids, d_q_vals, d_q_n_words, q_stride: int, d_db_ids, d_db_vals, d_db_n_words,
                           db_stride: int, d_seq, d_neigh, nn: int, d_exclude, d_state, d_workspace, d_out, guard: int = 0):
        """xfh_bowdb_query_device on device pointers; asynchronous.  d_out: pointer to the outputs laid out as bowdb_query_layout(B, n_slots,
        guard) says; d_state [B][n_slots] floats is updated in place"""
        o = self.bowdb_query_layout(B, n_slots, guard)
        check(lib().xfh_bowdb_query_device(self.h, B, n_slots, int(form), d_q_ids, d_q_vals, d_q_n_words, q_stride, d_db_ids, d_db_vals, d_db_n_words, db_stride,
                                           d_seq, d_neigh, nn, d_exclude, d_state, d_workspace, d_out + o["common"], d_out + o["score"], d_out + o["status"],
                                           d_out + o["header"], d_out + o["best_acc"], d_out + o["list_slot"], d_out + o["list_acc"], d_out + o["list_best"],
                                           d_out + o["cand_slot"], d_out + o["cand_acc"]), self.h)

    def bowdb_query(self, form: int, q_ids, q_vals, db_ids, db_vals, db_n_words, neigh, state, seq=None, exclude=None):
        """xfh_bowdb_query (host pointers, one query).  db_ids / db_vals [n_slots][db_stride], neigh [n_slots][nn]; state: float32 [n_slots],
        updated IN PLACE.  -> dict as bowdb_query_parse gives it"""
        qi, qv = np.ascontiguousarray(q_ids, np.uint32), np.ascontiguousarray(q_vals, np.float64)
        di, dv, dn = np.ascontiguousarray(db_ids, np.uint32), np.ascontiguousarray(db_vals, np.float64), np.ascontiguousarray(db_n_words, np.int32)
        n, stride = di.shape
        ng = np.ascontiguousarray(neigh, np.int32)
        ng = ng.reshape(n, -1) if ng.size else ng.reshape(n, 0)                                 # nn = 0: no neighbours at all
        nn = ng.shape[1]
        sq = _opt(seq, np.uint32)
        ex = _opt(exclude, np.uint8)
        assert len(qi) == len(qv) and dv.shape == di.shape and len(dn) == n and state.dtype == np.float32 and state.flags.c_contiguous and len(state) == n
        o = {name: np.zeros(n, dt) for name, dt in self.BOWDB_OUT}
        hd, ba = np.zeros(capi.BOWDB_HEADER_INTS, np.int32), np.zeros(1, np.float32)
        p = lambda a: None if a is None or a.size == 0 else a.ctypes.data
        check(lib().xfh_bowdb_query(self.h, n, int(form), p(qi), p(qv), len(qi), di.ctypes.data, dv.ctypes.data, dn.ctypes.data, stride, p(sq), p(ng), nn, p(ex),
                                    state.ctypes.data, o["common"].ctypes.data, o["score"].ctypes.data, o["status"].ctypes.data, hd.ctypes.data, ba.ctypes.data,
                                    o["list_slot"].ctypes.data, o["list_acc"].ctypes.data, o["list_best"].ctypes.data, o["cand_slot"].ctypes.data,
                                    o["cand_acc"].ctypes.data), self.h)
        o.update({k: int(hd[i]) for i, k in enumerate(self.BOWDB_HEADER)})
        o["header"], o["best_acc"] = hd, ba[0]
        return o

    # -- SearchByProjection of map points with a claim: the Sim3 and relocalisation forms (xfh_map_project / xfh_map_projection_search*) ----
    MAPPROJ_TABLE = (("match_idx", I32, ("B", "nq")), ("best_dist", I32, ("B", "nq")), ("n_window", I32, ("B", "nq")), ("n_tested", I32, ("B", "nq")),
                     ("level", I32, ("B", "nq")), ("proj", F32, ("B", "nq", 3)), ("assigned", I32, ("B", "nt")), ("n_matches", I32, ("B",)), ("status", U8, ("B", "nq")))
    MAPPROJ_OUT_INT = _names(MAPPROJ_TABLE, "nq")

    @staticmethod
    def map_project(Tcw, Ow, cam, bounds, th: float, scale_factors, ratio_max, form: int, xyz, normals, distances):
        """xfh_map_project (host): the per-point arithmetic of the map-point SearchByProjection forms for one pose -> (uvr[n][3], level[n], status[n])"""
        T = np.ascontiguousarray(Tcw, np.float32).reshape(12); O = np.ascontiguousarray(Ow, np.float32).reshape(3)
        sf = np.ascontiguousarray(scale_factors, np.float32); rm = np.ascontiguousarray(ratio_max, np.float32)
        p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3); nr = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(distances, np.float32).reshape(-1, 3)
        n = len(p)
        assert len(nr) == n and len(d) == n and len(rm) >= len(sf) - 1
        uvr = np.zeros((max(n, 1), 3), np.float32); lv = np.zeros(max(n, 1), np.int32); st = np.zeros(max(n, 1), np.uint8)
        check(lib().xfh_map_project(T.ctypes.data, O.ctypes.data, C.byref(cam), C.byref(capi.GridBounds(*bounds)), float(th), sf.ctypes.data, rm.ctypes.data,
                                    len(sf), int(form), p.ctypes.data, nr.ctypes.data, d.ctypes.data, n, uvr.ctypes.data, lv.ctypes.data, st.ctypes.data))
        return uvr[:n], lv[:n], st[:n]

    @staticmethod
    def map_projection_search_workspace_bytes(nq: int, nt: int, B: int = 1) -> int:
        return int(lib().xfh_map_projection_search_workspace_bytes(nq, nt, B))

    @staticmethod
    def map_projection_search_layout(B: int, nq: int, nt: int, guard: int = 0):
        """byte offsets of the outputs of map_projection_search_device inside one buffer (and its size under "bytes"); guard as in
        fuse_search_layout.  The workspace is a buffer of its own (map_projection_search_workspace_bytes)."""
        return Layout.of(Context.MAPPROJ_TABLE, guard, B=B, nq=nq, nt=nt)

    def map_projection_search_device(self, form: int, B: int, nq: int, d_points, d_normals, d_distances, d_query_desc, d_query_flags, d_Tcw, d_Ow, cam, bounds,
                                     th: float, scale_factors, ratio_max, d_grids, d_targets, target_stride: int, target_shared: int, nt: int, d_workspace,
                                     d_out, d_taken=None, init_dist: int = 256, accept_max: float = 100.0, proj: bool = True, guard: int = 0):
        """xfh_map_projection_search_device on device pointers; asynchronous.  d_out: pointer to the outputs laid out as
        map_projection_search_layout(B, nq, nt, guard) says (proj = False: the proj block is left alone)"""
        o = self.map_projection_search_layout(B, nq, nt, guard)
        sf = np.ascontiguousarray(scale_factors, np.float32); rm = np.ascontiguousarray(ratio_max, np.float32)
        check(lib().xfh_map_projection_search_device(self.h, int(form), B, nq, d_points, d_normals, d_distances, d_query_desc, d_query_flags, d_Tcw, d_Ow,
                                                     C.byref(cam), C.byref(capi.GridBounds(*bounds)), float(th), sf.ctypes.data, rm.ctypes.data, len(sf), d_grids,
                                                     d_targets, target_stride, int(target_shared), nt, d_taken, int(init_dist), float(accept_max), d_workspace,
                                                     d_out + o["status"], *[d_out + o[k] for k in self.MAPPROJ_OUT_INT], d_out + o["proj"] if proj else None,
                                                     d_out + o["assigned"], d_out + o["n_matches"]), self.h)

    def map_projection_search(self, form: int, points, normals, distances, query_desc, query_flags, Tcw, Ow, cam, bounds, th: float, scale_factors, ratio_max,
                              kps, targets, taken=None, init_dist: int = 256, accept_max: float = 100.0):
        """xfh_map_projection_search (host pointers, one problem) -> dict(status, match_idx, best_dist, n_window, n_tested, level, proj, assigned, n_matches)"""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3); nr = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(distances, np.float32).reshape(-1, 3); q = np.ascontiguousarray(query_desc, np.float32)
        fl = np.ascontiguousarray(query_flags, np.uint8); k = np.ascontiguousarray(kps, KP_DTYPE); tg = np.ascontiguousarray(targets, np.float32)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(12); O = np.ascontiguousarray(Ow, np.float32).reshape(3)
        sf = np.ascontiguousarray(scale_factors, np.float32); rm = np.ascontiguousarray(ratio_max, np.float32)
        nq, nt = len(p), len(k)
        tk = _opt(taken, np.uint8)
        assert len(nr) == nq and len(d) == nq and len(q) == nq and len(fl) == nq and len(tg) == nt and len(rm) >= len(sf) - 1 and (tk is None or len(tk) == nt)
        st = np.zeros(nq, np.uint8); oi = [np.zeros(nq, np.int32) for _ in range(5)]; proj = np.zeros((nq, 3), np.float32)
        asg = np.zeros(nt, np.int32); nm = np.zeros(1, np.int32)
        check(lib().xfh_map_projection_search(self.h, int(form), nq, p.ctypes.data, nr.ctypes.data, d.ctypes.data, q.ctypes.data, fl.ctypes.data, T.ctypes.data,
                                              O.ctypes.data, C.byref(cam), C.byref(capi.GridBounds(*bounds)), float(th), sf.ctypes.data, rm.ctypes.data, len(sf),
                                              k.ctypes.data, tg.ctypes.data, nt, _ptr(tk), int(init_dist), float(accept_max),
                                              st.ctypes.data, *[o.ctypes.data for o in oi], proj.ctypes.data, asg.ctypes.data, nm.ctypes.data), self.h)
        r = dict(zip(self.MAPPROJ_OUT_INT, oi))
        r.update(status=st, proj=proj, assigned=asg, n_matches=int(nm[0]))
        return r

    # -- SearchBySim3: two keyframes' map points into each other (xfh_sim3_project / xfh_sim3_search*) ---------------------------
    SIM3_SIDE_TABLE = (("match", I32, ("B", "n")), ("best_dist", I32, ("B", "n")), ("n_window", I32, ("B", "n")), ("n_tested", I32, ("B", "n")), ("level", I32, ("B", "n")),
                       ("proj", F32, ("B", "n", 3)), ("status", U8, ("B", "n")))
    SIM3_OUT_INT = _names(SIM3_SIDE_TABLE, "n")

    @staticmethod
    def sim3_project(Tqw, M, cam, bounds, th: float, scale_factors, ratio_max, xyz, distances):
        """xfh_sim3_project (host): the per-point arithmetic of ORBmatcher::SearchBySim3 for one pose and one Sim3 -> (uvr[n][3], level[n], status[n])"""
        T = np.ascontiguousarray(Tqw, np.float32).reshape(12); Mm = np.ascontiguousarray(M, np.float32).reshape(12)
        sf = np.ascontiguousarray(scale_factors, np.float32); rm = np.ascontiguousarray(ratio_max, np.float32)
        p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3); d = np.ascontiguousarray(distances, np.float32).reshape(-1, 3)
        n = len(p)
        assert len(d) == n and len(rm) >= len(sf) - 1
        uvr = np.zeros((max(n, 1), 3), np.float32); lv = np.zeros(max(n, 1), np.int32); st = np.zeros(max(n, 1), np.uint8)
        check(lib().xfh_sim3_project(T.ctypes.data, Mm.ctypes.data, C.byref(cam), C.byref(capi.GridBounds(*bounds)), float(th), sf.ctypes.data, rm.ctypes.data,
                                     len(sf), p.ctypes.data, d.ctypes.data, n, uvr.ctypes.data, lv.ctypes.data, st.ctypes.data))
        return uvr[:n], lv[:n], st[:n]

    @staticmethod
    def sim3_search_layout(B: int, n1: int, n2: int, guard: int = 0):
        """byte offsets of the outputs of sim3_search_device inside one buffer (and its size under "bytes"): the per-side arrays under
        "match1", "status2", ..., then "match12" and "n_found"; guard as in fuse_search_layout"""
        side = lambda s: tuple((name + s, dt, tuple(d + s if d == "n" else d for d in shape)) for name, dt, shape in Context.SIM3_SIDE_TABLE)
        return Layout.of(side("1") + side("2") + (("match12", I32, ("B", "n1")), ("n_found", I32, ("B",))), guard, B=B, n1=n1, n2=n2)

    @staticmethod
    def sim3_side(n: int, grid, desc, desc_stride: int, points, dist, mp_desc, flags, Tw, out, lay, s: str, proj: bool = True, kps=None):
        """one xfh_sim3_side from pointers (ints); its outputs lie at out + lay[name + s] (sim3_search_layout)"""
        return capi.Sim3Side(n, grid, kps, desc, desc_stride, points, dist, mp_desc, flags, Tw, out + lay["status" + s],
                             *[out + lay[k + s] for k in Context.SIM3_OUT_INT], out + lay["proj" + s] if proj else None)

    def sim3_search_device(self, B: int, side1_shared: int, side1, side2, d_M21, d_M12, cam, bounds, th: float, scale_factors, ratio_max, d_match12,
                           d_n_found, th_high: int = 1000):
        """xfh_sim3_search_device on device pointers; asynchronous.  side1 / side2: capi.Sim3Side (Context.sim3_side)"""
        sf = np.ascontiguousarray(scale_factors, np.float32); rm = np.ascontiguousarray(ratio_max, np.float32)
        check(lib().xfh_sim3_search_device(self.h, B, int(side1_shared), C.byref(side1), C.byref(side2), d_M21, d_M12, C.byref(cam),
                                           C.byref(capi.GridBounds(*bounds)), float(th), sf.ctypes.data, rm.ctypes.data, len(sf), int(th_high), d_match12,
                                           d_n_found), self.h)

    def sim3_search(self, side1, side2, M21, M12, cam, bounds, th: float, scale_factors, ratio_max, th_high: int = 1000):
        """xfh_sim3_search (host pointers, one pair).  side = dict(kps, desc, points, dist, mp_desc, flags, Tw) -> dict(match12, n_found, and per
        side s in "12": status, match, best_dist, n_window, n_tested, level, proj under name + s)"""
        sf = np.ascontiguousarray(scale_factors, np.float32); rm = np.ascontiguousarray(ratio_max, np.float32)
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        keep, sides, r = [], [], {}
        for s, sd in (("1", side1), ("2", side2)):
            k = np.ascontiguousarray(sd["kps"], KP_DTYPE); n = len(k)
            a = [f32(sd["desc"]), f32(sd["points"]).reshape(-1, 3), f32(sd["dist"]).reshape(-1, 3), f32(sd["mp_desc"]), np.ascontiguousarray(sd["flags"], np.uint8),
                 f32(sd["Tw"]).reshape(12)]
            assert all(len(x) == n for x in a[:5]) and len(rm) >= len(sf) - 1
            st = np.zeros(n, np.uint8); oi = [np.zeros(n, np.int32) for _ in range(5)]; proj = np.zeros((n, 3), np.float32)
            keep += [k, a, st, oi, proj]
            sides.append(capi.Sim3Side(n, None, k.ctypes.data, a[0].ctypes.data, 0, *[x.ctypes.data for x in a[1:]], st.ctypes.data,
                                       *[o.ctypes.data for o in oi], proj.ctypes.data))
            r.update({name + s: o for name, o in zip(self.SIM3_OUT_INT, oi)})
            r["status" + s] = st; r["proj" + s] = proj
        m21, m12 = f32(M21).reshape(12), f32(M12).reshape(12)
        match12 = np.zeros(sides[0].n, np.int32); nf = np.zeros(1, np.int32)
        check(lib().xfh_sim3_search(self.h, C.byref(sides[0]), C.byref(sides[1]), m21.ctypes.data, m12.ctypes.data, C.byref(cam), C.byref(capi.GridBounds(*bounds)),
                                    float(th), sf.ctypes.data, rm.ctypes.data, len(sf), int(th_high), match12.ctypes.data, nf.ctypes.data), self.h)
        r.update(match12=match12, n_found=int(nf[0]))
        return r

    # -- timing ---------------------------------------------------------------------------
    # -- SearchForInitialization with the reference's retraction order (xfh_init_accept / xfh_init_search*) --------------------------------
    INIT_TABLE = (("claim_idx", I32, ("B", "nq")), ("matches12", I32, ("B", "nq")), ("best_dist", I32, ("B", "nq")), ("second_dist", I32, ("B", "nq")),
                  ("n_window", I32, ("B", "nq")), ("n_tested", I32, ("B", "nq")), ("matches21", I32, ("B", "nt")), ("matched_distance", I32, ("B", "nt")),
                  ("n_matches", I32, ("B",)), ("status", U8, ("B", "nq")), ("prev_out", F32, ("B", "nq", 2)))
    INIT_OUT_Q, INIT_OUT_T = _names(INIT_TABLE, "nq"), _names(INIT_TABLE, "nt")

    @staticmethod
    def init_accept(best: int, second: int, th_low: int, nn_ratio: float) -> bool:
        """xfh_init_accept (host): the acceptance line of SearchForInitialization"""
        return bool(lib().xfh_init_accept(int(best), int(second), int(th_low), float(nn_ratio)))

    @staticmethod
    def init_search_workspace_bytes(nq: int, nt: int, B: int = 1) -> int:
        return int(lib().xfh_init_search_workspace_bytes(nq, nt, B))

    @staticmethod
    def init_search_layout(B: int, nq: int, nt: int, guard: int = 0):
        """byte offsets of the outputs of init_search_device inside one buffer (its size under "bytes", the library's list length under
        "K"); guard as in search_projection_layout.  The workspace is a buffer of its own (init_search_workspace_bytes)."""
        o = Layout.of(Context.INIT_TABLE, guard, B=B, nq=nq, nt=nt)
        o["K"] = int(lib().xfh_init_list_entries())
        return o

    def init_search_device(self, B: int, nq: int, d_query_desc, d_prev_matched, d_grids, d_targets, target_stride: int, nt: int, d_workspace, d_out,
                           window: float = 100.0, d_query_flags=None, d_target_xy=None, d_prev_out=None, th_low: int = 100, nn_ratio: float = 0.9, guard: int = 0):
        """xfh_init_search_device on device pointers; asynchronous.  d_out: pointer to the outputs laid out as init_search_layout(B, nq, nt,
        guard) says.  d_target_xy given: prev_out is written, into d_prev_out if that is given (it may be d_prev_matched) or into the layout's
        own array"""
        o = self.init_search_layout(B, nq, nt, guard)
        po = None if d_target_xy is None else (d_prev_out if d_prev_out is not None else d_out + o["prev_out"])
        check(lib().xfh_init_search_device(self.h, B, nq, d_query_desc, d_prev_matched, d_query_flags, float(window), d_grids, d_targets, target_stride,
                                           d_target_xy, nt, int(th_low), float(nn_ratio), d_workspace, d_out + o["status"],
                                           *[d_out + o[k] for k in self.INIT_OUT_Q + self.INIT_OUT_T], d_out + o["n_matches"], po), self.h)

    def init_search(self, query_desc, prev_matched, kps, bounds, targets, window: float = 100.0, query_flags=None, th_low: int = 100, nn_ratio: float = 0.9,
                    in_place: bool = False):
        """xfh_init_search (host pointers, one problem) -> dict(status, claim_idx, matches12, best_dist, second_dist, n_window, n_tested,
        matches21, matched_distance, n_matches, prev_out); in_place: prev_out is the (copied) prev_matched array itself"""
        q = np.ascontiguousarray(query_desc, np.float32); pm = np.array(prev_matched, np.float32, order="C").reshape(-1, 2)
        k = np.ascontiguousarray(kps, KP_DTYPE); tg = np.ascontiguousarray(targets, np.float32)
        fl = _opt(query_flags, np.uint8)
        nq, nt = len(q), len(k)
        assert len(pm) == nq and len(tg) == nt and (fl is None or len(fl) == nq)
        st = np.zeros(nq, np.uint8); oq = [np.zeros(nq, np.int32) for _ in self.INIT_OUT_Q]; ot = [np.zeros(nt, np.int32) for _ in self.INIT_OUT_T]
        nm = np.zeros(1, np.int32); po = pm if in_place else np.zeros((nq, 2), np.float32)
        check(lib().xfh_init_search(self.h, nq, q.ctypes.data, pm.ctypes.data, _ptr(fl), float(window), k.ctypes.data,
                                    C.byref(capi.GridBounds(*bounds)), tg.ctypes.data, nt, int(th_low), float(nn_ratio), st.ctypes.data,
                                    *[o.ctypes.data for o in oq + ot], nm.ctypes.data, po.ctypes.data), self.h)
        r = dict(zip(self.INIT_OUT_Q + self.INIT_OUT_T, oq + ot))
        r.update(status=st, n_matches=int(nm[0]), prev_out=po)
        return r

    # -- PoseOptimization --------------------------------------------------------------------
    POSE_HEADER = ("n_initial", "n_bad", "ret", "rounds", "iterations", "trials", "rejected", "ldlt_failures")
    POSE_TABLE = (("Tcw_out", F32, ("B", 12)), ("outlier", U8, ("B", "nt")), ("chi2", F32, ("B", "nt")), ("header", I32, ("B", 8)), ("final_chi2", F64, ("B",)))

    @staticmethod
    def pose_optimize_layout(B: int, nt: int, guard: int = 0):
        """the outputs of pose_optimize_device inside one buffer, in the order the call takes them; guard as in fuse_search_layout"""
        return Layout.of(Context.POSE_TABLE, guard, B=B, nt=nt)

    @staticmethod
    def pose_optimize_workspace_bytes(nt: int, B: int = 1) -> int:
        return int(lib().xfh_pose_optimize_workspace_bytes(nt, B))

    def pose_optimize_device(self, B: int, nt: int, nq: int, d_Tcw, cam, d_xy_un, d_uright, d_assigned, d_points, d_workspace, d_Tcw_out, d_outlier, d_chi2,
                             d_header, d_final_chi2, inv_sigma2: float = 1.0):
        """xfh_pose_optimize_device on device pointers; asynchronous.  d_uright may be None (all edges mono), d_Tcw_out may be d_Tcw"""
        check(lib().xfh_pose_optimize_device(self.h, B, nt, nq, d_Tcw, C.byref(cam), d_xy_un, d_uright, d_assigned, d_points, float(inv_sigma2), d_workspace,
                                             d_Tcw_out, d_outlier, d_chi2, d_header, d_final_chi2), self.h)

    def pose_optimize(self, Tcw, cam, xy_un, uright, assigned, points, inv_sigma2: float = 1.0):
        """xfh_pose_optimize (host pointers, one frame) -> dict(ret, Tcw, outlier, chi2, header, final_chi2); ret is the reference's return value"""
        T = np.ascontiguousarray(Tcw, np.float32).reshape(12); xy = np.ascontiguousarray(xy_un, np.float32).reshape(-1, 2)
        a = np.ascontiguousarray(assigned, np.int32); p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        ur = _opt(uright, np.float32)
        nt = len(a)
        assert len(xy) == nt and (ur is None or len(ur) == nt)
        To, ol, c2, hd, fc = np.zeros(12, np.float32), np.zeros(nt, np.uint8), np.zeros(nt, np.float32), np.zeros(8, np.int32), np.zeros(1, np.float64)
        check(lib().xfh_pose_optimize(self.h, nt, len(p), T.ctypes.data, C.byref(cam), xy.ctypes.data, _ptr(ur), a.ctypes.data,
                                      p.ctypes.data, float(inv_sigma2), To.ctypes.data, ol.ctypes.data, c2.ctypes.data, hd.ctypes.data, fc.ctypes.data), self.h)
        return dict(ret=int(hd[2]), Tcw=To.reshape(3, 4), outlier=ol, chi2=c2, header=dict(zip(self.POSE_HEADER, hd.tolist())), final_chi2=float(fc[0]))

    # -- OptimizeSim3 between the two Sim3 projection searches of loop detection (xfh_sim3_optimize*) ---------------------------
    SIM3_OPT_HEADER = ("n_corr", "n_in_kf2", "n_out_kf2", "n_bad", "n_bad_out_kf2", "n_more", "ret", "rounds", "iterations", "trials", "rejected", "ldlt_failures")

    SIM3_OPT_TABLE = (("assigned_out", I32, ("B", "n1")), ("status", U8, ("B", "n1")), ("chi2", F32, ("B", "n1", 2)), ("state", F64, ("B", 8)), ("S12_out", F32, ("B", 13)),
                      ("Tcw", F32, ("B", 12)), ("Ow", F32, ("B", 3)), ("header", I32, ("B", 16)), ("final_chi2", F64, ("B",)))

    @staticmethod
    def sim3_optimize_layout(B: int, n1: int, guard: int = 0):
        """the outputs of sim3_optimize_device inside one buffer, in the order the call takes them (S12_out with stride 13); guard as in
        fuse_search_layout"""
        return Layout.of(Context.SIM3_OPT_TABLE, guard, B=B, n1=n1)

    @staticmethod
    def sim3_optimize_workspace_bytes(n1: int, B: int = 1) -> int:
        return int(lib().xfh_sim3_optimize_workspace_bytes(n1, B))

    def sim3_optimize_device(self, B: int, n1: int, M1: int, nq: int, n2: int, side1_shared: bool, side1, side2, d_S12, S12_stride: int, d_Tmw, cam1, cam2,
                             d_workspace, d_assigned_out, d_pair_status, d_chi2, d_state, d_S12_out, S12_out_stride: int, d_Tcw, d_Ow, d_header, d_final_chi2,
                             th2: float = 10.0, fix_scale: bool = False, all_points: bool = False, inv_sigma2_1: float = 1.0, inv_sigma2_2: float = 1.0):
        """xfh_sim3_optimize_device on device pointers; asynchronous.  side1: (d_T1w, d_xy_un1, d_point1, d_points1); side2: (d_assigned, d_points2,
        d_flags2, d_index2, d_xy_un2, d_T2w).  d_S12 with stride XFH_SIM3_SOLVE_FLOATS is xfh_sim3_solve_device's d_floats + 12; d_assigned_out may
        be d_assigned, d_S12_out may be d_S12; d_Tmw (and with it d_Tcw, d_Ow) may be None"""
        check(lib().xfh_sim3_optimize_device(self.h, B, n1, M1, nq, n2, 1 if side1_shared else 0, *side1, *side2, d_S12, S12_stride, d_Tmw, C.byref(cam1),
                                             C.byref(cam2), float(th2), 1 if fix_scale else 0, 1 if all_points else 0, float(inv_sigma2_1), float(inv_sigma2_2),
                                             d_workspace, d_assigned_out, d_pair_status, d_chi2, d_state, d_S12_out, S12_out_stride, d_Tcw, d_Ow, d_header,
                                             d_final_chi2), self.h)

    def sim3_optimize(self, T1w, xy_un1, point1, points1, assigned, points2, flags2, index2, xy_un2, T2w, S12, cam1, cam2, Tmw=None, th2: float = 10.0,
                      fix_scale: bool = False, all_points: bool = False, inv_sigma2_1: float = 1.0, inv_sigma2_2: float = 1.0):
        """xfh_sim3_optimize (host pointers, one problem) -> dict(ret, assigned, status, chi2, state, S12, Tcw, Ow, header, final_chi2); ret is the
        reference's return value, assigned is vpMatches1 with -1 where a match was removed"""
        f32 = lambda a, shape: np.ascontiguousarray(a, np.float32).reshape(shape)
        i32 = lambda a: np.ascontiguousarray(a, np.int32).reshape(-1)
        ins = [f32(T1w, 12), f32(xy_un1, (-1, 2)), i32(point1), f32(points1, (-1, 3)), i32(assigned), f32(points2, (-1, 3)),
               np.ascontiguousarray(flags2, np.uint8).reshape(-1), i32(index2), f32(xy_un2, (-1, 2)), f32(T2w, 12), f32(S12, 13)]
        n1, M1, nq, n2 = len(ins[4]), len(ins[3]), len(ins[5]), len(ins[8])
        assert len(ins[1]) == n1 and len(ins[2]) == n1 and len(ins[6]) == nq and len(ins[7]) == nq
        tm = None if Tmw is None else f32(Tmw, 12)
        ao, st, c2, sv, so = np.zeros(n1, np.int32), np.zeros(n1, np.uint8), np.zeros((n1, 2), np.float32), np.zeros(8, np.float64), np.zeros(13, np.float32)
        To, Ow, hd, fc = np.zeros(12, np.float32), np.zeros(3, np.float32), np.zeros(16, np.int32), np.zeros(1, np.float64)
        check(lib().xfh_sim3_optimize(self.h, n1, M1, nq, n2, *[a.ctypes.data for a in ins], _ptr(tm), C.byref(cam1), C.byref(cam2),
                                      float(th2), 1 if fix_scale else 0, 1 if all_points else 0, float(inv_sigma2_1), float(inv_sigma2_2), ao.ctypes.data,
                                      st.ctypes.data, c2.ctypes.data, sv.ctypes.data, so.ctypes.data, None if tm is None else To.ctypes.data,
                                      None if tm is None else Ow.ctypes.data, hd.ctypes.data, fc.ctypes.data), self.h)
        return dict(ret=int(hd[6]), assigned=ao, status=st, chi2=c2, state=sv, S12=so, Tcw=None if tm is None else To.reshape(3, 4), Ow=None if tm is None else Ow,
                    header=dict(zip(self.SIM3_OPT_HEADER, hd.tolist())), final_chi2=float(fc[0]))

    # -- CreateNewMapPoints: triangulation of the matched pairs (xfh_triangulate*) ----------------------------------------------
    TRIANG_HEADER = ("matched", "tri_attempts", "stereo_attempts", "accepted", "new", "new_stereo", "superseded", "reserved")
    TRIANG_TABLE = (("status", U8, ("B", "n1")), ("kind", U8, ("B", "n1")), ("xyz", F32, ("B", "n1", 3)), ("header", I32, ("B", 8)), ("winner", I32, ("n1",)),
                    ("new_idx1", I32, ("n1",)), ("new_b", I32, ("n1",)), ("new_idx2", I32, ("n1",)), ("new_xyz", F32, ("n1", 3)), ("new_normal", F32, ("n1", 3)),
                    ("new_dist", F32, ("n1", 3)), ("n_new", I32, (1,)))
    TRIANG_CLAIM_OUT = _names(TRIANG_TABLE)[4:]                              # the claim's arrays: one set for the whole call, not one per neighbour

    @staticmethod
    def triangulate_layout(B: int, n1: int, guard: int = 0):
        """byte offsets of the outputs of triangulate_device inside one buffer (and its size under "bytes"); guard as in fuse_search_layout"""
        return Layout.of(Context.TRIANG_TABLE, guard, B=B, n1=n1)

    @staticmethod
    def triangulate_parse(raw: np.ndarray, lay, B: int, n1: int, claim: bool):
        """the bytes of a buffer laid out by triangulate_layout -> dict of arrays: without the claim its arrays are left out, with it n_new is an int"""
        r = {k: v for k, v in lay.parse(raw).items() if claim or k not in Context.TRIANG_CLAIM_OUT}
        assert r["status"].shape == (B, n1)
        if claim:
            r["n_new"] = int(r["n_new"][0])
        return r

    def triangulate_device(self, B: int, n1: int, n2: int, side1_shared: bool, cam, side1, side2, d_match12, d_out, sigma2: float = 1.0,
                           ratio_factor: float = 1.8, scale_last: float = 1.0, far_th: float = 0.0, inertial: bool = False, claim: bool = False, guard: int = 0):
        """xfh_triangulate_device on device pointers; asynchronous.  side1 / side2: (d_xy, d_xy_raw or None, d_uright or None, d_depth or None, d_Tcw, d_Ow);
        d_out: pointer to the outputs laid out as triangulate_layout(B, n1, guard) says"""
        o = self.triangulate_layout(B, n1, guard)
        flags = (capi.TRIANG_INERTIAL if inertial else 0) | (capi.TRIANG_CLAIM if claim else 0)
        co = [d_out + o[k] if claim else None for k in self.TRIANG_CLAIM_OUT]
        check(lib().xfh_triangulate_device(self.h, B, n1, n2, 1 if side1_shared else 0, flags, C.byref(cam), float(sigma2), float(ratio_factor), float(scale_last),
                                           float(far_th), *side1, *side2, d_match12, d_out + o["status"], d_out + o["kind"], d_out + o["xyz"], d_out + o["header"],
                                           *co), self.h)

    @staticmethod
    def _triang_side(k, B=None):
        """dict(xy, xy_raw (optional), ur, depth, Tcw, Ow) of one keyframe, or a list of B of them -> contiguous float32 arrays (None where absent)"""
        ks = [k] if B is None else list(k)
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        cat = lambda key: None if ks[0].get(key) is None else f32(np.concatenate([np.asarray(q[key], np.float32).reshape(len(q["xy"]), -1) for q in ks]))
        return [cat("xy"), cat("xy_raw"), cat("ur"), cat("depth") if ks[0].get("ur") is not None else None,
                f32(np.stack([np.asarray(q["Tcw"], np.float32).reshape(12) for q in ks])), f32(np.stack([np.asarray(q["Ow"], np.float32).reshape(3) for q in ks]))]

    def triangulate(self, cam, k1, k2s, match12, sigma2: float = 1.0, ratio_factor: float = 1.8, scale_last: float = 1.0, far_th: float = 0.0,
                    inertial: bool = False, claim: bool = True):
        """xfh_triangulate (host pointers): KF1 = k1 against the neighbours k2s (dicts with xy, xy_raw (optional), ur, depth, Tcw, Ow), match12 [B][n1]
        -> dict(status, kind, xyz, header and, with the claim, winner, new_idx1, new_b, new_idx2, new_xyz, new_normal, new_dist, n_new)"""
        B, n1, n2 = len(k2s), len(k1["xy"]), len(k2s[0]["xy"])
        s1, s2 = self._triang_side(k1), self._triang_side(k2s, B)
        m = np.ascontiguousarray(match12, np.int32).reshape(B, n1)
        st, kd, xyz, hd = np.zeros((B, n1), np.uint8), np.zeros((B, n1), np.uint8), np.zeros((B, n1, 3), np.float32), np.zeros((B, 8), np.int32)
        co = [np.zeros(n1, np.int32) for _ in range(4)] + [np.zeros((n1, 3), np.float32) for _ in range(3)] + [np.zeros(1, np.int32)]
        flags = (capi.TRIANG_INERTIAL if inertial else 0) | (capi.TRIANG_CLAIM if claim else 0)
        check(lib().xfh_triangulate(self.h, B, n1, n2, flags, C.byref(cam), float(sigma2), float(ratio_factor), float(scale_last), float(far_th),
                                    *[_ptr(a) for a in s1], *[_ptr(a) for a in s2], _ptr(m), _ptr(st), _ptr(kd), _ptr(xyz), _ptr(hd),
                                    *[_ptr(a) if claim else None for a in co]), self.h)
        r = dict(status=st, kind=kd, xyz=xyz, header=hd)
        if claim:
            r.update(zip(self.TRIANG_CLAIM_OUT, co)); r["n_new"] = int(co[7][0])
        return r

    @staticmethod
    def triangulate_pair(cam, o1, o2, sigma2: float = 1.0, ratio_factor: float = 1.8, scale_last: float = 1.0, far_th: float = 0.0, inertial: bool = False):
        """xfh_triangulate_pair: o1 / o2 = dict(xy, xy_raw (optional), ur, depth, Tcw, Ow) of ONE keypoint each
        -> dict(status, kind, x3D, normal, dist, x3Dh)"""
        f32 = lambda a: np.ascontiguousarray(a, np.float32).ravel()
        a = []
        for o in (o1, o2):
            raw = o.get("xy_raw")
            a += [f32(o["xy"]), None if raw is None else f32(raw), float(o["ur"]), float(o["depth"]), f32(o["Tcw"]), f32(o["Ow"])]
        ptr = lambda v: None if v is None else (v.ctypes.data if isinstance(v, np.ndarray) else v)
        st, kd = C.c_int(0), C.c_int(0)
        X, nrm, dst, xh = np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(4, np.float64)
        check(lib().xfh_triangulate_pair(C.byref(cam), capi.TRIANG_INERTIAL if inertial else 0, float(sigma2), float(ratio_factor), float(scale_last), float(far_th),
                                         *[ptr(v) for v in a], C.byref(st), C.byref(kd), ptr(X), ptr(nrm), ptr(dst), ptr(xh)))
        return dict(status=st.value, kind=kd.value, x3D=X, normal=nrm, dist=dst, x3Dh=xh)

    # -- MonocularInitialization: TwoViewReconstruction::Reconstruct (xfh_two_view*) -------------------------------------------------------
    TWO_VIEW_HEADER = ("N", "status", "model", "win_h", "win_f", "ngood0", "ngood1", "ngood2", "ngood3", "ngood4", "ngood5", "ngood6", "ngood7", "chosen",
                       "inliers_h", "inliers_f", "n_tri", "n_hyp", "n_matches_out")
    TWO_VIEW_TABLE = (("header", I32, ("B", capi.TWO_VIEW_HEADER_INTS)), ("floats", F32, ("B", capi.TWO_VIEW_FLOATS)), ("inl_h", U8, ("B", "n1")), ("inl_f", U8, ("B", "n1")),
                      ("tri", U8, ("B", "n1")), ("p3d", F32, ("B", "n1", 3)), ("matches_out", I32, ("B", "n1")))
    TWO_VIEW_OUT = _names(TWO_VIEW_TABLE)

    @staticmethod
    def two_view_cos(min_parallax_deg: float = 1.0) -> float:
        """the double the calls compare the parallax cosine with: cos(minParallax * pi / 180)"""
        return float(np.cos(float(min_parallax_deg) * np.pi / 180.0))

    @staticmethod
    def two_view_layout(B: int, n1: int, guard: int = 0):
        """byte offsets of the outputs of two_view_device inside one buffer (and its size under "bytes"); guard as in fuse_search_layout"""
        return Layout.of(Context.TWO_VIEW_TABLE, guard, B=B, n1=n1)

    @staticmethod
    def two_view_parse(raw: np.ndarray, lay, B: int, n1: int):
        """lay.parse(raw) under the name and arguments that callers of the hand-written layouts use"""
        return lay.parse(raw)

    def two_view_device(self, B: int, n1: int, n2: int, cam, d_xy1, d_xy2, d_matches12, d_draws, draws_stride: int, iters: int, rand_max: int, d_workspace,
                        d_out, sigma: float = 1.0, min_parallax_cos: float | None = None, min_triangulated: int = 50, guard: int = 0):
        """xfh_two_view_device on device pointers; asynchronous.  d_out: the outputs laid out as two_view_layout(B, n1, guard) says; d_workspace:
        xfh_two_view_workspace_bytes(n1, n2, iters, B) bytes"""
        o = self.two_view_layout(B, n1, guard)
        mpc = self.two_view_cos() if min_parallax_cos is None else float(min_parallax_cos)
        check(lib().xfh_two_view_device(self.h, B, n1, n2, d_xy1, d_xy2, d_matches12, C.byref(cam), float(sigma), iters, d_draws, draws_stride, rand_max, mpc,
                                        int(min_triangulated), d_workspace, *[d_out + o[k] for k in self.TWO_VIEW_OUT]), self.h)

    @staticmethod
    def _two_view_arrays(xy1, xy2, matches12, draws, prior=None):
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        m = np.ascontiguousarray(matches12, np.int32)
        B = 1 if m.ndim == 1 else m.shape[0]
        n1 = m.shape[-1]
        x1, x2 = f32(xy1).reshape(B, n1, 2), f32(xy2).reshape(B, -1, 2)
        d = np.ascontiguousarray(draws, np.int32)
        out = Context.two_view_layout(B, n1).zeros()
        out["matches_out"] = m.reshape(B, n1).copy()
        return B, n1, x2.shape[1], x1, x2, m, d, _with_prior(out, prior)

    @staticmethod
    def two_view_host(cam, xy1, xy2, matches12, draws, rand_max: int, sigma: float = 1.0, min_parallax_cos: float | None = None, min_triangulated: int = 50,
                      prior=None):
        """xfh_two_view_host: the whole rule on one host thread, no ctx.  matches12 [n1] or [B][n1]; draws [iters][8] shared, or [B][iters][8]
        -> dict(header, floats, inl_h, inl_f, tri, p3d, matches_out), each with a leading B"""
        B, n1, n2, x1, x2, m, d, out = Context._two_view_arrays(xy1, xy2, matches12, draws, prior)
        iters = d.shape[-2]
        stride = 0 if d.ndim == 2 else iters * 8
        ws = np.zeros(lib().xfh_two_view_workspace_bytes(n1, n2, iters, B) + 16, np.uint8)
        wp = (ws.ctypes.data + 15) & ~15
        mpc = Context.two_view_cos() if min_parallax_cos is None else float(min_parallax_cos)
        check(lib().xfh_two_view_host(B, n1, n2, x1.ctypes.data, x2.ctypes.data, m.ctypes.data, C.byref(cam), float(sigma), iters, d.ctypes.data, stride, rand_max,
                                      mpc, int(min_triangulated), wp, *[out[k].ctypes.data for k in Context.TWO_VIEW_OUT]))
        return out

    def two_view(self, cam, xy1, xy2, matches12, draws, rand_max: int, sigma: float = 1.0, min_parallax_cos: float | None = None, min_triangulated: int = 50,
                 prior=None):
        """xfh_two_view (host pointers, one problem) -> the dict of two_view_host with B = 1"""
        B, n1, n2, x1, x2, m, d, out = self._two_view_arrays(xy1, xy2, matches12, draws, prior)
        assert B == 1 and d.ndim == 2
        mpc = self.two_view_cos() if min_parallax_cos is None else float(min_parallax_cos)
        check(lib().xfh_two_view(self.h, n1, n2, x1.ctypes.data, x2.ctypes.data, m.ctypes.data, C.byref(cam), float(sigma), d.shape[0], d.ctypes.data, rand_max,
                                 mpc, int(min_triangulated), *[out[k].ctypes.data for k in self.TWO_VIEW_OUT]), self.h)
        return out

    @staticmethod
    def two_view_set(draws8, rand_max: int, N: int):
        d, s = np.ascontiguousarray(draws8, np.int32), np.zeros(8, np.int32)
        check(lib().xfh_two_view_set(d.ctypes.data, rand_max, N, s.ctypes.data))
        return s

    @staticmethod
    def two_view_fit(model: int, xy1n, xy2n):
        a, b, M = np.ascontiguousarray(xy1n, np.float32), np.ascontiguousarray(xy2n, np.float32), np.zeros(9, np.float32)
        check(lib().xfh_two_view_fit(model, a.ctypes.data, b.ctypes.data, M.ctypes.data))
        return M

    @staticmethod
    def two_view_score(model: int, M, sigma: float, xy1, xy2):
        """-> (chi2 [2], inlier, share of the score) of one match"""
        M, a, b = np.ascontiguousarray(M, np.float32), np.ascontiguousarray(xy1, np.float32), np.ascontiguousarray(xy2, np.float32)
        chi, inl, term = np.zeros(2, np.float32), C.c_int(0), C.c_float(0.0)
        check(lib().xfh_two_view_score(model, M.ctypes.data, float(sigma), a.ctypes.data, b.ctypes.data, chi.ctypes.data, C.byref(inl), C.byref(term)))
        return chi, inl.value, np.float32(term.value)

    @staticmethod
    def two_view_check_rt(cam, T21, sigma: float, xy1, xy2):
        """-> (verdict, cosine, p3d [3]) of one pair under T21 [3][4]"""
        T, a, b = np.ascontiguousarray(T21, np.float32), np.ascontiguousarray(xy1, np.float32), np.ascontiguousarray(xy2, np.float32)
        v, c, p = C.c_int(0), C.c_float(0.0), np.zeros(3, np.float32)
        check(lib().xfh_two_view_check_rt(C.byref(cam), T.ctypes.data, float(sigma), a.ctypes.data, b.ctypes.data, C.byref(v), C.byref(c), p.ctypes.data))
        return v.value, np.float32(c.value), p

    # -- LoopClosing::DetectCommonRegionsFromBoW: the merge of the BoW match lists and Sim3Solver (xfh_sim3_merge_matches*, xfh_sim3_solve*) ------------
    SIM3_SOLVE_HEADER = ("N", "status", "its", "winner", "n_inliers", "best", "best_count", "consumed")
    SIM3_SOLVE_TABLE = (("header", I32, ("B", capi.SIM3_SOLVE_HEADER_INTS)), ("floats", F32, ("B", capi.SIM3_SOLVE_FLOATS)), ("inliers", U8, ("B", "n1")),
                        ("Tcw", F32, ("B", 12)), ("Ow", F32, ("B", 3)))
    SIM3_SOLVE_OUT = _names(SIM3_SOLVE_TABLE)
    SIM3_MERGE_TABLE = (("matched", I32, ("n1",)), ("matched_kf", I32, ("n1",)), ("num_matches", I32, (1,)))

    @staticmethod
    def sim3_max_err(sigma2: float = 1.0) -> float:
        """(float)(size_t)(9.210 * mvLevelSigma2[0]): the reference keeps the threshold in a std::vector<size_t>"""
        return float(int(9.210 * float(np.float32(sigma2))))

    @staticmethod
    def sim3_solve_iterations(prob: float, min_inliers: int, max_its: int, N: int) -> int:
        return int(lib().xfh_sim3_solve_iterations(float(prob), int(min_inliers), int(max_its), int(N)))

    @staticmethod
    def sim3_solve_iterations_table(prob: float, min_inliers: int, max_its: int, n1: int) -> np.ndarray:
        t = np.zeros(n1 + 1, np.int32)
        check(lib().xfh_sim3_solve_iterations_table(float(prob), int(min_inliers), int(max_its), int(n1), t.ctypes.data))
        return t

    @staticmethod
    def sim3_solve_layout(B: int, n1: int, guard: int = 0):
        """byte offsets of the outputs of sim3_solve_device inside one buffer (and its size under "bytes"); guard as in fuse_search_layout"""
        return Layout.of(Context.SIM3_SOLVE_TABLE, guard, B=B, n1=n1)

    @staticmethod
    def sim3_solve_parse(raw: np.ndarray, lay, B: int, n1: int):
        """lay.parse(raw) under the name and arguments that callers of the hand-written layouts use"""
        return lay.parse(raw)

    @staticmethod
    def sim3_merge_layout(n1: int, guard: int = 0):
        """the outputs of sim3_merge_matches_device (d_matched, d_matched_kf, d_num_matches) inside one buffer; guard as in fuse_search_layout"""
        return Layout.of(Context.SIM3_MERGE_TABLE, guard, n1=n1)

    def sim3_solve_device(self, B: int, n1: int, M: int, d_points, d_point1, d_matched, d_T1w, T1w_stride: int, d_T2w, cam1, cam2, d_iters_of_N, max_iters: int,
                          d_draws, draws_stride: int, rand_max: int, d_workspace, d_out, min_inliers: int = 15, fix_scale: bool = False, max_err1: float = 9.0,
                          max_err2: float = 9.0, min_matches: int = 0, d_num_matches=None, guard: int = 0):
        """xfh_sim3_solve_device on device pointers; asynchronous.  d_out: the outputs laid out as sim3_solve_layout(B, n1, guard) says; d_workspace:
        xfh_sim3_solve_workspace_bytes(n1, M, B) bytes"""
        o = self.sim3_solve_layout(B, n1, guard)
        check(lib().xfh_sim3_solve_device(self.h, B, n1, M, d_points, d_point1, d_matched, d_T1w, T1w_stride, d_T2w, C.byref(cam1), C.byref(cam2), float(max_err1),
                                          float(max_err2), int(bool(fix_scale)), int(min_inliers), int(min_matches), d_num_matches, d_iters_of_N, max_iters, d_draws,
                                          draws_stride, rand_max, d_workspace, *[d_out + o[k] for k in self.SIM3_SOLVE_OUT]), self.h)

    @staticmethod
    def _sim3_solve_arrays(points, point1, matched, T1w, T2w, iters_of_N, draws, prior=None):
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        p1 = np.ascontiguousarray(point1, np.int32).ravel()
        m = np.ascontiguousarray(matched, np.int32)
        B = 1 if m.ndim == 1 else m.shape[0]
        n1 = m.shape[-1]
        assert len(p1) == n1
        t1, t2 = np.ascontiguousarray(T1w, np.float32), np.ascontiguousarray(T2w, np.float32).reshape(B, 12)
        t1 = t1.reshape(-1, 12)
        tb, d = np.ascontiguousarray(iters_of_N, np.int32), np.ascontiguousarray(draws, np.int32)
        assert len(tb) == n1 + 1 and t1.shape[0] in (1, B)
        return B, n1, len(pts), pts, p1, m, t1, t2, tb, d, _with_prior(Context.sim3_solve_layout(B, n1).zeros(), prior)

    @staticmethod
    def sim3_solve_host(cam1, cam2, points, point1, matched, T1w, T2w, iters_of_N, draws, rand_max: int, min_inliers: int = 15, fix_scale: bool = False,
                        max_err1: float = 9.0, max_err2: float = 9.0, min_matches: int = 0, num_matches=None, prior=None):
        """xfh_sim3_solve_host: the whole rule on one host thread, no ctx.  matched [n1] or [B][n1]; T1w [12] shared or [B][12]; draws [max_iters][3]
        shared or [B][max_iters][3] -> dict(header, floats, inliers, Tcw, Ow), each with a leading B"""
        B, n1, M, pts, p1, m, t1, t2, tb, d, out = Context._sim3_solve_arrays(points, point1, matched, T1w, T2w, iters_of_N, draws, prior)
        max_iters = d.shape[-2]
        ws = np.zeros(lib().xfh_sim3_solve_workspace_bytes(n1, M, B) + 16, np.uint8)
        wp = (ws.ctypes.data + 15) & ~15
        nm = None if num_matches is None else np.array([num_matches], np.int32)
        check(lib().xfh_sim3_solve_host(B, n1, M, pts.ctypes.data, p1.ctypes.data, m.ctypes.data, t1.ctypes.data, 0 if t1.shape[0] == 1 else 12, t2.ctypes.data,
                                        C.byref(cam1), C.byref(cam2), float(max_err1), float(max_err2), int(bool(fix_scale)), int(min_inliers), int(min_matches),
                                        _ptr(nm), tb.ctypes.data, max_iters, d.ctypes.data, 0 if d.ndim == 2 else max_iters * 3, rand_max,
                                        wp, *[out[k].ctypes.data for k in Context.SIM3_SOLVE_OUT]))
        return out

    def sim3_solve(self, cam1, cam2, points, point1, matched, T1w, T2w, iters_of_N, draws, rand_max: int, min_inliers: int = 15, fix_scale: bool = False,
                   max_err1: float = 9.0, max_err2: float = 9.0, prior=None):
        """xfh_sim3_solve (host pointers, one problem) -> the dict of sim3_solve_host with B = 1"""
        B, n1, M, pts, p1, m, t1, t2, tb, d, out = self._sim3_solve_arrays(points, point1, matched, T1w, T2w, iters_of_N, draws, prior)
        assert B == 1 and d.ndim == 2
        check(lib().xfh_sim3_solve(self.h, n1, M, pts.ctypes.data, p1.ctypes.data, m.ctypes.data, t1.ctypes.data, t2.ctypes.data, C.byref(cam1), C.byref(cam2),
                                   float(max_err1), float(max_err2), int(bool(fix_scale)), int(min_inliers), tb.ctypes.data, d.shape[0], d.ctypes.data, rand_max,
                                   *[out[k].ctypes.data for k in self.SIM3_SOLVE_OUT]), self.h)
        return out

    @staticmethod
    def sim3_solve_set(draws3, rand_max: int, N: int):
        d, s = np.ascontiguousarray(draws3, np.int32), np.zeros(3, np.int32)
        check(lib().xfh_sim3_solve_set(d.ctypes.data, rand_max, N, s.ctypes.data))
        return s

    @staticmethod
    def sim3_solve_horn(P1, P2, fix_scale: bool = False):
        """two point triples [3][3] (point j in row j) -> hyp [40]: T12 [12], R [9], t [3], s, T21 [12], zeros"""
        a, b, h = np.ascontiguousarray(P1, np.float32), np.ascontiguousarray(P2, np.float32), np.zeros(capi.SIM3_SOLVE_HYP_FLOATS, np.float32)
        check(lib().xfh_sim3_solve_horn(a.ctypes.data, b.ctypes.data, int(bool(fix_scale)), h.ctypes.data))
        return h

    @staticmethod
    def sim3_solve_check(T12, T21, cam1, cam2, X1, X2, max_err1: float = 9.0, max_err2: float = 9.0):
        """-> (err [2], inlier) of one correspondence"""
        a, b, x1, x2 = [np.ascontiguousarray(v, np.float32) for v in (T12, T21, X1, X2)]
        err, inl = np.zeros(2, np.float32), C.c_int(0)
        check(lib().xfh_sim3_solve_check(a.ctypes.data, b.ctypes.data, C.byref(cam1), C.byref(cam2), x1.ctypes.data, x2.ctypes.data, float(max_err1), float(max_err2),
                                         err.ctypes.data, C.byref(inl)))
        return err, inl.value

    @staticmethod
    def _sim3_merge_arrays(match12, point2):
        m, p2 = np.ascontiguousarray(match12, np.int32), np.ascontiguousarray(point2, np.int32)
        assert m.ndim == 2 and p2.ndim == 2 and m.shape[0] == p2.shape[0]
        n1 = m.shape[1]
        return (m.shape[0], n1, p2.shape[1], m, p2, *Context.sim3_merge_layout(n1).zeros().values())

    @staticmethod
    def sim3_merge_matches_host(match12, point2, M: int):
        """xfh_sim3_merge_matches_host: match12 [J][n1], point2 [J][n2] -> (matched [n1], matched_kf [n1], numBoWMatches)"""
        J, n1, n2, m, p2, o0, o1, o2 = Context._sim3_merge_arrays(match12, point2)
        ws = np.zeros(M + 4, np.int32)
        wp = (ws.ctypes.data + 15) & ~15
        check(lib().xfh_sim3_merge_matches_host(J, n1, n2, M, m.ctypes.data, p2.ctypes.data, wp, o0.ctypes.data, o1.ctypes.data, o2.ctypes.data))
        return o0, o1, int(o2[0])

    def sim3_merge_matches(self, match12, point2, M: int):
        """xfh_sim3_merge_matches (host pointers) -> as sim3_merge_matches_host"""
        J, n1, n2, m, p2, o0, o1, o2 = self._sim3_merge_arrays(match12, point2)
        check(lib().xfh_sim3_merge_matches(self.h, J, n1, n2, M, m.ctypes.data, p2.ctypes.data, o0.ctypes.data, o1.ctypes.data, o2.ctypes.data), self.h)
        return o0, o1, int(o2[0])

    def sim3_merge_matches_device(self, J: int, n1: int, n2: int, M: int, d_match12, d_point2, d_workspace, d_matched, d_matched_kf, d_num_matches):
        check(lib().xfh_sim3_merge_matches_device(self.h, J, n1, n2, M, d_match12, d_point2, d_workspace, d_matched, d_matched_kf, d_num_matches), self.h)

    # -- Tracking::Relocalization: MLPnPsolver between SearchByBoW and PoseOptimization (xfh_mlpnp_*) ------------------------------------------------------
    MLPNP_HEADER = ("N", "status", "its", "min_inliers", "winner", "n_inliers", "best", "best_count", "consumed", "refines", "planar")
    MLPNP_TABLE = (("header", I32, ("B", capi.MLPNP_HEADER_INTS)), ("Tcw", F32, ("B", 12)), ("inliers", U8, ("B", "n")), ("assigned_out", I32, ("B", "n")))
    MLPNP_OUT = _names(MLPNP_TABLE)
    MLPNP_STATUS = ("TOO_FEW", "NONE", "BEST", "REFINED")

    @staticmethod
    def mlpnp_iterations_table(n: int, prob: float = 0.99, min_inliers: int = 10, max_its: int = 300, min_set: int = 6, eps: float = 0.5):
        """xfh_mlpnp_iterations_table -> (iters_of_N [n + 1], min_inliers_of_N [n + 1]): SetRansacParameters for every N"""
        t, m = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32)
        check(lib().xfh_mlpnp_iterations_table(float(prob), int(min_inliers), int(max_its), int(min_set), float(eps), int(n), t.ctypes.data, m.ctypes.data))
        return t, m

    @staticmethod
    def mlpnp_layout(B: int, n: int, guard: int = 0):
        """byte offsets of the outputs of mlpnp_solve_device inside one buffer (and its size under "bytes"); guard as in fuse_search_layout"""
        return Layout.of(Context.MLPNP_TABLE, guard, B=B, n=n)

    @staticmethod
    def mlpnp_parse(raw: np.ndarray, lay, B: int, n: int):
        """lay.parse(raw) under the name and arguments that callers of the hand-written layouts use"""
        return lay.parse(raw)

    def mlpnp_solve_device(self, B: int, n: int, nq: int, d_xy_un, d_assigned, d_points, d_point_valid, cam, max_err: float, d_iters_of_N, d_min_inliers_of_N,
                           chunk: int, d_start_iter, max_iters: int, d_draws, draws_stride: int, rand_max: int, d_workspace, d_out, min_matches: int = 0,
                           d_n_matches=None, guard: int = 0):
        """xfh_mlpnp_solve_device on device pointers; asynchronous.  d_out: the outputs laid out as mlpnp_layout(B, n, guard) says; d_workspace:
        xfh_mlpnp_workspace_bytes(n, nq, B, max_iters) bytes"""
        o = self.mlpnp_layout(B, n, guard)
        check(lib().xfh_mlpnp_solve_device(self.h, B, n, nq, d_xy_un, d_assigned, d_points, d_point_valid, C.byref(cam), float(max_err), int(min_matches), d_n_matches,
                                           d_iters_of_N, d_min_inliers_of_N, int(chunk), d_start_iter, max_iters, d_draws, draws_stride, rand_max, d_workspace,
                                           *[d_out + o[k] for k in self.MLPNP_OUT]), self.h)

    @staticmethod
    def _mlpnp_arrays(xy_un, assigned, points, point_valid, tables, draws, prior=None):
        xy = np.ascontiguousarray(xy_un, np.float32).reshape(-1, 2)
        a = np.ascontiguousarray(assigned, np.int32)
        B, n = (1 if a.ndim == 1 else a.shape[0]), a.shape[-1]
        pts = np.ascontiguousarray(points, np.float32).reshape(B, -1, 3)
        nq = pts.shape[1]
        va = None if point_valid is None else np.ascontiguousarray(point_valid, np.uint8).reshape(B, nq)
        ti, tm = np.ascontiguousarray(tables[0], np.int32), np.ascontiguousarray(tables[1], np.int32)
        d = np.ascontiguousarray(draws, np.int32)
        assert len(xy) == n and len(ti) == n + 1 and len(tm) == n + 1 and d.shape[-1] == 6
        return B, n, nq, xy, a, pts, va, ti, tm, d, _with_prior(Context.mlpnp_layout(B, n).zeros(), prior)

    @staticmethod
    def mlpnp_solve_host(cam, xy_un, assigned, points, tables, draws, rand_max: int, max_err: float = 5.991, chunk: int = 5, start_iter=None, point_valid=None,
                         min_matches: int = 0, n_matches=None, prior=None):
        """xfh_mlpnp_solve_host: the whole rule on one host thread, no ctx.  assigned [n] or [B][n]; points [B][nq][3]; tables = (iters_of_N, min_inliers_of_N);
        draws [max_iters][6] shared or [B][max_iters][6]; start_iter None or [B] -> dict(header, Tcw, inliers, assigned_out), each with a leading B"""
        B, n, nq, xy, a, pts, va, ti, tm, d, out = Context._mlpnp_arrays(xy_un, assigned, points, point_valid, tables, draws, prior)
        max_iters = d.shape[-2]
        ws = np.zeros(lib().xfh_mlpnp_workspace_bytes(n, nq, B, max_iters) + 16, np.uint8)
        wp = (ws.ctypes.data + 15) & ~15
        nm = None if n_matches is None else np.ascontiguousarray(n_matches, np.int32).reshape(B)
        st = None if start_iter is None else np.ascontiguousarray(start_iter, np.int32).reshape(B)
        check(lib().xfh_mlpnp_solve_host(B, n, nq, xy.ctypes.data, a.ctypes.data, pts.ctypes.data, _ptr(va), C.byref(cam), float(max_err),
                                         int(min_matches), _ptr(nm), ti.ctypes.data, tm.ctypes.data, int(chunk),
                                         _ptr(st), max_iters, d.ctypes.data, 0 if d.ndim == 2 else max_iters * 6, rand_max, wp,
                                         *[out[k].ctypes.data for k in Context.MLPNP_OUT]))
        return out

    def mlpnp_solve(self, cam, xy_un, assigned, points, tables, draws, rand_max: int, max_err: float = 5.991, chunk: int = 5, start_iter: int = 0, point_valid=None,
                    prior=None):
        """xfh_mlpnp_solve (host pointers, one problem) -> the dict of mlpnp_solve_host with B = 1"""
        B, n, nq, xy, a, pts, va, ti, tm, d, out = self._mlpnp_arrays(xy_un, assigned, points, point_valid, tables, draws, prior)
        assert B == 1 and d.ndim == 2
        check(lib().xfh_mlpnp_solve(self.h, n, nq, xy.ctypes.data, a.ctypes.data, pts.ctypes.data, _ptr(va), C.byref(cam), float(max_err),
                                    ti.ctypes.data, tm.ctypes.data, int(chunk), int(start_iter), d.shape[0], d.ctypes.data, rand_max,
                                    *[out[k].ctypes.data for k in self.MLPNP_OUT]), self.h)
        return out

    @staticmethod
    def mlpnp_set(draws6, rand_max: int, N: int):
        d, s = np.ascontiguousarray(draws6, np.int32), np.zeros(6, np.int32)
        check(lib().xfh_mlpnp_set(d.ctypes.data, rand_max, N, s.ctypes.data))
        return s

    @staticmethod
    def mlpnp_nullspace(f):
        """bearing vector [3] (doubles) -> (r [3], s [3])"""
        a, rs = np.ascontiguousarray(f, np.float64), np.zeros(6, np.float64)
        check(lib().xfh_mlpnp_nullspace(a.ctypes.data, rs.ctypes.data))
        return rs[:3].copy(), rs[3:].copy()

    @staticmethod
    def mlpnp_compute_pose(f, p, use=None, fold: bool = False):
        """bearing vectors [m][3] and points [m][3] (floats), use [m] bytes or None -> (Rt [3][4] doubles, planar)"""
        a, b = np.ascontiguousarray(f, np.float32), np.ascontiguousarray(p, np.float32)
        u = _opt(use, np.uint8)
        Rt, planar = np.zeros(12, np.float64), C.c_int(0)
        check(lib().xfh_mlpnp_compute_pose(len(a), a.ctypes.data, b.ctypes.data, _ptr(u), int(bool(fold)), Rt.ctypes.data, C.byref(planar)))
        return Rt.reshape(3, 4), planar.value

    @staticmethod
    def mlpnp_check(Rt, cam, X, xy, max_err: float = 5.991):
        """-> (error2, inlier) of one correspondence under Rt [3][4] (doubles)"""
        T, x, k = np.ascontiguousarray(Rt, np.float64), np.ascontiguousarray(X, np.float32), np.ascontiguousarray(xy, np.float32)
        e, inl = C.c_float(0.0), C.c_int(0)
        check(lib().xfh_mlpnp_check(T.ctypes.data, C.byref(cam), x.ctypes.data, k.ctypes.data, float(max_err), C.byref(e), C.byref(inl)))
        return np.float32(e.value), inl.value

    def timing_enable(self, kernel_id: int, layer_mask: int = 0):
        check(lib().xfh_timing_enable(self.h, kernel_id, layer_mask), self.h)

    def timing_read(self):
        n = C.c_int(0); ms = C.c_double(0.0)
        check(lib().xfh_timing_read(self.h, C.byref(n), C.byref(ms)), self.h)
        return n.value, ms.value


def scale_tables(nlevels: int, scaleFactor: float):
    """mvScaleFactor, mvInvScaleFactor, mvLevelSigma2, mvInvLevelSigma2 (XFextractor.cc:80-96),
    fp32 arithmetic as in the reference"""
    sf = np.ones(nlevels, np.float32); s2 = np.ones(nlevels, np.float32)
    for i in range(1, nlevels):
        sf[i] = np.float32(sf[i - 1] * np.float32(scaleFactor))
        s2[i] = np.float32(sf[i] * sf[i])
    return sf, (np.float32(1.0) / sf).astype(np.float32), s2, (np.float32(1.0) / s2).astype(np.float32)


class XFextractor:
    """Drop-in for `ORB_SLAM3::XFextractor` (reference include/XFextractor.h:32-67)."""

    def __init__(self, nfeatures: int, scaleFactor: float, nlevels: int, iniThFAST: int, minThFAST: int,
                 weights: bytes | None = None, max_height: int = 480, max_width: int = 640, device: int = 0):
        self.nfeatures, self.scaleFactor, self.nlevels = nfeatures, float(np.float32(scaleFactor)), nlevels
        self.iniThFAST, self.minThFAST = iniThFAST, minThFAST
        self.mvScaleFactor, self.mvInvScaleFactor, self.mvLevelSigma2, self.mvInvLevelSigma2 = scale_tables(nlevels, scaleFactor)
        self.mvImagePyramid = [None] * nlevels          # sized, never filled (XFextractor.cc:98)
        self.ctx = Context(nfeatures, max_height, max_width, 1, device)
        if weights is not None:
            self.ctx.load_weights(weights)

    def __call__(self, image, mask=None, vLappingArea=(0, 0)):
        """returns (ret, keypoints[nfeatures], descriptors[nfeatures,64] or None); ret = -1 for
        an empty image, else monoIndex (XFextractor.cc:250-356)."""
        if image is None or getattr(image, "size", 0) == 0:
            return -1, None, None                        # :253-254
        image = np.asarray(image)
        if image.dtype != np.uint8 or image.ndim != 2:
            raise ValueError("image must be CV_8UC1")     # assert at :257
        H, W = image.shape
        img = np.ascontiguousarray(image)
        kps = np.zeros(self.nfeatures, KP_DTYPE)
        desc = np.zeros((self.nfeatures, 64), np.float32)
        nv, mono = C.c_int(0), C.c_int(0)
        check(lib().xfh_extract(self.ctx.h, img.ctypes.data, H, W, W, int(vLappingArea[0]), int(vLappingArea[1]),
                                kps.ctypes.data, desc.ctypes.data, C.byref(nv), C.byref(mono)), self.ctx.h)
        self.n_valid = nv.value
        if nv.value == 0:
            return mono.value, kps, None                 # _descriptors.release() (:350-353)
        return mono.value, kps, desc

    detectAndCompute = __call__

    def GetLevels(self): return self.nlevels
    def GetScaleFactor(self): return self.scaleFactor
    def GetScaleFactors(self): return self.mvScaleFactor
    def GetInverseScaleFactors(self): return self.mvInvScaleFactor
    def GetScaleSigmaSquares(self): return self.mvLevelSigma2
    def GetInverseScaleSigmaSquares(self): return self.mvInvLevelSigma2


class ORBmatcher:
    """The XFeat half of `ORB_SLAM3::ORBmatcher` (reference include/ORBmatcher.h:43,77)."""
    TH_HIGH = 1000      # ORBmatcher.cc:34 (USE_ORB unset)
    TH_LOW = 100        # ORBmatcher.cc:35

    def __init__(self, nnratio: float = 0.6, checkOri: bool = True, ctx: Context | None = None):
        self.mfNNratio, self.mbCheckOrientation = nnratio, checkOri
        self.ctx = ctx or Context(nfeatures=1, max_height=32, max_width=32)

    @staticmethod
    def DescriptorDistance(a: np.ndarray, b: np.ndarray) -> int:
        a = np.ascontiguousarray(a, np.float32).ravel(); b = np.ascontiguousarray(b, np.float32).ravel()
        return int(lib().xfh_descriptor_distance(a.ctypes.data, b.ctypes.data))

    def fuse(self, points, normals, distances, query_desc, query_flags, Tcw, Ow, cam, bounds, th: float, scale_factors, kps, targets, uright=None,
             sim3: bool = False, ratio_max=None):
        """The search of `ORBmatcher::Fuse` for one keyframe (ORBmatcher.cc:1333-1523; sim3 = True: the form of :1525-1640 with Tcw = [R | t/s]
        and Ow from the caller's decomposition: no chi-square gates, bestDist starts at INT_MAX).  -> (nFused, result dict of
        Context.fuse_search); the caller runs :1497-1516 resp. :1622-1636 over best_idx in query order."""
        sf = np.ascontiguousarray(scale_factors, np.float32)
        if ratio_max is None:
            ratio_max = Context.scale_level_thresholds(float(sf[1]) if len(sf) > 1 else 1.2, len(sf))
        r = self.ctx.fuse_search(points, normals, distances, query_desc, query_flags, Tcw, Ow, cam, bounds, th, sf, ratio_max, kps, targets, uright=uright,
                                 chi2=not sim3, init_dist=0x7fffffff if sim3 else 256, th_low=self.TH_LOW)
        return r["n_fused"], r

    def search_for_triangulation(self, node_of1, xy1, has1, desc1, node_of2, xy2, has2, desc2, F12, ep, uright1=None, uright2=None,
                                 only_stereo: bool = False, coarse: bool = False, scale_factor0: float = 1.0, level_sigma2_0: float = 1.0):
        """`ORBmatcher::SearchForTriangulation` for one keyframe pair (ORBmatcher.cc:1092-1331) without the rotation histogram
        -> (nmatches, vMatchedPairs in ascending idx1, result dict of Context.triangulation_search)"""
        r = self.ctx.triangulation_search(node_of1, xy1, has1, desc1, node_of2, xy2, has2, desc2, F12, ep, uright1=uright1, uright2=uright2,
                                          only_stereo=only_stereo, coarse=coarse, th_low=self.TH_LOW,
                                          epipole_r2=float(np.float32(100) * np.float32(scale_factor0)), unc=level_sigma2_0)
        m = r["match12"]
        return r["n_matches"], [(int(i), int(m[i])) for i in np.nonzero(m >= 0)[0]], r

    def triangulate(self, cam, k1, k2s, match12, level_sigma2_0: float = 1.0, scale_factor: float = 1.2, scale_factor_last: float = 1.0, far_th: float = 0.0,
                    inertial: bool = False):
        """The loop body of `LocalMapping::CreateNewMapPoints` (LocalMapping.cc:481-710) for all neighbours at once, with the claim
        -> list of (idx1, neighbour, idx2, x3D, normal, (mfMinDistance bound, mfMaxDistance bound, mfMaxDistance), bPointStereo) in the reference's creation
        order, and the result dict of Context.triangulate; the caller runs :694-709 over the list"""
        r = self.ctx.triangulate(cam, k1, k2s, match12, sigma2=level_sigma2_0, ratio_factor=float(np.float32(1.5) * np.float32(scale_factor)),
                                 scale_last=scale_factor_last, far_th=far_th, inertial=inertial, claim=True)
        out = []
        for j in range(r["n_new"]):
            i, b = int(r["new_idx1"][j]), int(r["new_b"][j])
            out.append((i, b, int(r["new_idx2"][j]), r["new_xyz"][j], r["new_normal"][j], r["new_dist"][j], bool(r["kind"][b, i] != 0)))
        return out, r

    def ComputeBoW(self, vocab_blob, desc, levelsup: int = 4):
        """`Frame::ComputeBoW` / `KeyFrame::ComputeBoW` (Frame.cc:936, KeyFrame.cc:105: mpORBvocabulary->transform(vCurrentDesc, mBowVec, mFeatVec, 4)) on a
        vocabulary blob of Context.vocab_pack, over every row of desc.  -> (mBowVec as a list of (word id, value) in ascending word id,
        node_of = mFeatVec flattened for search_by_bow / search_for_triangulation, result dict of Context.bow_transform)"""
        r = self.ctx.bow_transform(vocab_blob, desc, levelsup)
        return list(zip(r["bow_ids"].tolist(), r["bow_vals"].tolist())), r["node_of"], r

    def search_by_bow(self, node_of1, has1, desc1, node_of2, desc2):
        """`ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches)` (ORBmatcher.cc:408-610): side 1 = the keyframe (has1[i] != 0 where
        its map point i exists and is not bad), side 2 = the frame.  The rotation histogram removes nothing (every XFeat angle is -1).
        -> (nmatches, match12 = per keyframe keypoint the frame keypoint or -1, result dict of Context.bow_search; its assigned2 is
        vpMapPointMatches by frame keypoint)"""
        r = self.ctx.bow_search(node_of1, has1, desc1, node_of2, desc2, eligible2=None, strict_low=False, init_dist=256, th_low=self.TH_LOW,
                                nn_ratio=self.mfNNratio)
        return r["n_matches"], r["match12"], r

    def search_by_bow_keyframes(self, node_of1, has1, desc1, node_of2, has2, desc2):
        """`ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12)` (ORBmatcher.cc:950-1090): both sides need a good map point and the
        threshold is strict.  -> (nmatches, match12 = vpMatches12 by index, result dict of Context.bow_search)"""
        r = self.ctx.bow_search(node_of1, has1, desc1, node_of2, desc2, eligible2=has2, strict_low=True, init_dist=256, th_low=self.TH_LOW,
                                nn_ratio=self.mfNNratio)
        return r["n_matches"], r["match12"], r

    def _map_projection(self, form, accept_max, points, normals, distances, query_desc, query_flags, Tcw, Ow, cam, bounds, th, scale_factors, kps, targets, taken,
                        ratio_max):
        sf = np.ascontiguousarray(scale_factors, np.float32)
        if ratio_max is None:
            ratio_max = Context.scale_level_thresholds(float(sf[1]) if len(sf) > 1 else 1.2, len(sf))
        r = self.ctx.map_projection_search(form, points, normals, distances, query_desc, query_flags, Tcw, Ow, cam, bounds, th, sf, ratio_max, kps, targets,
                                           taken=taken, init_dist=256, accept_max=accept_max)
        return r["n_matches"], r

    def searchByProjectionSim3(self, points, normals, distances, query_desc, query_flags, Tcw, Ow, cam, bounds, th: float, ratioHamming: float, scale_factors,
                               kps, targets, taken=None, with_keyframes: bool = False, ratio_max=None):
        """`ORBmatcher::SearchByProjection(KeyFrame*, Sim3f& Scw, vpPoints, vpMatched, th, ratioHamming)` (ORBmatcher.cc:612-717; with_keyframes: the
        form of :719-831 with vpPointsKFs / vpMatchedKF, which projects with invz) for one keyframe.  Tcw = [R | t/s] and Ow from the caller's
        decomposition of Scw; taken[k] != 0 where vpMatched[k] is set at entry.  -> (nmatches, result dict of Context.map_projection_search);
        the caller writes vpMatched[k] = vpPoints[assigned[k]] (and vpMatchedKF[k] = vpPointsKFs[assigned[k]]) where assigned[k] >= 0."""
        accept = float(np.float32(self.TH_LOW) * np.float32(ratioHamming))                       # TH_LOW*ratioHamming: int times float (:708)
        return self._map_projection(capi.MAPPROJ_FORM_SIM3_KF if with_keyframes else capi.MAPPROJ_FORM_SIM3, accept, points, normals, distances, query_desc,
                                    query_flags, Tcw, Ow, cam, bounds, th, scale_factors, kps, targets, taken, ratio_max)

    def searchByProjectionReloc(self, points, normals, distances, query_desc, query_flags, Tcw, Ow, cam, bounds, th: float, ORBdist: int, scale_factors,
                                kps, targets, taken=None, ratio_max=None):
        """`ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame*, sAlreadyFound, th, ORBdist)` (ORBmatcher.cc:2074-2195) for one candidate
        keyframe: its map points (in keypoint order) into the current frame.  taken[k] != 0 where CurrentFrame.mvpMapPoints[k] is set at entry;
        normals are not read by this form.  -> (nmatches, result dict); the caller writes mvpMapPoints[k] where assigned[k] >= 0."""
        return self._map_projection(capi.MAPPROJ_FORM_RELOC, float(np.float32(int(ORBdist))), points, normals, distances, query_desc, query_flags, Tcw, Ow, cam,
                                    bounds, th, scale_factors, kps, targets, taken, ratio_max)

    def searchBySim3(self, side1, side2, M21, M12, cam, bounds, th: float, scale_factors, ratio_max=None):
        """`ORBmatcher::SearchBySim3` for one keyframe pair (ORBmatcher.cc:1642-1859).  side = dict(kps, desc, points, dist, mp_desc, flags, Tw) as
        Context.sim3_search takes it (flags bit0 = `pMP && !vbAlreadyMatched[i] && !pMP->isBad()`); M21 / M12 = the 3x4 [s*R | t] of S12.inverse() and
        S12.  -> (nFound, match12 = per keypoint of keyframe 1 the keypoint of keyframe 2 or -1, result dict of Context.sim3_search); the
        caller writes vpMatches12[i1] = vpMapPoints2[match12[i1]] (:1852)."""
        sf = np.ascontiguousarray(scale_factors, np.float32)
        if ratio_max is None:
            ratio_max = Context.scale_level_thresholds(float(sf[1]) if len(sf) > 1 else 1.2, len(sf))
        r = self.ctx.sim3_search(side1, side2, M21, M12, cam, bounds, th, sf, ratio_max, th_high=self.TH_HIGH)
        return r["n_found"], r["match12"], r

    def SearchForInitialization(self, kps1, desc1, kps2, desc2, prev_matched, windowSize: int = 10, bounds=None):
        """`ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize)` (ORBmatcher.cc:833-948).  kps1 / kps2: the
        frames' undistorted keypoints (KP_DTYPE; of kps1 only the count is used: every XFeat keypoint has octave 0, so `level1 > 0` skips
        none, and the rotation histogram removes nothing); prev_matched [n1][2]; bounds: F2's image bounds (default: 0, 0 and the ctx' image
        size).  -> (nmatches, vnMatches12, the updated prev_matched); the result dict of Context.init_search is kept in self.last_init"""
        k2 = np.ascontiguousarray(kps2, KP_DTYPE)
        b = bounds if bounds is not None else (0.0, 0.0, float(self.ctx.max_width), float(self.ctx.max_height))
        assert len(kps1) == len(desc1)
        r = self.ctx.init_search(desc1, prev_matched, k2, b, desc2, window=float(windowSize), th_low=self.TH_LOW, nn_ratio=self.mfNNratio)
        self.last_init = r
        return r["n_matches"], r["matches12"], r["prev_out"]

    def match(self, desc1: np.ndarray, desc2: np.ndarray, min_cossim: float = -1.0):
        """-> list of (queryIdx, trainIdx, distance) like std::vector<cv::DMatch>"""
        i1, i2, d = self.ctx.match_mnn(desc1, desc2, min_cossim)
        return list(zip(i1.tolist(), i2.tolist(), d.tolist()))


class KeyFrameDatabase:
    """`ORB_SLAM3::KeyFrameDatabase` without the inverted file (reference include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc): the BowVectors of
    the keyframes live in device arrays, one slot per keyframe, and a query scans them (Context.bowdb_query_device).  A slot is the caller's
    handle for a keyframe; the caller keeps the KeyFrame objects, erases a keyframe before it turns bad and owns the maps.  The two persistent
    scores (mRelocScore, mPlaceRecognitionScore) are two device arrays of the database, zero at the start."""

    def __init__(self, ctx: Context, n_slots: int, stride: int, nn: int = 10):
        assert 1 <= n_slots <= capi.BOWDB_MAX_SLOTS and 1 <= stride <= capi.GRID_MAX_N and 0 <= nn <= capi.BOWDB_MAX_NEIGHBOURS
        self.ctx, self.n_slots, self.stride, self.nn = ctx, n_slots, stride, nn
        self.next_seq = 0
        D = capi.DeviceBuffer
        z = lambda nbytes, fill=0: D(nbytes).upload(np.full(nbytes, fill, np.uint8))
        self.ids, self.vals, self.n_words, self.seq = z(4 * n_slots * stride, 0xFF), z(8 * n_slots * stride), z(4 * n_slots), z(4 * n_slots)
        self.neigh = z(4 * n_slots * max(nn, 1), 0xFF)                                         # -1: no neighbour
        self.state = {capi.BOWDB_FORM_RELOC: z(4 * n_slots), capi.BOWDB_FORM_NBEST: z(4 * n_slots)}
        self.q_ids, self.q_vals, self.q_n, self.excl = D(4 * stride), D(8 * stride), D(4), D(n_slots)
        self.ws = D(Context.bowdb_query_workspace_bytes(n_slots, 1))
        self.lay = Context.bowdb_query_layout(1, n_slots)
        self.out = D(self.lay["bytes"])

    def close(self):
        for b in (self.ids, self.vals, self.n_words, self.seq, self.neigh, self.q_ids, self.q_vals, self.q_n, self.excl, self.ws, self.out, *self.state.values()):
            b.free()

    @staticmethod
    def _put(buf, offset, arr):
        a = np.ascontiguousarray(arr)
        assert offset + a.nbytes <= buf.nbytes
        if a.nbytes:
            check(lib().xfh_memcpy_h2d(buf.ptr + offset, a.ctypes.data, a.nbytes))

    def add(self, slot: int, ids, vals, neighbours=()):
        """`KeyFrameDatabase::add(pKF)`: the keyframe's mBowVec (ascending word id) into a slot, at the end of the insertion order.
        neighbours: the slots of GetBestCovisibilityKeyFrames(nn), in its order (set_neighbours updates them later)"""
        i, v = np.ascontiguousarray(ids, np.uint32), np.ascontiguousarray(vals, np.float64)
        assert 0 <= slot < self.n_slots and len(i) == len(v) <= self.stride
        self._put(self.ids, 4 * slot * self.stride, i); self._put(self.vals, 8 * slot * self.stride, v)
        self._put(self.n_words, 4 * slot, np.array([len(i)], np.int32)); self._put(self.seq, 4 * slot, np.array([self.next_seq], np.uint32))
        self.next_seq += 1
        self.set_neighbours(slot, neighbours)

    def set_neighbours(self, slot: int, neighbours):
        ng = np.full(max(self.nn, 1), -1, np.int32)
        k = min(len(neighbours), self.nn)
        ng[:k] = np.asarray(neighbours, np.int32)[:k]
        self._put(self.neigh, 4 * slot * max(self.nn, 1), ng)

    def erase(self, slot: int):
        """`KeyFrameDatabase::erase(pKF)`: the slot is empty from now on"""
        assert 0 <= slot < self.n_slots
        self._put(self.n_words, 4 * slot, np.zeros(1, np.int32))

    def query(self, form: int, ids, vals, exclude=()):
        """one query -> dict as Context.bowdb_query_parse gives it.  exclude: the slots of the connected keyframes (and of the query keyframe)"""
        i, v = np.ascontiguousarray(ids, np.uint32), np.ascontiguousarray(vals, np.float64)
        assert len(i) == len(v) <= self.stride
        ex = np.zeros(self.n_slots, np.uint8)
        ex[np.asarray(list(exclude), np.int64)] = 1
        self._put(self.q_ids, 0, i); self._put(self.q_vals, 0, v); self._put(self.q_n, 0, np.array([len(i)], np.int32)); self._put(self.excl, 0, ex)
        self.ctx.bowdb_query_device(1, self.n_slots, form, self.q_ids.ptr, self.q_vals.ptr, self.q_n.ptr, self.stride, self.ids.ptr, self.vals.ptr,
                                    self.n_words.ptr, self.stride, self.seq.ptr, self.neigh.ptr if self.nn else None, self.nn, self.excl.ptr,
                                    self.state[form].ptr, self.ws.ptr, self.out.ptr)
        self.ctx.synchronize()
        return Context.bowdb_query_parse(self.out.download(np.uint8, self.lay["bytes"]), self.lay, 1, self.n_slots)[0]

    def DetectRelocalizationCandidates(self, ids, vals, map_of_slot=None, pMap=None):
        """`DetectRelocalizationCandidates(F, pMap)` (:733-845) -> the candidate slots in the reference's order.  map_of_slot[s] is compared with pMap
        (`if (pKFi->GetMap() != pMap) continue;`, :834); without it every candidate is returned"""
        r = self.query(capi.BOWDB_FORM_RELOC, ids, vals)
        cand = r["cand_slot"][:r["n_candidates"]].tolist()
        return [s for s in cand if map_of_slot is None or map_of_slot[s] == pMap]

    def DetectNBestCandidates(self, ids, vals, connected, nNumCandidates: int, map_of_slot, query_map, bad_maps=()):
        """`DetectNBestCandidates(pKF, vpLoopCand, vpMergeCand, nNumCandidates)` (:604-730) -> (vpLoopCand, vpMergeCand) as slots.  connected: the slots
        of pKF->GetConnectedKeyFrames() (add the slot of pKF itself when it is in the database); query_map: pKF->GetMap()"""
        r = self.query(capi.BOWDB_FORM_NBEST, ids, vals, exclude=connected)
        loop, merge = [], []
        for s in r["cand_slot"][:r["n_candidates"]].tolist():
            if not (len(loop) < nNumCandidates or len(merge) < nNumCandidates):
                break
            if map_of_slot[s] == query_map and len(loop) < nNumCandidates:
                loop.append(s)
            elif map_of_slot[s] != query_map and len(merge) < nNumCandidates and map_of_slot[s] not in bad_maps:
                merge.append(s)
        return loop, merge
