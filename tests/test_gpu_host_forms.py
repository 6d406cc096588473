"""The seven host-pointer entry points stage their arrays through ONE arena of the ctx (xfeatslam_amd/csrc/host_stage.h) that is shared
and regrown across calls.  One ctx (nfeatures 64), the seven forms interleaved with sizes that rise and fall -- counts whose byte sizes are no
multiple of the 256-byte piece alignment, one call far beyond the reservation xfh_create makes, small calls again -- optional arguments both
ways.  Every result equals the _device form of the same call on buffers the test uploads itself, every host output array sits inside a
sentinel-filled one whose margins stay untouched, and an early call repeated after the regrow returns the same bytes."""
import ctypes as C

import numpy as np
import pytest

from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context

pytestmark = pytest.mark.gpu

NF, BIG, SENT, MARGIN = 64, 1 << 30, 0xA5, 64
BOUNDS = (0.0, 0.0, 80.0, 60.0)


def cam_struct():
    return capi.Camera(fx=61.5, fy=60.25, cx=39.5, cy=30.25, k1=0.12, k2=-0.2, p1=0.001, p2=-0.002, k3=0.05, bf=40.0, width=80, height=60)


class Guarded:
    """a host output array of n items inside a larger one filled with the sentinel byte"""

    def __init__(self, n, dtype):
        self.full = np.full((n + 2 * MARGIN) * np.dtype(dtype).itemsize, SENT, np.uint8).view(dtype)
        self.mid = self.full[MARGIN:MARGIN + n]
        self.ptr = self.mid.ctypes.data

    def margins_untouched(self, used=None):
        b = self.full.view(np.uint8); it = self.full.itemsize
        end = MARGIN + (len(self.mid) if used is None else used)
        return bool((b[:MARGIN * it] == SENT).all() and (b[end * it:] == SENT).all())


def dev(arr, extra=256):
    a = np.ascontiguousarray(arr)
    return capi.DeviceBuffer(a.nbytes + extra).upload(a)


def descriptors(rs, n):
    d = rs.standard_normal((n, 64)).astype(np.float32)
    return d / np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-6).astype(np.float32)


def keypoints(rs, n):
    k = np.zeros(n, capi.KP_DTYPE)
    k["x"] = rs.uniform(0.5, 79.0, n); k["y"] = rs.uniform(0.5, 59.0, n); k["size"] = 1.0
    return k


def csr(rs, n_lists, limit, longest):
    ln = rs.randint(0, longest + 1, n_lists) if limit > 0 else np.zeros(n_lists, np.int64)
    off = np.concatenate([[0], np.cumsum(ln)]).astype(np.int32)
    return off, rs.randint(0, max(limit, 1), int(off[-1])).astype(np.int32)


class Forms:
    def __init__(self):
        self.L = capi.lib()
        self.ctx = Context(nfeatures=NF, max_height=64, max_width=96)
        self.h = self.ctx.h

    def ok(self, status):
        capi.check(status, self.h)

    # each method: the host form on guarded arrays, the device form on own buffers, equality, margins -> the host result's bytes
    def match_mnn(self, seed, n1, n2):
        rs = np.random.RandomState(seed)
        d1 = descriptors(rs, n1)
        d2 = np.ascontiguousarray(d1[rs.randint(0, n1, n2)] + 0.3 * descriptors(rs, n2), np.float32)      # (the global maximum is always mutual: n_matches > 0)
        nm = min(n1, n2)
        g = [Guarded(nm, np.int32), Guarded(nm, np.int32), Guarded(nm, np.float32)]
        n = C.c_int(-1)
        self.ok(self.L.xfh_match_mnn(self.h, d1.ctypes.data, n1, d2.ctypes.data, n2, -1.0, g[0].ptr, g[1].ptr, g[2].ptr, C.byref(n)))
        a, b, out = dev(d1), dev(d2), capi.DeviceBuffer(12 * nm + 512)
        self.ok(self.L.xfh_match_mnn_device(self.h, a.ptr, n1, b.ptr, n2, -1.0, out.ptr + 256, out.ptr + 256 + 4 * nm, out.ptr + 256 + 8 * nm, out.ptr))
        self.ctx.synchronize()
        k = int(out.download(np.int32, 1)[0])
        assert 0 < k <= nm and n.value == k, (n.value, k)
        for j, x in enumerate(g):
            assert np.array_equal(x.mid[:k].view(np.int32), out.download(np.int32, k, 256 + 4 * nm * j)), ("match_mnn", n1, n2, j)
            assert x.margins_untouched(used=k), ("match_mnn: entries past n_matches or margins written", n1, n2, j)      # past n_matches: still the sentinel
        for x in (a, b, out):
            x.free()
        return b"".join(x.mid[:k].tobytes() for x in g)

    def distance_i32(self, seed, n1, n2):
        rs = np.random.RandomState(seed)
        d1, d2 = descriptors(rs, n1), descriptors(rs, n2)
        g = Guarded(n1 * n2, np.int32)
        self.ok(self.L.xfh_distance_i32(self.h, d1.ctypes.data, n1, d2.ctypes.data, n2, g.ptr))
        a, b, out = dev(d1), dev(d2), capi.DeviceBuffer(4 * n1 * n2 + 256)
        self.ok(self.L.xfh_distance_i32_device(self.h, a.ptr, n1, b.ptr, n2, out.ptr))
        self.ctx.synchronize()
        assert np.array_equal(g.mid, out.download(np.int32, n1 * n2)) and g.margins_untouched(), ("distance_i32", n1, n2)
        for x in (a, b, out):
            x.free()
        return g.mid.tobytes()

    def best2_csr(self, seed, nq, nt, longest=9):
        rs = np.random.RandomState(seed)
        q, tg = descriptors(rs, nq), descriptors(rs, nt)
        off, ind = csr(rs, nq, nt, longest)
        g = [Guarded(nq, np.int32) for _ in range(4)]
        self.ok(self.L.xfh_best2_csr(self.h, q.ctypes.data, nq, tg.ctypes.data, nt, off.ctypes.data, ind.ctypes.data, BIG, *[x.ptr for x in g]))
        dq, dt, do, di, out = dev(q), dev(tg), dev(off), dev(ind), capi.DeviceBuffer(16 * nq + 256)
        self.ok(self.L.xfh_best2_csr_device(self.h, dq.ptr, nq, dt.ptr, nt, do.ptr, di.ptr, BIG, *[out.ptr + 4 * nq * j for j in range(4)]))
        self.ctx.synchronize()
        for j, x in enumerate(g):
            assert np.array_equal(x.mid, out.download(np.int32, nq, 4 * nq * j)) and x.margins_untouched(), ("best2_csr", nq, nt, j)
        for x in (dq, dt, do, di, out):
            x.free()
        return b"".join(x.mid.tobytes() for x in g)

    def distinctive_csr(self, seed, n_rows, n_groups, longest=7):
        rs = np.random.RandomState(seed)
        tb = descriptors(rs, n_rows)
        off, ind = csr(rs, n_groups, n_rows, longest)
        g = [Guarded(n_groups, np.int32) for _ in range(2)]
        self.ok(self.L.xfh_distinctive_csr(self.h, tb.ctypes.data, n_rows, off.ctypes.data, ind.ctypes.data, n_groups, g[0].ptr, g[1].ptr))
        dt, do, di, out = dev(tb), dev(off), dev(ind), capi.DeviceBuffer(8 * n_groups + 256)
        mg = int(np.diff(off).max())
        self.ok(self.L.xfh_distinctive_csr_device(self.h, dt.ptr, n_rows, do.ptr, di.ptr, n_groups, mg, out.ptr, out.ptr + 4 * n_groups))
        self.ctx.synchronize()
        for j, x in enumerate(g):
            assert np.array_equal(x.mid, out.download(np.int32, n_groups, 4 * n_groups * j)) and x.margins_untouched(), ("distinctive_csr", n_rows, n_groups, j)
        for x in (dt, do, di, out):
            x.free()
        return b"".join(x.mid.tobytes() for x in g)

    def scene(self, seed, nq, nt):
        """queries that sit near some of the targets, with descriptors that resemble them"""
        rs = np.random.RandomState(seed)
        k = keypoints(rs, nt); tg = descriptors(rs, nt)
        src = rs.randint(0, nt, nq)
        q = tg[src] + 0.2 * descriptors(rs, nq)
        uvr = np.stack([k["x"][src] + rs.uniform(-2, 2, nq), k["y"][src] + rs.uniform(-2, 2, nq), np.full(nq, 6.0)], 1).astype(np.float32)
        skip = (rs.uniform(size=nt) < 0.2).astype(np.uint8)
        ur = np.where(rs.uniform(size=nt) < 0.7, k["x"] - rs.uniform(0.5, 3, nt), -1.0).astype(np.float32)
        uq = (uvr[:, 0] - rs.uniform(0.5, 3, nq)).astype(np.float32)
        return k, tg, np.ascontiguousarray(q, np.float32), uvr, skip, ur, uq

    def search_window(self, seed, nq, nt, optional):
        k, tg, q, uvr, skip, ur, uq = self.scene(seed, nq, nt)
        p = lambda a: a.ctypes.data if optional else None
        g = [Guarded(nq, np.int32) for _ in range(5)]
        self.ok(self.L.xfh_search_window(self.h, q.ctypes.data, uvr.ctypes.data, nq, k.ctypes.data, C.byref(capi.GridBounds(*BOUNDS)), tg.ctypes.data, nt,
                                         p(skip), p(ur), p(uq), BIG, *[x.ptr for x in g]))
        dq, du, dk, dt, ds, dr, dy, out = dev(q), dev(uvr), dev(k), dev(tg), dev(skip), dev(ur), dev(uq), capi.DeviceBuffer(20 * nq + 256)
        grid = self.ctx.grid_build_device(dk.ptr, nt, BOUNDS)
        o = lambda b: b.ptr if optional else None
        self.ctx.search_window_device(dq.ptr, du.ptr, nq, grid.ptr, dt.ptr, nt, out.ptr, BIG, o(ds), o(dr), o(dy))
        self.ctx.synchronize()
        for j, x in enumerate(g):
            assert np.array_equal(x.mid, out.download(np.int32, nq, 4 * nq * j)) and x.margins_untouched(), ("search_window", nq, nt, optional, j)
        assert nq < 65 or (g[4].mid > 0).any()                                               # the scene does produce candidates
        for x in (dq, du, dk, dt, ds, dr, dy, out, grid):
            x.free()
        return b"".join(x.mid.tobytes() for x in g)

    def search_projection(self, seed, mode, nq, nt, optional, proj):
        k, tg, q, uvr, skip, ur, uq = self.scene(seed, nq, nt)
        rs = np.random.RandomState(seed + 1)
        cam = cam_struct()
        T = np.array([1, 0, 0, 0.01, 0, 1, 0, -0.02, 0, 0, 1, 0.03], np.float32)
        if mode == capi.PROJ_POINTS:                                                         # world points that land near the query positions
            z = rs.uniform(1.0, 4.0, nq).astype(np.float32)
            pts = np.stack([(uvr[:, 0] - cam.cx) / cam.fx * z, (uvr[:, 1] - cam.cy) / cam.fy * z, z], 1).astype(np.float32)
        else:
            pts = uvr
        fl = rs.choice(np.array([0, 1, 3, 3, 3], np.uint8), nq)
        given, points = mode == capi.PROJ_GIVEN, mode == capi.PROJ_POINTS
        p = lambda a, on=True: a.ctypes.data if on else None
        g = dict(status=Guarded(nq, np.uint8), match_idx=Guarded(nq, np.int32), best_dist=Guarded(nq, np.int32), second_dist=Guarded(nq, np.int32),
                 n_candidates=Guarded(nq, np.int32), proj=Guarded(3 * nq, np.float32), assigned=Guarded(nt, np.int32), n_matches=Guarded(1, np.int32))
        gb = capi.GridBounds(*BOUNDS)
        self.ok(self.L.xfh_search_projection(self.h, mode, nq, pts.ctypes.data, p(uq, given and optional), p(T, points), C.byref(cam) if points else None, C.byref(gb),
                                             8.0, q.ctypes.data, fl.ctypes.data, k.ctypes.data, tg.ctypes.data, nt, p(skip, optional), p(ur, optional), BIG, 1000, 0.9,
                                             g["status"].ptr, g["match_idx"].ptr, g["best_dist"].ptr, g["second_dist"].ptr, g["n_candidates"].ptr,
                                             g["proj"].ptr if proj else None, g["assigned"].ptr, g["n_matches"].ptr))
        lay = Context.search_projection_layout(1, nq, nt)
        dp, dq, dfl, dk, dt, ds, dr, dy, dT = dev(pts), dev(q), dev(fl), dev(k), dev(tg), dev(skip), dev(ur), dev(uq), dev(T)
        out, ws, dpo = capi.DeviceBuffer(lay["bytes"]), capi.DeviceBuffer(Context.search_projection_workspace_bytes(nq, nt, 1)), capi.DeviceBuffer(12 * nq + 256)
        grid = self.ctx.grid_build_device(dk.ptr, nt, BOUNDS)
        self.ctx.search_projection_device(mode, 1, nq, dp.ptr, dq.ptr, dfl.ptr, grid.ptr, dt.ptr, 0, nt, ws.ptr, out.ptr, radius=8.0, d_Tcw=dT.ptr if points else None,
                                          cam=cam if points else None, bounds=BOUNDS, d_ur_query=dy.ptr if given and optional else None,
                                          d_skip=ds.ptr if optional else None, d_uright=dr.ptr if optional else None, init_dist=BIG, nn_ratio=0.9,
                                          d_proj_out=dpo.ptr if proj else None)
        self.ctx.synchronize()
        for name, x in g.items():
            if name == "proj":
                want = dpo.download(np.float32, 3 * nq) if proj else x.mid                   # absent: the caller's array is never written
                assert np.array_equal(x.mid.view(np.uint32), want.view(np.uint32)), ("search_projection proj", mode, nq, nt)
            else:
                assert np.array_equal(x.mid, out.download(x.mid.dtype, len(x.mid), lay[name])), ("search_projection", name, mode, nq, nt, optional)
            assert x.margins_untouched(), ("search_projection margins", name, mode, nq, nt)
        assert nq < 65 or int(g["n_matches"].mid[0]) > 0                                     # the scene does produce matches
        for x in (dp, dq, dfl, dk, dt, ds, dr, dy, dT, out, ws, dpo, grid):
            x.free()
        return b"".join(x.mid.tobytes() for x in g.values())

    def frame_finish(self, seed, n, depth_u16):
        rs = np.random.RandomState(seed)
        k = keypoints(rs, n); cam = cam_struct()
        img = rs.randint(0, 6000, (60, 80)).astype(np.uint16) if depth_u16 else None
        g = [Guarded(2 * n, np.float32), Guarded(n, np.float32), Guarded(n, np.float32)]
        self.ok(self.L.xfh_frame_finish(self.h, k.ctypes.data, n, C.byref(cam), img.ctypes.data if depth_u16 else None,
                                        capi.DEPTH_U16 if depth_u16 else capi.DEPTH_NONE, 160, 1.0 / 5000.0, g[0].ptr, g[1].ptr, g[2].ptr))
        # the device form finishes extraction records of nfeatures keypoints; a keypoint's result depends on that keypoint alone, so the n
        # keypoints go through it in records of NF (the last one padded)
        rb, ko = self.L.xfh_record_bytes(NF), self.L.xfh_record_kps_offset()
        dimg = dev(img) if depth_u16 else None
        want = [np.zeros(0, np.float32)] * 3
        for lo in range(0, n, NF):
            part = np.zeros(NF, capi.KP_DTYPE); m = min(NF, n - lo); part[:m] = k[lo:lo + m]
            rec = np.zeros(rb, np.uint8); rec[ko:ko + part.nbytes] = part.view(np.uint8)
            dr = dev(rec)
            xy, ur, dz, _ = self.ctx.frame_finish_records(dr.ptr, 1, cam, d_depth=dimg.ptr if depth_u16 else None, depth_type=capi.DEPTH_U16 if depth_u16 else capi.DEPTH_NONE,
                                                          depth_pitch=160, depth_scale=1.0 / 5000.0, grid=False)
            self.ctx.synchronize()
            want = [np.concatenate([w, b.download(np.float32, c * m)]) for w, b, c in zip(want, (xy, ur, dz), (2, 1, 1))]
            for x in (dr, xy, ur, dz):
                x.free()
        for j, x in enumerate(g):
            assert np.array_equal(x.mid.view(np.uint32), want[j].view(np.uint32)) and x.margins_untouched(), ("frame_finish", n, depth_u16, j)
        assert depth_u16 == bool((g[2].mid > 0).any())
        if dimg:
            dimg.free()
        return b"".join(x.mid.tobytes() for x in g)


@pytest.fixture(scope="module")
def forms(gpu_lib):
    f = Forms()
    yield f
    f.ctx.close()


def test_interleaved_host_forms_share_one_arena(forms):
    f, P, G = forms, capi.PROJ_POINTS, capi.PROJ_GIVEN
    # counts at or below nfeatures: inside the reservation of xfh_create
    first = [f.match_mnn(1, 64, 64), f.best2_csr(2, 3, 65), f.search_window(3, 3, 64, True), f.frame_finish(4, 3, True), f.search_projection(5, P, 3, 64, True, True),
             f.distinctive_csr(6, 65, 3), f.distance_i32(7, 3, 1)]
    f.match_mnn(8, 1, 3); f.frame_finish(9, 1, False); f.search_window(10, 1, 1, False); f.best2_csr(11, 1, 0)
    f.search_projection(12, G, 1, 3, False, False); f.distinctive_csr(13, 0, 3)
    # rising, past the reservation: every one of these regrows the arena or reuses one regrown by a neighbour
    f.best2_csr(14, 257, 65); f.search_window(15, 65, 257, False); f.match_mnn(16, 257, 65); f.frame_finish(17, 257, True)
    f.search_projection(18, G, 65, 257, True, True); f.distinctive_csr(19, 257, 65); f.search_projection(20, P, 257, 65, False, False)
    f.distance_i32(21, 300, 300)
    f.search_window(22, 257, 65, True); f.frame_finish(23, 65, False)
    # small again, in a larger arena that holds the big calls' leftovers: the same bytes as the first time
    again = [f.match_mnn(1, 64, 64), f.best2_csr(2, 3, 65), f.search_window(3, 3, 64, True), f.frame_finish(4, 3, True), f.search_projection(5, P, 3, 64, True, True),
             f.distinctive_csr(6, 65, 3), f.distance_i32(7, 3, 1)]
    assert first == again
    f.search_projection(24, G, 3, 1, True, False); f.match_mnn(25, 3, 65)
