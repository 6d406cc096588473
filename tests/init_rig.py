"""The seeded scene of the monocular-initialisation tests in device memory (tests/test_gpu_init.py, tests/test_gpu_init_cpp.py,
tools/time_init.py): two frames extracted with the dense test weights from one image and a shifted, slightly warped copy
(tests/ref_init.py: warp), finished on the device (undistorted keypoints, grids), the seeded variants of tests/ref_init.py: plant, and one
guarded run of xfh_init_search_device.  prev_matched is F1's keypoints, as Tracking.cc:2486-2488 sets it.

Problem p of a run has its own window centres and query rows: the scene's rotated by p * ROLL places (the loop is sequential, so a rotated
block is another problem, not the same answers rotated); all problems search frame 1 with the planted target rows.  Problem 0 is the scene
whose conditions tests/test_init_ref.py asserts.  No test lives here."""
import numpy as np

import guarded
import ref_frame as RF
import ref_init as RI
import ref_window as RW
from projection_rig import GUARD, TUM1, F, H, W, cam_struct
from xfeatslam_amd import capi, synth
from xfeatslam_amd.extractor import Context

ROLL = 37
OUT_Q, OUT_T = Context.INIT_OUT_Q, Context.INIT_OUT_T


class InitRig:
    def __init__(self, L, blob, nf, seed, O):
        self.L, self.nf, self.seed, self.O = L, nf, seed, O
        self.ctx = Context(nfeatures=nf, max_height=H, max_width=W, max_batch=2)
        self.ctx.load_weights(blob)
        img = synth.image(H, W, seed)
        frames = np.stack([img, RI.warp(img)])
        self.din = capi.DeviceBuffer(frames.nbytes).upload(frames)
        self.rec = capi.DeviceBuffer(2 * self.ctx.rec_bytes)
        capi.check(L.xfh_extract_batch_device(self.ctx.h, self.din.ptr, 2, H, W, 0, 0, self.rec.ptr), self.ctx.h)
        self.bounds = Context.camera_bounds(cam_struct(TUM1))
        self.fin = self.ctx.frame_finish_records(self.rec.ptr, 2, cam_struct(TUM1), self.bounds, 0)
        self.ctx.synchronize()
        self.recs = self.ctx.parse_records(self.rec.download(np.uint8, 2 * self.ctx.rec_bytes), 2)
        self.xy = self.fin[0].download(F, 2 * nf * 2).reshape(2, nf, 2)
        self.x, self.y = self.xy[1][:, 0].copy(), self.xy[1][:, 1].copy()
        self.grid = RW.build(self.x, self.y, self.bounds)
        self.K = Context.init_search_layout(1, nf, nf)["K"]
        self.q, self.pm, self.tg, self.info = RI.plant(seed, self.xy[0], self.recs[0][1], self.xy[1], self.recs[1][1], self.K)
        self.valid1 = RW.valid_slots(nf, self.recs[0][2], self.recs[0][3])
        self.dtg = capi.DeviceBuffer(self.tg.nbytes).upload(self.tg)
        self.dgrid = self.fin[3].ptr + self.ctx.grid_bytes(nf)         # frame 1's blob
        self.dxy = self.fin[0].ptr + nf * 8                            # frame 1's undistorted keypoints
        self.bufs = []

    def dev(self, a):
        b = capi.DeviceBuffer(max(np.ascontiguousarray(a).nbytes, 16)).upload(a)
        self.bufs.append(b)
        return b

    def block(self, p, q=None, pm=None):
        """query rows and window centres of problem p"""
        return (np.roll(self.q if q is None else q, p * ROLL, 0), np.roll(self.pm if pm is None else pm, p * ROLL, 0))

    def run(self, B, window, first=0, flags=None, prev_out=True, in_place=False, q=None, pm=None, tg=None, th_low=RI.TH_LOW, ratio=0.9, fill=None):
        """problems first .. first + B - 1 -> (outputs per problem, raw bytes of the output buffer, workspace header ints [B][4])"""
        nf, ctx = self.nf, self.ctx
        blocks = [self.block(first + p, q, pm) for p in range(B)]
        dq = self.dev(np.ascontiguousarray(np.concatenate([b[0] for b in blocks]), F))
        pmh = np.ascontiguousarray(np.concatenate([b[1] for b in blocks]), F)
        # (the in-place run: the centres sit in a buffer of their own with guard bytes around them)
        dpm = guarded.Guarded(pmh.nbytes, GUARD, inner=pmh, what="prev_matched")
        dfl = self.dev(np.ascontiguousarray(np.concatenate([np.roll(flags, (first + p) * ROLL) for p in range(B)]), np.uint8)) if flags is not None else None
        dtg = self.dev(np.ascontiguousarray(tg, F)) if tg is not None else self.dtg
        lay = Context.init_search_layout(B, nf, nf, GUARD)
        out = guarded.outputs(lay)
        wsb = Context.init_search_workspace_bytes(nf, nf, B)
        ws = guarded.Guarded(wsb, GUARD, inner=fill)
        # every problem searches frame 1: its grid blob B times over, one set of rows (stride 0) and of coordinates per problem
        g = self.fin[3].download(np.uint8, ctx.grid_bytes(nf), ctx.grid_bytes(nf))
        dg = self.dev(np.tile(g, B))
        dxy = self.dev(np.tile(self.xy[1].reshape(-1), B)) if prev_out else None
        ctx.init_search_device(B, nf, dq.ptr, dpm.ptr, dg.ptr, dtg.ptr, 0, nf, ws.ptr, out.ptr, window=window, d_query_flags=dfl.ptr if dfl else None,
                               d_target_xy=dxy.ptr if dxy else None, d_prev_out=dpm.ptr if in_place else None, th_low=th_low, nn_ratio=ratio, guard=GUARD)
        ctx.synchronize()
        own = prev_out and not in_place                                # prev_out is written into the layout's own array
        raw = guarded.download(out, lay, skip=() if own else ("prev_out",))
        pmr = dpm.download()
        a = lay.parse(raw)
        if in_place:
            a["prev_out"] = pmr.view(F).reshape(B, nf, 2)
        else:
            assert pmr.tobytes() == pmh.tobytes(), "prev_matched was written"
        res = guarded.problems(a, B, [k for k in a if k != "prev_out" or prev_out or in_place])
        wraw = ws.download()
        hdr = np.stack([wraw[p * (wsb // B):p * (wsb // B) + 16].view(np.int32) for p in range(B)])
        out.free(); ws.free(); dpm.free()
        for b in self.bufs:
            b.free()
        self.bufs = []
        return res, raw, hdr

    def model(self, p, window, flags=None, q=None, pm=None, tg=None, th_low=RI.TH_LOW, ratio=0.9, form=RI.literal):
        """the restatement of problem p"""
        qq, pp = self.block(p, q, pm)
        fl = None if flags is None else np.roll(flags, p * ROLL)
        return form(self.O, qq, pp, window, self.grid, self.x, self.y, self.bounds, self.tg if tg is None else tg, flags=fl, th_low=th_low, nn_ratio=ratio,
                    txy=self.xy[1])

    def kps(self, f):
        k = np.zeros(self.nf, capi.KP_DTYPE); k["x"] = self.xy[f][:, 0]; k["y"] = self.xy[f][:, 1]
        return k

    def close(self):
        for x in (self.din, self.rec, self.dtg) + tuple(b for b in self.fin if b is not None):
            x.free()
        self.ctx.close()


def cpu_frames(O, blob_weights, nf, seed):
    """the two frames from the CPU oracle's extraction (tests/test_init_ref.py): undistorted keypoints, rows, valid mask of frame 0, bounds"""
    cam = RF.camera()
    orc = O.Oracle(blob_weights)
    img = synth.image(H, W, seed)
    out = []
    for im in (img, RI.warp(img)):
        k, d, nv, mono = orc.extract(im, nf, (0, 0))
        out.append((RF.undistort(cam, np.stack([k["x"], k["y"]], 1)), d, RW.valid_slots(nf, nv, mono)))
    return out, tuple(float(v) for v in RF.bounds(cam))
