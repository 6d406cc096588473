"""xfh_frame_finish_records_device (k_frame_finish) against the numpy restatement tests/ref_frame.py, stage by stage: every stage
is compared with the model evaluated on the DEVICE's own previous stage, so one failure names one stage.  Records come from real
extractions of seeded frames, depth images are seeded uint16 with about a third zeros and their fp32 conversions.  Every
comparison is equality of bits."""
import ctypes as C

import numpy as np
import pytest

import ref_frame as RF
import ref_window as RW
from xfeatslam_amd import capi, synth
from xfeatslam_amd.extractor import Context

pytestmark = pytest.mark.gpu

F = np.float32
H, W = 480, 640
SCALE = F(1) / F(RF.TUM1_DEPTH_FACTOR)
TUM1 = RF.camera()


def cam_struct(c):
    return capi.Camera(*[float(c[k]) for k in "fx fy cx cy k1 k2 p1 p2 k3 bf".split()], int(c["width"]), int(c["height"]))


def depth_images(B, seed, h=H, w=W, pitch_elems=None):
    """[B][h][pitch] raw uint16 with about a third zeros (the columns past w hold a value no test may see), and the fp32 conversion"""
    rng = np.random.RandomState(seed)
    pe = pitch_elems or w
    raw = np.full((B, h, pe), 0xBEEF, np.uint16)
    img = rng.randint(1, 65536, (B, h, w)).astype(np.uint16)
    img[rng.rand(B, h, w) < 1 / 3] = 0
    raw[:, :, :w] = img
    return raw, (raw.astype(F) * SCALE).astype(F)


class Rig:
    """a ctx, B extracted records in device memory and their host copies"""

    def __init__(self, L, blob, nf, B, lap, max_batch=None, h=H, w=W, seed=900):
        self.L, self.nf, self.B, self.h, self.w = L, nf, B, h, w
        self.cw = w                                                    # columns of the depth image the camera sees (its width)
        self.ctx = Context(nfeatures=nf, max_height=h, max_width=w, max_batch=max_batch or B)
        self.ctx.load_weights(blob)
        frames = np.stack([synth.image(h, w, seed + i) for i in range(B)])
        self.din = capi.DeviceBuffer(frames.nbytes).upload(frames)
        self.rec = capi.DeviceBuffer(B * self.ctx.rec_bytes)
        capi.check(L.xfh_extract_batch_device(self.ctx.h, self.din.ptr, B, h, w, lap[0], lap[1], self.rec.ptr), self.ctx.h)
        self.ctx.synchronize()
        self.recs = self.ctx.parse_records(self.rec.download(np.uint8, B * self.ctx.rec_bytes), B)

    def xy(self, b):
        k = self.recs[b][0]
        return np.stack([k["x"], k["y"]], 1).astype(F)

    def finish(self, cam, bounds, flags=0, depth=None, scale=1.0, grid=True, B=None):
        """-> xy_un [B][n][2], uright [B][n], depth [B][n], blobs [B][grid_bytes] (or None)"""
        B = B or self.B
        d = None if depth is None else capi.DeviceBuffer(depth.nbytes).upload(depth)
        dt = capi.DEPTH_NONE if depth is None else (capi.DEPTH_U16 if depth.dtype == np.uint16 else capi.DEPTH_F32)
        out = self.ctx.frame_finish_records(self.rec.ptr, B, cam_struct(cam), bounds, flags, d.ptr if d else None, dt,
                                            depth.strides[1] if depth is not None else 0, scale, grid)
        self.ctx.synchronize()
        nf = self.nf
        res = (out[0].download(F, B * nf * 2).reshape(B, nf, 2), out[1].download(F, B * nf).reshape(B, nf), out[2].download(F, B * nf).reshape(B, nf),
               out[3].download(np.uint8, B * self.ctx.grid_bytes(nf)).reshape(B, -1) if grid else None)
        for x in out + (d,):
            if x is not None:
                x.free()
        return res

    def close(self):
        self.din.free(); self.rec.free(); self.ctx.close()


def check_stages(rig, cam, bounds, res, depth, scale, flags=0, B=None):
    xy_un, ur, dz, blobs = res
    for b in range(B or rig.B):
        kps, _, nv, mono, _ = rig.recs[b]
        raw = rig.xy(b)
        assert RF.same_bits(xy_un[b], RF.undistort(cam, raw)), ("undistort", b)
        md, mr = RF.stereo(cam, raw, xy_un[b], None if depth is None else depth[b][:, :rig.cw], scale)      # on the DEVICE's xy_un
        assert RF.same_bits(dz[b], md), ("depth", b, np.nonzero(dz[b] != md)[0][:8])
        assert RF.same_bits(ur[b], mr), ("uright", b, np.nonzero(ur[b] != mr)[0][:8])
        if blobs is not None:
            use = RW.valid_slots(rig.nf, nv, mono) if flags else None
            rcs, ritems = RF.grid(xy_un[b], bounds, use)                                                    # on the DEVICE's xy_un
            cs, items = rig.ctx.grid_unpack(blobs[b], rig.nf)
            assert np.array_equal(cs, rcs) and np.array_equal(items, ritems), ("grid", b)
            assert np.array_equal(blobs[b], RW.make_blob(rcs, ritems, rig.nf, xy_un[b][:, 0].copy(), xy_un[b][:, 1].copy(), bounds, flags)), ("blob", b)


@pytest.mark.parametrize("lap", [(0, 0), (0, 1000)])
@pytest.mark.parametrize("nf", [1000, 4096])
@pytest.mark.parametrize("B,max_batch", [(1, 8), (5, 8), (8, 8)])          # B = 1, 5 and max_batch
def test_finish_matches_model_stage_by_stage(gpu_lib, weights_dense, B, max_batch, nf, lap):
    rig = Rig(gpu_lib, weights_dense[1], nf, B, lap, max_batch)
    bounds = Context.camera_bounds(cam_struct(TUM1))
    assert RF.same_bits(np.array(bounds, F), np.array(RF.bounds(TUM1), F))
    raw, f32 = depth_images(B, 31 + B)
    nv = [r[2] for r in rig.recs]
    print(f"B={B} nf={nf} lap={lap}: n_valid {min(nv)}..{max(nv)}")
    assert min(nv) > nf // 4                                        # real keypoints, and (nf = 4096) padding slots as well
    for depth, scale in ((raw, SCALE), (f32, 1.0)):
        res = rig.finish(TUM1, bounds, 0, depth, scale)
        check_stages(rig, TUM1, bounds, res, depth, scale)
        assert (res[2] > 0).mean() > 0.4 and (res[2] == -1).mean() > 0.15      # both branches of d > 0
    # the depth-stage mistakes the CPU test lists differ from the device on this data
    xy_un, ur, dz, _ = res
    for cor in ("depth_at_undistorted", "uright_from_raw", "d_ge_0"):
        md, mr = RF.stereo(TUM1, rig.xy(0), xy_un[0], f32[0], 1.0, corrupt=cor)
        assert not (RF.same_bits(md, dz[0]) and RF.same_bits(mr, ur[0])), cor
    res16 = rig.finish(TUM1, bounds, 0, raw, SCALE)
    md, mr = RF.stereo(TUM1, rig.xy(0), res16[0][0], raw[0], SCALE, corrupt="scale_f64")
    assert not RF.same_bits(md, res16[2][0])
    rig.close()


def test_k1_zero_is_the_merged_grid_build(gpu_lib, weights_dense):
    """k1 = 0 (the other coefficients non-zero): xy_un is the record's keypoints bit for bit, and the blob is byte for byte the one
    xfh_grid_build_records_device writes for the same records and bounds"""
    rig = Rig(gpu_lib, weights_dense[1], 4096, 3, (0, 0))
    cam = RF.camera(k1=0.0)
    bounds = Context.camera_bounds(cam_struct(cam))
    assert bounds == (0.0, 0.0, 640.0, 480.0)
    gb = rig.ctx.grid_bytes(rig.nf)
    for flags in (0, capi.GRID_SKIP_PADDING):
        xy_un, ur, dz, blobs = rig.finish(cam, bounds, flags)
        grids = rig.ctx.grid_build_records(rig.rec.ptr, rig.B, bounds, flags)
        rig.ctx.synchronize()
        ref = grids.download(np.uint8, rig.B * gb).reshape(rig.B, gb)
        grids.free()
        for b in range(rig.B):
            assert np.array_equal(xy_un[b].view(np.uint32), rig.xy(b).view(np.uint32))
            assert np.array_equal(blobs[b], ref[b]), (flags, b)
        assert np.all(ur == -1) and np.all(dz == -1)
    rig.close()


def test_options_and_padding(gpu_lib, weights_dense):
    nf = 4096
    # 240 x 320 frames cannot fill 4096 slots, so the records carry padding; their keypoints are keypoints of the TUM1 camera's
    # 480 x 640 image all the same (its upper left quarter), and the depth images have the camera's size
    rig = Rig(gpu_lib, weights_dense[1], nf, 2, (0, 0), h=240, w=320)
    rig.cw = W
    cs_cam = cam_struct(TUM1)
    bounds = Context.camera_bounds(cs_cam)
    raw, f32 = depth_images(2, 77, pitch_elems=W + 24)                            # a pitch wider than the row
    valid = [RW.valid_slots(nf, r[2], r[3]) for r in rig.recs]
    assert all((~v).sum() > 0 for v in valid)
    # padding slots: undistorted like any point, depth sampled at pixel (0, 0), binned in the cell of undistorted (0, 0)
    p0 = RF.undistort(TUM1, [[0, 0]])[0]
    px, py, ok = RW.cell_of(p0[:1], p0[1:], bounds)
    cell = int(px[0]) * 48 + int(py[0])
    assert ok[0] and cell != 0                                                    # not the cell (0, 0) of the raw grid
    for depth, scale in ((raw, SCALE), (f32, 1.0)):
        res = rig.finish(TUM1, bounds, 0, depth, scale)
        check_stages(rig, TUM1, bounds, res, depth, scale)
        for b in range(2):
            pad = np.nonzero(~valid[b])[0]
            assert RF.same_bits(res[0][b][pad], np.tile(p0, (len(pad), 1)))
            d00, r00 = RF.stereo(TUM1, [[0, 0]], [p0], depth[b][:, :W], scale)
            assert RF.same_bits(res[2][b][pad], np.full(len(pad), d00[0], F)) and RF.same_bits(res[1][b][pad], np.full(len(pad), r00[0], F))
            cs, items = rig.ctx.grid_unpack(res[3][b], nf)
            assert np.all(np.isin(pad, items[cs[cell]:cs[cell + 1]]))
        # XFH_GRID_SKIP_PADDING: out of the grid, side arrays unchanged
        res_s = rig.finish(TUM1, bounds, capi.GRID_SKIP_PADDING, depth, scale)
        check_stages(rig, TUM1, bounds, res_s, depth, scale, capi.GRID_SKIP_PADDING)
        assert all(RF.same_bits(a, b) for a, b in zip(res[:3], res_s[:3]))
        for b in range(2):
            cs, items = rig.ctx.grid_unpack(res_s[3][b], nf)
            assert not np.isin(np.nonzero(~valid[b])[0], items).any()
        # d_grids = NULL: side arrays only, the same values
        res_n = rig.finish(TUM1, None, 0, depth, scale, grid=False)
        assert all(RF.same_bits(a, b) for a, b in zip(res[:3], res_n[:3]))
    # XFH_DEPTH_NONE: the monocular constructor
    res = rig.finish(TUM1, bounds)
    check_stages(rig, TUM1, bounds, res, None, 1.0)
    assert np.all(res[1] == -1) and np.all(res[2] == -1)
    # B smaller than max_batch
    res1 = rig.finish(TUM1, bounds, 0, raw, SCALE, B=1)
    check_stages(rig, TUM1, bounds, res1, raw, SCALE, B=1)
    # the host-pointer convenience form
    xy, ur, dz = rig.ctx.frame_finish(rig.recs[1][0], cs_cam, raw[1], SCALE)
    full = rig.finish(TUM1, bounds, 0, raw, SCALE)
    assert RF.same_bits(xy, full[0][1]) and RF.same_bits(ur, full[1][1]) and RF.same_bits(dz, full[2][1])
    xy, ur, dz = rig.ctx.frame_finish(rig.recs[1][0], cs_cam)
    assert RF.same_bits(xy, full[0][1]) and np.all(ur == -1) and np.all(dz == -1)
    # the ctx reused at a smaller image size
    h2, w2 = 192, 256
    frames = np.stack([synth.image(h2, w2, 5 + i) for i in range(2)])
    rig.din.upload(frames)
    capi.check(gpu_lib.xfh_extract_batch_device(rig.ctx.h, rig.din.ptr, 2, h2, w2, 0, 0, rig.rec.ptr), rig.ctx.h)
    rig.ctx.synchronize()
    rig.recs = rig.ctx.parse_records(rig.rec.download(np.uint8, 2 * rig.ctx.rec_bytes), 2)
    rig.h, rig.w, rig.cw = h2, w2, w2
    small = RF.camera(fx=206.9, fy=206.6, cx=127.5, cy=102.1, width=w2, height=h2)
    sb = Context.camera_bounds(cam_struct(small))
    raw2, _ = depth_images(2, 78, h2, w2)
    res = rig.finish(small, sb, 0, raw2, SCALE)
    check_stages(rig, small, sb, res, raw2, SCALE)
    rig.close()


def test_depth_sampling_edges_on_the_device(gpu_lib):
    """an 8 x 6 depth image whose values name their pixel, sampled at the image's edges: the last row and column, (-1, 0) truncating
    to pixel 0, the first coordinate outside on either side, non-finite and huge ones; both depth types, k1 = 0 so u' = u"""
    cam = RF.camera(width=8, height=6, k1=0.0, bf=2.0)
    img = (np.arange(48, dtype=np.uint16).reshape(6, 8) + 1)
    xy = np.array([[0, 0], [7.9, 5.9], [-0.5, -0.99], [8, 0], [0, 6], [-1, 0], [np.nan, 1], [1, np.inf], [1e30, 1], [3.7, 2.2], [7, 5], [7.99, 0]], F)
    want = np.array([1, 48, 1, -1, -1, -1, -1, -1, -1, 20, 48, 8], F)
    k = np.zeros(len(xy), capi.KP_DTYPE); k["x"] = xy[:, 0]; k["y"] = xy[:, 1]
    ctx = Context(nfeatures=16, max_height=32, max_width=32)
    for depth, scale in ((img, 1.0), (img.astype(F), 1.0), (img, 0.5)):
        un, ur, dz = ctx.frame_finish(k, cam_struct(cam), depth, scale)
        assert RF.same_bits(un, xy)
        w = np.where(want > 0, want * F(scale), want).astype(F)
        assert RF.same_bits(dz, w), (dz, w)
        md, mr = RF.stereo(cam, xy, un, depth, scale)
        assert RF.same_bits(dz, md) and RF.same_bits(ur, mr)
        assert ur[0] == F(0) - F(2.0) / w[0] and ur[3] == -1
    ctx.close()


def test_chain_extract_finish_search(gpu_lib, oracle_mod, weights_dense):
    """extract two frames -> finish both -> search frame 1 with frame 0's undistorted keypoints, descriptors and uright: device
    pointers only between the calls.  Equals ref_window + the best-two oracle on host copies, all five arrays; and the grid of the
    RAW keypoints gives other candidate counts, so the inputs do exercise distortion."""
    L = gpu_lib
    nf = 1000
    ctx = Context(nfeatures=nf, max_height=H, max_width=W, max_batch=2)
    ctx.load_weights(weights_dense[1])
    f0 = synth.image(H, W, 8)
    frames = np.stack([f0, np.roll(f0, (1, 2), (0, 1))])
    din = capi.DeviceBuffer(frames.nbytes).upload(frames)
    rec = capi.DeviceBuffer(2 * ctx.rec_bytes)
    # depth in 8 x 8 blocks: none, 1 m, 2 m (disparities of 40 and 20 pixels: further apart than r), so a keypoint and its
    # neighbour two pixels on mostly share a depth while the window holds candidates of both
    yy, xx = np.mgrid[0:H, 0:W]
    raw = np.stack([np.array([0, 5000, 10000], np.uint16)[(xx // 8 + yy // 8) % 3]] * 2)
    dd = capi.DeviceBuffer(raw.nbytes).upload(raw)
    cam = cam_struct(TUM1)
    bounds = Context.camera_bounds(cam)
    uvr_d = capi.DeviceBuffer(nf * 12); out = capi.DeviceBuffer(nf * 20)
    r = 15.0
    # the chain: asynchronous calls on the ctx stream, no synchronisation between them.  (u, v, r) is assembled on the device from
    # xy_un in a real tracker; here it is uploaded after a first pass, as in test_extract_to_search_stays_on_the_device
    capi.check(L.xfh_extract_batch_device(ctx.h, din.ptr, 2, H, W, 0, 0, rec.ptr), ctx.h)
    fin = ctx.frame_finish_records(rec.ptr, 2, cam, bounds, 0, dd.ptr, capi.DEPTH_U16, 2 * W, SCALE)
    ctx.synchronize()
    xy0 = fin[0].download(F, nf * 2).reshape(nf, 2)
    uvr = np.concatenate([xy0, np.full((nf, 1), r, F)], 1).astype(F)
    uvr_d.upload(uvr)
    capi.check(L.xfh_extract_batch_device(ctx.h, din.ptr, 2, H, W, 0, 0, rec.ptr), ctx.h)
    ctx.frame_finish_records(rec.ptr, 2, cam, bounds, 0, dd.ptr, capi.DEPTH_U16, 2 * W, SCALE, out=fin)
    gb = ctx.grid_bytes(nf)
    ctx.search_window_device(rec.ptr + ctx.desc_off, uvr_d.ptr, nf, fin[3].ptr + gb, rec.ptr + ctx.rec_bytes + ctx.desc_off, nf, out.ptr, 256,
                             d_uright=fin[1].ptr + 4 * nf, d_ur_query=fin[1].ptr)
    ctx.synchronize()
    res = tuple(out.download(np.int32, 5 * nf).reshape(5, nf))
    (k0, d0, *_), (k1, d1, *_) = ctx.parse_records(rec.download(np.uint8, 2 * ctx.rec_bytes), 2)
    xy = fin[0].download(F, 4 * nf).reshape(2, nf, 2); ur = fin[1].download(F, 2 * nf).reshape(2, nf)
    assert RF.same_bits(xy[0], xy0)
    x1, y1 = xy[1][:, 0].copy(), xy[1][:, 1].copy()
    off, ind = RW.csr(RW.build(x1, y1, bounds), x1, y1, uvr, bounds, uright=ur[1], ur_query=ur[0])
    a = oracle_mod.best2_csr(d0, d1, off, ind, 256)
    for i in range(4):
        assert np.array_equal(res[i], a[i]), i
    assert np.array_equal(res[4], np.diff(off))
    off_nr, _ = RW.csr(RW.build(x1, y1, bounds), x1, y1, uvr, bounds)
    print(f"candidates per query {np.diff(off).mean():.2f} (without the right-coordinate check {np.diff(off_nr).mean():.2f}), matched under 256: {(res[0] >= 0).sum()}")
    assert np.diff(off).max() >= 2 and off[-1] < off_nr[-1] and (res[0] >= 0).sum() > 0
    # the same search on the grid of the RAW keypoints
    raw_b = (0.0, 0.0, float(W), float(H))
    g_raw = ctx.grid_build_records(rec.ptr, 2, raw_b, 0)
    ctx.search_window_device(rec.ptr + ctx.desc_off, uvr_d.ptr, nf, g_raw.ptr + gb, rec.ptr + ctx.rec_bytes + ctx.desc_off, nf, out.ptr, 256,
                             d_uright=fin[1].ptr + 4 * nf, d_ur_query=fin[1].ptr)
    ctx.synchronize()
    res_raw = out.download(np.int32, 5 * nf).reshape(5, nf)
    assert (res_raw[4] != res[4]).any()
    for x in (din, rec, dd, uvr_d, out, g_raw) + fin:
        x.free()
    ctx.close()


def test_invalid_arguments_leave_outputs_untouched(gpu_lib, weights_dense):
    L = gpu_lib
    rig = Rig(L, weights_dense[1], 1000, 2, (0, 0), max_batch=2, h=96, w=128)
    nf = rig.nf
    cam = RF.camera(width=128, height=96)
    gbytes = rig.ctx.grid_bytes(nf)
    sent = np.full(2 * nf * 4 * 4 + 2 * gbytes, 0xA5, np.uint8)
    o = capi.DeviceBuffer(sent.nbytes).upload(sent)
    xy, ur, dz, gr = o.ptr, o.ptr + 2 * nf * 8, o.ptr + 2 * nf * 12, o.ptr + 2 * nf * 16
    assert gr % 16 == 0
    depth = capi.DeviceBuffer(2 * 96 * 128 * 4).upload(np.zeros(2 * 96 * 128, F))
    ok_b = capi.GridBounds(0, 0, 128, 96)

    def call(rec=rig.rec.ptr, B=2, c=cam, d=depth.ptr, dt=capi.DEPTH_F32, pitch=512, b=ok_b, fl=0, xy=xy, ur=ur, dz=dz, gr=gr, ctx=rig.ctx.h):
        return L.xfh_frame_finish_records_device(ctx, rec, B, C.byref(cam_struct(c)) if c else None, d, dt, pitch, 1.0, C.byref(b) if b else None, fl, xy, ur, dz, gr)

    bad = [dict(B=0), dict(B=3), dict(B=-1), dict(pitch=508), dict(pitch=510), dict(dt=capi.DEPTH_U16, pitch=254), dict(dt=capi.DEPTH_U16, pitch=257),
           dict(c=RF.camera(width=0, height=96)), dict(c=RF.camera(width=128, height=-1)), dict(c=None), dict(dt=3), dict(dt=-1), dict(fl=2), dict(fl=4),
           dict(b=None), dict(b=capi.GridBounds(0, 0, 0, 96)), dict(b=capi.GridBounds(0, 0, float("nan"), 96)), dict(rec=None), dict(xy=None), dict(ur=None),
           dict(dz=None), dict(gr=gr + 4), dict(xy=xy + 2), dict(d=depth.ptr + 2), dict(ctx=None)]
    for kw in bad:
        assert call(**kw) == 1, kw
    rig.ctx.synchronize()
    assert np.array_equal(o.download(np.uint8, sent.nbytes), sent)
    # nfeatures > XFH_GRID_MAX_N: refused with a grid, accepted without one
    big = Context(nfeatures=capi.GRID_MAX_N + 8, max_height=32, max_width=32)
    rb = capi.DeviceBuffer(big.rec_bytes).upload(np.zeros(big.rec_bytes, np.uint8))
    ob = capi.DeviceBuffer(big.nfeatures * 16 + big.grid_bytes(big.nfeatures))
    args = (C.byref(cam_struct(cam)), None, 0, 0, 1.0, C.byref(ok_b), 0, ob.ptr, ob.ptr + big.nfeatures * 8, ob.ptr + big.nfeatures * 12)
    assert L.xfh_frame_finish_records_device(big.h, rb.ptr, 1, *args, ob.ptr + big.nfeatures * 16) == 1
    assert L.xfh_frame_finish_records_device(big.h, rb.ptr, 1, *args, None) == 0
    big.synchronize()
    p0 = RF.undistort(cam, [[0, 0]])                                               # an all-zero record: every slot is a keypoint at (0, 0)
    assert RF.same_bits(ob.download(F, big.nfeatures * 2).reshape(-1, 2), np.tile(p0, (big.nfeatures, 1))) and np.all(ob.download(F, big.nfeatures * 2, big.nfeatures * 8) == -1)
    # the valid call still works afterwards
    assert call() == 0
    rig.ctx.synchronize()
    for x in (o, depth, rb, ob):
        x.free()
    big.close(); rig.close()


def test_hostile_floats_complete_and_match_the_model(gpu_lib, weights_dense):
    """NaN / Inf / 1e30 keypoints (written into a copy of a record) and coefficients: valid launches whose bounds handling is
    checked -- every output equals the model wherever the model is finite, non-finite coordinates are not binned, depth of a
    keypoint outside the image is the 'outside' value"""
    rig = Rig(gpu_lib, weights_dense[1], 1000, 1, (0, 0))
    nf = rig.nf
    rawb = rig.rec.download(np.uint8, rig.ctx.rec_bytes)
    kps = rawb[rig.ctx.kps_off:rig.ctx.kps_off + 28 * nf].view(capi.KP_DTYPE)
    vals = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 3.4e38, -0.5, -1.0, 640.0, 639.99, 1e9, -1e9], F)
    for j in range(200):
        kps["x"][3 * j] = vals[j % len(vals)]
        kps["y"][3 * j + 1] = vals[(j // 2) % len(vals)]
    rig.rec.upload(rawb)
    rig.recs = rig.ctx.parse_records(rawb, 1)
    raw, f32 = depth_images(1, 5)
    f32[0, ::7, ::5] = np.nan; f32[0, 1::7, ::5] = np.inf; f32[0, 2::7, ::5] = -1.0                    # hostile depth values too
    bounds = Context.camera_bounds(cam_struct(TUM1))

    def check(cam, b, depth, scale):
        res = rig.finish(cam, b, 0, depth, scale)
        m_xy = RF.undistort(cam, rig.xy(0))
        fin = np.isfinite(m_xy).all(axis=1)
        assert RF.same_bits(res[0][0][fin], m_xy[fin]) and not np.isfinite(res[0][0][~fin]).all(axis=1).any()
        md, mr = RF.stereo(cam, rig.xy(0), res[0][0], depth[0], scale)
        assert RF.same_bits(res[2][0], md)
        ok = np.isfinite(mr)
        assert RF.same_bits(res[1][0][ok], mr[ok]) and not np.isfinite(res[1][0][~ok]).any()
        cs, items = rig.ctx.grid_unpack(res[3][0], nf)
        rcs, ritems = RF.grid(res[0][0], b)
        assert np.array_equal(cs, rcs) and np.array_equal(items, ritems)
        assert not np.isin(np.nonzero(~np.isfinite(res[0][0]).all(axis=1))[0], items).any()
        return res

    for depth, scale in ((raw, SCALE), (f32, 1.0)):
        res = check(TUM1, bounds, depth, scale)
        out = ~((rig.xy(0)[:, 0] > -1) & (rig.xy(0)[:, 0] < W) & (rig.xy(0)[:, 1] > -1) & (rig.xy(0)[:, 1] < H))
        assert out.sum() > 100 and np.all(res[2][0][out] == -1)                                     # outside the image: sample 0 -> -1
    for name in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "bf"):
        for v in (np.nan, np.inf, 1e30, 0.0):
            check(RF.camera(**{name: v}), bounds, raw, SCALE)
    check(TUM1, bounds, raw, F(np.nan)); check(TUM1, bounds, raw, F(np.inf))
    rig.close()
