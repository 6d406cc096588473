"""The extraction tail of the HIP path (k_nms_score, k_select, k_select_generic, k_desc) against the float64 reference
(tests/fp64_tail.py) on both sides of the launch predicates the layer matrix (tests/test_gpu_layers.py, nfeatures = 512) does not
cross.  Each case asserts from the record header or the sizes that it crossed its predicate:

  k_select (nfeatures <= 4096)           C <= 4096 with a cut (nf = 333) | C > 4096 (VGA, nf = 1000) | C < nf (padding slots,
                                         nf = 1000) | nf = 1 | XFH_SELECT_LEGACY=1 with C > 4096 (radix select + bitonic sort)
  k_select_generic (nfeatures > 4096)    4096 < C <= 16384: the bitonic sort in LDS (VGA, nf = 8000) | C > 16384: the bitonic sort
                                         in global memory (720p, nf = 8000, two frames)
  placement                              lapping bounds on keypoint columns (inclusive at both ends) | the rescale flag at
                                         170x230 (rw != 1)
  record producers                       xfh_extract (submit / collect: the host writes the padding) | the device-resident call that
                                         also emits the prepared match images (bit for bit the image of the record's rows)
  k_nms_score                            <true> (B <= 8) everywhere else | <false> at B <= 8 with XFH_NO_NMS_HEAT=1

Every call gets frames no earlier call has seen.  The log prints max err/tol per stage, the candidate counts and the accepted
near-ties.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import fp64_tail as FT
from fp64_layers import Report
from xfeatslam_amd import capi, synth, weights as WT
from xfeatslam_amd.extractor import Context

pytestmark = pytest.mark.gpu

REPORT = Report()
IMG_FAMILIES = ("noise", "steps", "blobs", "lowcontrast", "checker4", "gradient")
_seed = [5000]
_t0 = time.time()


def _frames(B, H, W):
    _seed[0] += 131
    s = _seed[0]
    return np.stack([synth.image(H, W, s + b) if b % 2 == 0 else synth.image_family(IMG_FAMILIES[(s + b) % len(IMG_FAMILIES)], H, W, s + b)
                     for b in range(B)])


def _ctx(nf, H, W, B, family="normal", flags=0):
    ctx = Context(nfeatures=nf, max_height=H, max_width=W, max_batch=B, flags=flags)
    ctx.load_weights(WT.pack_blob(WT.make_family(family, 5)))
    return ctx


def _getter(ctx, b):
    return lambda name: ctx.debug_tensor(capi.T[name], b)


def _check(case, get_of, recs, nf, lap, shape0, rescale=False, padding=True):
    """the tail of every frame; returns the TailChecks"""
    out = []
    for b, rec in enumerate(recs):
        tc = FT.check_frame(get_of(b), rec, nf, lap, shape0, rescale, padding, REPORT, case, b)
        print(f"{case} frame {b}: C = {tc.n_candidates}  N = {len(tc.ss)}  n_valid = {tc.n_valid}  mono = {tc.mono}  "
              f"near-ties = {tc.near_ties}")
        out.append(tc)
    for line in REPORT.lines(case):
        print(line)
    bad = [(c, s, v) for (c, s), v in REPORT.failures() if c == case]
    assert not bad, "bound exceeded:\n" + "\n".join(Report.fmt(*x) for x in bad)
    return out


SELECT_CASES = [
    # (case, H, W, B, nf, family, predicate on (C, nf))
    ("select-C<=4096-cut-nf333", 170, 230, 2, 333, "normal", lambda C, nf: nf < C <= 4096),
    ("select-padding-nf1000", 96, 128, 2, 1000, "normal", lambda C, nf: C < nf),
    ("select-nf1", 96, 160, 1, 1, "peaky", lambda C, nf: C > nf),
    ("select-C>4096-nf1000", 480, 640, 1, 1000, "normal", lambda C, nf: C > 4096),
    ("generic-lds-4096<C<=16384-nf8000", 480, 640, 1, 8000, "normal", lambda C, nf: 4096 < C <= 16384),
    ("generic-global-C>16384-nf8000", 720, 1280, 2, 8000, "normal", lambda C, nf: C > 16384),
]


@pytest.mark.parametrize("case,H,W,B,nf,family,crosses", SELECT_CASES, ids=[c[0] for c in SELECT_CASES])
def test_select_forms(gpu_lib, case, H, W, B, nf, family, crosses):
    ctx = _ctx(nf, H, W, B, family)
    try:
        lap = (W // 3, W // 2)
        recs = ctx.extract_batch(_frames(B, H, W), lap)
        tcs = _check(case, lambda b: _getter(ctx, b), recs, nf, lap, (H, W))
    finally:
        ctx.close()
    for tc in tcs:
        assert crosses(tc.n_cand, nf), (case, tc.n_cand, nf)
        assert tc.n_cand == tc.n_candidates


def test_lapping_bounds_on_keypoint_columns(gpu_lib, oracle_mod):
    """lap0 and lap1 on columns of valid keypoints (found first by the oracle on the same frames, CPU): both ends are inclusive"""
    H, W, B, nf = 170, 230, 2, 512
    fr = _frames(B, H, W)
    blob = WT.pack_blob(WT.make_family("normal", 5))
    kps, _, nv, _ = oracle_mod.Oracle(blob).extract(fr[0], nf, (0, 0))
    xs = np.unique(kps["x"][:nv].astype(np.int64))
    lap = (int(xs[len(xs) // 3]), int(xs[2 * len(xs) // 3]))
    ctx = _ctx(nf, H, W, B)
    try:
        recs = ctx.extract_batch(fr, lap)
        tcs = _check("lapping-on-columns", lambda b: _getter(ctx, b), recs, nf, lap, (H, W))
    finally:
        ctx.close()
    tc = tcs[0]
    for x in lap:
        assert ((tc.sx == x) & (tc.ss > 0)).any(), (lap, x)
    assert 0 < tc.mono < tc.n_valid


def test_rescale_flag(gpu_lib):
    H, W, B, nf = 170, 230, 2, 700
    assert W // 32 * 32 != W and H // 32 * 32 != H
    lap = (60, 140)
    ctx = _ctx(nf, H, W, B, flags=capi.FLAG_RESCALE_KEYPOINTS)
    try:
        recs = ctx.extract_batch(_frames(B, H, W), lap)
        tcs = _check("rescale-170x230", lambda b: _getter(ctx, b), recs, nf, lap, (H, W), rescale=True)
    finally:
        ctx.close()
    assert tcs[0].rw != 1 and tcs[0].rh != 1
    assert any(0 < tc.mono < tc.n_valid for tc in tcs)


def test_submit_collect_path(gpu_lib):
    """xfh_extract (submit + collect): k_desc leaves the padding slots alone (write_padding = 0), the host writes them"""
    H, W, nf = 96, 128, 600
    lap = (30, 70)
    ctx = _ctx(nf, H, W, 1)
    try:
        img = _frames(1, H, W)[0]
        kps = np.zeros(nf, capi.KP_DTYPE)
        kps["x"] = 123.0                                   # must be overwritten
        desc = np.full((nf, 64), 7.0, np.float32)
        import ctypes as C
        nv, mono = C.c_int(-1), C.c_int(-1)
        capi.check(capi.lib().xfh_extract(ctx.h, img.ctypes.data, H, W, W, lap[0], lap[1], kps.ctypes.data, desc.ctypes.data,
                                          C.byref(nv), C.byref(mono)), ctx.h)
        tcs = _check("submit-collect", lambda b: _getter(ctx, b), [(kps, desc, nv.value, mono.value, None)], nf, lap, (H, W))
    finally:
        ctx.close()
    assert tcs[0].n_candidates < nf and tcs[0].n_valid < nf                        # padding slots exist


def test_device_path_with_match_images(gpu_lib):
    """xfh_extract_batch_device_images: the records, and the prepared match image of every frame is bit for bit the image
    xfh_match_prepare_device makes of the record's descriptor rows (nf = 500: padding slots, and rows up to the panel boundary)"""
    L = capi.lib()
    H, W, B, nf = 96, 128, 2, 500
    lap = (20, 64)
    ctx = _ctx(nf, H, W, B)
    try:
        fr = _frames(B, H, W)
        rb, ib = ctx.rec_bytes, int(L.xfh_match_image_bytes(nf))
        d_in = capi.DeviceBuffer(fr.nbytes).upload(fr)
        d_rec, d_img, d_one = capi.DeviceBuffer(B * rb), capi.DeviceBuffer(B * ib), capi.DeviceBuffer(ib)
        capi.check(L.xfh_extract_batch_device_images(ctx.h, d_in.ptr, B, H, W, lap[0], lap[1], d_rec.ptr, d_img.ptr), ctx.h)
        ctx.synchronize()
        recs = ctx.parse_records(d_rec.download(np.uint8, B * rb), B)
        _check("device-images", lambda b: _getter(ctx, b), recs, nf, lap, (H, W))
        imgs = d_img.download(np.uint8, B * ib).reshape(B, ib)
        for b in range(B):
            capi.check(L.xfh_match_prepare_device(ctx.h, d_rec.ptr + b * rb + ctx.desc_off, nf, d_one.ptr), ctx.h)
            ctx.synchronize()
            assert np.array_equal(imgs[b], d_one.download(np.uint8, ib)), b
        assert any(r[2] < nf for r in recs)
        for buf in (d_in, d_rec, d_img, d_one):
            buf.free()
    finally:
        ctx.close()


KNOB_CASES = [
    # (knob, H, W, B, nf, predicate on (C, nf))
    ("XFH_SELECT_LEGACY", 480, 640, 1, 1000, lambda C, nf: C > 4096),
    ("XFH_NO_NMS_HEAT", 170, 230, 3, 512, lambda C, nf: C > 0),
]


@pytest.mark.parametrize("knob,H,W,B,nf,crosses", KNOB_CASES, ids=[c[0] for c in KNOB_CASES])
def test_tail_under_knob(gpu_lib, tmp_path, knob, H, W, B, nf, crosses):
    """the radix-select + bitonic form of k_select, and k_nms_score<false> with k_heads_heat at B <= 8: the knobs exist in the
    debug build only, so the extraction runs in a fresh worker process that loads it; the check runs here"""
    assert os.path.exists(capi.KNOBS_LIB_PATH), "run `make -C xfeatslam_amd/csrc knobs` (or __graft_entry__.build())"
    fr = _frames(B, H, W)
    lap = (W // 4, W // 2)
    np.save(tmp_path / "frames.npy", fr)
    out = tmp_path / "out.npz"
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "workers", "tail_worker.py")
    env = dict(os.environ, XFEAT_HIP_LIB=capi.KNOBS_LIB_PATH, **{knob: "1"})
    r = subprocess.run([sys.executable, worker, str(tmp_path / "frames.npy"), str(out), str(nf), str(lap[0]), str(lap[1]), "normal"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (knob, r.returncode, r.stderr[-2000:])
    z = np.load(out)
    ctx = Context.__new__(Context)                        # record layout only: no device context
    ctx.nfeatures, ctx.rec_bytes = nf, int(capi.lib().xfh_record_bytes(nf))
    ctx.kps_off, ctx.desc_off = int(capi.lib().xfh_record_kps_offset()), int(capi.lib().xfh_record_desc_offset(nf))
    recs = Context.parse_records(ctx, z["records"], B)
    tcs = _check(f"knob-{knob}", lambda b: (lambda name: z[f"{name}_{b}"]), recs, nf, lap, (H, W))
    for tc in tcs:
        assert crosses(tc.n_cand, nf), (knob, tc.n_cand)


def test_zz_tail_margins():
    """worst err/tol per tail stage over every case above (runs last in this module), and the module's wall time"""
    print(f"\nworst err/tol per stage over {len({c for c, _ in REPORT.rows})} cases:")
    for st, (case, v) in sorted(REPORT.worst_by_stage().items(), key=lambda kv: FT.STAGES.index(kv[0])):
        print(Report.fmt(case, st, v))
    print(f"test_gpu_tail wall time {time.time() - _t0:.1f} s")
    REPORT.assert_ok()
