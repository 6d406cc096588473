"""Every forward-pass stage of the HIP path against the float64 reference (tests/fp64_layers.py) under its derived bound, across the
shapes, batch regimes and BatchNorm modes that select different kernel forms.

Which case crosses which launch predicate (xfeatslam_amd/csrc/kernels_conv.hip, launch_basic_layer_t / launch_fusion_chain and
kernels_misc.hip, run_extract):
  persistent / consumer_fold (B > 8 | B <= 8)   720p B = 8 (the first call of the ctx-reuse case) | 330x420 B = 9 (persistent,
                                                k_bn_finalize, keypoint branch on the second stream, k_heads_kp, k_heads_heat)
  riders (k_conv_mfma_ride, B <= 8)             every B <= 8 case, batch and running statistics; folded riders at 96x128 B = 2
  small_batch (B <= 32: k_conv_mfma16)          96x160 B = 32 | B = 33 and 480x640 B = 64 (k_conv_mfma / _t, k_act_pyramid)
  split_channels (tiles x B <= 128)             64x32, 170x230 B = 3, 720p B = 1 at 1/32 | 720p B = 1 at 1/8 and 1/16, 480x640 B = 1
  XFH_M16_TALL (2x16 tiles x B > 256)           720p B = 1 (440), 96x160 B = 32 (384) | 480x640 B = 1 (150), 170x230 B = 3 (60)
  persistent grid cap (256 x per_cu)            480x640 B = 64, 96x160 B = 33 (grid-strided, frames that straddle a stride are
                                                checked) | 330x420 B = 9
  folded chain (3 stages, B <= 8)               96x128 B = 2 folded: heatmap_head.0 is handed on only (its map is refused and
                                                recomputed here) | 160x224 B = 12 folded (two-stage chain)
  folded BatchNorms at B > 32 / tall tiles      96x128 B = 33 folded (k_act_pyramid, k_conv_mfma_t, fused pyramid input with the
                                                bias + ReLU epilogue) | 720p B = 1 folded (k_conv_mfma16 tall tiles, folded riders)
  ctx reused at smaller sizes                   one ctx of 720x1280 x 8: 720p B8 -> 170x230 B3 -> 480x640 B1 -> 720p B2

Every checked frame's tail (tests/fp64_tail.py) is checked too, from the same device tensors and the call's records with a lapping
area: k_nms_score<true> (B <= 8) and <false> (B > 8), k_select at nfeatures = 512, k_desc with its padding slots.

Every call gets frames no earlier call of its ctx has seen (a seed per call), mixed image families and a constant frame in every
batched case, so a tensor the regime did not write, or a statistic / tile taken from the wrong frame, cannot pass.  The log prints
max err/tol per stage and case and the module's wall time.
"""
import time

import numpy as np
import pytest

import fp64_layers as F
import fp64_tail as FT
from xfeatslam_amd import capi, synth, weights as WT
from xfeatslam_amd.extractor import Context

pytestmark = pytest.mark.gpu

MODE_ID = {"batch": 0, "running": 1, "folded": 2}
IMG_FAMILIES = ("noise", "steps", "gradient", "blobs", "lowcontrast", "saturated", "checker4")
REPORT = F.Report()
_seed = [1000]
_t0 = time.time()


def _weights(family, seed, with_bn):
    if family.startswith("gain"):
        w = WT.make_synthetic(1234, float(family[4:]), with_bn=with_bn)
    else:
        w = WT.make_family(family, seed)
        if with_bn:
            bn = WT.make_synthetic(seed, 3.0, with_bn=True)
            for n, _ in WT.BN_TENSORS:
                w[n] = bn[n]
    return w


def _frames(B, H, W):
    """B frames no earlier call has seen; frame 1 (or 0 for B = 1 ... none) constant in batched calls"""
    _seed[0] += 97
    s = _seed[0]
    fr = np.stack([synth.image_family(IMG_FAMILIES[(s + b) % len(IMG_FAMILIES)], H, W, s + b) if (s + b) % 3 else synth.image(H, W, s + b)
                   for b in range(B)])
    if B > 1:
        fr[1] = 40 + s % 150
    return fr


def _check_frames(B, H, W):
    """all frames up to 12; above: first, last, the constant one and the frames holding tile number k x 256 of the grid-strided
    persistent kernels (1/4- and 1/8-resolution tile grids: 16 x 8 pixels)"""
    if B <= 12:
        return list(range(B))
    sel = {0, 1, B - 1}
    for d in (4, 8):
        nt = -(-(H // 32 * 32 // d) // 8) * -(-(W // 32 * 32 // d) // 16)
        for g in (256, 512, 768, 1024):
            if g // nt < B:
                sel.add(g // nt)
                if g % nt == 0 and g // nt > 0:
                    sel.add(g // nt - 1)
    return sorted(sel)


def _getter(ctx, b):
    def get(stage):
        tid = capi.T[stage] if stage in capi.T else (capi.T["RAW0"] + int(stage[3:]) if stage.startswith("RAW") else capi.T["STAT0"] + int(stage[4:]))
        try:
            return ctx.debug_tensor(tid, b)
        except capi.XfhError:
            return None
    return get


def run_case(ctx, case, frames, wt, mode):
    """one extract call on `ctx`, then every checked frame against the reference -- the forward pass (fp64_layers) and the tail
    from the same tensors and the call's records (fp64_tail: NMS, scores, selection, record, descriptors); returns the stages the
    call refused"""
    B, H, W = frames.shape
    lap = (W // 4, W // 2)                                  # a lapping area: front and back slots
    recs = ctx.extract_batch(frames, lap)
    refused = set()
    ties = []
    for b in _check_frames(B, H, W):
        get = _getter(ctx, b)
        fc = F.FrameCheck(get, frames[b], wt, mode, REPORT, case, b)
        fc.run()
        refused |= set(fc.missing)
        with pytest.raises(capi.XfhError):
            ctx.debug_tensor(capi.T["RAW0"], b)             # block1.0's map is never written
        tc = FT.check_frame(get, recs[b], ctx.nfeatures, lap, (H, W), report=REPORT, case=case, frame=b)
        ties.append(f"{b}:C={tc.n_candidates},N={len(tc.ss)},near-ties={tc.near_ties}")
    print(f"{case}: tail " + " ".join(ties))
    for line in REPORT.lines(case):
        print(line)
    bad = [(c, s, v) for (c, s), v in REPORT.failures() if c == case]
    assert not bad, "bound exceeded:\n" + "\n".join(F.Report.fmt(*x) for x in bad)
    return refused


CASES = [
    # (case, H, W, B, mode, weights)
    ("720p-b1-normal", 720, 1280, 1, "batch", "normal"),
    ("720p-b2-heavy", 720, 1280, 2, "batch", "heavy"),
    ("1080p-b1-scaled", 1080, 1920, 1, "batch", "scaled"),
    ("170x230-b3-dc", 170, 230, 3, "batch", "dc"),
    ("330x420-b9-heat_denormal", 330, 420, 9, "batch", "heat_denormal"),
    ("64x32-b1-pruned", 64, 32, 1, "batch", "pruned"),
    ("96x160-b32-peaky", 96, 160, 32, "batch", "peaky"),
    ("96x160-b33-peaky", 96, 160, 33, "batch", "peaky"),
    ("480x640-b64-gain6", 480, 640, 64, "batch", "gain6"),
    ("160x224-b2-running", 160, 224, 2, "running", "uniform"),
    ("160x224-b12-running", 160, 224, 12, "running", "uniform"),
    ("96x128-b2-folded", 96, 128, 2, "folded", "uniform"),
    ("96x128-b12-folded", 96, 128, 12, "folded", "uniform"),
    ("160x224-b2-folded", 160, 224, 2, "folded", "uniform"),
    ("160x224-b12-folded", 160, 224, 12, "folded", "uniform"),
    ("96x128-b33-folded", 96, 128, 33, "folded", "uniform"),
    ("720p-b1-folded", 720, 1280, 1, "folded", "uniform"),
]


def _expected_refusals(B, mode):
    # block1.0's map is never written (block1.1 recomputes it); heatmap_head.0 with folded BatchNorms at B <= 8: block_fusion.2 ->
    # heatmap_head.0 -> heatmap_head.1 in one kernel, the middle map is handed on in LDS only
    return {"RAW0", "RAW18"} if mode == "folded" and B <= 8 else {"RAW0"}


@pytest.mark.parametrize("case,H,W,B,mode,fam", CASES, ids=[c[0] for c in CASES])
def test_layers_match_fp64(gpu_lib, case, H, W, B, mode, fam):
    w = _weights(fam, 5, mode != "batch")
    wt = WT.unpack_blob(WT.pack_blob(w))
    ctx = Context(nfeatures=512, max_height=H, max_width=W, max_batch=B, bn_mode=MODE_ID[mode])
    try:
        ctx.load_weights(WT.pack_blob(w))
        refused = run_case(ctx, case, _frames(B, H, W), wt, mode)
        assert refused == _expected_refusals(B, mode), refused
    finally:
        ctx.close()


def test_one_ctx_at_changing_sizes(gpu_lib):
    """strides come from the ctx's maximum size, map sizes and partial counts from the call: a ctx of 720x1280 x 8 at four sizes"""
    w = _weights("normal", 6, False)
    wt = WT.unpack_blob(WT.pack_blob(w))
    ctx = Context(nfeatures=512, max_height=720, max_width=1280, max_batch=8)
    try:
        ctx.load_weights(WT.pack_blob(w))
        for k, (H, W, B) in enumerate([(720, 1280, 8), (170, 230, 3), (480, 640, 1), (720, 1280, 2)]):
            assert run_case(ctx, f"reuse{k}-{H}x{W}-b{B}", _frames(B, H, W), wt, "batch") == _expected_refusals(B, "batch")
    finally:
        ctx.close()


def test_zz_margins_over_the_matrix():
    """worst err/tol per stage over every case above (runs last in this module), and the module's wall time"""
    print(f"\nworst err/tol per stage over {len({c for c, _ in REPORT.rows})} cases:")
    for st, (case, v) in sorted(REPORT.worst_by_stage().items(), key=lambda kv: (F.STAGES + FT.STAGES).index(kv[0])):
        print(F.Report.fmt(case, st, v))
    print(f"test_gpu_layers wall time {time.time() - _t0:.1f} s")
    REPORT.assert_ok()
