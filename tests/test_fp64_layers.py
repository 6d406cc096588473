"""The float64 layer reference (tests/fp64_layers.py) itself: its operations against torch's float64 ones, its bound against the C
oracle's fp32 stage tensors (never too tight), and against deliberately broken stage tensors (never too loose)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import fp64_layers as F
from xfeatslam_amd import synth, weights as WT


def _t(x):
    """[H, W, C] -> torch [1, C, H, W]"""
    return torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1)[None]))


def _n(t):
    return t[0].numpy().transpose(1, 2, 0)


def _close(a, b):
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-300)


def _rand(shape, seed):
    return WT.uniform01(seed, 0, int(np.prod(shape))).reshape(shape) * 2.0 - 1.0


# ---- a. the reference's operations against torch float64 ------------------------------------------------------------------
@pytest.mark.parametrize("H,W,cin,cout,k,stride,pad", [(13, 17, 3, 5, 3, 1, 1), (13, 17, 3, 5, 3, 2, 1), (15, 9, 4, 6, 1, 1, 0),
                                                       (11, 21, 2, 3, 3, 1, 0), (7, 10, 5, 4, 3, 2, 0), (9, 11, 6, 7, 1, 2, 0)])
def test_conv2d_matches_torch(H, W, cin, cout, k, stride, pad):
    x, w = _rand((H, W, cin), 1), _rand((cout, cin, k, k), 2)
    _close(F.conv2d(x, w, stride, pad), _n(TF.conv2d(_t(x), torch.from_numpy(w), stride=stride, padding=pad)))


@pytest.mark.parametrize("H,W,Ho,Wo", [(5, 7, 10, 14), (5, 7, 20, 28), (9, 13, 4, 6), (23, 29, 16, 32), (22, 40, 88, 160), (1, 3, 4, 12)])
@pytest.mark.parametrize("ac", [False, True])
def test_bilinear_matches_torch(H, W, Ho, Wo, ac):
    x = _rand((H, W, 3), 3)
    # the source index is evaluated in fp32 as ATen's float kernel does; torch's float64 kernel indexes in fp64: the same taps and
    # weights wherever the fp32 index is exact, i.e. for these size ratios
    ref = _n(TF.interpolate(_t(x), size=(Ho, Wo), mode="bilinear", align_corners=ac))
    if not ac and (H / Ho, W / Wo) in ((0.5, 0.5), (0.25, 0.25)):
        _close(F.resize_bilinear(x, Ho, Wo, ac), ref)
    else:      # fp32 index and weights: within the image resize's bound (6u S + the index term) of torch's fp64 result
        out, sens = F.resize_bilinear(x, Ho, Wo, ac, sens=True)
        assert np.all(np.abs(out - ref) <= 6 * F.U * F.resize_bilinear(np.abs(x), Ho, Wo, ac) + sens)


def test_bilinear_fp32_index_is_atens():
    """the fp32 source index: the image resize of the forward pass against ATen's float32 kernel on u8/255 frames"""
    g = synth.image(170, 230, 3).astype(np.float64)[:, :, None] / 255.0
    ref = _n(TF.interpolate(_t(g).float(), size=(160, 224), mode="bilinear", align_corners=False)).astype(np.float64)
    out, sens = F.resize_bilinear(g, 160, 224, sens=True)
    assert np.all(np.abs(out - ref) <= 6 * F.U * out + sens + F.TINY)


def test_avg_pool_batch_norm_softmax_shuffle_unfold_match_torch():
    x = _rand((17, 23, 5), 4) * 3.0 + 0.7
    _close(F.avg_pool(x, 4), _n(TF.avg_pool2d(_t(x), 4, 4)))
    bn = TF.batch_norm(_t(x), None, None, training=True, eps=F.EPS)
    _close(F.batch_norm_train(x), _n(bn))
    inn = TF.instance_norm(_t(x[:, :, :1]), eps=F.EPS)
    _close(F.batch_norm_train(x[:, :, :1]), _n(inn))
    l = _rand((6, 5, 65), 5) * 30.0
    _close(F.softmax(l), _n(TF.softmax(_t(l), dim=1)))
    p = _rand((3, 4, 64), 6)
    _close(F.pixel_shuffle8(p)[:, :, None], _n(TF.pixel_shuffle(_t(p), 8)))
    img = _rand((24, 40, 1), 7)
    t = _t(img)
    u = t.unfold(2, 8, 8).unfold(3, 8, 8).reshape(1, 1, 3, 5, 64).permute(0, 1, 4, 2, 3).reshape(1, -1, 3, 5)   # XFeatModel::unfold2d
    _close(F.unfold2d(img[:, :, 0]), _n(u))
    z = np.linspace(-120, 40, 101)
    _close(F.sigmoid(z), torch.sigmoid(torch.from_numpy(z)).numpy())


# ---- b. the bound holds for the C oracle's fp32 tensors ------------------------------------------------------------------
def oracle_getter(O, orc):
    def get(st):
        if st.startswith("RAW"):
            return orc.tensor(O.T["RAW0"] + int(st[3:]))
        if st.startswith("STAT"):
            return orc.tensor(O.T["STAT0"] + int(st[4:]))
        return orc.tensor(O.T[st])
    return get


def _with_bn(w, seed):
    bn = WT.make_synthetic(seed, 3.0, with_bn=True)
    for n, _ in WT.BN_TENSORS:
        w[n] = bn[n]
    return w


SHAPES = [(64, 32), (170, 230), (100, 136)]
FAMILIES = ["normal", "dc", "heat_denormal", "heavy", "tiny", "pruned", "peaky"]


@pytest.mark.parametrize("family", FAMILIES)
def test_bound_holds_for_oracle_tensors(oracle_mod, family):
    rep = F.Report()
    blob = WT.pack_blob(WT.make_family(family, 7))
    wt = WT.unpack_blob(blob)
    orc = oracle_mod.Oracle(blob)
    for k, (H, W) in enumerate(SHAPES):
        for img in (synth.image_family(("noise", "steps", "lowcontrast")[k], H, W, 40 + k), np.full((H, W), 91 + k, np.uint8)):
            orc.extract(img, 512, (0, 0))
            F.FrameCheck(oracle_getter(oracle_mod, orc), img, wt, "batch", rep, f"{family}/{H}x{W}/{int(img.std() == 0)}").run()
    print("\n".join(rep.lines()))
    rep.assert_ok()
    assert {s for _, s in rep.rows} == set(F.STAGES)             # every stage compared (block1.0's map too: the oracle keeps it)


def test_bound_holds_for_oracle_tensors_running_stats(oracle_mod):
    rep = F.Report()
    blob = WT.pack_blob(_with_bn(WT.make_family("normal", 8), 8))
    orc = oracle_mod.Oracle(blob, bn_mode=1)
    for H, W in SHAPES[:2]:
        img = synth.image(H, W, 9)
        orc.extract(img, 512, (0, 0))
        F.FrameCheck(oracle_getter(oracle_mod, orc), img, WT.unpack_blob(blob), "running", rep, f"running/{H}x{W}").run()
    print("\n".join(rep.lines()))
    rep.assert_ok()


# ---- c. the bound has teeth: each mutation fails at the stage it is applied to ---------------------------------------------
@pytest.fixture(scope="module")
def two_frames(oracle_mod):
    blob = WT.pack_blob(WT.make_family("normal", 11))
    wt = WT.unpack_blob(blob)
    frames = []
    for seed in (21, 22):
        img = synth.image(170, 230, seed)
        orc = oracle_mod.Oracle(blob)
        orc.extract(img, 512, (0, 0))
        get = oracle_getter(oracle_mod, orc)
        frames.append((img, {s: get(s) for s in F.STAGES}))
    return wt, frames


def _check(wt, img, tensors, stage, layers, mutate=None):
    rep = F.Report()
    F.FrameCheck(lambda s: tensors.get(s), img, wt, "batch", rep, "m", mutate=mutate).run(layers)
    return rep


def _shape(fc, li):
    h, w = fc.layer_hw(li)
    return h, w, F.LAYERS[li][2]


def test_unmutated_frames_pass(two_frames):
    wt, frames = two_frames
    for img, t in frames:
        _check(wt, img, t, None, None).assert_ok()


def test_dropped_tap_column_at_a_tile_edge_fails(two_frames):
    wt, ((img, t), _) = two_frames
    for li in (2, 7, 17):                                    # direct kernel, 3x3 24 -> 64 s2 -> 64 -> 64 at 1/8, block_fusion.1
        fc = F.FrameCheck(lambda s: t.get(s), img, wt)
        x = fc.layer_input(li)[0]
        w = wt[F.LAYERS[li][0] + ".layer.0.weight"].astype(np.float64).copy()
        w[:, :, :, 1:] = 0.0                                 # the kx = 0 column of taps alone
        part = F.conv2d(x, w, F.LAYERS[li][4], 1)
        raw = t[f"RAW{li}"].reshape(_shape(fc, li)).astype(np.float64)
        raw[:, 16, :] -= part[:, 16, :]
        m = dict(t, **{f"RAW{li}": raw.astype(np.float32).reshape(-1)})
        assert _check(wt, img, m, None, [li]).stage_ratio("m", f"RAW{li}") > 1.0, li


def test_statistics_of_another_frame_fail(two_frames):
    wt, ((img, t), (_, t2)) = two_frames
    for li in (0, 5, 12, 19):
        m = dict(t, **{f"STAT{li}": t2[f"STAT{li}"]})
        assert _check(wt, img, m, None, [li]).stage_ratio("m", f"STAT{li}") > 1.0, li


def test_channel_shifted_by_one_row_fails(two_frames):
    wt, ((img, t), _) = two_frames
    for li, c in ((3, 5), (10, 17), (16, 63), (21, 0)):
        fc = F.FrameCheck(lambda s: t.get(s), img, wt)
        raw = t[f"RAW{li}"].reshape(_shape(fc, li)).copy()
        raw[:, :, c] = np.roll(raw[:, :, c], 1, axis=0)
        m = dict(t, **{f"RAW{li}": raw.reshape(-1)})
        assert _check(wt, img, m, None, [li]).stage_ratio("m", f"RAW{li}") > 1.0, li


def test_inputs_rounded_to_10_mantissa_bits_fail(two_frames):
    wt, ((img, t), _) = two_frames
    # (not the 128-channel layers at 1/32: on a 5 x 7 map the rounding noise, ~sqrt(K) 2^-11 relative, stays inside (K + 2) u S for
    # K = 1152 -- the bound is a worst case over every summation order)
    for li in (1, 4, 8, 11, 16, 20):
        fc = F.FrameCheck(lambda s: t.get(s), img, wt, mutate={"round_inputs": li})
        bad, _ = fc.layer_ref(li)
        m = dict(t, **{f"RAW{li}": bad.astype(np.float32).reshape(-1)})
        assert _check(wt, img, m, None, [li]).stage_ratio("m", f"RAW{li}") > 1.0, li


def test_fusion_upsample_with_align_corners_fails(two_frames):
    wt, ((img, t), _) = two_frames
    bad, _ = F.FrameCheck(lambda s: t.get(s), img, wt, mutate={"align_corners": True}).layer_ref(16)
    m = dict(t, RAW16=bad.astype(np.float32).reshape(-1))
    assert _check(wt, img, m, None, [16]).stage_ratio("m", "RAW16") > 1.0


def test_unfold_channel_order_transposed_fails(two_frames):
    wt, ((img, t), _) = two_frames
    bad, _ = F.FrameCheck(lambda s: t.get(s), img, wt, mutate={"unfold_transposed": True}).layer_ref(20)
    m = dict(t, RAW20=bad.astype(np.float32).reshape(-1))
    assert _check(wt, img, m, None, [20]).stage_ratio("m", "RAW20") > 1.0
