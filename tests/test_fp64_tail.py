"""The float64 reference of the extraction tail (tests/fp64_tail.py) itself: its operations against torch's float64 (and, for ATen's
fp32 source coordinate, float32) ones, its bound against the C oracle's records and stage tensors (never too tight), and against
deliberate corruptions (never too loose: each fails at the stage it hits)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import fp64_tail as T
from fp64_layers import Report
from xfeatslam_amd import synth, weights as WT


def _rand(shape, seed):
    return WT.uniform01(seed, 0, int(np.prod(shape))).reshape(shape)


def _grid(H, W, dtype=torch.float32):
    """InterpolateSparse2d::normgrid of every pixel (x, y) of an H x W frame, Long positions as the reference holds them:
    [1, H*W, 1, 2] (the true division of Long tensors runs in the default dtype, fp32)"""
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    pos = torch.stack([xx.reshape(-1), yy.reshape(-1)], -1)
    g = 2.0 * (pos / torch.tensor([W - 1, H - 1])) - 1.0
    return g.unsqueeze(-2)[None].to(dtype), pos


# ---- a. the reference's operations against torch -------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,window", [(37, 53, 5), (64, 96, 5), (40, 40, 3)])
def test_nms_mask_matches_max_pool2d(H, W, window):
    # values on a coarse grid: plateaus and equal neighbours (a plateau is all candidates), some below the threshold
    k = np.floor(_rand((H, W), 1) * 12.0) / 64.0
    t = torch.from_numpy(k)[None, None]
    lm = TF.max_pool2d(t, window, stride=1, padding=window // 2)
    want = ((t == lm) & (t > torch.tensor(0.05, dtype=torch.float32).double()))[0, 0].numpy()
    assert np.array_equal(T.nms_mask(k, window), want)
    # nonzero() of the mask is row-major: the candidate order is ascending linear index
    nz = torch.nonzero(torch.from_numpy(want)).numpy()
    assert np.array_equal(nz[:, 0] * W + nz[:, 1], np.flatnonzero(want))


@pytest.mark.parametrize("H,W", [(64, 96), (160, 224), (32, 32), (96, 128)])
def test_grid_sample_nearest_index_matches_aten(H, W):
    """every pixel, the last row and column included: ATen's fp32 coordinate and half-to-even rounding; x = W - 1 (y = H - 1)
    rounds to W (H), outside the map, and samples the zero padding"""
    grid, pos = _grid(H, W)
    code = torch.arange(1, H * W + 1, dtype=torch.float32).reshape(1, 1, H, W)        # exact in fp32; 0 = padding
    got = TF.grid_sample(code, grid, mode="nearest", align_corners=False)[0, 0, :, 0].numpy()
    x, y = pos[:, 0].numpy(), pos[:, 1].numpy()
    idx, inside = T.nearest_index(x, y, H, W)
    assert np.array_equal(np.where(inside, idx + 1, 0), got.astype(np.int64))
    assert not inside[(x == W - 1) | (y == H - 1)].any() and inside[(x < W - 1) & (y < H - 1)].all()
    assert np.array_equal(idx[inside], (y * W + x)[inside])                            # elsewhere the pixel itself


@pytest.mark.parametrize("H,W", [(64, 96), (160, 224), (96, 128), (704, 1280)])
def test_grid_sample_bilinear_matches_aten(H, W):
    h, w = H // 8, W // 8
    m = _rand((h, w), 2)
    grid, pos = _grid(H, W)
    x, y = pos[:, 0].numpy(), pos[:, 1].numpy()
    idx, wt, ew, cs = T.bilinear_weights(x, y, H, W, h, w)
    taps = np.where(wt > 0, m.reshape(-1)[idx], 0.0)
    ref = (wt * taps).sum(0)
    # ATen float32: the same coordinate (one rounding of the unnormalise) and fp32 weights: within 6u S + sum |t| ew
    m32 = m.astype(np.float32)
    got32 = TF.grid_sample(torch.from_numpy(m32)[None, None], grid, mode="bilinear", align_corners=False)[0, 0, :, 0].numpy()
    t32 = np.where(wt > 0, m32.astype(np.float64).reshape(-1)[idx], 0.0)
    ref32 = (wt * t32).sum(0)
    tol = 6 * T.U * np.abs(wt * t32).sum(0) + (np.abs(t32) * ew).sum(0) + 8 * T.TINY
    assert np.all(np.abs(got32 - ref32) <= tol)
    # ... and the device's coordinate (product rounded before the subtraction) stays within the coordinate term
    f = np.float32
    g1 = (grid[0, :, 0].numpy() + f(1)).astype(f)
    ixd, iyd = (g1[:, 0] * f(w / 2)).astype(f) - f(0.5), (g1[:, 1] * f(h / 2)).astype(f) - f(0.5)
    ix, iy = T.grid_coord(x, W, w), T.grid_coord(y, H, h)
    assert np.all(np.abs(ixd.astype(np.float64) - ix) <= T.coord_shift(ix)) and np.all(np.abs(iyd.astype(np.float64) - iy) <= T.coord_shift(iy))
    assert np.array_equal(np.floor(ixd), np.floor(ix)) and np.array_equal(np.floor(iyd), np.floor(iy))
    # ATen float64: the same taps and weights where its fp64 unnormalise of the same grid is the fp32 coordinate
    got64 = TF.grid_sample(torch.from_numpy(m)[None, None], grid.double(), mode="bilinear", align_corners=False)[0, 0, :, 0].numpy()
    g = grid[0, :, 0].double().numpy()
    exact = ((g[:, 0] + 1) * (w / 2) - 0.5 == ix) & ((g[:, 1] + 1) * (h / 2) - 0.5 == iy)
    assert exact.mean() > 0.05
    assert np.abs(got64[exact] - ref[exact]).max() <= 1e-15
    # the last column / row: half a tap in the zero padding
    last = (x == W - 1) & exact
    assert last.any() and np.all(wt[1][last] == 0) and np.all(wt[3][last] == 0)


def test_normalize_and_stable_descending_sort_match_torch():
    x = (_rand((9, 64), 3) - 0.5) * 3.0
    x[3] = 0.0
    x[5] = 1e-15                                           # below the eps: divided by 1e-12f
    # the eps of F.normalize on the fp32 map is 1e-12 as an fp32 scalar
    got = TF.normalize(torch.from_numpy(x), dim=-1, eps=T.EPS_N).numpy()
    assert np.abs(T.l2n(x) - got).max() <= 1e-15
    got32 = TF.normalize(torch.from_numpy(x[5:6]).float(), dim=-1).numpy()
    assert np.array_equal(got32, (np.float32(1e-15) / np.float32(1e-12)) * np.ones((1, 64), np.float32))
    # descending score, ties in ascending index (argsort of -scores, stable): the key order of the selection
    s = np.floor(_rand(500, 4) * 40.0) / 40.0
    s[:3] = -1.0
    order = torch.argsort(-torch.from_numpy(s), stable=True).numpy()
    key = np.lexsort((np.arange(s.size), -s))
    assert np.array_equal(order, key)


# ---- b. the bound holds for the C oracle's records and stage tensors -----------------------------------------------------
def oracle_tail(O, orc, img, nf, lap=(0, 0), rescale=False, report=None, case="", mutate=None):
    kps, desc, nv, mono = orc.extract(img, nf, lap)
    H0, W0 = img.shape
    H, W = H0 // 32 * 32, W0 // 32 * 32
    nc = orc.tensor(O.T["CAND"]).size // 3
    tc = T.TailCheck(orc.tensor(O.T["K1H"]).reshape(H, W), orc.tensor(O.T["H1"]), orc.tensor(O.T["FEATS"]), orc.tensor(O.T["SEL"]),
                     kps, desc, nv, mono, nc, nf, lap, (H0, W0), rescale, True, report, case, 0, mutate)
    return tc


ORACLE_CASES = [
    # (family, H, W, image family, nfeatures, lapping, rescale)
    ("normal", 170, 230, "noise", 512, (40, 120), False),
    ("normal", 170, 230, "noise", 4096, (40, 120), True),
    ("dc", 96, 128, "steps", 2048, (0, 0), False),
    ("dc", 100, 136, "const", 300, (0, 200), True),
    ("heat_denormal", 170, 230, "blobs", 333, (64, 64), False),
    ("peaky", 96, 160, "noise", 1, (0, 0), False),
    ("peaky", 170, 230, "const", 4096, (10, 100), False),
    ("heavy", 96, 128, "noise", 2048, (0, 0), False),
    ("tiny", 160, 224, "lowcontrast", 1000, (50, 51), False),
    ("pruned", 100, 136, "saturated", 64, (0, 0), True),
    ("scaled", 480, 640, "gradient", 4096, (100, 300), False),
    ("uniform", 480, 640, "noise", 8000, (0, 639), False),
]


def _img(fam, H, W, seed):
    return np.full((H, W), 77, np.uint8) if fam == "const" else synth.image_family(fam, H, W, seed)


def test_bound_holds_for_oracle_records(oracle_mod):
    rep = Report()
    info = []
    for k, (fam, H, W, imf, nf, lap, resc) in enumerate(ORACLE_CASES):
        orc = oracle_mod.Oracle(WT.pack_blob(WT.make_family(fam, 7)), rescale=resc)
        case = f"{fam}/{H}x{W}/{imf}/nf{nf}/lap{lap[0]}-{lap[1]}/r{int(resc)}"
        tc = oracle_tail(oracle_mod, orc, _img(imf, H, W, 30 + k), nf, lap, resc, rep, case)
        tc.run()
        info.append((case, tc.n_candidates, len(tc.ss), tc.n_valid, tc.near_ties))
    for case, C, N, nv, nt in info:
        print(f"{case:<44} C {C:>6} N {N:>5} n_valid {nv:>5} near-ties {nt}")
    print("\n".join(rep.lines()))
    rep.assert_ok()
    assert {s for _, s in rep.rows} == set(T.STAGES)
    assert any(C < N0 for (_, C, _, _, _), (_, _, _, _, N0, _, _) in zip(info, ORACLE_CASES))     # padding slots
    assert any(C > N0 for (_, C, _, _, _), (_, _, _, _, N0, _, _) in zip(info, ORACLE_CASES))     # a cut


# ---- c. the bound has teeth: each corruption fails at the stage it hits ---------------------------------------------------
@pytest.fixture(scope="module")
def frame(oracle_mod):
    """96x128, heavy weights, a noise frame whose candidates include pixel (0, 0) and score-0 ties (the last row / column);
    nfeatures above the candidate count, so every candidate is in SEL; the lapping bounds on two keypoint columns"""
    orc = oracle_mod.Oracle(WT.pack_blob(WT.make_family("heavy", 7)))
    img = synth.image_family("noise", 96, 128, 2)
    tc = oracle_tail(oracle_mod, orc, img, 2048)
    tc.run()
    xs = np.unique(tc.sx[tc.ss > 0])
    lap = (int(xs[len(xs) // 4]), int(xs[3 * len(xs) // 4]))
    return oracle_mod, orc, img, lap


def _run(frame, mutate=None, corrupt=None):
    O, orc, img, lap = frame
    rep = Report()
    tc = oracle_tail(O, orc, img, 2048, lap, report=rep, case="m", mutate=mutate)
    if corrupt:
        corrupt(tc)
    tc.run()
    return tc, {s: rep.stage_ratio("m", s) for s in T.STAGES if ("m", s) in rep.rows}


def test_the_frame_crosses_every_corruption(frame):
    tc, r = _run(frame)
    assert all(v <= 1.0 for v in r.values()), r
    assert set(r) == set(T.STAGES)
    pix = tc.sy * tc.W + tc.sx
    assert 0 in pix                                                      # the (0, 0) mask
    assert (tc.ss == 0).sum() >= 2                                       # exact ties
    lap = frame[3]
    assert ((tc.sx == lap[0]) & (tc.ss > 0)).any() and ((tc.sx == lap[1]) & (tc.ss > 0)).any()


def _fails_at(r, stage):
    order = T.STAGES
    assert r[stage] > 1.0, r
    assert all(r[s] <= 1.0 for s in order[:order.index(stage)]), r


@pytest.mark.parametrize("mutate,stage", [
    ({"window": 3}, "NMS"),
    ({"nearest": "floor"}, "SCORE"),
    ({"align_corners": True}, "SCORE"),
    ({"swap_xy": True}, "SCORE"),
    ({"no_origin_mask": True}, "SCORE"),
    ({"ties": "desc"}, "SELECT"),
    ({"lap_exclusive": True}, "SELECT"),
    ({"sample_raw": True}, "DESC"),
    ({"no_renorm": True}, "DESC"),
], ids=["window3x3", "nearest_floor", "align_corners", "swap_xy", "no_origin_mask", "ties_descending", "lap_exclusive",
        "sample_before_normalise", "no_renormalise"])
def test_reference_corruption_fails_at_its_stage(frame, mutate, stage):
    _fails_at(_run(frame, mutate=mutate)[1], stage)


def _round10(tc):
    tc.desc = T.round_mantissa(tc.desc.astype(np.float64), 10).astype(np.float32)


def _neighbour_slot(tc):
    tc.desc = tc.desc.copy()
    tc.desc[:tc.mono] = np.roll(tc.desc[:tc.mono], 1, axis=0)          # front slots only: the padding rows stay zero


@pytest.mark.parametrize("corrupt", [_round10, _neighbour_slot], ids=["desc_10_bits", "desc_from_neighbouring_slot"])
def test_descriptor_corruption_fails_at_desc(frame, corrupt):
    _fails_at(_run(frame, corrupt=corrupt)[1], "DESC")
