"""The device-side frame grid (k_grid_build) and the fused windowed best-two search (k_search_window) against the fp32
restatement of the reference (tests/ref_window.py), the bit-exact oracle of the best / second-best loop (oracle best2_csr) and
the existing k_best2_csr on the candidate lists the restatement builds.  Integer work: every comparison is exact."""
import numpy as np
import pytest

import ref_window as RW
from xfeatslam_amd import capi, synth, weights as WT
from xfeatslam_amd.extractor import Context

pytestmark = pytest.mark.gpu

F = np.float32
BOUNDS = {"vga": (0.0, 0.0, 640.0, 480.0), "720p": (0.0, 0.0, 1280.0, 720.0), "odd": (0.0, 0.0, 230.0, 170.0)}
RADII = [0.0, 0.5, 7.0, 15.0, 30.0, 100.0, 1e4]


@pytest.fixture(scope="module")
def wctx(gpu_lib):
    c = Context(nfeatures=64, max_height=32, max_width=32)
    yield c
    c.close()


def record_keypoints(n, n_valid, mono, bounds, seed):
    """n slots laid out like an extraction record: mono keypoints at the front, n_valid - mono at the back, default
    cv::KeyPoint() (0, 0, size 0) between them; pixel-centre coordinates like the extractor's, plus the border cases"""
    rng = np.random.RandomState(seed)
    k = np.zeros(n, capi.KP_DTYPE)
    valid = RW.valid_slots(n, n_valid, mono)
    nv = int(valid.sum())
    x = rng.randint(0, int(bounds[2]), nv).astype(F); y = rng.randint(0, int(bounds[3]), nv).astype(F)
    mnx, mny, iw, ih = RW.geom(bounds)
    m = min(nv // 4, 64)
    if m >= 4:
        # on cell borders: (x - min_x) * inv_w = k + 0.5 (as close as fp32 division gets), both neighbours of it, the last row / column
        kk = rng.randint(0, 64, m).astype(F)
        x[:m] = (kk + F(0.5)) / iw
        x[m:2 * m] = np.nextafter(x[:m], F(-1e9)); y[m:2 * m] = (rng.randint(0, 48, m).astype(F) + F(0.5)) / ih
        x[2 * m:3 * m] = F(bounds[2]) - F(1); y[2 * m:3 * m - m // 2] = F(bounds[3]) - F(1)
        x[3 * m:3 * m + 4] = [bounds[2] - 0.25, 0.0, bounds[2] / 2, 0.25]; y[3 * m:3 * m + 4] = [5.0, bounds[3] - 0.25, bounds[3] - 0.5, 0.25]
    k["x"][valid] = x; k["y"][valid] = y; k["size"][valid] = 1; k["angle"][valid] = -1
    return k, valid


@pytest.mark.parametrize("name", sorted(BOUNDS))
@pytest.mark.parametrize("n", [1, 600, 4096, 16384])
def test_grid_build_matches_reference(wctx, name, n):
    b = BOUNDS[name]
    n_valid = n if n == 1 else (n * 7) // 8
    mono = n_valid // 3
    k, valid = record_keypoints(n, n_valid, mono, b, 100 + n)
    for flags in (0, capi.GRID_SKIP_PADDING):
        g = wctx.grid_build(k, b, flags, header=(n_valid, mono))
        blob = wctx.grid_download(g, n)
        cs, items = wctx.grid_unpack(blob, n)
        rcs, ritems = RW.build(k["x"], k["y"], b, use=valid if flags else None)
        assert np.array_equal(cs, rcs) and np.array_equal(items, ritems), (name, n, flags)
        # the whole blob: header with bounds and inverse cell sizes, cell_start, (slot, x, y) per item
        assert np.array_equal(blob, RW.make_blob(rcs, ritems, n, k["x"], k["y"], b, flags))
        if n > 1 and not flags:
            c0 = items[:cs[1]]                                                     # the padding sits in cell (0, 0); slot order inside
            assert (~valid).sum() > 0 and np.all(np.isin(np.nonzero(~valid)[0], c0)) and np.all(np.diff(c0) > 0)
        g2 = wctx.grid_build(k, b, flags, header=(n_valid, mono))
        assert np.array_equal(wctx.grid_download(g2, n), blob)                 # deterministic
        g.free(); g2.free()
    # without a record header all slots are binned; the flag without a record is refused
    g = wctx.grid_build(k, b, 0)
    assert np.array_equal(wctx.grid_download(g, n), RW.make_blob(*RW.build(k["x"], k["y"], b), n, k["x"], k["y"], b, 0))
    with pytest.raises(capi.XfhError):
        wctx.grid_build(k, b, capi.GRID_SKIP_PADDING)
    g.free()


def test_grid_argument_checks(wctx):
    import ctypes as C
    L = capi.lib()
    d = capi.DeviceBuffer(capi.lib().xfh_grid_bytes(64) + 64)
    ok = capi.GridBounds(0, 0, 640, 480)
    call = lambda kp, n, gb, fl, gr: L.xfh_grid_build_device(wctx.h, kp, n, None, C.byref(gb) if gb else None, fl, gr)
    assert call(d.ptr, 4, ok, 0, d.ptr) == 0
    assert call(d.ptr, -1, ok, 0, d.ptr) == 1 and call(d.ptr, capi.GRID_MAX_N + 1, ok, 0, d.ptr) == 1
    assert call(None, 4, ok, 0, d.ptr) == 1 and call(d.ptr, 4, ok, 0, None) == 1 and call(d.ptr, 4, None, 0, d.ptr) == 1
    assert call(d.ptr, 4, ok, 0, d.ptr + 4) == 1 and call(d.ptr + 2, 4, ok, 0, d.ptr) == 1 and call(d.ptr, 4, ok, 2, d.ptr) == 1
    for bad in [(0, 0, 0, 480), (0, 0, 640, 0), (10, 0, 5, 480), (0, 0, float("nan"), 480), (0, 0, float("inf"), 480)]:
        assert call(d.ptr, 4, capi.GridBounds(*bad), 0, d.ptr) == 1
    sw = lambda q, nq, nt, ur, uq: L.xfh_search_window_device(wctx.h, q, d.ptr, nq, d.ptr, d.ptr, nt, None, ur, uq, 256, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr)
    assert sw(d.ptr, 0, 4, None, None) == 0
    assert sw(d.ptr, 1, 4, d.ptr, None) == 1 and sw(d.ptr, 1, 4, None, d.ptr) == 1         # the right check needs both arrays
    assert sw(None, 1, 4, None, None) == 1 and sw(d.ptr + 4, 1, 4, None, None) == 1 and sw(d.ptr, -1, 4, None, None) == 1 and sw(d.ptr, 1, -1, None, None) == 1
    wctx.synchronize()
    d.free()


def test_grid_build_records_is_eight_single_builds(gpu_lib, weights_dense):
    L = gpu_lib
    H, W, nf, B = 96, 128, 600, 8
    b = (0.0, 0.0, float(W), float(H))
    ctx = Context(nfeatures=nf, max_height=H, max_width=W, max_batch=B)
    ctx.load_weights(weights_dense[1])
    frames = np.stack([synth.image(H, W, 40 + i) for i in range(B)])
    din = capi.DeviceBuffer(frames.nbytes).upload(frames)
    rec = capi.DeviceBuffer(B * ctx.rec_bytes)
    capi.check(L.xfh_extract_batch_device(ctx.h, din.ptr, B, H, W, 0, 40, rec.ptr), ctx.h)
    gb = ctx.grid_bytes(nf)
    for flags in (0, capi.GRID_SKIP_PADDING):
        grids = ctx.grid_build_records(rec.ptr, B, b, flags)
        ctx.synchronize()
        allb = grids.download(np.uint8, B * gb)
        again = ctx.grid_build_records(rec.ptr, B, b, flags)
        ctx.synchronize()
        assert np.array_equal(again.download(np.uint8, B * gb), allb)
        recs = ctx.parse_records(rec.download(np.uint8, B * ctx.rec_bytes), B)
        for i in range(B):
            one = ctx.grid_build_device(rec.ptr + i * ctx.rec_bytes + ctx.kps_off, nf, b, flags, d_record=rec.ptr + i * ctx.rec_bytes)
            blob = ctx.grid_download(one, nf)
            assert np.array_equal(blob, allb[i * gb:(i + 1) * gb]), (flags, i)
            kps, _, nv, mono, _ = recs[i]
            use = RW.valid_slots(nf, nv, mono) if flags else None
            assert np.array_equal(blob, RW.make_blob(*RW.build(kps["x"], kps["y"], b, use), nf, kps["x"], kps["y"], b, flags))
            one.free()
        grids.free(); again.free()
    din.free(); rec.free(); ctx.close()


# ---- search -----------------------------------------------------------------------------------------------------------------
def scene(nt, n_valid, bounds, seed, nq, r):
    """targets: nt record slots (n_valid keypoints + padding with zero descriptor rows); queries: noisy copies of target
    descriptors placed a few pixels from their keypoint, plus queries on and outside the bounds (returned mask `outside`)"""
    rng = np.random.RandomState(seed)
    k, valid = record_keypoints(nt, n_valid, n_valid // 2, bounds, seed + 1)
    tg = np.zeros((nt, 64), F)
    d = rng.randn(int(valid.sum()), 64); d /= np.linalg.norm(d, axis=1, keepdims=True)
    tg[valid] = d.astype(F)
    vi = np.nonzero(valid)[0]
    src = vi[rng.randint(0, len(vi), nq)]
    q = tg[src] + rng.choice([0.03, 0.06, 0.1], nq)[:, None] * rng.randn(nq, 64)
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)
    uvr = np.zeros((nq, 3), F)
    uvr[:, 0] = k["x"][src] + rng.uniform(-3, 3, nq); uvr[:, 1] = k["y"][src] + rng.uniform(-3, 3, nq); uvr[:, 2] = r
    free = rng.rand(nq) < 0.06                                # a few of the queries anywhere in the image: these can come up empty at a small radius
    uvr[free, 0] = rng.uniform(0, bounds[2], int(free.sum())); uvr[free, 1] = rng.uniform(0, bounds[3], int(free.sum()))
    n_out = nq // 8
    outside = np.zeros(nq, bool); outside[:n_out] = True
    w, h = bounds[2], bounds[3]
    edge = np.array([(0, 0), (w, h), (w, 0), (0, h), (w / 2, 0), (-r, -r), (w + r, h + r), (-5, h / 2), (w + 5, h / 2), (w / 2, -40), (w / 2, h + 40),
                     (-3 * w, 10), (10, 3 * h), (-1e6, -1e6), (1e9, 1e9), (w - 0.5, h - 0.5)], F)
    uvr[:n_out, :2] = edge[np.arange(n_out) % len(edge)]
    return k, tg, q, uvr, outside


def run_search(ctx, k, tg, q, uvr, bounds, init, skip=None, uright=None, urq=None, flags=0, header=None):
    """upload, xfh_grid_build_device + xfh_search_window_device, download"""
    nq, nt = len(q), len(k)
    up = lambda a: None if a is None else capi.DeviceBuffer(max(np.ascontiguousarray(a).nbytes, 16)).upload(a)
    dq, du, dt, ds, dr, dz = up(q), up(uvr), up(tg), up(skip), up(uright), up(urq)
    g = ctx.grid_build(k, bounds, flags, header=header)
    out = capi.DeviceBuffer(max(20 * nq, 16))
    ptr = lambda b: None if b is None else b.ptr
    ctx.search_window_device(dq.ptr, du.ptr, nq, g.ptr, dt.ptr, nt, out.ptr, init, ptr(ds), ptr(dr), ptr(dz))
    ctx.synchronize()
    res = out.download(np.int32, 5 * nq).reshape(5, nq) if nq else np.zeros((5, 0), np.int32)
    for x in (dq, du, dt, ds, dr, dz, g, out):
        if x is not None:
            x.free()
    return tuple(res)


def check_against_lists(ctx, O, res, q, tg, off, ind, init):
    a = O.best2_csr(q, tg, off, ind, init)
    b = ctx.best2_csr(q, tg, off, ind, init)
    for i in range(4):
        assert np.array_equal(res[i], a[i]), (i, np.nonzero(res[i] != a[i])[0][:8])
        assert np.array_equal(res[i], b[i]), i
    assert np.array_equal(res[4], np.diff(off))


@pytest.mark.parametrize("r", RADII)
def test_search_window_matches_oracle_and_best2_csr(wctx, oracle_mod, r):
    b = BOUNDS["vga"]
    nt, nq = 4096, 640
    k, tg, q, uvr, outside = scene(nt, 3500, b, 7, nq, r)
    grid = RW.build(k["x"], k["y"], b)
    off, ind = RW.csr(grid, k["x"], k["y"], uvr, b)
    cnt = np.diff(off)[~outside]
    print(f"r={r}: inside queries {len(cnt)}, no candidate {np.mean(cnt == 0):.3f}, two or more {np.mean(cnt >= 2):.3f}, mean {cnt.mean():.1f}, max {np.diff(off).max()}")
    # coverage, decided on the reference lists alone: neither the empty path nor the two-best path may go untested
    if r >= 7:
        assert np.mean(cnt >= 2) >= 0.8
    if r == 7:
        assert 0.01 <= np.mean(cnt == 0) <= 0.10
    for init in (256, 1 << 30):
        res = run_search(wctx, k, tg, q, uvr, b, init)
        check_against_lists(wctx, oracle_mod, res, q, tg, off, ind, init)
        if r >= 7 and init == 256:
            assert (res[0] >= 0).mean() > 0.3 and (res[1] == 256).any()          # both "a match under 256" and "none" occur
    # the host-pointer convenience call
    res = wctx.search_window(q, uvr, k, b, tg, 256)
    check_against_lists(wctx, oracle_mod, res, q, tg, off, ind, 256)
    # skip mask
    rng = np.random.RandomState(5)
    skip = (rng.rand(nt) < 0.3).astype(np.uint8) * rng.randint(1, 256, nt).astype(np.uint8)
    off_s, ind_s = RW.csr(grid, k["x"], k["y"], uvr, b, skip=skip)
    check_against_lists(wctx, oracle_mod, run_search(wctx, k, tg, q, uvr, b, 256, skip=skip), q, tg, off_s, ind_s, 256)
    # right-coordinate check (and both filters together, through the host call)
    uright = np.where(rng.rand(nt) < 0.6, k["x"] - rng.uniform(0, 40, nt), -1).astype(F)
    urq = (uvr[:, 0] - rng.uniform(0, 40, nq)).astype(F)
    off_r, ind_r = RW.csr(grid, k["x"], k["y"], uvr, b, uright=uright, ur_query=urq)
    if 7 <= r <= 30:
        assert off_r[-1] < off[-1]                                               # the check removes something
    check_against_lists(wctx, oracle_mod, run_search(wctx, k, tg, q, uvr, b, 1 << 30, uright=uright, urq=urq), q, tg, off_r, ind_r, 1 << 30)
    off_b, ind_b = RW.csr(grid, k["x"], k["y"], uvr, b, skip=skip, uright=uright, ur_query=urq)
    check_against_lists(wctx, oracle_mod, wctx.search_window(q, uvr, k, b, tg, 256, skip=skip, uright=uright, ur_query=urq), q, tg, off_b, ind_b, 256)


def test_search_window_other_bounds_and_sizes(wctx, oracle_mod):
    for name, nt, r in [("720p", 16384, 15.0), ("odd", 600, 7.0), ("odd", 600, 1e4), ("720p", 4096, 30.0)]:
        b = BOUNDS[name]
        k, tg, q, uvr, _ = scene(nt, (nt * 7) // 8, b, 21, 256, r)
        off, ind = RW.csr(RW.build(k["x"], k["y"], b), k["x"], k["y"], uvr, b)
        check_against_lists(wctx, oracle_mod, run_search(wctx, k, tg, q, uvr, b, 256), q, tg, off, ind, 256)
    # nq = 0 and nt = 1
    b = BOUNDS["vga"]
    k, tg, q, uvr, _ = scene(1, 1, b, 3, 16, 1e4)
    off, ind = RW.csr(RW.build(k["x"], k["y"], b), k["x"], k["y"], uvr, b)
    res = run_search(wctx, k, tg, q, uvr, b, 1 << 30)
    check_against_lists(wctx, oracle_mod, res, q, tg, off, ind, 1 << 30)
    assert (res[4] == 1).any() and np.all(res[2] == -1)
    assert all(len(x) == 0 for x in run_search(wctx, k, tg, q[:0], uvr[:0], b, 256))
    assert all(len(x) == 0 for x in wctx.search_window(q[:0], uvr[:0], k, b, tg, 256))


def test_tie_goes_to_the_first_visited_not_the_lowest_index(wctx, oracle_mod):
    """Two candidates with IDENTICAL descriptors, the higher slot number in the earlier column: the reference's strict '<' keeps
    the one it visits first -- the higher slot number.  Built, not hoped for: 48 such pairs, one query each."""
    b = BOUNDS["vga"]
    npair = 48
    nt = 4 * npair
    rng = np.random.RandomState(9)
    k = np.zeros(nt, capi.KP_DTYPE); k["size"] = 1; k["angle"] = -1
    tg = rng.randn(nt, 64); tg = (tg / np.linalg.norm(tg, axis=1, keepdims=True)).astype(F)
    uvr = np.zeros((npair, 3), F); q = np.zeros((npair, 64), F)
    for p in range(npair):
        cx, cy = 40 + 70 * (p % 8), 40 + 70 * (p // 8)                       # cell size is 10 x 10: pairs are far apart
        lo, hi = p, nt - 1 - p                                                # lower slot in the LATER column (x + 12), higher slot in the earlier one
        k["x"][lo], k["y"][lo] = cx + 12, cy
        k["x"][hi], k["y"][hi] = cx, cy
        tg[hi] = tg[lo]
        far = 2 * npair + p                                                   # a third, different candidate: the runner-up must be the lower slot of the pair
        k["x"][far], k["y"][far] = cx + 5, cy + 9
        k["x"][npair + p], k["y"][npair + p] = 620, 10 + p                    # bystanders elsewhere
        qq = tg[lo] + 0.02 * rng.randn(64); q[p] = (qq / np.linalg.norm(qq)).astype(F)
        uvr[p] = (cx + 6, cy, 15)
    grid = RW.build(k["x"], k["y"], b)
    off, ind = RW.csr(grid, k["x"], k["y"], uvr, b)
    a = oracle_mod.best2_csr(q, tg, off, ind, 1 << 30)
    hi_idx = nt - 1 - np.arange(npair)
    # the data itself: in every list the higher slot precedes the lower one, and the oracle's winner is the higher slot with the lower as runner-up at the same distance
    kind = [(hi_idx[p] in ind[off[p]:off[p + 1]]) and list(ind[off[p]:off[p + 1]]).index(hi_idx[p]) < list(ind[off[p]:off[p + 1]]).index(p) for p in range(npair)]
    assert sum(kind) >= 32
    assert np.array_equal(a[0], hi_idx) and np.array_equal(a[2], np.arange(npair)) and np.array_equal(a[1], a[3])
    res = run_search(wctx, k, tg, q, uvr, b, 1 << 30)
    check_against_lists(wctx, oracle_mod, res, q, tg, off, ind, 1 << 30)
    assert np.array_equal(res[0], hi_idx) and np.all(res[0] > res[2])


def test_query_at_the_origin_meets_the_padding_cell(wctx, oracle_mod):
    """faithful mode: every padding slot sits at (0, 0) with a zero descriptor row, so a query at the origin has hundreds of
    candidates at one distance -- the winner is the first visited; with XFH_GRID_SKIP_PADDING they are gone"""
    b = BOUNDS["vga"]
    nt, n_valid = 4096, 3500
    k, tg, q, uvr, _ = scene(nt, n_valid, b, 13, 64, 15.0)
    uvr[:32, :2] = 0; uvr[32:48, :2] = (3.5, 2.5); q[:8] = 0
    valid = RW.valid_slots(nt, n_valid, n_valid // 2)
    for flags, use in ((0, None), (capi.GRID_SKIP_PADDING, valid)):
        off, ind = RW.csr(RW.build(k["x"], k["y"], b, use), k["x"], k["y"], uvr, b)
        n0 = np.diff(off)[0]
        assert (n0 > 500) if not flags else (n0 < 40)
        for init in (256, 1 << 30):
            res = run_search(wctx, k, tg, q, uvr, b, init, flags=flags, header=(n_valid, n_valid // 2))
            check_against_lists(wctx, oracle_mod, res, q, tg, off, ind, init)
        if not flags:
            pad = np.nonzero(~valid)[0]
            assert res[0][0] == pad[0] and res[2][0] == pad[1] and res[1][0] == res[3][0] == 0     # zero query against zero rows: first two padding slots


def test_non_finite_queries_have_no_candidates(wctx, oracle_mod):
    b = BOUNDS["vga"]
    k, tg, q, uvr, _ = scene(4096, 3500, b, 17, 128, 15.0)
    clean = run_search(wctx, k, tg, q, uvr, b, 256)
    bad = uvr.copy()
    hit = np.arange(0, 128, 5)
    vals = [np.nan, np.inf, -np.inf]
    for j, i in enumerate(hit):
        bad[i, j % 3] = vals[(j // 3) % 3]
    res = run_search(wctx, k, tg, q, bad, b, 256)
    assert np.all(res[4][hit] == 0) and np.all(res[0][hit] == -1) and np.all(res[2][hit] == -1) and np.all(res[1][hit] == 256) and np.all(res[3][hit] == 256)
    keep = np.setdiff1d(np.arange(128), hit)
    for x, y in zip(clean, res):
        assert np.array_equal(x[keep], y[keep])                                # the neighbours in the same launch are unaffected
    off, ind = RW.csr(RW.build(k["x"], k["y"], b), k["x"], k["y"], bad, b)
    check_against_lists(wctx, oracle_mod, res, q, tg, off, ind, 256)
    # huge but finite values and a negative radius: the documented saturation, no candidates
    odd = uvr.copy(); odd[::4, 0] = 3e38; odd[1::4, 2] = -7; odd[2::4, 1] = -3e38; odd[3::4, 2] = 3e38
    off, ind = RW.csr(RW.build(k["x"], k["y"], b), k["x"], k["y"], odd, b)
    check_against_lists(wctx, oracle_mod, run_search(wctx, k, tg, q, odd, b, 256), q, tg, off, ind, 256)


def test_extract_to_search_stays_on_the_device(gpu_lib, oracle_mod, weights_dense):
    """xfh_extract_batch_device of two consecutive frames -> xfh_grid_build_records_device -> xfh_search_window_device of frame
    t-1's descriptors at their own keypoint positions against frame t: only device pointers between the calls.  Equals the host
    route: download the records, ref_window lists, best2_csr."""
    L = gpu_lib
    H, W, nf = 192, 256, 1000
    b = (0.0, 0.0, float(W), float(H))
    ctx = Context(nfeatures=nf, max_height=H, max_width=W, max_batch=2)
    ctx.load_weights(weights_dense[1])
    f0 = synth.image(H, W, 8)
    frames = np.stack([f0, np.roll(f0, (1, 2), (0, 1))])                     # frame t = frame t-1 moved by (2, 1) pixels
    din = capi.DeviceBuffer(frames.nbytes).upload(frames)
    rec = capi.DeviceBuffer(2 * ctx.rec_bytes)
    uvr_d = capi.DeviceBuffer(nf * 12); out = capi.DeviceBuffer(nf * 20)
    # a first pass only to learn where frame t-1's keypoints are: (u, v, r) is the one input the caller (the tracker's projection)
    # supplies from the host
    capi.check(L.xfh_extract_batch_device(ctx.h, din.ptr, 2, H, W, 0, 0, rec.ptr), ctx.h)
    ctx.synchronize()
    k0 = ctx.parse_records(rec.download(np.uint8, 2 * ctx.rec_bytes), 2)[0][0]
    grids = capi.DeviceBuffer(2 * ctx.grid_bytes(nf))
    for r in (7.0, 15.0):
        uvr = np.stack([k0["x"], k0["y"], np.full(nf, r, F)], 1).astype(F)
        uvr_d.upload(uvr)
        ctx.synchronize()
        # the chain: three asynchronous calls on the ctx stream, device pointers only, no synchronisation between them
        capi.check(L.xfh_extract_batch_device(ctx.h, din.ptr, 2, H, W, 0, 0, rec.ptr), ctx.h)
        ctx.grid_build_records(rec.ptr, 2, b, capi.GRID_SKIP_PADDING, d_grids=grids)
        ctx.search_window_device(rec.ptr + ctx.desc_off, uvr_d.ptr, nf, grids.ptr + ctx.grid_bytes(nf), rec.ptr + ctx.rec_bytes + ctx.desc_off, nf, out.ptr, 256)
        ctx.synchronize()
        res = tuple(out.download(np.int32, 5 * nf).reshape(5, nf))
        (k0b, d0, nv0, mono0, _), (k1, d1, nv1, mono1, _) = ctx.parse_records(rec.download(np.uint8, 2 * ctx.rec_bytes), 2)
        assert np.array_equal(k0b, k0)
        use = RW.valid_slots(nf, nv1, mono1)
        off, ind = RW.csr(RW.build(k1["x"], k1["y"], b, use), k1["x"], k1["y"], uvr, b)
        print(f"r={r}: n_valid {nv0} / {nv1}, candidates per query {np.diff(off).mean():.2f}, matched under 256: {(res[0] >= 0).sum()}")
        assert np.diff(off).max() >= 2
        check_against_lists(ctx, oracle_mod, res, d0, d1, off, ind, 256)
    for x in (din, rec, uvr_d, out, grids):
        x.free()
    ctx.close()
