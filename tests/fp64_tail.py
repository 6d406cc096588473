"""Float64 reference of the extraction tail -- NMS, scores, top-k selection, record packing and descriptors -- evaluated from the
tensors the device materialised, with a derived error bound.

Written from the reference's semantics (XFextractor::operator(), NMS and getKptsHeatmap; InterpolateSparse2d::normgrid / forward
with grid_sample(align_corners=False, padding_mode=zeros)), in numpy only: no torch, no oracle.  Every stage is evaluated from the
device's own fp32 inputs (K1H, H1, FEATS, the selected keys SEL and the record), so one check isolates one kernel.

Stages
------
NMS (exact).  A candidate is a pixel with K1h == max over its 5x5 window (padded with -inf) and K1h > 0.05f, on the device's fp32
K1H: comparisons of fp32 values, no rounding.  The header's n_candidates equals the count; every selected key is a candidate.

SCORE (bounded).  score = nearest(K1h) * bilinear(H1) at the keypoint, -1 at pixel (0, 0).  The source coordinate is ATen's:
normgrid in fp32 (x / (W - 1), then 2 g - 1), grid_sample's align_corners=False unnormalise in fp32, ix = (g + 1) * (size / 2) - 0.5
with ONE rounding (ATen's CPU kernel fuses the multiply and the subtraction; tests/test_fp64_tail.py pins it).  The device rounds
the product first: both lie within u |(g + 1) size / 2| + u |ix| of the exact value, so they differ by at most
dix = u (3 |ix| + 1) + 4u^2.  No coordinate of a pixel lies within 1 / (2 (W - 1)) of a half-integer (nearest) or of an integer
(bilinear: x w / (W - 1) = k + 1/2 would need 2 x w = (2k + 1)(W - 1), even = odd), far beyond dix: the rounded index and the
bilinear cell are the same for both, and inside a cell the sample is linear in ix, so the shift moves it by at most
dix (b0 |t01 - t00| + b1 |t11 - t10|) (+ the same in y) -- the precedent of fp64_layers.resize_bilinear's index term.
nearest rounds half to even; at x = W - 1 the coordinate is exactly W - 0.5 and rounds to W (W is a multiple of 32), outside the
map: the zero padding makes that score 0.  Taps and products here are fp64 on the fp32 coordinate.  The device evaluates the
fractional weights in fp32: w = ix - floor(ix) (one rounding, |dw| <= u w), 1 - w (|d| <= u w + u (1 - w) <= u(1 + u)), so each
1-D weight a carries d1 = u (1 + u) and each 2-D weight P = a b

    |P_dev - a b|  <=  ew = d1 (a + b) + d1^2 + u (a b + d1 (a + b) + d1^2)

(the product's own rounding).  The sum ((t0 P0 + t1 P1) + t2 P2) + t3 P3 of K = 4 products rounds 7 times: (K + 2) u S with
S = sum |t_k P_k| (fp64_layers bound (1)); a subnormal tap adds 2^-150 per operation.  The taps are the device's H1, exact:

    |hb_dev - hb|  <=  tol_hb = 6 u S + sum_k |t_k| ew_k + (the coordinate term above) + 8 2^-149
    |score_dev - score|  <=  nv tol_hb (1 + u) + u |score| + 2^-149        (nv = the nearest K1h value, exact)

SELECT (exact on the device's scores, bounded against fp64).  SEL is in strictly ascending key order: descending score, ties in
ascending pixel index (argsort of -scores over nonzero()'s row-major candidates, stable); N = min(n_candidates, nfeatures).
The selected set must be the fp64 top N of the candidates: a candidate left out may rank above a selected one in fp64 only where
their score intervals [s - tol, s + tol] overlap (an accepted near-tie, counted).  The record (exact): valid = score > 0; a
valid key goes to the back (slots nfeatures - 1 downward, in rank order) when lap0 <= fp32(x * rw) <= lap1, both bounds inclusive,
else to the front (slots 0 upward); n_valid and mono_index count them; a slot holds KeyPoint(x * rw, y * rh, 1, -1, score) with
the response equal to SEL's score bit for bit, octave 0, class_id -1; padding slots (where the producer writes them) hold
KeyPoint() = (0, 0, 0, -1, 0, 0, -1) and zero descriptors.

DESC (bounded).  M = FEATS / max(||FEATS||_2, 1e-12f) per pixel, sampled bilinearly with zero padding at the keypoint, then
y = v / max(||v||_2, 1e-12f).  The device stores fp32 norms of fp64 sums of squares (one rounding u plus 64 2^-53 from the sum)
and divides by a refined reciprocal (div_by: a Newton step on v_rcp, then two fma residual corrections: within 1 ulp, counted as
2u), so each normalised tap carries |dm| <= 4u |m| (u + 2^-47 + 2u, rounded up).  With the weights above:

    |v_dev - v|  <=  tol_v = 6 u S + sum_k P_k 4u |m_k| + sum_k |m_k| ew_k + (the coordinate term) + 8 2^-149   (per channel)

Normalisation n(v) = v / max(||v||, eps): with N' = max(||v|| - ||tol_v||_2, eps) (norms and the max are 1-Lipschitz),

    |n(v_dev) - n(v)|_c  <=  (tol_v,c + |y_c| ||tol_v||_2) / N'

and the device's own norm and division add 4u |y_c| (+ 2^-149).  Where v nearly cancels, ||v|| - ||tol_v|| is small and the bound
widens with it instead of breaking; where ||v|| < eps both sides divide by eps exactly.

No per-stage factors: every check reports max err/tol (exact checks: tol 0), and err/tol <= 1 everywhere is the pass criterion.
"""
from __future__ import annotations

import numpy as np

from fp64_layers import TINY, U, Report

STAGES = ["NMS", "SCORE", "SELECT", "DESC"]
EPS_N = float(np.float32(1e-12))
THR = float(np.float32(0.05))
D1 = U * (1.0 + U)
KP_DEFAULT = (0.0, 0.0, 0.0, -1.0, 0.0, 0, -1)          # cv::KeyPoint(): x, y, size, angle, response, octave, class_id


# ---- fp64 operations -----------------------------------------------------------------------------------------------------
def nms_mask(k1h: np.ndarray, window: int = 5, thr: float = THR) -> np.ndarray:
    """max_pool2d(window, stride 1, pad window // 2, -inf padding) == x and x > thr"""
    H, W = k1h.shape
    p = window // 2
    a = np.full((H + 2 * p, W + 2 * p), -np.inf)
    a[p:p + H, p:p + W] = k1h
    rows = a[:, 0:W].copy()
    for d in range(1, window):
        np.maximum(rows, a[:, d:d + W], out=rows)
    m = rows[0:H].copy()
    for d in range(1, window):
        np.maximum(m, rows[d:d + H], out=m)
    return (k1h == m) & (k1h > thr)


def grid_coord(pos: np.ndarray, full: int, size: int, align_corners: bool = False) -> np.ndarray:
    """normgrid (fp32: pos / (full - 1), 2 g - 1) then grid_sample's unnormalise as ATen's CPU kernel evaluates it: (g + 1) in fp32,
    then (g + 1) * (size / 2) - 0.5 rounded to fp32 once (exact in fp64 before that rounding: 24 x 12 bits)"""
    f = np.float32
    g = (f(2) * (np.asarray(pos).astype(f) / f(full - 1))).astype(f) - f(1)
    g1 = (g + f(1)).astype(np.float64)
    if align_corners:
        return (g1 / 2 * (size - 1)).astype(f)
    return (g1 * (size / 2) - 0.5).astype(f)


def coord_shift(ix: np.ndarray) -> np.ndarray:
    """what the device's two roundings of the unnormalise (product, then subtraction) can move the coordinate by"""
    return U * (3.0 * np.abs(ix) + 1.0) + 4.0 * U * U


def nearest_index(x, y, H, W, mode="rint", align_corners=False):
    """grid_sample nearest on a [H, W] map sampled at pixel (x, y) of the same map: (flat index, inside)"""
    rnd = np.floor if mode == "floor" else np.rint        # np.rint: half to even, as nearbyint
    fx = rnd(grid_coord(x, W, W, align_corners).astype(np.float64))
    fy = rnd(grid_coord(y, H, H, align_corners).astype(np.float64))
    inside = (fx >= 0) & (fx <= W - 1) & (fy >= 0) & (fy <= H - 1)
    return (np.where(inside, fy, 0) * W + np.where(inside, fx, 0)).astype(np.int64), inside


def bilinear_weights(x, y, H, W, h, w, align_corners=False, swap=False):
    """grid_sample bilinear (zeros padding) of a [h, w] map at full-resolution pixels (x, y) of an H x W frame:
    flat tap indices [4, N], fp64 weights [4, N] (zero where a tap is outside), their device error bound ew [4, N] and the
    coordinate term's factors [4, N]: sum_k |t_k - t_partner(k)| c_k bounds what the coordinate shift moves the sample by"""
    if swap:
        ix, iy = grid_coord(y, H, w, align_corners), grid_coord(x, W, h, align_corners)
    else:
        ix, iy = grid_coord(x, W, w, align_corners), grid_coord(y, H, h, align_corners)
    ix, iy = ix.astype(np.float64), iy.astype(np.float64)
    x0, y0 = np.floor(ix), np.floor(iy)
    fx, fy = ix - x0, iy - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    idx, wt, ew = [], [], []
    for dy, dx, a, b in ((0, 0, 1 - fx, 1 - fy), (0, 1, fx, 1 - fy), (1, 0, 1 - fx, fy), (1, 1, fx, fy)):
        xx, yy = x0 + dx, y0 + dy
        ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        idx.append(np.where(ok, yy * w + xx, 0))
        wt.append(np.where(ok, a * b, 0.0))
        e = D1 * (a + b) + D1 * D1 + U * (a * b + D1 * (a + b) + D1 * D1)
        ew.append(np.where(ok, e, 0.0))
    # taps 0-1 and 2-3 differ in x (weights b = 1 - fy, fy), taps 0-2 and 1-3 in y (a = 1 - fx, fx): with d = t1 - t0 etc.,
    # |ds| <= dix (b0 |t1 - t0| + b1 |t3 - t2|) + diy (a0 |t2 - t0| + a1 |t3 - t1|)
    dix, diy = coord_shift(ix), coord_shift(iy)
    cs = np.array([dix * (1 - fy), dix * fy, diy * (1 - fx), diy * fx])
    return np.array(idx), np.array(wt), np.array(ew), cs


def shift_term(t: np.ndarray, cs: np.ndarray) -> np.ndarray:
    """the coordinate term for taps t [4, N, ...] (zero where outside) and bilinear_weights' factors cs [4, N]"""
    cs = cs.reshape(cs.shape + (1,) * (t.ndim - 2))
    return (cs[0] * np.abs(t[1] - t[0]) + cs[1] * np.abs(t[3] - t[2]) + cs[2] * np.abs(t[2] - t[0]) + cs[3] * np.abs(t[3] - t[1]))


def l2n(x: np.ndarray, axis: int = -1) -> np.ndarray:
    """F.normalize: x / max(||x||_2, 1e-12) (the eps as the fp32 tensor sees it)"""
    return x / np.maximum(np.sqrt((x * x).sum(axis=axis, keepdims=True)), EPS_N)


def round_mantissa(x: np.ndarray, bits: int) -> np.ndarray:
    m, e = np.frexp(x)
    return np.ldexp(np.round(m * 2.0 ** (bits + 1)) / 2.0 ** (bits + 1), e)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


# ---- one frame -----------------------------------------------------------------------------------------------------------
class TailCheck:
    """Checks the tail of one frame.

    K1H [H, W], H1 [H/8, W/8], FEATS [H/8 * W/8 * 64]: the device's fp32 maps.  sel [N, 3]: (x, y, score) of the selected keys in
    output order (xfh_debug_tensor SEL).  kps (KP_DTYPE [nfeatures]), desc [nfeatures, 64], n_valid, mono: the record; n_cand: its
    header's n_candidates.  shape0 = (H0, W0) of the input frame; rescale: keypoints in input coordinates (XFH_FLAG_RESCALE_KEYPOINTS).
    padding: whether the producer writes the padding slots.  `mutate` (tests of the bound only): deliberate reference changes,
    {"window": 3, "nearest": "floor", "align_corners": True, "swap_xy": True, "no_origin_mask": True, "ties": "desc",
     "lap_exclusive": True, "sample_raw": True, "no_renorm": True}.
    """

    def __init__(self, K1H, H1, FEATS, sel, kps, desc, n_valid, mono, n_cand, nfeatures, lapping=(0, 0), shape0=None,
                 rescale=False, padding=True, report: Report | None = None, case: str = "", frame: int = 0, mutate=None):
        self.k1h = np.asarray(K1H, np.float32).astype(np.float64)
        self.H, self.W = self.k1h.shape
        self.h, self.w = self.H // 8, self.W // 8
        self.h1 = np.asarray(H1, np.float64).reshape(-1)
        self.feats = np.asarray(FEATS, np.float64).reshape(self.h * self.w, 64)
        sel = np.asarray(sel, np.float32).reshape(-1, 3)
        self.sx, self.sy = sel[:, 0].astype(np.int64), sel[:, 1].astype(np.int64)
        self.ss = sel[:, 2].copy()
        self.kps, self.desc = kps, np.asarray(desc, np.float32)
        self.n_valid, self.mono, self.n_cand = int(n_valid), int(mono), None if n_cand is None else int(n_cand)
        self.nf, self.lap = int(nfeatures), (int(lapping[0]), int(lapping[1]))
        H0, W0 = shape0 if shape0 is not None else (self.H, self.W)
        f = np.float32
        self.rw = f(np.float64(W0) / self.W) if rescale else f(1)
        self.rh = f(np.float64(H0) / self.H) if rescale else f(1)
        self.padding = padding
        self.report = report if report is not None else Report()
        self.case, self.frame = case, frame
        self.mutate = mutate or {}
        self.near_ties = 0
        self.n_candidates = None

    def cmp(self, stage, dev, ref, tol):
        return self.report.compare(self.case, stage, self.frame, dev, ref, tol)

    def exact(self, stage, ok):
        """an exact predicate per element: err/tol is 0 where it holds, inf where not"""
        ok = np.atleast_1d(np.asarray(ok, bool))
        return self.cmp(stage, (~ok).astype(np.float64), np.zeros(ok.shape), np.zeros(ok.shape))

    # -- stages ------------------------------------------------------------------------------------
    def candidates(self):
        mask = nms_mask(self.k1h, int(self.mutate.get("window", 5)))
        return np.flatnonzero(mask.reshape(-1)), mask

    def scores(self, pix):
        """fp64 score and its bound at flat pixel indices"""
        H, W = self.H, self.W
        x, y = pix % W, pix // W
        ac = bool(self.mutate.get("align_corners"))
        ni, inside = nearest_index(x, y, H, W, self.mutate.get("nearest", "rint"), ac)
        nv = np.where(inside, self.k1h.reshape(-1)[ni], 0.0)
        idx, wt, ew, cs = bilinear_weights(x, y, H, W, self.h, self.w, ac, bool(self.mutate.get("swap_xy")))
        taps = np.where(wt > 0, self.h1[idx], 0.0)
        hb = (wt * taps).sum(axis=0)
        S = np.abs(wt * taps).sum(axis=0)
        tol_hb = 6.0 * U * S + (np.abs(taps) * ew).sum(axis=0) + shift_term(taps, cs) + 8.0 * TINY
        s = nv * hb
        tol = nv * tol_hb * (1.0 + U) + U * np.abs(s) + TINY
        if not self.mutate.get("no_origin_mask"):
            org = pix == 0
            s, tol = np.where(org, -1.0, s), np.where(org, 0.0, tol)
        return s, tol

    def check_nms(self):
        cand, mask = self.candidates()
        self.n_candidates = len(cand)
        if self.n_cand is not None:
            self.cmp("NMS", [self.n_cand], [len(cand)], [0.0])
        inb = (self.sx >= 0) & (self.sx < self.W) & (self.sy >= 0) & (self.sy < self.H)
        self.exact("NMS", inb & mask.reshape(-1)[np.where(inb, self.sy * self.W + self.sx, 0)])
        return cand

    def check_scores(self):
        pix = self.sy * self.W + self.sx
        s, tol = self.scores(pix)
        self.cmp("SCORE", self.ss, s, tol)

    def check_select(self, cand):
        N = len(self.ss)
        self.exact("SELECT", N == min(len(cand), self.nf))
        pix = self.sy * self.W + self.sx
        # strictly ascending key: score descending, ties by pixel index (ascending; "ties": "desc" is the wrong rule)
        a, b = self.ss[:-1], self.ss[1:]
        tie_ok = pix[:-1] > pix[1:] if self.mutate.get("ties") == "desc" else pix[:-1] < pix[1:]
        self.exact("SELECT", (bits(a) != bits(b)) & (a > b) | (bits(a) == bits(b)) & tie_ok)
        self.exact("SELECT", np.unique(pix).size == N)
        # the set against the fp64 top N: a candidate left out may rank above a selected one only within both bounds
        if N and N < len(cand):
            rest = np.setdiff1d(cand, pix, assume_unique=True)
            s_sel, t_sel = self.scores(pix)
            s_rest, t_rest = self.scores(rest)
            r, q = int(np.argmax(s_rest - t_rest)), int(np.argmin(s_sel + t_sel))
            self.cmp("SELECT", [max(s_rest[r] - s_sel[q], 0.0)], [0.0], [t_rest[r] + t_sel[q]])
            self.near_ties = int((s_rest > s_sel.min()).sum())
        self.check_record()

    def check_record(self):
        kps, nf = self.kps, self.nf
        f = np.float32
        valid = self.ss > 0
        kx = (self.sx.astype(f) * self.rw).astype(f)
        ky = (self.sy.astype(f) * self.rh).astype(f)
        lo, hi = f(self.lap[0]), f(self.lap[1])
        back = valid & ((kx > lo) & (kx < hi) if self.mutate.get("lap_exclusive") else (kx >= lo) & (kx <= hi))
        front = valid & ~back
        nF, nB = int(front.sum()), int(back.sum())
        self.exact("SELECT", [self.n_valid == nF + nB, self.mono == nF])
        slot = np.full(len(self.ss), -1, np.int64)
        slot[front] = np.arange(nF)
        slot[back] = nf - 1 - np.arange(nB)
        self.slot = slot
        rank = np.flatnonzero(slot >= 0)
        k = kps[slot[rank]]
        self.exact("SELECT", np.concatenate([
            bits(k["x"]) == bits(kx[rank]), bits(k["y"]) == bits(ky[rank]), k["size"] == 1, k["angle"] == -1,
            bits(k["response"]) == bits(self.ss[rank]), k["octave"] == 0, k["class_id"] == -1]))
        if self.padding:
            pad = np.ones(nf, bool)
            pad[slot[rank]] = False
            p = kps[pad]
            self.exact("SELECT", np.concatenate([p[n] == v for n, v in zip(p.dtype.names, KP_DEFAULT)]))
            self.exact("SELECT", bits(self.desc[pad]).reshape(-1) == 0)

    def descriptors(self, pix):
        """fp64 descriptors at flat pixel indices and their bound [N, 64]"""
        x, y = pix % self.W, pix // self.W
        idx, wt, ew, cs = bilinear_weights(x, y, self.H, self.W, self.h, self.w)
        F = self.feats
        M = F if self.mutate.get("sample_raw") else l2n(F)
        wt, ew = wt[:, :, None], ew[:, :, None]
        m = np.where(wt > 0, M[idx], 0.0)                      # [4, N, 64], zero padding
        v = (wt * m).sum(axis=0)
        am = np.abs(m)
        tol_v = (6.0 * U * (wt * am).sum(axis=0) + (wt * 4.0 * U * am).sum(axis=0) + (am * ew).sum(axis=0) + shift_term(m, cs)
                 + 8.0 * TINY)
        if self.mutate.get("no_renorm"):
            return v, tol_v
        nv = np.sqrt((v * v).sum(axis=1, keepdims=True))
        nt = np.sqrt((tol_v * tol_v).sum(axis=1, keepdims=True))
        y = v / np.maximum(nv, EPS_N)
        tol = (tol_v + np.abs(y) * nt) / np.maximum(nv - nt, EPS_N) + 4.0 * U * np.abs(y) + TINY
        return y, tol

    def check_desc(self):
        rank = np.flatnonzero(self.slot >= 0)
        if not rank.size:
            return
        y, tol = self.descriptors((self.sy * self.W + self.sx)[rank])
        self.cmp("DESC", self.desc[self.slot[rank]], y, tol)

    def run(self):
        cand = self.check_nms()
        self.check_scores()
        self.check_select(cand)
        self.check_desc()
        return self.report


def check_frame(get, rec, nfeatures, lapping, shape0, rescale=False, padding=True, report: Report | None = None, case: str = "",
                frame: int = 0) -> TailCheck:
    """the tail of one frame from a producer's stage tensors: get(name) -> flat fp32 array for "K1H", "H1", "FEATS", "SEL";
    rec = (kps, desc, n_valid, mono_index, n_candidates or None) as Context.parse_records returns it"""
    H0, W0 = shape0
    kps, desc, nv, mono, nc = rec
    tc = TailCheck(np.asarray(get("K1H")).reshape(H0 // 32 * 32, W0 // 32 * 32), get("H1"), get("FEATS"), get("SEL"), kps, desc, nv,
                   mono, nc, nfeatures, lapping, shape0, rescale, padding, report, case, frame)
    tc.run()
    return tc
