"""numpy fp32 restatement of the reference's frame grid and window query (test infrastructure, no GPU):

  Frame::AssignFeaturesToGrid  src/Frame.cc:569-599, with Frame::PosInGrid :918-929 and the inverse cell sizes :336-341
  Frame::GetFeaturesInArea     src/Frame.cc:850-916
  the candidate filters of ORBmatcher::SearchByProjection(Frame, Frame)  src/ORBmatcher.cc:1931-1941

Every expression is evaluated in np.float32 in the reference's operation order; `round` is C roundf (half away from zero).
The grid is (cell_start[64 * 48 + 1], items) with cell = ix * 48 + iy and, inside a cell, ascending keypoint index (push_back
order); a query returns its candidates in the reference's visiting order (ix outer, iy inner, cell order inside).
"""
import struct

import numpy as np

COLS, ROWS = 64, 48
F = np.float32


def geom(bounds):
    """(min_x, min_y, inv_w, inv_h) in fp32: mfGridElementWidthInv = 64 / (mnMaxX - mnMinX), Frame.cc:336-341"""
    mnx, mny, mxx, mxy = (F(b) for b in bounds)
    return mnx, mny, F(COLS) / (mxx - mnx), F(ROWS) / (mxy - mny)


def roundf(v):
    """C roundf on an fp32 array: half away from zero (trunc and the fractional part are exact in fp32)"""
    v = np.asarray(v, F)
    t = np.trunc(v)
    return (t + np.where(np.abs(v - t) >= F(0.5), np.sign(v), F(0)).astype(F)).astype(F)


def cell_of(x, y, bounds):
    """PosInGrid per keypoint: (posX, posY) as float arrays after round, and the mask of keypoints that are binned"""
    mnx, mny, iw, ih = geom(bounds)
    with np.errstate(all="ignore"):
        px = roundf((np.asarray(x, F) - mnx) * iw)
        py = roundf((np.asarray(y, F) - mny) * ih)
    ok = (px >= 0) & (px < COLS) & (py >= 0) & (py < ROWS)
    return px, py, ok


def valid_slots(n, n_valid, mono_index):
    """the valid slots of an extraction record: [0, mono_index) and [n - (n_valid - mono_index), n)"""
    i = np.arange(n)
    return (i < mono_index) | (i >= n - (n_valid - mono_index))


def build(x, y, bounds, use=None):
    """AssignFeaturesToGrid over all slots (`use`: boolean mask of the slots that take part, None = all)
    -> cell_start int32[3073], items int32[n_binned]"""
    px, py, ok = cell_of(x, y, bounds)
    if use is not None:
        ok = ok & np.asarray(use, bool)
    idx = np.nonzero(ok)[0]
    cell = (px[idx].astype(np.int64) * ROWS + py[idx].astype(np.int64))
    order = np.argsort(cell, kind="stable")                 # ascending index inside a cell
    items = idx[order].astype(np.int32)
    cell_start = np.searchsorted(cell[order], np.arange(COLS * ROWS + 1), side="left").astype(np.int32)
    return cell_start, items


def _sat(v, hi):
    """the saturation the library documents for a value the reference would convert with undefined behaviour"""
    return int(min(max(v, F(-1)), F(hi)))


def cell_window(u, v, r, bounds):
    """(c0x, c1x, c0y, c1y) of GetFeaturesInArea, or None where it returns early / the query is not finite"""
    u, v, r = F(u), F(v), F(r)
    if not (np.isfinite(u) and np.isfinite(v) and np.isfinite(r)):
        return None
    mnx, mny, iw, ih = geom(bounds)
    with np.errstate(all="ignore"):
        c0x = max(0, _sat(np.floor((u - mnx - r) * iw), COLS))
        if c0x >= COLS:
            return None
        c1x = min(COLS - 1, _sat(np.ceil((u - mnx + r) * iw), COLS))
        if c1x < 0:
            return None
        c0y = max(0, _sat(np.floor((v - mny - r) * ih), ROWS))
        if c0y >= ROWS:
            return None
        c1y = min(ROWS - 1, _sat(np.ceil((v - mny + r) * ih), ROWS))
        if c1y < 0:
            return None
    return c0x, c1x, c0y, c1y


def features_in_area(grid, x, y, u, v, r, bounds):
    """GetFeaturesInArea: keypoint indices in visiting order"""
    cell_start, items = grid
    w = cell_window(u, v, r, bounds)
    if w is None:
        return np.zeros(0, np.int32)
    c0x, c1x, c0y, c1y = w
    if c1y < c0y:
        return np.zeros(0, np.int32)
    # the cells c0y..c1y of one column are adjacent in cell = ix * 48 + iy: one slice per column, columns in ascending order
    parts = [items[cell_start[ix * ROWS + c0y]:cell_start[ix * ROWS + c1y + 1]] for ix in range(c0x, c1x + 1)]
    cand = np.concatenate(parts) if parts else np.zeros(0, np.int32)
    u, v, r = F(u), F(v), F(r)
    x = np.asarray(x, F); y = np.asarray(y, F)
    keep = (np.abs(x[cand] - u) < r) & (np.abs(y[cand] - v) < r)
    return cand[keep].astype(np.int32)


def csr(grid, x, y, uvr, bounds, skip=None, uright=None, ur_query=None):
    """the candidate lists of all queries, in visiting order, after the optional filters (ORBmatcher.cc:1931-1941)
    -> offsets int32[nq + 1], indices int32"""
    uvr = np.asarray(uvr, F).reshape(-1, 3)
    lists = []
    for q, (u, v, r) in enumerate(uvr):
        c = features_in_area(grid, x, y, u, v, r, bounds)
        if skip is not None:
            c = c[np.asarray(skip)[c] == 0]
        if uright is not None:
            ur = np.asarray(uright, F)[c]
            c = c[~((ur > 0) & (np.abs(F(ur_query[q]) - ur) > F(r)))]
        lists.append(c)
    off = np.concatenate([[0], np.cumsum([len(c) for c in lists])]).astype(np.int32)
    ind = (np.concatenate(lists) if lists else np.zeros(0)).astype(np.int32)
    return off, ind


def make_blob(cs, items, n, x, y, bounds, flags=0):
    """a grid blob as k_grid_build writes it (xfeatslam_amd/csrc/window_layout.h), made on the host"""
    mnx, mny, iw, ih = geom(bounds)
    hdr = struct.pack("<4i6f6i", 0x31474658, n, len(items), flags, bounds[0], bounds[1], bounds[2], bounds[3], iw, ih, *([0] * 6))
    csb = np.zeros(3088, np.int32); csb[:3073] = cs
    it = np.zeros(n, np.dtype([("i", "<i4"), ("x", "<f4"), ("y", "<f4"), ("p", "<i4")]))
    it["i"] = -1
    it["i"][:len(items)] = items; it["x"][:len(items)] = x[items]; it["y"][:len(items)] = y[items]
    return np.frombuffer(hdr + csb.tobytes() + it.tobytes(), np.uint8).copy()
