"""Optimizer::LocalBundleAdjustment on the device (xfh_local_ba*, include/xfeat_hip.h): the output block of the call stated once, and the wrappers.  The
problem is given as indices into two tables -- pose_table [rows][12] and point_table [rows][3], the map as the tracker's device calls read it -- and
a CSR of edges point by point; see the header for the rule."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .capi import check, lib
from .layout import Layout

HEADER = ("status", "free", "fixed_with_edge", "mono", "stereo", "iterations", "trials", "rejected", "ldlt_failures", "erase")
STATUS = {0: "OK", 1: "ABORTED", 2: "NOTHING_FREE", 3: "FREE_MISMATCH"}
MAX_FREE = 128
TABLE = (("Tcw_out", np.float32, ("nK", 12)), ("points_out", np.float32, ("nP", 3)), ("erase", np.uint8, ("nE",)), ("chi2", np.float32, ("nE",)),
         ("header", np.int32, (len(HEADER),)), ("final_chi2", np.float64, (1,)))
NAMES = tuple(t[0] for t in TABLE)


def local_ba_layout(nK: int, nP: int, nE: int, guard: int = 0) -> Layout:
    """the outputs of local_ba_device inside one buffer, in the order the call takes them; guard > 0 leaves that many bytes the call never writes
    around every array"""
    return Layout.of(TABLE, guard, nK=nK, nP=nP, nE=nE)


def workspace_bytes(nK: int, nP: int, nE: int, n_free: int) -> int:
    return int(lib().xfh_local_ba_workspace_bytes(nK, nP, nE, n_free))


def local_ba_device(ctx, nK: int, n_free: int, nP: int, nE: int, d_pose_table, pose_rows: int, d_point_table, point_rows: int, d_kf_row, d_kf_fixed, d_point_row,
                    d_edge_begin, d_edge_kf, d_edge_obs, cam, d_workspace, d_out, lay: Layout, inv_sigma2: float = 1.0, max_iterations: int = 10,
                    write_back: bool = False):
    """xfh_local_ba_device on device pointers; asynchronous on the ctx stream.  d_out: the address of a buffer of lay["bytes"] bytes, lay =
    local_ba_layout(nK, nP, nE, ..)"""
    check(lib().xfh_local_ba_device(ctx.h, nK, n_free, nP, nE, d_pose_table, pose_rows, d_point_table, point_rows, d_kf_row, d_kf_fixed, d_point_row, d_edge_begin,
                                    d_edge_kf, d_edge_obs, C.byref(cam), float(inv_sigma2), int(max_iterations), int(write_back), d_workspace,
                                    *[d_out + lay[k] for k in NAMES]), ctx.h)


def local_ba(ctx, pose_table, point_table, kf_row, kf_fixed, point_row, edge_begin, edge_kf, edge_obs, cam, inv_sigma2: float = 1.0, max_iterations: int = 10,
             write_back: bool = False):
    """xfh_local_ba (host pointers) -> dict(Tcw_out, points_out, erase, chi2, header (a dict), final_chi2, pose_table, point_table); the two tables
    are copies, refined in place when write_back is set"""
    T = np.ascontiguousarray(pose_table, np.float32).reshape(-1, 12).copy()
    X = np.ascontiguousarray(point_table, np.float32).reshape(-1, 3).copy()
    kr, kf, pr = np.ascontiguousarray(kf_row, np.int32), np.ascontiguousarray(kf_fixed, np.uint8), np.ascontiguousarray(point_row, np.int32)
    eb, ek, eo = np.ascontiguousarray(edge_begin, np.int32), np.ascontiguousarray(edge_kf, np.int32), np.ascontiguousarray(edge_obs, np.float32).reshape(-1, 3)
    nK, nP, nE = len(kr), len(pr), len(ek)
    assert len(kf) == nK and len(eb) == nP + 1 and len(eo) == nE
    o = local_ba_layout(nK, nP, nE).zeros()
    check(lib().xfh_local_ba(ctx.h, nK, int(np.sum(kf == 0)), nP, nE, T.ctypes.data, len(T), X.ctypes.data, len(X), kr.ctypes.data, kf.ctypes.data, pr.ctypes.data,
                             eb.ctypes.data, ek.ctypes.data, eo.ctypes.data, C.byref(cam), float(inv_sigma2), int(max_iterations), int(write_back),
                             *[o[k].ctypes.data for k in NAMES]), ctx.h)
    o["header"] = dict(zip(HEADER, o["header"].tolist()))
    o["final_chi2"] = float(o["final_chi2"][0])
    o["pose_table"], o["point_table"] = T, X
    return o
