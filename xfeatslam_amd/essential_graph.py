"""Optimizer::OptimizeEssentialGraph on the device (xfh_essential_graph*, include/xfeat_hip.h): the output block of the call stated once, and the
wrappers.  The problem is given as indices into two tables -- pose_table [rows][12] and point_table [rows][3], the map as the tracker's device calls
read it --, a table of Sim3 entries (CorrectedSim3 / NonCorrectedSim3 as CorrectLoop computed them) and three edge arrays in the reference's creation
order; see the header for the rule."""
from __future__ import annotations

import numpy as np

from .capi import check, lib
from .layout import Layout

HEADER = ("status", "free", "edges", "loop_edges", "iterations", "trials", "rejected", "ldlt_failures", "points")
STATUS = {0: "OK", 1: "NOTHING_FREE", 2: "FREE_MISMATCH", 3: "NO_EDGES"}
MAX_FREE = 192
MAX_ITERATIONS = 20
TABLE = (("Sim3_out", np.float64, ("nV", 8)), ("Tcw_out", np.float32, ("nV", 12)), ("points_out", np.float32, ("nP", 3)), ("chi2", np.float32, ("nE",)),
         ("header", np.int32, (len(HEADER),)), ("final_chi2", np.float64, (1,)))
NAMES = tuple(t[0] for t in TABLE)
INPUTS = (("pose_table", np.float32), ("point_table", np.float32), ("kf_row", np.int32), ("kf_fixed", np.uint8), ("corrected_index", np.int32),
          ("noncorrected_index", np.int32), ("sim3", np.float64), ("edge_i", np.int32), ("edge_j", np.int32), ("edge_kind", np.int32), ("point_row", np.int32),
          ("point_ref", np.int32))


def essential_graph_layout(nV: int, nP: int, nE: int, guard: int = 0) -> Layout:
    """the outputs of essential_graph_device inside one buffer, in the order the call takes them; guard > 0 leaves that many bytes the call never
    writes around every array"""
    return Layout.of(TABLE, guard, nV=nV, nP=nP, nE=nE)


def workspace_bytes(nV: int, nE: int, n_free: int) -> int:
    return int(lib().xfh_essential_graph_workspace_bytes(nV, nE, n_free))


def essential_graph_device(ctx, nV: int, n_free: int, nE: int, nP: int, nS: int, d_pose_table, pose_rows: int, d_point_table, point_rows: int, d_kf_row, d_kf_fixed,
                           d_corrected_index, d_noncorrected_index, d_sim3, d_edge_i, d_edge_j, d_edge_kind, d_point_row, d_point_ref, d_workspace, d_out, lay: Layout,
                           fix_scale: bool = False, max_iterations: int = MAX_ITERATIONS, write_back: bool = False):
    """xfh_essential_graph_device on device pointers; SYNCHRONOUS (the host reads a control record back after every trial).  d_out: the address of a
    buffer of lay["bytes"] bytes, lay = essential_graph_layout(nV, nP, nE, ..)"""
    check(lib().xfh_essential_graph_device(ctx.h, nV, n_free, nE, nP, nS, d_pose_table, pose_rows, d_point_table, point_rows, d_kf_row, d_kf_fixed, d_corrected_index,
                                           d_noncorrected_index, d_sim3, d_edge_i, d_edge_j, d_edge_kind, d_point_row, d_point_ref, int(fix_scale), int(max_iterations),
                                           int(write_back), d_workspace, *[d_out + lay[k] for k in NAMES]), ctx.h)


def host_arrays(p):
    """the inputs of a problem dict as the contiguous arrays the C ABI takes, in INPUTS order (copies)"""
    shapes = {"pose_table": (-1, 12), "point_table": (-1, 3), "sim3": (-1, 8)}
    return [np.ascontiguousarray(np.asarray(p[k], dt)).reshape(shapes.get(k, (-1,))).copy() for k, dt in INPUTS]


def essential_graph(ctx, pose_table, point_table, kf_row, kf_fixed, corrected_index, noncorrected_index, sim3, edge_i, edge_j, edge_kind, point_row, point_ref,
                    fix_scale: bool = False, max_iterations: int = MAX_ITERATIONS, write_back: bool = False):
    """xfh_essential_graph (host pointers) -> dict(Sim3_out, Tcw_out, points_out, chi2, header (a dict), final_chi2, pose_table, point_table); the two
    tables are copies, corrected in place when write_back is set"""
    a = host_arrays(dict(zip([k for k, _ in INPUTS], (pose_table, point_table, kf_row, kf_fixed, corrected_index, noncorrected_index, sim3, edge_i, edge_j, edge_kind,
                                                      point_row, point_ref))))
    nV, nS, nE, nP = len(a[2]), len(a[6]), len(a[7]), len(a[10])
    assert len(a[3]) == len(a[4]) == len(a[5]) == nV and len(a[8]) == len(a[9]) == nE and len(a[11]) == nP
    o = essential_graph_layout(nV, nP, nE).zeros()
    check(lib().xfh_essential_graph(ctx.h, nV, int(np.sum(a[3] == 0)), nE, nP, nS, a[0].ctypes.data, len(a[0]), a[1].ctypes.data, len(a[1]), *[x.ctypes.data for x in a[2:]],
                                    int(fix_scale), int(max_iterations), int(write_back), *[o[k].ctypes.data for k in NAMES]), ctx.h)
    o["header"] = dict(zip(HEADER, o["header"].tolist()))
    o["final_chi2"] = float(o["final_chi2"][0])
    o["pose_table"], o["point_table"] = a[0], a[1]
    return o
