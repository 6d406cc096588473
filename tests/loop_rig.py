"""The seeded scenes of the loop-closing / relocalisation tests in device memory (tests/test_gpu_loop.py, tools/time_loop.py): the five
extracted and finished frames of tests/projection_rig.py (imported, not changed), the map points of tests/ref_loop.py, and one guarded
run of xfh_map_projection_search_device or xfh_sim3_search_device.

Map projection: problem p searches frame p with pose p, its OWN query block (the scene's queries rotated by p * ROLL places -- the loop
is sequential, so a rotated block is another problem, not the same answers rotated) and its own taken bytes; with target_shared every
problem searches frame 0.  Problem 0 is the scene whose conditions tests/test_loop_ref.py asserts.
SearchBySim3: side 1 is frame 0, side 2 of problem p is frame p, each problem with its own Sim3 and poses and its own flags on side 1;
with side1_shared every problem reads problem 0's side 1.  No test lives here."""
import numpy as np

import guarded
import ref_fuse as RU
import ref_loop as RL
import ref_projection as RP
from projection_rig import GUARD, SHIFTS, TUM1, F, Rig, cam_struct
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context

SF, NL = 1.2, 8
ROLL = 37
MAP_INT = Context.MAPPROJ_OUT_INT
SIM3_INT = Context.SIM3_OUT_INT
SIDE_IN = ("points", "dist", "mp_desc", "flags")


class LoopRig:
    def __init__(self, L, blob, nf, seed, O):
        self.rig = r = Rig(L, blob, nf, seed)
        self.nf, self.ctx, self.bounds, self.O, self.seed = nf, r.ctx, r.bounds, O, seed
        self.sf = RU.scale_factors(SF, NL)
        self.rmax = Context.scale_level_thresholds(SF, NL)
        self.poses = np.stack([RP.pose(seed, (0, 0), cam=TUM1)] + [RP.pose(seed + p, SHIFTS[p - 1], cam=TUM1) for p in (1, 2, 3)])
        self.Ow = np.stack([RU.camera_centre(T) for T in self.poses])
        self.scene = RL.map_scene(O, seed, r.xy[0], r.recs[0][1], TUM1, self.poses[0], self.bounds, self.rmax)
        # SearchBySim3: problem 0 is the pair tests/test_loop_ref.py looks at (both keyframes are frame 0)
        self.pairs, self.s1, self.s2 = [], [], []
        for p in range(4):
            T1, T2, M21, M12 = RL.sim3_pair(seed + 10 * p, TUM1) if p == 0 else RL.sim3_pair(seed + 10 * p, TUM1, SHIFTS[p - 1])
            self.pairs.append((T1, T2, M21, M12))
            s1 = RL.sim3_side(seed, r.xy[0], r.recs[0][1], r.xy[p], r.recs[p][1], TUM1, T1, M21, self.bounds, self.rmax)
            s1["flags"] = np.roll(s1["flags"], p * ROLL)
            self.s1.append(s1)
            self.s2.append(RL.sim3_side(seed + 1 + p, r.xy[p], r.recs[p][1], r.xy[0], r.recs[0][1], TUM1, T2, M12, self.bounds, self.rmax))
        self.bufs = []
        self.grid0 = {}

    def dev(self, a):
        b = capi.DeviceBuffer(max(np.ascontiguousarray(a).nbytes, 16)).upload(a)
        self.bufs.append(b)
        return b

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []

    def grid0_tiled(self, B):
        """frame 0's grid blob B times over: side 1 of B unshared SearchBySim3 problems"""
        if B not in self.grid0:
            g = self.rig.fin[3].download(np.uint8, self.ctx.grid_bytes(self.nf))
            self.grid0[B] = capi.DeviceBuffer(B * len(g)).upload(np.tile(g, B))
        return self.grid0[B]

    # ---- map projection ----------------------------------------------------------------------------------------------------------
    def block(self, p, **over):
        """the query block and the taken bytes of problem p"""
        sc = dict(self.scene); sc.update({k: v for k, v in over.items() if v is not None})
        b = {k: np.roll(np.ascontiguousarray(sc[k]), p * ROLL, 0) for k in ("xyz", "normals", "dist", "flags", "qdesc")}
        b["taken"] = np.roll(sc["taken"], 13 * p)
        return b

    def run_map(self, B, th, form, accept, shared=False, first=0, taken=True, poses=None, Ow=None, **over):
        """problems first .. first + B - 1 -> (outputs per problem, raw bytes of the output buffer, workspace header ints [B][4])"""
        nf, ctx, r = self.nf, self.ctx, self.rig
        blocks = [self.block(first + p, **over) for p in range(B)]
        cat = lambda k, t: np.ascontiguousarray(np.concatenate([b[k] for b in blocks]), t)
        T = np.ascontiguousarray((self.poses if poses is None else poses)[first:first + B], F)
        Ow = np.ascontiguousarray((self.Ow if Ow is None else Ow)[first:first + B], F)
        d = [self.dev(a) for a in (cat("xyz", F), cat("normals", F), cat("dist", F), cat("qdesc", F), cat("flags", np.uint8), T, Ow)]
        dtk = self.dev(cat("taken", np.uint8)) if taken else None
        lay = Context.map_projection_search_layout(B, nf, nf, GUARD)
        out = guarded.outputs(lay)
        ws = guarded.Guarded(Context.map_projection_search_workspace_bytes(nf, nf, B), GUARD)
        f0 = 0 if shared else first
        ctx.map_projection_search_device(form, B, nf, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, d[5].ptr, d[6].ptr, cam_struct(TUM1), self.bounds, th,
                                         self.sf, self.rmax, r.fin[3].ptr + f0 * ctx.grid_bytes(nf), r.rec.ptr + f0 * ctx.rec_bytes + ctx.desc_off, ctx.rec_bytes,
                                         1 if shared else 0, nf, ws.ptr, out.ptr, d_taken=dtk.ptr if dtk else None, accept_max=accept, guard=GUARD)
        ctx.synchronize()
        raw = guarded.download(out, lay)
        res = guarded.problems(lay.parse(raw), B)
        per = Context.search_projection_workspace_bytes(nf, nf, 1)
        wraw = ws.download()
        hdr = np.stack([wraw[p * per:p * per + 16].view(np.int32) for p in range(B)])
        out.free(); ws.free(); self.free()
        return res, raw, hdr

    def model_map(self, f, status, level, u, v, r, blk, accept, taken=True):
        """the restatement's loop on frame f"""
        rg = self.rig
        x, y = rg.xy[f][:, 0].copy(), rg.xy[f][:, 1].copy()
        return RL.map_search(self.O, status, level, u, v, r, blk["qdesc"], rg.grids[f], x, y, self.bounds, rg.recs[f][1], taken=blk["taken"] if taken else None,
                             accept_max=accept)

    # ---- SearchBySim3 ------------------------------------------------------------------------------------------------------------------
    def problem(self, p, shared=False, **over):
        """(side 1, side 2, T1w, T2w, M21, M12) of problem p as host arrays; over: replacements by name (points1, dist2, T1w, M21, ...)"""
        T1, T2, M21, M12 = self.pairs[p]
        s1 = dict(self.s1[0 if shared else p]); s2 = dict(self.s2[p])
        if shared:
            T1 = self.pairs[0][0]
        for k, val in over.items():
            if val is None:
                continue
            if k[:-1] in SIDE_IN:
                (s1 if k[-1] == "1" else s2)[k[:-1]] = val
        T1, T2, M21, M12 = (over.get(n) if over.get(n) is not None else d for n, d in (("T1w", T1), ("T2w", T2), ("M21", M21), ("M12", M12)))
        return s1, s2, np.asarray(T1, F), np.asarray(T2, F), np.asarray(M21, F), np.asarray(M12, F)

    def run_sim3(self, B, th, shared=False, first=0, th_high=RL.TH_HIGH, **over):
        """problems first .. first + B - 1 -> (outputs per problem, raw bytes of the output buffer)"""
        nf, ctx, r = self.nf, self.ctx, self.rig
        pr = [self.problem(first + p, shared, **over) for p in range(B)]
        lay = Context.sim3_search_layout(B, nf, nf, GUARD)
        out = guarded.outputs(lay)
        types = dict(points=F, dist=F, mp_desc=F, flags=np.uint8)
        n1 = 1 if shared else B
        d1 = {k: self.dev(np.ascontiguousarray(np.concatenate([pr[p][0][k] for p in range(n1)]), types[k])) for k in SIDE_IN}
        d2 = {k: self.dev(np.ascontiguousarray(np.concatenate([pr[p][1][k] for p in range(B)]), types[k])) for k in SIDE_IN}
        dT1 = self.dev(np.stack([pr[p][2] for p in range(n1)])); dT2 = self.dev(np.stack([pr[p][3] for p in range(B)]))
        dM21 = self.dev(np.stack([pr[p][4] for p in range(B)])); dM12 = self.dev(np.stack([pr[p][5] for p in range(B)]))
        g1 = r.fin[3].ptr if shared else self.grid0_tiled(B).ptr
        rows = lambda f: r.rec.ptr + f * ctx.rec_bytes + ctx.desc_off
        side1 = Context.sim3_side(nf, g1, rows(0), 0, d1["points"].ptr, d1["dist"].ptr, d1["mp_desc"].ptr, d1["flags"].ptr, dT1.ptr, out.ptr, lay, "1")
        side2 = Context.sim3_side(nf, r.fin[3].ptr + first * ctx.grid_bytes(nf), rows(first), ctx.rec_bytes, d2["points"].ptr, d2["dist"].ptr, d2["mp_desc"].ptr,
                                  d2["flags"].ptr, dT2.ptr, out.ptr, lay, "2")
        ctx.sim3_search_device(B, 1 if shared else 0, side1, side2, dM21.ptr, dM12.ptr, cam_struct(TUM1), self.bounds, th, self.sf, self.rmax,
                               out.ptr + lay["match12"], out.ptr + lay["n_found"], th_high=th_high)
        ctx.synchronize()
        raw = guarded.download(out, lay)
        res = guarded.problems(lay.parse(raw), B)
        out.free(); self.free()
        return res, raw

    def model_sim3(self, f, status, level, u, v, r, mp_desc, th_high=RL.TH_HIGH):
        """one direction of the restatement: the queries search frame f"""
        rg = self.rig
        x, y = rg.xy[f][:, 0].copy(), rg.xy[f][:, 1].copy()
        return RL.sim3_search(self.O, status, level, u, v, r, mp_desc, rg.grids[f], x, y, self.bounds, rg.recs[f][1], th_high)

    def kps(self, f):
        k = np.zeros(self.nf, capi.KP_DTYPE); k["x"] = self.rig.xy[f][:, 0]; k["y"] = self.rig.xy[f][:, 1]
        return k

    def close(self):
        for b in self.grid0.values():
            b.free()
        self.rig.close()
