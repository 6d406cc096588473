"""The seeded scene of the Fuse tests in device memory (tests/test_gpu_fuse.py, tools/time_fuse.py): the five extracted and finished
frames of tests/projection_rig.py (imported, not changed), map points, normals, distances and descriptors from tests/ref_fuse.py, and
one guarded run of xfh_fuse_search_device.  Problem p searches frame p: problem 0's keyframe is the frame the map points were made
from (every query has its keypoint nearby), problems 1 .. 3 are that frame moved by projection_rig.SHIFTS.  With query_problem_stride
= nq problem p has its OWN query block, the scene's queries rotated by p * ROLL places (FuseRig.block), so a kernel that read block 0
for every problem would answer for the wrong query; with stride 0 there is the one unrotated block.  No test lives here."""
import numpy as np

import guarded
import ref_fuse as RU
import ref_projection as RP
from projection_rig import GUARD, SHIFTS, TUM1, F, Rig, cam_struct
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context

SF, NL = 1.2, 8
OUT_INT = Context.FUSE_OUT_INT
ROLL = 37                 # (odd: a problem's block is no multiple of the four queries of a workgroup away from the next one's)


class FuseRig:
    def __init__(self, L, blob, nf, seed):
        self.rig = r = Rig(L, blob, nf, seed)
        self.nf, self.ctx, self.bounds = nf, r.ctx, r.bounds
        self.sf = RU.scale_factors(SF, NL)
        self.rmax = Context.scale_level_thresholds(SF, NL)
        self.poses = np.stack([RP.pose(seed, (0, 0), cam=TUM1)] + [RP.pose(seed + p, SHIFTS[p - 1], cam=TUM1) for p in (1, 2, 3)])
        self.Ow = np.stack([RU.camera_centre(T) for T in self.poses])
        x, y = r.xy[0][:, 0].copy(), r.xy[0][:, 1].copy()
        self.xyz, self.normals, self.dist, self.flags = RU.scene(seed, r.xy[0], TUM1, self.poses[0], self.rmax, kf=(x, y, r.ur[0]))
        u, v = RU.project(self.poses[0], self.Ow[0], TUM1, self.bounds, 3.0, SF, NL, self.xyz, self.normals, self.dist)[:2]
        self.qdesc = RU.query_descriptors(seed, u, v, x, y, r.recs[0][1], r.recs[0][1])
        self.bufs = []

    def dev(self, a):
        b = capi.DeviceBuffer(max(np.ascontiguousarray(a).nbytes, 16)).upload(a)
        self.bufs.append(b)
        return b

    def block(self, p, xyz=None, normals=None, dist=None, flags=None):
        """the query block of problem p under query_problem_stride = nq: every per-query array rotated by p * ROLL places"""
        pick = lambda a, d: np.ascontiguousarray(d if a is None else a)
        return dict(xyz=np.roll(pick(xyz, self.xyz).astype(F), p * ROLL, 0), normals=np.roll(pick(normals, self.normals).astype(F), p * ROLL, 0),
                    dist=np.roll(pick(dist, self.dist).astype(F), p * ROLL, 0), flags=np.roll(pick(flags, self.flags).astype(np.uint8), p * ROLL),
                    qdesc=np.roll(self.qdesc, p * ROLL, 0))

    def run(self, B, stride0, th, chi2=True, init=256, th_low=RU.TH_LOW, xyz=None, normals=None, dist=None, flags=None, poses=None, Ow=None, uright=True, first=0):
        """B problems (problem p = frame first + p).  stride0: every problem reads ONE block of queries, block(0); otherwise problem p
        reads block(p).  -> (outputs per problem, raw bytes of the output buffer)"""
        nf, ctx, r = self.nf, self.ctx, self.rig
        pick = lambda a, d: np.ascontiguousarray(d if a is None else a)
        blocks = [self.block(p, xyz, normals, dist, flags) for p in range(1 if stride0 else B)]
        pts, nr, dd, fl, qd = (np.concatenate([b[k] for b in blocks]) for k in ("xyz", "normals", "dist", "flags", "qdesc"))
        T = pick(poses, self.poses)[first:first + B].astype(F); O = pick(Ow, self.Ow)[first:first + B].astype(F)
        lay = Context.fuse_search_layout(B, nf, GUARD)
        out = guarded.outputs(lay)
        d = [self.dev(a) for a in (pts, nr, dd, qd, fl, T, O)]
        ctx.fuse_search_device(B, nf, 0 if stride0 else nf, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, d[5].ptr, d[6].ptr, cam_struct(TUM1), self.bounds, th,
                               self.sf, self.rmax, r.fin[3].ptr + first * ctx.grid_bytes(nf), r.rec.ptr + first * ctx.rec_bytes + ctx.desc_off, ctx.rec_bytes, nf,
                               out.ptr, d_uright=r.fin[1].ptr + 4 * nf * first if uright else None, chi2=chi2, init_dist=init, th_low=th_low, guard=GUARD)
        ctx.synchronize()
        raw = guarded.download(out, lay)
        res = guarded.problems(lay.parse(raw), B)
        out.free()
        for b in self.bufs:
            b.free()
        self.bufs = []
        return res, raw

    def model(self, O, f, status, level, u, v, r, ur, chi2=True, init=256, th_low=RU.TH_LOW, uright=True, qdesc=None):
        """the restatement's search on frame f (qdesc: the descriptors of another block than block(0))"""
        rg = self.rig
        x, y = rg.xy[f][:, 0].copy(), rg.xy[f][:, 1].copy()
        return RU.search(O, status, level, u, v, r, ur, self.qdesc if qdesc is None else qdesc, rg.grids[f], x, y, self.bounds, rg.recs[f][1], uright=rg.ur[f] if uright else None,
                         chi2=chi2, init_dist=init, th_low=th_low)

    def close(self):
        self.rig.close()
