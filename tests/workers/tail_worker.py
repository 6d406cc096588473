"""Worker of tests/test_gpu_tail.py::test_tail_under_knob: one extraction through the DEBUG build of the library (libxfeat_hip_knobs.so)
with one test knob set in the environment.  argv: frames.npy, out.npz, nfeatures, lap0, lap1, weight family.  The records and the
stage tensors the tail check needs (K1H, H1, FEATS, SEL of every frame) go to out.npz; the check runs in the parent."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    frames_path, out_path, nf, lap0, lap1, family = sys.argv[1:7]
    import numpy as np
    from xfeatslam_amd import capi, weights as WT
    from xfeatslam_amd.extractor import Context
    assert capi.LIB_PATH.endswith("libxfeat_hip_knobs.so"), capi.LIB_PATH
    frames = np.load(frames_path)
    B, H, W = frames.shape
    ctx = Context(nfeatures=int(nf), max_height=H, max_width=W, max_batch=B)
    ctx.load_weights(WT.pack_blob(WT.make_family(family, 5)))
    raw = np.empty(B * ctx.rec_bytes, np.uint8)
    capi.check(capi.lib().xfh_extract_batch(ctx.h, frames.ctypes.data, B, H, W, int(lap0), int(lap1), raw.ctypes.data), ctx.h)
    out = {"records": raw}
    for b in range(B):
        for name in ("K1H", "H1", "FEATS", "SEL"):
            out[f"{name}_{b}"] = ctx.debug_tensor(capi.T[name], b)
    np.savez(out_path, **out)
    ctx.close()


if __name__ == "__main__":
    main()
