"""bench.py as every change runs it: a plain run (set up, warm up, K timed steps, one JSON line, none of the --full legs) and
--dump-outputs, whose files hold the records of the last timed step -- the records a ctx of its own produces for the same frames,
and the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "3", "--streams", "2", "--height", "96", "--width", "128"]


def _bench(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *ARGS, "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, lines                                        # stdout is the JSON line alone
    return json.loads(lines[0])


def _load(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_bench_plain_run_dumps_last_step_records(gpu_lib, tmp_path):
    import bench
    from xfeatslam_amd import synth, weights as WT
    from xfeatslam_amd.extractor import Context
    line = _bench(tmp_path / "a")
    assert (line["steps"], line["warmup"], line["n_gpus"]) == (3, 1, 1)
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "f32" and line["value"] > 0
    assert np.isclose(line["value"] * line["ms_per_step"] * 1e-3, 6, rtol=1e-9)          # 2 sub-batches x 3 frames per timed step
    for leg in ("roofline", "host_visible", "host_api", "match", "aux_kernels", "cpu_baseline", "parity", "bn_eval_modes"):
        assert leg not in line, leg                                      # --full only
    got = _load(tmp_path / "a")
    assert set(got) == {"header.npy", "frame_index.npy", "keypoints.npy", "descriptors.npy"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values()) and sum(a.nbytes for a in got.values()) < 64 << 20
    # the same frames and weights through a ctx of the test's own (per-frame statistics: the sub-batch a frame sat in does not matter)
    blob = WT.pack_blob(WT.make_synthetic(1234, bench.KP_GAIN, with_bn=True))
    ctx = Context(nfeatures=bench.NFEATURES, max_height=96, max_width=128, max_batch=6)
    ctx.load_weights(blob)
    want = ctx.extract_batch(synth.frames(6, 96, 128, seed=42))
    ctx.close()
    assert np.array_equal(got["header.npy"], np.array([[nv, mono, nc] for _, _, nv, mono, nc in want], np.float64))
    pick = got["frame_index.npy"].astype(int)
    assert pick.tolist() == list(range(6))                               # fewer frames than the sample size: all of them
    assert got["keypoints.npy"].shape == (6, bench.NFEATURES, 7) and got["descriptors.npy"].shape == (6, bench.NFEATURES, 64)
    for j, i in enumerate(pick):
        k, d = want[i][0], want[i][1]
        assert np.array_equal(got["keypoints.npy"][j], np.stack([k[f].astype(np.float32) for f in k.dtype.names], -1), equal_nan=True), i
        assert np.array_equal(got["descriptors.npy"][j], d, equal_nan=True), i
    # same arguments, same inputs: a second run writes the same outputs
    _bench(tmp_path / "b")
    again = _load(tmp_path / "b")
    assert all(np.array_equal(got[f], again[f], equal_nan=True) for f in got)
