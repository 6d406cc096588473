"""The large-batch keypoint head (k_heads_kp: keypoint_head.3 on the matrix cores, dustbin chain on the VALU, two lanes per cell in the
softmax) and the feature norms computed inside the fusion chain (k_chain1x1<FNRM>), both selected for batches > 8.

Every case checks the first and the last frame of a batch of 9 (the first size that takes these forms) or 12:
  * XFH_T_K1H and XFH_T_M1N bit-equal to the oracle's stage tensors (M1N: the GPU stores the norm per cell and never the normalised
    map; xfh_debug_tensor forms FEATS / norm, so one wrong norm shows in 64 values),
  * the same two tensors and the whole record bit-equal to the frame extracted alone (B = 1: k_heads_kp4 as a kernel or a rider,
    the norms riding on the NMS launch),
  * the record against the oracle's as test_gpu_extract.py does: counts, keypoint set, descriptors.
Shapes are in cells of 8 x 8 pixels, 128 cells per block and 32 per wave of the head kernel:
  32 x 64   ->  32 cells: one wave, the rest of the block empty
  96 x 160  -> 240 cells: one full block, then three full waves and a half one
  64 x 416  -> 416 cells: a partial last block; 52 cells per map row, so map rows straddle wave and block boundaries
BatchNorm modes: the oracle knows batch statistics and running statistics.  It has no folded mode (folding re-rounds the weights:
test_gpu_extract.py::test_running_folded_mode compares that mode by tolerance), so the folded case is compared bit for bit with
the B = 1 forms of the same mode only."""
import functools

import numpy as np
import pytest

from conftest import joined_desc_diff, kp_set
from xfeatslam_amd import capi, synth, weights as WT

pytestmark = pytest.mark.gpu
NF, LAP, DESC_TOL = 256, (0, 40), 1e-4
SHAPES = [(32, 64), (96, 160), (64, 416)]


@functools.lru_cache(maxsize=None)
def _blob(gain, with_bn):
    return WT.pack_blob(WT.make_synthetic(1234, gain, with_bn=with_bn))


@functools.lru_cache(maxsize=None)
def _frames(H, W):
    fr = synth.frames(12, H, W, seed=31)
    fr.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def _oracle(gain, with_bn, bn_mode, H, W, i):
    """(record, K1H, M1N) of frame i of _frames(H, W): computed once, shared by every case that needs it"""
    from oracle import oracle as O
    orc = O.Oracle(_blob(gain, with_bn), bn_mode=bn_mode)
    rec = orc.extract(_frames(H, W)[i], NF, LAP)
    return rec, orc.tensor(O.T["K1H"]), orc.tensor(O.T["M1N"])


def _extract(blob, fr, bn_mode, which):
    """records of every frame, and {frame: (K1H, M1N)} of the frames in `which`"""
    from xfeatslam_amd.extractor import Context
    B, H, W = fr.shape
    ctx = Context(nfeatures=NF, max_height=H, max_width=W, max_batch=B, bn_mode=bn_mode)
    ctx.load_weights(blob)
    recs = ctx.extract_batch(fr, LAP)
    tens = {i: (ctx.debug_tensor(capi.T["K1H"], i), ctx.debug_tensor(capi.T["M1N"], i)) for i in which}
    ctx.close()
    return recs, tens


def _same_record(a, b):
    return a[2:] == b[2:] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _check(H, W, B, gain=1.0, bn_mode=0, oracle_mode=0):
    """oracle_mode None: no oracle comparison (see the module text)"""
    with_bn = bn_mode != 0
    blob = _blob(gain, with_bn)
    fr = _frames(H, W)[:B]
    recs, tens = _extract(blob, fr, bn_mode, (0, B - 1))
    for i in (0, B - 1):
        k1h, m1n = tens[i]
        assert k1h.size == H * W and m1n.size == (H // 8) * (W // 8) * 64
        (rec1,), t1 = _extract(blob, fr[i:i + 1], bn_mode, (0,))
        assert np.array_equal(k1h, t1[0][0]), f"K1H of frame {i} differs from the B = 1 form"
        assert np.array_equal(m1n, t1[0][1]), f"M1N of frame {i} differs from the B = 1 form"
        assert _same_record(recs[i], rec1), f"record of frame {i} differs from the B = 1 form"
        if oracle_mode is None:
            continue
        (ok, od, onv, omono), ok1h, om1n = _oracle(gain, with_bn, oracle_mode, H, W, i)
        assert np.array_equal(k1h, ok1h), f"K1H of frame {i} differs from the oracle"
        assert np.array_equal(m1n, om1n), f"M1N of frame {i} differs from the oracle"
        hk, hd, hnv, hmono, _ = recs[i]
        assert (hnv, hmono) == (onv, omono) and kp_set(hk) == kp_set(ok), i
        dd, ds, n = joined_desc_diff(hk, hd, ok, od)
        assert n == onv and dd < DESC_TOL and ds < 1e-6, (i, dd, ds, n, onv)


@pytest.mark.parametrize("B", [9, 12])
@pytest.mark.parametrize("H,W", SHAPES)
def test_heads_and_norms_match_oracle_and_single_frame(gpu_lib, oracle_mod, H, W, B):
    _check(H, W, B)


@pytest.mark.parametrize("H,W", SHAPES)
def test_running_statistics(gpu_lib, oracle_mod, H, W):
    """statistics from the weight file, applied through the same slots the finalize kernel fills in batch mode"""
    _check(H, W, 12, bn_mode=1, oracle_mode=1)


@pytest.mark.parametrize("H,W", SHAPES)
def test_folded_batchnorm(gpu_lib, H, W):
    """BatchNorms folded into the weights: identity statistics in the slots; the two-stage chain with a bias + ReLU epilogue"""
    _check(H, W, 12, bn_mode=2, oracle_mode=None)


def test_large_keypoint_logits(gpu_lib):
    """the benchmark's weights (keypoint-logit gain 6.0): most softmax terms are small and some fall below 1e-20, where div_by's
    quotient may differ from IEEE division in the last denormal bits (heads_kp4.hip.h) -- existing behaviour that both batch forms
    share through the same helper, so they are compared with each other, bit for bit"""
    _check(96, 160, 12, gain=6.0, oracle_mode=None)
