#!/usr/bin/env python
"""bench.py -- XFeat front-end throughput on MI355X (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--height 480 --width 640] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

torch.distributed.run only LAUNCHES the ranks (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in the environment); this
script imports no torch: device memory, streams and the RCCL exchange all go through the C ABI of libxfeat_hip.so.

A "step" is one pass of the extraction hot path (XFextractor::operator(), reference src/XFextractor.cc:250-356) over
one batch of B distinct synthetic VGA frames per GPU, with the frames already resident in HBM and the 4096-row
(keypoints, descriptors) records left in HBM (the task's rule for `value`); with N > 1 the step also moves the records
with RCCL (frame i -> GPU i mod N; xfh_allgather_records by default, --gather root|compact for the cheaper
forms) on the ctx's communication stream, overlapped with the next step.  `value` = frames/s over all GPUs, `ms_per_step` =
milliseconds per timed step (K of them after W untimed ones).  A plain run does only that: set up, warm up, time the K steps,
print the JSON line.  --dump-outputs DIR also writes the records of the last timed step as .npy files (dump_outputs below; the
inputs are the same from run to run, so two builds can be compared output for output).  With --full the same JSON line carries:
  host_visible  SURVEY.md 8d read literally: the same frames from (pinned) HOST memory to records in HOST memory through
                xfh_extract_batch_submit / _wait (csrc/pipeline.cpp), PCIe inside the clock, with the fraction of the PCIe rate
  roofline      dominant extraction kernel (3x3 64->64 at 1/8 resolution): algorithmic flops / average launch duration of the
                kernel alone on the GPU (HIP events attached to every dispatch); `in_timed_region` = the same events inside the
                timed region, where the launches share the CUs with the other sub-batches
  configs3      BASELINE.json configs[3]: one 1280x720 frame per rank per step + the gather, all three gather forms (N > 1);
                with one GPU the batch of 8 on that GPU
  gather_forms  (N > 1) the headline workload under the two gather forms that are not the default
  extract_only  (N > 1) the headline workload without any exchange: extraction scaling apart from the gather
  single_frame  one frame per call, device resident (latency path)
  host_api      what the drop-in operator() really does: xfh_extract from host memory (H2D + kernels + record to host
                inside the clock), synchronous latency and pipelined (2 frames in flight) throughput, nfeatures 4096 / 1000
  match         4096 x 4096 MNN: whole call on raw descriptor rows (3 launches), on prepared images (2 launches), through
                the host API, and the MFMA roofline of k_mnn_gemm_img
  aux_kernels   k_dist_i32, k_best2_csr, k_distinctive_csr timings
  cpu_baseline  the oracle (oracle/, a C restatement of the reference; "port") on the host cores: all cores and 1 thread; and
                `libtorch_ops`: oracle/torch_restatement.py (the reference's own libtorch CPU operators, statement by statement)
                timed in a child process on the same cores
  parity        GPU output of frame 0 / the match against the oracle, and a near-tie audit of the discrete decisions
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3      # /opt/skills/guides/MI355X_MICROARCH.md, dense f32 MFMA

# MFMA-busy of the dominant kernels from the builder's SQ-counter pass over a serial 64-frame step (tools/pmc_kernels.sh -> profiles/r04_pmc_kernels_B64.json)
PMC_BUSY_SRC = ("profiles/r06_pmc_kernels_B64.json (the newest earlier round's file if that one is missing): SQ_VALU_MFMA_BUSY_CYCLES (busy SIMD-cycles, calibrated on a pure MFMA loop) / (launch duration x 1024 SIMDs x 2.4 GHz) from the "
                "builder's rocprofv3 --pmc pass over a serial 64-frame step; a constant in this run, not an observation of it")
_pmck = {}
for _tag in ("r06", "r05", "r04"):
    try:
        _pmck = json.load(open(os.path.join(ROOT, "profiles", _tag + "_pmc_kernels_B64.json")))["kernels"]
        break
    except Exception:
        pass

def pmc_busy(prefix):
    for k_, v_ in _pmck.items():
        if k_.startswith(prefix) and v_.get("mfma_busy_pct") is not None:
            return v_["mfma_busy_pct"] / 100.0
    return None

NFEATURES = 4096
KP_GAIN = 6.0                     # "dense" synthetic weights: > 4096 NMS candidates at VGA
DOMINANT_LAYERS = (7, 17)         # k_conv_mfma<64,64,3,1,4,2,1,16,PRO_BN,EPI_STATS,32>: block3.1, block_fusion.1


# (cin, cout, kernel, output resolution divisor) of every convolution of the network (reference src/XFeat.cc:27-103)
NET_CONVS = [(1, 4, 3, 1), (4, 8, 3, 2), (8, 8, 3, 2), (8, 24, 3, 4), (24, 24, 3, 4), (24, 24, 3, 4), (24, 64, 3, 8), (64, 64, 3, 8), (64, 64, 1, 8),
             (64, 64, 3, 16), (64, 64, 3, 16), (64, 64, 3, 16), (64, 128, 3, 32), (128, 128, 3, 32), (128, 128, 3, 32), (128, 64, 1, 32),
             (64, 64, 3, 8), (64, 64, 3, 8), (64, 64, 1, 8), (64, 64, 1, 8), (64, 64, 1, 8), (64, 1, 1, 8), (64, 64, 1, 8), (64, 64, 1, 8), (64, 64, 1, 8),
             (64, 65, 1, 8), (1, 24, 1, 4)]


def net_flops(H, W):
    """algorithmic flops of all convolutions of one frame (2 * K * K * Cin * Cout per output pixel): 2.62 GFLOP at VGA"""
    return float(sum(2 * k * k * ci * co * (H // d) * (W // d) for ci, co, k, d in NET_CONVS))


GATHER_TEXT = {"allgather": "all-gather (ncclAllGather) of the records", "root": "gather of the records into rank 0 (send / recv group)",
               "compact": "gather of the compact records (header + valid rows) into rank 0"}
BN_MODES = {"batch": 0, "running": 1, "folded": 2}
BN_TEXT = {"batch": "per-frame BatchNorm statistics", "running": "NOT the reference's semantics: running BatchNorm statistics, upstream eval()",
           "folded": "NOT the reference's semantics: eval() BatchNorm folded into the convolution weights"}


def conv_flops(H, W):
    """algorithmic flops per frame of the 3x3 64->64 layer at 1/8 resolution"""
    return 2.0 * (H // 8) * (W // 8) * 64 * 64 * 9


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def usable_cores():
    """hardware threads this process may really use: affinity mask, capped by the cgroup CPU quota"""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = min(n, max(1, int(int(q) / int(p))))
    except (OSError, ValueError):
        pass
    return max(1, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64, help="frames per sub-batch (per GPU per step: batch x streams)")
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--streams", type=int, default=4, help="sub-batches in flight per GPU (one ctx with its own HIP streams each)")
    ap.add_argument("--match-iters", type=int, default=300)
    ap.add_argument("--match-warm-ms", type=float, default=60.0, help="untimed C-loop calls in front of every measured loop of the match leg (the GPU's clock settles "
                                                                     "over ~20 ms of load); profiler passes that only count per launch set 0")
    ap.add_argument("--match-pairs", type=int, default=8, help="pairs of the batched match leg (frame 0 against this many partner frames in one call)")
    ap.add_argument("--cpu-frames", type=int, default=8, help="frames of the bounded all-core CPU-baseline sample (0 = skip)")
    ap.add_argument("--gather", choices=["allgather", "root", "compact"], default="allgather",
                    help="how the records reach the SLAM rank with N > 1: allgather = ncclAllGather (default: the collective BASELINE.json / SURVEY.md 8e name), "
                         "root = send/recv group into rank 0 only (rank 0 is the only consumer; an all-gather lands N x 298 MB per step in EVERY GPU), "
                         "compact = header + valid rows to rank 0")
    ap.add_argument("--force-comm", action="store_true", help="run the RCCL exchange also with one rank")
    ap.add_argument("--full", action="store_true", help="everything beyond the headline as well: the conv roofline (dispatch events inside the timed region, then an "
                                                        "isolated run), the multi-rank legs and the extra legs (host_visible / configs3 / host_api / match / aux / cpu / parity); "
                                                        "without it a run sets up, warms up, times the steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write the records the last timed step produced as .npy files into DIR "
                                                                        "(rank 0; float32 / float64, a fixed sample of frames, < 64 MB)")
    ap.add_argument("--no-legs", action="store_true", help="with --full: timed region and conv roofline only (no host_visible / configs3 / host_api / match / aux / cpu legs)")
    ap.add_argument("--host-steps", type=int, default=24, help="steps of the host-visible leg (each: the same frames per GPU as a timed step)")
    ap.add_argument("--libtorch-leg", type=str, default="", help=argparse.SUPPRESS)        # child process of the cpu_baseline leg: "threads,threads,..."
    ap.add_argument("--only-match-leg", action="store_true", help="of the extra legs run the matcher ones only (short traces for the PMC passes)")
    ap.add_argument("--no-bn-leg", action="store_true", help="skip the eval()-BatchNorm legs (their kernels share names with the headline's in a kernel trace)")
    ap.add_argument("--serial-branch", action="store_true", help="XFH_FLAG_SERIAL_BRANCH: no overlapping kernels (for per-kernel profiles)")
    ap.add_argument("--bn", choices=["batch", "running", "folded"], default="batch",
                    help="BatchNorm mode of the timed region: batch = the reference's per-frame statistics (the headline), running = upstream eval(), "
                         "folded = eval() folded into the weights at load (SURVEY.md N4)")
    args = ap.parse_args()
    if args.libtorch_leg:
        return libtorch_leg(args)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    rank = int(os.environ.get("RANK", 0)); local_rank = int(os.environ.get("LOCAL_RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    N = max(world, 1)
    use_comm = N > 1 or args.force_comm
    saved_stdout = None
    if use_comm:
        # RCCL prints a version banner on stdout when the communicator is created: keep stdout clean for the single JSON
        # line by pointing fd 1 at stderr until the result is printed
        sys.stdout.flush()
        saved_stdout = os.dup(1)
        os.dup2(2, 1)

    from xfeatslam_amd import capi, dist as xd, synth, weights as WT
    from xfeatslam_amd.extractor import Context
    lib = capi.lib()
    if lib.xfh_device_count() <= 0:
        raise SystemExit("bench.py needs an MI355X: libxfeat_hip.so has no CPU fallback")

    B, H, W, K = args.batch, args.height, args.width, args.steps
    dev = (local_rank % max(1, lib.xfh_device_count())) if N > 1 else 0      # (fewer GPUs than ranks only happens under the test stand-in for librccl)
    bn_mode = BN_MODES[args.bn]
    blob = WT.pack_blob(WT.make_synthetic(1234, KP_GAIN, with_bn=True))       # the running statistics are ignored in batch mode
    S = max(1, args.streams)
    ctxs = [Context(nfeatures=NFEATURES, max_height=H, max_width=W, max_batch=B, device=dev, bn_mode=bn_mode,
                    flags=capi.FLAG_SERIAL_BRANCH if args.serial_branch else 0) for _ in range(S)]
    for c_ in ctxs:
        c_.load_weights(blob)
    ctx = ctxs[0]
    # frame i of the global batch goes to rank i mod N (weak scaling: S*B frames per GPU per step); every frame is distinct
    frames = synth.frames(B * S, H, W, seed=42 + 1000 * rank)        # every frame of the step is distinct, also across sub-batches
    rec_bytes = ctx.rec_bytes
    nf = NFEATURES

    comm = None
    if use_comm:
        comm = xd.Comm(ctx, rank, N, os.environ.get("MASTER_ADDR", "127.0.0.1"), int(os.environ.get("MASTER_PORT", "29500")) + 17)
    d_in = capi.DeviceBuffer(frames.nbytes).upload(frames)
    d_rec = [capi.DeviceBuffer(S * B * rec_bytes) for _ in range(2 if use_comm else 1)]     # two generations under the exchange
    d_all_of = {}

    def gather_target(form, frames_per_rank):
        """two generations of the buffer the gather form `form` fills with `frames_per_rank` records per rank"""
        key = (form, frames_per_rank)
        if key not in d_all_of:
            if form == "allgather":
                nb = N * frames_per_rank * rec_bytes
            elif form == "root":
                nb = N * frames_per_rank * rec_bytes if rank == 0 else 16
            else:
                nb = N * int(lib.xfh_compact_bytes_max(nf, frames_per_rank)) if rank == 0 else 16
            d_all_of[key] = [capi.DeviceBuffer(nb) for _ in range(2)]
        return d_all_of[key]

    def gather(form, d_records, frames_per_rank, g):
        tgt = gather_target(form, frames_per_rank)[g].ptr
        if form == "allgather":
            comm.allgather_records(d_records, frames_per_rank, tgt, g)
        elif form == "root":
            comm.gather_records_root(d_records, frames_per_rank, tgt, 0, g)
        else:
            comm.gather_compact_root(d_records, frames_per_rank, tgt, 0, g)

    in_ptr, rec_ptr = d_in.ptr, d_rec[0].ptr
    step_no = [0]

    def step(form=None):
        form = form or args.gather
        # S sub-batches of B frames, each on its own ctx / stream; the exchange of generation g runs on the ctx's
        # communication stream while the next step extracts into the other generation
        g = step_no[0] & 1 if use_comm else 0
        exchange = use_comm and form != "none"             # "none": the extraction alone on every rank (multi-rank leg `extract_only`)
        if exchange:
            comm.fence(g)                                  # the collective that last read generation g has finished
            for c_ in ctxs[1:]:
                comm.fence_ctx(c_, g)
        for k, c_ in enumerate(ctxs):
            capi.check(lib.xfh_extract_batch_device(c_.h, in_ptr + k * B * H * W, B, H, W, 0, 0, d_rec[g].ptr + k * B * rec_bytes), c_.h)
        if exchange:
            for c_ in ctxs[1:]:
                comm.wait_ctx(c_)                          # the collective waits for every sub-batch, not only ctx 0's
            gather(form, d_rec[g].ptr, S * B, g)
        step_no[0] += 1

    def sync(value=0.0):
        """device idle on every rank, then a barrier (RCCL all-gather of one double); returns the max of `value`"""
        for c_ in ctxs:
            c_.synchronize()
        if use_comm:
            comm.synchronize()
            return comm.barrier_max(value)
        return value

    if use_comm:
        gather_target(args.gather, S * B)                  # allocated before the clock
    for _ in range(args.warmup):
        step()
    sync()
    # roofline of the dominant kernel: dispatch-attached HIP events (hipExtLaunchKernelGGL) on every launch of that kernel
    # INSIDE the timed region, on the streams the kernel runs on, in every ctx; rocprofv3 --kernel-trace of the same command
    # reports the same average.  With several sub-batches in flight a launch shares the CUs with the other ctx' kernels, so
    # its duration is longer than the kernel's own speed: that one is measured after the region (`isolated`, one ctx alone).
    layer_mask = sum(1 << l for l in DOMINANT_LAYERS)
    in_region = args.full and K * len(DOMINANT_LAYERS) <= 4096
    if in_region:
        for c_ in ctxs:
            c_.timing_enable(capi.K["CONV_MFMA"], layer_mask)
    sync()
    t0 = time.perf_counter()
    for _ in range(K):
        step()
    for c_ in ctxs:
        c_.synchronize()
    if use_comm:
        comm.synchronize()
    elapsed = sync(time.perf_counter() - t0)               # barrier; MAX over ranks
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, ctx, d_rec[(step_no[0] - 1) & 1 if use_comm else 0], S * B)
    n_conv, ms_conv = 0, 0.0
    if in_region:
        for c_ in ctxs:
            n_, ms_ = c_.timing_read()
            n_conv += n_; ms_conv += ms_
            c_.timing_enable(0)
    n_iso, ms_iso = 0, 0.0
    if args.full:
        ctx.timing_enable(capi.K["CONV_MFMA"], layer_mask)
        for _ in range(min(K, 40)):
            capi.check(lib.xfh_extract_batch_device(ctx.h, in_ptr, B, H, W, 0, 0, rec_ptr), ctx.h)
        ctx.synchronize()
        n_iso, ms_iso = ctx.timing_read()
        ctx.timing_enable(0)
    frames_per_s = N * B * S * K / elapsed

    def timed(fn, k, warm=2):
        """k calls of fn between two barriers; MAX over ranks of the elapsed time per call [s]"""
        for _ in range(warm):
            fn()
        sync()
        t_ = time.perf_counter()
        for _ in range(k):
            fn()
        for c_ in ctxs:
            c_.synchronize()
        if use_comm:
            comm.synchronize()
        return sync(time.perf_counter() - t_) / k

    multi = None
    if use_comm and args.full and not args.no_legs:
        multi = multi_rank_legs(args, lib, capi, synth, Context, xd, comm, ctx, blob, rank, N, dev, nf, rec_bytes, step, timed, gather, gather_target, B * S, step_no)

    if rank != 0:
        sync()                                             # rank 0 runs its extra legs, then everybody leaves together
        comm.close()
        return

    conv_us = ms_conv / max(n_conv, 1) * 1e3
    conv_tf = conv_flops(H, W) * B / (conv_us * 1e-6) / 1e12 if n_conv else 0.0
    iso_us = ms_iso / max(n_iso, 1) * 1e3
    iso_tf = conv_flops(H, W) * B / (iso_us * 1e-6) / 1e12 if n_iso else 0.0
    out = {
        "metric": "XFeat frames/s (VGA, 4096 kpts) + 4096x4096 desc-match pairs/s",
        "value": frames_per_s, "unit": "frames/s", "n_gpus": N, "steps": K, "warmup": args.warmup,
        "ms_per_step": elapsed / K * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"configs[1], HBM-resident (host-visible: {'config.host_visible_frames_per_s' if args.full else 'bench.py --full'}): {H}x{W} u8 frames, XFeat extract, nfeatures {nf}, {B * S} distinct frames per GPU per step "
                               f"({S} sub-batch(es) of {B}, each on its own ctx / HIP streams) ({BN_TEXT[args.bn]}), inputs and 4096-row records resident in HBM"
                               + (f", RCCL {GATHER_TEXT[args.gather]} through the C ABI (xfh_comm_*), overlapped with the next step" if use_comm else ""),
                   "frames_per_gpu_per_step": B * S, "sub_batches_in_flight": S, "height": H, "width": W, "nfeatures": nf,
                   "weights": f"synthetic seed 1234, keypoint-logit gain {KP_GAIN}", "parallelism": f"frames x{N}"},
    }
    traffic = None
    tpath = os.path.join(ROOT, "profiles", "pmc_traffic.json")     # written by tools/summarize_profiles.py from --pmc passes
    if os.path.exists(tpath):
        try:
            traffic = json.load(open(tpath))
        except Exception:
            traffic = None
    conv_traffic = None
    if traffic and traffic.get("conv_bytes_per_launch"):
        conv_traffic = traffic["conv_bytes_per_launch"] * (B / traffic["conv_batch"] if traffic.get("conv_batch") else 1.0)
    out["config"]["bn_mode"] = args.bn
    out["config"]["library"] = lib.xfh_version().decode()
    # which librccl moves the records (comm.cpp: $XFH_RCCL_LIB, else /opt/rocm/lib/librccl.so.1, ...; file of ncclAllGather, ncclGetVersion, HIP runtime on both sides) and in which form
    out["config"]["rccl"] = lib.xfh_comm_library().decode() if use_comm else "not loaded (one rank, no exchange)"
    out["config"]["gather_form"] = args.gather if use_comm else "none (one rank)"
    pmc_src = "profiles/pmc_traffic.json: the builder's separate rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE passes (tools/gpu_round.sh), corrected with the factors calibrated on known-byte-count kernels (xfh_bench_calib); a constant in this run, not an observation of it"
    step_tf = net_flops(H, W) * frames_per_s / N / 1e12
    out["step_roofline"] = {"what": "all convolutions of the network (algorithmic flops per frame) x frames/s per GPU of the timed region, against the f32 MFMA peak: "
                                    "the whole step, every non-convolution kernel and every gap included",
                            "flops_per_frame": net_flops(H, W), "achieved": step_tf, "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": step_tf / PEAK_F32_MFMA_TFLOPS}
    # the other roofline of SURVEY.md 8d, for completeness: bytes against the 8 TB/s of HBM.  Compulsory traffic (frame in, record out)
    # is 1.47 MB per frame; the PMC counters (profiles/pmc_traffic.json, separate --pmc passes) see every inter-layer map as well.
    comp = H * W + 4096 * (28 + 256)
    meas = traffic.get("extract_hbm_bytes_per_frame") if traffic else None
    out["step_roofline"]["hbm"] = {"peak_GBps": 8000.0, "compulsory_bytes_per_frame": comp, "compulsory_frac": comp * frames_per_s / N / 8e12,
                                   "measured_bytes_per_frame": meas, "measured_source": pmc_src if meas else None,
                                   "measured_GBps": (meas * frames_per_s / N / 1e9) if meas else None,
                                   "measured_frac": (meas * frames_per_s / N / 8e12) if meas else None,
                                   "note": "the step is bound by the vector / matrix pipe (frac above), not by HBM"}
    if args.full:
        kname = ("k_conv_mfma<64,64,3,...>" if B > 32 else "k_conv_mfma16<64,64,1,16,2,...> (16x16x4 tiles, the form for batches <= 32)") + " (block3.1, block_fusion.1: 3x3 64->64 at 1/8 res)" + ("" if args.bn != "folded" else ", bias+ReLU epilogue")
        out["roofline"] = {"kernel": kname,
                           "measured": f"HIP events attached to every dispatch of the kernel (hipExtLaunchKernelGGL): the same launches ({B} frames each) with ONE ctx alone on the GPU "
                                       "right after the timed region -- the kernel's own duration, the view rocprofv3 --kernel-trace gives of a serial run (profiles/r06_roofline_table_B64.md: "
                                       "`bench.py --full --streams 1 --batch 64 --serial-branch --only-match-leg` under rocprofv3, 191 us per launch on the box whose events read 192)",
                           "bound": "mfma", "achieved": iso_tf, "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": iso_tf / PEAK_F32_MFMA_TFLOPS,
                           "traffic": conv_traffic, "traffic_source": pmc_src if conv_traffic else None,
                           "mfma_busy": pmc_busy("k_conv_mfma<64, 64, 3, 1, 4, 2, 1, 16, 1, 0") if B > 32 else None, "mfma_busy_source": PMC_BUSY_SRC,
                           "avg_launch_us": iso_us, "launches": n_iso, "flops_per_launch": conv_flops(H, W) * B,
                           "in_timed_region": {"note": "the same events inside the timed region, all ctx" + (f": {S} sub-batches are in flight, a launch shares the CUs with the other ctx' kernels, so this "
                                                       "span is longer than the kernel's own speed (it measures neither the kernel nor the step)" if S > 1 else ""),
                                               "achieved": conv_tf, "frac": conv_tf / PEAK_F32_MFMA_TFLOPS, "avg_launch_us": conv_us, "launches": n_conv}}
    if multi is not None:
        out.update(multi)

    if args.full and not args.no_legs:
        legs(out, args, lib, capi, synth, Context, ctx, blob, frames, d_in, d_rec[0], B, H, W, nf, rec_bytes, traffic, N)

    flat_scalars(out, N)
    if use_comm:
        sync()
        comm.close()
    sys.stdout.flush()
    if saved_stdout is not None:
        C.CDLL(None).fflush(None)                          # RCCL's banner sits in the C stdio buffer of fd 1: out to stderr with it
        os.dup2(saved_stdout, 1)
    print(json.dumps(out), flush=True)


def flat_scalars(out, N):
    """The figures a reader of the driver's record needs, as flat scalars inside `config` and `roofline` (the driver's parser keeps scalars of those two
    objects and drops nested ones: BENCH_r04.json lost `host_visible`, `match` and `step_roofline`).  `value` stays the HBM-resident regime -- the bench
    contract: "inputs already resident in HBM when the timed region starts ... the PCIe-inclusive rate is never `value`" -- and SURVEY.md 8d's host-visible
    reading of the same metric sits next to it."""
    c, r = out["config"], out.get("roofline", {})                                      # `roofline`: --full only
    c["hbm_resident_fps_per_gpu"] = out["value"] / N
    if "host_visible" in out:
        hv = out["host_visible"]
        c["host_visible_frames_per_s"] = hv["value"]                                   # SURVEY.md 8d read literally: host memory -> host memory, PCIe inside the clock (rank 0's GPU)
        c["host_visible_blocking_fps"] = hv["blocking"]["value"]
        c["host_visible_vs_hbm_resident"] = hv["vs_hbm_resident"]
        if "one_frame_per_call" in hv:
            c["host_one_frame_per_call_fps"] = hv["one_frame_per_call"]["value"]
    if "single_frame" in out:
        c["single_frame_ms"] = out["single_frame"]["ms_per_frame"]
    if "step_roofline" in out:
        c["step_mfma_frac"] = out["step_roofline"]["frac"]
        r["step_frac"] = out["step_roofline"]["frac"]
    m = out.get("match")
    if m:
        flop = 2.0 * m["n1"] * m["n2"] * 64
        c["match_us_per_call"] = m["us_per_call"]
        c["match_pairs_per_s"] = m["pairs_per_s"]
        c["match_call_frac"] = flop / (m["us_per_call"] * 1e-6) / 1e12 / PEAK_F32_MFMA_TFLOPS
        c["match_gemm_us"] = m["roofline"]["avg_launch_us"]
        c["match_gemm_frac"] = m["roofline"]["frac"]
        r["match_gemm_frac"] = m["roofline"]["frac"]
        r["match_call_frac"] = c["match_call_frac"]
        if "batched" in m:
            c["match_batched_us_per_pair"] = m["batched"]["us_per_pair"]
            c["match_batched_pairs_per_s"] = m["batched"]["pairs_per_s"]
            c["match_batched_call_frac"] = flop / (m["batched"]["us_per_pair"] * 1e-6) / 1e12 / PEAK_F32_MFMA_TFLOPS
            c["match_batched_gemm_frac"] = m["batched"]["roofline"]["frac"]
        if "paced_30hz" in m:
            c["match_paced_30hz_us"] = m["paced_30hz"]["us_per_call_median"]
    ak = out.get("aux_kernels") or {}
    for k, v in ak.items():
        if k.startswith("k_dist_i32"):
            c["dist_i32_kernel_us"] = v["kernel_us"]
            if "frac_of_f32_mfma_peak" in v:
                c["dist_i32_mfma_frac"] = v["frac_of_f32_mfma_peak"]
    par = out.get("parity")
    if par:
        c["parity_keypoint_sets_equal"] = bool(par["keypoint_sets_equal"])
        c["parity_max_abs_desc_diff"] = par["max_abs_desc_diff"]
        c["parity_match_pairs_equal"] = bool(par["match_pairs_equal"])
    if isinstance(out.get("extract_only"), dict):                                      # multi-rank legs (N > 1): scaling with and without the exchange, side by side
        c["extract_only_frames_per_s"] = out["extract_only"]["frames_per_s"]
        c["gather_cost_frac"] = 1.0 - out["value"] / out["extract_only"]["frames_per_s"]
    for form, v in (out.get("gather_forms") or {}).items():
        if isinstance(v, dict) and "frames_per_s" in v:
            c[f"gather_{form}_frames_per_s"] = v["frames_per_s"]
    if isinstance(out.get("exchange_check"), dict):
        c["exchange_equal_serial_ctx"] = bool(out["exchange_check"]["equal_to_serial_ctx"])
        c["exchange_records_checked"] = out["exchange_check"]["records_checked"]
    c3 = out.get("configs3")
    if isinstance(c3, dict):
        for form, v in c3.get("per_gather_form", {}).items():
            c[f"configs3_{form}_frames_per_s"] = v["frames_per_s"]
            c[f"configs3_{form}_latency_ms"] = v["one_step_latency_ms"]
    c31 = out.get("configs3_one_gpu")
    if isinstance(c31, dict):
        c["configs3_one_gpu_frames_per_s"] = c31["device_resident"]["frames_per_s"]
    # Order and names for the driver's record: its parser keeps the first ~20 scalars of `config`, names cut at 40 characters (BENCH_r05.json lost the parity
    # flags and the paced match figure that way): what identifies the run and what a reader must see first, every name <= 32 characters.
    first = ["workload", "parallelism", "rccl", "gather_form", "extract_only_frames_per_s", "gather_cost_frac", "exchange_equal_serial_ctx",
             "parity_keypoint_sets_equal", "parity_match_pairs_equal", "parity_max_abs_desc_diff", "step_mfma_frac", "host_visible_frames_per_s", "single_frame_ms",
             "match_us_per_call", "match_call_frac", "match_gemm_frac", "match_paced_30hz_us", "match_batched_us_per_pair", "dist_i32_kernel_us",
             "frames_per_gpu_per_step", "sub_batches_in_flight", "bn_mode", "library"]
    out["config"] = {**{k: c[k] for k in first if k in c}, **{k: v for k, v in c.items() if k not in first}}
    assert all(len(k) <= 32 for k in out["config"]), [k for k in out["config"] if len(k) > 32]


DUMP_FRAMES = 32      # frames of the last timed step whose keypoints and descriptors --dump-outputs writes (37 MB at 4096 rows)


def dump_outputs(path, ctx, d_records, n_frames):
    """--dump-outputs DIR: what a caller of the timed path receives from its last step, the 4096-row records of the step's frames, as
    .npy files: header.npy float64 [n_frames, 3] (n_valid, mono_index, n_candidates of every frame); for a fixed, seeded sample of
    DUMP_FRAMES frames (frame_index.npy, float64) keypoints.npy float32 [n, rows, 7] (x, y, size, angle, response, octave, class_id)
    and descriptors.npy float32 [n, rows, 64].  The rows past n_valid are the record's padding, written by the kernels too."""
    os.makedirs(path, exist_ok=True)
    rb = ctx.rec_bytes
    head = np.stack([d_records.download(np.int32, 3, i * rb) for i in range(n_frames)]).astype(np.float64)
    pick = np.sort(np.random.default_rng(0).choice(n_frames, min(n_frames, DUMP_FRAMES), replace=False))
    recs = [ctx.parse_records(d_records.download(np.uint8, rb, int(i) * rb), 1)[0] for i in pick]
    kps = np.stack([np.stack([k[f].astype(np.float32) for f in k.dtype.names], -1) for k, *_ in recs])
    np.save(os.path.join(path, "header.npy"), head)
    np.save(os.path.join(path, "frame_index.npy"), pick.astype(np.float64))
    np.save(os.path.join(path, "keypoints.npy"), kps)
    np.save(os.path.join(path, "descriptors.npy"), np.stack([d for _, d, *_ in recs]).astype(np.float32))


PCIE_GBPS = 63.0      # PCIe 5.0 x16, one direction, after 128b/130b (tools/pcie_probe.py on the bench box: 56.5 GB/s for one copy stream)
C3_H, C3_W = 720, 1280



def multi_rank_legs(args, lib, capi, synth, Context, xd, comm, ctx, blob, rank, N, dev, nf, rec_bytes, step, timed, gather, gather_target, frames_per_rank, step_no):
    """collective legs, run by EVERY rank after the timed region: the headline workload under the other two gather forms, and
    BASELINE.json configs[3] itself -- one 1280x720 frame per rank per step (frame i of the batch of N -> rank i), extracted on the
    rank's GPU and gathered to rank 0, all three gather forms; reference consumer: the sequential loop of src/System.cc:197-233"""
    res = {}
    forms = ["allgather", "root", "compact"]
    k2 = max(3, min(10, args.steps))
    gf = {}
    for form in forms:
        if form == args.gather:
            continue
        gather_target(form, frames_per_rank)
        dt = timed(lambda: step(form), k2)
        gf[form] = {"frames_per_s": N * frames_per_rank / dt, "ms_per_step": dt * 1e3, "steps": k2}
    gf["note"] = f"the timed region's workload ({frames_per_rank} VGA frames per GPU per step) with the other gather forms; `value` uses --gather {args.gather}"
    res["gather_forms"] = gf
    # the same workload with NO exchange at all (every rank extracts, nobody gathers; barriers around the clock as everywhere): separates how the
    # extraction scales with N (one process per GPU: it should not change) from what the gather of N x frames_per_rank records costs
    comm.synchronize()
    dt = timed(lambda: step("none"), k2)
    comm.fence(0); comm.fence(1)
    res["extract_only"] = {"frames_per_s": N * frames_per_rank / dt, "ms_per_step": dt * 1e3, "steps": k2,
                           "note": "no gather: extraction on every rank, MAX over ranks of the step time; value / this = what the exchange costs at this N"}
    # ---- what rank 0 holds after the default exchange IS what a serial ctx produces for those frames: one step with xfh_allgather_records, then rank 0
    # regenerates the first frames of EVERY rank's shard (the frames are a function of (seed, rank)), extracts them alone on its own ctx and compares the
    # records field by field (header, keypoints, descriptors; statistics are per frame, so the batch a frame sat in does not matter)
    gather_target("allgather", frames_per_rank)
    timed(lambda: step("allgather"), 1, warm=0)             # one step between two barriers, every ctx and the communicator idle afterwards
    if rank == 0:
        nchk = min(2, frames_per_rank)
        tgt = gather_target("allgather", frames_per_rank)[(step_no[0] - 1) & 1]       # the generation the last step gathered into
        equal, checked = True, 0
        for r in range(N):
            fr = synth.frames(nchk, args.height, args.width, seed=42 + 1000 * r)
            d_f = capi.DeviceBuffer(fr.nbytes).upload(fr); d_r = capi.DeviceBuffer(nchk * rec_bytes)
            capi.check(lib.xfh_extract_batch_device(ctx.h, d_f.ptr, nchk, args.height, args.width, 0, 0, d_r.ptr), ctx.h)
            ctx.synchronize()
            want = ctx.parse_records(d_r.download(np.uint8, nchk * rec_bytes), nchk)
            got = ctx.parse_records(tgt.download(np.uint8, nchk * rec_bytes, r * frames_per_rank * rec_bytes), nchk)
            for a, b in zip(got, want):
                equal = equal and a[2:] == b[2:] and bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))
                checked += 1
            d_f.free(); d_r.free()
        res["exchange_check"] = {"records_checked": checked, "ranks": N, "equal_to_serial_ctx": bool(equal),
                                 "what": f"after one xfh_allgather_records step: the first {nchk} records of every rank's shard as they sit in rank 0's gathered buffer, against "
                                         "the same frames extracted alone on rank 0's ctx (header, keypoints, descriptors bit for bit)"}
    comm.barrier_max(0.0)
    # ---- configs[3] ---------------------------------------------------------------------------------------------------
    ctx3 = Context(nfeatures=nf, max_height=C3_H, max_width=C3_W, max_batch=1, device=dev)
    ctx3.load_weights(blob)
    fr3 = synth.frames(1, C3_H, C3_W, seed=4242 + rank)
    d_in3 = capi.DeviceBuffer(fr3.nbytes).upload(fr3)
    d_rec3 = [capi.DeviceBuffer(rec_bytes) for _ in range(2)]
    no = [0]

    def step3(form):
        g = no[0] & 1
        no[0] += 1
        comm.fence_ctx(ctx3, g)                            # the gather that last read generation g has finished
        capi.check(lib.xfh_extract_batch_device(ctx3.h, d_in3.ptr, 1, C3_H, C3_W, 0, 0, d_rec3[g].ptr), ctx3.h)
        comm.wait_ctx(ctx3)
        gather(form, d_rec3[g].ptr, 1, g)
    c3 = {}
    k3 = max(5, min(30, args.steps))
    for form in forms:
        gather_target(form, 1)
        dt = timed(lambda: step3(form), k3)
        # latency of ONE step: frame in HBM -> all records at rank 0, nothing else in flight
        lat = 0.0
        for _ in range(3):
            ctx3.synchronize(); comm.synchronize()
            comm.barrier_max(0.0)
            t_ = time.perf_counter()
            step3(form)
            ctx3.synchronize(); comm.synchronize()
            lat = max(lat, time.perf_counter() - t_) if _ == 0 else min(lat, time.perf_counter() - t_)
        lat = comm.barrier_max(lat)
        c3[form] = {"frames_per_s": N / dt, "ms_per_step": dt * 1e3, "steps": k3, "one_step_latency_ms": lat * 1e3}
    res["configs3"] = {"workload": f"configs[3]: a batch of {N} 1280x720 frames sharded one per GPU (frame i -> rank i), extracted at 704x1280 into 4096-row records on each GPU, "
                                   f"records gathered to rank 0 with RCCL through the C ABI (xfh_comm_*); steps back to back, the gather of step t overlaps the extraction of step t + 1",
                       "n_ranks": N, "per_gather_form": c3,
                       "note": "frames_per_s = N / step time (MAX over ranks); one_step_latency_ms = one isolated step, frame resident in HBM -> gather complete"}
    ctx3.synchronize(); comm.synchronize()
    ctx3.close()
    return res


def libtorch_leg(args):
    """child process of the cpu_baseline leg: oracle/torch_restatement.py -- the reference's own libtorch CPU operators, statement by
    statement (conv2d, batch_norm(training), instance_norm, interpolate, softmax, max_pool2d, nonzero, grid_sample, argsort, normalize;
    the reference itself cannot be built here: OpenCV) -- on the same synthetic frames / weights, for each thread count in the argument"""
    import torch
    from oracle import torch_restatement as TR
    from xfeatslam_amd import synth, weights as WT
    wt = WT.make_synthetic(1234, KP_GAIN)
    frames = synth.frames(4, args.height, args.width, seed=42)
    d1, d2 = synth.descriptor_sets(NFEATURES, NFEATURES, noise=0.1)
    res = {}
    for nthr in [int(v) for v in args.libtorch_leg.split(",")]:
        torch.set_num_threads(nthr)
        t0 = time.perf_counter()
        TR.extract(frames[0], wt, NFEATURES, (0, 0))
        warm = time.perf_counter() - t0
        nfr = max(1, min(8, int(5.0 / max(warm, 1e-3))))
        t0 = time.perf_counter()
        for i in range(nfr):
            TR.extract(frames[i % len(frames)], wt, NFEATURES, (0, 0))
        fdt = (time.perf_counter() - t0) / nfr
        t0 = time.perf_counter()
        TR.match_mnn(d1, d2)
        mdt = time.perf_counter() - t0
        res[str(nthr)] = {"frames_per_s": 1.0 / fdt, "frames": nfr, "match_pairs_per_s": NFEATURES * NFEATURES / mdt}
    print(json.dumps({"torch": torch.__version__, "legs": res}), flush=True)


def legs(out, args, lib, capi, synth, Context, ctx, blob, frames, d_in, d_recb, B, H, W, nf, rec_bytes, traffic, N):
    in_ptr, rec_ptr = d_in.ptr, d_recb.ptr
    # records of frames 0 and 1 on the ctx's own stream (the timed region may have left another generation here)
    capi.check(lib.xfh_extract_batch_device(ctx.h, in_ptr, B, H, W, 0, 0, rec_ptr), ctx.h)
    ctx.synchronize()

    # ---- configs[1] read literally: ONE frame per call (what a SLAM thread sees), device resident, back to back -------
    for _ in range(10):
        capi.check(lib.xfh_extract_batch_device(ctx.h, in_ptr, 1, H, W, 0, 0, rec_ptr), ctx.h)
    ctx.synchronize()
    t1 = time.perf_counter()
    n_single = 300 if not args.only_match_leg else 3
    for _ in range(n_single):
        capi.check(lib.xfh_extract_batch_device(ctx.h, in_ptr, 1, H, W, 0, 0, rec_ptr), ctx.h)
    ctx.synchronize()
    single_dt = (time.perf_counter() - t1) / n_single
    out["single_frame"] = {"ms_per_frame": single_dt * 1e3, "frames_per_s": 1.0 / single_dt,
                           "note": "one 480x640 frame per xfh_extract_batch_device call, back to back on one stream (latency path of configs[1], device resident)"}
    capi.check(lib.xfh_extract_batch_device(ctx.h, in_ptr, B, H, W, 0, 0, rec_ptr), ctx.h)   # restore the batch records
    ctx.synchronize()

    # ---- SURVEY.md 8d read literally: host-visible.  The step's frames from pinned host memory to records in pinned host memory
    # through the batch pipeline (csrc/pipeline.cpp: sub-batches of B frames drained by host-driven lanes), PCIe inside the clock
    if not args.only_match_leg:
        S = max(1, args.streams)
        nfr = S * B
        hin = capi.HostBuffer(nfr * H * W); hin.array[:] = frames.reshape(-1)[:nfr * H * W]
        houts = [capi.HostBuffer(nfr * rec_bytes) for _ in range(3)]
        hk = max(3, args.host_steps)
        for _ in range(3):
            capi.check(lib.xfh_extract_batch(ctx.h, hin.ptr, nfr, H, W, 0, 0, houts[0].ptr), ctx.h)
        t1 = time.perf_counter()
        for _ in range(hk):
            capi.check(lib.xfh_extract_batch(ctx.h, hin.ptr, nfr, H, W, 0, 0, houts[0].ptr), ctx.h)
        blocking_dt = (time.perf_counter() - t1) / hk
        t1 = time.perf_counter()
        # a streaming consumer: three record buffers in rotation, two steps submitted ahead of the one it waits for (submit(t + 2); wait() -> step t is
        # complete in houts[t % 3]), so that every lane always has its next sub-batch queued behind the one whose records are on their way out
        capi.check(lib.xfh_extract_batch_submit(ctx.h, hin.ptr, nfr, H, W, 0, 0, houts[0].ptr), ctx.h)
        if hk > 1:
            capi.check(lib.xfh_extract_batch_submit(ctx.h, hin.ptr, nfr, H, W, 0, 0, houts[1].ptr), ctx.h)
        for t in range(2, hk):
            capi.check(lib.xfh_extract_batch_submit(ctx.h, hin.ptr, nfr, H, W, 0, 0, houts[t % 3].ptr), ctx.h)
            capi.check(lib.xfh_extract_batch_wait(ctx.h), ctx.h)           # step t - 2 is complete in houts[(t - 2) % 3]: the consumer's turn
        for _ in range(min(hk, 2)):
            capi.check(lib.xfh_extract_batch_wait(ctx.h), ctx.h)
        piped_dt = (time.perf_counter() - t1) / hk
        got = ctx.parse_records(np.array(houts[(hk - 1) % 3].array[:2 * rec_bytes]), 2)
        dev_recs = ctx.parse_records(d_recb.download(np.uint8, rec_bytes * 2), 2) if B > 1 else None
        same = None if dev_recs is None else bool(all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:4] == b[2:4] for a, b in zip(got, dev_recs)))
        out_b, in_b = nfr * rec_bytes, nfr * H * W
        out["host_visible"] = {
            "value": nfr / piped_dt, "unit": "frames/s",
            "workload": f"SURVEY.md 8d metric read literally (host-visible): {nfr} distinct {H}x{W} u8 frames per step from pinned HOST memory -> {nfr} padded {nf}-row records "
                        f"(keypoints + descriptors, {rec_bytes} B each) in pinned HOST memory through xfh_extract_batch_submit / _wait: sub-batches of {B} frames drained by 6 host-driven "
                        "lanes (a worker thread per lane: copy in, kernels, copy out), the consumer rotates three record buffers (submit(t + 2); wait() -> step t); PCIe both ways inside the clock, pipeline fill and drain included",
            "ms_per_step": piped_dt * 1e3, "steps": hk, "frames_per_step": nfr,
            "blocking": {"value": nfr / blocking_dt, "ms_per_step": blocking_dt * 1e3, "note": "xfh_extract_batch per step (submit + drain): the last sub-batches' downloads are exposed"},
            "pcie": {"bytes_out_per_frame": rec_bytes, "bytes_in_per_frame": H * W, "out_GBps": out_b / piped_dt / 1e9, "in_GBps": in_b / piped_dt / 1e9,
                     "peak_GBps_per_direction": PCIE_GBPS, "out_frac_of_peak": out_b / piped_dt / 1e9 / PCIE_GBPS, "in_frac_of_peak": in_b / piped_dt / 1e9 / PCIE_GBPS},
            "vs_hbm_resident": (nfr / piped_dt) / (out["value"] / N),
            "records_equal_device_resident_path": same,
            "n_gpus": 1, "note": "one GPU (rank 0's); `value` of the line is the HBM-resident regime the bench contract prescribes"}
        for h in houts + [hin]:
            h.free()
        # ---- BASELINE.json configs[3] on ONE GPU: the batch of 8 1280x720 frames (the multi-rank form is `configs3` of a --gpus N run)
        c3 = Context(nfeatures=nf, max_height=C3_H, max_width=C3_W, max_batch=8, device=ctx.device)
        c3.load_weights(blob)
        fr3 = synth.frames(8, C3_H, C3_W, seed=4242)
        d_in3 = capi.DeviceBuffer(fr3.nbytes).upload(fr3); d_rec3 = capi.DeviceBuffer(8 * rec_bytes)
        for _ in range(3):
            capi.check(lib.xfh_extract_batch_device(c3.h, d_in3.ptr, 8, C3_H, C3_W, 0, 0, d_rec3.ptr), c3.h)
        c3.synchronize()
        t1 = time.perf_counter()
        for _ in range(20):
            capi.check(lib.xfh_extract_batch_device(c3.h, d_in3.ptr, 8, C3_H, C3_W, 0, 0, d_rec3.ptr), c3.h)
        c3.synchronize()
        dt3 = (time.perf_counter() - t1) / 20
        h3 = capi.HostBuffer(fr3.nbytes); h3.array[:] = fr3.reshape(-1); o3 = capi.HostBuffer(8 * rec_bytes)
        for _ in range(2):
            capi.check(lib.xfh_extract_batch(c3.h, h3.ptr, 8, C3_H, C3_W, 0, 0, o3.ptr), c3.h)
        t1 = time.perf_counter()
        for _ in range(20):
            capi.check(lib.xfh_extract_batch(c3.h, h3.ptr, 8, C3_H, C3_W, 0, 0, o3.ptr), c3.h)
        dt3h = (time.perf_counter() - t1) / 20
        out["configs3_one_gpu"] = {"workload": "configs[3] on one GPU: the batch of 8 1280x720 frames in one call (extracted at 704x1280, 4096-row records)",
                                   "device_resident": {"frames_per_s": 8 / dt3, "ms_per_batch": dt3 * 1e3},
                                   "host_visible_blocking": {"frames_per_s": 8 / dt3h, "ms_per_batch": dt3h * 1e3},
                                   "note": "the sharded form (one frame per GPU + RCCL gather) is the `configs3` key of a --gpus N run"}
        h3.free(); o3.free(); d_in3.free(); d_rec3.free(); c3.close()

    # ---- the same workload with upstream-XFeat eval() BatchNorm, exact (running) and folded into the weights
    if args.bn == "batch" and not args.no_bn_leg and not args.only_match_leg:
        bn = {}
        S = max(1, args.streams)
        for name in ("running", "folded"):
            fcs = [Context(nfeatures=nf, max_height=H, max_width=W, max_batch=B, device=ctx.device, bn_mode=BN_MODES[name]) for _ in range(S)]
            for fc in fcs:
                fc.load_weights(blob)
            d_r = capi.DeviceBuffer(S * B * rec_bytes)
            def bn_step():
                for k, fc in enumerate(fcs):
                    capi.check(lib.xfh_extract_batch_device(fc.h, in_ptr + k * B * H * W, B, H, W, 0, 0, d_r.ptr + k * B * rec_bytes), fc.h)
            for _ in range(2):
                bn_step()
            for fc in fcs:
                fc.synchronize()
            nrun = max(5, min(20, args.steps))
            t1 = time.perf_counter()
            for _ in range(nrun):
                bn_step()
            for fc in fcs:
                fc.synchronize()
            dt = (time.perf_counter() - t1) / nrun
            fc = fcs[0]
            fc.timing_enable(capi.K["CONV_MFMA"], sum(1 << l for l in DOMINANT_LAYERS))
            for _ in range(nrun):
                capi.check(lib.xfh_extract_batch_device(fc.h, in_ptr, B, H, W, 0, 0, d_r.ptr), fc.h)
            fc.synchronize()
            n_c, ms_c = fc.timing_read()
            fc.timing_enable(0)
            us = ms_c / max(n_c, 1) * 1e3
            tf = conv_flops(H, W) * B / (us * 1e-6) / 1e12 if n_c else 0.0
            bn[name] = {"frames_per_s": S * B / dt, "ms_per_step": dt * 1e3, "steps": nrun,
                        "roofline_isolated": {"kernel": "same 3x3 64->64 launches as the headline" + (", bias+ReLU epilogue, no statistics" if name == "folded" else ""),
                                              "bound": "mfma", "achieved": tf, "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": tf / PEAK_F32_MFMA_TFLOPS,
                                              "avg_launch_us": us, "launches": n_c}}
            # the latency path in this mode: one frame per call on a single-frame ctx, back to back, device resident (as `single_frame` of the default mode)
            f1 = Context(nfeatures=nf, max_height=H, max_width=W, max_batch=1, device=ctx.device, bn_mode=BN_MODES[name])
            f1.load_weights(blob)
            for _ in range(20):
                capi.check(lib.xfh_extract_batch_device(f1.h, in_ptr, 1, H, W, 0, 0, d_r.ptr), f1.h)
            f1.synchronize()
            n1 = 200
            t1 = time.perf_counter()
            for _ in range(n1):
                capi.check(lib.xfh_extract_batch_device(f1.h, in_ptr, 1, H, W, 0, 0, d_r.ptr), f1.h)
            f1.synchronize()
            bn[name]["single_frame"] = {"ms_per_frame": (time.perf_counter() - t1) / n1 * 1e3, "frames_per_s": n1 / (time.perf_counter() - t1)}
            f1.close()
            for fc in fcs:
                fc.close()
            d_r.free()
        bn["note"] = ("NOT the reference's semantics (its libtorch module stays in train mode, SURVEY.md Q1): upstream-XFeat eval() BatchNorm behind "
                      "cfg.bn_mode; 'folded' = W*rstd, bias -mean*rstd, ReLU in the conv epilogue, no statistics kernels or partials")
        out["bn_eval_modes"] = bn

    # ---- host API: the path the drop-in XFextractor::operator() takes (host image in, host keypoints / descriptors out)
    host = {}
    for nfh in ((4096, 1000) if not args.only_match_leg else ()):
        hc = Context(nfeatures=nfh, max_height=H, max_width=W, max_batch=1, device=ctx.device)
        hc.load_weights(blob)
        k = np.zeros(nfh, capi.KP_DTYPE); d = np.zeros((nfh, 64), np.float32); nv, mono = C.c_int(), C.c_int()
        fr = [np.ascontiguousarray(frames[i % len(frames)]) for i in range(8)]

        def blocking(i):
            capi.check(lib.xfh_extract(hc.h, fr[i % 8].ctypes.data, H, W, W, 0, 0, k.ctypes.data, d.ctypes.data, C.byref(nv), C.byref(mono)), hc.h)
        for i in range(10):
            blocking(i)
        t0 = time.perf_counter()
        n_it = 200
        for i in range(n_it):
            blocking(i)
        sync_dt = (time.perf_counter() - t0) / n_it
        nvalid = nv.value
        # pipelined: frame t+1 is submitted (H2D + kernels) before frame t is collected; XFH_MAX_INFLIGHT = 2
        capi.check(lib.xfh_extract_submit(hc.h, fr[0].ctypes.data, H, W, W, 0, 0), hc.h)
        t0 = time.perf_counter()
        for i in range(n_it):
            capi.check(lib.xfh_extract_submit(hc.h, fr[(i + 1) % 8].ctypes.data, H, W, W, 0, 0), hc.h)
            capi.check(lib.xfh_extract_collect(hc.h, k.ctypes.data, d.ctypes.data, C.byref(nv), C.byref(mono)), hc.h)
        pipe_dt = (time.perf_counter() - t0) / n_it
        capi.check(lib.xfh_extract_collect(hc.h, k.ctypes.data, d.ctypes.data, C.byref(nv), C.byref(mono)), hc.h)
        host[f"nfeatures_{nfh}"] = {"sync_ms_per_frame": sync_dt * 1e3, "sync_frames_per_s": 1.0 / sync_dt,
                                    "pipelined_ms_per_frame": pipe_dt * 1e3, "pipelined_frames_per_s": 1.0 / pipe_dt, "n_valid": nvalid}
        hc.close()
    host["note"] = ("xfh_extract / xfh_extract_submit+collect on one ctx: pageable host image -> pinned -> H2D -> kernels -> record written "
                    "to pinned host memory -> caller's buffers; everything inside the clock (SURVEY.md 8d 'host-visible')")
    out["host_api"] = host
    if "host_visible" in out:
        # the two regimes of the extraction metric side by side (SURVEY.md 8d defines it host-visible; the bench contract prescribes HBM-resident inputs for `value`)
        out["config"]["regimes_frames_per_s_one_gpu"] = {"hbm_resident (value / n_gpus)": out["value"] / N,
                                                        "host_visible (host memory -> host memory, PCIe both ways inside the clock; rank 0's GPU)": out["host_visible"]["value"]}
    if host.get("nfeatures_4096") and "host_visible" in out:
        out["host_visible"]["one_frame_per_call"] = {"value": host["nfeatures_4096"]["pipelined_frames_per_s"], "unit": "frames/s",
                                                     "note": "what a single SLAM thread sees: xfh_extract_submit / _collect, one frame per call, 2 frames in flight, pageable host memory in and out"}

    # ---- matching leg: 4096 x 4096 MNN on the descriptors of frame 0 vs frame 1 (device resident) ----------------------
    d1p = rec_ptr + ctx.desc_off
    d2p = rec_ptr + (rec_bytes if B > 1 else 0) + ctx.desc_off
    mout = capi.DeviceBuffer(12 * nf + 64)
    mo = (mout.ptr, mout.ptr + 4 * nf, mout.ptr + 8 * nf, mout.ptr + 12 * nf)

    def match():
        capi.check(lib.xfh_match_mnn_device(ctx.h, d1p, nf, d2p, nf, -1.0, *mo), ctx.h)
    # The GPU needs ~20 ms of continuous load to reach the clock it then holds (tools/gemm_b2b.py: the same 300 GEMM launches read 0.67, 0.70, 0.73,
    # 0.743, 0.743, ... of the peak in consecutive 6-ms windows after a pause), and every leg below starts after host-side work during which the
    # GPU was idle.  So each measured loop is preceded by WARM_MS of the SAME calls from a C loop (no foreign-function gaps), untimed.
    WARM_MS = max(args.match_warm_ms, 0.5)
    c_warm = C.c_double(0.0)

    def warm_raw():
        capi.check(lib.xfh_bench_match_raw(ctx.h, d1p, nf, d2p, nf, -1.0, *mo, int(WARM_MS * 1e3 / 32.0), C.byref(c_warm)), ctx.h)
    warm_raw()
    t0 = time.perf_counter()
    for _ in range(args.match_iters):
        match()
    ctx.synchronize()
    match_dt = (time.perf_counter() - t0) / args.match_iters
    warm_raw()
    c_raw = C.c_double(0.0)
    capi.check(lib.xfh_bench_match_raw(ctx.h, d1p, nf, d2p, nf, -1.0, *mo, max(args.match_iters, 50), C.byref(c_raw)), ctx.h)       # wall time per call, no events on the dispatches
    ctx.timing_enable(capi.K["MNN_GEMM"])
    capi.check(lib.xfh_bench_match_raw(ctx.h, d1p, nf, d2p, nf, -1.0, *mo, max(args.match_iters, 50), C.byref(c_warm)), ctx.h)      # the same loop with an event pair on every GEMM dispatch
    n_gemm, ms_gemm = ctx.timing_read()
    ctx.timing_enable(0)
    n_matches = int(mout.download(np.int32, 1, 12 * nf)[0])
    hm = (mout.download(np.int32, n_matches), mout.download(np.int32, n_matches, 4 * nf))
    # the device-resident hand-off: xfh_extract_batch_device_images writes each frame's descriptors also as the matcher's prepared
    # image (k_desc applies k_rownorm_img's function to the rows it has just produced), so a frame pair costs two launches
    ib = int(lib.xfh_match_image_bytes(nf))
    imgs = capi.DeviceBuffer(2 * ib)
    img1 = capi.DeviceBuffer(ib); img2 = capi.DeviceBuffer(ib)
    capi.check(lib.xfh_match_prepare_device(ctx.h, d1p, nf, img1.ptr), ctx.h)
    capi.check(lib.xfh_match_prepare_device(ctx.h, d2p, nf, img2.ptr), ctx.h)
    images_equal = None
    if B > 1:
        rec2 = capi.DeviceBuffer(2 * rec_bytes)
        capi.check(lib.xfh_extract_batch_device_images(ctx.h, in_ptr, 2, H, W, 0, 0, rec2.ptr, imgs.ptr), ctx.h)
        ctx.synchronize()
        images_equal = bool(np.array_equal(imgs.download(np.uint8, ib), img1.download(np.uint8, ib)) and
                            np.array_equal(imgs.download(np.uint8, ib, ib), img2.download(np.uint8, ib)))
        hand1, hand2 = imgs.ptr, imgs.ptr + ib
    else:
        hand1, hand2 = img1.ptr, img2.ptr
    c_prep = C.c_double(0.0)

    def warm_prepared():
        capi.check(lib.xfh_bench_match_prepared(ctx.h, hand1, nf, hand2, nf, -1.0, *mo, int(WARM_MS * 1e3 / 27.0), C.byref(c_warm)), ctx.h)
    # the hand-off call from a C loop, its GEMM dispatches carrying HIP events (GEMM, post, GEMM, post, ... back to back)
    warm_prepared()
    capi.check(lib.xfh_bench_match_prepared(ctx.h, hand1, nf, hand2, nf, -1.0, *mo, max(args.match_iters, 50), C.byref(c_prep)), ctx.h)   # wall time per call, no events on the dispatches
    ctx.timing_enable(capi.K["MNN_GEMM"])
    capi.check(lib.xfh_bench_match_prepared(ctx.h, hand1, nf, hand2, nf, -1.0, *mo, max(args.match_iters, 50), C.byref(c_warm)), ctx.h)   # the same loop with an event pair on every GEMM dispatch
    n_gemm_p, ms_gemm_p = ctx.timing_read()
    ctx.timing_enable(0)
    n_matches_h = int(mout.download(np.int32, 1, 12 * nf)[0])
    hh = (mout.download(np.int32, n_matches_h), mout.download(np.int32, n_matches_h, 4 * nf))

    def match_prepared():
        capi.check(lib.xfh_match_mnn_prepared_device(ctx.h, img1.ptr, nf, img2.ptr, nf, -1.0, *mo), ctx.h)
    warm_prepared()
    t0 = time.perf_counter()
    for _ in range(args.match_iters):
        match_prepared()
    ctx.synchronize()
    prep_dt = (time.perf_counter() - t0) / args.match_iters
    n_matches_p = int(mout.download(np.int32, 1, 12 * nf)[0])
    hp = (mout.download(np.int32, n_matches_p), mout.download(np.int32, n_matches_p, 4 * nf))
    # host API
    raw = d_recb.download(np.uint8, rec_bytes * min(B, 2))
    recs = ctx.parse_records(raw, min(B, 2))
    d1h, d2h = recs[0][1], recs[min(1, B - 1)][1]
    for _ in range(5):
        ctx.match_mnn(d1h, d2h)
    t0 = time.perf_counter()
    for _ in range(50):
        ctx.match_mnn(d1h, d2h)
    host_match_dt = (time.perf_counter() - t0) / 50
    gemm_b2b = C.c_double(0.0)
    gemm_b2b_windows = []
    for _ in range(12 if args.match_warm_ms > 0 else 1):    # consecutive windows of 300 launches; the last one is reported (the list shows the ramp)
        capi.check(lib.xfh_bench_mnn_gemm(ctx.h, img1.ptr, nf, img2.ptr, nf, 300, C.byref(gemm_b2b)), ctx.h)
        gemm_b2b_windows.append(round(gemm_b2b.value, 2))
    gemm_us_raw = ms_gemm / max(n_gemm, 1) * 1e3
    gemm_us_disp = ms_gemm_p / max(n_gemm_p, 1) * 1e3                  # per-dispatch events inside the hand-off call loop
    gemm_us = gemm_b2b.value                                            # HIP events around a region of 300 back-to-back launches / 300 (last window)
    gemm_flop = 2.0 * nf * nf * 64
    gemm_tf = gemm_flop / (gemm_us * 1e-6) / 1e12 if gemm_us else 0.0
    n_gemm = 300
    out["match"] = {"pairs_per_s": nf * nf / (c_prep.value * 1e-6), "us_per_call": c_prep.value, "n1": nf, "n2": nf, "n_matches": n_matches_h,
                    "call": "device-resident hand-off: the two frames' prepared images come out of xfh_extract_batch_device_images, the match is "
                            "xfh_match_mnn_prepared_device (k_mnn_gemm_img + k_mnn_post), calls back to back from a C loop (xfh_bench_match_prepared: "
                            "wall time between two stream events / calls)",
                    "images_from_extraction_equal_prepare_device": images_equal,
                    "pairs_equal_raw": bool(np.array_equal(hm[0], hh[0]) and np.array_equal(hm[1], hh[1])),
                    "raw_rows": {"pairs_per_s": nf * nf / (c_raw.value * 1e-6), "us_per_call": c_raw.value, "ctypes_loop_us_per_call": match_dt * 1e6,
                                 "call": "xfh_match_mnn_device on raw descriptor rows: k_rownorm_img + k_mnn_gemm_img + k_mnn_post (C loop / Python ctypes loop)"},
                    "prepared": {"pairs_per_s": nf * nf / prep_dt, "us_per_call": prep_dt * 1e6,
                                 "call": "xfh_match_mnn_prepared_device on two images made by xfh_match_prepare_device, from a Python ctypes loop",
                                 "pairs_equal_raw": bool(np.array_equal(hm[0], hp[0]) and np.array_equal(hm[1], hp[1]))},
                    "host_api_us_per_call": host_match_dt * 1e6,
                    "roofline": {"kernel": "k_mnn_gemm_img", "bound": "mfma", "achieved": gemm_tf, "peak": PEAK_F32_MFMA_TFLOPS,
                                 "unit": "TFLOP/s", "frac": gemm_tf / PEAK_F32_MFMA_TFLOPS,
                                 "traffic": (traffic or {}).get("gemm_bytes_per_launch"), "mfma_busy": pmc_busy("k_mnn_gemm_img"), "mfma_busy_source": PMC_BUSY_SRC, "avg_launch_us": gemm_us,
                                 "launches": n_gemm, "flops_per_launch": gemm_flop, "windows_us": gemm_b2b_windows,
                                 "measured": "two HIP events on the kernel's stream around a region of 300 launches of the kernel back to back (xfh_bench_mnn_gemm), elapsed / 300; "
                                             "twelve such regions in a row (windows_us), the last one reported.  The GPU reaches the clock it then holds only after ~20 ms of "
                                             "continuous load: the first windows after an idle gap read 0.67-0.70, the settled ones 0.74 (tools/gemm_b2b.py; rounds 1-3 timed this "
                                             "kernel inside the ramp).  rocprofv3 --kernel-trace of the same loop gives the same average for the settled launches "
                                             "(profiles/r04_gemm_b2b.md)",
                                 "per_dispatch_events_in_call_loop": {
                                     "avg_launch_us": gemm_us_disp, "frac": gemm_flop / (gemm_us_disp * 1e-6) / 1e12 / PEAK_F32_MFMA_TFLOPS if gemm_us_disp else 0.0, "launches": n_gemm_p,
                                     "note": "an event pair attached to every GEMM dispatch (hipExtLaunchKernelGGL) inside the C loop of two-launch hand-off calls (GEMM, post, GEMM, post, ...), "
                                             "after 60 ms of the same calls.  This view is longer than the kernel: the instrumented dispatch itself costs time (the same loop without the "
                                             "events runs 4-5 us per call faster: us_per_call), and in a busy queue the timestamps of neighbouring dispatches overlap (their sum exceeds "
                                             "the wall time, NOTES.md 5).  Rounds 1-3 reported this figure, measured cold, as the roofline"},
                                 "in_raw_rows_call": {"avg_launch_us": gemm_us_raw, "frac": gemm_flop / (gemm_us_raw * 1e-6) / 1e12 / PEAK_F32_MFMA_TFLOPS if gemm_us_raw else 0.0,
                                                      "note": "per-dispatch events inside the C loop of three-launch calls (k_rownorm_img in front), same warm-up"}}}

    # ---- many pairs in one call: frame 0 against P partners (the tracker's frame against previous frame / key frames / loop candidates; the
    # reference calls ORBmatcher::match once per pair).  One persistent GEMM launch (k_mnn_gemm_seg) + one post launch for all pairs.
    P = args.match_pairs
    nfr_img = min(B, P + 1)
    bimgs = capi.DeviceBuffer(nfr_img * ib); brec = capi.DeviceBuffer(nfr_img * rec_bytes)
    capi.check(lib.xfh_extract_batch_device_images(ctx.h, in_ptr, nfr_img, H, W, 0, 0, brec.ptr, bimgs.ptr), ctx.h)
    ctx.synchronize()
    partners = [1 + (k % max(nfr_img - 1, 1)) if nfr_img > 1 else 0 for k in range(P)]
    t_img1 = (C.c_void_p * P)(*[bimgs.ptr] * P); t_img2 = (C.c_void_p * P)(*[bimgs.ptr + j * ib for j in partners])
    t_n = (C.c_int * P)(*[nf] * P)
    bout = capi.DeviceBuffer(P * 12 * nf + 64); bcnt = capi.DeviceBuffer(4 * P + 64)
    t_i1 = (C.c_void_p * P)(*[bout.ptr + k * 12 * nf for k in range(P)]); t_i2 = (C.c_void_p * P)(*[bout.ptr + k * 12 * nf + 4 * nf for k in range(P)])
    t_ds = (C.c_void_p * P)(*[bout.ptr + k * 12 * nf + 8 * nf for k in range(P)])

    def match_batch():
        capi.check(lib.xfh_match_mnn_prepared_batch_device(ctx.h, P, t_img1, t_n, t_img2, t_n, -1.0, t_i1, t_i2, t_ds, bcnt.ptr), ctx.h)
    for _ in range(30):
        match_batch()
    ctx.synchronize()
    bk = bcnt.download(np.int32, P)
    batch_lists = [(bout.download(np.int32, int(bk[k]), k * 12 * nf), bout.download(np.int32, int(bk[k]), k * 12 * nf + 4 * nf),
                    bout.download(np.float32, int(bk[k]), k * 12 * nf + 8 * nf)) for k in range(P)]
    same = True                                             # the batched call against the pair-by-pair call, every pair
    for k in range(P):
        capi.check(lib.xfh_match_mnn_prepared_device(ctx.h, bimgs.ptr, nf, bimgs.ptr + partners[k] * ib, nf, -1.0, *mo), ctx.h)
        ctx.synchronize()
        nk = int(mout.download(np.int32, 1, 12 * nf)[0])
        same = same and nk == int(bk[k]) and np.array_equal(mout.download(np.int32, nk), batch_lists[k][0]) and \
            np.array_equal(mout.download(np.int32, nk, 4 * nf), batch_lists[k][1]) and np.array_equal(mout.download(np.float32, nk, 8 * nf), batch_lists[k][2])
    c_bat, c_seg = C.c_double(0.0), C.c_double(0.0)
    # whole calls back to back from a C loop (no foreign-function gap between the calls), the GEMM's dispatches carrying HIP events
    capi.check(lib.xfh_bench_match_batch(ctx.h, P, t_img1, t_n, t_img2, t_n, -1.0, t_i1, t_i2, t_ds, bcnt.ptr, int(WARM_MS * 1e3 / (21.0 * P)) + 1, C.byref(c_warm)), ctx.h)   # warm-up (above)
    capi.check(lib.xfh_bench_match_batch(ctx.h, P, t_img1, t_n, t_img2, t_n, -1.0, t_i1, t_i2, t_ds, bcnt.ptr, max(40, args.match_iters // P), C.byref(c_bat)), ctx.h)    # wall time per call, no events
    ctx.timing_enable(capi.K["MNN_GEMM_SEG"])
    capi.check(lib.xfh_bench_match_batch(ctx.h, P, t_img1, t_n, t_img2, t_n, -1.0, t_i1, t_i2, t_ds, bcnt.ptr, max(40, args.match_iters // P), C.byref(c_warm)), ctx.h)   # with an event pair per GEMM dispatch
    n_seg, ms_seg = ctx.timing_read()
    ctx.timing_enable(0)
    sclk_in = C.c_double(0.0)
    seg_windows = []
    for _ in range(6 if args.match_warm_ms > 0 else 1):
        capi.check(lib.xfh_bench_mnn_gemm_batch(ctx.h, P, t_img1, t_n, t_img2, t_n, 100, C.byref(c_seg), C.byref(sclk_in)), ctx.h)
        seg_windows.append(round(c_seg.value, 2))
    sclk, cpm = C.c_double(0.0), C.c_double(0.0)
    capi.check(lib.xfh_bench_sclk(ctx.h, 4096, C.byref(sclk), C.byref(cpm)), ctx.h)
    seg_us_disp = ms_seg / max(n_seg, 1) * 1e3                           # per-dispatch events inside the call loop
    seg_us = c_seg.value                                                # events around 100 back-to-back launches / 100 (last window)
    seg_flop = 2.0 * nf * nf * 64 * P
    peak_at_sclk = PEAK_F32_MFMA_TFLOPS * sclk_in.value / 2400.0         # 157.3 TFLOP/s = 256 CUs x 256 flop/clk x 2.4 GHz
    out["match"]["batched"] = {
        "pairs": P, "n1": nf, "n2": nf, "us_per_call": c_bat.value, "us_per_pair": c_bat.value / P, "pairs_per_s": P * nf * nf / (c_bat.value * 1e-6),
        "n_matches": [int(x) for x in bk],
        "call": f"xfh_match_mnn_prepared_batch_device: frame 0's prepared image against the images of {P} partner frames (as written by xfh_extract_batch_device_images), "
                "k_mnn_gemm_seg + k_mnn_post_batch, calls back to back from a C loop (xfh_bench_match_batch: wall time between two stream events / calls)",
        "pair_lists_equal_pair_by_pair_calls": bool(same),
        "roofline": {"kernel": "k_mnn_gemm_seg", "bound": "mfma", "achieved": seg_flop / (seg_us * 1e-6) / 1e12 if seg_us else 0.0, "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
                     "frac": seg_flop / (seg_us * 1e-6) / 1e12 / PEAK_F32_MFMA_TFLOPS if seg_us else 0.0, "mfma_busy": pmc_busy("k_mnn_gemm_seg"), "mfma_busy_source": PMC_BUSY_SRC,
                     "avg_launch_us": seg_us, "launches": 100, "flops_per_launch": seg_flop, "windows_us": seg_windows,
                     "measured": "two HIP events on the kernel's stream around a region of 100 launches of the kernel back to back (xfh_bench_mnn_gemm_batch), elapsed / 100; six such "
                                 "regions in a row after 60 ms of batched calls (windows_us), the last one reported (clock ramp and method: match.roofline.measured)",
                     "per_dispatch_events_in_call_loop": {
                         "avg_launch_us": seg_us_disp, "frac": seg_flop / (seg_us_disp * 1e-6) / 1e12 / PEAK_F32_MFMA_TFLOPS if n_seg else 0.0, "launches": n_seg,
                         "note": "an event pair attached to every GEMM dispatch inside the C loop of batched calls (xfh_bench_match_batch: GEMM, post, GEMM, post, ...): includes the "
                                 "instrumented dispatch's own cost and the overlap of neighbouring timestamps (match.roofline.per_dispatch_events_in_call_loop)"}}}
    # the clock the f32 MFMA peak is priced at (2.4 GHz -> 157.3 TFLOP/s) is not the clock the GPU holds under this load
    out["match"]["sclk_under_f32_mfma_load"] = {
        "sclk_mhz": sclk_in.value, "sclk_mhz_mfma_loop_on_constant_operands": sclk.value, "cycles_per_mfma_oldest_wave": cpm.value, "peak_at_sclk_TFLOPs": peak_at_sclk,
        "frac_of_peak_at_sclk": {"k_mnn_gemm_img": gemm_tf / peak_at_sclk if peak_at_sclk else None,
                                 "k_mnn_gemm_seg": seg_flop / (seg_us * 1e-6) / 1e12 / peak_at_sclk if (peak_at_sclk and seg_us) else None},
        "measured": "sclk_mhz: shader clocks (s_memtime) per 100 MHz reference tick (s_memrealtime) that workgroup 0 of k_mnn_gemm_seg saw across one launch of the batched "
                    "GEMM (xfh_bench_mnn_gemm_batch); the second figure: xfh_bench_sclk, every SIMD issuing v_mfma_f32_32x32x2_f32 back to back on constant operands. "
                    "f32 MFMAs and VALU instructions share the SIMD's vector pipe on gfx950 (profiles/r04_pipe_probe.log), so the ceiling of the GEMM with its arg-max "
                    "epilogue is below this peak as well: NOTES.md 5"}
    for b in (bimgs, brec, bout, bcnt):
        b.free()

    # ---- what a tracker at 30 Hz sees: ONE match call per 33 ms on an otherwise idle GPU, i.e. inside the clock ramp the back-to-back loops above
    # deliberately leave.  Two stream events around the single call (xfh_bench_match_prepared with one iteration).
    if not args.only_match_leg:
        paced = []
        c_one = C.c_double(0.0)
        for _ in range(24):
            time.sleep(0.033)
            capi.check(lib.xfh_bench_match_prepared(ctx.h, hand1, nf, hand2, nf, -1.0, *mo, 1, C.byref(c_one)), ctx.h)
            paced.append(c_one.value)
        paced_s = sorted(paced[4:])
        out["match"]["paced_30hz"] = {"us_per_call_median": paced_s[len(paced_s) // 2], "us_per_call_min": paced_s[0], "us_per_call_max": paced_s[-1], "calls": len(paced_s),
                                      "frac_of_peak": gemm_flop / (paced_s[len(paced_s) // 2] * 1e-6) / 1e12 / PEAK_F32_MFMA_TFLOPS,
                                      "note": "one xfh_match_mnn_prepared_device call every 33 ms from an idle GPU, two stream events around the call: the GPU never leaves its idle clock, "
                                              "so this is slower than `us_per_call` (calls back to back on a settled clock); it is what a 30 Hz tracker that matches once per frame gets"}

    # ---- the other matcher kernels (no timing anywhere in round 1) ----------------------------------------------------
    aux = {}
    rng = np.random.RandomState(1)
    for name, kid, fn in (
        ("k_dist_i32 4096x4096 (64 MB table)", "DIST_I32", lambda: ctx.distance_i32(d1h, d2h)),
        ("k_best2_csr 4096 queries x 64 candidates", "BEST2", None),
        ("k_distinctive_csr 4096 groups x 16 rows", "DISTINCTIVE", None)):
        if kid == "BEST2":
            off = (np.arange(nf + 1) * 64).astype(np.int32); ind = rng.randint(0, nf, nf * 64).astype(np.int32)
            fn = lambda: ctx.best2_csr(d1h, d2h, off, ind)
        if kid == "DISTINCTIVE":
            off2 = (np.arange(nf + 1) * 16).astype(np.int32); ind2 = rng.randint(0, nf, nf * 16).astype(np.int32)
            fn = lambda: ctx.distinctive_csr(d1h, off2, ind2)
        fn()
        ctx.timing_enable(capi.K[kid])
        for _ in range(5):
            fn()
        nl, ms = ctx.timing_read()
        ctx.timing_enable(0)
        aux[name] = {"kernel_us": ms / max(nl, 1) * 1e3, "launches": nl}
    # the dense table once more on device-resident rows, back to back (the five host-API calls above each start from an idle GPU, inside the clock ramp)
    dk = "k_dist_i32 4096x4096 (64 MB table)"
    aux[dk]["from_idle_kernel_us"] = aux[dk]["kernel_us"]
    b1 = capi.DeviceBuffer(d1h.nbytes).upload(d1h); b2 = capi.DeviceBuffer(d2h.nbytes).upload(d2h); tbl = capi.DeviceBuffer(4 * nf * nf)
    for _ in range(60):
        capi.check(lib.xfh_distance_i32_device(ctx.h, b1.ptr, nf, b2.ptr, nf, tbl.ptr), ctx.h)
    ctx.synchronize()
    ctx.timing_enable(capi.K["DIST_I32"])
    for _ in range(100):
        capi.check(lib.xfh_distance_i32_device(ctx.h, b1.ptr, nf, b2.ptr, nf, tbl.ptr), ctx.h)
    ctx.synchronize()
    nl, ms = ctx.timing_read(); ctx.timing_enable(0)
    aux[dk].update({"kernel_us": ms / max(nl, 1) * 1e3, "launches": nl,
                    "measured": "dispatch events over 100 back-to-back launches on device-resident rows after 60 of the same (settled clock); from_idle_kernel_us = the same kernel inside five host-API calls"})
    for b_ in (b1, b2, tbl):
        b_.free()
    aux[dk]["hbm_write_GBps"] = nf * nf * 4 / (aux[dk]["kernel_us"] * 1e-6) / 1e9
    aux[dk]["mfma_TFLOPs"] = 2.0 * nf * nf * 64 / (aux[dk]["kernel_us"] * 1e-6) / 1e12
    aux[dk]["frac_of_f32_mfma_peak"] = aux[dk]["mfma_TFLOPs"] / PEAK_F32_MFMA_TFLOPS
    out["aux_kernels"] = aux

    # ---- CPU baseline + parity verdict (N == 1 only) ------------------------------------------------------------------
    out["cpu_baseline"] = None
    out["parity"] = None
    if N == 1 and args.cpu_frames > 0:
        from oracle import oracle as O
        orc = O.Oracle(blob)
        ncores = usable_cores()
        cpu_legs = {}
        # 1 thread, and the best of {all usable hardware threads, 32, 16}: the oracle's OpenMP loops stop scaling (and on an
        # over-subscribed box collapse) well before a few hundred threads; every leg is bounded to a few seconds
        for nthr in sorted({1, ncores, min(ncores, 32), min(ncores, 16)}):
            O.set_threads(nthr)
            t0 = time.perf_counter()
            orc.extract(frames[0], nf, (0, 0))                          # warm-up, also sizes the leg
            warm = time.perf_counter() - t0
            nfr = max(1, min(args.cpu_frames if nthr > 1 else 2, int(6.0 / max(warm, 1e-3))))
            t0 = time.perf_counter()
            for i in range(nfr):
                orc.extract(frames[i % B], nf, (0, 0))
            fdt = (time.perf_counter() - t0) / nfr
            t0 = time.perf_counter()
            om = O.match_mnn(d1h, d2h)
            mdt = time.perf_counter() - t0
            cpu_legs[nthr] = (fdt, mdt, nfr)
        best = min((k for k in cpu_legs if k > 1), key=lambda k: cpu_legs[k][0], default=1)
        O.set_threads(best)
        ok, od, onv, omono = orc.extract(frames[0], nf, (0, 0))
        cand = orc.tensor(O.T["CAND"]).reshape(-1, 3)
        k1h = orc.tensor(O.T["K1H"])
        hk, hd, hnv, hmono, hnc = recs[0]
        vo, vh = ok["size"] > 0, hk["size"] > 0
        so = set(zip(ok["x"][vo].astype(int).tolist(), ok["y"][vo].astype(int).tolist()))
        sh = set(zip(hk["x"][vh].astype(int).tolist(), hk["y"][vh].astype(int).tolist()))
        po = {(int(k["x"]), int(k["y"])): i for i, k in enumerate(ok) if k["size"] > 0}
        ph = {(int(k["x"]), int(k["y"])): i for i, k in enumerate(hk) if k["size"] > 0}
        common = [k for k in po if k in ph]
        ddesc = max((float(np.abs(od[po[k]] - hd[ph[k]]).max()) for k in common), default=0.0)
        # near-tie audit: how many discrete decisions of this frame / match have a margin below 1e-6
        sc = np.sort(cand[:, 2].astype(np.float64))[::-1]
        top = sc[:min(len(sc), nf + 1)]
        cos = d1h.astype(np.float32) @ d2h.astype(np.float32).T        # audit only: not the kernel's summation order
        part = np.partition(cos, -2, axis=1)
        audit = {"margin": 1e-6,
                 "nms_threshold_pixels": int(np.count_nonzero(np.abs(k1h.astype(np.float64) - 0.05) < 1e-6)),
                 "score_positive_cut": int(np.count_nonzero(np.abs(sc) < 1e-6)),
                 "topk_cut_gap": float(top[nf - 1] - top[nf]) if len(top) > nf else None,
                 "topk_adjacent_score_pairs": int(np.count_nonzero(np.abs(np.diff(top)) < 1e-6)),
                 "mnn_rows_with_runner_up_gap": int(np.count_nonzero(part[:, -1] - part[:, -2] < 1e-6))}
        out["parity"] = {"keypoint_sets_equal": so == sh, "n_valid": [int(onv), int(hnv)], "max_abs_desc_diff": ddesc,
                         "match_pairs_equal": bool(np.array_equal(om[0], hm[0]) and np.array_equal(om[1], hm[1])),
                         "match_pairs_equal_prepared": bool(np.array_equal(om[0], hp[0]) and np.array_equal(om[1], hp[1])),
                         "n_candidates": int(hnc), "near_tie_audit": audit}
        fdt, mdt, nfr = cpu_legs[best]
        f1, m1, n1r = cpu_legs[1]
        # north_star: "the libtorch CPU path timed on the same box's host cores".  The reference itself cannot be built here (OpenCV);
        # its libtorch operator sequence can: oracle/torch_restatement.py in a child process (torch is imported nowhere else)
        import subprocess
        lt = None
        try:
            thr = sorted({1, min(ncores, 16), ncores})
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--libtorch-leg", ",".join(str(t) for t in thr), "--height", str(H), "--width", str(W)],
                               capture_output=True, text=True, timeout=420)
            if r.returncode == 0:
                lt = json.loads(r.stdout.strip().splitlines()[-1])
            else:
                lt = {"skipped": "child failed: " + r.stderr.strip()[-300:]}
        except Exception as e:       # noqa: BLE001
            lt = {"skipped": f"{type(e).__name__}: {e}"}
        if lt and "legs" in lt:
            bt = max(lt["legs"], key=lambda k: lt["legs"][k]["frames_per_s"])
            lt.update({"kind": "restatement of the reference's libtorch operator sequence (oracle/torch_restatement.py), NOT the reference binary",
                       "best": {"cores": int(bt), **lt["legs"][bt]}, "one_thread": lt["legs"].get("1")})
        out["cpu_baseline"] = {"value": 1.0 / fdt, "unit": "frames/s", "cores": best, "kind": "port", "cpu_model": cpu_model(),
                               "host_hardware_threads": os.cpu_count(), "usable_hardware_threads": ncores,
                               "sample": f"{nfr} of the same {H}x{W} frames through oracle/xfeat_oracle.c (OpenMP, {best} threads = the fastest of the thread counts tried); "
                                         f"4096x4096 MNN once: {nf * nf / mdt:.3e} pairs/s",
                               "match_pairs_per_s": nf * nf / mdt,
                               "one_thread": {"value": 1.0 / f1, "unit": "frames/s", "cores": 1, "match_pairs_per_s": nf * nf / m1,
                                              "sample": f"{n1r} frames, 4096x4096 MNN once, 1 thread"},
                               "legs": {str(k): {"frames_per_s": 1.0 / v[0], "match_pairs_per_s": nf * nf / v[1], "frames": v[2]} for k, v in sorted(cpu_legs.items())},
                               "libtorch_ops": lt}


if __name__ == "__main__":
    main()
