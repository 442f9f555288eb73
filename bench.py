#!/usr/bin/env python3
"""Throughput bench for the MI355X text-detection hot path.

    python bench.py --gpus N --steps K --warmup W

A step = one pass of the hot path over one batch of synthetic frames that are already resident in HBM:
fused preprocess (BGR uint8 720p -> 640x640 fp16) -> DBNet-ResNet18 (fp16 MFMA) -> post-process to boxes
[-> crop + CRNN + CTC decode when --workload full].  Workload at N=1 = BASELINE.json configs[1]
("Batch=32 720p frames, DBNet detector only, 1xMI355X fp16"); frames and "margin" weights as SURVEY.md 8d.
For N>1 every rank runs its own 32 frames (weak scaling, frames shard with no data-path collective); the
only exchange is the gather of detection records to every rank (RCCL all_gather of a small padded block).

Prints ONE JSON line on rank 0 (contract in the task statement) with `roofline` (dominant kernel = the
implicit-GEMM convolution, timed with HIP events on its launch stream across the timed region),
`cpu_baseline` (the CPU oracle timed on this host on a bounded sample of the same workload, in the two shapes of
BASELINE.md section 4: reference-shaped N=1 calls from 4 threads, and best-case batched) and `sustained` (the same step
back to back for >= 5 s after the timed region, with the shader clocks the host reports before and after).

Every leg rotates over ROTATE distinct resident batches (4 x 88 MB at 720p: more than the 256 MB Infinity Cache), so no
step reads a batch that an earlier step left in cache.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.join(ROOT, "video-text-detection-system_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

MFMA_PEAK_TFLOPS = 2500.0  # dense fp16, /opt/skills/guides/MI355X_MICROARCH.md "Peak BF16/FP16 MFMA ~2.5 PF dense"
HBM_PEAK_GBS = 8000.0      # HBM3E, same guide
ROTATE = 4                 # distinct resident input batches per rank


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--backbone", default="resnet18")
    ap.add_argument("--workload", default="full", choices=["full", "detector"],
                    help="full = BASELINE configs[2] (detect + recognize); detector = configs[1]")
    ap.add_argument("--recognizer", default="crnn", choices=["crnn", "trocr"],
                    help="crnn = BASELINE configs[2]; trocr = the Transformer recogniser of configs[4] (trocr-base-printed architecture, seeded weights)")
    ap.add_argument("--mixed", action="store_true",
                    help="BASELINE configs[4] batch: frames alternate 720p / 1080p; the pipeline groups them by shape (one device pass per "
                         "size, results back in frame order) exactly as process_video does")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="budget PER SHAPE for the cpu_baseline samples (0 = skip)")
    ap.add_argument("--sustain-seconds", type=float, default=5.0,
                    help="length of the sustained leg after the timed region (0 = skip); reported as `sustained`, never as `value`")
    ap.add_argument("--no-profile", action="store_true", help="skip the per-launch HIP-event timing")
    ap.add_argument("--upload", action="store_true",
                    help="PCIe-inclusive variant (not the headline value): every step uploads its batch from pinned host memory "
                         "on an upload stream")
    ap.add_argument("--layers-out", default=None, help="write the per-launch table as JSON to this path")
    ap.add_argument("--dry-run", action="store_true",
                    help="launcher / rendezvous / aggregation only (gloo, no GPU work): what the CPU test of the N>1 entry runs")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write the result dicts of the last timed step (rank 0) as DIR/<name>.npy "
                         "(float32 / float64): same arguments, same inputs, so two builds can be compared output for output")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def launch_ranks(args):
    """`python bench.py --gpus N` without a torchrun wrapper: this parent starts the N ranks itself as fresh child processes
    (one per GPU) and never touches the GPU (it does not even import torch), relays rank 0's JSON line and exits non-zero
    if any rank does.  Under `python -m torch.distributed.run ... bench.py --gpus N` WORLD_SIZE is already set and this is
    not taken."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *sys.argv[1:]], env=env,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr))
    import threading
    chunks = []
    reader = threading.Thread(target=lambda: chunks.append(procs[0].stdout.read()), daemon=True)
    reader.start()
    # a rank that dies leaves the others waiting in a collective: stop them (exact PIDs) instead of hanging with them
    while any(p.poll() is None for p in procs):
        if any(p.poll() not in (None, 0) for p in procs):
            for p in procs:
                if p.poll() is None:
                    p.terminate()
            break
        time.sleep(0.05)
    codes = []
    for p in procs:
        try:
            codes.append(p.wait(timeout=20))
        except subprocess.TimeoutExpired:
            p.kill()
            codes.append(p.wait())
    reader.join(timeout=5)
    for line in b"".join(chunks).decode().splitlines():   # the JSON line to stdout, library chatter (gloo banners) to stderr
        print(line, file=sys.stdout if line.lstrip().startswith("{") else sys.stderr)
    sys.stdout.flush()
    bad = [(r, c) for r, c in enumerate(codes) if c != 0]
    if bad:
        print(f"bench.py: ranks failed (rank, exit code): {bad}", file=sys.stderr)
        return 1
    return 0


def dry_run(args, rank, world):
    """The N>1 control flow without the GPU: rendezvous, barrier, MAX-over-ranks of the elapsed time, one JSON line."""
    if os.environ.get("VTD_BENCH_FAIL_RANK") == str(rank):   # test hook: this rank dies before the rendezvous
        raise SystemExit(3)
    import torch
    import torch.distributed as dist
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        dist.barrier()
    t0 = time.perf_counter()
    time.sleep(0.01 * (rank + 1))
    t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        ranks = [None] * world
        dist.all_gather_object(ranks, (rank, int(os.environ.get("LOCAL_RANK", "0"))))
    else:
        ranks = [(0, 0)]
    if rank == 0:
        print(json.dumps({"metric": "dry-run", "value": 0.0, "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "dry_run": True, "ranks": ranks, "elapsed_max_s": float(t.item())}))
    if world > 1:
        dist.destroy_process_group()


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: WORLD_SIZE={world} does not match --gpus {args.gpus}")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if args.dry_run:
        return dry_run(args, rank, world)
    import numpy as np
    import torch
    from vtd_amd._fixtures import synth, weights
    from vtd_amd.engine import DeviceFrames, detector_profile

    torch.cuda.set_device(local_rank % max(torch.cuda.device_count(), 1))
    if os.environ.get("VTD_BENCH_DET_PRIORITY") == "1":   # experiment: the caller's (detector) stream above the side streams
        torch.cuda.set_stream(torch.cuda.Stream(priority=-1))
    dist = None
    if world > 1:
        import torch.distributed as dist
        # backend "nccl" is RCCL on ROCm; VTD_DIST_BACKEND=gloo lets two ranks rehearse the N>1 path on one GPU
        dist.init_process_group(os.environ.get("VTD_DIST_BACKEND", "nccl"), rank=rank, world_size=world)

    B, H, W = args.batch, args.height, args.width
    SIZES = [(720, 1280), (1080, 1920)]
    if args.mixed and (args.upload or args.workload != "full" or B % 2):
        raise SystemExit("--mixed needs --workload full, an even --batch and no --upload")

    def host_batch(k):
        """Batch k of this rank (k = 0..ROTATE-1), every frame with its own seed: list of HxWx3 uint8 arrays."""
        base = (2000 if args.mixed else 100) + (rank * ROTATE + k) * B
        return [synth.text_frame(base + i, *(SIZES[i % 2] if args.mixed else (H, W)))[0] for i in range(B)]

    host_batches = [host_batch(k) for k in range(ROTATE)]
    frames = host_batches[0]                                   # the CPU baseline's sample comes from the same frames
    if args.mixed:      # resident per-frame tensors of two sizes: the pipeline groups them by shape at every step
        mixed_batches = [[torch.from_numpy(f).cuda() for f in hb] for hb in host_batches]
        dev_batches = None
    else:
        dev_batches = [DeviceFrames(np.stack(hb)) for hb in host_batches]
    resident_mb = sum(f.nbytes for hb in host_batches for f in hb) / 1e6
    if args.upload:
        pinned_batches = [torch.from_numpy(np.stack(hb)).pin_memory() for hb in host_batches]
        upload_stream = torch.cuda.Stream()
    sd = weights.margin_detector_state_dict(args.backbone, 0)
    from vtd_amd import nets as mynets
    from vtd_amd import shard
    from vtd_amd.pipeline import VideoTextPipeline
    os.environ["VTD_MAX_BATCH"] = str(B)
    if args.recognizer == "trocr":
        # Twelve steps' crops share one recogniser pass at B <= 32 (four above): a decode step costs about the same for 300 or 3000 live
        # rows, and the slot of a crop is 0.89 MB of encoder states (28 MB of keys / values in the reference's form, VTD_TROCR_XATTN=0: ask
        # for fewer tickets there).  360 / 372 / 394-408 / 410-426 frames/s at 4 / 6 / 8 / 12 tickets (tools/gpu_pass_sweep.sh; a pass holds at most
        # 4096 rows); results come that many steps later -- process_video returns when the
        # whole video is done, so the reference's caller does not see the difference.
        os.environ.setdefault("VTD_TROCR_PASS_TICKETS", "12" if B <= 32 else "4")
        os.environ.setdefault("VTD_TROCR_MAX_CROPS", "3456" if B <= 32 else "2560")
        # a full pass runs on the engine's worker thread while this thread keeps feeding the detector: the detector's launches of the next
        # pass's batches fall into the decode's launch-bound tail (+1 % here, +4.5 % on configs[4] with its 5.5-ms ResNet-50 detector passes)
        os.environ.setdefault("VTD_TROCR_ASYNC", "1")
        os.environ.setdefault("VTD_TROCR_SEEDED", "0")   # explicit opt-in: the architecture on synthetic weights (nothing is fetchable)
    pipe = VideoTextPipeline(use_transformer_ocr=args.recognizer == "trocr", backbone=args.backbone, batch_size=B)
    pipe.detector.max_detections = MAX_DET = 64
    pipe.detector.model._max_batch = B        # the engine is built at first use: size it for this batch (VTD_MAX_BATCH is read at import)
    pipe.detector.model.load_state_dict(sd)
    # VTD_BENCH_CRNN=default: torch-default-init recogniser weights (round-1 bench; every crop decodes to two characters)
    rec_sd = (mynets.seeded_state_dict(lambda: mynets.CRNN(97), seed=11) if os.environ.get("VTD_BENCH_CRNN") == "default"
              else weights.margin_crnn_state_dict(11))
    if args.recognizer == "crnn":
        pipe.recognizer.model.load_state_dict(rec_sd)
    eng = pipe.detector.model.engine()
    lib = eng.lib
    last = {}
    crops_seen = {"n": 0, "batches": 0}

    inflight = {"det": None}
    rec_q = []                             # jobs whose recogniser has been submitted, oldest first
    rec_lag = pipe._recognizer_lag() if args.workload == "full" else 1

    turn = {"k": 0}

    ahead = {}

    def next_batch():
        k = turn["k"] = (turn["k"] + 1) % ROTATE
        if not args.upload:
            return dev_batches[k]
        # --upload: the copy of the NEXT step's batch is issued now, behind this step's (a video loop has its next batch staged while
        # the current one is in the detector: pipeline._stage runs at push time, one batch ahead of the GPU); VTD_BENCH_UPLOAD_AHEAD=0
        # issues each copy at the start of its own step instead
        if os.environ.get("VTD_BENCH_UPLOAD_AHEAD", "1") == "0":
            return DeviceFrames(pinned_batches[k], stream=upload_stream)
        cur = ahead.pop(k, None) or DeviceFrames(pinned_batches[k], stream=upload_stream)
        ahead.clear()
        ahead[(k + 1) % ROTATE] = DeviceFrames(pinned_batches[(k + 1) % ROTATE], stream=upload_stream)
        return cur

    def note(results):
        last["results"] = results
        crops_seen["n"] += sum(len(r["detections"]) for r in results)
        crops_seen["batches"] += 1

    def step_detector():
        # the product's detector half, two batches in flight: enqueue batch i (preprocess -> DBNet on the caller's stream,
        # post-process + record copy on the side stream), then turn the records of batch i-1 into the result dicts
        t = pipe.detector.submit_batch(next_batch(), 0.5)
        if inflight["det"] is not None:
            last["detections"] = pipe.detector.finish_batch(inflight["det"])
        inflight["det"] = t
        return [(t["keep"][1][:B], t["keep"][2][:B])]

    def drain_detector():
        if inflight["det"] is not None:
            last["detections"] = pipe.detector.finish_batch(inflight["det"])
            inflight["det"] = None

    # full workload: the product's batched pass, software-pipelined three deep exactly as a video loop would run it --
    # detector(i) is enqueued, then the host collects the boxes of batch i-1 and enqueues its recogniser, then builds
    # the result dicts of batch i-2.  Every step retires one whole batch (result dicts included).
    def step_full():
        job = pipe.submit_detection(next_batch())
        keep = job["det"]["keep"]
        if inflight["det"] is not None:   # same order as VideoTextPipeline._pipeline_push: recogniser of batch i-1 first ...
            rec_q.append(pipe.submit_recognition(inflight["det"]))
        # ... then the result dicts of batch i-1-lag (lag = 1 for the CRNN; the Transformer recogniser keeps more tickets in flight so
        # that the encoder pass of the next recogniser pass runs beside the decode of the one being collected: pipeline._recognizer_lag)
        while len(rec_q) > rec_lag:
            note(pipe.collect(rec_q.pop(0)))
        inflight["det"] = job
        return [(keep[1][:B], keep[2][:B])]

    def drain_full():
        if inflight["det"] is not None:
            rec_q.append(pipe.submit_recognition(inflight["det"]))
            inflight["det"] = None
        while rec_q:
            note(pipe.collect(rec_q.pop(0)))

    # configs[4]: the batch alternates 720p / 1080p.  It goes through the very entry process_video uses (_pipeline_push): frames are
    # grouped by shape, each group is one device pass, the groups ride the three-deep pipeline and come back in frame order.
    mixed_info = [(i, i / 30.0) for i in range(B)]

    def step_mixed():
        k = turn["k"] = (turn["k"] + 1) % ROTATE
        done = pipe._pipeline_push(mixed_batches[k], mixed_info)
        if done:
            note(done)
        jobs = [j for j in pipe._inflight if not j.get("failed")][-len(SIZES):]   # this push's two shape groups
        return [(j["det"]["keep"][1], j["det"]["keep"][2]) for j in jobs if "det" in j]

    def drain_mixed():
        done = pipe._pipeline_drain()
        if done:
            note(done[-B:])

    step_once = step_mixed if args.mixed else step_full if args.workload == "full" else step_detector
    drain = drain_mixed if args.mixed else drain_full if args.workload == "full" else drain_detector

    def step():
        blocks = step_once()
        if world > 1:
            # the one exchange step of the path: detection records of every rank to every rank.  Enqueued on the stream
            # that produced them (the detector's post-process side stream), so it is ordered behind the records without
            # stalling the caller's stream, where the next batch's DBNet is already queued.
            side = pipe.detector._post_stream()
            with torch.cuda.stream(side if side is not None else torch.cuda.current_stream()):
                for rec, cnt in blocks:
                    last["gathered"] = shard.gather_detections(rec, cnt)
        return blocks

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # one priming pass over every resident batch whatever --warmup says: the first call at a batch size runs the per-layer
    # autotune and the workspace allocations (hundreds of ms), which are set-up cost, not a step of the path
    for _ in range(ROTATE if args.mixed else 1):
        step()
    drain()
    # From here on the loop runs as VideoTextPipeline.process_video runs it: with the long-lived heap out of the cyclic collector's
    # sight (vtd_amd.pipeline.quiet_gc; VTD_QUIET_GC=0 to see what the collector costs: 12 % of the sustained rate)
    from vtd_amd.pipeline import quiet_gc
    gc_guard = quiet_gc()
    gc_guard.__enter__()
    for _ in range(args.warmup):
        step()
    drain()
    barrier()
    # Untimed survey pass: every launch of the detector graph bracketed with HIP events -> per-launch table and the identity
    # of the dominant launch.  The timed region then brackets only that launch (2 events per step).
    survey, dom = [], -1
    if not args.no_profile:
        lib.vtd_detector_set_profiling(eng.handle, 1)
        for _ in range(3):  # one batch at a time, drained: every launch has the GPU to itself (no other stream running)
            step()
            drain()
            torch.cuda.synchronize()
        barrier()
        survey = detector_profile(eng)
        dom = max(range(len(survey)), key=lambda i: survey[i][1] if survey[i][3] > 0 else -1.0)
        lib.vtd_detector_set_profiling(eng.handle, 2 + dom)
    crops_seen["n"] = crops_seen["batches"] = 0
    teng = pipe.recognizer.model.engine() if args.recognizer == "trocr" and args.workload == "full" else None
    if teng is not None and not args.no_profile:
        teng.profile()                 # drop what the warm-up left
        teng.set_profiling(3)          # HIP events around every dense-GEMM launch of the encoder pass (bit 1: the kernel with the largest share
                                       # of the recogniser's time) and the decoder's cross-attention launch of layer 0 of every step (bit 0)
    stamps = []
    t0 = time.perf_counter()
    for _ in range(args.steps):
        blocks = step()
        stamps.append(time.perf_counter())
    drain()  # K batches submitted -> K batches retired (result dicts built) inside the timed region
    stamps.append(time.perf_counter())
    barrier()
    elapsed = time.perf_counter() - t0
    # what the caller received for the last timed step (the sustained leg below overwrites `last`)
    timed_last = last.get("results" if args.workload == "full" else "detections")
    if os.environ.get("VTD_BENCH_STAMPS") == "1" and rank == 0:
        print("per-step host times (ms): " + " ".join(f"{1e3 * (b - a):.2f}" for a, b in zip([t0] + stamps, stamps)) +
              f" | barrier {1e3 * (t0 + elapsed - stamps[-1]):.2f}", file=sys.stderr)
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    crops_per_step = crops_seen["n"] / max(crops_seen["batches"], 1)

    # ---- sanity: the timed path produced detections (not part of the timed region), and nothing was swallowed on the way: the product keeps
    # the reference's error convention (log, empty result, go on), under which a recogniser that fails every pass would post a splendid rate
    n_det = int(sum(int(cnt.sum().item()) for _, cnt in blocks))
    swallowed = dict(getattr(pipe, "error_counts", {}) or {})
    if swallowed:
        print(f"bench.py: the pipeline swallowed errors during the run ({swallowed}); no number is reported", file=sys.stderr)
        raise SystemExit(3)
    if args.workload == "full" and last.get("results") is not None:
        texts = [d.get("text", "") for r in last["results"] for d in r["detections"]]
        if texts and not any(texts):
            print("bench.py: every recognised text of the last batch is empty; no number is reported", file=sys.stderr)
            raise SystemExit(3)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, timed_last)

    roofline = None
    layer_rows = []
    if not args.no_profile:
        timed = detector_profile(eng)  # only slot `dom` carries events from the timed region
        lib.vtd_detector_set_profiling(eng.handle, 0)
        convs = []
        for name, ms, calls, macs in survey:
            layer_rows.append({"launch": name, "ms_total": ms, "calls": calls, "gmac_total": macs / 1e9,
                               "tflops": (2 * macs / (ms * 1e-3) / 1e12) if ms > 0 and macs > 0 else None})
            if macs > 0 and calls > 0:
                convs.append((name, ms / calls, macs / calls))
        name, ms, calls, macs = timed[dom]
        achieved = 2 * macs / (ms * 1e-3) / 1e12
        iso_ms, iso_calls, iso_macs = survey[dom][1], survey[dom][2], survey[dom][3]
        conv_us = sum(r[1] for r in convs) * 1e3  # per step, survey pass
        # algorithmic (reference-graph) FLOPs of the whole detector per step, SURVEY 8d: 69.8 GFLOP / frame for R18
        algo_flops_step = 2.0 * eng.macs_per_frame * B
        if args.backbone == "resnet18" and B == 32 and (H, W) == (720, 1280) and not args.mixed:
            traffic, traffic_detail, traffic_error = lookup_traffic(name)
        else:   # the committed PMC passes were taken on the default configuration: another trunk / batch moves other bytes per launch
            traffic, traffic_detail, traffic_error = None, None, None
        roofline = {"bound": "mfma", "kernel": name, "achieved": round(achieved, 2), "peak": MFMA_PEAK_TFLOPS,
                    "unit": "TFLOP/s", "frac": round(achieved / MFMA_PEAK_TFLOPS, 4), "traffic": traffic,
                    "traffic_unit": "HBM bytes per launch (read + written)", "traffic_detail": traffic_detail,
                    "launches": calls, "avg_launch_us": round(ms / calls * 1e3, 2),
                    "executed_gflop_per_launch": round(2 * macs / calls / 1e9, 3),
                    "alone_on_gpu": {"avg_launch_us": round(iso_ms / iso_calls * 1e3, 2),
                                     "tflops": round(2 * iso_macs / (iso_ms * 1e-3) / 1e12, 2),
                                     "frac": round(2 * iso_macs / (iso_ms * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS, 4),
                                     "what": "same launch in the untimed survey pass, one batch at a time: in the timed region the "
                                             "recogniser and post-process streams share the CUs with it, which stretches its wall time"},
                    "note": "achieved = FLOPs this launch EXECUTES / its HIP-event time on the launch stream; the composed conv replaces "
                            "lateral(C2)+top-down add+P2 smooth+head conv of the reference graph with ~3x fewer FLOPs, so the "
                            "reference-graph rate over all matrix launches is given as net_algorithmic_tflops; peak = nominal dense fp16 "
                            "(a bare MFMA loop sustains ~2.3 PFLOP/s on this part, tools/mfma_peak.hip)",
                    "all_mfma_launches_tflops_executed": round(sum(2 * r[2] for r in convs) / (conv_us * 1e-6) / 1e12, 2),
                    "net_algorithmic_tflops": round(algo_flops_step / (conv_us * 1e-6) / 1e12, 2),
                    "detector_mfma_launches_us_per_step": round(conv_us, 1)}
        if traffic_error:
            roofline["traffic_error"] = traffic_error
            print("bench.py: " + traffic_error, file=sys.stderr)
            if os.environ.get("VTD_BENCH_STRICT") == "1":
                raise SystemExit(2)
        if args.layers_out and rank == 0:
            with open(args.layers_out, "w") as f:
                json.dump(layer_rows, f, indent=1)

    if teng is not None and not args.no_profile:
        # The Transformer line is bound by its recogniser.  Its dominant kernel BY SHARE OF KERNEL TIME is the encoder pass's dense GEMM
        # (profiles/r03_trocr_pipeline_kernel_stats.csv: dense_gemm_kernel 33 % against 15.5 % for the decoder's cross-attention), an
        # MFMA-bound launch: `roofline` is that kernel's, FLOPs executed (2 M N K per launch) / its HIP-event time on the stream it is
        # launched on, inside the timed region.  The decoder's largest launch, the HBM-bound cross-attention (every live row's encoder states --
        # or, in the reference's form, its keys and values -- read once per layer and step), is kept as a secondary record.
        ms, calls, rows = teng.profile()
        gms, gcalls, gflops = teng.gemm_profile()
        teng.set_profiling(0)
        spec = pipe.recognizer.model.spec
        detector_roofline = roofline
        cross = None
        if calls:
            # bytes every live row's launch reads: keys + values of the layer ([T][D] fp16 each), or -- cross-attention on the raw encoder
            # states (engine.xattn) -- the encoder states themselves ([T][C] fp16, once)
            xattn = bool(getattr(teng, "xattn", False))
            per_row = spec.enc_tokens * (spec.enc_hidden * 2 if xattn else spec.dec_hidden * 2 * 2)
            bytes_total = rows * per_row
            achieved = bytes_total / (ms * 1e-3) / 1e9
            traffic, traffic_detail, traffic_error = lookup_traffic("dec_xattn" if xattn else "dec_cross_attn")   # its largest launch: rows stated in traffic_detail
            cross = {"bound": "hbm", "kernel": ("dec_xattn_kernel<24> (decoder cross-attention on the encoder states, trocr_xattn.hip), layer 0 of every step" if xattn else
                                                "dec_attn_kernel<false, 4, 10> (decoder cross-attention, trocr_decode.hip), layer 0 of every step"),
                     "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
                     "traffic": traffic, "traffic_unit": "HBM bytes per launch (read + written)", "traffic_detail": traffic_detail,
                     "launches": calls, "avg_launch_us": round(ms / calls * 1e3, 2), "avg_live_rows_per_launch": round(rows / calls, 1),
                     "algorithmic_bytes_per_launch": int(bytes_total / calls),
                     "note": ("algorithmic bytes = live rows x encoder tokens (577) x encoder width (768) x 2 B: the row's encoder states, read once per "
                              "launch (the same states for all 12 layers of a step: below ~280 live rows they stay in the 256 MB Infinity Cache, so "
                              "short launches can exceed the HBM rate); " if xattn else
                              "algorithmic bytes = live rows x encoder tokens (577) x d_model (1024) x 2 B x (K + V): every byte is read once per "
                              "launch; ") +
                             "rows that have emitted </s> are not read (the live list shrinks from ~1100 to a handful over a pass), so "
                             "late launches are latency-bound, not bandwidth-bound; peak = 8 TB/s HBM3E (MI355X_MICROARCH.md)"}
            if traffic_error:
                cross["traffic_error"] = traffic_error
                print("bench.py: " + traffic_error, file=sys.stderr)
        if gcalls:
            achieved = gflops / (gms * 1e-3) / 1e12
            roofline = {"bound": "mfma", "kernel": "dense_gemm_kernel<false, 16> / <true, 1> (dense_gemm.hip): the encoder pass's dense layers" +
                                                   ("" if getattr(teng, "xattn", False) else " and the cross-attention key / value projections"),
                        "achieved": round(achieved, 2), "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(achieved / MFMA_PEAK_TFLOPS, 4),
                        "traffic": None, "launches": gcalls, "avg_launch_us": round(gms / gcalls * 1e3, 2),
                        "executed_gflop_per_launch": round(gflops / gcalls / 1e9, 2),
                        "note": "the Transformer recogniser's kernel with the largest share of kernel time; achieved = executed FLOPs (2 M N K, "
                                "M = crops of the merged pass x 577 tokens) summed over every launch of the timed region / their summed HIP-event "
                                "time on the recogniser's stream; peak = nominal dense fp16",
                        "decoder_cross_attention": cross,
                        "detector_dominant_kernel": detector_roofline}
        elif cross is not None:   # (reduced architectures whose GEMMs stay on the implicit GEMM)
            roofline = dict(cross, detector_dominant_kernel=detector_roofline)

    # ---- sustained leg (not `value`): the same step back to back for >= --sustain-seconds, clocks before and after
    sustained = None
    if args.sustain_seconds > 0:
        n_sus = max(args.steps, int(args.sustain_seconds / (elapsed / args.steps)) + 1)   # same count on every rank (elapsed is the MAX)
        import threading
        clk0, samples, stop = read_sclk_mhz(), [], threading.Event()

        def sampler():   # the clocks DURING the leg (a read after it finds the card already idling at its lowest level)
            while not stop.wait(0.25):
                samples.append(read_sclk_mhz())

        th = threading.Thread(target=sampler, daemon=True)
        barrier()
        th.start()
        t1 = time.perf_counter()
        for _ in range(n_sus):
            step()
        drain()
        barrier()
        dt = time.perf_counter() - t1
        stop.set()
        th.join(timeout=2)
        if world > 1:
            t = torch.tensor([dt], dtype=torch.float64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        sustained = {"seconds": round(dt, 3), "steps": n_sus, "value": round(world * B * n_sus / dt, 2), "unit": "frames/s",
                     "ms_per_step": round(dt / n_sus * 1e3, 3), "vs_timed_region": round((world * B * n_sus / dt) / (world * B * args.steps / elapsed), 4),
                     "sclk_mhz_before": clk0,
                     "sclk_mhz_during": {"samples": len(samples),
                                         "min": [min(v) for v in zip(*samples)] if samples else None,
                                         "median": [sorted(v)[len(v) // 2] for v in zip(*samples)] if samples else None,
                                         "max": [max(v) for v in zip(*samples)] if samples else None},
                     "what": "same steps back to back, started right after the timed region; sclk = current level (pp_dpm_sclk) of every "
                             "card the host exposes under /sys/class/drm (ours is among them; the others belong to other tenants), read just "
                             "before the leg and every 0.25 s during it"}

    cpu_baseline = None
    if rank == 0 and args.gpus == 1 and args.cpu_seconds > 0:
        cpu_baseline = cpu_baselines(args, frames, sd, rec_sd)

    gc_guard.__exit__(None, None, None)
    if rank == 0:
        total_frames = world * B * args.steps
        out = {
            "metric": "frames/sec (detect+recognize) @720p, 1/2/4/8 MI355X; box IoU vs CPU ref",
            "value": round(total_frames / elapsed, 2),
            "unit": "frames/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f16",
            "data": "synthetic" + (" (uploaded from pinned host memory every step: PCIe-inclusive variant)" if args.upload else ""),
            "config": {"workload": (f"B={B} {H}p frames, DBNet-{args.backbone} detector only (preprocess+net+post-process), fp16"
                                    if args.workload == "detector" else
                                    f"B={B} {'mixed 720p/1080p (alternating, grouped by shape on the device path)' if args.mixed else str(H) + 'p'} frames, full pipeline: DBNet-{args.backbone} + crop + "
                                    + ("TrOCR (ViT-base-384 encoder + 12-layer decoder, greedy max_length=50)" if args.recognizer == "trocr"
                                       else "CRNN + CTC decode") + " -> result dicts, fp16"),
                       "global_batch": world * B, "frame": "alternating 720x1280 / 1080x1920" if args.mixed else [H, W], "backbone": args.backbone,
                       "parallelism": f"frames sharded over {world} rank(s), detections all-gathered",
                       "resident_input": f"{ROTATE} distinct batches per rank, {resident_mb:.0f} MB, visited round-robin",
                       "detections_last_step_rank0": n_det,
                       "crops_recognized_per_step_rank0": round(crops_per_step, 1),
                       "crops_recognized_last_step_rank0": (sum(len(r["detections"]) for r in last["results"]) if "results" in last else 0)},
            "roofline": roofline,
            "cpu_baseline": cpu_baseline,
            "sustained": sustained,
        }
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, per_frame):
    """The last timed step's results as float arrays, one row per detection in frame order: `frame` (index in the batch), `bbox` [N,4],
    `polygon` [N,4,2], `detection_confidence`, and for the full workload `text` [N,L] (Unicode code points, 0-padded) and
    `recognition_confidence`; `detections_per_frame` [B].  Above DUMP_LIMIT_BYTES a fixed, seeded sample of the rows is kept."""
    import numpy as np
    if per_frame is None:
        raise SystemExit("bench.py: --dump-outputs: the timed steps returned no results")
    full = bool(per_frame) and isinstance(per_frame[0], dict)   # pipeline result dicts; the detector workload returns detection lists
    per_frame = [r["detections"] if full else r for r in per_frame]
    dets = [(i, d) for i, r in enumerate(per_frame) for d in r]
    rows = {"frame": np.array([i for i, _ in dets], np.float64),
            "bbox": np.array([d["bbox"] for _, d in dets], np.float64).reshape(-1, 4),
            "polygon": np.array([d["polygon"] for _, d in dets], np.float64).reshape(-1, 4, 2),
            "detection_confidence": np.array([d["detection_confidence" if full else "confidence"] for _, d in dets], np.float64)}
    if full:
        width = max([len(d["text"]) for _, d in dets] + [1])
        text = np.zeros((len(dets), width), np.float32)
        for k, (_, d) in enumerate(dets):
            text[k, :len(d["text"])] = [ord(c) for c in d["text"]]
        rows["text"] = text
        rows["recognition_confidence"] = np.array([d["recognition_confidence"] for _, d in dets], np.float64)
    counts = np.array([len(r) for r in per_frame], np.float64)
    per_row = sum(a[:1].nbytes for a in rows.values())
    budget = DUMP_LIMIT_BYTES - counts.nbytes - 4096 * (len(rows) + 1)   # (an .npy header is at most a few hundred bytes)
    if per_row and len(dets) * per_row > budget:
        keep = np.sort(np.random.default_rng(0).choice(len(dets), budget // per_row, replace=False))
        rows = {k: a[keep] for k, a in rows.items()}
    rows["detections_per_frame"] = counts
    os.makedirs(out_dir, exist_ok=True)
    for name, a in rows.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def read_sclk_mhz():
    """Current shader-clock level of every card under /sys/class/drm (the line pp_dpm_sclk marks with '*'), in MHz."""
    import glob
    import re
    out = []
    for path in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk")):
        try:
            cur = [ln for ln in open(path).read().splitlines() if ln.rstrip().endswith("*")]
            m = re.search(r"(\d+)\s*Mhz", cur[0], re.I) if cur else None
            out.append(int(m.group(1)) if m else None)
        except OSError:
            out.append(None)
    return out


# launch-slot description (vtd_api.cpp: vtd_detector_get_profile) -> device kernel symbol of exactly that variant
KERNEL_SYMBOLS = (("head_entry_pair", "head_entry_pair_kernel("), ("head_entry_half", "head_entry_half_kernel<false>("),
                  ("head_entry_halo256", "head_entry_halo256_kernel<false>("), ("head_entry_halo ", "head_entry_halo_kernel<"),
                  ("classed", "true>("), ("dec_cross_attn", "dec_attn_kernel<false, 4"), ("dec_xattn", "dec_xattn_kernel<24>("))


def lookup_traffic(launch_name, profiles_dir=None):
    """HBM bytes per launch of the dominant kernel, from the newest committed rocprofv3 --pmc passes (profiles/r*_pmc_traffic_per_launch.json:
    separate FETCH_SIZE / WRITE_SIZE runs, FETCH_SIZE x2 per the gfx950 note; PMC counters cannot be collected inside this process).
    Returns (bytes, detail, error): a dominant kernel the file does not cover is an ERROR the JSON line carries (`traffic_error`) and
    tests/test_bench_launcher.py turns into a failing CPU test for the shipped selection -- never a silent null."""
    import glob
    files = sorted(glob.glob(os.path.join(profiles_dir or os.path.join(ROOT, "profiles"), "r*_pmc_traffic_per_launch.json")))
    if not files:
        return None, None, "roofline.traffic: no profiles/r*_pmc_traffic_per_launch.json in the tree"
    pmc_path = files[-1]
    symbol = next((sym for key, sym in KERNEL_SYMBOLS if key in launch_name), None)
    if symbol is None:
        return None, None, f"roofline.traffic: no kernel symbol known for the dominant launch {launch_name!r} (bench.py KERNEL_SYMBOLS)"
    try:
        pmc = json.load(open(pmc_path))
    except (OSError, ValueError) as e:
        return None, None, f"roofline.traffic: cannot read {pmc_path}: {e}"
    hits = [v for k, v in pmc.items() if symbol in k and v.get("launches", 0) >= 3]
    if not hits:
        return None, None, (f"roofline.traffic: {os.path.basename(pmc_path)} has no entry for kernel symbol {symbol!r}: the PMC passes are "
                            "stale for the kernel that now dominates -- re-run tools/gpu_evidence.sh and commit the summary")
    v = max(hits, key=lambda h: h["launches"])
    extra = {}
    if "dec_attn" in symbol:
        # the decoder's launches shrink with the live rows: cite the LARGEST grid (all rows live) and say how many rows that was, so the
        # figure can be set against the algorithmic bytes of the same launch (rows x 577 x 1024 x 2 B x 2)
        key = max((k for k, h in pmc.items() if symbol in k and h.get("launches", 0) >= 3), key=lambda k: int(k.rsplit("grid=", 1)[1]))
        v = pmc[key]
        rows_ = int(key.rsplit("grid=", 1)[1]) // (16 * 256)
        extra = {"live_rows_of_that_launch": rows_, "algorithmic_bytes_of_that_launch": rows_ * 577 * 1024 * 2 * 2}
    if "dec_xattn" in symbol:   # one 768-thread workgroup per live row; the row's encoder states [577][768] fp16 read once
        key = max((k for k, h in pmc.items() if symbol in k and h.get("launches", 0) >= 3), key=lambda k: int(k.rsplit("grid=", 1)[1]))
        v = pmc[key]
        rows_ = int(key.rsplit("grid=", 1)[1]) // 768
        extra = {"live_rows_of_that_launch": rows_, "algorithmic_bytes_of_that_launch": rows_ * 577 * 768 * 2}
    rd, wr = v["hbm_read_MB_corrected_x2"], v["hbm_write_MB"]
    detail = {**extra, "hbm_read_MB": round(rd, 2), "hbm_write_MB": round(wr, 2), "kernel_symbol": symbol,
              "source": "profiles/" + os.path.basename(pmc_path) + " (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes, median over launches, "
                        "FETCH_SIZE x2 per the gfx950 note)"}
    return int((rd + wr) * 1e6), detail, None


def cpu_baselines(args, frames, sd, rec_sd):
    """The oracle (CPU restatement, fp32 torch + C stages) timed on this host in the two shapes of BASELINE.md section 4, each on a bounded
    sample of the bench's own frames: (i) reference-shaped -- one N=1 detect per frame from 4 threads, then one recognise call per
    crop, as pipeliine.py:32,96-133 does; (ii) best-case batched -- all sampled frames in one forward, all crops in one batch."""
    import numpy as np
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from oracle import cstages, nets as onets, pipeline as opipe
    B = len(frames)
    # the 1-GPU box grants a 16-CPU share of a much larger host: more threads than that only thrash
    ncores = min(len(os.sched_getaffinity(0)), int(os.environ.get("VTD_CPU_CORES", "16")))
    torch.set_num_threads(ncores)
    full, trocr = args.workload == "full", args.recognizer == "trocr"
    if trocr:
        from oracle import trocr as otrocr
        from vtd_amd._fixtures import weights
        from vtd_amd.trocr_spec import BASE_PRINTED
        tsd = weights.trocr_state_dict(BASE_PRINTED, seed=int(os.environ.get("VTD_TROCR_SEEDED", "0") or 0))

    def crops_of(fr, dets):
        return [fr[d["bbox"][1]:d["bbox"][3], d["bbox"][0]:d["bbox"][2]] for d in dets
                if d["bbox"][2] > d["bbox"][0] and d["bbox"][3] > d["bbox"][1]]

    def recognise_one(crop):
        if trocr:
            return otrocr.recognize_ids([crop], tsd, BASE_PRINTED)
        return opipe.recognize_batch([crop], rec_sd)

    def recognise_all(crops):
        if not crops:
            return []
        if trocr:
            x = torch.stack([otrocr.preprocess(c, BASE_PRINTED) for c in crops])
            return otrocr.generate(otrocr.encode(x, tsd, BASE_PRINTED), tsd, BASE_PRINTED)[0]
        return opipe.recognize_batch(crops, rec_sd)

    opipe.detect(frames[0], sd, args.backbone, 0.5)  # warm-up (oneDNN primitive creation)
    # (i) reference-shaped: rounds of 4 frames, detect on a 4-thread pool, crops one by one (pipeliine.py:96-133)
    # (the Transformer recogniser costs seconds per crop on the CPU: its sample is one frame)
    done, t0 = 0, time.perf_counter()
    with ThreadPoolExecutor(max_workers=4) as pool:
        while done < B and time.perf_counter() - t0 < args.cpu_seconds:
            chunk = frames[done:done + (1 if trocr and full else 4)]
            dets = list(pool.map(lambda f: opipe.detect(f, sd, args.backbone, 0.5), chunk))
            if full:
                for fr, ds in zip(chunk, dets):
                    for crop in crops_of(fr, ds):
                        recognise_one(crop)
            done += len(chunk)
    dt_ref = time.perf_counter() - t0
    shaped = {"value": round(done / dt_ref, 3), "unit": "frames/s", "cores": ncores, "threads": "4 Python threads x torch intra-op pool",
              "sample": f"{done} of the step's {B} frames"}
    # (ii) best-case batched: one forward over the sample, every crop in one recogniser batch
    nb = B if args.cpu_seconds >= 10 and not trocr else max(1, min(B, 2 if trocr else 8))
    sample = frames[:nb]
    t0 = time.perf_counter()
    x = torch.cat([opipe.preprocess(f) for f in sample])
    prob = onets.dbnet_forward(x, sd, args.backbone)["probability"][:, 0].numpy()
    dets = [cstages.postprocess(prob[i], sample[i].shape[1], sample[i].shape[0], 0.5) for i in range(nb)]
    if full:
        recognise_all([c for fr, ds in zip(sample, dets) for c in crops_of(fr, ds)])
    dt_b = time.perf_counter() - t0
    batched = {"value": round(nb / dt_b, 3), "unit": "frames/s", "cores": ncores, "sample": f"one batched pass over {nb} of the step's {B} frames"}
    what = ("preprocess + DBNet-%s fp32 torch CPU + C post-process%s" %
            (args.backbone, ((" + TrOCR fp32 (ViT-base encoder, 12-layer decoder, greedy)" if trocr else " + cv-resize + CRNN fp32 + CTC decode")
                             if full else "")))
    best = max(shaped, batched, key=lambda r: r["value"])
    return {"value": best["value"], "unit": "frames/s", "cores": ncores, "kind": "port",
            "sample": ("best of the two shapes below (%s): %s; %s" % ("batched" if best is batched else "reference-shaped", best["sample"], what)),
            "reference_shaped_4_threads": shaped, "batched_B%d" % nb: batched}


if __name__ == "__main__":
    main()
