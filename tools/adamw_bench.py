"""The optimiser step of the detector's training loop on the GPU: torch.optim.AdamW as configure_optimizers builds it (torch's default
path), torch.optim.AdamW(fused=True) where the installed build accepts it on this device, and vtd_amd.training.AdamW (one multi-tensor HIP
pass per parameter group: vtd_adamw_step, csrc/adamw.hip), on the parameters of DBNet("resnet18", compute_threshold=True) and
DBNet("resnet50", compute_threshold=True) with every gradient present.  Each candidate owns its parameters and state, all read the same
gradients; the candidates ALTERNATE in one process: `--rounds` rounds of `--steps` steps each between two device events per candidate,
after `--warmup` steps each; reported per candidate are the median, the lowest and the highest round (microseconds per step).  Also: the
launches of one step (torch.profiler's device events), the 28 B per element the update must move (p, g, m, v in; p, m, v out) and the
time of that floor at `--hbm-tbs`, the achieved TB/s of the HIP step, and the host time of one HIP step() call -- a host clock around the
call with no synchronise: it measures the enqueue.  `--step` adds the whole training_step -> backward -> optimizer.step of
DBNet("resnet18", trainable="head+fpn+backbone") at `--batch` x 640 x 640 with either optimiser.  Prints one JSON line.

    python tools/adamw_bench.py [--rounds 5] [--steps 10] [--warmup 5] [--hbm-tbs 6.3] [--step] [--batch 32]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "video-text-detection-system_amd"), ROOT, os.path.dirname(os.path.abspath(__file__))]

import torch  # noqa: E402

from dbhead_train_bench import per_launch  # noqa: E402
from vtd_amd import _native, nets, training  # noqa: E402

BYTES_PER_ELEMENT = 28


def candidates(shapes, grads, lr, wd):
    """name -> (optimizer, params): own copies of the parameters (seeded values), shared gradient tensors."""
    gen = torch.Generator(device="cuda").manual_seed(1)
    start = [torch.randn(s, generator=gen, device="cuda") * 0.05 for s in shapes]
    out = {}
    for name, make in (("torch_default", lambda ps: torch.optim.AdamW(ps, lr=lr, weight_decay=wd)),
                       ("torch_fused", lambda ps: torch.optim.AdamW(ps, lr=lr, weight_decay=wd, fused=True)),
                       ("hip", lambda ps: training.AdamW(ps, lr=lr, weight_decay=wd))):
        params = [t.clone().requires_grad_() for t in start]
        for p, g in zip(params, grads):
            p.grad = g
        try:
            opt = make(params)
            opt.step()   # state creation, code objects
            torch.cuda.synchronize()
        except (RuntimeError, ValueError) as e:
            if name != "torch_fused":
                raise
            out[name] = str(e).splitlines()[0][:200]   # this build or device has no fused AdamW: reported, not timed
            continue
        out[name] = (opt, params)
    return out


def bench_model(backbone, args):
    model = nets.DBNet(backbone, compute_threshold=True)
    shapes = [tuple(p.shape) for p in model.parameters()]
    del model
    gen = torch.Generator(device="cuda").manual_seed(2)
    grads = [torch.randn(s, generator=gen, device="cuda") * 1e-3 for s in shapes]
    elements = sum(g.numel() for g in grads)
    floor_us = elements * BYTES_PER_ELEMENT / (args.hbm_tbs * 1e6)
    res = {"tensors": len(shapes), "elements": elements, "bytes_per_step": elements * BYTES_PER_ELEMENT, "floor_us": round(floor_us, 1),
           "arrays_MB_per_candidate": round(elements * 16 / 2 ** 20, 1)}
    cands = candidates(shapes, grads, 1e-4, 1e-5)
    live = {k: v for k, v in cands.items() if not isinstance(v, str)}
    for k, v in cands.items():
        if isinstance(v, str):
            res[k] = {"unavailable": v}
    for opt, _ in live.values():
        for _ in range(args.warmup):
            opt.step()
    torch.cuda.synchronize()
    rounds = {k: [] for k in live}
    for _ in range(args.rounds):
        for k, (opt, _) in live.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                opt.step()
            b.record()
            b.synchronize()
            rounds[k].append(a.elapsed_time(b) * 1e3 / args.steps)
    for k, (opt, _) in live.items():
        launches = per_launch(opt.step, [])
        names = {}
        for nm, _us in launches:
            names[nm] = names.get(nm, 0) + 1
        med = statistics.median(rounds[k])
        res[k] = {"us_per_step": round(med, 1), "lowest_round_us": round(min(rounds[k]), 1), "highest_round_us": round(max(rounds[k]), 1),
                  "steps_timed": args.rounds * args.steps, "TBps": round(elements * BYTES_PER_ELEMENT / med / 1e6, 2),
                  "launches": len(launches), "kernel_us_sum": round(sum(us for _, us in launches), 1), "launch_table": names}
    # the enqueue: a host clock around step() with nothing to wait for behind it and no synchronise after it
    opt = live["hip"][0]
    torch.cuda.synchronize()
    host = []
    for _ in range(20):
        t0 = time.perf_counter()
        opt.step()
        host.append((time.perf_counter() - t0) * 1e6)
        torch.cuda.synchronize()
    res["hip"]["host_enqueue_us"] = round(statistics.median(host), 1)
    fastest_torch = min(res[k]["us_per_step"] for k in live if k != "hip")
    res["hip_over_fastest_torch"] = round(res["hip"]["us_per_step"] / fastest_torch, 3)
    return res


def bench_step(args):
    """training_step -> backward -> optimizer.step of the whole detector, per optimiser, alternating."""
    from vtd_amd._fixtures.weights import stress_detector_state_dict
    gen = torch.Generator().manual_seed(3)
    x = torch.randn((args.batch, 3, 640, 640), generator=gen).cuda()
    shape = (args.batch, 1, 640, 640)
    targets = {"probability_map": (torch.rand(shape, generator=gen) < 0.2).float().cuda(),
               "threshold_map": (0.3 + 0.4 * torch.rand(shape, generator=gen)).cuda()}
    runs = {}
    for name in ("torch", "hip"):
        net = nets.DBNet("resnet18", compute_threshold=True, trainable="head+fpn+backbone")
        net.load_state_dict(stress_detector_state_dict("resnet18", 17))
        net.cuda().train()
        mod = training.TextDetectionLightningModule(net, optimizer=name)
        opt = mod.configure_optimizers()["optimizer"]

        def step(mod=mod, opt=opt, with_opt=True):
            loss = mod.training_step((x, targets), 0)
            opt.zero_grad()
            loss.backward()
            if with_opt:
                opt.step()
        runs[name] = step
    for fn in runs.values():
        for _ in range(max(2, args.warmup // 2)):
            fn()
    torch.cuda.synchronize()
    keys = [("torch", True), ("hip", True), ("hip", False)]
    times = {k: [] for k in keys}
    for _ in range(args.rounds):
        for name, with_opt in keys:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(2):
                runs[name](with_opt=with_opt)
            b.record()
            b.synchronize()
            times[(name, with_opt)].append(a.elapsed_time(b) / 2)
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"batch": args.batch, "trainable": "head+fpn+backbone", "steps_timed": 2 * args.rounds,
            "step_ms_torch_adamw": round(med[("torch", True)], 3), "step_ms_hip_adamw": round(med[("hip", True)], 3),
            "step_ms_without_optimizer": round(med[("hip", False)], 3),
            "hip_adamw_share_of_step": round((med[("hip", True)] - med[("hip", False)]) / med[("hip", True)], 4),
            "torch_adamw_share_of_step": round((med[("torch", True)] - med[("hip", False)]) / med[("torch", True)], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="steps per round and candidate (rounds x steps >= 50 are timed)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="HBM streaming rate for the bytes-moved floor, TB/s")
    ap.add_argument("--step", action="store_true", help="also time the whole training step with either optimiser")
    ap.add_argument("--batch", type=int, default=32)
    args = ap.parse_args()
    _native.require()
    res = {"hbm_tbs": args.hbm_tbs, "bytes_per_element": BYTES_PER_ELEMENT}
    for backbone in ("resnet18", "resnet50"):
        res[backbone] = bench_model(backbone, args)
        torch.cuda.empty_cache()
    if args.step:
        res["training_step"] = bench_step(args)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
