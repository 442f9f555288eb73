"""The res3 + res4 + res5 + FPN + DB head training step (forward + backward) on ResNet-50's product shape (C2 160 x 160 x 256, C3 80 x 80 x
512, C4 40 x 40 x 1024, C5 20 x 20 x 2048, P2 160 x 160): the HIP kernels (csrc/bottleneck_train.hip at all three widths, csrc/fpn_train.hip,
csrc/dbhead_train.hip through FeaturePyramidNetwork.forward_padded(taps, head=head, res5=res5, res4=res4, res3=res3)) against the res4 + res5
+ FPN + head step on the same C2 and a fixed C3 (forward_padded([C2, C3], head=head, res5=res5, res4=res4)), so that res3's share is a
difference of two of this tool's own numbers, and torch eager autograd of the same thirteen Bottlenecks (eval-mode BatchNorm) + FPN + head
in fp32 with its own res3 share, on the same GPU.  The C2 tap is a fixed random tensor and the upstream map gradients fixed tensors of
~1e-7, so only the trained stages are timed.  Then the train-mode trunk-engine call of the mode, DetectorEngine.forward_c2(x) (the stem and
res2), against forward_trunk(x)[:1] (the whole trunk), on `--batch` frames of 640 x 640.  Every call is timed on its own with HIP events
after `--warmup` calls of each variant, the variants alternating; the figure of a variant is the median of its `--iters` calls.  Per-launch
times of one step come from torch.profiler in a pass of their own after the timing.  Prints one JSON line.

    python tools/res3_train_bench.py [--batch 32] [--iters 15] [--warmup 3] [--no-torch] [--no-engine]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/res3_train_bench.py --step-only --iters 5

`--step-only` runs the HIP step of this mode alone, `--warmup` + `--iters` times, and prints nothing but the count: for a profiler run of its
own, whose per-kernel totals then belong to this step and nothing else.
"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "video-text-detection-system_amd"), ROOT, os.path.dirname(os.path.abspath(__file__))]

import torch  # noqa: E402

from dbhead_train_bench import per_launch  # noqa: E402
from fpn_train_bench import wiring  # noqa: E402
from res4_train_bench import medians  # noqa: E402
from res5_train_bench import torch_bottleneck  # noqa: E402
from vtd_amd import nets  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch comparison")
    ap.add_argument("--no-engine", action="store_true", help="skip the trunk-engine calls")
    ap.add_argument("--step-only", action="store_true", help="run the HIP step of this mode alone (for a profiler run of its own)")
    args = ap.parse_args()
    n, h5, w5, c5 = args.batch, 20, 20, 2048
    H, W = 8 * h5, 8 * w5
    torch.manual_seed(0)
    mk = lambda f, seed: (lambda m: (m.load_state_dict(nets.seeded_state_dict(f, seed)), m)[1])(f())  # noqa: E731
    res3 = torch.nn.Sequential(mk(lambda: nets.Bottleneck(256, 128, 2), 13), *(mk(lambda: nets.Bottleneck(512, 128, 1), 14 + i) for i in range(3))).cuda()
    res4 = torch.nn.Sequential(mk(lambda: nets.Bottleneck(512, 256, 2), 6), *(mk(lambda: nets.Bottleneck(1024, 256, 1), 7 + i) for i in range(5))).cuda()
    res5 = torch.nn.Sequential(mk(lambda: nets.Bottleneck(1024, 512, 2), 3), mk(lambda: nets.Bottleneck(2048, 512, 1), 4),
                               mk(lambda: nets.Bottleneck(2048, 512, 1), 5)).cuda()
    fpn = mk(lambda: nets.FeaturePyramidNetwork(c5), 2).cuda()
    head = mk(lambda: nets.DBHead(256), 1).cuda().train()
    rres3, rres4, rres5, rfpn, rhead = (copy.deepcopy(m) for m in (res3, res4, res5, fpn, head))
    g = torch.Generator(device="cuda").manual_seed(0)
    c2 = (torch.randn((n, c5 >> 3, H, W), generator=g, device="cuda") * 0.5).half()
    padded = [nets.pack_tap(c2)]
    c3p = nets.forward_res3_padded(res3, padded[0])
    c3f = c3p[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).float().contiguous()
    gp = torch.randn((n, 1, 4 * H, 4 * W), generator=g, device="cuda") * 1e-7
    gt = torch.randn((n, 1, 4 * H, 4 * W), generator=g, device="cuda") * 1e-7

    def zero(*mods):
        for m in mods:
            m.zero_grad(set_to_none=True)

    def hip_step():
        zero(res3, res4, res5, fpn, head)
        out = fpn.forward_padded(padded, head=head, res5=res5, res4=res4, res3=res3)
        torch.autograd.backward([out["probability"], out["threshold"]], [gp, gt])

    def hip_res4_step():
        zero(res4, res5, fpn, head)
        out = fpn.forward_padded(padded + [c3p], head=head, res5=res5, res4=res4)
        torch.autograd.backward([out["probability"], out["threshold"]], [gp, gt])

    def torch_tail(c3):
        x, taps = c3, [c2.float(), c3]
        for stage in (rres4, rres5):
            for b in stage:
                x = torch_bottleneck(b, x)
            taps.append(x)
        p2 = wiring(rfpn, taps)
        torch.autograd.backward([rhead.probability_head(p2), rhead.threshold_head(p2)], [gp, gt])

    def torch_step():
        zero(rres3, rres4, rres5, rfpn, rhead)
        x = c2.float()
        for b in rres3:
            x = torch_bottleneck(b, x)
        torch_tail(x)

    def torch_res4_step():
        zero(rres4, rres5, rfpn, rhead)
        torch_tail(c3f)

    if args.step_only:
        for _ in range(args.warmup + args.iters):
            hip_step()
        torch.cuda.synchronize()
        print(json.dumps({"batch": n, "hip_steps": args.warmup + args.iters}))
        return
    steps = {"hip_step_ms": hip_step, "hip_res4_step_ms": hip_res4_step}
    if not args.no_torch:
        steps.update({"torch_fp32_step_ms": torch_step, "torch_fp32_res4_step_ms": torch_res4_step})
    med, spread = medians(steps, args.iters, args.warmup)
    res = {"batch": n, "c2": [256, H, W], "c3": [512, 4 * h5, 4 * w5], "c4": [1024, 2 * h5, 2 * w5], "c5": [c5, h5, w5], "iters": args.iters}
    res.update({k: round(v, 3) for k, v in med.items()})
    res["min_max_ms"] = {k: [round(x, 3) for x in v] for k, v in spread.items()}
    res["res3_ms"] = round(med["hip_step_ms"] - med["hip_res4_step_ms"], 3)
    if not args.no_torch:
        res["torch_fp32_res3_ms"] = round(med["torch_fp32_step_ms"] - med["torch_fp32_res4_step_ms"], 3)
        res["speedup_vs_torch_fp32"] = round(med["torch_fp32_step_ms"] / med["hip_step_ms"], 2)
        res["res3_speedup_vs_torch_fp32"] = round(res["torch_fp32_res3_ms"] / max(res["res3_ms"], 1e-9), 2)
    launches = per_launch(hip_step, [])
    res["hip_launches"] = len(launches)
    by = {}
    for nm, us in launches:
        by.setdefault(nm, [0, 0.0])
        by[nm][0] += 1
        by[nm][1] += us
    res["hip_by_kernel_us"] = sorted(([nm, c, round(us, 1)] for nm, (c, us) in by.items()), key=lambda r: -r[2])
    if not args.no_engine:
        # the train-mode trunk-engine call: the mode's forward_c2 against what the modes above it call, on the same engine
        torch.cuda.empty_cache()
        from vtd_amd.engine import DetectorEngine
        eng = DetectorEngine("resnet50", nets.seeded_state_dict(lambda: nets.DBNet("resnet50"), 5), max_batch=n, options={"fuse_fpn_head": 0})
        x = torch.randn((n, 3, 640, 640), generator=g, device="cuda")
        emed, espread = medians({"engine_forward_c2_ms": lambda: eng.forward_c2(x), "engine_forward_trunk_ms": lambda: eng.forward_trunk(x)[:1]},
                                args.iters, args.warmup)
        res.update({k: round(v, 3) for k, v in emed.items()})
        res["min_max_ms"].update({k: [round(v, 3) for v in vs] for k, vs in espread.items()})
        res["engine_saved_ms"] = round(emed["engine_forward_trunk_ms"] - emed["engine_forward_c2_ms"], 3)
        eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
