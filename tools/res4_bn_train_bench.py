"""The res4 + res5 + FPN + DB head training step (forward + backward) with batch-statistics BatchNorm in the trained Bottleneck stages, on
ResNet-50's product shape (C3 80 x 80 x 512, C4 40 x 40 x 1024, C5 20 x 20 x 2048, P2 160 x 160), for the two modes that have it: "res5"
(FeaturePyramidNetwork.forward_padded(taps, head=head, res5=res5, res_batch_stats=True) on [C2, C3, C4]) and "res4" (the same with
res4=res4 on [C2, C3]): csrc/bottleneck_bn_train.hip, the vtd_bottleneck_bn_train_* entries, the stages in train() mode, their running
statistics updated every step.  Each is timed against the frozen step of the same mode (the same call without the keyword:
csrc/bottleneck_train.hip) and against torch eager autograd of the same Bottlenecks in train() mode (F.batch_norm(..., training=True)) +
FPN + head in fp32, on the same GPU.  The trunk taps are fixed random tensors and the upstream map gradients fixed tensors of ~1e-7, so
only the trained stages are timed.  Every step is timed on its own with HIP events after `--warmup` steps of each variant, the variants
alternating; the figure of a variant is the median of its `--iters` steps.  Per-launch times of one batch step of the res4 mode come from
torch.profiler in a pass of their own after the timing, with the bytes the fp32 z round trips imply beside them.  `--frozen-only` times
the two frozen steps alone, which a library from before the batch-statistics entries can run too.  `--step-only` runs the batch step of
the res4 mode alone, `--warmup` + `--iters` times, and prints nothing but the count: for a profiler run of its own, whose per-kernel totals
then belong to this step and nothing else.  Prints one JSON line.

    python tools/res4_bn_train_bench.py [--batch 32] [--iters 15] [--warmup 3] [--no-torch] [--frozen-only]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/res4_bn_train_bench.py --step-only --iters 5
"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "video-text-detection-system_amd"), ROOT, os.path.dirname(os.path.abspath(__file__))]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from dbhead_train_bench import per_launch  # noqa: E402
from fpn_train_bench import wiring  # noqa: E402
from res4_train_bench import medians  # noqa: E402
from vtd_amd import nets  # noqa: E402


def torch_bottleneck_train(b, x):
    """The Bottleneck in torch ops with train-mode BatchNorm (the running statistics move, as the modules' would)."""
    bn = lambda m, t: F.batch_norm(t, m.running_mean, m.running_var, m.weight, m.bias, True, m.momentum, m.eps)  # noqa: E731
    a1 = F.relu(bn(b.bn1, F.conv2d(x, b.conv1.weight)))
    a2 = F.relu(bn(b.bn2, F.conv2d(a1, b.conv2.weight, None, b.stride, 1)))
    idt = bn(b.downsample[1], F.conv2d(x, b.downsample[0].weight, None, b.stride)) if hasattr(b, "downsample") else x
    return F.relu(bn(b.bn3, F.conv2d(a2, b.conv3.weight)) + idt)


def z_bytes(n, h3, w3):
    """The bytes of the fp32 z round trips of one batch step per mode: per pair one write and two reads forward (statistics, apply) and two
    reads backward (reduce, form) of z [rows][C] fp32.  Rows: conv1's are the block's input rows, the others' its output rows."""
    def block(rows_in, rows_out, W, ds):
        return 4 * (rows_in * W + rows_out * W + rows_out * 4 * W * (2 if ds else 1))
    m4, m5 = n * (h3 // 2) * (w3 // 2), n * (h3 // 4) * (w3 // 4)
    res5 = block(m4, m5, 512, True) + 2 * block(m5, m5, 512, False)
    res4 = block(n * h3 * w3, m4, 256, True) + 5 * block(m4, m4, 256, False)
    return {"res5": 5 * res5, "res4": 5 * (res4 + res5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch comparison")
    ap.add_argument("--frozen-only", action="store_true", help="time the two frozen steps alone")
    ap.add_argument("--step-only", action="store_true", help="run the batch step of the res4 mode alone (for a profiler run of its own)")
    args = ap.parse_args()
    n, h5, w5, c5 = args.batch, 20, 20, 2048
    H, W = 8 * h5, 8 * w5
    torch.manual_seed(0)
    mk = lambda f, seed: (lambda m: (m.load_state_dict(nets.seeded_state_dict(f, seed)), m)[1])(f())  # noqa: E731
    res4 = torch.nn.Sequential(mk(lambda: nets.Bottleneck(512, 256, 2), 6), *(mk(lambda: nets.Bottleneck(1024, 256, 1), 7 + i) for i in range(5))).cuda()
    res5 = torch.nn.Sequential(mk(lambda: nets.Bottleneck(1024, 512, 2), 3), mk(lambda: nets.Bottleneck(2048, 512, 1), 4),
                               mk(lambda: nets.Bottleneck(2048, 512, 1), 5)).cuda()
    fpn = mk(lambda: nets.FeaturePyramidNetwork(c5), 2).cuda()
    head = mk(lambda: nets.DBHead(256), 1).cuda().train()
    res4.train()
    res5.train()
    rres4, rres5, rfpn, rhead = copy.deepcopy(res4), copy.deepcopy(res5), copy.deepcopy(fpn), copy.deepcopy(head)
    g = torch.Generator(device="cuda").manual_seed(0)
    feats = [(torch.randn((n, c5 >> (3 - lv), h5 << (3 - lv), w5 << (3 - lv)), generator=g, device="cuda") * 0.5).half() for lv in range(2)]
    padded = [nets.pack_tap(t) for t in feats]
    c4p = nets.forward_res4_padded(res4, padded[1])
    c4f = c4p[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).float().contiguous()
    gp = torch.randn((n, 1, 4 * H, 4 * W), generator=g, device="cuda") * 1e-7
    gt = torch.randn((n, 1, 4 * H, 4 * W), generator=g, device="cuda") * 1e-7

    def zero(*mods):
        for m in mods:
            m.zero_grad(set_to_none=True)

    def hip(deep, **kw):
        def step():
            zero(res4, res5, fpn, head)
            if deep:
                out = fpn.forward_padded(padded, head=head, res5=res5, res4=res4, **kw)
            else:
                out = fpn.forward_padded(padded + [c4p], head=head, res5=res5, **kw)
            torch.autograd.backward([out["probability"], out["threshold"]], [gp, gt])
        return step

    def torch_step(deep):
        def step():
            zero(rres4, rres5, rfpn, rhead)
            x = feats[1].float() if deep else c4f
            c4 = x
            if deep:
                for b in rres4:
                    x = torch_bottleneck_train(b, x)
                c4 = x
            for b in rres5:
                x = torch_bottleneck_train(b, x)
            p2 = wiring(rfpn, [feats[0].float(), feats[1].float(), c4, x])
            torch.autograd.backward([rhead.probability_head(p2), rhead.threshold_head(p2)], [gp, gt])
        return step

    if args.step_only:
        step = hip(True, res_batch_stats=True)
        for _ in range(args.warmup + args.iters):
            step()
        torch.cuda.synchronize()
        print(json.dumps({"batch": n, "batch_res4_steps": args.warmup + args.iters}))
        return
    steps = {"frozen_res4_step_ms": hip(True), "frozen_res5_step_ms": hip(False)}
    if not args.frozen_only:
        steps.update({"batch_res4_step_ms": hip(True, res_batch_stats=True), "batch_res5_step_ms": hip(False, res_batch_stats=True)})
        if not args.no_torch:
            steps.update({"torch_fp32_train_res4_step_ms": torch_step(True), "torch_fp32_train_res5_step_ms": torch_step(False)})
    med, spread = medians(steps, args.iters, args.warmup)
    res = {"batch": n, "c3": [512, 4 * h5, 4 * w5], "c4": [1024, 2 * h5, 2 * w5], "c5": [c5, h5, w5], "iters": args.iters}
    res.update({k: round(v, 3) for k, v in med.items()})
    res["min_max_ms"] = {k: [round(x, 3) for x in v] for k, v in spread.items()}
    if not args.frozen_only:
        zb = z_bytes(n, 4 * h5, 4 * w5)
        for mode in ("res5", "res4"):
            res[f"batch_minus_frozen_{mode}_ms"] = round(med[f"batch_{mode}_step_ms"] - med[f"frozen_{mode}_step_ms"], 3)
            res[f"z_round_trip_bytes_{mode}"] = zb[mode]
            if not args.no_torch:
                res[f"speedup_vs_torch_fp32_train_{mode}"] = round(med[f"torch_fp32_train_{mode}_step_ms"] / med[f"batch_{mode}_step_ms"], 2)
        launches = per_launch(steps["batch_res4_step_ms"], [])
        res["hip_launches"] = len(launches)
        by = {}
        for nm, us in launches:
            by.setdefault(nm, [0, 0.0])
            by[nm][0] += 1
            by[nm][1] += us
        res["hip_by_kernel_us"] = sorted(([nm, c, round(us, 1)] for nm, (c, us) in by.items()), key=lambda r: -r[2])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
