"""The whole ResNet-50 detector's training step (forward + backward) on the product shape (a 640 x 640 image, pooled 160 x 160 x 64, C2 160 x
160 x 256 .. C5 20 x 20 x 2048, P2 160 x 160), in the three deepest modes: the HIP kernels through
FeaturePyramidNetwork.forward_padded([C2], head=, res5=, res4=, res3=) (the "head+fpn+res5+res4+res3" step, on the C2 that res2 gives),
forward_padded([pool], ..., res2=) (the "...+res2" step, on the pooled tap the stem gives) and forward_padded([image], ..., res2=, stem=)
(the "...+res2+stem" step, on the packed image), so that what res2 and the stem add are differences of this tool's own numbers; and torch
eager autograd of the same sixteen Bottlenecks (eval-mode BatchNorm), stem, FPN and head in fp32 with the same tensors trainable, on the same
GPU.  The image is a fixed random tensor and the upstream map gradients fixed tensors of ~1e-7, so only the trained stages are timed.  Every
call is timed on its own with HIP events after `--warmup` calls of each variant, the variants alternating; the figure of a variant is the
median of its `--iters` calls.  Per-launch times of the whole-detector step come from torch.profiler in a pass of their own after the
timing.  Prints one JSON line.

    python tools/res2_train_bench.py [--batch 32] [--iters 15] [--warmup 3] [--no-torch]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/res2_train_bench.py --step-only --iters 5

`--step-only` runs the HIP whole-detector step alone, `--warmup` + `--iters` times, and prints nothing but the count: for a profiler run of
its own, whose per-kernel totals then belong to this step and nothing else.
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
from res5_train_bench import torch_bottleneck  # noqa: E402
from vtd_amd import nets  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch comparison")
    ap.add_argument("--step-only", action="store_true", help="run the HIP whole-detector step alone (for a profiler run of its own)")
    args = ap.parse_args()
    n, h5, w5, c5 = args.batch, 20, 20, 2048
    H, W = 8 * h5, 8 * w5
    torch.manual_seed(0)
    mk = lambda f, seed: (lambda m: (m.load_state_dict(nets.seeded_state_dict(f, seed)), m)[1])(f())  # noqa: E731
    trunk = mk(lambda: nets.make_trunk("resnet50"), 5).cuda()
    stem, (res2, res3, res4, res5) = (trunk[0], trunk[1]), trunk[4:8]
    fpn = mk(lambda: nets.FeaturePyramidNetwork(c5), 2).cuda()
    head = mk(lambda: nets.DBHead(256), 1).cuda().train()
    rtrunk, rfpn, rhead = (copy.deepcopy(m) for m in (trunk, fpn, head))
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((n, 3, 4 * H, 4 * W), generator=g, device="cuda")
    image = nets.pack_image(x)
    poolp = nets.forward_stem_padded(stem[0], stem[1], image)
    c2p = nets.forward_res2_padded(res2, poolp)
    unpad = lambda t: t[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).float().contiguous()  # noqa: E731
    poolf, c2f = unpad(poolp), unpad(c2p)
    gp = torch.randn((n, 1, 4 * H, 4 * W), generator=g, device="cuda") * 1e-7
    gt = torch.randn((n, 1, 4 * H, 4 * W), generator=g, device="cuda") * 1e-7
    upper = {"head": head, "res5": res5, "res4": res4, "res3": res3}

    def hip(taps, **lower):
        for m in (trunk, fpn, head):
            m.zero_grad(set_to_none=True)
        out = fpn.forward_padded(taps, **upper, **lower)
        torch.autograd.backward([out["probability"], out["threshold"]], [gp, gt])

    def torch_from(t, first):
        """Eager fp32 from the input of stage `first` (4 .. 7: res2 .. res5) on; the stages below it are not part of the graph."""
        for m in (rtrunk, rfpn, rhead):
            m.zero_grad(set_to_none=True)
        taps = [t] if first == 5 else []
        for i in range(first, 8):
            for b in rtrunk[i]:
                t = torch_bottleneck(b, t)
            taps.append(t)
        p2 = wiring(rfpn, taps)
        torch.autograd.backward([rhead.probability_head(p2), rhead.threshold_head(p2)], [gp, gt])

    def torch_whole():
        conv, bn = rtrunk[0], rtrunk[1]
        z = F.relu(F.batch_norm(F.conv2d(x, conv.weight, None, 2, 3), bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps))
        torch_from(F.max_pool2d(z, 3, 2, 1), 4)

    hip_whole = lambda: hip([image], res2=res2, stem=stem)  # noqa: E731
    if args.step_only:
        for _ in range(args.warmup + args.iters):
            hip_whole()
        torch.cuda.synchronize()
        print(json.dumps({"batch": n, "hip_steps": args.warmup + args.iters}))
        return
    steps = {"hip_res3_step_ms": lambda: hip([c2p]), "hip_res2_step_ms": lambda: hip([poolp], res2=res2), "hip_whole_step_ms": hip_whole}
    if not args.no_torch:
        steps.update({"torch_fp32_res3_step_ms": lambda: torch_from(c2f, 5), "torch_fp32_res2_step_ms": lambda: torch_from(poolf, 4),
                      "torch_fp32_whole_step_ms": torch_whole})
    med, spread = medians(steps, args.iters, args.warmup)
    res = {"batch": n, "image": [3, 4 * H, 4 * W], "pool": [64, H, W], "c2": [256, H, W], "c5": [c5, h5, w5], "iters": args.iters}
    res.update({k: round(v, 3) for k, v in med.items()})
    res["min_max_ms"] = {k: [round(v, 3) for v in vs] for k, vs in spread.items()}
    res["res2_ms"] = round(med["hip_res2_step_ms"] - med["hip_res3_step_ms"], 3)
    res["stem_ms"] = round(med["hip_whole_step_ms"] - med["hip_res2_step_ms"], 3)
    if not args.no_torch:
        res["torch_fp32_res2_ms"] = round(med["torch_fp32_res2_step_ms"] - med["torch_fp32_res3_step_ms"], 3)
        res["torch_fp32_stem_ms"] = round(med["torch_fp32_whole_step_ms"] - med["torch_fp32_res2_step_ms"], 3)
        for k in ("res3", "res2", "whole"):
            res[f"{k}_speedup_vs_torch_fp32"] = round(med[f"torch_fp32_{k}_step_ms"] / med[f"hip_{k}_step_ms"], 2)
        res["res2_share_speedup_vs_torch_fp32"] = round(res["torch_fp32_res2_ms"] / max(res["res2_ms"], 1e-9), 2)
    launches = per_launch(hip_whole, [])
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
