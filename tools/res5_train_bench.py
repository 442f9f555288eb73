"""The res5 + FPN + DB head training step (forward + backward) on ResNet-50's product shape (C4 40 x 40 x 1024, C5 20 x 20 x 2048, P2
160 x 160): the HIP kernels (csrc/bottleneck_train.hip, csrc/fpn_train.hip, csrc/dbhead_train.hip through
FeaturePyramidNetwork.forward_padded(taps, head=head, res5=res5)) against the "head+fpn" step on the same taps (forward_padded(taps,
head=head) with a fixed C5) and torch eager autograd of the same three Bottlenecks (eval-mode BatchNorm) + FPN + head in fp32, on the same
GPU.  The trunk taps are fixed random tensors and the upstream map gradients fixed tensors of ~1e-7, so only the trained stages are timed.
HIP events around `--iters` steps after `--warmup`; per-launch times of one step from torch.profiler.  Prints one JSON line.

    python tools/res5_train_bench.py [--batch 32] [--iters 10] [--warmup 3] [--no-torch]
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

from dbhead_train_bench import per_launch, timed  # noqa: E402
from fpn_train_bench import wiring  # noqa: E402
from vtd_amd import nets  # noqa: E402


def torch_bottleneck(b, x):
    bn = lambda m, t: F.batch_norm(t, m.running_mean, m.running_var, m.weight, m.bias, False, 0.0, m.eps)  # noqa: E731
    a1 = F.relu(bn(b.bn1, F.conv2d(x, b.conv1.weight)))
    a2 = F.relu(bn(b.bn2, F.conv2d(a1, b.conv2.weight, None, b.stride, 1)))
    idt = bn(b.downsample[1], F.conv2d(x, b.downsample[0].weight, None, b.stride)) if hasattr(b, "downsample") else x
    return F.relu(bn(b.bn3, F.conv2d(a2, b.conv3.weight)) + idt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch comparison")
    args = ap.parse_args()
    n, h5, w5, c5 = args.batch, 20, 20, 2048
    H, W = 8 * h5, 8 * w5
    torch.manual_seed(0)
    mk = lambda f, seed: (lambda m: (m.load_state_dict(nets.seeded_state_dict(f, seed)), m)[1])(f())  # noqa: E731
    res5 = torch.nn.Sequential(mk(lambda: nets.Bottleneck(1024, 512, 2), 3), mk(lambda: nets.Bottleneck(2048, 512, 1), 4),
                               mk(lambda: nets.Bottleneck(2048, 512, 1), 5)).cuda()
    fpn = mk(lambda: nets.FeaturePyramidNetwork(c5), 2).cuda()
    head = mk(lambda: nets.DBHead(256), 1).cuda().train()
    rres5, rfpn, rhead = copy.deepcopy(res5), copy.deepcopy(fpn), copy.deepcopy(head)
    g = torch.Generator(device="cuda").manual_seed(0)
    feats = [(torch.randn((n, c5 >> (3 - lv), h5 << (3 - lv), w5 << (3 - lv)), generator=g, device="cuda") * 0.5).half() for lv in range(3)]
    padded = [nets.pack_tap(t) for t in feats]
    c5p = nets.forward_res5_padded(res5, padded[2])
    gp = torch.randn((n, 1, 4 * H, 4 * W), generator=g, device="cuda") * 1e-7
    gt = torch.randn((n, 1, 4 * H, 4 * W), generator=g, device="cuda") * 1e-7

    def zero(*mods):
        for m in mods:
            m.zero_grad(set_to_none=True)

    def hip_step():
        zero(res5, fpn, head)
        out = fpn.forward_padded(padded, head=head, res5=res5)
        torch.autograd.backward([out["probability"], out["threshold"]], [gp, gt])

    def hip_head_fpn_step():
        zero(fpn, head)
        out = fpn.forward_padded(padded + [c5p], head=head)
        torch.autograd.backward([out["probability"], out["threshold"]], [gp, gt])

    def torch_step():
        zero(rres5, rfpn, rhead)
        x = feats[2].float()
        for b in rres5:
            x = torch_bottleneck(b, x)
        p2 = wiring(rfpn, [feats[0].float(), feats[1].float(), feats[2].float(), x])
        torch.autograd.backward([rhead.probability_head(p2), rhead.threshold_head(p2)], [gp, gt])

    def torch_head_fpn_step():
        zero(rfpn, rhead)
        p2 = wiring(rfpn, [feats[0].float(), feats[1].float(), feats[2].float(), c5f])
        torch.autograd.backward([rhead.probability_head(p2), rhead.threshold_head(p2)], [gp, gt])

    res = {"batch": n, "c4": [1024, 2 * h5, 2 * w5], "c5": [c5, h5, w5]}
    res["hip_step_ms"] = round(timed(hip_step, args.iters, args.warmup), 3)
    res["hip_head_fpn_step_ms"] = round(timed(hip_head_fpn_step, args.iters, args.warmup), 3)
    res["res5_ms"] = round(res["hip_step_ms"] - res["hip_head_fpn_step_ms"], 3)
    res["hip_per_kernel_us"] = [[nm, round(us, 1)] for nm, us in per_launch(hip_step, [])]
    if not args.no_torch:
        c5f = c5p[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).float().contiguous()
        res["torch_fp32_step_ms"] = round(timed(torch_step, args.iters, args.warmup), 3)
        res["torch_fp32_head_fpn_step_ms"] = round(timed(torch_head_fpn_step, args.iters, args.warmup), 3)
        res["torch_fp32_res5_ms"] = round(res["torch_fp32_step_ms"] - res["torch_fp32_head_fpn_step_ms"], 3)
        res["speedup_vs_torch_fp32"] = round(res["torch_fp32_step_ms"] / res["hip_step_ms"], 2)
        res["res5_speedup_vs_torch_fp32"] = round(res["torch_fp32_res5_ms"] / max(res["res5_ms"], 1e-9), 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
