"""The layer3 + layer4 + FPN + DB head training step (forward + backward) at B = 32 on the product shape (C3 80 x 80, C4 40 x 40, C5 20 x 20,
P2 160 x 160, ResNet-18 channels): the HIP kernels (csrc/resblock_train.hip with the strided input gradient, csrc/fpn_train.hip,
csrc/dbhead_train.hip through FeaturePyramidNetwork.forward_padded(taps, head=head, layer4=layer4, layer3=layer3)) against the
"head+fpn+layer4" step of the stage before on the same C2, C3 and a fixed C4 (forward_padded(taps, head=head, layer4=layer4)) and torch
eager autograd of the same layer3 + layer4 (eval-mode BatchNorm) + FPN + head in fp32.  The trunk taps are fixed random tensors and the
upstream map gradients fixed tensors of ~1e-7, so only the trained stages are timed.  HIP events around `--iters` steps after `--warmup`;
per-launch times of one step from torch.profiler; the time of layer4.0's strided input gradient (the zero-inserted plane through the
stride-1 3x3 path: 4x the multiply-adds of a phase-split form) is reported on its own.  Prints one JSON line.

    python tools/layer3_train_bench.py [--batch 32] [--iters 10] [--warmup 3] [--no-torch]
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


def torch_block(b, x):
    bn = lambda m, t: F.batch_norm(t, m.running_mean, m.running_var, m.weight, m.bias, False, 0.0, m.eps)  # noqa: E731
    a1 = F.relu(bn(b.bn1, F.conv2d(x, b.conv1.weight, None, b.stride, 1)))
    idt = bn(b.downsample[1], F.conv2d(x, b.downsample[0].weight, None, b.stride)) if hasattr(b, "downsample") else x
    return F.relu(bn(b.bn2, F.conv2d(a1, b.conv2.weight, None, 1, 1)) + idt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch comparison")
    args = ap.parse_args()
    n, h5, w5, c5 = args.batch, 20, 20, 512
    H, W = 8 * h5, 8 * w5
    torch.manual_seed(0)
    mk = lambda f, seed: (lambda m: (m.load_state_dict(nets.seeded_state_dict(f, seed)), m)[1])(f())  # noqa: E731
    l3 = torch.nn.Sequential(mk(lambda: nets.BasicBlock(128, 256, 2), 5), mk(lambda: nets.BasicBlock(256, 256, 1), 6)).cuda()
    l4 = torch.nn.Sequential(mk(lambda: nets.BasicBlock(256, 512, 2), 3), mk(lambda: nets.BasicBlock(512, 512, 1), 4)).cuda()
    fpn = mk(lambda: nets.FeaturePyramidNetwork(c5), 2).cuda()
    head = mk(lambda: nets.DBHead(256), 1).cuda().train()
    rl3, rl4, rfpn, rhead = copy.deepcopy(l3), copy.deepcopy(l4), copy.deepcopy(fpn), copy.deepcopy(head)
    g = torch.Generator(device="cuda").manual_seed(0)
    feats = [(torch.randn((n, c5 >> (3 - lv), h5 << (3 - lv), w5 << (3 - lv)), generator=g, device="cuda") * 0.5).half() for lv in range(2)]
    padded = [nets.pack_tap(t) for t in feats]
    c4p = nets.forward_layer3_padded(l3, padded[1])
    gp = torch.randn((n, 1, 4 * H, 4 * W), generator=g, device="cuda") * 1e-7
    gt = torch.randn((n, 1, 4 * H, 4 * W), generator=g, device="cuda") * 1e-7

    def zero(*mods):
        for m in mods:
            m.zero_grad(set_to_none=True)

    def hip_step():
        zero(l3, l4, fpn, head)
        out = fpn.forward_padded(padded, head=head, layer4=l4, layer3=l3)
        torch.autograd.backward([out["probability"], out["threshold"]], [gp, gt])

    def hip_layer4_step():
        zero(l4, fpn, head)
        out = fpn.forward_padded(padded + [c4p], head=head, layer4=l4)
        torch.autograd.backward([out["probability"], out["threshold"]], [gp, gt])

    def torch_step():
        zero(rl3, rl4, rfpn, rhead)
        c4 = torch_block(rl3[1], torch_block(rl3[0], feats[1].float()))
        p2 = wiring(rfpn, [feats[0].float(), feats[1].float(), c4, torch_block(rl4[1], torch_block(rl4[0], c4))])
        torch.autograd.backward([rhead.probability_head(p2), rhead.threshold_head(p2)], [gp, gt])

    res = {"batch": n, "c3": [128, 4 * h5, 4 * w5], "c4": [256, 2 * h5, 2 * w5], "c5": [c5, h5, w5]}
    res["hip_step_ms"] = round(timed(hip_step, args.iters, args.warmup), 3)
    res["hip_layer4_step_ms"] = round(timed(hip_layer4_step, args.iters, args.warmup), 3)
    res["layer3_and_dc4_ms"] = round(res["hip_step_ms"] - res["hip_layer4_step_ms"], 3)
    launches = per_launch(hip_step, [])
    res["hip_per_kernel_us"] = [[nm, round(us, 1)] for nm, us in launches]
    # layer4.0's strided input gradient: the step has one rb_add_downsample_kernel launch (layer3.0 forms no input gradient); the second
    # conv_igemm launch before it is the GEMM over the zero-inserted plane (M = n 40 40 rows, K = 9 * 512, 256 columns)
    flop = 2.0 * n * 4 * h5 * w5 * 256 * 4608
    res["gflop"] = {"strided_dgrad_zero_inserted": round(flop / 1e9, 1), "strided_dgrad_phase_split": round(flop / 4e9, 1)}
    adds = [i for i, (nm, _) in enumerate(launches) if nm.startswith("rb_add_downsample_kernel")]
    if len(adds) == 1:
        convs = [i for i in range(adds[0]) if launches[i][0].startswith("conv_igemm")]
        if len(convs) >= 2:
            us = launches[convs[-2]][1]
            res["strided_dgrad_gemm_us"] = round(us, 1)
            res["strided_dgrad_gemm_tflops_zero_inserted"] = round(flop / (us * 1e-6) / 1e12, 1)
    if not args.no_torch:
        res["torch_fp32_step_ms"] = round(timed(torch_step, args.iters, args.warmup), 3)
        res["speedup_vs_torch_fp32"] = round(res["torch_fp32_step_ms"] / res["hip_step_ms"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
