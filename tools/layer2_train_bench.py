"""The layer2 + layer3 + layer4 + FPN + DB head training step (forward + backward) at B = 32 on the product shape (C2 160 x 160, C3 80 x 80,
C4 40 x 40, C5 20 x 20, P2 160 x 160, ResNet-18 channels): the HIP kernels (csrc/resblock_train.hip with the 128-wide blocks and the
64-channel weight gradients, csrc/fpn_train.hip, csrc/dbhead_train.hip through FeaturePyramidNetwork.forward_padded(taps, head=head,
layer4=layer4, layer3=layer3, layer2=layer2)) against the "head+fpn+layer4+layer3" step of the stage before on the same C2 and a fixed C3
(forward_padded(taps, head=head, layer4=layer4, layer3=layer3)) and torch eager autograd of the same layer2 + layer3 + layer4 (eval-mode
BatchNorm) + FPN + head in fp32.  The C2 tap is a fixed random tensor and the upstream map gradients fixed tensors of ~1e-7, so only the
trained stages are timed.  HIP events around `--iters` steps after `--warmup`; per-launch times of one step from torch.profiler.  Reported
on their own: the four weight-gradient launches of a 128-wide block that the slab rule is judged by (layer2.0's conv2, downsample and
conv1, layer2.1's conv2) with their slab counts and grids, and the GEMM of layer3.0's strided input gradient (the zero-inserted plane
through the stride-1 3x3 path: 4x the multiply-adds of a phase-split form).  Prints one JSON line.

    python tools/layer2_train_bench.py [--batch 32] [--iters 10] [--warmup 3] [--no-torch]
"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "video-text-detection-system_amd"), ROOT, os.path.dirname(os.path.abspath(__file__))]

import torch  # noqa: E402

from dbhead_train_bench import per_launch, timed  # noqa: E402
from fpn_train_bench import wiring  # noqa: E402
from layer3_train_bench import torch_block  # noqa: E402
from vtd_amd import nets  # noqa: E402


def slabs128(rows, ksz, xc):
    """csrc/resblock_train.hip's rule for a 128-wide block: (q-tiles, slabs) of one weight-gradient launch."""
    nqt = (ksz * ksz * xc + 127) // 128
    return nqt, min((512 + nqt - 1) // nqt, (rows + 1023) // 1024)


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
    l2 = torch.nn.Sequential(mk(lambda: nets.BasicBlock(64, 128, 2), 7), mk(lambda: nets.BasicBlock(128, 128, 1), 8)).cuda()
    l3 = torch.nn.Sequential(mk(lambda: nets.BasicBlock(128, 256, 2), 5), mk(lambda: nets.BasicBlock(256, 256, 1), 6)).cuda()
    l4 = torch.nn.Sequential(mk(lambda: nets.BasicBlock(256, 512, 2), 3), mk(lambda: nets.BasicBlock(512, 512, 1), 4)).cuda()
    fpn = mk(lambda: nets.FeaturePyramidNetwork(c5), 2).cuda()
    head = mk(lambda: nets.DBHead(256), 1).cuda().train()
    rl2, rl3, rl4, rfpn, rhead = (copy.deepcopy(m) for m in (l2, l3, l4, fpn, head))
    g = torch.Generator(device="cuda").manual_seed(0)
    c2 = (torch.randn((n, 64, H, W), generator=g, device="cuda") * 0.5).half()
    c2p = nets.pack_tap(c2)
    c3p = nets.forward_layer2_padded(l2, c2p)
    gp = torch.randn((n, 1, 4 * H, 4 * W), generator=g, device="cuda") * 1e-7
    gt = torch.randn((n, 1, 4 * H, 4 * W), generator=g, device="cuda") * 1e-7

    def zero(*mods):
        for m in mods:
            m.zero_grad(set_to_none=True)

    def hip_step():
        zero(l2, l3, l4, fpn, head)
        out = fpn.forward_padded([c2p], head=head, layer4=l4, layer3=l3, layer2=l2)
        torch.autograd.backward([out["probability"], out["threshold"]], [gp, gt])

    def hip_layer3_step():
        zero(l3, l4, fpn, head)
        out = fpn.forward_padded([c2p, c3p], head=head, layer4=l4, layer3=l3)
        torch.autograd.backward([out["probability"], out["threshold"]], [gp, gt])

    def torch_step():
        zero(rl2, rl3, rl4, rfpn, rhead)
        c3 = torch_block(rl2[1], torch_block(rl2[0], c2.float()))
        c4 = torch_block(rl3[1], torch_block(rl3[0], c3))
        p2 = wiring(rfpn, [c2.float(), c3, c4, torch_block(rl4[1], torch_block(rl4[0], c4))])
        torch.autograd.backward([rhead.probability_head(p2), rhead.threshold_head(p2)], [gp, gt])

    res = {"batch": n, "c2": [64, H, W], "c3": [128, 4 * h5, 4 * w5], "c4": [256, 2 * h5, 2 * w5], "c5": [c5, h5, w5]}
    res["hip_step_ms"] = round(timed(hip_step, args.iters, args.warmup), 3)
    res["hip_layer3_step_ms"] = round(timed(hip_layer3_step, args.iters, args.warmup), 3)
    res["layer2_and_dc3_ms"] = round(res["hip_step_ms"] - res["hip_layer3_step_ms"], 3)
    launches = per_launch(hip_step, [])
    res["hip_per_kernel_us"] = [[nm, round(us, 1)] for nm, us in launches]
    # the backward runs the blocks from layer4.1 down, so the last seven weight-gradient launches of the step are layer2's: layer2.1's conv2
    # and conv1, then layer2.0's conv2, downsample and conv1 (csrc/resblock_train.hip: launch_backward)
    rows = n * 4 * h5 * 4 * w5
    wg = [(i, us) for i, (nm, us) in enumerate(launches) if "wgrad_kernel" in nm]
    if len(wg) >= 5:
        names = ("layer2.1.conv2", "layer2.1.conv1", "layer2.0.conv2", "layer2.0.downsample", "layer2.0.conv1")
        shapes = ((3, 128), (3, 128), (3, 128), (1, 64), (3, 64))
        res["layer2_wgrad"] = {}
        for name, (ksz, xc), (_, us) in zip(names, shapes, wg[-5:]):
            nqt, s = slabs128(rows, ksz, xc)
            res["layer2_wgrad"][name] = {"us": round(us, 1), "slabs": s, "grid": [nqt * s, 1], "share_of_step": round(us * 1e-3 / res["hip_step_ms"], 4)}
    # layer3.0's strided input gradient: the rb_add_downsample_kernel launches of the step are layer4.0's, then layer3.0's (layer2.0 forms
    # none); the second conv_igemm launch before the latter is the GEMM over the zero-inserted plane (M = n 80 80 rows, K = 9 * 256, 128 columns)
    flop = 2.0 * n * 16 * h5 * w5 * 128 * 2304
    res["gflop"] = {"layer3_strided_dgrad_zero_inserted": round(flop / 1e9, 1), "layer3_strided_dgrad_phase_split": round(flop / 4e9, 1)}
    adds = [i for i, (nm, _) in enumerate(launches) if nm.startswith("rb_add_downsample_kernel")]
    if len(adds) == 2:
        convs = [i for i in range(adds[1]) if launches[i][0].startswith("conv_igemm")]
        if len(convs) >= 2:
            us = launches[convs[-2]][1]
            res["layer3_strided_dgrad_gemm_us"] = round(us, 1)
            res["layer3_strided_dgrad_gemm_share_of_step"] = round(us * 1e-3 / res["hip_step_ms"], 4)
    if not args.no_torch:
        res["torch_fp32_step_ms"] = round(timed(torch_step, args.iters, args.warmup), 3)
        res["speedup_vs_torch_fp32"] = round(res["torch_fp32_step_ms"] / res["hip_step_ms"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
