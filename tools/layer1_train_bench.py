"""The layer1 + layer2 + layer3 + layer4 + FPN + DB head training step (forward + backward) at B = 32 on the product shape (pooled stem output
and C2 160 x 160, C3 80 x 80, C4 40 x 40, C5 20 x 20, P2 160 x 160, ResNet-18 channels): the HIP kernels (csrc/resblock_train.hip with the
64-wide block, csrc/fpn_train.hip, csrc/dbhead_train.hip through FeaturePyramidNetwork.forward_padded([pool], head=head, layer4=layer4,
layer3=layer3, layer2=layer2, layer1=layer1)) against the "head+fpn+layer4+layer3+layer2" step of the stage before on a fixed C2
(forward_padded([c2], head=head, layer4=layer4, layer3=layer3, layer2=layer2)), same library, same run, and torch eager autograd of the same
modules (eval-mode BatchNorm in the trunk) in fp32.  The pool tap is a fixed random tensor and the upstream map gradients fixed tensors of
~1e-7, so only the trained stages are timed.  HIP events around `--iters` steps after `--warmup`; per-launch times of one step from
torch.profiler.  Reported on their own: layer1's four weight-gradient launches (MODE 5: 5 q-tiles x slabs workgroups) with their slab count
and grid, its three input-gradient GEMMs (conv2^T twice, conv1^T once: layer1.0 forms no dx), and the block's workspace bytes at this batch.
Prints one JSON line.

    python tools/layer1_train_bench.py [--batch 32] [--iters 10] [--warmup 3] [--no-torch]
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
from layer2_train_bench import slabs128  # noqa: E402
from layer3_train_bench import torch_block  # noqa: E402
from vtd_amd import _native, nets  # noqa: E402


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
    l1 = torch.nn.Sequential(mk(lambda: nets.BasicBlock(64, 64, 1), 9), mk(lambda: nets.BasicBlock(64, 64, 1), 10)).cuda()
    l2 = torch.nn.Sequential(mk(lambda: nets.BasicBlock(64, 128, 2), 7), mk(lambda: nets.BasicBlock(128, 128, 1), 8)).cuda()
    l3 = torch.nn.Sequential(mk(lambda: nets.BasicBlock(128, 256, 2), 5), mk(lambda: nets.BasicBlock(256, 256, 1), 6)).cuda()
    l4 = torch.nn.Sequential(mk(lambda: nets.BasicBlock(256, 512, 2), 3), mk(lambda: nets.BasicBlock(512, 512, 1), 4)).cuda()
    fpn = mk(lambda: nets.FeaturePyramidNetwork(c5), 2).cuda()
    head = mk(lambda: nets.DBHead(256), 1).cuda().train()
    rl1, rl2, rl3, rl4, rfpn, rhead = (copy.deepcopy(m) for m in (l1, l2, l3, l4, fpn, head))
    g = torch.Generator(device="cuda").manual_seed(0)
    pool = (torch.randn((n, 64, H, W), generator=g, device="cuda") * 0.5).abs().half()      # non-negative, as a max-pooled ReLU output
    poolp = nets.pack_tap(pool)
    c2p = nets.forward_layer1_padded(l1, poolp)
    gp = torch.randn((n, 1, 4 * H, 4 * W), generator=g, device="cuda") * 1e-7
    gt = torch.randn((n, 1, 4 * H, 4 * W), generator=g, device="cuda") * 1e-7

    def zero(*mods):
        for m in mods:
            m.zero_grad(set_to_none=True)

    def hip_step():
        zero(l1, l2, l3, l4, fpn, head)
        out = fpn.forward_padded([poolp], head=head, layer4=l4, layer3=l3, layer2=l2, layer1=l1)
        torch.autograd.backward([out["probability"], out["threshold"]], [gp, gt])

    def hip_layer2_step():
        zero(l2, l3, l4, fpn, head)
        out = fpn.forward_padded([c2p], head=head, layer4=l4, layer3=l3, layer2=l2)
        torch.autograd.backward([out["probability"], out["threshold"]], [gp, gt])

    def torch_step():
        zero(rl1, rl2, rl3, rl4, rfpn, rhead)
        c2 = torch_block(rl1[1], torch_block(rl1[0], pool.float()))
        c3 = torch_block(rl2[1], torch_block(rl2[0], c2))
        c4 = torch_block(rl3[1], torch_block(rl3[0], c3))
        p2 = wiring(rfpn, [c2, c3, c4, torch_block(rl4[1], torch_block(rl4[0], c4))])
        torch.autograd.backward([rhead.probability_head(p2), rhead.threshold_head(p2)], [gp, gt])

    lib = _native.require()
    res = {"batch": n, "pool": [64, H, W], "c2": [64, H, W], "c3": [128, 4 * h5, 4 * w5], "c4": [256, 2 * h5, 2 * w5], "c5": [c5, h5, w5]}
    res["layer1_block_workspace_bytes"] = {"forward": int(lib.vtd_block64_train_workspace_bytes(n, H, W, 64, 64, 1, 0)),
                                           "backward": int(lib.vtd_block64_train_workspace_bytes(n, H, W, 64, 64, 1, 1))}
    res["hip_step_ms"] = round(timed(hip_step, args.iters, args.warmup), 3)
    res["hip_layer2_step_ms"] = round(timed(hip_layer2_step, args.iters, args.warmup), 3)
    res["layer1_and_dc2_ms"] = round(res["hip_step_ms"] - res["hip_layer2_step_ms"], 3)
    launches = per_launch(hip_step, [])
    res["hip_per_kernel_us"] = [[nm, round(us, 1)] for nm, us in launches]
    # the backward runs the blocks from layer4.1 down, so the last four weight-gradient launches of the step are layer1's (layer1.1's conv2
    # and conv1, then layer1.0's) and the last three conv_igemm launches its input-gradient GEMMs (csrc/resblock_train.hip: launch_backward)
    rows = n * H * W
    nqt, s = slabs128(rows, 3, 64)
    wg = [us for nm, us in launches if "wgrad_kernel" in nm]
    if len(wg) >= 4:
        res["layer1_wgrad"] = {name: {"us": round(us, 1), "slabs": s, "grid": [nqt * s, 1], "share_of_step": round(us * 1e-3 / res["hip_step_ms"], 4)}
                               for name, us in zip(("layer1.1.conv2", "layer1.1.conv1", "layer1.0.conv2", "layer1.0.conv1"), wg[-4:])}
    dg = [us for nm, us in launches if nm.startswith("conv_igemm")]
    if len(dg) >= 3:
        res["layer1_dgrad"] = {name: {"us": round(us, 1), "share_of_step": round(us * 1e-3 / res["hip_step_ms"], 4)}
                               for name, us in zip(("layer1.1.conv2^T", "layer1.1.conv1^T (dx)", "layer1.0.conv2^T"), dg[-3:])}
    if not args.no_torch:
        res["torch_fp32_step_ms"] = round(timed(torch_step, args.iters, args.warmup), 3)
        res["speedup_vs_torch_fp32"] = round(res["torch_fp32_step_ms"] / res["hip_step_ms"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
