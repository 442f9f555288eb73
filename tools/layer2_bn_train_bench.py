"""The layer2 + layer3 + layer4 + FPN + DB head training step (forward + backward) at the product shape of the
"head+fpn+layer4+layer3+layer2" mode (n = 2, a 640 x 640 image: C2 160 x 160, C3 80 x 80, C4 40 x 40, C5 20 x 20, ResNet-18 channels) with the
trunk BatchNorm mode frozen (FeaturePyramidNetwork.forward_padded([C2], head=head, layer4=layer4, layer3=layer3, layer2=layer2):
csrc/resblock_train.hip) and batch (the same call with trunk_batch_stats=("layer2", "layer3", "layer4"): csrc/resblock_bn_train.hip, the
vtd_trunk_bn_train_* entries, the three stages in train() mode, their running statistics updated every step, layer3.0's and layer4.0's input
gradients formed with batch statistics).  The modules, the C2 tap and the upstream map gradients are those of tools/layer2_train_bench.py, so
the frozen figure here is that tool's `hip_step_ms` at the same --batch.  HIP events around `--iters` steps after `--warmup`, `--rounds` times
with the two modes alternating (the median is reported, and every round's time, so the spread is visible), profiler off; per-launch times
of one batch-mode step from torch.profiler, taken afterwards in a pass of its own, with the launch count and the summed time of layer2's
bt_* launches (the kernels of csrc/resblock_bn_train.hip that the frozen path does not have).  Prints one JSON line.

    python tools/layer2_bn_train_bench.py [--batch 2] [--iters 100] [--warmup 10] [--rounds 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "video-text-detection-system_amd"), ROOT, os.path.dirname(os.path.abspath(__file__))]

import torch  # noqa: E402

from dbhead_train_bench import per_launch, timed  # noqa: E402
from vtd_amd import nets  # noqa: E402

STAGES = ("layer2", "layer3", "layer4")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    n, h5, w5, c5 = args.batch, 20, 20, 512
    H, W = 8 * h5, 8 * w5
    torch.manual_seed(0)
    mk = lambda f, seed: (lambda m: (m.load_state_dict(nets.seeded_state_dict(f, seed)), m)[1])(f())  # noqa: E731
    l2 = torch.nn.Sequential(mk(lambda: nets.BasicBlock(64, 128, 2), 7), mk(lambda: nets.BasicBlock(128, 128, 1), 8)).cuda().train()
    l3 = torch.nn.Sequential(mk(lambda: nets.BasicBlock(128, 256, 2), 5), mk(lambda: nets.BasicBlock(256, 256, 1), 6)).cuda().train()
    l4 = torch.nn.Sequential(mk(lambda: nets.BasicBlock(256, 512, 2), 3), mk(lambda: nets.BasicBlock(512, 512, 1), 4)).cuda().train()
    fpn = mk(lambda: nets.FeaturePyramidNetwork(c5), 2).cuda()
    head = mk(lambda: nets.DBHead(256), 1).cuda().train()
    g = torch.Generator(device="cuda").manual_seed(0)
    c2p = nets.pack_tap((torch.randn((n, 64, H, W), generator=g, device="cuda") * 0.5).half())
    gp = torch.randn((n, 1, 4 * H, 4 * W), generator=g, device="cuda") * 1e-7
    gt = torch.randn((n, 1, 4 * H, 4 * W), generator=g, device="cuda") * 1e-7

    def step(batch):
        for m in (l2, l3, l4, fpn, head):
            m.zero_grad(set_to_none=True)
        out = fpn.forward_padded([c2p], head=head, layer4=l4, layer3=l3, layer2=l2, trunk_batch_stats=STAGES if batch else False)
        torch.autograd.backward([out["probability"], out["threshold"]], [gp, gt])

    res = {"batch": n, "c2": [64, H, W], "c3": [128, 4 * h5, 4 * w5], "c4": [256, 2 * h5, 2 * w5], "c5": [c5, h5, w5]}
    rounds = {"frozen": [], "batch": []}
    for _ in range(max(1, args.rounds)):
        rounds["frozen"].append(round(timed(lambda: step(False), args.iters, args.warmup), 3))
        rounds["batch"].append(round(timed(lambda: step(True), args.iters, args.warmup), 3))
    res["iters"], res["rounds_ms"] = args.iters, rounds
    res["frozen_step_ms"], res["batch_step_ms"] = (sorted(v)[len(v) // 2] for v in (rounds["frozen"], rounds["batch"]))
    res["batch_minus_frozen_ms"] = round(res["batch_step_ms"] - res["frozen_step_ms"], 3)
    launches = per_launch(lambda: step(True), [])
    res["batch_per_kernel_us"] = [[nm, round(us, 1)] for nm, us in launches]
    res["launches"] = len(launches)
    # the bt_* launches of a block (csrc/resblock_bn_train.hip): forward, a pack per convolution and {stats partial, stats finish, apply} per
    # pair: 12 with a downsample, 8 without.  Backward, {reduce, finish, form} per pair, a dw per weight gradient, a dgrad pack per
    # transposed convolution and the downsample add: a stride-1 block with dx 10, a stride-2 block with dx 16, without 13.  The forward runs
    # layer2.0 first and the backward layer2.0 last, so layer2's are the step's first 12 + 8 and last 10 + 13
    bt = [(nm, us) for nm, us in launches if nm.startswith("bt_")]
    res["bt_launches"], res["bt_us"] = len(bt), round(sum(us for _, us in bt), 1)
    if len(bt) == 3 * 20 + 2 * 26 + 23:
        mine = bt[:20] + bt[-23:]
        res["layer2_bt_launches"], res["layer2_bt_us"] = len(mine), round(sum(us for _, us in mine), 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
