"""The layer1 + layer2 + layer3 + layer4 + FPN + DB head training step (forward + backward) at the product shape of the
"head+fpn+layer4+layer3+layer2+layer1" mode (n = 2, a 640 x 640 image: the pooled stem output and C2 160 x 160, C3 80 x 80, C4 40 x 40,
C5 20 x 20, ResNet-18 channels) with the trunk BatchNorm mode frozen (FeaturePyramidNetwork.forward_padded([pool], head=head, layer4=layer4,
layer3=layer3, layer2=layer2, layer1=layer1): csrc/resblock_train.hip, layer1 on the vtd_block64_train_* entries) and batch (the same call with
trunk_batch_stats=("layer1", "layer2", "layer3", "layer4"): csrc/resblock_bn_train.hip, all eight blocks on the vtd_trunk_bn_train_* entries,
the four stages in train() mode, their running statistics updated every step, layer2.0's, layer3.0's and layer4.0's input gradients formed
with batch statistics).  The upper stages, the FPN, the head and the upstream map gradients are those of tools/layer2_bn_train_bench.py.  HIP
events around `--iters` steps after `--warmup`, `--rounds` times with the two modes alternating (the median is reported, and every round's
time, so the spread is visible), profiler off; per-launch times of one batch-mode step from torch.profiler, taken afterwards in a pass of its
own (`--no-launches` leaves it out), with the launch count and the summed time of layer1's bt_* launches (the kernels of
csrc/resblock_bn_train.hip that the frozen path does not have).  `--frozen-only` times the frozen mode alone, which a library from before
the 64-wide batch path can run too.  Prints one JSON line.

    python tools/layer1_bn_train_bench.py [--batch 2] [--iters 100] [--warmup 10] [--rounds 3] [--no-launches] [--frozen-only]
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

STAGES = ("layer1", "layer2", "layer3", "layer4")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-launches", action="store_true")
    ap.add_argument("--frozen-only", action="store_true")
    args = ap.parse_args()
    n, h5, w5, c5 = args.batch, 20, 20, 512
    H, W = 8 * h5, 8 * w5
    torch.manual_seed(0)
    mk = lambda f, seed: (lambda m: (m.load_state_dict(nets.seeded_state_dict(f, seed)), m)[1])(f())  # noqa: E731
    l1 = torch.nn.Sequential(mk(lambda: nets.BasicBlock(64, 64, 1), 9), mk(lambda: nets.BasicBlock(64, 64, 1), 10)).cuda().train()
    l2 = torch.nn.Sequential(mk(lambda: nets.BasicBlock(64, 128, 2), 7), mk(lambda: nets.BasicBlock(128, 128, 1), 8)).cuda().train()
    l3 = torch.nn.Sequential(mk(lambda: nets.BasicBlock(128, 256, 2), 5), mk(lambda: nets.BasicBlock(256, 256, 1), 6)).cuda().train()
    l4 = torch.nn.Sequential(mk(lambda: nets.BasicBlock(256, 512, 2), 3), mk(lambda: nets.BasicBlock(512, 512, 1), 4)).cuda().train()
    fpn = mk(lambda: nets.FeaturePyramidNetwork(c5), 2).cuda()
    head = mk(lambda: nets.DBHead(256), 1).cuda().train()
    g = torch.Generator(device="cuda").manual_seed(0)
    # the pooled stem output: a max-pool of ReLU outputs, not negative
    poolp = nets.pack_tap((torch.randn((n, 64, H, W), generator=g, device="cuda") * 0.5).clamp_(min=0).half())
    gp = torch.randn((n, 1, 4 * H, 4 * W), generator=g, device="cuda") * 1e-7
    gt = torch.randn((n, 1, 4 * H, 4 * W), generator=g, device="cuda") * 1e-7

    def step(batch):
        for m in (l1, l2, l3, l4, fpn, head):
            m.zero_grad(set_to_none=True)
        out = fpn.forward_padded([poolp], head=head, layer4=l4, layer3=l3, layer2=l2, layer1=l1, trunk_batch_stats=STAGES if batch else False)
        torch.autograd.backward([out["probability"], out["threshold"]], [gp, gt])

    res = {"batch": n, "pool": [64, H, W], "c2": [64, H, W], "c3": [128, 4 * h5, 4 * w5], "c4": [256, 2 * h5, 2 * w5], "c5": [c5, h5, w5]}
    rounds = {"frozen": []} if args.frozen_only else {"frozen": [], "batch": []}
    for _ in range(max(1, args.rounds)):
        for mode in rounds:
            rounds[mode].append(round(timed(lambda: step(mode == "batch"), args.iters, args.warmup), 3))
    res["iters"], res["rounds_ms"] = args.iters, rounds
    for mode, v in rounds.items():
        res[mode + "_step_ms"] = sorted(v)[len(v) // 2]
    if not args.frozen_only:
        res["batch_minus_frozen_ms"] = round(res["batch_step_ms"] - res["frozen_step_ms"], 3)
    if not args.no_launches and not args.frozen_only:
        launches = per_launch(lambda: step(True), [])
        res["batch_per_kernel_us"] = [[nm, round(us, 1)] for nm, us in launches]
        res["launches"] = len(launches)
        # the bt_* launches of a block (csrc/resblock_bn_train.hip): forward, a pack per convolution and {stats partial, stats finish, apply} per
        # pair: 12 with a downsample, 8 without.  Backward, {reduce, finish, form} per pair, a dw per weight gradient, a dgrad pack per
        # transposed convolution and the downsample add: a stride-1 block with dx 10 and without 9, a stride-2 block with dx 16.  The forward
        # runs layer1 first and the backward layer1 last, so layer1's are the step's first 8 + 8 and last 10 + 9
        bt = [(nm, us) for nm, us in launches if nm.startswith("bt_")]
        res["bt_launches"], res["bt_us"] = len(bt), round(sum(us for _, us in bt), 1)
        if len(bt) == 16 + 3 * 20 + 3 * 26 + 19:
            mine = bt[:16] + bt[-19:]
            res["layer1_bt_launches"], res["layer1_bt_us"] = len(mine), round(sum(us for _, us in mine), 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
