"""The layer3 + layer4 + FPN + DB head training step (forward + backward) at the product shape of the "head+fpn+layer4+layer3" mode (n = 2, a
640 x 640 image: C2 160 x 160, C3 80 x 80, C4 40 x 40, C5 20 x 20, ResNet-18 channels) with the trunk BatchNorm mode frozen
(FeaturePyramidNetwork.forward_padded(taps, head=head, layer4=layer4, layer3=layer3): csrc/resblock_train.hip) and batch (the same call with
trunk_batch_stats=("layer3", "layer4"): csrc/resblock_bn_train.hip, the vtd_block_bn_train_* entries, both stages in train() mode, their
running statistics updated every step, layer4.0's input gradient formed with batch statistics).  The trunk taps are fixed random tensors and the upstream
map gradients fixed tensors of ~1e-7, so only the trained stages are timed.  HIP events around
`--iters` steps after `--warmup`, `--rounds` times with the two modes alternating (the median is reported, and every round's time, so the
spread is visible); per-launch times of one batch-mode step from torch.profiler, taken afterwards.  Prints one JSON line.

    python tools/layer3_bn_train_bench.py [--batch 2] [--iters 200] [--warmup 20] [--rounds 3]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    n, h5, w5, c5 = args.batch, 20, 20, 512
    H, W = 8 * h5, 8 * w5
    torch.manual_seed(0)
    mk = lambda f, seed: (lambda m: (m.load_state_dict(nets.seeded_state_dict(f, seed)), m)[1])(f())  # noqa: E731
    l3 = torch.nn.Sequential(mk(lambda: nets.BasicBlock(128, 256, 2), 5), mk(lambda: nets.BasicBlock(256, 256, 1), 6)).cuda().train()
    l4 = torch.nn.Sequential(mk(lambda: nets.BasicBlock(256, 512, 2), 3), mk(lambda: nets.BasicBlock(512, 512, 1), 4)).cuda().train()
    fpn = mk(lambda: nets.FeaturePyramidNetwork(c5), 2).cuda()
    head = mk(lambda: nets.DBHead(256), 1).cuda().train()
    g = torch.Generator(device="cuda").manual_seed(0)
    feats = [(torch.randn((n, c5 >> (3 - lv), h5 << (3 - lv), w5 << (3 - lv)), generator=g, device="cuda") * 0.5).half() for lv in range(2)]
    padded = [nets.pack_tap(t) for t in feats]
    gp = torch.randn((n, 1, 4 * H, 4 * W), generator=g, device="cuda") * 1e-7
    gt = torch.randn((n, 1, 4 * H, 4 * W), generator=g, device="cuda") * 1e-7

    def step(batch):
        for m in (l3, l4, fpn, head):
            m.zero_grad(set_to_none=True)
        out = fpn.forward_padded(padded, head=head, layer4=l4, layer3=l3, trunk_batch_stats=("layer3", "layer4") if batch else False)
        torch.autograd.backward([out["probability"], out["threshold"]], [gp, gt])

    res = {"batch": n, "c3": [128, 4 * h5, 4 * w5], "c4": [256, 2 * h5, 2 * w5], "c5": [c5, h5, w5]}
    rounds = {"frozen": [], "batch": []}
    for _ in range(max(1, args.rounds)):
        rounds["frozen"].append(round(timed(lambda: step(False), args.iters, args.warmup), 3))
        rounds["batch"].append(round(timed(lambda: step(True), args.iters, args.warmup), 3))
    res["iters"], res["rounds_ms"] = args.iters, rounds
    res["frozen_step_ms"], res["batch_step_ms"] = (sorted(v)[len(v) // 2] for v in (rounds["frozen"], rounds["batch"]))
    res["batch_minus_frozen_ms"] = round(res["batch_step_ms"] - res["frozen_step_ms"], 3)
    res["batch_per_kernel_us"] = [[nm, round(us, 1)] for nm, us in per_launch(lambda: step(True), [])]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
