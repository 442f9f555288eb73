"""The stem's training step (forward + backward) at the product shape (n = 2, a 640 x 640 image: the conv map 320 x 320, the pooled map
160 x 160) with the stem's BatchNorm frozen (nets.stem_train: csrc/stem_train.hip behind vtd_stem_train_*, one fused forward launch, the conv
map never in HBM) and batch (nets.stem_bn_train: vtd_stem_bn_train_* with the BatchNorm in train() mode -- the conv map z [204 800][64] fp32
goes through HBM once per direction, the statistics, the running update and the full BatchNorm backward run).  The stem frozen under four
batch stages has no public spelling (forward_padded refuses it), so the two modes time the stem's own forward and backward; the whole
stem -> layer1 -> .. -> layer4 -> FPN -> head node with stem_batch_stats=True is timed beside them as `node_batch_step_ms`, on the stages, FPN,
head and upstream map gradients of tools/layer1_bn_train_bench.py, whose batch figure is that node without the stem.  HIP events around
`--iters` steps after `--warmup`, `--rounds` times with the two modes alternating (the median is reported, and every round's time, so the
spread is visible), profiler off; per-launch times of one batch-mode stem step from torch.profiler, taken afterwards in a pass of its own
(`--no-launches` leaves it out), with the summed time of the launches the frozen path does not have and the bytes of z per step.
`--frozen-only` times the frozen mode alone, which a library from before the batch path can run too.  Prints one JSON line.

    python tools/stem_bn_train_bench.py [--batch 2] [--iters 100] [--warmup 10] [--rounds 3] [--no-launches] [--frozen-only] [--no-node]
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
# the launches of a batch-mode stem step that the frozen path does not have: the raw-weight pack, the z-writing forward, the statistics, the
# pool pass, and the backward's reduce, finish, form and dW (the weight-gradient kernel itself is shared)
NEW = ("sb_", "stem_train_forward_kernel<true>")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-launches", action="store_true")
    ap.add_argument("--frozen-only", action="store_true")
    ap.add_argument("--no-node", action="store_true")
    args = ap.parse_args()
    n, h5, w5, c5 = args.batch, 20, 20, 512
    H, W = 32 * h5, 32 * w5
    torch.manual_seed(0)
    mk = lambda f, seed: (lambda m: (m.load_state_dict(nets.seeded_state_dict(f, seed)), m)[1])(f())  # noqa: E731
    stem = mk(lambda: torch.nn.Sequential(*nets.make_trunk("resnet18")[:2]), 11).cuda()
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((n, 3, H, W), generator=g, device="cuda")
    up = torch.randn((n, 64, H // 4, W // 4), generator=g, device="cuda") * 1e-4

    def step(batch):
        stem.zero_grad(set_to_none=True)
        stem.train(batch)
        (nets.stem_bn_train if batch else nets.stem_train)(stem[0], stem[1], x).backward(up)

    res = {"batch": n, "image": [3, H, W], "conv": [64, H // 2, W // 2], "pool": [64, H // 4, W // 4]}
    rounds = {"frozen": []} if args.frozen_only else {"frozen": [], "batch": []}
    for _ in range(max(1, args.rounds)):
        for mode in rounds:
            rounds[mode].append(round(timed(lambda: step(mode == "batch"), args.iters, args.warmup), 3))
    res["iters"], res["rounds_ms"] = args.iters, rounds
    for mode, v in rounds.items():
        res["stem_" + mode + "_step_ms"] = sorted(v)[len(v) // 2]
    if args.frozen_only:
        print(json.dumps(res))
        return
    res["batch_minus_frozen_ms"] = round(res["stem_batch_step_ms"] - res["stem_frozen_step_ms"], 3)
    res["z_bytes"] = n * (H // 2) * (W // 2) * 64 * 4
    if not args.no_node:
        l1 = torch.nn.Sequential(mk(lambda: nets.BasicBlock(64, 64, 1), 9), mk(lambda: nets.BasicBlock(64, 64, 1), 10)).cuda().train()
        l2 = torch.nn.Sequential(mk(lambda: nets.BasicBlock(64, 128, 2), 7), mk(lambda: nets.BasicBlock(128, 128, 1), 8)).cuda().train()
        l3 = torch.nn.Sequential(mk(lambda: nets.BasicBlock(128, 256, 2), 5), mk(lambda: nets.BasicBlock(256, 256, 1), 6)).cuda().train()
        l4 = torch.nn.Sequential(mk(lambda: nets.BasicBlock(256, 512, 2), 3), mk(lambda: nets.BasicBlock(512, 512, 1), 4)).cuda().train()
        fpn = mk(lambda: nets.FeaturePyramidNetwork(c5), 2).cuda()
        head = mk(lambda: nets.DBHead(256), 1).cuda().train()
        gp = torch.randn((n, 1, H, W), generator=g, device="cuda") * 1e-7
        gt = torch.randn((n, 1, H, W), generator=g, device="cuda") * 1e-7
        image = nets.pack_image(x)
        stem.train()

        def node():
            for m in (stem, l1, l2, l3, l4, fpn, head):
                m.zero_grad(set_to_none=True)
            out = fpn.forward_padded([image], head=head, layer4=l4, layer3=l3, layer2=l2, layer1=l1, stem=(stem[0], stem[1]), trunk_batch_stats=STAGES,
                                     stem_batch_stats=True)
            torch.autograd.backward([out["probability"], out["threshold"]], [gp, gt])

        v = [round(timed(node, args.iters, args.warmup), 3) for _ in range(max(1, args.rounds))]
        res["node_rounds_ms"], res["node_batch_step_ms"] = v, sorted(v)[len(v) // 2]
    if not args.no_launches:
        launches = per_launch(lambda: step(True), [])
        res["batch_per_kernel_us"] = [[nm, round(us, 1)] for nm, us in launches]
        res["launches"] = len(launches)
        new = [(nm, us) for nm, us in launches if nm.startswith(NEW)]
        res["new_launches"], res["new_us"] = len(new), round(sum(us for _, us in new), 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
