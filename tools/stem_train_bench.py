"""The whole-detector training step (forward + backward) at B = 32 on the product shape (image 640 x 640, pooled stem output and C2 160 x 160,
C3 80 x 80, C4 40 x 40, C5 20 x 20, ResNet-18 channels): the HIP kernels with the stem (csrc/stem_train.hip) in front, through
FeaturePyramidNetwork.forward_padded([image], head=head, layer4=.., layer3=.., layer2=.., layer1=.., stem=(conv, bn)), against the layer1-mode
step of the stage before on the pooled tap the stem produced (forward_padded([pool], ..., layer1=layer1): same library, same run; it is
tools/layer1_train_bench.py's hip_step, so that tool on an earlier commit gives that commit's figure of the same step), and torch eager
autograd of the same modules
(eval-mode BatchNorm in the trunk) in fp32.  The image is a fixed random tensor and the upstream map gradients fixed tensors of ~1e-7.
HIP events around `--iters` steps after `--warmup`; per-launch times of one step from torch.profiler.  Reported on their own: the stem's
forward launches (fold, ring, forward) and backward launches (reduce, finish, form, weight gradient, param) with the weight gradient's slab
count, the bytes each side must move and the time that floor takes at `--hbm-tbs`, and the stem's workspace bytes at this batch.
Prints one JSON line.

    python tools/stem_train_bench.py [--batch 32] [--iters 10] [--warmup 3] [--no-torch]
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
from layer3_train_bench import torch_block  # noqa: E402
from vtd_amd import _native, nets  # noqa: E402

FWD_KERNELS = ("st_fold_kernel", "st_zero_ring_kernel", "stem_train_forward_kernel")
BWD_KERNELS = ("st_reduce_kernel", "st_finish_kernel", "st_form_kernel", "stem_train_wgrad_kernel", "st_param_kernel")


def torch_stem(conv, bn, x):
    return F.max_pool2d(F.relu(F.batch_norm(conv(x), bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)), 3, 2, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch comparison")
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM bandwidth for the bytes-moved floor, TB/s")
    args = ap.parse_args()
    n, h5, w5, c5 = args.batch, 20, 20, 512
    H, W = 8 * h5, 8 * w5
    torch.manual_seed(0)
    mk = lambda f, seed: (lambda m: (m.load_state_dict(nets.seeded_state_dict(f, seed)), m)[1])(f())  # noqa: E731
    stem = mk(lambda: torch.nn.Sequential(*nets.make_trunk("resnet18")[:2]), 11).cuda()
    l1 = torch.nn.Sequential(mk(lambda: nets.BasicBlock(64, 64, 1), 9), mk(lambda: nets.BasicBlock(64, 64, 1), 10)).cuda()
    l2 = torch.nn.Sequential(mk(lambda: nets.BasicBlock(64, 128, 2), 7), mk(lambda: nets.BasicBlock(128, 128, 1), 8)).cuda()
    l3 = torch.nn.Sequential(mk(lambda: nets.BasicBlock(128, 256, 2), 5), mk(lambda: nets.BasicBlock(256, 256, 1), 6)).cuda()
    l4 = torch.nn.Sequential(mk(lambda: nets.BasicBlock(256, 512, 2), 3), mk(lambda: nets.BasicBlock(512, 512, 1), 4)).cuda()
    fpn = mk(lambda: nets.FeaturePyramidNetwork(c5), 2).cuda()
    head = mk(lambda: nets.DBHead(256), 1).cuda().train()
    rstem, rl1, rl2, rl3, rl4, rfpn, rhead = (copy.deepcopy(m) for m in (stem, l1, l2, l3, l4, fpn, head))
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((n, 3, 4 * H, 4 * W), generator=g, device="cuda")
    poolp = nets.forward_stem_padded(stem[0], stem[1], nets.pack_image(x))
    gp = torch.randn((n, 1, 4 * H, 4 * W), generator=g, device="cuda") * 1e-7
    gt = torch.randn((n, 1, 4 * H, 4 * W), generator=g, device="cuda") * 1e-7

    def zero(*mods):
        for m in mods:
            m.zero_grad(set_to_none=True)

    def hip_step():      # the image is packed inside the step, as the product's train-mode forward does
        zero(stem, l1, l2, l3, l4, fpn, head)
        out = fpn.forward_padded([nets.pack_image(x)], head=head, layer4=l4, layer3=l3, layer2=l2, layer1=l1, stem=(stem[0], stem[1]))
        torch.autograd.backward([out["probability"], out["threshold"]], [gp, gt])

    def hip_layer1_step():
        zero(l1, l2, l3, l4, fpn, head)
        out = fpn.forward_padded([poolp], head=head, layer4=l4, layer3=l3, layer2=l2, layer1=l1)
        torch.autograd.backward([out["probability"], out["threshold"]], [gp, gt])

    def torch_step():
        zero(rstem, rl1, rl2, rl3, rl4, rfpn, rhead)
        c2 = torch_block(rl1[1], torch_block(rl1[0], torch_stem(rstem[0], rstem[1], x)))
        c3 = torch_block(rl2[1], torch_block(rl2[0], c2))
        c4 = torch_block(rl3[1], torch_block(rl3[0], c3))
        p2 = wiring(rfpn, [c2, c3, c4, torch_block(rl4[1], torch_block(rl4[0], c4))])
        torch.autograd.backward([rhead.probability_head(p2), rhead.threshold_head(p2)], [gp, gt])

    res = {"batch": n, "image": [3, 4 * H, 4 * W], "pool": [64, H, W]}
    res["hip_layer1_step_ms"] = round(timed(hip_layer1_step, args.iters, args.warmup), 3)
    lib = _native.require()
    res["stem_workspace_bytes"] = {"forward": int(lib.vtd_stem_train_workspace_bytes(n, 4 * H, 4 * W, 0)),
                                   "backward": int(lib.vtd_stem_train_workspace_bytes(n, 4 * H, 4 * W, 1))}
    res["hip_step_ms"] = round(timed(hip_step, args.iters, args.warmup), 3)
    res["stem_and_layer1_dx_ms"] = round(res["hip_step_ms"] - res["hip_layer1_step_ms"], 3)
    launches = per_launch(hip_step, [])
    res["hip_per_kernel_us"] = [[nm, round(us, 1)] for nm, us in launches]
    pick = lambda names: {k: round(sum(us for nm, us in launches if nm.startswith(k)), 1) for k in names}  # noqa: E731
    fwd, bwd = pick(FWD_KERNELS), pick(BWD_KERNELS)
    rows = n * 2 * H * 2 * W
    slabs = max(1, min(512, (rows + 1023) // 1024))
    pooled = n * H * W * 64
    # forward: the image tap in, the pooled tap and the indices out.  backward: dpool (twice: the sums, then the gather), the pooled tap
    # (twice) and the indices in, dZ out and in again, the image tap in
    image_bytes = n * (4 * H + 6) * (4 * W + 6) * 8
    fwd_bytes = image_bytes + pooled * 2 + pooled
    bwd_bytes = 2 * pooled * 4 + 2 * pooled * 2 + pooled + 2 * rows * 64 * 2 + image_bytes
    res["stem_forward"] = {"us": fwd, "total_us": round(sum(fwd.values()), 1), "bytes": fwd_bytes,
                           "floor_us": round(fwd_bytes / (args.hbm_tbs * 1e6), 1)}
    res["stem_backward"] = {"us": bwd, "total_us": round(sum(bwd.values()), 1), "bytes": bwd_bytes,
                            "floor_us": round(bwd_bytes / (args.hbm_tbs * 1e6), 1), "wgrad_slabs": slabs, "wgrad_rows": rows}
    res["pack_image_us"] = round(sum(us for nm, us in launches if nm.startswith("st_pack_kernel")), 1)
    if not args.no_torch:
        res["torch_fp32_step_ms"] = round(timed(torch_step, args.iters, args.warmup), 3)
        res["speedup_vs_torch_fp32"] = round(res["torch_fp32_step_ms"] / res["hip_step_ms"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
