"""The FPN's input gradients (csrc/fpn_train.hip, vtd_fpn_train_backward_input) at B = 32 on the product shape (C5 20 x 20, P2 160 x 160):
the FPN backward from a fixed dP2 without input gradients, with dC5 alone and with all four, timed with HIP events around `--iters` calls
after `--warmup`.  The difference to the plain backward is what the request costs (per level: pack the transposed weights, form the fp16
operand again, one GEMM with M = n h w, K = 256, N = C_k); TFLOP/s are the GEMMs' FLOPs over that difference, so they include the two
element-wise passes.  Prints one JSON line.

    python tools/fpn_input_grad_bench.py [--backbone resnet18|resnet50] [--batch 32] [--iters 10] [--warmup 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "video-text-detection-system_amd"), ROOT, os.path.dirname(os.path.abspath(__file__))]

import torch  # noqa: E402

from dbhead_train_bench import timed  # noqa: E402
from vtd_amd import nets  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", default="resnet18", choices=["resnet18", "resnet50"])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    n, h5, w5 = args.batch, 20, 20
    c5 = nets.trunk_out_channels(args.backbone)
    geom = (n, h5, w5, c5)
    H, W = 8 * h5, 8 * w5
    fpn = nets.FeaturePyramidNetwork(c5)
    fpn.load_state_dict(nets.seeded_state_dict(lambda: nets.FeaturePyramidNetwork(c5), 2))
    fpn = fpn.cuda()
    params = [p.detach() for p in fpn.live_parameters()]
    g = torch.Generator(device="cuda").manual_seed(0)
    taps = tuple(nets.pack_tap((torch.randn((n, c5 >> (3 - lv), h5 << (3 - lv), w5 << (3 - lv)), generator=g, device="cuda") * 0.5).half())
                 for lv in range(4))
    _, ws = nets._fpn_forward_raw(taps, geom, params)
    dp2 = torch.randn((n, H, W, 256), generator=g, device="cuda") * 1e-7
    dscale = torch.ones(2, dtype=torch.float32, device="cuda")

    res = {"backbone": args.backbone, "batch": n, "c5": [c5, h5, w5]}
    ms = {}
    for name, mask in (("backward", 0), ("backward_dc5", 8), ("backward_dc2_to_dc5", 15)):
        ms[name] = timed(lambda: nets._fpn_backward_raw(taps, geom, params, ws, dp2, dscale, mask), args.iters, args.warmup)
        res[name + "_ms"] = round(ms[name], 3)
    M = n * H * W
    flop = [2.0 * (M >> (2 * lv)) * 256 * (c5 >> (3 - lv)) for lv in range(4)]
    res["gflop"] = [round(x / 1e9, 1) for x in flop]
    res["dc5_ms"] = round(ms["backward_dc5"] - ms["backward"], 3)
    res["dc2_to_dc5_ms"] = round(ms["backward_dc2_to_dc5"] - ms["backward"], 3)
    if res["dc5_ms"] > 0:
        res["dc5_tflops"] = round(flop[3] / (res["dc5_ms"] * 1e-3) / 1e12, 1)
    if res["dc2_to_dc5_ms"] > 0:
        res["dc2_to_dc5_tflops"] = round(sum(flop) / (res["dc2_to_dc5_ms"] * 1e-3) / 1e12, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
