"""The FPN + DB head training step (forward + backward, BatchNorm in train mode) at B = 32 on the product shape (C5 20 x 20, P2 160 x 160):
the HIP kernels (csrc/fpn_train.hip and csrc/dbhead_train.hip through FeaturePyramidNetwork.forward_padded(taps, head)) against torch eager
autograd of the same FPN + head on the same GPU, in fp32 and under torch.autocast(float16).  The trunk taps are fixed random tensors and
the upstream map gradients fixed tensors of ~1e-7 (the loss gradient's size at this batch), so only the FPN and the head are timed.  HIP
events around `--iters` steps after `--warmup`; per-launch times of one step from torch.profiler, with TFLOP/s for the GEMMs and TB/s for
the element-wise passes of the FPN.  Prints one JSON line.

    python tools/fpn_train_bench.py [--backbone resnet18|resnet50] [--batch 32] [--iters 10] [--warmup 3] [--no-torch]
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
from vtd_amd import nets  # noqa: E402

# the conv_igemm launches of one step, in launch order (vtd_launch_fpn_forward, vtd_launch_dbhead_forward / _backward / _backward_input,
# vtd_launch_fpn_backward)
CONV_LABELS = ["fpn_lateral_c5", "fpn_lateral_c4", "fpn_lateral_c3", "fpn_lateral_c2", "fpn_conv3x3_forward", "head_conv3x3_forward",
               "head_convt1_forward_b0", "head_convt1_forward_b1", "head_convt1_dgrad_b0", "head_convt1_dgrad_b1", "head_conv3x3_dgrad",
               "fpn_conv3x3_dgrad"]


def wiring(fpn, feats):
    last = fpn.inner_blocks[0](feats[3])
    for i in range(1, 4):
        last = fpn.inner_blocks[i](feats[3 - i]) + F.interpolate(last, scale_factor=2, mode="nearest")
    return fpn.layer_blocks[3](last)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", default="resnet18", choices=["resnet18", "resnet50"])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="skip the two torch comparisons")
    args = ap.parse_args()
    n, h5, w5 = args.batch, 20, 20
    c5 = nets.trunk_out_channels(args.backbone)
    H, W = 8 * h5, 8 * w5
    torch.manual_seed(0)
    fpn = nets.FeaturePyramidNetwork(c5)
    fpn.load_state_dict(nets.seeded_state_dict(lambda: nets.FeaturePyramidNetwork(c5), 2))
    head = nets.DBHead(256)
    head.load_state_dict(nets.seeded_state_dict(lambda: nets.DBHead(256), 1))
    fpn, head = fpn.cuda(), head.cuda().train()
    rfpn, rhead = copy.deepcopy(fpn), copy.deepcopy(head)
    g = torch.Generator(device="cuda").manual_seed(0)
    feats = [(torch.randn((n, c5 >> (3 - lv), h5 << (3 - lv), w5 << (3 - lv)), generator=g, device="cuda") * 0.5).half() for lv in range(4)]
    padded = [nets.pack_tap(t) for t in feats]
    gp = torch.randn((n, 1, 4 * H, 4 * W), generator=g, device="cuda") * 1e-7
    gt = torch.randn((n, 1, 4 * H, 4 * W), generator=g, device="cuda") * 1e-7

    def hip_step():
        fpn.zero_grad(set_to_none=True)
        head.zero_grad(set_to_none=True)
        out = fpn.forward_padded(padded, head=head)
        torch.autograd.backward([out["probability"], out["threshold"]], [gp, gt])

    def hip_fwd():
        with torch.no_grad():
            fpn.forward_padded(padded, head=head)

    feats32 = None

    def torch_step():
        rfpn.zero_grad(set_to_none=True)
        rhead.zero_grad(set_to_none=True)
        p2 = wiring(rfpn, feats32)
        torch.autograd.backward([rhead.probability_head(p2), rhead.threshold_head(p2)], [gp, gt])

    def torch_autocast_step():
        rfpn.zero_grad(set_to_none=True)
        rhead.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            p2 = wiring(rfpn, feats)
            p, t = rhead.probability_head(p2), rhead.threshold_head(p2)
        torch.autograd.backward([p, t], [gp.to(p.dtype), gt.to(t.dtype)])

    res = {"backbone": args.backbone, "batch": n, "c5": [c5, h5, w5], "p2": [256, H, W]}
    res["hip_step_ms"] = round(timed(hip_step, args.iters, args.warmup), 3)
    res["hip_forward_ms"] = round(timed(hip_fwd, args.iters, args.warmup), 3)
    launches = per_launch(hip_step, CONV_LABELS)
    res["hip_per_kernel_us"] = [[nm, round(us, 1)] for nm, us in launches]
    t = {}
    for nm, us in launches:
        t[nm] = t.get(nm, 0.0) + us
    res["hip_kernels_sum_us"] = round(sum(t.values()), 1)
    M = n * H * W
    k3 = 2.0 * M * 256 * 2304          # 966 GFLOP at B = 32: forward 3x3, its dgrad and its wgrad alike
    lat = [2.0 * (M >> (2 * lv)) * 256 * (c5 >> (3 - lv)) for lv in range(4)]   # per level C2..C5, forward and wgrad alike
    tf = {}
    for lbl, fl in (("fpn_conv3x3_forward", k3), ("fpn_conv3x3_dgrad", k3), ("fpn_lateral_c2", lat[0]), ("fpn_lateral_c3", lat[1]),
                    ("fpn_lateral_c4", lat[2]), ("fpn_lateral_c5", lat[3]), ("head_conv3x3_dgrad", 2.0 * M * 256 * 1152)):
        if t.get(lbl):
            tf[lbl] = fl / (t[lbl] * 1e-6) / 1e12
    # wgrad<0> runs twice per step (the head's conv: 128 columns; the FPN's: 256), wgrad<2> four times (C2..C5, in that order)
    wg0 = [us for nm, us in launches if nm.startswith("dbhead_train_wgrad_kernel<0>")]
    wg2 = [us for nm, us in launches if nm.startswith("dbhead_train_wgrad_kernel<2>")]
    if len(wg0) == 2:
        tf["head_conv3x3_wgrad"] = k3 / 2 / (wg0[0] * 1e-6) / 1e12
        tf["fpn_conv3x3_wgrad"] = k3 / (wg0[1] * 1e-6) / 1e12
    if len(wg2) == 4:
        for lv in range(4):
            tf[f"fpn_lateral_wgrad_c{lv + 2}"] = lat[lv] / (wg2[lv] * 1e-6) / 1e12
    res["gflop"] = {"conv3x3": round(k3 / 1e9, 1), "laterals": [round(x / 1e9, 1) for x in lat]}
    res["tflops"] = {k: round(v, 1) for k, v in tf.items()}
    # HBM passes of the FPN's backward: bytes each streaming kernel must move, summed over its launches of one step
    lv_rows = [M >> (2 * lv) for lv in range(4)]
    pad = n * (H + 2) * (W + 2) * 256 * 2
    bytes_ = {"fpn_train_reduce_kernel": (M + sum(lv_rows)) * 256 * 4,
              "fpn_train_form_kernel": (M + sum(lv_rows)) * 256 * 6 + pad,
              "fpn_train_sumpool_kernel": sum(lv_rows[lv - 1] * 256 * 4 + lv_rows[lv] * 256 * 4 for lv in range(1, 4))}
    res["hbm_tb_per_s"] = {k: round(b / (t[k] * 1e-6) / 1e12, 2) for k, b in bytes_.items() if t.get(k)}
    if not args.no_torch:
        feats32 = [f.float() for f in feats]
        res["torch_fp32_step_ms"] = round(timed(torch_step, args.iters, args.warmup), 3)
        feats32 = None
        res["torch_autocast_fp16_step_ms"] = round(timed(torch_autocast_step, args.iters, args.warmup), 3)
        res["speedup_vs_torch_fp32"] = round(res["torch_fp32_step_ms"] / res["hip_step_ms"], 2)
        res["speedup_vs_torch_autocast"] = round(res["torch_autocast_fp16_step_ms"] / res["hip_step_ms"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
