"""The DB head's training step (forward + backward, both branches, BatchNorm in train mode) at B = 32 on 160 x 160 P2 features: the HIP
kernels (csrc/dbhead_train.hip through vtd_amd.nets.DBHead) against torch eager autograd of the same head on the same GPU, in fp32 and
under torch.autocast(float16).  The upstream map gradients are fixed tensors of ~1e-7 (the loss gradient's size at this batch), so only
the head is timed.  HIP events around `--iters` steps after `--warmup`; per-launch times of one step from torch.profiler.  Prints one
JSON line.  `--input-grad` adds the gradient of the features on both sides (dgrad into P2: `head(features, input_grad=True)`, which also
packs the NCHW features and unpacks their gradient inside the step; torch with `features.requires_grad`).

    python tools/dbhead_train_bench.py [--batch 32] [--iters 20] [--warmup 5] [--input-grad]
"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "video-text-detection-system_amd"), ROOT]

import torch  # noqa: E402

from vtd_amd import nets  # noqa: E402


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters   # milliseconds per step


def _clean(names):
    """Readable kernel names: demangled (c++filt when the profiler reports mangled symbols), without the return type, the anonymous
    namespace and the argument list -- 'dbhead_train_wgrad_kernel<0>'."""
    import re
    import subprocess
    mangled = [n for n in names if n.startswith("_Z")]
    dem = {}
    if mangled:
        try:
            out = subprocess.run([os.environ.get("CXXFILT", "c++filt")], input="\n".join(mangled), capture_output=True, text=True, timeout=30).stdout.splitlines()
            dem = dict(zip(mangled, out))
        except (OSError, subprocess.SubprocessError):
            dem = {}
    res = []
    for n in names:
        m = re.match(r"_ZN12_GLOBAL__N_1(\d+)(\w+)", n) if n not in dem or dem[n] == n else None
        if m:   # no demangler: the anonymous-namespace kernels of this project, first template argument only
            base, rest = m.group(2)[:int(m.group(1))], m.group(2)[int(m.group(1)):]
            a = re.match(r"ILi(\d+)E|I(DF16_)|I(f)E", rest)
            arg = "" if not a else "<%s>" % (a.group(1) or ("_Float16" if a.group(2) else "float"))
            res.append(base + arg)
            continue
        d = dem.get(n, n).replace("(anonymous namespace)::", "")
        d = re.sub(r"^void ", "", d).split("(")[0]
        res.append(d.split("::")[-1] if "<" not in d else d[d.rfind("::", 0, d.index("<")) + 2 if "::" in d[:d.index("<")] else 0:])
    return res


# the conv_igemm launches of one step, in launch order (vtd_launch_dbhead_forward / _backward)
CONV_LABELS = ["conv3x3_forward", "convt1_forward_b0", "convt1_forward_b1", "convt1_dgrad_b0", "convt1_dgrad_b1", "conv3x3_dgrad"]


def per_launch(fn, labels=None):
    """[(label, microseconds)] of every kernel one step launches, in launch order (torch.profiler's device events)."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    evs = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and e.time_range.elapsed_us() > 0]
    evs.sort(key=lambda e: e.time_range.start)
    names = _clean([e.name for e in evs])
    labels = CONV_LABELS if labels is None else labels
    out, conv = [], 0
    for e, nm in zip(evs, names):
        if nm.startswith("conv_igemm"):
            nm = labels[conv] if conv < len(labels) else nm
            conv += 1
        out.append((nm, float(e.time_range.elapsed_us())))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--input-grad", action="store_true")
    args = ap.parse_args()
    n, H, W = args.batch, 160, 160
    torch.manual_seed(0)
    head = nets.DBHead(256)
    head.load_state_dict(nets.seeded_state_dict(lambda: nets.DBHead(256), 1))
    head = head.cuda().train()
    ref = copy.deepcopy(head)
    g = torch.Generator(device="cuda").manual_seed(0)
    feats = (torch.randn((n, 256, H, W), generator=g, device="cuda") * 0.5).half().float()
    padded = nets.pack_features(feats)
    gp = torch.randn((n, 1, 4 * H, 4 * W), generator=g, device="cuda") * 1e-7
    gt = torch.randn((n, 1, 4 * H, 4 * W), generator=g, device="cuda") * 1e-7

    if args.input_grad:
        feats.requires_grad_(True)

    def hip_step():
        head.zero_grad(set_to_none=True)
        feats.grad = None
        out = head(feats, input_grad=True) if args.input_grad else head.forward_padded(padded, H, W)
        torch.autograd.backward([out["probability"], out["threshold"]], [gp, gt])

    def hip_fwd():
        with torch.no_grad():
            head.forward_padded(padded, H, W)

    def torch_step():
        ref.zero_grad(set_to_none=True)
        feats.grad = None
        torch.autograd.backward([ref.probability_head(feats), ref.threshold_head(feats)], [gp, gt])

    def torch_autocast_step():
        ref.zero_grad(set_to_none=True)
        feats.grad = None
        with torch.autocast("cuda", dtype=torch.float16):
            p, t = ref.probability_head(feats), ref.threshold_head(feats)
        torch.autograd.backward([p, t], [gp.to(p.dtype), gt.to(t.dtype)])

    res = {"batch": n, "features": [256, H, W], "input_grad": bool(args.input_grad)}
    res["hip_step_ms"] = round(timed(hip_step, args.iters, args.warmup), 3)
    res["hip_forward_ms"] = round(timed(hip_fwd, args.iters, args.warmup), 3)
    res["torch_fp32_step_ms"] = round(timed(torch_step, args.iters, args.warmup), 3)
    res["torch_autocast_fp16_step_ms"] = round(timed(torch_autocast_step, args.iters, args.warmup), 3)
    launches = per_launch(hip_step)
    res["hip_per_kernel_us"] = [[nm, round(us, 1)] for nm, us in launches]
    t = {}
    for nm, us in launches:
        t[nm] = t.get(nm, 0.0) + us
    res["hip_kernels_sum_us"] = round(sum(t.values()), 1)
    M1 = n * H * W
    M2 = 4 * M1
    conv_flop = 2.0 * M1 * 128 * 2304   # conv 3x3, both branches: the forward and the weight gradient alike (483 GFLOP at B = 32)
    res["conv3x3_gflop"] = round(conv_flop / 1e9, 1)
    tf = {}
    if t.get("conv3x3_forward"):
        tf["conv3x3_forward"] = conv_flop / (t["conv3x3_forward"] * 1e-6) / 1e12
    if t.get("conv3x3_dgrad"):
        tf["conv3x3_dgrad"] = 2.0 * M1 * 256 * 1152 / (t["conv3x3_dgrad"] * 1e-6) / 1e12   # K = 9 x 128, N = 256: 483 GFLOP at B = 32
    wg = [k for k in t if k.startswith("dbhead_train_wgrad_kernel<0>")]
    if wg:
        tf["conv3x3_wgrad"] = conv_flop / (t[wg[0]] * 1e-6) / 1e12
    convt_flop = 2.0 * M1 * 256 * 128   # ConvT1 forward per branch: K = 128 (a1 hi | lo), N = 256
    dgrad_flop = 2.0 * M1 * 64 * 256    # ConvT1 input gradient per branch
    for lbl, fl in (("convt1_forward_b0", convt_flop), ("convt1_forward_b1", convt_flop), ("convt1_dgrad_b0", dgrad_flop),
                    ("convt1_dgrad_b1", dgrad_flop)):
        if t.get(lbl):
            tf[lbl] = fl / (t[lbl] * 1e-6) / 1e12
    wg1 = [k for k in t if k.startswith("dbhead_train_wgrad_kernel<1>")]
    if wg1:
        tf["convt1_wgrad"] = 2 * 2.0 * M1 * 64 * 256 / (t[wg1[0]] * 1e-6) / 1e12
    res["tflops"] = {k: round(v, 1) for k, v in tf.items()}
    # HBM passes: bytes each streaming kernel must move (layouts of dbhead_train.hip; the maps' 4 sub-pixels per z pixel read once)
    bytes_ = {"dbhead_train_stats_partial_kernel<float>": M1 * 128 * 4, "dbhead_train_stats_partial_kernel<_Float16>": M2 * 128 * 2,
              "dbhead_train_bn_relu_kernel": M1 * 128 * 8, "dbhead_train_convt2_sigmoid_kernel": M2 * 128 * 2 + 32 * M2,
              "dbhead_train_bwd_reduce_kernel<2>": M2 * 128 * 2 + 64 * M2, "dbhead_train_bwd_form_kernel<2>": M2 * 128 * 4 + 64 * M2,
              "dbhead_train_bwd_reduce_kernel<1>": M1 * 128 * 8, "dbhead_train_bwd_form_kernel<1>": M1 * 128 * 10,
              "dbhead_train_pad_dy1_kernel": M1 * 128 * 2 + n * (H + 2) * (W + 2) * 128 * 2,
              "dbhead_train_unpack_input_grad_kernel": M1 * 256 * 8, "dbhead_train_pack_features_kernel<float>": M1 * 256 * 6}
    res["hbm_tb_per_s"] = {k: round(b / (t[k] * 1e-6) / 1e12, 2) for k, b in bytes_.items() if t.get(k)}
    res["speedup_vs_torch_fp32"] = round(res["torch_fp32_step_ms"] / res["hip_step_ms"], 2)
    res["speedup_vs_torch_autocast"] = round(res["torch_autocast_fp16_step_ms"] / res["hip_step_ms"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
