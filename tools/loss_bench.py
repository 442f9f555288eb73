"""The training step's loss layer at B = 32 x 640 x 640 on the GPU: HIP forward + backward (vtd_dbloss_forward / vtd_dbloss_backward through
vtd_amd.training) and the validation counts kernel (vtd_binary_counts_accumulate), against torch eager autograd of the reference loss
(two nn.BCELoss terms + the Dice formula of trainer.py:135-142) and the reference's validation metric path (maps to the host + sklearn
formula on counts, timed without sklearn itself).  HIP events around `--iters` repetitions after `--warmup`; prints one JSON line.
"kernel_*" times are the C entry points alone on preallocated buffers; "hip_*" are the Python surface (allocation and autograd included).

    python tools/loss_bench.py [--batch 32] [--iters 50] [--warmup 10]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "video-text-detection-system_amd"), ROOT]

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from vtd_amd import _native, training  # noqa: E402


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
    return a.elapsed_time(b) * 1e3 / iters   # microseconds per repetition


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    shape = (args.batch, 1, 640, 640)
    prob = torch.sigmoid(torch.randn(shape, generator=g, device="cuda") * 2)
    thresh = torch.sigmoid(torch.randn(shape, generator=g, device="cuda"))
    prob_t = (torch.rand(shape, generator=g, device="cuda") < 0.15).float()
    thresh_t = 0.3 + 0.4 * torch.rand(shape, generator=g, device="cuda")
    targets = {"probability_map": prob_t, "threshold_map": thresh_t}
    p, th = prob.clone().requires_grad_(), thresh.clone().requires_grad_()
    n = prob.numel()

    def hip_fwd():
        with torch.no_grad():
            training.detection_loss({"probability": prob, "threshold": thresh}, targets)

    def hip_fwd_bwd():
        p.grad = th.grad = None
        training.detection_loss({"probability": p, "threshold": th}, targets)["loss"].backward()

    bce = nn.BCELoss()

    def torch_fwd_bwd():
        p.grad = th.grad = None
        pv, tv = p.view(-1), prob_t.view(-1)
        d = 1 - (2. * (pv * tv).sum() + 1e-5) / (pv.sum() + tv.sum() + 1e-5)
        (bce(p, prob_t) + bce(th, thresh_t) + d).backward()

    counts = training.BinaryMetricCounts()

    def hip_counts():
        counts.update(prob, prob_t)

    def torch_counts():   # the reference's on_validation_epoch_end up to sklearn: threshold, flatten, copy both maps to the host
        (prob.flatten() > 0.5).float().cpu()
        prob_t.flatten().cpu()

    # the kernels alone: the C entry points on preallocated buffers (no allocation, no autograd bookkeeping between launches)
    lib = _native.require()
    ws = torch.empty(int(lib.vtd_dbloss_workspace_bytes()), dtype=torch.uint8, device="cuda")
    out4, sums5 = torch.empty(4, device="cuda"), torch.empty(5, dtype=torch.float64, device="cuda")
    gout = torch.tensor([0.0, 0.0, 0.0, 1.0], device="cuda")
    gp, gt, c4 = torch.empty_like(prob), torch.empty_like(prob), torch.zeros(4, dtype=torch.int64, device="cuda")
    P = {k: C.c_void_p(v.data_ptr()) for k, v in dict(prob=prob, thresh=thresh, prob_t=prob_t, thresh_t=thresh_t, ws=ws, out4=out4,
                                                          sums5=sums5, gout=gout, gp=gp, gt=gt, c4=c4).items()}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def k_fwd():
        return lib.vtd_dbloss_forward(P["prob"], P["thresh"], P["prob_t"], P["thresh_t"], n, 1e-5, P["ws"], P["out4"], P["sums5"], stream)

    def k_bwd():
        return lib.vtd_dbloss_backward(P["prob"], P["thresh"], P["prob_t"], P["thresh_t"], n, 1e-5, P["sums5"], P["gout"], P["gp"], P["gt"], stream)

    def k_counts():
        return lib.vtd_binary_counts_accumulate(P["prob"], P["prob_t"], n, 0.5, P["c4"], stream)

    for f in (k_fwd, k_bwd, k_counts):
        _native.check(f(), f.__name__)
    res = {"batch": args.batch, "positions": n}
    for name, fn in (("kernel_forward_us", k_fwd), ("kernel_backward_us", k_bwd), ("kernel_counts_us", k_counts),
                     ("hip_forward_us", hip_fwd), ("hip_forward_backward_us", hip_fwd_bwd), ("torch_forward_backward_us", torch_fwd_bwd),
                     ("hip_counts_us", hip_counts), ("torch_counts_to_host_us", torch_counts)):
        res[name] = round(timed(fn, args.iters, args.warmup), 1)
    # HBM bytes each kernel must move: forward 16 B / position, backward 24 B, counts 8 B
    for key, per in (("forward", 16), ("backward", 24), ("counts", 8)):
        res[f"kernel_{key}_TBps"] = round(per * n / (res[f"kernel_{key}_us"] * 1e-6) / 1e12, 2)
    res["speedup_forward_backward"] = round(res["torch_forward_backward_us"] / res["hip_forward_backward_us"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
