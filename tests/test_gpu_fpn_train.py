"""The gradient of the DB head's input (dgrad into P2, csrc/dbhead_train.hip: vtd_dbhead_train_backward_input) on the GPU: the first
stage of training the FPN with the head.  `head(features, input_grad=True)` hands `features` its gradient; everything else about the head
is the parent's, bit for bit.

The fp64 reference is tests/test_gpu_dbhead_train.py's: nets.DBHead's own sub-Sequentials under CPU autograd in float64, fed the features
rounded to fp16 and the two GEMM weights rounded to fp16 as the kernels pack them, and the same upstream map gradients.  Metric: relative
L2 error of the whole input-gradient tensor.  Bounds are per case, DESIGN.md section 4's convention: 3x the level measured on an MI355X,
under the ceiling of 1e-2 for gradients."""
import copy

import numpy as np
import pytest
import torch

from vtd_amd import nets, training

GRAD_CEILING = 1e-2
# case -> bound on the relative L2 error of d loss / d features ("Bounds of tests/test_gpu_fpn_train.py")
BOUNDS = {
    "small_train": 1.3e-3,   # measured 4.13e-4 ([3,256,13,11]; 3.95e-4 at [2,256,24,20])
    "tiny_train": 1.1e-3,    # 3.53e-4
    "small_eval": 1e-2,      # 8.33e-3 (3x is over the ceiling): the head's eval-mode level, as its conv 3x3 weight gradient (8.5e-3)
    "tiny_eval": 9e-4,       # 2.87e-4
    "imbalanced": 5.4e-3,    # 1.79e-3 with both maps' gradients (3.25e-4 / 3.20e-4 with the threshold's alone / the two swapped)
    "b32": 2.7e-3,           # 8.85e-4
}
assert max(BOUNDS.values()) <= GRAD_CEILING


def _rounded_head_double(head):
    ref = copy.deepcopy(head).cpu().double()
    with torch.no_grad():
        for seq in (ref.probability_head, ref.threshold_head):
            for i in (0, 3):
                seq[i].weight.copy_(seq[i].weight.half().double())
    return ref


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _seeded_head(seed):
    head = nets.DBHead(256)
    head.load_state_dict(nets.seeded_state_dict(lambda: nets.DBHead(256), seed))
    return head.cuda()


def _random_targets(shape, gen):
    return {"probability_map": (torch.rand(shape, generator=gen) > 0.7).float(), "threshold_map": torch.rand(shape, generator=gen) * 0.6 + 0.2}


def _loss_step(head, feats, targets, input_grad):
    """HIP forward + HIP loss + backward; returns the upstream map gradients the head's backward was given."""
    out = head(feats, input_grad=True) if input_grad else head(feats)
    out["probability"].retain_grad()
    out["threshold"].retain_grad()
    training.detection_loss(out, {k: v.cuda() for k, v in targets.items()})["loss"].backward()
    return out["probability"].grad, out["threshold"].grad


def _param_grads(head):
    return [p.grad.detach().clone() for p in head.parameters()]


def _reference_input_grad(ref, feats64, ups):
    x = feats64.clone().requires_grad_(True)
    torch.autograd.backward([ref.probability_head(x), ref.threshold_head(x)], [ups[0].double().cpu(), ups[1].double().cpu()])
    return x.grad


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 24, 20), (3, 13, 11), (2, 4, 3)])
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_head_input_gradient_against_fp64(hip, shape, mode):
    n, H, W = shape
    gen = torch.Generator().manual_seed(11 + H)
    head = _seeded_head(5 + W).train(mode == "train")
    plain = copy.deepcopy(head)            # the same step without the input gradient: its parameter gradients are the yardstick bits
    ref = _rounded_head_double(head).train(mode == "train")
    feats = (torch.randn((n, 256, H, W), generator=gen) * 0.5).half().float()
    targets = _random_targets((n, 1, 4 * H, 4 * W), gen)
    x = feats.cuda().requires_grad_(True)
    ups = _loss_step(head, x, targets, True)
    _loss_step(plain, feats.cuda(), targets, False)
    assert x.grad is not None and x.grad.shape == x.shape and x.grad.dtype == torch.float32
    want = _reference_input_grad(ref, feats.double(), ups)
    err = _rel(x.grad.double().cpu().numpy(), want.numpy())
    case = ("tiny_" if H * W < 100 else "small_") + mode
    print(f"MEASURED {case} [{n},256,{H},{W}] {mode}: input gradient {err:.3g} (|g| = {float(want.norm()):.3g})")
    got_p, plain_p = _param_grads(head), _param_grads(plain)
    assert len(got_p) == 20 and all(torch.equal(a, b) for a, b in zip(got_p, plain_p)), "input_grad changed a parameter gradient's bits"
    assert all(torch.equal(a, b) for a, b in zip(head.buffers(), plain.buffers()))
    assert err <= BOUNDS[case], f"input gradient relative error {err:.3g} > {BOUNDS[case]}"


@pytest.mark.gpu
def test_branches_with_different_scales_sum_in_one_gemm(hip):
    """The threshold map's upstream gradient 2^-10 of the probability map's: the two branches' dy1 get different power-of-two scales, and
    the ratio folded into one branch's packed weights must make the single GEMM's sum right for both."""
    n, H, W = 2, 24, 20
    gen = torch.Generator().manual_seed(31)
    head = _seeded_head(13).train()
    ref = _rounded_head_double(head).train()
    feats = (torch.randn((n, 256, H, W), generator=gen) * 0.5).half().float()
    gp = torch.randn((n, 1, 4 * H, 4 * W), generator=gen) * 1e-4
    gt = torch.randn((n, 1, 4 * H, 4 * W), generator=gen) * 1e-4 / 1024
    errs = {}
    for name, ups in (("both", (gp, gt)), ("threshold only", (torch.zeros_like(gp), gt)), ("swapped", (gt, gp))):
        h = copy.deepcopy(head)
        x = feats.cuda().requires_grad_(True)
        out = h(x, input_grad=True)
        torch.autograd.backward([out["probability"], out["threshold"]], [ups[0].cuda(), ups[1].cuda()])
        want = _reference_input_grad(copy.deepcopy(ref), feats.double(), ups)
        errs[name] = _rel(x.grad.double().cpu().numpy(), want.numpy())
    print("MEASURED imbalanced: input gradient " + ", ".join(f"{k} {v:.3g}" for k, v in errs.items()))
    assert max(errs.values()) <= BOUNDS["imbalanced"], errs


@pytest.mark.gpu
def test_b32_input_gradient_matches_torch_gpu_fp32(hip):
    """B = 32 x 160^2 with the loss's own ~1e-7 upstream gradients, against torch GPU fp32 autograd of the same head."""
    n, H, W = 32, 160, 160
    gen = torch.Generator(device="cuda").manual_seed(99)
    head = _seeded_head(41).train()
    feats = (torch.randn((n, 256, H, W), generator=gen, device="cuda") * 0.5).half().float()
    tg = {"probability_map": (torch.rand((n, 1, 640, 640), generator=gen, device="cuda") > 0.7).float(),
          "threshold_map": torch.rand((n, 1, 640, 640), generator=gen, device="cuda") * 0.6 + 0.2}
    ref = copy.deepcopy(head)
    with torch.no_grad():
        for seq in (ref.probability_head, ref.threshold_head):
            for i in (0, 3):
                seq[i].weight.copy_(seq[i].weight.half().float())
    x = feats.clone().requires_grad_(True)
    ups = _loss_step(head, x, tg, True)
    assert float(ups[0].abs().median()) < 1e-6
    xr = feats.clone().requires_grad_(True)
    torch.autograd.backward([ref.probability_head(xr), ref.threshold_head(xr)], [ups[0], ups[1]])
    err = float((x.grad.double() - xr.grad.double()).norm() / xr.grad.double().norm())
    print(f"MEASURED b32: input gradient {err:.3g} (|g| = {float(xr.grad.norm()):.3g})")
    assert err <= BOUNDS["b32"], err


@pytest.mark.gpu
def test_input_gradient_is_bitwise_repeatable(hip):
    gen = torch.Generator().manual_seed(2)
    head = _seeded_head(9).train()
    state = copy.deepcopy(head.state_dict())
    feats = (torch.randn((2, 256, 40, 36), generator=gen) * 0.5).half().float().cuda()
    tg = _random_targets((2, 1, 160, 144), gen)
    runs = []
    for _ in range(2):
        head.load_state_dict(state)
        head.zero_grad(set_to_none=True)
        x = feats.clone().requires_grad_(True)
        _loss_step(head, x, tg, True)
        runs.append([x.grad.detach().clone()] + _param_grads(head))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_input_gradient_only_on_request(hip):
    head = _seeded_head(3).train()
    feats = torch.randn((1, 256, 8, 8)).cuda()
    with pytest.raises(RuntimeError, match="dgrad into P2"):
        head(feats.clone().requires_grad_(True))
    # features that do not require grad: input_grad=True changes nothing
    a, b = copy.deepcopy(head), copy.deepcopy(head)
    oa, ob = a(feats, input_grad=True), b(feats)
    assert torch.equal(oa["probability"], ob["probability"]) and torch.equal(oa["threshold"], ob["threshold"])
    # fp16 features receive an fp16 gradient of their own shape
    x = feats.half().requires_grad_(True)
    out = head(x, input_grad=True)
    (out["probability"].sum() + out["threshold"].sum()).backward()
    assert x.grad.dtype == torch.float16 and x.grad.shape == x.shape and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
    # frozen head parameters: the features still receive their gradient
    frozen = copy.deepcopy(head)
    for p in frozen.parameters():
        p.requires_grad_(False)
    y = feats.clone().requires_grad_(True)
    out = frozen(y, input_grad=True)
    (out["probability"].sum() + out["threshold"].sum()).backward()
    assert y.grad is not None and float(y.grad.abs().max()) > 0
