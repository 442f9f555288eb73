"""DB head training on the HIP kernels (csrc/dbhead_train.hip): parity with fp64 torch autograd, the product DBNet(trainable='head') path,
B = 32 gradients of ~1e-7 against torch GPU fp32 autograd, trained-then-inferred maps, repeatability and the default path unchanged.

The fp64 reference is nets.DBHead's own sub-Sequentials (torch ops, CPU, float64) fed the features and the weights the kernels use: the
features rounded to fp16 (their storage format), the two GEMM weights (conv 3x3, ConvT1) rounded to fp16 as the kernels pack them.
Bounds are per case, DESIGN.md section 4's: 3x the level measured on an MI355X, under the ceilings of 1e-2 (gradients, relative L2 per
tensor) and 2e-3 (maps, max |dp|).  Running statistics are held through the batch statistic each update implies,
(after - (1 - momentum) before) / momentum, so that biased for unbiased variance (a 1 / (n - 1) relative change) is visible."""
import copy

import numpy as np
import pytest
import torch

from vtd_amd import nets, training

GRAD_CEILING, MAP_CEILING = 1e-2, 2e-3
# case -> bounds: "grad" worst per-tensor relative L2 error of the parameter gradients, "map" max |dp| of the two
# maps, "stat" worst relative L2 error of the batch statistic implied by a running-stat update (after three steps: of the running values)
BOUNDS = {
    "small_train": {"grad": 1.5e-3, "map": 1.3e-3, "stat": 6e-5},     # measured 4.95e-4, 4.14e-4, 1.85e-5
    "tiny_train": {"grad": 1.2e-3, "map": 9e-4, "stat": 3e-4},        # 3.73e-4, 2.74e-4, 9.54e-5
    "small_eval": {"grad": 1e-2, "map": 8e-5, "stat": 0.0},           # 8.5e-3 (3x is over the ceiling), 2.57e-5; eval writes no stats
    "tiny_eval": {"grad": 1e-3, "map": 7e-5, "stat": 0.0},            # 3.02e-4, 2.06e-5
    "product_resnet18": {"grad": 8.5e-3, "map": 2e-3, "stat": 6e-6},  # 2.79e-3, 9.01e-4 (3x is over the ceiling), 1.81e-6
    "product_resnet50": {"grad": 1e-2, "map": 2e-3, "stat": 8e-6},    # 4.03e-3 (3x is over the ceiling), 8.61e-4 (idem), 2.48e-6
    "b32": {"grad": 1.1e-3, "map": 2e-3},                             # 3.63e-4, 6.86e-4 (3x is over the ceiling)
    "three_steps": {"stat": 8e-7},                                    # 2.43e-7
}
MOMENTUM = 0.1


def _rounded_head_double(head):
    """A CPU float64 copy of `head` with the GEMM weights rounded to fp16 as the kernels pack them."""
    ref = copy.deepcopy(head).cpu().double()
    with torch.no_grad():
        for seq in (ref.probability_head, ref.threshold_head):
            for i in (0, 3):
                seq[i].weight.copy_(seq[i].weight.half().double())
    return ref


def _ref_forward(ref, feats64):
    return ref.probability_head(feats64), ref.threshold_head(feats64)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _grad_errors(head, ref, training_mode):
    """{name: error} per learnable tensor.  The bias in front of a train-mode BatchNorm has an exactly-zero gradient in exact arithmetic
    (both sides are rounding noise): its error is taken relative to the following BatchNorm's beta gradient (the same sum of dy)."""
    errs = {}
    for br in ("probability_head", "threshold_head"):
        hs, rs = getattr(head, br), getattr(ref, br)
        for i, attr in ((0, "weight"), (0, "bias"), (1, "weight"), (1, "bias"), (3, "weight"), (3, "bias"), (4, "weight"), (4, "bias"),
                        (6, "weight"), (6, "bias")):
            g = getattr(hs[i], attr).grad.detach().double().cpu().numpy()
            r = getattr(rs[i], attr).grad.detach().numpy()
            if training_mode and attr == "bias" and i in (0, 3):
                nxt = getattr(rs[i + 1], "bias").grad.detach().numpy()
                errs[f"{br}.{i}.{attr}"] = float(np.linalg.norm(g - r) / max(np.linalg.norm(nxt), 1e-300))
            else:
                errs[f"{br}.{i}.{attr}"] = _rel(g, r)
    return errs


def _random_targets(shape, gen):
    return {"probability_map": (torch.rand(shape, generator=gen) > 0.7).float(), "threshold_map": torch.rand(shape, generator=gen) * 0.6 + 0.2}


def _head_step(head, feats32, targets, padded=None):
    """One HIP forward + HIP loss backward; returns (maps, upstream gradients)."""
    out = head(feats32) if padded is None else head.forward_padded(padded, feats32.shape[2], feats32.shape[3])
    out["probability"].retain_grad()
    out["threshold"].retain_grad()
    tg = {k: v.cuda() for k, v in targets.items()}
    loss = training.detection_loss(out, tg)["loss"]
    loss.backward()
    return out, (out["probability"].grad, out["threshold"].grad)


def _bn_stats(head):
    return {(br, i, a): getattr(getattr(head, br)[i], a).detach().double().cpu().clone()
            for br in ("probability_head", "threshold_head") for i in (1, 4) for a in ("running_mean", "running_var")}


def _check_parity(head, ref, feats64, out, ups, training_mode, what, case):
    """`ref` has not run yet: its running statistics are those `head` had before its forward."""
    bounds = BOUNDS[case]
    before = _bn_stats(ref)
    rp, rt = _ref_forward(ref, feats64)
    dmap = max(float((got.detach().double().cpu() - want.detach()).abs().max()) for got, want in ((out["probability"], rp), (out["threshold"], rt)))
    torch.autograd.backward([rp, rt], [ups[0].double().cpu(), ups[1].double().cpu()])
    errs = _grad_errors(head, ref, training_mode)
    worst = max(errs, key=errs.get)
    dstat = 0.0
    if training_mode:
        got_s, ref_s = _bn_stats(head), _bn_stats(ref)
        for k in before:   # the batch statistic each update implies
            implied = lambda d: ((d[k] - (1 - MOMENTUM) * before[k]) / MOMENTUM).numpy()  # noqa: E731
            dstat = max(dstat, _rel(implied(got_s), implied(ref_s)))
        for br in ("probability_head", "threshold_head"):
            for i in (1, 4):
                assert int(getattr(head, br)[i].num_batches_tracked) == int(getattr(ref, br)[i].num_batches_tracked)
    ct1 = max(v for k, v in errs.items() if k.endswith(".3.weight"))
    print(f"MEASURED {case} {what}: grad {errs[worst]:.3g} ({worst}), map {dmap:.3g}, stat {dstat:.3g}, ConvT1 weight {ct1:.3g}")
    assert dmap <= bounds["map"], f"{what}: map max |dp| = {dmap:.3g} > {bounds['map']}"
    assert errs[worst] <= bounds["grad"], f"{what}: gradient of {worst}: relative error {errs[worst]:.3g} > {bounds['grad']} ({errs})"
    assert dstat <= bounds["stat"], f"{what}: implied batch statistic relative error {dstat:.3g} > {bounds['stat']}"
    return errs


def _seeded_head(seed):
    torch.manual_seed(seed)
    head = nets.DBHead(256)
    sd = nets.seeded_state_dict(lambda: nets.DBHead(256), seed)
    head.load_state_dict(sd)
    return head.cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 24, 20), (3, 13, 11), (2, 4, 3)])
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_stage_parity_small_shapes(hip, shape, mode):
    n, H, W = shape
    gen = torch.Generator().manual_seed(11 + H)
    head = _seeded_head(5 + W)
    head.train(mode == "train")
    ref = _rounded_head_double(head)
    ref.train(mode == "train")
    feats = (torch.randn((n, 256, H, W), generator=gen) * 0.5).half().float()
    out, ups = _head_step(head, feats.cuda(), _random_targets((n, 1, 4 * H, 4 * W), gen))
    case = ("tiny_" if H * W < 100 else "small_") + mode
    _check_parity(head, ref, feats.double(), out, ups, mode == "train", f"[{n},256,{H},{W}] {mode}", case)
    if mode == "eval":   # eval mode leaves the running statistics alone
        for seq_h, seq_r in ((head.probability_head, ref.probability_head), (head.threshold_head, ref.threshold_head)):
            assert torch.equal(seq_h[1].running_mean.cpu().double(), seq_r[1].running_mean)
            assert int(seq_h[1].num_batches_tracked) == 0


def _padded_to_nchw64(padded):
    return padded[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).double().cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("backbone,batch", [("resnet18", 2), ("resnet50", 1)])
def test_product_training_step_and_adamw(hip, backbone, batch):
    from vtd_amd._fixtures.weights import stress_detector_state_dict
    torch.manual_seed(3)
    net = nets.DBNet(backbone, compute_threshold=True, trainable="head")
    net.load_state_dict(stress_detector_state_dict(backbone, 17))
    net.cuda().train()
    mod = training.TextDetectionLightningModule(net)
    opt = mod.configure_optimizers()["optimizer"]
    gen = torch.Generator().manual_seed(23)
    x = torch.randn((batch, 3, 640, 640), generator=gen).cuda()
    targets = _random_targets((batch, 1, 640, 640), gen)
    # the engine's own P2, stage-isolated reference
    feats = net.features_engine().forward_features(x)
    ref = _rounded_head_double(net.head)
    ref.train()
    captured = {}
    orig = nets.DBHead.forward_padded

    def spy(self, f, H, W):
        out = orig(self, f, H, W)
        out["probability"].retain_grad()
        out["threshold"].retain_grad()
        captured["out"] = out
        return out

    nets.DBHead.forward_padded = spy
    try:
        loss = mod.training_step((x, targets), 0)
    finally:
        nets.DBHead.forward_padded = orig
    loss.backward()
    out = captured["out"]
    assert all(p.grad is None for p in net.backbone.parameters()) and all(p.grad is None for p in net.fpn.parameters())
    _check_parity(net.head, ref, _padded_to_nchw64(feats), out, (out["probability"].grad, out["threshold"].grad), True, f"{backbone} B={batch}",
                  "product_" + backbone)
    before = [p.detach().clone() for p in net.head.parameters()]
    opt.step()
    assert all(not torch.equal(a, b) for a, b in zip(before, net.head.parameters()))


@pytest.mark.gpu
def test_b32_gradients_match_torch_gpu_fp32(hip):
    """~1e-7 per-element loss gradients at B = 32 x 640^2: fp16 operands without the exact scale would flush them."""
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
    out, ups = _head_step(head, feats, tg)
    assert float(ups[0].abs().median()) < 1e-6   # most upstream gradients are below fp16's smallest normal (6.1e-5)
    rp, rt = ref.probability_head(feats), ref.threshold_head(feats)
    torch.autograd.backward([rp, rt], [ups[0], ups[1]])
    dmap = max(float((got - want).detach().abs().max()) for got, want in ((out["probability"], rp), (out["threshold"], rt)))
    errs = {}
    for br in ("probability_head", "threshold_head"):
        for (i, a) in ((0, "weight"), (1, "weight"), (1, "bias"), (3, "weight"), (4, "weight"), (4, "bias"), (6, "weight"), (6, "bias")):
            g = getattr(getattr(head, br)[i], a).grad.double()
            r = getattr(getattr(ref, br)[i], a).grad.double()
            errs[f"{br}.{i}.{a}"] = float((g - r).norm() / r.norm())
    worst = max(errs, key=errs.get)
    print(f"MEASURED b32: grad {errs[worst]:.3g} ({worst}), map {dmap:.3g}")
    assert dmap <= BOUNDS["b32"]["map"], dmap
    assert errs[worst] <= BOUNDS["b32"]["grad"], errs


@pytest.mark.gpu
def test_trained_model_infers_with_what_it_learned(hip):
    from vtd_amd._fixtures.weights import stress_detector_state_dict
    net = nets.DBNet("resnet18", compute_threshold=True, trainable="head")
    net.load_state_dict(stress_detector_state_dict("resnet18", 5))
    net.cuda()
    mod = training.TextDetectionLightningModule(net)
    opt = mod.configure_optimizers()["optimizer"]
    gen = torch.Generator().manual_seed(7)
    ref = _rounded_head_double(net.head)
    for step in range(3):
        net.train()
        x = torch.randn((2, 3, 640, 640), generator=gen).cuda()
        feats = _padded_to_nchw64(net.features_engine().forward_features(x))
        # the reference chain: this step's parameters, its own running statistics
        with torch.no_grad():
            cur = _rounded_head_double(net.head)
            for seq_r, seq_c in ((ref.probability_head, cur.probability_head), (ref.threshold_head, cur.threshold_head)):
                for i in (0, 1, 3, 4, 6):
                    for a in ("weight", "bias"):
                        getattr(seq_r[i], a).copy_(getattr(seq_c[i], a))
        ref.train()
        _ref_forward(ref, feats)
        loss = mod.training_step((x, _random_targets((2, 1, 640, 640), gen)), step)
        opt.zero_grad()
        loss.backward()
        opt.step()
    net.eval()
    x = torch.randn((2, 3, 640, 640), generator=gen).cuda()
    with torch.no_grad():
        got = net(x)
    fresh = nets.DBNet("resnet18", compute_threshold=True)
    fresh.load_state_dict(net.state_dict())
    want = fresh(x)
    assert torch.equal(got["probability"], want["probability"]) and torch.equal(got["threshold"], want["threshold"])
    worst = 0.0
    for br in ("probability_head", "threshold_head"):
        for i in (1, 4):
            bn, rb = getattr(net.head, br)[i], getattr(ref, br)[i]
            assert int(bn.num_batches_tracked) == 3
            for a in ("running_mean", "running_var"):
                worst = max(worst, _rel(getattr(bn, a).double().cpu().numpy(), getattr(rb, a).numpy()))
    print(f"MEASURED three_steps: stat {worst:.3g}")
    assert worst <= BOUNDS["three_steps"]["stat"], worst


@pytest.mark.gpu
def test_step_is_bitwise_repeatable(hip):
    gen = torch.Generator().manual_seed(2)
    head = _seeded_head(9).train()
    state = copy.deepcopy(head.state_dict())
    feats = (torch.randn((2, 256, 40, 36), generator=gen) * 0.5).half().float().cuda()
    tg = _random_targets((2, 1, 160, 144), gen)
    runs = []
    for _ in range(2):
        head.load_state_dict(state)
        head.zero_grad(set_to_none=True)
        _head_step(head, feats, tg)
        runs.append([t.detach().clone() for t in [p.grad for p in head.parameters()] + list(head.buffers())])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_default_path_unchanged_and_refusals(hip):
    from vtd_amd._fixtures.weights import stress_detector_state_dict
    net = nets.DBNet("resnet18", compute_threshold=True)
    net.load_state_dict(stress_detector_state_dict("resnet18", 3))
    x = torch.randn((1, 3, 640, 640), generator=torch.Generator().manual_seed(1)).cuda()
    net.train()
    with torch.enable_grad():
        a = net(x)
    net.eval()
    b = net(x)
    assert not a["probability"].requires_grad and not a["threshold"].requires_grad
    assert torch.equal(a["probability"], b["probability"]) and torch.equal(a["threshold"], b["threshold"])
    net.set_trainable("head")
    net.cuda().train()
    net.backbone[0].weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match="trunk / FPN is not implemented"):
        net(x)
