"""Backward into the trunk taps on the GPU, first stage: the FPN's input gradients dC2..dC5 (csrc/fpn_train.hip,
vtd_fpn_train_backward_input) through `fpn([C2, C3, C4, C5], input_grad=True)`.

The fp64 reference is the module's own wiring under CPU autograd in float64, as in tests/test_gpu_fpn_neck_train.py: fed the
taps rounded to fp16, the GEMM weights rounded to fp16 as the kernels pack them, and the same upstream gradient.  Metric: relative L2 error
per tensor.  Bounds are per case, DESIGN.md section 4's convention: 3x the level measured on an MI355X, under the ceiling of 1e-2 for
gradients."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vtd_amd import nets

GRAD_CEILING = 1e-2
# case -> bound on the relative L2 error of dC2..dC5 ("Bounds of tests/test_gpu_layer4_train.py"); measured values behind
BOUNDS = {
    "input_resnet18": 9.1e-4,    # measured 3.02e-4 (dC5 at C5 = 3x2; worst of the three sizes and the four levels)
    "input_resnet50": 8.9e-4,    # 2.95e-4 (dC5 at C5 = 5x4, dC3 at 1x1)
}
assert all(v <= GRAD_CEILING for v in BOUNDS.values())

PLANS = {"resnet18": 512, "resnet50": 2048}
FPN_NAMES = [f"inner_blocks.{i}.weight" for i in range(4)] + [f"inner_blocks.{i}.bias" for i in range(4)] + ["layer_blocks.3.weight", "layer_blocks.3.bias"]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _seeded_fpn(c5, seed):
    fpn = nets.FeaturePyramidNetwork(c5)
    fpn.load_state_dict(nets.seeded_state_dict(lambda: nets.FeaturePyramidNetwork(c5), seed))
    return fpn.cuda()


def _rounded_fpn(fpn):
    """A float64 CPU copy of `fpn` with the GEMM weights rounded to fp16 as the kernels pack them (biases stay fp32 values)."""
    ref = copy.deepcopy(fpn).to(device="cpu", dtype=torch.float64)
    with torch.no_grad():
        for m in list(ref.inner_blocks) + [ref.layer_blocks[3]]:
            m.weight.copy_(m.weight.half().double())
    return ref


def _wiring(fpn, feats):
    last = fpn.inner_blocks[0](feats[3])
    for i in range(1, 4):
        last = fpn.inner_blocks[i](feats[3 - i]) + F.interpolate(last, scale_factor=2, mode="nearest")
    return fpn.layer_blocks[3](last)


def _taps(n, c5, h5, w5, gen):
    """Random taps C2..C5 with fp16-representable values."""
    return [(torch.randn((n, c5 >> (3 - lv), h5 << (3 - lv), w5 << (3 - lv)), generator=gen) * 0.5).half().float() for lv in range(4)]


def _param_grads(fpn):
    sd = dict(fpn.named_parameters())
    return [sd[k].grad.detach().clone() for k in FPN_NAMES]


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(3, 2), (1, 1), (5, 4)])
@pytest.mark.parametrize("backbone", sorted(PLANS))
def test_fpn_input_gradients_against_fp64(hip, backbone, size):
    c5, (h5, w5), n = PLANS[backbone], size, 2
    gen = torch.Generator().manual_seed(41 + h5)
    fpn = _seeded_fpn(c5, 5 + w5)
    ref = _rounded_fpn(fpn)
    feats = _taps(n, c5, h5, w5, gen)
    up = torch.randn((n, 256, 8 * h5, 8 * w5), generator=gen)

    # the reference: autograd of the wiring in float64
    rfeats = [t.double().requires_grad_(True) for t in feats]
    _wiring(ref, rfeats).backward(up.double())

    # all four input gradients
    xs = [t.cuda().requires_grad_(True) for t in feats]
    p2 = fpn(xs, input_grad=True)
    assert p2.dtype == torch.float32 and p2.requires_grad
    p2.backward(up.cuda())
    errs = {}
    for lv, (x, r) in enumerate(zip(xs, rfeats)):
        assert x.grad is not None and x.grad.shape == x.shape and x.grad.dtype == torch.float32
        assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
        errs[f"dC{lv + 2}"] = _rel(x.grad.double().cpu().numpy(), r.grad.numpy())
    worst = max(errs, key=errs.get)
    print(f"MEASURED input_{backbone} C5={h5}x{w5}: " + ", ".join(f"{k} {v:.3g}" for k, v in errs.items()))
    with_input = _param_grads(fpn)

    # the ten parameter gradients and P2 are the bits of a run without input gradients
    fpn.zero_grad(set_to_none=True)
    plain = fpn([t.cuda() for t in feats])
    assert torch.equal(plain, p2)
    plain.backward(up.cuda())
    for k, a, b in zip(FPN_NAMES, with_input, _param_grads(fpn)):
        assert torch.equal(a, b), f"asking for input gradients changed the bits of {k}"

    # C5 alone: the same dC5 bits, and nothing for the others; an fp16 feature receives an fp16 gradient
    fpn.zero_grad(set_to_none=True)
    only = [t.cuda() for t in feats[:3]] + [feats[3].cuda().requires_grad_(True)]
    fpn(only, input_grad=True).backward(up.cuda())
    assert torch.equal(only[3].grad, xs[3].grad) and all(t.grad is None for t in only[:3])
    for k, a, b in zip(FPN_NAMES, with_input, _param_grads(fpn)):
        assert torch.equal(a, b), f"asking for dC5 alone changed the bits of {k}"
    half = [t.cuda() for t in feats[:2]] + [feats[2].cuda().half().requires_grad_(True), feats[3].cuda()]
    fpn(half, input_grad=True).backward(up.cuda())
    assert half[2].grad.dtype == torch.float16 and torch.equal(half[2].grad, xs[2].grad.half())

    # without the request the call still refuses
    with pytest.raises(RuntimeError, match="backward into the trunk is not built"):
        fpn(xs)
    b = BOUNDS["input_" + backbone]
    assert errs[worst] <= b, f"{worst}: relative error {errs[worst]:.3g} > {b} ({errs})"


@pytest.mark.gpu
def test_input_gradients_bitwise_repeatable_and_scaled(hip):
    """Two runs give the same bits, and an upstream gradient of the loss's own size (~1e-7, below fp16's smallest normal) comes through:
    the operands carry exact power-of-two scales."""
    c5, n, h5, w5 = 512, 2, 5, 4
    gen = torch.Generator().manual_seed(6)
    fpn = _seeded_fpn(c5, 11)
    feats = _taps(n, c5, h5, w5, gen)
    up = torch.randn((n, 256, 8 * h5, 8 * w5), generator=gen)
    runs = []
    for scale in (1.0, 1.0, 2.0 ** -23):
        xs = [t.cuda().requires_grad_(True) for t in feats]
        fpn(xs, input_grad=True).backward(up.cuda() * scale)
        runs.append([x.grad for x in xs])
    for a, b, c in zip(*runs):
        assert torch.equal(a, b)
        assert torch.equal(c, a * 2.0 ** -23), "a power-of-two smaller upstream gradient must give the same bits, scaled"


# ---- BasicBlock training (csrc/resblock_train.hip): the two blocks of ResNet-18's layer4
MAP_CEILING = 2e-3
BLOCK_NAMES = {False: ["conv1.weight", "bn1.weight", "bn1.bias", "conv2.weight", "bn2.weight", "bn2.bias"],
               True: ["conv1.weight", "bn1.weight", "bn1.bias", "conv2.weight", "bn2.weight", "bn2.bias", "downsample.0.weight", "downsample.1.weight",
                      "downsample.1.bias"]}


def _seeded_block(cin, stride, seed):
    blk = nets.BasicBlock(cin, 512, stride)
    blk.load_state_dict(nets.seeded_state_dict(lambda: nets.BasicBlock(cin, 512, stride), seed))
    with torch.no_grad():      # torchvision's zero_init_residual gives gamma = 0; a negative gamma flips the sign of the folded weights
        blk.bn2.weight[3] = 0.0
        blk.bn2.weight[7] = -0.75
    return blk.cuda()


def _ste(w):
    """The folded weight rounded to fp16 as the kernels pack it, straight through: the reference still differentiates the unfolded tensors."""
    return w + (w.half().double() - w).detach()


def _ref_conv_bn(x, conv, bn, stride, pad):
    rstd = 1.0 / torch.sqrt(bn.running_var + bn.eps)
    scale = bn.weight * rstd
    return F.conv2d(x, _ste(conv.weight * scale[:, None, None, None]), None, stride, pad) + (bn.bias - bn.running_mean * scale)[None, :, None, None]


def _ref_block(ref, x):
    """The block in float64 with frozen-statistics BatchNorm, the activation a1 rounded to fp16 as the kernels store it (straight through)."""
    a1 = F.relu(_ref_conv_bn(x, ref.conv1, ref.bn1, ref.stride, 1))
    a1 = a1 + (a1.half().double() - a1).detach()
    idt = x
    if hasattr(ref, "downsample"):
        idt = _ref_conv_bn(x, ref.downsample[0], ref.downsample[1], ref.stride, 0)
        idt = idt + (idt.half().double() - idt).detach()
    return F.relu(_ref_conv_bn(a1, ref.conv2, ref.bn2, 1, 1) + idt)


def _block_case(blk, cin, stride, size, want_dx):
    h, w = size
    gen = torch.Generator().manual_seed(7 * h + w)
    x = (torch.randn((2, cin, h * stride, w * stride), generator=gen) * 0.5).half().float()
    up = torch.randn((2, 512, h, w), generator=gen)
    ref = copy.deepcopy(blk).to(device="cpu", dtype=torch.float64)
    stats_before = [b.detach().clone() for b in blk.buffers()]
    xr = x.double().requires_grad_(want_dx)
    yr = _ref_block(ref, xr)
    xg = x.cuda().requires_grad_(want_dx)
    y = blk.train()(xg)
    assert y.shape == (2, 512, h, w) and y.dtype == torch.float32
    agree = ((y.detach().cpu() > 0) == (yr.detach() > 0)).float()
    yr.backward(up.double())
    y.backward(up.cuda())
    assert all(torch.equal(a, b) for a, b in zip(stats_before, blk.buffers())), "frozen statistics were written"
    names = BLOCK_NAMES[hasattr(blk, "downsample")]
    got, want = dict(blk.named_parameters()), dict(ref.named_parameters())
    errs = {k: _rel(got[k].grad.double().cpu().numpy(), want[k].grad.numpy()) for k in names}
    e_y = _rel(y.detach().double().cpu().numpy(), yr.detach().numpy())
    e_dx = _rel(xg.grad.double().cpu().numpy(), xr.grad.numpy()) if want_dx else None
    return e_y, errs, e_dx, float(agree.mean())


BLOCK_BOUNDS = {
    # 3x the level measured on an MI355X, worst of the three sizes (and of the six / nine parameter gradients: conv1.weight)
    "stride1": {"y": 6.3e-4, "grad": 9.5e-4, "dx": 1.4e-4},    # measured 2.08e-4, 3.14e-4, 4.65e-5
    "stride2": {"y": 6.3e-4, "grad": 9.6e-4},                  # 2.07e-4, 3.18e-4
}


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(3, 2), (1, 1), (5, 4)])
def test_stride1_block_against_fp64(hip, size):
    blk = _seeded_block(512, 1, 21)
    e_y, errs, e_dx, agree = _block_case(blk, 512, 1, size, True)
    worst = max(errs, key=errs.get)
    print(f"MEASURED stride1 {size[0]}x{size[1]}: y {e_y:.3g}, grad {errs[worst]:.3g} ({worst}), dx {e_dx:.3g}, sign agreement {agree:.5f}; {errs}")
    assert agree > 0.99      # the two outputs agree about the ReLU signs (measured: everywhere)
    b = BLOCK_BOUNDS["stride1"]
    assert e_y <= b["y"] and errs[worst] <= b["grad"] and e_dx <= b["dx"], (e_y, errs, e_dx)


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(3, 2), (1, 1), (5, 4)])
def test_stride2_block_against_fp64(hip, size):
    blk = _seeded_block(256, 2, 22)
    e_y, errs, _, agree = _block_case(blk, 256, 2, size, False)
    worst = max(errs, key=errs.get)
    print(f"MEASURED stride2 {size[0]}x{size[1]}: y {e_y:.3g}, grad {errs[worst]:.3g} ({worst}), sign agreement {agree:.5f}; {errs}")
    assert agree > 0.99 and len(errs) == 9
    with pytest.raises(RuntimeError, match="stride-2 block"):
        blk(torch.zeros((1, 256, 2, 2), device="cuda", requires_grad=True))
    with pytest.raises(RuntimeError, match="layer4 only"):
        nets.BasicBlock(128, 256, 2).cuda()(torch.zeros((1, 128, 2, 2), device="cuda"))
    b = BLOCK_BOUNDS["stride2"]
    assert e_y <= b["y"] and errs[worst] <= b["grad"], (e_y, errs)


@pytest.mark.gpu
def test_block_bitwise_repeatable(hip):
    blk = _seeded_block(512, 1, 23)
    gen = torch.Generator().manual_seed(1)
    x = (torch.randn((2, 512, 5, 4), generator=gen) * 0.5).half().float().cuda()
    up = torch.randn((2, 512, 5, 4), generator=gen).cuda()
    runs = []
    for _ in range(2):
        blk.zero_grad(set_to_none=True)
        xg = x.clone().requires_grad_(True)
        y = blk(xg)
        y.backward(up)
        runs.append([y.detach(), xg.grad] + [p.grad.clone() for p in blk.parameters()])
    assert len(runs[0]) == 8 and all(torch.equal(a, b) for a, b in zip(*runs))


# ---- layer4 -> FPN -> head -> HIP loss on padded taps, and the product path
import test_gpu_fpn_neck_train as neck  # noqa: E402  (the head / FPN reference helpers of the stage before)

from vtd_amd import training  # noqa: E402

# worst gradient per stage, C5 = 3x2, n = 2: measured 4.93e-3 (layer4, 1.bn1.bias), 6.69e-3 (FPN, layer_blocks.3.bias), 2.66e-3 (head,
# probability_head.0.weight).  3x the first two is over the ceiling: their bound is the ceiling.  The levels are several times those of
# the FPN -> head chain of tests/test_gpu_fpn_neck_train.py (7.7e-4, 4.0e-4), whose C5 is random instead of a ReLU output; not decomposed
CHAIN_BOUNDS = {"layer4": GRAD_CEILING, "fpn": GRAD_CEILING, "head": 8.0e-3}
L4_NAMES = [f"0.{k}" for k in BLOCK_NAMES[True]] + [f"1.{k}" for k in BLOCK_NAMES[False]]


def _seeded_layer4(seed):
    l4 = torch.nn.Sequential(_seeded_block(256, 2, seed), _seeded_block(512, 1, seed + 1))
    return l4.cuda()


def _chain_setup():
    n, h5, w5 = 2, 3, 2
    gen = torch.Generator().manual_seed(37)
    l4, fpn, head = _seeded_layer4(31), _seeded_fpn(512, 6), neck._seeded_head(8).train()
    feats = _taps(n, 512, h5, w5, gen)[:3]
    targets = neck._random_targets((n, 1, 32 * h5, 32 * w5), gen)
    padded = [nets.pack_tap(t.cuda()) for t in feats]
    return l4, fpn, head, feats, targets, padded


def _chain_step(l4, fpn, head, padded, targets):
    out = fpn.forward_padded(padded, head=head, layer4=l4)
    out["probability"].retain_grad()
    out["threshold"].retain_grad()
    training.detection_loss(out, {k: v.cuda() for k, v in targets.items()})["loss"].backward()
    return out, (out["probability"].grad, out["threshold"].grad)


@pytest.mark.gpu
def test_chain_layer4_fpn_head_loss_against_fp64(hip):
    """Stage-isolated at C5 and P2: the reference head reads the P2 the kernels stored, the reference FPN the C5 they
    stored; the gradient chain is end to end: the reference layer4's upstream gradient is the reference FPN's dC5."""
    l4, fpn, head, feats, targets, padded = _chain_setup()
    rl4 = copy.deepcopy(l4).to(device="cpu", dtype=torch.float64)
    rfpn, rhead = _rounded_fpn(fpn), neck._rounded_head(head).train()
    out, ups = _chain_step(l4, fpn, head, padded, targets)
    c5p = nets.forward_layer4_padded(l4, padded[2])
    p2p = fpn.forward_padded(padded + [c5p])
    # reference, back to front
    x = p2p[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).double().cpu().contiguous().requires_grad_(True)
    torch.autograd.backward([rhead.probability_head(x), rhead.threshold_head(x)], [u.double().cpu() for u in ups])
    c5 = c5p[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).double().cpu().contiguous().requires_grad_(True)
    _wiring(rfpn, [t.double() for t in feats] + [c5]).backward(x.grad)
    mid = _ref_block(rl4[0], feats[2].double())
    mid = mid + (mid.half().double() - mid).detach()
    _ref_block(rl4[1], mid).backward(c5.grad)
    got, want = dict(l4.named_parameters()), dict(rl4.named_parameters())
    le = {k: _rel(got[k].grad.double().cpu().numpy(), want[k].grad.numpy()) for k in L4_NAMES}
    fe, he = neck._fpn_errors(fpn, rfpn), neck._head_errors(head, rhead)
    assert len(le) == 15 and len(fe) == 10 and len(he) == 20
    wl, wf, wh = max(le, key=le.get), max(fe, key=fe.get), max(he, key=he.get)
    print(f"MEASURED chain: layer4 grad {le[wl]:.3g} ({wl}), fpn grad {fe[wf]:.3g} ({wf}), head grad {he[wh]:.3g} ({wh}); {le}")
    assert le[wl] <= CHAIN_BOUNDS["layer4"], le
    assert fe[wf] <= CHAIN_BOUNDS["fpn"], fe
    assert he[wh] <= CHAIN_BOUNDS["head"], he


@pytest.mark.gpu
def test_chain_bitwise_repeatable(hip):
    l4, fpn, head, feats, targets, padded = _chain_setup()
    state = copy.deepcopy(head.state_dict())
    runs = []
    for _ in range(2):
        head.load_state_dict(state)
        for m in (l4, fpn, head):
            m.zero_grad(set_to_none=True)
        out, _ = _chain_step(l4, fpn, head, padded, targets)
        runs.append([out["probability"].detach(), out["threshold"].detach()] + [p.grad.clone() for p in l4.parameters()] +
                    [p.grad.clone() for p in fpn.live_parameters()] + [p.grad.clone() for p in head.parameters()])
    assert len(runs[0]) == 47
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_product_head_fpn_layer4_training_step(hip):
    from vtd_amd._fixtures.weights import stress_detector_state_dict
    torch.manual_seed(3)
    net = nets.DBNet("resnet18", compute_threshold=True, trainable="head+fpn+layer4")
    net.load_state_dict(stress_detector_state_dict("resnet18", 17))
    net.cuda().train()
    gen = torch.Generator().manual_seed(23)
    x = torch.randn((2, 3, 640, 640), generator=gen).cuda()
    targets = neck._random_targets((2, 1, 640, 640), gen)
    te = net.trunk_engine()
    stats = {k: v.detach().clone() for k, v in net.backbone[7].state_dict().items() if "running" in k or "num_batches" in k}
    assert len(stats) == 15
    mod = training.TextDetectionLightningModule(net)
    opt = mod.configure_optimizers()["optimizer"]
    loss = mod.training_step((x, targets), 0)
    opt.zero_grad()
    loss.backward()
    l4 = dict(net.backbone[7].named_parameters())
    assert len(l4) == 15
    for k, p in l4.items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, f"backbone.7.{k}"
    for i in range(7):
        assert all(p.grad is None for p in net.backbone[i].parameters())
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    opt.step()
    after = net.state_dict()
    for k in l4:
        assert not torch.equal(before["backbone.7." + k], after["backbone.7." + k]), f"backbone.7.{k} did not change"
    for k in before:
        if k.startswith("backbone.") and not k.startswith("backbone.7."):
            assert torch.equal(before[k], after[k]), f"{k} changed"
    assert net.trunk_engine() is te, "an optimizer step on layer4 / FPN / head weights rebuilt the trunk engine"
    for k, v in stats.items():
        assert torch.equal(v, net.backbone[7].state_dict()[k]), f"layer4's {k} was written"
    # a second step runs on the stepped layer4 weights (folded on the device in every call), on the same engine
    loss2 = mod.training_step((x, targets), 1)
    assert bool(torch.isfinite(loss2)) and float(loss2) != float(loss)
    # a following eval() forward runs the fused inference engine on the stepped weights
    net.eval()
    with torch.no_grad():
        got = net(x)
    fresh = nets.DBNet("resnet18", compute_threshold=True)
    fresh.load_state_dict(net.state_dict())
    with torch.no_grad():
        want = fresh.cuda().eval()(x)
    assert torch.equal(got["probability"], want["probability"]) and torch.equal(got["threshold"], want["threshold"])
