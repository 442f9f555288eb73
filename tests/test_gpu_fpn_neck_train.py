"""FPN training on the HIP kernels (csrc/fpn_train.hip) on the GPU: `fpn([C2, C3, C4, C5])` stand-alone, the FPN -> DB head chain under the
HIP loss, and the product path DBNet(trainable="head+fpn").

The fp64 reference is the module's own wiring (L5 = inner_blocks[0](C5), L(k) = inner_blocks[5-k](C(k)) + nearest-2x(L(k+1)),
P2 = layer_blocks[3](L2)) under CPU autograd in float64, fed the taps rounded to fp16, the GEMM weights rounded to fp16 as the kernels pack
them, and the same upstream gradient.  Metric: relative L2 error per tensor.  Bounds are per case, DESIGN.md section 4's convention: 3x the
level measured on an MI355X, under the ceilings of 2e-3 for the forward map and 1e-2 for gradients."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vtd_amd import nets, training

MAP_CEILING = 2e-3
GRAD_CEILING = 1e-2
# case -> bounds on the relative L2 error ("Bounds of tests/test_gpu_fpn_neck_train.py"); measured values behind each
BOUNDS = {
    "alone_resnet18": {"p2": 1.2e-3, "grad": 1.2e-3},    # measured 3.86e-4, 3.90e-4 (worst of the three sizes and the ten tensors)
    "alone_resnet50": {"p2": 1.2e-3, "grad": 1.2e-3},    # 3.92e-4, 3.87e-4
    "chain_resnet18": {"fpn": 2.4e-3, "head": 1.3e-3},   # 7.70e-4 (layer_blocks.3.bias), 4.04e-4; stage-isolated at P2 (_reference_chain)
    "chain_resnet50": {"fpn": 3.1e-3, "head": 1.2e-3},   # 1.02e-3 (layer_blocks.3.bias), 3.87e-4
    "imbalanced": {"fpn": 1e-2},                         # 4.25e-3 with the threshold map's gradient alone (3x is over the ceiling); both 6.58e-4, swapped 1.64e-3
    "b32": {"fpn": 2.8e-3, "head": 4.3e-4},              # 9.08e-4 (inner_blocks.3.bias), 1.41e-4
}
assert all(v <= (MAP_CEILING if k == "p2" else GRAD_CEILING) for b in BOUNDS.values() for k, v in b.items())

PLANS = {"resnet18": 512, "resnet50": 2048}
FPN_NAMES = [f"inner_blocks.{i}.weight" for i in range(4)] + [f"inner_blocks.{i}.bias" for i in range(4)] + ["layer_blocks.3.weight", "layer_blocks.3.bias"]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _seeded_fpn(c5, seed):
    fpn = nets.FeaturePyramidNetwork(c5)
    fpn.load_state_dict(nets.seeded_state_dict(lambda: nets.FeaturePyramidNetwork(c5), seed))
    return fpn.cuda()


def _seeded_head(seed):
    head = nets.DBHead(256)
    head.load_state_dict(nets.seeded_state_dict(lambda: nets.DBHead(256), seed))
    return head.cuda()


def _rounded_fpn(fpn, dtype=torch.float64, device="cpu"):
    """A copy of `fpn` with the GEMM weights rounded to fp16 as the kernels pack them (biases stay fp32 values)."""
    ref = copy.deepcopy(fpn).to(device=device, dtype=dtype)
    with torch.no_grad():
        for m in list(ref.inner_blocks) + [ref.layer_blocks[3]]:
            m.weight.copy_(m.weight.half().to(dtype))
    return ref


def _rounded_head(head, dtype=torch.float64, device="cpu"):
    ref = copy.deepcopy(head).to(device=device, dtype=dtype)
    with torch.no_grad():
        for seq in (ref.probability_head, ref.threshold_head):
            for i in (0, 3):
                seq[i].weight.copy_(seq[i].weight.half().to(dtype))
    return ref


def _wiring(fpn, feats):
    """The reference wiring in torch ops on [C2, C3, C4, C5]."""
    last = fpn.inner_blocks[0](feats[3])
    for i in range(1, 4):
        last = fpn.inner_blocks[i](feats[3 - i]) + F.interpolate(last, scale_factor=2, mode="nearest")
    return fpn.layer_blocks[3](last)


def _taps(n, c5, h5, w5, gen, device="cpu"):
    """Random taps C2..C5 with fp16-representable values."""
    return [(torch.randn((n, c5 >> (3 - lv), h5 << (3 - lv), w5 << (3 - lv)), generator=gen, device=device) * 0.5).half().float() for lv in range(4)]


def _fpn_grads(fpn):
    sd = dict(fpn.named_parameters())
    return {k: sd[k].grad for k in FPN_NAMES}


def _fpn_errors(fpn, ref):
    got, want = _fpn_grads(fpn), _fpn_grads(ref)
    return {k: _rel(got[k].detach().double().cpu().numpy(), want[k].detach().double().cpu().numpy()) for k in FPN_NAMES}


def _head_errors(head, ref, training_mode=True):
    """As tests/test_gpu_dbhead_train.py: the bias in front of a train-mode BatchNorm has an exactly-zero gradient in exact arithmetic; its
    error is taken relative to the following BatchNorm's beta gradient (the same sum of dy)."""
    errs = {}
    for br in ("probability_head", "threshold_head"):
        hs, rs = getattr(head, br), getattr(ref, br)
        for i, attr in ((0, "weight"), (0, "bias"), (1, "weight"), (1, "bias"), (3, "weight"), (3, "bias"), (4, "weight"), (4, "bias"),
                        (6, "weight"), (6, "bias")):
            g = getattr(hs[i], attr).grad.detach().double().cpu().numpy()
            r = getattr(rs[i], attr).grad.detach().double().cpu().numpy()
            if training_mode and attr == "bias" and i in (0, 3):
                nxt = getattr(rs[i + 1], "bias").grad.detach().double().cpu().numpy()
                errs[f"{br}.{i}.{attr}"] = float(np.linalg.norm(g - r) / max(np.linalg.norm(nxt), 1e-300))
            else:
                errs[f"{br}.{i}.{attr}"] = _rel(g, r)
    return errs


def _random_targets(shape, gen, device="cpu"):
    return {"probability_map": (torch.rand(shape, generator=gen, device=device) > 0.7).float(),
            "threshold_map": torch.rand(shape, generator=gen, device=device) * 0.6 + 0.2}


def _reference_chain(rfpn, rhead, feats, p2_padded, ups):
    """Backward of the reference chain under the upstream map gradients `ups`, stage-isolated at P2 as the head's own product test is
    (tests/test_gpu_dbhead_train.py: "the engine's own P2"): the reference head reads the P2 the kernels stored (fp16), its input gradient
    is the reference wiring's upstream gradient.  The gradient chain is end to end; only the activations are isolated.  Without the
    isolation the train-mode BatchNorm backward at n = 2 turns the fp16 storage of P2 (3.9e-4 relative, the `alone` cases) into 2.7e-2 on
    every one of the 30 gradients, the head's own included although their bits are those of head.forward_padded (measured on an MI355X):
    that is the sensitivity of the loss to its input, not an error of either backward."""
    ref_p = next(rfpn.parameters())
    x = p2_padded[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).to(device=ref_p.device, dtype=ref_p.dtype).contiguous().requires_grad_(True)
    torch.autograd.backward([rhead.probability_head(x), rhead.threshold_head(x)], [u.to(device=ref_p.device, dtype=ref_p.dtype) for u in ups])
    _wiring(rfpn, [t.to(device=ref_p.device, dtype=ref_p.dtype) for t in feats]).backward(x.grad)


def _chain_step(fpn, head, padded_taps, targets):
    """FPN -> head on the HIP kernels + the HIP loss + backward; returns (maps, the upstream map gradients)."""
    out = fpn.forward_padded(padded_taps, head=head)
    out["probability"].retain_grad()
    out["threshold"].retain_grad()
    training.detection_loss(out, {k: v.cuda() for k, v in targets.items()})["loss"].backward()
    return out, (out["probability"].grad, out["threshold"].grad)


# ---- the FPN alone
@pytest.mark.gpu
@pytest.mark.parametrize("size", [(3, 2), (1, 1), (5, 4)])
@pytest.mark.parametrize("backbone", sorted(PLANS))
def test_fpn_alone_against_fp64(hip, backbone, size):
    c5, (h5, w5), n = PLANS[backbone], size, 2
    gen = torch.Generator().manual_seed(17 + h5)
    fpn = _seeded_fpn(c5, 3 + w5)
    ref = _rounded_fpn(fpn)
    feats = _taps(n, c5, h5, w5, gen)
    up = torch.randn((n, 256, 8 * h5, 8 * w5), generator=gen)
    p2 = fpn([t.cuda() for t in feats])
    assert p2.shape == (n, 256, 8 * h5, 8 * w5) and p2.dtype == torch.float32 and p2.requires_grad
    p2.backward(up.cuda())
    want = _wiring(ref, [t.double() for t in feats])
    want.backward(up.double())
    e_p2 = _rel(p2.detach().double().cpu().numpy(), want.detach().numpy())
    errs = _fpn_errors(fpn, ref)
    worst = max(errs, key=errs.get)
    print(f"MEASURED alone_{backbone} C5={h5}x{w5}: p2 {e_p2:.3g}, grad {errs[worst]:.3g} ({worst})")
    for i in range(3):   # dead blocks: no gradient, as torch autograd leaves it
        assert fpn.layer_blocks[i].weight.grad is None and fpn.layer_blocks[i].bias.grad is None
        assert ref.layer_blocks[i].weight.grad is None
    # fp16 features give the same bits as their fp32 copies
    fpn.zero_grad(set_to_none=True)
    p2h = fpn([t.cuda().half() for t in feats])
    assert torch.equal(p2h, p2)
    b = BOUNDS["alone_" + backbone]
    assert e_p2 <= b["p2"], f"P2 relative error {e_p2:.3g} > {b['p2']}"
    assert errs[worst] <= b["grad"], f"gradient of {worst}: relative error {errs[worst]:.3g} > {b['grad']} ({errs})"


# ---- FPN -> head -> HIP loss
@pytest.mark.gpu
@pytest.mark.parametrize("backbone", sorted(PLANS))
def test_chain_with_head_and_loss_against_fp64(hip, backbone):
    c5, n, h5, w5 = PLANS[backbone], 2, 3, 2
    gen = torch.Generator().manual_seed(29)
    fpn, head = _seeded_fpn(c5, 6), _seeded_head(8).train()
    plain = copy.deepcopy(head)   # the same head on the same padded P2 through forward_padded: the yardstick bits
    rfpn, rhead = _rounded_fpn(fpn), _rounded_head(head).train()
    feats = _taps(n, c5, h5, w5, gen)
    targets = _random_targets((n, 1, 32 * h5, 32 * w5), gen)
    padded = [nets.pack_tap(t.cuda()) for t in feats]
    out, ups = _chain_step(fpn, head, padded, targets)
    p2_padded = fpn.forward_padded(padded)
    _reference_chain(rfpn, rhead, feats, p2_padded, ups)
    fe, he = _fpn_errors(fpn, rfpn), _head_errors(head, rhead)
    wf, wh = max(fe, key=fe.get), max(he, key=he.get)
    print(f"MEASURED chain_{backbone}: fpn grad {fe[wf]:.3g} ({wf}), head grad {he[wh]:.3g} ({wh})")
    assert all(fpn.layer_blocks[i].weight.grad is None for i in range(3))
    # the FPN path does not disturb the head's bits
    o2 = plain.forward_padded(p2_padded, 8 * h5, 8 * w5)
    training.detection_loss(o2, {k: v.cuda() for k, v in targets.items()})["loss"].backward()
    assert torch.equal(o2["probability"], out["probability"]) and torch.equal(o2["threshold"], out["threshold"])
    got, want = [p.grad for p in head.parameters()], [p.grad for p in plain.parameters()]
    assert len(got) == 20 and all(torch.equal(a, b) for a, b in zip(got, want)), "the chained path changed a head gradient's bits"
    assert all(torch.equal(a, b) for a, b in zip(head.buffers(), plain.buffers()))
    b = BOUNDS["chain_" + backbone]
    assert fe[wf] <= b["fpn"], f"gradient of {wf}: {fe[wf]:.3g} > {b['fpn']} ({fe})"
    assert he[wh] <= b["head"], f"gradient of {wh}: {he[wh]:.3g} > {b['head']} ({he})"


@pytest.mark.gpu
def test_upstream_gradients_of_very_different_size(hip):
    """The threshold map's upstream gradient 2^-10 of the probability map's (the `imbalanced` case of tests/test_gpu_fpn_train.py): dP2
    arrives with the head's common scale and the FPN's own scales must carry it on."""
    c5, n, h5, w5 = 512, 2, 3, 2
    gen = torch.Generator().manual_seed(31)
    fpn, head = _seeded_fpn(c5, 12), _seeded_head(13).train()
    rfpn, rhead = _rounded_fpn(fpn), _rounded_head(head).train()
    feats = _taps(n, c5, h5, w5, gen)
    padded = [nets.pack_tap(t.cuda()) for t in feats]
    gp = torch.randn((n, 1, 32 * h5, 32 * w5), generator=gen) * 1e-4
    gt = torch.randn((n, 1, 32 * h5, 32 * w5), generator=gen) * 1e-4 / 1024
    worst = {}
    for name, ups in (("both", (gp, gt)), ("threshold only", (torch.zeros_like(gp), gt)), ("swapped", (gt, gp))):
        f, h, rf, rh = (copy.deepcopy(m) for m in (fpn, head, rfpn, rhead))
        out = f.forward_padded(padded, head=h)
        torch.autograd.backward([out["probability"], out["threshold"]], [ups[0].cuda(), ups[1].cuda()])
        _reference_chain(rf, rh, feats, f.forward_padded(padded), ups)
        errs = _fpn_errors(f, rf)
        worst[name] = max(errs.values())
    print("MEASURED imbalanced: fpn grad " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) <= BOUNDS["imbalanced"]["fpn"], worst


@pytest.mark.gpu
def test_b32_product_shape_matches_torch_gpu_fp32(hip):
    """B = 32 at the product shape (C5 20x20, ResNet-18 channels) with the loss's own ~1e-7 upstream gradients, against torch GPU fp32
    autograd of the same FPN + head: fp16 operands without the exact scales would flush them."""
    c5, n, h5, w5 = 512, 32, 20, 20
    gen = torch.Generator(device="cuda").manual_seed(99)
    fpn, head = _seeded_fpn(c5, 40), _seeded_head(41).train()
    rfpn, rhead = _rounded_fpn(fpn, torch.float32, "cuda"), _rounded_head(head, torch.float32, "cuda").train()
    feats = _taps(n, c5, h5, w5, gen, device="cuda")
    targets = _random_targets((n, 1, 640, 640), gen, device="cuda")
    padded = [nets.pack_tap(t) for t in feats]
    out, ups = _chain_step(fpn, head, padded, targets)
    assert float(ups[0].abs().median()) < 1e-6   # most upstream gradients are below fp16's smallest normal (6.1e-5)
    _reference_chain(rfpn, rhead, feats, fpn.forward_padded(padded), ups)
    fe, he = _fpn_errors(fpn, rfpn), _head_errors(head, rhead)
    wf, wh = max(fe, key=fe.get), max(he, key=he.get)
    print(f"MEASURED b32: fpn grad {fe[wf]:.3g} ({wf}), head grad {he[wh]:.3g} ({wh})")
    for k, g in list(_fpn_grads(fpn).items()) + [(k, p.grad) for k, p in head.named_parameters()]:
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, f"{k}: the gradient is all zeros or not finite"
    assert fe[wf] <= BOUNDS["b32"]["fpn"], fe
    assert he[wh] <= BOUNDS["b32"]["head"], he


@pytest.mark.gpu
def test_bitwise_repeatable(hip):
    c5, n, h5, w5 = 512, 2, 5, 4
    gen = torch.Generator().manual_seed(2)
    fpn, head = _seeded_fpn(c5, 9), _seeded_head(9).train()
    state = copy.deepcopy(head.state_dict())
    padded = [nets.pack_tap(t.cuda()) for t in _taps(n, c5, h5, w5, gen)]
    targets = _random_targets((n, 1, 32 * h5, 32 * w5), gen)
    runs = []
    for _ in range(2):
        head.load_state_dict(state)
        head.zero_grad(set_to_none=True)
        fpn.zero_grad(set_to_none=True)
        _chain_step(fpn, head, padded, targets)
        runs.append([fpn.forward_padded(padded)] + [g.detach().clone() for g in _fpn_grads(fpn).values()] + [p.grad.detach().clone() for p in head.parameters()])
    assert len(runs[0]) == 31
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- the product path
@pytest.mark.gpu
@pytest.mark.parametrize("backbone,batch", [("resnet18", 2), ("resnet50", 1)])
def test_product_head_fpn_training_step(hip, backbone, batch):
    from vtd_amd._fixtures.weights import stress_detector_state_dict
    torch.manual_seed(3)
    sd = stress_detector_state_dict(backbone, 17)
    net = nets.DBNet(backbone, compute_threshold=True, trainable="head+fpn")
    net.load_state_dict(sd)
    net.cuda().train()
    gen = torch.Generator().manual_seed(23)
    x = torch.randn((batch, 3, 640, 640), generator=gen).cuda()
    targets = _random_targets((batch, 1, 640, 640), gen)
    # forward_trunk hands out the engine's own taps
    te = net.trunk_engine()
    taps = te.forward_trunk(x)
    for lv, t in enumerate(taps):
        want = te.read_tap(f"c{lv + 2}", batch)
        assert t.shape == (batch, want.shape[2] + 2, want.shape[3] + 2, want.shape[1]) and t.dtype == torch.float16
        assert np.array_equal(t[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).float().cpu().numpy(), want)
        assert float(t[:, 0].abs().max()) == 0 and float(t[:, :, -1].abs().max()) == 0

    mod = training.TextDetectionLightningModule(net)
    opt = mod.configure_optimizers()["optimizer"]
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    loss = mod.training_step((x, targets), 0)
    opt.zero_grad()
    loss.backward()
    assert all(p.grad is None for p in net.backbone.parameters())
    opt.step()
    after = net.state_dict()
    live = {"fpn." + k for k in FPN_NAMES} | {"head." + k for k, _ in net.head.named_parameters()}
    assert len(live) == 30
    for k in before:
        if k in live:
            assert not torch.equal(before[k], after[k]), f"{k} did not change"
        elif k.startswith("backbone.") or k.startswith("fpn."):
            assert torch.equal(before[k], after[k]), f"{k} changed"
    assert net.trunk_engine() is te, "an optimizer step on FPN / head weights rebuilt the trunk engine"
    # a following eval() forward runs the fused inference engine on the stepped weights
    net.eval()
    with torch.no_grad():
        got = net(x)
    fresh = nets.DBNet(backbone, compute_threshold=True)
    fresh.load_state_dict(net.state_dict())
    with torch.no_grad():
        want = fresh.cuda().eval()(x)
    assert torch.equal(got["probability"], want["probability"]) and torch.equal(got["threshold"], want["threshold"])
    # "head" mode on the same weights still refuses an FPN parameter that requires grad
    old = nets.DBNet(backbone, compute_threshold=True, trainable="head")
    old.load_state_dict(sd)
    old.fpn.inner_blocks[0].weight.requires_grad_(True)
    old.cuda().train()
    with pytest.raises(RuntimeError, match="requires grad"):
        old(x)
