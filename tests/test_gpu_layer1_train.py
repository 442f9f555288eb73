"""Training ResNet-18's layer1 on the GPU (csrc/resblock_train.hip: the 64-wide block behind vtd_block64_train_*, csrc/wgrad_mfma.h: MODE 5):
the block (64 -> 64, stride 1) through `nets.basic_block_train` at four sizes, the last the smallest multi-slab one, its bit checks,
`DetectorEngine.forward_pool`, the chain layer1 -> layer2 -> layer3 -> layer4 -> FPN -> head -> HIP loss on a padded pool tap, and the product
mode "head+fpn+layer4+layer3+layer2+layer1".

The fp64 references are CPU autograd of the same wiring, built like tests/test_gpu_layer4_train.py's `_ref_block`: folded weights and stored
activations rounded to fp16, straight through, frozen statistics.  Metric: relative L2 error per tensor, as tests/test_gpu_layer3_train.py.
Bounds follow DESIGN.md section 4's convention: 3x the level measured on an MI355X, never above the ceilings (2e-3 for maps, 1e-2 for
gradients); the measured values stand beside them."""
import copy

import numpy as np
import pytest
import torch

import test_gpu_fpn_neck_train as neck
import test_gpu_layer3_train as l3t
import test_gpu_layer4_train as l4t
import test_layer1_train as l1c
from vtd_amd import nets, training
from vtd_amd.nets import forward_layer1_padded  # noqa: F401  (the feature under test: absent before it)

MAP_CEILING, GRAD_CEILING = 2e-3, 1e-2
CIN, WIDTH, STRIDE = 64, 64, 1
# n = 2.  23 x 23 is the smallest multi-slab case: 1058 rows make two slabs under the rule min(ceil(512 / 5), ceil(rows / 1024)) -- 544 rows
# (529 rounded up to the 32-row chunk) and a last slab of 514, which ends inside a chunk.  The reduce has ceil(1058 / 256) = 5 partials of 212
# rows (four quarters of 53), the last of 210; the convolutions have 9 tiles of 128 rows
SIZES = [(1, 1), (3, 2), (5, 4), (23, 23)]
LARGE = (23, 23)
# bounds on y, the worst parameter gradient and dx: 3x the worst of the four sizes measured on an MI355X: 2.38e-4 (1x1), 3.54e-4 (bn1.weight,
# 1x1; 3.04e-4 at 23x23), 5.87e-5 (23x23).  No ReLU-mask element differs from the reference's at any of the four sizes (67 712 at 23x23), so
# unlike the 128-wide block's the multi-slab size sits at the level of the small ones
BLOCK_BOUNDS = {"y": 7.2e-4, "grad": 1.1e-3, "dx": 1.8e-4}
# worst gradient per stage of the chain at C5 = 3x2, n = 2: measured 4.00e-3 (layer1, 0.bn2.bias), 8.49e-3 (layer2, 1.bn1.bias), 6.93e-4 (layer3,
# 0.downsample.1.weight), 6.34e-4 (layer4, 0.downsample.0.weight), 5.93e-4 (FPN, inner_blocks.0.weight), 4.16e-4 (head,
# probability_head.0.weight).  3x the first two exceeds the ceiling the layer2 chain uses, so the ceiling is their bound.  One ReLU-mask element
# of C2 (of 49 152) differs from the reference's, none of C3.  layer2.0's dx is 0.40 of dC2's norm, the FPN's dC2 0.92
CHAIN_BOUNDS = {"layer1": GRAD_CEILING, "layer2": GRAD_CEILING, "layer3": 2.1e-3, "layer4": 1.9e-3, "fpn": 1.8e-3, "head": 1.3e-3}
assert BLOCK_BOUNDS["y"] <= MAP_CEILING and BLOCK_BOUNDS["grad"] <= GRAD_CEILING and BLOCK_BOUNDS["dx"] <= GRAD_CEILING
assert all(v <= GRAD_CEILING for v in CHAIN_BOUNDS.values())

_rel, _ref_block, BLOCK_NAMES = l4t._rel, l4t._ref_block, l4t.BLOCK_NAMES
_seeded_block, _inputs, _param_grads, _unpad, _rounded = l3t._seeded_block, l3t._inputs, l3t._param_grads, l3t._unpad, l3t._rounded
MODE = "head+fpn+layer4+layer3+layer2+layer1"

_REFS = {}


def _reference(size):
    """(block, x, up, reference y, reference parameter gradients, reference dx), computed once per size."""
    if size not in _REFS:
        blk = _seeded_block(CIN, WIDTH, STRIDE, 101)
        x, up = _inputs(CIN, WIDTH, STRIDE, size)
        ref = copy.deepcopy(blk).to(device="cpu", dtype=torch.float64)
        xr = x.double().requires_grad_(True)
        yr = _ref_block(ref, xr)
        yr.backward(up.double())
        want = dict(ref.named_parameters())
        _REFS[size] = (blk, x, up, yr.detach(), {k: want[k].grad.clone() for k in BLOCK_NAMES[False]}, xr.grad.clone())
    return _REFS[size]


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_block_against_fp64(hip, size):
    blk, x, up, yr, gr, dxr = _reference(size)
    assert float(blk.bn2.weight[3].detach()) == 0.0 and float(blk.bn2.weight[7].detach()) < 0      # a gamma = 0 channel and a gamma < 0 channel
    blk.zero_grad(set_to_none=True)
    stats_before = [b.detach().clone() for b in blk.buffers()]
    xg = x.cuda().requires_grad_(True)
    y = nets.basic_block_train(blk.train(), xg)
    assert y.shape == (2, WIDTH, *size) and y.dtype == torch.float32 and y.requires_grad
    y.backward(up.cuda())
    assert all(torch.equal(a, b) for a, b in zip(stats_before, blk.buffers())), "frozen statistics were written"
    assert xg.grad is not None and xg.grad.shape == x.shape and bool(torch.isfinite(xg.grad).all()) and float(xg.grad.abs().max()) > 0
    got = dict(blk.named_parameters())
    errs = {k: _rel(got[k].grad.double().cpu().numpy(), gr[k].numpy()) for k in gr}
    assert len(errs) == 6      # every learnable tensor of the block (the stage's two blocks have 12)
    e_y = _rel(y.detach().double().cpu().numpy(), yr.numpy())
    e_dx = _rel(xg.grad.double().cpu().numpy(), dxr.numpy())
    differ = int(((y.detach().cpu() > 0) != (yr > 0)).sum())
    agree = 1.0 - differ / yr.numel()
    worst = max(errs, key=errs.get)
    print(f"MEASURED block l1 {size[0]}x{size[1]}: y {e_y:.3g}, grad {errs[worst]:.3g} ({worst}), dx {e_dx:.3g}, sign agreement {agree:.5f} "
          f"({differ} of {yr.numel()} mask elements differ); {errs}")
    assert agree > 0.99
    assert e_y <= BLOCK_BOUNDS["y"] and errs[worst] <= BLOCK_BOUNDS["grad"] and e_dx <= BLOCK_BOUNDS["dx"], (e_y, errs, e_dx)


@pytest.mark.gpu
def test_block_bit_checks(hip):
    """At the multi-slab size: two runs give the same bits; the parameter gradients are the same bits with and without dx; an upstream
    gradient smaller by 2^-23 gives the same dx bits, scaled."""
    blk = _seeded_block(CIN, WIDTH, STRIDE, 103)
    x, up = _inputs(CIN, WIDTH, STRIDE, LARGE)
    runs = []
    for scale, want_dx in ((1.0, True), (1.0, True), (2.0 ** -23, True), (1.0, False)):
        blk.zero_grad(set_to_none=True)
        xg = x.cuda().requires_grad_(want_dx)
        y = nets.basic_block_train(blk, xg)
        y.backward(up.cuda() * scale)
        assert (xg.grad is not None) == want_dx
        runs.append([y.detach(), xg.grad] + _param_grads(blk))
    assert len(runs[0]) == 2 + 6
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
    assert torch.equal(runs[2][1], runs[0][1] * 2.0 ** -23), "a power-of-two smaller upstream gradient must give the same dx bits, scaled"
    assert float(runs[2][1].abs().max()) > 0
    assert torch.equal(runs[3][0], runs[0][0]) and all(torch.equal(a, b) for a, b in zip(runs[3][2:], runs[0][2:])), \
        "the parameter gradients must not depend on whether dx is formed"


# ---- the pooled stem output from the trunk engine
@pytest.mark.gpu
@pytest.mark.parametrize("options", [{"fuse_stem_pool": 1, "fuse_fpn_head": 0}, {"fuse_stem_pool": 0, "fuse_fpn_head": 1}],
                         ids=["fused_stem_pool", "separate_pool"])
def test_forward_pool(hip, options):
    from vtd_amd.engine import DetectorEngine
    sd = nets.seeded_state_dict(lambda: nets.DBNet("resnet18"), seed=5)
    eng = DetectorEngine("resnet18", sd, max_batch=2, options=options)
    x = torch.randn((2, 3, 640, 640), generator=torch.Generator().manual_seed(1))
    tap = eng.forward_pool(x)
    torch.cuda.synchronize()
    want = eng.read_tap("pool", 2)      # the engine's own tap after the same forward: [2,64,160,160] float32
    assert tap.shape == (2, 162, 162, 64) and tap.dtype == torch.float16 and tap.is_contiguous()
    inner = tap[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).float().cpu().numpy()
    assert np.array_equal(inner, want) and float(np.abs(want).max()) > 0 and float(want.min()) >= 0
    t = tap.float()
    assert float(t[:, 0].abs().max()) == 0 and float(t[:, -1].abs().max()) == 0 and float(t[:, :, 0].abs().max()) == 0 \
        and float(t[:, :, -1].abs().max()) == 0, "the ring must be zero"
    eng.close()


# ---- layer1 -> layer2 -> layer3 -> layer4 -> FPN -> head -> HIP loss on a padded pool tap of 24 x 16
L1_NAMES = [f"{b}.{k}" for b in (0, 1) for k in BLOCK_NAMES[False]]
L_NAMES = l3t.L_NAMES


def _chain_setup():
    """The modules and inputs of tests/test_layer1_train.py's chain control (its seed makes both summands of dC2 matter), on the device."""
    mods, pool, targets = l1c.chain_modules()
    l1, l2, l3, l4, fpn, head = (m.cuda() for m in mods)
    return l1, l2, l3, l4, fpn, head.train(), pool, targets, nets.pack_tap(pool.cuda())


def _chain_step(l1, l2, l3, l4, fpn, head, poolp, targets):
    out = fpn.forward_padded([poolp], head=head, layer4=l4, layer3=l3, layer2=l2, layer1=l1)
    out["probability"].retain_grad()
    out["threshold"].retain_grad()
    training.detection_loss(out, {k: v.cuda() for k, v in targets.items()})["loss"].backward()
    return out, (out["probability"].grad, out["threshold"].grad)


@pytest.mark.gpu
def test_chain_layer1_to_head_loss_against_fp64(hip):
    """Stage-isolated at C2, C3, C4, C5 and P2: the reference head reads the P2 the kernels stored, the reference FPN the C2 .. C5 they
    stored, each reference stage the input tap they stored.  The gradient chain is end to end: the reference layer4's upstream gradient is
    the reference FPN's dC5, each stage below receives the reference dx of the stage above plus the reference FPN's gradient of the same
    tap; the reference layer1's is the reference layer2.0's dx plus the reference FPN's dC2."""
    l1, l2, l3, l4, fpn, head, pool, targets, poolp = _chain_setup()
    rl1, rl2, rl3, rl4 = (copy.deepcopy(m).to(device="cpu", dtype=torch.float64) for m in (l1, l2, l3, l4))
    rfpn, rhead = l4t._rounded_fpn(fpn), neck._rounded_head(head).train()
    out, ups = _chain_step(l1, l2, l3, l4, fpn, head, poolp, targets)
    c2p = nets.forward_layer1_padded(l1, poolp)
    assert c2p.shape == (2, 26, 18, 64) and c2p.dtype == torch.float16 and not c2p.requires_grad
    c3p = nets.forward_layer2_padded(l2, c2p)
    c4p = nets.forward_layer3_padded(l3, c3p)
    c5p = nets.forward_layer4_padded(l4, c4p)
    p2p = fpn.forward_padded([c2p, c3p, c4p, c5p])
    # reference, back to front
    x = _unpad(p2p).requires_grad_(True)
    torch.autograd.backward([rhead.probability_head(x), rhead.threshold_head(x)], [u.double().cpu() for u in ups])
    c2f, c3f, c4f, c5 = (_unpad(t).requires_grad_(True) for t in (c2p, c3p, c4p, c5p))
    l4t._wiring(rfpn, [c2f, c3f, c4f, c5]).backward(x.grad)
    c4b = _unpad(c4p).requires_grad_(True)
    _ref_block(rl4[1], _rounded(_ref_block(rl4[0], c4b))).backward(c5.grad)
    c3b = _unpad(c3p).requires_grad_(True)
    _ref_block(rl3[1], _rounded(_ref_block(rl3[0], c3b))).backward(c4b.grad + c4f.grad)
    c2b = _unpad(c2p).requires_grad_(True)
    r3 = _ref_block(rl2[1], _rounded(_ref_block(rl2[0], c2b)))
    r3.backward(c3b.grad + c3f.grad)
    dc2 = c2b.grad + c2f.grad
    shares = float(c2b.grad.norm() / dc2.norm()), float(c2f.grad.norm() / dc2.norm())
    r2 = _ref_block(rl1[1], _rounded(_ref_block(rl1[0], pool.double())))
    r2.backward(dc2)
    # ReLU-mask elements in which a reference stage's output and the stored tap differ: each carries a whole upstream element
    flips = {"C2": int(((r2 > 0) != (c2b > 0)).sum()), "C3": int(((r3 > 0) != (c3b > 0)).sum())}
    errs = {}
    for name, m, r, names in (("layer1", l1, rl1, L1_NAMES), ("layer2", l2, rl2, L_NAMES), ("layer3", l3, rl3, L_NAMES), ("layer4", l4, rl4, L_NAMES)):
        got, want = dict(m.named_parameters()), dict(r.named_parameters())
        errs[name] = {k: _rel(got[k].grad.double().cpu().numpy(), want[k].grad.numpy()) for k in names}
    errs["fpn"], errs["head"] = neck._fpn_errors(fpn, rfpn), neck._head_errors(head, rhead)
    assert [len(errs[k]) for k in ("layer1", "layer2", "layer3", "layer4", "fpn", "head")] == [12, 15, 15, 15, 10, 20]
    worst = {k: max(v, key=v.get) for k, v in errs.items()}
    print("MEASURED chain1: " + ", ".join(f"{k} grad {errs[k][worst[k]]:.3g} ({worst[k]})" for k in errs) +
          f"; shares of dC2: layer2.0's dx {shares[0]:.3g}, the FPN's {shares[1]:.3g}; mask elements that differ {flips}; {errs['layer1']}; {errs['layer2']}")
    assert min(shares) >= 10 * GRAD_CEILING, "both summands of dC2 must matter in this case, or leaving one out would pass"
    for k in errs:
        assert errs[k][worst[k]] <= CHAIN_BOUNDS[k], (k, errs[k])


@pytest.mark.gpu
def test_chain_bitwise_repeatable(hip):
    l1, l2, l3, l4, fpn, head, pool, targets, poolp = _chain_setup()
    state = copy.deepcopy(head.state_dict())
    runs = []
    for _ in range(2):
        head.load_state_dict(state)
        for m in (l1, l2, l3, l4, fpn, head):
            m.zero_grad(set_to_none=True)
        out, _ = _chain_step(l1, l2, l3, l4, fpn, head, poolp, targets)
        runs.append([out["probability"].detach(), out["threshold"].detach()] + [p.grad.clone() for m in (l1, l2, l3, l4) for p in m.parameters()] +
                    [p.grad.clone() for p in fpn.live_parameters()] + [p.grad.clone() for p in head.parameters()])
    assert len(runs[0]) == 2 + 87
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_product_layer1_training_step(hip):
    from vtd_amd._fixtures.weights import stress_detector_state_dict
    torch.manual_seed(3)
    net = nets.DBNet("resnet18", compute_threshold=True, trainable=MODE)
    net.load_state_dict(stress_detector_state_dict("resnet18", 17))
    net.cuda().train()
    gen = torch.Generator().manual_seed(23)
    x = torch.randn((2, 3, 640, 640), generator=gen).cuda()
    targets = neck._random_targets((2, 1, 640, 640), gen)
    te = net.trunk_engine()
    stats = {k: v.detach().clone() for k, v in net.backbone.state_dict().items() if "running" in k or "num_batches" in k}
    assert len(stats) == 60      # the stem's BatchNorm and 4 + 3 x 5 in the stages, three buffers each
    mod = training.TextDetectionLightningModule(net)
    opt = mod.configure_optimizers()["optimizer"]
    loss = mod.training_step((x, targets), 0)
    opt.zero_grad()
    loss.backward()
    trained = l1c._trained(net)
    assert len(trained) == 87
    for p in trained:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())
    assert all(float(p.grad.abs().max()) > 0 for p in net.backbone[4].parameters()), "a layer1 gradient is all zero"
    assert sum(1 for p in trained if float(p.grad.abs().max()) > 0) == 87
    for i in range(4):
        assert all(p.grad is None for p in net.backbone[i].parameters())
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    opt.step()
    after = net.state_dict()
    assert sum(1 for k in before if k.startswith("backbone.4.") and not torch.equal(before[k], after[k])) == 12
    for k in ("backbone.0.weight", "backbone.1.weight", "backbone.1.bias"):
        assert torch.equal(before[k], after[k]), f"{k} moved"
    assert net.trunk_engine() is te, "an optimizer step on layer1 .. layer4 / FPN / head weights rebuilt the trunk engine"
    for k, v in stats.items():
        assert torch.equal(v, net.backbone.state_dict()[k]), f"backbone.{k} was written"
    loss2 = mod.training_step((x, targets), 1)      # the second forward runs on the stepped weights
    assert bool(torch.isfinite(loss2)) and float(loss2.detach()) != float(loss.detach())
