"""Training ResNet-18's layer2 on the GPU (csrc/resblock_train.hip: the 128-wide blocks, csrc/wgrad_mfma.h: MODE 4 over the 64-channel C2):
the two new block geometries through `nets.basic_block_train` with the input gradient of either stride, one multi-slab case per geometry,
the chain layer2 -> layer3 -> layer4 -> FPN -> head -> HIP loss on a padded C2, and the product mode "head+fpn+layer4+layer3+layer2".

The fp64 references are CPU autograd of the same wiring, built like tests/test_gpu_layer4_train.py's `_ref_block`: folded weights and stored
activations rounded to fp16, straight through, frozen statistics.  Metric: relative L2 error per tensor, as tests/test_gpu_layer3_train.py.
Bounds follow DESIGN.md section 4's convention: 3x the level measured on an MI355X, never above the ceilings (2e-3 for maps, 1e-2 for
gradients); the measured values stand beside them."""
import copy

import pytest
import torch

import test_gpu_fpn_neck_train as neck
import test_gpu_layer3_train as l3t
import test_gpu_layer4_train as l4t
from vtd_amd import nets, training
from vtd_amd.nets import forward_layer2_padded  # noqa: F401  (the feature under test: absent before it)

MAP_CEILING, GRAD_CEILING = 2e-3, 1e-2
GEOMETRIES = {"l2s2": (64, 128, 2), "l2s1": (128, 128, 1)}
SIZES = [(1, 1), (3, 2), (5, 4)]
# The multi-slab case.  A 128-wide block's weight-gradient launch of q q-tiles cuts its rows into min(ceil(512 / q), ceil(rows / 1024)) slabs
# of ceil(rows / slabs) rows rounded up to the 32-row chunk (csrc/resblock_train.hip: wg_slabs128, slab_rows); q is 9, 5 or 1, so every
# launch has two slabs from 1025 rows on.  n = 2, output 23 x 23: 1058 rows = a slab of 544 (529 rounded up) and a last slab of 514 rows, 16
# chunks and 2 rows: not full, and it ends inside a chunk.  The reduce has ceil(1058 / 256) = 5 partials of 212 rows (two halves of 106), the
# last of 210; the convolutions have 9 tiles of 128 rows, the stride-2 block's input gradient (2 x 46 x 46 = 4232 rows, 64 columns) 17 of 256
LARGE = (23, 23)
# geometry -> bounds on y, the worst parameter gradient and dx: 3x the worst of the sizes measured on an MI355X (behind each line)
BLOCK_BOUNDS = {
    "l2s2": {"y": 6.3e-4, "grad": 8.9e-4, "dx": 6.6e-4},      # measured 2.08e-4, 2.95e-4 (bn1.weight), 2.20e-4 (the strided dgrad, 23x23)
    # 2.07e-4, 1.74e-3 (bn1.bias, 23x23), 1.44e-3 (23x23).  The three small sizes give 3.07e-4 (conv1.weight) and 4.74e-5, layer3's level;
    # at 23x23 one of the 135 424 output elements is 0 where the reference has 2.8e-6 (upstream gradient -0.37 there), so the ReLU masks
    # differ in that element and every gradient carries it (bn2.bias, a plain sum of g2: 1.45e-3 against 2.7e-8 at the small sizes).  With
    # the upstream gradient zeroed at that element the same case measures 3.49e-4 (bn1.weight) and 5.93e-5: rounding level.  The bound
    # follows the measured worst all the same.  The stride-2 block at 23x23 has no such element
    "l2s1": {"y": 6.3e-4, "grad": 5.3e-3, "dx": 4.4e-3},
}
# worst gradient per stage of the chain at C5 = 3x2, n = 2: measured 8.33e-3 (layer2, 1.bn2.bias), 4.47e-3 (layer3, 1.bn1.bias), 7.79e-4 (layer4,
# 0.downsample.1.weight), 7.68e-4 (FPN, inner_blocks.0.weight), 4.17e-4 (head, threshold_head.0.weight).  3x the first two exceeds the
# ceiling the layer4 chain uses, so the ceiling is their bound.  The FPN's dC3 is 0.93 of dC3's norm here
CHAIN_BOUNDS = {"layer2": GRAD_CEILING, "layer3": GRAD_CEILING, "layer4": 2.4e-3, "fpn": 2.4e-3, "head": 1.3e-3}
assert all(b["y"] <= MAP_CEILING and b["grad"] <= GRAD_CEILING and b["dx"] <= GRAD_CEILING for b in BLOCK_BOUNDS.values())
assert all(v <= GRAD_CEILING for v in CHAIN_BOUNDS.values())

_rel, _ref_block, BLOCK_NAMES = l4t._rel, l4t._ref_block, l4t.BLOCK_NAMES
_seeded_block, _inputs, _param_grads, _unpad, _rounded = l3t._seeded_block, l3t._inputs, l3t._param_grads, l3t._unpad, l3t._rounded
MODE = "head+fpn+layer4+layer3+layer2"

_REFS = {}


def _reference(key, size):
    """(block, x, up, reference y, reference parameter gradients, reference dx), computed once per case."""
    if (key, size) not in _REFS:
        cin, width, stride = GEOMETRIES[key]
        blk = _seeded_block(cin, width, stride, 80 + cin // 64 + stride)
        x, up = _inputs(cin, width, stride, size)
        ref = copy.deepcopy(blk).to(device="cpu", dtype=torch.float64)
        xr = x.double().requires_grad_(True)
        yr = _ref_block(ref, xr)
        yr.backward(up.double())
        want = dict(ref.named_parameters())
        _REFS[(key, size)] = (blk, x, up, yr.detach(), {k: want[k].grad.clone() for k in BLOCK_NAMES[stride == 2]}, xr.grad.clone())
    return _REFS[(key, size)]


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES + [LARGE])
@pytest.mark.parametrize("key", sorted(GEOMETRIES))
def test_block_against_fp64(hip, key, size):
    cin, width, stride = GEOMETRIES[key]
    blk, x, up, yr, gr, dxr = _reference(key, size)
    assert float(blk.bn2.weight[3]) == 0.0 and float(blk.bn2.weight[7]) < 0      # a gamma = 0 channel and a gamma < 0 channel
    blk.zero_grad(set_to_none=True)
    stats_before = [b.detach().clone() for b in blk.buffers()]
    xg = x.cuda().requires_grad_(True)
    y = nets.basic_block_train(blk.train(), xg)
    assert y.shape == (2, width, *size) and y.dtype == torch.float32 and y.requires_grad
    y.backward(up.cuda())
    assert all(torch.equal(a, b) for a, b in zip(stats_before, blk.buffers())), "frozen statistics were written"
    assert xg.grad is not None and xg.grad.shape == x.shape and bool(torch.isfinite(xg.grad).all()) and float(xg.grad.abs().max()) > 0
    got = dict(blk.named_parameters())
    errs = {k: _rel(got[k].grad.double().cpu().numpy(), gr[k].numpy()) for k in gr}
    assert len(errs) == (9 if stride == 2 else 6)      # every learnable tensor of the block (the stage's two blocks have 15)
    e_y = _rel(y.detach().double().cpu().numpy(), yr.numpy())
    e_dx = _rel(xg.grad.double().cpu().numpy(), dxr.numpy())
    agree = float(((y.detach().cpu() > 0) == (yr > 0)).float().mean())
    worst = max(errs, key=errs.get)
    print(f"MEASURED block {key} {size[0]}x{size[1]}: y {e_y:.3g}, grad {errs[worst]:.3g} ({worst}), dx {e_dx:.3g}, sign agreement {agree:.5f}; {errs}")
    assert agree > 0.99
    b = BLOCK_BOUNDS[key]
    assert e_y <= b["y"] and errs[worst] <= b["grad"] and e_dx <= b["dx"], (e_y, errs, e_dx)


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(GEOMETRIES))
def test_block_bitwise_repeatable_and_scaled(hip, key):
    """Two runs give the same bits at the multi-slab size; an upstream gradient smaller by 2^-23 gives the same dx bits, scaled."""
    cin, width, stride = GEOMETRIES[key]
    blk = _seeded_block(cin, width, stride, 83)
    x, up = _inputs(cin, width, stride, LARGE)
    runs = []
    for scale in (1.0, 1.0, 2.0 ** -23):
        blk.zero_grad(set_to_none=True)
        xg = x.cuda().requires_grad_(True)
        y = nets.basic_block_train(blk, xg)
        y.backward(up.cuda() * scale)
        runs.append([y.detach(), xg.grad] + _param_grads(blk))
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
    assert torch.equal(runs[2][1], runs[0][1] * 2.0 ** -23), "a power-of-two smaller upstream gradient must give the same dx bits, scaled"
    assert float(runs[2][1].abs().max()) > 0


# ---- layer2 -> layer3 -> layer4 -> FPN -> head -> HIP loss on a padded C2
L_NAMES = l3t.L_NAMES


def _chain_setup():
    n, h5, w5 = 2, 3, 2
    gen = torch.Generator().manual_seed(57)
    l2 = torch.nn.Sequential(_seeded_block(64, 128, 2, 91), _seeded_block(128, 128, 1, 92)).cuda()
    l3 = torch.nn.Sequential(_seeded_block(128, 256, 2, 93), _seeded_block(256, 256, 1, 94)).cuda()
    l4 = torch.nn.Sequential(_seeded_block(256, 512, 2, 95), _seeded_block(512, 512, 1, 96)).cuda()
    fpn, head = l4t._seeded_fpn(512, 6), neck._seeded_head(8).train()
    c2 = l4t._taps(n, 512, h5, w5, gen)[0]
    targets = neck._random_targets((n, 1, 32 * h5, 32 * w5), gen)
    return l2, l3, l4, fpn, head, c2, targets, nets.pack_tap(c2.cuda())


def _chain_step(l2, l3, l4, fpn, head, c2p, targets):
    out = fpn.forward_padded([c2p], head=head, layer4=l4, layer3=l3, layer2=l2)
    out["probability"].retain_grad()
    out["threshold"].retain_grad()
    training.detection_loss(out, {k: v.cuda() for k, v in targets.items()})["loss"].backward()
    return out, (out["probability"].grad, out["threshold"].grad)


@pytest.mark.gpu
def test_chain_layer2_layer3_layer4_fpn_head_loss_against_fp64(hip):
    """Stage-isolated at C3, C4, C5 and P2: the reference head reads the P2 the kernels stored, the reference FPN the C3, C4 and C5 they
    stored, the reference layer4 that C4, the reference layer3 that C3.  The gradient chain is end to end: the reference layer4's upstream
    gradient is the reference FPN's dC5, the reference layer3's is the reference layer4.0's dx plus the reference FPN's dC4, the reference
    layer2's is the reference layer3.0's dx plus the reference FPN's dC3."""
    l2, l3, l4, fpn, head, c2, targets, c2p = _chain_setup()
    rl2, rl3, rl4 = (copy.deepcopy(m).to(device="cpu", dtype=torch.float64) for m in (l2, l3, l4))
    rfpn, rhead = l4t._rounded_fpn(fpn), neck._rounded_head(head).train()
    out, ups = _chain_step(l2, l3, l4, fpn, head, c2p, targets)
    c3p = nets.forward_layer2_padded(l2, c2p)
    assert c3p.shape == (2, 14, 10, 128) and c3p.dtype == torch.float16 and not c3p.requires_grad
    c4p = nets.forward_layer3_padded(l3, c3p)
    c5p = nets.forward_layer4_padded(l4, c4p)
    p2p = fpn.forward_padded([c2p, c3p, c4p, c5p])
    # reference, back to front
    x = _unpad(p2p).requires_grad_(True)
    torch.autograd.backward([rhead.probability_head(x), rhead.threshold_head(x)], [u.double().cpu() for u in ups])
    c3f, c4f, c5 = (_unpad(t).requires_grad_(True) for t in (c3p, c4p, c5p))
    l4t._wiring(rfpn, [c2.double(), c3f, c4f, c5]).backward(x.grad)
    c4b = _unpad(c4p).requires_grad_(True)
    _ref_block(rl4[1], _rounded(_ref_block(rl4[0], c4b))).backward(c5.grad)
    c3b = _unpad(c3p).requires_grad_(True)
    _ref_block(rl3[1], _rounded(_ref_block(rl3[0], c3b))).backward(c4b.grad + c4f.grad)
    share = float(c3f.grad.norm() / (c3b.grad + c3f.grad).norm())
    _ref_block(rl2[1], _rounded(_ref_block(rl2[0], c2.double()))).backward(c3b.grad + c3f.grad)
    errs = {}
    for name, m, r in (("layer2", l2, rl2), ("layer3", l3, rl3), ("layer4", l4, rl4)):
        got, want = dict(m.named_parameters()), dict(r.named_parameters())
        errs[name] = {k: _rel(got[k].grad.double().cpu().numpy(), want[k].grad.numpy()) for k in L_NAMES}
    errs["fpn"], errs["head"] = neck._fpn_errors(fpn, rfpn), neck._head_errors(head, rhead)
    assert [len(errs[k]) for k in ("layer2", "layer3", "layer4", "fpn", "head")] == [15, 15, 15, 10, 20]
    worst = {k: max(v, key=v.get) for k, v in errs.items()}
    print("MEASURED chain2: " + ", ".join(f"{k} grad {errs[k][worst[k]]:.3g} ({worst[k]})" for k in errs) +
          f"; the FPN's share of dC3 {share:.3g}; {errs['layer2']}")
    assert share > 10 * GRAD_CEILING, "the FPN's dC3 must matter in this case, or leaving it out would pass"
    for k in errs:
        assert errs[k][worst[k]] <= CHAIN_BOUNDS[k], (k, errs[k])


@pytest.mark.gpu
def test_chain_bitwise_repeatable(hip):
    l2, l3, l4, fpn, head, c2, targets, c2p = _chain_setup()
    state = copy.deepcopy(head.state_dict())
    runs = []
    for _ in range(2):
        head.load_state_dict(state)
        for m in (l2, l3, l4, fpn, head):
            m.zero_grad(set_to_none=True)
        out, _ = _chain_step(l2, l3, l4, fpn, head, c2p, targets)
        runs.append([out["probability"].detach(), out["threshold"].detach()] + [p.grad.clone() for m in (l2, l3, l4) for p in m.parameters()] +
                    [p.grad.clone() for p in fpn.live_parameters()] + [p.grad.clone() for p in head.parameters()])
    assert len(runs[0]) == 2 + 45 + 10 + 20
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_product_head_fpn_layer4_layer3_layer2_training_step(hip):
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
    trained = {f"backbone.{i}.{k}": p for i in (5, 6, 7) for k, p in net.backbone[i].named_parameters()}
    assert len(trained) == 45
    for k, p in trained.items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k
    for i in range(5):
        assert all(p.grad is None for p in net.backbone[i].parameters())
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    opt.step()
    after = net.state_dict()
    learnable = {k for k, _ in net.named_parameters()}
    for k in before:      # one step changes exactly the trained tensors: layer2's 15 parameters move, backbone.0 .. backbone.4 keep their bits
        is_trained = k in learnable and not k.startswith(tuple(f"backbone.{i}." for i in range(5))) and not k.startswith(("fpn.layer_blocks.0",
                                                                                                                          "fpn.layer_blocks.1",
                                                                                                                          "fpn.layer_blocks.2"))
        if k.startswith("backbone."):
            assert torch.equal(before[k], after[k]) != is_trained, f"{k}: trained {is_trained}"
        elif is_trained:
            assert not torch.equal(before[k], after[k]), f"{k} did not change"
    assert sum(1 for k in before if k.startswith("backbone.5.") and not torch.equal(before[k], after[k])) == 15
    assert net.trunk_engine() is te, "an optimizer step on layer2 / layer3 / layer4 / FPN / head weights rebuilt the trunk engine"
    for k, v in stats.items():
        assert torch.equal(v, net.backbone.state_dict()[k]), f"backbone.{k} was written"
    loss2 = mod.training_step((x, targets), 1)
    assert bool(torch.isfinite(loss2)) and float(loss2.detach()) != float(loss.detach())
    # a following eval() forward runs the fused inference engine on the stepped weights
    net.eval()
    with torch.no_grad():
        got = net(x)
    fresh = nets.DBNet("resnet18", compute_threshold=True)
    fresh.load_state_dict(net.state_dict())
    with torch.no_grad():
        want = fresh.cuda().eval()(x)
    assert torch.equal(got["probability"], want["probability"]) and torch.equal(got["threshold"], want["threshold"])
