"""Train-mode (batch-statistics) BatchNorm for ResNet-18's layer4 on the GPU (csrc/resblock_bn_train.hip): the two BasicBlocks through
`nets.basic_block_train(block, x, batch_stats=True)`, the layer4 -> FPN -> head node with `trunk_batch_stats=True`, and
`DBNet("resnet18", trainable="head+fpn+layer4", trunk_bn="batch")`.

The fp64 reference is CPU autograd in float64, the convention of tests/test_gpu_layer4_train.py: the block written with
F.batch_norm(..., training=True), fed x rounded to fp16 and the raw convolution weights rounded to fp16 straight through (the kernels pack
them unfolded); a1 and the downsample's normalised output are rounded to fp16 straight through, where the kernels store them.  Metric:
relative L2 error per tensor.  Bounds: 3x the level measured on an MI355X, worst over the sizes, under the ceilings of 2e-3 for maps and
1e-2 for gradients."""
import copy

import pytest
import torch
import torch.nn.functional as F

import test_gpu_layer4_train as frozen      # the helpers of the frozen-statistics stage: seeded blocks, the FPN / head references

from vtd_amd import nets, training

neck = frozen.neck
_rel, _ste = frozen._rel, frozen._ste
MAP_CEILING, GRAD_CEILING = 2e-3, 1e-2
SIZES = [(3, 2), (5, 4), (12, 11)]      # 12 x 11: M = 264 rows, two reduce workgroups and a last weight-gradient K chunk of 8 rows

BLOCK_BOUNDS = {
    # 3x the level measured on an MI355X, worst of the three sizes (grad: worst of the six / nine parameter gradients), never above the ceiling.
    # The gradient levels are set by 12 x 11: up to 5 x 4 every output agrees with the reference about its ReLU sign and the worst gradient
    # is 2.9e-4 on both blocks; at 12 x 11 (135168 outputs) 1 output of the stride-1 block and 3 of the stride-2 block sit so close to zero that
    # the fp16 operands put them on the other side.  Each flips one element of g2 = dy (y > 0), i.e. |dy_i| / |g2| ~ 1 / sqrt(67584) = 3.8e-3
    # of the upstream gradient of every parameter at once (3 flips: 6.6e-3): the measured levels.  3x the stride-2 level is over the ceiling:
    # its bound is the ceiling.
    "stride1": {"y": 6.3e-4, "grad": 3.9e-3, "dx": 3.7e-3, "stats": 2.2e-5, "running": 6.9e-6},    # measured 2.08e-4, 1.27e-3 (bn2.bias), 1.23e-3, 7.16e-6, 2.30e-6
    "stride2": {"y": 6.3e-4, "grad": GRAD_CEILING, "stats": 4.1e-5, "running": 1.3e-5},            # 2.09e-4, 6.57e-3 (bn1.weight), 1.35e-5, 4.02e-6
}
assert all(b[k] <= (MAP_CEILING if k in ("y", "stats", "running") else GRAD_CEILING) for b in BLOCK_BOUNDS.values() for k in b)
# the 15 layer4 gradients of the chain at C5 = 3 x 2: measured 5.38e-4 (0.conv1.weight)
CHAIN_LAYER4_BOUND = 1.7e-3
assert CHAIN_LAYER4_BOUND <= GRAD_CEILING


def _ref_pair(x, conv, bn, stride, pad, seen):
    z = F.conv2d(x, _ste(conv.weight), None, stride, pad)
    seen.append((z.detach().mean((0, 2, 3)), z.detach().var((0, 2, 3), unbiased=False)))
    return F.batch_norm(z, bn.running_mean, bn.running_var, bn.weight, bn.bias, True, bn.momentum, bn.eps)      # updates the buffers


def _ref_block(ref, x, seen=None):
    """The block in float64 with train-mode BatchNorm; `seen` collects (mu, sigma^2) of bn1, bn2 and the downsample's BatchNorm, the order of
    the kernels' statistics rows."""
    s1, s2, sd = [], [], []
    a1 = F.relu(_ref_pair(x, ref.conv1, ref.bn1, ref.stride, 1, s1))
    a1 = a1 + (a1.half().double() - a1).detach()
    idt = x
    if hasattr(ref, "downsample"):
        idt = _ref_pair(x, ref.downsample[0], ref.downsample[1], ref.stride, 0, sd)
        idt = idt + (idt.half().double() - idt).detach()
    y = F.relu(_ref_pair(a1, ref.conv2, ref.bn2, 1, 1, s2) + idt)
    if seen is not None:
        seen += s1 + s2 + sd
    return y


def _bns(blk):
    return [blk.bn1, blk.bn2] + ([blk.downsample[1]] if hasattr(blk, "downsample") else [])


def _block_case(blk, cin, stride, size, want_dx):
    h, w = size
    gen = torch.Generator().manual_seed(7 * h + w)
    x = (torch.randn((2, cin, h * stride, w * stride), generator=gen) * 0.5).half().float()
    up = torch.randn((2, 512, h, w), generator=gen)
    blk.train()
    ref = copy.deepcopy(blk).to(device="cpu", dtype=torch.float64)
    xr = x.double().requires_grad_(want_dx)
    seen = []
    yr = _ref_block(ref, xr, seen)
    # the statistics the forward reports, on a copy of the block (the call moves the running statistics)
    probe = copy.deepcopy(blk)
    (c_in, width, st), eps, learn, stats = probe._train_operands(torch.device("cuda", torch.cuda.current_device()))
    with torch.no_grad():
        _, _, bstats = nets._block_forward_raw(nets.pack_tap(x.cuda()), (2, h * stride, w * stride, c_in, width, st), eps, learn, stats,
                                               bn=(True, probe.bn1.momentum))
    e_stats = max(_rel(bstats[i, j].double().cpu().numpy(), seen[i][j].numpy()) for i in range(len(seen)) for j in range(2))
    if len(seen) == 2:
        assert bool(torch.isnan(bstats[2]).all()), "the third statistics row was written without a downsample"
    xg = x.cuda().requires_grad_(want_dx)
    y = nets.basic_block_train(blk, xg, batch_stats=True)
    assert y.shape == (2, 512, h, w) and y.dtype == torch.float32
    agree = ((y.detach().cpu() > 0) == (yr.detach() > 0)).float()
    yr.backward(up.double())
    y.backward(up.cuda())
    e_run = 0.0
    for a, b, p in zip(_bns(blk), _bns(ref), _bns(probe)):
        assert int(a.num_batches_tracked) == 1
        assert torch.equal(a.running_mean, p.running_mean) and torch.equal(a.running_var, p.running_var)
        e_run = max(e_run, _rel(a.running_mean.double().cpu().numpy(), b.running_mean.numpy()), _rel(a.running_var.double().cpu().numpy(), b.running_var.numpy()))
    names = frozen.BLOCK_NAMES[hasattr(blk, "downsample")]
    got, want = dict(blk.named_parameters()), dict(ref.named_parameters())
    errs = {k: _rel(got[k].grad.double().cpu().numpy(), want[k].grad.numpy()) for k in names}
    for k in names:
        assert bool(torch.isfinite(got[k].grad).all()), k
    # gamma = 0 (bn2 channel 3): conv2's weight gradient of that channel vanishes exactly, dgamma does not
    assert float(got["conv2.weight"].grad[3].abs().max()) == 0.0 and float(got["bn2.weight"].grad[3].abs()) > 0
    e_y = _rel(y.detach().double().cpu().numpy(), yr.detach().numpy())
    e_dx = _rel(xg.grad.double().cpu().numpy(), xr.grad.numpy()) if want_dx else None
    return e_y, errs, e_dx, float(agree.mean()), e_stats, e_run


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_stride1_block_against_fp64(hip, size):
    blk = frozen._seeded_block(512, 1, 21)
    e_y, errs, e_dx, agree, e_stats, e_run = _block_case(blk, 512, 1, size, True)
    worst = max(errs, key=errs.get)
    print(f"MEASURED bn stride1 {size[0]}x{size[1]}: y {e_y:.3g}, grad {errs[worst]:.3g} ({worst}), dx {e_dx:.3g}, stats {e_stats:.3g}, "
          f"running {e_run:.3g}, sign agreement {agree:.5f}; {errs}")
    assert agree > 0.99 and len(errs) == 6
    b = BLOCK_BOUNDS["stride1"]
    assert e_y <= b["y"] and errs[worst] <= b["grad"] and e_dx <= b["dx"] and e_stats <= b["stats"] and e_run <= b["running"], (e_y, errs, e_dx, e_stats,
                                                                                                                             e_run)


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_stride2_block_against_fp64(hip, size):
    blk = frozen._seeded_block(256, 2, 22)
    e_y, errs, _, agree, e_stats, e_run = _block_case(blk, 256, 2, size, False)
    worst = max(errs, key=errs.get)
    print(f"MEASURED bn stride2 {size[0]}x{size[1]}: y {e_y:.3g}, grad {errs[worst]:.3g} ({worst}), stats {e_stats:.3g}, running {e_run:.3g}, "
          f"sign agreement {agree:.5f}; {errs}")
    assert agree > 0.99 and len(errs) == 9
    with pytest.raises(RuntimeError, match="stride-2 block"):
        nets.basic_block_train(blk, torch.zeros((2, 256, 2, 2), device="cuda", requires_grad=True), batch_stats=True)
    with pytest.raises(ValueError, match="more than one value"):
        nets.basic_block_train(blk, torch.zeros((1, 256, 2, 2), device="cuda"), batch_stats=True)
    b = BLOCK_BOUNDS["stride2"]
    assert e_y <= b["y"] and errs[worst] <= b["grad"] and e_stats <= b["stats"] and e_run <= b["running"], (e_y, errs, e_stats, e_run)


def _run(blk, x, up, want_dx, batch_stats=True):
    blk.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(want_dx)
    y = nets.basic_block_train(blk, xg, batch_stats=True) if batch_stats else nets.basic_block_train(blk, xg)
    y.backward(up)
    return [y.detach()] + ([xg.grad] if want_dx else []) + [p.grad.clone() for p in blk.parameters()]


@pytest.mark.gpu
@pytest.mark.parametrize("cin,stride", [(512, 1), (256, 2)])
def test_eval_mode_is_the_frozen_path(hip, cin, stride):
    blk = frozen._seeded_block(cin, stride, 24).eval()
    gen = torch.Generator().manual_seed(2)
    x = (torch.randn((2, cin, 5 * stride, 4 * stride), generator=gen) * 0.5).half().float().cuda()
    up = torch.randn((2, 512, 5, 4), generator=gen).cuda()
    buffers = [b.detach().clone() for b in blk.buffers()]
    want = _run(blk, x, up, stride == 1, batch_stats=False)
    got = _run(blk, x, up, stride == 1)
    assert len(got) == len(want) == (8 if stride == 1 else 10)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert all(torch.equal(a, b) for a, b in zip(buffers, blk.buffers())), "eval() wrote the buffers"


@pytest.mark.gpu
@pytest.mark.parametrize("cin,stride", [(512, 1), (256, 2)])
def test_bitwise_repeatable_and_scaled(hip, cin, stride):
    blk = frozen._seeded_block(cin, stride, 23).train()
    gen = torch.Generator().manual_seed(1)
    x = (torch.randn((2, cin, 12 * stride, 11 * stride), generator=gen) * 0.5).half().float().cuda()
    up = torch.randn((2, 512, 12, 11), generator=gen).cuda()
    state = copy.deepcopy(blk.state_dict())
    runs, buffers = [], []
    for scale in (1.0, 1.0, 2.0 ** -23):
        blk.load_state_dict(state)
        runs.append(_run(blk, x, up * scale, stride == 1))
        buffers.append([b.detach().clone() for b in blk.buffers()])
    for a, b, c in zip(*runs):
        assert torch.equal(a, b)
    for a, b in zip(buffers[0], buffers[1]):
        assert torch.equal(a, b)
    assert torch.equal(runs[2][0], runs[0][0])
    for a, c in zip(runs[0][1:], runs[2][1:]):
        assert torch.equal(c, a * 2.0 ** -23), "a power-of-two smaller upstream gradient must give the same bits, scaled"


# ---- layer4 -> FPN -> head -> HIP loss on padded taps
def _chain_step(l4, fpn, head, padded, targets):
    out = fpn.forward_padded(padded, head=head, layer4=l4, trunk_batch_stats=True)
    out["probability"].retain_grad()
    out["threshold"].retain_grad()
    training.detection_loss(out, {k: v.cuda() for k, v in targets.items()})["loss"].backward()
    return out, (out["probability"].grad, out["threshold"].grad)


@pytest.mark.gpu
def test_chain_layer4_fpn_head_loss_against_fp64(hip):
    """Stage-isolated at C5 and P2 as tests/test_gpu_layer4_train.py's chain: the reference head reads the P2 the kernels stored, the
    reference FPN the C5 they stored; the reference layer4 (train-mode BatchNorm) takes the reference FPN's dC5."""
    l4, fpn, head, feats, targets, padded = frozen._chain_setup()
    l4.train()
    rl4 = copy.deepcopy(l4).to(device="cpu", dtype=torch.float64)
    rfpn, rhead = frozen._rounded_fpn(fpn), neck._rounded_head(head).train()
    probe = copy.deepcopy(l4)      # C5 as the kernels store it, from the same starting buffers
    _, geoms, eps, learn, stats = nets._stage_operands(nets._STAGES[3], probe, padded[2])
    with torch.no_grad():
        midp, _, _ = nets._block_forward_raw(padded[2], geoms[0], eps, learn[0], stats[0], bn=(True, 0.1))
        c5p, _, _ = nets._block_forward_raw(midp, geoms[1], eps, learn[1], stats[1], bn=(True, 0.1))
    out, ups = _chain_step(l4, fpn, head, padded, targets)
    p2p = fpn.forward_padded(padded + [c5p])
    x = p2p[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).double().cpu().contiguous().requires_grad_(True)
    torch.autograd.backward([rhead.probability_head(x), rhead.threshold_head(x)], [u.double().cpu() for u in ups])
    c5 = c5p[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).double().cpu().contiguous().requires_grad_(True)
    frozen._wiring(rfpn, [t.double() for t in feats] + [c5]).backward(x.grad)
    mid = _ref_block(rl4[0], feats[2].double())
    mid = mid + (mid.half().double() - mid).detach()
    _ref_block(rl4[1], mid).backward(c5.grad)
    got, want = dict(l4.named_parameters()), dict(rl4.named_parameters())
    le = {k: _rel(got[k].grad.double().cpu().numpy(), want[k].grad.numpy()) for k in frozen.L4_NAMES}
    assert len(le) == 15
    wl = max(le, key=le.get)
    print(f"MEASURED bn chain: layer4 grad {le[wl]:.3g} ({wl}); {le}")
    for b in l4:
        for bn in _bns(b):
            assert int(bn.num_batches_tracked) == 1
    for a, p in zip(l4.buffers(), probe.buffers()):
        if a.dtype == torch.float32:
            assert torch.equal(a, p)
    assert le[wl] <= CHAIN_LAYER4_BOUND, le


# ---- the product path
@pytest.mark.gpu
def test_product_step_with_batch_statistics(hip):
    from vtd_amd._fixtures.weights import stress_detector_state_dict
    torch.manual_seed(3)
    sd = stress_detector_state_dict("resnet18", 17)
    gen = torch.Generator().manual_seed(23)
    x = torch.randn((2, 3, 640, 640), generator=gen).cuda()
    targets = neck._random_targets((2, 1, 640, 640), gen)

    net = nets.DBNet("resnet18", compute_threshold=True, trainable="head+fpn+layer4", trunk_bn="batch")
    net.load_state_dict(sd)
    net.cuda().train()
    te = net.trunk_engine()
    mod = training.TextDetectionLightningModule(net)
    opt = mod.configure_optimizers()["optimizer"]
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    loss = mod.training_step((x, targets), 0)
    opt.zero_grad()
    loss.backward()
    l4 = dict(net.backbone[7].named_parameters())
    assert len(l4) == 15
    for k, p in l4.items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, f"backbone.7.{k}"
    for i in range(7):
        assert all(p.grad is None for p in net.backbone[i].parameters())
    opt.step()
    after = net.state_dict()
    for k in l4:
        assert not torch.equal(before["backbone.7." + k], after["backbone.7." + k]), f"backbone.7.{k} did not change"
    moved = [k for k in before if k.startswith("backbone.7.") and "running" in k]
    counts = [k for k in before if k.startswith("backbone.7.") and "num_batches" in k]
    assert len(moved) == 10 and len(counts) == 5
    for k in moved:
        assert bool(torch.isfinite(after[k]).all()) and not torch.equal(before[k], after[k]), f"{k} did not move"
    for k in counts:
        assert int(after[k]) == 1, k
    for k in before:
        if k.startswith("backbone.") and not k.startswith("backbone.7."):
            assert torch.equal(before[k], after[k]), f"{k} changed"
    assert net.trunk_engine() is te, "a step on layer4 / FPN / head tensors rebuilt the trunk engine"
    loss2 = mod.training_step((x, targets), 1)
    assert bool(torch.isfinite(loss2)) and float(loss2) != float(loss)
    assert all(int(net.state_dict()[k]) == 2 for k in counts)
    # a following eval() forward runs the fused inference engine on the stepped weights and the moved statistics
    net.eval()
    with torch.no_grad():
        got = net(x)
    fresh = nets.DBNet("resnet18", compute_threshold=True)
    fresh.load_state_dict(net.state_dict())
    with torch.no_grad():
        want = fresh.cuda().eval()(x)
    assert torch.equal(got["probability"], want["probability"]) and torch.equal(got["threshold"], want["threshold"])

    # the same network with the default trunk_bn leaves backbone.7's buffers alone
    net0 = nets.DBNet("resnet18", compute_threshold=True, trainable="head+fpn+layer4")
    net0.load_state_dict(sd)
    net0.cuda().train()
    mod0 = training.TextDetectionLightningModule(net0)
    mod0.training_step((x, targets), 0).backward()
    for k, v in net0.backbone[7].state_dict().items():
        if "running" in k or "num_batches" in k:
            assert torch.equal(v, before["backbone.7." + k].to(v.device)), f"the default mode wrote backbone.7.{k}"
