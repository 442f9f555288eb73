"""Train-mode (batch-statistics) BatchNorm for ResNet-18's layer3 and the strided input gradient on that path, on the GPU
(csrc/resblock_bn_train.hip, the vtd_block_bn_train_* entries): the blocks through `nets.basic_block_bn_train(block, x)`, the layer3 ->
layer4 -> FPN -> head node with `trunk_batch_stats=("layer3", "layer4")`, and
`DBNet("resnet18", trainable="head+fpn+layer4+layer3", trunk_bn=("layer3", "layer4"))`.

The fp64 reference is CPU autograd in float64 of tests/test_gpu_layer4_bn_train.py's `_ref_block`: the block written with
F.batch_norm(..., training=True), fed x rounded to fp16 and the raw convolution weights rounded to fp16 straight through; a1 and the
downsample's normalised output are rounded to fp16 straight through, where the kernels store them.  Blocks come from
tests/test_gpu_layer3_train.py's `_seeded_block` (gamma = 0 in bn2's channel 3, gamma < 0 in channel 7).  Metric: relative L2 error per tensor.
Bounds: 3x the level measured on an MI355X, worst over the sizes, never above the ceilings of 2e-3 for maps, statistics and running buffers
and 1e-2 for gradients and dx; 3x is the project's standing allowance for the seed-to-seed spread of an fp16-operand
path."""
import copy

import pytest
import torch

import test_gpu_fpn_neck_train as neck
import test_gpu_layer3_train as l3t
import test_gpu_layer4_bn_train as bn4
import test_gpu_layer4_train as l4t
from vtd_amd import nets, training
from vtd_amd.nets import basic_block_bn_train  # noqa: F401  (the feature under test: absent before it)

_rel, BLOCK_NAMES = l4t._rel, l4t.BLOCK_NAMES
MAP_CEILING, GRAD_CEILING = 2e-3, 1e-2
GEOMETRIES = l3t.GEOMETRIES      # l3s2, l3s1, l4s2, l4s1 -> (cin, width, stride)
SIZES = [(3, 2), (5, 4), (12, 11)]      # 12 x 11: M = 264 rows, two reduce workgroups of 132 rows (quarters of 33) and a last weight-gradient
#                                         K chunk of 8 rows.  1 x 1 is left out: with M = 2 values per channel dz is pure cancellation
SEEDS = {"l3s1": 81, "l3s2": 82, "l4s2": 83}
MODE = "head+fpn+layer4+layer3"
STAGES = ("layer3", "layer4")

# geometry -> bounds: 3x the level measured on an MI355X, worst of the three sizes (grad: worst of the six / nine parameter gradients), never
# above the ceiling.  The measured levels stand behind each line.  Both layer3 blocks agree with the reference about every ReLU sign at all
# three sizes (0 flips of 3072, 10240 and 67584 outputs) and sit at the frozen path's level, 12 x 11 included.  layer4's stride-2 block has 0
# flips up to 5 x 4 (grad 2.96e-4, dx 2.63e-4) and 1 flip of 135168 outputs at 12 x 11: that output flips one element of g2 = dy (y > 0) and
# moves every gradient and dx at once (tests/test_gpu_layer4_bn_train.py describes the same at its seeds), which sets that block's levels.
BLOCK_BOUNDS = {
    # measured 2.12e-4, 2.98e-4 (conv1.weight), 2.75e-4, 6.32e-6, 1.92e-6
    "l3s1": {"y": 6.4e-4, "grad": 9.0e-4, "dx": 8.3e-4, "stats": 1.9e-5, "running": 5.8e-6},
    # 2.13e-4, 3.04e-4 (conv1.weight), 2.65e-4, 1.59e-6, 5.86e-7
    "l3s2": {"y": 6.4e-4, "grad": 9.2e-4, "dx": 8.0e-4, "stats": 4.8e-6, "running": 1.8e-6},
    # 2.08e-4, 2.09e-3 (bn1.bias, 12 x 11, 1 flip), 2.03e-3 (12 x 11), 5.89e-6, 1.69e-6
    "l4s2": {"y": 6.3e-4, "grad": 6.3e-3, "dx": 6.1e-3, "stats": 1.8e-5, "running": 5.1e-6},
}
assert all(b[k] <= (MAP_CEILING if k in ("y", "stats", "running") else GRAD_CEILING) for b in BLOCK_BOUNDS.values() for k in b)
# the chain at C5 = 3 x 2, n = 2: the worst of layer3's 15 and of layer4's 15 gradients, measured 6.92e-3 (layer3, 1.bn2.bias) and 8.35e-3
# (layer4, 1.conv1.weight); 3x each is over the ceiling: the bound is the ceiling.  The levels are those of ReLU sign flips, not of the
# blocks (2-3e-4 each above): all thirty gradients sit at 5.7e-3 .. 8.4e-3 alike, layer4.1's included, whose kernels and upstream dC5 this
# stage does not touch, and only layer4's 1.bn2.weight, whose sum weights g2 by xh, is at 4.9e-4 -- the signature the layer4 file found.  With
# M = 12 values per channel at C5 the batch statistics move every output, so outputs near zero differ from the frozen chain's (7-8e-4 on the
# same modules in tests/test_gpu_layer3_train.py).  The test prints the flips of the four block outputs beside the levels: measured 0, 0, 0
# and 1 (of 6144 outputs of layer4.1, that is of C5: one element of 1 / sqrt(3072) of g2's norm at the top of the whole backward chain).
# The running buffers after the step: measured 3.23e-5.
CHAIN_BOUNDS = {"layer3": GRAD_CEILING, "layer4": GRAD_CEILING}
CHAIN_RUNNING_BOUND = 9.7e-5
assert all(v <= GRAD_CEILING for v in CHAIN_BOUNDS.values()) and CHAIN_RUNNING_BOUND <= MAP_CEILING


def _bns(blk):
    return [blk.bn1, blk.bn2] + ([blk.downsample[1]] if hasattr(blk, "downsample") else [])


def _param_grads(blk):
    got = dict(blk.named_parameters())
    return [got[k].grad.detach().clone() for k in BLOCK_NAMES[hasattr(blk, "downsample")]]


_REFS = {}


def _reference(key, size):
    """(the block's starting state, x, up, and the fp64 reference's y, parameter gradients, dx, batch statistics and moved running
    buffers), computed once per case and left unchanged."""
    if (key, size) not in _REFS:
        cin, width, stride = GEOMETRIES[key]
        blk = l3t._seeded_block(cin, width, stride, SEEDS[key]).train()
        x, up = l3t._inputs(cin, width, stride, size)
        ref = copy.deepcopy(blk).to(device="cpu", dtype=torch.float64)
        xr = x.double().requires_grad_(True)
        seen = []
        yr = bn4._ref_block(ref, xr, seen)
        yr.backward(up.double())
        want = dict(ref.named_parameters())
        running = [(b.running_mean.clone(), b.running_var.clone()) for b in _bns(ref)]
        _REFS[(key, size)] = (blk, copy.deepcopy(blk.state_dict()), x, up, yr.detach(), {k: want[k].grad.clone() for k in BLOCK_NAMES[stride == 2]},
                              xr.grad.clone(), seen, running)
    return _REFS[(key, size)]


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("key", sorted(SEEDS))
def test_block_against_fp64(hip, key, size):
    """layer3's two blocks (y, the six / nine gradients, dx, the statistics, the running buffers and the counters) and layer4's stride-2
    block, whose dx is new on this path."""
    cin, width, stride = GEOMETRIES[key]
    blk, state, x, up, yr, gr, dxr, seen, running = _reference(key, size)
    blk.load_state_dict(state)
    blk.zero_grad(set_to_none=True)
    h, w = size
    # the statistics the forward reports, on a copy of the block (the call moves the running statistics)
    probe = copy.deepcopy(blk)
    geom, eps, learn, stats = probe._train_operands(torch.device("cuda", torch.cuda.current_device()), general=True)
    with torch.no_grad():
        _, _, bstats = nets._block_forward_raw(nets.pack_tap(x.cuda()), (2, h * stride, w * stride, *geom), eps, learn, stats, nets._BLOCK_BN,
                                               (True, probe.bn1.momentum))
    e_stats = max(_rel(bstats[i, j].double().cpu().numpy(), seen[i][j].numpy()) for i in range(len(seen)) for j in range(2))
    if len(seen) == 2:
        assert bool(torch.isnan(bstats[2]).all()), "the third statistics row was written without a downsample"
    xg = x.cuda().requires_grad_(True)
    y = nets.basic_block_bn_train(blk, xg)
    assert y.shape == (2, width, h, w) and y.dtype == torch.float32 and y.requires_grad
    y.backward(up.cuda())
    e_run = 0.0
    for a, (rm, rv), p in zip(_bns(blk), running, _bns(probe)):
        assert int(a.num_batches_tracked) == 1
        assert torch.equal(a.running_mean, p.running_mean) and torch.equal(a.running_var, p.running_var)
        e_run = max(e_run, _rel(a.running_mean.double().cpu().numpy(), rm.numpy()), _rel(a.running_var.double().cpu().numpy(), rv.numpy()))
    got = dict(blk.named_parameters())
    errs = {k: _rel(got[k].grad.double().cpu().numpy(), gr[k].numpy()) for k in gr}
    assert len(errs) == (9 if stride == 2 else 6) and all(bool(torch.isfinite(got[k].grad).all()) for k in gr)
    # gamma = 0 (bn2 channel 3): conv2's weight gradient of that channel vanishes exactly, dgamma does not
    assert float(got["conv2.weight"].grad[3].abs().max()) == 0.0 and float(got["bn2.weight"].grad[3].abs()) > 0
    assert xg.grad is not None and xg.grad.shape == x.shape and bool(torch.isfinite(xg.grad).all())
    e_y = _rel(y.detach().double().cpu().numpy(), yr.numpy())
    e_dx = _rel(xg.grad.double().cpu().numpy(), dxr.numpy())
    disagree = (y.detach().cpu() > 0) != (yr > 0)
    flips, agree = int(disagree.sum()), 1.0 - float(disagree.float().mean())
    worst = max(errs, key=errs.get)
    print(f"MEASURED bn3 {key} {h}x{w}: y {e_y:.3g}, grad {errs[worst]:.3g} ({worst}), dx {e_dx:.3g}, stats {e_stats:.3g}, running {e_run:.3g}, "
          f"ReLU sign flips {flips} of {disagree.numel()} (agreement {agree:.5f}); {errs}")
    assert agree > 0.99      # a cap, not a measurement: the reference's own fp16-rounded forward stays far inside it
    b = BLOCK_BOUNDS[key]
    assert e_y <= b["y"] and errs[worst] <= b["grad"] and e_dx <= b["dx"] and e_stats <= b["stats"] and e_run <= b["running"], (e_y, errs, e_dx, e_stats,
                                                                                                                             e_run)


def _run(fn, blk, x, up, want_dx):
    blk.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(want_dx)
    y = fn(blk, xg)
    y.backward(up)
    return [y.detach()] + ([xg.grad] if want_dx else []) + _param_grads(blk)


def _gpu_inputs(key, size):
    x, up = l3t._inputs(*GEOMETRIES[key], size)
    return x.cuda(), up.cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["l4s1", "l4s2"])
def test_layer4_geometries_are_the_bits_of_the_old_entries(hip, key):
    """vtd_block_bn_train_* against vtd_resblock_bn_train_* on deep copies: equal y, parameter gradients, running buffers and, at stride 1,
    dx.  The old entries form no dx at stride 2; the new entries' parameter gradients do not depend on it."""
    cin, width, stride = GEOMETRIES[key]
    old = l3t._seeded_block(cin, width, stride, 91).train()
    new, new_dx = copy.deepcopy(old), copy.deepcopy(old)
    x, up = _gpu_inputs(key, (5, 4))
    want = _run(lambda b, t: nets.basic_block_train(b, t, batch_stats=True), old, x, up, stride == 1)
    got = _run(nets.basic_block_bn_train, new, x, up, stride == 1)
    assert len(got) == len(want) == (8 if stride == 1 else 10)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), i
    for a, b in zip(new.buffers(), old.buffers()):
        assert torch.equal(a, b)
    assert all(int(b.num_batches_tracked) == 1 for b in _bns(new))
    if stride == 2:
        with_dx = _run(nets.basic_block_bn_train, new_dx, x, up, True)
        assert len(with_dx) == 11 and float(with_dx[1].abs().max()) > 0
        for a, b in zip([with_dx[0]] + with_dx[2:], want):
            assert torch.equal(a, b)
        with pytest.raises(RuntimeError, match="stride-2 block"):      # the old spelling still refuses it
            nets.basic_block_train(old, x.clone().requires_grad_(True), batch_stats=True)


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(GEOMETRIES))
def test_eval_mode_is_the_frozen_path(hip, key):
    cin, width, stride = GEOMETRIES[key]
    blk = l3t._seeded_block(cin, width, stride, 92).eval()
    x, up = _gpu_inputs(key, (5, 4))
    buffers = [b.detach().clone() for b in blk.buffers()]
    want = _run(nets.basic_block_train, blk, x, up, True)
    got = _run(nets.basic_block_bn_train, blk, x, up, True)
    assert len(got) == len(want) == (11 if stride == 2 else 8)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), i
    assert all(torch.equal(a, b) for a, b in zip(buffers, blk.buffers())), "eval() wrote the buffers"


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["l3s2", "l4s2"])
def test_bitwise_repeatable_scaled_and_independent_of_dx(hip, key):
    cin, width, stride = GEOMETRIES[key]
    blk = l3t._seeded_block(cin, width, stride, 93).train()
    x, up = _gpu_inputs(key, (12, 11))
    state = copy.deepcopy(blk.state_dict())
    runs, buffers = [], []
    for scale, want_dx in ((1.0, True), (1.0, True), (2.0 ** -23, True), (1.0, False)):
        blk.load_state_dict(state)
        runs.append(_run(nets.basic_block_bn_train, blk, x, up * scale, want_dx))
        buffers.append([b.detach().clone() for b in blk.buffers()])
    assert len(runs[0]) == 11 and len(runs[3]) == 10 and float(runs[0][1].abs().max()) > 0
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    for other in buffers[1:]:
        assert all(torch.equal(a, b) for a, b in zip(buffers[0], other))
    assert torch.equal(runs[2][0], runs[0][0])
    for a, c in zip(runs[0][1:], runs[2][1:]):
        assert torch.equal(c, a * 2.0 ** -23), "a power-of-two smaller upstream gradient must give the same bits, scaled"
    for a, b in zip([runs[0][0]] + runs[0][2:], runs[3]):
        assert torch.equal(a, b), "the parameter gradients must not depend on whether dx is formed"


# ---- layer3 -> layer4 -> FPN -> head -> HIP loss on padded taps
_CHAIN = {}


def _loss_step(out, targets):
    out["probability"].retain_grad()
    out["threshold"].retain_grad()
    training.detection_loss(out, {k: v.cuda() for k, v in targets.items()})["loss"].backward()
    return out["probability"].grad, out["threshold"].grad


def _chain():
    """One step of the deeper node, computed once: the modules after it, deep copies of them from before it, the taps, and C4 / C5 as the
    kernels store them (from a probe with the same starting buffers)."""
    if not _CHAIN:
        l3, l4, fpn, head, feats, targets, padded = l3t._chain_setup()
        l3.train()
        l4.train()
        start = copy.deepcopy((l3, l4, fpn, head))
        probe = copy.deepcopy((l3, l4))
        x, taps = padded[1], []
        with torch.no_grad():
            for st, layer in zip(nets._STAGES[2:], probe):
                _, geoms, eps, learn, stats = nets._stage_operands(st, layer, x)
                for g, lr, s in zip(geoms, learn, stats):
                    x = nets._block_forward_raw(x, g, eps, lr, s, nets._BLOCK_BN, (True, 0.1))[0]
                    taps.append(x)
        out = fpn.forward_padded(padded, head=head, layer4=l4, layer3=l3, trunk_batch_stats=STAGES)
        ups = _loss_step(out, targets)
        _CHAIN.update(mods=(l3, l4, fpn, head), start=start, probe=probe, feats=feats, targets=targets, padded=padded, c4p=taps[1], c5p=taps[3],
                      mids=(taps[0], taps[2]), out=out, ups=ups)
    return _CHAIN


@pytest.mark.gpu
def test_chain_layer3_layer4_fpn_head_loss_against_fp64(hip):
    """Stage-isolated at C4, C5 and P2 as tests/test_gpu_layer3_train.py's chain, with train-mode BatchNorm in the reference stages: the
    reference layer4's upstream gradient is the reference FPN's dC5, the reference layer3's is the reference layer4.0's dx plus the reference
    FPN's dC4."""
    c = _chain()
    l3, l4, fpn, head = c["mods"]
    rl3, rl4 = (copy.deepcopy(m).to(device="cpu", dtype=torch.float64) for m in c["start"][:2])
    rfpn, rhead = l4t._rounded_fpn(fpn), neck._rounded_head(c["start"][3]).train()
    c4p, c5p, feats = c["c4p"], c["c5p"], c["feats"]
    assert c4p.shape == (2, 8, 6, 256) and c5p.shape == (2, 5, 4, 512)
    p2p = fpn.forward_padded(c["padded"] + [c4p, c5p])
    x = l3t._unpad(p2p).requires_grad_(True)
    torch.autograd.backward([rhead.probability_head(x), rhead.threshold_head(x)], [u.double().cpu() for u in c["ups"]])
    c4f, c5 = l3t._unpad(c4p).requires_grad_(True), l3t._unpad(c5p).requires_grad_(True)
    l4t._wiring(rfpn, [t.double() for t in feats] + [c4f, c5]).backward(x.grad)
    c4b = l3t._unpad(c4p).requires_grad_(True)
    mid4 = bn4._ref_block(rl4[0], c4b)
    c5r = bn4._ref_block(rl4[1], l3t._rounded(mid4))
    c5r.backward(c5.grad)
    share = float(c4f.grad.norm() / (c4b.grad + c4f.grad).norm())
    mid3 = bn4._ref_block(rl3[0], feats[1].double())
    c4r = bn4._ref_block(rl3[1], l3t._rounded(mid3))
    c4r.backward(c4b.grad + c4f.grad)
    # the outputs whose ReLU sign differs from the reference's, per block from layer3.0 up (each stage's reference on the input the kernels had)
    flips = [int(((l3t._unpad(t) > 0) != (r.detach() > 0)).sum()) for t, r in zip((c["mids"][0], c4p, c["mids"][1], c5p), (mid3, c4r, mid4, c5r))]
    errs = {}
    for name, m, r in (("layer3", l3, rl3), ("layer4", l4, rl4)):
        got, want = dict(m.named_parameters()), dict(r.named_parameters())
        errs[name] = {k: _rel(got[k].grad.double().cpu().numpy(), want[k].grad.numpy()) for k in l3t.L_NAMES}
    assert [len(errs[k]) for k in ("layer3", "layer4")] == [15, 15]
    worst = {k: max(v, key=v.get) for k, v in errs.items()}
    e_run = 0.0
    for m, r, p in zip((l3, l4), (rl3, rl4), c["probe"]):
        for blk, rblk, pblk in zip(m, r, p):
            for a, b, q in zip(_bns(blk), _bns(rblk), _bns(pblk)):
                assert int(a.num_batches_tracked) == 1
                assert torch.equal(a.running_mean, q.running_mean) and torch.equal(a.running_var, q.running_var)
                e_run = max(e_run, _rel(a.running_mean.double().cpu().numpy(), b.running_mean.numpy()),
                            _rel(a.running_var.double().cpu().numpy(), b.running_var.numpy()))
    print("MEASURED bn3 chain: " + ", ".join(f"{k} grad {errs[k][worst[k]]:.3g} ({worst[k]})" for k in errs) +
          f"; running buffers {e_run:.3g}; the FPN's share of dC4 {share:.3g}; ReLU sign flips of layer3.0, layer3.1, layer4.0, layer4.1: "
          f"{flips} of {[mid3.numel(), c4r.numel(), mid4.numel(), c5r.numel()]} outputs; {errs}")
    assert share > 10 * GRAD_CEILING, "the FPN's dC4 must matter in this case, or leaving it out would pass"
    assert e_run <= CHAIN_RUNNING_BOUND
    for k in errs:
        assert errs[k][worst[k]] <= CHAIN_BOUNDS[k], (k, errs[k])


@pytest.mark.gpu
def test_ladder_layer4_batch_node_on_the_deeper_nodes_c4(hip):
    """The layer4-only batch node (trunk_batch_stats=True, the 512-only entries, no dx) on the C4 the deeper node produced, from deep copies of
    the same starting modules: the same bits for both maps, layer4's 15, the FPN's 10 and the head's 20 gradients, and layer4's running
    buffers."""
    c = _chain()
    l3, l4, fpn, head = c["mods"]
    _, l4b, fpnb, headb = copy.deepcopy(c["start"])
    out = fpnb.forward_padded(c["padded"] + [c["c4p"]], head=headb, layer4=l4b, trunk_batch_stats=True)
    _loss_step(out, c["targets"])
    assert torch.equal(out["probability"], c["out"]["probability"]) and torch.equal(out["threshold"], c["out"]["threshold"])
    pairs = list(zip(l4.parameters(), l4b.parameters())) + list(zip(fpn.live_parameters(), fpnb.live_parameters())) + \
        list(zip(head.parameters(), headb.parameters()))
    assert len(pairs) == 15 + 10 + 20
    differ = [i for i, (a, b) in enumerate(pairs) if not torch.equal(a.grad, b.grad)]
    assert all(float(a.grad.abs().max()) > 0 for a, _ in pairs) and not differ, differ
    moved = 0
    for (k, a), b, s in zip(l4.state_dict().items(), l4b.state_dict().values(), c["start"][1].state_dict().values()):
        assert torch.equal(a, b), k
        moved += ("running" in k or "num_batches" in k) and not torch.equal(a, s)
    assert moved == 15      # ten running buffers and five counters


# ---- the product path
@pytest.mark.gpu
def test_product_step_with_batch_statistics_in_layer3_and_layer4(hip):
    from vtd_amd._fixtures.weights import stress_detector_state_dict
    torch.manual_seed(3)
    sd = stress_detector_state_dict("resnet18", 17)
    gen = torch.Generator().manual_seed(23)
    x = torch.randn((2, 3, 640, 640), generator=gen).cuda()
    targets = neck._random_targets((2, 1, 640, 640), gen)

    net = nets.DBNet("resnet18", compute_threshold=True, trainable=MODE, trunk_bn=STAGES)
    net.load_state_dict(sd)
    net.cuda().train()
    te = net.trunk_engine()
    mod = training.TextDetectionLightningModule(net)
    opt = mod.configure_optimizers()["optimizer"]
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    loss = mod.training_step((x, targets), 0)
    opt.zero_grad()
    loss.backward()
    trained = {f"backbone.{i}.{k}": p for i in (6, 7) for k, p in net.backbone[i].named_parameters()}
    assert len(trained) == 30
    for k, p in trained.items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k
    for i in range(6):
        assert all(p.grad is None for p in net.backbone[i].parameters())
    opt.step()
    after = net.state_dict()
    for k in trained:
        assert not torch.equal(before[k], after[k]), f"{k} did not change"
    moved = [k for k in before if k.startswith(("backbone.6.", "backbone.7.")) and "running" in k]
    counts = [k for k in before if k.startswith(("backbone.6.", "backbone.7.")) and "num_batches" in k]
    assert len(moved) == 20 and len(counts) == 10
    for k in moved:
        assert bool(torch.isfinite(after[k]).all()) and not torch.equal(before[k], after[k]), f"{k} did not move"
    for k in counts:
        assert int(after[k]) == 1, k
    for k in before:
        if k.startswith("backbone.") and not k.startswith(("backbone.6.", "backbone.7.")):
            assert torch.equal(before[k], after[k]), f"{k} changed"
    assert net.trunk_engine() is te, "a step on layer3 / layer4 / FPN / head tensors rebuilt the trunk engine"
    loss2 = mod.training_step((x, targets), 1)
    assert bool(torch.isfinite(loss2)) and float(loss2) != float(loss)
    assert all(int(net.state_dict()[k]) == 2 for k in counts)
    assert net.trunk_engine() is te
    # a following eval() forward runs the fused inference engine on the stepped weights and the moved statistics
    net.eval()
    with torch.no_grad():
        got = net(x)
    fresh = nets.DBNet("resnet18", compute_threshold=True)
    fresh.load_state_dict(net.state_dict())
    with torch.no_grad():
        want = fresh.cuda().eval()(x)
    assert torch.equal(got["probability"], want["probability"]) and torch.equal(got["threshold"], want["threshold"])
