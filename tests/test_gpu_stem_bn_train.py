"""Train-mode (batch-statistics) BatchNorm for ResNet-18's stem on the GPU (csrc/stem_train.hip behind vtd_stem_bn_train_*): the stem through
`nets.stem_bn_train(conv, bn, x)`, the stem -> layer1 -> layer2 -> layer3 -> layer4 -> FPN -> head node with `stem_batch_stats=True`, and
`DBNet("resnet18", trainable="head+fpn+backbone", trunk_bn="backbone")`.

The fp64 reference is CPU autograd in float64: x as given (fp16-representable), the raw convolution weights rounded to fp16 straight through,
F.batch_norm(..., training=True), ReLU, a rounded to fp16 straight through (the kernels form a in fp16 and pool it without storing it),
max_pool2d(3, 2, 1, return_indices=True).  The stem is tests/test_stem_train.py's `stem_modules(71)`: gamma = 0 with beta > 0 in channel 3,
gamma = -0.75 in channel 7.  Metric: relative L2 error per tensor.  Bounds: 3x the level measured on an MI355X, worst over the sizes, never
above the ceilings of 2e-3 for maps, statistics and running buffers and 1e-2 for gradients; 3x is the project's standing
allowance for an fp16-operand path.

Seed 71 was fixed before any GPU run: for seeds 71 .. 78 a float32 evaluation of this reference agrees with the float64 one on every ReLU
sign and on every pooling index of a live element at the four sizes and at 2 x 2.  It was not re-picked after the GPU numbers."""
import copy

import pytest
import torch

import test_gpu_fpn_neck_train as neck
import test_gpu_layer1_bn_train as l1bn
import test_gpu_layer3_train as l3t
import test_gpu_layer4_bn_train as bn4
import test_gpu_layer4_train as l4t
import test_gpu_stem_train as gst
import test_stem_bn_train as sbc
import test_stem_train as sc
from vtd_amd import nets, training  # noqa: F401
from vtd_amd.nets import stem_bn_train  # noqa: F401  (the feature under test: absent before it)

_rel, _unpad, _rounded, _loss_step = l4t._rel, l3t._unpad, l3t._rounded, l1bn._loss_step
MAP_CEILING, GRAD_CEILING = 2e-3, 1e-2
SIZES, LARGE, ZERO_CH, NEG_CH = sc.SIZES, sc.LARGE, sc.ZERO_CH, sc.NEG_CH      # the sizes' arithmetic stands in tests/test_stem_bn_train.py
STEM_NAMES = gst.STEM_NAMES
SEED = 71
IDX_CAP = 0.01      # the share of live pooled elements whose index may differ from torch's: a condition, the reference alone is at 0
STAGES = l1bn.STAGES
MODE = "head+fpn+backbone"

# bounds: 3x the level measured on an MI355X, worst of the four sizes (grad: worst of the three gradients), never above the ceiling.
# Measured (4 x 4, 10 x 14, 36 x 44, 54 x 38): pool 0, 0, 0, 1.50e-7 (the pooled values are fp16 and the reference rounds a to fp16: at the
# first three sizes every pooled value has the reference's bits); grad 1.77e-4, 1.97e-4, 2.04e-4, 2.09e-4 (0.weight at every size; 1.weight
# is at 8.8e-8 .. 1.04e-7 and 1.bias at 2.1e-8 .. 3.0e-8: fp64 sums of fp32 values); statistics 9.92e-8, 9.35e-8, 1.28e-7, 1.70e-7; running
# buffers 2.78e-8, 2.56e-8, 2.81e-8, 2.86e-8.  No index of a live pooled element differs from torch's (0 of 126, 1475, 12 579 and 17 742) and
# no ReLU sign (0 of 128, 1536, 12 672 and 17 920 pooled values).  The multi-workgroup, two-slab size sits at the level of the small ones
STEM_BOUNDS = {"pool": 4.5e-7, "grad": 6.3e-4, "stats": 5.1e-7, "running": 8.6e-8}
assert all(STEM_BOUNDS[k] <= (GRAD_CEILING if k == "grad" else MAP_CEILING) for k in ("pool", "grad", "stats", "running"))
# the node at C5 = 3 x 2 (a 96 x 64 image, pool and C2 = 24 x 16), n = 2, at the seeds of tests/test_stem_bn_train.py (chosen on the CPU, not
# re-picked): the worst of the stem's three gradients, measured 3.38e-3 (1.bias; 0.weight 2.35e-3, 1.weight 2.87e-3), its running buffers at
# 2.74e-8.  On the MI355X three of the nine outputs have one ReLU sign each that differs from the reference stage's (layer1.0, layer1.1 and
# layer3.1: [0, 1, 1, 0, 0, 0, 1, 0, 0]), which the float32 stand-in did not have; the stages above sit at 4.46e-3 (layer1), 1.72e-3, 2.60e-3
# and 6.16e-4, and the stem below them inherits their dpool: its three gradients move together, which is an upstream gradient and not a
# kernel of the stem -- the stem test above has the same kernels at 2.1e-4.  3x the measured level is over the ceiling, so the ceiling is
# the bound
NODE_BOUND = GRAD_CEILING
assert NODE_BOUND <= GRAD_CEILING


def _stem_gpu(seed=SEED):
    conv, bn = sc.stem_modules(seed)
    return torch.nn.Sequential(conv, bn).cuda().train()


_REFS = {}


def _reference(size):
    """(the stem, its starting state, x, up, and the fp64 reference's pooled map, window codes, gradients, batch statistics and moved running
    buffers), computed once per size and left unchanged."""
    if size not in _REFS:
        stem = _stem_gpu()
        x, up = sc.stem_inputs(size)
        ref = copy.deepcopy(stem).to(device="cpu", dtype=torch.float64)
        seen = []
        pool, idx = sbc.ref_stem_bn(ref, x.double(), seen)
        pool.backward(up.double())
        want = dict(ref.named_parameters())
        _REFS[size] = (stem, copy.deepcopy(stem.state_dict()), x, up, pool.detach(), gst._codes(idx, size[1] // 2),
                       {k: want[k].grad.clone() for k in STEM_NAMES}, seen[0], (ref[1].running_mean.clone(), ref[1].running_var.clone()))
    return _REFS[size]


def _raw_forward(stem, x):
    """The raw training = 1 forward on a copy of the stem: (the pooled padded tap, the index bytes, stats_dev, the copy)."""
    probe = copy.deepcopy(stem)
    tap = nets.pack_image(x)
    geom, eps, learn, stats = nets._stem_operands(probe[0], probe[1], tap)
    out = torch.full((2, 64), float("nan"), dtype=torch.float32, device=tap.device)
    with torch.no_grad():
        poolp, idx, _ = nets._stem_forward_raw(tap, geom, eps, [t.detach() for t in learn], stats, (True, probe[1].momentum), out)
    return poolp, idx, out, probe


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stem_bn_against_fp64(hip, size):
    stem, state, x, up, pr, cr, gr, seen, running = _reference(size)
    stem.load_state_dict(state)
    stem.zero_grad(set_to_none=True)
    assert float(stem[1].weight[ZERO_CH].detach()) == 0.0 and float(stem[1].bias[ZERO_CH].detach()) > 0 and float(stem[1].weight[NEG_CH].detach()) < 0
    xg = x.cuda()
    poolp, idx, bstats, probe = _raw_forward(stem, xg)
    e_stats = max(_rel(bstats[j].double().cpu().numpy(), seen[j].numpy()) for j in range(2))
    y = nets.stem_bn_train(stem[0], stem[1], xg)
    assert y.shape == pr.shape and y.dtype == torch.float32 and y.requires_grad
    y.backward(up.cuda())
    assert xg.grad is None
    assert int(stem[1].num_batches_tracked) == 1
    assert torch.equal(stem[1].running_mean, probe[1].running_mean) and torch.equal(stem[1].running_var, probe[1].running_var)
    e_run = max(_rel(stem[1].running_mean.double().cpu().numpy(), running[0].numpy()), _rel(stem[1].running_var.double().cpu().numpy(), running[1].numpy()))
    got = dict(stem.named_parameters())
    errs = {k: _rel(got[k].grad.double().cpu().numpy(), gr[k].numpy()) for k in STEM_NAMES}
    assert all(bool(torch.isfinite(got[k].grad).all()) for k in STEM_NAMES)
    e_pool = _rel(y.detach().double().cpu().numpy(), pr.numpy())
    assert torch.equal(poolp[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).float(), y.detach()) and idx.dtype == torch.uint8
    t = poolp.float()
    assert float(t[:, 0].abs().max()) == 0 and float(t[:, -1].abs().max()) == 0 and float(t[:, :, 0].abs().max()) == 0 \
        and float(t[:, :, -1].abs().max()) == 0, "the ring must be zero"
    cg = idx.permute(0, 3, 1, 2).cpu().long()
    live = (y.detach().cpu() > 0) | (pr > 0)
    differ = int(((cg != cr) & live).sum())
    share = differ / max(int(live.sum()), 1)
    disagree = (y.detach().cpu() > 0) != (pr > 0)
    agree = 1.0 - float(disagree.float().mean())
    worst = max(errs, key=errs.get)
    print(f"MEASURED stem bn {size[0]}x{size[1]}: pool {e_pool:.3g}, grad {errs[worst]:.3g} ({worst}), stats {e_stats:.3g}, running {e_run:.3g}, indices "
          f"that differ {differ} of {int(live.sum())} live, ReLU sign flips {int(disagree.sum())} of {disagree.numel()}; {errs}")
    # conditions, not measurements: the reference's own float32 evaluation is at 0 and 1.0 at this seed
    assert share <= IDX_CAP, (differ, int(live.sum()))
    assert agree > 0.99
    # gamma = 0: the weight gradient of that channel vanishes exactly, dgamma does not
    assert float(got["0.weight"].grad[ZERO_CH].abs().max()) == 0.0 and float(got["1.weight"].grad[ZERO_CH].abs()) > 0
    b = STEM_BOUNDS
    assert e_pool <= b["pool"] and errs[worst] <= b["grad"] and e_stats <= b["stats"] and e_run <= b["running"], (e_pool, errs, e_stats, e_run)


def _run(fn, stem, x, up):
    stem.zero_grad(set_to_none=True)
    y = fn(stem[0], stem[1], x)
    y.backward(up)
    return [y.detach()] + [p.grad.clone() for p in stem.parameters()]


@pytest.mark.gpu
def test_two_rows_finite_and_repeatable(hip):
    """A 2 x 2 image at n = 2: M = 2 rows, fourteen of the sixteen parts are empty, and dz is pure cancellation with two values per channel,
    so there is no accuracy bound: every output is finite, two runs from one starting state give the same bits, and the counter advances."""
    stem = _stem_gpu(72)
    x, up = (t.cuda() for t in sc.stem_inputs((2, 2)))
    state = copy.deepcopy(stem.state_dict())
    runs, buffers = [], []
    for _ in range(2):
        stem.load_state_dict(state)
        runs.append(_run(nets.stem_bn_train, stem, x, up))
        buffers.append([b.detach().clone() for b in stem.buffers()])
        assert int(stem[1].num_batches_tracked) == 1
    assert len(runs[0]) == 4 and all(bool(torch.isfinite(t).all()) for t in runs[0]) and all(bool(torch.isfinite(b).all()) for b in buffers[0])
    assert all(torch.equal(a, b) for a, b in zip(*runs)) and all(torch.equal(a, b) for a, b in zip(*buffers))
    _run(nets.stem_bn_train, stem, x, up)
    assert int(stem[1].num_batches_tracked) == 2
    assert not torch.equal(stem[1].running_mean, state["1.running_mean"].to(stem[1].running_mean.device))


@pytest.mark.gpu
def test_eval_mode_is_the_frozen_path(hip):
    """eval(): the bits of nets.stem_train (the vtd_stem_train_* path) for the pooled map and the three gradients, and no buffer is written."""
    stem = _stem_gpu(73).eval()
    x, up = (t.cuda() for t in sc.stem_inputs((10, 14)))
    buffers = [b.detach().clone() for b in stem.buffers()]
    want = _run(nets.stem_train, stem, x, up)
    got = _run(nets.stem_bn_train, stem, x, up)
    assert len(got) == len(want) == 4 and float(got[1].abs().max()) > 0
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), i
    assert all(torch.equal(a, b) for a, b in zip(buffers, stem.buffers())), "eval() wrote the buffers"


@pytest.mark.gpu
def test_bitwise_repeatable_and_scaled(hip):
    """At the multi-slab size (five statistics workgroups, two weight-gradient slabs): two runs give the same bits, and an upstream gradient
    smaller by 2^-23 gives the same gradient bits, scaled."""
    stem = _stem_gpu(73)
    x, up = (t.cuda() for t in sc.stem_inputs(LARGE))
    state = copy.deepcopy(stem.state_dict())
    runs, buffers = [], []
    for scale in (1.0, 1.0, 2.0 ** -23):
        stem.load_state_dict(state)
        runs.append(_run(nets.stem_bn_train, stem, x, up * scale))
        buffers.append([b.detach().clone() for b in stem.buffers()])
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
    for other in buffers[1:]:
        assert all(torch.equal(a, b) for a, b in zip(buffers[0], other))
    assert torch.equal(runs[2][0], runs[0][0])
    for a, c in zip(runs[0][1:], runs[2][1:]):
        assert float(c.abs().max()) > 0 and torch.equal(c, a * 2.0 ** -23), "a power-of-two smaller upstream gradient must give the same bits, scaled"


# ---- stem -> layer1 -> layer2 -> layer3 -> layer4 -> FPN -> head -> HIP loss on a 96 x 64 image (pooled 24 x 16, C5 = 3 x 2)
_CHAIN = {}


def _chain():
    """One step of the whole-backbone batch node, computed once: the modules after it, deep copies of them from before it, the image, and the
    pooled tap and the eight block outputs as the kernels store them (from a probe with the same starting buffers)."""
    if not _CHAIN:
        stem, blocks, fpn, head, x, targets = sbc.chain_modules()
        stem = stem.cuda().train()
        l1, l2, l3, l4 = (torch.nn.Sequential(*blocks[i:i + 2]).cuda().train() for i in (0, 2, 4, 6))
        fpn, head = fpn.cuda(), head.cuda().train()
        tap = nets.pack_image(x.cuda())
        start = copy.deepcopy((stem, l1, l2, l3, l4, fpn, head))
        poolp, _, _, sprobe = _raw_forward(stem, x.cuda())
        probe = copy.deepcopy((l1, l2, l3, l4))
        t, taps = poolp, []
        with torch.no_grad():
            for st, layer in zip(nets._STAGES, probe):
                _, geoms, eps, learn, stats = nets._stage_operands(st, layer, t)
                for g, lr, s in zip(geoms, learn, stats):
                    t = nets._block_forward_raw(t, g, eps, lr, s, nets._TRUNK_BN, (True, 0.1))[0]
                    taps.append(t)
        out = fpn.forward_padded([tap], head=head, layer4=l4, layer3=l3, layer2=l2, layer1=l1, stem=(stem[0], stem[1]), trunk_batch_stats=STAGES,
                                 stem_batch_stats=True)
        ups = _loss_step(out, targets)
        _CHAIN.update(mods=(stem, l1, l2, l3, l4, fpn, head), start=start, sprobe=sprobe, x=x, targets=targets, poolp=poolp, taps=taps, out=out, ups=ups)
    return _CHAIN


@pytest.mark.gpu
def test_ladder_node_with_batch_stem(hip):
    """The four-stage batch node on the pooled tap the stem wrote, from deep copies of the same starting modules: the same bits for both maps,
    the 87 upper gradients and the four stages' buffers.  The stem's three gradients are finite and non-zero, its two running buffers moved and
    its counter is 1."""
    c = _chain()
    stem, l1, l2, l3, l4, fpn, head = c["mods"]
    stem0, l1b, l2b, l3b, l4b, fpnb, headb = copy.deepcopy(c["start"])
    assert c["poolp"].shape == (2, 26, 18, 64)
    out = fpnb.forward_padded([c["poolp"]], head=headb, layer4=l4b, layer3=l3b, layer2=l2b, layer1=l1b, trunk_batch_stats=STAGES)
    _loss_step(out, c["targets"])
    assert torch.equal(out["probability"], c["out"]["probability"]) and torch.equal(out["threshold"], c["out"]["threshold"])
    pairs = [(a, b) for m, mb in ((l1, l1b), (l2, l2b), (l3, l3b), (l4, l4b)) for a, b in zip(m.parameters(), mb.parameters())] + \
        list(zip(fpn.live_parameters(), fpnb.live_parameters())) + list(zip(head.parameters(), headb.parameters()))
    assert len(pairs) == 87
    differ = [i for i, (a, b) in enumerate(pairs) if not torch.equal(a.grad, b.grad)]
    assert all(float(a.grad.abs().max()) > 0 for a, _ in pairs) and not differ, differ
    for m, mb in ((l1, l1b), (l2, l2b), (l3, l3b), (l4, l4b)):
        for (k, a), b in zip(m.state_dict().items(), mb.state_dict().values()):
            assert torch.equal(a, b), k
    for p in stem.parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
    assert not torch.equal(stem[1].running_mean, stem0[1].running_mean) and not torch.equal(stem[1].running_var, stem0[1].running_var)
    assert torch.equal(stem[1].running_mean, c["sprobe"][1].running_mean) and torch.equal(stem[1].running_var, c["sprobe"][1].running_var)
    assert int(stem[1].num_batches_tracked) == 1 and int(stem0[1].num_batches_tracked) == 0


@pytest.mark.gpu
def test_node_stem_against_fp64(hip):
    """Stage-isolated, built like tests/test_gpu_stem_train.py's chain test with the train-mode references of tests/test_gpu_layer1_bn_train.py's
    node test: the reference stem reads the image, each reference above it the tap the kernels stored.  The gradient chain is end to end: the
    reference stem's upstream gradient is the reference layer1.0's dx."""
    c = _chain()
    stem, l1, l2, l3, l4, fpn, head = c["mods"]
    rstem, rl1, rl2, rl3, rl4 = (copy.deepcopy(m).to(device="cpu", dtype=torch.float64) for m in c["start"][:5])
    rfpn, rhead = l4t._rounded_fpn(fpn), neck._rounded_head(c["start"][6]).train()
    mid1p, c2p, mid2p, c3p, mid3p, c4p, mid4p, c5p = c["taps"]
    assert c2p.shape == (2, 26, 18, 64) and c5p.shape == (2, 5, 4, 512)
    p2p = fpn.forward_padded([c2p, c3p, c4p, c5p])
    x = _unpad(p2p).requires_grad_(True)
    torch.autograd.backward([rhead.probability_head(x), rhead.threshold_head(x)], [u.double().cpu() for u in c["ups"]])
    c2f, c3f, c4f, c5 = (_unpad(t).requires_grad_(True) for t in (c2p, c3p, c4p, c5p))
    l4t._wiring(rfpn, [c2f, c3f, c4f, c5]).backward(x.grad)
    c4b = _unpad(c4p).requires_grad_(True)
    mid4 = bn4._ref_block(rl4[0], c4b)
    c5r = bn4._ref_block(rl4[1], _rounded(mid4))
    c5r.backward(c5.grad)
    c3b = _unpad(c3p).requires_grad_(True)
    mid3 = bn4._ref_block(rl3[0], c3b)
    c4r = bn4._ref_block(rl3[1], _rounded(mid3))
    c4r.backward(c4b.grad + c4f.grad)
    c2b = _unpad(c2p).requires_grad_(True)
    mid2 = bn4._ref_block(rl2[0], c2b)
    c3r = bn4._ref_block(rl2[1], _rounded(mid2))
    c3r.backward(c3b.grad + c3f.grad)
    poolb = _unpad(c["poolp"]).requires_grad_(True)
    mid1 = bn4._ref_block(rl1[0], poolb)
    c2r = bn4._ref_block(rl1[1], _rounded(mid1))
    c2r.backward(c2b.grad + c2f.grad)
    dpool = poolb.grad      # the reference layer1.0's dx: the conv path's transpose plus the identity's g2
    pool_r, _ = sbc.ref_stem_bn(rstem, c["x"].double(), [])
    pool_r.backward(dpool)
    refs = (pool_r, mid1, c2r, mid2, c3r, mid3, c4r, mid4, c5r)
    flips = [int(((_unpad(t) > 0) != (r.detach() > 0)).sum()) for t, r in zip([c["poolp"]] + c["taps"], refs)]
    # what of layer1.0's dx reaches the stem: its part at live pooled elements, as a share of the whole
    reach = float((dpool * (pool_r.detach() > 0)).norm() / dpool.norm())
    got, want = dict(stem.named_parameters()), dict(rstem.named_parameters())
    errs = {k: _rel(got[k].grad.double().cpu().numpy(), want[k].grad.numpy()) for k in STEM_NAMES}
    assert all(bool(torch.isfinite(got[k].grad).all()) and float(got[k].grad.abs().max()) > 0 for k in STEM_NAMES)
    worst = max(errs, key=errs.get)
    upper = {}
    for name, m, r in (("layer1", l1, rl1), ("layer2", l2, rl2), ("layer3", l3, rl3), ("layer4", l4, rl4)):
        gm, wm = dict(m.named_parameters()), dict(r.named_parameters())
        upper[name] = max(_rel(gm[k].grad.double().cpu().numpy(), wm[k].grad.numpy()) for k in (l1bn.L1_NAMES if name == "layer1" else l3t.L_NAMES))
    e_run = max(_rel(stem[1].running_mean.double().cpu().numpy(), rstem[1].running_mean.numpy()),
                _rel(stem[1].running_var.double().cpu().numpy(), rstem[1].running_var.numpy()))
    print(f"MEASURED stem bn node: stem grad {errs[worst]:.3g} ({worst}); running buffers {e_run:.3g}; the share of layer1.0's dx at live pooled elements "
          f"{reach:.3g}; ReLU sign flips of the pooled map, layer1.0, layer1.1, layer2.0, layer2.1, layer3.0, layer3.1, layer4.0, layer4.1: {flips} of "
          f"{[r.numel() for r in refs]} outputs; the worst gradient of the stages above: {', '.join(f'{k} {v:.3g}' for k, v in upper.items())}; {errs}")
    assert reach > 10 * GRAD_CEILING, "layer1.0's dx must carry the stem's signal in this case, or a stem that drops it would pass"
    assert e_run <= STEM_BOUNDS["running"]
    assert errs[worst] <= NODE_BOUND, errs


# ---- the product path
@pytest.mark.gpu
def test_product_step_with_batch_statistics_in_the_whole_backbone(hip):
    from vtd_amd._fixtures.weights import stress_detector_state_dict
    torch.manual_seed(3)
    sd = stress_detector_state_dict("resnet18", 17)
    gen = torch.Generator().manual_seed(23)
    x = torch.randn((2, 3, 640, 640), generator=gen).cuda()
    targets = neck._random_targets((2, 1, 640, 640), gen)

    net = nets.DBNet("resnet18", compute_threshold=True, trainable=MODE, trunk_bn="backbone")
    net.load_state_dict(sd)
    net.cuda().train()
    mod = training.TextDetectionLightningModule(net)
    opt = mod.configure_optimizers()["optimizer"]
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    loss = mod.training_step((x, targets), 0)
    opt.zero_grad()
    loss.backward()
    assert "_trunk_engine" not in net.__dict__ or net.__dict__["_trunk_engine"] is None, "the train-mode forward built a trunk engine"
    trained = sc._trained(net)
    assert len(trained) == 90
    for p in trained:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
    values = [p.detach().clone() for p in trained]
    opt.step()
    assert all(not torch.equal(a, p.detach()) for a, p in zip(values, trained)), "a trained tensor did not change"
    after = net.state_dict()
    moved = [k for k in before if k.startswith("backbone.") and "running" in k]
    counts = [k for k in before if k.startswith("backbone.") and "num_batches" in k]
    assert len(moved) == 40 and len(counts) == 20      # the stem's BatchNorm and 4 + 3 x 5 in the stages
    for k in moved:
        assert bool(torch.isfinite(after[k]).all()) and not torch.equal(before[k], after[k]), f"{k} did not move"
    for k in counts:
        assert int(after[k]) == 1, k
    loss2 = mod.training_step((x, targets), 1)
    assert bool(torch.isfinite(loss2)) and float(loss2.detach()) != float(loss.detach())
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
    # with the default trunk_bn the same mode leaves all 60 buffers alone
    frozen = nets.DBNet("resnet18", compute_threshold=True, trainable=MODE)
    frozen.load_state_dict(sd)
    frozen.cuda().train()
    assert frozen.trunk_bn == "frozen"
    out = frozen(x)
    (out["probability"].mean() + out["threshold"].mean()).backward()
    kept = frozen.state_dict()
    for k in moved + counts:
        assert torch.equal(kept[k].cpu(), sd[k]), f"{k} was written with frozen statistics"
    assert len(moved + counts) == 60
