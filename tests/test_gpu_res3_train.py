"""ResNet-50's res3 (four 128-wide Bottlenecks) on the HIP training kernels (csrc/bottleneck_train.hip at W = 128, the
vtd_bottleneck128_train_* entries), on the GPU: one block through `nets.bottleneck128_train`, the res3 -> res4 -> res5 -> FPN -> head node on
a padded C2 tap, the engine's stop at C2 (`DetectorEngine.forward_c2`) and the product's "head+fpn+res5+res4+res3" mode.

The fp64 reference is tests/test_gpu_res5_train.py's, and the conditioning helpers are tests/test_gpu_res4_train.py's, both taken by
import: the block in float64 under CPU autograd with eval-mode BatchNorm, the folded GEMM weights rounded to fp16 straight through and the
stored activations (a1, a2, id, and the block outputs between blocks) rounded to fp16 straight through.  Metric: relative L2 error per
tensor.  Bounds follow DESIGN.md section 4's convention: 3x the level measured on an MI355X against that reference, under the ceilings of
1e-2 for gradients and 2e-3 for maps.

Conditioning, as in the res4 file.  At width 128 one flipped ReLU mask moves the gradients below it by about sqrt(2 / (n h w 128)) in
relative L2: 2.3e-2 at a 3x2 output with n = 2 and 1.0e-2 at 5x4, at or above the gradient ceiling.  Every case is therefore conditioned on
the CPU, from the reference alone:
  * the small blocks by seed: the input seed is the first from 100 up at which the smallest non-zero ReLU argument exceeds RELU_MARGIN;
  * the many-rows blocks and the thirteen-block chain by construction (`_condition` of the res4 file)."""
import copy

import pytest
import torch

import test_gpu_fpn_neck_train as neck
import test_gpu_layer4_train as l4t
import test_gpu_res5_train as r5t
from test_gpu_layer4_train import _rel
from test_gpu_res4_train import CONSTRUCTED_MARGIN, RES4_NAMES, _condition, _load_from, _seeded_res4
from test_gpu_res5_train import GRAD_CEILING, MAP_CEILING, RELU_MARGIN, _f16, _names, _ref_bottleneck, _relu_margin
from vtd_amd import nets, training

GEOMS = {1: 512, 2: 256}      # stride -> cin
RES3_NAMES = [f"0.{k}" for k in _names(True)] + [f"{i}.{k}" for i in range(1, 4) for k in _names(False)]
assert len(RES3_NAMES) == 39 and len(RES4_NAMES) == 57 and len(r5t.RES5_NAMES) == 30

# 3x the level measured on an MI355X (worst of the cases of each test), capped by the ceilings; the measured levels behind
BLOCK_BOUNDS = {
    "stride1": {"y": 6.3e-4, "grad": 1.2e-3, "dx": 8.1e-5},      # measured 2.10e-4 (5x4), 3.87e-4 (bn1.weight at 1x1), 2.70e-5 (5x4)
    "stride2": {"y": 6.2e-4, "grad": 1.2e-3, "dx": 6.4e-4},      # 2.07e-4 (n = 1, 5x3), 4.05e-4 (bn1.weight at n = 1, 5x3), 2.12e-4 (3x2)
    "rows_stride1": {"y": 5.7e-4, "grad": 1.4e-3, "dx": 8.9e-5},      # 1.90e-4, 4.55e-4 (bn1.weight), 2.97e-5
    "rows_stride2": {"y": 6.1e-4, "grad": 1.2e-3, "dx": 6.4e-4},      # 2.02e-4, 3.87e-4 (bn1.weight), 2.12e-4
}
# worst gradient per stage, C5 = 3x2, n = 2, all thirteen blocks conditioned by construction: measured 8.43e-4 (res3, 3.bn2.weight), 1.04e-3
# (res4, 4.bn1.weight), 9.98e-4 (res5, 2.conv2.weight), 6.11e-4 (FPN, layer_blocks.3.weight), 4.33e-4 (head, probability_head.0.weight).  No
# stage stands out: the level is arithmetic (fp16 operands through up to thirteen blocks), not a flipped mask, which alone would be 9e-3 at
# C3 = 12x8.  The end-to-end maps, printed and not bounded: C3 2.24e-4, C4 5.21e-4, C5 6.72e-4
CHAIN_BOUNDS = {"res3": 2.5e-3, "res4": 3.1e-3, "res5": 3.0e-3, "fpn": 1.8e-3, "head": 1.3e-3}
assert all(v <= (MAP_CEILING if k == "y" else GRAD_CEILING) for b in BLOCK_BOUNDS.values() for k, v in b.items())
assert all(v <= GRAD_CEILING for v in CHAIN_BOUNDS.values())

BLOCK_SEEDS = {1: 91, 2: 92}
# the first input seed from 100 up with a ReLU margin above RELU_MARGIN, per (stride, n, output size), for the block seeds above; asserted
# in the test, from the reference alone.  n = 1 at 5x3 is the odd row count per workgroup: 15 rows in one workgroup of the 512-wide reduce,
# halves of 8 and 7 rows, and a 10x6 input at stride 2
INPUT_SEEDS = {(1, 2, (3, 2)): 100, (1, 2, (1, 1)): 100, (1, 2, (5, 4)): 100, (1, 1, (5, 3)): 100,
               (2, 2, (3, 2)): 100, (2, 2, (1, 1)): 100, (2, 2, (5, 4)): 100, (2, 1, (5, 3)): 101}
CASES = [(2, (3, 2)), (2, (1, 1)), (2, (5, 4)), (1, (5, 3))]


def _seeded_bottleneck128(stride, seed):
    """tests/test_gpu_res4_train.py's `_seeded_bottleneck256` at width 128, on the CPU (the caller moves it)."""
    cin = GEOMS[stride]
    blk = nets.Bottleneck(cin, 128, stride)
    blk.load_state_dict(nets.seeded_state_dict(lambda: nets.Bottleneck(cin, 128, stride), seed))
    with torch.no_grad():      # torchvision's zero_init_residual gives bn3's gamma = 0; a negative gamma flips the sign of the folded weights
        blk.bn3.weight[3] = 0.0
        blk.bn3.weight[7] = -0.75
    return blk


def _inputs(stride, n, h, w, seed):
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn((n, GEOMS[stride], h * stride, w * stride), generator=gen) * 0.5).half().float()
    return x, torch.randn((n, 512, h, w), generator=gen)


def _block_case(blk, ref, x, up):
    """(error of y, errors of the parameter gradients, error of dx, ReLU sign agreement) of one CUDA block against its fp64 reference."""
    stats_before = [b.detach().clone() for b in blk.buffers()]
    xr = x.double().requires_grad_(True)
    yr = _ref_bottleneck(ref, xr)
    yr.backward(up.double())
    xg = x.cuda().requires_grad_(True)
    y = nets.bottleneck128_train(blk.train(), xg)
    assert y.shape == up.shape and y.dtype == torch.float32 and y.requires_grad
    agree = ((y.detach().cpu() > 0) == (yr.detach() > 0)).float().mean()
    y.backward(up.cuda())
    assert all(torch.equal(a, b) for a, b in zip(stats_before, blk.buffers())), "frozen statistics were written"
    names = _names(hasattr(blk, "downsample"))
    got, want = dict(blk.named_parameters()), dict(ref.named_parameters())
    assert sorted(names) == sorted(got)
    for k in names:
        assert got[k].grad is not None and bool(torch.isfinite(got[k].grad).all()), k
    errs = {k: _rel(got[k].grad.double().cpu().numpy(), want[k].grad.numpy()) for k in names}
    assert xg.grad is not None and xg.grad.shape == x.shape
    return (_rel(y.detach().double().cpu().numpy(), yr.detach().numpy()), errs, _rel(xg.grad.double().cpu().numpy(), xr.grad.numpy()), float(agree))


def _judge(tag, label, e_y, errs, e_dx, agree):
    worst = max(errs, key=errs.get)
    print(f"MEASURED {tag} {label}: y {e_y:.3g}, grad {errs[worst]:.3g} ({worst}), dx {e_dx:.3g}, sign agreement {agree:.5f}; {errs}")
    assert agree > 0.99      # the two outputs agree about the ReLU signs
    b = BLOCK_BOUNDS[tag]
    assert e_y <= b["y"] and errs[worst] <= b["grad"] and e_dx <= b["dx"], (e_y, errs, e_dx)


@pytest.mark.gpu
@pytest.mark.parametrize("n,size", CASES)
@pytest.mark.parametrize("stride", [1, 2])
def test_block_against_fp64(hip, stride, n, size):
    blk = _seeded_bottleneck128(stride, BLOCK_SEEDS[stride])
    ref = copy.deepcopy(blk).double()
    seed = INPUT_SEEDS[stride, n, size]
    margins = [_relu_margin(ref, _inputs(stride, n, *size, s)[0].double()) for s in range(100, seed + 1)]
    assert all(m <= RELU_MARGIN for m in margins[:-1]) and margins[-1] > RELU_MARGIN, f"the first conditioned input seed is not {seed}: {margins}"
    x, up = _inputs(stride, n, *size, seed)
    e_y, errs, e_dx, agree = _block_case(blk.cuda(), ref, x, up)
    assert len(errs) == (12 if stride == 2 else 9)
    _judge(f"stride{stride}", f"n={n} {size[0]}x{size[1]}", e_y, errs, e_dx, agree)


# n = 2 at a 24x22 output: C2 48x44 for the stride-2 block (4224 input rows: conv1's weight gradient sums five slabs under res3's slab rule)
# and C3 24x22 for the stride-1 block; 1056 output rows: 33 workgroups of the 512-wide reduce (32 rows each, halves of 16), 5 of the 128-wide
# (17 over the 4224 rows), and two slabs in every weight gradient over the output's rows
ROWS = {1: (1, 2, 24, 22, 97), 2: (2, 2, 24, 22, 98)}


def _rows_case(stride, seed):
    """(the float32 CPU block, its conditioned fp64 reference, x, the upstream gradient) of the many-rows case."""
    blk = _seeded_bottleneck128(stride, seed)
    ref = copy.deepcopy(blk).double()
    x, up = _inputs(*ROWS[stride])
    _condition(ref, x.double())
    margin = _relu_margin(ref, x.double())
    assert margin > CONSTRUCTED_MARGIN, margin
    return _load_from(blk, ref), ref, x, up


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 2])
def test_block_at_many_rows_against_fp64(hip, stride):
    blk, ref, x, up = _rows_case(stride, 93)
    assert x.shape[0] * x.shape[2] * x.shape[3] == (4224 if stride == 2 else 1056) and up.shape[0] * up.shape[2] * up.shape[3] == 1056
    e_y, errs, e_dx, agree = _block_case(blk.cuda(), ref, x, up)
    _judge(f"rows_stride{stride}", "24x22", e_y, errs, e_dx, agree)


def _run_block(blk, x, up):
    blk.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(True)
    y = nets.bottleneck128_train(blk, xg)
    y.backward(up)
    return [y.detach(), xg.grad] + [p.grad.clone() for p in blk.parameters()]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["stride1_5x4", "stride2_5x4", "stride2_rows4224"])
def test_block_bitwise_repeatable_and_scaled(hip, case):
    """Two runs give the same bits, and an upstream gradient 2^-23 times the size gives the same bits, scaled: every scale is a power of two."""
    stride, n, h, w, seed = {"stride1_5x4": (1, 2, 5, 4, 3), "stride2_5x4": (2, 2, 5, 4, 4), "stride2_rows4224": ROWS[2]}[case]
    blk = _seeded_bottleneck128(stride, 94).cuda()
    x, up = (t.cuda() for t in _inputs(stride, n, h, w, seed))
    a, b, c = _run_block(blk, x, up), _run_block(blk, x, up), _run_block(blk, x, up * 2.0 ** -23)
    assert len(a) == (14 if stride == 2 else 11)
    for i, (p, q, r) in enumerate(zip(a, b, c)):
        assert torch.equal(p, q), i
        assert torch.equal(r, p if i == 0 else p * 2.0 ** -23), f"tensor {i}: a power-of-two smaller upstream gradient must give the same bits, scaled"


# ---- res3 -> res4 -> res5 -> FPN -> head -> HIP loss on a padded C2 tap
def _seeded_res3(seed):
    return torch.nn.Sequential(_seeded_bottleneck128(2, seed), *(_seeded_bottleneck128(1, seed + i) for i in range(1, 4)))


def _chain_setup(conditioned=False):
    """res4's chain setup (n = 2, C2 24x16, C3 12x8, C5 3x2) one stage further down.  With `conditioned` the thirteen blocks are bias-shifted
    on the fp64 reference from the lowest block up and the shifted state is loaded into the GPU modules; the references come back too."""
    n, h5, w5 = 2, 3, 2
    gen = torch.Generator().manual_seed(r5t.CHAIN_SEED)
    res3, res4, res5, fpn, head = _seeded_res3(101), _seeded_res4(81), r5t._seeded_res5(61), l4t._seeded_fpn(2048, 6), neck._seeded_head(8).train()
    feats = l4t._taps(n, 2048, h5, w5, gen)[:1]
    targets = neck._random_targets((n, 1, 32 * h5, 32 * w5), gen)
    refs = None
    if conditioned:
        refs = [copy.deepcopy(b).to(device="cpu", dtype=torch.float64) for b in list(res3) + list(res4) + list(res5)]
        x = feats[0].double()
        for ref, blk in zip(refs, list(res3) + list(res4) + list(res5)):
            xin, x = x, _condition(ref, x)
            assert _relu_margin(ref, xin) > CONSTRUCTED_MARGIN
            _load_from(blk, ref)
    padded = [nets.pack_tap(t.cuda()) for t in feats]
    return res3.cuda(), res4.cuda(), res5, fpn, head, feats, targets, padded, refs


def _node_grads(*mods):
    """The gradients of (res3,) res4, res5 (all parameters), the FPN (its live ones) and the head, one list per module."""
    *stages, fpn, head = mods
    return [[p.grad.clone() for p in m.parameters()] for m in stages] + [[p.grad.clone() for p in fpn.live_parameters()],
                                                                         [p.grad.clone() for p in head.parameters()]]


@pytest.mark.gpu
def test_ladder_res3_node_gives_the_bits_of_the_res4_node(hip):
    """The node one stage deeper gives the bits of the res4 node fed the C3 that forward_res3_padded gives: two maps and 117 gradients."""
    res3, res4, res5, fpn, head, feats, targets, padded, _ = _chain_setup()
    state = copy.deepcopy(head.state_dict())
    out, _ = r5t._loss_backward(fpn.forward_padded(padded, head=head, res5=res5, res4=res4, res3=res3), targets)
    g3, g4, g5, gf, gh = _node_grads(res3, res4, res5, fpn, head)
    assert len(g3) == 39 and len(g4) == 57 and len(g5) == 30 and len(gf) == 10 and len(gh) == 20
    c3p = nets.forward_res3_padded(res3, padded[0])
    assert c3p.shape == (2, 14, 10, 512) and c3p.dtype == torch.float16
    assert float(c3p[:, 0].abs().max()) == 0 and float(c3p[:, :, 0].abs().max()) == 0 and float(c3p[:, -1].abs().max()) == 0 and \
        float(c3p[:, :, -1].abs().max()) == 0 and float(c3p[:, 1:-1, 1:-1].abs().max()) > 0
    head.load_state_dict(state)
    for m in (res4, res5, fpn, head):
        m.zero_grad(set_to_none=True)
    out2, _ = r5t._loss_backward(fpn.forward_padded(padded + [c3p], head=head, res5=res5, res4=res4), targets)
    same = [(out["probability"], out2["probability"]), (out["threshold"], out2["threshold"])] + \
        list(zip(g4 + g5 + gf + gh, [g for gs in _node_grads(res4, res5, fpn, head) for g in gs]))
    assert len(same) == 119
    for i, (a, b) in enumerate(same):
        assert torch.equal(a, b), i


@pytest.mark.gpu
def test_chain_res3_res4_res5_fpn_head_loss_against_fp64(hip):
    """Stage-isolated at C5 and P2, as the res4 chain test: the reference head reads the P2 the kernels stored, the
    reference FPN the C3, C4 and C5 they stored; the gradient chain is end to end: the reference res5's upstream gradient is the reference
    FPN's dC5, the reference res4's the reference res5's dx plus the reference FPN's dC4, the reference res3's the reference res4's dx plus
    the reference FPN's dC3.  Then the chain twice: the same bits."""
    res3, res4, res5, fpn, head, feats, targets, padded, refs = _chain_setup(conditioned=True)
    rfpn, rhead = l4t._rounded_fpn(fpn), neck._rounded_head(head).train()
    state = copy.deepcopy(head.state_dict())
    stages = (res3, res4, res5)
    stats_before = [b.detach().clone() for m in stages for b in m.buffers()]
    out, ups = r5t._loss_backward(fpn.forward_padded(padded, head=head, res5=res5, res4=res4, res3=res3), targets)
    assert all(torch.equal(a, b) for a, b in zip(stats_before, [b for m in stages for b in m.buffers()])), "frozen statistics were written"
    g3, g4, g5, gf, gh = _node_grads(res3, res4, res5, fpn, head)
    assert len(g3) == 39 and len(g4) == 57 and len(g5) == 30 and len(gf) == 10 and len(gh) == 20
    first = [out["probability"].detach(), out["threshold"].detach()] + g3 + g4 + g5 + gf + gh
    c3p = nets.forward_res3_padded(res3, padded[0])
    c4p = nets.forward_res4_padded(res4, c3p)
    c5p = nets.forward_res5_padded(res5, c4p)
    p2p = fpn.forward_padded(padded + [c3p, c4p, c5p])
    # reference, back to front
    unpad = lambda t: t[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).double().cpu().contiguous().requires_grad_(True)  # noqa: E731
    x = unpad(p2p)
    torch.autograd.backward([rhead.probability_head(x), rhead.threshold_head(x)], [u.double().cpu() for u in ups])
    c3, c4, c5 = unpad(c3p), unpad(c4p), unpad(c5p)
    l4t._wiring(rfpn, [feats[0].double(), c3, c4, c5]).backward(x.grad)
    mid, mids = feats[0].double(), []
    for i, ref in enumerate(refs):
        assert _relu_margin(ref, mid.detach()) > CONSTRUCTED_MARGIN, f"block {i} is not conditioned"
        mid = _ref_bottleneck(ref, mid)
        if i < 12:
            mid = _f16(mid)
        mids.append(mid)
    e_c3 = _rel(c3.detach().numpy(), mids[3].detach().numpy())
    e_c4 = _rel(c4.detach().numpy(), mids[9].detach().numpy())
    e_c5 = _rel(c5.detach().numpy(), _f16(mids[12]).detach().numpy())
    # dC4 = the reference res5's dx + the reference FPN's dC4; dC3 = the reference res4's dx + the reference FPN's dC3
    torch.autograd.backward([mids[12], mids[9], mids[3]], [c5.grad, c4.grad, c3.grad])
    rres3, rres4, rres5 = torch.nn.Sequential(*refs[:4]), torch.nn.Sequential(*refs[4:10]), torch.nn.Sequential(*refs[10:])
    errs = lambda mod, rmod, names: {k: _rel(dict(mod.named_parameters())[k].grad.double().cpu().numpy(),  # noqa: E731
                                             dict(rmod.named_parameters())[k].grad.numpy()) for k in names}
    e3, e4, e5 = errs(res3, rres3, RES3_NAMES), errs(res4, rres4, RES4_NAMES), errs(res5, rres5, r5t.RES5_NAMES)
    fe, he = neck._fpn_errors(fpn, rfpn), neck._head_errors(head, rhead)
    assert len(e3) == 39 and len(e4) == 57 and len(e5) == 30 and len(fe) == 10 and len(he) == 20
    w3, w4, w5, wf, wh = (max(e, key=e.get) for e in (e3, e4, e5, fe, he))
    print(f"MEASURED chain: C3 {e_c3:.3g}, C4 {e_c4:.3g}, C5 {e_c5:.3g}, res3 grad {e3[w3]:.3g} ({w3}), res4 grad {e4[w4]:.3g} ({w4}), "
          f"res5 grad {e5[w5]:.3g} ({w5}), fpn grad {fe[wf]:.3g} ({wf}), head grad {he[wh]:.3g} ({wh}); {e3} {e4} {e5}")
    # bitwise repeatable: two maps, 39 + 57 + 30 + 10 + 20 gradients
    head.load_state_dict(state)
    for m in (res3, res4, res5, fpn, head):
        m.zero_grad(set_to_none=True)
    out2, _ = r5t._loss_backward(fpn.forward_padded(padded, head=head, res5=res5, res4=res4, res3=res3), targets)
    second = [out2["probability"].detach(), out2["threshold"].detach()] + [g for gs in _node_grads(res3, res4, res5, fpn, head) for g in gs]
    assert len(first) == len(second) == 158
    for i, (a, b) in enumerate(zip(first, second)):
        assert torch.equal(a, b), i
    assert e3[w3] <= CHAIN_BOUNDS["res3"], e3
    assert e4[w4] <= CHAIN_BOUNDS["res4"], e4
    assert e5[w5] <= CHAIN_BOUNDS["res5"], e5
    assert fe[wf] <= CHAIN_BOUNDS["fpn"], fe
    assert he[wh] <= CHAIN_BOUNDS["head"], he


# ---- the engine's stop at C2
@pytest.mark.gpu
@pytest.mark.parametrize("backbone", ["resnet50", "resnet18"])
def test_forward_c2_gives_forward_trunks_bits(hip, backbone):
    from vtd_amd.engine import DetectorEngine
    sd = nets.seeded_state_dict(lambda: nets.DBNet(backbone), seed=5)
    eng = DetectorEngine(backbone, sd, max_batch=1, options={"fuse_fpn_head": 0})
    x = torch.randn((1, 3, 640, 640), generator=torch.Generator().manual_seed(0))
    want = eng.forward_trunk(x)[0]
    got = eng.forward_c2(x)
    assert got.shape == want.shape == (1, 162, 162, 256 if backbone == "resnet50" else 64) and got.dtype == torch.float16
    assert got.data_ptr() != want.data_ptr() and torch.equal(got, want) and float(got.abs().max()) > 0
    assert torch.equal(eng.forward_c2(x), want)      # after a whole-trunk call and after its own
    eng.close()


@pytest.mark.gpu
def test_product_head_fpn_res5_res4_res3_training_step(hip):
    from vtd_amd._fixtures.weights import stress_detector_state_dict
    torch.manual_seed(3)
    net = nets.DBNet("resnet50", compute_threshold=True, trainable="head+fpn+res5+res4+res3")
    net.load_state_dict(stress_detector_state_dict("resnet50", 17))
    net.cuda().train()
    gen = torch.Generator().manual_seed(23)
    x = torch.randn((1, 3, 640, 640), generator=gen).cuda()
    targets = neck._random_targets((1, 1, 640, 640), gen)
    te = net.trunk_engine()
    trained = ("backbone.5.", "backbone.6.", "backbone.7.")
    stats = {k: v.detach().clone() for k, v in net.state_dict().items() if k.startswith(trained) and ("running" in k or "num_batches" in k)}
    assert len(stats) == 39 + 57 + 30
    mod = training.TextDetectionLightningModule(net)
    opt = mod.configure_optimizers()["optimizer"]
    loss = mod.training_step((x, targets), 0)
    opt.zero_grad()
    loss.backward()
    trunk = {k: p for k, p in net.named_parameters() if k.startswith(trained)}
    assert len(trunk) == 126
    for k, p in trunk.items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k
    for i in range(5):
        assert all(p.grad is None for p in net.backbone[i].parameters())
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    opt.step()
    after = net.state_dict()
    for k in trunk:
        assert not torch.equal(before[k], after[k]), f"{k} did not change"
    for k in before:
        if k.startswith("backbone.") and not k.startswith(trained):
            assert torch.equal(before[k], after[k]), f"{k} changed"
    assert net.trunk_engine() is te, "an optimizer step on res3 / res4 / res5 / FPN / head weights rebuilt the trunk engine"
    for k, v in stats.items():
        assert torch.equal(v, net.state_dict()[k]), f"{k} was written"
    # a second step runs on the stepped weights (folded on the device in every call), on the same engine
    loss2 = mod.training_step((x, targets), 1)
    assert bool(torch.isfinite(loss2)) and float(loss2) != float(loss)
    # a following eval() forward runs the fused inference engine on the stepped weights
    net.eval()
    with torch.no_grad():
        got = net(x)
    fresh = nets.DBNet("resnet50", compute_threshold=True)
    fresh.load_state_dict(net.state_dict())
    with torch.no_grad():
        want = fresh.cuda().eval()(x)
    assert torch.equal(got["probability"], want["probability"]) and torch.equal(got["threshold"], want["threshold"])
