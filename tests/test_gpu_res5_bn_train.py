"""Train-mode (batch-statistics) BatchNorm for ResNet-50's res5 and res4 on the GPU (csrc/bottleneck_bn_train.hip, the
vtd_bottleneck_bn_train_* entries): the four Bottleneck geometries through `nets.bottleneck_bn_train(block, x)`, the res4 -> res5 -> FPN ->
head node with `res_batch_stats=True`, and `DBNet("resnet50", trainable="head+fpn+res5+res4", trunk_bn="bottleneck")`.

The fp64 reference is CPU autograd in float64, the convention of tests/test_gpu_layer4_bn_train.py: the block written with
F.batch_norm(..., training=True), fed x rounded to fp16 and the raw convolution weights rounded to fp16 straight through (the kernels pack
them unfolded); a1, a2 and the downsample's normalised output are rounded to fp16 straight through, where the kernels store them.  Metric:
relative L2 error per tensor.  Bounds: 3x the level measured on an MI355X, worst over the sizes, under the ceilings of 2e-3 for maps,
statistics and running buffers and 1e-2 for gradients."""
import copy

import pytest
import torch
import torch.nn.functional as F

import test_gpu_fpn_neck_train as neck
import test_gpu_layer4_train as l4t
import test_gpu_res4_train as r4t
import test_gpu_res5_train as r5t
from test_gpu_layer4_train import _rel, _ste
from test_gpu_res5_train import GRAD_CEILING, MAP_CEILING, _f16, _names
from vtd_amd import nets, training

# (width, stride) -> cin: res5's and res4's two geometries each
GEOMS = {(512, 2): 1024, (512, 1): 2048, (256, 2): 512, (256, 1): 1024}
# 3 x 2: M = 12 rows, parts of the W-wide reduces without rows and one workgroup everywhere.  12 x 11: M = 264, nine 4W-wide reduce workgroups
# (30 rows each, 24 in the last), two W-wide ones, five for bn1's 1056 input rows at stride 2, and a last weight-gradient K chunk of 8 rows
SIZES = [(3, 2), (5, 4), (12, 11)]

# Conditioning.  One flipped element of the mask y > 0 moves g3 = dy (y > 0), the upstream gradient of every parameter at once, by about
# sqrt(2 / (n h w 4W)) in relative L2: 9e-3 at W = 512 and 3 x 2, 5e-3 at 5 x 4 (7e-3 at W = 256) -- the gradient ceiling itself, from one or
# two elements; a flipped a1 or a2 element is worth as much to the gradients below it.  Under batch statistics the ReLU arguments are
# normalised, so with the seeded biases about 0.4 / sigma of them lie within a unit of zero, and a first run on seeded blocks had 2 and 4
# flips among the 81920 outputs of the two W = 512 cases at 5 x 4 (6.5e-3 and 1.6e-2 on the worst gradient) with every tensor of the flip-free
# 3 x 2 cases at 3.7e-4.  A flip is no error of the kernels: the argument's sign is decided below the fp16 operands' resolution.  So every
# case is conditioned on the CPU, from the reference alone, in the two ways of the frozen tests:
#   * by construction (tests/test_gpu_res4_train.py's `_condition`, milder): each BatchNorm bias is set per channel so that the ReLU
#     argument's batch mean sits S standard deviations from zero, the sign alternating by channel.  S = 2 thins the arguments near zero out
#     7.4-fold (the normal density at 2, 0.054, against 0.4) and keeps the masks data-dependent: 2.3 % of a channel's arguments lie on the
#     other side; S = 3 thins them out 90-fold (0.0044) with 0.13 % on the other side.  S is the smaller of the two at which the expected
#     number of arguments within RELU_MARGIN of zero, N 2 phi(S) RELU_MARGIN over the case's N arguments of the three ReLUs, is at most 1
#     (`_sigmas`): 2 up to 5 x 4, 3 at 12 x 11.  Not more than needed: a train-mode BatchNorm removes a constant added to its input channel,
#     so where the ReLU in front of it is the identity for a whole channel the gradient of that channel's bias upstream is zero, and the more
#     a case is shifted the more bn1.bias' and bn2.bias' gradients are sums that cancel: they are the worst tensors of every case, 1e-3 at
#     S = 2 and 4e-3 at S = 3 with every other tensor at 3e-4 (and at S = 3 and 3 x 2, twelve rows, their reference value is exactly zero);
#   * by seed: the input seed is the first from 100 up at which no argument of the three ReLUs of the conditioned reference is within
#     RELU_MARGIN of zero.  tests/test_gpu_res5_train.py's margin (5e-6) covers the fp32 accumulation alone and says that the one-ulp
#     differences of the stored fp16 activations come on top; one ulp of an activation below 1 is 2^-11 = 4.9e-4, times 0.1, the upper
#     range of the seeded weights at K = 512 (standard deviation 0.06), is 5e-5 for one differing input: the margin here.
# Both thin the flips out, neither can exclude them; the flips of y that remain are printed with the levels.
RELU_MARGIN = 5e-5
PHI = {2.0: 0.05399, 3.0: 0.004432}      # the standard normal density at S


def _sigmas(width, stride, size, n=2):
    """The shift of a block case: the smaller S of (2, 3) with at most one argument expected within RELU_MARGIN of zero."""
    m = n * size[0] * size[1]
    args = m * stride * stride * width + m * width + m * 4 * width      # a1 at the input's extent, a2, y
    return next((s for s in (2.0, 3.0) if args * 2 * PHI[s] * RELU_MARGIN <= 1.0), 3.0)


# (width, stride, size) -> the first input seed from 100 up whose conditioned reference has a ReLU margin above RELU_MARGIN (block seeds
# 30 + stride); the margin of the seed is asserted in the test
INPUT_SEEDS = {(512, 2, (3, 2)): 100, (512, 2, (5, 4)): 101, (512, 2, (12, 11)): 101, (512, 1, (3, 2)): 100, (512, 1, (5, 4)): 106,
               (512, 1, (12, 11)): 100, (256, 2, (3, 2)): 100, (256, 2, (5, 4)): 100, (256, 2, (12, 11)): 101, (256, 1, (3, 2)): 100,
               (256, 1, (5, 4)): 100, (256, 1, (12, 11)): 100}

BLOCK_BOUNDS = {
    # 3x the level measured on an MI355X, worst of the three sizes (grad: worst of the nine / twelve parameter gradients), never above the
    # ceiling.  No output of the twelve cases flipped its ReLU sign.  The worst gradient is bn2.bias everywhere, the cancelling sum the
    # conditioning note explains: 1.0e-3 .. 1.3e-3 at 3 x 2 and 5 x 4 (S = 2) and 3.3e-3 .. 3.9e-3 at 12 x 11 (S = 3), above a third of the
    # ceiling from the cancellation, not from a flip; every other gradient of every case is between 6e-8 and 1.1e-3.  3x the 12 x 11 level
    # is over the ceiling for three of the four blocks: their bound is the ceiling.
    (512, 2): {"y": 6.4e-4, "grad": GRAD_CEILING, "dx": 8.6e-4, "stats": 1.9e-4, "running": 4.7e-5},      # measured 2.14e-4, 3.86e-3, 2.85e-4, 6.45e-5, 1.56e-5
    (512, 1): {"y": 6.4e-4, "grad": 9.9e-3, "dx": 9.2e-4, "stats": 1.6e-4, "running": 3.7e-5},            # 2.14e-4, 3.31e-3, 3.07e-4, 5.23e-5, 1.23e-5
    (256, 2): {"y": 6.4e-4, "grad": GRAD_CEILING, "dx": 8.6e-4, "stats": 1.2e-4, "running": 2.8e-5},      # 2.13e-4, 3.80e-3, 2.88e-4, 3.94e-5, 9.33e-6
    (256, 1): {"y": 6.4e-4, "grad": GRAD_CEILING, "dx": 9.5e-4, "stats": 1.9e-4, "running": 5.0e-5},      # 2.13e-4, 3.39e-3, 3.17e-4, 6.24e-5, 1.67e-5
}
assert all(b[k] <= (MAP_CEILING if k in ("y", "stats", "running") else GRAD_CEILING) for b in BLOCK_BOUNDS.values() for k in b)


ZERO_GAMMA = 4      # bn3's channel with gamma = 0: an even one, which `_condition` leaves mostly active, so that its dgamma is not masked away


def _seeded(width, stride, seed):
    """tests/test_gpu_res5_train.py's `_seeded_bottleneck` at either width, on the CPU (the caller moves it): bn3's gamma is 0 in channel
    ZERO_GAMMA and negative in channel 7."""
    cin = GEOMS[width, stride]
    blk = nets.Bottleneck(cin, width, stride)
    blk.load_state_dict(nets.seeded_state_dict(lambda: nets.Bottleneck(cin, width, stride), seed))
    with torch.no_grad():
        blk.bn3.weight[ZERO_GAMMA] = 0.0
        blk.bn3.weight[7] = -0.75
    return blk


def _inputs(width, stride, h, w, seed, n=2):
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn((n, GEOMS[width, stride], h * stride, w * stride), generator=gen) * 0.5).half().float()
    return x, torch.randn((n, 4 * width, h, w), generator=gen)


def _ref_pair(x, conv, bn, stride, pad, seen):
    z = F.conv2d(x, _ste(conv.weight), None, stride, pad)
    seen.append((z.detach().mean((0, 2, 3)), z.detach().var((0, 2, 3), unbiased=False)))
    return F.batch_norm(z, bn.running_mean, bn.running_var, bn.weight, bn.bias, True, bn.momentum, bn.eps)      # updates the buffers


def _ref_bottleneck(ref, x, seen=None):
    """The block in float64 with train-mode BatchNorm; `seen` collects (mu, sigma^2) of bn1, bn2, bn3 and the downsample's BatchNorm, the
    order of the kernels' statistics rows."""
    s1, s2, s3, sd = [], [], [], []
    a1 = _f16(F.relu(_ref_pair(x, ref.conv1, ref.bn1, 1, 0, s1)))
    a2 = _f16(F.relu(_ref_pair(a1, ref.conv2, ref.bn2, ref.stride, 1, s2)))
    idt = x
    if hasattr(ref, "downsample"):
        idt = _f16(_ref_pair(x, ref.downsample[0], ref.downsample[1], ref.stride, 0, sd))
    y = F.relu(_ref_pair(a2, ref.conv3, ref.bn3, 1, 0, s3) + idt)
    if seen is not None:
        seen += s1 + s2 + s3 + sd
    return y


def _bn_free(z, bn):
    """Train-mode BatchNorm of z in float64 that touches no buffer."""
    return F.batch_norm(z, None, None, bn.weight, bn.bias, True, 0.0, bn.eps)


def _relu_args(ref, x):
    """The arguments of the block's three ReLUs in the fp64 train-mode reference, no buffer touched."""
    with torch.no_grad():
        z1 = _bn_free(F.conv2d(x, ref.conv1.weight.half().double()), ref.bn1)
        z2 = _bn_free(F.conv2d(_f16(F.relu(z1)), ref.conv2.weight.half().double(), None, ref.stride, 1), ref.bn2)
        idt = x
        if hasattr(ref, "downsample"):
            idt = _f16(_bn_free(F.conv2d(x, ref.downsample[0].weight.half().double(), None, ref.stride), ref.downsample[1]))
        z3 = _bn_free(F.conv2d(_f16(F.relu(z2)), ref.conv3.weight.half().double()), ref.bn3) + idt
        return z1, z2, z3


def _condition(ref, x, sigmas=2.0):
    """Condition the float64 reference block on the input x by construction, from the reference alone (tests/test_gpu_res4_train.py's
    `_condition` under batch statistics): stage by stage (bn1, then bn2 given the new a1, then bn3 given the new a2) each BatchNorm bias is
    set per channel so that the ReLU argument's batch mean sits `sigmas` of that channel's standard deviation from zero, the sign alternating
    by channel.  The masks stay data-dependent (2.3 % of a channel's arguments lie on the other side of zero at 2 sigma); what goes is the
    bulk of the arguments near zero.  The new biases are fp32 values: the GPU block holds the same numbers."""
    for i, bn in enumerate((ref.bn1, ref.bn2, ref.bn3)):
        z = _relu_args(ref, x)[i]
        with torch.no_grad():
            mean, std = z.mean((0, 2, 3)), z.std((0, 2, 3), unbiased=False)
            sign = torch.ones_like(mean)
            sign[1::2] = -1.0
            bn.bias.copy_((bn.bias + sign * sigmas * std.clamp_min(1e-3) - mean).float().double())
    return min(float(z[z != 0].abs().min()) for z in _relu_args(ref, x))


def _bns(blk):
    return [blk.bn1, blk.bn2, blk.bn3] + ([blk.downsample[1]] if hasattr(blk, "downsample") else [])


def _block_case(blk, width, stride, size):
    h, w = size
    x, up = _inputs(width, stride, h, w, INPUT_SEEDS[width, stride, size])
    ref = copy.deepcopy(blk).to(device="cpu", dtype=torch.float64)
    margin = _condition(ref, x.double(), _sigmas(width, stride, size))
    assert margin > RELU_MARGIN, f"the case is not conditioned (margin {margin:.3g}): take the next input seed (see RELU_MARGIN)"
    blk.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    blk.cuda().train()
    xr = x.double().requires_grad_(True)
    seen = []
    yr = _ref_bottleneck(ref, xr, seen)
    # the statistics the forward reports, on a copy of the block (the call moves the running statistics)
    probe = copy.deepcopy(blk)
    geom, eps, learn, stats = nets._bottleneck_operands(probe, torch.device("cuda", torch.cuda.current_device()), nets._BOTTLENECK_BN_GEOMETRIES,
                                                        nets._BOTTLENECK_BN_BUILT)
    with torch.no_grad():
        _, _, bstats = nets._block_forward_raw(nets.pack_tap(x.cuda()), (2, h * stride, w * stride, *geom), eps, learn, stats, nets._BOTTLENECK_BN,
                                               bn=(True, probe.bn1.momentum))
    assert bstats.shape == (4, 2, 4 * width)
    cols = [width, width, 4 * width, 4 * width]
    e_stats = max(_rel(bstats[i, j, :cols[i]].double().cpu().numpy(), seen[i][j].numpy()) for i in range(len(seen)) for j in range(2))
    # what the call does not write is left untouched: the W-wide rows' other columns, the fourth row without a downsample
    assert bool(torch.isnan(bstats[:2, :, width:]).all()), "a W-wide statistics row was written past its first W columns"
    if len(seen) == 3:
        assert bool(torch.isnan(bstats[3]).all()), "the fourth statistics row was written without a downsample"
    xg = x.cuda().requires_grad_(True)
    y = nets.bottleneck_bn_train(blk, xg)
    assert y.shape == up.shape and y.dtype == torch.float32
    agree = ((y.detach().cpu() > 0) == (yr.detach() > 0)).float()
    flips = int((1 - agree).sum())
    yr.backward(up.double())
    y.backward(up.cuda())
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(xg.grad).all())
    e_run = 0.0
    for a, b, p in zip(_bns(blk), _bns(ref), _bns(probe)):
        assert int(a.num_batches_tracked) == 1
        assert torch.equal(a.running_mean, p.running_mean) and torch.equal(a.running_var, p.running_var)
        e_run = max(e_run, _rel(a.running_mean.double().cpu().numpy(), b.running_mean.numpy()), _rel(a.running_var.double().cpu().numpy(), b.running_var.numpy()))
    names = _names(hasattr(blk, "downsample"))
    got, want = dict(blk.named_parameters()), dict(ref.named_parameters())
    assert sorted(names) == sorted(got)
    errs = {k: _rel(got[k].grad.double().cpu().numpy(), want[k].grad.numpy()) for k in names}
    for k in names:
        assert bool(torch.isfinite(got[k].grad).all()), k
    # gamma = 0 (bn3 channel ZERO_GAMMA): conv3's weight gradient of that channel vanishes exactly, dgamma does not
    assert float(got["conv3.weight"].grad[ZERO_GAMMA].abs().max()) == 0.0 and float(got["bn3.weight"].grad[ZERO_GAMMA].abs()) > 0
    e_y = _rel(y.detach().double().cpu().numpy(), yr.detach().numpy())
    e_dx = _rel(xg.grad.double().cpu().numpy(), xr.grad.numpy())
    return e_y, errs, e_dx, float(agree.mean()), flips, e_stats, e_run


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("width,stride", list(GEOMS))
def test_block_against_fp64(hip, width, stride, size):
    blk = _seeded(width, stride, 30 + stride)
    e_y, errs, e_dx, agree, flips, e_stats, e_run = _block_case(blk, width, stride, size)
    worst = max(errs, key=errs.get)
    print(f"MEASURED bn bottleneck W{width} stride{stride} {size[0]}x{size[1]}: y {e_y:.3g}, grad {errs[worst]:.3g} ({worst}), dx {e_dx:.3g}, "
          f"stats {e_stats:.3g}, running {e_run:.3g}, sign agreement {agree:.5f} ({flips} flips of y); {errs}")
    assert agree > 0.99 and len(errs) == (12 if stride == 2 else 9)
    b = BLOCK_BOUNDS[width, stride]
    assert e_y <= b["y"] and errs[worst] <= b["grad"] and e_dx <= b["dx"] and e_stats <= b["stats"] and e_run <= b["running"], (e_y, errs, e_dx, e_stats,
                                                                                                                             e_run)


def _run(blk, x, up, fn):
    blk.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(True)
    y = fn(blk, xg)
    y.backward(up)
    return [y.detach(), xg.grad] + [p.grad.clone() for p in blk.parameters()]


@pytest.mark.gpu
@pytest.mark.parametrize("width,stride", list(GEOMS))
def test_eval_mode_is_the_frozen_path(hip, width, stride):
    blk = _seeded(width, stride, 24).cuda().eval()
    x, up = (t.cuda() for t in _inputs(width, stride, 5, 4, 2))
    buffers = [b.detach().clone() for b in blk.buffers()]
    want = _run(blk, x, up, nets.bottleneck_train if width == 512 else nets.bottleneck256_train)
    got = _run(blk, x, up, nets.bottleneck_bn_train)
    assert len(got) == len(want) == (14 if stride == 2 else 11)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), i
    assert all(torch.equal(a, b) for a, b in zip(buffers, blk.buffers())), "eval() wrote the buffers"


@pytest.mark.gpu
@pytest.mark.parametrize("width,stride", list(GEOMS))
def test_bitwise_repeatable_and_scaled(hip, width, stride):
    blk = _seeded(width, stride, 23).cuda().train()
    x, up = (t.cuda() for t in _inputs(width, stride, 12, 11, 1))
    state = copy.deepcopy(blk.state_dict())
    runs, buffers = [], []
    for scale in (1.0, 1.0, 2.0 ** 8, 2.0 ** -8):
        blk.load_state_dict(state)
        runs.append(_run(blk, x, up * scale, nets.bottleneck_bn_train))
        buffers.append([b.detach().clone() for b in blk.buffers()])
    for i, (a, b) in enumerate(zip(runs[0], runs[1])):
        assert torch.equal(a, b), i
    for a, b in zip(buffers[0], buffers[1]):
        assert torch.equal(a, b)
    for run, scale in ((runs[2], 2.0 ** 8), (runs[3], 2.0 ** -8)):
        assert torch.equal(run[0], runs[0][0])
        for i, (a, c) in enumerate(zip(runs[0][1:], run[1:])):
            assert torch.equal(c, a * scale), f"tensor {i}: an upstream gradient times a power of two must give the same bits, scaled"


# ---- res4 -> res5 -> FPN -> head -> HIP loss on padded taps, batch statistics in all nine blocks
# worst gradient per stage at C5 = 3 x 2, n = 2, nine blocks conditioned at S = 2: 3x the level measured on an MI355X: 1.41e-3 (res4,
# 2.bn2.bias; the other res4 gradients 4.5e-4 .. 8.2e-4), 1.42e-3 (res5, 1.bn2.bias), 6.23e-4 (FPN, layer_blocks.3.weight), 3.60e-4 (head,
# probability_head.0.weight), 2.14e-5 (the 58 running buffers); the smallest ReLU argument on the stored taps was 4.8e-5
CHAIN_BOUNDS = {"res4": 4.3e-3, "res5": 4.3e-3, "fpn": 1.9e-3, "head": 1.1e-3, "running": 6.5e-5}
assert all(v <= (MAP_CEILING if k == "running" else GRAD_CEILING) for k, v in CHAIN_BOUNDS.items())
CHAIN_SEED = 171      # the first from tests/test_gpu_res5_train.py's 163 up at which every block of the chain, conditioned at S = 2, has a margin above RELU_MARGIN (asserted)


def _out_free(ref, x):
    """The reference block's output rounded to fp16 as the kernels store it, no buffer touched: the next block's input."""
    return _f16(F.relu(_relu_args(ref, x)[2])).detach()


def _chain_setup():
    """tests/test_gpu_res4_train.py's chain (n = 2, C2 24x16, C3 12x8, C5 3x2) with the nine blocks conditioned under batch statistics from the
    lowest block up on the fp64 references, whose state is loaded into the GPU modules."""
    n, h5, w5 = 2, 3, 2
    gen = torch.Generator().manual_seed(CHAIN_SEED)
    res4 = torch.nn.Sequential(_seeded(256, 2, 81), *(_seeded(256, 1, 81 + i) for i in range(1, 6)))
    res5 = torch.nn.Sequential(_seeded(512, 2, 61), _seeded(512, 1, 62), _seeded(512, 1, 63))
    fpn, head = l4t._seeded_fpn(2048, 6), neck._seeded_head(8).train()
    feats = l4t._taps(n, 2048, h5, w5, gen)[:2]
    targets = neck._random_targets((n, 1, 32 * h5, 32 * w5), gen)
    refs = [copy.deepcopy(b).to(device="cpu", dtype=torch.float64) for b in list(res4) + list(res5)]
    x, margins = feats[1].double(), []
    for ref, blk in zip(refs, list(res4) + list(res5)):
        margins.append(_condition(ref, x))
        x = _out_free(ref, x)
        blk.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    assert min(margins) > RELU_MARGIN, f"the chain is not conditioned: {margins}"
    padded = [nets.pack_tap(t.cuda()) for t in feats]
    return res4.cuda().train(), res5.cuda().train(), fpn, head, feats, targets, padded, refs


def _stage_taps(layers, tap):
    """The padded taps the blocks of the stages write under batch statistics, one per block, on deep copies from the same starting buffers:
    C4 is the sixth and C5 the ninth of (res4, res5) on C3."""
    outs, x = [], tap
    with torch.no_grad():
        for layer in layers:
            for blk in copy.deepcopy(layer):
                geom, eps, learn, stats = nets._bottleneck_operands(blk, tap.device, nets._BOTTLENECK_BN_GEOMETRIES, nets._BOTTLENECK_BN_BUILT)
                g = (x.shape[0], x.shape[1] - 2, x.shape[2] - 2, *geom)
                x = nets._block_forward_raw(x, g, eps, learn, stats, nets._BOTTLENECK_BN, bn=(True, blk.bn1.momentum))[0]
                outs.append(x)
    return outs


@pytest.mark.gpu
def test_chain_res4_res5_fpn_head_loss_against_fp64(hip):
    """Isolated at every stored tap (DESIGN.md section 4's stage isolation, one block at a time): the reference head reads the P2 the
    kernels stored, the reference FPN the C4 and C5 they stored, and each reference block the input tap the kernels stored.  Under batch
    statistics at 12 to 48 rows per channel the one-ulp differences of a stored fp16 tap move the next block's statistics, so arguments
    drift by 1e-3 over nine blocks (C5 is at 9e-4 end to end) and no margin a chain of this size can be conditioned to keeps its masks:
    a run with the reference chained forward had res5's last block at 4e-3 and everything below at 4e-2.  The gradient chain is end to end
    through the nine train-mode reference blocks: block i's upstream gradient is the reference block i + 1's input gradient (res5.0's plus
    the reference FPN's dC4)."""
    res4, res5, fpn, head, feats, targets, padded, refs = _chain_setup()
    rfpn, rhead = l4t._rounded_fpn(fpn), neck._rounded_head(head).train()
    outs = _stage_taps((res4, res5), padded[1])
    c4p, c5p = outs[5], outs[8]
    out, ups = r5t._loss_backward(fpn.forward_padded(padded, head=head, res5=res5, res4=res4, res_batch_stats=True), targets)
    p2p = fpn.forward_padded(padded + [c4p, c5p])
    unpad = lambda t: t[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).double().cpu().contiguous().requires_grad_(True)  # noqa: E731
    x = unpad(p2p)
    torch.autograd.backward([rhead.probability_head(x), rhead.threshold_head(x)], [u.double().cpu() for u in ups])
    c4, c5 = unpad(c4p), unpad(c5p)
    l4t._wiring(rfpn, [t.double() for t in feats] + [c4, c5]).backward(x.grad)
    ins = [feats[1].double()] + [unpad(o) for o in outs[:8]]
    margin = min(float(z[z != 0].abs().min()) for ref, xin in zip(refs, ins) for z in _relu_args(ref, xin.detach()))
    ys = [_ref_bottleneck(ref, xin) for ref, xin in zip(refs, ins)]      # moves the reference's running buffers, once
    e_c4 = _rel(c4.detach().numpy(), _f16(ys[5]).detach().numpy())
    e_c5 = _rel(c5.detach().numpy(), _f16(ys[8]).detach().numpy())
    up = c5.grad
    for i in reversed(range(9)):
        ys[i].backward(up)
        if i:
            up = ins[i].grad + (c4.grad if i == 6 else 0)      # dC4 = the reference res5's dx + the reference FPN's dC4
    rres4, rres5 = torch.nn.Sequential(*refs[:6]), torch.nn.Sequential(*refs[6:])
    e4 = {k: _rel(dict(res4.named_parameters())[k].grad.double().cpu().numpy(), dict(rres4.named_parameters())[k].grad.numpy()) for k in r4t.RES4_NAMES}
    e5 = {k: _rel(dict(res5.named_parameters())[k].grad.double().cpu().numpy(), dict(rres5.named_parameters())[k].grad.numpy()) for k in r5t.RES5_NAMES}
    fe, he = neck._fpn_errors(fpn, rfpn), neck._head_errors(head, rhead)
    assert len(e4) == 57 and len(e5) == 30 and len(fe) == 10 and len(he) == 20
    e_run, counters = 0.0, 0
    for got, want in ((res4, rres4), (res5, rres5)):
        for (k, a), b in zip(got.named_buffers(), want.buffers()):
            assert bool(torch.isfinite(a).all()), k
            if a.dtype == torch.float32:
                e_run = max(e_run, _rel(a.double().cpu().numpy(), b.numpy()))
            else:
                counters += int(a) == 1
    assert counters == 29, "num_batches_tracked of the 29 BatchNorms"
    w4, w5, wf, wh = max(e4, key=e4.get), max(e5, key=e5.get), max(fe, key=fe.get), max(he, key=he.get)
    print(f"MEASURED bn chain: smallest ReLU argument on the stored taps {margin:.3g}, C4 {e_c4:.3g}, C5 {e_c5:.3g}, res4 grad {e4[w4]:.3g} ({w4}), res5 grad {e5[w5]:.3g} ({w5}), fpn grad {fe[wf]:.3g} ({wf}), "
          f"head grad {he[wh]:.3g} ({wh}), running {e_run:.3g}; {e4} {e5}")
    assert e4[w4] <= CHAIN_BOUNDS["res4"], e4
    assert e5[w5] <= CHAIN_BOUNDS["res5"], e5
    assert fe[wf] <= CHAIN_BOUNDS["fpn"], fe
    assert he[wh] <= CHAIN_BOUNDS["head"], he
    assert e_run <= CHAIN_BOUNDS["running"]


@pytest.mark.gpu
def test_res5_node_gives_the_bits_of_the_deeper_node(hip):
    """The property the node documents: a block's parameter gradients do not depend on whether its input gradient is formed, so the res5 node
    fed the C4 the deeper node produced gives that node's maps, res5 / FPN / head gradients and res5 buffers, bit for bit."""
    res4, res5, fpn, head, feats, targets, padded, _ = _chain_setup()
    state5, stateh = copy.deepcopy(res5.state_dict()), copy.deepcopy(head.state_dict())
    c4p = _stage_taps((res4,), padded[1])[-1]
    out, _ = r5t._loss_backward(fpn.forward_padded(padded, head=head, res5=res5, res4=res4, res_batch_stats=("res4", "res5")), targets)
    first = [out["probability"].detach(), out["threshold"].detach()] + [p.grad.clone() for m in (res5, fpn, head) for p in
                                                                        (m.live_parameters() if m is fpn else m.parameters())]
    buffers = [b.detach().clone() for b in res5.buffers()]
    res5.load_state_dict(state5)
    head.load_state_dict(stateh)
    for m in (res5, fpn, head):
        m.zero_grad(set_to_none=True)
    out2, _ = r5t._loss_backward(fpn.forward_padded(padded + [c4p], head=head, res5=res5, res_batch_stats=True), targets)
    second = [out2["probability"].detach(), out2["threshold"].detach()] + [p.grad for m in (res5, fpn, head) for p in
                                                                           (m.live_parameters() if m is fpn else m.parameters())]
    assert len(first) == len(second) == 62
    for i, (a, b) in enumerate(zip(first, second)):
        assert torch.equal(a, b), i
    for a, b in zip(buffers, res5.buffers()):
        assert torch.equal(a, b)
    assert all(int(bn.num_batches_tracked) == 1 for blk in res5 for bn in _bns(blk))


# ---- the product path
@pytest.mark.gpu
def test_product_step_with_batch_statistics(hip):
    """One training_step + AdamW step of the "head+fpn+res5+res4" mode under trunk_bn="bottleneck".  The batch is 2 x 3 x 640 x 640: the
    detector engine that gives the frozen part of the trunk takes 640 x 640 frames only."""
    from vtd_amd._fixtures.weights import stress_detector_state_dict
    torch.manual_seed(3)
    net = nets.DBNet("resnet50", compute_threshold=True, trainable="head+fpn+res5+res4", trunk_bn="bottleneck")
    net.load_state_dict(stress_detector_state_dict("resnet50", 17))
    net.cuda()
    gen = torch.Generator().manual_seed(23)
    x = torch.randn((2, 3, 640, 640), generator=gen).cuda()
    targets = neck._random_targets((2, 1, 640, 640), gen)
    net.eval()
    with torch.no_grad():
        before_map = net(x)["probability"].clone()
    net.train()
    trained = ("backbone.6.", "backbone.7.")
    mod = training.TextDetectionLightningModule(net)
    opt = mod.configure_optimizers()["optimizer"]
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    loss = mod.training_step((x, targets), 0)
    assert bool(torch.isfinite(loss))
    opt.zero_grad()
    loss.backward()
    trunk = {k: p for k, p in net.named_parameters() if k.startswith(trained)}
    assert len(trunk) == 87
    for k, p in trunk.items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k
    for i in range(6):
        assert all(p.grad is None for p in net.backbone[i].parameters())
    opt.step()
    after = net.state_dict()
    moved = [k for k in before if k.startswith(trained) and "running" in k]
    counts = [k for k in before if k.startswith(trained) and "num_batches" in k]
    assert len(moved) == 58 and len(counts) == 29
    for k in moved:
        assert bool(torch.isfinite(after[k]).all()) and not torch.equal(before[k], after[k]), f"{k} did not move"
    for k in counts:
        assert int(after[k]) == int(before[k]) + 1, k
    for k in trunk:
        assert not torch.equal(before[k], after[k]), f"{k} did not change"
    for k in before:      # every frozen tensor and buffer, bit for bit
        if k.startswith("backbone.") and not k.startswith(trained):
            assert torch.equal(before[k], after[k]), f"{k} changed"
    # a following eval() forward runs the fused inference engine on the stepped weights and the moved statistics
    net.eval()
    with torch.no_grad():
        got = net(x)
    assert bool(torch.isfinite(got["probability"]).all()) and not torch.equal(got["probability"], before_map)
    fresh = nets.DBNet("resnet50", compute_threshold=True)
    fresh.load_state_dict(net.state_dict())
    with torch.no_grad():
        want = fresh.cuda().eval()(x)
    assert torch.equal(got["probability"], want["probability"]) and torch.equal(got["threshold"], want["threshold"])
