"""Training ResNet-18's layer1 (csrc/resblock_train.hip: the 64-wide block behind the vtd_block64_train_* entries; csrc/wgrad_mfma.h: MODE 5,
the 64-row tile over a 64-channel input), without a device: the new symbols, the workspace query and the refusals of the new entry family,
the pins of the old families restated, the weight gradient written out in fp64 as MODE 5 gathers it (five q-tiles of two 64-column groups,
a tap per group, the last group empty, slabs by the kernel's own rule) against torch autograd -- with the MODE 3 decode as a control that
must miss --, the quarter reduce's summation order, dC2 as the sum of layer2.0's input gradient and the FPN's dC2 on the chain the GPU test
runs, and the bookkeeping of the mode "head+fpn+layer4+layer3+layer2+layer1"."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_layer3_train as l3c
from vtd_amd import _native, nets
from vtd_amd.nets import forward_layer1_padded  # noqa: F401  (the feature under test: absent before it)

# no GPU gradient bound is above the project's ceiling for gradients (tests/test_gpu_layer1_train.py): a control that misses by 10x the
# ceiling misses by 10x every bound
GRAD_CEILING = 1e-2
GEOMETRY = (64, 64, 1)
WIDER = ((64, 128, 2), (128, 128, 1), (128, 256, 2), (256, 256, 1), (256, 512, 2), (512, 512, 1))
MODE = "head+fpn+layer4+layer3+layer2+layer1"
L2_MODE = "head+fpn+layer4+layer3+layer2"
NARROWER = ("head+fpn+layer4+layer3+layer2", "head+fpn+layer4+layer3", "head+fpn+layer4", "head+fpn", "head")

_rel, _aligned = l3c._rel, l3c._aligned


# ---- C ABI, no device
def test_layer1_symbols_and_error_text():
    lib = _native.load()
    for name in ("vtd_block64_train_workspace_bytes", "vtd_block64_train_forward", "vtd_block64_train_backward", "vtd_detector_forward_pool"):
        assert name in _native.SIGNATURES and hasattr(lib, name), name
    for code in (-3201, -3202):
        assert b"64-wide block training" in lib.vtd_strerror(code)
    assert b"geometry" in lib.vtd_strerror(-3201) and b"misaligned" in lib.vtd_strerror(-3202)
    # the other families' texts are unchanged
    assert b"ResNet block training" in lib.vtd_strerror(-3101) and b"BasicBlock training" in lib.vtd_strerror(-3001)


def test_layer1_workspace_query():
    ws = _native.load().vtd_block64_train_workspace_bytes
    for n, h, w in ((2, 6, 4), (2, 2, 2), (32, 160, 160)):
        for mode in (0, 1):
            b = ws(n, h, w, *GEOMETRY, mode)
            assert b > 0 and b % 256 == 0, (n, h, w, mode)
    for mode in (0, 1):
        assert ws(32, 160, 160, *GEOMETRY, mode) > ws(2, 6, 4, *GEOMETRY, mode) > ws(2, 2, 2, *GEOMETRY, mode)
    # one geometry and no other: the six wider ones belong to vtd_resblock_train_*
    for cin, width, stride in WIDER:
        for mode in (0, 1):
            assert ws(2, 6, 4, cin, width, stride, mode) == -3201, (cin, width, stride)
    for bad in ((2, 6, 4, 32, 64, 1), (2, 6, 4, 128, 64, 1), (2, 6, 4, 64, 64, 2), (2, 6, 4, 32, 64, 2), (0, 6, 4, 64, 64, 1), (2, -6, 4, 64, 64, 1),
                (2, 6, -1, 64, 64, 1), (2, 0, 4, 64, 64, 1), (-1, 6, 4, 64, 64, 1)):
        assert ws(*bad, 0) == -3201 and ws(*bad, 1) == -3201, bad
    for mode in (2, -1):
        assert ws(2, 6, 4, *GEOMETRY, mode) == -3201


def test_layer1_argument_and_alignment_errors():
    lib = _native.load()
    keep = [_aligned(4096) for _ in range(3)]
    a, b, c = (k[1] for k in keep)
    st = _native.BasicBlockParams(*([a] * 15))
    sp = C.byref(st)
    fwd, bwd = lib.vtd_block64_train_forward, lib.vtd_block64_train_backward
    # every refusal comes before any launch, so none of this needs a device
    g = (2, 6, 4, *GEOMETRY)
    assert fwd(None, *g, sp, 1e-5, b, c, None) == -3201
    assert fwd(a, *g, None, 1e-5, b, c, None) == -3201
    assert fwd(a, *g, sp, 1e-5, None, c, None) == -3201
    assert fwd(a, *g, sp, 1e-5, b, None, None) == -3201
    assert fwd(a, *g, sp, 0.0, b, c, None) == -3201
    assert fwd(a, *g, sp, 1e-5, C.c_void_p(b.value + 128), c, None) == -3202          # a misaligned workspace
    assert fwd(C.c_void_p(a.value + 8), *g, sp, 1e-5, b, c, None) == -3202            # a misaligned x
    assert fwd(a, *g, sp, 1e-5, b, C.c_void_p(c.value + 8), None) == -3202            # a misaligned y
    assert bwd(a, *g, sp, 1e-5, b, c, None, a, sp, b, None, None, None) == -3201          # no dy
    assert bwd(a, *g, sp, 1e-5, b, c, a, None, sp, b, None, None, None) == -3201          # no dscale
    assert bwd(a, *g, sp, 1e-5, b, c, a, a, None, b, None, None, None) == -3201           # no place for the gradients
    assert bwd(a, *g, sp, 1e-5, b, c, a, a, sp, None, None, None, None) == -3201          # no scratch
    assert bwd(a, *g, sp, 0.0, b, c, a, a, sp, b, None, None, None) == -3201              # eps = 0
    assert bwd(a, *g, sp, 1e-5, b, c, a, a, sp, b, c, None, None) == -3201                # dx without a place for its scale
    assert bwd(a, *g, sp, 1e-5, C.c_void_p(b.value + 128), c, a, a, sp, b, None, None, None) == -3202     # a misaligned workspace
    assert bwd(C.c_void_p(a.value + 8), *g, sp, 1e-5, b, c, a, a, sp, b, None, None, None) == -3202       # a misaligned x
    assert bwd(a, *g, sp, 1e-5, b, c, a, a, sp, C.c_void_p(b.value + 128), None, None, None) == -3202     # a misaligned scratch
    assert bwd(a, *g, sp, 1e-5, b, c, a, a, sp, b, C.c_void_p(c.value + 8), a, None) == -3202             # a misaligned dx
    assert bwd(a, *g, sp, 1e-5, b, c, a, C.c_void_p(a.value + 4), sp, b, None, None, None) == -3202
    nods = _native.BasicBlockParams(*([a] * 10))      # the identity block ignores ds_*: the refusal is the workspace's
    assert fwd(a, *g, C.byref(nods), 1e-5, C.c_void_p(b.value + 128), c, None) == -3202
    for cin, width, stride in WIDER + ((64, 64, 2), (32, 64, 1)):
        assert fwd(a, 2, 6, 4, cin, width, stride, sp, 1e-5, b, c, None) == -3201
        assert bwd(a, 2, 6, 4, cin, width, stride, sp, 1e-5, b, c, a, a, sp, b, c, a, None) == -3201
    assert lib.vtd_detector_forward_pool(None, 1, a, None) == -1100      # the detector entries' argument error


def test_pins_of_the_other_entry_families_hold():
    lib = _native.load()
    keep = [_aligned(4096) for _ in range(3)]
    a, b, c = (k[1] for k in keep)
    sp = C.byref(_native.BasicBlockParams(*([a] * 15)))
    for mode in (0, 1):
        assert lib.vtd_resblock_train_workspace_bytes(2, 6, 4, 64, 64, 1, mode) == -3101
        assert lib.vtd_basicblock_train_workspace_bytes(2, 6, 4, 64, 64, 1, mode) == -3001
    assert lib.vtd_resblock_train_forward(a, 2, 6, 4, 64, 64, 1, sp, 1e-5, b, c, None) == -3101
    assert lib.vtd_resblock_train_backward(a, 2, 6, 4, 64, 64, 1, sp, 1e-5, b, c, a, a, sp, b, c, a, None) == -3101
    assert lib.vtd_basicblock_train_forward(a, 2, 6, 4, 64, 64, 1, sp, 1e-5, b, c, None) == -3001
    with pytest.raises(RuntimeError, match="layer3 and layer4"):
        nets.BasicBlock(64, 64, 1)._train_operands(torch.device("cpu"), general=True)
    with pytest.raises(RuntimeError, match="layer4 only"):
        nets.BasicBlock(64, 64, 1)._train_operands(torch.device("cpu"))


def test_python_refusals_old_and_new():
    with pytest.raises(ValueError, match="CUDA"):      # the geometry is accepted: the refusal is the CPU tensor's
        nets.basic_block_train(nets.BasicBlock(64, 64, 1), torch.zeros((1, 64, 2, 2)))
    with pytest.raises(ValueError, match="CUDA"):      # likewise: the parameters are not on a device
        nets.BasicBlock(64, 64, 1)._train_operands(torch.device("cpu"), general=True, narrow=True)
    with pytest.raises(RuntimeError, match="layer3 and layer4"):      # the new keyword admits layer1's block and nothing else
        nets.BasicBlock(64, 128, 1)._train_operands(torch.device("cpu"), general=True, narrow=True)
    with pytest.raises(RuntimeError, match="layer4 only"):
        nets.BasicBlock(128, 128, 1)._train_operands(torch.device("cpu"), narrow=True)
    with pytest.raises(ValueError, match="must be a"):
        nets.basic_block_train(nets.BasicBlock(64, 64, 1), torch.zeros((1, 128, 2, 2)))
    with pytest.raises(RuntimeError, match="Bottleneck training is not built"):
        nets.forward_layer1_padded(nets.make_trunk("resnet50")[4], torch.zeros((1, 6, 6, 64)))
    with pytest.raises(ValueError, match="needs layer2, layer3, layer4 and the DBHead"):
        nets.FeaturePyramidNetwork(512).forward_padded([None], layer1=nets.make_trunk("resnet18")[4])
    trunk = nets.make_trunk("resnet18")
    with pytest.raises(ValueError, match="needs layer2, layer3, layer4 and the DBHead"):
        nets.FeaturePyramidNetwork(512).forward_padded([None], head=nets.DBHead(256), layer4=trunk[7], layer3=trunk[6], layer1=trunk[4])
    assert "seven blocks" in nets.basic_block_train.__doc__


# ---- the weight gradient as MODE 5 gathers it, against autograd, at the kernel's own sizes: 64 gradient columns (one 64-row tile), a
# 64-channel input, K = 9 * 64 = 576 = 4.5 q-tiles of 128 columns
XC, PW, QT, GRP = 64, 64, 128, 64
SIZES = [(1, 1), (3, 2), (5, 4), (23, 23)]


def _slabs(rows, nqt):
    """csrc/resblock_train.hip: wg_slabs128 and slab_rows (32-row chunks)."""
    s = max(1, min((512 + nqt - 1) // nqt, (rows + 1023) // 1024))
    return s, ((rows + s - 1) // s + 31) // 32 * 32


def _wgrad_case(h, w, seed=31):
    gen = torch.Generator().manual_seed(seed + 10 * h + w)
    x = torch.randn((2, XC, h, w), generator=gen).double()
    wt = (torch.randn((PW, XC, 3, 3), generator=gen).double() * 0.1).requires_grad_(True)
    g = torch.randn((2, PW, h, w), generator=gen).double()
    return x, wt, g


def _mode5_wgrad(x, g, slabs=None, bug=None):
    """G[p][q] = sum over the slabs, in slab order, of sum_m g[m][p] B[m][q], as dbhead_train_wgrad_kernel<5> and rb_param_kernel form it:
    q-tile qt, group grp -> q0 = 128 qt + 64 grp, tap = q0 / xc, first channel q0 % xc; the group at q0 = 576 loads zeros and is not
    stored.  A slab is the flat [64][576] array the kernel writes, the input the flat ring-padded NHWC array it reads."""
    n, xc, h, w = x.shape
    P, K = g.shape[1], 9 * xc
    nqt = (K + QT - 1) // QT
    assert (xc, P, K, nqt) == (64, 64, 576, 5)
    xp = np.zeros((n, h + 2, w + 2, xc))
    xp[:, 1:-1, 1:-1, :] = x.permute(0, 2, 3, 1).numpy()
    flat = np.concatenate([xp.reshape(-1), np.zeros(QT)])
    a = g.permute(0, 2, 3, 1).reshape(-1, P).numpy()                # [M][P]
    M = a.shape[0]
    img, y, xx = (v.reshape(-1) for v in np.meshgrid(np.arange(n), np.arange(h), np.arange(w), indexing="ij"))
    S, slab_len = slabs if slabs is not None else _slabs(M, nqt)
    total = np.zeros(P * K)
    for sl in range(S):
        r0, r1 = sl * slab_len, min((sl + 1) * slab_len, M)
        slab = np.zeros(P * K + QT)
        for qt in range(nqt):
            for grp in range(2):
                q0 = QT * qt + GRP * grp
                if bug == "one_tap_per_qtile":                      # MODE 3's decode: the tap of the q-tile's first column for both groups
                    tap = (QT * qt) // xc
                    c0 = QT * qt - tap * xc + GRP * grp
                else:
                    tap, c0 = q0 // xc, q0 % xc
                if q0 >= K:
                    continue                                        # loads zeros, stores nothing
                ky, kx = tap // 3, tap % 3
                rows = slice(r0, max(r0, r1))
                base = (((img[rows] * (h + 2) + y[rows] + ky) * (w + 2)) + xx[rows] + kx) * xc + c0
                tile = a[rows].T @ flat[base[:, None] + np.arange(GRP)[None, :]]      # [P][64]
                for p in range(P):
                    slab[p * K + q0:p * K + q0 + GRP] = tile[p]
        total = total + slab[:P * K]
    return torch.from_numpy(total.reshape(P, 9, xc)).permute(0, 2, 1).reshape(P, xc, 3, 3)


@pytest.mark.parametrize("size", SIZES)
def test_mode5_weight_gradient_matches_autograd(size):
    x, wt, g = _wgrad_case(*size)
    F.conv2d(x, wt, None, 1, 1).backward(g)
    rows = 2 * size[0] * size[1]
    S, slab_len = _slabs(rows, 5)
    if size == (23, 23):      # the smallest multi-slab case: 1058 rows = a slab of 544 and one of 514, which ends inside a 32-row chunk
        assert (S, slab_len) == (2, 544) and (rows - slab_len) % 32 == 2
    else:
        assert S == 1
    got = _mode5_wgrad(x, g)
    assert got.shape == wt.shape and _rel(got.numpy(), wt.grad.numpy()) <= 1e-12
    # two uneven slabs at every size: the second is shorter, and empty where the first chunk holds every row
    forced = _mode5_wgrad(x, g, slabs=(2, ((rows + 1) // 2 + 31) // 32 * 32))
    assert _rel(forced.numpy(), wt.grad.numpy()) <= 1e-12
    assert _slabs(32 * 160 * 160, 5) == (103, 7968)      # the product shape at B = 32: min(ceil(512 / 5), 800) slabs


# No control can show at a 1x1 output: the taps the wrong decode exchanges read the zero ring there
@pytest.mark.parametrize("size", SIZES[1:])
def test_mode5_weight_gradient_negative_control(size):
    x, wt, g = _wgrad_case(*size)
    F.conv2d(x, wt, None, 1, 1).backward(g)
    err = _rel(_mode5_wgrad(x, g, bug="one_tap_per_qtile").numpy(), wt.grad.numpy())
    assert err >= 10 * GRAD_CEILING, f"MODE 3's decode at {size}: error {err:.3g} is not 10x the bound {GRAD_CEILING}"


@pytest.mark.parametrize("rows", [2, 12, 40, 1058, 70000])
def test_quarter_reduce_order(rows):
    """rb_reduce64_kernel and rb_finish_kernel written out: ceil(rows / 256) workgroups (at most 256) of `per` rows, each cut into four
    quarters at ceil(k r / 4), the partial (q0 + q1) + (q2 + q3), the partials added in workgroup order."""
    v = torch.randn((rows, 64), generator=torch.Generator().manual_seed(rows)).double().numpy()
    G = min(256, max(1, (rows + 255) // 256))
    per = (rows + G - 1) // G
    total, seen = np.zeros(64), 0
    for g in range(G):
        m0 = min(g * per, rows)
        m1 = min(m0 + per, rows)
        r = m1 - m0
        cuts = [m0 + (k * r + 3) // 4 for k in range(5)]
        assert cuts[0] == m0 and cuts[4] == m1 and all(0 <= b - a <= (r + 3) // 4 for a, b in zip(cuts, cuts[1:]))
        q = [v[a:b].sum(axis=0) for a, b in zip(cuts, cuts[1:])]
        total = total + ((q[0] + q[1]) + (q[2] + q[3]))
        seen += r
    assert seen == rows
    if rows == 1058:      # the GPU test's multi-slab case: five partials of 212 rows, quarters of 53
        assert (G, per) == (5, 212)
    assert _rel(total, v.sum(axis=0)) <= 1e-12


# ---- the chain layer1 -> layer2 -> layer3 -> layer4 -> FPN -> head -> loss on a pool tap of 24 x 16 (C5 = 3 x 2), n = 2: the modules and
# inputs of tests/test_gpu_layer1_train.py's chain case, built here on the CPU.  The seed is chosen so that both summands of dC2 matter
CHAIN_SEED = 61
CHAIN_N, CHAIN_H5, CHAIN_W5 = 2, 3, 2


def seeded_block_cpu(cin, width, stride, seed):
    """tests/test_gpu_layer3_train.py's _seeded_block, left on the CPU."""
    blk = nets.BasicBlock(cin, width, stride)
    blk.load_state_dict(nets.seeded_state_dict(lambda: nets.BasicBlock(cin, width, stride), seed))
    with torch.no_grad():      # a gamma = 0 channel (zero_init_residual) and a gamma < 0 channel (the folded weights change sign)
        blk.bn2.weight[3] = 0.0
        blk.bn2.weight[7] = -0.75
    return blk


def chain_modules(seed=CHAIN_SEED):
    """(layer1, layer2, layer3, layer4, fpn, head) on the CPU in float32, the pool tap [2,64,24,16] (fp16-representable, non-negative as a
    max-pooled ReLU output is) and the targets.  layer2 .. layer4, the FPN, the head and the targets are those of the layer2 chain case
    (tests/test_gpu_layer2_train.py: _chain_setup), so that the figures of the stages above layer1 stand beside that case's; `seed` gives
    layer1's two blocks and the pool tap."""
    l1 = torch.nn.Sequential(seeded_block_cpu(64, 64, 1, seed), seeded_block_cpu(64, 64, 1, seed + 1))
    l2 = torch.nn.Sequential(seeded_block_cpu(64, 128, 2, 91), seeded_block_cpu(128, 128, 1, 92))
    l3 = torch.nn.Sequential(seeded_block_cpu(128, 256, 2, 93), seeded_block_cpu(256, 256, 1, 94))
    l4 = torch.nn.Sequential(seeded_block_cpu(256, 512, 2, 95), seeded_block_cpu(512, 512, 1, 96))
    fpn = nets.FeaturePyramidNetwork(512)
    fpn.load_state_dict(nets.seeded_state_dict(lambda: nets.FeaturePyramidNetwork(512), 6))
    head = nets.DBHead(256)
    head.load_state_dict(nets.seeded_state_dict(lambda: nets.DBHead(256), 8))
    gen = torch.Generator().manual_seed(57)
    for lv in range(4):      # that case draws its four taps first
        torch.randn((CHAIN_N, 512 >> (3 - lv), CHAIN_H5 << (3 - lv), CHAIN_W5 << (3 - lv)), generator=gen)
    shape = (CHAIN_N, 1, 32 * CHAIN_H5, 32 * CHAIN_W5)
    targets = {"probability_map": (torch.rand(shape, generator=gen) > 0.7).float(), "threshold_map": torch.rand(shape, generator=gen) * 0.6 + 0.2}
    pool = (torch.randn((CHAIN_N, 64, 8 * CHAIN_H5, 8 * CHAIN_W5), generator=torch.Generator().manual_seed(seed + 10)) * 0.5).abs().half().float()
    return (l1, l2, l3, l4, fpn, head.train()), pool, targets


def _plain_block(blk, x):
    """The block with frozen-statistics BatchNorm in torch ops."""
    def conv_bn(t, conv, bn, stride, pad):
        sc = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        return F.conv2d(t, conv.weight, None, stride, pad) * sc[None, :, None, None] + (bn.bias - bn.running_mean * sc)[None, :, None, None]
    a1 = F.relu(conv_bn(x, blk.conv1, blk.bn1, blk.stride, 1))
    idt = conv_bn(x, blk.downsample[0], blk.downsample[1], blk.stride, 0) if hasattr(blk, "downsample") else x
    return F.relu(conv_bn(a1, blk.conv2, blk.bn2, 1, 1) + idt)


def _loss(prob, thresh, targets):
    """app/ml/training/trainer.py:48-56: two BCE terms and the Dice loss (oracle/loss.py)."""
    pm, tm = targets["probability_map"].double(), targets["threshold_map"].double()
    dice = 1.0 - (2.0 * (prob * pm).sum() + 1e-5) / (prob.sum() + pm.sum() + 1e-5)
    return F.binary_cross_entropy(prob, pm) + F.binary_cross_entropy(thresh, tm) + dice


_CHAIN = {}


def _chain_fp64(drop=None):
    """fp64 CPU autograd of the chain, cut at C2 so that its two consumers' gradients are seen apart: (layer2.0's dx, the FPN's dC2, layer1's
    twelve gradients with `drop` ("trunk" or "fpn") left out of dC2).  The two summands are computed once."""
    if "parts" not in _CHAIN:
        mods, pool, targets = chain_modules()
        l1, l2, l3, l4, fpn, head = (copy.deepcopy(m).double() for m in mods)
        c2 = _plain_block(l1[1], _plain_block(l1[0], pool.double()))
        to_l2, to_fpn = c2.detach().requires_grad_(True), c2.detach().requires_grad_(True)
        c3 = _plain_block(l2[1], _plain_block(l2[0], to_l2))
        c4 = _plain_block(l3[1], _plain_block(l3[0], c3))
        c5 = _plain_block(l4[1], _plain_block(l4[0], c4))
        last = fpn.inner_blocks[0](c5)
        for i, t in enumerate((c4, c3, to_fpn), 1):
            last = fpn.inner_blocks[i](t) + F.interpolate(last, scale_factor=2, mode="nearest")
        p2 = fpn.layer_blocks[3](last)
        _loss(head.probability_head(p2), head.threshold_head(p2), targets).backward()
        _CHAIN["parts"] = (l1, c2, to_l2.grad.clone(), to_fpn.grad.clone())
    l1, c2, d_trunk, d_fpn = _CHAIN["parts"]
    l1.zero_grad(set_to_none=True)
    up = (0 if drop == "trunk" else d_trunk) + (0 if drop == "fpn" else d_fpn)
    c2.backward(up, retain_graph=True)
    return d_trunk, d_fpn, {k: p.grad.clone() for k, p in l1.named_parameters()}


def test_dc2_is_the_sum_of_both_consumers_and_both_matter():
    d_trunk, d_fpn, want = _chain_fp64()
    assert len(want) == 12
    total = float((d_trunk + d_fpn).norm())
    shares = float(d_trunk.norm()) / total, float(d_fpn.norm()) / total
    print(f"shares of dC2's norm at seed {CHAIN_SEED}: layer2.0's dx {shares[0]:.3g}, the FPN's dC2 {shares[1]:.3g}")
    assert min(shares) >= 0.1, shares
    for drop in ("trunk", "fpn"):
        _, _, got = _chain_fp64(drop)
        worst = max(_rel(got[k].numpy(), want[k].numpy()) for k in want)
        assert worst >= 10 * GRAD_CEILING, f"dC2 without the {drop} summand moves layer1's gradients by {worst:.3g} only"
    _, _, again = _chain_fp64()
    assert all(torch.equal(again[k], want[k]) for k in want)


# ---- the product mode
def _trained(net):
    return [p for i in (4, 5, 6, 7) for p in net.backbone[i].parameters()] + list(net.fpn.live_parameters()) + list(net.head.parameters())


def test_layer1_mode():
    net = nets.DBNet("resnet18", trainable=MODE)
    assert net.trainable == MODE
    for i in range(4):
        assert not any(p.requires_grad for p in net.backbone[i].parameters()), i
    for m in (net.backbone[4], net.backbone[5], net.backbone[6], net.backbone[7], net.fpn, net.head):
        assert all(p.requires_grad for p in m.parameters())
    assert len(list(net.backbone[4].parameters())) == 12 and len(list(net.backbone[4].buffers())) == 12
    # the tensors that receive a gradient: the layer2 mode's 75 and layer1's 12
    assert len(_trained(net)) == 87 and all(p.requires_grad for p in _trained(net))
    l2net = nets.DBNet("resnet18", trainable=L2_MODE)
    assert sum(1 for p in _trained(l2net) if p.requires_grad) == 75
    frozen = [k for k, p in net.named_parameters() if not p.requires_grad]
    assert frozen == ["backbone.0.weight", "backbone.1.weight", "backbone.1.bias"]
    # the eval-mode rebuild is keyed on layer1's tensors too (12 parameters, 4 BatchNorms x 3 buffers)
    assert len(net._head_tensor_versions()) == len(l2net._head_tensor_versions()) + 24
    # the state dict is the reference's, whatever the mode
    assert list(net.state_dict()) == list(nets.DBNet("resnet18").state_dict())
    assert MODE in nets.DBNet.set_trainable.__doc__


def test_mode_refusals():
    with pytest.raises(ValueError, match="Bottleneck training is not built"):
        nets.DBNet("resnet50", trainable=MODE)
    with pytest.raises(ValueError, match="Bottleneck training is not built"):
        nets.DBNet("resnet50").set_trainable(MODE)
    # the names that were refused stay refused
    for mode in ("layer4", "head+layer4", "head+fpn+layer3", "all", "layer3", "head+fpn+layer3+layer2", "head+fpn+layer3+layer4", "layer2",
                 "head+fpn+layer2+layer3+layer4", "head+fpn+layer4+layer2", "layer1", "head+fpn+layer4+layer3+layer1", "head+fpn+layer1",
                 "head+fpn+layer1+layer2+layer3+layer4", "head+fpn+layer4+layer3+layer2+layer1+stem"):
        with pytest.raises(ValueError, match="trainable"):
            nets.DBNet("resnet18", trainable=mode)
    # a stem tensor that requires grad is refused in a train-mode forward, before anything touches a device
    for pick in (lambda n: n.backbone[0].weight, lambda n: n.backbone[1].bias):
        net = nets.DBNet("resnet18", trainable=MODE)
        pick(net).requires_grad_(True)
        with pytest.raises(RuntimeError, match="backward below layer1 is not"):
            net.train()(torch.zeros((1, 3, 640, 640)))
    # the narrower mode keeps its refusal text
    net2 = nets.DBNet("resnet18", trainable=L2_MODE)
    net2.backbone[4][1].conv2.weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match="backward below layer2 is not"):
        net2.train()(torch.zeros((1, 3, 640, 640)))


def test_switching_between_modes():
    grads = lambda net, i: [p.requires_grad for p in net.backbone[i].parameters()]  # noqa: E731
    first_frozen = {"head+fpn+layer4+layer3+layer2": 5, "head+fpn+layer4+layer3": 6, "head+fpn+layer4": 7, "head+fpn": 8, "head": 8}
    net = nets.DBNet("resnet18", trainable=L2_MODE)
    assert not any(grads(net, 4)) and all(grads(net, 5))
    for other in NARROWER:
        net.set_trainable(MODE)
        assert all(all(grads(net, i)) for i in (4, 5, 6, 7)) and not any(p.requires_grad for i in range(4) for p in net.backbone[i].parameters())
        assert all(p.requires_grad for m in (net.fpn, net.head) for p in m.parameters())
        net.set_trainable(other)      # and back: layer1 is frozen again, with every stage the narrower mode does not train
        for i in range(4, 8):
            assert all(grads(net, i)) if i >= first_frozen[other] else not any(grads(net, i)), (other, i)
        assert all(p.requires_grad for p in net.fpn.parameters()) == (other != "head")
        assert all(p.requires_grad for p in net.head.parameters())
    net.set_trainable(MODE)
    assert len(_trained(net)) == 87 and all(p.requires_grad for p in _trained(net))
