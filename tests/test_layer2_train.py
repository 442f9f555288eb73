"""Training ResNet-18's layer2 (csrc/resblock_train.hip: the 128-wide blocks; csrc/wgrad_mfma.h: MODE 4, the weight gradients over a 64-channel
input), without a device: the workspace query and the refusals of the two new geometries, the weight gradient written out in fp64 as
MODE 4 gathers it (K laid out as tap * xc + ci, a tap per 64-column group, the half-empty last q-tile masked) against torch autograd, dC3 as
the sum of its three consumers' transposes -- with negative controls that must miss autograd by at least 10x the GPU tests' gradient bound
-- and the bookkeeping of the mode "head+fpn+layer4+layer3+layer2"."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_layer3_train as l3c
from vtd_amd import _native, nets
from vtd_amd.nets import forward_layer2_padded  # noqa: F401  (the feature under test: absent before it)

# no GPU gradient bound is above the project's ceiling for gradients (tests/test_gpu_layer2_train.py): a control that misses by 10x the
# ceiling misses by 10x every bound
GRAD_CEILING = 1e-2
NEW_GEOMETRIES = ((64, 128, 2), (128, 128, 1))
MODE = "head+fpn+layer4+layer3+layer2"
L3_MODE = "head+fpn+layer4+layer3"

_rel, _aligned = l3c._rel, l3c._aligned


# ---- C ABI, no device
def test_layer2_workspace_query():
    ws = _native.load().vtd_resblock_train_workspace_bytes
    for cin, width, stride in NEW_GEOMETRIES:
        for n, h, w in ((2, 6, 4), (2, 2, 2), (32, 80, 80)):
            for mode in (0, 1):
                b = ws(n, h, w, cin, width, stride, mode)
                assert b > 0 and b % 256 == 0, (n, h, w, cin, width, stride, mode)
        assert ws(32, 80, 80, cin, width, stride, 1) > ws(2, 2, 2, cin, width, stride, 1)
    for h, w in ((5, 4), (6, 3), (1, 1)):      # odd extents with stride 2
        assert ws(2, h, w, 64, 128, 2, 0) == -3101 and ws(2, h, w, 64, 128, 2, 1) == -3101
    # what stays refused: layer1's 64-wide block, the wrong stride for a channel pair, widths that are no stage of ResNet-18
    for mode in (0, 1):
        assert ws(2, 6, 4, 64, 64, 1, mode) == -3101
    for bad in ((2, 6, 4, 64, 128, 1), (2, 6, 4, 128, 128, 2), (2, 6, 4, 32, 64, 2), (2, 6, 4, 64, 256, 2), (0, 6, 4, 64, 128, 2), (2, 6, -1, 128, 128, 1)):
        assert ws(*bad, 0) == -3101, bad
    for mode in (2, -1):
        assert ws(2, 6, 4, 64, 128, 2, mode) == -3101
    # the old family keeps its gate: layer4's two geometries, -3001 for everything else
    old = _native.load().vtd_basicblock_train_workspace_bytes
    for cin, width, stride in NEW_GEOMETRIES:
        assert old(2, 6, 4, cin, width, stride, 0) == -3001 and old(2, 6, 4, cin, width, stride, 1) == -3001


def test_layer2_argument_and_alignment_errors():
    lib = _native.load()
    keep = [_aligned(4096) for _ in range(3)]
    a, b, c = (k[1] for k in keep)
    st = _native.BasicBlockParams(*([a] * 15))
    sp = C.byref(st)
    fwd, bwd = lib.vtd_resblock_train_forward, lib.vtd_resblock_train_backward
    # every refusal comes before any launch, so none of this needs a device
    for cin, width, stride in NEW_GEOMETRIES:
        g = (2, 6, 4, cin, width, stride)
        assert fwd(None, *g, sp, 1e-5, b, c, None) == -3101
        assert fwd(a, *g, None, 1e-5, b, c, None) == -3101
        assert fwd(a, *g, sp, 0.0, b, c, None) == -3101
        assert fwd(a, *g, sp, 1e-5, C.c_void_p(b.value + 128), c, None) == -3102
        assert fwd(C.c_void_p(a.value + 8), *g, sp, 1e-5, b, c, None) == -3102
        assert bwd(a, *g, sp, 1e-5, b, c, None, a, sp, b, None, None, None) == -3101          # no dy
        assert bwd(a, *g, sp, 1e-5, b, c, a, a, sp, None, None, None, None) == -3101          # no scratch
        assert bwd(a, *g, sp, 1e-5, b, c, a, a, sp, b, c, None, None) == -3101                # dx without a place for its scale
        assert bwd(a, *g, sp, 1e-5, b, c, a, a, sp, C.c_void_p(b.value + 128), None, None, None) == -3102
        assert bwd(a, *g, sp, 1e-5, b, c, a, a, sp, b, C.c_void_p(c.value + 8), a, None) == -3102     # a misaligned dx, either stride
    nods = _native.BasicBlockParams(*([a] * 10))
    assert fwd(a, 2, 6, 4, 64, 128, 2, C.byref(nods), 1e-5, b, c, None) == -3101      # a stride-2 block needs its downsample
    assert fwd(a, 2, 5, 4, 64, 128, 2, sp, 1e-5, b, c, None) == -3101
    assert fwd(a, 2, 6, 4, 64, 64, 1, sp, 1e-5, b, c, None) == -3101
    assert lib.vtd_basicblock_train_forward(a, 2, 6, 4, 128, 128, 1, sp, 1e-5, b, c, None) == -3001


def test_python_refusals_old_and_new():
    for blk, ch in ((nets.BasicBlock(64, 128, 2), 64), (nets.BasicBlock(128, 128, 1), 128)):
        with pytest.raises(ValueError, match="CUDA"):      # the geometry is accepted: the refusal is the CPU tensor's
            nets.basic_block_train(blk, torch.zeros((1, ch, 2, 2)))
    with pytest.raises(RuntimeError, match="layer3 and layer4"):
        nets.BasicBlock(64, 64, 1)._train_operands(torch.device("cpu"), general=True)
    with pytest.raises(RuntimeError, match="layer4 only"):
        nets.BasicBlock(128, 256, 2)._train_operands(torch.device("cpu"))
    with pytest.raises(RuntimeError, match="layer4 only"):
        nets.BasicBlock(64, 128, 2)._train_operands(torch.device("cpu"))
    with pytest.raises(RuntimeError, match="parameter containers"):
        nets.Bottleneck(256, 64, 1)(torch.zeros((1, 256, 2, 2)))
    with pytest.raises(RuntimeError, match="Bottleneck training is not built"):
        nets.forward_layer2_padded(nets.make_trunk("resnet50")[5], torch.zeros((1, 6, 6, 64)))
    with pytest.raises(ValueError, match="needs layer3, layer4 and the DBHead"):
        nets.FeaturePyramidNetwork(512).forward_padded([None], layer2=nets.make_trunk("resnet18")[5])


# ---- the weight gradient as MODE 4 gathers it, against autograd.  The kernel's q-tile is 128 columns in two groups of 64 and layer2.0's
# input has xc = 64 channels = one group; here the group is GW = 4 columns, the q-tile 8 and xc = 4, with 5 output channels: the same ratio,
# so K = 9 * 4 = 36 is 4.5 q-tiles (every q-tile holds two taps, the last is half empty) and K = 4 is half a q-tile, as K = 576 and K = 64 are
GW = 4


def _wgrad_case(h, w, ksz, seed=21):
    gen = torch.Generator().manual_seed(seed + 10 * h + w + ksz)
    x = torch.randn((2, GW, 2 * h, 2 * w), generator=gen).double()
    wt = (torch.randn((5, GW, ksz, ksz), generator=gen).double() * 0.3).requires_grad_(True)
    g = torch.randn((2, 5, h, w), generator=gen).double()
    return x, wt, g


def _mode4_wgrad(x, g, ksz, stride, bug=None):
    """G[p][q] = sum_m g[m][p] B[m][q], q = tap * xc + ci, as dbhead_train_wgrad_kernel<4> forms it from the ring-padded NHWC input: q-tile qt,
    group grp -> q0 = 2 GW qt + GW grp, tap = q0 / xc, first channel q0 % xc; groups at or past K load zeros and are not stored.  The
    slab is the flat [P][K] array the kernel writes, the input the flat padded array it reads."""
    n, xc, hin, win = x.shape
    P, h, w = g.shape[1], g.shape[2], g.shape[3]
    K, o = ksz * ksz * xc, 1 - ksz // 2
    xp = np.zeros((n, hin + 2, win + 2, xc))
    xp[:, 1:-1, 1:-1, :] = x.permute(0, 2, 3, 1).numpy()
    flat = np.concatenate([xp.reshape(-1), np.zeros(2 * GW)])
    a = g.permute(0, 2, 3, 1).reshape(-1, P).numpy()                # [M][P]
    img, y, xx = np.meshgrid(np.arange(n), np.arange(h), np.arange(w), indexing="ij")
    img, y, xx = img.reshape(-1), y.reshape(-1), xx.reshape(-1)
    slab = np.zeros(P * K + 2 * GW)
    for qt in range((K + 2 * GW - 1) // (2 * GW)):
        for grp in range(2):
            q0 = 2 * GW * qt + GW * grp
            if bug == "one_tap_per_qtile":                          # MODE 3's decode: the tap of the q-tile's first column for both groups
                tap = (2 * GW * qt) // xc
                c0 = 2 * GW * qt - tap * xc + GW * grp
            else:
                tap, c0 = q0 // xc, q0 % xc
            active = q0 < K
            if active:
                ky, kx = tap // ksz, tap % ksz
                base = (((img * (hin + 2) + y * stride + ky + o) * (win + 2)) + xx * stride + kx + o) * xc + c0
                B = flat[base[:, None] + np.arange(GW)[None, :]]    # [M][GW]
            else:
                B = np.zeros((a.shape[0], GW))
            if not active and bug != "last_qtile_stored":
                continue
            tile = a.T @ B                                          # [P][GW]
            for p in range(P):
                slab[p * K + q0:p * K + q0 + GW] = tile[p]
    G = slab[:P * K].reshape(P, ksz * ksz, xc)                      # [co][tap][ci]
    return torch.from_numpy(G).permute(0, 2, 1).reshape(P, xc, ksz, ksz)


SIZES = [(1, 1), (3, 2), (5, 4)]
CONVS = [(3, 2), (1, 2)]      # layer2.0's conv1 and its downsample: (ksz, stride)


@pytest.mark.parametrize("conv", CONVS)
@pytest.mark.parametrize("size", SIZES)
def test_mode4_weight_gradient_matches_autograd(size, conv):
    ksz, stride = conv
    x, wt, g = _wgrad_case(*size, ksz)
    F.conv2d(x, wt, None, stride, ksz // 2).backward(g)
    got = _mode4_wgrad(x, g, ksz, stride)
    assert got.shape == wt.shape and _rel(got.numpy(), wt.grad.numpy()) <= 1e-12


# A 1x1 window has one tap, so the two decodes agree there: that control is the 3x3 window's alone.  No control can show at a 1x1 output of
# a 2x2 input: the taps the wrong decode exchanges (3 and 5 for the pixels right of 2 and 4) and tap 0, whose columns the unmasked store
# overwrites, all read the zero ring there, so their gradients are zero either way
@pytest.mark.parametrize("conv,bug", [((3, 2), "one_tap_per_qtile"), ((3, 2), "last_qtile_stored"), ((1, 2), "last_qtile_stored")])
@pytest.mark.parametrize("size", SIZES[1:])
def test_mode4_weight_gradient_negative_controls(size, conv, bug):
    ksz, stride = conv
    x, wt, g = _wgrad_case(*size, ksz)
    F.conv2d(x, wt, None, stride, ksz // 2).backward(g)
    err = _rel(_mode4_wgrad(x, g, ksz, stride, bug).numpy(), wt.grad.numpy())
    assert err >= 10 * GRAD_CEILING, f"{bug} at {size}, {ksz}x{ksz}: error {err:.3g} is not 10x the bound {GRAD_CEILING}"


@pytest.mark.parametrize("bug", [None, "conv1_left_out", "downsample_left_out", "fpn_dc3_left_out"])
@pytest.mark.parametrize("size", SIZES)
def test_dc3_is_the_sum_of_its_three_consumers(bug, size):
    """C3 feeds layer3.0 (3x3 stride 2 and the 1x1 stride-2 downsample) and the FPN's lateral: dC3 is the sum of the three transposes, the
    first two as the strided input gradient forms them (tests/test_layer3_train.py)."""
    x, w1, wd, g1, g2 = l3c._strided_case(*size, seed=13)
    gen = torch.Generator().manual_seed(79)
    lat = torch.randn((4, 6, 1, 1), generator=gen).double() * 0.3
    gl = torch.randn((2, 4, x.shape[2], x.shape[3]), generator=gen).double()
    torch.autograd.backward([F.conv2d(x, w1, None, 2, 1), F.conv2d(x, wd, None, 2, 0), F.conv2d(x, lat)], [g1, g2, gl])
    got = torch.zeros_like(x.detach())
    if bug != "conv1_left_out":
        got = got + l3c._conv1_transpose(g1, w1)
    if bug != "downsample_left_out":
        got = l3c._downsample_transpose(got, g2, wd)
    if bug != "fpn_dc3_left_out":
        got = got + torch.einsum("nohw,oc->nchw", gl, lat[:, :, 0, 0])
    err = _rel(got.numpy(), x.grad.numpy())
    assert err <= 1e-12 if bug is None else err >= 10 * GRAD_CEILING, f"{bug}: {err:.3g}"


# ---- the product mode
def test_head_fpn_layer4_layer3_layer2_mode():
    net = nets.DBNet("resnet18", trainable=MODE)
    assert net.trainable == MODE
    for i in range(5):
        assert not any(p.requires_grad for p in net.backbone[i].parameters()), i
    for m in (net.backbone[5], net.backbone[6], net.backbone[7], net.fpn, net.head):
        assert all(p.requires_grad for p in m.parameters())
    assert len(list(net.backbone[5].parameters())) == 15 and len(list(net.backbone[5].buffers())) == 15
    # the eval-mode rebuild is keyed on layer2's tensors too (15 parameters, 5 BatchNorms x 3 buffers)
    assert len(net._head_tensor_versions()) == len(nets.DBNet("resnet18", trainable=L3_MODE)._head_tensor_versions()) + 30
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
                 "head+fpn+layer2+layer3+layer4", "head+fpn+layer4+layer2"):
        with pytest.raises(ValueError, match="trainable"):
            nets.DBNet("resnet18", trainable=mode)
    # a frozen trunk tensor that requires grad is refused in a train-mode forward, before anything touches a device
    net = nets.DBNet("resnet18", trainable=MODE)
    net.backbone[4][1].conv2.weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match="backward below layer2 is not"):
        net.train()(torch.zeros((1, 3, 640, 640)))
    # the two narrower modes keep their refusal texts
    net3 = nets.DBNet("resnet18", trainable=L3_MODE)
    net3.backbone[5][1].conv2.weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match="backward below layer3 is not"):
        net3.train()(torch.zeros((1, 3, 640, 640)))
    net4 = nets.DBNet("resnet18", trainable="head+fpn+layer4")
    net4.backbone[6][0].conv1.weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match="backward below layer4 is not"):
        net4.train()(torch.zeros((1, 3, 640, 640)))


def test_switching_between_modes():
    grads = lambda net, i: [p.requires_grad for p in net.backbone[i].parameters()]  # noqa: E731
    net = nets.DBNet("resnet18", trainable=L3_MODE)
    assert not any(grads(net, 5)) and all(grads(net, 6)) and all(grads(net, 7))
    net.set_trainable(MODE)
    assert all(grads(net, 5)) and all(grads(net, 6)) and all(grads(net, 7)) and not any(grads(net, 4))
    net.set_trainable(L3_MODE)      # and back: layer2 is frozen again
    assert not any(grads(net, 5)) and all(grads(net, 6))
    net.set_trainable(MODE).set_trainable("head+fpn+layer4")
    assert not any(grads(net, 5)) and not any(grads(net, 6)) and all(grads(net, 7))
    net.set_trainable(MODE).set_trainable("head+fpn")
    assert not any(p.requires_grad for p in net.backbone.parameters()) and all(p.requires_grad for p in net.fpn.parameters())
    net.set_trainable("head")
    assert not any(p.requires_grad for p in net.fpn.parameters())
    net.set_trainable(MODE)
    for m in (net.backbone[5], net.backbone[6], net.backbone[7], net.fpn, net.head):
        assert all(p.requires_grad for p in m.parameters())
    assert not any(p.requires_grad for i in range(5) for p in net.backbone[i].parameters())
