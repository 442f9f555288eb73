"""Training ResNet-18's layer3 (csrc/resblock_train.hip: the vtd_resblock_train_* entries, the strided input gradient, 256-wide blocks),
without a device: the new C entry points exist and refuse bad arguments before any launch, the workspace query, the old entries' answers,
the stride-2 input gradient written out in fp64 as the kernels form it (zero insertion into the even positions, the stride-1 path on the
rotated, transposed weights, the downsample's transpose on the even positions) against torch autograd -- with negative controls that must
miss autograd by at least 10x the GPU tests' gradient bound -- and the bookkeeping of the mode "head+fpn+layer4+layer3"."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vtd_amd import _native, nets
from vtd_amd.nets import basic_block_train, forward_layer3_padded  # noqa: F401  (the feature under test: absent before it)

# no GPU gradient bound is above the project's ceiling for gradients (tests/test_gpu_layer3_train.py): a control that misses by 10x the
# ceiling misses by 10x every bound
GRAD_CEILING = 1e-2
GEOMETRIES = ((128, 256, 2), (256, 256, 1), (256, 512, 2), (512, 512, 1))
MODE = "head+fpn+layer4+layer3"


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _aligned(nbytes, align=256):
    raw = (C.c_char * (nbytes + 2 * align))()
    return raw, C.c_void_p((C.addressof(raw) + align - 1) // align * align)


# ---- C ABI, no device
def test_resblock_symbols_and_error_text():
    lib = _native.load()
    for name in ("vtd_resblock_train_workspace_bytes", "vtd_resblock_train_forward", "vtd_resblock_train_backward", "vtd_resblock_train_combine"):
        assert name in _native.SIGNATURES and hasattr(lib, name), name
    for code in (-3101, -3102):
        assert b"ResNet block training" in lib.vtd_strerror(code)
    assert b"geometry" in lib.vtd_strerror(-3101) and b"misaligned" in lib.vtd_strerror(-3102)
    # the old family's text is unchanged
    assert b"stride-2" in lib.vtd_strerror(-3003) and b"BasicBlock training" in lib.vtd_strerror(-3001)


def test_resblock_workspace_query():
    ws = _native.load().vtd_resblock_train_workspace_bytes
    for cin, width, stride in GEOMETRIES:
        for n, h, w in ((2, 6, 4), (2, 2, 2), (32, 40, 40)):
            for mode in (0, 1):
                b = ws(n, h, w, cin, width, stride, mode)
                assert b > 0 and b % 256 == 0, (n, h, w, cin, width, stride, mode)
        # the backward's scratch of a stride-2 block holds the zero-inserted plane of the input's size: more than the parameters alone
        assert ws(32, 40, 40, cin, width, stride, 1) > ws(2, 2, 2, cin, width, stride, 1)
    for cin, width in ((128, 256), (256, 512)):      # odd extents with stride 2
        for h, w in ((5, 4), (6, 3), (1, 1)):
            assert ws(2, h, w, cin, width, 2, 0) == -3101 and ws(2, h, w, cin, width, 2, 1) == -3101
    for bad in ((0, 6, 4, 128, 256, 2), (0, 6, 4, 512, 512, 1), (2, 6, 4, 64, 64, 1), (2, 6, 4, 512, 2048, 1), (2, 6, 4, 128, 256, 1), (2, 6, 4, 256, 256, 2),
                (2, 6, 4, 128, 512, 2), (2, 0, 4, 256, 256, 1), (2, 6, -1, 256, 256, 1)):
        assert ws(*bad, 0) == -3101, bad
    for mode in (2, -1):
        assert ws(2, 6, 4, 128, 256, 2, mode) == -3101


def test_resblock_argument_and_alignment_errors():
    lib = _native.load()
    keep = [_aligned(4096) for _ in range(3)]
    a, b, c = (k[1] for k in keep)
    st = _native.BasicBlockParams(*([a] * 15))
    sp = C.byref(st)
    fwd, bwd, comb = lib.vtd_resblock_train_forward, lib.vtd_resblock_train_backward, lib.vtd_resblock_train_combine
    # every refusal comes before any launch, so none of this needs a device
    for cin, width, stride in GEOMETRIES:
        g = (2, 6, 4, cin, width, stride)
        assert fwd(None, *g, sp, 1e-5, b, c, None) == -3101
        assert fwd(a, *g, None, 1e-5, b, c, None) == -3101
        assert fwd(a, *g, sp, 1e-5, None, c, None) == -3101
        assert fwd(a, *g, sp, 1e-5, b, None, None) == -3101
        assert fwd(a, *g, sp, 0.0, b, c, None) == -3101
        assert fwd(a, *g, sp, 1e-5, C.c_void_p(b.value + 128), c, None) == -3102
        assert fwd(C.c_void_p(a.value + 8), *g, sp, 1e-5, b, c, None) == -3102
        assert bwd(a, *g, sp, 1e-5, b, c, None, a, sp, b, None, None, None) == -3101          # no dy
        assert bwd(a, *g, sp, 1e-5, b, c, a, None, sp, b, None, None, None) == -3101          # no dscale
        assert bwd(a, *g, sp, 1e-5, b, c, a, a, None, b, None, None, None) == -3101           # no place for the gradients
        assert bwd(a, *g, sp, 1e-5, b, c, a, a, sp, None, None, None, None) == -3101          # no scratch
        assert bwd(a, *g, sp, 1e-5, b, c, a, a, sp, b, c, None, None) == -3101                # dx without a place for its scale
        assert bwd(a, *g, sp, 1e-5, b, c, a, C.c_void_p(a.value + 4), sp, b, None, None, None) == -3102
        assert bwd(a, *g, sp, 1e-5, b, c, a, a, sp, C.c_void_p(b.value + 128), None, None, None) == -3102
        assert bwd(a, *g, sp, 1e-5, b, c, a, a, sp, b, C.c_void_p(c.value + 8), a, None) == -3102     # a misaligned dx, either stride
        assert bwd(a, *g, sp, 1e-5, b, c, a, a, sp, b, c, C.c_void_p(a.value + 4), None) == -3102
    nods = _native.BasicBlockParams(*([a] * 10))
    for cin, width in ((128, 256), (256, 512)):      # a stride-2 block needs its downsample
        assert fwd(a, 2, 6, 4, cin, width, 2, C.byref(nods), 1e-5, b, c, None) == -3101
        assert bwd(a, 2, 6, 4, cin, width, 2, C.byref(nods), 1e-5, b, c, a, a, sp, b, c, a, None) == -3101
    assert fwd(a, 2, 6, 4, 256, 256, 1, C.byref(nods), 1e-5, C.c_void_p(b.value + 128), c, None) == -3102      # stride 1 ignores ds_*
    assert fwd(a, 2, 5, 4, 128, 256, 2, sp, 1e-5, b, c, None) == -3101
    assert fwd(a, 2, 6, 4, 64, 64, 1, sp, 1e-5, b, c, None) == -3101
    # the combine
    assert comb(None, a, b, b, 64, c, None) == -3101 and comb(a, None, b, b, 64, c, None) == -3101 and comb(a, a, None, b, 64, c, None) == -3101
    assert comb(a, a, b, None, 64, c, None) == -3101 and comb(a, a, b, b, 64, None, None) == -3101
    assert comb(a, a, b, b, 0, c, None) == -3101 and comb(a, a, b, b, 6, c, None) == -3101 and comb(a, a, b, b, 64, a, None) == -3101
    assert comb(C.c_void_p(a.value + 4), a, b, b, 64, c, None) == -3102 and comb(a, a, b, b, 64, C.c_void_p(c.value + 4), None) == -3102


def test_old_basicblock_entries_answer_as_before():
    lib = _native.load()
    ws = lib.vtd_basicblock_train_workspace_bytes
    for geom in ((2, 6, 4, 256, 512, 2), (2, 3, 2, 512, 512, 1), (32, 40, 40, 256, 512, 2), (32, 20, 20, 512, 512, 1)):
        assert ws(*geom, 0) > 0 and ws(*geom, 1) > 0 and ws(*geom, 0) % 256 == 0
    for bad in ((2, 6, 4, 128, 256, 2), (2, 6, 4, 256, 256, 1), (2, 6, 4, 256, 512, 1), (2, 6, 4, 512, 512, 2), (2, 5, 4, 256, 512, 2), (2, 6, 3, 256, 512, 2),
                (0, 6, 4, 256, 512, 2), (2, 0, 4, 512, 512, 1), (2, 3, 2, 512, 2048, 1), (2, 3, 2, 64, 64, 1)):
        assert ws(*bad, 0) == -3001, bad
    assert ws(2, 3, 2, 512, 512, 1, 2) == -3001
    # layer4's stride-2 scratch: the old entry has no strided dgrad and no room for one; the new entry's is larger by its plane and panel
    new = lib.vtd_resblock_train_workspace_bytes
    assert new(2, 6, 4, 256, 512, 2, 1) > ws(2, 6, 4, 256, 512, 2, 1) and new(2, 3, 2, 512, 512, 1, 1) == ws(2, 3, 2, 512, 512, 1, 1)
    assert new(2, 6, 4, 256, 512, 2, 0) == ws(2, 6, 4, 256, 512, 2, 0)
    keep = [_aligned(4096) for _ in range(3)]
    a, b, c = (k[1] for k in keep)
    st = _native.BasicBlockParams(*([a] * 15))
    sp = C.byref(st)
    fwd, bwd = lib.vtd_basicblock_train_forward, lib.vtd_basicblock_train_backward
    assert fwd(None, 2, 3, 2, 512, 512, 1, sp, 1e-5, b, c, None) == -3001
    assert fwd(a, 2, 3, 2, 128, 128, 1, sp, 1e-5, b, c, None) == -3001
    assert fwd(a, 2, 6, 4, 128, 256, 2, sp, 1e-5, b, c, None) == -3001 and fwd(a, 2, 3, 2, 256, 256, 1, sp, 1e-5, b, c, None) == -3001
    assert fwd(a, 2, 3, 2, 512, 512, 1, sp, 1e-5, C.c_void_p(b.value + 128), c, None) == -3002
    assert bwd(a, 2, 6, 4, 256, 512, 2, sp, 1e-5, b, c, a, a, sp, b, c, a, None) == -3003   # still no input gradient for the stride-2 block here
    assert bwd(a, 2, 3, 2, 512, 512, 1, sp, 1e-5, b, c, a, a, sp, b, c, None, None) == -3001
    assert bwd(a, 2, 3, 2, 512, 512, 1, sp, 1e-5, b, c, a, C.c_void_p(a.value + 4), sp, b, None, None, None) == -3002
    assert bwd(a, 2, 3, 2, 512, 512, 1, sp, 1e-5, b, c, None, a, sp, b, None, None, None) == -3001


def test_python_refusals_old_and_new():
    with pytest.raises(ValueError, match="CUDA"):
        nets.basic_block_train(nets.BasicBlock(128, 256, 2), torch.zeros((1, 128, 2, 2)))
    with pytest.raises(ValueError, match="must be a"):
        nets.basic_block_train(nets.BasicBlock(256, 256, 1), torch.zeros((1, 128, 2, 2)))
    with pytest.raises(RuntimeError, match="Bottleneck"):
        nets.basic_block_train(nets.Bottleneck(256, 64, 1), torch.zeros((1, 256, 2, 2)))
    with pytest.raises(RuntimeError, match="layer3 and layer4"):
        nets.BasicBlock(64, 64, 1)._train_operands(torch.device("cpu"), general=True)
    # BasicBlock.__call__ keeps its refusal
    with pytest.raises(RuntimeError, match="layer4 only"):
        nets.BasicBlock(128, 256, 2)._train_operands(torch.device("cpu"))
    with pytest.raises(RuntimeError, match="Bottleneck training is not built"):
        nets._stage_operands(nets._STAGES[2], nets.make_trunk("resnet50")[6], torch.zeros((1, 6, 6, 128)))
    with pytest.raises(RuntimeError, match="Bottleneck training is not built"):
        nets.forward_layer3_padded(nets.make_trunk("resnet50")[6], torch.zeros((1, 6, 6, 128)))
    with pytest.raises(ValueError, match="needs layer4 and the DBHead"):
        nets.FeaturePyramidNetwork(512).forward_padded([None, None], layer3=nets.make_trunk("resnet18")[6])


# ---- the strided input gradient as the kernels form it, against autograd.  6 -> 5 channels: a wrong phase, tap or rotation misses by the
# same relative amount at any width
def _strided_case(h, w, seed=9):
    gen = torch.Generator().manual_seed(seed + 10 * h + w)
    cin, cout = 6, 5
    x = torch.randn((2, cin, 2 * h, 2 * w), generator=gen).double().requires_grad_(True)
    w1 = torch.randn((cout, cin, 3, 3), generator=gen).double() * 0.3
    wd = torch.randn((cout, cin, 1, 1), generator=gen).double() * 0.3
    g1 = torch.randn((2, cout, h, w), generator=gen).double()
    g2 = torch.randn((2, cout, h, w), generator=gen).double()
    return x, w1, wd, g1, g2


def _conv1_transpose(g1, w1, bug=None):
    """conv1^T(g1) for a 3x3 stride-2 pad-1 convolution at 2h x 2w: g1 at the even positions of a zeroed ring-padded plane, then the stride-1
    window over it with the weights rotated by 180 degrees and transposed.  Row 2h - 1 reads the ring where o = h would be."""
    n, co, h, w = g1.shape
    z = torch.zeros((n, co, 2 * h + 2, 2 * w + 2), dtype=g1.dtype)       # ring of one pixel
    if bug == "phases_swapped":
        z[:, :, 2:2 * h + 2:2, 2:2 * w + 2:2] = g1                           # odd interior positions
    else:
        z[:, :, 1:2 * h + 1:2, 1:2 * w + 1:2] = g1                           # interior (2o, 2p) = padded (2o + 1, 2p + 1)
    if bug == "out_of_range_tap_kept":                                       # o = h and p = w read the last row / column again
        z[:, :, 2 * h + 1, :] = z[:, :, 2 * h - 1, :]
        z[:, :, :, 2 * w + 1] = z[:, :, :, 2 * w - 1]
    wt = w1.transpose(0, 1)
    if bug != "unrotated_weights":
        wt = wt.flip(-1, -2)
    return F.conv2d(z, wt)


def _downsample_transpose(dx, g2, wd, bug=None):
    t = torch.einsum("nohw,oc->nchw", g2, wd[:, :, 0, 0])
    out = dx.clone()
    if bug == "downsample_on_odd_positions":
        out[:, :, 1::2, 1::2] += t
    else:
        out[:, :, 0::2, 0::2] += t
    return out


SIZES = [(1, 1), (3, 2), (5, 4)]


@pytest.mark.parametrize("size", SIZES)
def test_strided_dgrad_3x3_matches_autograd(size):
    x, w1, wd, g1, g2 = _strided_case(*size)
    F.conv2d(x, w1, None, 2, 1).backward(g1)
    got = _conv1_transpose(g1, w1)
    assert got.shape == x.shape and _rel(got.numpy(), x.grad.numpy()) <= 1e-12
    # even rows take the centre tap only, odd rows the two outer taps: row 0 never sees w1[:, :, 0] or w1[:, :, 2]
    centre, outer = w1.clone(), w1.clone()
    centre[:, :, 0::2, :] = 0
    outer[:, :, 1, :] = 0
    assert _rel(_conv1_transpose(g1, centre)[:, :, 0::2].numpy(), got[:, :, 0::2].numpy()) <= 1e-12
    assert _rel(_conv1_transpose(g1, outer)[:, :, 1::2].numpy(), got[:, :, 1::2].numpy()) <= 1e-12


@pytest.mark.parametrize("size", SIZES)
def test_strided_dgrad_1x1_path_matches_autograd(size):
    x, w1, wd, g1, g2 = _strided_case(*size)
    F.conv2d(x, wd, None, 2, 0).backward(g2)
    got = _downsample_transpose(torch.zeros_like(x.detach()), g2, wd)
    assert _rel(got.numpy(), x.grad.numpy()) <= 1e-12
    assert float(got[:, :, 1::2].abs().max()) == 0 and float(got[:, :, :, 1::2].abs().max()) == 0      # even (row, column) positions only


@pytest.mark.parametrize("size", SIZES)
def test_strided_dgrad_of_the_block_matches_autograd(size):
    x, w1, wd, g1, g2 = _strided_case(*size)
    torch.autograd.backward([F.conv2d(x, w1, None, 2, 1), F.conv2d(x, wd, None, 2, 0)], [g1, g2])
    got = _downsample_transpose(_conv1_transpose(g1, w1), g2, wd)
    assert _rel(got.numpy(), x.grad.numpy()) <= 1e-12


@pytest.mark.parametrize("bug", ["phases_swapped", "out_of_range_tap_kept", "downsample_on_odd_positions", "unrotated_weights"])
@pytest.mark.parametrize("size", SIZES)
def test_strided_dgrad_negative_controls(bug, size):
    x, w1, wd, g1, g2 = _strided_case(*size)
    torch.autograd.backward([F.conv2d(x, w1, None, 2, 1), F.conv2d(x, wd, None, 2, 0)], [g1, g2])
    got = _downsample_transpose(_conv1_transpose(g1, w1, bug), g2, wd, bug)
    err = _rel(got.numpy(), x.grad.numpy())
    assert err >= 10 * GRAD_CEILING, f"{bug} at {size}: error {err:.3g} is not 10x the bound {GRAD_CEILING}"


@pytest.mark.parametrize("bug", [None, "fpn_dc4_left_out"])
@pytest.mark.parametrize("size", SIZES)
def test_dc4_is_the_sum_of_both_consumers(bug, size):
    """C4 feeds layer4.0 (3x3 stride 2 and the 1x1 stride-2 downsample) and the FPN's lateral: dC4 is the sum of the three transposes."""
    x, w1, wd, g1, g2 = _strided_case(*size)
    gen = torch.Generator().manual_seed(77)
    lat = torch.randn((4, 6, 1, 1), generator=gen).double() * 0.3
    gl = torch.randn((2, 4, x.shape[2], x.shape[3]), generator=gen).double()
    torch.autograd.backward([F.conv2d(x, w1, None, 2, 1), F.conv2d(x, wd, None, 2, 0), F.conv2d(x, lat)], [g1, g2, gl])
    got = _downsample_transpose(_conv1_transpose(g1, w1), g2, wd)
    if bug is None:
        got = got + torch.einsum("nohw,oc->nchw", gl, lat[:, :, 0, 0])
    err = _rel(got.numpy(), x.grad.numpy())
    assert err <= 1e-12 if bug is None else err >= 10 * GRAD_CEILING, f"{bug}: {err:.3g}"


# ---- the product mode
def test_head_fpn_layer4_layer3_mode():
    net = nets.DBNet("resnet18", trainable=MODE)
    assert net.trainable == MODE
    for i in range(6):
        assert not any(p.requires_grad for p in net.backbone[i].parameters()), i
    for m in (net.backbone[6], net.backbone[7], net.fpn, net.head):
        assert all(p.requires_grad for p in m.parameters())
    assert len(list(net.backbone[6].parameters())) == 15 and len(list(net.backbone[6].buffers())) == 15
    # the eval-mode rebuild is keyed on layer3's tensors too (15 parameters, 5 BatchNorms x 3 buffers)
    l4 = nets.DBNet("resnet18", trainable="head+fpn+layer4")
    assert len(net._head_tensor_versions()) == len(l4._head_tensor_versions()) + 30
    assert len(l4._head_tensor_versions()) == len(nets.DBNet("resnet18", trainable="head+fpn")._head_tensor_versions()) + 30
    # the state dict is the reference's, whatever the mode
    assert list(net.state_dict()) == list(nets.DBNet("resnet18").state_dict())
    assert MODE in nets.DBNet.set_trainable.__doc__


def test_mode_refusals():
    with pytest.raises(ValueError, match="Bottleneck"):
        nets.DBNet("resnet50", trainable=MODE)
    with pytest.raises(ValueError, match="Bottleneck"):
        nets.DBNet("resnet50").set_trainable(MODE)
    # the names that were refused stay refused
    for mode in ("layer4", "head+layer4", "head+fpn+layer3", "all", "layer3", "head+fpn+layer3+layer4"):
        with pytest.raises(ValueError, match="trainable"):
            nets.DBNet("resnet18", trainable=mode)
    # a frozen trunk tensor that requires grad is refused in a train-mode forward, before anything touches a device
    net = nets.DBNet("resnet18", trainable=MODE)
    net.backbone[5][1].conv2.weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match="backward below layer3"):
        net.train()(torch.zeros((1, 3, 640, 640)))
    # the layer4 mode's own refusal names layer4, as before
    net4 = nets.DBNet("resnet18", trainable="head+fpn+layer4")
    net4.backbone[6][0].conv1.weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match="backward below layer4 is not"):
        net4.train()(torch.zeros((1, 3, 640, 640)))


def test_switching_between_modes():
    grads = lambda net, i: [p.requires_grad for p in net.backbone[i].parameters()]  # noqa: E731
    net = nets.DBNet("resnet18", trainable="head+fpn+layer4")
    assert not any(grads(net, 6)) and all(grads(net, 7))
    net.set_trainable(MODE)
    assert all(grads(net, 6)) and all(grads(net, 7)) and not any(grads(net, 5))
    net.set_trainable("head+fpn+layer4")      # and back: layer3 is frozen again
    assert not any(grads(net, 6)) and all(grads(net, 7))
    net.set_trainable(MODE).set_trainable("head+fpn")
    assert not any(p.requires_grad for p in net.backbone.parameters()) and all(p.requires_grad for p in net.fpn.parameters())
    net.set_trainable("head")
    assert not any(p.requires_grad for p in net.fpn.parameters())
    net.set_trainable(MODE)
    for m in (net.backbone[6], net.backbone[7], net.fpn, net.head):
        assert all(p.requires_grad for p in m.parameters())
    assert not any(p.requires_grad for i in range(6) for p in net.backbone[i].parameters())
