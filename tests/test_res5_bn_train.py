"""Train-mode (batch-statistics) BatchNorm for ResNet-50's res5 and res4 (csrc/bottleneck_bn_train.hip, the vtd_bottleneck_bn_train_*
entries), without a device: the header, the exports and the binding table agree on the three new symbols; the entries refuse bad
arguments before any launch (-4001 / -4002) and the workspace query equals its documented formula and covers the frozen families'; the
Python surface -- `nets.bottleneck_bn_train`, `forward_padded(..., res_batch_stats=)` and `DBNet(..., trunk_bn="bottleneck")` -- accepts what
is built and refuses everything else before a device is looked at, leaving the network as it was; and the older refusals on the five
ResNet-50 modes stand.  tests/test_gpu_res5_bn_train.py checks the kernels themselves."""
import ctypes as C
import os
import re

import pytest
import torch

from vtd_amd import _native, nets

ENTRIES = ("vtd_bottleneck_bn_train_workspace_bytes", "vtd_bottleneck_bn_train_forward", "vtd_bottleneck_bn_train_backward")
GEOMS = [(1024, 512, 2), (2048, 512, 1), (512, 256, 2), (1024, 256, 1)]
RES_MODES = ("head+fpn+res5", "head+fpn+res5+res4", "head+fpn+res5+res4+res3", "head+fpn+res5+res4+res3+res2", "head+fpn+res5+res4+res3+res2+stem")
BN_MODES = RES_MODES[:2]
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "vtd.h")


def _aligned(nbytes, align=256):
    raw = (C.c_char * (nbytes + 2 * align))()
    return raw, C.c_void_p((C.addressof(raw) + align - 1) // align * align)


def _struct(buf, fields=_native.BOTTLENECK_FIELDS):
    st = _native.BottleneckParams()
    for f in fields:
        setattr(st, f, buf)
    return st


LEARN_FIELDS = [f for f in _native.BOTTLENECK_FIELDS if not f.endswith(("_mean", "_var"))]


# ---- C ABI, no device
def test_header_exports_and_bindings_agree():
    lib = _native.load()
    text = open(HEADER).read()
    for name in ENTRIES:
        assert name in _native.SIGNATURES and hasattr(lib, name), name
        assert len(re.findall(r"^int(?:64_t)? " + name + r"\(", text, re.M)) == 1, name      # declared once
        # the signatures are vtd_trunk_bn_train_*'s with the Bottleneck struct
        res, args = _native.SIGNATURES[name]
        tres, targs = _native.SIGNATURES[name.replace("bottleneck_bn", "trunk_bn")]
        assert res == tres and len(args) == len(targs)
        for a, b in zip(args, targs):
            assert a == b or (a == C.POINTER(_native.BottleneckParams) and b == C.POINTER(_native.BasicBlockParams)), name
    for code in (-4001, -4002):
        msg = lib.vtd_strerror(code)
        assert b"Bottleneck batch-statistics training" in msg and b"validation error" not in msg
    assert b"misaligned" in lib.vtd_strerror(-4002)
    assert "-4001" in text and "-4002" in text


def _workspace_formula(n, hin, win, cin, W, stride, mode):
    """include/vtd.h, vtd_bottleneck_bn_train_workspace_bytes: the family's own sum (the query answers the larger of it and the frozen one)."""
    a256 = lambda b: (b + 255) // 256 * 256  # noqa: E731
    S = lambda r: min(8, max(1, -(-r // 4096)))  # noqa: E731
    h, w, ds = hin // stride, win // stride, int(stride == 2)
    pin, pout, M, Min = n * (hin + 2) * (win + 2), n * (h + 2) * (w + 2), n * h * w, n * hin * win
    if mode == 0:
        return (a256(2 * pin * W) + a256(2 * pout * W) + ds * a256(8 * pout * W) + a256(4 * Min * W) + a256(4 * M * W) + (1 + ds) * a256(16 * M * W) +
                a256(2 * W * cin) + a256(18 * W * W) + a256(8 * W * W) + ds * a256(8 * W * cin) + a256(16 * W) + a256(256 * 96 * W) + 2 * a256(16 * W) +
                (1 + ds) * a256(64 * W) + a256(8 * W))
    return (a256(16 * M * W) + a256(4 * M * W) + a256(4 * Min * W) + a256(2 * max(4 * M * W, Min * W)) + a256(8 * pout * W) + 2 * a256(2 * pin * W) +
            a256(18 * W * W) + a256(16 * W) + a256(256 * 64 * W) + a256(256 * 32 * W) + a256(48 * W) + a256(64) +
            a256(4 * max(S(M) * 9 * W * W, S(Min) * W * cin)))


def test_workspace_query():
    lib = _native.load()
    ws = lib.vtd_bottleneck_bn_train_workspace_bytes
    frozen = {512: lib.vtd_bottleneck_train_workspace_bytes, 256: lib.vtd_bottleneck256_train_workspace_bytes}
    for n, h, w in ((1, 2, 2), (2, 6, 4), (2, 24, 22), (32, 40, 40)):
        for cin, width, stride in GEOMS:
            for mode in (0, 1):
                got, old = ws(n, h, w, cin, width, stride, mode), frozen[width](n, h, w, cin, width, stride, mode)
                assert old > 0 and got >= old and got % 256 == 0      # either value of `training` runs in one allocation
                assert got == max(old, _workspace_formula(n, h, w, cin, width, stride, mode)), (n, h, w, cin, width, stride, mode)
    # the figures include/vtd.h gives at n = 32: a 40 x 40 res5 input and an 80 x 80 res4 input, workspace and scratch
    text = open(HEADER).read()
    for g in ((32, 40, 40, 1024, 512, 2), (32, 80, 80, 512, 256, 2)):
        for mode in (0, 1):
            assert f"{ws(*g, mode)} bytes" in text, (g, mode)
    bad = [(2, 6, 4, 256, 128, 2), (2, 6, 4, 512, 128, 1),      # width 128: res3 is not built
           (2, 6, 4, 64, 64, 1), (2, 6, 4, 256, 64, 1),      # width 64: res2 is not built
           (2, 5, 4, 1024, 512, 2), (2, 6, 3, 512, 256, 2),      # an odd extent at stride 2
           (2, 6, 4, 1024, 512, 1), (2, 6, 4, 2048, 512, 2), (2, 6, 4, 512, 256, 1), (2, 6, 4, 1024, 1024, 1),      # no such block
           (0, 6, 4, 1024, 512, 2), (2, 0, 4, 2048, 512, 1), (1 << 16, 6, 4, 1024, 512, 2), (2, 4098, 4, 512, 256, 2)]
    for g in bad:
        assert ws(*g, 0) == -4001 and ws(*g, 1) == -4001, g
    for mode in (2, -1):      # a mode outside {0, 1}
        assert ws(2, 6, 4, 1024, 512, 2, mode) == -4001


@pytest.mark.parametrize("cin,width,stride", GEOMS)
def test_forward_refusals_come_before_any_launch(cin, width, stride):
    fwd = _native.load().vtd_bottleneck_bn_train_forward
    keep = [_aligned(4096) for _ in range(5)]
    x, ws, y, w, stats = (k[1] for k in keep)
    st = _struct(w)
    good = [x, 2, 6, 4, cin, width, stride, C.byref(st), 1, 0.1, 1e-5, ws, y, stats, None]
    for i in (0, 7, 11, 12):      # x, params, workspace, y: a null pointer
        a = list(good)
        a[i] = None
        assert fwd(*a) == -4001, i
    for i, v in ((8, 2), (8, -1), (9, 1.5), (9, -0.1), (10, 0.0), (1, 0), (4, 128), (5, 128), (5, 64), (6, 3 - stride)):
        a = list(good)      # training outside {0, 1}, momentum outside [0, 1], eps, geometry
        a[i] = v
        assert fwd(*a) == -4001, (i, v)
    for training in (0, 1):
        st2 = _struct(w)
        st2.bn3_var = None
        a = list(good)
        a[7], a[8] = C.byref(st2), training
        assert fwd(*a) == -4001
    # training = 1 with n h w = 1: no variance of one row
    one = [x, 1, stride, stride, cin, width, stride, C.byref(st), 1, 0.1, 1e-5, ws, y, None, None]
    assert fwd(*one) == -4001
    for i, off in ((0, 8), (12, 8), (11, 128), (13, 2)):      # a misaligned tap, output, workspace, statistics
        a = list(good)
        a[i] = C.c_void_p(a[i].value + off)
        assert fwd(*a) == -4002, i
    st3 = _struct(w)
    st3.conv3_w = C.c_void_p(w.value + 2)
    a = list(good)
    a[7] = C.byref(st3)
    assert fwd(*a) == -4002


@pytest.mark.parametrize("cin,width,stride", GEOMS)
def test_backward_refusals_come_before_any_launch(cin, width, stride):
    bwd = _native.load().vtd_bottleneck_bn_train_backward
    keep = [_aligned(4096) for _ in range(9)]
    x, ws, y, dy, dscale, scratch, dx, dxscale, w = (k[1] for k in keep)
    st, gst = _struct(w), _struct(w, LEARN_FIELDS)
    good = [x, 2, 6, 4, cin, width, stride, C.byref(st), 1, 1e-5, ws, y, dy, dscale, C.byref(gst), scratch, dx, dxscale, None]
    for i in (0, 7, 10, 11, 12, 13, 14, 15, 17):      # every pointer but dx, which is optional; dx without its scale is refused
        a = list(good)
        a[i] = None
        assert bwd(*a) == -4001, i
    for i, v in ((8, 2), (9, 0.0), (5, 128), (6, 3 - stride)):
        a = list(good)
        a[i] = v
        assert bwd(*a) == -4001, (i, v)
    one = list(good)
    one[1:4] = [1, stride, stride]
    assert bwd(*one) == -4001
    for i, off in ((0, 8), (11, 8), (12, 8), (16, 8), (10, 128), (15, 128), (13, 4), (17, 4)):
        a = list(good)
        a[i] = C.c_void_p(a[i].value + off)
        assert bwd(*a) == -4002, i


# ---- the Python surface
def _blocks():
    return {g: nets.Bottleneck(*g) for g in GEOMS}


def test_bottleneck_bn_train_refusals():
    blocks = _blocks()
    for other in (nets.Bottleneck(256, 128, 2), nets.Bottleneck(512, 128, 1), nets.Bottleneck(64, 64, 1), nets.Bottleneck(256, 64, 1),
                  nets.Bottleneck(512, 512, 1), nets.BasicBlock(256, 512, 2)):
        with pytest.raises(RuntimeError, match="res5 and res4"):
            nets.bottleneck_bn_train(other, torch.zeros((2, 256, 2, 2)))
    for (cin, width, stride), blk in blocks.items():
        with pytest.raises(ValueError, match=rf"\[n,{cin},H,W\]"):
            nets.bottleneck_bn_train(blk, torch.zeros((2, cin + 8, 4, 4)))
        with pytest.raises(ValueError, match="CUDA"):      # everything built passes the checks that need no device, then the device is asked for
            nets.bottleneck_bn_train(blk, torch.zeros((2, cin, 4, 4)))
        if stride == 2:
            with pytest.raises(RuntimeError, match="even extents"):
                nets.bottleneck_bn_train(blk, torch.zeros((2, cin, 3, 4)))
        with pytest.raises(ValueError, match="more than one value"):
            nets.bottleneck_bn_train(blk.train(), torch.zeros((1, cin, stride, stride)))
    blk = nets.Bottleneck(2048, 512, 1)
    blk.bn2.momentum = None
    with pytest.raises(ValueError, match="momentum=None"):
        nets.bottleneck_bn_train(blk, torch.zeros((2, 2048, 2, 2)))
    blk.bn2.momentum = 0.2
    with pytest.raises(ValueError, match="one fixed momentum"):
        nets.bottleneck_bn_train(blk, torch.zeros((2, 2048, 2, 2)))
    blk.bn2.momentum, blk.bn3.eps = 0.1, 1e-3
    with pytest.raises(ValueError, match="one eps"):
        nets.bottleneck_bn_train(blk, torch.zeros((2, 2048, 2, 2)))
    assert nets._BOTTLENECK_BN == "vtd_bottleneck_bn_train" and nets._BOTTLENECK_BN in nets._BN_FAMILIES


def _grad_pattern(net):
    return tuple(p.requires_grad for p in net.parameters())


def test_bottleneck_is_accepted_on_the_two_modes():
    for mode, first in zip(BN_MODES, (7, 6)):
        net = nets.DBNet("resnet50", trainable=mode, trunk_bn="bottleneck")
        assert net.trainable == mode and net.trunk_bn == "bottleneck"
        assert _grad_pattern(net) == _grad_pattern(nets.DBNet("resnet50", trainable=mode))      # what trains does not depend on trunk_bn
        for i in range(8):
            assert all(p.requires_grad == (i >= first) for p in net.backbone[i].parameters()), i
        assert all(p.requires_grad for p in list(net.fpn.parameters()) + list(net.head.parameters()))
    net = nets.DBNet("resnet50", trainable=BN_MODES[0])
    assert net.trunk_bn == "frozen"
    assert net.set_trainable(BN_MODES[1], "bottleneck").trunk_bn == "bottleneck"
    assert net.set_trainable(BN_MODES[0]).trunk_bn == "bottleneck" and net.trainable == BN_MODES[0]      # None keeps the spelling
    assert net.set_trainable(BN_MODES[0], "frozen").trunk_bn == "frozen"
    bns = [m for i in (6, 7) for m in net.backbone[i].modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(bns) == 29 and len([m for m in net.backbone[7].modules() if isinstance(m, torch.nn.BatchNorm2d)]) == 10


def test_bottleneck_is_refused_everywhere_else():
    for mode in ("head+fpn+layer4", "head+fpn+layer4+layer3", "head+fpn+backbone", None, "head", "head+fpn"):
        with pytest.raises(ValueError, match="res5 and res4"):
            nets.DBNet("resnet18", trainable=mode, trunk_bn="bottleneck")
    for mode in RES_MODES[2:] + (None, "head", "head+fpn"):
        with pytest.raises(ValueError, match="res3, res2 and the stem keep frozen statistics"):
            nets.DBNet("resnet50", trainable=mode, trunk_bn="bottleneck")
    # a refusal leaves the network as it was
    net = nets.DBNet("resnet50", trainable=BN_MODES[1], trunk_bn="bottleneck")
    pattern = _grad_pattern(net)
    for mode in RES_MODES[2:] + (None, "head", "head+fpn"):
        with pytest.raises(ValueError, match="trunk_bn='bottleneck'"):
            net.set_trainable(mode)      # the kept "bottleneck" does not fit the new mode
        assert net.trainable == BN_MODES[1] and net.trunk_bn == "bottleneck" and _grad_pattern(net) == pattern
    r18 = nets.DBNet("resnet18", trainable="head+fpn+layer4", trunk_bn="batch")
    with pytest.raises(ValueError, match="trunk_bn='bottleneck'"):
        r18.set_trainable("head+fpn+layer4", "bottleneck")
    assert r18.trainable == "head+fpn+layer4" and r18.trunk_bn == "batch"


def test_the_old_refusals_stand_on_all_five_modes():
    for mode in RES_MODES:
        for bn in ("batch", "trained", "backbone", ("res5",), ("res5", "res4"), ("res4", "res5"), ("layer4",), "bogus", 3):
            with pytest.raises(ValueError):
                nets.DBNet("resnet50", trainable=mode, trunk_bn=bn)
        net = nets.DBNet("resnet50", trainable=mode)
        for bn in ("batch", "trained", "backbone"):
            with pytest.raises(ValueError, match="frozen-statistics"):
                net.set_trainable(mode, trunk_bn=bn)
        assert net.trainable == mode and net.trunk_bn == "frozen"


def _res(width, n):
    cin = {512: 1024, 256: 512, 128: 256}[width]
    return torch.nn.Sequential(nets.Bottleneck(cin, width, 2), *(nets.Bottleneck(4 * width, width, 1) for _ in range(n - 1)))


def test_forward_padded_res_batch_stats_refusals():
    """On shapes alone: the taps are CPU tensors, and every refusal of the keyword comes before a device is looked at."""
    fpn, head = nets.FeaturePyramidNetwork(2048), nets.DBHead(256)
    res5, res4, res3 = _res(512, 3), _res(256, 6), _res(128, 4)
    r18 = nets.make_trunk("resnet18")
    taps = [torch.zeros((2, 26, 18, 256), dtype=torch.float16), torch.zeros((2, 14, 10, 512), dtype=torch.float16),
            torch.zeros((2, 8, 6, 1024), dtype=torch.float16)]
    kw = dict(head=head, res5=res5, res_batch_stats=True)
    for extra in (dict(res4=res4, res3=res3), dict(res4=res4, res3=res3, res2=_res(128, 3)), dict(stem=(r18[0], r18[1])), dict(layer4=r18[7]),
                  dict(layer3=r18[6]), dict(trunk_batch_stats=True), dict(trunk_batch_stats=("layer4",)), dict(stem_batch_stats=True), dict(head=None),
                  dict(res5=None), dict(res5=None, res4=res4)):
        with pytest.raises(ValueError, match="res_batch_stats"):
            fpn.forward_padded(taps, **{**kw, **extra})
    for bad in (("res4", "res5"), ("res4",), ("res5", "res4"), ("layer4",), "res5", 1.5):      # not the stages given
        with pytest.raises(ValueError, match="exactly the res stages given"):
            fpn.forward_padded(taps, **{**kw, "res_batch_stats": bad})
    with pytest.raises(ValueError, match="exactly the res stages given"):
        fpn.forward_padded(taps[:2], head=head, res5=res5, res4=res4, res_batch_stats=("res5",))
    # what is spelled right gets as far as the taps' device, in either spelling and at either depth
    for t, k in ((taps, dict(res_batch_stats=True)), (taps, dict(res_batch_stats=("res5",))), (taps[:2], dict(res4=res4, res_batch_stats=True)),
                 (taps[:2], dict(res4=res4, res_batch_stats=["res4", "res5"]))):
        with pytest.raises(ValueError, match="padded taps must be contiguous float16 CUDA tensors"):
            fpn.forward_padded(t, head=head, res5=res5, **k)
    # trunk_batch_stats and stem_batch_stats stay refused with res arguments, as before the keyword
    for k in (dict(trunk_batch_stats=True), dict(stem_batch_stats=True)):
        with pytest.raises(ValueError, match="frozen-statistics BatchNorm"):
            fpn.forward_padded(taps, head=head, res5=res5, **k)
        with pytest.raises(ValueError, match="frozen-statistics BatchNorm"):
            fpn.forward_padded(taps[:2], head=head, res5=res5, res4=res4, **k)
