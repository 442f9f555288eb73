"""Train-mode (batch-statistics) BatchNorm for ResNet-18's layer1 (csrc/resblock_bn_train.hip at width 64, the seventh geometry of the
vtd_trunk_bn_train_* entries), without a device: the workspace query and the refusals before any launch for (64, 64, 1), the fixed
sixteen-part order of the 64-wide per-channel reductions written out in numpy -- with a control that pairs the parts linearly and must differ
in a bit --, the refusals and acceptances of the new Python spellings (`trunk_block_bn_train` on the 64-wide block, the four-stage tuple of
`forward_padded`, `DBNet(trainable="head+fpn+layer4+layer3+layer2+layer1", trunk_bn="trained")`), and the call schedule of the layer1 ->
layer2 -> layer3 -> layer4 -> FPN -> head node with batch statistics."""
import ctypes as C
import pathlib

import numpy as np
import pytest
import torch

import test_layer2_bn_train as l2c
import test_trunk_train_schedule as sched
from vtd_amd import _native, nets

GEOM = (64, 64, 1)
STAGES = ("layer1", "layer2", "layer3", "layer4")
MODE4 = "head+fpn+layer4+layer3+layer2+layer1"
MODE3 = "head+fpn+layer4+layer3+layer2"
STEM_FROZEN = r"stem keeps? frozen statistics"
_aligned = l2c._aligned


# ---- C ABI, no device
def test_header_names_the_seventh_geometry():
    lib = _native.load()
    header = (pathlib.Path(__file__).resolve().parents[1] / "include" / "vtd.h").read_text()
    assert "cin 64, width 64, stride 1" in header and "sixteen parts" in header and "vtd_block64_train_forward / _backward" in header
    assert b"batch-statistics" in lib.vtd_strerror(-3701)


def test_workspace_query():
    lib = _native.load()
    ws, frozen = lib.vtd_trunk_bn_train_workspace_bytes, lib.vtd_block64_train_workspace_bytes
    for h, w in ((3, 2), (12, 11), (23, 23)):
        geom = (2, h, w, *GEOM)
        for mode in (0, 1):
            assert ws(*geom, mode) > 0 and ws(*geom, mode) % 256 == 0, (geom, mode)
            assert frozen(*geom, mode) > 0 and ws(*geom, mode) >= frozen(*geom, mode)      # training = 0 runs the frozen path in the same allocation
    # the backward's scratch holds the slabs of the 64-wide rule: min(ceil(512 / 5), ceil(rows / 1024)) slabs of [64][576] floats
    assert ws(2, 23, 23, *GEOM, 1) - ws(2, 3, 2, *GEOM, 1) >= 64 * 576 * 4
    # the gate is written out: the rule "cin == width / 2 at stride 2" does not admit a 64-wide stride-2 block
    for cin, width, stride in ((64, 64, 2), (32, 64, 2)):
        for mode in (0, 1):
            assert ws(2, 6, 4, cin, width, stride, mode) == -3701
    assert ws(0, 3, 2, *GEOM, 0) == -3701
    for mode in (-1, 2):
        assert ws(2, 3, 2, *GEOM, mode) == -3701
    # the older families keep refusing the 64-wide block
    for mode in (0, 1):
        assert lib.vtd_block_bn_train_workspace_bytes(2, 3, 2, *GEOM, mode) == -3501
        assert lib.vtd_resblock_bn_train_workspace_bytes(2, 3, 2, *GEOM, mode) == -3401


def test_refusals_before_any_launch():
    lib = _native.load()
    keep = [_aligned(4096) for _ in range(3)]
    a, b, c = (k[1] for k in keep)
    st = _native.BasicBlockParams(*([a] * 15))
    sp = C.byref(st)
    fwd, bwd = lib.vtd_trunk_bn_train_forward, lib.vtd_trunk_bn_train_backward
    s1 = (2, 3, 2, *GEOM)
    for tr in (0, 1):
        # -3701: null pointers, eps <= 0, the 64-wide geometries that are not layer1's
        assert fwd(None, *s1, sp, tr, 0.1, 1e-5, b, c, None, None) == -3701
        assert fwd(a, *s1, None, tr, 0.1, 1e-5, b, c, None, None) == -3701
        assert fwd(a, *s1, sp, tr, 0.1, 1e-5, None, c, None, None) == -3701
        assert fwd(a, *s1, sp, tr, 0.1, 1e-5, b, None, None, None) == -3701
        assert fwd(a, *s1, sp, tr, 0.1, 0.0, b, c, None, None) == -3701
        assert fwd(a, *s1, sp, tr, 0.1, -1e-5, b, c, None, None) == -3701
        for cin, wd, stride in ((64, 64, 2), (32, 64, 2), (128, 64, 1)):
            geom = (2, 6, 4, cin, wd, stride)
            assert fwd(a, *geom, sp, tr, 0.1, 1e-5, b, c, None, None) == -3701, geom
            assert bwd(a, *geom, sp, tr, 1e-5, b, c, a, a, sp, b, None, None, None) == -3701, geom
        nobn2 = _native.BasicBlockParams(*([a] * 5))      # conv2 and its BatchNorm are missing
        assert fwd(a, *s1, C.byref(nobn2), tr, 0.1, 1e-5, b, c, None, None) == -3701
        assert bwd(a, *s1, sp, tr, 1e-5, None, c, a, a, sp, b, None, None, None) == -3701
        assert bwd(a, *s1, sp, tr, 1e-5, b, None, a, a, sp, b, None, None, None) == -3701
        assert bwd(a, *s1, sp, tr, 1e-5, b, c, None, a, sp, b, None, None, None) == -3701
        assert bwd(a, *s1, sp, tr, 1e-5, b, c, a, None, sp, b, None, None, None) == -3701
        assert bwd(a, *s1, sp, tr, 0.0, b, c, a, a, sp, b, None, None, None) == -3701
        assert bwd(a, *s1, sp, tr, 1e-5, b, c, a, a, None, b, None, None, None) == -3701
        assert bwd(a, *s1, sp, tr, 1e-5, b, c, a, a, sp, None, None, None, None) == -3701
        assert bwd(a, *s1, sp, tr, 1e-5, b, c, a, a, sp, b, c, None, None) == -3701      # dx without a place for its scale
        # the block has no downsample: a struct without one is enough, and gets as far as the alignment check
        nods = _native.BasicBlockParams(*([a] * 10))
        assert fwd(a, *s1, C.byref(nods), tr, 0.1, 1e-5, C.c_void_p(b.value + 128), c, None, None) == -3702
        # -3702: each misalignment
        assert fwd(a, *s1, sp, tr, 0.1, 1e-5, C.c_void_p(b.value + 128), c, None, None) == -3702      # the workspace
        assert fwd(C.c_void_p(a.value + 8), *s1, sp, tr, 0.1, 1e-5, b, c, None, None) == -3702      # x
        assert fwd(a, *s1, sp, tr, 0.1, 1e-5, b, C.c_void_p(c.value + 8), None, None) == -3702      # y
        assert fwd(a, *s1, sp, tr, 0.1, 1e-5, b, c, C.c_void_p(a.value + 2), None) == -3702      # the statistics
        assert bwd(C.c_void_p(a.value + 8), *s1, sp, tr, 1e-5, b, c, a, a, sp, b, None, None, None) == -3702
        assert bwd(a, *s1, sp, tr, 1e-5, C.c_void_p(b.value + 128), c, a, a, sp, b, None, None, None) == -3702
        assert bwd(a, *s1, sp, tr, 1e-5, b, C.c_void_p(c.value + 8), a, a, sp, b, None, None, None) == -3702
        assert bwd(a, *s1, sp, tr, 1e-5, b, c, C.c_void_p(a.value + 4), a, sp, b, None, None, None) == -3702      # dy
        assert bwd(a, *s1, sp, tr, 1e-5, b, c, a, C.c_void_p(a.value + 4), sp, b, None, None, None) == -3702      # its scale
        assert bwd(a, *s1, sp, tr, 1e-5, b, c, a, a, sp, C.c_void_p(b.value + 128), None, None, None) == -3702      # the scratch
        assert bwd(a, *s1, sp, tr, 1e-5, b, c, a, a, sp, b, C.c_void_p(c.value + 4), a, None) == -3702      # dx
        assert bwd(a, *s1, sp, tr, 1e-5, b, c, a, a, sp, b, c, C.c_void_p(a.value + 4), None) == -3702      # its scale
    # training outside {0, 1}, momentum outside [0, 1] or NaN
    for tr in (2, -1):
        assert fwd(a, *s1, sp, tr, 0.1, 1e-5, b, c, None, None) == -3701
        assert bwd(a, *s1, sp, tr, 1e-5, b, c, a, a, sp, b, None, None, None) == -3701
    for mom in (1.5, -0.1, float("nan")):
        assert fwd(a, *s1, sp, 1, mom, 1e-5, b, c, None, None) == -3701
    # training = 1 with n h w = 1: one value per channel has no variance
    one = (1, 1, 1, *GEOM)
    assert fwd(a, *one, sp, 1, 0.1, 1e-5, b, c, None, None) == -3701
    assert bwd(a, *one, sp, 1, 1e-5, b, c, a, a, sp, b, None, None, None) == -3701
    # the older families keep their own answers for layer1's geometry
    assert lib.vtd_block_bn_train_forward(a, *s1, sp, 1, 0.1, 1e-5, b, c, None, None) == -3501
    assert lib.vtd_block_bn_train_backward(a, *s1, sp, 1, 1e-5, b, c, a, a, sp, b, None, None, None) == -3501
    assert lib.vtd_resblock_bn_train_forward(a, *s1, sp, 1, 0.1, 1e-5, b, c, None, None) == -3401
    assert lib.vtd_resblock_bn_train_backward(a, *s1, sp, 1, 1e-5, b, c, a, a, sp, b, None, None, None) == -3401
    assert b"batch-statistics" in lib.vtd_strerror(-3701)


# ---- the fixed order of the 64-wide per-channel reductions (include/vtd.h): sixteen parts per workgroup cut at ceil(k r / 16), the
# eight-part order of width 128 on each half, then lower + upper; the workgroups in order
def _cuts16(r):
    return [(k * r + 15) // 16 for k in range(17)]


def _reduce64(v, pairing="tree"):
    """The channel sums of v [rows][C] in the kernels' order, fp64.  pairing="linear" is the control: the same parts summed left to right."""
    rows = v.shape[0]
    red = min(256, max(1, -(-rows // 256)))
    per = -(-rows // red)
    total = np.zeros(v.shape[1], np.float64)
    for g in range(red):
        m0, m1 = min(g * per, rows), min(g * per + per, rows)
        cuts = _cuts16(m1 - m0)
        q = []
        for k in range(16):
            s = np.zeros(v.shape[1], np.float64)
            for m in range(m0 + cuts[k], m0 + cuts[k + 1]):      # row order; a part without rows stays an exact zero
                s = s + v[m].astype(np.float64)
            q.append(s)
        if pairing == "tree":
            lower = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]))
            upper = ((q[8] + q[9]) + (q[10] + q[11])) + ((q[12] + q[13]) + (q[14] + q[15]))
            part = lower + upper
        else:
            part = q[0]
            for k in range(1, 16):
                part = part + q[k]
        total = total + part      # workgroup order
    return total


def test_reduce_order_of_the_64_wide_block():
    # the GPU tests' sizes at n = 2.  1 x 1: two rows, fourteen empty parts; 3 x 2: twelve rows, four empty parts
    assert sum(a == b for a, b in zip(_cuts16(2), _cuts16(2)[1:])) == 14
    assert sum(a == b for a, b in zip(_cuts16(12), _cuts16(12)[1:])) == 4
    # 12 x 11: 264 rows are two workgroups of 132 rows, parts of 9 and 8 rows
    assert sorted({b - a for a, b in zip(_cuts16(132), _cuts16(132)[1:])}) == [8, 9]
    # 23 x 23: 1058 rows are five workgroups of 212 rows, the last of 210
    assert min(256, -(-1058 // 256)) == 5 and -(-1058 // 5) == 212 and 1058 - 4 * 212 == 210
    assert sorted({b - a for a, b in zip(_cuts16(212), _cuts16(212)[1:])}) == [13, 14]
    for r in range(0, 300):      # a partition of the rows, in order, whatever r
        cuts = _cuts16(r)
        assert cuts[0] == 0 and cuts[16] == r and all(x <= y for x, y in zip(cuts, cuts[1:]))
    rng = np.random.default_rng(6)
    differs = 0
    for rows in (1, 2, 12, 17, 40, 264, 1058):
        v = (rng.standard_normal((rows, 8)) * 3 + 0.5).astype(np.float32)
        sq = v.astype(np.float64) ** 2      # the sums of z^2 and of g xh add fp64 products of fp32 values, which round: there the order shows
        got = _reduce64(sq)
        assert np.all(np.abs(got - sq.sum(0)) <= 1e-13 * sq.sum(0)), rows
        differs += int(np.any(got != _reduce64(sq, "linear")))
    assert differs > 0, "the pairing of the sixteen parts is pinned: a linear sum of the same parts must differ in a bit on some input"


# ---- the Python surface: blocks
def test_trunk_block_bn_train_accepts_the_64_wide_block():
    # as far as the device check, with an input that requires grad (the parent refuses the geometry with RuntimeError)
    with pytest.raises(ValueError, match="CUDA"):
        nets.trunk_block_bn_train(nets.BasicBlock(*GEOM), torch.zeros((2, 64, 2, 2), requires_grad=True))
    with pytest.raises(ValueError, match="CUDA"):
        nets.trunk_block_bn_train(nets.BasicBlock(*GEOM).eval(), torch.zeros((2, 64, 2, 2)))
    blk = nets.BasicBlock(*GEOM)
    with pytest.raises(ValueError, match="must be a"):      # a wrong channel count
        nets.trunk_block_bn_train(blk, torch.zeros((2, 128, 2, 2)))
    blk.bn2.momentum = None
    with pytest.raises(ValueError, match="momentum"):
        nets.trunk_block_bn_train(blk, torch.zeros((2, 64, 2, 2)))
    blk.bn2.momentum = 0.2      # differing momenta
    with pytest.raises(ValueError, match="momentum"):
        nets.trunk_block_bn_train(blk, torch.zeros((2, 64, 2, 2)))
    # what is built is named before the device is looked at, for a 64-wide block that is not layer1's too
    for bad in (nets.BasicBlock(64, 64, 2), nets.BasicBlock(32, 64, 2), nets.BasicBlock(64, 256, 2)):
        with pytest.raises(RuntimeError, match="layer1, layer2, layer3 and layer4"):
            nets.trunk_block_bn_train(bad, torch.zeros((2, bad.conv1.in_channels, 4, 4)))
    # the older spellings keep refusing the 64-wide block
    with pytest.raises(RuntimeError, match="layer3 and layer4"):
        nets.basic_block_bn_train(nets.BasicBlock(*GEOM), torch.zeros((2, 64, 4, 4)))
    with pytest.raises(RuntimeError, match="layer4 only"):
        nets.basic_block_train(nets.BasicBlock(*GEOM), torch.zeros((2, 64, 4, 4)), batch_stats=True)


# ---- the Python surface: forward_padded
def _node():
    trunk = nets.make_trunk("resnet18")
    stages = dict(layer4=trunk[7], layer3=trunk[6], layer2=trunk[5], layer1=trunk[4])
    return trunk, nets.FeaturePyramidNetwork(512), nets.DBHead(256), [torch.zeros((1, 18, 18, 64), dtype=torch.float16)], stages


def test_forward_padded_accepts_the_four_stage_tuple():
    trunk, fpn, head, taps, stages = _node()
    # the accepted node goes on to its own checks: CPU taps are refused as without the argument, for a tuple and for a list
    for spelling in (STAGES, list(STAGES)):
        with pytest.raises(ValueError, match="CUDA"):
            fpn.forward_padded(taps, head=head, trunk_batch_stats=spelling, **stages)
    # without layer1, without a stage above it, or with the stem: the message names the node that is built
    upper = {k: v for k, v in stages.items() if k != "layer1"}
    with pytest.raises(ValueError, match="layer1 -> layer2 -> layer3 -> layer4 -> FPN -> head"):
        fpn.forward_padded(taps, head=head, trunk_batch_stats=STAGES, **upper)
    with pytest.raises(ValueError, match="layer1 -> layer2 -> layer3 -> layer4 -> FPN -> head"):
        fpn.forward_padded(taps, head=head, trunk_batch_stats=STAGES, **{k: v for k, v in stages.items() if k != "layer3"})
    with pytest.raises(ValueError, match="takes no stem"):
        fpn.forward_padded(taps, head=head, stem=(trunk[0], trunk[1]), trunk_batch_stats=STAGES, **stages)
    # the stem with any shorter spelling stays refused too
    with pytest.raises(ValueError, match="layer2 -> layer3 -> layer4 -> FPN -> head"):
        fpn.forward_padded(taps, head=head, stem=(trunk[0], trunk[1]), trunk_batch_stats=STAGES[1:], **stages)
    with pytest.raises(ValueError):
        fpn.forward_padded(taps, head=head, stem=(trunk[0], trunk[1]), trunk_batch_stats=True, **stages)
    # the three-stage tuple with layer1 passed keeps its message
    with pytest.raises(ValueError, match="layer2 -> layer3 -> layer4 -> FPN -> head"):
        fpn.forward_padded(taps, head=head, trunk_batch_stats=STAGES[1:], **stages)
    # misordered and partial tuples: the message names the tuples that are built, the four-stage one among them
    for bad in (("layer1",), ("layer1", "layer2"), ("layer1", "layer2", "layer3"), ("layer4", "layer3", "layer2", "layer1"),
                ("layer2", "layer1", "layer3", "layer4"), ("layer1", "layer3", "layer4"), ("layer1", "layer2", "layer3", "layer4", "stem"),
                ("stem", "layer1", "layer2", "layer3", "layer4")):
        with pytest.raises(ValueError, match=r"\('layer1', 'layer2', 'layer3', 'layer4'\)"):
            fpn.forward_padded(taps, head=head, trunk_batch_stats=bad, **stages)


@pytest.mark.parametrize("what", ["eps", "mode", "momentum", "no momentum"])
def test_forward_padded_plan_is_node_wide(what):
    """One mode, one momentum and one eps over the eight blocks, else ValueError -- before the taps' device is looked at (they are CPU
    tensors, which the accepted node refuses with another message)."""
    trunk, fpn, head, taps, stages = _node()
    if what == "eps":
        trunk[4][1].bn1.eps = 1e-3
    elif what == "mode":
        trunk[4][0].eval()
    elif what == "momentum":
        trunk[4][1].bn2.momentum = 0.2
    else:
        trunk[4][0].bn1.momentum = None
    with pytest.raises(ValueError, match="eight blocks must have one BatchNorm eps" if what == "eps" else "eight blocks must be in one mode"):
        fpn.forward_padded(taps, head=head, trunk_batch_stats=STAGES, **stages)
    # and a difference above layer1 is seen as well
    trunk, fpn, head, taps, stages = _node()
    trunk[7][1].bn2.momentum = 0.3
    with pytest.raises(ValueError, match="one mode"):
        fpn.forward_padded(taps, head=head, trunk_batch_stats=STAGES, **stages)


# ---- the Python surface: DBNet
def test_dbnet_trunk_bn_trained_on_the_layer1_mode():
    net = nets.DBNet("resnet18", trainable=MODE4, trunk_bn="trained")
    assert net.trainable == MODE4 and net.trunk_bn == "trained"
    assert list(net.state_dict()) == list(nets.DBNet("resnet18").state_dict())      # the state dict is the reference's, whatever the mode
    assert [i for i in range(8) if any(p.requires_grad for p in net.backbone[i].parameters())] == [4, 5, 6, 7]
    assert all(p.requires_grad for i in (4, 5, 6, 7) for p in net.backbone[i].parameters())
    assert not any(p.requires_grad for i in (0, 1) for p in net.backbone[i].parameters())
    # set_trainable keeps "trained" over the four stage modes, as for the three-stage mode, and refuses where it does not fit
    for mode in ("head+fpn+layer4", MODE3, MODE4):
        assert net.set_trainable(mode).trunk_bn == "trained" and net.trainable == mode
    net.set_trainable(MODE4)
    with pytest.raises(ValueError, match=STEM_FROZEN):      # the kept "trained" does not fit the whole-backbone mode
        net.set_trainable("head+fpn+backbone")
    assert net.trainable == MODE4 and net.trunk_bn == "trained"      # and the network is as it was
    assert [i for i in range(8) if any(p.requires_grad for p in net.backbone[i].parameters())] == [4, 5, 6, 7]
    assert net.set_trainable("head+fpn+backbone", "frozen").trunk_bn == "frozen"
    assert net.set_trainable(MODE4, "trained").trunk_bn == "trained"
    assert net.set_trainable(None, "frozen").trunk_bn == "frozen"
    # refused, with a message that says the stem keeps frozen statistics
    with pytest.raises(ValueError, match=STEM_FROZEN):
        nets.DBNet("resnet18", trainable="head+fpn+backbone", trunk_bn="trained")
    with pytest.raises(ValueError, match=STEM_FROZEN):      # the four-stage tuple spelled on DBNet
        nets.DBNet("resnet18", trainable=MODE4, trunk_bn=STAGES)
    with pytest.raises(ValueError, match="names exactly the residual stages"):
        nets.DBNet("resnet18", trainable=MODE4, trunk_bn=list(STAGES))
    for mode in (None, "head+fpn", MODE4):
        with pytest.raises(ValueError):
            nets.DBNet("resnet50", trainable=mode, trunk_bn="trained")
    with pytest.raises(ValueError, match=STEM_FROZEN):
        nets.DBNet("resnet50", trainable=None, trunk_bn="trained")
    for mode in (MODE3, MODE4, "head+fpn+backbone"):      # "batch" on any mode but layer4's
        with pytest.raises(ValueError, match="built for layer4 only.*" + STEM_FROZEN):
            nets.DBNet("resnet18", trainable=mode, trunk_bn="batch")
    assert nets.DBNet("resnet18", trainable=MODE4).trunk_bn == "frozen"      # the default


def test_dbnet_passes_the_four_stages_to_the_node(monkeypatch):
    """The train-mode forward hands the trunk engine's pooled tap, the four stages and the four-stage tuple to forward_padded."""
    net = nets.DBNet("resnet18", trainable=MODE4, trunk_bn="trained")
    seen = {}

    class Engine:
        def forward_pool(self, x):
            return "pool"

        def forward_trunk(self, x):
            raise AssertionError("the layer1 mode reads the pooled tap, not the FPN levels")

    def forward_padded(taps, **kw):
        seen.update(kw, taps=taps)
        return "out"

    monkeypatch.setattr(net, "trunk_engine", lambda: Engine())
    monkeypatch.setattr(net.fpn, "forward_padded", forward_padded)
    for m in (net.backbone[4], net.backbone[5], net.backbone[6], net.backbone[7], net.fpn, net.head):
        monkeypatch.setattr(m, "cuda", lambda: None)
    version = net._version
    assert net.train()(torch.zeros((2, 3, 640, 640))) == "out"
    assert seen["taps"] == ["pool"] and seen["trunk_batch_stats"] == STAGES and seen["head"] is net.head
    for j in (1, 2, 3, 4):
        assert seen[f"layer{j}"] is net.backbone[3 + j]
    assert "stem" not in seen
    assert net._version == version + 1      # the running statistics moved: the next eval() forward rebuilds the inference engine
    # layer1's tensors are among those whose versions the eval() forward watches
    watched = len(net._head_tensor_versions())
    above = len(nets.DBNet("resnet18", trainable=MODE3)._head_tensor_versions())
    assert len(list(net.backbone[4].parameters())) == 12 and len([k for k, _ in net.backbone[4].named_buffers() if "running" in k]) == 8
    assert watched - above == len(list(net.backbone[4].parameters())) + len(list(net.backbone[4].buffers())) == 12 + 12
    before = net._head_tensor_versions()
    net.backbone[4][1].bn2.running_var.add_(1.0)
    assert net._head_tensor_versions() != before
    # with the default trunk_bn the same forward passes no stage names
    frozen = nets.DBNet("resnet18", trainable=MODE4)
    monkeypatch.setattr(frozen, "trunk_engine", lambda: Engine())
    monkeypatch.setattr(frozen.fpn, "forward_padded", forward_padded)
    for m in (frozen.backbone[4], frozen.backbone[5], frozen.backbone[6], frozen.backbone[7], frozen.fpn, frozen.head):
        monkeypatch.setattr(m, "cuda", lambda: None)
    assert frozen.train()(torch.zeros((2, 3, 640, 640))) == "out" and seen["trunk_batch_stats"] is False


# ---- the call schedule of the new node, with the recording fakes of tests/test_trunk_train_schedule.py
NB = "vtd_trunk_bn_train"
MODE = (True, 0.1)


def test_schedule_of_the_four_stage_node_with_batch_statistics(monkeypatch):
    assert nets._TRUNK_BN == NB
    events, params = sched._run(monkeypatch, taps=("pool",), nblocks=8, entries=(NB,) * 8, bn=MODE)
    want = [
        ("block_fwd", 0, NB, MODE, "pool"), ("block_fwd", 1, NB, MODE, "y0"), ("block_fwd", 2, NB, MODE, "y1"), ("block_fwd", 3, NB, MODE, "y2"),
        ("block_fwd", 4, NB, MODE, "y3"), ("block_fwd", 5, NB, MODE, "y4"), ("block_fwd", 6, NB, MODE, "y5"), ("block_fwd", 7, NB, MODE, "y6"),
        ("fpn_fwd", ("y1", "y3", "y5", "y7")), sched.HEAD_FWD, sched.HEAD_BWD,
        ("fpn_bwd", ("y1", "y3", "y5", "y7"), "fws", "dp2", "dp2s", 8 | 4 | 2 | 1),      # all four input gradients
        ("block_bwd", 7, NB, MODE, "y6", "y7", "dC5", "sC5", True),
        ("block_bwd", 6, NB, MODE, "y5", "y6", "dx7", "dxs7", True),      # layer4.0 forms its dx
        ("combine", "dx6", "dxs6", "dC4", "sC4"),
        ("block_bwd", 5, NB, MODE, "y4", "y5", "dx6", "sum6", True),
        ("block_bwd", 4, NB, MODE, "y3", "y4", "dx5", "dxs5", True),      # layer3.0 forms its dx
        ("combine", "dx4", "dxs4", "dC3", "sC3"),
        ("block_bwd", 3, NB, MODE, "y2", "y3", "dx4", "sum4", True),
        ("block_bwd", 2, NB, MODE, "y1", "y2", "dx3", "dxs3", True),      # layer2.0 forms its dx
        ("combine", "dx2", "dxs2", "dC2", "sC2"),
        ("block_bwd", 1, NB, MODE, "y0", "y1", "dx2", "sum2", True),
        ("block_bwd", 0, NB, MODE, "pool", "y0", "dx1", "dxs1", False),     # layer1.0 forms none
    ]
    assert events == want, "\n".join(f"{'  ' if a == b else '!!'} {a}   |   {b}" for a, b in zip(events + [None] * len(want), want + [None] * len(events)))
    asked = [e[1] for e in events if e[0] == "block_bwd" and e[-1]]
    assert asked == [7, 6, 5, 4, 3, 2, 1] and sum(e[0] == "combine" for e in events) == 3
    assert len(params) == 87 and [float(p.grad) for p in params] == [float(i) for i in range(87)]


def test_raw_wrappers_keep_the_trunk_family_for_the_64_wide_block(monkeypatch):
    """With `bn`, the raw wrappers run vtd_trunk_bn_train_* on layer1's geometry in either mode: the frozen hand-over is the library's."""
    asked = []

    def workspace(query, args, device):
        asked.append((query, args))
        raise LookupError

    monkeypatch.setattr(nets, "_native_workspace", workspace)
    t = torch.zeros(1)
    geom = (2, 6, 4, *GEOM)
    for bn in ((True, 0.1), (False, 0.1)):
        with pytest.raises(LookupError):
            nets._block_forward_raw(t, geom, 1e-5, [t] * 6, [t] * 4, nets._TRUNK_BN, bn)
        with pytest.raises(LookupError):
            nets._block_backward_raw(t, geom, 1e-5, [t] * 6, [t] * 4, t, t, t, t, True, nets._TRUNK_BN, bn)
        assert asked[-2:] == [("vtd_trunk_bn_train_workspace_bytes", (*geom, 0)), ("vtd_trunk_bn_train_workspace_bytes", (*geom, 1))]
