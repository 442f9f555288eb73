"""Train-mode (batch-statistics) BatchNorm for ResNet-18's layer3 and the strided input gradient on that path (csrc/resblock_bn_train.hip,
the vtd_block_bn_train_* entries), without a device: the three C entry points exist and refuse bad arguments before any launch, the
workspace query, the stride-2 block's dx written out in fp64 torch as the kernels form it against autograd -- with negative controls that
must miss by at least 10x the GPU tests' gradient ceiling --, the fixed order of the 256-wide per-channel reductions written out in numpy,
the refusals and acceptances of the new Python spellings, and the call schedule of the layer3 -> layer4 -> FPN -> head node with batch
statistics."""
import ctypes as C
import pathlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_trunk_train_schedule as sched
from vtd_amd import _native, nets

ENTRIES = ("vtd_block_bn_train_workspace_bytes", "vtd_block_bn_train_forward", "vtd_block_bn_train_backward")
GEOMETRIES = ((128, 256, 2), (256, 256, 1), (256, 512, 2), (512, 512, 1))
GRAD_CEILING = 1e-2      # the GPU tests' ceiling on gradients and dx (tests/test_gpu_layer3_bn_train.py)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _aligned(nbytes, align=256):
    raw = (C.c_char * (nbytes + 2 * align))()
    return raw, C.c_void_p((C.addressof(raw) + align - 1) // align * align)


# ---- C ABI, no device
def test_symbols_in_header_library_and_binding_table():
    lib = _native.load()
    header = (pathlib.Path(__file__).resolve().parents[1] / "include" / "vtd.h").read_text()
    for name in ENTRIES:
        assert name + "(" in header, name
        assert name in _native.SIGNATURES and hasattr(lib, name), name
    for code in (-3501, -3502):
        assert b"batch-statistics" in lib.vtd_strerror(code)
    assert lib.vtd_strerror(-3501) != lib.vtd_strerror(-3401) and lib.vtd_strerror(-3502) != lib.vtd_strerror(-3501)


def test_workspace_query():
    lib = _native.load()
    ws, frozen = lib.vtd_block_bn_train_workspace_bytes, lib.vtd_resblock_train_workspace_bytes
    for cin, width, stride in GEOMETRIES:
        for h, w in ((3, 2), (12, 11), (20, 20)):
            geom = (2, h * stride, w * stride, cin, width, stride)
            for mode in (0, 1):
                assert ws(*geom, mode) > 0 and ws(*geom, mode) % 256 == 0, (geom, mode)
                assert ws(*geom, mode) >= frozen(*geom, mode)      # training = 0 runs the general frozen path in the same allocation
    # the layer4 geometries: at least what the 512-only entries ask for (the stride-2 block's scratch also holds the strided dx's planes)
    old = lib.vtd_resblock_bn_train_workspace_bytes
    assert ws(2, 6, 4, 256, 512, 2, 0) == old(2, 6, 4, 256, 512, 2, 0) and ws(2, 6, 4, 256, 512, 2, 1) > old(2, 6, 4, 256, 512, 2, 1)
    assert all(ws(2, 3, 2, 512, 512, 1, m) == old(2, 3, 2, 512, 512, 1, m) for m in (0, 1))
    for bad in ((2, 6, 4, 64, 128, 2), (2, 3, 2, 64, 64, 1), (2, 3, 2, 128, 128, 1), (2, 5, 4, 128, 256, 2), (2, 6, 4, 256, 256, 2),
                (2, 6, 4, 128, 512, 2), (0, 3, 2, 256, 256, 1)):
        assert ws(*bad, 0) == -3501 and ws(*bad, 1) == -3501, bad
    for mode in (-1, 2):
        assert ws(2, 3, 2, 256, 256, 1, mode) == -3501 and ws(2, 6, 4, 128, 256, 2, mode) == -3501


def test_refusals_before_any_launch():
    lib = _native.load()
    keep = [_aligned(4096) for _ in range(3)]
    a, b, c = (k[1] for k in keep)
    st = _native.BasicBlockParams(*([a] * 15))
    sp = C.byref(st)
    fwd, bwd = lib.vtd_block_bn_train_forward, lib.vtd_block_bn_train_backward
    for s1, s2 in (((2, 3, 2, 256, 256, 1), (2, 6, 4, 128, 256, 2)), ((2, 3, 2, 512, 512, 1), (2, 6, 4, 256, 512, 2))):
        cin2, width = s2[3], s2[4]
        for tr in (0, 1):
            # -3501: null pointers, eps <= 0, odd extents at stride 2, the geometries that are not built
            assert fwd(None, *s1, sp, tr, 0.1, 1e-5, b, c, None, None) == -3501
            assert fwd(a, *s1, None, tr, 0.1, 1e-5, b, c, None, None) == -3501
            assert fwd(a, *s1, sp, tr, 0.1, 1e-5, None, c, None, None) == -3501
            assert fwd(a, *s1, sp, tr, 0.1, 1e-5, b, None, None, None) == -3501
            assert fwd(a, *s1, sp, tr, 0.1, 0.0, b, c, None, None) == -3501
            assert fwd(a, *s1, sp, tr, 0.1, -1e-5, b, c, None, None) == -3501
            assert fwd(a, 2, 5, 4, cin2, width, 2, sp, tr, 0.1, 1e-5, b, c, None, None) == -3501
            assert fwd(a, 2, 6, 3, cin2, width, 2, sp, tr, 0.1, 1e-5, b, c, None, None) == -3501
            for geom in ((2, 6, 4, 64, 128, 2), (2, 3, 2, 64, 64, 1), (2, 3, 2, 128, 128, 1)):
                assert fwd(a, *geom, sp, tr, 0.1, 1e-5, b, c, None, None) == -3501, geom
                assert bwd(a, *geom, sp, tr, 1e-5, b, c, a, a, sp, b, None, None, None) == -3501, geom
            nods = _native.BasicBlockParams(*([a] * 10))
            assert fwd(a, *s2, C.byref(nods), tr, 0.1, 1e-5, b, c, None, None) == -3501      # the stride-2 block needs its downsample
            assert bwd(a, *s1, sp, tr, 1e-5, b, c, None, a, sp, b, None, None, None) == -3501
            assert bwd(a, *s1, sp, tr, 0.0, b, c, a, a, sp, b, None, None, None) == -3501
            assert bwd(a, *s1, sp, tr, 1e-5, b, c, a, a, None, b, None, None, None) == -3501
            assert bwd(a, *s1, sp, tr, 1e-5, b, c, a, a, sp, None, None, None, None) == -3501
            assert bwd(a, *s1, sp, tr, 1e-5, b, c, a, a, sp, b, c, None, None) == -3501      # dx without a place for its scale
            assert bwd(a, *s2, sp, tr, 1e-5, b, c, a, a, sp, b, c, None, None) == -3501
            assert bwd(a, 2, 5, 4, cin2, width, 2, sp, tr, 1e-5, b, c, a, a, sp, b, None, None, None) == -3501
            # -3502: alignment
            assert fwd(a, *s1, sp, tr, 0.1, 1e-5, C.c_void_p(b.value + 128), c, None, None) == -3502
            assert fwd(C.c_void_p(a.value + 8), *s1, sp, tr, 0.1, 1e-5, b, c, None, None) == -3502
            assert bwd(a, *s1, sp, tr, 1e-5, b, c, C.c_void_p(a.value + 4), a, sp, b, None, None, None) == -3502      # a misaligned dy
            assert bwd(a, *s1, sp, tr, 1e-5, b, c, a, C.c_void_p(a.value + 4), sp, b, None, None, None) == -3502
            # a dx on the stride-2 block is accepted: with a misaligned dx the call gets as far as the alignment check, past every argument
            # check (the 512-only entries answer -3403 here), and nothing launches
            assert bwd(a, *s2, sp, tr, 1e-5, b, c, a, a, sp, b, C.c_void_p(c.value + 4), a, None) == -3502
            assert bwd(a, *s2, sp, tr, 1e-5, b, c, a, a, sp, b, c, C.c_void_p(a.value + 4), None) == -3502
        # training outside {0, 1}, momentum outside [0, 1] or NaN
        for tr in (2, -1):
            assert fwd(a, *s1, sp, tr, 0.1, 1e-5, b, c, None, None) == -3501
            assert bwd(a, *s1, sp, tr, 1e-5, b, c, a, a, sp, b, None, None, None) == -3501
        for mom in (1.5, -0.1, float("nan")):
            assert fwd(a, *s1, sp, 1, mom, 1e-5, b, c, None, None) == -3501
        # training = 1 with n h w = 1: one value per channel has no variance
        one, one2 = (1, 1, 1, s1[3], width, 1), (1, 2, 2, cin2, width, 2)
        assert fwd(a, *one, sp, 1, 0.1, 1e-5, b, c, None, None) == -3501
        assert bwd(a, *one, sp, 1, 1e-5, b, c, a, a, sp, b, None, None, None) == -3501
        assert fwd(a, *one2, sp, 1, 0.1, 1e-5, b, c, None, None) == -3501
        assert bwd(a, *one2, sp, 1, 1e-5, b, c, a, a, sp, b, None, None, None) == -3501
    # the 512-only entries keep their own answers
    assert lib.vtd_resblock_bn_train_forward(a, 2, 6, 4, 128, 256, 2, sp, 1, 0.1, 1e-5, b, c, None, None) == -3401
    assert lib.vtd_resblock_bn_train_backward(a, 2, 6, 4, 256, 512, 2, sp, 1, 1e-5, b, c, a, a, sp, b, c, a, None) == -3403


# ---- the stride-2 block's dx as the kernels form it, against autograd in fp64.  Reduced channel counts (6 -> 5), as in
# tests/test_layer4_bn_train.py: a relative L2 miss of a wrong formula does not depend on the width.
EPS = 1e-5
GAMMA = [1.3, 0.0, -0.75, 0.4, 2.0]      # a gamma = 0 channel and a gamma < 0 channel, on every BatchNorm of the case


def _strided_case(seed=5, hw=(6, 4)):
    """A stride-2 block's input side in fp64: z1 = conv1(x) (3x3, stride 2), zd = ds(x) (1x1, stride 2), each through its own train-mode
    BatchNorm; upstream gradients g1 (at bn1's output) and g2 (at the downsample BatchNorm's output); autograd's dx."""
    gen = torch.Generator().manual_seed(seed)
    cin, cout = 6, 5
    x = torch.randn((2, cin, *hw), generator=gen).double().requires_grad_(True)
    w1 = torch.randn((cout, cin, 3, 3), generator=gen).double()
    wd = torch.randn((cout, cin, 1, 1), generator=gen).double()
    gam1, gamd = torch.tensor(GAMMA).double(), torch.tensor(GAMMA[::-1]).double()
    bet = torch.randn(cout, generator=gen).double()
    z1, zd = F.conv2d(x, w1, None, 2, 1), F.conv2d(x, wd, None, 2, 0)
    o1 = F.batch_norm(z1, None, None, gam1, bet, True, 0.1, EPS)
    od = F.batch_norm(zd, None, None, gamd, bet, True, 0.1, EPS)
    g1 = torch.randn(o1.shape, generator=gen).double() + 0.5
    g2 = torch.randn(od.shape, generator=gen).double() - 0.25
    torch.autograd.backward([o1, od], [g1, g2])
    return x.detach(), w1, wd, gam1, gamd, z1.detach(), zd.detach(), g1, g2, x.grad.clone()


def _dz(z, g, gam):
    """dz = gamma rstd (g - s1 / M - xh s2 / M), as bt_form_kernel forms it."""
    M = z.numel() // z.shape[1]
    b = lambda v: v[None, :, None, None]  # noqa: E731
    mu, var = z.mean((0, 2, 3)), z.var((0, 2, 3), unbiased=False)
    rstd = 1.0 / torch.sqrt(var + EPS)
    xh = (z - b(mu)) * b(rstd)
    return b(gam * rstd) * (g - b(g.sum((0, 2, 3))) / M - xh * b((g * xh).sum((0, 2, 3))) / M)


def _strided_dx(x, w1, wd, gam1, gamd, z1, zd, g1, g2, bug=None):
    """dx as csrc/resblock_bn_train.hip forms it: dz1 at the even positions of a zero plane of the input's extent, the stride-1 3x3
    convolution with the weights rotated by 180 degrees and transposed, plus ds^T(dz_d) -- the downsample BatchNorm's own dz -- at the
    even (row, column) positions."""
    n, cin, H, W = x.shape
    dz1, dzd = _dz(z1, g1, gam1), _dz(zd, g2, gamd)
    plane = torch.zeros((n, w1.shape[0], H, W), dtype=torch.float64)
    off = 1 if bug == "odd_positions" else 0
    plane[:, :, off::2, off::2] = dz1
    wt = w1 if bug == "unrotated_weights" else w1.flip(2, 3)
    dx = F.conv2d(plane, wt.transpose(0, 1), None, 1, 1)
    if bug != "downsample_left_out":
        t = torch.einsum("nohw,oc->nchw", g2 if bug == "ds_of_g2" else dzd, wd[:, :, 0, 0])
        dx[:, :, 0::2, 0::2] += t
    return dx


def test_strided_dx_matches_autograd():
    case = _strided_case()
    dx = _strided_dx(*case[:-1])
    assert _rel(dx.numpy(), case[-1].numpy()) <= 1e-12
    x, w1, wd, gam1, gamd, z1, zd, g1, g2, _ = case
    assert float(_dz(z1, g1, gam1)[:, 1].abs().max()) == 0 and float(_dz(z1, g1, gam1)[:, 2].abs().max()) > 0      # gamma = 0, gamma < 0
    assert float(_dz(zd, g2, gamd)[:, 3].abs().max()) == 0
    # another extent, another seed
    case = _strided_case(seed=9, hw=(4, 10))
    assert _rel(_strided_dx(*case[:-1]).numpy(), case[-1].numpy()) <= 1e-12


@pytest.mark.parametrize("bug", ["ds_of_g2", "downsample_left_out", "odd_positions", "unrotated_weights"])
def test_strided_dx_negative_controls_miss_by_ten_times_the_ceiling(bug):
    case = _strided_case()
    err = _rel(_strided_dx(*case[:-1], bug=bug).numpy(), case[-1].numpy())
    assert err >= 10 * GRAD_CEILING, f"{bug}: error {err:.3g} is not 10x the ceiling {GRAD_CEILING}"


def test_downsample_scale_factor_is_exact():
    """dz_d's total scale is dscale scd, dz1's dscale sc2 sc1 (each a power of two): sc2 sc1 / scd brings the first to the second in fp32
    without rounding, small and large exponents alike."""
    for e2, e1, ed in ((14, 9, 17), (-60, 30, 45), (100, 20, -3), (-120, 0, -119)):
        sc2, sc1, scd = (np.float32(2.0) ** np.float32(e) for e in (e2, e1, ed))
        mul = np.float32(sc2 * sc1) / scd
        assert float(mul) == 2.0 ** (e2 + e1 - ed)
        v = np.float32(0.7310585975646973)
        assert float(v * mul) == float(v) * 2.0 ** (e2 + e1 - ed)


# ---- the fixed order of the 256-wide per-channel reductions (include/vtd.h): four quarters per workgroup, (q0 + q1) + (q2 + q3), the
# workgroups in order
def _quarter_cuts(r):
    return [(k * r + 3) // 4 for k in range(5)]


def _reduce256(v):
    """The channel sums of v [rows][C] in the kernels' order, fp64."""
    rows = v.shape[0]
    red = min(256, max(1, -(-rows // 256)))
    per = -(-rows // red)
    total = np.zeros(v.shape[1], np.float64)
    for g in range(red):
        m0, m1 = min(g * per, rows), min(g * per + per, rows)
        cuts = _quarter_cuts(m1 - m0)
        q = []
        for k in range(4):
            s = np.zeros(v.shape[1], np.float64)
            for m in range(m0 + cuts[k], m0 + cuts[k + 1]):      # row order
                s = s + v[m].astype(np.float64)
            q.append(s)
        total = total + ((q[0] + q[1]) + (q[2] + q[3]))      # workgroup order
    return total


def test_reduce_order_of_the_256_wide_blocks():
    assert _quarter_cuts(1) == [0, 1, 1, 1, 1]      # ceil(k / 4): one row, the first quarter has it
    assert _quarter_cuts(2) == [0, 1, 1, 2, 2]
    assert _quarter_cuts(3) == [0, 1, 2, 3, 3]
    assert _quarter_cuts(5) == [0, 2, 3, 4, 5]
    assert _quarter_cuts(66) == [0, 17, 33, 50, 66]
    assert _quarter_cuts(132) == [0, 33, 66, 99, 132]      # the GPU tests' 12 x 11 case: two workgroups of 132 rows, quarters of 33
    for r in range(0, 300):      # a partition of the rows, in order, whatever r
        cuts = _quarter_cuts(r)
        assert cuts[0] == 0 and cuts[4] == r and all(a <= b for a, b in zip(cuts, cuts[1:]))
    rng = np.random.default_rng(4)
    for rows in (1, 2, 3, 5, 66, 264, 700):
        v = (rng.standard_normal((rows, 8)) * 3 + 0.5).astype(np.float32)
        want = v.astype(np.float64).sum(0)
        got = _reduce256(v)
        assert np.all(np.abs(got - want) <= 1e-13 * np.abs(v.astype(np.float64)).sum(0)), rows


# ---- the Python surface
def test_basic_block_bn_train_refusals():
    with pytest.raises(RuntimeError, match="Bottleneck training is not built"):
        nets.basic_block_bn_train(nets.Bottleneck(256, 64, 1), torch.zeros((1, 256, 2, 2)))
    for blk, x in ((nets.BasicBlock(64, 128, 2), torch.zeros((2, 64, 4, 4))), (nets.BasicBlock(128, 128, 1), torch.zeros((2, 128, 2, 2))),
                   (nets.BasicBlock(64, 64, 1), torch.zeros((2, 64, 2, 2)))):
        with pytest.raises(RuntimeError, match="layer3 and layer4"):      # what is built is named before the device is looked at
            nets.basic_block_bn_train(blk, x)
    # the four geometries get as far as the device check
    for cin, width, stride in GEOMETRIES:
        with pytest.raises(ValueError, match="CUDA"):
            nets.basic_block_bn_train(nets.BasicBlock(cin, width, stride), torch.zeros((2, cin, 2 * stride, 2 * stride), requires_grad=True))
    blk = nets.BasicBlock(256, 256, 1)
    with pytest.raises(ValueError, match="must be a"):
        nets.basic_block_bn_train(blk, torch.zeros((2, 128, 2, 2)))
    blk.bn2.momentum = None
    with pytest.raises(ValueError, match="momentum"):
        nets.basic_block_bn_train(blk, torch.zeros((2, 256, 2, 2)))
    blk.bn2.momentum = 0.2      # differing momenta
    with pytest.raises(ValueError, match="momentum"):
        nets.basic_block_bn_train(blk, torch.zeros((2, 256, 2, 2)))


def test_forward_padded_accepts_stage_tuples():
    trunk = nets.make_trunk("resnet18")
    fpn, head = nets.FeaturePyramidNetwork(512), nets.DBHead(256)
    taps = [torch.zeros((1, 18, 18, 64), dtype=torch.float16), torch.zeros((1, 10, 10, 128), dtype=torch.float16)]
    c4 = torch.zeros((1, 6, 6, 256), dtype=torch.float16)
    for bad in (("layer3",), ("layer4", "layer3"), ("layer2", "layer3", "layer4"), (), ("layer4", "layer4"), ["stem"]):
        with pytest.raises(ValueError, match=r"\('layer3', 'layer4'\)"):      # the message names what is built
            fpn.forward_padded(taps, head=head, layer4=trunk[7], layer3=trunk[6], trunk_batch_stats=bad)
    # ("layer3", "layer4") is the node of exactly those stages
    with pytest.raises(ValueError, match="layer3 -> layer4 -> FPN -> head"):
        fpn.forward_padded(taps + [c4], head=head, layer4=trunk[7], trunk_batch_stats=("layer3", "layer4"))
    with pytest.raises(ValueError, match="layer3 -> layer4 -> FPN -> head"):
        fpn.forward_padded(taps, head=head, layer4=trunk[7], layer3=trunk[6], layer2=trunk[5], trunk_batch_stats=("layer3", "layer4"))
    # ("layer4",) means what True means
    with pytest.raises(ValueError, match="layer4 only"):
        fpn.forward_padded(taps, head=head, layer4=trunk[7], layer3=trunk[6], trunk_batch_stats=("layer4",))
    with pytest.raises(ValueError, match="CUDA"):
        fpn.forward_padded(taps + [c4], head=head, layer4=trunk[7], trunk_batch_stats=("layer4",))
    # the accepted node goes on to its own checks: CPU taps are refused as without the argument, for a tuple and for a list
    for spelling in (("layer3", "layer4"), ["layer3", "layer4"]):
        with pytest.raises(ValueError, match="CUDA"):
            fpn.forward_padded(taps, head=head, layer4=trunk[7], layer3=trunk[6], trunk_batch_stats=spelling)


def test_forward_padded_plan_is_node_wide():
    """One mode, one momentum and one eps over the four blocks, else ValueError -- before the taps' device is looked at."""
    fpn, head = nets.FeaturePyramidNetwork(512), nets.DBHead(256)
    taps = [torch.zeros((1, 18, 18, 64), dtype=torch.float16), torch.zeros((1, 10, 10, 128), dtype=torch.float16)]
    trunk = nets.make_trunk("resnet18")
    trunk[7][1].bn1.eps = 1e-3
    with pytest.raises(ValueError, match="one BatchNorm eps"):
        fpn.forward_padded(taps, head=head, layer4=trunk[7], layer3=trunk[6], trunk_batch_stats=("layer3", "layer4"))


def test_dbnet_trunk_bn_tuples():
    net = nets.DBNet("resnet18", trainable="head+fpn+layer4+layer3", trunk_bn=("layer3", "layer4"))
    assert net.trainable == "head+fpn+layer4+layer3" and net.trunk_bn == ("layer3", "layer4")
    assert list(net.state_dict()) == list(nets.DBNet("resnet18").state_dict())      # the state dict is the reference's, whatever the mode
    assert [i for i in range(8) if any(p.requires_grad for p in net.backbone[i].parameters())] == [6, 7]
    with pytest.raises(ValueError, match=r"\('layer3', 'layer4'\)"):      # the kept tuple does not fit the new mode
        net.set_trainable(None)
    assert net.trainable == "head+fpn+layer4+layer3" and net.trunk_bn == ("layer3", "layer4")      # and the network is as it was
    assert net.set_trainable("head+fpn+layer4+layer3").trunk_bn == ("layer3", "layer4")
    assert net.set_trainable("head+fpn+layer4+layer3", ["layer3", "layer4"]).trunk_bn == ("layer3", "layer4")
    assert net.set_trainable(None, "frozen").trunk_bn == "frozen"
    # ("layer4",) goes with the layer4 mode
    net4 = nets.DBNet("resnet18", trainable="head+fpn+layer4", trunk_bn=("layer4",))
    assert net4.trainable == "head+fpn+layer4" and net4.trunk_bn == ("layer4",)
    # the tuple names exactly the residual stages the mode trains
    for mode, bn in (("head+fpn+layer4", ("layer3", "layer4")), ("head+fpn+layer4+layer3+layer2", ("layer3", "layer4")),
                     ("head+fpn+layer4+layer3", ("layer4",)), ("head+fpn+layer4+layer3", ("layer4", "layer3")), ("head+fpn", ("layer4",)),
                     (None, ("layer3", "layer4")), ("head+fpn+layer4+layer3+layer2", ("layer2", "layer3", "layer4")), ("head+fpn+layer4", ()),
                     ("head+fpn+backbone", ("layer3", "layer4")), (None, ()), ("head+fpn+layer4", (["layer4"],))):
        with pytest.raises(ValueError, match="names exactly the residual stages"):
            nets.DBNet("resnet18", trainable=mode, trunk_bn=bn)
    with pytest.raises(ValueError):
        nets.DBNet("resnet50", trainable="head+fpn+layer4+layer3", trunk_bn=("layer3", "layer4"))
    with pytest.raises(ValueError, match="names exactly the residual stages"):
        nets.DBNet("resnet50", trainable="head+fpn", trunk_bn=("layer3", "layer4"))
    # the strings are unchanged
    with pytest.raises(ValueError, match="built for layer4 only"):
        nets.DBNet("resnet18", trainable="head+fpn+layer4+layer3", trunk_bn="batch")
    with pytest.raises(ValueError, match="trunk_bn must be"):
        nets.DBNet("resnet18", trainable="head+fpn+layer4+layer3", trunk_bn="train")


def test_dbnet_passes_the_tuple_to_the_node(monkeypatch):
    """The train-mode forward hands the trunk engine's C2 and C3, layer3, layer4 and the tuple to forward_padded."""
    net = nets.DBNet("resnet18", trainable="head+fpn+layer4+layer3", trunk_bn=("layer3", "layer4"))
    seen = {}

    class Engine:
        def forward_trunk(self, x):
            return ["C2", "C3", "C4", "C5"]

    def forward_padded(taps, **kw):
        seen.update(kw, taps=taps)
        return "out"

    monkeypatch.setattr(net, "trunk_engine", lambda: Engine())
    monkeypatch.setattr(net.fpn, "forward_padded", forward_padded)
    for m in (net.backbone[6], net.backbone[7], net.fpn, net.head):
        monkeypatch.setattr(m, "cuda", lambda: None)
    version = net._version
    assert net.train()(torch.zeros((2, 3, 640, 640))) == "out"
    assert seen["taps"] == ["C2", "C3"] and seen["trunk_batch_stats"] == ("layer3", "layer4") and seen["head"] is net.head
    assert seen["layer3"] is net.backbone[6] and seen["layer4"] is net.backbone[7] and "layer2" not in seen
    assert net._version == version + 1      # the running statistics moved: the next eval() forward rebuilds the inference engine
    # the trained stages' buffers are among the tensors whose versions the eval() forward watches
    watched = len(net._head_tensor_versions())
    frozen_mode = len(nets.DBNet("resnet18", trainable="head+fpn+layer4")._head_tensor_versions())
    assert watched - frozen_mode == len(list(net.backbone[6].parameters())) + len(list(net.backbone[6].buffers())) == 15 + 15


# ---- the call schedule of the new depth, with the recording fakes of tests/test_trunk_train_schedule.py
NB = "vtd_block_bn_train"
MODE = (True, 0.1)


def test_schedule_of_the_layer3_layer4_node_with_batch_statistics(monkeypatch):
    events, params = sched._run(monkeypatch, taps=("C2", "C3"), nblocks=4, entries=(NB,) * 4, bn=MODE)
    want = [
        ("block_fwd", 0, NB, MODE, "C3"), ("block_fwd", 1, NB, MODE, "y0"), ("block_fwd", 2, NB, MODE, "y1"), ("block_fwd", 3, NB, MODE, "y2"),
        ("fpn_fwd", ("C2", "C3", "y1", "y3")), sched.HEAD_FWD, sched.HEAD_BWD,
        ("fpn_bwd", ("C2", "C3", "y1", "y3"), "fws", "dp2", "dp2s", 8 | 4),
        ("block_bwd", 3, NB, MODE, "y2", "y3", "dC5", "sC5", True),
        ("block_bwd", 2, NB, MODE, "y1", "y2", "dx3", "dxs3", True),      # layer4.0 forms its dx: the strided dgrad with batch statistics
        ("combine", "dx2", "dxs2", "dC4", "sC4"),                        # the one combine: layer4.0's dx + the FPN's dC4
        ("block_bwd", 1, NB, MODE, "y0", "y1", "dx2", "sum2", True),
        ("block_bwd", 0, NB, MODE, "C3", "y0", "dx1", "dxs1", False),    # layer3.0 forms none
    ]
    assert events == want, "\n".join(f"{'  ' if a == b else '!!'} {a}   |   {b}" for a, b in zip(events + [None] * len(want), want + [None] * len(events)))
    assert sum(e[0] == "combine" for e in events) == 1
    assert len(params) == 60 and [float(p.grad) for p in params] == [float(i) for i in range(60)]


def test_raw_wrappers_pick_the_entry_family(monkeypatch):
    """With `bn`, the raw wrappers run vtd_block_bn_train_* when the entry names that family and vtd_resblock_bn_train_* otherwise, as the
    callers of the 512-only entries expect."""
    asked = []

    def workspace(query, args, device):
        asked.append(query)
        raise LookupError

    monkeypatch.setattr(nets, "_native_workspace", workspace)
    t = torch.zeros(1)
    geom = (2, 6, 4, 128, 256, 2)
    for entry, want in ((nets._BLOCK_BN, "vtd_block_bn_train"), (nets._RESBLOCK, "vtd_resblock_bn_train"), (nets._BASICBLOCK, "vtd_resblock_bn_train")):
        with pytest.raises(LookupError):
            nets._block_forward_raw(t, geom, 1e-5, [t] * 9, [t] * 6, entry, (True, 0.1))
        with pytest.raises(LookupError):
            nets._block_backward_raw(t, geom, 1e-5, [t] * 9, [t] * 6, t, t, t, t, True, entry, (True, 0.1))
        assert asked[-2:] == [want + "_workspace_bytes"] * 2
    with pytest.raises(LookupError):
        nets._block_forward_raw(t, geom, 1e-5, [t] * 9, [t] * 6, nets._RESBLOCK, None)
    assert asked[-1] == "vtd_resblock_train_workspace_bytes"
