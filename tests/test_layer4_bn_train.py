"""Train-mode (batch-statistics) BatchNorm for ResNet-18's layer4 (csrc/resblock_bn_train.hip), without a device: the three C entry points
exist and refuse bad arguments before any launch, the workspace query, the train-mode identities written out as the kernels compute them
(dz, dgamma = sum g xh, dbeta = sum g, dW = dz^T im2col(x), the running update) against torch autograd in fp64 -- with negative controls
that must miss by at least 10x the GPU tests' gradient bound -- and the Python surface's refusals."""
import ctypes as C
import pathlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vtd_amd import _native, nets

ENTRIES = ("vtd_resblock_bn_train_workspace_bytes", "vtd_resblock_bn_train_forward", "vtd_resblock_bn_train_backward")
# the GPU tests' bound on the blocks' parameter gradients (tests/test_gpu_layer4_bn_train.py BLOCK_BOUNDS, the larger of the two blocks': the
# ceiling)
BLOCK_GRAD_BOUND = 1e-2


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
    for code in (-3401, -3402, -3403):
        assert b"batch-statistics" in lib.vtd_strerror(code)
    assert b"stride-2" in lib.vtd_strerror(-3403)


def test_workspace_query():
    ws = _native.load().vtd_resblock_bn_train_workspace_bytes
    frozen = _native.load().vtd_basicblock_train_workspace_bytes
    for geom in ((2, 6, 4, 256, 512, 2), (2, 3, 2, 512, 512, 1), (2, 40, 40, 256, 512, 2), (2, 20, 20, 512, 512, 1)):
        for mode in (0, 1):
            assert ws(*geom, mode) > 0 and ws(*geom, mode) % 256 == 0, (geom, mode)
            assert ws(*geom, mode) >= frozen(*geom, mode)      # training = 0 runs the frozen path in the same allocation
    for bad in ((2, 6, 4, 128, 256, 2), (2, 3, 2, 64, 64, 1), (2, 5, 4, 256, 512, 2), (2, 6, 4, 512, 512, 2), (0, 3, 2, 512, 512, 1)):
        assert ws(*bad, 0) < 0 and ws(*bad, 1) < 0, bad
    for mode in (-1, 2):
        assert ws(2, 3, 2, 512, 512, 1, mode) < 0 and ws(2, 6, 4, 256, 512, 2, mode) < 0


def test_refusals_before_any_launch():
    lib = _native.load()
    keep = [_aligned(4096) for _ in range(3)]
    a, b, c = (k[1] for k in keep)
    st = _native.BasicBlockParams(*([a] * 15))
    sp = C.byref(st)
    fwd, bwd = lib.vtd_resblock_bn_train_forward, lib.vtd_resblock_bn_train_backward
    s1, s2 = (2, 3, 2, 512, 512, 1), (2, 6, 4, 256, 512, 2)
    for tr in (0, 1):
        # -3401: null pointers, eps <= 0, odd extents at stride 2, another geometry
        assert fwd(None, *s1, sp, tr, 0.1, 1e-5, b, c, None, None) == -3401
        assert fwd(a, *s1, None, tr, 0.1, 1e-5, b, c, None, None) == -3401
        assert fwd(a, *s1, sp, tr, 0.1, 1e-5, None, c, None, None) == -3401
        assert fwd(a, *s1, sp, tr, 0.1, 0.0, b, c, None, None) == -3401
        assert fwd(a, *s1, sp, tr, 0.1, -1e-5, b, c, None, None) == -3401
        assert fwd(a, 2, 5, 4, 256, 512, 2, sp, tr, 0.1, 1e-5, b, c, None, None) == -3401
        assert fwd(a, 2, 6, 3, 256, 512, 2, sp, tr, 0.1, 1e-5, b, c, None, None) == -3401
        assert fwd(a, 2, 6, 4, 128, 256, 2, sp, tr, 0.1, 1e-5, b, c, None, None) == -3401
        nods = _native.BasicBlockParams(*([a] * 10))
        assert fwd(a, *s2, C.byref(nods), tr, 0.1, 1e-5, b, c, None, None) == -3401      # the stride-2 block needs its downsample
        assert bwd(a, *s1, sp, tr, 1e-5, b, c, None, a, sp, b, None, None, None) == -3401
        assert bwd(a, *s1, sp, tr, 0.0, b, c, a, a, sp, b, None, None, None) == -3401
        assert bwd(a, *s1, sp, tr, 1e-5, b, c, a, a, None, b, None, None, None) == -3401
        assert bwd(a, *s1, sp, tr, 1e-5, b, c, a, a, sp, b, c, None, None) == -3401      # dx without a place for its scale
        assert bwd(a, 2, 5, 4, 256, 512, 2, sp, tr, 1e-5, b, c, a, a, sp, b, None, None, None) == -3401
        # -3402: alignment
        assert fwd(a, *s1, sp, tr, 0.1, 1e-5, C.c_void_p(b.value + 128), c, None, None) == -3402
        assert bwd(a, *s1, sp, tr, 1e-5, b, c, C.c_void_p(a.value + 4), a, sp, b, None, None, None) == -3402      # a misaligned dy
        assert bwd(a, *s1, sp, tr, 1e-5, b, c, a, C.c_void_p(a.value + 4), sp, b, None, None, None) == -3402
        # -3403: no input gradient for the stride-2 block
        assert bwd(a, *s2, sp, tr, 1e-5, b, c, a, a, sp, b, c, a, None) == -3403
    # training = 1 with n h w = 1: one value per channel has no variance (torch raises too); training = 0 has no such limit, and a
    # `training` outside {0, 1} or a momentum outside [0, 1] is an argument error
    one = (1, 1, 1, 512, 512, 1)
    assert fwd(a, *one, sp, 1, 0.1, 1e-5, b, c, None, None) == -3401
    assert bwd(a, *one, sp, 1, 1e-5, b, c, a, a, sp, b, None, None, None) == -3401
    assert fwd(a, 1, 2, 2, 256, 512, 2, sp, 1, 0.1, 1e-5, b, c, None, None) == -3401
    assert fwd(a, *s1, sp, 2, 0.1, 1e-5, b, c, None, None) == -3401
    assert fwd(a, *s1, sp, 1, 1.5, 1e-5, b, c, None, None) == -3401
    assert fwd(a, *s1, sp, 1, float("nan"), 1e-5, b, c, None, None) == -3401


# ---- the train-mode identities as the kernels form them, against autograd in fp64.  Reduced channel counts (6 -> 5) as in
# tests/test_layer4_train.py: a relative L2 miss of a wrong formula does not depend on the width.
EPS, MOMENTUM = 1e-5, 0.1


def _case(stride, ksz, seed=3, hw=(6, 4)):
    gen = torch.Generator().manual_seed(seed)
    cin, cout = 6, 5
    x = torch.randn((2, cin, *hw), generator=gen).double()
    w = torch.randn((cout, cin, ksz, ksz), generator=gen).double().requires_grad_(True)
    gam = torch.tensor([1.3, 0.0, -0.75, 0.4, 2.0]).double().requires_grad_(True)      # a gamma = 0 channel and a gamma < 0 channel
    bet = torch.randn(cout, generator=gen).double().requires_grad_(True)
    rmean, rvar = torch.randn(cout, generator=gen).double(), (torch.rand(cout, generator=gen) + 0.5).double()
    before = (rmean.clone(), rvar.clone())
    z = F.conv2d(x, w, None, stride, ksz // 2)
    z.retain_grad()
    y = F.batch_norm(z, rmean, rvar, gam, bet, True, MOMENTUM, EPS)      # updates rmean / rvar in place, as the module does
    g = torch.randn(y.shape, generator=gen).double() + 0.5      # with a mean per channel: the s1 / M term is there to remove exactly that
    y.backward(g)
    return x, w, gam, bet, z, g, before, (rmean, rvar)


def _identities(x, w, gam, z, g, stride, ksz, bug=None):
    """(dz, dgamma, dbeta, dW, mu, the variance for the running update) as csrc/resblock_bn_train.hip forms them."""
    cout = w.shape[0]
    zd = z.detach()
    M = zd.numel() // cout
    mu, var = zd.mean((0, 2, 3)), zd.var((0, 2, 3), unbiased=False)
    rstd = 1.0 / torch.sqrt(var + EPS)
    b = lambda v: v[None, :, None, None]  # noqa: E731
    xh = (zd - b(mu)) * b(rstd)
    s1, s2 = g.sum((0, 2, 3)), (g * xh).sum((0, 2, 3))
    t1 = 0.0 if bug == "s1_term_dropped" else b(s1) / M
    t2 = 0.0 if bug == "xhat_s2_term_dropped" else xh * b(s2) / M
    dz = b(gam.detach() * rstd) * (g - t1 - t2)
    cols = F.unfold(x, ksz, padding=ksz // 2, stride=stride)      # [n][cin k k][pix]
    dw = torch.einsum("ncp,nkp->ck", dz.reshape(dz.shape[0], cout, -1), cols)
    if bug == "gamma_rstd_twice":      # the frozen path's factor on top of a dz that carries it already
        dw = (gam.detach() * rstd)[:, None] * dw
    run_var = var if bug == "biased_running_var" else var * M / (M - 1)
    return dz, s2, s1, dw, mu, run_var


@pytest.mark.parametrize("stride,ksz", [(1, 3), (2, 3), (2, 1)])
def test_train_mode_identities_match_autograd(stride, ksz):
    x, w, gam, bet, z, g, (rmean0, rvar0), (rmean, rvar) = _case(stride, ksz)
    dz, dgam, dbet, dw, mu, run_var = _identities(x, w, gam, z, g, stride, ksz)
    assert _rel(dz.numpy(), z.grad.numpy()) <= 1e-12
    assert _rel(dgam.numpy(), gam.grad.numpy()) <= 1e-12 and _rel(dbet.numpy(), bet.grad.numpy()) <= 1e-12
    assert _rel(dw.numpy(), w.grad.reshape(w.shape[0], -1).numpy()) <= 1e-12
    # the running update, from the buffers the case started with
    assert _rel(((1 - MOMENTUM) * rmean0 + MOMENTUM * mu).numpy(), rmean.numpy()) <= 1e-12
    assert _rel(((1 - MOMENTUM) * rvar0 + MOMENTUM * run_var).numpy(), rvar.numpy()) <= 1e-12
    assert float(gam.grad[1].abs()) > 0 and float(w.grad[1].abs().max()) == 0 and float(dw[1].abs().max()) == 0      # gamma = 0
    assert float(dz[:, 2].abs().max()) > 0      # gamma < 0: an ordinary channel


@pytest.mark.parametrize("bug", ["xhat_s2_term_dropped", "s1_term_dropped", "biased_running_var", "gamma_rstd_twice"])
@pytest.mark.parametrize("stride,ksz", [(1, 3), (2, 3), (2, 1)])
def test_negative_controls_miss_by_ten_times_the_bound(bug, stride, ksz):
    # M = 8 values per channel: the biased variance misses the unbiased one by 1 / M of the moving part
    x, w, gam, bet, z, g, (_, rvar0), (_, rvar) = _case(stride, ksz, hw=(2 * stride, 2 * stride))
    assert z.numel() // z.shape[1] == 8
    dz, dgam, dbet, dw, mu, run_var = _identities(x, w, gam, z, g, stride, ksz, bug)
    # the moving part of the running variance: what the update adds to (1 - momentum) var
    e_run = _rel((MOMENTUM * run_var).numpy(), (rvar - (1 - MOMENTUM) * rvar0).numpy())
    err = max(_rel(dz.numpy(), z.grad.numpy()), _rel(dw.numpy(), w.grad.reshape(w.shape[0], -1).numpy()), e_run)
    assert err >= 10 * BLOCK_GRAD_BOUND, f"{bug}: error {err:.3g} is not 10x the bound {BLOCK_GRAD_BOUND}"


# ---- the Python surface
def test_trunk_bn_modes():
    net = nets.DBNet("resnet18", trainable="head+fpn+layer4", trunk_bn="batch")
    assert net.trainable == "head+fpn+layer4" and net.trunk_bn == "batch"
    assert nets.DBNet("resnet18", trainable="head+fpn+layer4").trunk_bn == "frozen" and nets.DBNet("resnet18").trunk_bn == "frozen"
    # the state dict is the reference's, whatever the mode
    assert list(net.state_dict()) == list(nets.DBNet("resnet18").state_dict())
    # set_trainable keeps trunk_bn when it is not given, and takes a new one
    assert net.set_trainable("head+fpn+layer4").trunk_bn == "batch"
    assert net.set_trainable("head+fpn+layer4", trunk_bn="frozen").trunk_bn == "frozen"
    assert net.set_trainable("head+fpn+layer4").trunk_bn == "frozen"
    assert net.set_trainable("head+fpn+layer4", "batch").trunk_bn == "batch"
    # every other mode refuses "batch", naming what is built, and leaves the network as it was
    for mode in (None, "head", "head+fpn", "head+fpn+layer4+layer3", "head+fpn+layer4+layer3+layer2", "head+fpn+layer4+layer3+layer2+layer1",
                 "head+fpn+backbone"):
        with pytest.raises(ValueError, match="built for layer4 only"):
            nets.DBNet("resnet18", trainable=mode, trunk_bn="batch")
        with pytest.raises(ValueError, match="built for layer4 only"):
            net.set_trainable(mode)      # the kept "batch" does not fit the new mode
        assert net.trainable == "head+fpn+layer4" and net.trunk_bn == "batch"
    for bad in ("train", "eval", "", 1, True):
        with pytest.raises(ValueError, match="trunk_bn must be"):
            nets.DBNet("resnet18", trainable="head+fpn+layer4", trunk_bn=bad)
    # resnet50 keeps its message for the stage modes, and has no train-mode trunk BatchNorm in any other
    with pytest.raises(ValueError, match="Bottleneck training is not built"):
        nets.DBNet("resnet50", trainable="head+fpn+layer4", trunk_bn="batch")
    with pytest.raises(ValueError, match="built for layer4 only"):
        nets.DBNet("resnet50", trunk_bn="batch")
    with pytest.raises(ValueError, match="built for layer4 only"):
        nets.DBNet("resnet50", trainable="head+fpn", trunk_bn="batch")
    assert nets.DBNet("resnet50", trainable="head+fpn", trunk_bn="frozen").trunk_bn == "frozen"


def test_basic_block_train_batch_stats_refusals():
    blk = nets.BasicBlock(512, 512, 1)
    with pytest.raises(ValueError, match="CUDA"):
        nets.basic_block_train(blk, torch.zeros((2, 512, 2, 2)), batch_stats=True)
    with pytest.raises(RuntimeError, match="layer4 only"):      # a layer3 block: what is built is named before the device is looked at
        nets.basic_block_train(nets.BasicBlock(128, 256, 2), torch.zeros((2, 128, 4, 4)), batch_stats=True)
    with pytest.raises(RuntimeError, match="layer4 only"):
        nets.basic_block_train(nets.BasicBlock(64, 64, 1), torch.zeros((2, 64, 4, 4)), batch_stats=True)
    blk.bn2.momentum = None
    with pytest.raises(ValueError, match="momentum"):
        nets.basic_block_train(blk, torch.zeros((2, 512, 2, 2)), batch_stats=True)
    blk.bn2.momentum = 0.2      # differing momenta
    with pytest.raises(ValueError, match="momentum"):
        nets.basic_block_train(blk, torch.zeros((2, 512, 2, 2)), batch_stats=True)
    with pytest.raises(RuntimeError, match="Bottleneck training is not built"):
        nets.basic_block_train(nets.Bottleneck(256, 64, 1), torch.zeros((1, 256, 2, 2)), batch_stats=True)
    # without the flag the call is today's: the device check alone
    with pytest.raises(ValueError, match="CUDA"):
        nets.basic_block_train(blk, torch.zeros((2, 512, 2, 2)))


def test_forward_padded_flag_is_the_layer4_node_only():
    trunk = nets.make_trunk("resnet18")
    fpn, head = nets.FeaturePyramidNetwork(512), nets.DBHead(256)
    taps = [torch.zeros((1, 4, 4, 64), dtype=torch.float16), torch.zeros((1, 3, 3, 128), dtype=torch.float16)]
    with pytest.raises(ValueError, match="layer4 only"):
        fpn.forward_padded(taps, head=head, layer4=trunk[7], layer3=trunk[6], trunk_batch_stats=True)
    with pytest.raises(ValueError, match="layer4 only"):
        fpn.forward_padded(taps, head=head, layer4=trunk[7], layer3=trunk[6], layer2=trunk[5], trunk_batch_stats=True)
    with pytest.raises(ValueError, match="layer4 only"):
        fpn.forward_padded(taps, head=head, trunk_batch_stats=True)
    # the node itself goes on to its own checks: CPU taps are refused as without the flag
    with pytest.raises(ValueError, match="CUDA"):
        fpn.forward_padded(taps + [torch.zeros((1, 4, 4, 256), dtype=torch.float16)], head=head, layer4=trunk[7], trunk_batch_stats=True)
