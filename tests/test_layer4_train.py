"""Backward into the trunk taps, first stage (csrc/fpn_train.hip: vtd_fpn_train_backward_input), without a device: the new C entry points
exist and refuse bad arguments before any launch, the workspace query, the API's refusals, and the fp64 input gradients written out as the
kernels compute them (per level one GEMM with the lateral's transposed weights on the sum-pooled dL(k)) against torch autograd of the
reference wiring -- with negative controls that must miss autograd by at least 10x the GPU tests' bound."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vtd_amd import _native, nets

# the GPU tests' bounds on dC2..dC5 (tests/test_gpu_layer4_train.py) and the shapes of their cases: (n, c5 channels, h5, w5)
BOUNDS = {"input_resnet18": 9.1e-4, "input_resnet50": 8.9e-4}
GPU_CASES = {"input_resnet18": [(2, 512, 3, 2), (2, 512, 1, 1), (2, 512, 5, 4)], "input_resnet50": [(2, 2048, 3, 2), (2, 2048, 1, 1), (2, 2048, 5, 4)]}


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _aligned(nbytes, align=256):
    raw = (C.c_char * (nbytes + 2 * align))()
    return raw, C.c_void_p((C.addressof(raw) + align - 1) // align * align)


def _params(buf):
    st = _native.FpnParams()
    for i in range(4):
        st.inner_w[i] = buf
        st.inner_b[i] = buf
    st.layer_w = buf
    st.layer_b = buf
    return st


# ---- C ABI, no device
def test_new_symbols_are_exported_and_bound():
    lib = _native.load()
    for name in ("vtd_fpn_train_input_workspace_bytes", "vtd_fpn_train_backward_input", "vtd_fpn_train_unpack_tap_grad"):
        assert name in _native.SIGNATURES and hasattr(lib, name), name


def test_input_workspace_query():
    lib = _native.load()
    ws, wsi = lib.vtd_fpn_train_workspace_bytes, lib.vtd_fpn_train_input_workspace_bytes
    a256 = lambda x: (x + 255) // 256 * 256  # noqa: E731
    for c5 in (512, 2048):
        for n, h5, w5 in ((1, 1, 1), (2, 3, 2), (2, 5, 4), (32, 20, 20)):
            # the backward's scratch, then the four transposed weight panels and a zero bias row
            want = ws(n, h5, w5, c5, 1) + sum(a256((c5 >> k) * 256 * 2) for k in range(4)) + a256(c5 * 4)
            assert wsi(n, h5, w5, c5) == want, (n, h5, w5, c5)
    for bad in ((0, 3, 2, 512), (2, 0, 2, 512), (2, 3, -1, 512), (2, 3, 2, 0), (2, 3, 2, 256), (2, 3, 2, 768), (2, 3, 2, 8192), (2, 3, 2, 520),
                (1 << 15, 1 << 8, 1 << 8, 512), (128, 40, 40, 512)):
        assert wsi(*bad) == -2902, bad
    # the existing query keeps its two modes
    assert ws(2, 3, 2, 512, 2) == -2902


def test_backward_input_argument_and_alignment_errors():
    lib = _native.load()
    keep = [_aligned(4096) for _ in range(4)]
    scratch, w, out, dscale = (k[1] for k in keep)
    st = _params(w)
    sp = C.byref(st)
    outs = _native.FpnTaps(out, out, out, out)
    op = C.byref(outs)
    bwi = lib.vtd_fpn_train_backward_input
    # every refusal comes before any launch, so none of this needs a device
    assert bwi(2, 3, 2, 512, None, scratch, 15, op, dscale, None) == -2902
    assert bwi(2, 3, 2, 512, sp, None, 15, op, dscale, None) == -2902
    assert bwi(2, 3, 2, 512, sp, scratch, 15, None, dscale, None) == -2902
    assert bwi(2, 3, 2, 512, sp, scratch, 15, op, None, None) == -2902
    for mask in (0, 16, -1):
        assert bwi(2, 3, 2, 512, sp, scratch, mask, op, dscale, None) == -2902
    for n, h, wd, c5 in ((0, 3, 2, 512), (2, 0, 2, 512), (2, 3, -1, 512), (2, 3, 2, 640), (2, 3, 2, 64), (1 << 15, 1 << 8, 1 << 8, 512)):
        assert bwi(n, h, wd, c5, sp, scratch, 15, op, dscale, None) == -2902
    # a requested level needs its destination and its lateral's weights; level lv reads inner_w[3 - lv]
    missing = _native.FpnTaps(out, out, None, out)
    assert bwi(2, 3, 2, 512, sp, scratch, 4, C.byref(missing), dscale, None) == -2902
    bad = _params(w)
    bad.inner_w[0] = None
    assert bwi(2, 3, 2, 512, C.byref(bad), scratch, 8, op, dscale, None) == -2902
    bad = _params(w)
    bad.inner_w[3] = C.c_void_p(w.value + 2)
    assert bwi(2, 3, 2, 512, C.byref(bad), scratch, 1, op, dscale, None) == -2902
    assert bwi(2, 3, 2, 512, sp, C.c_void_p(scratch.value + 128), 15, op, dscale, None) == -2903
    assert bwi(2, 3, 2, 512, sp, scratch, 15, op, C.c_void_p(dscale.value + 4), None) == -2903
    odd = _native.FpnTaps(out, C.c_void_p(out.value + 8), out, out)
    assert bwi(2, 3, 2, 512, sp, scratch, 2, C.byref(odd), dscale, None) == -2903
    un = lib.vtd_fpn_train_unpack_tap_grad
    assert un(None, dscale, 2, 64, 4, 4, out, None) == -2902 and un(w, None, 2, 64, 4, 4, out, None) == -2902
    assert un(w, dscale, 2, 64, 4, 4, None, None) == -2902
    for n, ch, h, wd in ((0, 64, 4, 4), (1 << 16, 64, 4, 4), (2, 0, 4, 4), (2, 72, 4, 4), (2, 8192, 4, 4), (2, 64, 0, 4), (2, 64, 4, -1)):
        assert un(w, dscale, n, ch, h, wd, out, None) == -2902
    assert un(C.c_void_p(w.value + 8), dscale, 2, 64, 4, 4, out, None) == -2903
    assert un(w, C.c_void_p(dscale.value + 4), 2, 64, 4, 4, out, None) == -2903
    assert un(w, dscale, 2, 64, 4, 4, C.c_void_p(out.value + 2), None) == -2903


# ---- API
def _feats(n, c5, h5, w5, gen=None):
    return [torch.randn((n, c5 >> (3 - lv), h5 << (3 - lv), w5 << (3 - lv)), generator=gen) for lv in range(4)]


def test_input_grad_is_an_explicit_request():
    fpn = nets.FeaturePyramidNetwork(512)
    feats = _feats(1, 512, 2, 1)
    feats[3].requires_grad_(True)
    with pytest.raises(RuntimeError, match="backward into the trunk is not built"):     # the plain call refuses as before
        fpn(feats)
    with pytest.raises(ValueError, match="CUDA"):      # with the request the call goes on to the device check: there is no CPU path
        fpn(feats, input_grad=True)
    with pytest.raises(ValueError, match="doublings"):
        fpn(feats[:2] + [torch.randn((1, 256, 5, 2)), feats[3]], input_grad=True)


# ---- the input gradients as the kernels form them, against autograd of the reference wiring
def _wiring(fpn, feats):
    last = fpn.inner_blocks[0](feats[3])
    for i in range(1, 4):
        last = fpn.inner_blocks[i](feats[3 - i]) + F.interpolate(last, scale_factor=2, mode="nearest")
    return fpn.layer_blocks[3](last)


def _input_grads_as_the_kernels_form_them(fpn, dp2, bug=None):
    """dC2..dC5 from dP2 [n,256,H,W] in fp64: dL2 = conv3x3^T(dP2), dL(k+1) = sumpool2x2(dL(k)), dC(k) = inner_blocks[5-k].weight^T dL(k)
    (a GEMM over the pixels, K = 256).  `bug` injects a kernel-style mistake."""
    dl = F.conv2d(dp2, fpn.layer_blocks[3].weight.detach().transpose(0, 1).flip(-1, -2), padding=1)
    out = []
    for lv in range(4):
        if lv:
            dl = F.avg_pool2d(dl, 2) * (1.0 if bug == "average_pool" else 4.0)
        src = dp2 if bug == "reads_dp2" and lv == 0 else dl
        w = fpn.inner_blocks[lv if bug == "lateral_order_reversed" else 3 - lv].weight.detach()[:, :, 0, 0]     # [256][C]
        if bug == "weights_not_transposed" and w.shape[1] == 256:
            w = w.t()
        g = torch.einsum("nohw,oc->nchw", src, w)
        out.append(g * 2.0 if bug == "scale_not_undone" else g)
    return out


def _case(n, c5, h5, w5, seed=4):
    gen = torch.Generator().manual_seed(seed)
    fpn = nets.FeaturePyramidNetwork(c5)
    fpn.load_state_dict(nets.seeded_state_dict(lambda: nets.FeaturePyramidNetwork(c5), 8))
    fpn = fpn.double()
    feats = [(t * 0.5).half().double().requires_grad_(True) for t in _feats(n, c5, h5, w5, gen)]
    dp2 = torch.randn((n, 256, 8 * h5, 8 * w5), generator=gen).double()
    _wiring(fpn, feats).backward(dp2)
    return fpn, dp2, [t.grad.detach() for t in feats]


ALL_CASES = [(k, shp) for k in sorted(GPU_CASES) for shp in GPU_CASES[k]]


@pytest.mark.parametrize("case,shape", ALL_CASES)
def test_written_out_input_gradients_match_autograd(case, shape):
    fpn, dp2, want = _case(*shape)
    got = _input_grads_as_the_kernels_form_them(fpn, dp2)
    for lv in range(4):
        assert got[lv].shape == want[lv].shape
        assert _rel(got[lv].numpy(), want[lv].numpy()) <= 1e-12, lv


@pytest.mark.parametrize("bug", ["average_pool", "reads_dp2", "lateral_order_reversed", "weights_not_transposed", "scale_not_undone"])
@pytest.mark.parametrize("case,shape", ALL_CASES)
def test_negative_controls_are_rejected_by_ten_times_the_bound(bug, case, shape):
    fpn, dp2, want = _case(*shape)
    try:
        got = _input_grads_as_the_kernels_form_them(fpn, dp2, bug)
    except RuntimeError:     # a reversed lateral order multiplies tensors whose shapes do not fit: that alone is a miss of 100 %
        assert bug == "lateral_order_reversed"
        return
    errs = [(_rel(got[lv].numpy(), want[lv].numpy()) if got[lv].shape == want[lv].shape else 1.0) for lv in range(4)]
    assert max(errs) >= 10 * BOUNDS[case], f"{bug}: error {max(errs):.3g} is not 10x the bound {BOUNDS[case]}"


# ---- BasicBlock training (csrc/resblock_train.hip), without a device.  The written-out references below are torch restatements checked
# against autograd: they test the formulas and the controls, not the kernels (tests/test_gpu_layer4_train.py does that).  They run on
# reduced channel counts (6 -> 5 and 8 instead of 256 / 512) at the GPU tests' spatial sizes: a relative L2 miss of a wrong formula does
# not depend on the width, and fp64 autograd of a 512-wide 3x3 block per control would take most of the CPU suite's time.
def test_basicblock_symbols_errors_and_workspace():
    lib = _native.load()
    for name in ("vtd_basicblock_train_workspace_bytes", "vtd_basicblock_train_forward", "vtd_basicblock_train_backward"):
        assert name in _native.SIGNATURES and hasattr(lib, name), name
    for code in (-3001, -3002, -3003):
        assert b"BasicBlock training" in lib.vtd_strerror(code)
    assert b"stride-2" in lib.vtd_strerror(-3003)
    ws = lib.vtd_basicblock_train_workspace_bytes
    for geom in ((2, 6, 4, 256, 512, 2), (2, 3, 2, 512, 512, 1), (32, 40, 40, 256, 512, 2), (32, 20, 20, 512, 512, 1)):
        assert ws(*geom, 0) > 0 and ws(*geom, 1) > 0 and ws(*geom, 0) % 256 == 0
    # every other geometry is refused: other widths, stride 2 without the 256 -> 512 plan, odd extents, an unknown mode
    for bad in ((2, 6, 4, 128, 256, 2), (2, 6, 4, 256, 512, 1), (2, 6, 4, 512, 512, 2), (2, 5, 4, 256, 512, 2), (2, 6, 3, 256, 512, 2),
                (0, 6, 4, 256, 512, 2), (2, 0, 4, 512, 512, 1), (2, 3, 2, 512, 2048, 1), (2, 3, 2, 64, 64, 1)):
        assert ws(*bad, 0) == -3001, bad
    assert ws(2, 3, 2, 512, 512, 1, 2) == -3001
    keep = [_aligned(4096) for _ in range(3)]
    a, b, c = (k[1] for k in keep)
    st = _native.BasicBlockParams(*([a] * 15))
    fwd, bwd = lib.vtd_basicblock_train_forward, lib.vtd_basicblock_train_backward
    sp = C.byref(st)
    # refusals come before any launch
    assert fwd(None, 2, 3, 2, 512, 512, 1, sp, 1e-5, b, c, None) == -3001
    assert fwd(a, 2, 3, 2, 512, 512, 1, None, 1e-5, b, c, None) == -3001
    assert fwd(a, 2, 3, 2, 128, 128, 1, sp, 1e-5, b, c, None) == -3001
    assert fwd(a, 2, 3, 2, 512, 512, 1, sp, 0.0, b, c, None) == -3001
    assert fwd(a, 2, 3, 2, 512, 512, 1, sp, 1e-5, C.c_void_p(b.value + 128), c, None) == -3002
    nods = _native.BasicBlockParams(*([a] * 10))
    assert fwd(a, 2, 6, 4, 256, 512, 2, C.byref(nods), 1e-5, b, c, None) == -3001      # the stride-2 block needs its downsample
    assert bwd(a, 2, 6, 4, 256, 512, 2, sp, 1e-5, b, c, a, a, sp, b, c, a, None) == -3003   # no input gradient for the stride-2 block
    assert bwd(a, 2, 3, 2, 512, 512, 1, sp, 1e-5, b, c, a, a, sp, b, c, None, None) == -3001     # dx without a place for its scale
    assert bwd(a, 2, 3, 2, 512, 512, 1, sp, 1e-5, b, c, a, C.c_void_p(a.value + 4), sp, b, None, None, None) == -3002
    assert bwd(a, 2, 3, 2, 512, 512, 1, sp, 1e-5, b, c, None, a, sp, b, None, None, None) == -3001


def test_basicblock_call_refusals():
    with pytest.raises(ValueError, match="CUDA"):
        nets.BasicBlock(512, 512, 1)(torch.zeros((1, 512, 2, 2)))
    with pytest.raises(ValueError, match="must be a"):
        nets.BasicBlock(512, 512, 1)(torch.zeros((1, 256, 2, 2)))
    with pytest.raises(RuntimeError, match="parameter containers"):
        nets.Bottleneck(256, 64, 1)(torch.zeros((1, 256, 2, 2)))


def _conv_bn_case(stride, ksz, seed=3):
    gen = torch.Generator().manual_seed(seed)
    cin, cout = 6, 5
    x = torch.randn((2, cin, 6, 4), generator=gen).double()
    w = torch.randn((cout, cin, ksz, ksz), generator=gen).double().requires_grad_(True)
    gam = torch.tensor([1.3, 0.0, -0.75, 0.4, 2.0]).double().requires_grad_(True)      # a gamma = 0 channel and a gamma < 0 channel
    bet = torch.randn(cout, generator=gen).double().requires_grad_(True)
    mean, var = torch.randn(cout, generator=gen).double(), (torch.rand(cout, generator=gen) + 0.5).double()
    y = F.batch_norm(F.conv2d(x, w, None, stride, ksz // 2), mean, var, gam, bet, False, 0.0, 1e-5)
    g = torch.randn(y.shape, generator=gen).double()
    y.backward(g)
    return x, w, gam, bet, mean, var, g


def _identities(x, w, gam, mean, var, g, stride, ksz, bug=None):
    """dW, dbeta, dgamma as csrc/resblock_train.hip forms them: G = g^T im2col(x) (the gather at `stride`), s = sum g."""
    cout = w.shape[0]
    cols = F.unfold(x, ksz, padding=ksz // 2, stride=1 if bug == "stride2_gather_at_stride1" else stride)      # [n][cin k k][pix]
    if bug == "stride2_gather_at_stride1":
        cols = cols[:, :, :g.shape[2] * g.shape[3]]
    G = torch.einsum("ncp,nkp->ck", g.reshape(g.shape[0], cout, -1), cols)
    s = g.sum((0, 2, 3))
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    wd = w.detach().reshape(cout, -1)
    dgam = rstd * ((wd * G).sum(1) - (0.0 if bug == "dgamma_without_mean" else mean * s))
    return (gam.detach() * rstd)[:, None] * G, s, dgam


@pytest.mark.parametrize("stride,ksz", [(1, 3), (2, 3), (2, 1)])
def test_conv_bn_identities_match_autograd(stride, ksz):
    x, w, gam, bet, mean, var, g = _conv_bn_case(stride, ksz)
    dw, dbet, dgam = _identities(x, w, gam, mean, var, g, stride, ksz)
    assert _rel(dw.numpy(), w.grad.reshape(w.shape[0], -1).numpy()) <= 1e-12
    assert _rel(dbet.numpy(), bet.grad.numpy()) <= 1e-12 and _rel(dgam.numpy(), gam.grad.numpy()) <= 1e-12
    assert float(gam.grad[1].abs()) > 0 and float(w.grad[1].abs().max()) == 0      # gamma = 0: dW vanishes, dgamma does not


# the GPU tests' gradient bound for the blocks (tests/test_gpu_layer4_train.py BLOCK_BOUNDS)
BLOCK_GRAD_BOUND = 9.6e-4


@pytest.mark.parametrize("bug", ["stride2_gather_at_stride1", "dgamma_without_mean"])
def test_conv_bn_negative_controls(bug):
    x, w, gam, bet, mean, var, g = _conv_bn_case(2, 3)
    dw, _, dgam = _identities(x, w, gam, mean, var, g, 2, 3, bug)
    err = max(_rel(dw.numpy(), w.grad.reshape(5, -1).numpy()), _rel(dgam.numpy(), gam.grad.numpy()))
    assert err >= 10 * BLOCK_GRAD_BOUND, f"{bug}: {err:.3g}"


def _block_ref(x, p, bug=None):
    """The stride-1 block in fp64 with frozen statistics, written out with explicit masks so a mistake can be injected in the backward."""
    f = lambda w, bn: w * (bn[0] / torch.sqrt(bn[3] + 1e-5))[:, None, None, None]  # noqa: E731
    sh = lambda bn: (bn[1] - bn[2] * bn[0] / torch.sqrt(bn[3] + 1e-5))[None, :, None, None]  # noqa: E731
    w1, w2 = f(p["w1"], p["bn1"]), f(p["w2"], p["bn2"])
    a1 = F.relu(F.conv2d(x, w1, padding=1) + sh(p["bn1"]))
    y = F.relu(F.conv2d(a1, w2, padding=1) + sh(p["bn2"]) + x)

    def dx_from(dy):
        g2 = dy if bug == "relu_mask_left_out" else dy * (y > 0)
        wt = w2.transpose(0, 1) if bug == "unrotated_dgrad" else w2.transpose(0, 1).flip(-1, -2)
        g1 = F.conv2d(g2, wt, padding=1) * (a1 > 0)
        dx = F.conv2d(g1, w1.transpose(0, 1).flip(-1, -2), padding=1)
        return dx if bug == "identity_dropped" else dx + g2
    return y, dx_from


@pytest.mark.parametrize("bug", [None, "relu_mask_left_out", "identity_dropped", "unrotated_dgrad"])
def test_block_input_gradient_written_out(bug):
    gen = torch.Generator().manual_seed(5)
    c = 8
    bn = lambda: [1 + 0.3 * torch.randn(c, generator=gen).double(), torch.randn(c, generator=gen).double() * 0.1,  # noqa: E731
                  torch.randn(c, generator=gen).double() * 0.05, (1 + 0.2 * torch.rand(c, generator=gen)).double()]
    p = {"w1": torch.randn((c, c, 3, 3), generator=gen).double() * 0.2, "w2": torch.randn((c, c, 3, 3), generator=gen).double() * 0.2, "bn1": bn(), "bn2": bn()}
    x = torch.randn((2, c, 5, 4), generator=gen).double().requires_grad_(True)
    y, dx_from = _block_ref(x, p, bug)
    dy = torch.randn(y.shape, generator=gen).double()
    y.backward(dy)
    err = _rel(dx_from(dy).detach().numpy(), x.grad.numpy())
    if bug is None:
        assert err <= 1e-12
    else:
        assert err >= 10 * BLOCK_GRAD_BOUND, f"{bug}: {err:.3g}"


# ---- the product mode
def test_head_fpn_layer4_mode():
    net = nets.DBNet("resnet18", trainable="head+fpn+layer4")
    assert net.trainable == "head+fpn+layer4"
    for i in range(7):
        assert not any(p.requires_grad for p in net.backbone[i].parameters()), i
    for m in (net.backbone[7], net.fpn, net.head):
        assert all(p.requires_grad for p in m.parameters())
    assert len(list(net.backbone[7].parameters())) == 15
    # Bottleneck training is not built
    with pytest.raises(ValueError, match="Bottleneck training is not built"):
        nets.DBNet("resnet50", trainable="head+fpn+layer4")
    with pytest.raises(ValueError, match="Bottleneck training is not built"):
        nets.DBNet("resnet50").set_trainable("head+fpn+layer4")
    for mode in ("layer4", "head+layer4", "head+fpn+layer3", "all"):
        with pytest.raises(ValueError, match="trainable"):
            nets.DBNet("resnet18", trainable=mode)
    # the state dict is the reference's, whatever the mode
    assert list(net.state_dict()) == list(nets.DBNet("resnet18").state_dict())
    # switching from a narrower mode turns layer4 back on; the narrower modes behave as before
    net2 = nets.DBNet("resnet18", trainable="head+fpn")
    assert not any(p.requires_grad for p in net2.backbone.parameters())
    net2.set_trainable("head+fpn+layer4")
    assert all(p.requires_grad for p in net2.backbone[7].parameters()) and not any(p.requires_grad for p in net2.backbone[6].parameters())
    # the eval-mode rebuild is keyed on layer4's tensors too (15 parameters, 5 BatchNorms x 3 buffers)
    assert len(net._head_tensor_versions()) == len(nets.DBNet("resnet18", trainable="head+fpn")._head_tensor_versions()) + 30
    # a frozen trunk tensor that requires grad is refused in a train-mode forward, before anything touches a device
    net.backbone[4][0].conv1.weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match="backward below layer4 is not"):
        net.train()(torch.zeros((1, 3, 640, 640)))
    with pytest.raises(RuntimeError, match="Bottleneck training is not built"):
        nets._stage_operands(nets._STAGES[3], nets.make_trunk("resnet50")[7], torch.zeros((1, 4, 4, 256)))
