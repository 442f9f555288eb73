"""FPN training (csrc/fpn_train.hip) without a device: argument checks of the new C entry points, the workspace-size query, the API's
refusals, and the fp64 backward written out as the kernels compute it (rotated and transposed 3x3, the sum-pool chain, per-level 1x1
weight gradients) against torch autograd of the reference wiring -- with negative controls that must miss autograd by at least 10x the
GPU tests' bound."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vtd_amd import _native, nets

# the GPU tests' gradient bounds (tests/test_gpu_fpn_neck_train.py) and the shapes of their cases: (n, c5 channels, h5, w5)
BOUNDS = {"alone_resnet18": 1.2e-3, "alone_resnet50": 1.2e-3, "chain_resnet18": 2.4e-3, "chain_resnet50": 3.1e-3}
GPU_CASES = {"alone_resnet18": (2, 512, 5, 4), "alone_resnet50": (2, 2048, 1, 1), "chain_resnet18": (2, 512, 3, 2), "chain_resnet50": (2, 2048, 3, 2)}


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


# ---- C ABI, no device
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


def test_error_strings():
    lib = _native.load()
    assert b"fuse_fpn_head=0" in lib.vtd_strerror(-2901)
    assert b"FPN training" in lib.vtd_strerror(-2902) and b"argument" in lib.vtd_strerror(-2902)
    assert b"FPN training" in lib.vtd_strerror(-2903) and b"misaligned" in lib.vtd_strerror(-2903)


def test_workspace_query():
    lib = _native.load()
    ws = lib.vtd_fpn_train_workspace_bytes
    a256 = lambda x: (x + 255) // 256 * 256  # noqa: E731
    for c5 in (512, 2048):
        for mode in (0, 1):
            sizes = [ws(n, 3, 2, c5, mode) for n in (1, 2, 3, 5, 8, 32)]
            assert all(s > 0 and s % 256 == 0 for s in sizes), (c5, mode, sizes)
            assert all(b > a for a, b in zip(sizes, sizes[1:])), (c5, mode, sizes)
    # mode 0 = the four padded laterals, the five weight panels and the bias rows
    n, h5, w5, c5 = 2, 3, 2, 512
    want = sum(a256(n * ((h5 << k) + 2) * ((w5 << k) + 2) * 256 * 2) for k in range(4)) + sum(a256(256 * (c5 >> k) * 2) for k in range(4))
    assert ws(n, h5, w5, c5, 0) == want + 256 * 2304 * 2 + 5 * 256 * 4
    # the product shape fits
    assert ws(32, 20, 20, 2048, 0) > 0 and ws(32, 20, 20, 2048, 1) > 0
    for bad in ((0, 3, 2, 512), (2, 0, 2, 512), (2, 3, -1, 512), (2, 3, 2, 0), (2, 3, 2, 256), (2, 3, 2, 768), (2, 3, 2, 8192), (2, 3, 2, 520),
                (1 << 15, 1 << 8, 1 << 8, 512), (128, 40, 40, 512)):
        for mode in (0, 1):
            assert ws(*bad, mode) == -2902, bad
    assert ws(2, 3, 2, 512, 2) == -2902 and ws(2, 3, 2, 512, -1) == -2902


def test_forward_and_backward_argument_and_alignment_errors():
    lib = _native.load()
    keep = [_aligned(4096) for _ in range(6)]
    ws, p2, w, tap, dp2, dscale = (k[1] for k in keep)
    st, gst = _params(w), _params(w)
    taps = _native.FpnTaps(tap, tap, tap, tap)
    fwd, bwd = lib.vtd_fpn_train_forward, lib.vtd_fpn_train_backward
    tp, sp, gp = C.byref(taps), C.byref(st), C.byref(gst)
    # every refusal comes before any launch, so none of this needs a device
    assert fwd(None, 2, 3, 2, 512, sp, ws, p2, None) == -2902
    assert fwd(tp, 2, 3, 2, 512, None, ws, p2, None) == -2902
    assert fwd(tp, 2, 3, 2, 512, sp, None, p2, None) == -2902
    assert fwd(tp, 2, 3, 2, 512, sp, ws, None, None) == -2902
    for n, h, wd, c5 in ((0, 3, 2, 512), (2, 0, 2, 512), (2, 3, -1, 512), (2, 3, 2, 640), (2, 3, 2, 64), (1 << 15, 1 << 8, 1 << 8, 512)):
        assert fwd(tp, n, h, wd, c5, sp, ws, p2, None) == -2902
        assert bwd(tp, n, h, wd, c5, sp, ws, dp2, dscale, gp, ws, None) == -2902
    for field in ("layer_w", "layer_b"):
        bad = _params(w)
        setattr(bad, field, None)
        assert fwd(tp, 2, 3, 2, 512, C.byref(bad), ws, p2, None) == -2902
        assert bwd(tp, 2, 3, 2, 512, sp, ws, dp2, dscale, C.byref(bad), ws, None) == -2902
    bad = _params(w)
    bad.inner_w[2] = None
    assert fwd(tp, 2, 3, 2, 512, C.byref(bad), ws, p2, None) == -2902
    bad = _params(w)
    bad.inner_b[1] = C.c_void_p(w.value + 2)            # a float pointer that is not 4-byte aligned
    assert fwd(tp, 2, 3, 2, 512, C.byref(bad), ws, p2, None) == -2902
    assert bwd(tp, 2, 3, 2, 512, sp, ws, dp2, dscale, C.byref(bad), ws, None) == -2902
    missing = _native.FpnTaps(tap, tap, None, tap)
    assert fwd(C.byref(missing), 2, 3, 2, 512, sp, ws, p2, None) == -2902
    assert bwd(C.byref(missing), 2, 3, 2, 512, sp, ws, dp2, dscale, gp, ws, None) == -2902
    odd = _native.FpnTaps(tap, C.c_void_p(tap.value + 8), tap, tap)
    assert fwd(C.byref(odd), 2, 3, 2, 512, sp, ws, p2, None) == -2903
    assert bwd(C.byref(odd), 2, 3, 2, 512, sp, ws, dp2, dscale, gp, ws, None) == -2903
    assert fwd(tp, 2, 3, 2, 512, sp, C.c_void_p(ws.value + 128), p2, None) == -2903
    assert fwd(tp, 2, 3, 2, 512, sp, ws, C.c_void_p(p2.value + 8), None) == -2903
    assert bwd(tp, 2, 3, 2, 512, sp, None, dp2, dscale, gp, ws, None) == -2902
    assert bwd(tp, 2, 3, 2, 512, sp, ws, None, dscale, gp, ws, None) == -2902
    assert bwd(tp, 2, 3, 2, 512, sp, ws, dp2, None, gp, ws, None) == -2902
    assert bwd(tp, 2, 3, 2, 512, sp, ws, dp2, dscale, None, ws, None) == -2902
    assert bwd(tp, 2, 3, 2, 512, sp, ws, dp2, dscale, gp, None, None) == -2902
    assert bwd(tp, 2, 3, 2, 512, None, ws, dp2, dscale, gp, ws, None) == -2902
    assert bwd(tp, 2, 3, 2, 512, sp, C.c_void_p(ws.value + 128), dp2, dscale, gp, ws, None) == -2903
    assert bwd(tp, 2, 3, 2, 512, sp, ws, dp2, dscale, gp, C.c_void_p(ws.value + 128), None) == -2903
    assert bwd(tp, 2, 3, 2, 512, sp, ws, C.c_void_p(dp2.value + 8), dscale, gp, ws, None) == -2903
    assert bwd(tp, 2, 3, 2, 512, sp, ws, dp2, C.c_void_p(dscale.value + 4), gp, ws, None) == -2903


def test_layout_entry_points_argument_and_alignment_errors():
    lib = _native.load()
    keep = [_aligned(4096) for _ in range(2)]
    a, b = (k[1] for k in keep)
    pack = lib.vtd_fpn_train_pack_tap
    assert pack(None, 0, 2, 64, 4, 4, b, None) == -2902 and pack(a, 0, 2, 64, 4, 4, None, None) == -2902
    for n, ch, h, w in ((0, 64, 4, 4), (2, 0, 4, 4), (2, 72, 4, 4), (2, 8192, 4, 4), (2, 64, 0, 4), (2, 64, 4, -1), (1 << 12, 512, 1 << 10, 1 << 10)):
        assert pack(a, 0, n, ch, h, w, b, None) == -2902
    assert pack(a, 2, 2, 64, 4, 4, b, None) == -2902        # dtype
    assert pack(a, 0, 2, 64, 4, 4, C.c_void_p(b.value + 8), None) == -2903
    un = lib.vtd_fpn_train_unpack_p2
    assert un(None, 2, 4, 4, b, None) == -2902 and un(a, 2, 4, 4, None, None) == -2902 and un(a, 0, 4, 4, b, None) == -2902
    assert un(a, 2, 4, 0, b, None) == -2902 and un(a, 1 << 16, 4, 4, b, None) == -2902
    assert un(C.c_void_p(a.value + 8), 2, 4, 4, b, None) == -2903 and un(a, 2, 4, 4, C.c_void_p(b.value + 2), None) == -2903
    pg = lib.vtd_fpn_train_pack_grad
    assert pg(None, 2, 4, 4, b, None) == -2902 and pg(a, 2, 4, 4, None, None) == -2902 and pg(a, 2, 0, 4, b, None) == -2902
    assert pg(a, 1 << 16, 4, 4, b, None) == -2902
    assert pg(C.c_void_p(a.value + 2), 2, 4, 4, b, None) == -2903 and pg(a, 2, 4, 4, C.c_void_p(b.value + 8), None) == -2903
    # the trunk export refuses a missing handle or buffer before it touches anything
    ft = lib.vtd_detector_forward_trunk
    assert ft(None, 1, a, a, a, a, None) != 0


# ---- API
def test_head_fpn_mode_is_accepted_and_the_old_names_are_not():
    net = nets.DBNet("resnet18", trainable="head+fpn")
    assert net.trainable == "head+fpn"
    assert not any(p.requires_grad for p in net.backbone.parameters())
    assert all(p.requires_grad for p in net.fpn.parameters()) and all(p.requires_grad for p in net.head.parameters())
    for mode in ("fpn_head", "fpn", "all"):
        with pytest.raises(ValueError, match="trainable"):
            nets.DBNet("resnet18", trainable=mode)
    # "head" still freezes the FPN, and None leaves everything alone
    assert not any(p.requires_grad for p in nets.DBNet("resnet18", trainable="head").fpn.parameters())
    assert all(p.requires_grad for p in nets.DBNet("resnet18").backbone.parameters())
    # the versions the eval-mode rebuild is keyed on include the FPN's tensors in the new mode only
    assert len(net._head_tensor_versions()) == len(nets.DBNet("resnet18", trainable="head")._head_tensor_versions()) + 16


def _feats(n, c5, h5, w5, gen=None):
    return [torch.randn((n, c5 >> (3 - lv), h5 << (3 - lv), w5 << (3 - lv)), generator=gen) for lv in range(4)]


def test_fpn_call_refusals():
    fpn = nets.FeaturePyramidNetwork(512)
    good = _feats(1, 512, 2, 1)
    with pytest.raises(ValueError, match="CUDA"):
        fpn(good)
    with pytest.raises(ValueError, match="four"):
        fpn(good[:3])
    with pytest.raises(ValueError, match="four"):
        fpn(good[0])
    bad = list(good)
    bad[0] = torch.randn((1, 128, 16, 8))
    with pytest.raises(ValueError, match="channels"):
        fpn(bad)
    with pytest.raises(ValueError, match="channels"):      # the lateral index order: inner_blocks[0] reads C5, not C2
        fpn(good[::-1])
    bad = list(good)
    bad[1] = torch.randn((1, 128, 8, 5))
    with pytest.raises(ValueError, match="doublings"):
        fpn(bad)
    bad = list(good)
    bad[2] = torch.randn((2, 256, 4, 2))
    with pytest.raises(ValueError, match="doublings"):
        fpn(bad)
    bad = list(good)
    bad[3] = bad[3].clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="backward into the trunk is not built"):
        fpn(bad)
    with pytest.raises(ValueError, match="multiple of 512"):
        nets.FeaturePyramidNetwork(256)([torch.randn((1, 256 >> (3 - lv), 1 << (3 - lv), 1 << (3 - lv))) for lv in range(4)])
    with pytest.raises(ValueError, match="padded taps"):
        fpn.forward_padded(good)


# ---- the backward as the kernels compute it, against autograd of the reference wiring
def _wiring(fpn, feats):
    last = fpn.inner_blocks[0](feats[3])
    for i in range(1, 4):
        last = fpn.inner_blocks[i](feats[3 - i]) + F.interpolate(last, scale_factor=2, mode="nearest")
    return fpn.layer_blocks[3](last)


def _lateral_l2(fpn, feats):
    last = fpn.inner_blocks[0](feats[3])
    for i in range(1, 4):
        last = fpn.inner_blocks[i](feats[3 - i]) + F.interpolate(last, scale_factor=2, mode="nearest")
    return last


def _backward_as_the_kernels_form_it(fpn, feats, dp2, bug=None):
    """The ten gradients from dP2 [n,256,H,W] in fp64, step by step as csrc/fpn_train.hip forms them.  `bug` injects a kernel-style
    mistake.  Returns {state-dict key: gradient}."""
    w3 = fpn.layer_blocks[3].weight.detach()
    l2 = _lateral_l2(fpn, feats).detach()
    n = dp2.shape[0]
    # 3x3 weight gradient: dW[co][ci][tap] = sum_pix dP2[pix][co] L2[pix + tap][ci] (im2col of the zero-padded L2), bias = sum_pix dP2
    cols = F.unfold(l2, 3, padding=1).reshape(n, 256, 9, -1)                  # [n][ci][tap][pix]
    dw3 = torch.einsum("nop,nctp->oct", dp2.reshape(n, 256, -1), cols).reshape(256, 256, 3, 3)
    out = {"layer_blocks.3.weight": dw3, "layer_blocks.3.bias": dp2.sum((0, 2, 3))}
    # dL2 = conv3x3^T(dP2): the window rotated by 180 degrees, the weights transposed
    wd = w3.transpose(0, 1)
    if bug != "unrotated_taps":
        wd = wd.flip(-1, -2)
    dl = F.conv2d(dp2, wd, padding=1)
    for lv in range(4):      # level 2 + lv reads C(2 + lv) and belongs to inner_blocks[3 - lv]
        if lv:
            if bug == "top_down_left_out":
                dl = torch.zeros_like(F.avg_pool2d(dl, 2))
            else:
                dl = F.avg_pool2d(dl, 2) * (1.0 if bug == "average_pool" else 4.0)      # the 2x2 sum-pool: the adjoint of nearest-2x
        idx = lv if bug == "lateral_order_reversed" else 3 - lv
        x = feats[lv]
        dw = torch.einsum("nop,ncp->oc", dl.reshape(n, 256, -1), x.reshape(n, x.shape[1], -1))
        out[f"inner_blocks.{idx}.weight"] = dw.reshape(256, -1, 1, 1)
        out[f"inner_blocks.{idx}.bias"] = dl.sum((0, 2, 3))
    return out


def _case(case, seed=4):
    n, c5, h5, w5 = GPU_CASES[case]
    gen = torch.Generator().manual_seed(seed)
    fpn = nets.FeaturePyramidNetwork(c5)
    fpn.load_state_dict(nets.seeded_state_dict(lambda: nets.FeaturePyramidNetwork(c5), 8))
    fpn = fpn.double()
    feats = [(t * 0.5).half().double() for t in _feats(n, c5, h5, w5, gen)]
    dp2 = torch.randn((n, 256, 8 * h5, 8 * w5), generator=gen).double()
    _wiring(fpn, feats).backward(dp2)
    want = {k: p.grad.detach() for k, p in fpn.named_parameters() if p.grad is not None}
    return fpn, feats, dp2, want


@pytest.mark.parametrize("case", sorted(GPU_CASES))
def test_written_out_backward_matches_autograd(case):
    fpn, feats, dp2, want = _case(case)
    assert len(want) == 10 and not any(k.startswith(("layer_blocks.0", "layer_blocks.1", "layer_blocks.2")) for k in want)
    got = _backward_as_the_kernels_form_it(fpn, feats, dp2)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].shape == want[k].shape
        assert _rel(got[k].numpy(), want[k].numpy()) <= 1e-12, k


@pytest.mark.parametrize("bug", ["unrotated_taps", "average_pool", "top_down_left_out", "lateral_order_reversed"])
@pytest.mark.parametrize("case", sorted(GPU_CASES))
def test_negative_controls_are_rejected_by_ten_times_the_bound(bug, case):
    fpn, feats, dp2, want = _case(case)
    got = _backward_as_the_kernels_form_it(fpn, feats, dp2, bug)
    # a reversed lateral order gives tensors of another shape: that alone is a miss of 100 %
    errs = {k: (_rel(got[k].numpy(), want[k].numpy()) if got[k].shape == want[k].shape else 1.0) for k in want}
    worst = max(errs.values())
    assert worst >= 10 * BOUNDS[case], f"{bug}: error {worst:.3g} is not 10x the bound {BOUNDS[case]}"
