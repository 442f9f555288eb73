"""The gradient of the DB head's input (dgrad into P2) without a device: argument checks of the new C entry points, the workspace-size
query's modes, the API's refusals, and negative controls of the fp64 reference at the GPU cases' shapes -- the dgrad written out as the
kernels compute it (one transposed 3x3 convolution of both branches' dy1), with a kernel-style mistake injected, must be rejected by at
least 10x the GPU tests' bound."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vtd_amd import _native, nets

# the GPU tests' bounds (tests/test_gpu_fpn_train.py) and the shapes of their cases
BOUNDS = {"small_train": 1.3e-3, "tiny_train": 1.1e-3}
GPU_CASES = {"small_train": (2, 256, 24, 20), "tiny_train": (2, 256, 4, 3)}


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


# ---- C ABI, no device
def _aligned(nbytes, align=256):
    raw = (C.c_char * (nbytes + 2 * align))()
    return raw, C.c_void_p((C.addressof(raw) + align - 1) // align * align)


def test_backward_input_argument_and_alignment_errors():
    lib = _native.load()
    assert b"DB head training" in lib.vtd_strerror(-2802) and b"argument" in lib.vtd_strerror(-2802)
    assert b"DB head training" in lib.vtd_strerror(-2803) and b"misaligned" in lib.vtd_strerror(-2803)
    keep = [_aligned(4096) for _ in range(4)]
    scratch, dfeats, dscale, w = (k[1] for k in keep)
    st = _native.DbHeadParams()
    fn = lib.vtd_dbhead_train_backward_input
    # every refusal comes before any launch, so none of this needs a device
    assert fn(2, 8, 8, None, scratch, dfeats, dscale, None) == -2802
    assert fn(2, 8, 8, C.byref(st), scratch, dfeats, dscale, None) == -2802        # conv_w pointers missing
    st.branch[0].conv_w = w
    assert fn(2, 8, 8, C.byref(st), scratch, dfeats, dscale, None) == -2802        # one branch still missing
    st.branch[1].conv_w = w
    for n, h, wd in ((0, 8, 8), (2, 0, 8), (2, 8, -1), (1 << 15, 1 << 8, 1 << 8)):
        assert fn(n, h, wd, C.byref(st), scratch, dfeats, dscale, None) == -2802
    assert fn(2, 8, 8, C.byref(st), None, dfeats, dscale, None) == -2802
    assert fn(2, 8, 8, C.byref(st), scratch, None, dscale, None) == -2802
    assert fn(2, 8, 8, C.byref(st), scratch, dfeats, None, None) == -2802
    st.branch[1].conv_w = C.c_void_p(w.value + 2)
    assert fn(2, 8, 8, C.byref(st), scratch, dfeats, dscale, None) == -2802        # a float pointer that is not 4-byte aligned
    st.branch[1].conv_w = w
    assert fn(2, 8, 8, C.byref(st), C.c_void_p(scratch.value + 128), dfeats, dscale, None) == -2803
    assert fn(2, 8, 8, C.byref(st), scratch, C.c_void_p(dfeats.value + 8), dscale, None) == -2803
    assert fn(2, 8, 8, C.byref(st), scratch, dfeats, C.c_void_p(dscale.value + 4), None) == -2803
    un = lib.vtd_dbhead_unpack_input_grad
    assert un(None, dscale, 2, 8, 8, w, None) == -2802 and un(dfeats, None, 2, 8, 8, w, None) == -2802
    assert un(dfeats, dscale, 2, 8, 8, None, None) == -2802 and un(dfeats, dscale, 2, 0, 8, w, None) == -2802
    assert un(C.c_void_p(dfeats.value + 4), dscale, 2, 8, 8, w, None) == -2803
    assert un(dfeats, dscale, 2, 8, 8, C.c_void_p(w.value + 2), None) == -2803


def test_workspace_modes():
    lib = _native.load()
    ws = lib.vtd_dbhead_train_workspace_bytes
    # modes 0 and 1 are what they were before mode 2 existed
    assert ws(2, 24, 20, 0) == 5904384 and ws(2, 24, 20, 1) == 12340736
    a256 = lambda x: (x + 255) // 256 * 256  # noqa: E731
    for n, h, w in ((1, 1, 1), (2, 4, 3), (2, 24, 20), (3, 13, 11), (32, 160, 160)):
        m1, m2 = ws(n, h, w, 1), ws(n, h, w, 2)
        # mode 2 = mode 1 (the backward's own layout, first) + padded dy1 + the packed dgrad weights + a zero bias row
        assert m2 - m1 == a256(n * (h + 2) * (w + 2) * 128 * 2) + 256 * 1152 * 2 + 1024
        assert m1 % 256 == 0 and m2 % 256 == 0
    for mode in (0, 1, 2):
        sizes = [ws(n, 24, 20, mode) for n in (1, 2, 3, 5, 8, 32)]
        assert all(b > a for a, b in zip(sizes, sizes[1:])), (mode, sizes)
        assert ws(0, 24, 20, mode) == -2802 and ws(2, 24, 0, mode) == -2802


# ---- API refusals
def test_input_grad_keyword_and_absent_modes():
    head = nets.DBHead(256)
    x = torch.zeros((1, 256, 4, 4), requires_grad=True)
    with pytest.raises(RuntimeError, match="dgrad into P2"):
        head(x)
    with pytest.raises(RuntimeError, match="input_grad=True"):
        head(x)
    with pytest.raises(ValueError, match="CUDA"):      # accepted as a request; the kernels still need a device tensor
        head(x, input_grad=True)
    with pytest.raises(ValueError):
        head(torch.zeros((1, 128, 4, 4), requires_grad=True), input_grad=True)
    # the FPN does not train yet: no mode may claim it does
    for mode in ("fpn_head", "fpn", "all"):
        with pytest.raises(ValueError, match="trainable"):
            nets.DBNet("resnet18", trainable=mode)


# ---- negative controls
def _dgrad_as_the_kernels_form_it(head, dy1, bug=None):
    """dP2 from the two branches' dy1 [n,64,H,W]: one 3x3 convolution over the 128 stacked channels with the window rotated by 180
    degrees and the weights transposed (csrc/dbhead_train.hip, pack_dgrad).  `bug` injects a kernel-style mistake."""
    ws = []
    for b, seq in enumerate((head.probability_head, head.threshold_head)):
        wd = seq[0].weight.detach().transpose(0, 1)     # [256 ci][64 co][3][3]
        if bug != "unflipped_taps":
            wd = wd.flip(-1, -2)
        if bug == "scales_not_equalised" and b == 1:
            wd = wd * 2.0
        if bug == "one_branch_left_out" and b == 1:
            wd = wd * 0.0
        ws.append(wd)
    return F.conv2d(torch.cat(dy1, 1), torch.cat(ws, 1), padding=1)


def _run(shape, seed=4):
    """The head under fp64 autograd with the reference loss: (head, d loss / d features, [dy1 of each branch])."""
    gen = torch.Generator().manual_seed(seed)
    head = nets.DBHead(256)
    head.load_state_dict(nets.seeded_state_dict(lambda: nets.DBHead(256), 8))
    head = head.double().train()
    n, _, H, W = shape
    x = (torch.randn(shape, generator=gen) * 0.5).half().double().requires_grad_(True)
    pt = (torch.rand((n, 1, 4 * H, 4 * W), generator=gen) > 0.7).double()
    tt = torch.rand((n, 1, 4 * H, 4 * W), generator=gen).double() * 0.6 + 0.2
    ys, outs = [], []
    for seq in (head.probability_head, head.threshold_head):
        y = seq[0](x)
        y.retain_grad()
        ys.append(y)
        outs.append(seq[1:](y))
    p, t = outs
    bce = torch.nn.BCELoss()
    pv, tv = p.reshape(-1), pt.reshape(-1)
    loss = bce(p, pt) + bce(t, tt) + 1 - (2.0 * (pv * tv).sum() + 1e-5) / (pv.sum() + tv.sum() + 1e-5)
    loss.backward()
    return head, x.grad.detach(), [y.grad.detach() for y in ys]


@pytest.mark.parametrize("case", sorted(GPU_CASES))
def test_written_out_dgrad_matches_autograd(case):
    head, xgrad, dy1 = _run(GPU_CASES[case])
    assert _rel(_dgrad_as_the_kernels_form_it(head, dy1).numpy(), xgrad.numpy()) <= 1e-12


@pytest.mark.parametrize("bug", ["unflipped_taps", "one_branch_left_out", "scales_not_equalised"])
@pytest.mark.parametrize("case", sorted(GPU_CASES))
def test_negative_controls_are_rejected_by_ten_times_the_bound(bug, case):
    head, xgrad, dy1 = _run(GPU_CASES[case])
    err = _rel(_dgrad_as_the_kernels_form_it(head, dy1, bug).numpy(), xgrad.numpy())
    assert err >= 10 * BOUNDS[case], f"{bug}: error {err:.3g} is not 10x the bound {BOUNDS[case]}"
