"""Training ResNet-18's stem (csrc/stem_train.hip behind the vtd_stem_train_* entries), without a device: the new symbols, the workspace
query and the refusals of the new entry family, the bookkeeping of the mode "head+fpn+backbone", and fp64 controls of what the kernels
compute: the index-routing backward (m at pooled resolution, dZ gathered by the first-maximum index, G, the three formulae) against torch
autograd of the plain stem, with last-maximum routing as a control that must miss; the window-membership rule of the gather; and the weight
gradient in the kernel's own column order (q = 32 ky + 4 kx + ci: 224 columns, 147 kept) and slab rule against
torch.nn.grad.conv2d_weight at the GPU test's sizes."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_layer3_train as l3c
from vtd_amd import _native, nets
from vtd_amd.nets import forward_stem_padded, stem_train  # noqa: F401  (the feature under test: absent before it)

# no GPU gradient bound is above the project's ceiling for gradients (tests/test_gpu_stem_train.py): a control that misses by 10x the ceiling
# misses by 10x every bound
GRAD_CEILING = 1e-2
MODE = "head+fpn+backbone"
L1_MODE = "head+fpn+layer4+layer3+layer2+layer1"
NARROWER = (L1_MODE, "head+fpn+layer4+layer3+layer2", "head+fpn+layer4+layer3", "head+fpn+layer4", "head+fpn", "head")
# n = 2 and image sizes (H, W) of the GPU test.  (4, 4): a 1x1 pooled map.  (10, 14): conv 5x7, odd, so the pool's bottom and right padding is
# touched.  (36, 44): pooled 9x11, four forward tiles of 7x8, partial in both directions.  (54, 38): conv 27x19 = 513 pixels, 1026 rows: the
# smallest row count above 1024, so min(512, ceil(rows / 1024)) = 2 slabs of ceil(513 / 32) * 32 = 544 rows; the last holds 482 = 15 * 32 + 2
# rows and ends inside a 32-row chunk
SIZES = [(4, 4), (10, 14), (36, 44), (54, 38)]
LARGE = (54, 38)
ZERO_CH, NEG_CH = 3, 7      # the gamma = 0, beta > 0 channel and the gamma < 0 channel

_rel, _aligned = l3c._rel, l3c._aligned


# ---- C ABI, no device
def test_stem_symbols_and_error_text():
    lib = _native.load()
    for name in ("vtd_stem_train_pack_input", "vtd_stem_train_workspace_bytes", "vtd_stem_train_forward", "vtd_stem_train_backward"):
        assert name in _native.SIGNATURES and hasattr(lib, name), name
    for code in (-3301, -3302):
        assert b"stem training" in lib.vtd_strerror(code)
    assert b"geometry" in lib.vtd_strerror(-3301) and b"misaligned" in lib.vtd_strerror(-3302)
    # the other families' texts are unchanged
    assert b"64-wide block training" in lib.vtd_strerror(-3201) and b"ResNet block training" in lib.vtd_strerror(-3101)
    assert [f for f, _ in _native.StemParams._fields_] == ["w", "gamma", "beta", "mean", "var"]


def test_stem_workspace_query():
    ws = _native.load().vtd_stem_train_workspace_bytes
    shapes = ((2, 4, 4), (2, 36, 44), (2, 640, 640), (32, 640, 640))
    for n, h, w in shapes:
        for mode in (0, 1):
            b = ws(n, h, w, mode)
            assert b > 0 and b % 256 == 0, (n, h, w, mode)
    # the backward's scratch (dZ and the slabs) grows with the size and with n; the forward's workspace holds the folded weights and the
    # bias alone, so it does not depend on the shape
    assert ws(32, 640, 640, 1) > ws(2, 640, 640, 1) > ws(2, 36, 44, 1) > ws(2, 4, 4, 1)
    assert ws(32, 640, 640, 0) == ws(2, 4, 4, 0) >= 7 * 4 * 64 * 8 * 2 + 64 * 4
    for bad in ((2, 5, 4), (2, 4, 7), (2, 0, 4), (2, 4, 0), (2, -4, 4), (2, 4, -2), (0, 4, 4), (-1, 4, 4), (2, 1, 4)):
        assert ws(*bad, 0) == -3301 and ws(*bad, 1) == -3301, bad
    for mode in (2, -1):
        assert ws(2, 4, 4, mode) == -3301


def test_stem_argument_and_alignment_errors():
    lib = _native.load()
    keep = [_aligned(4096) for _ in range(3)]
    a, b, c = (k[1] for k in keep)
    off = lambda p, k: C.c_void_p(p.value + k)  # noqa: E731
    st = _native.StemParams(*([a] * 5))
    sp = C.byref(st)
    pack, fwd, bwd = lib.vtd_stem_train_pack_input, lib.vtd_stem_train_forward, lib.vtd_stem_train_backward
    # every refusal comes before any launch, so none of this needs a device
    assert pack(None, 0, 2, 4, 4, b, None) == -3301 and pack(a, 0, 2, 4, 4, None, None) == -3301
    assert pack(a, 2, 2, 4, 4, b, None) == -3301 and pack(a, 0, 2, 5, 4, b, None) == -3301 and pack(a, 0, 0, 4, 4, b, None) == -3301
    assert pack(off(a, 2), 0, 2, 4, 4, b, None) == -3302 and pack(a, 1, 2, 4, 4, off(b, 8), None) == -3302
    g = (2, 4, 4)
    assert fwd(None, *g, sp, 1e-5, b, c, a, None) == -3301
    assert fwd(a, *g, None, 1e-5, b, c, a, None) == -3301
    assert fwd(a, *g, sp, 1e-5, None, c, a, None) == -3301
    assert fwd(a, *g, sp, 1e-5, b, None, a, None) == -3301
    assert fwd(a, *g, sp, 1e-5, b, c, None, None) == -3301
    assert fwd(a, *g, sp, 0.0, b, c, a, None) == -3301
    assert fwd(a, *g, C.byref(_native.StemParams(a, a, a, a, None)), 1e-5, b, c, a, None) == -3301      # no running variance
    for bad in ((2, 5, 4), (2, 4, 6 + 1), (2, 0, 4), (2, 4, -4), (0, 4, 4)):
        assert fwd(a, *bad, sp, 1e-5, b, c, a, None) == -3301, bad
        assert bwd(a, *bad, sp, 1e-5, b, c, a, a, a, sp, b, None) == -3301, bad
    assert fwd(a, *g, sp, 1e-5, off(b, 128), c, a, None) == -3302          # a misaligned workspace
    assert fwd(off(a, 8), *g, sp, 1e-5, b, c, a, None) == -3302            # a misaligned image tap
    assert fwd(a, *g, sp, 1e-5, b, off(c, 8), a, None) == -3302            # a misaligned pooled tap
    assert fwd(a, *g, sp, 1e-5, b, c, off(a, 4), None) == -3302            # misaligned indices
    assert bwd(a, *g, sp, 1e-5, b, c, a, None, a, sp, b, None) == -3301        # no dpool
    assert bwd(a, *g, sp, 1e-5, b, c, a, a, None, sp, b, None) == -3301        # no dscale
    assert bwd(a, *g, sp, 1e-5, b, c, a, a, a, None, b, None) == -3301         # no place for the gradients
    assert bwd(a, *g, sp, 1e-5, b, c, a, a, a, sp, None, None) == -3301        # no scratch
    assert bwd(a, *g, sp, 1e-5, b, c, None, a, a, sp, b, None) == -3301        # no indices
    assert bwd(a, *g, sp, 0.0, b, c, a, a, a, sp, b, None) == -3301            # eps = 0
    assert bwd(a, *g, sp, 1e-5, off(b, 128), c, a, a, a, sp, b, None) == -3302     # a misaligned workspace
    assert bwd(a, *g, sp, 1e-5, b, c, a, a, a, sp, off(b, 128), None) == -3302     # a misaligned scratch
    assert bwd(a, *g, sp, 1e-5, b, c, a, off(a, 8), a, sp, b, None) == -3302       # a misaligned dpool
    assert bwd(a, *g, sp, 1e-5, b, c, a, a, off(a, 4), sp, b, None) == -3302       # a misaligned dscale
    assert bwd(off(a, 8), *g, sp, 1e-5, b, c, a, a, a, sp, b, None) == -3302       # a misaligned image tap
    # no existing entry's gate moved
    blk = C.byref(_native.BasicBlockParams(*([a] * 15)))
    assert lib.vtd_block64_train_forward(a, 2, 6, 4, 64, 128, 2, blk, 1e-5, b, c, None) == -3201
    assert lib.vtd_resblock_train_forward(a, 2, 6, 4, 64, 64, 1, blk, 1e-5, b, c, None) == -3101


def test_python_refusals():
    conv, bn = nets.make_trunk("resnet18")[:2]
    with pytest.raises(ValueError, match="CUDA"):
        nets.stem_train(conv, bn, torch.zeros((1, 3, 4, 4)))
    with pytest.raises(ValueError, match=r"\[n,3,H,W\]"):
        nets.pack_image(torch.zeros((1, 4, 4, 4)))
    with pytest.raises(ValueError, match="image tap"):
        nets.forward_stem_padded(conv, bn, torch.zeros((1, 10, 10, 4)))      # not a float16 CUDA tap
    with pytest.raises(RuntimeError, match="built for ResNet's stem"):
        nets.forward_stem_padded(torch.nn.Conv2d(3, 64, 3, 2, 1, bias=False), bn, torch.zeros((1, 10, 10, 4)))
    fpn, trunk = nets.FeaturePyramidNetwork(512), nets.make_trunk("resnet18")
    with pytest.raises(ValueError, match="needs layer1, layer2, layer3, layer4 and the DBHead"):
        fpn.forward_padded([None], head=nets.DBHead(256), layer4=trunk[7], layer3=trunk[6], layer2=trunk[5], stem=(trunk[0], trunk[1]))
    with pytest.raises(ValueError, match="pair"):
        fpn.forward_padded([None], head=nets.DBHead(256), layer4=trunk[7], layer3=trunk[6], layer2=trunk[5], layer1=trunk[4], stem=trunk[0])
    assert "basic_block_train" in nets.stem_train.__doc__


# ---- the product mode
def _trained(net):
    return list(net.backbone.parameters()) + list(net.fpn.live_parameters()) + list(net.head.parameters())


def test_backbone_mode():
    net = nets.DBNet("resnet18", trainable=MODE)
    assert net.trainable == MODE
    assert len(_trained(net)) == 90 and all(p.requires_grad for p in _trained(net))
    frozen = [k for k, p in net.named_parameters() if not p.requires_grad]
    assert frozen == []
    l1net = nets.DBNet("resnet18", trainable=L1_MODE)
    assert sum(1 for p in _trained(l1net) if p.requires_grad) == 87
    # the eval-mode rebuild is keyed on the stem's three parameters and three buffers too
    assert len(net._head_tensor_versions()) == len(l1net._head_tensor_versions()) + 6
    # the state dict is the reference's, whatever the mode
    assert list(net.state_dict()) == list(nets.DBNet("resnet18").state_dict())
    assert MODE in nets.DBNet.set_trainable.__doc__


def test_backbone_mode_refusals():
    with pytest.raises(ValueError, match="Bottleneck training is not built"):
        nets.DBNet("resnet50", trainable=MODE)
    with pytest.raises(ValueError, match="Bottleneck training is not built"):
        nets.DBNet("resnet50").set_trainable(MODE)
    for mode in ("all", L1_MODE + "+stem", "backbone", "head+backbone", "head+fpn+stem", "head+fpn+backbone+stem"):
        with pytest.raises(ValueError, match="trainable"):
            nets.DBNet("resnet18", trainable=mode)
    # the layer1 mode keeps its refusal
    net = nets.DBNet("resnet18", trainable=L1_MODE)
    net.backbone[0].weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match="backward below layer1 is not"):
        net.train()(torch.zeros((1, 3, 640, 640)))
    # a tensor frozen by hand is refused in a train-mode forward, before anything touches a device
    net = nets.DBNet("resnet18", trainable=MODE)
    net.backbone[1].bias.requires_grad_(False)
    with pytest.raises(RuntimeError, match="trains every tensor"):
        net.train()(torch.zeros((1, 3, 640, 640)))
    with pytest.raises(ValueError, match=r"\[n,3,H,W\]"):
        nets.DBNet("resnet18", trainable=MODE).train()(torch.zeros((1, 1, 640, 640)))


def test_switching_between_modes():
    flags = lambda net: [p.requires_grad for p in net.parameters()]  # noqa: E731
    for other in NARROWER:
        want = flags(nets.DBNet("resnet18", trainable=other))
        net = nets.DBNet("resnet18", trainable=MODE)
        assert all(flags(net))
        net.set_trainable(other)
        assert flags(net) == want, other
        net.set_trainable(MODE)      # and back
        assert all(flags(net)) and len(_trained(net)) == 90
        net.set_trainable(other)
        assert flags(net) == want, other


# ---- fp64 controls of what the kernels compute
def stem_modules(seed=71):
    """(conv, bn) of the stem on the CPU in float32, with non-trivial statistics, a random beta, a gamma = 0, beta > 0 channel (constant and
    positive: every pooling window of it is a full tie) and a gamma < 0 channel (the folded weights change sign)."""
    make = lambda: torch.nn.Sequential(*nets.make_trunk("resnet18")[:2])  # noqa: E731
    stem = make()
    stem.load_state_dict(nets.seeded_state_dict(make, seed))
    with torch.no_grad():
        stem[1].bias.copy_(0.1 * torch.randn(64, generator=torch.Generator().manual_seed(seed + 1)))
        stem[1].weight[ZERO_CH] = 0.0
        stem[1].bias[ZERO_CH] = 0.5
        stem[1].weight[NEG_CH] = -0.75
    return stem[0], stem[1]


def stem_inputs(size, n=2):
    """(the image with fp16-representable values, an upstream gradient of the pooled map's shape)."""
    H, W = size
    gen = torch.Generator().manual_seed(13 * H + W)
    x = (torch.randn((n, 3, H, W), generator=gen) * 0.5).half().float()
    up = torch.randn((n, 64, (H // 2 + 1) // 2, (W // 2 + 1) // 2), generator=gen)
    return x, up


def window_codes(z, last=False):
    """The pooled map of z [n,C,hc,wc] and, per pooled element, the window position 3 ky + kx of the first (or last) maximum in scan order
    among the in-image positions."""
    win = F.pad(z, (1, 1, 1, 1), value=float("-inf")).unfold(2, 3, 2).unfold(3, 3, 2).reshape(*z.shape[:2], -1, 9)
    hp, wp = (z.shape[2] + 1) // 2, (z.shape[3] + 1) // 2
    mx = win.max(-1).values
    eq = win == mx[..., None]
    codes = torch.arange(9)
    code = torch.where(eq, codes, torch.tensor(-1 if last else 9)).max(-1).values if last else torch.where(eq, codes, torch.tensor(9)).min(-1).values
    return mx.reshape(*z.shape[:2], hp, wp), code.reshape(*z.shape[:2], hp, wp)


def route(m, code, hc, wc):
    """dZ [n,C,hc,wc]: conv pixel (y, x) takes m of every window (py, px) that holds it -- 2 py - 1 <= y <= 2 py + 1, columns alike -- and
    whose code names it."""
    n, ch, hp, wp = m.shape
    dz = torch.zeros((n, ch, hc, wc), dtype=m.dtype)
    for y in range(hc):
        for py in ([y // 2] if y % 2 == 0 else [(y - 1) // 2, (y + 1) // 2]):      # the kernel's rule: even one window, odd two
            if py >= hp:
                continue
            for x in range(wc):
                for px in ([x // 2] if x % 2 == 0 else [(x - 1) // 2, (x + 1) // 2]):
                    if px >= wp:
                        continue
                    c = 3 * (y - 2 * py + 1) + (x - 2 * px + 1)
                    dz[:, :, y, x] += m[:, :, py, px] * (code[:, :, py, px] == c)
    return dz


def slabs(rows):
    """csrc/stem_train.hip: wg_slabs and slab_rows (32-row chunks)."""
    s = max(1, min(512, (rows + 1023) // 1024))
    return s, ((rows + s - 1) // s + 31) // 32 * 32


def kernel_order_wgrad(x, dz, bug=None):
    """dW [64,3,7,7] from G[c][q] = sum over the slabs, in slab order, of sum_rows dZ[row][c] X[row][q] with q = 32 ky + 4 kx + ci, kx < 8: X
    is gathered from the flat ring-3 NHWC4 image at pixel (2y + ky, 2x + kx); the eighth pixel and the fourth channel are computed and
    dropped."""
    n, _, H, W = x.shape
    hc, wc = H // 2, W // 2
    tap = np.zeros((n, H + 6, W + 6, 4))
    tap[:, 3:-3, 3:-3, :3] = x.permute(0, 2, 3, 1).numpy()
    flat = tap.reshape(-1)
    a = dz.permute(0, 2, 3, 1).reshape(-1, 64).numpy()
    img, y, xx = (v.reshape(-1) for v in np.meshgrid(np.arange(n), np.arange(hc), np.arange(wc), indexing="ij"))
    rows = a.shape[0]
    S, slab_len = slabs(rows)
    G = np.zeros((64, 224))
    for sl in range(S):
        r = slice(sl * slab_len, min((sl + 1) * slab_len, rows))
        slab = np.zeros((64, 224))
        for ky in range(7):
            step = 1 if bug == "stride1" else 2
            base = ((img[r] * (H + 6) + step * y[r] + ky) * (W + 6) + step * xx[r]) * 4      # 32 halfs = 8 pixels x 4 channels from here
            slab[:, 32 * ky:32 * ky + 32] = a[r].T @ flat[base[:, None] + np.arange(32)[None, :]]
        G = G + slab
    q = np.array([[[32 * ky + 4 * kx + ci for kx in range(7)] for ky in range(7)] for ci in range(3)])
    return torch.from_numpy(G[:, q]), G


def test_window_membership_rule():
    """The gather's rule -- an even conv coordinate lies in one window, an odd one in two, those past the pooled map dropped -- names exactly
    the windows that hold the coordinate, for even and odd conv sizes."""
    for hc in (1, 2, 5, 7, 18, 27):
        hp = (hc + 1) // 2
        for y in range(hc):
            rule = [py for py in ([y // 2] if y % 2 == 0 else [(y - 1) // 2, (y + 1) // 2]) if py < hp]
            assert rule == [py for py in range(hp) if 0 <= y - (2 * py - 1) <= 2], (hc, y)


@pytest.mark.parametrize("rows", [2, 12, 140, 3600, 819200])
def test_quarter_reduce_order(rows):
    """st_reduce_kernel and st_finish_kernel written out (rb_reduce64_kernel's order over pooled pixels): G = min(256, ceil(rows / 256))
    workgroups of ceil(rows / G) rows, each cut into four quarters at ceil(k r / 4) and added as (q0 + q1) + (q2 + q3); the partials added
    in workgroup order.  Every row is summed exactly once."""
    v = torch.randn((rows, 4), generator=torch.Generator().manual_seed(rows)).double().numpy()
    G = min(256, max(1, (rows + 255) // 256))
    per = (rows + G - 1) // G
    total, seen = np.zeros(4), 0
    for g in range(G):
        m0 = min(g * per, rows)
        m1 = min(m0 + per, rows)
        r = m1 - m0
        cuts = [m0 + (k * r + 3) // 4 for k in range(5)]
        assert cuts[0] == m0 and cuts[4] == m1 and all(b >= a for a, b in zip(cuts, cuts[1:]))
        q = [v[a:b].sum(axis=0) for a, b in zip(cuts, cuts[1:])]
        total = total + ((q[0] + q[1]) + (q[2] + q[3]))
        seen += r
    assert seen == rows
    if rows == 819200:      # the pooled map of B = 32 at the product shape: 256 partials of 3200 rows, quarters of 800
        assert (G, per) == (256, 3200)
    assert _rel(total, v.sum(axis=0)) <= 1e-12


_CONTROL = {}


def _control_case():
    if not _CONTROL:
        conv, bn = (m.double() for m in stem_modules())
        x, up = (t.double() for t in stem_inputs((10, 14)))
        rstd = 1.0 / torch.sqrt(bn.running_var + bn.eps)
        z = F.relu(F.conv2d(x, conv.weight, None, 2, 3) * (bn.weight * rstd)[None, :, None, None]
                   + (bn.bias - bn.running_mean * bn.weight * rstd)[None, :, None, None])
        F.max_pool2d(z, 3, 2, 1).backward(up)
        want = [conv.weight.grad.clone(), bn.weight.grad.clone(), bn.bias.grad.clone()]
        _CONTROL.update(conv=conv, bn=bn, x=x, up=up, z=z.detach(), rstd=rstd.detach(), want=want)
    return _CONTROL


def _routed_grads(c, last=False):
    """The kernels' backward in fp64: m, dZ by index routing, G in the kernel's column order, the three formulae."""
    conv, bn, x, up, z, rstd = c["conv"], c["bn"], c["x"], c["up"], c["z"], c["rstd"]
    pool, code = window_codes(z, last)
    m = up * (pool > 0)
    dbeta = m.sum((0, 2, 3))
    dz = route(m, code, z.shape[2], z.shape[3])
    G, _ = kernel_order_wgrad(x, dz)
    w, gam, mean = conv.weight.detach(), bn.weight.detach(), bn.running_mean
    dw = (gam * rstd)[:, None, None, None] * G
    dgamma = rstd * ((w * G).sum((1, 2, 3)) - mean * dbeta)
    return [dw, dgamma, dbeta]


def test_index_routing_backward_matches_autograd():
    c = _control_case()
    gam, bet = c["bn"].weight.detach(), c["bn"].bias.detach()
    assert float(gam[ZERO_CH]) == 0.0 and float(bet[ZERO_CH]) > 0 and float(gam[NEG_CH]) < 0
    assert float(c["z"][:, ZERO_CH].min()) == float(c["z"][:, ZERO_CH].max()) > 0, "the gamma = 0 channel is constant and positive"
    for got, want in zip(_routed_grads(c), c["want"]):
        assert got.shape == want.shape and _rel(got.numpy(), want.numpy()) <= 1e-12
    # torch's own CPU indices are the first maximum in scan order
    _, idx = F.max_pool2d(c["z"], 3, 2, 1, return_indices=True)
    pool, code = window_codes(c["z"])
    hp, wp, wc = pool.shape[2], pool.shape[3], c["z"].shape[3]
    py, px = torch.meshgrid(torch.arange(hp), torch.arange(wp), indexing="ij")
    assert torch.equal(idx, (2 * py - 1 + code // 3) * wc + (2 * px - 1 + code % 3))


def test_index_routing_negative_control():
    """In the gamma = 0 channel every window is a full tie, so its dgamma depends on the first-maximum rule alone: routing to the last maximum
    must move it by at least 10x the gradient ceiling, or the case proves nothing."""
    c = _control_case()
    want = float(c["want"][1][ZERO_CH])
    got = float(_routed_grads(c, last=True)[1][ZERO_CH])
    assert abs(want) > 0 and abs(got - want) / abs(want) >= 10 * GRAD_CEILING, (got, want)


@pytest.mark.parametrize("size", SIZES)
def test_weight_gradient_in_kernel_column_order(size):
    H, W = size
    gen = torch.Generator().manual_seed(5 * H + W)
    x = torch.randn((2, 3, H, W), generator=gen).double()
    dz = torch.randn((2, 64, H // 2, W // 2), generator=gen).double()
    want = torch.nn.grad.conv2d_weight(x, (64, 3, 7, 7), dz, stride=2, padding=3)
    rows = 2 * (H // 2) * (W // 2)
    S, slab_len = slabs(rows)
    if size == LARGE:      # the smallest multi-slab case: 1026 rows = a slab of 544 and one of 482, which ends inside a 32-row chunk
        assert (S, slab_len) == (2, 544) and (rows - slab_len) % 32 == 2
    else:
        assert S == 1
    got, G = kernel_order_wgrad(x, dz)
    assert got.shape == want.shape and _rel(got.numpy(), want.numpy()) <= 1e-12
    assert G.shape == (64, 224) and got.numel() == 64 * 147
    assert float(np.abs(G[:, 3::4]).max()) == 0.0, "the fourth channel's columns multiply zeros"
    assert slabs(32 * 320 * 320) == (512, 6400)      # the product shape at B = 32
    if min(size) > 4:      # control, at the sizes with more than one pooled pixel: a gather at stride 1 instead of the conv's 2 must miss
        err = _rel(kernel_order_wgrad(x, dz, bug="stride1")[0].numpy(), want.numpy())
        assert err >= 10 * GRAD_CEILING, err
