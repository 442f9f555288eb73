"""Train-mode (batch-statistics) BatchNorm for ResNet-18's stem (csrc/stem_train.hip behind the vtd_stem_bn_train_* entries), without a device:
the new symbols and error texts, the workspace query and the refusals before any launch, the new Python spellings (`nets.stem_bn_train`,
`forward_padded(..., stem_batch_stats=True)`, `DBNet(trainable="head+fpn+backbone", trunk_bn="backbone")`), and fp64 controls of the
arithmetic the kernels implement: s1 and s2 taken at pooled resolution and the dense dz against torch autograd of the plain train-mode stem,
with controls that must miss; the geometry of the reductions at the GPU test's sizes; and the tile-ownership rule of the z-writing forward.
The float32 stand-in of the GPU node test's chain, by which its seeds were chosen, stands here too."""
import copy
import ctypes as C
import pathlib

import pytest
import torch
import torch.nn.functional as F

import test_layer1_bn_train as l1b
import test_layer1_train as l1c
import test_stem_train as sc
from vtd_amd import _native, nets
from vtd_amd.nets import stem_bn_train  # noqa: F401  (the feature under test: absent before it)

GRAD_CEILING = sc.GRAD_CEILING
SIZES, LARGE, ZERO_CH, NEG_CH = sc.SIZES, sc.LARGE, sc.ZERO_CH, sc.NEG_CH
MODE, L1_MODE, STAGES = sc.MODE, sc.L1_MODE, l1b.STAGES
STEM_FROZEN = l1b.STEM_FROZEN
_rel, _aligned = sc._rel, sc._aligned


# ---- C ABI, no device
def test_symbols_and_error_texts():
    lib = _native.load()
    for name in ("vtd_stem_bn_train_workspace_bytes", "vtd_stem_bn_train_forward", "vtd_stem_bn_train_backward"):
        assert name in _native.SIGNATURES and hasattr(lib, name), name
    texts = [lib.vtd_strerror(code) for code in (-3801, -3802, -3301, -3302)]
    assert len(set(texts)) == 4
    assert b"stem batch-statistics training" in texts[0] and b"stem batch-statistics training" in texts[1] and b"misaligned" in texts[1]
    assert b"stem training" in texts[2] and b"batch-statistics" not in texts[2]      # the frozen family's texts are unchanged
    header = (pathlib.Path(__file__).resolve().parents[1] / "include" / "vtd.h").read_text()
    assert "vtd_stem_bn_train_forward" in header and "-3801" in header and "(y / 14, x / 16)" in header


def test_workspace_query():
    lib = _native.load()
    ws, frozen = lib.vtd_stem_bn_train_workspace_bytes, lib.vtd_stem_train_workspace_bytes
    for n, h, w in ((2, 2, 2), (2, 4, 4), (2, 36, 44), (2, 54, 38), (2, 640, 640), (32, 640, 640)):
        for mode in (0, 1):
            assert ws(n, h, w, mode) > 0 and ws(n, h, w, mode) % 256 == 0, (n, h, w, mode)
            assert ws(n, h, w, mode) >= frozen(n, h, w, mode)      # training = 0 runs the frozen path in the same allocation
        assert ws(n, h, w, 0) >= n * (h // 2) * (w // 2) * 64 * 4      # z [n hc wc][64] fp32 stays in the forward's workspace
    assert ws(2, 640, 640, 0) >= 204800 * 64 * 4      # 52 MB at the bench shape
    for bad in ((2, 5, 4), (2, 4, 7), (2, 0, 4), (2, 4, 0), (2, -4, 4), (0, 4, 4), (-1, 4, 4), (2, 1, 4)):
        assert ws(*bad, 0) == -3801 and ws(*bad, 1) == -3801, bad
    for mode in (2, -1):
        assert ws(2, 4, 4, mode) == -3801
    assert frozen(2, 5, 4, 0) == -3301      # the frozen query keeps its own answer


def test_argument_and_alignment_errors():
    lib = _native.load()
    keep = [_aligned(4096) for _ in range(3)]
    a, b, c = (k[1] for k in keep)
    off = lambda p, k: C.c_void_p(p.value + k)  # noqa: E731
    sp = C.byref(_native.StemParams(*([a] * 5)))
    fwd, bwd = lib.vtd_stem_bn_train_forward, lib.vtd_stem_bn_train_backward
    g = (2, 4, 4)
    # every refusal comes before any launch, so none of this needs a device
    for tr in (0, 1):
        assert fwd(None, *g, sp, tr, 0.1, 1e-5, b, c, a, None, None) == -3801
        assert fwd(a, *g, None, tr, 0.1, 1e-5, b, c, a, None, None) == -3801
        assert fwd(a, *g, sp, tr, 0.1, 1e-5, None, c, a, None, None) == -3801
        assert fwd(a, *g, sp, tr, 0.1, 1e-5, b, None, a, None, None) == -3801
        assert fwd(a, *g, sp, tr, 0.1, 1e-5, b, c, None, None, None) == -3801
        assert fwd(a, *g, sp, tr, 0.1, 0.0, b, c, a, None, None) == -3801
        assert fwd(a, *g, sp, tr, 0.1, -1e-5, b, c, a, None, None) == -3801
        assert fwd(a, *g, C.byref(_native.StemParams(a, a, a, a, None)), tr, 0.1, 1e-5, b, c, a, None, None) == -3801      # no running variance
        for bad in ((2, 5, 4), (2, 4, 7), (2, 0, 4), (2, 4, -4), (0, 4, 4)):
            assert fwd(a, *bad, sp, tr, 0.1, 1e-5, b, c, a, None, None) == -3801, bad
            assert bwd(a, *bad, sp, tr, 1e-5, b, c, a, a, a, sp, b, None) == -3801, bad
        assert fwd(a, *g, sp, tr, 0.1, 1e-5, off(b, 128), c, a, None, None) == -3802          # a misaligned workspace
        assert fwd(off(a, 8), *g, sp, tr, 0.1, 1e-5, b, c, a, None, None) == -3802            # a misaligned image tap
        assert fwd(a, *g, sp, tr, 0.1, 1e-5, b, off(c, 8), a, None, None) == -3802            # a misaligned pooled tap
        assert fwd(a, *g, sp, tr, 0.1, 1e-5, b, c, off(a, 4), None, None) == -3802            # misaligned indices
        assert fwd(a, *g, sp, tr, 0.1, 1e-5, b, c, a, off(a, 2), None) == -3802               # misaligned statistics
        assert bwd(None, *g, sp, tr, 1e-5, b, c, a, a, a, sp, b, None) == -3801
        assert bwd(a, *g, None, tr, 1e-5, b, c, a, a, a, sp, b, None) == -3801
        assert bwd(a, *g, sp, tr, 1e-5, None, c, a, a, a, sp, b, None) == -3801            # no workspace
        assert bwd(a, *g, sp, tr, 1e-5, b, None, a, a, a, sp, b, None) == -3801            # no pooled tap
        assert bwd(a, *g, sp, tr, 1e-5, b, c, None, a, a, sp, b, None) == -3801            # no indices
        assert bwd(a, *g, sp, tr, 1e-5, b, c, a, None, a, sp, b, None) == -3801            # no dpool
        assert bwd(a, *g, sp, tr, 1e-5, b, c, a, a, None, sp, b, None) == -3801            # no dscale
        assert bwd(a, *g, sp, tr, 1e-5, b, c, a, a, a, None, b, None) == -3801             # no place for the gradients
        assert bwd(a, *g, sp, tr, 1e-5, b, c, a, a, a, sp, None, None) == -3801            # no scratch
        assert bwd(a, *g, sp, tr, 0.0, b, c, a, a, a, sp, b, None) == -3801                # eps = 0
        assert bwd(a, *g, sp, tr, 1e-5, off(b, 128), c, a, a, a, sp, b, None) == -3802     # a misaligned workspace
        assert bwd(a, *g, sp, tr, 1e-5, b, c, a, a, a, sp, off(b, 128), None) == -3802     # a misaligned scratch
        assert bwd(a, *g, sp, tr, 1e-5, b, c, a, off(a, 8), a, sp, b, None) == -3802       # a misaligned dpool
        assert bwd(a, *g, sp, tr, 1e-5, b, c, a, a, off(a, 4), sp, b, None) == -3802       # a misaligned dscale
        assert bwd(off(a, 8), *g, sp, tr, 1e-5, b, c, a, a, a, sp, b, None) == -3802       # a misaligned image tap
    # training outside {0, 1}, momentum outside [0, 1] or NaN (the frozen path has no momentum: only training = 1 looks at it)
    for tr in (2, -1):
        assert fwd(a, *g, sp, tr, 0.1, 1e-5, b, c, a, None, None) == -3801
        assert bwd(a, *g, sp, tr, 1e-5, b, c, a, a, a, sp, b, None) == -3801
    for mom in (1.5, -0.1, float("nan")):
        assert fwd(a, *g, sp, 1, mom, 1e-5, b, c, a, None, None) == -3801
    # training = 1 at n = 1, 2 x 2: one conv pixel, one value per channel has no variance
    one = (1, 2, 2)
    assert fwd(a, *one, sp, 1, 0.1, 1e-5, b, c, a, None, None) == -3801
    assert bwd(a, *one, sp, 1, 1e-5, b, c, a, a, a, sp, b, None) == -3801
    assert lib.vtd_stem_bn_train_workspace_bytes(*one, 0) > 0      # the shape itself is built: training = 0 runs it
    # no existing entry's gate moved
    assert lib.vtd_stem_train_forward(None, *g, sp, 1e-5, b, c, a, None) == -3301
    assert lib.vtd_stem_train_forward(a, *g, sp, 1e-5, off(b, 128), c, a, None) == -3302


# ---- the Python surface
def test_stem_bn_train_refusals():
    conv, bn = nets.make_trunk("resnet18")[:2]
    for mode in (True, False):
        bn.train(mode)
        with pytest.raises(ValueError, match="CUDA"):
            nets.stem_bn_train(conv, bn, torch.zeros((2, 3, 4, 4)))
    with pytest.raises(ValueError, match=r"\[n,3,H,W\]"):
        nets.stem_bn_train(conv, bn, torch.zeros((2, 4, 4, 4)))
    bn.momentum = None
    with pytest.raises(ValueError, match="momentum=None, the cumulative average, is not built"):      # the blocks' words
        nets.stem_bn_train(conv, bn, torch.zeros((2, 3, 4, 4)))
    blk = nets.BasicBlock(64, 64, 1)
    blk.bn1.momentum = None
    with pytest.raises(ValueError, match="momentum=None, the cumulative average, is not built"):
        nets.trunk_block_bn_train(blk, torch.zeros((2, 64, 2, 2)))
    assert "trunk_block_bn_train" in nets.stem_bn_train.__doc__ and "stem_train" in nets.stem_bn_train.__doc__


def _node():
    trunk = nets.make_trunk("resnet18")
    stages = dict(layer4=trunk[7], layer3=trunk[6], layer2=trunk[5], layer1=trunk[4])
    return trunk, nets.FeaturePyramidNetwork(512), nets.DBHead(256), [torch.zeros((1, 70, 70, 4), dtype=torch.float16)], stages


def test_forward_padded_stem_batch_stats():
    trunk, fpn, head, taps, stages = _node()
    stem = (trunk[0], trunk[1])
    node = "stem -> layer1 -> layer2 -> layer3 -> layer4 -> FPN -> head node with batch statistics"
    # the accepted node goes on to its own checks: a CPU image tap is refused as without the keyword, for a tuple and for a list
    for spelling in (STAGES, list(STAGES)):
        with pytest.raises(ValueError, match="image tap"):
            fpn.forward_padded(taps, head=head, stem=stem, trunk_batch_stats=spelling, stem_batch_stats=True, **stages)
    with pytest.raises(ValueError, match=node):      # without the stem
        fpn.forward_padded(taps, head=head, trunk_batch_stats=STAGES, stem_batch_stats=True, **stages)
    with pytest.raises(ValueError, match=node):      # the stem is a pair
        fpn.forward_padded(taps, head=head, stem=trunk[0], trunk_batch_stats=STAGES, stem_batch_stats=True, **stages)
    for short in (STAGES[1:], STAGES[2:], ("layer4",), True, False, ("stem",) + STAGES):      # anything but the four-stage tuple
        with pytest.raises(ValueError, match=node):
            fpn.forward_padded(taps, head=head, stem=stem, trunk_batch_stats=short, stem_batch_stats=True, **stages)
    with pytest.raises(ValueError, match=node):      # without a stage
        fpn.forward_padded(taps, head=head, stem=stem, trunk_batch_stats=STAGES, stem_batch_stats=True, **{k: v for k, v in stages.items() if k != "layer3"})
    with pytest.raises(ValueError, match=node):      # without the head
        fpn.forward_padded(taps, stem=stem, trunk_batch_stats=STAGES, stem_batch_stats=True, **stages)
    with pytest.raises(ValueError, match=node):      # True or False, nothing else
        fpn.forward_padded(taps, head=head, stem=stem, trunk_batch_stats=STAGES, stem_batch_stats=("stem",), **stages)
    # the stem's BatchNorm in another mode than the eight blocks
    trunk[1].eval()
    with pytest.raises(ValueError, match="mode .* of the eight blocks"):
        fpn.forward_padded(taps, head=head, stem=stem, trunk_batch_stats=STAGES, stem_batch_stats=True, **stages)
    trunk[1].train()
    for layer in stages.values():
        layer.eval()
    with pytest.raises(ValueError, match="mode .* of the eight blocks"):
        fpn.forward_padded(taps, head=head, stem=stem, trunk_batch_stats=STAGES, stem_batch_stats=True, **stages)
    trunk[1].eval()      # all in eval(): accepted, as far as the device check
    with pytest.raises(ValueError, match="image tap"):
        fpn.forward_padded(taps, head=head, stem=stem, trunk_batch_stats=STAGES, stem_batch_stats=True, **stages)
    # the stem keeps its own eps and momentum; the blocks' node-wide checks still hold
    trunk, fpn, head, taps, stages = _node()
    trunk[1].eps, trunk[1].momentum = 1e-3, 0.3
    with pytest.raises(ValueError, match="image tap"):
        fpn.forward_padded(taps, head=head, stem=(trunk[0], trunk[1]), trunk_batch_stats=STAGES, stem_batch_stats=True, **stages)
    trunk[1].momentum = None
    with pytest.raises(ValueError, match="momentum=None"):
        fpn.forward_padded(taps, head=head, stem=(trunk[0], trunk[1]), trunk_batch_stats=STAGES, stem_batch_stats=True, **stages)
    trunk[1].momentum = 0.1
    trunk[4][1].bn2.momentum = 0.2
    with pytest.raises(ValueError, match="eight blocks must be in one mode"):
        fpn.forward_padded(taps, head=head, stem=(trunk[0], trunk[1]), trunk_batch_stats=STAGES, stem_batch_stats=True, **stages)
    # without the keyword every call behaves as before
    trunk, fpn, head, taps, stages = _node()
    with pytest.raises(ValueError, match="takes no stem"):
        fpn.forward_padded(taps, head=head, stem=(trunk[0], trunk[1]), trunk_batch_stats=STAGES, **stages)
    with pytest.raises(ValueError, match="takes no stem"):
        fpn.forward_padded(taps, head=head, stem=(trunk[0], trunk[1]), trunk_batch_stats=STAGES, stem_batch_stats=False, **stages)


def test_dbnet_trunk_bn_backbone():
    net = nets.DBNet("resnet18", trainable=MODE, trunk_bn="backbone")
    assert net.trainable == MODE and net.trunk_bn == "backbone"
    assert list(net.state_dict()) == list(nets.DBNet("resnet18").state_dict())      # the state dict is the reference's, whatever the mode
    assert len(sc._trained(net)) == 90 and all(p.requires_grad for p in net.parameters())
    assert net.set_trainable(MODE).trunk_bn == "backbone"      # kept when trunk_bn is not given
    # refused where it does not fit, and the network is as it was
    for other in (L1_MODE, "head+fpn+layer4", "head+fpn", "head", None):
        with pytest.raises(ValueError, match="trunk_bn='backbone'"):
            net.set_trainable(other)
        assert net.trainable == MODE and net.trunk_bn == "backbone" and all(p.requires_grad for p in net.parameters())
    assert net.set_trainable(L1_MODE, "trained").trunk_bn == "trained"
    assert not net.backbone[0].weight.requires_grad
    assert net.set_trainable(MODE, "backbone").trunk_bn == "backbone" and net.backbone[0].weight.requires_grad
    assert net.set_trainable(None, "frozen").trunk_bn == "frozen"
    for other in (L1_MODE, "head+fpn+layer4+layer3", "head+fpn", None):
        with pytest.raises(ValueError, match="trunk_bn='backbone'.*trainable='head\\+fpn\\+backbone' on resnet18"):
            nets.DBNet("resnet18", trainable=other, trunk_bn="backbone")
    for mode in (None, "head+fpn", MODE):
        with pytest.raises(ValueError):
            nets.DBNet("resnet50", trainable=mode, trunk_bn="backbone")
    # the older spellings stay refused on the backbone mode, and say which spelling trains the stem's statistics
    with pytest.raises(ValueError, match=STEM_FROZEN + ".*trunk_bn='backbone'"):
        nets.DBNet("resnet18", trainable=MODE, trunk_bn="trained")
    with pytest.raises(ValueError, match=STEM_FROZEN):
        nets.DBNet("resnet18", trainable=MODE, trunk_bn=STAGES)
    with pytest.raises(ValueError, match="built for layer4 only.*" + STEM_FROZEN):
        nets.DBNet("resnet18", trainable=MODE, trunk_bn="batch")
    with pytest.raises(ValueError, match="trunk_bn must be"):
        nets.DBNet("resnet18", trainable=MODE, trunk_bn="stem")
    assert nets.DBNet("resnet18", trainable=MODE).trunk_bn == "frozen"      # the default
    assert "'backbone'" in nets.DBNet.set_trainable.__doc__ or '"backbone"' in nets.DBNet.set_trainable.__doc__


def test_dbnet_passes_the_batch_stem_to_the_node(monkeypatch):
    """The train-mode forward packs the image and hands the stem, the four stages, the four-stage tuple and stem_batch_stats=True to
    forward_padded; with the default trunk_bn it passes neither keyword."""
    seen = {}

    def forward_padded(taps, **kw):
        seen.clear()
        seen.update(kw, taps=taps)
        return "out"

    monkeypatch.setattr(nets, "pack_image", lambda x: "image")
    for trunk_bn in ("backbone", "frozen"):
        net = nets.DBNet("resnet18", trainable=MODE, trunk_bn=trunk_bn)
        monkeypatch.setattr(net.fpn, "forward_padded", forward_padded)
        monkeypatch.setattr(net, "trunk_engine", lambda: pytest.fail("the backbone mode reads no trunk engine"))
        for m in (net.backbone, net.fpn, net.head):
            monkeypatch.setattr(m, "cuda", lambda: None)
        version = net._version
        assert net.train()(torch.zeros((2, 3, 640, 640))) == "out"
        assert seen["taps"] == ["image"] and seen["head"] is net.head and seen["stem"] == (net.backbone[0], net.backbone[1])
        for j in (1, 2, 3, 4):
            assert seen[f"layer{j}"] is net.backbone[3 + j]
        if trunk_bn == "backbone":
            assert seen["stem_batch_stats"] is True and seen["trunk_batch_stats"] == STAGES
        else:
            assert "stem_batch_stats" not in seen and "trunk_batch_stats" not in seen
        assert net._version == version + 1      # the running statistics moved: the next eval() forward rebuilds the inference engine
    # the stem's buffers are among the tensors the eval() forward watches
    net = nets.DBNet("resnet18", trainable=MODE, trunk_bn="backbone")
    before = net._head_tensor_versions()
    net.backbone[1].running_var.add_(1.0)
    assert net._head_tensor_versions() != before


def test_raw_wrappers_take_the_batch_family(monkeypatch):
    """With `bn`, the raw wrappers run vtd_stem_bn_train_* in either mode (the frozen hand-over is the library's); without it, vtd_stem_train_*."""
    asked = []

    def workspace(query, args, device):
        asked.append((query, args))
        raise LookupError

    monkeypatch.setattr(nets, "_native_workspace", workspace)
    t = torch.zeros(1)
    for bn in ((True, 0.1), (False, 0.1), None):
        extra = () if bn is None else (bn,)
        with pytest.raises(LookupError):
            nets._stem_forward_raw(t, (2, 4, 4), 1e-5, [t] * 3, [t] * 2, *extra)
        with pytest.raises(LookupError):
            nets._stem_backward_raw(t, (2, 4, 4), 1e-5, [t] * 3, [t] * 2, t, t, t, t, t, *extra)
    bnq, frq = "vtd_stem_bn_train_workspace_bytes", "vtd_stem_train_workspace_bytes"
    assert asked == [(bnq, (2, 4, 4, 0)), (bnq, (2, 4, 4, 1))] * 2 + [(frq, (2, 4, 4, 0)), (frq, (2, 4, 4, 1))]


# ---- fp64 controls of the arithmetic the kernels implement
def _ste(w):
    return w + (w.half().to(w.dtype) - w).detach()


def ref_stem_bn(ref, x, seen):
    """The stem in ref's dtype with train-mode BatchNorm, the reference of tests/test_gpu_stem_bn_train.py: the convolution weights rounded to
    fp16 straight through, a = relu(bn(z)) rounded to fp16 straight through, (pooled map, torch's CPU indices).  `seen` collects (mu,
    sigma^2); the call moves ref's running buffers."""
    conv, bn = ref
    z = F.conv2d(x, _ste(conv.weight), None, 2, 3)
    seen.append((z.detach().mean((0, 2, 3)), z.detach().var((0, 2, 3), unbiased=False)))
    a = F.relu(F.batch_norm(z, bn.running_mean, bn.running_var, bn.weight, bn.bias, True, bn.momentum, bn.eps))
    a = a + (a.half().to(a.dtype) - a).detach()
    return F.max_pool2d(a, 3, 2, 1, return_indices=True)


_CONTROL = {}


def _control_case(size):
    """Autograd of the plain train-mode stem in fp64 (nothing rounded), and the quantities the kernels start from."""
    if size not in _CONTROL:
        conv, bn = (copy.deepcopy(m).double() for m in sc.stem_modules())
        x, up = (t.double() for t in sc.stem_inputs(size))
        z = F.conv2d(x, conv.weight, None, 2, 3)
        a = F.relu(F.batch_norm(z, None, None, bn.weight, bn.bias, True, 0.1, bn.eps))
        F.max_pool2d(a, 3, 2, 1).backward(up)
        want = [conv.weight.grad.clone(), bn.weight.grad.clone(), bn.bias.grad.clone()]
        _CONTROL[size] = dict(conv=conv, bn=bn, x=x, up=up, z=z.detach(), a=a.detach(), want=want)
    return _CONTROL[size]


def _kernel_grads(c, bug=None):
    """The kernels' backward in fp64: m = up (pool > 0); s1 = sum m and s2 = sum m xh[the position idx names] at pooled resolution; g gathered
    by the window-membership rule; dz = gamma rstd (g - s1 / M - xh s2 / M), M the conv rows; dW from dz in the kernel's column order."""
    bn, x, up, z, a = c["bn"], c["x"], c["up"], c["z"], c["a"]
    n, _, hc, wc = z.shape
    mu, var = z.mean((0, 2, 3)), z.var((0, 2, 3), unbiased=False)
    rstd = 1.0 / torch.sqrt(var + bn.eps)
    xh = (z - mu[None, :, None, None]) * rstd[None, :, None, None]
    pool, code = sc.window_codes(a)
    hp, wp = pool.shape[2:]
    m = up * (pool > 0)
    py, px = torch.meshgrid(torch.arange(hp), torch.arange(wp), indexing="ij")
    cy, cx = (2 * py - 1 + code // 3).clamp(0, hc - 1), (2 * px - 1 + code % 3).clamp(0, wc - 1)      # in-image wherever m is not 0
    xh_at = xh.reshape(n, 64, -1).gather(2, (cy * wc + cx).reshape(n, 64, -1)).reshape(n, 64, hp, wp)
    s1, s2 = m.sum((0, 2, 3)), (m * xh_at).sum((0, 2, 3))
    M = n * hp * wp if bug == "pooled rows" else n * hc * wc
    g = sc.route(m, code, hc, wc)
    third = 0.0 if bug == "no s2 term" else xh * (s2 / M)[None, :, None, None]
    dz = (bn.weight.detach() * rstd)[None, :, None, None] * (g - (s1 / M)[None, :, None, None] - third)
    return [sc.kernel_order_wgrad(x, dz)[0], s2, s1], (g, xh)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pooled_resolution_sums_and_dense_dz_match_autograd(size):
    c = _control_case(size)
    gam, bet = c["bn"].weight.detach(), c["bn"].bias.detach()
    assert float(gam[ZERO_CH]) == 0.0 and float(bet[ZERO_CH]) > 0 and float(gam[NEG_CH]) < 0
    (dw, dgamma, dbeta), (g, xh) = _kernel_grads(c)
    # every live pooled element routes to exactly one conv position: the pooled-resolution sums are the sums over the conv map of g and g xh
    assert _rel(dbeta.numpy(), g.sum((0, 2, 3)).numpy()) <= 1e-13 and _rel(dgamma.numpy(), (g * xh).sum((0, 2, 3)).numpy()) <= 1e-13
    for got, want in zip((dw, dgamma, dbeta), c["want"]):
        assert got.shape == want.shape and _rel(got.numpy(), want.numpy()) <= 1e-12
    assert float(dw[ZERO_CH].abs().max()) == 0.0 and float(dgamma[ZERO_CH].abs()) > 0      # gamma = 0: dW vanishes exactly, dgamma does not


@pytest.mark.parametrize("bug", ["no s2 term", "pooled rows"])
def test_negative_controls(bug):
    """Leaving out the xh s2 / M term, or dividing by the pooled row count, must miss dW by at least 10x the gradient ceiling."""
    c = _control_case((10, 14))
    (dw, _, _), _ = _kernel_grads(c, bug)
    err = _rel(dw.numpy(), c["want"][0].numpy())
    assert err >= 10 * GRAD_CEILING, (bug, err)


def test_reduce_geometry_of_the_four_sizes():
    """The statistics' rows are the conv pixels M = n hc wc: min(256, ceil(M / 256)) workgroups of ceil(M / workgroups) rows, sixteen parts
    each (tests/test_layer1_bn_train.py writes the order out)."""
    geo = {}
    for H, W in SIZES:
        M = 2 * (H // 2) * (W // 2)
        red = min(256, max(1, -(-M // 256)))
        per = -(-M // red)
        geo[(H, W)] = (M, red, per, M - (red - 1) * per, sc.slabs(M)[0])
    assert geo[(4, 4)][:3] == (8, 1, 8) and sum(x == y for x, y in zip(l1b._cuts16(8), l1b._cuts16(8)[1:])) == 8      # eight empty parts
    assert geo[(10, 14)][:3] == (70, 1, 70)
    assert geo[(36, 44)][:4] == (792, 4, 198, 198)
    assert geo[(54, 38)] == (1026, 5, 206, 202, 2)      # a last workgroup of 202 rows, and two weight-gradient slabs
    assert sum(x == y for x, y in zip(l1b._cuts16(2), l1b._cuts16(2)[1:])) == 14      # the 2 x 2 image: M = 2
    assert 2 * 320 * 320 == 204800 and min(256, -(-204800 // 256)) == 256 and -(-204800 // 256) == 800      # the bench shape


@pytest.mark.parametrize("size", SIZES + [(2, 2), (68, 84)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_tile_ownership_covers_every_conv_pixel_once(size):
    """The forward's tile (ty, tx) computes conv rows 14 ty - 1 .. 14 ty + 13 and columns 16 tx - 1 .. 16 tx + 15 (15 x 17, the pool's halo) and
    writes its local rows 1 .. 14 and columns 1 .. 16 that lie inside the conv map: every conv pixel is written by exactly one tile, the
    tile (y // 14, x // 16).  (68, 84) has three tiles per direction."""
    hc, wc = size[0] // 2, size[1] // 2
    hp, wp = (hc + 1) // 2, (wc + 1) // 2
    tiles_y, tiles_x = -(-hp // 7), -(-wp // 8)
    if size == (68, 84):
        assert (tiles_y, tiles_x) == (3, 3)
    writes = torch.zeros((hc, wc), dtype=torch.int64)
    owner = torch.full((hc, wc, 2), -1)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            for pix in range(256):      # the 256 GEMM rows of the tile, the last one idle
                c_row, c_col = divmod(pix, 17)
                cy, cx = 14 * ty - 1 + c_row, 16 * tx - 1 + c_col
                if 1 <= c_row <= 14 and 1 <= c_col <= 16 and cy < hc and cx < wc:
                    writes[cy, cx] += 1
                    owner[cy, cx] = torch.tensor([ty, tx])
    assert int(writes.min()) == 1 and int(writes.max()) == 1
    ys, xs = torch.meshgrid(torch.arange(hc), torch.arange(wc), indexing="ij")
    assert torch.equal(owner[..., 0], ys // 14) and torch.equal(owner[..., 1], xs // 16)


# ---- the chain of the GPU node test (tests/test_gpu_stem_bn_train.py) and the float32 stand-in by which its seeds were chosen
# The node test is stage-isolated, so a ReLU sign that differs between a reference stage's output and the stored tap moves one element of a
# mask and with it every gradient below, whatever the kernels do (tests/test_gpu_layer2_bn_train.py, at CHAIN_BASE).  The seeds were chosen on
# the CPU before the first GPU run by the protocol written there: a float32 evaluation of the whole chain on the image (every stage reading
# the stage before's output rounded to fp16) stands in for the kernels, the float64 references are built on its taps as the node test builds
# them on the kernels', and a seed pair is taken only if the two agree on every ReLU sign of the pooled map and of all eight block outputs.
# Layer2 .. layer4, the FPN, the head and the targets are tests/test_layer1_train.py's chain; the image is tests/test_gpu_stem_train.py's chain
# image (unit variance).  Layer1's seed stays that chain's own (61); the stem's seeds were tried upwards from that file's 75 (flips of the
# pooled map, layer1.0, layer1.1, layer2.0, layer2.1, layer3.0, layer3.1, layer4.0, layer4.1):
#   75: [0, 0, 3, 0, 0, 0, 0, 0, 1]
#   76: [0, 0, 0, 0, 1, 0, 0, 0, 0]
#   77: [0, 0, 1, 0, 1, 0, 1, 0, 0]
#   78: [0, 0, 2, 0, 4, 0, 2, 0, 0]
#   79: [0, 0, 0, 0, 0, 0, 0, 0, 0]      the first without a flip: taken
CHAIN_STEM_SEED, CHAIN_L1_SEED, CHAIN_IMAGE_SCALE = 79, l1c.CHAIN_SEED, 2.0


def chain_modules(stem_seed=CHAIN_STEM_SEED, l1_seed=CHAIN_L1_SEED):
    """(the stem, the eight blocks, the FPN, the head, the image [2,3,96,64], the targets) on the CPU in float32, all in train mode."""
    (l1, l2, l3, l4, fpn, head), _, targets = l1c.chain_modules(l1_seed)
    stem = torch.nn.Sequential(*sc.stem_modules(stem_seed)).train()
    x = (sc.stem_inputs((96, 64))[0] * CHAIN_IMAGE_SCALE).half().float()
    return stem, [b.train() for m in (l1, l2, l3, l4) for b in m], fpn, head.train(), x, targets


def _ref_block_bn(blk, x):
    """A BasicBlock in x's dtype with train-mode BatchNorm, conv weights and a1 (and the downsample's output) rounded to fp16."""
    def pair(t, conv, bn, stride, pad):
        z = F.conv2d(t, conv.weight.half().to(t.dtype), None, stride, pad)
        return F.batch_norm(z, None, None, bn.weight, bn.bias, True, 0.1, bn.eps)
    a1 = F.relu(pair(x, blk.conv1, blk.bn1, blk.stride, 1)).half().to(x.dtype)
    idt = pair(x, blk.downsample[0], blk.downsample[1], blk.stride, 0).half().to(x.dtype) if hasattr(blk, "downsample") else x
    return F.relu(pair(a1, blk.conv2, blk.bn2, 1, 1) + idt)


def chain_flips(stem_seed=CHAIN_STEM_SEED, l1_seed=CHAIN_L1_SEED):
    """ReLU signs that differ between the float32 stand-in and the float64 references built on its taps: the pooled map, then the eight
    block outputs."""
    stem, blocks, _, _, x, _ = chain_modules(stem_seed, l1_seed)
    with torch.no_grad():
        pool32 = ref_stem_bn(copy.deepcopy(stem), x, [])[0]
        pool64 = ref_stem_bn(copy.deepcopy(stem).double(), x.double(), [])[0]
        flips = [int(((pool32 > 0) != (pool64 > 0)).sum())]
        t = pool32      # fp16-representable: a was rounded
        for i in range(0, 8, 2):
            b0, b1 = blocks[i], blocks[i + 1]
            mid32 = _ref_block_bn(b0, t)
            out32 = _ref_block_bn(b1, mid32.half().float())
            d0, d1 = copy.deepcopy(b0).double(), copy.deepcopy(b1).double()
            mid64 = _ref_block_bn(d0, t.double())
            out64 = _ref_block_bn(d1, mid64.half().double())      # the reference stage's second block reads its own first block's output
            flips += [int(((mid32 > 0) != (mid64 > 0)).sum()), int(((out32 > 0) != (out64 > 0)).sum())]
            t = out32.half().float()
    return flips


def test_chain_seeds_have_no_flip_in_the_float32_stand_in():
    flips = chain_flips()
    print(f"flips of the float32 stand-in against float64 at stem seed {CHAIN_STEM_SEED}, layer1 seed {CHAIN_L1_SEED}: {flips}")
    assert len(flips) == 9 and flips == [0] * 9
