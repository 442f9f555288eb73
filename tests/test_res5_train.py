"""ResNet-50's last stage (res5) on the HIP training kernels (csrc/bottleneck_train.hip), without a device: the new C entry points exist and
refuse bad arguments before any launch, the workspace query equals its documented formula, the Python surface's refusals, the
"head+fpn+res5" mode's bookkeeping, and the Bottleneck backward written out in fp64 exactly as the kernels form it (the masks, the
transposed 1x1 GEMMs, the zero-inserted plane, the downsample's transpose at the even positions, the convolution + BatchNorm identities)
against torch autograd -- with negative controls that must miss autograd by at least 10x the GPU tests' gradient ceiling.

The written-out reference runs on 8-wide blocks (16 -> 8 -> 32 at stride 2, 32 -> 8 -> 32 at stride 1): a relative L2 miss of a wrong
formula does not depend on the width.  tests/test_gpu_res5_train.py checks the kernels themselves."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vtd_amd import _native, nets

GRAD_CEILING = 1e-2      # of tests/test_gpu_res5_train.py
GEOMS = {2: (1024, 512, 2), 1: (2048, 512, 1)}


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _aligned(nbytes, align=256):
    raw = (C.c_char * (nbytes + 2 * align))()
    return raw, C.c_void_p((C.addressof(raw) + align - 1) // align * align)


# ---- C ABI, no device
def test_new_symbols_are_exported_and_bound():
    lib = _native.load()
    for name in ("vtd_bottleneck_train_workspace_bytes", "vtd_bottleneck_train_forward", "vtd_bottleneck_train_backward"):
        assert name in _native.SIGNATURES and hasattr(lib, name), name
    assert len(_native.BottleneckParams._fields_) == 20 and C.sizeof(_native.BottleneckParams) == 20 * C.sizeof(C.c_void_p)
    for code in (-3901, -3902):
        assert b"Bottleneck training" in lib.vtd_strerror(code)


def _workspace_formula(n, hin, win, cin, stride, mode):
    """include/vtd.h, vtd_bottleneck_train_workspace_bytes."""
    a256 = lambda b: (b + 255) // 256 * 256  # noqa: E731
    S = lambda r: min(8, max(1, -(-r // 4096)))  # noqa: E731
    W, h, w, ds = 512, hin // stride, win // stride, stride == 2
    pin, pout, M, Min = n * (hin + 2) * (win + 2), n * (h + 2) * (w + 2), n * h * w, n * hin * win
    if mode == 0:
        return (a256(2 * pin * W) + a256(2 * pout * W) + (a256(2 * pout * 4 * W) if ds else 0) + a256(2 * W * cin) + a256(2 * W * 9 * W) +
                a256(2 * 4 * W * W) + (a256(2 * 4 * W * cin) if ds else 0) + a256(4 * (2 * W + 2 * 4 * W)))
    return (a256(4 * M * 4 * W) + a256(4 * M * W) + a256(4 * Min * W) + a256(2 * M * 4 * W) + a256(2 * M * W) + a256(2 * Min * W) +
            a256(2 * pout * 4 * W) + 2 * a256(2 * pin * W) + a256(2 * W * 9 * W) + a256(4 * 4 * W) + a256(8 * 256 * 4 * W) + a256(4 * 256) +
            a256(8 * 4 * W) + 2 * a256(8 * W) + a256(48) + a256(4 * max(S(M) * W * 9 * W, S(Min) * W * cin)))


def test_workspace_query_equals_its_formula():
    ws = _native.load().vtd_bottleneck_train_workspace_bytes
    for n, h, w in ((1, 2, 2), (2, 6, 4), (32, 40, 40)):
        for stride, (cin, width, _) in GEOMS.items():
            for mode in (0, 1):
                got = ws(n, h, w, cin, width, stride, mode)
                assert got == _workspace_formula(n, h, w, cin, stride, mode) and got % 256 == 0, (n, h, w, stride, mode)
    bad = [(2, 6, 4, 1024, 256, 2),      # width 256
           (2, 6, 4, 512, 512, 2), (2, 6, 4, 512, 512, 1),      # cin 512
           (2, 5, 4, 1024, 512, 2), (2, 6, 3, 1024, 512, 2),      # stride 2 with odd extents
           (2, 6, 4, 1024, 512, 1),      # stride 1 with cin 1024
           (2, 6, 4, 2048, 512, 2), (2, 6, 4, 2048, 512, 3),
           (0, 6, 4, 1024, 512, 2), (2, 0, 4, 2048, 512, 1), (2, 6, -2, 1024, 512, 2),      # zero extents
           (1 << 16, 6, 4, 1024, 512, 2), (2, 4098, 4, 1024, 512, 2), (2, 4, 8192, 2048, 512, 1), (4096, 64, 64, 2048, 512, 1)]      # huge
    for g in bad:
        assert ws(*g, 0) == -3901 and ws(*g, 1) == -3901, g
    assert ws(2, 6, 4, 1024, 512, 2, 2) == -3901 and ws(2, 6, 4, 1024, 512, 2, -1) == -3901


def _struct(buf, fields=_native.BOTTLENECK_FIELDS):
    st = _native.BottleneckParams()
    for f in fields:
        setattr(st, f, buf)
    return st


DS_FIELDS = [f for f in _native.BOTTLENECK_FIELDS if f.startswith("ds_")]
LEARN_FIELDS = [f for f in _native.BOTTLENECK_FIELDS if not f.endswith(("_mean", "_var"))]


@pytest.mark.parametrize("stride", [2, 1])
def test_forward_argument_and_alignment_errors(stride):
    """Every refusal comes before any launch, so none of this needs a device."""
    fwd = _native.load().vtd_bottleneck_train_forward
    keep = [_aligned(4096) for _ in range(4)]
    x, ws, y, w = (k[1] for k in keep)
    cin, width, _ = GEOMS[stride]
    st = _struct(w)
    good = [x, 2, 6, 4, cin, width, stride, C.byref(st), 1e-5, ws, y, None]
    for i in (0, 7, 9, 10):      # x, params, workspace, y
        a = list(good)
        a[i] = None
        assert fwd(*a) == -3901, i
    for i, v in ((1, 0), (2, 0), (3, -4), (4, 512), (5, 256), (6, 3 - stride), (8, 0.0), (8, -1.0), (1, 1 << 16), (2, 4098)):      # mis-sized
        a = list(good)
        a[i] = v
        assert fwd(*a) == -3901, (i, v)
    if stride == 2:
        a = list(good)
        a[2] = 5
        assert fwd(*a) == -3901
    for f in _native.BOTTLENECK_FIELDS:
        if stride == 1 and f in DS_FIELDS:      # the identity block ignores ds_*: such a call would pass the checks and launch
            continue
        for value, want in ((None, -3901), (C.c_void_p(w.value + 2), -3902)):
            st2 = _struct(w)
            setattr(st2, f, value)
            a = list(good)
            a[7] = C.byref(st2)
            assert fwd(*a) == want, f
    for i, off in ((0, 8), (10, 8), (9, 128)):      # x and y 16 bytes, the workspace 256
        a = list(good)
        a[i] = C.c_void_p(a[i].value + off)
        assert fwd(*a) == -3902, i


@pytest.mark.parametrize("stride", [2, 1])
def test_backward_argument_and_alignment_errors(stride):
    bwd = _native.load().vtd_bottleneck_train_backward
    keep = [_aligned(4096) for _ in range(9)]
    x, ws, y, dy, dscale, scratch, dx, dxscale, w = (k[1] for k in keep)
    cin, width, _ = GEOMS[stride]
    st, gst = _struct(w), _struct(w, LEARN_FIELDS)
    good = [x, 2, 6, 4, cin, width, stride, C.byref(st), 1e-5, ws, y, dy, dscale, C.byref(gst), scratch, dx, dxscale, None]
    for i in (0, 7, 9, 10, 11, 12, 13, 14, 16):      # every pointer but dx, which is optional; dx without its scale is refused
        a = list(good)
        a[i] = None
        assert bwd(*a) == -3901, i
    for i, v in ((1, 0), (2, 0), (3, -4), (4, 512), (5, 256), (6, 3 - stride), (8, 0.0), (1, 1 << 16), (3, 4098)):
        a = list(good)
        a[i] = v
        assert bwd(*a) == -3901, (i, v)
    for which, fields in ((7, _native.BOTTLENECK_FIELDS), (13, LEARN_FIELDS)):
        for f in fields:
            if stride == 1 and f in DS_FIELDS:
                continue
            for value, want in ((None, -3901), (C.c_void_p(w.value + 2), -3902)):
                s2 = _struct(w, fields)
                setattr(s2, f, value)
                a = list(good)
                a[which] = C.byref(s2)
                assert bwd(*a) == want, (which, f)
    for i, off in ((0, 8), (10, 8), (11, 8), (15, 8), (9, 128), (14, 128), (12, 4), (16, 4)):
        a = list(good)
        a[i] = C.c_void_p(a[i].value + off)
        assert bwd(*a) == -3902, i


# ---- the Python surface's refusals
def test_bottleneck_train_refusals():
    b2, b1 = nets.Bottleneck(1024, 512, 2), nets.Bottleneck(2048, 512, 1)
    with pytest.raises(RuntimeError, match="parameter containers"):      # the module call keeps refusing
        b1(torch.zeros((1, 2048, 2, 2)))
    for other in (nets.BasicBlock(512, 512, 1), nets.Bottleneck(256, 64, 1), nets.Bottleneck(512, 256, 2), nets.Bottleneck(1024, 512, 1),
                  torch.nn.Conv2d(4, 4, 1)):
        with pytest.raises(RuntimeError, match="1024 -> 512 -> 2048 stride 2"):
            nets.bottleneck_train(other, torch.zeros((1, 1024, 2, 2)))
    with pytest.raises(ValueError, match="CUDA"):
        nets.bottleneck_train(b2, torch.zeros((1, 1024, 4, 2)))
    with pytest.raises(ValueError, match="CUDA"):
        nets.bottleneck_train(b1, torch.zeros((1, 2048, 3, 1), dtype=torch.float16))
    with pytest.raises(RuntimeError, match="even extents"):
        nets.bottleneck_train(b2, torch.zeros((1, 1024, 3, 2)))
    for x in (torch.zeros((1, 2048, 4, 2)), torch.zeros((1024, 4, 2)), None):      # a wrong channel count, not a 4-d tensor
        with pytest.raises(ValueError, match=r"\[n,1024,H,W\]"):
            nets.bottleneck_train(b2, x)
    odd = nets.Bottleneck(2048, 512, 1)
    odd.bn3.eps = 1e-3
    with pytest.raises(ValueError, match="one eps"):
        nets.bottleneck_train(odd, torch.zeros((1, 2048, 2, 2)))
    nostats = nets.Bottleneck(2048, 512, 1)
    nostats.bn2 = torch.nn.BatchNorm2d(512, track_running_stats=False)
    with pytest.raises(ValueError, match="running stats"):
        nets.bottleneck_train(nostats, torch.zeros((1, 2048, 2, 2)))
    # the BasicBlock functions keep refusing a Bottleneck as they did
    for fn in (nets.basic_block_train, nets.basic_block_bn_train, nets.trunk_block_bn_train):
        with pytest.raises(RuntimeError, match="Bottleneck training is not built"):
            fn(b1, torch.zeros((1, 2048, 2, 2)))


def _meta_taps(n=1, h5=1, w5=1):
    return [torch.empty((n, (h5 << (3 - lv)) + 2, (w5 << (3 - lv)) + 2, 2048 >> (3 - lv)), dtype=torch.float16) for lv in range(3)]


def test_forward_padded_res5_refusals():
    net = nets.DBNet("resnet50")
    r18 = nets.DBNet("resnet18")
    fpn, head, res5 = net.fpn, net.head, net.backbone[7]
    taps = _meta_taps()
    for kw in ({"layer4": r18.backbone[7]}, {"layer3": r18.backbone[6]}, {"layer2": r18.backbone[5]}, {"layer1": r18.backbone[4]},
               {"stem": (r18.backbone[0], r18.backbone[1])}, {"trunk_batch_stats": True}, {"trunk_batch_stats": ("layer4",)}, {"stem_batch_stats": True}):
        with pytest.raises(ValueError, match="res5 -> FPN -> head node"):
            fpn.forward_padded(taps, head=head, res5=res5, **kw)
    with pytest.raises(ValueError, match="needs the DBHead"):
        fpn.forward_padded(taps, res5=res5)
    with pytest.raises(ValueError, match="CUDA"):      # CPU taps: there is no CPU path
        fpn.forward_padded(taps, head=head, res5=res5)
    with pytest.raises(ValueError, match=r"\[C2, C3, C4\]"):
        fpn.forward_padded(taps[:2], head=head, res5=res5)
    # the stage itself, judged on shapes alone: ResNet-18's layer4, a shortened stage, a C4 of odd extents or the wrong width
    c4 = torch.empty((1, 4, 4, 1024), dtype=torch.float16, device="meta")
    for layer, tap in ((r18.backbone[7], c4), (torch.nn.Sequential(*list(res5)[:2]), c4), (net.backbone[6], c4),
                       (res5, torch.empty((1, 5, 4, 1024), dtype=torch.float16, device="meta")),
                       (res5, torch.empty((1, 4, 4, 512), dtype=torch.float16, device="meta"))):
        with pytest.raises(RuntimeError, match="three Bottlenecks of width 512"):
            nets._res_operands(nets._RES_STAGES[3], layer, tap, torch.device("cpu"))
    with pytest.raises(RuntimeError, match="three Bottlenecks of width 512"):
        nets.forward_res5_padded(r18.backbone[7], torch.empty((1, 4, 4, 1024), dtype=torch.float16))
    with pytest.raises(ValueError, match="CUDA"):
        nets.forward_res5_padded(res5, torch.empty((1, 4, 4, 1024), dtype=torch.float16))
    # the ResNet-18 stage helpers keep refusing Bottleneck stages
    with pytest.raises(RuntimeError, match="Bottleneck training is not built"):
        nets._stage_operands(nets._STAGES[3], res5, c4)
    with pytest.raises(RuntimeError, match="Bottleneck training is not built"):
        nets.forward_layer4_padded(res5, c4)


def test_node_walks_three_blocks_in_one_stage(monkeypatch):
    """The trunk node on a plan of three blocks per stage: C5 is the third block's output, dC5 alone is asked of the FPN, blocks 2 and 1 form
    their input gradients and block 0 none, and nothing is combined.  The raw wrappers are replaced by recorders (no device)."""
    ev = []
    mk = lambda *shape: torch.zeros(shape)  # noqa: E731

    def block_fwd(tap, geom, eps, learn, stats, entry="x", bn=None):
        ev.append(("fwd", stats, entry, bn, tuple(tap.shape)))
        n, h, w, cin, width, stride = geom
        return mk(n, h // stride + 2, w // stride + 2, 4 * width), mk(8)

    def block_bwd(tap, geom, eps, learn, stats, ws, y, dy, dscale, want_dx, entry="x", bn=None):
        ev.append(("bwd", stats, entry, tuple(dy.shape), bool(want_dx)))
        n, h, w, cin, width, stride = geom
        return [p.detach().clone() for p in learn], (mk(n, h, w, cin) if want_dx else None), (mk(2) if want_dx else None)

    def fpn_bwd(taps, geom, params, ws, dp2, dscale, input_mask=0):
        ev.append(("fpn_bwd", tuple(t.shape[3] for t in taps), input_mask))
        n, h5, w5, c5 = geom
        return [p.detach().clone() for p in params], [None, None, None, mk(n, h5, w5, c5)], torch.zeros((4, 2))

    monkeypatch.setattr(nets, "_block_forward_raw", block_fwd)
    monkeypatch.setattr(nets, "_block_backward_raw", block_bwd)
    monkeypatch.setattr(nets, "_fpn_forward_raw", lambda taps, geom, params: (ev.append(("fpn_fwd", tuple(t.shape[3] for t in taps))), (mk(1, 10, 10, 256), mk(8)))[1])
    monkeypatch.setattr(nets, "_fpn_backward_raw", fpn_bwd)
    monkeypatch.setattr(nets, "_head_forward_raw", lambda feats, hw, *a: (mk(8), mk(1, 1, 32, 32), mk(1, 1, 32, 32), mk(4, 2, 64)))
    monkeypatch.setattr(nets, "_head_backward_raw", lambda feats, hw, tr, ws, prob, thresh, params, gp, gt, want: ([p.detach().clone() for p in params], mk(1, 8, 8, 256), mk(2)))
    monkeypatch.setattr(nets, "_combine_scaled", lambda *a: pytest.fail("nothing is combined in the res5 node"))
    geoms = [(1, 2, 2, 1024, 512, 2), (1, 1, 1, 2048, 512, 1), (1, 1, 1, 2048, 512, 1)]
    blocks = tuple(nets._BlockPlan(g, i, nets._BOTTLENECK, 12 if i == 0 else 9) for i, g in enumerate(geoms))
    plan = nets._TrunkPlan(tuple(_meta_taps()), (1, 1, 1, 2048), (True, 0.1, 1e-5, ()), None, blocks, 1e-5, None, 3)
    params = [torch.full((1,), float(i), requires_grad=True) for i in range(30 + 30)]
    prob, thresh, _ = nets._TrunkFPNHeadTrainFn.apply(plan, *params)
    torch.autograd.backward([prob, thresh], [torch.ones_like(prob), torch.ones_like(thresh)])
    B = nets._BOTTLENECK
    assert ev == [("fwd", 0, B, None, (1, 4, 4, 1024)), ("fwd", 1, B, None, (1, 3, 3, 2048)), ("fwd", 2, B, None, (1, 3, 3, 2048)),
                  ("fpn_fwd", (256, 512, 1024, 2048)), ("fpn_bwd", (256, 512, 1024, 2048), 8),
                  ("bwd", 2, B, (1, 1, 1, 2048), True), ("bwd", 1, B, (1, 1, 1, 2048), True), ("bwd", 0, B, (1, 1, 1, 2048), False)]
    assert all(p.grad is not None and float(p.grad) == float(i) for i, p in enumerate(params))
    assert nets._TrunkPlan((), None, None, None, (), None, None).per == 2      # ResNet-18's plans keep two blocks per stage


# ---- the "head+fpn+res5" mode
def _grad_pattern(net):
    return {k: p.requires_grad for k, p in net.named_parameters()}


def test_res5_mode_bookkeeping():
    keys = list(nets.DBNet("resnet50").state_dict())
    net = nets.DBNet("resnet50", trainable="head+fpn+res5")
    assert net.trainable == "head+fpn+res5" and net.trunk_bn == "frozen"
    assert list(net.state_dict()) == keys
    pat = _grad_pattern(net)
    trained = [k for k, v in pat.items() if v]
    assert all(k.startswith(("backbone.7.", "fpn.", "head.")) for k in trained)
    assert not any(v for k, v in pat.items() if k.startswith("backbone.") and not k.startswith("backbone.7."))
    assert sum(k.startswith("backbone.7.") for k in trained) == 30 and len(list(net.backbone[7].buffers())) == 30      # 12 + 9 + 9
    assert all(v for k, v in pat.items() if k.startswith(("fpn.", "head.")))
    # the fused inference engine is rebuilt after res5's tensors change: the version key covers its 30 parameters and 30 buffers
    n_head = len(list(net.head.parameters())) + len(list(net.head.buffers()))
    assert len(net._head_tensor_versions()) == n_head + len(list(net.fpn.parameters())) + 60
    v0 = net._head_tensor_versions()
    with torch.no_grad():
        net.backbone[7][2].bn3.running_var.add_(1.0)
    assert net._head_tensor_versions() != v0
    # switching from and to "head+fpn"
    net.set_trainable("head+fpn")
    assert not any(v for k, v in _grad_pattern(net).items() if k.startswith("backbone."))
    assert net.set_trainable("head+fpn+res5") is net and _grad_pattern(net) == pat
    other = nets.DBNet("resnet50", trainable="head+fpn").set_trainable("head+fpn+res5")
    assert _grad_pattern(other) == pat


def test_res5_mode_refusals():
    with pytest.raises(ValueError, match=r"head\+fpn\+layer4"):
        nets.DBNet("resnet18", trainable="head+fpn+res5")
    r18 = nets.DBNet("resnet18", trainable="head+fpn")
    with pytest.raises(ValueError, match=r"head\+fpn\+layer4"):
        r18.set_trainable("head+fpn+res5")
    assert r18.trainable == "head+fpn"
    for bn in ("batch", "trained", "backbone", ("layer4",), ("res5",), "bogus", 3):
        with pytest.raises(ValueError):
            nets.DBNet("resnet50", trainable="head+fpn+res5", trunk_bn=bn)
    net = nets.DBNet("resnet50", trainable="head+fpn+res5")
    with pytest.raises(ValueError, match="frozen-statistics"):
        net.set_trainable("head+fpn+res5", trunk_bn="batch")
    assert net.trainable == "head+fpn+res5" and net.trunk_bn == "frozen"
    # the older spellings keep refusing resnet50
    for mode in nets._STAGE_MODES + (nets._BACKBONE_MODE,):
        with pytest.raises(ValueError, match="Bottleneck training is not built"):
            nets.DBNet("resnet50", trainable=mode)
        with pytest.raises(ValueError, match="Bottleneck training is not built"):
            net.set_trainable(mode)
    # a frozen trunk tensor that requires grad is refused in a train-mode forward before anything touches a device
    net.train()
    net.backbone[6][0].conv1.weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match=r"backbone\.6\.0\.conv1\.weight requires grad"):
        net(torch.zeros((1, 3, 640, 640)))


# ---- the Bottleneck backward as the kernels form it, in fp64, against autograd
WIDTH = 8


def _small_block(stride, seed):
    cin = 2 * WIDTH if stride == 2 else 4 * WIDTH
    blk = nets.Bottleneck(cin, WIDTH, stride)
    blk.load_state_dict(nets.seeded_state_dict(lambda: nets.Bottleneck(cin, WIDTH, stride), seed))
    with torch.no_grad():
        blk.bn3.weight[3] = 0.0
        blk.bn3.weight[7] = -0.75
        blk.bn1.weight[2] = 0.0
        blk.bn2.weight[5] = -1.25
    return blk.double()


def _pairs(blk):
    return nets._bottleneck_pairs(blk)


def _fold(conv, bn):
    rstd = 1.0 / torch.sqrt(bn.running_var + bn.eps)
    scale = bn.weight * rstd
    return conv.weight * scale[:, None, None, None], bn.bias - bn.running_mean * scale, scale, rstd


def _block_forward(blk, x):
    s = blk.stride
    (w1, b1, _, _), (w2, b2, _, _), (w3, b3, _, _) = (_fold(c, b) for c, b in _pairs(blk)[:3])
    bias = lambda b: b[None, :, None, None]  # noqa: E731
    a1 = F.relu(F.conv2d(x, w1) + bias(b1))
    a2 = F.relu(F.conv2d(a1, w2, None, s, 1) + bias(b2))
    idt = x
    if hasattr(blk, "downsample"):
        wd, bd, _, _ = _fold(*_pairs(blk)[3])
        idt = F.conv2d(x, wd, None, s) + bias(bd)
    return a1, a2, F.relu(F.conv2d(a2, w3) + bias(b3) + idt)


def _pair_grads(g, inp, conv, bn, ksz, stride, bug_gather=False):
    """dW = gamma rstd G, dbeta = s, dgamma = rstd (sum_k w G - mean s) with G = g^T im2col(inp) and s = sum g: nothing divides by gamma."""
    if bug_gather:      # conv1's gather at the output's extent: every second row and column of its input and of its gradient
        g, inp = g[:, :, ::2, ::2], inp[:, :, ::2, ::2]
    cols = F.unfold(inp, ksz, padding=ksz // 2, stride=stride)      # [n, cin k k, L], (ci, ky, kx) order
    G = torch.einsum("nol,nkl->ok", g.flatten(2), cols).reshape(conv.weight.shape)
    ssum = g.sum((0, 2, 3))
    _, _, scale, rstd = _fold(conv, bn)
    return (scale[:, None, None, None] * G, rstd * ((conv.weight * G).sum((1, 2, 3)) - bn.running_mean * ssum), ssum)


def _backward_as_the_kernels_form_it(blk, x, dy, bug=None):
    """(the 9 or 12 gradients in the order conv, gamma, beta per pair, dx)."""
    with torch.no_grad():
        s, ds = blk.stride, hasattr(blk, "downsample")
        pairs = _pairs(blk)
        a1, a2, y = _block_forward(blk, x)
        w1, w2, w3 = (_fold(c, b)[0] for c, b in pairs[:3])
        g3 = dy * (y > 0)      # the gradient at bn3's output, and of the identity path
        da2 = torch.einsum("nohw,oc->nchw", g3, w3[:, :, 0, 0])      # conv3^T: a 1x1 GEMM on the transposed folded weights
        g2 = da2 if bug == "a2_mask_left_out" else da2 * (a2 > 0)
        plane = g2
        if s == 2:      # g2 at the even positions of a zeroed plane of the input's extent
            plane = torch.zeros((g2.shape[0], g2.shape[1], x.shape[2], x.shape[3]), dtype=g2.dtype)
            plane[:, :, 0::2, 0::2] = g2
        wt = w2.transpose(0, 1) if bug == "unrotated_3x3" else w2.transpose(0, 1).flip(-1, -2)
        g1 = F.conv2d(plane, wt, padding=1) * (a1 > 0)      # the stride-1 path on the rotated, transposed weights; at the input's extent
        dx = torch.einsum("nohw,oc->nchw", g1, w1[:, :, 0, 0])
        if bug != "identity_dropped":
            if ds:
                t = torch.einsum("nohw,oc->nchw", g3, _fold(*pairs[3])[0][:, :, 0, 0])
                off = 1 if bug == "ds_on_odd_positions" else 0
                dx[:, :, off::2, off::2] += t
            else:
                dx = dx + g3
        grads = [*_pair_grads(g1, x, *pairs[0], 1, 1, bug_gather=bug == "conv1_gather_at_output_extent"),
                 *_pair_grads(g2, a1, *pairs[1], 3, s), *_pair_grads(g3, a2, *pairs[2], 1, 1)]
        if ds:
            grads += _pair_grads(g3, x, *pairs[3], 1, s)
        return grads, dx


def _autograd_case(stride, seed=5):
    blk = _small_block(stride, 40 + stride)
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((2, blk.conv1.in_channels, 5 * stride, 4 * stride), generator=gen).double().requires_grad_(True)
    dy = torch.randn((2, 4 * WIDTH, 5, 4), generator=gen).double()
    blk.eval()
    y = F.relu(blk.bn3(blk.conv3(F.relu(blk.bn2(blk.conv2(F.relu(blk.bn1(blk.conv1(x)))))))) +
               (blk.downsample(x) if hasattr(blk, "downsample") else x))
    y.backward(dy)
    want = [t.grad for conv, bn in _pairs(blk) for t in (conv.weight, bn.weight, bn.bias)]
    return blk, x.detach(), dy, want, x.grad


@pytest.mark.parametrize("stride", [1, 2])
def test_written_out_backward_matches_autograd(stride):
    blk, x, dy, want, want_dx = _autograd_case(stride)
    got, dx = _backward_as_the_kernels_form_it(blk, x, dy)
    assert len(got) == len(want) == (12 if stride == 2 else 9)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and _rel(a.numpy(), b.numpy()) <= 1e-12, i
    assert _rel(dx.numpy(), want_dx.numpy()) <= 1e-12
    # gamma = 0 channels: their dgamma is formed without dividing by gamma, and is not zero
    assert float(blk.bn3.weight[3].detach()) == 0.0 and float(got[7][3].abs()) > 0


CONTROLS = [("a2_mask_left_out", 1), ("a2_mask_left_out", 2), ("unrotated_3x3", 1), ("unrotated_3x3", 2), ("ds_on_odd_positions", 2),
            ("identity_dropped", 1), ("identity_dropped", 2), ("conv1_gather_at_output_extent", 2)]


@pytest.mark.parametrize("bug,stride", CONTROLS)
def test_negative_controls_miss_autograd_by_ten_times_the_ceiling(bug, stride):
    blk, x, dy, want, want_dx = _autograd_case(stride)
    got, dx = _backward_as_the_kernels_form_it(blk, x, dy, bug)
    errs = [_rel(a.numpy(), b.numpy()) for a, b in zip(got, want)] + [_rel(dx.numpy(), want_dx.numpy())]
    assert max(errs) >= 10 * GRAD_CEILING, f"{bug} at stride {stride}: error {max(errs):.3g} is not 10x the ceiling {GRAD_CEILING}"
