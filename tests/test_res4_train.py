"""ResNet-50's res4 (six 256-wide Bottlenecks) on the HIP training kernels (csrc/bottleneck_train.hip at W = 256), without a device: the
vtd_bottleneck256_train_* entries exist and refuse bad arguments before any launch, the workspace query equals its documented formula, the
Python surface's refusals, the res4 -> res5 -> FPN -> head node's walk over nine blocks in two stages, the "head+fpn+res5+res4" mode's
bookkeeping, and the Bottleneck backward written out in fp64 as the kernels form it at the real width 256 against torch autograd.

The helpers are tests/test_res5_train.py's, taken by import; tests/test_gpu_res4_train.py checks the kernels themselves."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import test_res5_train as r5
from test_res5_train import DS_FIELDS, LEARN_FIELDS, _aligned, _rel, _struct
from vtd_amd import _native, nets

GEOMS = {2: (512, 256, 2), 1: (1024, 256, 1)}
ERR_ARG, ERR_ALIGN = -3903, -3904


# ---- C ABI, no device
def test_new_symbols_are_exported_and_bound():
    lib = _native.load()
    for name in ("vtd_bottleneck256_train_workspace_bytes", "vtd_bottleneck256_train_forward", "vtd_bottleneck256_train_backward"):
        assert name in _native.SIGNATURES and hasattr(lib, name), name
        assert _native.SIGNATURES[name] == _native.SIGNATURES[name.replace("bottleneck256", "bottleneck")]      # same signatures, same struct
    for code in (ERR_ARG, ERR_ALIGN):
        assert b"256-wide Bottleneck training" in lib.vtd_strerror(code)
    assert lib.vtd_strerror(ERR_ARG) != lib.vtd_strerror(-3901) and lib.vtd_strerror(ERR_ALIGN) != lib.vtd_strerror(-3902)


def _workspace_formula(n, hin, win, cin, stride, mode):
    """include/vtd.h, vtd_bottleneck256_train_workspace_bytes."""
    a256 = lambda b: (b + 255) // 256 * 256  # noqa: E731
    S = lambda r: min(8, max(1, -(-r // 4096)))  # noqa: E731
    W, h, w, ds = 256, hin // stride, win // stride, stride == 2
    pin, pout, M, Min = n * (hin + 2) * (win + 2), n * (h + 2) * (w + 2), n * h * w, n * hin * win
    if mode == 0:
        return (a256(2 * pin * W) + a256(2 * pout * W) + (a256(2 * pout * 4 * W) if ds else 0) + a256(2 * W * cin) + a256(2 * W * 9 * W) +
                a256(2 * 4 * W * W) + (a256(2 * 4 * W * cin) if ds else 0) + a256(4 * (2 * W + 2 * 4 * W)))
    return (a256(4 * M * 4 * W) + a256(4 * M * W) + a256(4 * Min * W) + a256(2 * M * 4 * W) + a256(2 * M * W) + a256(2 * Min * W) +
            a256(2 * pout * 4 * W) + 2 * a256(2 * pin * W) + a256(2 * W * 9 * W) + a256(4 * 4 * W) + a256(8 * 256 * 4 * W) + a256(4 * 256) +
            a256(8 * 4 * W) + 2 * a256(8 * W) + a256(48) + a256(4 * max(S(M) * W * 9 * W, S(Min) * W * cin)))


def test_workspace_query_equals_its_formula():
    ws = _native.load().vtd_bottleneck256_train_workspace_bytes
    for n, h, w in ((1, 2, 2), (2, 6, 4), (32, 80, 80)):
        for stride, (cin, width, _) in GEOMS.items():
            for mode in (0, 1):
                got = ws(n, h, w, cin, width, stride, mode)
                assert got == _workspace_formula(n, h, w, cin, stride, mode) and got % 256 == 0, (n, h, w, stride, mode)
    bad = [(2, 6, 4, 1024, 512, 2), (2, 6, 4, 2048, 512, 1),      # width 512: res5's geometries belong to vtd_bottleneck_train_*
           (2, 6, 4, 512, 512, 2), (2, 6, 4, 1024, 128, 1),
           (2, 6, 4, 256, 256, 2), (2, 6, 4, 256, 256, 1), (2, 6, 4, 2048, 256, 1),      # cin mismatches
           (2, 5, 4, 512, 256, 2), (2, 6, 3, 512, 256, 2),      # stride 2 with odd extents
           (2, 6, 4, 512, 256, 1),      # stride 1 with cin 512
           (2, 6, 4, 1024, 256, 2), (2, 6, 4, 1024, 256, 3),
           (0, 6, 4, 512, 256, 2), (2, 0, 4, 1024, 256, 1), (2, 6, -2, 512, 256, 2),      # zero extents
           (1 << 16, 6, 4, 512, 256, 2), (2, 4098, 4, 512, 256, 2), (2, 4, 8192, 1024, 256, 1), (8192, 64, 64, 1024, 256, 1)]      # huge
    for g in bad:
        assert ws(*g, 0) == ERR_ARG and ws(*g, 1) == ERR_ARG, g
    assert ws(2, 6, 4, 512, 256, 2, 2) == ERR_ARG and ws(2, 6, 4, 512, 256, 2, -1) == ERR_ARG
    # and the res5 entries keep refusing width 256, with their own code
    old = _native.load().vtd_bottleneck_train_workspace_bytes
    for stride, (cin, width, _) in GEOMS.items():
        assert old(2, 6, 4, cin, width, stride, 0) == -3901 and old(2, 6, 4, cin, width, stride, 1) == -3901


@pytest.mark.parametrize("stride", [2, 1])
def test_forward_argument_and_alignment_errors(stride):
    """Every refusal comes before any launch, so none of this needs a device."""
    fwd = _native.load().vtd_bottleneck256_train_forward
    keep = [_aligned(4096) for _ in range(4)]
    x, ws, y, w = (k[1] for k in keep)
    cin, width, _ = GEOMS[stride]
    st = _struct(w)
    good = [x, 2, 6, 4, cin, width, stride, C.byref(st), 1e-5, ws, y, None]
    for i in (0, 7, 9, 10):      # x, params, workspace, y
        a = list(good)
        a[i] = None
        assert fwd(*a) == ERR_ARG, i
    for i, v in ((1, 0), (2, 0), (3, -4), (4, 256), (4, 2048), (5, 512), (5, 128), (6, 3 - stride), (8, 0.0), (8, -1.0), (1, 1 << 16), (2, 4098)):
        a = list(good)
        a[i] = v
        assert fwd(*a) == ERR_ARG, (i, v)
    if stride == 2:
        a = list(good)
        a[2] = 5
        assert fwd(*a) == ERR_ARG
    for f in _native.BOTTLENECK_FIELDS:
        if stride == 1 and f in DS_FIELDS:      # the identity block ignores ds_*: such a call would pass the checks and launch
            continue
        for value, want in ((None, ERR_ARG), (C.c_void_p(w.value + 2), ERR_ALIGN)):
            st2 = _struct(w)
            setattr(st2, f, value)
            a = list(good)
            a[7] = C.byref(st2)
            assert fwd(*a) == want, f
    for i, off in ((0, 8), (10, 8), (9, 128)):      # x and y 16 bytes, the workspace 256
        a = list(good)
        a[i] = C.c_void_p(a[i].value + off)
        assert fwd(*a) == ERR_ALIGN, i


@pytest.mark.parametrize("stride", [2, 1])
def test_backward_argument_and_alignment_errors(stride):
    bwd = _native.load().vtd_bottleneck256_train_backward
    keep = [_aligned(4096) for _ in range(9)]
    x, ws, y, dy, dscale, scratch, dx, dxscale, w = (k[1] for k in keep)
    cin, width, _ = GEOMS[stride]
    st, gst = _struct(w), _struct(w, LEARN_FIELDS)
    good = [x, 2, 6, 4, cin, width, stride, C.byref(st), 1e-5, ws, y, dy, dscale, C.byref(gst), scratch, dx, dxscale, None]
    for i in (0, 7, 9, 10, 11, 12, 13, 14, 16):      # every pointer but dx, which is optional; dx without its scale is refused
        a = list(good)
        a[i] = None
        assert bwd(*a) == ERR_ARG, i
    for i, v in ((1, 0), (2, 0), (3, -4), (4, 256), (4, 2048), (5, 512), (6, 3 - stride), (8, 0.0), (1, 1 << 16), (3, 4098)):
        a = list(good)
        a[i] = v
        assert bwd(*a) == ERR_ARG, (i, v)
    for which, fields in ((7, _native.BOTTLENECK_FIELDS), (13, LEARN_FIELDS)):
        for f in fields:
            if stride == 1 and f in DS_FIELDS:
                continue
            for value, want in ((None, ERR_ARG), (C.c_void_p(w.value + 2), ERR_ALIGN)):
                s2 = _struct(w, fields)
                setattr(s2, f, value)
                a = list(good)
                a[which] = C.byref(s2)
                assert bwd(*a) == want, (which, f)
    for i, off in ((0, 8), (10, 8), (11, 8), (15, 8), (9, 128), (14, 128), (12, 4), (16, 4)):
        a = list(good)
        a[i] = C.c_void_p(a[i].value + off)
        assert bwd(*a) == ERR_ALIGN, i


# ---- the Python surface's refusals
def test_bottleneck256_train_refusals():
    b2, b1 = nets.Bottleneck(512, 256, 2), nets.Bottleneck(1024, 256, 1)
    for other in (nets.BasicBlock(256, 256, 1), nets.Bottleneck(256, 64, 1), nets.Bottleneck(1024, 512, 2), nets.Bottleneck(2048, 512, 1),
                  nets.Bottleneck(512, 256, 1), torch.nn.Conv2d(4, 4, 1)):
        with pytest.raises(RuntimeError, match="512 -> 256 -> 1024 stride 2"):
            nets.bottleneck256_train(other, torch.zeros((1, 512, 2, 2)))
    with pytest.raises(ValueError, match="CUDA"):
        nets.bottleneck256_train(b2, torch.zeros((1, 512, 4, 2)))
    with pytest.raises(ValueError, match="CUDA"):
        nets.bottleneck256_train(b1, torch.zeros((1, 1024, 3, 1), dtype=torch.float16))
    with pytest.raises(RuntimeError, match="even extents"):
        nets.bottleneck256_train(b2, torch.zeros((1, 512, 3, 2)))
    for x in (torch.zeros((1, 1024, 4, 2)), torch.zeros((512, 4, 2)), None):      # a wrong channel count, not a 4-d tensor
        with pytest.raises(ValueError, match=r"\[n,512,H,W\]"):
            nets.bottleneck256_train(b2, x)
    odd = nets.Bottleneck(1024, 256, 1)
    odd.bn3.eps = 1e-3
    with pytest.raises(ValueError, match="one eps"):
        nets.bottleneck256_train(odd, torch.zeros((1, 1024, 2, 2)))
    nostats = nets.Bottleneck(1024, 256, 1)
    nostats.bn2 = torch.nn.BatchNorm2d(256, track_running_stats=False)
    with pytest.raises(ValueError, match="running stats"):
        nets.bottleneck256_train(nostats, torch.zeros((1, 1024, 2, 2)))
    # bottleneck_train keeps refusing the 256-wide blocks, with res5's text
    for blk, cin in ((b2, 512), (b1, 1024)):
        with pytest.raises(RuntimeError, match="1024 -> 512 -> 2048 stride 2"):
            nets.bottleneck_train(blk, torch.zeros((1, cin, 2, 2)))


def _meta_taps(n=1, h5=1, w5=1):
    return r5._meta_taps(n, h5, w5)[:2]      # [C2, C3]


def test_forward_padded_res4_refusals():
    net = nets.DBNet("resnet50")
    r18 = nets.DBNet("resnet18")
    fpn, head, res5, res4 = net.fpn, net.head, net.backbone[7], net.backbone[6]
    taps = _meta_taps()
    for kw in ({"layer4": r18.backbone[7]}, {"layer3": r18.backbone[6]}, {"layer2": r18.backbone[5]}, {"layer1": r18.backbone[4]},
               {"stem": (r18.backbone[0], r18.backbone[1])}, {"trunk_batch_stats": True}, {"trunk_batch_stats": ("layer4",)}, {"stem_batch_stats": True}):
        with pytest.raises(ValueError, match="res4 -> res5 -> FPN -> head node"):
            fpn.forward_padded(taps, head=head, res5=res5, res4=res4, **kw)
    with pytest.raises(ValueError, match="needs res5 too"):
        fpn.forward_padded(taps, head=head, res4=res4)
    with pytest.raises(ValueError, match="needs res5 too"):
        fpn.forward_padded(taps, head=head, res4=res4, layer4=r18.backbone[7])
    with pytest.raises(ValueError, match="needs the DBHead"):
        fpn.forward_padded(taps, res5=res5, res4=res4)
    with pytest.raises(ValueError, match="CUDA"):      # CPU taps: there is no CPU path
        fpn.forward_padded(taps, head=head, res5=res5, res4=res4)
    with pytest.raises(ValueError, match=r"\[C2, C3\]"):
        fpn.forward_padded(taps[:1], head=head, res5=res5, res4=res4)
    # the stage itself, judged on shapes alone: ResNet-18's layer3, a shortened stage, res5, a C3 of odd extents or the wrong width
    c3 = torch.empty((1, 6, 6, 512), dtype=torch.float16, device="meta")
    for layer, tap in ((r18.backbone[6], c3), (torch.nn.Sequential(*list(res4)[:5]), c3), (torch.nn.Sequential(*list(res4)[1:], res4[1]), c3),
                       (res5, c3), (net.backbone[5], c3), (None, c3),
                       (res4, torch.empty((1, 7, 6, 512), dtype=torch.float16, device="meta")),
                       (res4, torch.empty((1, 6, 2, 512), dtype=torch.float16, device="meta")),
                       (res4, torch.empty((1, 6, 6, 1024), dtype=torch.float16, device="meta"))):
        with pytest.raises(RuntimeError, match="six Bottlenecks of width 256"):
            nets._res_operands(nets._RES_STAGES[2], layer, tap, torch.device("cpu"))
    odd = nets.DBNet("resnet50").backbone[6]
    odd[4].bn2.eps = 1e-3
    with pytest.raises(ValueError, match="one eps"):
        nets._res_operands(nets._RES_STAGES[2], odd, c3, torch.device("cpu"))
    with pytest.raises(RuntimeError, match="six Bottlenecks of width 256"):
        nets.forward_res4_padded(r18.backbone[6], torch.empty((1, 6, 6, 512), dtype=torch.float16))
    with pytest.raises(ValueError, match="CUDA"):
        nets.forward_res4_padded(res4, torch.empty((1, 6, 6, 512), dtype=torch.float16))
    with pytest.raises(ValueError, match="padded taps"):
        nets.forward_res4_padded(res4, None)
    # the ResNet-18 stage helpers keep refusing Bottleneck stages
    with pytest.raises(RuntimeError, match="Bottleneck training is not built"):
        nets._stage_operands(nets._STAGES[2], res4, c3)
    with pytest.raises(RuntimeError, match="Bottleneck training is not built"):
        nets.forward_layer3_padded(res4, c3)


def test_node_walks_nine_blocks_in_two_stages(monkeypatch):
    """The trunk node on the plan per = (6, 3): C4 is the sixth block's output and C5 the ninth's, dC5 and dC4 are asked of the FPN, blocks
    8 .. 1 form their input gradients and block 0 none, and block 6's dx is combined with the FPN's dC4, once.  The raw wrappers are
    replaced by recorders (no device)."""
    ev, dxs, combined = [], {}, []
    mk = lambda *shape: torch.zeros(shape)  # noqa: E731
    dc4 = mk(1, 2, 2, 1024)

    def block_fwd(tap, geom, eps, learn, stats, entry="x", bn=None):
        ev.append(("fwd", stats, entry, bn, tuple(tap.shape)))
        n, h, w, cin, width, stride = geom
        return mk(n, h // stride + 2, w // stride + 2, 4 * width), mk(8)

    def block_bwd(tap, geom, eps, learn, stats, ws, y, dy, dscale, want_dx, entry="x", bn=None):
        ev.append(("bwd", stats, entry, tuple(dy.shape), bool(want_dx)))
        n, h, w, cin, width, stride = geom
        dxs[stats] = mk(n, h, w, cin) if want_dx else None
        return [p.detach().clone() for p in learn], dxs[stats], (mk(2) if want_dx else None)

    def fpn_bwd(taps, geom, params, ws, dp2, dscale, input_mask=0):
        ev.append(("fpn_bwd", tuple(t.shape[3] for t in taps), input_mask))
        n, h5, w5, c5 = geom
        return [p.detach().clone() for p in params], [None, None, dc4, mk(n, h5, w5, c5)], torch.zeros((4, 2))

    def combine(a, ascale, b, bscale):
        combined.append((a, b))
        return a, ascale

    monkeypatch.setattr(nets, "_block_forward_raw", block_fwd)
    monkeypatch.setattr(nets, "_block_backward_raw", block_bwd)
    monkeypatch.setattr(nets, "_fpn_forward_raw", lambda taps, geom, params: (ev.append(("fpn_fwd", tuple(t.shape[3] for t in taps))), (mk(1, 10, 10, 256), mk(8)))[1])
    monkeypatch.setattr(nets, "_fpn_backward_raw", fpn_bwd)
    monkeypatch.setattr(nets, "_head_forward_raw", lambda feats, hw, *a: (mk(8), mk(1, 1, 32, 32), mk(1, 1, 32, 32), mk(4, 2, 64)))
    monkeypatch.setattr(nets, "_head_backward_raw", lambda feats, hw, tr, ws, prob, thresh, params, gp, gt, want: ([p.detach().clone() for p in params], mk(1, 8, 8, 256), mk(2)))
    monkeypatch.setattr(nets, "_combine_scaled", combine)
    B4, B5 = nets._BOTTLENECK256, nets._BOTTLENECK
    assert B4 == "vtd_bottleneck256_train" and B5 == "vtd_bottleneck_train"
    geoms = [(1, 4, 4, 512, 256, 2)] + [(1, 2, 2, 1024, 256, 1)] * 5 + [(1, 2, 2, 1024, 512, 2), (1, 1, 1, 2048, 512, 1), (1, 1, 1, 2048, 512, 1)]
    blocks = tuple(nets._BlockPlan(g, i, B4 if i < 6 else B5, 12 if i in (0, 6) else 9) for i, g in enumerate(geoms))
    plan = nets._TrunkPlan(tuple(_meta_taps()), (1, 1, 1, 2048), (True, 0.1, 1e-5, ()), None, blocks, 1e-5, None, (6, 3))
    params = [torch.full((1,), float(i), requires_grad=True) for i in range(57 + 30 + 30)]
    prob, thresh, _ = nets._TrunkFPNHeadTrainFn.apply(plan, *params)
    torch.autograd.backward([prob, thresh], [torch.ones_like(prob), torch.ones_like(thresh)])
    c4, c5 = (1, 4, 4, 1024), (1, 3, 3, 2048)
    assert ev == ([("fwd", 0, B4, None, (1, 6, 6, 512))] + [("fwd", i, B4, None, c4) for i in range(1, 6)] +
                  [("fwd", 6, B5, None, c4), ("fwd", 7, B5, None, c5), ("fwd", 8, B5, None, c5),
                   ("fpn_fwd", (256, 512, 1024, 2048)), ("fpn_bwd", (256, 512, 1024, 2048), 12),
                   ("bwd", 8, B5, (1, 1, 1, 2048), True), ("bwd", 7, B5, (1, 1, 1, 2048), True), ("bwd", 6, B5, (1, 1, 1, 2048), True)] +
                  [("bwd", i, B4, (1, 2, 2, 1024), i > 0) for i in (5, 4, 3, 2, 1, 0)])
    assert len(combined) == 1 and combined[0][0] is dxs[6] and combined[0][1] is dc4      # res5.0's strided dx + the FPN's dC4, once
    assert dxs[0] is None      # no dC3
    assert all(p.grad is not None and float(p.grad) == float(i) for i, p in enumerate(params))
    # an int keeps meaning "every stage"; the default stays 2
    assert nets._TrunkPlan((), None, None, None, (), None, None).per == 2
    assert nets._TrunkFPNHeadTrainFn._stages(nets._TrunkPlan((), None, None, None, blocks[:6], None, None, 3)) == ([0, 3], [2, 5])
    assert nets._TrunkFPNHeadTrainFn._stages(nets._TrunkPlan((), None, None, None, blocks[:8], None, None)) == ([0, 2, 4, 6], [1, 3, 5, 7])
    assert nets._TrunkFPNHeadTrainFn._stages(plan) == ([0, 6], [5, 8])


# ---- the "head+fpn+res5+res4" mode
MODE = "head+fpn+res5+res4"


def _grad_pattern(net):
    return {k: p.requires_grad for k, p in net.named_parameters()}


def test_res4_mode_bookkeeping():
    keys = list(nets.DBNet("resnet50").state_dict())
    net = nets.DBNet("resnet50", trainable=MODE)
    assert net.trainable == MODE and net.trunk_bn == "frozen" and net._first_trained() == 6
    assert list(net.state_dict()) == keys
    pat = _grad_pattern(net)
    trained = [k for k, v in pat.items() if v]
    assert all(k.startswith(("backbone.6.", "backbone.7.", "fpn.", "head.")) for k in trained)
    assert not any(v for k, v in pat.items() if k.startswith("backbone.") and not k.startswith(("backbone.6.", "backbone.7.")))
    assert sum(k.startswith("backbone.6.") for k in trained) == 57 and len(list(net.backbone[6].buffers())) == 57      # 12 + 5 x 9
    assert sum(k.startswith("backbone.7.") for k in trained) == 30 and len(list(net.backbone[7].buffers())) == 30
    assert all(v for k, v in pat.items() if k.startswith(("fpn.", "head.")))
    assert len(nets.FeaturePyramidNetwork.live_parameters(net.fpn)) == 10 and len(list(net.head.parameters())) == 20      # 117 train in the node
    # the fused inference engine is rebuilt after res4's or res5's tensors change: the key covers 30 + 30 and 57 + 57 tensors
    n_head = len(list(net.head.parameters())) + len(list(net.head.buffers()))
    assert len(net._head_tensor_versions()) == n_head + len(list(net.fpn.parameters())) + 60 + 114
    v0 = net._head_tensor_versions()
    with torch.no_grad():
        net.backbone[6][5].bn3.running_var.add_(1.0)
    v1 = net._head_tensor_versions()
    assert v1 != v0
    with torch.no_grad():
        net.backbone[6][0].downsample[0].weight.mul_(1.0)
    assert net._head_tensor_versions() != v1
    # switching between the modes, both ways
    net.set_trainable("head+fpn+res5")
    p5 = _grad_pattern(net)
    assert not any(v for k, v in p5.items() if k.startswith("backbone.") and not k.startswith("backbone.7."))
    assert len(net._head_tensor_versions()) == n_head + len(list(net.fpn.parameters())) + 60
    assert net.set_trainable(MODE) is net and _grad_pattern(net) == pat
    net.set_trainable("head+fpn")
    assert not any(v for k, v in _grad_pattern(net).items() if k.startswith("backbone."))
    assert _grad_pattern(net.set_trainable(MODE)) == pat
    assert _grad_pattern(nets.DBNet("resnet50", trainable="head+fpn+res5").set_trainable(MODE)) == pat
    assert _grad_pattern(nets.DBNet("resnet50", trainable=MODE).set_trainable("head+fpn+res5")) == p5


def test_res4_mode_refusals():
    with pytest.raises(ValueError, match=r"head\+fpn\+layer4\+layer3"):
        nets.DBNet("resnet18", trainable=MODE)
    r18 = nets.DBNet("resnet18", trainable="head+fpn")
    with pytest.raises(ValueError, match=r"head\+fpn\+layer4\+layer3"):
        r18.set_trainable(MODE)
    assert r18.trainable == "head+fpn"
    for bn in ("batch", "trained", "backbone", ("layer4",), ("layer3", "layer4"), ("res5", "res4"), "bogus", 3):
        with pytest.raises(ValueError):
            nets.DBNet("resnet50", trainable=MODE, trunk_bn=bn)
    net = nets.DBNet("resnet50", trainable=MODE)
    for bn in ("batch", "trained"):
        with pytest.raises(ValueError, match="frozen-statistics"):
            net.set_trainable(MODE, trunk_bn=bn)
    assert net.trainable == MODE and net.trunk_bn == "frozen"
    # a frozen trunk tensor that requires grad is refused in a train-mode forward before anything touches a device; backbone.6 may
    net.train()
    net.backbone[5][0].conv1.weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match=r"backbone\.5\.0\.conv1\.weight requires grad"):
        net(torch.zeros((1, 3, 640, 640)))


# ---- the 256-wide Bottleneck backward as the kernels form it, in fp64, against autograd: tests/test_res5_train.py's restatement at the
# real widths (512 -> 256 -> 1024 at stride 2, 1024 -> 256 -> 1024 at stride 1)
def _block256(stride, seed):
    cin = GEOMS[stride][0]
    blk = nets.Bottleneck(cin, 256, stride)
    blk.load_state_dict(nets.seeded_state_dict(lambda: nets.Bottleneck(cin, 256, stride), seed))
    with torch.no_grad():
        blk.bn3.weight[3] = 0.0
        blk.bn3.weight[7] = -0.75
        blk.bn1.weight[2] = 0.0
        blk.bn2.weight[5] = -1.25
    return blk.double().eval()


def _autograd_case256(stride):
    blk = _block256(stride, 70 + stride)
    gen = torch.Generator().manual_seed(9)
    x = torch.randn((2, blk.conv1.in_channels, 3 * stride, 2 * stride), generator=gen).double().requires_grad_(True)
    dy = torch.randn((2, 1024, 3, 2), generator=gen).double()
    y = F.relu(blk.bn3(blk.conv3(F.relu(blk.bn2(blk.conv2(F.relu(blk.bn1(blk.conv1(x)))))))) + (blk.downsample(x) if hasattr(blk, "downsample") else x))
    y.backward(dy)
    return blk, x.detach(), dy, [t.grad for conv, bn in r5._pairs(blk) for t in (conv.weight, bn.weight, bn.bias)], x.grad


@pytest.mark.parametrize("stride", [1, 2])
def test_written_out_backward_matches_autograd_at_width_256(stride):
    blk, x, dy, want, want_dx = _autograd_case256(stride)
    assert nets._bottleneck_check(blk, nets._BOTTLENECK256_GEOMETRIES, nets._BOTTLENECK256_BUILT)[0] == GEOMS[stride]
    got, dx = r5._backward_as_the_kernels_form_it(blk, x, dy)
    assert len(got) == len(want) == (12 if stride == 2 else 9)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and _rel(a.numpy(), b.numpy()) <= 1e-12, i
    assert dx.shape == x.shape and _rel(dx.numpy(), want_dx.numpy()) <= 1e-12
    assert float(blk.bn3.weight[3].detach()) == 0.0 and float(got[7][3].abs()) > 0      # dgamma of a gamma = 0 channel: nothing divides by gamma
    # a negative control: the downsample's transpose on the odd positions (stride 2) or the identity dropped (stride 1) misses by 10x the ceiling
    bad, bdx = r5._backward_as_the_kernels_form_it(blk, x, dy, "ds_on_odd_positions" if stride == 2 else "identity_dropped")
    assert _rel(bdx.numpy(), want_dx.numpy()) >= 10 * r5.GRAD_CEILING
