"""ResNet-50's res3 (four 128-wide Bottlenecks) on the HIP training kernels (csrc/bottleneck_train.hip at W = 128), without a device: the
vtd_bottleneck128_train_* entries and vtd_detector_forward_c2 exist and refuse bad arguments before any launch, the workspace query equals
its documented formula (the res3 family's weight-gradient slab rule included), the Python surface's refusals, the res3 -> res4 -> res5 ->
FPN -> head node's walk over thirteen blocks in three stages, and the "head+fpn+res5+res4+res3" mode's bookkeeping.

The helpers are tests/test_res5_train.py's, taken by import; tests/test_gpu_res3_train.py checks the kernels themselves."""
import ctypes as C

import pytest
import torch

import test_res5_train as r5
from test_res5_train import DS_FIELDS, LEARN_FIELDS, _aligned, _struct
from vtd_amd import _native, nets
from vtd_amd.engine import DetectorEngine

GEOMS = {2: (256, 128, 2), 1: (512, 128, 1)}
ERR_ARG, ERR_ALIGN = -3905, -3906
MODE = "head+fpn+res5+res4+res3"


# ---- C ABI, no device
def test_new_symbols_are_exported_and_bound():
    lib = _native.load()
    for name in ("vtd_bottleneck128_train_workspace_bytes", "vtd_bottleneck128_train_forward", "vtd_bottleneck128_train_backward"):
        assert name in _native.SIGNATURES and hasattr(lib, name), name
        assert _native.SIGNATURES[name] == _native.SIGNATURES[name.replace("bottleneck128", "bottleneck")]      # same signatures, same struct
    for code in (ERR_ARG, ERR_ALIGN):
        assert b"128-wide Bottleneck training" in lib.vtd_strerror(code)
    assert lib.vtd_strerror(ERR_ARG) not in (lib.vtd_strerror(-3901), lib.vtd_strerror(-3903))
    assert lib.vtd_strerror(ERR_ALIGN) not in (lib.vtd_strerror(-3902), lib.vtd_strerror(-3904))
    # the engine's stop at C2: forward_pool's signature, and the detector entries' argument error without a handle
    assert "vtd_detector_forward_c2" in _native.SIGNATURES and hasattr(lib, "vtd_detector_forward_c2")
    assert _native.SIGNATURES["vtd_detector_forward_c2"] == _native.SIGNATURES["vtd_detector_forward_pool"]
    keep, a = _aligned(64)
    assert lib.vtd_detector_forward_c2(None, 1, a, None) == -1100
    assert callable(DetectorEngine.forward_c2)


def _workspace_formula(n, hin, win, cin, stride, mode):
    """include/vtd.h, vtd_bottleneck128_train_workspace_bytes."""
    a256 = lambda b: (b + 255) // 256 * 256  # noqa: E731
    T = lambda r, wgs: min(-(-512 // wgs), max(1, -(-r // 1024)))  # noqa: E731
    W, h, w, ds = 128, hin // stride, win // stride, stride == 2
    pin, pout, M, Min = n * (hin + 2) * (win + 2), n * (h + 2) * (w + 2), n * h * w, n * hin * win
    if mode == 0:
        return (a256(2 * pin * W) + a256(2 * pout * W) + (a256(2 * pout * 4 * W) if ds else 0) + a256(2 * W * cin) + a256(2 * W * 9 * W) +
                a256(2 * 4 * W * W) + (a256(2 * 4 * W * cin) if ds else 0) + a256(4 * (2 * W + 2 * 4 * W)))
    slab = max(T(M, 9) * W * 9 * W, T(Min, cin // 128) * W * cin, T(M, 4) * 4 * W * W, T(M, 4 * cin // 128) * 4 * W * cin if ds else 0)
    return (a256(4 * M * 4 * W) + a256(4 * M * W) + a256(4 * Min * W) + a256(2 * M * 4 * W) + a256(2 * M * W) + a256(2 * Min * W) +
            a256(2 * pout * 4 * W) + 2 * a256(2 * pin * W) + a256(2 * W * 9 * W) + a256(4 * 4 * W) + a256(8 * 256 * 4 * W) + a256(4 * 256) +
            a256(8 * 4 * W) + 2 * a256(8 * W) + a256(48) + a256(4 * slab))


def test_workspace_query_equals_its_formula():
    ws = _native.load().vtd_bottleneck128_train_workspace_bytes
    for n, h, w in ((1, 2, 2), (2, 6, 4), (2, 48, 44), (32, 160, 160), (32, 80, 80)):
        for stride, (cin, width, _) in GEOMS.items():
            for mode in (0, 1):
                got = ws(n, h, w, cin, width, stride, mode)
                assert got > 0 and got == _workspace_formula(n, h, w, cin, stride, mode) and got % 256 == 0, (n, h, w, stride, mode)
    # the slab buffer at the product's rows: 512 workgroups in every launch, 33.6 MB whichever launch is the largest
    T = lambda r, wgs: min(-(-512 // wgs), max(1, -(-r // 1024)))  # noqa: E731
    assert [T(204800, 9), T(819200, 2), T(204800, 4), T(204800, 8), T(204800, 16)] == [57, 256, 128, 64, 32]
    assert max(57 * 128 * 1152, 256 * 128 * 256, 128 * 512 * 128, 64 * 512 * 256) * 4 == 33619968
    bad = [(2, 6, 4, 512, 256, 2), (2, 6, 4, 1024, 256, 1),      # width 256: res4's geometries belong to vtd_bottleneck256_train_*
           (2, 6, 4, 1024, 512, 2), (2, 6, 4, 2048, 512, 1),      # width 512: res5's
           (2, 6, 4, 256, 256, 2), (2, 6, 4, 512, 64, 1),
           (2, 6, 4, 128, 128, 2), (2, 6, 4, 128, 128, 1), (2, 6, 4, 1024, 128, 1),      # cin mismatches
           (2, 5, 4, 256, 128, 2), (2, 6, 3, 256, 128, 2),      # stride 2 with odd extents
           (2, 6, 4, 256, 128, 1),      # stride 1 with cin 256: res2's geometry, not built
           (2, 6, 4, 512, 128, 2), (2, 6, 4, 512, 128, 3),
           (0, 6, 4, 256, 128, 2), (2, 0, 4, 512, 128, 1), (2, 6, -2, 256, 128, 2),      # zero extents
           (1 << 16, 6, 4, 256, 128, 2), (2, 4098, 4, 256, 128, 2), (2, 4, 8192, 512, 128, 1), (16384, 64, 64, 512, 128, 1)]      # huge
    for g in bad:
        assert ws(*g, 0) == ERR_ARG and ws(*g, 1) == ERR_ARG, g
    assert ws(2, 6, 4, 256, 128, 2, 2) == ERR_ARG and ws(2, 6, 4, 256, 128, 2, -1) == ERR_ARG
    # and the res5 and res4 entries keep refusing width 128, with their own codes
    lib = _native.load()
    for stride, (cin, width, _) in GEOMS.items():
        for mode in (0, 1):
            assert lib.vtd_bottleneck_train_workspace_bytes(2, 6, 4, cin, width, stride, mode) == -3901
            assert lib.vtd_bottleneck256_train_workspace_bytes(2, 6, 4, cin, width, stride, mode) == -3903


@pytest.mark.parametrize("stride", [2, 1])
def test_forward_argument_and_alignment_errors(stride):
    """Every refusal comes before any launch, so none of this needs a device."""
    fwd = _native.load().vtd_bottleneck128_train_forward
    keep = [_aligned(4096) for _ in range(4)]
    x, ws, y, w = (k[1] for k in keep)
    cin, width, _ = GEOMS[stride]
    st = _struct(w)
    good = [x, 2, 6, 4, cin, width, stride, C.byref(st), 1e-5, ws, y, None]
    for i in (0, 7, 9, 10):      # x, params, workspace, y
        a = list(good)
        a[i] = None
        assert fwd(*a) == ERR_ARG, i
    for i, v in ((1, 0), (2, 0), (3, -4), (4, 128), (4, 1024), (5, 256), (5, 512), (5, 64), (6, 3 - stride), (8, 0.0), (8, -1.0), (1, 1 << 16),
                 (2, 4098)):
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
    bwd = _native.load().vtd_bottleneck128_train_backward
    keep = [_aligned(4096) for _ in range(9)]
    x, ws, y, dy, dscale, scratch, dx, dxscale, w = (k[1] for k in keep)
    cin, width, _ = GEOMS[stride]
    st, gst = _struct(w), _struct(w, LEARN_FIELDS)
    good = [x, 2, 6, 4, cin, width, stride, C.byref(st), 1e-5, ws, y, dy, dscale, C.byref(gst), scratch, dx, dxscale, None]
    for i in (0, 7, 9, 10, 11, 12, 13, 14, 16):      # every pointer but dx, which is optional; dx without its scale is refused
        a = list(good)
        a[i] = None
        assert bwd(*a) == ERR_ARG, i
    for i, v in ((1, 0), (2, 0), (3, -4), (4, 128), (4, 1024), (5, 256), (6, 3 - stride), (8, 0.0), (1, 1 << 16), (3, 4098)):
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
def test_bottleneck128_train_refusals():
    b2, b1 = nets.Bottleneck(256, 128, 2), nets.Bottleneck(512, 128, 1)
    assert nets._BOTTLENECK128 == "vtd_bottleneck128_train" and nets._BOTTLENECK128 in nets._BOTTLENECK_FAMILIES
    assert nets._BOTTLENECK128_GEOMETRIES == ((256, 128, 2, True), (512, 128, 1, False))
    for blk, stride in ((b2, 2), (b1, 1)):
        assert nets._bottleneck_check(blk, nets._BOTTLENECK128_GEOMETRIES, nets._BOTTLENECK128_BUILT)[0] == GEOMS[stride]
    for other in (nets.BasicBlock(128, 128, 1), nets.Bottleneck(256, 64, 1), nets.Bottleneck(512, 256, 2), nets.Bottleneck(1024, 256, 1),
                  nets.Bottleneck(2048, 512, 1), nets.Bottleneck(256, 128, 1), torch.nn.Conv2d(4, 4, 1)):
        with pytest.raises(RuntimeError, match="256 -> 128 -> 512 stride 2"):
            nets.bottleneck128_train(other, torch.zeros((1, 256, 2, 2)))
    with pytest.raises(ValueError, match="CUDA"):
        nets.bottleneck128_train(b2, torch.zeros((1, 256, 4, 2)))
    with pytest.raises(ValueError, match="CUDA"):
        nets.bottleneck128_train(b1, torch.zeros((1, 512, 3, 1), dtype=torch.float16))
    with pytest.raises(RuntimeError, match="even extents"):
        nets.bottleneck128_train(b2, torch.zeros((1, 256, 3, 2)))
    for x in (torch.zeros((1, 512, 4, 2)), torch.zeros((256, 4, 2)), None):      # a wrong channel count, not a 4-d tensor
        with pytest.raises(ValueError, match=r"\[n,256,H,W\]"):
            nets.bottleneck128_train(b2, x)
    odd = nets.Bottleneck(512, 128, 1)
    odd.bn3.eps = 1e-3
    with pytest.raises(ValueError, match="one eps"):
        nets.bottleneck128_train(odd, torch.zeros((1, 512, 2, 2)))
    nostats = nets.Bottleneck(512, 128, 1)
    nostats.bn2 = torch.nn.BatchNorm2d(128, track_running_stats=False)
    with pytest.raises(ValueError, match="running stats"):
        nets.bottleneck128_train(nostats, torch.zeros((1, 512, 2, 2)))
    # the other two families keep refusing the 128-wide blocks, with their own texts
    for blk, cin in ((b2, 256), (b1, 512)):
        with pytest.raises(RuntimeError, match="1024 -> 512 -> 2048 stride 2"):
            nets.bottleneck_train(blk, torch.zeros((1, cin, 2, 2)))
        with pytest.raises(RuntimeError, match="512 -> 256 -> 1024 stride 2"):
            nets.bottleneck256_train(blk, torch.zeros((1, cin, 2, 2)))


def _meta_taps(n=1, h5=1, w5=1):
    return r5._meta_taps(n, h5, w5)[:1]      # [C2]


def test_forward_padded_res3_refusals():
    net = nets.DBNet("resnet50")
    r18 = nets.DBNet("resnet18")
    fpn, head, res5, res4, res3 = net.fpn, net.head, net.backbone[7], net.backbone[6], net.backbone[5]
    taps = _meta_taps()
    for kw in ({"layer4": r18.backbone[7]}, {"layer3": r18.backbone[6]}, {"layer2": r18.backbone[5]}, {"layer1": r18.backbone[4]},
               {"stem": (r18.backbone[0], r18.backbone[1])}, {"trunk_batch_stats": True}, {"trunk_batch_stats": ("layer4",)}, {"stem_batch_stats": True}):
        with pytest.raises(ValueError, match="res3 -> res4 -> res5 -> FPN -> head node"):
            fpn.forward_padded(taps, head=head, res5=res5, res4=res4, res3=res3, **kw)
    for kw in ({}, {"res5": res5}, {"res4": res4}, {"layer4": r18.backbone[7]}):
        with pytest.raises(ValueError, match="needs res4 and res5 too"):
            fpn.forward_padded(taps, head=head, res3=res3, **kw)
    with pytest.raises(ValueError, match="needs the DBHead"):
        fpn.forward_padded(taps, res5=res5, res4=res4, res3=res3)
    with pytest.raises(ValueError, match="CUDA"):      # CPU taps: there is no CPU path
        fpn.forward_padded(taps, head=head, res5=res5, res4=res4, res3=res3)
    with pytest.raises(ValueError, match=r"\[C2\]"):
        fpn.forward_padded([], head=head, res5=res5, res4=res4, res3=res3)
    # the stage itself, judged on shapes alone: ResNet-18's layer2, a shortened stage, res4, res2, a C2 of odd extents or the wrong width
    c2 = torch.empty((1, 10, 10, 256), dtype=torch.float16, device="meta")
    for layer, tap in ((r18.backbone[5], c2), (torch.nn.Sequential(*list(res3)[:3]), c2), (torch.nn.Sequential(*list(res3)[1:], res3[1]), c2),
                       (res4, c2), (net.backbone[4], c2), (None, c2),
                       (res3, torch.empty((1, 11, 10, 256), dtype=torch.float16, device="meta")),
                       (res3, torch.empty((1, 10, 2, 256), dtype=torch.float16, device="meta")),
                       (res3, torch.empty((1, 10, 10, 512), dtype=torch.float16, device="meta"))):
        with pytest.raises(RuntimeError, match="four Bottlenecks of width 128"):
            nets._res_operands(nets._RES_STAGES[1], layer, tap, torch.device("cpu"))
    odd =nets.DBNet("resnet50").backbone[5]
    odd[2].bn2.eps = 1e-3
    with pytest.raises(ValueError, match="one eps"):
        nets._res_operands(nets._RES_STAGES[1], odd, c2, torch.device("cpu"))
    with pytest.raises(RuntimeError, match="four Bottlenecks of width 128"):
        nets.forward_res3_padded(r18.backbone[5], torch.empty((1, 10, 10, 256), dtype=torch.float16))
    with pytest.raises(ValueError, match="CUDA"):
        nets.forward_res3_padded(res3, torch.empty((1, 10, 10, 256), dtype=torch.float16))
    with pytest.raises(ValueError, match="padded taps"):
        nets.forward_res3_padded(res3, None)
    # the ResNet-18 stage helpers keep refusing Bottleneck stages
    with pytest.raises(RuntimeError, match="Bottleneck training is not built"):
        nets._stage_operands(nets._STAGES[1], res3, c2)
    with pytest.raises(RuntimeError, match="Bottleneck training is not built"):
        nets.forward_layer2_padded(res3, c2)


def test_node_walks_thirteen_blocks_in_three_stages(monkeypatch):
    """The trunk node on the plan per = (4, 6, 3): C3 is the fourth block's output, C4 the tenth's and C5 the thirteenth's; dC5, dC4 and dC3 are
    asked of the FPN; blocks 12 .. 1 form their input gradients and block 0 none (no dC2); block 10's dx is combined with the FPN's dC4 and
    block 4's with its dC3, once each.  The raw wrappers are replaced by recorders (no device)."""
    ev, dxs, combined = [], {}, []
    mk = lambda *shape: torch.zeros(shape)  # noqa: E731
    dc3, dc4 = mk(1, 4, 4, 512), mk(1, 2, 2, 1024)

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
        return [p.detach().clone() for p in params], [None, dc3, dc4, mk(n, h5, w5, c5)], torch.zeros((4, 2))

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
    B3, B4, B5 = nets._BOTTLENECK128, nets._BOTTLENECK256, nets._BOTTLENECK
    geoms = ([(1, 8, 8, 256, 128, 2)] + [(1, 4, 4, 512, 128, 1)] * 3 + [(1, 4, 4, 512, 256, 2)] + [(1, 2, 2, 1024, 256, 1)] * 5 +
             [(1, 2, 2, 1024, 512, 2), (1, 1, 1, 2048, 512, 1), (1, 1, 1, 2048, 512, 1)])
    fam = lambda i: B3 if i < 4 else B4 if i < 10 else B5  # noqa: E731
    blocks = tuple(nets._BlockPlan(g, i, fam(i), 12 if i in (0, 4, 10) else 9) for i, g in enumerate(geoms))
    plan = nets._TrunkPlan(tuple(_meta_taps()), (1, 1, 1, 2048), (True, 0.1, 1e-5, ()), None, blocks, 1e-5, None, (4, 6, 3))
    params = [torch.full((1,), float(i), requires_grad=True) for i in range(39 + 57 + 30 + 30)]
    assert len(params) == 156
    prob, thresh, _ = nets._TrunkFPNHeadTrainFn.apply(plan, *params)
    torch.autograd.backward([prob, thresh], [torch.ones_like(prob), torch.ones_like(thresh)])
    c3, c4, c5 = (1, 6, 6, 512), (1, 4, 4, 1024), (1, 3, 3, 2048)
    assert ev == ([("fwd", 0, B3, None, (1, 10, 10, 256))] + [("fwd", i, B3, None, c3) for i in range(1, 4)] +
                  [("fwd", 4, B4, None, c3)] + [("fwd", i, B4, None, c4) for i in range(5, 10)] +
                  [("fwd", 10, B5, None, c4), ("fwd", 11, B5, None, c5), ("fwd", 12, B5, None, c5),
                   ("fpn_fwd", (256, 512, 1024, 2048)), ("fpn_bwd", (256, 512, 1024, 2048), 14),
                   ("bwd", 12, B5, (1, 1, 1, 2048), True), ("bwd", 11, B5, (1, 1, 1, 2048), True), ("bwd", 10, B5, (1, 1, 1, 2048), True)] +
                  [("bwd", i, B4, (1, 2, 2, 1024), True) for i in (9, 8, 7, 6, 5, 4)] +
                  [("bwd", i, B3, (1, 4, 4, 512), i > 0) for i in (3, 2, 1, 0)])
    assert len(combined) == 2
    assert combined[0][0] is dxs[10] and combined[0][1] is dc4      # res5.0's strided dx + the FPN's dC4, once
    assert combined[1][0] is dxs[4] and combined[1][1] is dc3      # res4.0's strided dx + the FPN's dC3, once
    assert dxs[0] is None      # no dC2
    assert all(p.grad is not None and float(p.grad) == float(i) for i, p in enumerate(params))
    assert nets._TrunkFPNHeadTrainFn._stages(plan) == ([0, 4, 10], [3, 9, 12])


# ---- the "head+fpn+res5+res4+res3" mode
def _grad_pattern(net):
    return {k: p.requires_grad for k, p in net.named_parameters()}


def test_res3_mode_bookkeeping():
    keys = list(nets.DBNet("resnet50").state_dict())
    net = nets.DBNet("resnet50", compute_threshold=True, trainable=MODE)
    assert net.trainable == MODE and net.trunk_bn == "frozen" and net._first_trained() == 5
    assert list(net.state_dict()) == keys
    pat = _grad_pattern(net)
    trained = [k for k, v in pat.items() if v]
    stages = ("backbone.5.", "backbone.6.", "backbone.7.")
    assert all(k.startswith(stages + ("fpn.", "head.")) for k in trained)
    assert not any(v for k, v in pat.items() if k.startswith("backbone.") and not k.startswith(stages))      # backbone.0 .. backbone.4
    assert sum(k.startswith("backbone.5.") for k in trained) == 39 and len(list(net.backbone[5].buffers())) == 39      # 12 + 3 x 9
    assert sum(k.startswith("backbone.6.") for k in trained) == 57 and sum(k.startswith("backbone.7.") for k in trained) == 30
    assert all(v for k, v in pat.items() if k.startswith(("fpn.", "head.")))
    assert len(nets.FeaturePyramidNetwork.live_parameters(net.fpn)) == 10 and len(list(net.head.parameters())) == 20
    assert 39 + 57 + 30 + 10 + 20 == 156      # what trains in the node
    # the fused inference engine is rebuilt after any trained stage's tensors change: the key covers 2 x (30 + 57 + 39) trunk tensors
    n_head = len(list(net.head.parameters())) + len(list(net.head.buffers()))
    assert len(net._head_tensor_versions()) == n_head + len(list(net.fpn.parameters())) + 60 + 114 + 78
    v0 = net._head_tensor_versions()
    with torch.no_grad():
        net.backbone[5][3].bn3.running_var.add_(1.0)
    v1 = net._head_tensor_versions()
    assert v1 != v0
    with torch.no_grad():
        net.backbone[5][0].downsample[0].weight.mul_(1.0)
    assert net._head_tensor_versions() != v1
    # switching between the modes, both ways
    net.set_trainable("head+fpn+res5+res4")
    p4 = _grad_pattern(net)
    assert not any(v for k, v in p4.items() if k.startswith("backbone.") and not k.startswith(stages[1:]))
    assert len(net._head_tensor_versions()) == n_head + len(list(net.fpn.parameters())) + 60 + 114
    assert net.set_trainable(MODE) is net and _grad_pattern(net) == pat
    net.set_trainable("head+fpn+res5")
    assert not any(v for k, v in _grad_pattern(net).items() if k.startswith("backbone.") and not k.startswith("backbone.7."))
    assert _grad_pattern(net.set_trainable(MODE)) == pat
    net.set_trainable("head+fpn")
    assert not any(v for k, v in _grad_pattern(net).items() if k.startswith("backbone."))
    assert _grad_pattern(net.set_trainable(MODE)) == pat
    assert _grad_pattern(nets.DBNet("resnet50", trainable="head+fpn+res5+res4").set_trainable(MODE)) == pat
    assert _grad_pattern(nets.DBNet("resnet50", trainable=MODE).set_trainable("head+fpn+res5+res4")) == p4


def test_res3_mode_refusals():
    with pytest.raises(ValueError, match=r"head\+fpn\+layer4\+layer3\+layer2"):
        nets.DBNet("resnet18", trainable=MODE)
    r18 = nets.DBNet("resnet18", trainable="head+fpn")
    before = _grad_pattern(r18)
    with pytest.raises(ValueError, match=r"head\+fpn\+layer4\+layer3\+layer2"):
        r18.set_trainable(MODE)
    assert r18.trainable == "head+fpn" and _grad_pattern(r18) == before
    for bn in ("batch", "trained", "backbone", ("layer4",), ("layer2", "layer3", "layer4"), ("res5", "res4", "res3"), "bogus", 3):
        with pytest.raises(ValueError):
            nets.DBNet("resnet50", trainable=MODE, trunk_bn=bn)
    # a refused set_trainable leaves the network as it was, from either side
    net = nets.DBNet("resnet50", trainable=MODE)
    pat = _grad_pattern(net)
    for bn in ("batch", "trained"):
        with pytest.raises(ValueError, match="frozen-statistics"):
            net.set_trainable(MODE, trunk_bn=bn)
    assert net.trainable == MODE and net.trunk_bn == "frozen" and _grad_pattern(net) == pat
    other = nets.DBNet("resnet50", trainable="head+fpn+res5+res4")
    p4 = _grad_pattern(other)
    with pytest.raises(ValueError, match="res3, res4 and res5 train with frozen-statistics"):
        other.set_trainable(MODE, trunk_bn="batch")
    assert other.trainable == "head+fpn+res5+res4" and other.trunk_bn == "frozen" and _grad_pattern(other) == p4
    # a frozen trunk tensor that requires grad is refused in a train-mode forward before anything touches a device; backbone.5 may
    net.train()
    net.backbone[4][2].conv3.weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match=r"backbone\.4\.2\.conv3\.weight requires grad, but backward below res3 is not implemented"):
        net(torch.zeros((1, 3, 640, 640)))
