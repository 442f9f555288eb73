"""ResNet-50's res2 (three 64-wide Bottlenecks) and whole backbone on the HIP training kernels (csrc/bottleneck_train.hip at W = 64), without
a device: the vtd_bottleneck64_train_* entries exist and refuse bad arguments before any launch, the workspace query equals its documented
formula (the slab rule at the product's rows included), the Python surface's refusals, the res2 -> res3 -> res4 -> res5 -> FPN -> head
node's walk over sixteen blocks in four stages (with and without the stem), and the bookkeeping of the "head+fpn+res5+res4+res3+res2" and
"head+fpn+res5+res4+res3+res2+stem" modes.

The helpers are tests/test_res5_train.py's, taken by import; tests/test_gpu_res2_train.py checks the kernels themselves."""
import ctypes as C

import pytest
import torch

from test_res5_train import DS_FIELDS, LEARN_FIELDS, _aligned, _meta_taps, _struct
from vtd_amd import _native, nets

GEOMS = {"ds": (64, 64, 1), "id": (256, 64, 1)}      # both at stride 1; "ds" has the 1x1 downsample at stride 1
ERR_ARG, ERR_ALIGN = -3907, -3908
MODE, WHOLE = "head+fpn+res5+res4+res3+res2", "head+fpn+res5+res4+res3+res2+stem"
RES3_MODE = "head+fpn+res5+res4+res3"


# ---- C ABI, no device
def test_new_symbols_are_exported_and_bound():
    lib = _native.load()
    for name in ("vtd_bottleneck64_train_workspace_bytes", "vtd_bottleneck64_train_forward", "vtd_bottleneck64_train_backward"):
        assert name in _native.SIGNATURES and hasattr(lib, name), name
        assert _native.SIGNATURES[name] == _native.SIGNATURES[name.replace("bottleneck64", "bottleneck")]      # same signatures, same struct
    for code in (ERR_ARG, ERR_ALIGN):
        assert b"64-wide Bottleneck training" in lib.vtd_strerror(code)
    assert lib.vtd_strerror(ERR_ARG) not in (lib.vtd_strerror(-3901), lib.vtd_strerror(-3903), lib.vtd_strerror(-3905))
    assert lib.vtd_strerror(ERR_ALIGN) not in (lib.vtd_strerror(-3902), lib.vtd_strerror(-3904), lib.vtd_strerror(-3906))


def _T(r, wgs):
    """The slabs of a weight-gradient launch over r rows with `wgs` workgroups per slab: 512 workgroups when the rows allow slabs of 1024."""
    return min(-(-512 // wgs), max(1, -(-r // 1024)))


def _workspace_formula(n, h, w, cin, mode):
    """include/vtd.h, vtd_bottleneck64_train_workspace_bytes: both geometries run at stride 1, so pin = pout and Min = M."""
    a256 = lambda b: (b + 255) // 256 * 256  # noqa: E731
    W, ds = 64, cin == 64
    p, M = n * (h + 2) * (w + 2), n * h * w
    if mode == 0:
        return (a256(2 * p * W) + a256(2 * p * W) + (a256(2 * p * 4 * W) if ds else 0) + a256(2 * W * cin) + a256(2 * W * 9 * W) +
                a256(2 * 4 * W * W) + (a256(2 * 4 * W * cin) if ds else 0) + a256(4 * (2 * W + 2 * 4 * W)))
    # conv2: 5 q-tiles (K = 576) of one column tile; conv1: ceil(cin / 128) q-tiles of one; conv3 and the downsample: one q-tile of two
    slab = max(_T(M, 5) * W * 9 * W, _T(M, -(-cin // 128)) * W * cin, _T(M, 2) * 4 * W * W, _T(M, 2) * 4 * W * cin if ds else 0)
    return (a256(4 * M * 4 * W) + a256(4 * M * W) + a256(4 * M * W) + a256(2 * M * 4 * W) + a256(2 * M * W) + a256(2 * M * W) +
            a256(2 * p * 4 * W) + 2 * a256(2 * p * W) + a256(2 * W * 9 * W) + a256(4 * 4 * W) + a256(8 * 256 * 4 * W) + a256(4 * 256) +
            a256(8 * 4 * W) + 2 * a256(8 * W) + a256(48) + a256(4 * slab))


def test_workspace_query_equals_its_formula():
    ws = _native.load().vtd_bottleneck64_train_workspace_bytes
    for n, h, w in ((1, 2, 2), (2, 6, 4), (2, 48, 44), (32, 160, 160)):
        for cin, width, stride in GEOMS.values():
            for mode in (0, 1):
                got = ws(n, h, w, cin, width, stride, mode)
                assert got > 0 and got == _workspace_formula(n, h, w, cin, mode) and got % 256 == 0, (n, h, w, cin, mode)
    # the slab term at the product's rows (n = 32, 160 x 160: 819 200 rows): 512 or 515 workgroups in every launch, 16.8 MB
    assert [_T(819200, 5), _T(819200, 2), _T(819200, 1)] == [103, 256, 512] and [_T(4224, 5), _T(4224, 2), _T(4224, 1)] == [5, 5, 5]
    assert max(103 * 64 * 576, 256 * 64 * 256, 256 * 256 * 64, 512 * 64 * 64) * 4 == 16777216
    bad = [(2, 6, 4, 256, 128, 2), (2, 6, 4, 512, 128, 1), (2, 6, 4, 512, 256, 2), (2, 6, 4, 2048, 512, 1),      # the other families' geometries
           (2, 6, 4, 64, 64, 2), (2, 6, 4, 256, 64, 2), (2, 6, 4, 64, 64, 0), (2, 6, 4, 256, 64, 3),      # stride 2: res2 has none
           (2, 6, 4, 128, 64, 1), (2, 6, 4, 512, 64, 1), (2, 6, 4, 64, 128, 1), (2, 6, 4, 64, 32, 1),      # cin and width mismatches
           (0, 6, 4, 64, 64, 1), (2, 0, 4, 256, 64, 1), (2, 6, -2, 64, 64, 1),      # zero extents
           (1 << 16, 6, 4, 64, 64, 1), (2, 4098, 4, 64, 64, 1), (2, 4, 8192, 256, 64, 1),
           (65535, 128, 128, 256, 64, 1), (65535, 254, 254, 64, 64, 1)]      # 2^31 elements or more: pin 256 and pout 256
    for g in bad:
        assert ws(*g, 0) == ERR_ARG and ws(*g, 1) == ERR_ARG, g
    assert ws(2, 6, 4, 64, 64, 1, 2) == ERR_ARG and ws(2, 6, 4, 64, 64, 1, -1) == ERR_ARG
    # odd extents are fine at stride 1
    assert ws(1, 5, 3, 64, 64, 1, 1) > 0 and ws(1, 7, 3, 256, 64, 1, 1) > 0
    # and the other three families keep refusing width 64, with their own codes
    lib = _native.load()
    for cin, width, stride in GEOMS.values():
        for mode in (0, 1):
            assert lib.vtd_bottleneck_train_workspace_bytes(2, 6, 4, cin, width, stride, mode) == -3901
            assert lib.vtd_bottleneck256_train_workspace_bytes(2, 6, 4, cin, width, stride, mode) == -3903
            assert lib.vtd_bottleneck128_train_workspace_bytes(2, 6, 4, cin, width, stride, mode) == -3905


@pytest.mark.parametrize("geo", ["ds", "id"])
def test_forward_argument_and_alignment_errors(geo):
    """Every refusal comes before any launch, so none of this needs a device."""
    fwd = _native.load().vtd_bottleneck64_train_forward
    keep = [_aligned(4096) for _ in range(4)]
    x, ws, y, w = (k[1] for k in keep)
    cin, width, stride = GEOMS[geo]
    st = _struct(w)
    good = [x, 2, 6, 4, cin, width, stride, C.byref(st), 1e-5, ws, y, None]
    for i in (0, 7, 9, 10):      # x, params, workspace, y
        a = list(good)
        a[i] = None
        assert fwd(*a) == ERR_ARG, i
    for i, v in ((1, 0), (2, 0), (3, -4), (4, 128), (4, 512), (5, 128), (5, 256), (5, 512), (6, 2), (6, 0), (8, 0.0), (8, -1.0), (1, 1 << 16),
                 (2, 4098)):
        a = list(good)
        a[i] = v
        assert fwd(*a) == ERR_ARG, (i, v)
    for f in _native.BOTTLENECK_FIELDS:
        if geo == "id" and f in DS_FIELDS:      # the identity block ignores ds_*: such a call would pass the checks and launch
            continue
        for value, want in ((None, ERR_ARG), (C.c_void_p(w.value + 2), ERR_ALIGN)):      # a null ds_* at cin 64 among them
            st2 = _struct(w)
            setattr(st2, f, value)
            a = list(good)
            a[7] = C.byref(st2)
            assert fwd(*a) == want, f
    for i, off in ((0, 8), (10, 8), (9, 128)):      # x and y 16 bytes, the workspace 256
        a = list(good)
        a[i] = C.c_void_p(a[i].value + off)
        assert fwd(*a) == ERR_ALIGN, i


@pytest.mark.parametrize("geo", ["ds", "id"])
def test_backward_argument_and_alignment_errors(geo):
    bwd = _native.load().vtd_bottleneck64_train_backward
    keep = [_aligned(4096) for _ in range(9)]
    x, ws, y, dy, dscale, scratch, dx, dxscale, w = (k[1] for k in keep)
    cin, width, stride = GEOMS[geo]
    st, gst = _struct(w), _struct(w, LEARN_FIELDS)
    good = [x, 2, 6, 4, cin, width, stride, C.byref(st), 1e-5, ws, y, dy, dscale, C.byref(gst), scratch, dx, dxscale, None]
    for i in (0, 7, 9, 10, 11, 12, 13, 14, 16):      # every pointer but dx, which is optional; dx without its scale (16) is refused
        a = list(good)
        a[i] = None
        assert bwd(*a) == ERR_ARG, i
    for i, v in ((1, 0), (2, 0), (3, -4), (4, 128), (4, 512), (5, 128), (6, 2), (8, 0.0), (1, 1 << 16), (3, 4098)):
        a = list(good)
        a[i] = v
        assert bwd(*a) == ERR_ARG, (i, v)
    for which, fields in ((7, _native.BOTTLENECK_FIELDS), (13, LEARN_FIELDS)):
        for f in fields:
            if geo == "id" and f in DS_FIELDS:
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
def test_bottleneck64_train_refusals():
    bd, bi = nets.Bottleneck(64, 64, 1), nets.Bottleneck(256, 64, 1)
    assert hasattr(bd, "downsample") and not hasattr(bi, "downsample")
    assert nets._BOTTLENECK64 == "vtd_bottleneck64_train" and nets._BOTTLENECK64 in nets._BOTTLENECK_FAMILIES
    assert nets._BOTTLENECK64_GEOMETRIES == ((64, 64, 1, True), (256, 64, 1, False))
    for blk, geo in ((bd, "ds"), (bi, "id")):
        assert nets._bottleneck_check(blk, nets._BOTTLENECK64_GEOMETRIES, nets._BOTTLENECK64_BUILT)[0] == GEOMS[geo]
    for other in (nets.BasicBlock(64, 64, 1), nets.Bottleneck(256, 128, 2), nets.Bottleneck(512, 128, 1), nets.Bottleneck(128, 64, 1),
                  nets.Bottleneck(2048, 512, 1), nets.Bottleneck(64, 64, 2), nets.Bottleneck(256, 64, 2), torch.nn.Conv2d(4, 4, 1)):
        with pytest.raises(RuntimeError, match="64 -> 64 -> 256 stride 1"):
            nets.bottleneck64_train(other, torch.zeros((1, 64, 2, 2)))
    with pytest.raises(ValueError, match="CUDA"):
        nets.bottleneck64_train(bd, torch.zeros((1, 64, 3, 2)))      # odd extents are fine at stride 1: the CPU tensor is what is refused
    with pytest.raises(ValueError, match="CUDA"):
        nets.bottleneck64_train(bi, torch.zeros((1, 256, 3, 1), dtype=torch.float16))
    for x in (torch.zeros((1, 256, 4, 2)), torch.zeros((64, 4, 2)), None):      # a wrong channel count, not a 4-d tensor
        with pytest.raises(ValueError, match=r"\[n,64,H,W\]"):
            nets.bottleneck64_train(bd, x)
    odd = nets.Bottleneck(256, 64, 1)
    odd.bn3.eps = 1e-3
    with pytest.raises(ValueError, match="one eps"):
        nets.bottleneck64_train(odd, torch.zeros((1, 256, 2, 2)))
    # the other three families keep refusing the 64-wide blocks, with their own texts
    for blk, cin in ((bd, 64), (bi, 256)):
        with pytest.raises(RuntimeError, match="1024 -> 512 -> 2048 stride 2"):
            nets.bottleneck_train(blk, torch.zeros((1, cin, 2, 2)))
        with pytest.raises(RuntimeError, match="512 -> 256 -> 1024 stride 2"):
            nets.bottleneck256_train(blk, torch.zeros((1, cin, 2, 2)))
        with pytest.raises(RuntimeError, match="256 -> 128 -> 512 stride 2"):
            nets.bottleneck128_train(blk, torch.zeros((1, cin, 2, 2)))


def _pool(n=1, h=8, w=8, c=64, device=None):
    return torch.empty((n, h + 2, w + 2, c), dtype=torch.float16, **({} if device is None else {"device": device}))


def test_forward_padded_res2_refusals():
    net = nets.DBNet("resnet50")
    r18 = nets.DBNet("resnet18")
    fpn, head, res5, res4, res3, res2 = net.fpn, net.head, net.backbone[7], net.backbone[6], net.backbone[5], net.backbone[4]
    stem = (net.backbone[0], net.backbone[1])
    all4 = {"res5": res5, "res4": res4, "res3": res3, "res2": res2}
    taps = [_pool()]
    for kw in ({"layer4": r18.backbone[7]}, {"layer3": r18.backbone[6]}, {"layer2": r18.backbone[5]}, {"layer1": r18.backbone[4]},
               {"trunk_batch_stats": True}, {"trunk_batch_stats": ("layer4",)}, {"stem_batch_stats": True}, {"stem": stem, "stem_batch_stats": True}):
        with pytest.raises(ValueError, match="res2 -> res3 -> res4 -> res5 -> FPN -> head node"):
            fpn.forward_padded(taps, head=head, **all4, **kw)
    for kw in ({}, {"res5": res5}, {"res4": res4}, {"res3": res3}, {"res5": res5, "res4": res4}, {"res5": res5, "res3": res3},
               {"res4": res4, "res3": res3}, {"layer4": r18.backbone[7]}, {"stem": stem}):
        with pytest.raises(ValueError, match="needs res3, res4 and res5 too"):
            fpn.forward_padded(taps, head=head, res2=res2, **kw)
    with pytest.raises(ValueError, match="needs the DBHead"):
        fpn.forward_padded(taps, **all4)
    with pytest.raises(ValueError, match="needs the DBHead"):
        fpn.forward_padded(taps, stem=stem, **all4)
    with pytest.raises(ValueError, match="CUDA"):      # CPU taps: there is no CPU path
        fpn.forward_padded(taps, head=head, **all4)
    with pytest.raises(ValueError, match=r"\[pool\]"):
        fpn.forward_padded([], head=head, **all4)
    with pytest.raises(ValueError, match=r"\[image\]"):
        fpn.forward_padded([], head=head, stem=stem, **all4)
    with pytest.raises(ValueError, match="pair"):
        fpn.forward_padded(taps, head=head, stem=net.backbone[0], **all4)
    # `stem=` without `res2=` still gives the res3 node's message
    with pytest.raises(ValueError, match="res3 -> res4 -> res5 -> FPN -> head node"):
        fpn.forward_padded(taps, head=head, res5=res5, res4=res4, res3=res3, stem=stem)
    # the stage itself, judged on shapes alone: ResNet-18's layer1, a shortened or reordered stage, res3, a pooled tap of the wrong width
    p = _pool(device="meta")
    for layer, tap in ((r18.backbone[4], p), (torch.nn.Sequential(*list(res2)[:2]), p), (torch.nn.Sequential(*list(res2)[1:], res2[1]), p),
                       (torch.nn.Sequential(*list(res2), res2[2]), p), (res3, p), (None, p), (res2, _pool(c=256, device="meta")),
                       (res2, _pool(c=128, device="meta")), (res2, torch.empty((1, 10, 2, 64), dtype=torch.float16, device="meta")), (res2, None)):
        with pytest.raises(RuntimeError, match="three Bottlenecks of width 64"):
            nets._res_operands(nets._RES_STAGES[0], layer, tap, torch.device("cpu"))
    # shapes alone: any extent passes the stage, odd ones included; what is refused next is the CPU parameters
    with pytest.raises(ValueError, match="CUDA"):
        nets._res_operands(nets._RES_STAGES[0], res2, _pool(2, 5, 3, device="meta"), torch.device("cpu"))
    odd = nets.DBNet("resnet50").backbone[4]
    odd[2].bn2.eps = 1e-3
    with pytest.raises(ValueError, match="one eps"):
        nets._res_operands(nets._RES_STAGES[0], odd, p, torch.device("cpu"))
    with pytest.raises(RuntimeError, match="three Bottlenecks of width 64"):
        nets.forward_res2_padded(r18.backbone[4], _pool())
    with pytest.raises(ValueError, match="CUDA"):
        nets.forward_res2_padded(res2, _pool())
    with pytest.raises(ValueError, match="padded taps"):
        nets.forward_res2_padded(res2, None)
    # the ResNet-18 stage helpers keep refusing Bottleneck stages
    with pytest.raises(RuntimeError, match="Bottleneck training is not built"):
        nets._stage_operands(nets._STAGES[0], res2, p)
    with pytest.raises(RuntimeError, match="Bottleneck training is not built"):
        nets.forward_layer1_padded(res2, p)


@pytest.fixture
def recorded(monkeypatch):
    """The raw wrappers replaced by recorders (no device), as tests/test_res3_train.py does."""
    ev, dxs, combined = [], {}, []
    mk = lambda *shape: torch.zeros(shape)  # noqa: E731
    dtaps = [mk(1, 8, 8, 256), mk(1, 4, 4, 512), mk(1, 2, 2, 1024)]

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
        return [p.detach().clone() for p in params], [*dtaps, mk(n, h5, w5, c5)], torch.zeros((4, 2))

    def combine(a, ascale, b, bscale):
        combined.append((a, b))
        return a, ascale

    def stem_fwd(tap, geom, eps, learn, stats, *bn):
        ev.append(("stem_fwd", tuple(tap.shape), bn))
        return mk(1, 10, 10, 64), mk(1, 8, 8, 64), mk(8)

    def stem_bwd(tap, geom, eps, learn, stats, ws, pool, idx, d, ds, *bn):
        ev.append(("stem_bwd", tuple(d.shape), d is dxs[0]))
        return tuple(p.detach().clone() for p in learn)

    monkeypatch.setattr(nets, "_block_forward_raw", block_fwd)
    monkeypatch.setattr(nets, "_block_backward_raw", block_bwd)
    monkeypatch.setattr(nets, "_fpn_forward_raw", lambda taps, geom, params: (ev.append(("fpn_fwd", tuple(t.shape[3] for t in taps))), (mk(1, 10, 10, 256), mk(8)))[1])
    monkeypatch.setattr(nets, "_fpn_backward_raw", fpn_bwd)
    monkeypatch.setattr(nets, "_head_forward_raw", lambda feats, hw, *a: (mk(8), mk(1, 1, 32, 32), mk(1, 1, 32, 32), mk(4, 2, 64)))
    monkeypatch.setattr(nets, "_head_backward_raw", lambda feats, hw, tr, ws, prob, thresh, params, gp, gt, want: ([p.detach().clone() for p in params], mk(1, 8, 8, 256), mk(2)))
    monkeypatch.setattr(nets, "_combine_scaled", combine)
    monkeypatch.setattr(nets, "_stem_forward_raw", stem_fwd)
    monkeypatch.setattr(nets, "_stem_backward_raw", stem_bwd)
    return ev, dxs, combined, dtaps


B2, B3, B4, B5 = "vtd_bottleneck64_train", "vtd_bottleneck128_train", "vtd_bottleneck256_train", "vtd_bottleneck_train"
WALK_GEOMS = ([(1, 8, 8, 64, 64, 1)] + [(1, 8, 8, 256, 64, 1)] * 2 + [(1, 8, 8, 256, 128, 2)] + [(1, 4, 4, 512, 128, 1)] * 3 +
              [(1, 4, 4, 512, 256, 2)] + [(1, 2, 2, 1024, 256, 1)] * 5 + [(1, 2, 2, 1024, 512, 2), (1, 1, 1, 2048, 512, 1), (1, 1, 1, 2048, 512, 1)])


def _walk_plan(stem):
    fam = lambda i: B2 if i < 3 else B3 if i < 7 else B4 if i < 13 else B5  # noqa: E731
    blocks = tuple(nets._BlockPlan(g, i, fam(i), 12 if i in (0, 3, 7, 13) else 9) for i, g in enumerate(WALK_GEOMS))
    tap = torch.empty((1, 38, 38, 4), dtype=torch.float16) if stem else _pool()
    splan = ((1, 32, 32), 1e-5, ()) if stem else None
    return nets._TrunkPlan((tap,), (1, 1, 1, 2048), (True, 0.1, 1e-5, ()), splan, blocks, 1e-5, None, (3, 4, 6, 3))


@pytest.mark.parametrize("stem", [False, True])
def test_node_walks_sixteen_blocks_in_four_stages(recorded, stem):
    """The trunk node on the plan per = (3, 4, 6, 3): C2 .. C5 are the outputs of blocks 3, 7, 13 and 16 (counted from one); the FPN is asked
    for dC2 .. dC5 (mask 15); block 13's dx is combined with the FPN's dC4, block 7's with its dC3 and block 3's with its dC2, once each;
    block 0, res2.0, forms its dx only with a stem, and that dx is then the stem's dpool."""
    ev, dxs, combined, (dc2, dc3, dc4) = recorded
    plan = _walk_plan(stem)
    assert nets._TrunkFPNHeadTrainFn._stages(plan) == ([0, 3, 7, 13], [2, 6, 12, 15])
    params = [torch.full((1,), float(i), requires_grad=True) for i in range((3 if stem else 0) + 30 + 39 + 57 + 30 + 30)]
    assert len(params) == (189 if stem else 186)
    prob, thresh, _ = nets._TrunkFPNHeadTrainFn.apply(plan, *params)
    torch.autograd.backward([prob, thresh], [torch.ones_like(prob), torch.ones_like(thresh)])
    pool, c2, c3, c4, c5 = (1, 10, 10, 64), (1, 10, 10, 256), (1, 6, 6, 512), (1, 4, 4, 1024), (1, 3, 3, 2048)
    want = ([("stem_fwd", (1, 38, 38, 4), ())] if stem else []) + \
        [("fwd", 0, B2, None, pool), ("fwd", 1, B2, None, c2), ("fwd", 2, B2, None, c2), ("fwd", 3, B3, None, c2)] + \
        [("fwd", i, B3, None, c3) for i in range(4, 7)] + [("fwd", 7, B4, None, c3)] + [("fwd", i, B4, None, c4) for i in range(8, 13)] + \
        [("fwd", 13, B5, None, c4), ("fwd", 14, B5, None, c5), ("fwd", 15, B5, None, c5),
         ("fpn_fwd", (256, 512, 1024, 2048)), ("fpn_bwd", (256, 512, 1024, 2048), 15)] + \
        [("bwd", i, B5, (1, 1, 1, 2048), True) for i in (15, 14, 13)] + [("bwd", i, B4, (1, 2, 2, 1024), True) for i in (12, 11, 10, 9, 8, 7)] + \
        [("bwd", i, B3, (1, 4, 4, 512), True) for i in (6, 5, 4, 3)] + [("bwd", i, B2, (1, 8, 8, 256), i > 0 or stem) for i in (2, 1, 0)] + \
        ([("stem_bwd", (1, 8, 8, 64), True)] if stem else [])
    assert ev == want
    assert len(combined) == 3
    assert combined[0][0] is dxs[13] and combined[0][1] is dc4      # res5.0's strided dx + the FPN's dC4, once
    assert combined[1][0] is dxs[7] and combined[1][1] is dc3      # res4.0's strided dx + the FPN's dC3, once
    assert combined[2][0] is dxs[3] and combined[2][1] is dc2      # res3.0's strided dx + the FPN's dC2, once
    assert (dxs[0] is not None) == stem      # res2.0's dx: the stem's dpool, or not formed
    assert all(p.grad is not None and float(p.grad) == float(i) for i, p in enumerate(params))


def _plans_seen(monkeypatch):
    """forward_padded without a device: the device checks pass, the parameters' operands are the modules' own tensors, and the node is
    replaced by a recorder of (plan, learnable tensors)."""
    seen = []
    monkeypatch.setattr(nets, "_check_padded_taps", lambda taps: None)
    monkeypatch.setattr(nets.FeaturePyramidNetwork, "_live_checked", lambda self, dev: self.live_parameters())
    monkeypatch.setattr(nets.DBHead, "_train_operands", lambda self, dev: ([self.probability_head[1]], [p for p in self.parameters()], []))
    monkeypatch.setattr(nets, "_bottleneck_operands", lambda b, dev, *family: (None, None, [p for p in b.parameters()], [x for x in b.buffers()]))
    monkeypatch.setattr(nets.FeaturePyramidNetwork, "_run_node", staticmethod(lambda head, bns, plan, *learn: seen.append((plan, learn))))
    return seen


# the plans of the three shallower nodes at n = 2 and a C5 of 1 x 1 (C4 2 x 2, C3 4 x 4, C2 8 x 8), recorded from the four per-depth
# builders that the one builder replaced: every block's (n, h, w, cin, width, stride) and the count of its learnable tensors
G3 = [(2, 8, 8, 256, 128, 2), (2, 4, 4, 512, 128, 1), (2, 4, 4, 512, 128, 1), (2, 4, 4, 512, 128, 1)]
G4 = [(2, 4, 4, 512, 256, 2), (2, 2, 2, 1024, 256, 1), (2, 2, 2, 1024, 256, 1), (2, 2, 2, 1024, 256, 1), (2, 2, 2, 1024, 256, 1), (2, 2, 2, 1024, 256, 1)]
G5 = [(2, 2, 2, 1024, 512, 2), (2, 1, 1, 2048, 512, 1), (2, 1, 1, 2048, 512, 1)]
N3, N4, N5 = [12, 9, 9, 9], [12, 9, 9, 9, 9, 9], [12, 9, 9]
BN = "vtd_bottleneck_bn_train"
DEPTHS = {      # node: (the taps it reads, the backbone slots it runs, per, geometries, entries, learnable counts, batch statistics)
    "res5": (3, (7,), 3, G5, [B5] * 3, N5, False),
    "res4": (2, (6, 7), (6, 3), G4 + G5, [B4] * 6 + [B5] * 3, N4 + N5, False),
    "res3": (1, (5, 6, 7), (4, 6, 3), G3 + G4 + G5, [B3] * 4 + [B4] * 6 + [B5] * 3, N3 + N4 + N5, False),
    "res5 batch": (3, (7,), 3, G5, [BN] * 3, N5, True),
    "res4 batch": (2, (6, 7), (6, 3), G4 + G5, [BN] * 9, N4 + N5, True),
}


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("node", list(DEPTHS))
def test_forward_padded_builds_the_plan_at_every_depth(monkeypatch, node, training):
    """forward_padded at the three shallower depths and on both batch-statistics nodes: the whole plan, and the learnable tensors by
    identity -- the stages' in block order, then the FPN's ten, then the head's twenty.  A batch node advances num_batches_tracked on the
    10 / 29 BatchNorms of its stages in train() and on none in eval()."""
    ntaps, slots, per, geoms, entries, nlearn, batch = DEPTHS[node]
    net = nets.DBNet("resnet50").train(training)
    seen = _plans_seen(monkeypatch)
    bns = [m for m in net.backbone.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(bns) == 53 and not any(int(m.num_batches_tracked) for m in bns)
    kw = {f"res{i - 2}": net.backbone[i] for i in slots}
    assert net.fpn.forward_padded(_meta_taps(2)[:ntaps], head=net.head, res_batch_stats=batch, **kw) is None and len(seen) == 1
    plan, learn = seen[0]
    assert plan.per == per and type(plan.per) is type(per) and plan.geom == (2, 1, 1, 2048) and plan.beps == 1e-5 and plan.stem is None
    assert plan.bn == ((training, 0.1) if batch else None) and plan.head == (training, 0.1, 1e-5, ())
    assert [tuple(t.shape) for t in plan.taps] == [(2, 10, 10, 256), (2, 6, 6, 512), (2, 4, 4, 1024)][:ntaps]
    assert [b.geom for b in plan.blocks] == geoms and [b.entry for b in plan.blocks] == entries and [b.nlearn for b in plan.blocks] == nlearn
    blocks = [b for i in slots for b in net.backbone[i]]
    want = [p for b in blocks for p in b.parameters()] + net.fpn.live_parameters() + list(net.head.parameters())
    assert len(learn) == len(want) == sum(nlearn) + 10 + 20 and all(a is b for a, b in zip(learn, want))
    assert all(len(b.stats) == len(list(m.buffers())) and all(s is t for s, t in zip(b.stats, m.buffers())) for b, m in zip(plan.blocks, blocks))
    stage_bns = {id(m) for b in blocks for m in b.modules() if isinstance(m, torch.nn.BatchNorm2d)}
    assert len(stage_bns) == {(7,): 10, (6, 7): 29, (5, 6, 7): 42}[slots]
    assert [int(m.num_batches_tracked) for m in bns] == [int(batch and training and id(m) in stage_bns) for m in bns]


def test_forward_padded_builds_the_four_stage_plan(monkeypatch):
    """forward_padded(res2=...) hands the node sixteen blocks in the families' order with per = (3, 4, 6, 3); with `stem=` the plan has the
    stem too and the tap is the image."""
    net = nets.DBNet("resnet50")
    seen = _plans_seen(monkeypatch)
    kw = {"head": net.head, "res5": net.backbone[7], "res4": net.backbone[6], "res3": net.backbone[5], "res2": net.backbone[4]}
    net.fpn.forward_padded([_pool(2, 24, 16)], **kw)
    plan, learn = seen[-1]
    assert plan.per == (3, 4, 6, 3) and plan.stem is None and len(plan.blocks) == 16 and plan.geom == (2, 3, 2, 2048) and plan.bn is None
    assert [b.entry for b in plan.blocks] == [B2] * 3 + [B3] * 4 + [B4] * 6 + [B5] * 3
    assert [b.geom for b in plan.blocks[:4]] == [(2, 24, 16, 64, 64, 1), (2, 24, 16, 256, 64, 1), (2, 24, 16, 256, 64, 1), (2, 24, 16, 256, 128, 2)]
    assert [b.nlearn for b in plan.blocks] == [12, 9, 9, 12, 9, 9, 9, 12, 9, 9, 9, 9, 9, 12, 9, 9] and len(learn) == 186
    assert learn[0] is net.backbone[4][0].conv1.weight
    # the node needs extents that are multiples of 8 (C5 is an eighth of the pooled tap); judged on the shape, before the node runs
    for h, w in ((12, 8), (8, 4), (7, 8), (20, 16)):
        with pytest.raises(RuntimeError, match="multiples of 8"):
            net.fpn.forward_padded([_pool(1, h, w)], **kw)
    assert len(seen) == 1
    monkeypatch.setattr(nets, "_stem_operands", lambda conv, bn, tap: ((2, 96, 64), 1e-5, [conv.weight, bn.weight, bn.bias], [bn.running_mean, bn.running_var]))
    net.fpn.forward_padded([torch.empty((2, 102, 70, 4), dtype=torch.float16)], stem=(net.backbone[0], net.backbone[1]), **kw)
    plan2, learn2 = seen[-1]
    assert plan2.stem is not None and len(plan2.stem) == 3 and plan2.stem[0] == (2, 96, 64) and plan2.blocks == plan.blocks and plan2.per == plan.per
    assert len(learn2) == 189 and learn2[0] is net.backbone[0].weight and all(a is b for a, b in zip(learn2[3:], learn))


# ---- the two modes
def _grad_pattern(net):
    return {k: p.requires_grad for k, p in net.named_parameters()}


def test_res2_mode_bookkeeping():
    keys = list(nets.DBNet("resnet50").state_dict())
    net = nets.DBNet("resnet50", compute_threshold=True, trainable=MODE)
    assert net.trainable == MODE and net.trunk_bn == "frozen" and net._first_trained() == 4
    assert list(net.state_dict()) == keys
    pat = _grad_pattern(net)
    trained = [k for k, v in pat.items() if v]
    stages = ("backbone.4.", "backbone.5.", "backbone.6.", "backbone.7.")
    assert all(k.startswith(stages + ("fpn.", "head.")) for k in trained)
    assert not any(v for k, v in pat.items() if k.startswith("backbone.") and not k.startswith(stages))      # the stem
    assert sum(k.startswith("backbone.4.") for k in trained) == 30 and len(list(net.backbone[4].buffers())) == 30      # 12 + 2 x 9
    assert [sum(k.startswith(s) for k in trained) for s in stages[1:]] == [39, 57, 30]
    assert len(nets.FeaturePyramidNetwork.live_parameters(net.fpn)) == 10 and len(list(net.head.parameters())) == 20
    assert 30 + 39 + 57 + 30 + 10 + 20 == 186      # what trains in the node
    # the fused inference engine is rebuilt after any trained stage's tensors change: the key covers 2 x (30 + 57 + 39 + 30) trunk tensors
    n_head = len(list(net.head.parameters())) + len(list(net.head.buffers()))
    assert len(net._head_tensor_versions()) == n_head + len(list(net.fpn.parameters())) + 60 + 114 + 78 + 60
    v0 = net._head_tensor_versions()
    with torch.no_grad():
        net.backbone[4][2].bn3.running_var.add_(1.0)
    v1 = net._head_tensor_versions()
    assert v1 != v0
    with torch.no_grad():
        net.backbone[4][0].downsample[0].weight.mul_(1.0)
    v2 = net._head_tensor_versions()
    assert v2 != v1
    with torch.no_grad():      # the frozen stem is the trunk engine's key, not this one's
        net.backbone[0].weight.mul_(1.0)
    assert net._head_tensor_versions() == v2
    # switching between the modes, both ways
    net.set_trainable(RES3_MODE)
    p3 = _grad_pattern(net)
    assert not any(v for k, v in p3.items() if k.startswith("backbone.") and not k.startswith(stages[1:]))
    assert len(net._head_tensor_versions()) == n_head + len(list(net.fpn.parameters())) + 60 + 114 + 78
    assert net.set_trainable(MODE) is net and _grad_pattern(net) == pat
    net.set_trainable("head+fpn")
    assert not any(v for k, v in _grad_pattern(net).items() if k.startswith("backbone."))
    assert _grad_pattern(net.set_trainable(MODE)) == pat
    net.set_trainable(WHOLE)
    assert all(_grad_pattern(net).values())
    assert _grad_pattern(net.set_trainable(MODE)) == pat
    assert _grad_pattern(nets.DBNet("resnet50", trainable=MODE).set_trainable(RES3_MODE)) == p3


def test_whole_mode_bookkeeping():
    keys = list(nets.DBNet("resnet50").state_dict())
    net = nets.DBNet("resnet50", compute_threshold=True, trainable=WHOLE)
    assert net.trainable == WHOLE and net.trunk_bn == "frozen" and list(net.state_dict()) == keys
    pat = _grad_pattern(net)
    assert all(pat.values())
    assert sum(k.startswith("backbone.") for k in pat) == 3 + 30 + 39 + 57 + 30
    assert 159 + 10 + 20 == 189      # what trains in the node: the FPN's six dead tensors require grad and receive none
    n_head = len(list(net.head.parameters())) + len(list(net.head.buffers()))
    assert len(net._head_tensor_versions()) == n_head + len(list(net.fpn.parameters())) + 60 + 114 + 78 + 60 + 6
    v0 = net._head_tensor_versions()
    with torch.no_grad():
        net.backbone[0].weight.mul_(1.0)
    v1 = net._head_tensor_versions()
    assert v1 != v0
    with torch.no_grad():
        net.backbone[1].running_mean.add_(1.0)
    assert net._head_tensor_versions() != v1
    # from a narrower mode and back
    assert _grad_pattern(nets.DBNet("resnet50", trainable="head").set_trainable(WHOLE)) == pat
    p2 = _grad_pattern(nets.DBNet("resnet50", trainable=MODE))
    assert _grad_pattern(net.set_trainable(MODE)) == p2 and _grad_pattern(net.set_trainable(WHOLE)) == pat
    # a train-mode forward refuses a frozen tensor and a wrong input before anything touches a device
    net.train()
    with pytest.raises(ValueError, match=r"\[n,3,H,W\]"):
        net(torch.zeros((1, 4, 640, 640)))
    net.backbone[4][1].conv2.weight.requires_grad_(False)
    with pytest.raises(RuntimeError, match=r"backbone\.4\.1\.conv2\.weight does not require grad, but this mode trains every tensor"):
        net(torch.zeros((1, 3, 640, 640)))


@pytest.mark.parametrize("mode", [MODE, WHOLE])
def test_mode_refusals(mode):
    r18_name = "head+fpn+backbone" if mode == WHOLE else "head+fpn+layer4+layer3+layer2+layer1"
    with pytest.raises(ValueError, match=r"trains? with trainable='" + r18_name.replace("+", r"\+") + "'"):
        nets.DBNet("resnet18", trainable=mode)
    r18 = nets.DBNet("resnet18", trainable="head+fpn")
    before = _grad_pattern(r18)
    with pytest.raises(ValueError, match=r18_name.replace("+", r"\+")):
        r18.set_trainable(mode)
    assert r18.trainable == "head+fpn" and _grad_pattern(r18) == before
    for bn in ("batch", "trained", "backbone", ("layer4",), ("layer1", "layer2", "layer3", "layer4"), ("res5", "res4", "res3", "res2"), "bogus", 3):
        with pytest.raises(ValueError):
            nets.DBNet("resnet50", trainable=mode, trunk_bn=bn)
    # a refused set_trainable leaves the network as it was, from either side
    net = nets.DBNet("resnet50", trainable=mode)
    pat = _grad_pattern(net)
    for bn in ("batch", "trained", "backbone"):
        with pytest.raises(ValueError, match="frozen-statistics"):
            net.set_trainable(mode, trunk_bn=bn)
    assert net.trainable == mode and net.trunk_bn == "frozen" and _grad_pattern(net) == pat
    other = nets.DBNet("resnet50", trainable=RES3_MODE)
    p3 = _grad_pattern(other)
    with pytest.raises(ValueError, match="train with frozen-statistics"):
        other.set_trainable(mode, trunk_bn="batch")
    assert other.trainable == RES3_MODE and other.trunk_bn == "frozen" and _grad_pattern(other) == p3


def test_older_spellings_stay_refused_and_the_res2_mode_guards_the_stem():
    # ResNet-18's names are still refused on resnet50, the whole-detector one included
    for name in ("head+fpn+backbone", "head+fpn+layer4", "head+fpn+layer4+layer3", "head+fpn+layer4+layer3+layer2", "head+fpn+layer4+layer3+layer2+layer1"):
        with pytest.raises(ValueError, match="Bottleneck training is not built"):
            nets.DBNet("resnet50", trainable=name)
    for name in ("head+fpn+res2", "head+fpn+res5+res4+res3+res2+res1", "head+fpn+stem"):
        with pytest.raises(ValueError):
            nets.DBNet("resnet50", trainable=name)
    # in the res2 mode a stem tensor that requires grad is refused in a train-mode forward before anything touches a device; backbone.4 may
    net = nets.DBNet("resnet50", trainable=MODE).train()
    net.backbone[1].bias.requires_grad_(True)
    with pytest.raises(RuntimeError, match=r"backbone\.1\.bias requires grad, but backward below res2 is not implemented"):
        net(torch.zeros((1, 3, 640, 640)))
    # and in the res3 mode a res2 tensor still is
    net3 = nets.DBNet("resnet50", trainable=RES3_MODE).train()
    net3.backbone[4][2].conv3.weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match=r"backbone\.4\.2\.conv3\.weight requires grad, but backward below res3 is not implemented"):
        net3(torch.zeros((1, 3, 640, 640)))
