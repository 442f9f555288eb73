"""Train-mode (batch-statistics) BatchNorm for ResNet-18's layer2 (csrc/resblock_bn_train.hip at width 128, the vtd_trunk_bn_train_* entries),
without a device: the three C entry points exist and refuse bad arguments before any launch, the workspace query, the fixed eight-part order
of the 128-wide per-channel reductions written out in numpy -- with a control that pairs the parts linearly and must differ in a bit --, dz,
dgamma, dbeta, dW and the running update written out in fp64 torch as the kernels form them, the operands in the weight-gradient kernel's K
order (a tap per 64-column group over the 64-channel input), against autograd -- with negative controls that must miss by at least 10x the
GPU tests' gradient ceiling --, the refusals and acceptances of the new Python spellings, and the call schedule of the layer2 -> layer3 ->
layer4 -> FPN -> head node with batch statistics."""
import ctypes as C
import pathlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_trunk_train_schedule as sched
from vtd_amd import _native, nets
from vtd_amd.nets import trunk_block_bn_train  # noqa: F401  (the feature under test: absent before it)

ENTRIES = ("vtd_trunk_bn_train_workspace_bytes", "vtd_trunk_bn_train_forward", "vtd_trunk_bn_train_backward")
GEOMETRIES = ((64, 128, 2), (128, 128, 1), (128, 256, 2), (256, 256, 1), (256, 512, 2), (512, 512, 1))
NOT_RESNET18 = ((64, 256, 2), (128, 128, 2), (96, 128, 1))      # geometries no ResNet-18 stage has
GRAD_CEILING = 1e-2      # the GPU tests' ceiling on gradients and dx (tests/test_gpu_layer2_bn_train.py)
STAGES = ("layer2", "layer3", "layer4")
MODE3 = "head+fpn+layer4+layer3+layer2"


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
    for code in (-3701, -3702):
        assert b"batch-statistics" in lib.vtd_strerror(code)
    assert len({lib.vtd_strerror(code) for code in (-3701, -3702, -3501)}) == 3


def test_workspace_query():
    lib = _native.load()
    ws, frozen, old = lib.vtd_trunk_bn_train_workspace_bytes, lib.vtd_resblock_train_workspace_bytes, lib.vtd_block_bn_train_workspace_bytes
    for cin, width, stride in GEOMETRIES:
        for h, w in ((3, 2), (12, 11), (23, 23)):
            geom = (2, h * stride, w * stride, cin, width, stride)
            for mode in (0, 1):
                assert ws(*geom, mode) > 0 and ws(*geom, mode) % 256 == 0, (geom, mode)
                assert ws(*geom, mode) >= frozen(*geom, mode)      # training = 0 runs the frozen path in the same allocation
                if width > 128:
                    assert ws(*geom, mode) == old(*geom, mode)      # the four old geometries: the same layouts
    for cin, width, stride in NOT_RESNET18:
        assert ws(2, 6, 4, cin, width, stride, 0) == -3701 and ws(2, 6, 4, cin, width, stride, 1) == -3701
    assert ws(2, 5, 4, 64, 128, 2, 0) == -3701 and ws(0, 3, 2, 128, 128, 1, 0) == -3701
    for mode in (-1, 2):
        assert ws(2, 3, 2, 128, 128, 1, mode) == -3701 and ws(2, 6, 4, 64, 128, 2, mode) == -3701
    # the older family keeps refusing layer2's geometries
    assert old(2, 6, 4, 64, 128, 2, 0) == -3501 and old(2, 3, 2, 128, 128, 1, 1) == -3501


def test_refusals_before_any_launch():
    lib = _native.load()
    keep = [_aligned(4096) for _ in range(3)]
    a, b, c = (k[1] for k in keep)
    st = _native.BasicBlockParams(*([a] * 15))
    sp = C.byref(st)
    fwd, bwd = lib.vtd_trunk_bn_train_forward, lib.vtd_trunk_bn_train_backward
    for s1, s2 in (((2, 3, 2, 128, 128, 1), (2, 6, 4, 64, 128, 2)), ((2, 3, 2, 256, 256, 1), (2, 6, 4, 128, 256, 2)),
                   ((2, 3, 2, 512, 512, 1), (2, 6, 4, 256, 512, 2))):
        cin2, width = s2[3], s2[4]
        for tr in (0, 1):
            # -3701: null pointers, eps <= 0, odd extents at stride 2, geometries no ResNet-18 stage has
            assert fwd(None, *s1, sp, tr, 0.1, 1e-5, b, c, None, None) == -3701
            assert fwd(a, *s1, None, tr, 0.1, 1e-5, b, c, None, None) == -3701
            assert fwd(a, *s1, sp, tr, 0.1, 1e-5, None, c, None, None) == -3701
            assert fwd(a, *s1, sp, tr, 0.1, 1e-5, b, None, None, None) == -3701
            assert fwd(a, *s1, sp, tr, 0.1, 0.0, b, c, None, None) == -3701
            assert fwd(a, *s1, sp, tr, 0.1, -1e-5, b, c, None, None) == -3701
            assert fwd(a, 2, 5, 4, cin2, width, 2, sp, tr, 0.1, 1e-5, b, c, None, None) == -3701
            assert fwd(a, 2, 6, 3, cin2, width, 2, sp, tr, 0.1, 1e-5, b, c, None, None) == -3701
            for cin, wd, stride in NOT_RESNET18:
                geom = (2, 6, 4, cin, wd, stride)
                assert fwd(a, *geom, sp, tr, 0.1, 1e-5, b, c, None, None) == -3701, geom
                assert bwd(a, *geom, sp, tr, 1e-5, b, c, a, a, sp, b, None, None, None) == -3701, geom
            nods = _native.BasicBlockParams(*([a] * 10))
            assert fwd(a, *s2, C.byref(nods), tr, 0.1, 1e-5, b, c, None, None) == -3701      # the stride-2 block needs its downsample
            assert bwd(a, *s2, C.byref(nods), tr, 1e-5, b, c, a, a, sp, b, None, None, None) == -3701
            assert bwd(a, *s1, sp, tr, 1e-5, b, c, None, a, sp, b, None, None, None) == -3701
            assert bwd(a, *s1, sp, tr, 0.0, b, c, a, a, sp, b, None, None, None) == -3701
            assert bwd(a, *s1, sp, tr, 1e-5, b, c, a, a, None, b, None, None, None) == -3701
            assert bwd(a, *s1, sp, tr, 1e-5, b, c, a, a, sp, None, None, None, None) == -3701
            assert bwd(a, *s1, sp, tr, 1e-5, b, c, a, a, sp, b, c, None, None) == -3701      # dx without a place for its scale
            assert bwd(a, *s2, sp, tr, 1e-5, b, c, a, a, sp, b, c, None, None) == -3701
            assert bwd(a, 2, 5, 4, cin2, width, 2, sp, tr, 1e-5, b, c, a, a, sp, b, None, None, None) == -3701
            # -3702: alignment
            assert fwd(a, *s1, sp, tr, 0.1, 1e-5, C.c_void_p(b.value + 128), c, None, None) == -3702
            assert fwd(C.c_void_p(a.value + 8), *s1, sp, tr, 0.1, 1e-5, b, c, None, None) == -3702
            assert bwd(a, *s1, sp, tr, 1e-5, b, c, C.c_void_p(a.value + 4), a, sp, b, None, None, None) == -3702      # a misaligned dy
            assert bwd(a, *s1, sp, tr, 1e-5, b, c, a, C.c_void_p(a.value + 4), sp, b, None, None, None) == -3702
            # a dx on the stride-2 block is accepted: with a misaligned dx the call gets past every argument check, and nothing launches
            assert bwd(a, *s2, sp, tr, 1e-5, b, c, a, a, sp, b, C.c_void_p(c.value + 4), a, None) == -3702
            assert bwd(a, *s2, sp, tr, 1e-5, b, c, a, a, sp, b, c, C.c_void_p(a.value + 4), None) == -3702
        # training outside {0, 1}, momentum outside [0, 1] or NaN
        for tr in (2, -1):
            assert fwd(a, *s1, sp, tr, 0.1, 1e-5, b, c, None, None) == -3701
            assert bwd(a, *s1, sp, tr, 1e-5, b, c, a, a, sp, b, None, None, None) == -3701
        for mom in (1.5, -0.1, float("nan")):
            assert fwd(a, *s1, sp, 1, mom, 1e-5, b, c, None, None) == -3701
            assert fwd(a, *s2, sp, 1, mom, 1e-5, b, c, None, None) == -3701
        # training = 1 with n h w = 1: one value per channel has no variance
        one, one2 = (1, 1, 1, s1[3], width, 1), (1, 2, 2, cin2, width, 2)
        assert fwd(a, *one, sp, 1, 0.1, 1e-5, b, c, None, None) == -3701
        assert bwd(a, *one, sp, 1, 1e-5, b, c, a, a, sp, b, None, None, None) == -3701
        assert fwd(a, *one2, sp, 1, 0.1, 1e-5, b, c, None, None) == -3701
        assert bwd(a, *one2, sp, 1, 1e-5, b, c, a, a, sp, b, None, None, None) == -3701
    # the older families keep their own answers for layer2's geometries
    assert lib.vtd_block_bn_train_forward(a, 2, 6, 4, 64, 128, 2, sp, 1, 0.1, 1e-5, b, c, None, None) == -3501
    assert lib.vtd_block_bn_train_backward(a, 2, 3, 2, 128, 128, 1, sp, 1, 1e-5, b, c, a, a, sp, b, None, None, None) == -3501
    assert lib.vtd_resblock_bn_train_forward(a, 2, 3, 2, 128, 128, 1, sp, 1, 0.1, 1e-5, b, c, None, None) == -3401


# ---- the fixed order of the 128-wide per-channel reductions (include/vtd.h): eight parts per workgroup cut at ceil(k r / 8),
# ((q0 + q1) + (q2 + q3)) + ((q4 + q5) + (q6 + q7)), the workgroups in order
def _eighth_cuts(r):
    return [(k * r + 7) // 8 for k in range(9)]


def _reduce128(v, pairing="tree"):
    """The channel sums of v [rows][C] in the kernels' order, fp64.  pairing="linear" is the control: the same parts summed left to right."""
    rows = v.shape[0]
    red = min(256, max(1, -(-rows // 256)))
    per = -(-rows // red)
    total = np.zeros(v.shape[1], np.float64)
    for g in range(red):
        m0, m1 = min(g * per, rows), min(g * per + per, rows)
        cuts = _eighth_cuts(m1 - m0)
        q = []
        for k in range(8):
            s = np.zeros(v.shape[1], np.float64)
            for m in range(m0 + cuts[k], m0 + cuts[k + 1]):      # row order
                s = s + v[m].astype(np.float64)
            q.append(s)
        if pairing == "tree":
            part = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]))
        else:
            part = q[0]
            for k in range(1, 8):
                part = part + q[k]
        total = total + part      # workgroup order
    return total


def test_reduce_order_of_the_128_wide_blocks():
    assert _eighth_cuts(1) == [0, 1, 1, 1, 1, 1, 1, 1, 1]      # ceil(k / 8): one row, the first part has it
    assert _eighth_cuts(3) == [0, 1, 1, 2, 2, 2, 3, 3, 3]
    assert _eighth_cuts(9) == [0, 2, 3, 4, 5, 6, 7, 8, 9]
    # the GPU tests' 12 x 11 case: 264 rows are two workgroups of 132 rows, eighths of 17 and 16 rows
    assert _eighth_cuts(132) == [0, 17, 33, 50, 66, 83, 99, 116, 132]
    # the 23 x 23 case: 1058 rows are five workgroups of 212 rows, the last of 210
    assert min(256, -(-1058 // 256)) == 5 and -(-1058 // 5) == 212 and 1058 - 4 * 212 == 210
    assert _eighth_cuts(212) == [0, 27, 53, 80, 106, 133, 159, 186, 212]
    assert _eighth_cuts(210) == [0, 27, 53, 79, 105, 132, 158, 184, 210]
    for r in range(0, 300):      # a partition of the rows, in order, whatever r
        cuts = _eighth_cuts(r)
        assert cuts[0] == 0 and cuts[8] == r and all(x <= y for x, y in zip(cuts, cuts[1:]))
    rng = np.random.default_rng(4)
    differs = 0
    for rows in (1, 2, 3, 7, 9, 66, 264, 1058):
        v = (rng.standard_normal((rows, 8)) * 3 + 0.5).astype(np.float32)
        want = v.astype(np.float64).sum(0)
        got = _reduce128(v)
        assert np.all(np.abs(got - want) <= 1e-13 * np.abs(v.astype(np.float64)).sum(0)), rows
        # the sums of z^2 and of g xh add fp64 products of fp32 values, which round: there the order shows
        sq = v.astype(np.float64) ** 2
        got = _reduce128(sq)
        assert np.all(np.abs(got - sq.sum(0)) <= 1e-13 * sq.sum(0)), rows
        differs += int(np.any(got != _reduce128(sq, "linear")))
    assert differs > 0, "the pairing of the eight parts is pinned: a linear sum of the same parts must differ in a bit on some input"


# ---- dz, dgamma, dbeta, dW and the running update as the kernels form them, against autograd in fp64.  The input has the real 64 or 128
# channels, because the weight-gradient kernel's K order depends on them; the width is reduced (128 -> 5): a relative L2 miss of a wrong
# formula does not depend on it.
EPS, MOMENTUM = 1e-5, 0.1
GAMMA = [1.3, 0.0, -0.75, 0.4, 2.0]      # a gamma = 0 channel and a gamma < 0 channel
CASES = {"l2s2-conv1": (64, 2, 3), "l2s2-downsample": (64, 2, 1), "l2s1-conv1": (128, 1, 3)}


def _case(cin, stride, ksz, seed=5, hw=(3, 2)):
    gen = torch.Generator().manual_seed(seed + cin + ksz)
    cout, (h, w) = len(GAMMA), hw
    x = torch.randn((2, cin, h * stride, w * stride), generator=gen).double()
    wt = (torch.randn((cout, cin, ksz, ksz), generator=gen).double() / (cin * ksz * ksz) ** 0.5).requires_grad_(True)
    gam, bet = torch.tensor(GAMMA).double().requires_grad_(True), torch.randn(cout, generator=gen).double().requires_grad_(True)
    rmean, rvar = torch.randn(cout, generator=gen).double() * 0.05, 1.0 + 0.2 * torch.rand(cout, generator=gen).double()
    start = (rmean.clone(), rvar.clone())
    z = F.conv2d(x, wt, None, stride, ksz // 2)
    z.retain_grad()
    o = F.batch_norm(z, rmean, rvar, gam, bet, True, MOMENTUM, EPS)
    g = torch.randn(o.shape, generator=gen).double() + 0.5
    o.backward(g)
    return dict(x=x, w=wt.detach(), gam=gam.detach(), z=z.detach(), g=g, dz=z.grad, dw=wt.grad, dgam=gam.grad, dbet=bet.grad, start=start,
                running=(rmean, rvar), cin=cin, stride=stride, ksz=ksz)


def _rows(t):
    """[n, C, h, w] -> the kernels' [n h w][C]."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _bn_backward(z, g, gam, bug=None):
    """(dz, dgamma, dbeta, mu, sigma^2) on rows [M][C], as bt_bwd_reduce / bt_bwd_finish / bt_form form them."""
    M = z.shape[0]
    mu, var = z.mean(0), z.var(0, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + EPS)
    xh = (z - mu) * rstd
    s1, s2 = g.sum(0), (g * xh).sum(0)
    dz = gam * rstd * (g - s1 / M - (0 if bug == "s2_term_dropped" else xh * s2 / M))
    return dz, s2, s1, mu, var


def _gather(x, cin, stride, ksz, h, w, bug=None):
    """B [M][K], K = ksz^2 cin: the weight-gradient kernel's operand in its K order.  A q-tile is 128 columns, two groups of 64; over a
    64-channel input (wgrad_mfma.h MODE 4) each group decodes its own tap, group 2 qt + grp holding channels (128 qt + 64 grp) % cin of tap
    (128 qt + 64 grp) / cin, and columns at or past K are not stored; over 128 channels (MODE 3) the q-tile decodes one tap."""
    n, K, st = x.shape[0], ksz * ksz * cin, 1 if bug == "stride1_gather" else stride
    xp = F.pad(x, (1, 1, 1, 1))      # the ring-padded tap
    B = torch.zeros((n * h * w, K), dtype=torch.float64)
    o = 1 - (ksz >> 1)
    for qt in range((K + 127) // 128):
        for grp in range(2):
            q0 = qt * 128 + grp * 64
            if q0 >= K:
                continue
            if cin & 127:
                tap, c0 = q0 // cin, q0 % cin
            else:
                tap = (qt * 128) // cin
                c0 = qt * 128 - tap * cin + grp * 64
            ky, kx = tap // ksz, tap % ksz
            win = xp[:, c0:c0 + 64, ky + o:ky + o + st * (h - 1) + 1:st, kx + o:kx + o + st * (w - 1) + 1:st]
            B[:, q0:q0 + 64] = _rows(win)
    return B


def _dw(dz, B, cin, ksz):
    """dW [c][ci][tap] = sum_m dz[m][c] B[m][tap cin + ci], as bt_dw_kernel stores it."""
    G = dz.t() @ B
    return G.reshape(dz.shape[1], ksz * ksz, cin).permute(0, 2, 1).reshape(dz.shape[1], cin, ksz, ksz)


@pytest.mark.parametrize("name", sorted(CASES))
def test_formulas_match_autograd(name):
    c = _case(*CASES[name])
    h, w = c["z"].shape[2:]
    z, g = _rows(c["z"]), _rows(c["g"])
    M = z.shape[0]
    dz, dgam, dbet, mu, var = _bn_backward(z, g, c["gam"])
    assert _rel(dz, _rows(c["dz"])) <= 1e-12
    assert _rel(dgam, c["dgam"]) <= 1e-12 and _rel(dbet, c["dbet"]) <= 1e-12
    assert float(dz[:, 1].abs().max()) == 0 and float(dgam[1].abs()) > 0 and float(dz[:, 2].abs().max()) > 0      # gamma = 0, gamma < 0
    B = _gather(c["x"], c["cin"], c["stride"], c["ksz"], h, w)
    assert _rel(B @ c["w"].permute(0, 2, 3, 1).reshape(len(GAMMA), -1).t(), z) <= 1e-12      # the forward panel's k = tap cin + ci
    dw = _dw(dz, B, c["cin"], c["ksz"])
    assert _rel(dw, c["dw"]) <= 1e-12 and float(dw[1].abs().max()) == 0
    # torch's running update: the unbiased variance, M / (M - 1)
    rmean, rvar = c["start"]
    assert _rel((1 - MOMENTUM) * rmean + MOMENTUM * mu, c["running"][0]) <= 1e-12
    assert _rel((1 - MOMENTUM) * rvar + MOMENTUM * var * M / (M - 1), c["running"][1]) <= 1e-12
    # another seed, another extent
    c = _case(*CASES[name], seed=9, hw=(2, 5))
    dz = _bn_backward(_rows(c["z"]), _rows(c["g"]), c["gam"])[0]
    assert _rel(_dw(dz, _gather(c["x"], c["cin"], c["stride"], c["ksz"], 2, 5), c["cin"], c["ksz"]), c["dw"]) <= 1e-12


def test_negative_controls_miss_by_ten_times_the_ceiling():
    for name in sorted(CASES):
        c = _case(*CASES[name])
        h, w = c["z"].shape[2:]
        z, g = _rows(c["z"]), _rows(c["g"])
        err = _rel(_bn_backward(z, g, c["gam"], bug="s2_term_dropped")[0], _rows(c["dz"]))
        assert err >= 10 * GRAD_CEILING, f"{name}: dz without xh s2 / M misses by {err:.3g} only"
        if c["stride"] == 2:
            dz = _bn_backward(z, g, c["gam"])[0]
            err = _rel(_dw(dz, _gather(c["x"], c["cin"], 2, c["ksz"], h, w, bug="stride1_gather"), c["cin"], c["ksz"]), c["dw"])
            assert err >= 10 * GRAD_CEILING, f"{name}: a stride-1 gather misses by {err:.3g} only"


# ---- the Python surface
def test_trunk_block_bn_train_refusals_and_acceptances():
    with pytest.raises(RuntimeError, match="Bottleneck training is not built"):
        nets.trunk_block_bn_train(nets.Bottleneck(256, 64, 1), torch.zeros((1, 256, 2, 2)))
    # the six geometries get as far as the device check, with an input that requires grad at either stride
    for cin, width, stride in GEOMETRIES:
        with pytest.raises(ValueError, match="CUDA"):
            nets.trunk_block_bn_train(nets.BasicBlock(cin, width, stride), torch.zeros((2, cin, 2 * stride, 2 * stride), requires_grad=True))
    with pytest.raises(RuntimeError, match="layer2, layer3 and layer4"):      # what is built is named before the device is looked at
        nets.trunk_block_bn_train(nets.BasicBlock(64, 256, 2), torch.zeros((2, 64, 4, 4)))
    blk = nets.BasicBlock(128, 128, 1)
    with pytest.raises(ValueError, match="must be a"):
        nets.trunk_block_bn_train(blk, torch.zeros((2, 64, 2, 2)))
    blk.bn2.momentum = None
    with pytest.raises(ValueError, match="momentum"):
        nets.trunk_block_bn_train(blk, torch.zeros((2, 128, 2, 2)))
    blk.bn2.momentum = 0.2      # differing momenta
    with pytest.raises(ValueError, match="momentum"):
        nets.trunk_block_bn_train(blk, torch.zeros((2, 128, 2, 2)))
    # the older spelling keeps refusing layer2's blocks
    with pytest.raises(RuntimeError, match="layer3 and layer4"):
        nets.basic_block_bn_train(nets.BasicBlock(64, 128, 2), torch.zeros((2, 64, 4, 4)))


def _node():
    trunk = nets.make_trunk("resnet18")
    return trunk, nets.FeaturePyramidNetwork(512), nets.DBHead(256), [torch.zeros((1, 18, 18, 64), dtype=torch.float16)]


def test_forward_padded_accepts_the_three_stage_tuple():
    trunk, fpn, head, taps = _node()
    stages = dict(layer4=trunk[7], layer3=trunk[6], layer2=trunk[5])
    # the accepted node goes on to its own checks: CPU taps are refused as without the argument, for a tuple and for a list
    for spelling in (STAGES, list(STAGES)):
        with pytest.raises(ValueError, match="CUDA"):
            fpn.forward_padded(taps, head=head, trunk_batch_stats=spelling, **stages)
    # the tuple without layer2, or with a stage below it
    with pytest.raises(ValueError, match=r"\('layer3', 'layer4'\)"):
        fpn.forward_padded(taps, head=head, layer4=trunk[7], layer3=trunk[6], trunk_batch_stats=STAGES)
    with pytest.raises(ValueError, match="layer2 -> layer3 -> layer4 -> FPN -> head"):
        fpn.forward_padded(taps, head=head, layer1=trunk[4], trunk_batch_stats=STAGES, **stages)
    with pytest.raises(ValueError, match="layer3 -> layer4 -> FPN -> head"):
        fpn.forward_padded(taps, head=head, trunk_batch_stats=("layer3", "layer4"), **stages)
    for bad in (("layer2",), ("layer2", "layer3"), ("layer4", "layer3", "layer2"), ("layer2", "layer4")):
        with pytest.raises(ValueError, match=r"\('layer3', 'layer4'\)"):
            fpn.forward_padded(taps, head=head, trunk_batch_stats=bad, **stages)


@pytest.mark.parametrize("what", ["eps", "mode", "momentum", "no momentum"])
def test_forward_padded_plan_is_node_wide(what):
    """One mode, one momentum and one eps over the six blocks, else ValueError -- before the taps' device is looked at."""
    trunk, fpn, head, taps = _node()
    if what == "eps":
        trunk[5][1].bn1.eps = 1e-3
    elif what == "mode":
        trunk[6][0].eval()
    elif what == "momentum":
        trunk[5][0].downsample[1].momentum = 0.2
    else:
        trunk[7][1].bn2.momentum = None
    with pytest.raises(ValueError, match="one BatchNorm eps" if what == "eps" else "one mode"):
        fpn.forward_padded(taps, head=head, layer4=trunk[7], layer3=trunk[6], layer2=trunk[5], trunk_batch_stats=STAGES)


def test_dbnet_trunk_bn_trained():
    net = nets.DBNet("resnet18", trainable=MODE3, trunk_bn="trained")
    assert net.trainable == MODE3 and net.trunk_bn == "trained"
    assert list(net.state_dict()) == list(nets.DBNet("resnet18").state_dict())      # the state dict is the reference's, whatever the mode
    assert [i for i in range(8) if any(p.requires_grad for p in net.backbone[i].parameters())] == [5, 6, 7]
    assert all(p.requires_grad for i in (5, 6, 7) for p in net.backbone[i].parameters())
    with pytest.raises(ValueError, match="trunk_bn='trained'"):      # the kept "trained" does not fit the new mode
        net.set_trainable(None)
    assert net.trainable == MODE3 and net.trunk_bn == "trained"      # and the network is as it was
    assert [i for i in range(8) if any(p.requires_grad for p in net.backbone[i].parameters())] == [5, 6, 7]
    for mode in ("head+fpn+layer4", "head+fpn+layer4+layer3", MODE3):
        assert nets.DBNet("resnet18", trainable=mode, trunk_bn="trained").trunk_bn == "trained"
        assert net.set_trainable(mode).trunk_bn == "trained"
    assert net.set_trainable(None, "frozen").trunk_bn == "frozen"
    for mode in (None, "head", "head+fpn"):
        with pytest.raises(ValueError, match="trunk_bn='trained'"):
            nets.DBNet("resnet18", trainable=mode, trunk_bn="trained")
    for mode in (None, "head+fpn", "head+fpn+layer4", MODE3):
        with pytest.raises(ValueError):
            nets.DBNet("resnet50", trainable=mode, trunk_bn="trained")
    # the tuple spelling of the three stages stays refused on DBNet, and the default stays "frozen"
    with pytest.raises(ValueError, match="names exactly the residual stages"):
        nets.DBNet("resnet18", trainable=MODE3, trunk_bn=STAGES)
    assert nets.DBNet("resnet18", trainable=MODE3).trunk_bn == "frozen"


@pytest.mark.parametrize("mode, taps, stages", [("head+fpn+layer4", ["C2", "C3", "C4"], ("layer4",)),
                                                ("head+fpn+layer4+layer3", ["C2", "C3"], ("layer3", "layer4")), (MODE3, ["C2"], STAGES)])
def test_dbnet_passes_the_stages_to_the_node(monkeypatch, mode, taps, stages):
    """The train-mode forward hands the trunk engine's taps below the lowest trained stage, the trained stages and their names to
    forward_padded: with every stage from layer2 up, ["C2"], the three stages and the three-stage tuple."""
    net = nets.DBNet("resnet18", trainable=mode, trunk_bn="trained")
    seen = {}

    class Engine:
        def forward_trunk(self, x):
            return ["C2", "C3", "C4", "C5"]

    def forward_padded(taps, **kw):
        seen.update(kw, taps=taps)
        return "out"

    monkeypatch.setattr(net, "trunk_engine", lambda: Engine())
    monkeypatch.setattr(net.fpn, "forward_padded", forward_padded)
    for m in (net.backbone[5], net.backbone[6], net.backbone[7], net.fpn, net.head):
        monkeypatch.setattr(m, "cuda", lambda: None)
    version = net._version
    assert net.train()(torch.zeros((2, 3, 640, 640))) == "out"
    assert seen["taps"] == taps and seen["trunk_batch_stats"] == stages and seen["head"] is net.head
    for j in (2, 3, 4):
        if f"layer{j}" in stages:
            assert seen[f"layer{j}"] is net.backbone[3 + j]
        else:
            assert f"layer{j}" not in seen
    assert "layer1" not in seen and "stem" not in seen
    assert net._version == version + 1      # the running statistics moved: the next eval() forward rebuilds the inference engine
    if mode == MODE3:      # the trained stages' buffers are among the tensors whose versions the eval() forward watches
        watched = len(net._head_tensor_versions())
        above = len(nets.DBNet("resnet18", trainable="head+fpn+layer4+layer3")._head_tensor_versions())
        assert watched - above == len(list(net.backbone[5].parameters())) + len(list(net.backbone[5].buffers())) == 15 + 15
        before = net._head_tensor_versions()
        net.backbone[5][1].bn2.running_var.add_(1.0)
        assert net._head_tensor_versions() != before


# ---- the call schedule of the new node, with the recording fakes of tests/test_trunk_train_schedule.py
NB = "vtd_trunk_bn_train"
MODE = (True, 0.1)


def test_schedule_of_the_layer2_layer3_layer4_node_with_batch_statistics(monkeypatch):
    assert nets._TRUNK_BN == NB
    events, params = sched._run(monkeypatch, taps=("C2",), nblocks=6, entries=(NB,) * 6, bn=MODE)
    want = [
        ("block_fwd", 0, NB, MODE, "C2"), ("block_fwd", 1, NB, MODE, "y0"), ("block_fwd", 2, NB, MODE, "y1"), ("block_fwd", 3, NB, MODE, "y2"),
        ("block_fwd", 4, NB, MODE, "y3"), ("block_fwd", 5, NB, MODE, "y4"),
        ("fpn_fwd", ("C2", "y1", "y3", "y5")), sched.HEAD_FWD, sched.HEAD_BWD,
        ("fpn_bwd", ("C2", "y1", "y3", "y5"), "fws", "dp2", "dp2s", 8 | 4 | 2),
        ("block_bwd", 5, NB, MODE, "y4", "y5", "dC5", "sC5", True),
        ("block_bwd", 4, NB, MODE, "y3", "y4", "dx5", "dxs5", True),      # layer4.0 forms its dx
        ("combine", "dx4", "dxs4", "dC4", "sC4"),
        ("block_bwd", 3, NB, MODE, "y2", "y3", "dx4", "sum4", True),
        ("block_bwd", 2, NB, MODE, "y1", "y2", "dx3", "dxs3", True),      # layer3.0 forms its dx
        ("combine", "dx2", "dxs2", "dC3", "sC3"),
        ("block_bwd", 1, NB, MODE, "y0", "y1", "dx2", "sum2", True),
        ("block_bwd", 0, NB, MODE, "C2", "y0", "dx1", "dxs1", False),     # layer2.0 forms none
    ]
    assert events == want, "\n".join(f"{'  ' if a == b else '!!'} {a}   |   {b}" for a, b in zip(events + [None] * len(want), want + [None] * len(events)))
    asked = [e[1] for e in events if e[0] == "block_bwd" and e[-1]]
    assert asked == [5, 4, 3, 2, 1] and sum(e[0] == "combine" for e in events) == 2
    assert len(params) == 75 and [float(p.grad) for p in params] == [float(i) for i in range(75)]


def test_raw_wrappers_keep_the_trunk_family(monkeypatch):
    """With `bn`, the raw wrappers run vtd_trunk_bn_train_* when the entry names that family."""
    asked = []

    def workspace(query, args, device):
        asked.append(query)
        raise LookupError

    monkeypatch.setattr(nets, "_native_workspace", workspace)
    t = torch.zeros(1)
    geom = (2, 6, 4, 64, 128, 2)
    for bn in ((True, 0.1), (False, 0.1)):
        with pytest.raises(LookupError):
            nets._block_forward_raw(t, geom, 1e-5, [t] * 9, [t] * 6, nets._TRUNK_BN, bn)
        with pytest.raises(LookupError):
            nets._block_backward_raw(t, geom, 1e-5, [t] * 9, [t] * 6, t, t, t, t, True, nets._TRUNK_BN, bn)
        assert asked[-2:] == ["vtd_trunk_bn_train_workspace_bytes"] * 2
