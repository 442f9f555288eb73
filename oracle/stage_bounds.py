"""fp64 stage references for the detector, each with a rigorous per-element error bound.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  Every stage takes the GPU's own input tap -- the exact fp16 values the
engine stored (vtd_api.cpp read_tensor_nchw) -- and returns a StageOut for the next tap:

    value  the stage computed in float64 from those inputs, with the weights the engine actually multiplies by
           (BatchNorm folded as fold_bn / build_conv do: scale and shift in double, weights half(float(double(w) * scale)))
    bound  a per-element bound on |GPU - value| for a correct kernel
    mag    the accumulation magnitude of the stage's last operation (|W|*|x| + |bias| + |residual|), the natural scale of
           its rounding error; check_stage normalises the error by it for the sharpness check

so a stage is judged in isolation: no error builds up from the stem onward.

Error model (fp16 MFMA products are exact in fp32; u16 = 2^-11, u32 = 2^-24, unit roundoffs):

    E_out = (1 + s)|W| * E_in  +  (c_acc + s) (|W| * |x|)  +  c_acc (|bias| + |residual|)  +  E_residual
            +  u16 (|y| + E_pre) + 2^-25                                   at every point where the product stores fp16

  * c_acc: a K-term dot product summed in fp32 in any order, plus the fp32 bias and residual additions and the rounding of
    the bias itself to fp32, is K + 3 additions of terms whose absolute sum is |W|*|x| + |bias| + |residual|.  Recursive
    summation in any order and with any blocking (MFMA partial sums included) has error <= gamma_{n-1} sum|t_i| with
    gamma_n = n u32 / (1 - n u32) (Higham, Accuracy and Stability of Numerical Algorithms, 4.2); n = K + 3 terms give
    c_acc = gamma_{K+3}.  The bias rounding (|float(b) - b| <= u32 |b|) is covered by the same gamma.
  * s: relative slack on |W| for weights the engine rounds where the reference does not: the host-composed head entry
    (u16 for the fp16 rounding plus 2^-14 for the fp32 intermediate products of compose_head_entry) and the last ConvT of the
    head (fp32 weights on the generic path, fp16 on the head-tail kernel: u16).  Everywhere else the reference multiplies by
    the same fp16 weights, s = 0.
  * ReLU and max are 1-Lipschitz; a residual adds its own bound.
  * Activations the engine never materialises (the 320^2 ConvT intermediate, the stem map inside the fused stem+pool) are
    treated as rounded to fp16 anyway: that only enlarges the bound.
  * The magnitude pass (|W|*|x|, |W|*E) has no cancellation, so it runs in fp32 and is inflated by (1 + 2(K+1) u32).
  * Probability: the logit is bounded as above plus 4 u32 (|l| + 1) for the fp32 exp; |dp| <= max sigma'(xi) E_logit + 2 u32
    with xi over [ref - E, ref + E].

Sharpness: the hard bound is a worst case (it grows like K u32); real errors are ~sqrt(K) smaller, so a bug can hide under
it.  check_stage therefore also compares the 99.9th percentile of z = |got - ref| / mag per region (interior, 2-pixel
border ring, rows of the last partial implicit-GEMM tile of the last frame, frames other than frame 0) with a per-stage
threshold T_stage calibrated on an MI355X (GPU parity).

All functions accept any H x W (even, so that the stride-2 stages and the composed head entry's parity classes line up).
"""
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

U16 = 2.0 ** -11
U32 = 2.0 ** -24
SUB16 = 2.0 ** -25          # half the spacing of fp16 subnormals: absolute rounding floor
COMPOSE_SLACK = U16 + 2.0 ** -14
IGEMM_TILE_ROWS = (128, 208, 256, 272)   # conv_igemm.hip tile heights (rows = output pixels of the whole batch)

_STAGES = {"resnet18": ("basic", (2, 2, 2, 2)), "resnet50": ("bottleneck", (3, 4, 6, 3))}
_WIDTH = (64, 128, 256, 512)

StageOut = namedtuple("StageOut", "value bound mag")

# Per-stage sharpness thresholds on the 99.9th percentile of z = |got - ref| / mag (3x the level of the first correct
# MI355X run; DESIGN.md, GPU parity).
T_STAGE = {                       # measured level on the MI355X (max over configurations and regions) x 3
    "stem": 6.5e-4,               # 2.16e-4
    "pool": 0.0,                  # bit-exact
    "stem_pool": 6.5e-4,          # 2.14e-4
    "c2": 2.8e-3,                 # 9.16e-4
    "c3": 3.1e-3,                 # 1.03e-3
    "c4": 4.0e-3,                 # 1.31e-3
    "c5": 1.2e-3,                 # 3.79e-4
    "p2": 1.8e-4,                 # 5.73e-5
    "head1": 9.2e-5,              # 3.04e-5
    "head1_composed": 4.8e-5,     # 1.58e-5
    "probability": 7.8e-4,        # 2.57e-4
    "threshold": 1.6e-3,          # 5.16e-4
}


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def _d(t):
    return t.detach().to(torch.float64) if torch.is_tensor(t) else torch.from_numpy(np.asarray(t)).to(torch.float64)


def h16(t):
    """double -> float -> half -> double, as the host packs weights ((half_t)(float)(double))."""
    return t.to(torch.float32).to(torch.float16).to(torch.float64)


def up2(t):
    return t.repeat_interleave(2, dim=-2).repeat_interleave(2, dim=-1)


def _conv64(x, w, stride=1, pad=0, circular=False):
    """fp64 convolution as a few large matmuls (torch's own fp64 conv is ~10x slower than its dgemm)."""
    n, c, h, wd = x.shape
    o, _, kh, kw = w.shape
    ho, wo = (h + 2 * pad - kh) // stride + 1, (wd + 2 * pad - kw) // stride + 1
    xp = F.pad(x, (pad,) * 4, mode="circular" if circular else "constant") if pad else x
    if c * kh * kw <= 640 and kh * kw > 1:
        cols = F.unfold(xp, (kh, kw), stride=stride)                     # [n, c*kh*kw, ho*wo]
        return torch.matmul(w.reshape(o, -1), cols).view(n, o, ho, wo)
    out = x.new_zeros(n, o, ho * wo)
    for r in range(kh):
        for s in range(kw):
            xs = xp[:, :, r:r + stride * (ho - 1) + 1:stride, s:s + stride * (wo - 1) + 1:stride].reshape(n, c, ho * wo)
            out += torch.matmul(w[:, :, r, s], xs)
    return out.view(n, o, ho, wo)


def _absconv(x, wabs, stride=1, pad=0):
    """fp32 convolution of non-negative operands, inflated so that it is an upper bound of the exact value."""
    k = wabs.shape[1] * wabs.shape[2] * wabs.shape[3]
    y = F.conv2d(x.to(torch.float32), wabs.to(torch.float32), None, stride, pad)
    return y.to(torch.float64) * (1.0 + 2.0 * (k + 1) * U32)


def _convt64(x, w):
    """ConvTranspose2d(k=2, s=2), w [cin, cout, 2, 2]."""
    n, c, h, wd = x.shape
    co = w.shape[1]
    y = torch.matmul(w.permute(1, 2, 3, 0).reshape(co * 4, c), x.reshape(n, c, h * wd))   # [n, co*4, h*w]
    return y.view(n, co, 2, 2, h, wd).permute(0, 1, 4, 2, 5, 3).reshape(n, co, 2 * h, 2 * wd)


def _absconvt(x, wabs):
    y = F.conv_transpose2d(x.to(torch.float32), wabs.to(torch.float32), None, 2)
    return y.to(torch.float64) * (1.0 + 2.0 * (wabs.shape[0] + 1) * U32)


def tail_rows(n, h, w):
    """Output pixels (flattened over the batch) of the last partial implicit-GEMM tile, for the union of the tile heights."""
    m = n * h * w
    r = max(m % bm for bm in IGEMM_TILE_ROWS) or 256
    return min(r, h * w)


def regions(shape, frames=None, batch=None):
    """Boolean masks [N,1,H,W] of the four sharpness regions of a tap of `shape` (N,C,H,W).  `frames`: the engine's frame
    index of each row when only some frames of a batch of `batch` are checked (default: all of them)."""
    n, _, h, w = shape
    frames = list(range(n)) if frames is None else list(frames)
    batch = n if batch is None else batch
    ring = np.zeros((h, w), bool)
    ring[:2] = ring[-2:] = True
    ring[:, :2] = ring[:, -2:] = True
    out = {"interior": np.broadcast_to(~ring, (n, 1, h, w)), "border": np.broadcast_to(ring, (n, 1, h, w))}
    tail = np.zeros((n, 1, h * w), bool)
    if batch - 1 in frames:
        tail[frames.index(batch - 1), 0, h * w - tail_rows(batch, h, w):] = True
    out["last_tile"] = tail.reshape(n, 1, h, w)
    later = np.zeros((n, 1, h, w), bool)
    later[[i for i, f in enumerate(frames) if f != 0]] = True
    if later.any():
        out["frames_1+"] = later
    return out


class Act:
    """An activation in the reference: value (fp64), error bound (fp64) and the last op's accumulation magnitude."""

    def __init__(self, v, e=None, m=None):
        self.v, self.e = v, (torch.zeros_like(v) if e is None else e)
        self.m = v.abs() if m is None else m

    def out(self):
        return StageOut(self.v, self.e, self.m)


def _store(v, e):
    """fp16 store of a value known to within e."""
    return e + U16 * (v.abs() + e) + SUB16


class StageRef:
    """Folded weights of one detector state dict and the fp64 stage functions on them.

    `fault` (tests only): (kind, op name) makes the reference compute a plausible kernel bug instead, so that negative
    controls can be built from it: 'drop_k' (one 32-channel K chunk of one 3x3 tap), 'wrap' (circular padding),
    'tail_prev' (rows of the last partial tile from the previous frame), 'res_roll' (residual from the neighbouring frame),
    'up_shift' (nearest up-sampling shifted by one pixel; op name 'fpn.<i>')."""

    def __init__(self, state_dict, backbone, fault=None):
        self.sd = {k: _d(v) for k, v in state_dict.items() if not k.endswith("num_batches_tracked")}
        self.backbone = backbone
        self.kind, self.counts = _STAGES[backbone]
        self.fault = fault or (None, None)
        self._ops = {}
        self._composed = {}

    # ---- folding (vtd_api.cpp fold_bn / build_conv / build_convt) ----
    def fold(self, bn, bias_key, cout):
        sd = self.sd
        scale = torch.ones(cout, dtype=torch.float64)
        shift = torch.zeros(cout, dtype=torch.float64)
        b = sd[bias_key] if bias_key else None
        if bn:
            s = sd[bn + ".weight"].to(torch.float32).to(torch.float64) / torch.sqrt(sd[bn + ".running_var"] + 1e-5)
            scale = s
            shift = sd[bn + ".bias"] + ((b if b is not None else 0.0) - sd[bn + ".running_mean"]) * s
        elif b is not None:
            shift = b.clone()
        return scale, shift

    def conv(self, wkey, bn, bias_key=""):
        key = (wkey, bn, bias_key)
        if key not in self._ops:
            w = self.sd[wkey]
            scale, shift = self.fold(bn, bias_key, w.shape[0])
            wq = h16(w * scale[:, None, None, None])
            self._ops[key] = (wq, wq.abs(), shift)
        return self._ops[key]

    def convt(self, wkey, bn, bias_key):
        key = (wkey, bn, bias_key)
        if key not in self._ops:
            w = self.sd[wkey]                                    # [cin, cout, 2, 2]
            scale, shift = self.fold(bn, bias_key, w.shape[1])
            wq = h16(w * scale[None, :, None, None])
            self._ops[key] = (wq, wq.abs(), shift)
        return self._ops[key]

    # ---- one stored convolution ----
    def _op(self, name, x, wq, wabs, bias, stride, pad, relu=True, res=None, second=None, store=True):
        """x: Act.  res: Act added before the ReLU.  second: (Act, wq2, wabs2, bias2, stride2), a 1x1 projection folded into
        the same accumulation (conv_igemm.hip DUAL)."""
        kind, target = self.fault
        hit = target == name
        wv = wq
        if hit and kind == "drop_k":
            wv = wq.clone()
            wv[:, 32:64, 0, wq.shape[3] - 1] = 0.0
        v = _conv64(x.v, wv, stride, pad, circular=hit and kind == "wrap") + bias[:, None, None]
        k = wq.shape[1] * wq.shape[2] * wq.shape[3]
        both = _absconv(torch.cat([x.v.abs(), x.e]), wabs, stride, pad)
        nb = x.v.shape[0]
        mag, e = both[:nb] + bias.abs()[:, None, None], both[nb:]
        if second is not None:
            x2, wq2, wabs2, b2, s2 = second
            x2v = x2.v.roll(1, 0) if hit and kind == "res_roll" else x2.v
            v = v + _conv64(x2v, wq2, s2, 0) + b2[:, None, None]
            both2 = _absconv(torch.cat([x2.v.abs(), x2.e]), wabs2, s2, 0)
            mag, e = mag + both2[:nb] + b2.abs()[:, None, None], e + both2[nb:]
            k += wq2.shape[1]
        if res is not None:
            rv = res.v.roll(1, 0) if hit and kind == "res_roll" else res.v
            v = v + rv
            mag, e = mag + res.v.abs(), e + res.e
        e = e + gamma(k + 3) * mag
        if relu:
            v = v.clamp_min(0.0)
        if hit and kind == "tail_prev" and v.shape[0] > 1:
            n, c, h, w = v.shape
            r = tail_rows(n, h, w)
            flat = v.reshape(n, c, h * w).clone()
            flat[-1, :, h * w - r:] = flat[-2, :, h * w - r:]
            v = flat.view(n, c, h, w)
        if store:
            e = _store(v, e)
        return Act(v, e, mag)

    # ---- trunk ----
    def stem(self, inp):
        """input -> stem (conv 7x7/s2/p3 + BN + ReLU)."""
        return self._stem(Act(_d(inp)[:, :3])).out()

    def _stem(self, x):
        wq, wabs, b = self.conv("backbone.0.weight", "backbone.1")
        return self._op("backbone.0", x, wq, wabs, b, 2, 3)

    @staticmethod
    def pool(stem):
        """stem -> pool (max 3x3/s2/p1 over fp16 values): bit-exact."""
        v = F.max_pool2d(_d(stem), 3, 2, 1)
        return StageOut(v, torch.zeros_like(v), v.abs())

    def stem_pool(self, inp):
        """input -> pool through the fused kernel: the stem map is never stored (treated as rounded)."""
        s = self._stem(Act(_d(inp)[:, :3]))
        v = F.max_pool2d(s.v, 3, 2, 1)
        return StageOut(v, F.max_pool2d(s.e, 3, 2, 1), F.max_pool2d(s.m, 3, 2, 1))

    def _block(self, x, pre, cin, st, b, fold_ds):
        width = _WIDTH[st]
        cout = width * 4 if self.kind == "bottleneck" else width
        stride = 2 if (b == 0 and st > 0) else 1
        proj = stride != 1 or cin != cout
        ds = second = None
        if proj:
            dq, dabs, db = self.conv(pre + ".downsample.0.weight", pre + ".downsample.1")
            if fold_ds:
                second = (x, dq, dabs, db, stride)
            else:
                ds = self._op(pre + ".downsample", x, dq, dabs, db, stride, 0, relu=False)
        res = None if second is not None else (ds if ds is not None else x)
        if self.kind == "basic":
            w1 = self.conv(pre + ".conv1.weight", pre + ".bn1")
            t1 = self._op(pre + ".conv1", x, *w1, stride, 1)
            w2 = self.conv(pre + ".conv2.weight", pre + ".bn2")
            return self._op(pre + ".conv2", t1, *w2, 1, 1, res=res, second=second), cout
        w1 = self.conv(pre + ".conv1.weight", pre + ".bn1")
        t1 = self._op(pre + ".conv1", x, *w1, 1, 0)
        w2 = self.conv(pre + ".conv2.weight", pre + ".bn2")
        t2 = self._op(pre + ".conv2", t1, *w2, stride, 1)
        w3 = self.conv(pre + ".conv3.weight", pre + ".bn3")
        return self._op(pre + ".conv3", t2, *w3, 1, 0, res=res, second=second), cout

    def layer(self, st, x, fold_ds=True):
        """pool -> c2 (st = 0), c2 -> c3, c3 -> c4, c4 -> c5: one ResNet stage, its block outputs and intermediates stored
        fp16; fold_ds: the downsample projection rides in the block's last conv (no fp16 rounding of the projected map)."""
        a = Act(_d(x))
        cin = a.v.shape[1]
        for b in range(self.counts[st]):
            a, cin = self._block(a, f"backbone.{4 + st}.{b}", cin, st, b, fold_ds)
        return a.out()

    # ---- FPN and head ----
    def _lateral(self, i, feat, last):
        wq, wabs, b = self.conv(f"fpn.inner_blocks.{i}.weight", "", f"fpn.inner_blocks.{i}.bias")
        res = None
        if last is not None:
            kind, target = self.fault
            upv = up2(last.v)
            if kind == "up_shift" and target == f"fpn.{i}":
                upv = upv.roll(1, -1)
            res = Act(upv, up2(last.e), None)
        return self._op(f"fpn.inner_blocks.{i}", Act(_d(feat)), wq, wabs, b, 1, 0, relu=False, res=res)

    def l3(self, c3, c4, c5):
        last = self._lateral(0, c5, None)
        last = self._lateral(1, c4, last)
        return self._lateral(2, c3, last)

    def _p2(self, c2, c3, c4, c5):
        l2 = self._lateral(3, c2, self.l3(c3, c4, c5))
        wq, wabs, b = self.conv("fpn.layer_blocks.3.weight", "", "fpn.layer_blocks.3.bias")
        return self._op("fpn.layer_blocks.3", l2, wq, wabs, b, 1, 1, relu=False)

    def p2(self, c2, c3, c4, c5):
        """{c2..c5} -> p2 (laterals with the top-down nearest-2x adds, each stored fp16, then the 3x3 smooth)."""
        return self._p2(c2, c3, c4, c5).out()

    def _head1(self, p2, branch):
        hp = f"head.{branch}_head."
        wq, wabs, b = self.conv(hp + "0.weight", hp + "1", hp + "0.bias")
        return self._op(hp + "0", p2, wq, wabs, b, 1, 1)

    def head1(self, p2, branch="probability"):
        """p2 -> head1 (3x3 conv + BN + ReLU)."""
        return self._head1(Act(_d(p2)), branch).out()

    def _composed_weights(self, branch):
        """|W| of compose_head_entry per (row kind, column kind): C2 part [64, c2, 5, 5] and L3 part [64, 256, 3, 3], BN scale
        applied; kinds 0 first row, 1 interior even, 2 interior odd, 3 last row.  Plus a per-channel bound on |bias|."""
        if branch in self._composed:
            return self._composed[branch]
        sd, hp = self.sd, f"head.{branch}_head."
        wl, bl = sd["fpn.inner_blocks.3.weight"][:, :, 0, 0], sd["fpn.inner_blocks.3.bias"]
        ws, bs = sd["fpn.layer_blocks.3.weight"], sd["fpn.layer_blocks.3.bias"]
        wh, bh = sd[hp + "0.weight"], sd[hp + "0.bias"]
        scale, shift = self.fold(hp + "1", "", 64)
        g = torch.einsum("omt,mcs->tsoc", wh.reshape(64, 256, 9), ws.reshape(256, 256, 9))   # [9(t), 9(s), 64, 256]
        cls_w = {}
        for cy in range(3):
            for cx in range(3):
                wc = torch.zeros(5, 5, 64, 256, dtype=torch.float64)
                for ty in range(-1, 2):
                    for tx in range(-1, 2):
                        if (cy == 0 and ty < 0) or (cy == 2 and ty > 0) or (cx == 0 and tx < 0) or (cx == 2 and tx > 0):
                            continue
                        for sy in range(-1, 2):
                            for sx in range(-1, 2):
                                wc[ty + sy + 2, tx + sx + 2] += g[(ty + 1) * 3 + tx + 1, (sy + 1) * 3 + sx + 1]
                cls_w[(cy, cx)] = wc
        out = {}
        for yk in range(4):
            for xk in range(4):
                cy, cx = (0, 1, 1, 2)[yk], (0, 1, 1, 2)[xk]
                wc = cls_w[(cy, cx)]
                a, b = int(yk >= 2), int(xk >= 2)
                w_c2 = torch.einsum("yxoc,ck->okyx", wc, wl) * scale[:, None, None, None]
                w_l3 = torch.zeros(64, 256, 3, 3, dtype=torch.float64)
                for uy in range(-2, 3):
                    for ux in range(-2, 3):
                        w_l3[:, :, (a + uy) // 2 + 1, (b + ux) // 2 + 1] += wc[uy + 2, ux + 2]
                w_l3 *= scale[:, None, None, None]
                out[(yk, xk)] = (w_c2.abs().float(), w_l3.abs().float())
        gabs = g.abs().sum((0, 1))                                          # >= |Wc| of every class, summed over u
        bias_bound = scale.abs() * (bh.abs() + (wh.abs().sum((2, 3)) @ bs.abs()) + gabs @ bl.abs()) + shift.abs()
        self._composed[branch] = (out, bias_bound)
        return self._composed[branch]

    def _head1_composed(self, c2, c3, c4, c5, branch):
        c2v = _d(c2)
        l3 = self.l3(c3, c4, c5)
        sd, hp = self.sd, f"head.{branch}_head."
        # value: the reference graph itself in fp64 with the state dict's weights (the composition is exact algebra)
        l2 = _conv64(c2v, sd["fpn.inner_blocks.3.weight"]) + sd["fpn.inner_blocks.3.bias"][:, None, None] + up2(l3.v)
        p2 = _conv64(l2, sd["fpn.layer_blocks.3.weight"], 1, 1) + sd["fpn.layer_blocks.3.bias"][:, None, None]
        scale, shift = self.fold(hp + "1", hp + "0.bias", 64)
        v = (_conv64(p2, sd[hp + "0.weight"], 1, 1) * scale[:, None, None] + shift[:, None, None]).clamp_min(0.0)
        # magnitude and propagated L3 error through |W| of each weight class
        wcls, bias_bound = self._composed_weights(branch)
        n, _, h, w = c2v.shape
        kinds = lambda size: torch.tensor([0] + [1 + (i & 1) for i in range(1, size - 1)] + [3])
        yk, xk = kinds(h), kinds(w)
        nb = n
        l3in = torch.cat([l3.v.abs(), l3.e]).float()
        mag = torch.zeros(n, 64, h, w, dtype=torch.float64)
        e = torch.zeros_like(mag)
        infl = 1.0 + 2.0 * (c2v.shape[1] * 25 + 2304 + 1) * U32
        for (a, b), (w_c2, w_l3) in wcls.items():
            rows, cols = (yk == a).nonzero()[:, 0], (xk == b).nonzero()[:, 0]
            if len(rows) == 0 or len(cols) == 0:
                continue
            m2 = F.conv2d(c2v.abs().float(), w_c2, None, 1, 2)[:, :, rows][:, :, :, cols]
            m3 = up2(F.conv2d(l3in, w_l3, None, 1, 1))[:, :, rows][:, :, :, cols]
            mag[:, :, rows[:, None], cols] = (m2 + m3[:nb]).double() * infl
            e[:, :, rows[:, None], cols] = m3[nb:].double() * infl
        mag = mag + bias_bound[:, None, None]
        k = c2v.shape[1] * 25 + 2304
        e = (1 + COMPOSE_SLACK) * e + (gamma(k + 3) + COMPOSE_SLACK) * mag
        return Act(v, _store(v, e), mag)

    def head1_composed(self, c2, c3, c4, c5, branch="probability"):
        """{c2..c5} -> head1 through the composed entry (laterals of C5, C4, C3 stored fp16 as L3; then one classed conv on
        C2 and L3 with host-composed fp16 weights)."""
        return self._head1_composed(c2, c3, c4, c5, branch).out()

    def _tail(self, h1, branch):
        hp = f"head.{branch}_head."
        wq, wabs, b = self.convt(hp + "3.weight", hp + "4", hp + "3.bias")
        v = _convt64(h1.v, wq) + b[:, None, None]
        both = _absconvt(torch.cat([h1.v.abs(), h1.e]), wabs)
        nb = h1.v.shape[0]
        mag = both[:nb] + b.abs()[:, None, None]
        e = both[nb:] + gamma(64 + 3) * mag
        v = v.clamp_min(0.0)
        h2 = Act(v, _store(v, e), mag)
        w6, b6 = self.sd[hp + "6.weight"], self.sd[hp + "6.bias"]
        l = _convt64(h2.v, w6) + b6[:, None, None]
        both = _absconvt(torch.cat([h2.v.abs(), h2.e]), w6.abs())
        mag = both[:nb] + b6.abs()[:, None, None]
        e = (1 + U16) * both[nb:] + (gamma(64 + 3) + U16) * mag + 4 * U32 * (l.abs() + 1.0)
        return l, e, mag

    def prob(self, h1, branch="probability"):
        """head1 -> probability (ConvT + BN + ReLU, ConvT + sigmoid), compared through the logit: |dp| <= max sigma' E + 2 u32."""
        return self._prob(Act(_d(h1)), branch)

    def _prob(self, h1, branch):
        l, e, mag = self._tail(h1, branch)
        p = torch.sigmoid(l)
        nearest = torch.where(l.abs() <= e, torch.zeros_like(l), l.abs() - e)   # |xi| closest to 0 within the interval
        dmax = torch.sigmoid(nearest) * torch.sigmoid(-nearest)
        dref = p * (1 - p)
        return StageOut(p, dmax * e + 2 * U32, dref * mag + 2 * U32)

    def threshold(self, p2, branch="threshold"):
        """p2 -> threshold map (unfused graph; its head1 is never tapped)."""
        return self._prob(self._head1(Act(_d(p2)), branch), branch)

    def threshold_composed(self, c2, c3, c4, c5, branch="threshold"):
        """{c2..c5} -> threshold map through the composed entry."""
        return self._prob(self._head1_composed(c2, c3, c4, c5, branch), branch)


# ---- the checker ----
def _p999(z):
    if z.size == 0:
        return 0.0
    k = min(z.size - 1, int(math.ceil(0.999 * z.size)) - 1)
    return float(np.partition(z, k)[k])


def check_stage(got, ref, bound, mag, regions_=None, t_stage=None, name="", hard=True, frames=None):
    """Hard check: |got - ref| <= bound everywhere (the failure names the worst element, its region and the ratio).
    Sharpness check: per region, the 99.9th percentile of z = |got - ref| / mag is <= t_stage.
    Returns {'usage': max |d| / bound, 'z': {region: p99.9}, 'worst': (frame, channel, y, x), 'ok': bool}."""
    got = np.asarray(got, np.float64)
    ref = ref.numpy() if torch.is_tensor(ref) else np.asarray(ref, np.float64)
    bound = bound.numpy() if torch.is_tensor(bound) else np.asarray(bound, np.float64)
    mag = mag.numpy() if torch.is_tensor(mag) else np.asarray(mag, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    regions_ = regions(got.shape) if regions_ is None else regions_
    d = np.abs(got - ref)
    d[np.isnan(got)] = np.inf
    ratio = d / np.maximum(bound, 1e-300)
    worst = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    usage = float(ratio[worst])
    where = [r for r, m in regions_.items() if m[worst[0], 0, worst[2], worst[3]]]
    z = d / np.maximum(mag, 2.0 ** -24)
    zs = {}
    for r, m in regions_.items():
        zs[r] = _p999(z[np.broadcast_to(m, z.shape)])
    worst_frame = int(worst[0]) if frames is None else int(list(frames)[worst[0]])
    stats = {"usage": usage, "z": zs, "worst": (worst_frame,) + tuple(int(i) for i in worst[1:])}
    msgs = []
    if hard and not usage <= 1.0:
        msgs.append(f"{name}: |got-ref| exceeds the bound at (frame, channel, y, x) = {stats['worst']} ({','.join(where) or '-'}): "
                    f"got {got[worst]:.6g} ref {ref[worst]:.6g} bound {bound[worst]:.3g} ratio {usage:.3g}")
    if t_stage is not None:
        bad = {r: v for r, v in zs.items() if v > t_stage}
        if bad:
            msgs.append(f"{name}: z p99.9 above T_stage={t_stage:.3g} in " + ", ".join(f"{r} {v:.3g}" for r, v in bad.items()))
    stats["ok"] = not msgs
    stats["msg"] = "; ".join(msgs)
    return stats


def assert_stage(got, ref_out, t_stage=None, name="", regions_=None, frames=None):
    st = check_stage(got, ref_out.value, ref_out.bound, ref_out.mag, regions_, t_stage, name, frames=frames)
    assert st["ok"], st["msg"]
    return st
