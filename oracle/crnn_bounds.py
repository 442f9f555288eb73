"""Stage-isolated fp64 references of the CRNN recogniser and their error model (TEST INFRASTRUCTURE ONLY, see oracle/__init__.py).
The CRNN's counterpart of oracle/stage_bounds.py and oracle/trocr_bounds.py, built on the restatement in oracle/nets.py.

Ten stages, cut at the engine's taps (vtd_recognizer_read_tap); every stage starts from the GPU's own input tap, so no error builds up:

  conv1        input: the caller's [n,3,32,128] tensor rounded to fp16 (the kernel's `tile[..] = (half_t)v`), or on the crop path the
               `resized` tap as half(float(u8) / 255.0f)                                  output: the `conv1` tap
  conv2..7     input: the previous tap                                                     output: `conv2`..`conv6`, `cnn` (conv7)
  lstm0, lstm1 input: the `cnn` / `h0` tap, and the GPU's own `h0` / `h1` tap for h_{t-1}  output: `h0` / `h1`
  logits       input: the `h1` tap                                                         output: the fp32 logits

Weights as the engine multiplies by them: BatchNorm folded in double as fold_bn / build_conv do and rounded half(float(double(w) *
scale)) -- conv1 included (its (r*3+s)*3+c packing is a layout, not a value) -- with the shift rounded to fp32; W_hh, W_ih and the
classifier weight half(float); b_ih + b_hh added in fp32 (build_recognizer_graph); classifier bias fp32.

Every stage function returns an Eval: `exact` (fp64 throughout), `stored` (the same with a round to fp16 wherever the engine stores or
consumes fp16), `scale` (what the error is measured in) and `bound` (an analytic per-element hard bound, or None):

  conv     stored rounds the output (the pool sits inside the stage: max commutes with the monotone rounding).  scale = |W|*|x| + |b|,
           the accumulation magnitude, as stage_bounds._absconv computes it, max-pooled with the output.  bound = the fp16 store of a
           K-term fp32 accumulation, stage_bounds._store(v, gamma(K + 3) * scale), max-pooled (max is 1-Lipschitz).
  lstm     stored rounds xs (the hoisted GEMM x W_ih^T + b stores fp16) and h_t.  TEACHER-FORCED IN h: at step t the reference takes
           h_{t-1} from the GPU's own output tap -- the exact fp16 value the kernel reads back from LDS -- and carries its own cell state
           in fp64 from c = 0, so every step of every crop and direction is judged on its own and the first wrong step is the one that
           fails; an error in c can only grow linearly (the forget gate is at most 1).  Forward starts at t = 0, reverse at t = 30;
           output = forward units 0-255, then reverse units 256-511.  scale = 1.  Without a tap (htap=None) the stage runs free.
  logits   stored == exact (no fp16 inside): bound = gamma(K + 3) * scale with K = 512 is the whole check.

Metric z = |got - exact| / scale; level = the maximum and the 99.9th percentile of z per region; bound on a level = FACTOR = 3 x the
level of `stored` against `exact`, per stage, region and statistic.  The factor multiplies the EMULATED level, never a GPU measurement;
it covers another sample of the same rounding errors and the fp32 accumulation order.

Regions.  conv: interior, 1-pixel border ring (`cnn`: columns 0 and 30), the rows of the last partial implicit-GEMM tile of the last
crop (stage_bounds.tail_rows on the launch's un-pooled M, mapped to the pooled pixels it finishes; conv1: the last workgroup = the last
pooled row), crops other than crop 0.  lstm: the first processed step of each direction, all other steps, crops 0-15, the crops of the
last 16-crop group, forward units, reverse units.  logits: crop 0, other crops.

``fault=`` makes an evaluation compute a plausible kernel bug (tests/test_crnn_bounds.py: the checker must reject each):
  conv  drop_k (one 32-channel K chunk of one tap), wrap (circular padding), pool22 (a (2,1) pool taken over 2x2 windows; a (2,2) pool
        shifted by one column)
  lstm  whh_chunk (h units 224-255 ignored in W_hh h), gate_order (g and o swapped), rev_start (the reverse direction's first step
        reads xs of t = 0, the forward direction's initial prefetch row), group_clamp (crops >= 16 read xs of crop i - 16), c_carry
        (the crop D - 1 clamp applied to the cell state: every crop of the last group carries crop D - 1's c)"""
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from . import stage_bounds as sb
from .stage_bounds import _absconv, _conv64, _d, _store, gamma, h16

FACTOR = 3.0
T, HID = 31, 256
CONVS = ((0, 1, 1, (2, 2)), (4, 5, 1, (2, 2)), (8, 9, 1, None), (11, 12, 1, (2, 1)), (15, 16, 1, None), (18, 19, 1, (2, 1)), (22, 23, 0, None))
CONV_TAPS = ("conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "cnn")
CONV_FAULTS, LSTM_FAULTS = ("drop_k", "wrap", "pool22"), ("whh_chunk", "gate_order", "rev_start", "group_clamp", "c_carry")

Eval = namedtuple("Eval", "exact stored scale bound")


def r16(x):
    return x.to(torch.float16).to(x.dtype)


def input_from_tensor(x):
    """conv1's input on the tensor path: the caller's fp32 [n,3,32,128] as the kernel converts it"""
    return torch.as_tensor(np.asarray(x)).to(torch.float32).to(torch.float16).to(torch.float64)


def input_from_resized(tap):
    """conv1's input on the crop path: the `resized` tap [n,32,128,3] (uint8 values) as half(float(u8) / 255.0f), NCHW"""
    u8 = torch.as_tensor(np.asarray(tap)).to(torch.float32)
    return (u8 / torch.tensor(255.0, dtype=torch.float32)).to(torch.float16).to(torch.float64).permute(0, 3, 1, 2).contiguous()


def seq_of(tap):
    """[n,512,1,31] (the NCHW view the taps come back in) -> [n,31,512] fp64"""
    return _d(tap)[:, :, 0].transpose(1, 2).contiguous()


class StageRef:
    probe = None   # a dict: the LSTM stage records xs / W_hh h / gate pre-activations into it (tests/test_crnn_bounds.py)

    def __init__(self, state_dict):
        self.sd = {k: _d(v) for k, v in state_dict.items() if not k.endswith("num_batches_tracked")}
        self.convs = []
        for ci, bi, pad, pool in CONVS:
            w = self.sd[f"cnn.{ci}.weight"]
            scale, shift = sb.StageRef.fold(self, f"cnn.{bi}", f"cnn.{ci}.bias", w.shape[0])
            wq = h16(w * scale[:, None, None, None])
            self.convs.append((wq, wq.abs(), shift.to(torch.float32).to(torch.float64), pad, pool))
        self.rnn = {}
        for layer in range(2):
            for rev in (0, 1):
                suf = f"_l{layer}" + ("_reverse" if rev else "")
                f32 = lambda k: self.sd[k + suf].to(torch.float32)
                self.rnn[(layer, rev)] = (h16(self.sd["rnn.weight_ih" + suf]), h16(self.sd["rnn.weight_hh" + suf]),
                                          (f32("rnn.bias_ih") + f32("rnn.bias_hh")).to(torch.float64))
        self.wc = h16(self.sd["classifier.weight"])
        self.bc = self.sd["classifier.bias"].to(torch.float32).to(torch.float64)

    def equivalent_state_dict(self):
        """An fp64 reference-format state dict of the network the stages compute: folded convolutions behind identity BatchNorms, the
        rounded LSTM / classifier weights (oracle.nets.crnn_forward on it is the chained `exact` evaluation)."""
        sd = {}
        for (ci, bi, _, _), (wq, _, shift, _, _) in zip(CONVS, self.convs):
            c = wq.shape[0]
            sd[f"cnn.{ci}.weight"], sd[f"cnn.{ci}.bias"] = wq, shift
            sd[f"cnn.{bi}.weight"], sd[f"cnn.{bi}.bias"] = torch.ones(c, dtype=torch.float64), torch.zeros(c, dtype=torch.float64)
            sd[f"cnn.{bi}.running_mean"] = torch.zeros(c, dtype=torch.float64)
            sd[f"cnn.{bi}.running_var"] = torch.full((c,), 1.0 - 1e-5, dtype=torch.float64)
        for (layer, rev), (wih, whh, b) in self.rnn.items():
            suf = f"_l{layer}" + ("_reverse" if rev else "")
            sd["rnn.weight_ih" + suf], sd["rnn.weight_hh" + suf] = wih, whh
            sd["rnn.bias_ih" + suf], sd["rnn.bias_hh" + suf] = b, torch.zeros_like(b)
        sd["classifier.weight"], sd["classifier.bias"] = self.wc, self.bc
        return sd

    # ------------------------------------------------------------------------------------------------------------ convolutions
    @torch.no_grad()
    def conv(self, k, x, fault=None):
        """stage conv<k>, k = 1..7: x [n,cin,h,w] (fp16 values) -> Eval of the tap behind its ReLU and pool"""
        wq, wabs, shift, pad, pool = self.convs[k - 1]
        x = _d(x)
        wv = wq
        if fault == "drop_k":
            wv = wq.clone()
            wv[:, 32:64, 0, wq.shape[3] - 1] = 0.0
        pre = _conv64(x, wv, 1, pad, circular=fault == "wrap") + shift[:, None, None]
        mag = _absconv(x.abs(), wabs, 1, pad) + shift.abs()[:, None, None]
        kk = wq.shape[1] * wq.shape[2] * wq.shape[3]
        v = pre.clamp_min(0.0)
        bound = _store(v, gamma(kk + 3) * mag)
        if pool is not None:
            if fault == "pool22" and pool == (2, 1):
                v = F.max_pool2d(F.pad(v, (0, 1, 0, 0), mode="replicate"), (2, 2), (2, 1))
            elif fault == "pool22":
                v = F.max_pool2d(v.roll(-1, 3), pool, pool)
            else:
                v = F.max_pool2d(v, pool, pool)
            mag, bound = F.max_pool2d(mag, pool, pool), F.max_pool2d(bound, pool, pool)
        return Eval(v, r16(v), mag, bound)

    # ------------------------------------------------------------------------------------------------------------ LSTM
    def _rec(self, name, t):
        if self.probe is not None:
            self.probe.setdefault(name, []).append(t)

    def _direction(self, layer, rev, xs, hprev_all, stored, fault):
        """one direction: xs [n,T,1024] as the recurrence reads it; hprev_all [n,T,256] (teacher forcing: h_{t-1} of every step) or None"""
        _, whh, _ = self.rnn[(layer, rev)]
        n = xs.shape[0]
        if fault == "group_clamp" and n > 16:
            xs = xs[[i if i < 16 else i - 16 for i in range(n)]]
        rec_all = None
        if hprev_all is not None:
            if fault == "whh_chunk":
                hprev_all = hprev_all.clone()
                hprev_all[..., 224:256] = 0.0
            rec_all = hprev_all @ whh.t()
            self._rec(f"rec{layer}{rev}", rec_all)
        g0 = 16 * ((n - 1) // 16)
        h, c = xs.new_zeros(n, HID), xs.new_zeros(n, HID)
        out = xs.new_zeros(n, T, HID)
        for step in range(T):
            t = T - 1 - step if rev else step
            x_t = xs[:, 0] if (fault == "rev_start" and rev and step == 0) else xs[:, t]
            if rec_all is not None:
                rec = rec_all[:, t]
            else:
                hp = h
                if fault == "whh_chunk":
                    hp = h.clone()
                    hp[:, 224:256] = 0.0
                rec = hp @ whh.t()
                self._rec(f"rec{layer}{rev}", rec)
            pre = x_t + rec
            self._rec(f"pre{layer}{rev}", pre)
            i, f, g, o = pre.chunk(4, dim=1)
            if fault == "gate_order":
                g, o = o, g
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            if fault == "c_carry":
                c = c.clone()
                c[g0:] = c[n - 1]
            h = torch.sigmoid(o) * torch.tanh(c)
            if stored:
                h = r16(h)
            out[:, t] = h
        return out

    @torch.no_grad()
    def lstm(self, layer, x, htap=None, fault=None):
        """stage lstm<layer>: x [n,31,512] (fp16 values: seq_of(`cnn`) or seq_of(`h0`)), htap [n,31,512] the GPU's output of this
        layer (None: free-running) -> Eval of [n,31,512]"""
        x = _d(x)
        outs = {False: [], True: []}
        for rev in (0, 1):
            wih, _, b = self.rnn[(layer, rev)]
            xs = x @ wih.t() + b
            self._rec(f"xs{layer}{rev}", xs)
            hprev = None
            if htap is not None:
                hd = _d(htap)[:, :, rev * HID:(rev + 1) * HID]
                hprev = torch.zeros_like(hd)
                if rev:
                    hprev[:, :-1] = hd[:, 1:]
                else:
                    hprev[:, 1:] = hd[:, :-1]
            for stored in (False, True):
                probe, self.probe = self.probe, (None if stored else self.probe)   # the conditions are pinned on `exact`
                outs[stored].append(self._direction(layer, rev, r16(xs) if stored else xs, hprev, stored, fault))
                self.probe = probe
        exact, stored = torch.cat(outs[False], dim=2), torch.cat(outs[True], dim=2)
        return Eval(exact, stored, torch.ones((), dtype=torch.float64), None)

    # ------------------------------------------------------------------------------------------------------------ classifier
    @torch.no_grad()
    def logits(self, h1):
        """stage logits: h1 [n,31,512] (fp16 values) -> Eval of [n,31,V]; stored is exact, the bound is the fp32 accumulation term"""
        h1 = _d(h1)
        v = h1 @ self.wc.t() + self.bc
        mag = h1.abs() @ self.wc.abs().t() + self.bc.abs()
        return Eval(v, v, mag, gamma(h1.shape[-1] + 3) * mag)

    # ------------------------------------------------------------------------------------------------------------ the chain
    @torch.no_grad()
    def forward_exact(self, x):
        """the `exact` evaluations chained free-running from fp16 input values: (logits, {tap: value})"""
        taps, y = {}, _d(x)
        for k, name in enumerate(CONV_TAPS, 1):
            y = taps[name] = self.conv(k, y).exact
        seq = y[:, :, 0].transpose(1, 2)
        for layer in range(2):
            seq = taps[f"h{layer}"] = self.lstm(layer, seq).exact
        return self.logits(seq).exact, taps


# ---------------------------------------------------------------------------------------------------------------- regions
def conv_regions(shape, k):
    """boolean masks [n,1,h,w] of a conv tap of `shape` (n,c,h,w), stage k"""
    n, _, h, w = shape
    ring = np.zeros((h, w), bool)
    if k == 7:
        ring[:, 0] = ring[:, -1] = True
    else:
        ring[0] = ring[-1] = True
        ring[:, 0] = ring[:, -1] = True
    reg = {"interior": np.broadcast_to(~ring, (n, 1, h, w)), "border": np.broadcast_to(ring, (n, 1, h, w))}
    ph, pw = CONVS[k - 1][3] or (1, 1)
    if k == 1:
        last = w                                                 # crnn_conv1_pool_kernel: one workgroup per pooled row
    else:
        last = -(-sb.tail_rows(n, h * ph, w * pw) // (ph * pw))  # pooled pixels the last partial tile of the un-pooled map finishes
    tail = np.zeros((n, 1, h * w), bool)
    tail[n - 1, 0, h * w - min(last, h * w):] = True
    reg["last_tile"] = tail.reshape(n, 1, h, w)
    if n > 1:
        later = np.zeros((n, 1, h, w), bool)
        later[1:] = True
        reg["crops_1+"] = later
    return reg


def lstm_regions(n):
    """boolean masks [n,31,512] (or broadcastable) of an LSTM layer's output"""
    first = np.zeros((1, T, 2 * HID), bool)
    first[0, 0, :HID] = True
    first[0, T - 1, HID:] = True
    crops = np.arange(n)[:, None, None]
    units = np.arange(2 * HID)[None, None, :]
    full = (n, T, 2 * HID)
    return {"first step": np.broadcast_to(first, full), "other steps": np.broadcast_to(~first, full),
            "crops 0-15": np.broadcast_to(crops < 16, full), "last group": np.broadcast_to(crops >= 16 * ((n - 1) // 16), full),
            "fwd units": np.broadcast_to(units < HID, full), "rev units": np.broadcast_to(units >= HID, full)}


def logit_regions(n, v):
    crops = np.arange(n)[:, None, None]
    reg = {"crop 0": np.broadcast_to(crops == 0, (n, T, v))}
    if n > 1:
        reg["crops 1+"] = np.broadcast_to(crops > 0, (n, T, v))
    return reg


# ---------------------------------------------------------------------------------------------------------------- levels, check
def _np(t):
    return t.numpy() if torch.is_tensor(t) else np.asarray(t, np.float64)


def z_of(got, ev):
    d = np.abs(np.asarray(_np(got), np.float64) - _np(ev.exact))
    d[np.isnan(d)] = np.inf
    return d / np.maximum(_np(ev.scale), 2.0 ** -24)


def levels(z, regions):
    """{(region, 'max' | 'p99.9'): level}"""
    out = {}
    for name, m in regions.items():
        zr = z[np.broadcast_to(m, z.shape)]
        if zr.size:
            out[(name, "max")] = float(zr.max())
            out[(name, "p99.9")] = sb._p999(zr)
    return out


def check(got, ev, regions, what=""):
    """Levels of `got` against FACTOR x the levels of ev.stored (both against ev.exact, in units of ev.scale), and |got - exact|
    against ev.bound where the stage has one.  Returns {'ok', 'usage' (worst level / bound over the table; for `logits` the hard
    bound's usage), 'hard' (max |got - exact| / ev.bound or None), 'table': {key: (emulated level, bound, level, usage)}}."""
    z = z_of(got, ev)
    lv = levels(z, regions)
    hard = None
    if ev.bound is not None:
        hard = float((np.abs(np.asarray(_np(got), np.float64) - _np(ev.exact)) / np.maximum(_np(ev.bound), 1e-300)).max())
    if ev.stored is ev.exact:      # no fp16 inside the stage: the analytic term is the bound
        g = float((_np(ev.bound) / _np(ev.scale)).max())
        table = {k: (0.0, g, v, v / g) for k, v in lv.items()}
    else:
        em = levels(z_of(ev.stored, ev), regions)
        table = {k: (em[k], FACTOR * em[k], v, (v / (FACTOR * em[k]) if em[k] > 0 else (0.0 if v == 0 else math.inf))) for k, v in lv.items()}
    usage = max(t[3] for t in table.values())
    ok = usage <= 1.0 and (hard is None or hard <= 1.0)
    return {"ok": ok, "usage": usage, "hard": hard, "table": table, "what": what}


def report(st):
    lines = [f"{st['what']:34s} {k[0]:12s} {k[1]:6s} emulated {t[0]:.3e}  bound {t[1]:.3e}  level {t[2]:.3e}  usage {t[3]:.3f}"
             for k, t in st["table"].items()]
    if st["hard"] is not None:
        lines.append(f"{st['what']:34s} hard bound usage {st['hard']:.3f}")
    return "\n".join(lines)


def assert_stage(got, ev, regions, what=""):
    st = check(got, ev, regions, what)
    print(report(st))
    assert st["ok"], f"{what}: over its bound (usage {st['usage']:.2f}, hard {st['hard']})\n{report(st)}"
    return st
