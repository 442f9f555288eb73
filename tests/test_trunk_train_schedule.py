"""The call schedule of the one trunk training node (nets._TrunkFPNHeadTrainFn), without a device: recording fakes stand in for the raw
wrappers of the stem, the blocks, the FPN, the head and the scaled add, the node runs on a hand-built plan at each depth, and the recorded
sequence -- which call, on which block, through which entry family, with which tensors, whether a dx is asked for, the FPN's input mask, the
FPN level of each scaled add -- is compared with the sequence of the per-depth node classes this node replaced, written out below from
their code.  Every parameter carries its position as its value and the fakes hand a parameter's value back as its gradient, so the number
and the order of the returned gradients are checked too."""
import pytest
import torch

from vtd_amd import nets

BB, RB, B64, BN = "vtd_basicblock_train", "vtd_resblock_train", "vtd_block64_train", "vtd_resblock_bn_train"
N, H5, W5 = 2, 3, 2
# (cin, width, stride, extent of the input as a multiple of C5's, learnable tensors) of layer1.0 .. layer4.1
BLOCKS = ((64, 64, 1, 8, 6), (64, 64, 1, 8, 6), (64, 128, 2, 8, 9), (128, 128, 1, 4, 6), (128, 256, 2, 4, 9), (256, 256, 1, 2, 6), (256, 512, 2, 2, 9),
          (512, 512, 1, 1, 6))
TAPS = {"pool": (8, 64), "C2": (8, 64), "C3": (4, 128), "C4": (2, 256), "C5": (1, 512)}


class Recorder:
    def __init__(self, monkeypatch):
        self.events, self.names = [], {}
        for name in ("_stem_forward_raw", "_stem_backward_raw", "_block_forward_raw", "_block_backward_raw", "_fpn_forward_raw", "_fpn_backward_raw",
                     "_head_forward_raw", "_head_backward_raw", "_combine_scaled"):
            monkeypatch.setattr(nets, name, getattr(self, name))

    def new(self, name, shape, dtype=torch.float32):
        t = torch.zeros(shape, dtype=dtype)
        self.names[t.data_ptr()] = name
        return t

    def name(self, t):
        return self.names[t.data_ptr()]

    @staticmethod
    def mark(learn):
        """The block a group of learnable tensors belongs to: parameter values are positions, blocks are told apart by their first tensor."""
        return int(learn[0])

    def _stem_forward_raw(self, tap, geom, eps, learn, stats):
        self.events.append(("stem_fwd", self.name(tap), [int(p) for p in learn]))
        n, H, W = geom
        hp, wp = (H // 2 + 1) // 2, (W // 2 + 1) // 2
        return self.new("pool", (n, hp + 2, wp + 2, 64), torch.float16), self.new("idx", (n, hp, wp, 64), torch.uint8), self.new("sws", (8,), torch.uint8)

    def _stem_backward_raw(self, tap, geom, eps, learn, stats, ws, pool, idx, dpool, dscale):
        self.events.append(("stem_bwd", self.name(tap), self.name(ws), self.name(pool), self.name(idx), self.name(dpool), self.name(dscale)))
        return [p.detach().clone() for p in learn]

    def _block_forward_raw(self, tap, geom, eps, learn, stats, entry="vtd_basicblock_train", bn=None):
        i = self.block_of[self.mark(learn)]
        assert stats == ("stats", i) and len(learn) == BLOCKS[-len(self.block_of):][i][4]
        self.events.append(("block_fwd", i, entry, bn, self.name(tap)))
        n, h, w, cin, width, stride = geom
        out = (self.new(f"y{i}", (n, h // stride + 2, w // stride + 2, width), torch.float16), self.new(f"ws{i}", (8,), torch.uint8))
        return out + (self.new(f"bstats{i}", (3, 2, width)),) if bn is not None else out

    def _block_backward_raw(self, tap, geom, eps, learn, stats, ws, y, dy, dscale, want_dx, entry="vtd_basicblock_train", bn=None):
        i = self.block_of[self.mark(learn)]
        assert stats == ("stats", i) and self.name(ws) == f"ws{i}"
        self.events.append(("block_bwd", i, entry, bn, self.name(tap), self.name(y), self.name(dy), self.name(dscale), bool(want_dx)))
        n, h, w, cin, width, stride = geom
        dx = self.new(f"dx{i}", (n, h, w, cin)) if want_dx else None
        dxs = self.new(f"dxs{i}", (2,)) if want_dx else None
        return [p.detach().clone() for p in learn], dx, dxs

    def _fpn_forward_raw(self, taps, geom, params):
        self.events.append(("fpn_fwd", tuple(self.name(t) for t in taps)))
        n, h5, w5, _ = geom
        return self.new("p2", (n, 8 * h5 + 2, 8 * w5 + 2, 256), torch.float16), self.new("fws", (8,), torch.uint8)

    def _fpn_backward_raw(self, taps, geom, params, ws, dp2, dscale, input_mask=0):
        self.events.append(("fpn_bwd", tuple(self.name(t) for t in taps), self.name(ws), self.name(dp2), self.name(dscale), input_mask))
        grads = [p.detach().clone() for p in params]
        if not input_mask:
            return grads
        n, h5, w5, c5 = geom
        dtaps = [self.new(f"dC{lv + 2}", (n, h5 << (3 - lv), w5 << (3 - lv), c5 >> (3 - lv))) if (input_mask >> lv) & 1 else None for lv in range(4)]
        scales = torch.zeros((4, 2))
        for lv in range(4):
            self.names[scales[lv].data_ptr()] = f"sC{lv + 2}"
        return grads, dtaps, scales

    def _head_forward_raw(self, feats, hw, training, momentum, eps, buffers, params):
        self.events.append(("head_fwd", self.name(feats), bool(training), momentum, eps, buffers))
        n, (H, W) = feats.shape[0], hw
        return self.new("hws", (8,), torch.uint8), self.new("prob", (n, 1, 4 * H, 4 * W)), self.new("thresh", (n, 1, 4 * H, 4 * W)), self.new("hstats", (4, 2, 64))

    def _head_backward_raw(self, feats, hw, training, ws, prob, thresh, params, grad_prob, grad_thresh, want_input):
        self.events.append(("head_bwd", self.name(feats), bool(training), self.name(ws), self.name(prob), self.name(thresh), bool(want_input)))
        n, (H, W) = feats.shape[0], hw
        return [p.detach().clone() for p in params], self.new("dp2", (n, H, W, 256)), self.new("dp2s", (2,))

    def _combine_scaled(self, a, ascale, b, bscale):
        self.events.append(("combine", self.name(a), self.name(ascale), self.name(b), self.name(bscale)))
        return a, self.new("sum" + self.name(a)[2:], (2,))


def _run(monkeypatch, taps, nblocks, entries, stem=False, bn=None):
    """One forward and backward of the node on a plan with the top `nblocks` blocks of ResNet-18: (the recorded events, the parameters)."""
    rec = Recorder(monkeypatch)
    if stem:
        tensors = (rec.new("image", (N, 32 * H5 + 6, 32 * W5 + 6, 4), torch.float16),)
    else:
        tensors = tuple(rec.new(t, (N, TAPS[t][0] * H5 + 2, TAPS[t][0] * W5 + 2, TAPS[t][1]), torch.float16) for t in taps)
    specs = BLOCKS[len(BLOCKS) - nblocks:]
    blocks = tuple(nets._BlockPlan((N, m * H5, m * W5, cin, width, stride), ("stats", i), entries[i], nlearn)
                   for i, (cin, width, stride, m, nlearn) in enumerate(specs))
    plan = nets._TrunkPlan(taps=tensors, geom=(N, H5, W5, 512), head=(True, 0.1, 1e-5, ("hbuffers",)),
                           stem=((N, 32 * H5, 32 * W5), 1e-5, ("sstats",)) if stem else None, blocks=blocks, beps=1e-5, bn=bn)
    count = (3 if stem else 0) + sum(s[4] for s in specs) + 10 + 20
    params = [torch.full((1,), float(i), requires_grad=True) for i in range(count)]
    rec.block_of, at = {}, 3 if stem else 0
    for i, s in enumerate(specs):
        rec.block_of[at] = i
        at += s[4]
    prob, thresh, stats = nets._TrunkFPNHeadTrainFn.apply(plan, *params)
    assert rec.name(prob) == "prob" and rec.name(thresh) == "thresh" and not stats.requires_grad
    torch.autograd.backward([prob, thresh], [torch.ones_like(prob), torch.ones_like(thresh)])
    return rec.events, params


HEAD_FWD = ("head_fwd", "p2", True, 0.1, 1e-5, ("hbuffers",))
HEAD_BWD = ("head_bwd", "p2", True, "hws", "prob", "thresh", True)

CASES = {
    # _FPNHeadTrainFn
    "zero": (dict(taps=("C2", "C3", "C4", "C5"), nblocks=0, entries=()), 30, [
        ("fpn_fwd", ("C2", "C3", "C4", "C5")), HEAD_FWD, HEAD_BWD,
        ("fpn_bwd", ("C2", "C3", "C4", "C5"), "fws", "dp2", "dp2s", 0),
    ]),
    # _Layer4FPNHeadTrainFn
    "layer4": (dict(taps=("C2", "C3", "C4"), nblocks=2, entries=(BB, BB)), 45, [
        ("block_fwd", 0, BB, None, "C4"), ("block_fwd", 1, BB, None, "y0"),
        ("fpn_fwd", ("C2", "C3", "C4", "y1")), HEAD_FWD, HEAD_BWD,
        ("fpn_bwd", ("C2", "C3", "C4", "y1"), "fws", "dp2", "dp2s", 8),
        ("block_bwd", 1, BB, None, "y0", "y1", "dC5", "sC5", True),
        ("block_bwd", 0, BB, None, "C4", "y0", "dx1", "dxs1", False),
    ]),
    # _Layer4BNFPNHeadTrainFn
    "layer4-bn": (dict(taps=("C2", "C3", "C4"), nblocks=2, entries=(BN, BN), bn=(True, 0.1)), 45, [
        ("block_fwd", 0, BN, (True, 0.1), "C4"), ("block_fwd", 1, BN, (True, 0.1), "y0"),
        ("fpn_fwd", ("C2", "C3", "C4", "y1")), HEAD_FWD, HEAD_BWD,
        ("fpn_bwd", ("C2", "C3", "C4", "y1"), "fws", "dp2", "dp2s", 8),
        ("block_bwd", 1, BN, (True, 0.1), "y0", "y1", "dC5", "sC5", True),
        ("block_bwd", 0, BN, (True, 0.1), "C4", "y0", "dx1", "dxs1", False),
    ]),
    # _Layer3Layer4FPNHeadTrainFn
    "layer3": (dict(taps=("C2", "C3"), nblocks=4, entries=(RB,) * 4), 60, [
        ("block_fwd", 0, RB, None, "C3"), ("block_fwd", 1, RB, None, "y0"), ("block_fwd", 2, RB, None, "y1"), ("block_fwd", 3, RB, None, "y2"),
        ("fpn_fwd", ("C2", "C3", "y1", "y3")), HEAD_FWD, HEAD_BWD,
        ("fpn_bwd", ("C2", "C3", "y1", "y3"), "fws", "dp2", "dp2s", 12),
        ("block_bwd", 3, RB, None, "y2", "y3", "dC5", "sC5", True),
        ("block_bwd", 2, RB, None, "y1", "y2", "dx3", "dxs3", True),
        ("combine", "dx2", "dxs2", "dC4", "sC4"),
        ("block_bwd", 1, RB, None, "y0", "y1", "dx2", "sum2", True),
        ("block_bwd", 0, RB, None, "C3", "y0", "dx1", "dxs1", False),
    ]),
    # _Layer2Layer3Layer4FPNHeadTrainFn
    "layer2": (dict(taps=("C2",), nblocks=6, entries=(RB,) * 6), 75, [
        ("block_fwd", 0, RB, None, "C2"), ("block_fwd", 1, RB, None, "y0"), ("block_fwd", 2, RB, None, "y1"), ("block_fwd", 3, RB, None, "y2"),
        ("block_fwd", 4, RB, None, "y3"), ("block_fwd", 5, RB, None, "y4"),
        ("fpn_fwd", ("C2", "y1", "y3", "y5")), HEAD_FWD, HEAD_BWD,
        ("fpn_bwd", ("C2", "y1", "y3", "y5"), "fws", "dp2", "dp2s", 14),
        ("block_bwd", 5, RB, None, "y4", "y5", "dC5", "sC5", True),
        ("block_bwd", 4, RB, None, "y3", "y4", "dx5", "dxs5", True),
        ("combine", "dx4", "dxs4", "dC4", "sC4"),
        ("block_bwd", 3, RB, None, "y2", "y3", "dx4", "sum4", True),
        ("block_bwd", 2, RB, None, "y1", "y2", "dx3", "dxs3", True),
        ("combine", "dx2", "dxs2", "dC3", "sC3"),
        ("block_bwd", 1, RB, None, "y0", "y1", "dx2", "sum2", True),
        ("block_bwd", 0, RB, None, "C2", "y0", "dx1", "dxs1", False),
    ]),
    # _Layer1Layer2Layer3Layer4FPNHeadTrainFn
    "layer1": (dict(taps=("pool",), nblocks=8, entries=(B64, B64) + (RB,) * 6), 87, [
        ("block_fwd", 0, B64, None, "pool"), ("block_fwd", 1, B64, None, "y0"), ("block_fwd", 2, RB, None, "y1"), ("block_fwd", 3, RB, None, "y2"),
        ("block_fwd", 4, RB, None, "y3"), ("block_fwd", 5, RB, None, "y4"), ("block_fwd", 6, RB, None, "y5"), ("block_fwd", 7, RB, None, "y6"),
        ("fpn_fwd", ("y1", "y3", "y5", "y7")), HEAD_FWD, HEAD_BWD,
        ("fpn_bwd", ("y1", "y3", "y5", "y7"), "fws", "dp2", "dp2s", 15),
        ("block_bwd", 7, RB, None, "y6", "y7", "dC5", "sC5", True),
        ("block_bwd", 6, RB, None, "y5", "y6", "dx7", "dxs7", True),
        ("combine", "dx6", "dxs6", "dC4", "sC4"),
        ("block_bwd", 5, RB, None, "y4", "y5", "dx6", "sum6", True),
        ("block_bwd", 4, RB, None, "y3", "y4", "dx5", "dxs5", True),
        ("combine", "dx4", "dxs4", "dC3", "sC3"),
        ("block_bwd", 3, RB, None, "y2", "y3", "dx4", "sum4", True),
        ("block_bwd", 2, RB, None, "y1", "y2", "dx3", "dxs3", True),
        ("combine", "dx2", "dxs2", "dC2", "sC2"),
        ("block_bwd", 1, B64, None, "y0", "y1", "dx2", "sum2", True),
        ("block_bwd", 0, B64, None, "pool", "y0", "dx1", "dxs1", False),
    ]),
    # _StemLayer1Layer2Layer3Layer4FPNHeadTrainFn
    "stem": (dict(taps=(), nblocks=8, entries=(B64, B64) + (RB,) * 6, stem=True), 90, [
        ("stem_fwd", "image", [0, 1, 2]),
        ("block_fwd", 0, B64, None, "pool"), ("block_fwd", 1, B64, None, "y0"), ("block_fwd", 2, RB, None, "y1"), ("block_fwd", 3, RB, None, "y2"),
        ("block_fwd", 4, RB, None, "y3"), ("block_fwd", 5, RB, None, "y4"), ("block_fwd", 6, RB, None, "y5"), ("block_fwd", 7, RB, None, "y6"),
        ("fpn_fwd", ("y1", "y3", "y5", "y7")), HEAD_FWD, HEAD_BWD,
        ("fpn_bwd", ("y1", "y3", "y5", "y7"), "fws", "dp2", "dp2s", 15),
        ("block_bwd", 7, RB, None, "y6", "y7", "dC5", "sC5", True),
        ("block_bwd", 6, RB, None, "y5", "y6", "dx7", "dxs7", True),
        ("combine", "dx6", "dxs6", "dC4", "sC4"),
        ("block_bwd", 5, RB, None, "y4", "y5", "dx6", "sum6", True),
        ("block_bwd", 4, RB, None, "y3", "y4", "dx5", "dxs5", True),
        ("combine", "dx4", "dxs4", "dC3", "sC3"),
        ("block_bwd", 3, RB, None, "y2", "y3", "dx4", "sum4", True),
        ("block_bwd", 2, RB, None, "y1", "y2", "dx3", "dxs3", True),
        ("combine", "dx2", "dxs2", "dC2", "sC2"),
        ("block_bwd", 1, B64, None, "y0", "y1", "dx2", "sum2", True),
        ("block_bwd", 0, B64, None, "pool", "y0", "dx1", "dxs1", True),
        ("stem_bwd", "image", "sws", "pool", "idx", "dx0", "dxs0"),
    ]),
}


@pytest.mark.parametrize("case", list(CASES))
def test_trunk_node_call_schedule(monkeypatch, case):
    kwargs, count, want = CASES[case]
    events, params = _run(monkeypatch, **kwargs)
    assert events == want, "\n".join(f"{'  ' if a == b else '!!'} {a}   |   {b}" for a, b in zip(events + [None] * len(want), want + [None] * len(events)))
    # one gradient per learnable tensor, each at its own position: the stem's, the blocks' from the lowest up, the FPN's ten, the head's twenty
    assert len(params) == count and [None if p.grad is None else float(p.grad) for p in params] == [float(i) for i in range(count)]
