"""The CRNN's stage-isolated fp64 references (oracle/crnn_bounds.py), their checker and the stress fixture, on the CPU.

* weights.stress_crnn_state_dict makes the recurrence matter: the conditions are asserted from the reference alone, on glyph crops;
* the levels of `stored` against `exact` are finite and positive for every stage but `logits` (printed as a table);
* every plausible kernel bug injected into an evaluation is rejected, with a level of at least 3 x the bound it is held to;
* `stored` under another rounding sample (inputs moved by one fp16 ulp at a seeded 1 % of positions, re-referenced) stays under the
  bound drawn from the first sample: the factor 3 has room;
* the chained `exact` evaluation is oracle.nets.crnn_forward in fp64 on the weights rounded the same way.

The stand-in for the GPU's taps is the chain of `stored` evaluations.  Convolution stages run on 3 crops; the LSTM stages on 19 (one
full 16-crop group and a last group of three, so that the group faults are expressible), from fp32 oracle features rounded to fp16."""
import numpy as np
import pytest
import torch

from oracle import crnn_bounds as cb
from oracle import nets as onets
from vtd_amd._fixtures import synth, weights

SEED, CONV_CROPS, LSTM_CROPS = 5, 3, 19
_S = {}


def ref():
    if "ref" not in _S:
        _S["sd"] = weights.stress_crnn_state_dict(SEED)
        _S["ref"] = cb.StageRef(_S["sd"])
    return _S["ref"]


def conv_case():
    """{k: (input tap, Eval)} for k = 1..7 on the stand-in chain"""
    if "conv" not in _S:
        out, x = {}, cb.input_from_tensor(synth.glyph_batch(31, CONV_CROPS))
        for k in range(1, 8):
            out[k] = (x, ref().conv(k, x))
            x = out[k][1].stored
        _S["conv"] = out
    return _S["conv"]


def lstm_case():
    """{layer: (input sequence, stand-in tap, teacher-forced Eval)} on 19 crops"""
    if "lstm" not in _S:
        r = ref()
        with torch.no_grad():
            feat = onets.crnn_cnn(torch.from_numpy(synth.glyph_batch(32, LSTM_CROPS)), {k: v.float() for k, v in _S["sd"].items()})
        seq, out = cb.seq_of(cb.r16(feat.double())), {}
        for layer in range(2):
            tap = r.lstm(layer, seq).stored             # free-running, rounded where the engine rounds: what a correct GPU would hold
            out[layer] = (seq, tap, r.lstm(layer, seq, htap=tap))
            seq = tap
        _S["lstm"] = out
    return _S["lstm"]


def _show(what, table):
    for k, t in table.items():
        print(f"{what:10s} {k[0]:12s} {k[1]:6s} " + "  ".join(f"{v:.3e}" for v in t))


def test_stress_fixture_makes_the_recurrence_matter():
    r = cb.StageRef(weights.stress_crnn_state_dict(SEED))
    r.probe = {}
    n = 8
    logits, taps = r.forward_exact(cb.input_from_tensor(synth.glyph_batch(33, n)))
    flat = lambda key: torch.cat([t.reshape(-1) for t in r.probe[key]])
    for layer in range(2):
        for rev in range(2):
            k = f"{layer}{rev}"
            rec, xs, pre = flat("rec" + k), flat("xs" + k), flat("pre" + k)
            ratio = float(rec.pow(2).mean().sqrt() / xs.pow(2).mean().sqrt())
            sat = float((pre.abs() > 4).double().mean())
            print(f"layer {layer} dir {rev}: RMS(W_hh h) / RMS(xs) = {ratio:.3f}, |pre-activation| > 4: {sat:.3f}, max|xs| = {float(xs.abs().max()):.1f}")
            assert ratio >= 0.5
            assert 0.05 <= sat <= 0.60
            assert float(xs.abs().max()) < 1000
    for name in cb.CONV_TAPS:
        zeros, peak = float((taps[name] == 0).double().mean()), float(taps[name].max())
        print(f"{name}: zeros after ReLU {zeros:.3f}, max {peak:.2f}")
        assert 0.20 <= zeros <= 0.80, name
        assert peak < 10000, name
    h0 = taps["h0"]
    apart = min(float((h0[i] - h0[j]).abs().max()) for i in range(n) for j in range(i))
    print("free-running exact h0: smallest max|difference| between two crops", apart)
    assert apart > 0.5


def test_levels_are_finite_and_positive():
    rows = []
    for k, (x, ev) in conv_case().items():
        rows.append((cb.CONV_TAPS[k - 1], cb.levels(cb.z_of(ev.stored, ev), cb.conv_regions(tuple(ev.exact.shape), k))))
    for layer, (seq, tap, ev) in lstm_case().items():
        rows.append((f"h{layer}", cb.levels(cb.z_of(ev.stored, ev), cb.lstm_regions(LSTM_CROPS))))
    print("stage      region       stat   emulated level (stored against exact)")
    for name, lv in rows:
        for key, v in lv.items():
            print(f"{name:10s} {key[0]:12s} {key[1]:6s} {v:.3e}")
            assert np.isfinite(v) and v > 0, (name, key)
    ev = ref().logits(lstm_case()[1][1])
    assert ev.stored is ev.exact
    print(f"logits     hard bound gamma(515) = {cb.gamma(515):.3e} of the accumulation magnitude (no fp16 inside the stage)")


FAULTS = [("drop_k", "conv2"), ("drop_k", "conv5"), ("drop_k", "cnn"), ("wrap", "conv1"), ("wrap", "conv3"), ("wrap", "conv6"),
          ("pool22", "conv1"), ("pool22", "conv2"), ("pool22", "conv4"), ("pool22", "conv6")]
FAULTS += [(f, f"h{layer}") for f in cb.LSTM_FAULTS for layer in range(2)]


@pytest.mark.parametrize("fault,stage", FAULTS, ids=[f"{f}-{s}" for f, s in FAULTS])
def test_fault_is_rejected(fault, stage):
    if stage.startswith("h"):
        seq, tap, ev = lstm_case()[int(stage[1])]
        bad = ref().lstm(int(stage[1]), seq, htap=tap, fault=fault).stored
        good = cb.check(tap, ev, cb.lstm_regions(LSTM_CROPS), stage)
        st = cb.check(bad, ev, cb.lstm_regions(LSTM_CROPS), f"{stage} {fault}")
    else:
        k = cb.CONV_TAPS.index(stage) + 1
        x, ev = conv_case()[k]
        bad = ref().conv(k, x, fault=fault).stored
        good = cb.check(ev.stored, ev, cb.conv_regions(tuple(ev.exact.shape), k), stage)
        st = cb.check(bad, ev, cb.conv_regions(tuple(ev.exact.shape), k), f"{stage} {fault}")
    assert good["ok"], "the stand-in itself passes"
    print(cb.report(st))
    print(f"fault {fault} in {stage}: level / bound = {st['usage']:.1f}")
    assert not st["ok"]
    assert st["usage"] >= 3, (fault, stage, st["usage"])


def _one_ulp(x, seed):
    """x (fp16 values, fp64) with a seeded 1 % of positions moved one fp16 ulp away from zero"""
    h = x.to(torch.float16).contiguous()
    bits = h.view(torch.int16).clone()
    pick = torch.rand(bits.shape, generator=torch.Generator().manual_seed(seed)) < 0.01
    bits[pick] += 1
    return bits.view(torch.float16).to(torch.float64)


def test_another_rounding_sample_stays_under_the_bound():
    worst = {}
    for k, (x, ev) in conv_case().items():
        ev2 = ref().conv(k, _one_ulp(x, 100 + k))
        reg = cb.conv_regions(tuple(ev.exact.shape), k)
        em, lv = cb.levels(cb.z_of(ev.stored, ev), reg), cb.levels(cb.z_of(ev2.stored, ev2), reg)
        worst[cb.CONV_TAPS[k - 1]] = max(lv[key] / (cb.FACTOR * em[key]) for key in lv)
    for layer, (seq, tap, ev) in lstm_case().items():
        ev2 = ref().lstm(layer, _one_ulp(seq, 200 + layer), htap=tap)
        reg = cb.lstm_regions(LSTM_CROPS)
        em, lv = cb.levels(cb.z_of(ev.stored, ev), reg), cb.levels(cb.z_of(ev2.stored, ev2), reg)
        worst[f"h{layer}"] = max(lv[key] / (cb.FACTOR * em[key]) for key in lv)
    for name, u in worst.items():
        print(f"{name}: another rounding sample uses {u:.3f} of the bound")
        assert u <= 1.0, name


def test_chain_is_crnn_forward_in_fp64():
    r = ref()
    x = cb.input_from_tensor(synth.glyph_batch(34, 2))
    logits, taps = r.forward_exact(x)
    want, feat, layers = onets.crnn_forward(x, r.equivalent_state_dict(), return_layers=True)
    for name, a, b in (("cnn", taps["cnn"], feat), ("h0", taps["h0"], layers[0]), ("h1", taps["h1"], layers[1]), ("logits", logits, want)):
        rel = float((a - b).abs().max() / b.abs().max())
        print(f"{name}: chained exact stages against crnn_forward in fp64, relative {rel:.2e}")
        assert rel < 1e-9, name
