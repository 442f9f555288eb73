"""The detector's stage-isolated fp64 references (oracle/stage_bounds.py) and their checker, on the CPU.

A stand-in "GPU" output -- the fp64 reference plus simulated fp32 reorder noise, rounded to fp16 -- must pass every stage;
plausible kernel bugs injected into the reference must be rejected with a z signal at least 10x the stage's T_stage."""
import numpy as np
import pytest
import torch

from oracle import nets as onets
from oracle import stage_bounds as sb
from vtd_amd._fixtures import weights

SIZE, N = 96, 2   # input 96^2: C3 is 12x12, so the last partial tile of the last frame is 80 of its 144 pixels


def stand_in(out, seed, k=2304, fp16=True):
    """The reference as a correct kernel would return it: fp32 reorder noise ~ sqrt(K) u32 of the magnitude, then the store."""
    g = torch.Generator().manual_seed(seed)
    noise = torch.randn(out.value.shape, generator=g, dtype=torch.float64) * (np.sqrt(k) * sb.U32) * out.mag
    v = out.value + noise
    return (v.to(torch.float32).to(torch.float16) if fp16 else v.to(torch.float32)).to(torch.float32).numpy()


def _chain(sd, backbone, seed=3):
    """Stand-in taps of a whole forward at SIZE^2, each stage computed from the previous stand-in tap."""
    ref = sb.StageRef(sd, backbone)
    x = weights._stress_batch(seed, N, SIZE).to(torch.float16).float().numpy()
    taps = {"input": x}
    taps["stem"] = stand_in(ref.stem(x), 1, 147)
    taps["pool"] = sb.StageRef.pool(taps["stem"]).value.float().numpy()
    prev = taps["pool"]
    for st in range(4):
        prev = taps[f"c{st + 2}"] = stand_in(ref.layer(st, prev), 10 + st)
    c = [taps[f"c{i}"] for i in range(2, 6)]
    taps["p2"] = stand_in(ref.p2(*c), 20)
    taps["head1"] = stand_in(ref.head1(taps["p2"]), 21)
    return ref, taps


@pytest.fixture(scope="module", params=["resnet18", "resnet50"])
def chain(request):
    sd = weights.stress_detector_state_dict(request.param, 5)
    ref, taps = _chain(sd, request.param)
    return request.param, sd, ref, taps


def test_stress_weights_are_discriminating():
    """Activations O(1) and inside fp16; logits spread over [-4, 4] on text frames (the probability check means something)."""
    for backbone in ("resnet18", "resnet50"):
        sd = weights.stress_detector_state_dict(backbone, 5)
        out = onets.dbnet_forward(weights._stress_batch(11, 2, 256), sd, backbone, want_threshold=True, return_taps=True)
        peak = max(float(t.abs().max()) for t in out["taps"] + [out["p2"]])
        print(backbone, "max |tap|", peak)
        assert peak < 1e3
        for k in ("probability", "threshold"):
            lg = torch.logit(out[k].double().clamp(1e-12, 1 - 1e-12))
            print(backbone, k, "logit range", float(lg.min()), float(lg.max()))
            assert float(lg.min()) <= -4 and float(lg.max()) >= 4


def test_reference_matches_fp32_oracle(chain):
    """The fp64 stage functions compute the same network as oracle/nets.py (up to the fp16 weight rounding)."""
    backbone, sd, ref, taps = chain
    x = torch.from_numpy(taps["input"])
    want = onets.dbnet_forward(x, sd, backbone, return_taps=True)
    got = ref.layer(0, ref.stem_pool(x).value)
    rel = float((got.value - want["taps"][0].double()).abs().max() / want["taps"][0].abs().max())
    print(backbone, "c2 from the input, fp64 stages vs fp32 oracle", rel)
    assert rel < 1e-2
    o = ref.head1_composed(*[taps[f"c{i}"] for i in range(2, 6)])
    u = ref.head1(ref.p2(*[taps[f"c{i}"] for i in range(2, 6)]).value)
    rel = float((o.value - u.value).abs().max() / u.value.abs().max())
    print(backbone, "head1: composed-entry reference vs layer-by-layer reference", rel)
    assert rel < 2e-3


def test_stand_in_passes_every_stage(chain):
    backbone, sd, ref, taps = chain
    c = [taps[f"c{i}"] for i in range(2, 6)]
    checks = [("stem", taps["stem"], ref.stem(taps["input"])),
              ("pool", taps["pool"], sb.StageRef.pool(taps["stem"])),
              ("stem_pool", stand_in(ref.stem_pool(taps["input"]), 2, 147), ref.stem_pool(taps["input"])),
              ("c2", taps["c2"], ref.layer(0, taps["pool"])),
              ("c3", taps["c3"], ref.layer(1, taps["c2"])),
              ("c4", taps["c4"], ref.layer(2, taps["c3"])),
              ("c5", taps["c5"], ref.layer(3, taps["c4"])),
              ("p2", taps["p2"], ref.p2(*c)),
              ("head1", taps["head1"], ref.head1(taps["p2"])),
              ("head1_composed", stand_in(ref.head1_composed(*c), 30, 3904), ref.head1_composed(*c))]
    pr = ref.prob(taps["head1"])
    checks.append(("probability", stand_in(pr, 31, 64, fp16=False), pr))
    th = ref.threshold_composed(*c)
    checks.append(("threshold", stand_in(th, 32, 64, fp16=False), th))
    for name, got, out in checks:
        st = sb.assert_stage(got, out, sb.T_STAGE[name], f"{backbone} {name}")
        print(f"{backbone} {name:15s} bound usage {st['usage']:.3f}  z p99.9 " +
              " ".join(f"{r} {v:.2e}" for r, v in st["z"].items()))
        if name == "pool":
            assert st["usage"] == 0.0 and np.array_equal(got, out.value.numpy())


def _edit(sd, fn):
    sd = {k: v.clone() for k, v in sd.items()}
    fn(sd)
    return sd


def _drop_shift(sd, p="backbone.5.0.bn2"):
    sd[p + ".bias"] = sd[p + ".running_mean"] * sd[p + ".weight"] / torch.sqrt(sd[p + ".running_var"] + 1e-5)


def _roll_stats(sd, p="backbone.5.0.bn2"):
    sd[p + ".running_mean"] = sd[p + ".running_mean"].roll(8)
    sd[p + ".running_var"] = sd[p + ".running_var"].roll(8)


def _convt_class(sd, p="head.probability_head.3.weight"):
    sd[p][:, :, 1, 1] = sd[p][:, :, 0, 0]


LAST = {"resnet18": "conv2", "resnet50": "conv3"}
CONTROLS = [
    ("K chunk of one 3x3 tap dropped", "c3", lambda b: ("drop_k", "backbone.5.1.conv2"), None),
    ("BN shift dropped", "c3", None, _drop_shift),
    ("BN stats rolled by 8 channels", "c3", None, _roll_stats),
    ("border computed with wrap-around", "c3", lambda b: ("wrap", "backbone.5.1.conv2"), None),
    ("last partial tile from the previous frame", "c3", lambda b: ("tail_prev", f"backbone.5.1.{LAST[b]}"), None),
    ("residual from the neighbouring frame", "c3", lambda b: ("res_roll", f"backbone.5.1.{LAST[b]}"), None),
    ("top-down upsample shifted by one pixel", "p2", lambda b: ("up_shift", "fpn.3"), None),
    ("ConvT parity class with another class's weights", "probability", None, _convt_class),
]


def _stage(ref, name, taps):
    c = [taps[f"c{i}"] for i in range(2, 6)]
    return {"c3": lambda: ref.layer(1, taps["c2"]), "p2": lambda: ref.p2(*c),
            "probability": lambda: ref.prob(taps["head1"])}[name]()


@pytest.mark.parametrize("control", CONTROLS, ids=[c[0] for c in CONTROLS])
def test_negative_control_is_rejected(chain, control):
    label, stage, fault, edit = control
    backbone, sd, ref, taps = chain
    bad = sb.StageRef(_edit(sd, edit) if edit else sd, backbone, fault(backbone) if fault else None)
    good_out = _stage(ref, stage, taps)
    got = stand_in(_stage(bad, stage, taps), 40, fp16=stage != "probability")
    t = sb.T_STAGE[stage]
    st = sb.check_stage(got, good_out.value, good_out.bound, good_out.mag, None, t, f"{backbone} {stage}")
    signal = max(st["z"].values())
    print(f"control [{backbone}] {label}: stage {stage} z p99.9 {signal:.3e} / T_stage {t:.1e} = ratio {signal / t:.1f}  "
          f"(hard bound usage {st['usage']:.1f}) per region {st['z']}")
    assert not st["ok"]
    assert signal / t >= 10, (label, signal, t)
