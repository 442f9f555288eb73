"""GPU parity, stage by stage: every tap the engine stores is checked against the fp64 reference of its own stage computed
from the engine's own input tap (oracle/stage_bounds.py), with stress weights (calibrated BatchNorm, biases of activation
size, logits over [-4, 4]) on text and random frames.  Hard check: no element outside the propagated error bound.  Sharpness
check: the 99.9th percentile of |got - ref| / magnitude per region (interior, border ring, last partial tile, later frames)
under the stage's T_stage.  Prints per stage and configuration the bound usage and the z percentiles."""
import hashlib
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from oracle import pipeline as opipe
from oracle import stage_bounds as sb
from vtd_amd._fixtures import synth, weights

pytestmark = pytest.mark.gpu

if os.environ.get("OMP_NUM_THREADS", "").isdigit():
    torch.set_num_threads(int(os.environ["OMP_NUM_THREADS"]))

LAYER = {"fuse_fpn_head": 0, "fuse_stem_pool": 0, "head_tail_kernel": 0}
_CACHE = OrderedDict()   # (stage, flags, input digest) -> StageOut: configurations with bit-identical inputs share references
_SD, _REF = {}, {}


def _stress(backbone):
    if backbone not in _SD:
        _SD[backbone] = weights.stress_detector_state_dict(backbone, 5)
        _REF[backbone] = sb.StageRef(_SD[backbone], backbone)
    return _SD[backbone], _REF[backbone]


def _frames(n, seed):
    """Text frames with a random frame at every third position, preprocessed as the product's reference does."""
    out = []
    for i in range(n):
        f = synth.random_frames(seed + i, 1)[0] if i % 3 == 1 else synth.text_frame(seed + i)[0]
        out.append(opipe.preprocess(f))
    return torch.cat(out)


def _cached(key, arrays, fn):
    h = hashlib.sha1(repr(key).encode())
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    k = h.hexdigest()
    if k in _CACHE:
        _CACHE.move_to_end(k)
        return _CACHE[k]
    out = fn()
    _CACHE[k] = out
    while len(_CACHE) > 12:
        _CACHE.popitem(last=False)
    return out


def _run(backbone, n, options=None, seed=700, threshold=True):
    from vtd_amd.engine import DetectorEngine, detector_profile
    sd, _ = _stress(backbone)
    opts = dict(options or {})
    x = _frames(n, seed)
    eng = DetectorEngine(backbone, sd, max_batch=n, options=opts)
    try:
        out = eng.forward(x, want_threshold=threshold)
        taps = {"probability": out["probability"].cpu().numpy()}
        if threshold:
            taps["threshold"] = out["threshold"].cpu().numpy()
        names = ["input", "pool", "c2", "c3", "c4", "c5", "head1"]
        if opts.get("fuse_stem_pool", 1) == 0:
            names.append("stem")
        if opts.get("fuse_fpn_head", 1) == 0:
            names.append("p2")
        for t in names:
            taps[t] = eng.read_tap(t, n)
        kernels = [r[0] for r in detector_profile(eng)]
    finally:
        eng.close()
    return taps, kernels


def _check_all(label, backbone, taps, frames=None, fold_ds=True):
    """Every stage whose taps exist; returns {stage: stats}."""
    _, ref = _stress(backbone)
    n = taps["input"].shape[0]
    frames = list(range(n)) if frames is None else list(frames)
    t = {k: v[frames] for k, v in taps.items()}
    c = [t[f"c{i}"] for i in range(2, 6)]
    jobs = []
    if "stem" in t:
        jobs += [("stem", "stem", [t["input"]], lambda: ref.stem(t["input"])),
                 ("pool", "pool", [t["stem"]], lambda: sb.StageRef.pool(t["stem"]))]
    else:
        jobs.append(("pool", "stem_pool", [t["input"]], lambda: ref.stem_pool(t["input"])))
    prev = "pool"
    for st in range(4):
        name = f"c{st + 2}"
        jobs.append((name, name, [t[prev]], (lambda st=st, prev=prev: ref.layer(st, t[prev], fold_ds))))
        prev = name
    if "p2" in t:
        jobs += [("p2", "p2", c, lambda: ref.p2(*c)),
                 ("head1", "head1", [t["p2"]], lambda: ref.head1(t["p2"]))]
        if "threshold" in t:
            jobs.append(("threshold", "threshold", [t["p2"]], lambda: ref.threshold(t["p2"])))
    else:
        jobs.append(("head1", "head1_composed", c, lambda: ref.head1_composed(*c)))
        if "threshold" in t:
            jobs.append(("threshold", "threshold", c, lambda: ref.threshold_composed(*c)))
    jobs.append(("probability", "probability", [t["head1"]], lambda: ref.prob(t["head1"])))
    stats, failures = {}, []
    for tap, stage, inputs, fn in jobs:
        out = _cached((backbone, stage, fold_ds, frames, n), inputs, fn)
        regs = sb.regions(t[tap].shape, frames, n)
        st = sb.check_stage(t[tap], out.value, out.bound, out.mag, regs, sb.T_STAGE[stage], f"{label} {stage}", frames=frames)
        print(f"[{label}] {stage:15s} bound usage {st['usage']:.3e}  z p99.9 " +
              " ".join(f"{r} {v:.2e}" for r, v in st["z"].items()) + ("" if st["ok"] else "  FAIL"))
        stats[stage] = st
        if not st["ok"]:
            failures.append(st["msg"])
    assert not failures, "\n".join(failures)
    return stats


R18_CONFIGS = [
    ("layer-by-layer", LAYER, {}, None),
    ("defaults", {}, {}, None),
    ("igemm lds-epilogue", {}, {"VTD_HALO_CONV": "0", "VTD_EPI_DIRECT": "0"}, None),
    ("igemm register-epilogue", {}, {"VTD_HALO_CONV": "0", "VTD_EPI_DIRECT": "1"}, None),
    ("halo 1", {"fuse_fpn_head": 0}, {"VTD_FORCE_HALO": "1", "VTD_HALO_CONV": "1"}, ("conv_halo", 7)),
    ("halo 2 duo 0", {"fuse_fpn_head": 0}, {"VTD_FORCE_HALO": "2", "VTD_HALO_CONV": "1", "VTD_C64_DUO": "0"}, ("c64_persistent", 4)),
    ("halo 2 duo 1", {"fuse_fpn_head": 0}, {"VTD_FORCE_HALO": "2", "VTD_HALO_CONV": "1", "VTD_C64_DUO": "1"}, ("c64_persistent", 4)),
    ("halo 3", {"fuse_fpn_head": 0}, {"VTD_FORCE_HALO": "3", "VTD_HALO_CONV": "1"}, ("conv_halo64", 7)),
    ("fuse_downsample 0", {"fuse_downsample": 0}, {"VTD_HALO_CONV": "0"}, None),
    ("fuse_downsample 1", {"fuse_downsample": 1}, {"VTD_HALO_CONV": "0"}, None),
    ("pointwise", {}, {"VTD_FORCE_POINTWISE": "1"}, ("pointwise128", 1)),
] + [(f"classed {c}", {}, {"VTD_FORCE_CLASSED_CFG": str(c)}, (k, 1)) for c, k in
     ((8, "128,64,s2,classed"), (9, "128,64,s3,classed"), (10, "256,64,s2,classed"), (11, "256,64,s3,classed"),
      (102, "head_entry_halo M"), (103, "head_entry_halo256"), (105, "head_entry_pair"), (107, "head_entry_half"))]


@pytest.mark.parametrize("cfg", R18_CONFIGS, ids=[c[0] for c in R18_CONFIGS])
def test_r18_stages(hip, monkeypatch, cfg):
    label, options, env, want = cfg
    if label in ("classed 105", "classed 107") and b"+experimental" not in hip.vtd_version():
        pytest.skip("candidates 105 / 107 (csrc/experimental/) are only in an instrumented build: VTD_LIB_VARIANT=<tag> "
                    "VTD_EXTRA_HIPCC_FLAGS=-DVTD_EXPERIMENTAL_CANDIDATES")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    taps, kernels = _run("resnet18", 3, options)
    if want is not None:
        assert sum(want[0] in k for k in kernels) >= want[1], (want, kernels)
    _check_all(f"r18 {label}", "resnet18", taps, fold_ds=bool(options.get("fuse_downsample", 1)))


@pytest.mark.parametrize("cfg", [("layer-by-layer", LAYER, {}, None), ("defaults", {}, {}, None),
                                 ("classed 102", {}, {"VTD_FORCE_CLASSED_CFG": "102"}, "head_entry_halo"),
                                 ("classed 103", {}, {"VTD_FORCE_CLASSED_CFG": "103"}, "head_entry_halo256")],
                         ids=lambda c: c[0])
def test_r50_stages(hip, monkeypatch, cfg):
    label, options, env, want = cfg
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    taps, kernels = _run("resnet50", 2, options, seed=800)
    if want is not None:
        assert any(want in k for k in kernels), kernels
    _check_all(f"r50 {label}", "resnet50", taps)


def test_r18_production_batch_32(hip):
    """B = 32 with default options: the tuning table's production pick.  Frames 0, 15 and 31."""
    taps, _ = _run("resnet18", 32, None, seed=900, threshold=False)
    _check_all("r18 B=32", "resnet18", taps, frames=(0, 15, 31))


def test_gpu_negative_control_is_rejected(hip):
    """The comparison is not vacuous: the GPU's c3 against a reference built from ANOTHER frame's c2 must fail."""
    _, ref = _stress("resnet18")
    taps, _ = _run("resnet18", 2, LAYER, seed=710, threshold=False)
    wrong = ref.layer(1, taps["c2"][[1, 0]])
    st = sb.check_stage(taps["c3"], wrong.value, wrong.bound, wrong.mag, None, sb.T_STAGE["c3"], "c3 from the other frame's c2")
    print("GPU negative control: usage", st["usage"], "z", st["z"])
    assert not st["ok"]
    assert max(st["z"].values()) >= 10 * sb.T_STAGE["c3"]
