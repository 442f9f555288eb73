"""GPU parity of the CRNN recogniser, stage by stage, with the stress weights (weights.stress_crnn_state_dict): every tap the engine
stores -- conv1..conv6, cnn, h0, h1 -- and the logits against the fp64 reference of its own stage computed from the engine's own input
tap (oracle/crnn_bounds.py).  The LSTM stages are teacher-forced in h: step t of the reference reads h_{t-1} from the GPU's own tap, so
every step of every crop and direction is judged on its own.  Bound: 3 x the level of the CPU emulation of the engine's fp16 storage
points, per stage, region and statistic (maximum and 99.9th percentile of |got - exact| / scale); the convolution stages also against
the analytic per-element bound of an fp32 accumulation stored as fp16, the logits against gamma(515) x the accumulation magnitude alone.
Every case prints stage, region, emulated level, bound, GPU level and usage.

Crop counts 1, 16, 17, 33: one workgroup of the LSTM kernel with one live lane, a full 16-crop group, one crop in a second group, one
in a third; 17 x 31 = 527 and 33 x 31 = 1023 rows leave the last convolution's last tile partial at every tile height.

The recogniser has no profile call.  Under VTD_FORCE_HALO the selection's contest is left to the halo kernels and its result joins the
tuning text: the halo cases confirm from it that conv3's slot (8x32 map, 128 -> 256) holds a halo candidate's id (mode 3: the pinned
one's).  A tile forced through VTD_FORCE_CONV_CFG is taken before the table and leaves no trace in it, so those cases cannot confirm
from here which tile ran: they pin the environment the selection reads, as tests/test_gpu_recognizer.py does, and check whatever ran
against the reference."""
import hashlib
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from oracle import crnn_bounds as cb
from vtd_amd._fixtures import synth, weights

pytestmark = pytest.mark.gpu

if os.environ.get("OMP_NUM_THREADS", "").isdigit():
    torch.set_num_threads(int(os.environ["OMP_NUM_THREADS"]))

SEED, MAX_CROPS = 5, 48
TAPS = cb.CONV_TAPS[:-1] + ("cnn", "h0", "h1")
_CACHE = OrderedDict()   # (stage, input digest) -> Eval: cases with bit-identical inputs share references
_REF = {}


def _stress():
    if not _REF:
        _REF["sd"] = weights.stress_crnn_state_dict(SEED)
        _REF["ref"] = cb.StageRef(_REF["sd"])
    return _REF["sd"], _REF["ref"]


def _cached(key, arrays, fn):
    h = hashlib.sha1(repr(key).encode())
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    k = h.hexdigest()
    if k not in _CACHE:
        _CACHE[k] = fn()
        while len(_CACHE) > 24:
            _CACHE.popitem(last=False)
    _CACHE.move_to_end(k)
    return _CACHE[k]


def _glyphs(seed, n):
    return torch.from_numpy(synth.glyph_batch(seed, n))


def _forward(eng, x=None, frames=None, boxes=None):
    """one forward on `eng`: {"input": conv1's input as the kernel converts it, every tap, "logits"}"""
    if x is not None:
        n = x.shape[0]
        logits = eng.forward_logits(x).cpu().numpy()
        out = {"input": cb.input_from_tensor(x).numpy()}
    else:
        from vtd_amd.engine import DeviceFrames
        n = len(boxes)
        logits = eng.forward_crops(DeviceFrames(frames), boxes).cpu().numpy()
        out = {"resized": eng.read_tap("resized", n)}
        out["input"] = cb.input_from_resized(out["resized"]).numpy()
    out["logits"], out["tuning"] = logits, eng.tuning_text()
    for t in TAPS:
        out[t] = eng.read_tap(t, n)
    return out


def _crop_inputs():
    """two 720x1280 frames and 17 boxes, none reaching outside: glyph crops pasted at their own size, a box ending exactly at the
    frame's right and bottom edge, a box 1 px wide, a box 1 px high and a zero-width box"""
    frames = np.stack([synth.text_frame(7)[0], synth.random_frames(8, 1)[0]])
    boxes = []
    for i in range(13):
        g = synth.glyph_crop(9000 + i)
        f, y, x = i % 2, 20 + 50 * i, 30 + 60 * i
        frames[f, y:y + g.shape[0], x:x + g.shape[1]] = g
        boxes.append((f, x, y, x + g.shape[1], y + g.shape[0]))
    boxes += [(1, 1000, 600, 1280, 720), (1, 5, 5, 6, 700), (0, 640, 100, 1279, 101), (0, 300, 200, 300, 260)]
    assert len(boxes) == 17 and all(0 <= b[1] <= b[3] <= 1280 and 0 <= b[2] <= b[4] <= 720 for b in boxes)
    return frames, boxes


def _run(ncrops, options=None, env=None, path="tensor"):
    """A fresh engine under `env`, one forward of `ncrops` crops, every tap and the logits."""
    from vtd_amd.engine import RecognizerEngine
    sd, _ = _stress()
    with pytest.MonkeyPatch.context() as mp:
        for k, v in (env or {}).items():
            mp.setenv(k, str(v))
        eng = RecognizerEngine(97, sd, max_crops=MAX_CROPS, options=options)
        try:
            if path == "tensor":
                return _forward(eng, x=_glyphs(41, ncrops))
            frames, boxes = _crop_inputs()
            assert len(boxes) == ncrops
            return _forward(eng, frames=frames, boxes=boxes)
        finally:
            eng.close()


def _evals(taps):
    """{stage: (what the GPU holds, Eval, regions)} for the ten stages, references shared through the cache"""
    _, ref = _stress()
    n = taps["logits"].shape[0]
    out, prev = OrderedDict(), taps["input"]
    for k, name in enumerate(cb.CONV_TAPS, 1):
        ev = _cached(("conv", k), [prev], lambda: ref.conv(k, prev))
        out[name] = (taps[name], ev, cb.conv_regions(taps[name].shape, k))
        prev = taps[name]
    seq = cb.seq_of(taps["cnn"])
    for layer in range(2):
        h = cb.seq_of(taps[f"h{layer}"])
        ev = _cached(("lstm", layer), [seq.numpy(), h.numpy()], lambda: ref.lstm(layer, seq, htap=h))
        out[f"h{layer}"] = (h.numpy(), ev, cb.lstm_regions(n))
        seq = h
    ev = _cached(("logits",), [seq.numpy()], lambda: ref.logits(seq))
    out["logits"] = (taps["logits"], ev, cb.logit_regions(n, taps["logits"].shape[2]))
    return out


def _check_all(what, taps):
    """every stage under its bound in every region; prints the whole table before it asserts"""
    stats, bad = {}, []
    for name, (got, ev, reg) in _evals(taps).items():
        assert np.isfinite(got).all(), name
        st = stats[name] = cb.check(got, ev, reg, f"{what} {name}")
        print(cb.report(st))
        if not st["ok"]:
            bad.append(f"{name}: usage {st['usage']:.2f}, hard-bound usage {st['hard']}")
    print(what, "largest usage per stage:", "  ".join(f"{k} {v['usage']:.3f}" for k, v in stats.items()))
    assert not bad, f"{what}: over the bound -- " + "; ".join(bad)
    return stats


@pytest.mark.parametrize("ncrops", [1, 16, 17, 33])
def test_default_graph(hip, ncrops):
    _check_all(f"{ncrops} crops", _run(ncrops))


def test_separate_pools(hip):
    _check_all("17 crops fuse_pools=0", _run(17, options={"fuse_pools": 0}))


@pytest.mark.parametrize("cfg", [0, 1, 3, 5, 12, 13, 14, 15])
def test_forced_implicit_gemm_tiles(hip, cfg):
    _check_all(f"17 crops igemm cfg {cfg}", _run(17, env={"VTD_HALO_CONV": "0", "VTD_FORCE_CONV_CFG": cfg}))


CONV3_SLOT = "conv|in8x32x128|out8x32|co256|"


def _slot_ids(tuning_text, prefix):
    return {int(ln.split()[-1]) for ln in tuning_text.splitlines() if ln.startswith(prefix)}


def _halo_candidates():
    """{id: (VTD_FORCE_HALO digit that pins it or '', name)} of the selection's conv_halo rows (vtd_conv_candidate_at)"""
    import ctypes
    from vtd_amd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    cid, border, digit, name = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.create_string_buffer(64)
    rows, index = {}, 0
    while lib.vtd_conv_candidate_at(index, ctypes.byref(cid), ctypes.byref(border), ctypes.byref(digit), name, len(name)) > 0:
        if name.value.decode().startswith("conv_halo"):
            rows[cid.value] = (chr(digit.value) if digit.value else "", name.value.decode())
        index += 1
    return rows


@pytest.mark.parametrize("mode", [1, 3])
def test_forced_halo_kernels(hip, mode):
    """VTD_FORCE_HALO=1 leaves the contest to the halo kernels alone (whichever of them is fastest takes the slot), 3 pins conv_halo64."""
    from vtd_amd.engine import shipped_tuning_text
    taps = _run(17, env={"VTD_FORCE_HALO": mode})
    halo = _halo_candidates()
    want = set(halo) if mode == 1 else {i for i, (d, _) in halo.items() if d == str(mode)}
    ran, shipped = _slot_ids(taps["tuning"], CONV3_SLOT), _slot_ids(shipped_tuning_text(), CONV3_SLOT)
    print(f"VTD_FORCE_HALO={mode}: candidates {sorted(want)}; conv3 slot ids after the run {sorted(ran)}, in the shipped table {sorted(shipped)}")
    assert want and ran & want and not shipped & set(halo), "a forced halo kernel took conv3's slot in this run"
    _check_all(f"17 crops halo mode {mode}", taps)


def test_crop_path(hip):
    """17 boxes through forward_crops; conv1's input is the `resized` tap.  The zero-width box's resized crop is all zero and its stages
    still match their references."""
    taps = _run(17, path="crops")
    assert not taps["resized"][16].any() and taps["resized"][:16].any(axis=(1, 2, 3)).all()
    _check_all("17 boxes crop path", taps)


def test_stale_state_on_one_engine(hip):
    """5 crops, then 33 other crops, then the first 5 again on the same engine: nothing of the larger batch (LSTM lanes of dead crops,
    tap rows past the batch, the tuned bucket) shows in the third run -- bit for bit the first, and under the stage bounds."""
    from vtd_amd.engine import RecognizerEngine
    sd, _ = _stress()
    eng = RecognizerEngine(97, sd, max_crops=MAX_CROPS)
    try:
        first = _forward(eng, x=_glyphs(43, 5))
        _forward(eng, x=_glyphs(44, 33))
        third = _forward(eng, x=_glyphs(43, 5))
    finally:
        eng.close()
    for name in TAPS + ("logits",):
        assert np.array_equal(first[name], third[name]), name
    _check_all("5 crops after 33", third)


def test_negative_control_is_rejected(hip):
    """the h0 tap of crop i against the reference of crop i + 1 must fail, far outside the bound"""
    got, ev, reg = _evals(_run(17))["h0"]
    st = cb.check(np.roll(got, 1, axis=0), ev, reg, "h0 of crop i vs reference of crop i + 1")
    print(cb.report(st))
    assert not st["ok"] and st["usage"] >= 10
