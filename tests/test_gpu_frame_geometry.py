"""GPU parity of the three kernels whose work depends on the incoming frame's size: the Pillow-bilinear pre-process to 640 x 640
(four code paths, csrc/detector_misc.hip) at every size class of tests/test_frame_geometry.py's plan table, and the CRNN crop
(crop_resize_kernel, csrc/recognizer.hip) over a sweep of box sizes and over boxes it must refuse.  Every comparison is bit-exact
against the CPU oracle."""
import ctypes

import numpy as np
import pytest

import test_frame_geometry as geo
from oracle import cstages
from oracle import pipeline as opipe
from vtd_amd import _native
from vtd_amd import nets as mynets
from vtd_amd._fixtures import synth, weights

pytestmark = pytest.mark.gpu

SIZES = list(geo.PLAN) + list(geo.DEGENERATE)
TOO_LARGE = (2400, 3840)


@pytest.fixture(scope="module")
def det(hip):
    from vtd_amd.engine import DetectorEngine
    sd = mynets.seeded_state_dict(lambda: mynets.DBNet("resnet18"), seed=5)
    eng = DetectorEngine("resnet18", sd, max_batch=2)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def plans(hip):
    return geo.bind(ctypes.CDLL(_native.LIB_PATH))


def _preprocess(eng, frames):
    from vtd_amd.engine import DeviceFrames
    with eng.lock:
        eng._set_input(DeviceFrames(frames))
    return eng.read_tap("input", len(frames))


def _reference(frame):
    return opipe.preprocess(frame)[0].numpy().astype(np.float16).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def test_the_sizes_cover_every_dispatch_path():
    paths = [geo.PLAN[s][3] for s in geo.PLAN] + list(geo.DEGENERATE.values())
    assert set(paths) == {geo.FAST5, geo.FAST7, geo.GENERIC_VEC, geo.GENERIC_BYTES}
    assert min(paths.count(p) for p in set(paths)) >= 2


@pytest.mark.parametrize("shape", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_preprocess_bit_exact_per_size_class(det, plans, shape):
    """K1 at one size of every class: the integer resample bit-exact, the normalisation identical after fp16 rounding."""
    H, W = shape
    rc, ksx, ksy, max_rows, path, lds = geo.plan(plans, H, W)
    if shape in geo.PLAN:
        assert (rc, ksx, ksy, max_rows, path) == (0,) + geo.PLAN[shape]
    else:
        assert (rc, ksx, ksy, path) == (0, 3, 3, geo.DEGENERATE[shape])
    assert 0 < lds <= geo.LDS_LIMIT
    frames = synth.random_frames(H + W, 2, H, W)
    frames[1] = synth.text_frame(3, H, W)[0]
    got = _preprocess(det, frames)
    for i in range(2):
        ref = _reference(frames[i])
        assert np.array_equal(_bits(got[i]), _bits(ref)), f"{geo.PATH_NAMES[path]}, frame {i}: max |d| {np.abs(got[i] - ref).max()}"


def test_size_switching_leaves_no_stale_state(det, plans):
    """One handle, sizes in turn: the (H, W) table cache and the launcher's per-kernel LDS attributes carry nothing over, and a refused
    size neither launches nor disturbs what follows."""
    wide = synth.random_frames(11, 1, 1280, 1920)
    tiny = synth.random_frames(12, 1, 2, 3)
    tall = synth.random_frames(13, 1, 1280, 720)
    first = _preprocess(det, wide)
    assert np.array_equal(_bits(first[0]), _bits(_reference(wide[0])))
    assert np.array_equal(_bits(_preprocess(det, tiny)[0]), _bits(_reference(tiny[0])))
    tall_bits = _preprocess(det, tall)
    assert np.array_equal(_bits(tall_bits[0]), _bits(_reference(tall[0])))
    assert np.array_equal(_bits(_preprocess(det, wide)), _bits(first))

    assert geo.plan(plans, *TOO_LARGE)[0] == geo.REFUSED
    with pytest.raises(_native.NativeError, match=r"\(-1010\)"):
        _preprocess(det, np.zeros((1,) + TOO_LARGE + (3,), np.uint8))
    assert np.array_equal(_bits(det.read_tap("input", 1)), _bits(first)), "a refused size writes nothing"
    assert np.array_equal(_bits(_preprocess(det, tall)), _bits(tall_bits))


# ---- CRNN crop

CROP_H, CROP_W = 300, 517     # row stride 1551 bytes: odd
BOX_WIDTHS = (1, 2, 3, 5, 64, 127, 128, 129, 255, 256, 257, 511, 517)
BOX_HEIGHTS = (1, 2, 3, 16, 31, 32, 33, 63, 64, 65, 128, 300)


@pytest.fixture(scope="module")
def rec(hip):
    from vtd_amd.engine import RecognizerEngine
    eng = RecognizerEngine(97, weights.calibrated_crnn_state_dict(11), max_crops=256)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def crop_frames():
    return synth.random_frames(21, 3, CROP_H, CROP_W)


def _sweep_boxes():
    """every width x every height; the corner a box sits in, and its frame, cycle with the box's number"""
    rng = np.random.default_rng(5)
    boxes = []
    for w in BOX_WIDTHS:
        for h in BOX_HEIGHTS:
            k = len(boxes)
            free_x, free_y = CROP_W - w, CROP_H - h
            x1 = (0, free_x, 0, free_x, int(rng.integers(0, free_x + 1)))[k % 5]
            y1 = (0, free_y, free_y, 0, int(rng.integers(0, free_y + 1)))[k % 5]
            boxes.append((k % 3, x1, y1, x1 + w, y1 + h))
    return boxes


def _crops(eng, frames, boxes):
    from vtd_amd.engine import DeviceFrames
    with eng.lock:
        n = eng.load_crops(DeviceFrames(frames), boxes)
    assert n == len(boxes)
    return eng.read_tap("resized", n)


def _expected_crop(frames, box):
    f, x1, y1, x2, y2 = box
    return cstages.cv_resize_linear(frames[f][y1:y2, x1:x2], 128, 32).astype(np.float32)


def test_crop_sweep_bit_exact(rec, crop_frames):
    boxes = _sweep_boxes()
    assert len(boxes) == 156 and len(set(boxes)) == 156
    sizes = {(b[3] - b[1], b[4] - b[2]) for b in boxes}
    assert {(256, 64), (255, 64), (256, 63), (128, 32)} <= sizes      # the 2 x 2 area route, its two near misses, the identity
    assert {b[0] for b in boxes} == {0, 1, 2}
    inner = [b for b in boxes if b[3] - b[1] < CROP_W and b[4] - b[2] < CROP_H]
    for touches in (lambda b: b[1] == 0, lambda b: b[2] == 0, lambda b: b[3] == CROP_W, lambda b: b[4] == CROP_H):
        assert sum(1 for b in inner if touches(b)) >= 20
    got = _crops(rec, crop_frames, boxes)
    for i, box in enumerate(boxes):
        exp = _expected_crop(crop_frames, box)
        if (box[3] - box[1], box[4] - box[2]) == (128, 32):
            assert np.array_equal(exp, crop_frames[box[0]][box[2]:box[4], box[1]:box[3]])
        assert np.array_equal(got[i], exp), (i, box, float(np.abs(got[i] - exp).max()))


def test_crop_refuses_boxes_outside_the_batch(rec, crop_frames):
    """A box that names no frame of the batch, leaves its frame or has no extent gives an all-zero crop (nothing is read for it); the
    boxes around it are served as usual.  The buffer holds non-zero crops before, so the zeros are written, not left over."""
    n_frames = len(crop_frames)
    valid = [(k % 3, 7 * k, 5 * k, 7 * k + 60 + 9 * k, 5 * k + 20 + 3 * k) for k in range(10)]
    invalid = [(n_frames, 10, 10, 138, 42), (n_frames + 5, 10, 10, 138, 42), (-1, 10, 10, 138, 42),
               (0, -1, 10, 127, 42), (1, 10, -1, 138, 31), (2, 400, 10, CROP_W + 1, 42), (0, 10, 280, 138, CROP_H + 1),
               (1, 50, 10, 50, 42), (2, 10, 40, 138, 30)]
    mixed = [b for pair in zip(valid, invalid) for b in pair] + valid[len(invalid):]
    assert len(mixed) == 19 and all(0 <= b[1] < b[3] <= CROP_W and 0 <= b[2] < b[4] <= CROP_H for b in valid)

    before = _crops(rec, crop_frames, (valid * 2)[:len(mixed)])
    assert all(before[i].any() for i in range(len(mixed)))
    got = _crops(rec, crop_frames, mixed)
    for i, box in enumerate(mixed):
        if box in invalid:
            assert not got[i].any(), (i, box)
        else:
            assert np.array_equal(got[i], _expected_crop(crop_frames, box)), (i, box)
