"""Frame geometry without a GPU: the Pillow coefficient tables the resample kernels read (pillow_axis, csrc/vtd_api.cpp) against Pillow
itself, and the pre-process launcher's choice of kernel per frame size (vtd_preprocess_path, csrc/detector_misc.hip), both through the
two internal C helpers vtd_preprocess_axis / vtd_preprocess_plan."""
import ctypes
import os

import numpy as np
import pytest
from PIL import Image

from vtd_amd import _native

ERR_ARG, ERR_CAPACITY, REFUSED = -1100, -1107, -1010
LDS_LIMIT = 160 * 1024
FAST5, FAST7, GENERIC_VEC, GENERIC_BYTES = 0, 1, 2, 3   # vtd_preprocess_path's numbering
PATH_NAMES = {FAST5: "fast<5,5>", FAST7: "fast<7,5>", GENERIC_VEC: "generic, 16-byte row loads", GENERIC_BYTES: "generic, byte loads"}

# (H, W) -> (ksx, ksy, max_rows, path): one row per size class of the 640 x 640 pre-process; the GPU file runs
# every row (tests/test_gpu_frame_geometry.py imports this table)
PLAN = {
    (644, 644): (5, 5, 18, FAST5),              # smallest fast size
    (1280, 720): (5, 5, 34, FAST5),             # portrait, narrow W, most rows
    (1280, 1280): (5, 5, 34, FAST5),            # scale exactly 2
    (644, 1284): (7, 5, 18, FAST7),             # smallest 7-tap width
    (1280, 1920): (7, 5, 34, FAST7),            # largest LDS of the fast path
    (641, 1282): (7, 5, 17, GENERIC_BYTES),     # misses the fast path by W % 4 only
    (1281, 1280): (5, 7, 35, GENERIC_VEC),      # misses it by ksy only
    (1280, 2048): (9, 5, 34, GENERIC_VEC),      # W <= 2048 but 9 taps
    (540, 960): (5, 3, 15, GENERIC_VEC),        # down in x, up in y
    (480, 854): (5, 3, 14, GENERIC_BYTES),
    (1920, 1080): (5, 7, 51, GENERIC_BYTES),    # portrait 1080p
    (1440, 2560): (9, 7, 38, GENERIC_VEC),
    (2160, 3840): (13, 9, 58, GENERIC_VEC),     # 157 440 B of LDS
}
# degenerate windows: 3 x 3 taps, the generic kernel in both of its forms
DEGENERATE = {(1, 1): GENERIC_BYTES, (2, 3): GENERIC_BYTES, (16, 16): GENERIC_VEC, (1, 640): GENERIC_VEC, (640, 1): GENERIC_BYTES}
OLD_SIZES = [(720, 1280), (1080, 1920), (480, 640), (640, 640), (333, 517)]   # test_gpu_detector.py::test_preprocess_bit_exact
TOO_LARGE = [(2400, 3840), (2304, 4096), (4320, 7680)]
NAMED = sorted({v for hw in list(PLAN) + list(DEGENERATE) + OLD_SIZES + TOO_LARGE + [(2160, 4096)] for v in hw})


def bind(lib):
    """the two helpers' signatures (they are not in include/vtd.h, so not in the binding table either)"""
    ip = ctypes.POINTER(ctypes.c_int)
    lib.vtd_preprocess_axis.argtypes = [ctypes.c_int, ctypes.c_int, ip, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    lib.vtd_preprocess_plan.argtypes = [ctypes.c_int, ctypes.c_int, ip, ip, ip, ip, ip]
    return lib


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    assert os.path.basename(_native.LIB_PATH) == "libvtd_hip.so"
    return bind(ctypes.CDLL(_native.LIB_PATH))


def axis_tables(lib, in_size, out_size):
    """(bounds [out_size, 2], kk [out_size, ksize]) of pillow_axis(in_size, out_size)"""
    cap = out_size * (2 * (-(-in_size // out_size)) + 3)
    ksize, bounds, kk = ctypes.c_int(), np.full((out_size, 2), -1, np.int32), np.full(cap, -1, np.int32)
    assert lib.vtd_preprocess_axis(in_size, out_size, ctypes.byref(ksize), bounds.ctypes.data, kk.ctypes.data, cap) == 0
    assert 3 <= ksize.value and out_size * ksize.value <= cap
    return bounds, kk[:out_size * ksize.value].reshape(out_size, ksize.value)


def plan(lib, H, W):
    """(return code, ksx, ksy, max_rows, path, lds_bytes)"""
    v = [ctypes.c_int(-7) for _ in range(5)]
    rc = lib.vtd_preprocess_plan(H, W, *(ctypes.byref(x) for x in v))
    return (rc,) + tuple(x.value for x in v)


def resample_rows(img, bounds, kk):
    """One pass of the kernels' integer resample (the header comment of csrc/detector_misc.hip) down axis 0 of a uint8 [n, m] image:
    out[o] = clip8((2^21 + sum_t kk[o, t] * img[bounds[o, 0] + t]) >> 22) over t < bounds[o, 1]."""
    n = img.shape[0]
    xmin, cnt = bounds[:, 0].astype(np.int64), bounds[:, 1]
    assert (xmin >= 0).all() and (cnt >= 1).all() and (xmin + cnt <= n).all() and cnt.max() <= kk.shape[1]
    assert (kk >= 0).all() and (kk.astype(np.int64).sum(1) * 255 + (1 << 21) < 1 << 31).all()   # int32 accumulators hold it
    wide = img.astype(np.int32)
    acc = np.full((len(bounds), img.shape[1]), 1 << 21, np.int32)
    for t in range(kk.shape[1]):
        live = t < cnt
        acc += np.where(live, kk[:, t], 0)[:, None] * wide[np.minimum(xmin + t, n - 1)]
    return np.clip(acc >> 22, 0, 255).astype(np.uint8)


def sweep_sizes(target):
    if target == 640:
        return sorted(set(range(1, 701)) | set(range(700, 4401, 7)) | set(NAMED))
    return sorted(set(range(1, 401)) | {640, 1100, 1280})


@pytest.mark.parametrize("target", [640, 384, 96])
def test_tables_reproduce_pillow_on_each_axis(lib, target):
    """The tables drive a numpy restatement of the kernels' arithmetic; Pillow resizes the same n x target image down its rows and its
    transpose along its columns (the other pass is the identity in both), bit for bit."""
    rng = np.random.default_rng(target)
    for n in sweep_sizes(target):
        img = rng.integers(0, 256, (n, target), dtype=np.uint8)
        img[:, :8] = np.repeat(rng.integers(0, 2, (n, 1), dtype=np.uint8) * 255, 8, axis=1)   # full-swing edges: the clip and the rounding at both ends
        bounds, kk = axis_tables(lib, n, target)
        scale = max(n / target, 1.0)
        assert kk.shape[1] == 2 * int(np.ceil(scale)) + 1
        mine = resample_rows(img, bounds, kk)
        down = np.asarray(Image.fromarray(img).resize((target, target), Image.BILINEAR))
        assert np.array_equal(mine, down), f"vertical {n} -> {target}"
        across = np.asarray(Image.fromarray(np.ascontiguousarray(img.T)).resize((target, target), Image.BILINEAR))
        assert np.array_equal(mine.T, across), f"horizontal {n} -> {target}"


def test_plan_is_pinned_per_size_class(lib):
    for (H, W), want in PLAN.items():
        rc, ksx, ksy, max_rows, path, lds = plan(lib, H, W)
        assert rc == 0 and (ksx, ksy, max_rows, path) == want, (H, W, rc, ksx, ksy, max_rows, PATH_NAMES.get(path))
        assert 0 < lds <= LDS_LIMIT
    for (H, W), want in DEGENERATE.items():
        rc, ksx, ksy, max_rows, path, lds = plan(lib, H, W)
        assert rc == 0 and (ksx, ksy, path) == (3, 3, want), (H, W, rc, ksx, ksy, PATH_NAMES.get(path))
    assert {v[3] for v in PLAN.values()} == set(PATH_NAMES) and set(DEGENERATE.values()) == {GENERIC_VEC, GENERIC_BYTES}
    assert plan(lib, 1280, 1920)[5] == 119856 and plan(lib, 2160, 3840)[5] == 157440
    # the five sizes the suite has always run keep their classes
    assert [plan(lib, H, W)[4] for H, W in OLD_SIZES] == [FAST5, FAST7, GENERIC_VEC, GENERIC_VEC, GENERIC_BYTES]


def test_plan_refuses_what_the_launcher_refuses(lib):
    for H, W in TOO_LARGE:
        rc, ksx, ksy, max_rows, path, lds = plan(lib, H, W)
        assert rc == REFUSED and path == -1, (H, W, rc, path)
    rc, ksx, ksy, max_rows, path, lds = plan(lib, 2160, 4096)    # DCI 4K still fits
    assert (rc, path, lds) == (0, GENERIC_VEC, 160512)


def test_no_plan_asks_for_more_lds_than_the_kernels_are_granted(lib):
    heights = sorted(set(range(1, 4401, 61)) | set(NAMED))
    widths = sorted(set(range(1, 4401, 13)) | set(NAMED))
    seen = set()
    for H in heights:
        for W in widths:
            rc, ksx, ksy, max_rows, path, lds = plan(lib, H, W)
            assert rc in (0, REFUSED), (H, W, rc)
            if rc == 0:
                assert path in PATH_NAMES and 0 < lds <= LDS_LIMIT, (H, W, path, lds)
                if path in (FAST5, FAST7):   # what the fast kernels are written for
                    assert W % 4 == 0 and W <= 2048 and ksy == 5 and ksx == (5 if path == FAST5 else 7), (H, W, ksx, ksy)
                seen.add(path)
            else:
                assert path == -1
                seen.add(rc)
    assert seen == set(PATH_NAMES) | {REFUSED}


def test_helpers_refuse_bad_arguments(lib):
    ksize, bounds, kk = ctypes.c_int(), np.zeros((640, 2), np.int32), np.zeros(640 * 5, np.int32)
    good = (1280, 640, ctypes.byref(ksize), bounds.ctypes.data, kk.ctypes.data, kk.size)
    assert lib.vtd_preprocess_axis(*good) == 0 and ksize.value == 5
    assert lib.vtd_preprocess_axis(0, *good[1:]) == ERR_ARG and lib.vtd_preprocess_axis(-3, *good[1:]) == ERR_ARG
    assert lib.vtd_preprocess_axis(1280, 0, *good[2:]) == ERR_ARG and lib.vtd_preprocess_axis(1 << 20, *good[1:]) == ERR_ARG
    for hole in (2, 3, 4):
        assert lib.vtd_preprocess_axis(*good[:hole], None, *good[hole + 1:]) == ERR_ARG
    kk[:] = -1
    assert lib.vtd_preprocess_axis(*good[:5], kk.size - 1) == ERR_CAPACITY and lib.vtd_preprocess_axis(*good[:5], -1) == ERR_CAPACITY
    assert (kk == -1).all(), "a short buffer is left untouched"

    v = [ctypes.c_int() for _ in range(5)]
    refs = [ctypes.byref(x) for x in v]
    assert lib.vtd_preprocess_plan(720, 1280, *refs) == 0
    for H, W in ((0, 1280), (720, 0), (-1, 1280), (720, -1), (1 << 20, 1280), (720, 1 << 20)):
        assert lib.vtd_preprocess_plan(H, W, *refs) == ERR_ARG, (H, W)
    for hole in range(5):
        assert lib.vtd_preprocess_plan(720, 1280, *refs[:hole], None, *refs[hole + 1:]) == ERR_ARG
