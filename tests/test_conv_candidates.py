"""The table of convolution kernel candidates (csrc/conv_select.cpp) read through its two internal C helpers: no GPU, no compute calls."""
import ctypes
import os

import pytest

from vtd_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {100: "conv_halo", 101: "conv_halo_c64_persistent", 102: "head_entry_halo", 103: "head_entry_halo256", 104: "conv_halo64",
         105: "head_entry_pair", 106: "pointwise128", 107: "head_entry_half", 108: "conv_halo_small"}


def candidate_rows(lib):
    """[(id, needs_border, force_halo digit or "", name)] in table order."""
    rows, count, index = [], 1, 0
    while index < count:
        cid, border, digit, name = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.create_string_buffer(64)
        count = lib.vtd_conv_candidate_at(index, ctypes.byref(cid), ctypes.byref(border), ctypes.byref(digit), name, len(name))
        assert count > 0, count
        rows.append((cid.value, bool(border.value), chr(digit.value) if digit.value else "", name.value.decode()))
        index += 1
    return rows


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    assert os.path.basename(_native.LIB_PATH) == "libvtd_hip.so"
    return ctypes.CDLL(_native.LIB_PATH)


def test_candidate_table_of_the_product_library(lib):
    rows = candidate_rows(lib)
    ids = [r[0] for r in rows]
    n_igemm = lib.vtd_conv_igemm_config_count()
    assert n_igemm > 0
    assert len(set(ids)) == len(ids)
    assert not [i for i in ids if 0 <= i < n_igemm]
    assert set(ids) == {100, 101, 102, 103, 104, 106, 108}   # 105 / 107 are candidates of the instrumented build only
    assert ids == [102, 103, 106, 100, 101, 104, 108]         # the order the contest tries them in
    assert {r[0] for r in rows if r[1]} == {102, 103}
    assert {r[0]: r[2] for r in rows if r[2]} == {101: "2", 104: "3", 108: "4"}
    assert {r[0]: r[3] for r in rows} == {i: NAMES[i] for i in ids}


def test_candidate_at_refuses_bad_arguments(lib):
    cid, border, digit, name = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.create_string_buffer(64)
    args = (ctypes.byref(cid), ctypes.byref(border), ctypes.byref(digit), name, len(name))
    count = lib.vtd_conv_candidate_at(0, *args)
    assert lib.vtd_conv_candidate_at(-1, *args) < 0 and lib.vtd_conv_candidate_at(count, *args) < 0
    assert lib.vtd_conv_candidate_at(0, None, *args[1:]) < 0 and lib.vtd_conv_candidate_at(0, *args[:3], None, 64) < 0
    assert lib.vtd_conv_candidate_at(0, *args[:4], 0) < 0


def test_every_id_of_the_shipped_table_is_a_known_kernel(lib):
    """A row of vtd_amd/tuning/gfx950.txt that names an id the library does not carry would be ignored and its slot re-contested on
    every start, silently."""
    known = set(range(lib.vtd_conv_igemm_config_count())) | {r[0] for r in candidate_rows(lib)}
    path = os.path.join(ROOT, "video-text-detection-system_amd", "vtd_amd", "tuning", "gfx950.txt")
    lines = [ln for ln in open(path).read().splitlines() if ln.strip() and not ln.startswith("#")]
    assert len(lines) >= 300
    used = {int(ln.split()[-1]) for ln in lines}
    assert used <= known, sorted(used - known)
    assert used & {r[0] for r in candidate_rows(lib)}, "the shipped table uses the special kernels"
