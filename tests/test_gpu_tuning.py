"""Deterministic kernel selection (include/vtd.h: vtd_*_set_tuning): with the shipped table two engines built in separate
processes pick the same kernels and produce bit-identical probability maps / logits; a table entry really steers the
launch; invalid entries are ignored."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from vtd_amd import nets as mynets
from vtd_amd._fixtures import synth, weights

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import hashlib, json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import numpy as np, torch
from vtd_amd import nets as mynets
from vtd_amd._fixtures import synth, weights
from vtd_amd.engine import DetectorEngine, DeviceFrames, RecognizerEngine
sd = mynets.seeded_state_dict(lambda: mynets.DBNet("resnet18"), seed=5)
eng = DetectorEngine("resnet18", sd, max_batch=4)
frames = np.stack([synth.text_frame(60 + i)[0] for i in range(3)])
prob = eng.forward(DeviceFrames(frames))["probability"].cpu().numpy()
rec = RecognizerEngine(97, weights.calibrated_crnn_state_dict(11), max_crops=8)
logits = rec.forward_logits(torch.from_numpy(synth.glyph_batch(21, 8))).cpu().numpy()
print(json.dumps({"prob": hashlib.sha256(prob.tobytes()).hexdigest(), "logits": hashlib.sha256(logits.tobytes()).hexdigest(),
                  "det_tuning": eng.tuning(), "rec_tuning": rec.tuning(),
                  "measured": [eng.tuning_measured, rec.tuning_measured]}))
"""


def _child():
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(ROOT, "video-text-detection-system_amd"), ROOT],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_two_processes_same_kernels_bit_identical_outputs(hip):
    from vtd_amd.engine import shipped_tuning_text
    assert shipped_tuning_text(), "the package ships a kernel-selection table (vtd_amd/tuning/gfx950.txt)"
    a, b = _child(), _child()
    assert a["det_tuning"] == b["det_tuning"] and a["rec_tuning"] == b["rec_tuning"]
    assert a["prob"] == b["prob"] and a["logits"] == b["logits"]
    # the shipped table covers these shapes: nothing was decided by a timing contest in either process
    assert a["measured"] == [False, False] and b["measured"] == [False, False]


def test_table_entries_steer_the_launch_and_invalid_ones_are_ignored(hip, monkeypatch):
    from vtd_amd.engine import DetectorEngine
    sd = mynets.seeded_state_dict(lambda: mynets.DBNet("resnet18"), seed=5)
    x = torch.randn(2, 3, 640, 640, generator=torch.Generator().manual_seed(0))
    monkeypatch.setenv("VTD_TUNING", "0")     # start from an empty table: every entry below is one of this engine's own slots
    eng = DetectorEngine("resnet18", sd, max_batch=2)
    try:
        assert eng.tuning() == {}
        ref = eng.forward(x)["probability"].cpu().numpy()
        table = eng.tuning()
        assert eng.tuning_measured
        keys = [k for k in table if k.endswith("|n2")]
        assert len(keys) >= 15 and len(keys) == len(table)
        # move every implicit-GEMM slot of this bucket to another valid tile shape: the table reports the new ids, the launch
        # descriptions name the forced tile (the entry was honoured), outputs stay within the fp16 tolerance (the tile shapes
        # share one K walk, so they may even agree bit for bit)
        from vtd_amd.engine import detector_profile
        forced = {k: (5 if table[k] != 5 else 6) for k in keys if table[k] < 8 or 12 <= table[k] <= 16}   # implicit-GEMM tile ids
        assert len(forced) >= 8
        eng.set_tuning("".join(f"{k} {v}\n" for k, v in forced.items()) + "# a comment line\nconv|bogus|n2 3\n")
        out = eng.forward(x)["probability"].cpu().numpy()
        now = eng.tuning()
        assert all(now[k] == v for k, v in forced.items())
        names = [row[0] for row in detector_profile(eng)]
        assert sum("conv_igemm<128,64,s2>" in nm or "conv_igemm<128,64,s3>" in nm for nm in names) >= len(forced)
        assert float(np.abs(out - ref).max()) <= 2e-3
        # an id that is not valid for the slot is ignored: the contest decides and overwrites it
        bad_key = keys[0]
        eng.set_tuning(f"{bad_key} 77\n")
        eng.forward(x)
        assert eng.tuning()[bad_key] != 77
        assert eng.lib.vtd_detector_set_tuning(eng.handle, b"no value here\n") != 0
    finally:
        eng.close()


def test_profile_labels_and_border_slot_follow_the_candidate_table(hip):
    """One ResNet-18 forward on the shipped table: every launch slot the table gives to a kernel candidate (id >= 100) is
    labelled with the name the candidate table (csrc/conv_select.cpp) holds for that id, and the BORDER slot runs if and only if
    the head-entry slot before it took a row that leaves the border classes to it.  A label carries M/img, N and K of its slot,
    a table key ho x wo, cout and K: slots are matched to entries on these three."""
    import ctypes
    import re
    from test_conv_candidates import candidate_rows
    from vtd_amd import _native
    from vtd_amd.engine import DetectorEngine, detector_profile
    rows = candidate_rows(ctypes.CDLL(_native.LIB_PATH))
    name_of = {r[0]: r[3] for r in rows}
    id_of = {r[3]: r[0] for r in rows}
    border_ids = {r[0] for r in rows if r[1]}
    eng = DetectorEngine("resnet18", mynets.seeded_state_dict(lambda: mynets.DBNet("resnet18"), seed=5), max_batch=1)
    try:
        assert eng.lib.vtd_detector_set_profiling(eng.handle, 1) == 0
        eng.forward(torch.randn(1, 3, 640, 640, generator=torch.Generator().manual_seed(0)))
        table_ids = {}   # (M/img, N, K) -> ids of the table's entries for bucket 1
        for key, cfg in eng.tuning().items():
            m = re.fullmatch(r"conv\|in\d+x\d+x\d+\|out(\d+)x(\d+)\|co(\d+)\|K(\d+)\|.*\|n1", key)
            if m:
                ho, wo, co, K = map(int, m.groups())
                table_ids.setdefault((ho * wo, co, K), set()).add(cfg)
        profile = detector_profile(eng)
        seen, expected, head_entry_id, border_calls = set(), set(), None, None
        for i, (label, _, calls, _) in enumerate(profile):
            if "border classes of the composed head entry" in label:
                border_calls = calls
                prev = profile[i - 1][0].split(" ")[0]
                assert "composed" in profile[i - 1][0]
                head_entry_id = id_of.get(prev)   # None: an implicit-GEMM tile did every class
                continue
            m = re.search(r" M/img=(\d+) N=(\d+) K=(\d+)", label)
            if not m or calls == 0:
                continue
            shape = tuple(map(int, m.groups()))
            expected |= {(shape, name_of.get(cfg, cfg)) for cfg in table_ids.get(shape, ()) if cfg >= 100}
            stem = label.split(" ")[0]
            if stem in id_of:
                seen.add((shape, stem))
        # a slot carries a candidate's name exactly where the table gives that shape to that candidate, and the graph has such slots
        assert seen and seen == expected, (seen, expected)
        assert border_calls is not None
        assert (border_calls > 0) == (head_entry_id in border_ids), (border_calls, head_entry_id)
    finally:
        eng.close()


@pytest.mark.parametrize("backbone,batches,reps", [("resnet18", (32, 5, 16, 1), 16), ("resnet50", (8,), 12)])
def test_asynchronous_kernels_are_bitwise_repeatable_under_load(hip, backbone, batches, reps):
    """Every hot kernel keeps loads in flight across barriers behind counted `s_waitcnt vmcnt(N)` (LDS-DMA rings in stem_pool,
    head_tail, pointwise, conv_igemm, the halo kernels).  A read that is ordered only by luck passes a parity check whenever the
    DMA happens to land first; what exposes it is timing noise.  Run the B = 32 detector graph (the shipped kernel selection) 24
    times on the same batch while the recogniser hammers a second stream, at two batch sizes, and demand identical bits."""
    from vtd_amd.engine import DetectorEngine, DeviceFrames, RecognizerEngine
    sd = weights.margin_detector_state_dict(backbone, 0)
    opts = {k: int(v) for k, v in (kv.split("=") for kv in os.environ.get("VTD_SOAK_OPTIONS", "").split(",") if kv)}  # bisecting aid
    eng = DetectorEngine(backbone, sd, max_batch=max(batches), options=opts or None)
    rec = RecognizerEngine(97, weights.calibrated_crnn_state_dict(11), max_crops=512)
    crops = torch.from_numpy(synth.glyph_batch(5, 272)).cuda()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    try:
        for n in batches:
            frames = DeviceFrames(np.stack([synth.text_frame(300 + i)[0] for i in range(n)]))
            ref, ref_logits = None, None
            for it in range(reps * int(os.environ.get("VTD_SOAK_FACTOR", "1"))):   # tools/gpu_soak.sh raises the factor
                with torch.cuda.stream(side):
                    logits = rec.forward_logits(crops)
                    if it % 3 == 0:
                        logits = rec.forward_logits(crops)   # vary the phase between the two streams
                prob = eng.forward(frames)["probability"]
                torch.cuda.synchronize()
                if ref is None:
                    ref, ref_logits = prob.clone(), logits.clone()
                else:
                    assert torch.equal(prob, ref), f"detector output changed on repetition {it} at batch {n}"
                    assert torch.equal(logits, ref_logits), f"recogniser logits changed on repetition {it}"
    finally:
        eng.close()
        rec.close()
