"""GPU parity of the Transformer recogniser, stage by stage, on the edge architectures A, B, C (vtd_amd/trocr_spec.py) with the stress
weights: the encoder tap against the fp64 reference of the encoder computed from the engine's own pixel tap, and the teacher-forced
logits of every step against the fp64 reference of the decoder computed from the engine's own encoder tap (oracle/trocr_bounds.py).
Bound: 3 x the level of the CPU emulation of the engine's fp16 storage points, per region, for the maximum and the 99.9th percentile
of |got - exact| / row RMS.  Every case prints the emulated level, the bound, the GPU's level and the bound usage.

Crop counts: 3 (spec C also 1).  The dense GEMM takes 256 rows or more, and three crops of spec A are 195 token rows, so A's
VTD_DENSE_GEMM=1 cases run at 4 crops (260 rows: a second row tile of four rows) and at 21 / 70 crops."""
import hashlib
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from oracle import trocr_bounds as tb
from vtd_amd import trocr_spec as ts
from vtd_amd._fixtures import weights

pytestmark = pytest.mark.gpu

if os.environ.get("OMP_NUM_THREADS", "").isdigit():
    torch.set_num_threads(int(os.environ["OMP_NUM_THREADS"]))

SPECS = {"A": ts.STAGE_A, "B": ts.STAGE_B, "C": ts.STAGE_C}
SEED = 3
_CACHE = OrderedDict()   # (what, input digest) -> reference: cases with bit-identical inputs share it
_REF = {}


def _stress(name):
    if name not in _REF:
        sd = weights.stress_trocr_state_dict(SPECS[name], SEED)
        _REF[name] = (sd, tb.StageRef(sd, SPECS[name]))
    return _REF[name]


def _cached(key, arrays, fn):
    h = hashlib.sha1(repr(key).encode())
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    k = h.hexdigest()
    if k not in _CACHE:
        _CACHE[k] = fn()
        while len(_CACHE) > 16:
            _CACHE.popitem(last=False)
    _CACHE.move_to_end(k)
    return _CACHE[k]


def _run(name, crops, xattn, dense, monkeypatch, length=None):
    """One engine, one forced decode: (pixel tap, encoder tap, logits of the forced steps, forced ids, the form that ran)."""
    from vtd_amd.engine import TrOCREngine
    spec = SPECS[name]
    sd, _ = _stress(name)
    monkeypatch.setenv("VTD_DENSE_GEMM", str(dense))
    px = weights.stress_trocr_pixels(spec, crops, 1)
    ids = weights.stress_trocr_ids(spec, crops, length or spec.max_length, 1)
    eng = TrOCREngine(spec, sd, max_crops=crops, xattn=bool(xattn))
    try:
        assert eng.xattn == (bool(xattn) and name != "C"), "spec C (320-wide states, 17 heads) keeps the key / value form"
        eng.set_profiling(2)   # brackets the dense-GEMM launches of the encoder pass
        got_ids, logits = eng.generate_pixels(px, forced=ids.numpy(), want_logits=True)
        _, launches, _ = eng.gemm_profile()
        px_tap, enc_tap = eng.read_tap("pixel_values", crops), eng.read_tap("encoder", crops)
        form = int(eng.xattn)
    finally:
        eng.close()
    assert np.array_equal(got_ids.numpy()[:, :ids.shape[1]], ids.numpy())
    assert np.array_equal(px_tap, px.numpy()), "the pixel values are fp16-representable: the tap returns them"
    if dense:
        want = 1 + 4 * spec.enc_layers + (0 if form else 2 * spec.dec_layers)
        assert launches == want, f"dense_gemm_kernel launches of the encoder pass: {launches}, expected {want}"
    else:
        assert launches == 0
    return px_tap, enc_tap, logits.numpy()[:, :ids.shape[1] - 1].astype(np.float64), ids, form


def _check_stages(name, what, px_tap, enc_tap, logits, ids, form, rows=None):
    _, ref = _stress(name)
    exact = _cached((name, "enc", 0), [px_tap], lambda: ref.encoder(px_tap))
    stored = _cached((name, "enc", 1), [px_tap], lambda: ref.encoder(px_tap, stored=True))
    assert np.isfinite(enc_tap).all() and np.isfinite(logits).all()
    e = tb.assert_stage(enc_tap, exact, stored, tb.encoder_regions(exact.shape[1]), f"{what} encoder")
    lex = _cached((name, "dec", 0), [enc_tap, ids.numpy()], lambda: ref.decoder(enc_tap, ids))
    lst = _cached((name, "dec", 1, form), [enc_tap, ids.numpy()], lambda: ref.decoder(enc_tap, ids, stored=True, form=form))
    d = tb.assert_stage(logits, lex, lst, tb.decoder_regions(lex.shape[1]), f"{what} decoder", rows)
    return e, d, (lex, lst)


CASES = [("A", 3, 1, 0), ("A", 3, 0, 0), ("A", 4, 1, 1), ("A", 4, 0, 1),
         ("B", 3, 1, 0), ("B", 3, 0, 0), ("B", 3, 1, 1), ("B", 3, 0, 1),
         ("C", 3, 1, 0), ("C", 3, 1, 1), ("C", 1, 1, 0), ("C", 1, 1, 1)]


@pytest.mark.parametrize("name,crops,xattn,dense", CASES, ids=[f"{n}-{c}crops-xattn{x}-dense{d}" for n, c, x, d in CASES])
def test_stages_against_fp64_references(hip, monkeypatch, name, crops, xattn, dense):
    """Both stages over every step the spec allows (spec C: 79 forced steps, so the self-attention runs over more than 64 keys)."""
    what = f"{name} {crops} crops xattn={xattn} dense={dense}"
    _check_stages(name, what, *_run(name, crops, xattn, dense, monkeypatch))


TALL = [(21, 1, 1), (70, 0, 1), (260, 1, 0)]


@pytest.mark.parametrize("crops,xattn,dense", TALL, ids=[f"A-{c}crops-xattn{x}-dense{d}" for c, x, d in TALL])
def test_tall_live_lists_against_fp64_references(hip, monkeypatch, crops, xattn, dense):
    """dec_gemm's taller tiles against a reference, not against each other: 21 crops (<2,2>: 17-32 rows), 70 (<4,2> with six rows in a
    second 64-row tile), 260 (<4,4> on every projection), four forced steps, on the rows at the tile edges, the last row and a tenth."""
    rows = tb.sample_rows(crops)
    _check_stages("A", f"A {crops} crops xattn={xattn} dense={dense}", *_run("A", crops, xattn, dense, monkeypatch, length=5), rows=rows)


def test_gpu_negative_control_is_rejected(hip, monkeypatch):
    """the logits of crop i against the reference of crop i + 1 must fail, far outside the bound"""
    px_tap, enc_tap, logits, ids, form = _run("A", 3, 1, 0, monkeypatch)
    _, _, (lex, lst) = _check_stages("A", "A 3 crops (control)", px_tap, enc_tap, logits, ids, form)
    st = tb.check(np.roll(logits, 1, axis=0), lex, lst, tb.decoder_regions(lex.shape[1]), "A logits of crop i vs reference of crop i + 1")
    print(tb.report(st))
    assert not st["ok"] and st["usage"] >= 10


COMPACTION = dict(seed=SEED, eos_gain=4.0, project=False, crops=40, pixel_seed=9)   # tests/test_trocr_bounds.py pins it on the CPU


def test_compaction_free_running_equals_padded_decode_and_the_oracle(hip, monkeypatch):
    """40 crops of spec A, free-running: rows end at different steps and the live list shrinks through 32 and 16 rows (three tile
    heights in one decode).  The ids equal the padded decode's bit for bit, and the fp64 oracle's on every crop whose top-2 gap stays
    above twice the decoder bound."""
    from vtd_amd.engine import TrOCREngine
    spec, n = ts.STAGE_A, COMPACTION["crops"]
    sd = weights.stress_trocr_state_dict(spec, COMPACTION["seed"], eos_gain=COMPACTION["eos_gain"], project=COMPACTION["project"])
    px = weights.stress_trocr_pixels(spec, n, COMPACTION["pixel_seed"])
    eng = TrOCREngine(spec, sd, max_crops=n, xattn=True)
    try:
        assert eng.xattn
        monkeypatch.setenv("VTD_TROCR_COMPACT", "1")
        ids_live = eng.generate_pixels(px)[0].numpy()
        steps_live = eng.last_steps
        enc_tap = eng.read_tap("encoder", n)
        monkeypatch.setenv("VTD_TROCR_COMPACT", "0")
        ids_padded = eng.generate_pixels(px)[0].numpy()
    finally:
        eng.close()
    assert np.array_equal(ids_live, ids_padded)
    ref = tb.StageRef(sd, spec)
    ids_ref, ok, finish, worst = tb.compaction_reference(ref, enc_tap)
    want = np.full(ids_live.shape, spec.pad_token_id, dtype=np.int64)
    want[:, :ids_ref.shape[1]] = ids_ref.numpy()
    ended = [int(np.argmax(r[1:] == spec.eos_token_id)) if (r[1:] == spec.eos_token_id).any() else spec.max_length - 1 for r in ids_live]
    live = [sum(e > s for e in ended) for s in range(spec.max_length - 1)]
    print(f"compaction: {steps_live} steps enqueued, rows end at steps {sorted(set(ended))}, live rows after each step {live}, decoder bound "
          f"{worst:.3e}, well-posed crops {int(ok.sum())} / {n}, crops equal to the oracle {int((ids_live == want).all(1).sum())}")
    assert len(set(ended)) >= 3 and min(live) < 16 and any(16 < v <= 32 for v in live)
    assert int(ok.sum()) * 2 >= n
    assert np.array_equal(ids_live[ok.numpy()], want[ok.numpy()])
