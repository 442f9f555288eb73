"""GPU parity of the Transformer recogniser (TrOCR; include/vtd.h vtd_trocr_*) against the fp32 oracle and the golden
vectors produced by the locally installed transformers classes.

Tensor level on the reduced architecture (every byte of the goldens stored): processor output bit-exact after the shared fp16
rounding, encoder states and teacher-forced logits within tolerances far below the inter-crop variation, with negative
controls.  Token level on the full trocr-base-printed architecture: greedy ids identical to transformers' generate() on the
margin-selected crops; the reference's surface (TransformerRecognizer / TextRecognizer(use_transformer=True) /
VideoTextPipeline() with default arguments) constructs and runs."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import trocr as otrocr
from vtd_amd._fixtures import synth, weights
from vtd_amd.trocr_spec import BASE_PRINTED, TINY

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny(hip):
    from vtd_amd.engine import TrOCREngine
    sd = weights.trocr_state_dict(TINY, seed=3, w_std=0.025, cross_gain=4.0)
    eng = TrOCREngine(TINY, sd, max_crops=16)
    yield eng, sd
    eng.close()


@pytest.fixture(scope="module")
def base(hip):
    from vtd_amd.engine import TrOCREngine
    sd = weights.trocr_state_dict(BASE_PRINTED, seed=0)
    eng = TrOCREngine(BASE_PRINTED, sd, max_crops=16, slots=2)   # (two encoder-output slots: the slot-independence test uses both)
    yield eng, sd
    eng.close()


def _crops_in_frames(crops):
    """Lay crops out inside one 720p frame batch; returns (frames [n,720,1280,3], boxes)."""
    frames = np.zeros((len(crops), 720, 1280, 3), np.uint8)
    boxes = []
    for i, c in enumerate(crops):
        h, w = c.shape[:2]
        y0, x0 = 17 + 3 * i, 29 + 5 * i
        frames[i, y0:y0 + h, x0:x0 + w] = c
        boxes.append((i, x0, y0, x0 + w, y0 + h))
    return frames, boxes


def test_processor_bit_exact(tiny, base):
    """crop -> BGR2RGB -> Pillow bilinear -> /255 -> (x-0.5)/0.5 on the device == the oracle's preprocess, rounded to fp16, for
    up- and down-scaled crops (both target sizes: 96 and 384)."""
    from vtd_amd.engine import DeviceFrames
    rng = np.random.default_rng(5)
    crops = [synth.glyph_crop(800 + i) for i in range(5)] + [rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
                                                             for h, w in ((11, 17), (300, 500), (640, 1100), (96, 96), (1, 40))]
    frames, boxes = _crops_in_frames(crops)
    for eng, spec in ((tiny[0], TINY), (base[0], BASE_PRINTED)):
        with eng.lock:
            n = eng.encode_crops(DeviceFrames(frames), boxes)
        got = eng.read_tap("pixel_values", n)
        for i, c in enumerate(crops):
            want = otrocr.preprocess(c, spec).half().float().numpy()
            assert np.array_equal(got[i], want), (spec.image_size, i)


def test_tiny_encoder_and_teacher_forced_logits(tiny, golden_dir):
    """Reduced architecture vs the transformers golden: encoder last_hidden_state and the logits of every step on the golden's
    own token path (teacher forcing, so one near-tie cannot derail the comparison)."""
    eng, sd = tiny
    g = np.load(os.path.join(golden_dir, "trocr_tiny.npz"))
    x = torch.stack([otrocr.preprocess(synth.glyph_crop(600 + i), TINY) for i in range(12)])
    ids, logits = eng.generate_pixels(x, forced=g["ids"], want_logits=True)
    enc = eng.read_tap("encoder", 12)
    want_enc = g["enc"]
    between = min(float(np.abs(want_enc[i] - want_enc[j]).max()) for i in range(12) for j in range(i))
    err_enc = float(np.abs(enc - want_enc).max())
    print("encoder max abs err", err_enc, "inter-crop variation", between)
    assert err_enc <= 2e-2 and between >= 50 * err_enc
    want = g["logits"]
    steps = want.shape[1]
    live = (g["ids"][:, :-1] != 1) | (np.arange(steps)[None] == 0)
    got = logits.numpy()[:, :steps]
    err = float(np.abs(got - want)[live].max())
    pair = min(float(np.abs(want[i, 0] - want[j, 0]).max()) for i in range(12) for j in range(i))
    print("logit max abs err", err, "inter-crop variation of the first step", pair)
    assert err <= pair / 20
    assert np.array_equal(ids.numpy()[:, :g["ids"].shape[1]], g["ids"])
    # arg-max agrees at every live step whose golden top-2 gap exceeds twice the error bound
    top2 = np.sort(want, axis=2)[..., -2:]
    sure = live & ((top2[..., 1] - top2[..., 0]) >= 2 * pair / 20)
    assert sure.mean() > 0.5 and np.array_equal(got.argmax(2)[sure], want.argmax(2)[sure])


def test_tiny_negative_controls_and_greedy_equals_oracle(tiny, golden_dir):
    eng, sd = tiny
    g = np.load(os.path.join(golden_dir, "trocr_tiny.npz"))
    want = g["logits"]
    pair = min(float(np.abs(want[i, 0] - want[j, 0]).max()) for i in range(12) for j in range(i))
    # a blank image is far outside the tolerance of every golden crop: ignoring the input would be caught
    blank = torch.full((1, 3, 96, 96), -1.0)
    _, lg = eng.generate_pixels(blank, forced=g["ids"][:1], want_logits=True)
    assert float(np.abs(want[:, 0] - lg.numpy()[0, 0]).max(axis=1).min()) > 10 * pair / 20
    # free-running greedy search from crops of resident frames == the oracle's greedy search wherever the oracle's margin allows
    from vtd_amd.engine import DeviceFrames, trim_generated
    crops = [synth.glyph_crop(600 + i) for i in range(12)]
    frames, boxes = _crops_in_frames(crops)
    ids = eng.generate_crops(DeviceFrames(frames), boxes)
    got = trim_generated(ids, TINY)
    checked = 0
    for i, c in enumerate(crops):
        enc = otrocr.encode(otrocr.preprocess(c, TINY).unsqueeze(0), sd, TINY)
        oid, olog = otrocr.generate(enc, sd, TINY)
        top2 = olog[0].topk(2, dim=1).values
        if float((top2[:, 0] - top2[:, 1]).min()) >= 2 * pair / 20:
            assert got[i] == [t for t in oid[0].tolist()], i
            checked += 1
    assert checked >= 6


def test_base_greedy_ids_match_transformers_generate(base, golden_dir):
    """The full trocr-base-printed architecture: token ids identical to VisionEncoderDecoderModel.generate(max_length=50) on
    >= 8 crops (margin-selected: every step's top-2 gap >= 0.015 in fp32), different crops give different sequences, and the
    first-step logits agree to a tolerance 1/5 of the smallest selected gap."""
    from vtd_amd.engine import DeviceFrames, trim_generated
    eng, sd = base
    man = json.load(open(os.path.join(golden_dir, "trocr_manifest.json")))["base"]
    g = np.load(os.path.join(golden_dir, "trocr_base.npz"))
    rows = man["rows"]
    assert len(rows) >= 8
    crops = [synth.glyph_crop(r["seed"]) for r in rows]
    frames, boxes = _crops_in_frames(crops)
    ids = eng.generate_crops(DeviceFrames(frames), boxes)
    got = trim_generated(ids, BASE_PRINTED)
    assert got == [r["ids"] for r in rows]
    assert len({tuple(s) for s in got}) >= 6
    with eng.lock:
        eng.encode_crops(DeviceFrames(frames[:1]), boxes[:1])
        _, lg = eng.generate_current(1, max_length=2, want_logits=True)
    enc = eng.read_tap("encoder", 1)
    err = float(np.abs(lg.numpy()[0, 0] - g["first_logits"]).max())
    print("base first-step logit max abs err", err, "encoder cls err", float(np.abs(enc[0, 0] - g["enc_cls"]).max()))
    assert err <= 0.015 / 5
    assert float(np.abs(enc[0, 0] - g["enc_cls"]).max()) <= 2e-2 and float(np.abs(enc[0, [1, 100, 576]] - g["enc_rows"]).max()) <= 2e-2


def test_transformer_recognizer_surface_and_default_pipeline(base, golden_dir, monkeypatch):
    """text_recognizer.py:39-69,71-84 and pipeliine.py:18-32 / app/tasks/video_processing.py:33-37: the worker's constructor call
    works; recognize() returns the reference's dict with the hard-coded 0.95 confidence; errors degrade to empty text."""
    from vtd_amd.pipeline import VideoTextPipeline
    from vtd_amd.recognizer import TextRecognizer, TransformerRecognizer
    eng, sd = base
    man = json.load(open(os.path.join(golden_dir, "trocr_manifest.json")))["base"]
    # no checkpoint on disk and no opt-in: construction raises, as from_pretrained does offline (text_recognizer.py:40-42) --
    # strings of synthetic weights never reach results by accident
    monkeypatch.delenv("VTD_TROCR_SEEDED", raising=False)
    monkeypatch.delenv("VTD_TROCR_CHECKPOINT", raising=False)
    with pytest.raises(OSError):
        TextRecognizer(use_transformer=True)
    with pytest.raises(OSError):
        VideoTextPipeline(backbone="resnet18")
    assert TransformerRecognizer("seeded:3").synthetic
    monkeypatch.setenv("VTD_TROCR_SEEDED", "0")     # the explicit opt-in benches and tests use
    rec = TextRecognizer(use_transformer=True)
    assert rec.use_transformer and isinstance(rec.model, TransformerRecognizer) and len(rec.vocab) == 97 and rec.model.synthetic
    rec.model.load_state_dict(sd)
    crop = synth.glyph_crop(man["rows"][0]["seed"])
    out = rec.recognize(crop)
    assert out["confidence"] == 0.95 and isinstance(out["text"], str) and out["text"]
    assert rec.model.recognize_ids([crop])[0] == man["rows"][0]["ids"]
    assert rec.recognize(None) == {"text": "", "confidence": 0.0}
    assert rec.recognize_batch([crop, np.zeros((0, 4, 3), np.uint8)])[1] == {"text": "", "confidence": 0.0}
    # the Celery worker's call (use_transformer_ocr=True, confidence_threshold=..., batch_size=...) and the bare default
    monkeypatch.setenv("VTD_BACKBONE", "resnet18")
    pipe = VideoTextPipeline(use_transformer_ocr=True, confidence_threshold=0.5, batch_size=16)
    assert pipe.recognizer.use_transformer
    pipe.detector.model.load_state_dict(weights.margin_detector_state_dict("resnet18", 0))
    pipe.recognizer.model = rec.model           # share the engine that is already built
    frame = synth.text_frame(123)[0]
    res = pipe.process_single_frame(frame)
    assert len(res["detections"]) >= 3 and all(d["recognition_confidence"] == 0.95 for d in res["detections"])
    json.dumps(res)


def test_decode_on_live_rows_only_equals_the_padded_decode_bit_for_bit(base, monkeypatch):
    """generate() drops a row from the decoder's live list once it has emitted </s> (trocr_decode.hip: dec_advance), where the reference
    keeps computing it and pads.  A row's arithmetic does not depend on its position in the list (fixed K order per output, split-K
    chosen from K alone), so the ids of EVERY crop -- well-posed or not -- equal those of the padded decode (VTD_TROCR_COMPACT=0) exactly,
    and the call stops as soon as the longest row is done."""
    from vtd_amd.engine import trim_generated
    eng, sd = base
    px = torch.stack([otrocr.preprocess(synth.glyph_crop(950 + i), BASE_PRINTED) for i in range(14)])
    outs, steps = {}, {}
    for mode in ("1", "0"):
        monkeypatch.setenv("VTD_TROCR_COMPACT", mode)
        ids, _ = eng.generate_pixels(px)
        outs[mode], steps[mode] = ids.numpy().copy(), eng.last_steps
    assert np.array_equal(outs["1"], outs["0"])
    lens = [len(r) for r in trim_generated(torch.from_numpy(outs["1"]), BASE_PRINTED)]
    print("generated lengths", lens, "decoder steps enqueued", steps)
    assert len(set(lens)) >= 3 and min(lens) < max(lens)              # rows really leave the list at different steps
    assert max(lens) - 1 <= steps["1"] <= min(max(lens) + 2, BASE_PRINTED.max_length - 1)   # stops at most two (lagged) steps after the last </s>


def test_decode_is_bitwise_repeatable_and_slots_are_independent(base):
    """Two runs of the same teacher-forced decode give identical logit bits (no atomics, fixed split-K, lagged host row counts never
    decide arithmetic); crops encoded into slot 1 while slot 0 still waits for its decode come out as if run alone."""
    eng, sd = base
    a = torch.stack([otrocr.preprocess(synth.glyph_crop(960 + i), BASE_PRINTED) for i in range(5)])
    b = torch.stack([otrocr.preprocess(synth.glyph_crop(970 + i), BASE_PRINTED) for i in range(3)])
    ids_a, _ = eng.generate_pixels(a)
    ids_b, _ = eng.generate_pixels(b)
    _, lg1 = eng.generate_pixels(a, forced=ids_a.numpy()[:, :6], want_logits=True, max_length=8)
    _, lg2 = eng.generate_pixels(a, forced=ids_a.numpy()[:, :6], want_logits=True, max_length=8)
    assert np.array_equal(lg1.numpy(), lg2.numpy())
    with eng.lock:
        na = eng.encode_pixels(a, slot=0)
        nb = eng.encode_pixels(b, slot=1)          # slot 0 not decoded yet: its keys / values must survive this pass
        got_b, _ = eng.generate_current(nb, slot=1)
        got_a, _ = eng.generate_current(na, slot=0)
    assert np.array_equal(got_a.numpy(), ids_a.numpy()) and np.array_equal(got_b.numpy(), ids_b.numpy())


def test_queued_tickets_share_one_pass_and_equal_the_synchronous_calls(base, monkeypatch):
    """TrOCREngine.submit_crops only queues; finish() runs ONE encoder pass + ONE decode for everything queued (crops of several frame
    batches, of different frame sizes too, staged into one slot).  Three tickets: two small ones that merge (one of them from 1080p
    frames), one larger than max_crops (cut into two passes, the queue flushed to make room) -- every ticket's ids equal
    generate_crops on its own boxes, and with VTD_TROCR_MERGE=0 (every ticket on its own) as well."""
    from vtd_amd.engine import DeviceFrames
    eng, sd = base
    groups = [[synth.glyph_crop(980 + i) for i in range(4)], [synth.glyph_crop(1030 + i) for i in range(5)],
              [synth.glyph_crop(990 + i) for i in range(eng.max_crops + 3)]]
    batches = []
    for gi, crops in enumerate(groups):
        frames, boxes = _crops_in_frames(crops[:8])
        if gi == 1:   # a frame batch of another size in the same pass
            big = np.zeros((frames.shape[0], 1080, 1920, 3), np.uint8)
            big[:, :720, :1280] = frames
            frames = big
        # more crops than frames fit: reuse the first frames' boxes cyclically (same content, same ids)
        boxes = [boxes[i % len(boxes)] for i in range(len(crops))]
        batches.append((DeviceFrames(frames), boxes))
    want = [eng.generate_crops(fr, bx).numpy() for fr, bx in batches]
    for merge in ("1", "0"):
        monkeypatch.setenv("VTD_TROCR_MERGE", merge)
        t0 = eng.submit_crops(*batches[0])
        t1 = eng.submit_crops(*batches[1])
        assert (t0["parts"] is None and t1["parts"] is None) == (merge == "1")     # queued, nothing enqueued yet
        got0 = eng.finish(t0).numpy()                                               # flushes t0 + t1 as one pass of 9 rows
        assert t1["parts"] is not None
        t2 = eng.submit_crops(*batches[2])
        got1 = eng.finish(t1).numpy()
        got2 = eng.finish(t2).numpy()
        for g, w in zip((got0, got1, got2), want):
            assert np.array_equal(g, w)


def test_pipelined_passes_equal_the_synchronous_calls(base, monkeypatch):
    """Passes of queued tickets, each encoder pass with its decode right behind it on the caller's stream, while another stream keeps
    the machine busy.  Driven the way _pipeline_push drives it -- `pipeline_lag` tickets in flight behind the one asked for -- every
    ticket's ids must equal generate_crops on its own boxes, with passes of two tickets (the default) and of four."""
    from vtd_amd.engine import DeviceFrames, TrOCREngine
    eng, sd = base
    assert eng.pipeline_lag == 1
    batches = []
    for gi, n in enumerate((4, 6, 3, 5, 7, 2, 4)):
        frames, boxes = _crops_in_frames([synth.glyph_crop(1100 + 10 * gi + i) for i in range(n)])
        batches.append((DeviceFrames(frames), boxes))
    want = [eng.generate_crops(fr, bx).numpy() for fr, bx in batches]
    side = torch.cuda.Stream()
    noise = torch.randn(2048, 2048, device="cuda")

    def drive(engine):
        tickets, got = [], []
        for k, (fr, bx) in enumerate(batches):
            with torch.cuda.stream(side):          # something else keeps the machine busy
                for _ in range(4):
                    noise.mul_(1.0001)
            tickets.append(engine.submit_crops(fr, bx))
            if k >= engine.pipeline_lag:
                got.append(engine.finish(tickets[k - engine.pipeline_lag]).numpy())
        for t in tickets[len(got):]:
            got.append(engine.finish(t).numpy())
        return got

    for g, w in zip(drive(eng), want):
        assert np.array_equal(g, w)
    monkeypatch.setenv("VTD_TROCR_PASS_TICKETS", "4")
    other = TrOCREngine(BASE_PRINTED, sd, max_crops=32)
    try:
        assert other.pipeline_lag == 3
        for g, w in zip(drive(other), want):
            assert np.array_equal(g, w)
    finally:
        other.close()
    side.synchronize()


def test_pass_taller_than_the_dense_gemms_32_bit_offsets_runs_as_row_blocks(base):
    """dense_gemm.hip addresses its A operand with 32-bit element offsets: at the 3072-wide fc2 input that is 699 k rows = 1211 crops.  A
    recogniser pass of 1300 crops (five tickets' worth; bench.py with VTD_TROCR_PASS_TICKETS >= 5 gets there) must run -- as row blocks
    -- and give every crop the ids it gets in a small pass, instead of failing validation and being swallowed as empty strings (what a
    first 6-ticket run did, at a splendid 662 frames/s)."""
    from vtd_amd.engine import DeviceFrames, TrOCREngine
    eng, sd = base
    crops = [synth.glyph_crop(1300 + i) for i in range(8)]
    frames, boxes = _crops_in_frames(crops)
    dev = DeviceFrames(frames)
    want = eng.generate_crops(dev, boxes).numpy()
    big = TrOCREngine(BASE_PRINTED, sd, max_crops=1304)
    try:
        many = [boxes[i % 8] for i in range(1300)]
        got = big.generate_crops(dev, many).numpy()
    finally:
        big.close()
    for i in range(1300):
        assert np.array_equal(got[i], want[i % 8]), i


def test_dense_gemm_encoder_pass_matches_goldens_and_repeats_bitwise(base, golden_dir, monkeypatch):
    """dense_gemm.hip (256 x 256 tiles, LDS-DMA ring three stages ahead behind counted waits, two wave groups one barrier interval
    apart) forced onto every dense layer of the encoder pass it fits (VTD_DENSE_GEMM=1; by default it takes them from ~80 crops up):
    encoder states and first-step logits against the transformers golden at the implicit-GEMM path's tolerances, greedy ids of the
    margin-selected crops identical, the two GEMM paths within a fraction of that tolerance of each other, and -- a staged-operand
    kernel that reads a buffer one barrier early is wrong only now and then -- eight runs under a concurrent stream bit-identical."""
    from vtd_amd.engine import DeviceFrames, trim_generated
    eng, sd = base
    man = json.load(open(os.path.join(golden_dir, "trocr_manifest.json")))["base"]
    g = np.load(os.path.join(golden_dir, "trocr_base.npz"))
    crops = [synth.glyph_crop(r["seed"]) for r in man["rows"]]
    frames, boxes = _crops_in_frames(crops)
    dev = DeviceFrames(frames)

    def run():
        ids = eng.generate_crops(dev, boxes)
        return trim_generated(ids, BASE_PRINTED), eng.read_tap("encoder", len(crops))

    monkeypatch.setenv("VTD_DENSE_GEMM", "0")
    ids_ig, enc_ig = run()
    monkeypatch.setenv("VTD_DENSE_GEMM", "1")
    ids_dg, enc_dg = run()
    assert ids_dg == [r["ids"] for r in man["rows"]] == ids_ig
    err = float(np.abs(enc_dg[0, 0] - g["enc_cls"]).max())
    between = float(np.abs(enc_dg - enc_ig).max())
    print("dense-GEMM encoder: cls err vs golden", err, "max |dense - implicit|", between)
    assert err <= 2e-2 and float(np.abs(enc_dg[0, [1, 100, 576]] - g["enc_rows"]).max()) <= 2e-2
    assert between <= 1e-2
    # repeatability under load: a second stream keeps the CUs and the memory system busy while the encoder pass runs
    side = torch.cuda.Stream()
    noise = torch.randn(4096, 4096, device="cuda")
    for _ in range(8):
        with torch.cuda.stream(side):
            for _ in range(6):
                noise = noise * 1.0001 + 0.5
        with eng.lock:
            eng.encode_crops(dev, boxes)
        again = eng.read_tap("encoder", len(crops))
        assert np.array_equal(again, enc_dg)
    side.synchronize()
    # The measurement variants of dense_gemm.hip (among them knock-out variants that produce WRONG results) are not in the product
    # library: their switch, once read by an instrumented build only, must leave the product's encoder states untouched.
    for var in ("32", "64", "4"):
        monkeypatch.setenv("VTD_DGM_VARIANT", var)
        with eng.lock:
            eng.encode_crops(dev, boxes)
        assert np.array_equal(eng.read_tap("encoder", len(crops)), enc_dg), var


def test_cross_attention_on_the_encoder_states_equals_the_key_value_form(tiny, base, golden_dir):
    """csrc/trocr_xattn.hip attends over the raw encoder states with a composed query (q_h Wk_h) and projects the attended state
    (Wv_h) afterwards -- algebraically the reference's attention over K = E Wk^T + bk, V = E Wv^T + bv (q . bk is the same for every
    token and leaves the softmax; the probabilities sum to 1, so bv passes through).  Both forms of one checkpoint: teacher-forced
    logits within the tolerance the goldens are held to, identical greedy ids on the margin-selected golden crops, the other form's
    encoder states untouched, bit-repeatable."""
    from vtd_amd.engine import DeviceFrames, TrOCREngine, trim_generated
    g = np.load(os.path.join(golden_dir, "trocr_tiny.npz"))
    want = g["logits"]
    pair = min(float(np.abs(want[i, 0] - want[j, 0]).max()) for i in range(12) for j in range(i))
    for (eng, sd), spec in ((tiny, TINY), (base, BASE_PRINTED)):
        other = TrOCREngine(spec, sd, max_crops=16, xattn=not eng.xattn)
        try:
            assert other.xattn != eng.xattn
            if spec is TINY:
                x = torch.stack([otrocr.preprocess(synth.glyph_crop(600 + i), TINY) for i in range(12)])
                forced = g["ids"]
            else:
                x = torch.stack([otrocr.preprocess(synth.glyph_crop(960 + i), BASE_PRINTED) for i in range(7)])
                forced = eng.generate_pixels(x)[0].numpy()[:, :8]
            ids_a, lg_a = eng.generate_pixels(x, forced=forced, want_logits=True, max_length=forced.shape[1] + 1)
            enc_a = eng.read_tap("encoder", len(x))
            ids_b, lg_b = other.generate_pixels(x, forced=forced, want_logits=True, max_length=forced.shape[1] + 1)
            enc_b = other.read_tap("encoder", len(x))
            assert np.array_equal(enc_a, enc_b)
            steps = forced.shape[1]
            live = (forced[:, :-1] != spec.pad_token_id) | (np.arange(steps - 1)[None] == 0)
            a, b = lg_a.numpy()[:, :steps - 1], lg_b.numpy()[:, :steps - 1]
            err = float(np.abs(a - b)[live].max())
            print(spec.image_size, "logit max abs difference between the two forms", err)
            assert err <= (pair / 20 if spec is TINY else 0.015 / 5)
            _, lg_b2 = other.generate_pixels(x, forced=forced, want_logits=True, max_length=forced.shape[1] + 1)
            assert np.array_equal(lg_b.numpy(), lg_b2.numpy())
            if spec is BASE_PRINTED:
                man = json.load(open(os.path.join(golden_dir, "trocr_manifest.json")))["base"]["rows"]
                frames, boxes = _crops_in_frames([synth.glyph_crop(r["seed"]) for r in man])
                got = trim_generated(other.generate_crops(DeviceFrames(frames), boxes), BASE_PRINTED)
                assert got == [r["ids"] for r in man]
        finally:
            other.close()


def test_passes_on_the_worker_thread_equal_the_synchronous_calls(base, monkeypatch):
    """VTD_TROCR_ASYNC=1: a full pass (two tickets here) goes to the engine's worker thread, which stages, encodes and decodes it while the
    submitting thread carries on; finish() of such a ticket waits for the worker, finish() of a ticket still in the queue flushes it in
    the calling thread.  Five tickets -> two passes on the worker + one leftover: every ticket's ids equal generate_crops on its own boxes;
    discard_queue drops what the worker has not started."""
    from vtd_amd._native import NativeError
    from vtd_amd.engine import DeviceFrames, TrOCREngine
    eng, sd = base
    monkeypatch.setenv("VTD_TROCR_ASYNC", "1")
    monkeypatch.setenv("VTD_TROCR_PASS_TICKETS", "2")
    a = TrOCREngine(BASE_PRINTED, sd, max_crops=16)
    try:
        assert a.async_passes and a.pipeline_lag == 3
        batches = []
        for gi in range(5):
            frames, boxes = _crops_in_frames([synth.glyph_crop(1100 + 7 * gi + i) for i in range(3 + gi % 2)])
            batches.append((DeviceFrames(frames), boxes))
        want = [eng.generate_crops(fr, bx).numpy() for fr, bx in batches]
        tickets = [a.submit_crops(fr, bx) for fr, bx in batches]
        assert all("ready" in t for t in tickets[:4]) and "ready" not in tickets[4]
        for i in (4, 0, 3, 1, 2):      # any order
            assert np.array_equal(a.finish(tickets[i]).numpy(), want[i]), i
        # an abandoned video: queued passes are dropped, their tickets report the failure instead of hanging
        more = [a.submit_crops(fr, bx) for fr, bx in batches[:4]]
        a.discard_queue()
        for t in more:
            try:
                a.finish(t)
            except Exception:
                pass
        t = a.submit_crops(*batches[0])
        t2 = a.submit_crops(*batches[1])
        assert np.array_equal(a.finish(t).numpy(), want[0]) and np.array_equal(a.finish(t2).numpy(), want[1])
    finally:
        a.close()
    with pytest.raises(NativeError):   # a closed engine takes no more tickets
        a.submit_crops(*batches[0])


def test_panel_major_gemm_inputs_change_no_bit(base, monkeypatch):
    """The encoder pass's dense layers read their fp16 inputs and weights K-panel-major ([K / 32][rows][32]: an LDS-DMA piece of the dense
    GEMM is then 1 KB of contiguous memory; the LayerNorm, the attention and the GELU GEMM write that order when every consumer of the pass
    is a dense GEMM).  Same values, same products, same order: encoder states and logits equal the row-major build's (VTD_DENSE_PANEL=0) bit
    for bit, at a pass size that takes the dense path."""
    from vtd_amd.engine import TrOCREngine
    eng, sd = base
    monkeypatch.setenv("VTD_DENSE_GEMM", "1")          # the dense path wherever the shape allows (16 crops x 577 tokens = 37 row tiles)
    x = torch.stack([otrocr.preprocess(synth.glyph_crop(1200 + i), BASE_PRINTED) for i in range(16)])
    outs = []
    for panel in ("1", "0"):
        monkeypatch.setenv("VTD_DENSE_PANEL", panel)
        e = TrOCREngine(BASE_PRINTED, sd, max_crops=16)
        try:
            ids, lg = e.generate_pixels(x, want_logits=True, max_length=6)
            outs.append((e.read_tap("encoder", 16).copy(), ids.numpy().copy(), lg.numpy().copy()))
        finally:
            e.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])
    assert float(np.abs(outs[0][0]).max()) > 0.1


def test_tall_decoder_gemm_equals_the_small_one_bit_for_bit(hip, monkeypatch):
    """From 768 live rows up the decoder's projections run on dec_gemm_tall_kernel (operands staged through LDS, 128 x 128 tiles on 16
    waves); below, on dec_gemm_kernel (operands streamed into registers).  Both sum K in the same four quarters in the same order, so the
    choice -- a function of the host's lagged row bound -- must not show in a single bit: 800 crops, teacher-forced logits of three steps
    (every projection incl. the vocabulary's, split-K slabs, GELU) and greedy ids with either kernel."""
    from vtd_amd.engine import TrOCREngine
    sd = weights.trocr_state_dict(BASE_PRINTED, seed=0)
    eng = TrOCREngine(BASE_PRINTED, sd, max_crops=800)
    try:
        g = torch.Generator().manual_seed(11)
        base = torch.stack([otrocr.preprocess(synth.glyph_crop(1300 + i), BASE_PRINTED) for i in range(8)])
        x = base[torch.arange(800) % 8] + 0.05 * torch.randn((800, 3, 384, 384), generator=g)
        outs = []
        for lds_from in ("768", "1000000"):
            monkeypatch.setenv("VTD_DEC_GEMM_LDS", lds_from)
            ids, lg = eng.generate_pixels(x, want_logits=True, max_length=4)
            outs.append((ids.numpy().copy(), lg.numpy().copy()))
        assert np.array_equal(outs[0][0], outs[1][0])
        assert np.array_equal(outs[0][1], outs[1][1])
        assert float(np.abs(outs[0][1]).max()) > 1.0 and len({tuple(r) for r in outs[0][0].tolist()}) >= 4
    finally:
        eng.close()
