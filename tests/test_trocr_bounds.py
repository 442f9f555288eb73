"""The Transformer recogniser's stage-isolated fp64 references (oracle/trocr_bounds.py) and their checker, on the CPU.

* the stress weights make all three attentions discriminating on the edge architectures A, B, C (vtd_amd/trocr_spec.py);
* a stand-in "GPU" output -- the `stored` evaluation carried out in fp32 arithmetic, i.e. the same rounding points plus fp32
  accumulation noise -- passes every case;
* the reference's own error (the `exact` evaluation in fp32 against fp64) is under 1 % of every bound;
* every plausible kernel bug injected into the reference is rejected with a level of at least 10 x the bound.

Row-maximum condition: the median row-maximum probability must lie between 10 / keys and 0.9.  A self-attention row of step s has
s + 1 keys, so for rows of fewer than 20 keys 10 / keys is capped at 0.5 (10 / keys >= 1 cannot be met below 11 keys): the lower
limit is min(10 / keys, 0.5) per row, compared through the median of row maximum / limit."""
import numpy as np
import pytest
import torch

from oracle import trocr as otrocr
from oracle import trocr_bounds as tb
from vtd_amd import trocr_spec as ts
from vtd_amd._fixtures import weights

SPECS = {"A": ts.STAGE_A, "B": ts.STAGE_B, "C": ts.STAGE_C}
FORMS = {"A": (1, 0), "B": (1, 0), "C": (0,)}
SEED, CROPS = 3, 3


class Case:
    """exact / stored evaluations of both stages of one spec on the seeded inputs, each computed once"""

    def __init__(self, name, crops=CROPS, length=None):
        self.name, self.spec = name, SPECS[name]
        self.sd = weights.stress_trocr_state_dict(self.spec, SEED)
        self.ref = tb.StageRef(self.sd, self.spec)
        self.px = weights.stress_trocr_pixels(self.spec, crops, 1)
        self.ids = weights.stress_trocr_ids(self.spec, crops, length or self.spec.max_length, 1)
        self.enc = self.ref.encoder(self.px)
        self.enc_stored = self.ref.encoder(self.px, stored=True)
        self.eregions = tb.encoder_regions(self.enc.shape[1])
        self.logits = self.ref.decoder(self.enc, self.ids)
        self.dregions = tb.decoder_regions(self.logits.shape[1])
        self._stored = {}

    def dec_stored(self, form):
        if form not in self._stored:
            self._stored[form] = self.ref.decoder(self.enc, self.ids, stored=True, form=form)
        return self._stored[form]


_CASES = {}


def case(name, crops=CROPS, length=None):
    key = (name, crops, length)
    if key not in _CASES:
        _CASES[key] = Case(name, crops, length)
    return _CASES[key]


@pytest.mark.parametrize("name", list(SPECS))
def test_stress_weights_are_discriminating(name):
    c = case(name)
    ref = tb.StageRef(c.sd, c.spec)
    ref.probe = {}
    enc = ref.encoder(c.px)
    for form in FORMS[name]:   # (form 1 also holds the composed query and the attended encoder state in fp16)
        ref.decoder(enc, c.ids, form=form)
    pr = ref.probe
    assert set(c.sd) == set(weights.trocr_state_dict(c.spec, 0)), "same keys as trocr_state_dict"
    print(name, "peak of the fp16-held activations", pr["fp16_peak"])
    assert pr["fp16_peak"] < 1e3
    g = torch.cat([t.reshape(-1) for t in pr["gelu_in"]])
    print(name, "GELU inputs", float(g.min()), float(g.max()))
    assert float(g.min()) <= -3 and float(g.max()) >= 3
    for kind in ("enc_scores", "self_scores", "cross_scores"):
        for sc in pr[kind]:
            if kind == "self_scores":
                sc = sc[:, :, 4:]   # steps >= 4
            fin = sc[torch.isfinite(sc)]
            keys = torch.isfinite(sc).sum(-1).double()
            pmax = torch.softmax(sc, -1).max(-1).values
            low = (10.0 / keys).clamp(max=0.5)
            print(f"{name} {kind}: scores [{float(fin.min()):.2f}, {float(fin.max()):.2f}]  median row-max p {float(pmax.median()):.3f}  "
                  f"median 10/keys {float((10 / keys).median()):.3f}  median p / limit {float((pmax / low).median()):.2f}")
            assert float(fin.min()) < -4 and float(fin.max()) > 4
            assert float((pmax / low).median()) >= 1.0 and float(pmax.median()) <= 0.9
    for k, v in c.sd.items():   # LayerNorm parameters and biases of activation size
        if ("layernorm" in k or "layer_norm" in k) and k.endswith(".weight"):
            assert 0.45 <= float(v.min()) and float(v.max()) <= 2.05, k
        elif k.endswith(".bias"):
            assert 0.2 <= float(v.std()) <= 4.0, (k, float(v.std()))


@pytest.mark.parametrize("name", list(SPECS))
def test_reference_matches_fp32_oracle(name):
    """The stage functions compute the network of oracle/trocr.py (up to the fp16 rounding of the weights)."""
    c = case(name)
    want = otrocr.encode(c.px, c.sd, c.spec)
    rel = float(tb.rel_error(want, c.enc).max())
    print(name, "encoder: fp64 stage reference vs fp32 oracle", rel)
    assert rel < 2e-2
    _, lg = otrocr.generate(want, c.sd, c.spec, forced=c.ids)
    rel = float(tb.rel_error(lg, c.logits).max())
    print(name, "decoder: fp64 stage reference (from its own encoder states) vs fp32 oracle", rel)
    assert rel < 5e-2
    for form in FORMS[name]:   # both cross-attention forms are the same function
        rel = float(tb.rel_error(c.ref.decoder(c.enc, c.ids, form=form), c.logits).max())
        assert rel < 1e-9, (form, rel)


@pytest.mark.parametrize("name", list(SPECS))
def test_stand_in_passes_and_reference_error_is_small(name):
    c = case(name)
    r32 = tb.StageRef(c.sd, c.spec, torch.float32)
    tb.assert_stage(r32.encoder(c.px, stored=True), c.enc, c.enc_stored, c.eregions, f"{name} encoder stand-in")
    st = tb.check(r32.encoder(c.px), c.enc, c.enc_stored, c.eregions, f"{name} encoder exact fp32")
    print(tb.report(st))
    assert st["usage"] < 0.01
    for form in FORMS[name]:
        tb.assert_stage(r32.decoder(c.enc, c.ids, stored=True, form=form), c.logits, c.dec_stored(form), c.dregions,
                        f"{name} decoder form {form} stand-in")
    st = tb.check(r32.decoder(c.enc, c.ids), c.logits, c.dec_stored(FORMS[name][0]), c.dregions, f"{name} decoder exact fp32")
    print(tb.report(st))
    assert st["usage"] < 0.01


# (label, stage, spec, cross-attention form, fault)
FAULTS = [
    ("attention scale applied twice", "encoder", "A", None, "scale_twice"),
    ("decoder q-scale omitted", "decoder", "A", 1, "no_q_scale"),
    ("last key dropped, encoder T=65", "encoder", "A", None, "drop_last_key"),
    ("last key dropped, encoder T=257", "encoder", "C", None, "drop_last_key"),
    ("last key dropped, cross-attention on encoder states", "decoder", "A", 1, "drop_last_key"),
    ("last key dropped, cross-attention on keys / values", "decoder", "C", 0, "drop_last_key"),
    ("newest key dropped from the self-attention cache", "decoder", "C", 0, "drop_newest_key"),
    ("key block left un-rescaled, encoder", "encoder", "B", None, "keep_block"),
    ("token chunk left un-rescaled, cross-attention", "decoder", "B", 1, "keep_block"),
    ("tanh-GELU, encoder", "encoder", "C", None, "tanh_gelu"),
    ("tanh-GELU, decoder", "decoder", "A", 1, "tanh_gelu"),
    ("decoder position offset 1", "decoder", "A", 1, "pos_offset"),
    ("last split-K slab of self_attn.out_proj dropped (4 slabs)", "decoder", "B", 1, "drop_slab"),
    ("last split-K slab of self_attn.out_proj dropped (2 slabs)", "decoder", "A", 1, "drop_slab"),
    ("fc2 bias added once per slab (4 slabs)", "decoder", "A", 1, "bias_per_slab"),
    ("fc2 bias added once per slab (8 slabs)", "decoder", "B", 0, "bias_per_slab"),
    ("last N mod 256 columns of fc1 zero", "encoder", "C", None, "zero_cols"),
]


@pytest.mark.parametrize("fault", FAULTS, ids=[f[0] for f in FAULTS])
def test_fault_is_rejected(fault):
    label, stage, name, form, what = fault
    c = case(name)
    if stage == "encoder":
        st = tb.check(c.ref.encoder(c.px, stored=True, fault=what), c.enc, c.enc_stored, c.eregions, label)
    else:
        st = tb.check(c.ref.decoder(c.enc, c.ids, stored=True, form=form, fault=what), c.logits, c.dec_stored(form), c.dregions, label)
    print(tb.report(st))
    print(f"fault [{name}] {label}: level / bound = {st['usage']:.1f}")
    assert not st["ok"]
    assert st["usage"] >= 10, (label, st["usage"])


@pytest.mark.parametrize("crops,first", [(21, 16), (70, 32), (260, 64)], ids=["<2,2> rows>=16", "<4,2> rows>=32", "<4,4> rows>=64"])
def test_tile_row_fault_is_rejected(crops, first):
    """fc1 rows past the first 16 / 32 / 64 computed from row 0's input, at the crop counts of the three taller dec_gemm tiles,
    seen through the rows the GPU case checks (tile edges, the last row, a random tenth)."""
    c = case("A", crops, 5)
    rows = tb.sample_rows(crops)
    good = tb.check(c.dec_stored(1), c.logits, c.dec_stored(1), c.dregions, "stored", rows)
    assert good["ok"]
    st = tb.check(c.ref.decoder(c.enc, c.ids, stored=True, form=1, fault=("row0", first)), c.logits, c.dec_stored(1), c.dregions,
                  f"rows >= {first} from row 0 at {crops} crops", rows)
    print(tb.report(st))
    print(f"fault [A] fc1 rows >= {first} from row 0's input at {crops} crops: level / bound = {st['usage']:.1f}")
    assert not st["ok"] and st["usage"] >= 10, st["usage"]


COMPACTION = dict(seed=SEED, eos_gain=4.0, project=False, crops=40, pixel_seed=9)   # tests/test_gpu_trocr_stages.py runs the same case


def compaction_inputs():
    sd = weights.stress_trocr_state_dict(ts.STAGE_A, COMPACTION["seed"], eos_gain=COMPACTION["eos_gain"], project=COMPACTION["project"])
    return sd, weights.stress_trocr_pixels(ts.STAGE_A, COMPACTION["crops"], COMPACTION["pixel_seed"])


def test_compaction_case_is_well_posed_on_the_reference_alone():
    """The free-running case of the GPU suite, on the CPU: rows end at >= 3 different steps, the live count falls through 32 and 16,
    and at least half of the crops keep a top-2 gap above twice the decoder bound at every step."""
    sd, px = compaction_inputs()
    ref = tb.StageRef(sd, ts.STAGE_A)
    ids, ok, finish, worst = tb.compaction_reference(ref, ref.encoder(px))
    live = [int((finish > s).sum()) for s in range(ts.STAGE_A.max_length - 1)]
    print("finish steps", sorted(set(finish.tolist())), "live rows after each step", live, "decoder bound", worst, "well-posed crops", int(ok.sum()))
    assert len(set(finish.tolist())) >= 3
    assert live[0] > 16 and min(live) < 16 and any(16 < v <= 32 for v in live)
    assert int(ok.sum()) * 2 >= len(ok) + 8, "margin over one half for the GPU run, whose encoder states differ in the last bits"
