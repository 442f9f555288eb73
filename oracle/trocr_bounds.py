"""Stage-isolated fp64 references of the Transformer recogniser and their error model (TEST INFRASTRUCTURE ONLY, see
oracle/__init__.py).  The recogniser's counterpart of oracle/stage_bounds.py, built on the restatement in oracle/trocr.py.

Two stages, cut at taps the engine already has:

  encoder   input: the engine's ``pixel_values`` tap (fp16 values)       output: the ``encoder`` tap (fp32 states after the final LN)
  decoder   input: the ``encoder`` tap rounded to fp16 (what the slot and the key / value projections read) + forced ids
            output: the fp32 logits of every step of ``generate_pixels(..., forced=, want_logits=True)``

Two CPU evaluations of each stage:

  exact     fp64 throughout.  GEMM weights are rounded to fp16 as the engine uploads them (every 2-D+ ``.weight`` except the two
            embedding tables, which are looked up in fp32; a tied output projection is the fp16 copy of ``embed_tokens``); biases,
            LayerNorm parameters, [CLS], positions and the residual streams are fp32 in the engine and stay unrounded here.
  stored    the same with a round-to-fp16 wherever csrc/trocr_graph.inc stores or consumes fp16:
              encoder   ln16 (every LayerNorm output that feeds a GEMM); qkv; q after the 1/8 pre-scale (exact: a power of two);
                        the softmax numerators exp(s - running max) of every 64-key block as the PV product reads them (the row sum
                        stays fp32); att16; ffn16 (after GELU); enc16 / ln16 of the final LayerNorm (the decoder's input)
              decoder   d16 (every LayerNorm output); qkv16 and with it the K / V caches; q16; datt16 (self- and cross-attention
                        outputs); dffn16 (after GELU);
                        form 1 (attention on the raw encoder states): the composed weights wkt / wv16 (= the fp16 k_proj / v_proj
                        weights), qp16 (composed query), the numerators of every 16-token chunk, cp16 (attended state);
                        form 0 (key / value form): ck_buf / cv_buf
            The decoder's softmax in dec_attn runs in fp32 (no fp16 probabilities); logits are fp32.

Error metric: |got - exact| / RMS of the row of ``exact`` (encoder: a token's state; decoder: the logit row of a crop and step).
Level: the maximum and the 99.9th percentile of that over a region.  Bound: 3 x the level of ``stored`` against ``exact``, per stage,
spec, region and statistic -- the factor is applied to the EMULATED level, never to a measured one.  It covers what the emulation
cannot draw: another sample of the same rounding errors, and fp32 accumulation order (K 2^-24 against fp16's 2^-11).

Regions: encoder -- token 0, tokens 0..63, tokens past the last full 64-key block (= past the last full 128-query tile at 257);
decoder -- step 0, steps 1..63, steps >= 64.

``fault=`` injects one kernel bug into an evaluation (tests/test_trocr_bounds.py: the checker must reject each)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from .trocr import _heads, _lin, _ln

FACTOR = 3.0
ENC_KEY_BLOCK, XATTN_CHUNK = 64, 16
_FP32_TABLES = ("decoder.model.decoder.embed_tokens.weight", "decoder.model.decoder.embed_positions.weight")


def r16(x):
    return x.to(torch.float16).to(x.dtype)


def pick_split(k, split_max=8):
    """split-K of the decoder's N = D projections (vtd_trocr_generate_slot: a function of K only)"""
    ks = 1
    while ks < split_max and k // ks > 256 and k % (ks * 2 * 128) == 0:
        ks *= 2
    return ks


def _flash(s, v, block, r, keep_block=None):
    """softmax(s) v by key blocks with a running maximum, as the two flash kernels do: numerators relative to the running maximum go
    through `r` into the PV product, the row sum does not.  keep_block = j: when block j arrives the accumulated output is NOT
    rescaled (fault)."""
    m = torch.full(s.shape[:-1], -math.inf, dtype=s.dtype)
    l = torch.zeros_like(m)
    o = torch.zeros(s.shape[:-1] + (v.shape[-1],), dtype=s.dtype)
    for j, k0 in enumerate(range(0, s.shape[-1], block)):
        sb = s[..., k0:k0 + block]
        m_new = torch.maximum(m, sb.max(-1).values)
        corr = torch.exp(m - m_new)
        p = torch.exp(sb - m_new[..., None])
        l = l * corr + p.sum(-1)
        o = o * (torch.ones_like(corr) if j == keep_block else corr)[..., None] + r(p) @ v[..., k0:k0 + block, :]
        m = m_new
    return o / l[..., None]


class StageRef:
    def __init__(self, sd, spec, dtype=torch.float64):
        self.spec, self.dtype = spec, dtype
        self.sd = {}
        for k, v in sd.items():
            v = v.detach().float()
            if k.endswith(".weight") and v.dim() >= 2 and k not in _FP32_TABLES:
                v = v.half().float()
            self.sd[k] = v.to(dtype)
        if "decoder.output_projection.weight" not in self.sd:
            self.sd["decoder.output_projection.weight"] = sd[_FP32_TABLES[0]].detach().float().half().to(dtype)

    probe = None   # a dict: the evaluations record into it what the stress-weight conditions are pinned on (tests/test_trocr_bounds.py)

    def _rec(self, name, t):
        if self.probe is not None:
            self.probe.setdefault(name, []).append(t)

    def _r(self, stored):
        def r(x):   # every place the engine holds fp16
            if self.probe is not None:
                self.probe["fp16_peak"] = max(self.probe.get("fp16_peak", 0.0), float(x.abs().max()))
            return r16(x) if stored else x
        return r

    def _gelu(self, x, fault):
        self._rec("gelu_in", x)
        if fault == "tanh_gelu":
            return F.gelu(x, approximate="tanh")
        return 0.5 * x * torch.special.erfc(x * -0.7071067811865476)   # = x Phi(x), without 1 + erf's cancellation in the left tail

    # ------------------------------------------------------------------------------------------------------------ encoder
    @torch.no_grad()
    def encoder(self, pixel_values, stored=False, fault=None):
        """[B,3,S,S] (the engine's pixel tap) -> encoder states [B,T,C] (the `encoder` tap).
        faults: scale_twice | drop_last_key | keep_block | tanh_gelu | zero_cols"""
        sd, s, r = self.sd, self.spec, self._r(stored)
        e = "encoder.embeddings."
        px = torch.as_tensor(pixel_values).to(self.dtype)
        x = F.conv2d(px, sd[e + "patch_embeddings.projection.weight"], sd[e + "patch_embeddings.projection.bias"], stride=s.patch_size)
        x = x.flatten(2).transpose(1, 2)
        x = torch.cat([sd[e + "cls_token"].expand(x.shape[0], -1, -1), x], dim=1) + sd[e + "position_embeddings"]
        for i in range(s.enc_layers):
            p = f"encoder.encoder.layer.{i}."
            y = r(_ln(x, sd, p + "layernorm_before", s.enc_ln_eps))
            q, k, v = (_heads(r(_lin(y, sd, p + "attention.attention." + n)), s.enc_heads) for n in ("query", "key", "value"))
            q = r(q * 0.125)
            if fault == "scale_twice" and i == 0:
                q = q * 0.125
            sc = q @ k.transpose(-1, -2)
            if fault == "drop_last_key":
                sc[..., -1] = -math.inf
            self._rec("enc_scores", sc)
            a = _flash(sc, v, ENC_KEY_BLOCK, r, 1 if fault == "keep_block" else None)
            a = r(a.transpose(1, 2).reshape(x.shape))
            x = x + _lin(a, sd, p + "attention.output.dense")
            y = r(_ln(x, sd, p + "layernorm_after", s.enc_ln_eps))
            h = r(self._gelu(_lin(y, sd, p + "intermediate.dense"), fault))
            if fault == "zero_cols" and i == 0 and s.enc_ffn % 256:
                h[..., -(s.enc_ffn % 256):] = 0
            x = x + _lin(h, sd, p + "output.dense")
        return _ln(x, sd, "encoder.layernorm", s.enc_ln_eps)

    # ------------------------------------------------------------------------------------------------------------ decoder
    @torch.no_grad()
    def decoder(self, enc, forced, stored=False, form=0, fault=None):
        """enc [B,T,C] (the encoder tap; rounded to fp16 here), forced [B,L] ids -> logits [B, L-1, V] of steps 0..L-2 (teacher
        forcing: all steps at once under a causal mask -- every step's K / V rows are the ones the cache holds).
        faults: no_q_scale | drop_last_key | drop_newest_key | keep_block | tanh_gelu | pos_offset | drop_slab | bias_per_slab |
        ("row0", first_row)"""
        sd, s, r = self.sd, self.spec, self._r(stored)
        q_ = "decoder.model.decoder."
        H, D = s.dec_heads, s.dec_hidden
        enc = r16(torch.as_tensor(enc).to(self.dtype))
        ids = torch.as_tensor(np.asarray(forced)).long()[:, :-1]
        B, L = ids.shape
        scale = 1.0 if fault == "no_q_scale" else 0.125
        row0 = fault[1] if isinstance(fault, tuple) and fault[0] == "row0" else None
        off = 1 if fault == "pos_offset" else 2
        x = sd[q_ + "embed_tokens.weight"][ids] + sd[q_ + "embed_positions.weight"][off:off + L]
        x = _ln(x, sd, q_ + "layernorm_embedding", s.dec_ln_eps)
        causal = torch.tril(torch.ones(L, L, dtype=torch.bool))
        if fault == "drop_newest_key":
            causal = causal & ~torch.eye(L, dtype=torch.bool)
            causal[0, 0] = True

        def split_lin(a, p, ks):   # an N = D projection that runs as ks split-K slabs, summed with the bias by the LayerNorm behind it
            if fault == "drop_slab" and ks > 1 and p.endswith("layers.0.self_attn.out_proj"):
                a = a.clone()
                a[..., -(a.shape[-1] // ks):] = 0
            y = F.linear(a, sd[p + ".weight"])
            return y + sd[p + ".bias"] * (ks if fault == "bias_per_slab" and p.endswith("layers.0.fc2") else 1)

        ks_d, ks_f = pick_split(D), pick_split(s.dec_ffn)
        for i in range(s.dec_layers):
            p = q_ + f"layers.{i}."
            d16 = r(x)
            q = _heads(r(_lin(d16, sd, p + "self_attn.q_proj") * scale), H)
            k = _heads(r(_lin(d16, sd, p + "self_attn.k_proj")), H)
            v = _heads(r(_lin(d16, sd, p + "self_attn.v_proj")), H)
            sc = (q @ k.transpose(-1, -2)).masked_fill(~causal, -math.inf)
            self._rec("self_scores", sc)
            a = r((torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(B, L, D))
            x = _ln(x + split_lin(a, p + "self_attn.out_proj", ks_d), sd, p + "self_attn_layer_norm", s.dec_ln_eps)
            d16 = r(x)
            qc = _heads(r(_lin(d16, sd, p + "encoder_attn.q_proj") * scale), H)
            wk, wv = sd[p + "encoder_attn.k_proj.weight"], sd[p + "encoder_attn.v_proj.weight"]
            if form == 1:   # composed query -> attention over the encoder states themselves -> value projection (trocr_xattn.hip)
                qp = r(torch.einsum("bhld,hdc->bhlc", qc, wk.view(H, 64, -1)))
                sc = qp @ enc[:, None].transpose(-1, -2)
                if fault == "drop_last_key":
                    sc[..., -1] = -math.inf
                self._rec("cross_scores", sc)
                cp = r(_flash(sc, enc[:, None].expand(-1, H, -1, -1), XATTN_CHUNK, r, 1 if fault == "keep_block" else None))
                a = torch.einsum("bhlc,hdc->bhld", cp, wv.view(H, 64, -1)) + sd[p + "encoder_attn.v_proj.bias"].view(1, H, 1, 64)
            else:
                ck = _heads(r(F.linear(enc, wk, sd[p + "encoder_attn.k_proj.bias"])), H)
                cv = _heads(r(F.linear(enc, wv, sd[p + "encoder_attn.v_proj.bias"])), H)
                sc = qc @ ck.transpose(-1, -2)
                if fault == "drop_last_key":
                    sc[..., -1] = -math.inf
                self._rec("cross_scores", sc)
                a = torch.softmax(sc, -1) @ cv
            a = r(a.transpose(1, 2).reshape(B, L, D))
            x = _ln(x + split_lin(a, p + "encoder_attn.out_proj", ks_d), sd, p + "encoder_attn_layer_norm", s.dec_ln_eps)
            d16 = r(x)
            if row0 is not None and i == 0:   # rows >= row0 of the fc1 launch computed from row 0's input
                d16 = d16.clone()
                d16[row0:] = d16[0]
            h = r(self._gelu(_lin(d16, sd, p + "fc1"), fault))
            x = _ln(x + split_lin(h, p + "fc2", ks_f), sd, p + "final_layer_norm", s.dec_ln_eps)
        return F.linear(r(x), sd["decoder.output_projection.weight"])


# ---------------------------------------------------------------------------------------------------------------- regions, levels, check
def encoder_regions(tokens):
    tail = tokens // ENC_KEY_BLOCK * ENC_KEY_BLOCK
    reg = {"token 0": slice(0, 1), "tokens 0-63": slice(0, min(64, tokens))}
    if tail < tokens:
        reg[f"tokens {tail}+"] = slice(tail, tokens)
    return reg


def decoder_regions(steps):
    reg = {"step 0": slice(0, 1)}
    if steps > 1:
        reg["steps 1-63"] = slice(1, min(64, steps))
    if steps > 64:
        reg["steps 64+"] = slice(64, steps)
    return reg


def sample_rows(n, seed=0):
    """crop rows a tall decode is checked on: the edges of the 16-, 32- and 64-row tiles, the last row, and a random tenth"""
    rows = {r for r in (0, 15, 16, 31, 32, 63, 64, n - 1) if r < n}
    rows |= set(np.random.default_rng(seed).choice(n, max(1, n // 10), replace=False).tolist())
    return sorted(rows)


def rel_error(got, exact):
    """|got - exact| / RMS of exact's row, fp64 [B, rows, width]"""
    exact = torch.as_tensor(exact).double()
    got = torch.as_tensor(np.asarray(got)).double()
    return (got - exact).abs() / exact.pow(2).mean(-1, keepdim=True).sqrt()


def levels(got, exact, regions, rows=None):
    """{(region, 'max' | 'p99.9'): level}; rows: indices of dimension 0 to look at (default all)"""
    z = rel_error(got, exact)
    if rows is not None:
        z = z[rows]
    out = {}
    for name, sl in regions.items():
        zr = z[:, sl].reshape(-1)
        if zr.numel() == 0:
            continue
        out[(name, "max")] = float(zr.max())
        out[(name, "p99.9")] = float(np.quantile(zr.numpy(), 0.999))
    return out


def bounds(stored, exact, regions, rows=None):
    return {k: FACTOR * v for k, v in levels(stored, exact, regions, rows).items()}


def check(got, exact, stored, regions, what="", rows=None):
    """Levels of `got` against FACTOR x the levels of `stored`.  Returns {'ok', 'usage' (worst level / bound), 'table': {key: (emulated
    level, bound, level, usage)}}."""
    lv, em = levels(got, exact, regions, rows), levels(stored, exact, regions, rows)
    table = {k: (em[k], FACTOR * em[k], lv[k], lv[k] / (FACTOR * em[k])) for k in lv}
    usage = max(t[3] for t in table.values())
    return {"ok": usage <= 1.0, "usage": usage, "table": table, "what": what}


def report(st):
    return "\n".join(f"{st['what']:40s} {k[0]:12s} {k[1]:6s} emulated {t[0]:.3e}  bound {t[1]:.3e}  level {t[2]:.3e}  usage {t[3]:.3f}"
                     for k, t in st["table"].items())


def assert_stage(got, exact, stored, regions, what="", rows=None):
    st = check(got, exact, stored, regions, what, rows)
    print(report(st))
    assert st["ok"], f"{what}: level exceeds {FACTOR} x the emulated level (usage {st['usage']:.2f})\n{report(st)}"
    return st


# ---------------------------------------------------------------------------------------------------------------- free-running decode
@torch.no_grad()
def greedy(ref, enc):
    """Greedy search of the `exact` evaluation on encoder states (rounded to fp16 as the engine reads them).  Returns (ids [B, L] as
    generate pads them, logits [B, steps, V] fp64, finish [B]: the step whose arg-max was <eos>, or `steps` for a row that never ends)."""
    from . import trocr as otrocr
    enc = r16(torch.as_tensor(enc).to(ref.dtype))
    ids, logits = otrocr.generate(enc, ref.sd, ref.spec)
    steps = logits.shape[1]
    finish = torch.full((ids.shape[0],), steps, dtype=torch.long)
    for b in range(ids.shape[0]):
        hit = (ids[b, 1:] == ref.spec.eos_token_id).nonzero()
        if len(hit):
            finish[b] = int(hit[0])
    return ids, logits, finish


def well_posed(logits, finish, bound_rel):
    """crops whose top-2 logit gap exceeds 2 x the decoder bound (bound_rel x the row's RMS) at every step up to the one that ends them"""
    top = logits.topk(2, dim=-1).values
    gap = top[..., 0] - top[..., 1]
    need = 2.0 * bound_rel * logits.pow(2).mean(-1).sqrt()
    live = torch.arange(logits.shape[1])[None, :] <= finish[:, None]
    return ((gap > need) | ~live).all(1)


def compaction_reference(ref, enc):
    """greedy ids of the fp64 evaluation, the crops on which they are well-posed against the decoder bound, and the live-row history"""
    ids, logits, finish = greedy(ref, enc)
    exact = ref.decoder(enc, ids)
    assert float((exact[:, :logits.shape[1]] - logits).abs().max()) < 1e-9   # the step-by-step oracle and the stage function agree
    bound = bounds(ref.decoder(enc, ids, stored=True, form=1), exact, decoder_regions(exact.shape[1]))
    worst = max(v for k, v in bound.items() if k[1] == "max")
    return ids, well_posed(logits, finish, worst), finish, worst
