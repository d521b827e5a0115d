"""Golden vectors of DiffSinger's FastSpeech2MIDI, from the REFERENCE's own class (run in the build container only).

    python tests/golden/make_golden_fs2.py [name ...]     # needs /root/reference; writes tests/golden/fs2_*.npz (or the named ones)

The real `modules.diffsinger_midi.fs2.FastSpeech2MIDI` is constructed on the CPU with the approach of make_golden_pe.py:
`utils.hparams.hparams` is used as the plain dict it is and updated with the keys the class reads; empty stub modules stand in
for `librosa` and `pycwt`, which the imports pull in and the inference path never calls (`transformers` is imported BEFORE the
stubs are installed: its availability probe raises on a stub without `__spec__`); the dictionary is an object with `__len__`
and `pad()`.  Weights are `WT.make_fs2_state_dict(cfg, seed=17)` loaded with strict=True and are not stored, except
`dur_predictor.linear.bias`, which the generator moves so that the median duration of the live tokens of the first case is
3 - 5 frames (random weights put it near 0); the later cases reuse that bias, except fs2_ph384_b2_t9 (predictor_hidden = 384,
one encoder and one decoder layer: other weights), which moves its own the same way.

Durations are a rounding, so the input seed is searched (deterministically, at most 64 attempts from the case's first seed on)
until NO live token of the case lies within the bf16x3 gate of a rounding boundary:
    |exp(xs) - 1 - (k + 1/2)| <= exp(xs) * 2e-4 * max|xs|      for the nearest integer k >= 0
(asserted), which makes exact equality of dur_choice and mel2ph a fair demand of the device.

Each case is also run once in float64 (the same module, .double()); the largest fp32 - fp64 differences of encoder_out, xs,
decoder_inp and mel_out are stored: the reference's own rounding, the floor under the gates of tests/test_fs2_host.py.
"""
import copy
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
NS = os.path.join("/root/reference", "NeuralSeq")

from audiogpt_amd import config as C          # noqa: E402
from audiogpt_amd import weights as WT         # noqa: E402

HP_KEYS = ("hidden_size", "enc_layers", "dec_layers", "num_heads", "enc_ffn_kernel_size", "dec_ffn_kernel_size",
           "dur_predictor_layers", "dur_predictor_kernel", "predictor_hidden", "audio_num_mel_bins", "ffn_padding", "ffn_act",
           "dur_loss", "rel_pos", "use_pos_embed", "encoder_type", "decoder_type", "use_pitch_embed", "use_energy_embed",
           "use_spk_id", "use_spk_embed", "use_bert")
HP_EXTRA = dict(dropout=0.1, predictor_dropout=0.5, predictor_grad=0.1, use_split_spk_id=False)
MARGIN_GATE = 2e-4
FLOATS = ("encoder_out", "xs", "decoder_inp", "mel_out")


class Dictionary:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def pad(self):
        return 0


def load_reference():
    sys.path.insert(0, NS)
    import transformers  # noqa: F401      (before the stubs: its availability probe reads librosa's __spec__)
    for name in ("librosa", "pycwt", "pycwt.wavelet"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["pycwt"].wavelet = sys.modules["pycwt.wavelet"]          # (utils/cwt.py: from pycwt import wavelet)
    from utils.hparams import hparams
    import modules.diffsinger_midi.fs2 as fs2
    return fs2, hparams


def make_inputs(B, T, pads, vocab, seed):
    """pads: {sample: token positions that are padding}."""
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(1, vocab, (B, T), generator=g)
    midi = torch.randint(40, 90, (B, T), generator=g)
    dur = torch.rand(B, T, generator=g) * 0.9 + 0.1
    slur = torch.randint(0, 2, (B, T), generator=g)
    for b, pos in pads.items():
        for t in pos:
            tok[b, t], midi[b, t], dur[b, t], slur[b, t] = 0, 0, 0.0, 0
    return dict(txt_tokens=tok, pitch_midi=midi, midi_dur=dur, is_slur=slur)


def run(model, inp, mel2ph=None, double=False, skip_decoder=False):
    enc = []
    hook = model.encoder.register_forward_hook(lambda m, i, o: enc.append(o.detach().clone()))
    try:
        with torch.no_grad():
            ret = model(inp["txt_tokens"], mel2ph=mel2ph, skip_decoder=skip_decoder, infer=True, pitch_midi=inp["pitch_midi"],
                        midi_dur=inp["midi_dur"].double() if double else inp["midi_dur"], is_slur=inp["is_slur"])
    finally:
        hook.remove()
    out = dict(encoder_out=enc[0], xs=ret["dur"].reshape(ret["dur"].shape[0], -1), mel2ph=ret["mel2ph"],
               decoder_inp=ret["decoder_inp"])
    if not skip_decoder:
        out["mel_out"] = ret["mel_out"]
    if "dur_choice" in ret:
        out["dur_choice"] = ret["dur_choice"]
    return out


def near_boundary(xs, live):
    """Live tokens within the bf16x3 gate of a rounding boundary of round(exp(xs) - 1)."""
    x = xs.double()[live]
    e = x.exp()
    k = torch.clamp(torch.floor(e - 1.0), min=0)
    dist = torch.minimum((e - 1.0 - (k + 0.5)).abs(), (e - 1.0 - (k - 0.5).clamp(min=0.5)).abs())
    return int((dist <= e * MARGIN_GATE * float(xs.abs().max())).sum())


def build_model(fs2, hparams, cfg, linear_bias=None):
    hparams.update({k: cfg[k] for k in HP_KEYS})
    hparams.update(HP_EXTRA)
    sd = WT.make_fs2_state_dict(cfg, seed=17)
    model = fs2.FastSpeech2MIDI(Dictionary(cfg["vocab_size"])).eval()
    model.load_state_dict(sd, strict=True)
    if linear_bias is not None:
        with torch.no_grad():
            model.dur_predictor.linear.bias.copy_(torch.as_tensor(linear_bias))
    return model, sd


def case(fs2, hparams, tag, cfg, shapes, seed, linear_bias=None, accept=None, given=None):
    """shapes: [(prefix, B, T, pads)].  given: {prefix: mel2ph} handed to the network.  accept(prefix, inp, out) -> bool: the
    case's own conditions on a candidate.  Returns the arrays of one npz and the duration bias used."""
    model, sd = build_model(fs2, hparams, cfg, linear_bias)
    out = {"keys": np.asarray(list(model.state_dict().keys()))}
    inps, res, tries = {}, {}, {}
    for i, (p, B, T, pads) in enumerate(shapes):          # each shape searches its own seed
        m2p = given[p] if given else None
        for attempt in range(64):
            inp = make_inputs(B, T, pads, cfg["vocab_size"], seed + attempt + 100 * i)
            if linear_bias is None and i == 0:
                with torch.no_grad():
                    model.dur_predictor.linear.bias.copy_(sd["dur_predictor.linear.bias"])
                r = run(model, inp, skip_decoder=True)          # (the unmoved bias may give 0 frames: no decoder run on them)
                with torch.no_grad():          # median of exp(xs) - 1 at 4 frames
                    model.dur_predictor.linear.bias += float(np.log(5.0)) - r["xs"][inp["txt_tokens"] > 0].median()
            try:
                r = run(model, inp, mel2ph=m2p)
            except RuntimeError:          # a candidate whose durations sum to 0 frames: the reference's decoder cannot take it
                continue
            ok = near_boundary(r["xs"], inp["txt_tokens"] > 0) == 0 and all(bool(torch.isfinite(r[k]).all()) for k in FLOATS)
            ok = ok and (m2p is not None or int(r["dur_choice"].sum(-1).min()) >= 1)
            if ok and (accept is None or accept(p, inp, r)):
                break
        else:
            raise AssertionError((tag, p))
        inps[p], res[p], tries[p] = inp, r, attempt
    m64 = copy.deepcopy(model).double()
    for p, B, T, pads in shapes:
        r, inp = res[p], inps[p]
        live = inp["txt_tokens"] > 0
        assert near_boundary(r["xs"], live) == 0, tag
        m2p = given[p] if given else None
        r64 = run(m64, inp, mel2ph=m2p, double=True)
        assert torch.equal(r64["mel2ph"], r["mel2ph"]), tag
        pre = p + "." if p else ""
        for k, v in inp.items():
            out[pre + k] = v.numpy()
        if m2p is not None:
            out[pre + "mel2ph_in"] = m2p.numpy()
        for k, v in r.items():
            out[pre + k] = v.numpy()
        for k in FLOATS:
            out[pre + "floor_" + k] = np.float64((r[k].double() - r64[k]).abs().max())
        d = r.get("dur_choice")
        print("%s %s[%d, %d] seed+%d  T_mel %d  totals %s  median live dur %s  max|xs| %.2f  fp32-fp64: %s" % (
            tag, pre, B, T, tries[p], r["mel2ph"].shape[1], (r["mel2ph"] > 0).sum(-1).tolist(),
            "-" if d is None else "%.1f" % float(d[live].float().median()), float(r["xs"].abs().max()),
            " ".join("%s %.1e (max|ref| %.2f)" % (k, out[pre + "floor_" + k], float(r[k].abs().max())) for k in FLOATS)))
    bias = model.dur_predictor.linear.bias.detach().clone().numpy()
    out["linear_bias"] = bias
    out["cfg"] = np.asarray(repr(dict(cfg)))
    return out, bias


def main():
    fs2, hparams = load_reference()
    base = dict(C.FASTSPEECH2_MIDI)
    cases = {}

    def accept_b2(p, inp, r):
        live = inp["txt_tokens"] > 0
        med = float(r["dur_choice"][live].float().median())
        tot = r["dur_choice"].sum(-1)
        # the decoder crosses a 128-query tile; whole key tiles are hidden for the shorter sample only
        return 3 <= med <= 5 and r["mel2ph"].shape[1] > 128 and int(tot.max() - tot.min()) >= 64

    pads33 = {0: [11], 1: range(20, 33)}
    cases["fs2_b2_t33"], bias = case(fs2, hparams, "b2_t33", base, [("", 2, 33, pads33)], seed=51, accept=accept_b2)
    cases["fs2_short"], _ = case(fs2, hparams, "short", base, [("t1", 1, 1, {}), ("t4", 1, 4, {})], seed=52, linear_bias=bias,
                                 accept=lambda p, inp, r: r["mel2ph"].shape[1] < 9)
    # a caller's mel2ph [2, 70]: token 5 of sample 0 has no frame; the trailing zeros differ per sample
    d0 = [3] * 33
    d0[5], d0[11] = 0, 0
    d0 = d0[:24] + [0] * 9                                  # 22 tokens x 3 = 66 frames, 4 trailing zeros
    d1 = [2] * 20 + [0] * 13                                # 40 frames, 30 trailing zeros
    m2p = torch.zeros(2, 70, dtype=torch.long)
    for b, d in enumerate((d0, d1)):
        idx = [t + 1 for t, n in enumerate(d) for _ in range(n)]
        m2p[b, :len(idx)] = torch.tensor(idx)
    assert int((m2p[0] > 0).sum()) == 66 and int((m2p[1] > 0).sum()) == 40
    cases["fs2_given_mel2ph"], _ = case(fs2, hparams, "given_mel2ph", base, [("", 2, 33, pads33)], seed=53, linear_bias=bias,
                                        given={"": m2p})
    # a predictor wider than one float4 per lane (the duration head's second register layout): small, its own duration bias
    wide = dict(base, predictor_hidden=384, enc_layers=1, dec_layers=1)
    cases["fs2_ph384_b2_t9"], _ = case(fs2, hparams, "ph384_b2_t9", wide, [("", 2, 9, {1: range(6, 9)})], seed=54)
    only = sys.argv[1:]          # names of the files to (re)write; none: all of them
    for name, arrays in cases.items():
        if only and name not in only:
            continue
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(name, "%d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
