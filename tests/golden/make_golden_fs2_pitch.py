"""Golden vectors of FastSpeech2MIDI WITH its pitch branch (use_pitch_embed, pitch_type 'frame'), from the REFERENCE's own class
(run in the build container only, on the CPU).

    python tests/golden/make_golden_fs2_pitch.py [name ...]     # writes tests/golden/fs2_pitch_*.npz (or the named ones)

The model is built as make_golden_fs2.py builds it (hparams as a dict, stub librosa / pycwt, strict=True load of
WT.make_fs2_state_dict(cfg, seed=17)); its helpers are imported from there.  The duration bias is the one fs2_b2_t33.npz stores:
the tensors outside the pitch branch are the same with and without use_pitch_embed, so the durations are that file's.

Random weights give pitch_pred ~ 0: f0 ~ 1 Hz, every frame in bin 1.  So the generator moves pitch_predictor.linear and stores
it (`pitch_linear_weight` [2, C_p], `pitch_linear_bias` [2]; no other weight is stored):
  row 0  scaled and shifted so that the predicted log2 f0 over the live frames of the case's first candidate has median 7.8
         (~ 220 Hz) and a standard deviation of half an octave
  row 1  scaled to a standard deviation of 4 and shifted so that 30 % of those frames have a logit > 0 (unvoiced)
The input seed is searched (deterministically, at most 64 attempts; the first candidate of the predicted case is fs2_b2_t33's
own inputs) until: no live token within the bf16x3 gate of a duration rounding boundary (make_golden_fs2.near_boundary); every
live frame's voicing logit clear of 0 by that gate, |logit| > 2e-4 * max|pitch_pred|; 20 - 40 % of the live frames unvoiced.

A coarse bin is ~3.9 mel wide and the gate on a log2 f0 of ~8.5 moves the mel by ~0.3 at 220 Hz, so bins cannot all be kept
clear of a rounding boundary: the frames that are not are FLAGGED (`flagged`, bool [B, T_mel]): a voiced live frame with a
predicted f0 where (int)(m + 0.5) differs between the predictions v - d and v + d, d = 2e-4 * max|pitch_pred[..., 0]|, m in
float64.  Asserted here, on the reference alone: flagged <= 30 % of the live frames, >= 20 distinct bins, both voicings (the big
predicted case).  With a caller's f0 (placed at bin centres) nothing is flagged: every integer is exact by construction.

`coarse` is what pitch_embed was called with (a forward hook); `decoder_inp_origin` the expanded encoder states (the reference's
own pad + gather on the hooked encoder output).  `pitch_pred` is ret['pitch_pred'] as the reference leaves it: channel 0 zeroed
on padding frames when f0 was predicted (fs2.py:215-216 writes through the view).  A caller's f0 is handed over as a clone and
stored as it was before the call.  Each case is also run in float64; the largest fp32 - fp64 differences are stored as floor_*
(decoder_inp over the rows whose bin agrees, mel_out only where every bin agrees, else nan)."""
import copy
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import make_golden_fs2 as G                    # noqa: E402
from audiogpt_amd import config as C           # noqa: E402
from audiogpt_amd import weights as WT         # noqa: E402

PITCH_KEYS = ("pitch_type", "use_uv", "pitch_norm", "pitch_ar", "predictor_layers", "predictor_kernel", "f0_mean", "f0_std")
GATE = G.MARGIN_GATE
F0_MEL_MIN = 1127 * np.log(1 + 50.0 / 700)
F0_MEL_MAX = 1127 * np.log(1 + 1100.0 / 700)


def coarse64(f0):
    """f0_to_coarse in float64 (f0 in Hz, 0 = unvoiced)."""
    f0 = np.asarray(f0, dtype=np.float64)
    m = 1127 * np.log(1 + f0 / 700)
    m = np.where(m > 0, (m - F0_MEL_MIN) * 254 / (F0_MEL_MAX - F0_MEL_MIN) + 1, m)
    return np.floor(np.clip(m, 1, 255) + 0.5).astype(np.int64)


def bin_centre_hz(k):
    """The f0 whose scaled mel is exactly k (bin k holds [k - 1/2, k + 1/2))."""
    mel = (np.asarray(k, dtype=np.float64) - 1) * (F0_MEL_MAX - F0_MEL_MIN) / 254 + F0_MEL_MIN
    return 700 * (np.exp(mel / 1127) - 1)


def denorm64(v, cfg):
    v = np.asarray(v, dtype=np.float64)
    return 2.0 ** v if cfg["pitch_norm"] == "log" else v * cfg["f0_std"] + cfg["f0_mean"]


def build_model(fs2, hparams, cfg, dur_bias, linear=None):
    hparams.update({k: cfg[k] for k in G.HP_KEYS + PITCH_KEYS})
    hparams.update(G.HP_EXTRA)
    model = fs2.FastSpeech2MIDI(G.Dictionary(cfg["vocab_size"])).eval()
    model.load_state_dict(WT.make_fs2_state_dict(cfg, seed=17), strict=True)
    with torch.no_grad():
        model.dur_predictor.linear.bias.copy_(torch.as_tensor(dur_bias))
        if linear is not None:
            model.pitch_predictor.linear.weight.copy_(torch.as_tensor(linear[0]))
            model.pitch_predictor.linear.bias.copy_(torch.as_tensor(linear[1]))
    return model


def run(model, inp, mel2ph=None, f0=None, uv=None, double=False):
    enc, coarse = [], []
    hooks = [model.encoder.register_forward_hook(lambda m, i, o: enc.append(o.detach().clone())),
             model.pitch_embed.register_forward_hook(lambda m, i, o: coarse.append(i[0].detach().clone()))]
    try:
        with torch.no_grad():
            f0_arg = None if f0 is None else (f0.double() if double else f0.clone())          # (the reference writes into it)
            ret = model(inp["txt_tokens"], mel2ph=mel2ph, f0=f0_arg, uv=None if uv is None else uv.clone(), infer=True,
                        pitch_midi=inp["pitch_midi"], midi_dur=inp["midi_dur"].double() if double else inp["midi_dur"],
                        is_slur=inp["is_slur"])
    finally:
        for h in hooks:
            h.remove()
    m2p = ret["mel2ph"]
    origin = torch.gather(F.pad(enc[0], [0, 0, 1, 0]), 1, m2p[..., None].repeat([1, 1, enc[0].shape[-1]]))
    out = dict(xs=ret["dur"].reshape(ret["dur"].shape[0], -1), mel2ph=m2p, decoder_inp_origin=origin, pitch_pred=ret["pitch_pred"],
               f0_denorm=ret["f0_denorm"], coarse=coarse[0], decoder_inp=ret["decoder_inp"], mel_out=ret["mel_out"])
    if "dur_choice" in ret:
        out["dur_choice"] = ret["dur_choice"]
    assert set(ret) == {"dur", "mel2ph", "decoder_inp", "pitch_pred", "f0_denorm", "mel_out"} | ({"dur_choice"} if mel2ph is None else set())
    return out


def move_linear(model, r):
    """Row 0 -> median 7.8, std 0.5 over the live frames; row 1 -> std 4, its 70th percentile at 0."""
    live = r["mel2ph"] > 0
    v, u = r["pitch_pred"][..., 0][live].double(), r["pitch_pred"][..., 1][live].double()
    lin = model.pitch_predictor.linear
    with torch.no_grad():
        s0 = 0.5 / float(v.std())
        lin.weight[0] *= s0
        lin.bias[0] = lin.bias[0] * s0 + (7.8 - s0 * float(v.median()))
        s1 = 4.0 / float(u.std())
        lin.weight[1] *= s1
        lin.bias[1] = lin.bias[1] * s1 - s1 * float(torch.quantile(u, 0.7))
    return lin.weight.detach().clone().numpy(), lin.bias.detach().clone().numpy()


def flag(r, cfg, predicted_f0):
    """Voiced live frames whose bin a change of the bf16x3 gate in the prediction can move."""
    live = (r["mel2ph"] > 0).numpy()
    if not predicted_f0:
        return np.zeros_like(live)
    v = r["pitch_pred"][..., 0].double().numpy()
    d = GATE * float(np.abs(v).max())
    voiced = live & (r["f0_denorm"].numpy() > 0)
    return voiced & (coarse64(denorm64(v - d, cfg)) != coarse64(denorm64(v + d, cfg)))


def logits_clear(r, use_uv_pred):
    if not use_uv_pred:
        return True
    live = r["mel2ph"] > 0
    return bool((r["pitch_pred"][..., 1][live].abs() > GATE * float(r["pitch_pred"].abs().max())).all())


def case(fs2, hparams, tag, cfg, shapes, dur_bias, linear=None, accept=None):
    """shapes: [(prefix, candidates(attempt) -> inputs, given {mel2ph, f0, uv} or a function of the inputs)].  Returns the arrays
    of one npz and the pitch linear used."""
    model = build_model(fs2, hparams, cfg, dur_bias, linear)
    out = {"keys": np.asarray(list(model.state_dict().keys()))}
    chosen = []
    for i, (p, cand, given) in enumerate(shapes):
        for attempt in range(64):
            inp = cand(attempt)
            kw = {k: v for k, v in (given or {}).items()}
            if linear is None and i == 0 and attempt == 0:
                linear = move_linear(model, run(model, inp, **kw))
            try:
                r = run(model, inp, **kw)
            except RuntimeError:          # a candidate whose durations sum to 0 frames
                continue
            live = r["mel2ph"] > 0
            ok = G.near_boundary(r["xs"], inp["txt_tokens"] > 0) == 0 and all(bool(torch.isfinite(r[k]).all()) for k in ("pitch_pred", "mel_out"))
            ok = ok and ("mel2ph" in kw or int(r["dur_choice"].sum(-1).min()) >= 1)
            ok = ok and logits_clear(r, cfg["use_uv"] and "uv" not in kw)
            if ok and "uv" not in kw and live.sum() >= 50:
                share = float((r["pitch_pred"][..., 1][live] > 0).float().mean())
                ok = 0.2 <= share <= 0.4
            if ok and (accept is None or accept(p, inp, r)):
                break
        else:
            raise AssertionError((tag, p))
        chosen.append((p, inp, kw, r, attempt))
    m64 = copy.deepcopy(model).double()
    for p, inp, kw, r, attempt in chosen:
        r64 = run(m64, inp, double=True, **kw)
        assert torch.equal(r64["mel2ph"], r["mel2ph"]), tag
        live = (r["mel2ph"] > 0).numpy()
        fl = flag(r, cfg, "f0" not in kw)
        pre = p + "." if p else ""
        for k, v in inp.items():
            out[pre + k] = v.numpy()
        for k, v in kw.items():
            out[pre + k + "_in"] = v.numpy()
        for k, v in r.items():
            out[pre + k] = v.numpy()
        out[pre + "flagged"] = fl
        # the reference's own conditions
        c, c64 = r["coarse"].numpy(), r64["coarse"].numpy()
        assert c.min() >= 1 and c.max() <= 255
        assert bool((c[~live] == 1).all()) and bool((r["f0_denorm"].numpy()[~live] == 0).all())
        assert bool((c == c64)[~fl].all()), (tag, "an unflagged frame whose bin differs between fp32 and fp64")
        assert np.array_equal(c[~fl], coarse64(r["f0_denorm"].double().numpy())[~fl])
        assert fl.sum() <= 0.3 * live.sum(), (tag, int(fl.sum()), int(live.sum()))
        assert logits_clear(r, cfg["use_uv"] and "uv" not in kw)
        same = c == c64
        d = lambda k: (r[k].double() - r64[k]).abs()      # noqa: E731
        out[pre + "floor_pitch_pred"] = np.float64(d("pitch_pred").max())
        out[pre + "floor_f0_denorm"] = np.float64(d("f0_denorm").max())
        out[pre + "floor_decoder_inp"] = np.float64(d("decoder_inp")[torch.from_numpy(same)].max())
        out[pre + "floor_mel_out"] = np.float64(d("mel_out").max()) if same.all() else np.float64("nan")
        voiced = live & (r["f0_denorm"].numpy() > 0)
        print("%s %s seed+%d  T_mel %d  live %d  unvoiced %d  flagged %d  bins %d  voiced Hz %.0f..%.0f  max|pitch_pred| %.2f  "
              "fp32-fp64: pitch_pred %.1e f0_denorm %.1e decoder_inp %.1e mel_out %.1e  bins differing %d" % (
                  tag, pre, attempt, r["mel2ph"].shape[1], live.sum(), (live & ~voiced).sum(), fl.sum(), len(np.unique(c[live])),
                  r["f0_denorm"].numpy()[voiced].min(), r["f0_denorm"].numpy()[voiced].max(), float(r["pitch_pred"].abs().max()),
                  out[pre + "floor_pitch_pred"], out[pre + "floor_f0_denorm"], out[pre + "floor_decoder_inp"],
                  out[pre + "floor_mel_out"], (~same).sum()))
    out["linear_bias"] = np.asarray(dur_bias, dtype=np.float32)
    out["pitch_linear_weight"], out["pitch_linear_bias"] = linear
    out["cfg"] = np.asarray(repr(dict(cfg)))
    return out, linear


def given_f0(live, cfg):
    """A caller's f0 at bin centres for the live frames [B, T_mel] (bool), normalised as the cfg's pitch_norm wants it: one
    below f0_min (bin 1), bins 1 / 2 and 254 / 255 adjacent, one above f0_max (bin 255), then bins spread over the table.
    -> (f0 [B, T_mel] float32, the bins by construction)."""
    head = [40.0, float(bin_centre_hz(1)), float(bin_centre_hz(2)), float(bin_centre_hz(254)), float(bin_centre_hz(255)), 1500.0]
    f0 = np.zeros(live.shape, dtype=np.float64)
    for b in range(live.shape[0]):
        n = int(live[b].sum())
        ks = 3 + (np.arange(max(n - len(head), 0)) * 37 + 11 * b) % 251          # bins 3 .. 253
        hz = np.asarray(head + [float(bin_centre_hz(k)) for k in ks])[:n]
        f0[b, :n] = hz
    bins = coarse64(f0)
    norm = np.log2(np.where(f0 > 0, f0, 1.0)) if cfg["pitch_norm"] == "log" else (f0 - cfg["f0_mean"]) / cfg["f0_std"]
    norm = np.where(live, norm, 0.0).astype(np.float32)
    # exact by construction: the fp32 value handed over, denormalised in float64, lies within 0.2 of the bin's centre
    hz32 = denorm64(norm, cfg)
    m = (1127 * np.log(1 + hz32 / 700) - F0_MEL_MIN) * 254 / (F0_MEL_MAX - F0_MEL_MIN) + 1
    inner = live & (hz32 >= 50.0) & (hz32 <= 1100.0)
    assert float(np.abs(m - np.rint(m))[inner].max()) < 0.2
    return torch.from_numpy(norm), bins


def main():
    fs2, hparams = G.load_reference()
    base = dict(C.FASTSPEECH2_MIDI_CASCADE)
    z = np.load(os.path.join(HERE, "fs2_b2_t33.npz"))
    dur_bias = z["linear_bias"]
    first = {k: torch.from_numpy(z[k]) for k in ("txt_tokens", "pitch_midi", "midi_dur", "is_slur")}
    pads33 = {0: [11], 1: range(20, 33)}
    cases = {}

    def accept_b2(p, inp, r):
        live = r["mel2ph"] > 0
        tot = live.sum(-1)
        c = r["coarse"][live]
        uv = r["pitch_pred"][..., 1][live] > 0
        return (r["mel2ph"].shape[1] > 128 and int(tot.max() - tot.min()) >= 64 and len(torch.unique(c)) >= 20
                and bool(uv.any()) and bool((~uv).any()))

    # ---- everything predicted, on fs2_b2_t33's inputs (a later candidate only if those fail a condition above)
    cand33 = lambda a: first if a == 0 else G.make_inputs(2, 33, pads33, base["vocab_size"], 151 + a)      # noqa: E731
    cases["fs2_pitch_b2_t33"], linear = case(fs2, hparams, "b2_t33", base, [("", cand33, None)], dur_bias, accept=accept_b2)
    g = cases["fs2_pitch_b2_t33"]
    live = g["mel2ph"] > 0
    assert len(np.unique(g["coarse"][live])) >= 20 and g["flagged"].sum() <= 0.3 * live.sum()
    assert np.array_equal(g["mel2ph"], z["mel2ph"]) or not np.array_equal(g["txt_tokens"], z["txt_tokens"])

    # ---- a caller's mel2ph (fs2_given_mel2ph's: 66 and 40 live frames of 70), f0 at bin centres and uv; then the same f0 with
    # the voicing predicted
    zg = np.load(os.path.join(HERE, "fs2_given_mel2ph.npz"))
    m2p = torch.from_numpy(zg["mel2ph_in"])
    f0, bins = given_f0((m2p > 0).numpy(), base)
    uv = ((torch.arange(70)[None, :] + torch.tensor([[0], [2]])) % 5 == 3).float() * (m2p > 0).float()
    uv[:, :6] = 0.0          # (the edge bins at the head of each sample stay voiced)
    candg = lambda a: G.make_inputs(2, 33, pads33, base["vocab_size"], 153 + a)      # noqa: E731
    # (the predicted voicing is the stricter search; the given-uv form then takes the score it found)
    cases["fs2_pitch_given_f0"], _ = case(fs2, hparams, "given_f0", base, [("", candg, dict(mel2ph=m2p, f0=f0))], dur_bias, linear)
    g = cases["fs2_pitch_given_f0"]
    unv = g["pitch_pred"][..., 1] > 0
    assert np.array_equal(g["coarse"], np.where(unv | (m2p.numpy() == 0), 1, bins)) and unv[m2p.numpy() > 0].any()
    same = {k: torch.from_numpy(g[k]) for k in ("txt_tokens", "pitch_midi", "midi_dur", "is_slur")}
    cases["fs2_pitch_given_f0_uv"], _ = case(fs2, hparams, "given_f0_uv", base, [("", lambda a: same, dict(mel2ph=m2p, f0=f0, uv=uv))],
                                             dur_bias, linear)
    g = cases["fs2_pitch_given_f0_uv"]
    assert np.array_equal(g["coarse"], np.where((uv.numpy() > 0) | (m2p.numpy() == 0), 1, bins))
    assert {1, 2, 254, 255} <= set(g["coarse"][0, :6].tolist())

    # ---- fewer rows than one block
    short = [("t1", lambda a: G.make_inputs(1, 1, {}, base["vocab_size"], 152 + a), None),
             ("t4", lambda a: G.make_inputs(1, 4, {}, base["vocab_size"], 252 + a), None)]
    cases["fs2_pitch_short"], _ = case(fs2, hparams, "short", base, short, dur_bias, linear,
                                       accept=lambda p, inp, r: r["mel2ph"].shape[1] < 9)

    # ---- the head's second register layout: its own weights, so its own duration bias (fs2_ph384_b2_t9's) and pitch linear
    wide = dict(base, predictor_hidden=384, enc_layers=1, dec_layers=1, predictor_layers=2)
    zw = np.load(os.path.join(HERE, "fs2_ph384_b2_t9.npz"))
    firstw = {k: torch.from_numpy(zw[k]) for k in ("txt_tokens", "pitch_midi", "midi_dur", "is_slur")}
    candw = lambda a: firstw if a == 0 else G.make_inputs(2, 9, {1: range(6, 9)}, base["vocab_size"], 154 + a)      # noqa: E731
    cases["fs2_pitch_ph384_b2_t9"], _ = case(fs2, hparams, "ph384_b2_t9", wide, [("", candw, None)], zw["linear_bias"])

    # ---- pitch_norm 'standard', a caller's f0 and uv, small: [2, 13] frames, 13 and 7 live
    std = dict(base, pitch_norm="standard", f0_mean=220.0, f0_std=60.0)
    m2s = torch.zeros(2, 13, dtype=torch.long)
    for b, d in enumerate(([1, 2, 1, 2, 1, 2, 1, 2, 1], [1, 1, 2, 1, 1, 1])):
        idx = [t + 1 for t, n in enumerate(d) for _ in range(n)]
        m2s[b, :len(idx)] = torch.tensor(idx)
    f0s, bins_s = given_f0((m2s > 0).numpy(), std)
    uvs = ((torch.arange(13)[None, :] + torch.tensor([[0], [1]])) % 4 == 2).float() * (m2s > 0).float()
    uvs[:, :6] = 0.0
    cands = lambda a: G.make_inputs(2, 9, {1: range(6, 9)}, base["vocab_size"], 155 + a)      # noqa: E731
    cases["fs2_pitch_standard"], _ = case(fs2, hparams, "standard", std, [("", cands, dict(mel2ph=m2s, f0=f0s, uv=uvs))], dur_bias, linear)
    g = cases["fs2_pitch_standard"]
    assert np.array_equal(g["coarse"], np.where((uvs.numpy() > 0) | (m2s.numpy() == 0), 1, bins_s))

    only = sys.argv[1:]          # names of the files to (re)write; none: all of them
    for name, arrays in cases.items():
        if only and name not in only:
            continue
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(name, "%d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
