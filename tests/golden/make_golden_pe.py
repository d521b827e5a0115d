"""Golden vectors of DiffSinger's PitchExtractor, from the REFERENCE's own class (run in the build container only).

    python tests/golden/make_golden_pe.py      # needs /root/reference; writes tests/golden/pe_*.npz

The real `modules.fastspeech.pe.PitchExtractor` is constructed on the CPU with the approach of make_golden_ds_ddpm.py:
`utils.hparams.hparams` is used as the plain dict it is and updated per case with the keys the class reads, and an empty stub
module stands in for `librosa`, which `utils.pitch_utils` imports and the inference path never calls.  Weights are
`WT.make_pe_state_dict(cfg, seed=13)` loaded with strict=True and are not stored, except the two values of
`pitch_predictor.linear.bias`, which the generator moves (random weights put the f0 channel and the voicing logit nowhere
near a trained network's range):
  * bias[1] is shifted by the median voicing logit of the non-padding frames (the midpoint of the two middle ones), so that
    25 - 75 % of them are voiced (asserted)
  * bias[0] is shifted so that the median f0 lands at 220 Hz ('log'; every f0 within 10 Hz .. 10 kHz, asserted) or at f0_mean
The mel's seed is searched (deterministically, from the case's first seed on) until the voicing-margin condition of
tests/test_gpu_pe.py holds for the reference itself: frames whose |voicing logit| <= 2e-4 * max|pitch_pred| (the bf16x3 gate)
are at most 1 % of the frames, and none in a case under 100 frames.

Each case is also run once in float64 (the same module, .double()); the largest fp32 - fp64 differences of pitch_pred and of
mel_hidden are stored: the reference's own rounding, the floor under the gates of tests/test_pe_host.py.
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

HP_KEYS = ("hidden_size", "predictor_hidden", "predictor_kernel", "ffn_padding", "pitch_type", "use_uv", "pitch_norm", "f0_mean",
           "f0_std")
MARGIN_GATE = 2e-4


def load_reference():
    sys.path.insert(0, NS)
    sys.modules.setdefault("librosa", types.ModuleType("librosa"))
    from utils.hparams import hparams
    import modules.fastspeech.pe as pe
    return pe, hparams


def mel_input(B, T, zero_frames, seed):
    g = torch.Generator().manual_seed(seed)
    mel = torch.rand(B, T, 80, generator=g) * 6.0 - 5.0
    for b, frames in zero_frames.items():
        for t in frames:
            mel[b, t] = 0.0
    return mel


def run(model, mel):
    hid = []
    hook = model.pitch_predictor.register_forward_hook(lambda m, i, o: hid.append(i[0].detach().clone()))
    try:
        with torch.no_grad():
            ret = model(mel)
    finally:
        hook.remove()
    return hid[0], ret["pitch_pred"], ret["f0_denorm_pred"]


def case(pe, hparams, tag, cfg, shapes, seed, linear_bias=None):
    """shapes: [(prefix, B, T, zero_frames)].  Returns the arrays of one npz and the linear bias used."""
    hparams.update({k: cfg[k] for k in HP_KEYS})
    sd = WT.make_pe_state_dict(cfg, seed=13)
    model = pe.PitchExtractor(cfg["n_mel_bins"], cfg["conv_layers"]).eval()
    model.load_state_dict(sd, strict=True)
    out = {"keys": np.asarray(list(model.state_dict().keys()))}
    big = [s for s in shapes if s[1] * s[2] >= 37]
    for attempt in range(64):
        mels = {p: mel_input(B, T, z, seed + attempt + 100 * i) for i, (p, B, T, z) in enumerate(shapes)}
        if linear_bias is None and big:
            with torch.no_grad():
                model.pitch_predictor.linear.bias.copy_(sd["pitch_predictor.linear.bias"])
            p, B, T, z = big[0]
            _, pp, _ = run(model, mels[p])
            live = mels[p].abs().sum(-1) != 0
            with torch.no_grad():
                v = pp[..., 1][live].sort().values          # (between the two middle logits: the median itself is some frame's)
                model.pitch_predictor.linear.bias[1] -= 0.5 * (v[v.numel() // 2 - 1] + v[v.numel() // 2])
                target = np.log2(220.0) if cfg["pitch_norm"] == "log" else 0.0
                model.pitch_predictor.linear.bias[0] += target - pp[..., 0][live].median()
        elif linear_bias is not None:
            with torch.no_grad():
                model.pitch_predictor.linear.bias.copy_(torch.as_tensor(linear_bias))
        ok = True
        res = {}
        for p, B, T, z in shapes:
            hid, pp, f0 = run(model, mels[p])
            res[p] = (hid, pp, f0)
            live = mels[p].abs().sum(-1) != 0
            near = int((pp[..., 1].abs() <= MARGIN_GATE * pp.abs().max()).sum())
            frames = B * T
            if near > (frames // 100 if frames >= 100 else 0):
                ok = False
            if frames >= 37 and cfg["use_uv"]:
                voiced = float((pp[..., 1][live] <= 0).float().mean())
                if not 0.25 <= voiced <= 0.75:
                    ok = False
        if ok:
            break
    assert ok, tag
    m64 = copy.deepcopy(model).double()
    for p, B, T, z in shapes:
        hid, pp, f0 = res[p]
        live = mels[p].abs().sum(-1) != 0
        if B * T >= 37 and cfg["use_uv"]:
            voiced = float((pp[..., 1][live] <= 0).float().mean())
            assert 0.25 <= voiced <= 0.75, (tag, voiced)
        if cfg["pitch_norm"] == "log" and B * T >= 37:
            v = f0[f0 > 0]
            assert float(v.min()) >= 10.0 and float(v.max()) <= 1e4, (tag, float(v.min()), float(v.max()))
        assert bool((f0[~live] == 0).all())
        hid64, pp64, _ = run(m64, mels[p].double())
        pre = p + "." if p else ""
        out.update({pre + "mel": mels[p].numpy(), pre + "mel_hidden": hid.numpy(), pre + "pitch_pred": pp.numpy(),
                    pre + "f0_denorm_pred": f0.numpy(),
                    pre + "floor_pitch_pred": np.float64((pp.double() - pp64).abs().max()),
                    pre + "floor_mel_hidden": np.float64((hid.double() - hid64).abs().max())})
        print("%s %s[%d, %d] seed+%d  voiced %.0f %%  f0 %.1f .. %.1f  max|pp| %.2f  near-margin frames %d  fp32-fp64: pp %.1e hidden %.1e"
              % (tag, pre, B, T, attempt, 100 * float((f0[live] > 0).float().mean()), float(f0[f0 > 0].min()) if (f0 > 0).any() else 0,
                 float(f0.max()), float(pp.abs().max()), int((pp[..., 1].abs() <= MARGIN_GATE * pp.abs().max()).sum()),
                 out[pre + "floor_pitch_pred"], out[pre + "floor_mel_hidden"]))
    bias = model.pitch_predictor.linear.bias.detach().clone().numpy()
    out["linear_bias"] = bias
    out["cfg"] = np.asarray(repr({k: cfg[k] for k in HP_KEYS + ("n_mel_bins", "conv_layers")}))
    return out, bias


def main():
    pe, hparams = load_reference()
    base = dict(C.PITCH_EXTRACTOR)
    zf3 = {0: range(32, 37), 1: [10]}
    cases = {}
    cases["pe_b3_t37"], bias = case(pe, hparams, "b3_t37", base, [("", 3, 37, zf3)], seed=31)
    cases["pe_cl0_b2_t37"], _ = case(pe, hparams, "cl0_b2_t37", dict(base, conv_layers=0), [("", 2, 37, zf3)], seed=32)
    cases["pe_b2_t129"], _ = case(pe, hparams, "b2_t129", base, [("", 2, 129, {0: range(120, 129), 1: [64]})], seed=33)
    cases["pe_short"], _ = case(pe, hparams, "short", base, [("t1", 1, 1, {}), ("t4", 1, 4, {})], seed=34, linear_bias=bias)
    cases["pe_std_nouv_b2_t37"], _ = case(pe, hparams, "std_nouv_b2_t37",
                                          dict(base, pitch_norm="standard", f0_mean=200.0, f0_std=50.0, use_uv=False),
                                          [("", 2, 37, zf3)], seed=35)
    cases["pe_ph384_b2_t37"], _ = case(pe, hparams, "ph384_b2_t37", dict(base, predictor_hidden=384), [("", 2, 37, zf3)], seed=36)
    for name, arrays in cases.items():
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(name, "%d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
