"""Host-side yardstick for the FastSpeech2MIDI pitch-branch tests: the golden cases' loader (tests/golden/fs2_pitch_*.npz, written
by tests/golden/make_golden_fs2_pitch.py from the reference's own class) and a float32 torch restatement of the pitch tail --
denorm_f0, f0_to_coarse, the pitch_embed gather and the mask.  Nothing here calls the library.

Restates NeuralSeq/modules/fastspeech/fs2.py:209-220,132 (pitch_type 'frame'), utils/pitch_utils.py:15-31 (f0_to_coarse) and
:63-76 (denorm_f0); tests/test_fs2_pitch_host.py holds it against the reference's own outputs."""
import ast
import hashlib
import os

import numpy as np
import torch

from audiogpt_amd import weights as WT

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# (file, array prefix) of every golden forward
CASES = [("fs2_pitch_b2_t33", ""), ("fs2_pitch_given_f0_uv", ""), ("fs2_pitch_given_f0", ""), ("fs2_pitch_short", "t1."),
         ("fs2_pitch_short", "t4."), ("fs2_pitch_ph384_b2_t9", ""), ("fs2_pitch_standard", "")]
GIVEN_F0 = ("fs2_pitch_given_f0_uv", "fs2_pitch_given_f0", "fs2_pitch_standard")
F0_BIN, F0_MAX, F0_MIN = 256, 1100.0, 50.0
F0_MEL_MIN = 1127 * np.log(1 + F0_MIN / 700)
F0_MEL_MAX = 1127 * np.log(1 + F0_MAX / 700)
NOT_ARRAYS = ("cfg", "linear_bias", "keys", "pitch_linear_weight", "pitch_linear_bias")


def load_case(name, prefix=""):
    """-> (cfg, state dict with the generator's duration bias and pitch linear, {inputs, outputs, flagged, floor_*, keys});
    `mel2ph_in` / `f0_in` / `uv_in` are present where the case hands them to the network."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cfg = ast.literal_eval(str(z["cfg"]))
    sd = WT.make_fs2_state_dict(cfg, seed=17)
    sd["dur_predictor.linear.bias"] = torch.from_numpy(z["linear_bias"]).clone()
    sd["pitch_predictor.linear.weight"] = torch.from_numpy(z["pitch_linear_weight"]).clone()
    sd["pitch_predictor.linear.bias"] = torch.from_numpy(z["pitch_linear_bias"]).clone()
    g = {k[len(prefix):]: z[k] for k in z.files if k.startswith(prefix) and k not in NOT_ARRAYS}
    g["keys"] = [str(k) for k in z["keys"]]
    return cfg, sd, g


def inputs(g):
    """The golden's inputs as the class takes them."""
    t = lambda k: torch.from_numpy(g[k]).clone() if k in g else None      # noqa: E731
    return dict(txt_tokens=t("txt_tokens"), pitch_midi=t("pitch_midi"), midi_dur=t("midi_dur"), is_slur=t("is_slur"),
                mel2ph=t("mel2ph_in"), f0=t("f0_in"), uv=t("uv_in"))


def f0_to_coarse(f0):
    """utils/pitch_utils.py:22-31 on an fp32 tensor: Python scalars against fp32 data, the reference's operation order."""
    m = 1127 * (1 + f0 / 700).log()
    m[m > 0] = (m[m > 0] - F0_MEL_MIN) * (F0_BIN - 2) / (F0_MEL_MAX - F0_MEL_MIN) + 1
    m[m <= 1] = 1
    m[m > F0_BIN - 1] = F0_BIN - 1
    return (m + 0.5).long()


def tail(cfg, pitch_pred, origin, mel2ph, pitch_embed, f0=None, uv=None):
    """pitch_pred [B, T, 2], origin [B, T, H], mel2ph [B, T] long, pitch_embed [300, H], a caller's f0 / uv [B, T] or None ->
    (f0_denorm [B, T], coarse [B, T] long, decoder_inp [B, T, H]), fp32."""
    pad = mel2ph == 0
    f0 = pitch_pred[:, :, 0] if f0 is None else f0
    if cfg["use_uv"] and uv is None:
        uv = pitch_pred[:, :, 1] > 0
    f = 2 ** f0 if cfg["pitch_norm"] == "log" else f0 * cfg["f0_std"] + cfg["f0_mean"]
    f = f.clone()
    if uv is not None and cfg["use_uv"]:
        f[uv > 0] = 0
    f[pad] = 0
    coarse = f0_to_coarse(f)
    dec = (origin + pitch_embed[coarse]) * (~pad).float()[:, :, None]
    return f, coarse, dec


def state_dict_hash(sd):
    """sha256 over the keys, in order, and the bytes of their tensors."""
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()
