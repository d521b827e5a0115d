"""Host-side yardstick for the PitchExtractor tests: a functional torch restatement of the network over a state dict, in the
dtype of its input (fp32 or fp64), and the golden cases' loader.  Nothing here calls the library.

Restates NeuralSeq/modules/fastspeech/pe.py:7-149 (Prenet, ConvStacks, PitchExtractor), tts_modules.py:217-260 (PitchPredictor),
utils/__init__.py:145-157 (make_positions), commons/common_layers.py:104-121 (the sinusoid table) and
utils/pitch_utils.py:63-76 (denorm_f0); tests/test_pe_host.py holds it against the reference's own outputs."""
import ast
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from audiogpt_amd import weights as WT

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# (file, array prefix) of every golden forward; frames = B * T
CASES = [("pe_b3_t37", ""), ("pe_cl0_b2_t37", ""), ("pe_b2_t129", ""), ("pe_short", "t1."), ("pe_short", "t4."),
         ("pe_std_nouv_b2_t37", ""), ("pe_ph384_b2_t37", "")]
EPS = 1e-5


def load_case(name, prefix=""):
    """-> (cfg, state dict with the generator's linear bias, {mel, mel_hidden, pitch_pred, f0_denorm_pred, floor_*, keys})."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cfg = ast.literal_eval(str(z["cfg"]))
    sd = WT.make_pe_state_dict(cfg, seed=13)
    sd["pitch_predictor.linear.bias"] = torch.from_numpy(z["linear_bias"]).clone()
    g = {k[len(prefix):]: z[k] for k in z.files if k.startswith(prefix) and k not in ("cfg", "linear_bias", "keys")}
    g["keys"] = [str(k) for k in z["keys"]]
    return cfg, sd, g


def make_positions(ch0):
    """ch0 [B, T] -> positions [B, T] (long): the running count of non-zero entries where the entry is non-zero, else 0."""
    mask = ch0.ne(0).int()
    return (torch.cumsum(mask, dim=1).type_as(mask) * mask).long()


def sinusoid_table(rows, dim):
    """get_embedding(rows, dim, padding_idx = 0): fp32 throughout, row 0 zero."""
    half = dim // 2
    freq = torch.exp(torch.arange(half, dtype=torch.float) * -(math.log(10000) / (half - 1)))
    ang = torch.arange(rows, dtype=torch.float).unsqueeze(1) * freq.unsqueeze(0)
    tab = torch.cat([torch.sin(ang), torch.cos(ang)], dim=1)
    tab[0] = 0
    return tab


def forward(sd, cfg, mel):
    """mel [B, T, n_mel_bins] -> (mel_hidden [B, T, H], pitch_pred [B, T, 2], f0 [B, T]) in mel's dtype."""
    dt = mel.dtype
    w = lambda k: sd[k].to(dt)      # noqa: E731
    pad = mel.abs().sum(-1).eq(0)
    keep = (~pad).to(dt)[:, None, :]
    x = mel.transpose(1, 2)
    for i in range(3):
        p = "mel_prenet.layers.%d." % i
        x = F.relu(F.conv1d(x, w(p + "0.weight"), w(p + "0.bias"), padding=2))
        x = (x - w(p + "2.running_mean")[:, None]) / torch.sqrt(w(p + "2.running_var")[:, None] + EPS)
        x = (x * w(p + "2.weight")[:, None] + w(p + "2.bias")[:, None]) * keep
    x = F.linear(x.transpose(1, 2), w("mel_prenet.out_proj.weight"), w("mel_prenet.out_proj.bias")) * keep.transpose(1, 2)
    H = x.shape[-1]
    if cfg["conv_layers"] > 0:
        x = F.linear(x, w("mel_encoder.in_proj.weight"), w("mel_encoder.in_proj.bias")).transpose(1, 2)
        for i in range(cfg["conv_layers"]):
            p = "mel_encoder.conv.%d." % i
            y = F.conv1d(x, w(p + "conv.conv.weight"), w(p + "conv.conv.bias"), padding=2)
            x = x + F.relu(F.group_norm(y, H // 16, w(p + "norm.weight"), w(p + "norm.bias"), EPS))
        x = F.linear(x.transpose(1, 2), w("mel_encoder.out_proj.weight"), w("mel_encoder.out_proj.bias"))
    hidden = x
    T = x.shape[1]
    pos = make_positions(x[..., 0])
    tab = sinusoid_table(max(4096, T + 1), H).to(dt)
    x = x + w("pitch_predictor.pos_embed_alpha") * tab[pos]
    k = cfg["predictor_kernel"]
    x = x.transpose(1, 2)
    for i in range(5):
        p = "pitch_predictor.conv.%d." % i
        x = F.relu(F.conv1d(F.pad(x, ((k - 1) // 2, (k - 1) // 2)), w(p + "1.weight"), w(p + "1.bias")))
        x = F.layer_norm(x.transpose(1, 2), (x.shape[1],), w(p + "3.weight"), w(p + "3.bias"), EPS).transpose(1, 2)
    pp = F.linear(x.transpose(1, 2), w("pitch_predictor.linear.weight"), w("pitch_predictor.linear.bias"))
    f0 = pp[..., 0]
    f0 = 2 ** f0 if cfg["pitch_norm"] == "log" else f0 * cfg["f0_std"] + cfg["f0_mean"]
    if cfg["pitch_type"] == "frame" and cfg["use_uv"]:
        f0 = torch.where(pp[..., 1] > 0, torch.zeros_like(f0), f0)
    f0 = torch.where(pad, torch.zeros_like(f0), f0)
    return hidden, pp, f0
