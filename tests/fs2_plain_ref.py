"""The plain FastSpeech2's goldens (tests/golden/fs2_plain_*.npz, written by make_golden_fs2_plain.py from the reference's own
class) and a float32 restatement of what is new in it beside FastSpeech2MIDI: the token-counted positions, the embedding
(modules/fastspeech/tts_modules.py:352-375) and the energy tail (modules/fastspeech/fs2.py:128-132, 165-172).  The host tests
hold the restatement against the goldens; the GPU tests hold the device against the goldens."""
import ast
import math
import os

import numpy as np
import torch

from audiogpt_amd import weights as WT

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# (file, array prefix) of every golden forward
CASES = [("fs2_plain_b2_t33", ""), ("fs2_plain_energy_spk_b2_t33", ""), ("fs2_plain_given", ""), ("fs2_plain_short", "t1."),
         ("fs2_plain_short", "t4."), ("fs2_plain_relpos_b2_t9", ""), ("fs2_plain_ph384_b2_t9", "")]
PREDICTED = [c for c in CASES if c[0] != "fs2_plain_given"]      # the cases with predicted durations
NOT_ARRAYS = ("cfg", "keys", "linear_bias", "pitch_linear_weight", "pitch_linear_bias", "energy_linear_weight", "energy_linear_bias")
SEED = 19


def load_case(name, prefix=""):
    """-> (cfg, state dict with the generator's moved weights, {inputs, outputs, flags, floor_*, keys}); `mel2ph_in` / `f0_in` /
    `uv_in` / `energy_in` are present where the case hands them to the network, `spk_ids` / `spk_vec` and `spk` with speakers."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cfg = ast.literal_eval(str(z["cfg"]))
    sd = WT.make_fs2_plain_state_dict(cfg, seed=SEED)
    sd["dur_predictor.linear.bias"] = torch.from_numpy(z["linear_bias"]).clone()
    for name_ in ("pitch", "energy"):
        if name_ + "_linear_weight" in z.files:
            sd[name_ + "_predictor.linear.weight"] = torch.from_numpy(z[name_ + "_linear_weight"]).clone()
            sd[name_ + "_predictor.linear.bias"] = torch.from_numpy(z[name_ + "_linear_bias"]).clone()
    g = {k[len(prefix):]: z[k] for k in z.files if k.startswith(prefix) and k not in NOT_ARRAYS}
    g["keys"] = [str(k) for k in z["keys"]]
    return cfg, sd, g


def call_args(cfg, g):
    """The golden's inputs as diffsinger.FastSpeech2.forward takes them: (txt_tokens, kwargs)."""
    t = lambda k: torch.from_numpy(g[k]).clone() if k in g else None      # noqa: E731
    kw = dict(mel2ph=t("mel2ph_in"), f0=t("f0_in"), uv=t("uv_in"), energy=t("energy_in"))
    if cfg["use_spk_id"]:
        ids = t("spk_ids")
        kw.update(spk_embed=ids[0], spk_embed_dur_id=ids[1], spk_embed_f0_id=ids[2])
    elif cfg["use_spk_embed"]:
        kw["spk_embed"] = t("spk_vec")
    return t("txt_tokens"), kw


def origin(g):
    """decoder_inp_origin: the reference's pad + gather of the encoder states by mel2ph (exact: a copy of rows)."""
    enc, m2p = torch.from_numpy(g["encoder_out"]), torch.from_numpy(g["mel2ph"])
    padded = torch.nn.functional.pad(enc, [0, 0, 1, 0])
    return torch.gather(padded, 1, m2p[..., None].repeat(1, 1, enc.shape[-1]))


def sinusoid_table(rows, dim):
    """SinusoidalPositionalEmbedding.get_embedding(rows, dim, padding_idx = 0) (common_layers.py:104-121)."""
    half = dim // 2
    e = torch.exp(torch.arange(half, dtype=torch.float) * -(math.log(10000) / (half - 1)))
    e = torch.arange(rows, dtype=torch.float).unsqueeze(1) * e.unsqueeze(0)
    tab = torch.cat([torch.sin(e), torch.cos(e)], dim=1).view(rows, -1)
    tab[0, :] = 0
    return tab


def rel_table(T, dim, max_len=5000):
    """RelPositionalEncoding's first T rows (espnet_positional_embedding.py:24-45 with reverse = True): row t holds position
    max_len - 1 - t."""
    pos = torch.arange(max_len - 1, -1, -1.0, dtype=torch.float32)[:T].unsqueeze(1)
    div = torch.exp(torch.arange(0, dim, 2, dtype=torch.float32) * -(math.log(10000.0) / dim))
    pe = torch.zeros(T, dim)
    pe[:, 0::2], pe[:, 1::2] = torch.sin(pos * div), torch.cos(pos * div)
    return pe


def positions(tok):
    """make_positions with padding_idx 0: the count of live tokens up to and including this one, 0 on a padding token."""
    live = (tok != 0).long()
    return torch.cumsum(live, dim=1) * live


def embed(cfg, tok, table_weight):
    """forward_embedding and FFTBlocks' first mask: [B, T] tokens -> [B, T, H], fp32."""
    H = cfg["hidden_size"]
    scale = math.sqrt(H)
    x = scale * table_weight[tok]
    if cfg["rel_pos"]:
        x = x * scale + rel_table(tok.shape[1], H)[None]
    else:
        x = x + sinusoid_table(tok.shape[1] + 1, H)[positions(tok)]
    return x * (tok != 0).float()[:, :, None]


def energy_bin(e):
    """clamp(e * 256 // 4, max = 255) as the reference computes it on an fp32 tensor, with the device's clamp at 0."""
    return torch.clamp(torch.clamp(e * 256 // 4, max=255), min=0).long()


def energy_tail(acc, energy_pred, mel2ph, energy_embed, spk=None, energy=None):
    """acc [B, T, H] (decoder_inp so far), energy_pred [B, T], mel2ph [B, T] long, energy_embed [256, H], spk [B, H] or None, a
    caller's energy [B, T] or None -> (bins [B, T] long, decoder_inp [B, T, H]), fp32, summed in the reference's order."""
    bins = energy_bin(energy_pred if energy is None else energy)
    dec = acc + energy_embed[bins]
    if spk is not None:
        dec = dec + spk[:, None, :]
    return bins, dec * (mel2ph > 0).float()[:, :, None]
