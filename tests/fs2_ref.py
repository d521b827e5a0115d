"""Host-side yardstick for the FastSpeech2MIDI tests: a functional torch restatement of the network over a state dict, in a
chosen dtype (fp32 or fp64), the golden cases' loader, and the float64 masked-attention reference with the seeded inputs of the
operator test.  Nothing here calls the library.

Restates NeuralSeq/modules/diffsinger_midi/fs2.py:11-118, modules/fastspeech/fs2.py:112-163,222-226, tts_modules.py:98-118
(DurationPredictor), :204-214 (LengthRegulator), :307-332 (FFTBlocks), commons/common_layers.py:502-521,563-587 (the FFN and
EncSALayer; MultiheadAttention with bias = False written out), espnet_positional_embedding.py:24-45,102-113;
tests/test_fs2_host.py holds it against the reference's own outputs."""
import ast
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from audiogpt_amd import weights as WT
from tests import attn_ref as A
from tests import pe_ref as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# (file, array prefix) of every golden forward
CASES = [("fs2_b2_t33", ""), ("fs2_short", "t1."), ("fs2_short", "t4."), ("fs2_given_mel2ph", ""), ("fs2_ph384_b2_t9", "")]
FLOATS = ("encoder_out", "xs", "decoder_inp", "mel_out")
EPS = 1e-5
REL_MAX_LEN = 5000


def load_case(name, prefix=""):
    """-> (cfg, state dict with the generator's duration bias, {inputs, outputs, floor_*, keys}); `mel2ph_in` is present where
    the case hands the network a mel2ph."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cfg = ast.literal_eval(str(z["cfg"]))
    sd = WT.make_fs2_state_dict(cfg, seed=17)
    sd["dur_predictor.linear.bias"] = torch.from_numpy(z["linear_bias"]).clone()
    g = {k[len(prefix):]: z[k] for k in z.files if k.startswith(prefix) and k not in ("cfg", "linear_bias", "keys")}
    g["keys"] = [str(k) for k in z["keys"]]
    return cfg, sd, g


def inputs(g):
    """The golden's inputs as the class takes them."""
    t = lambda k: torch.from_numpy(g[k])      # noqa: E731
    return dict(txt_tokens=t("txt_tokens"), pitch_midi=t("pitch_midi"), midi_dur=t("midi_dur"), is_slur=t("is_slur"),
                mel2ph=t("mel2ph_in") if "mel2ph_in" in g else None)


def rel_pos_table(T, dim):
    """RelPositionalEncoding.pe[:T] in fp32: row i holds position max_len - 1 - i."""
    pos = torch.arange(REL_MAX_LEN - 1, -1, -1.0, dtype=torch.float32).unsqueeze(1)
    div = torch.exp(torch.arange(0, dim, 2, dtype=torch.float32) * -(math.log(10000.0) / dim))
    pe = torch.zeros(REL_MAX_LEN, dim)
    pe[:, 0::2] = torch.sin(pos * div)
    pe[:, 1::2] = torch.cos(pos * div)
    return pe[:T]


def masked_attention(q, k, v, heads, alpha, hidden):
    """softmax(alpha q k^T + mask) v per head in the inputs' dtype.  q [B, Nq, heads * dh], k / v [B, Nk, heads * dh], hidden
    [B, Nk] bool (True = the key is hidden from every query of the sample) -> [B, Nq, heads * dh]."""
    B, Nq, Cc = q.shape
    sp = lambda t: t.reshape(B, t.shape[1], heads, Cc // heads).permute(0, 2, 1, 3)      # noqa: E731
    s = torch.matmul(sp(q), sp(k).transpose(-1, -2)) * alpha
    s = s.masked_fill(hidden[:, None, None, :], -math.inf)
    return torch.matmul(torch.softmax(s, dim=-1), sp(v)).permute(0, 2, 1, 3).reshape(B, Nq, Cc)


def fft_blocks(sd, name, x, pad, heads, n_layers, k, dt):
    """FFTBlocks.forward from `x * nonpadding` on (tts_modules.py:320-326).  x [B, T, H], pad [B, T] bool."""
    w = lambda key: sd[key].to(dt)      # noqa: E731
    H = x.shape[-1]
    keep = (~pad).to(dt)[:, :, None]
    x = x * keep
    for i in range(n_layers):
        p = "%s.layers.%d.op." % (name, i)
        y = F.layer_norm(x, (H,), w(p + "layer_norm1.weight"), w(p + "layer_norm1.bias"), EPS)
        q, kk, v = F.linear(y, w(p + "self_attn.in_proj_weight")).chunk(3, dim=-1)
        y = masked_attention(q, kk, v, heads, (H // heads) ** -0.5, pad)
        x = (x + F.linear(y, w(p + "self_attn.out_proj.weight"))) * keep
        y = F.layer_norm(x, (H,), w(p + "layer_norm2.weight"), w(p + "layer_norm2.bias"), EPS)
        y = F.conv1d(y.transpose(1, 2), w(p + "ffn.ffn_1.weight"), w(p + "ffn.ffn_1.bias"), padding=k // 2).transpose(1, 2)
        y = F.gelu(y * k ** -0.5)
        x = (x + F.linear(y, w(p + "ffn.ffn_2.weight"), w(p + "ffn.ffn_2.bias"))) * keep
    return F.layer_norm(x, (H,), w(name + ".layer_norm.weight"), w(name + ".layer_norm.bias"), EPS) * keep


def length_regulate(dur):
    """LengthRegulator.forward: dur [B, T] long -> mel2ph [B, max_b sum(dur)] long."""
    cum = torch.cumsum(dur, 1)
    prev = F.pad(cum, [1, -1])
    pos = torch.arange(int(dur.sum(-1).max()))[None, None]
    mask = (pos >= prev[:, :, None]) & (pos < cum[:, :, None])
    return (torch.arange(1, dur.shape[1] + 1)[None, :, None] * mask.long()).sum(1)


def encode(sd, cfg, txt_tokens, pitch_midi, midi_dur=None, is_slur=None, dtype=torch.float32):
    """The encoder half of forward with the duration predictor -> (encoder_out [B, T, H], xs [B, T], dur_choice [B, T] long) in
    `dtype`."""
    dt = dtype
    w = lambda key: sd[key].to(dt)      # noqa: E731
    H, heads = cfg["hidden_size"], cfg["num_heads"]
    B, T = txt_tokens.shape
    scale = math.sqrt(H)
    x = scale * w("encoder.embed_tokens.weight")[txt_tokens] + w("midi_embed.weight")[pitch_midi]
    if midi_dur is not None:
        x = x + F.linear(midi_dur.to(dt)[:, :, None], w("midi_dur_layer.weight"), w("midi_dur_layer.bias"))
    if is_slur is not None:
        x = x + w("is_slur_embed.weight")[is_slur]
    x = x * scale + rel_pos_table(T, H).to(dt)[None]
    pad = txt_tokens.eq(0)
    enc = fft_blocks(sd, "encoder", x, pad, heads, cfg["enc_layers"], cfg["enc_ffn_kernel_size"], dt)
    xs, dur = durations(sd, cfg, enc, pad, dt)
    return enc, xs, dur


def durations(sd, cfg, enc, pad, dt):
    """DurationPredictor on the encoder states and out2dur -> (xs [B, T], dur_choice [B, T] long) in `dt`; pad [B, T] bool."""
    w = lambda key: sd[key].to(dt)      # noqa: E731
    keep = (~pad).to(dt)
    k = cfg["dur_predictor_kernel"]
    y = (enc * keep[:, :, None]).transpose(1, 2)
    for i in range(cfg["dur_predictor_layers"]):
        p = "dur_predictor.conv.%d." % i
        y = F.relu(F.conv1d(F.pad(y, ((k - 1) // 2, (k - 1) // 2)), w(p + "1.weight"), w(p + "1.bias")))
        y = F.layer_norm(y.transpose(1, 2), (y.shape[1],), w(p + "3.weight"), w(p + "3.bias"), EPS).transpose(1, 2)
        y = y * keep[:, None, :]
    xs = F.linear(y.transpose(1, 2), w("dur_predictor.linear.weight"), w("dur_predictor.linear.bias"))[..., 0] * keep
    dur = torch.clamp(torch.round(xs.exp() - 1.0), min=0).long()
    return xs, dur


def forward(sd, cfg, txt_tokens, pitch_midi, midi_dur=None, is_slur=None, mel2ph=None, dtype=torch.float32):
    """-> dict(encoder_out [B, T, H], xs [B, T], dur_choice [B, T] long, mel2ph [B, T_mel] long, decoder_inp, mel_out) in `dtype`;
    dur_choice and mel2ph come from the prediction when mel2ph is None."""
    dt = dtype
    enc, xs, dur = encode(sd, cfg, txt_tokens, pitch_midi, midi_dur, is_slur, dt)
    if mel2ph is None:
        mel2ph = length_regulate(dur * (~txt_tokens.eq(0)).long())
    out = decode(sd, cfg, enc, mel2ph, dt)
    return dict(encoder_out=enc, xs=xs, dur_choice=dur, mel2ph=out["mel2ph"], decoder_inp=out["decoder_inp"], mel_out=out["mel_out"])


def expand(encoder_out, mel2ph):
    """FastSpeech2.forward's expand and mask (fs2.py:117-122,132): encoder_out [B, T, H], mel2ph [B, T_mel] long -> decoder_inp."""
    H = encoder_out.shape[-1]
    tgt = (mel2ph > 0).to(encoder_out.dtype)[:, :, None]
    return torch.gather(F.pad(encoder_out, [0, 0, 1, 0]), 1, mel2ph[..., None].repeat(1, 1, H)) * tgt


def run_decoder(sd, cfg, decoder_inp, mel2ph, dtype=torch.float32):
    """FastSpeech2.run_decoder (fs2.py:222-226): decoder_inp [B, T_mel, H] (an all-zero row is padding), mel2ph [B, T_mel] ->
    mel_out [B, T_mel, mel bins] in `dtype`."""
    dt = dtype
    w = lambda key: sd[key].to(dt)      # noqa: E731
    H = cfg["hidden_size"]
    dec_inp = decoder_inp.to(dt)
    tgt = (mel2ph > 0).to(dt)[:, :, None]
    dpad = dec_inp.abs().sum(-1).eq(0)
    Tm = dec_inp.shape[1]
    tab = P.sinusoid_table(max(2000, Tm + 1), H).to(dt)
    x = dec_inp + w("decoder.pos_embed_alpha") * tab[P.make_positions(dec_inp[..., 0])]
    x = fft_blocks(sd, "decoder", x, dpad, cfg["num_heads"], cfg["dec_layers"], cfg["dec_ffn_kernel_size"], dt)
    return F.linear(x, w("mel_out.weight"), w("mel_out.bias")) * tgt


def decode(sd, cfg, encoder_out, mel2ph, dtype=torch.float32):
    """The decoder half of forward: encoder_out [B, T, H], mel2ph [B, T_mel] -> dict(mel2ph long, decoder_inp, mel_out) in
    `dtype`."""
    mel2ph = mel2ph.long()
    dec_inp = expand(encoder_out.to(dtype), mel2ph)
    return dict(mel2ph=mel2ph, decoder_inp=dec_inp, mel_out=run_decoder(sd, cfg, dec_inp, mel2ph, dtype))


# ---- the masked-attention operator test (tests/test_gpu_fs2.py): float64 reference and seeded inputs, heads = 2, dh = 128

OP_HEADS, OP_DH = 2, 128


def op_hidden(B, N, case):
    """The key masks of the operator test, [B, N] bool (True = hidden)."""
    h = torch.zeros(B, N, dtype=torch.bool)
    if case == "none":
        pass
    elif case == "last2":
        h[:, -2:] = True
    elif case == "tail_sample1":
        h[1, 20:] = True
    elif case == "first32":
        h[:, :32] = True
    elif case == "interior_and_tail":
        h[:, 40:75] = True          # covers tile 2 (keys 64 .. 95) only in part, tile 1 from its middle
        h[:, 120:] = True
        h[0, 32:64] = True          # sample 0 alone loses the whole of tile 1
    else:
        raise KeyError(case)
    return h


# (Nq = Nk, B, mask)
OP_SHAPES = ((1, 1, "none"), (5, 1, "last2"), (33, 2, "tail_sample1"), (70, 2, "first32"), (129, 2, "interior_and_tail"))


def op_inputs(N, B, case):
    """The seeded inputs of one operator case: q, k, v [B, N, heads, dh] fp32 (heads told apart as attn_ref.random_qkv does) and
    its key mask."""
    q, k, v = A.random_qkv(B, OP_HEADS, OP_DH, N, N, 100 + N, distinct_heads=True)
    return q, k, v, op_hidden(B, N, case)


def masked_attention_ref(q, k, v, heads, alpha, hidden):
    """float64; q / k / v [B, N, heads, dh] as tests/attn_ref.py lays them out -> [B, Nq, heads, dh]."""
    B, Nq = q.shape[:2]
    f = lambda t: t.detach().to("cpu", torch.float64).reshape(B, t.shape[1], -1)      # noqa: E731
    return masked_attention(f(q), f(k), f(v), heads, float(alpha), hidden).reshape(B, Nq, heads, -1)


def sharp_hidden_qkv(B, heads, dh, L, alpha, seed):
    """Built like attn_ref.causal_qkv(kind="next"): keys are c times random unit vectors, alpha c^2 = 20 nats, and query i is c
    times the direction of the odd key next to it (i | 1, the last odd key for the last query).  Every odd key is hidden, so
    EVERY query points at a hidden key; v rows alternate in sign with the key index, so the visible keys are all positive and
    admitting one hidden key is an error of the size of the tensor's range at that row.  -> q, k, v, hidden [B, L] bool."""
    assert L >= 2
    c = math.sqrt(A.CAUSAL_NATS / alpha)
    u = torch.randn(B, L, heads, dh, generator=A.gen(seed), dtype=torch.float64)
    u = u / u.norm(dim=-1, keepdim=True)
    i = torch.arange(L)
    last_odd = L - 1 if (L - 1) % 2 == 1 else L - 2
    t = (i | 1).clamp_max(last_odd)
    sign = (1.0 - 2.0 * (i % 2)).to(torch.float32)[None, :, None, None]
    v = sign * (1.0 + i.to(torch.float32)[None, :, None, None] / L) + 0.25 * torch.randn(B, L, heads, dh, generator=A.gen(seed + 1))
    hidden = torch.zeros(B, L, dtype=torch.bool)
    hidden[:, 1::2] = True
    return (c * u[:, t]).to(torch.float32), (c * u).to(torch.float32), v, hidden
