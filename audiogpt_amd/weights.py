"""Seeded random-weight factory and checkpoint helpers, in the reference state_dict key layout.

No checkpoints ship with the reference (download.sh fetches them), and a randomly initialised
reference UNet outputs exactly 0 because of `zero_module` (openaimodel.py:229-231,312,686;
attention.py:244-248).  The factory therefore draws EVERY tensor, including the zero-init ones,
from a seeded generator, and emits the key names a real checkpoint has so the
same loader serves real weights later:

  UNet      `model.diffusion_model.`-relative keys  (openaimodel.py:516-693)
  VAE       `first_stage_model.`-relative keys      (model.py:368-533, autoencoder.py:318-324)
  HiFi-GAN  `conv_pre.weight_g/_v`, `ups.{i}.*`, `resblocks.{n}.convs{1,2}.{j}.*`, `conv_post.*`
            (NeuralSeq/modules/hifigan/hifigan.py:104-142)
  BigVGAN   as HiFi-GAN with `ups.{i}.0.*` and `resblocks.{n}.activations.{m}.act.{alpha,beta}`,
            `activation_post.act.*` (bigvgan/models.py:133-179)
"""
import math

import torch


class _Gen:
    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)

    def normal(self, shape, std):
        return torch.randn(shape, generator=self.g, dtype=torch.float32) * std

    def weight(self, shape, gain=1.0):
        fan_in = 1
        for s in shape[1:]:
            fan_in *= s
        return self.normal(shape, gain / math.sqrt(fan_in))

    def bias(self, n):
        return self.normal((n,), 0.05)

    def gamma(self, n):
        return 1.0 + self.normal((n,), 0.1)

    def beta(self, n):
        return self.normal((n,), 0.1)


# ----------------------------------------------------------------------------- UNet
def unet_layers(cfg):
    """Block structure of the reference UNet constructor (openaimodel.py:516-693).

    Returns (input_blocks, middle_block, output_blocks); each block is a list of layers:
    ("conv",cin,cout) ("res",cin,cout,updown) ("st",ch,heads,dim_head) ("attn",ch,heads)
    ("down",ch) ("up",ch).
    """
    mc, mult, nrb = cfg["model_channels"], cfg["channel_mult"], cfg["num_res_blocks"]
    st, nhc = cfg["use_spatial_transformer"], cfg["num_head_channels"]
    state = {"heads": cfg["num_heads"]}

    def attn(ch):
        if nhc == -1:
            heads, dh = state["heads"], ch // state["heads"]
        else:
            heads, dh = ch // nhc, nhc
            state["heads"] = heads
        if cfg["legacy"]:
            dh = ch // heads if st else nhc
        if st:
            return ("st", ch, heads, dh)
        return ("attn", ch, heads if dh == -1 else ch // dh)

    inp, chans, ch, ds = [[("conv", cfg["in_channels"], mc)]], [mc], mc, 1
    for level, m in enumerate(mult):
        for _ in range(nrb):
            blk = [("res", ch, m * mc, None)]
            ch = m * mc
            if ds in cfg["attention_resolutions"]:
                blk.append(attn(ch))
            inp.append(blk)
            chans.append(ch)
        if level != len(mult) - 1:
            inp.append([("res", ch, ch, "down")] if cfg["resblock_updown"] else [("down", ch)])
            chans.append(ch)
            ds *= 2
    mid = [("res", ch, ch, None), attn(ch), ("res", ch, ch, None)]
    out = []
    for level, m in list(enumerate(mult))[::-1]:
        for i in range(nrb + 1):
            ich = chans.pop()
            blk = [("res", ch + ich, mc * m, None)]
            ch = mc * m
            if ds in cfg["attention_resolutions"]:
                blk.append(attn(ch))
            if level and i == nrb:
                blk.append(("res", ch, ch, "up") if cfg["resblock_updown"] else ("up", ch))
                ds //= 2
            out.append(blk)
    return inp, mid, out


def _unet_layer_tensors(sd, g, p, layer, cfg, emb_dim):
    kind = layer[0]
    if kind == "conv":
        sd[p + "weight"] = g.weight((layer[2], layer[1], 3, 3))
        sd[p + "bias"] = g.bias(layer[2])
    elif kind == "res":
        cin, cout = layer[1], layer[2]
        sd[p + "in_layers.0.weight"], sd[p + "in_layers.0.bias"] = g.gamma(cin), g.beta(cin)
        sd[p + "in_layers.2.weight"], sd[p + "in_layers.2.bias"] = g.weight((cout, cin, 3, 3)), g.bias(cout)
        sd[p + "emb_layers.1.weight"], sd[p + "emb_layers.1.bias"] = g.weight((cout, emb_dim)), g.bias(cout)
        sd[p + "out_layers.0.weight"], sd[p + "out_layers.0.bias"] = g.gamma(cout), g.beta(cout)
        sd[p + "out_layers.3.weight"], sd[p + "out_layers.3.bias"] = g.weight((cout, cout, 3, 3), 0.5), g.bias(cout)
        if cin != cout:
            sd[p + "skip_connection.weight"] = g.weight((cout, cin, 1, 1))
            sd[p + "skip_connection.bias"] = g.bias(cout)
    elif kind == "st":
        ch, heads, dh = layer[1], layer[2], layer[3]
        inner = heads * dh
        ctx = cfg["context_dim"]
        sd[p + "norm.weight"], sd[p + "norm.bias"] = g.gamma(ch), g.beta(ch)
        sd[p + "proj_in.weight"], sd[p + "proj_in.bias"] = g.weight((inner, ch, 1, 1)), g.bias(inner)
        for d in range(cfg.get("transformer_depth", 1)):
            t = p + f"transformer_blocks.{d}."
            for name, kdim in (("attn1", inner), ("attn2", ctx)):
                sd[t + name + ".to_q.weight"] = g.weight((inner, inner))
                sd[t + name + ".to_k.weight"] = g.weight((inner, kdim))
                sd[t + name + ".to_v.weight"] = g.weight((inner, kdim))
                sd[t + name + ".to_out.0.weight"] = g.weight((inner, inner), 0.5)
                sd[t + name + ".to_out.0.bias"] = g.bias(inner)
            sd[t + "ff.net.0.proj.weight"] = g.weight((inner * 8, inner))
            sd[t + "ff.net.0.proj.bias"] = g.bias(inner * 8)
            sd[t + "ff.net.2.weight"] = g.weight((inner, inner * 4), 0.5)
            sd[t + "ff.net.2.bias"] = g.bias(inner)
            for n in (1, 2, 3):
                sd[t + f"norm{n}.weight"], sd[t + f"norm{n}.bias"] = g.gamma(inner), g.beta(inner)
        sd[p + "proj_out.weight"], sd[p + "proj_out.bias"] = g.weight((ch, inner, 1, 1), 0.5), g.bias(ch)
    elif kind == "attn":
        ch = layer[1]
        sd[p + "norm.weight"], sd[p + "norm.bias"] = g.gamma(ch), g.beta(ch)
        sd[p + "qkv.weight"], sd[p + "qkv.bias"] = g.weight((3 * ch, ch, 1)), g.bias(3 * ch)
        sd[p + "proj_out.weight"], sd[p + "proj_out.bias"] = g.weight((ch, ch, 1), 0.5), g.bias(ch)
    elif kind == "down":
        ch = layer[1]
        sd[p + "op.weight"], sd[p + "op.bias"] = g.weight((ch, ch, 3, 3)), g.bias(ch)
    elif kind == "up":
        ch = layer[1]
        sd[p + "conv.weight"], sd[p + "conv.bias"] = g.weight((ch, ch, 3, 3)), g.bias(ch)
    else:
        raise ValueError(kind)


def make_unet_state_dict(cfg, seed=0):
    g = _Gen(seed)
    mc = cfg["model_channels"]
    emb = mc * 4
    sd = {}
    sd["time_embed.0.weight"], sd["time_embed.0.bias"] = g.weight((emb, mc)), g.bias(emb)
    sd["time_embed.2.weight"], sd["time_embed.2.bias"] = g.weight((emb, emb)), g.bias(emb)
    inp, mid, out = unet_layers(cfg)
    for i, blk in enumerate(inp):
        for j, layer in enumerate(blk):
            _unet_layer_tensors(sd, g, f"input_blocks.{i}.{j}.", layer, cfg, emb)
    for j, layer in enumerate(mid):
        _unet_layer_tensors(sd, g, f"middle_block.{j}.", layer, cfg, emb)
    for i, blk in enumerate(out):
        for j, layer in enumerate(blk):
            _unet_layer_tensors(sd, g, f"output_blocks.{i}.{j}.", layer, cfg, emb)
    sd["out.0.weight"], sd["out.0.bias"] = g.gamma(mc), g.beta(mc)
    sd["out.2.weight"] = g.weight((cfg["out_channels"], mc, 3, 3))
    sd["out.2.bias"] = g.bias(cfg["out_channels"])
    return sd


# ----------------------------------------------------------------------------- VAE
def _vae_res(sd, g, p, cin, cout):
    sd[p + "norm1.weight"], sd[p + "norm1.bias"] = g.gamma(cin), g.beta(cin)
    sd[p + "conv1.weight"], sd[p + "conv1.bias"] = g.weight((cout, cin, 3, 3)), g.bias(cout)
    sd[p + "norm2.weight"], sd[p + "norm2.bias"] = g.gamma(cout), g.beta(cout)
    sd[p + "conv2.weight"], sd[p + "conv2.bias"] = g.weight((cout, cout, 3, 3), 0.5), g.bias(cout)
    if cin != cout:
        sd[p + "nin_shortcut.weight"] = g.weight((cout, cin, 1, 1))
        sd[p + "nin_shortcut.bias"] = g.bias(cout)


def _vae_attn(sd, g, p, c):
    sd[p + "norm.weight"], sd[p + "norm.bias"] = g.gamma(c), g.beta(c)
    for n in ("q", "k", "v"):
        sd[p + n + ".weight"], sd[p + n + ".bias"] = g.weight((c, c, 1, 1)), g.bias(c)
    sd[p + "proj_out.weight"], sd[p + "proj_out.bias"] = g.weight((c, c, 1, 1), 0.5), g.bias(c)


def make_vae_state_dict(dd, seed=1, with_encoder=True):
    """Keys relative to `first_stage_model.`: decoder.*, encoder.*, quant_conv.*, post_quant_conv.*"""
    g = _Gen(seed)
    sd = {}
    ch, mult, nrb = dd["ch"], dd["ch_mult"], dd["num_res_blocks"]
    nres = len(mult)
    zc, ed = dd["z_channels"], dd["embed_dim"]
    # ---- decoder (model.py:462-533)
    p = "decoder."
    block_in = ch * mult[-1]
    curr = dd["resolution"] // 2 ** (nres - 1)
    sd[p + "conv_in.weight"], sd[p + "conv_in.bias"] = g.weight((block_in, zc, 3, 3)), g.bias(block_in)
    _vae_res(sd, g, p + "mid.block_1.", block_in, block_in)
    _vae_attn(sd, g, p + "mid.attn_1.", block_in)
    _vae_res(sd, g, p + "mid.block_2.", block_in, block_in)
    for lvl in reversed(range(nres)):
        block_out = ch * mult[lvl]
        for ib in range(nrb + 1):
            _vae_res(sd, g, p + f"up.{lvl}.block.{ib}.", block_in, block_out)
            block_in = block_out
            if curr in dd["attn_resolutions"]:
                _vae_attn(sd, g, p + f"up.{lvl}.attn.{ib}.", block_in)
        if lvl != 0:
            sd[p + f"up.{lvl}.upsample.conv.weight"] = g.weight((block_in, block_in, 3, 3))
            sd[p + f"up.{lvl}.upsample.conv.bias"] = g.bias(block_in)
            curr *= 2
    sd[p + "norm_out.weight"], sd[p + "norm_out.bias"] = g.gamma(block_in), g.beta(block_in)
    sd[p + "conv_out.weight"] = g.weight((dd["out_ch"], block_in, 3, 3))
    sd[p + "conv_out.bias"] = g.bias(dd["out_ch"])
    sd["post_quant_conv.weight"], sd["post_quant_conv.bias"] = g.weight((zc, ed, 1, 1)), g.bias(zc)
    if not with_encoder:
        return sd
    # ---- encoder (model.py:368-432)
    p = "encoder."
    in_mult = (1,) + tuple(mult)
    curr = dd["resolution"]
    sd[p + "conv_in.weight"], sd[p + "conv_in.bias"] = g.weight((ch, dd["in_channels"], 3, 3)), g.bias(ch)
    for lvl in range(nres):
        block_in = ch * in_mult[lvl]
        block_out = ch * mult[lvl]
        for ib in range(nrb):
            _vae_res(sd, g, p + f"down.{lvl}.block.{ib}.", block_in, block_out)
            block_in = block_out
            if curr in dd["attn_resolutions"]:
                _vae_attn(sd, g, p + f"down.{lvl}.attn.{ib}.", block_in)
        if lvl != nres - 1:
            sd[p + f"down.{lvl}.downsample.conv.weight"] = g.weight((block_in, block_in, 3, 3))
            sd[p + f"down.{lvl}.downsample.conv.bias"] = g.bias(block_in)
            curr //= 2
    _vae_res(sd, g, p + "mid.block_1.", block_in, block_in)
    _vae_attn(sd, g, p + "mid.attn_1.", block_in)
    _vae_res(sd, g, p + "mid.block_2.", block_in, block_in)
    sd[p + "norm_out.weight"], sd[p + "norm_out.bias"] = g.gamma(block_in), g.beta(block_in)
    oc = 2 * zc if dd["double_z"] else zc
    sd[p + "conv_out.weight"], sd[p + "conv_out.bias"] = g.weight((oc, block_in, 3, 3)), g.bias(oc)
    sd["quant_conv.weight"], sd["quant_conv.bias"] = g.weight((2 * ed, oc, 1, 1)), g.bias(2 * ed)
    return sd


# ----------------------------------------------------------------------------- vocoders
def _wn(sd, g, name, shape, gain=1.0, transpose=False):
    """Emit a weight-norm pair the way torch.nn.utils.weight_norm stores it (dim=0)."""
    # Conv1d weight is [Cout, Cin, k]; ConvTranspose1d weight is [Cin, Cout, k] (dim 0 = in-channels)
    fan = (shape[0] if transpose else shape[1]) * shape[2]
    target = gain / math.sqrt(fan)            # element std wanted for the folded weight
    v = g.normal(shape, 1.0)
    per_row = math.sqrt(shape[1] * shape[2])  # ~ ||v|| over dims != 0
    # g such that g*v/||v|| has element std ~= target, with a seeded +-20 % spread per dim-0 row
    sd[name + ".weight_g"] = (target * per_row) * (1.0 + g.normal((shape[0], 1, 1), 0.2)).abs()
    sd[name + ".weight_v"] = v


def make_vocoder_state_dict(cfg, seed=2):
    g = _Gen(seed)
    sd = {}
    uic = cfg["upsample_initial_channel"]
    big = cfg["kind"] == "bigvgan"
    _wn(sd, g, "conv_pre", (uic, cfg["num_mels"], 7))
    sd["conv_pre.bias"] = g.bias(uic)

    def snake_param(n):
        # activations.py:29-34,83-90: log-scale parameters start at 0, linear ones at 1 (1 / alpha must stay bounded)
        if cfg.get("snake_logscale", False):
            return g.normal((n,), 0.3)
        return (1.0 + g.normal((n,), 0.2)).clamp(min=0.4)

    nk = len(cfg["resblock_kernel_sizes"])
    ch = uic
    for i, (u, k) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
        cin, cout = uic // 2 ** i, uic // 2 ** (i + 1)
        name = f"ups.{i}.0" if big else f"ups.{i}"
        # each output sample sees k/u taps of cin channels
        _wn(sd, g, name, (cin, cout, k), gain=math.sqrt(u), transpose=True)
        sd[name + ".bias"] = g.bias(cout)
        ch = cout
        for j, (rk, rd) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"])):
            p = f"resblocks.{i * nk + j}."
            rb2 = str(cfg.get("resblock", "1")) != "1"          # ResBlock2 / AMPBlock2: one conv (and one activation) per dilation
            for m in range(len(rd)):
                if rb2:
                    _wn(sd, g, p + f"convs.{m}", (ch, ch, rk), gain=0.6)
                    sd[p + f"convs.{m}.bias"] = g.bias(ch)
                    continue
                _wn(sd, g, p + f"convs1.{m}", (ch, ch, rk), gain=1.0)
                sd[p + f"convs1.{m}.bias"] = g.bias(ch)
                _wn(sd, g, p + f"convs2.{m}", (ch, ch, rk), gain=0.4)
                sd[p + f"convs2.{m}.bias"] = g.bias(ch)
            if big:
                for m in range((1 if rb2 else 2) * len(rd)):
                    sd[p + f"activations.{m}.act.alpha"] = snake_param(ch)
                    if cfg["activation"] == "snakebeta":
                        sd[p + f"activations.{m}.act.beta"] = snake_param(ch)
    if big:
        sd["activation_post.act.alpha"] = snake_param(ch)
        if cfg["activation"] == "snakebeta":
            sd["activation_post.act.beta"] = snake_param(ch)
    _wn(sd, g, "conv_post", (1, ch, 7), gain=0.3)
    sd["conv_post.bias"] = g.bias(1)
    if cfg.get("use_pitch_embed"):
        # NSF branch (hifigan.py:111-132): harmonic merge Linear(9 -> 1) and one plain Conv1d per stage
        sd["m_source.l_linear.weight"] = g.normal((1, 9), 0.6)
        sd["m_source.l_linear.bias"] = g.bias(1)
        rates = cfg["upsample_rates"]
        for i in range(len(rates)):
            c_cur = uic // 2 ** (i + 1)
            if i + 1 < len(rates):
                s_f0 = 1
                for r in rates[i + 1:]:
                    s_f0 *= r
                kk = 2 * s_f0
            else:
                kk = 1
            sd[f"noise_convs.{i}.weight"] = g.normal((c_cur, 1, kk), 1.0 / math.sqrt(kk))
            sd[f"noise_convs.{i}.bias"] = g.bias(c_cur)
    return sd


def make_diffnet_state_dict(cfg, seed=7):
    """DiffNet (NeuralSeq/modules/diff/net.py:84-105) in the reference key layout; the zero-initialised
    output_projection (:105) is re-randomised like the UNet's zero modules."""
    g = _Gen(seed)
    C, H, M = cfg["residual_channels"], cfg["hidden_size"], cfg["in_dims"]
    sd = {"input_projection.weight": g.normal((C, M, 1), 1.0 / math.sqrt(M)), "input_projection.bias": g.bias(C),
          "mlp.0.weight": g.normal((4 * C, C), 1.0 / math.sqrt(C)), "mlp.0.bias": g.bias(4 * C),
          "mlp.2.weight": g.normal((C, 4 * C), 1.0 / math.sqrt(4 * C)), "mlp.2.bias": g.bias(C)}
    for i in range(cfg["residual_layers"]):
        p = f"residual_layers.{i}."
        sd[p + "dilated_conv.weight"] = g.normal((2 * C, C, 3), 1.0 / math.sqrt(3 * C))
        sd[p + "dilated_conv.bias"] = g.bias(2 * C)
        sd[p + "diffusion_projection.weight"] = g.normal((C, C), 1.0 / math.sqrt(C))
        sd[p + "diffusion_projection.bias"] = g.bias(C)
        sd[p + "conditioner_projection.weight"] = g.normal((2 * C, H, 1), 1.0 / math.sqrt(H))
        sd[p + "conditioner_projection.bias"] = g.bias(2 * C)
        sd[p + "output_projection.weight"] = g.normal((2 * C, C, 1), 1.0 / math.sqrt(C))
        sd[p + "output_projection.bias"] = g.bias(2 * C)
    sd["skip_projection.weight"] = g.normal((C, C, 1), 1.0 / math.sqrt(C))
    sd["skip_projection.bias"] = g.bias(C)
    sd["output_projection.weight"] = g.normal((M, C, 1), 1.0 / math.sqrt(C))
    sd["output_projection.bias"] = g.bias(M)
    return sd


def make_pe_state_dict(cfg, seed=13):
    """PitchExtractor (NeuralSeq/modules/fastspeech/pe.py:119-133) in the reference key layout, bookkeeping entries included
    (BatchNorm's num_batches_tracked, embed_positions._float_tensor): 59 keys at the defaults.  The BatchNorm running
    statistics and affine and pos_embed_alpha are drawn away from their initial values, so a loader that skipped them shows."""
    g, sd = _Gen(seed), {}
    H, M, k = cfg["hidden_size"], cfg["n_mel_bins"], 5
    Cp = cfg["predictor_hidden"] if cfg["predictor_hidden"] > 0 else H
    kp = cfg["predictor_kernel"]
    for i in range(3):
        p, cin = f"mel_prenet.layers.{i}.", (M if i == 0 else H)
        sd[p + "0.weight"], sd[p + "0.bias"] = g.weight((H, cin, k), 1.4), g.bias(H)
        sd[p + "2.weight"], sd[p + "2.bias"] = g.gamma(H), g.beta(H)
        sd[p + "2.running_mean"] = 0.3 + g.normal((H,), 0.3)
        sd[p + "2.running_var"] = 0.5 + torch.rand((H,), generator=g.g, dtype=torch.float32)
        sd[p + "2.num_batches_tracked"] = torch.tensor(1000 + i, dtype=torch.long)
    sd["mel_prenet.out_proj.weight"], sd["mel_prenet.out_proj.bias"] = g.weight((H, H)), g.bias(H)
    if cfg["conv_layers"] > 0:
        sd["mel_encoder.in_proj.weight"], sd["mel_encoder.in_proj.bias"] = g.weight((H, H)), g.bias(H)
        for i in range(cfg["conv_layers"]):
            p = f"mel_encoder.conv.{i}."
            sd[p + "conv.conv.weight"], sd[p + "conv.conv.bias"] = g.weight((H, H, k)), g.bias(H)
            sd[p + "norm.weight"], sd[p + "norm.bias"] = g.gamma(H), g.beta(H)
        sd["mel_encoder.out_proj.weight"], sd["mel_encoder.out_proj.bias"] = g.weight((H, H)), g.bias(H)
    for i in range(5):
        p, cin = f"pitch_predictor.conv.{i}.", (H if i == 0 else Cp)
        sd[p + "1.weight"], sd[p + "1.bias"] = g.weight((Cp, cin, kp), 1.4), g.bias(Cp)
        sd[p + "3.weight"], sd[p + "3.bias"] = g.gamma(Cp), g.beta(Cp)
    sd["pitch_predictor.linear.weight"], sd["pitch_predictor.linear.bias"] = g.weight((2, Cp)), g.bias(2)
    sd["pitch_predictor.embed_positions._float_tensor"] = torch.zeros(1, dtype=torch.float32)
    sd["pitch_predictor.pos_embed_alpha"] = torch.tensor([0.7], dtype=torch.float32)
    return sd


def _invconv_near(g, n_split=4):
    """InvConvNear's tensors as its constructor makes them (glow_modules.py:123-143): a random orthogonal matrix with a positive
    determinant, LU-decomposed with partial pivoting -- drawn again until the permutation is not the identity and sign_s has both
    signs, so a loader that skipped either shows.  log_s is moved off the decomposition's (whose sum is 0 for an orthogonal
    matrix), so the log-determinant term is not vacuous."""
    while True:
        q = torch.linalg.qr(g.normal((n_split, n_split), 1.0).double())[0]
        if torch.det(q) < 0:
            q[:, 0] = -q[:, 0]
        lu, piv = torch.linalg.lu_factor(q)
        p, l, u = torch.lu_unpack(lu, piv)
        s = torch.diagonal(u)
        sign = torch.sign(s)
        if not torch.equal(p, torch.eye(n_split, dtype=p.dtype)) and sign.min() < 0 < sign.max():
            break
    f = torch.float32
    return {"l": l.to(f), "log_s": (torch.log(s.abs()).to(f) + g.normal((n_split,), 0.1)), "u": torch.triu(u, 1).to(f), "p": p.to(f),
            "sign_s": sign.to(f), "l_mask": torch.tril(torch.ones(n_split, n_split), -1), "eye": torch.eye(n_split)}


def make_glow_state_dict(cfg, seed=23, coupling_gain=1.0):
    """The Glow post-net (NeuralSeq/modules/GenerSpeech/model/glow_modules.py:496-554) in the reference key layout: 35 keys per
    block at GenerSpeech's configuration (280 in all; 420 at PortaSpeech's), convolutions as weight-norm pairs, InvConvNear's
    l / log_s / u / p / sign_s / l_mask / eye, and with share_wn_layers = n the group's in_layers / res_skip_layers repeated under
    every member's keys (the same tensors).  What the reference initialises to nothing is drawn: `end` (zero at init, which makes
    every coupling the identity) and ActNorm's logs / bias.  coupling_gain scales those draws (the couplings' amplification
    compounds over the blocks)."""
    g, sd = _Gen(seed), {}
    C, H, k, L = cfg["in_channels"], cfg["hidden_channels"], cfg["kernel_size"], cfg["n_layers"]
    gin, share, share_cond = cfg["gin_channels"], cfg["share_wn_layers"], bool(cfg["share_cond_layers"])
    if gin and share_cond:
        sd["cond_layer.bias"] = g.bias(2 * H * L)
        _wn(sd, g, "cond_layer", (2 * H * L, 2 * gin, 1))
    wn = None
    for b in range(cfg["n_blocks"]):
        pa, pi, pc = "flows.%d." % (3 * b), "flows.%d." % (3 * b + 1), "flows.%d." % (3 * b + 2)
        sd[pa + "logs"] = g.normal((1, 2 * C, 1), 0.1 * coupling_gain)
        sd[pa + "bias"] = g.normal((1, 2 * C, 1), 0.1)
        for name, t in _invconv_near(g).items():
            sd[pi + name] = t
        sd[pc + "start.bias"] = g.bias(H)
        _wn(sd, g, pc + "start", (H, C, 1))
        sd[pc + "end.weight"] = g.normal((2 * C, H, 1), 0.3 * coupling_gain / math.sqrt(H))
        sd[pc + "end.bias"] = g.normal((2 * C,), 0.05 * coupling_gain)
        if wn is None or share <= 0 or b % share == 0:
            wn = {}
            for i in range(L):
                wn["in_layers.%d.bias" % i] = g.bias(2 * H)
                _wn(wn, g, "in_layers.%d" % i, (2 * H, H, k))
            for i in range(L):
                n_out = 2 * H if i < L - 1 else H
                wn["res_skip_layers.%d.bias" % i] = g.bias(n_out)
                _wn(wn, g, "res_skip_layers.%d" % i, (n_out, H, 1))
        for name, t in wn.items():
            sd[pc + "wn." + name] = t
        if gin and not share_cond:
            sd[pc + "wn.cond_layer.bias"] = g.bias(2 * H * L)
            _wn(sd, g, pc + "wn.cond_layer", (2 * H * L, 2 * gin, 1))
    return sd


def make_fs2_state_dict(cfg, seed=17):
    """FastSpeech2MIDI (NeuralSeq/modules/diffsinger_midi/fs2.py:46-53 over modules/fastspeech/fs2.py:22-55) in the reference key
    layout and order: 116 keys at config.FASTSPEECH2_MIDI, the shared `encoder_embed_tokens.weight` / `encoder.embed_tokens.weight`
    (one tensor) and the `decoder.embed_positions._float_tensor` bookkeeping entry included.  The LayerNorm affines are drawn away
    from 1 / 0 (the LayerNorm of a zero padding row is its bias, which leaks into live rows through the FFN convolution) and
    decoder.pos_embed_alpha away from 1, so a port that skipped either shows.  Row 0 of the token and MIDI tables is the padding
    row and is zero, as nn.Embedding(padding_idx = 0) keeps it.  With cfg['use_pitch_embed'] (config.FASTSPEECH2_MIDI_CASCADE) the
    25 keys of the pitch branch are added (pitch_embed, pitch_predictor: 141 keys); every other tensor is the same with and without
    it, for every seed."""
    g, sd = _Gen(seed), {}
    H, V, M = cfg["hidden_size"], cfg["vocab_size"], cfg["audio_num_mel_bins"]
    Cp = cfg["predictor_hidden"] if cfg["predictor_hidden"] > 0 else H
    kd = cfg["dur_predictor_kernel"]

    def table(rows, pad):
        w = g.normal((rows, H), H ** -0.5)
        if pad:
            w[0] = 0.0
        return w

    def fft(name, n_layers, k):
        for i in range(n_layers):
            p = f"{name}.layers.{i}.op."
            sd[p + "layer_norm1.weight"], sd[p + "layer_norm1.bias"] = g.gamma(H), g.beta(H)
            sd[p + "self_attn.in_proj_weight"] = g.weight((3 * H, H), 1.4)
            sd[p + "self_attn.out_proj.weight"] = g.weight((H, H))
            sd[p + "layer_norm2.weight"], sd[p + "layer_norm2.bias"] = g.gamma(H), g.beta(H)
            sd[p + "ffn.ffn_1.weight"], sd[p + "ffn.ffn_1.bias"] = g.weight((4 * H, H, k), 1.4), g.bias(4 * H)
            sd[p + "ffn.ffn_2.weight"], sd[p + "ffn.ffn_2.bias"] = g.weight((H, 4 * H)), g.bias(H)
        sd[f"{name}.layer_norm.weight"], sd[f"{name}.layer_norm.bias"] = g.gamma(H), g.beta(H)

    sd["encoder_embed_tokens.weight"] = table(V, True)
    sd["decoder.pos_embed_alpha"] = torch.tensor([0.8], dtype=torch.float32)
    sd["decoder.embed_positions._float_tensor"] = torch.zeros(1, dtype=torch.float32)
    fft("decoder", cfg["dec_layers"], cfg["dec_ffn_kernel_size"])
    sd["mel_out.weight"], sd["mel_out.bias"] = g.weight((M, H)), g.bias(M)
    for i in range(cfg["dur_predictor_layers"]):
        p, cin = f"dur_predictor.conv.{i}.", (H if i == 0 else Cp)
        sd[p + "1.weight"], sd[p + "1.bias"] = g.weight((Cp, cin, kd), 1.4), g.bias(Cp)
        sd[p + "3.weight"], sd[p + "3.bias"] = g.gamma(Cp), g.beta(Cp)
    sd["dur_predictor.linear.weight"], sd["dur_predictor.linear.bias"] = g.weight((1, Cp)), g.bias(1)
    fft("encoder", cfg["enc_layers"], cfg["enc_ffn_kernel_size"])
    sd["encoder.embed_tokens.weight"] = sd["encoder_embed_tokens.weight"]
    sd["midi_embed.weight"] = table(300, True)
    sd["midi_dur_layer.weight"], sd["midi_dur_layer.bias"] = g.weight((H, 1)), g.bias(H)
    sd["is_slur_embed.weight"] = table(2, False)
    if not cfg.get("use_pitch_embed"):
        return sd
    # The pitch branch (fs2.py:56-64): drawn AFTER everything above, so the tensors above are the same with and without it, then
    # put where the reference's state_dict() has them, between dur_predictor and encoder.  pitch_embed's row 0 is its padding row.
    kp, pitch = cfg.get("predictor_kernel", 5), {}
    pitch["pitch_embed.weight"] = table(300, True)
    pitch["pitch_predictor.pos_embed_alpha"] = torch.tensor([0.7], dtype=torch.float32)
    for i in range(cfg.get("predictor_layers", 5)):
        p, cin = f"pitch_predictor.conv.{i}.", (H if i == 0 else Cp)
        pitch[p + "1.weight"], pitch[p + "1.bias"] = g.weight((Cp, cin, kp), 1.4), g.bias(Cp)
        pitch[p + "3.weight"], pitch[p + "3.bias"] = g.gamma(Cp), g.beta(Cp)
    n_out = 2 if cfg.get("pitch_type", "frame") == "frame" else 1
    pitch["pitch_predictor.linear.weight"], pitch["pitch_predictor.linear.bias"] = g.weight((n_out, Cp)), g.bias(n_out)
    pitch["pitch_predictor.embed_positions._float_tensor"] = torch.zeros(1, dtype=torch.float32)
    out = {}
    for k, v in sd.items():
        out[k] = v
        if k == "dur_predictor.linear.bias":
            out.update(pitch)
    return out


def make_fs2_plain_state_dict(cfg, seed=19):
    """The plain FastSpeech2 (NeuralSeq/modules/fastspeech/fs2.py:22-72) in the reference key layout and order, bookkeeping
    entries included: encoder_embed_tokens, encoder (its `embed_positions._float_tensor` without rel_pos), decoder, mel_out,
    spk_embed_proj / spk_embed_f0 / spk_embed_dur (by use_spk_id / use_split_spk_id / use_spk_embed), dur_predictor, pitch_embed and
    pitch_predictor (use_pitch_embed), energy_embed and energy_predictor (use_energy_embed): 130 keys at config.FASTSPEECH2 with
    energy and split speaker ids.  Drawn as make_fs2_state_dict draws: LayerNorm affines away from 1 / 0, the pos_embed_alphas away
    from 1, row 0 of the token, pitch and energy tables zero (nn.Embedding(padding_idx = 0)); the speaker tables have no padding
    row.  The optional branches are drawn after everything else, so the shared tensors do not depend on the flags."""
    g, sd = _Gen(seed), {}
    H, V, M = cfg["hidden_size"], cfg["vocab_size"], cfg["audio_num_mel_bins"]
    Cp = cfg["predictor_hidden"] if cfg["predictor_hidden"] > 0 else H

    def table(rows, pad):
        w = g.normal((rows, H), H ** -0.5)
        if pad:
            w[0] = 0.0
        return w

    def fft(name, n_layers, k, into):
        for i in range(n_layers):
            p = f"{name}.layers.{i}.op."
            into[p + "layer_norm1.weight"], into[p + "layer_norm1.bias"] = g.gamma(H), g.beta(H)
            into[p + "self_attn.in_proj_weight"] = g.weight((3 * H, H), 1.4)
            into[p + "self_attn.out_proj.weight"] = g.weight((H, H))
            into[p + "layer_norm2.weight"], into[p + "layer_norm2.bias"] = g.gamma(H), g.beta(H)
            into[p + "ffn.ffn_1.weight"], into[p + "ffn.ffn_1.bias"] = g.weight((4 * H, H, k), 1.4), g.bias(4 * H)
            into[p + "ffn.ffn_2.weight"], into[p + "ffn.ffn_2.bias"] = g.weight((H, 4 * H)), g.bias(H)
        into[f"{name}.layer_norm.weight"], into[f"{name}.layer_norm.bias"] = g.gamma(H), g.beta(H)

    def predictor(name, n_layers, k, n_out, alpha, into):
        if alpha is not None:
            into[name + ".pos_embed_alpha"] = torch.tensor([alpha], dtype=torch.float32)
        for i in range(n_layers):
            p, cin = f"{name}.conv.{i}.", (H if i == 0 else Cp)
            into[p + "1.weight"], into[p + "1.bias"] = g.weight((Cp, cin, k), 1.4), g.bias(Cp)
            into[p + "3.weight"], into[p + "3.bias"] = g.gamma(Cp), g.beta(Cp)
        into[name + ".linear.weight"], into[name + ".linear.bias"] = g.weight((n_out, Cp)), g.bias(n_out)
        if alpha is not None:
            into[name + ".embed_positions._float_tensor"] = torch.zeros(1, dtype=torch.float32)

    sd["encoder_embed_tokens.weight"] = table(V, True)
    fft("encoder", cfg["enc_layers"], cfg["enc_ffn_kernel_size"], sd)
    sd["encoder.embed_tokens.weight"] = sd["encoder_embed_tokens.weight"]
    if not cfg.get("rel_pos"):
        sd["encoder.embed_positions._float_tensor"] = torch.zeros(1, dtype=torch.float32)
    sd["decoder.pos_embed_alpha"] = torch.tensor([0.8], dtype=torch.float32)
    sd["decoder.embed_positions._float_tensor"] = torch.zeros(1, dtype=torch.float32)
    fft("decoder", cfg["dec_layers"], cfg["dec_ffn_kernel_size"], sd)
    sd["mel_out.weight"], sd["mel_out.bias"] = g.weight((M, H)), g.bias(M)
    dur = {}
    predictor("dur_predictor", cfg["dur_predictor_layers"], cfg["dur_predictor_kernel"], 1, None, dur)
    spk, pitch, energy = {}, {}, {}
    if cfg.get("use_pitch_embed"):
        pitch["pitch_embed.weight"] = table(300, True)
        predictor("pitch_predictor", cfg.get("predictor_layers", 5), cfg.get("predictor_kernel", 5),
                  2 if cfg.get("pitch_type", "frame") == "frame" else 1, 0.7, pitch)
    if cfg.get("use_energy_embed"):
        energy["energy_embed.weight"] = table(256, True)
        predictor("energy_predictor", cfg.get("predictor_layers", 5), cfg.get("predictor_kernel", 5), 1, 0.6, energy)
    if cfg.get("use_spk_id"):
        names = ("spk_embed_proj", "spk_embed_f0", "spk_embed_dur") if cfg.get("use_split_spk_id") else ("spk_embed_proj",)
        for name in names:
            spk[name + ".weight"] = g.normal((cfg["num_spk"] + 1, H), 0.5)
    elif cfg.get("use_spk_embed"):
        spk["spk_embed_proj.weight"], spk["spk_embed_proj.bias"] = g.weight((H, 256)), g.bias(H)
    return {**sd, **spk, **dur, **pitch, **energy}


# ----------------------------------------------------------------------------- conditioning encoders
def make_clap_text_state_dict(cfg, seed=11):
    """`caption_encoder.`-relative keys of the CLAP checkpoint FrozenCLAPEmbedder loads (encoders/modules.py:179-183):
    `base.*` = transformers BertModel (without its pooler, which the path never runs), `projection.*` = CLAP/clap.py:8-20."""
    g, sd = _Gen(seed), {}
    W, F, D = cfg["width"], cfg["mlp_dim"], cfg["d_proj"]
    e = "base.embeddings."
    sd[e + "word_embeddings.weight"] = g.normal((cfg["vocab"], W), 0.5)
    sd[e + "position_embeddings.weight"] = g.normal((cfg["max_positions"], W), 0.3)
    sd[e + "token_type_embeddings.weight"] = g.normal((cfg["type_vocab"], W), 0.3)
    sd[e + "LayerNorm.weight"], sd[e + "LayerNorm.bias"] = g.gamma(W), g.beta(W)
    for i in range(cfg["layers"]):
        p = "base.encoder.layer.%d." % i
        for n in ("query", "key", "value"):
            sd[p + "attention.self.%s.weight" % n] = g.weight((W, W), 1.5 if n != "value" else 1.0)
            sd[p + "attention.self.%s.bias" % n] = g.bias(W)
        sd[p + "attention.output.dense.weight"], sd[p + "attention.output.dense.bias"] = g.weight((W, W)), g.bias(W)
        sd[p + "attention.output.LayerNorm.weight"], sd[p + "attention.output.LayerNorm.bias"] = g.gamma(W), g.beta(W)
        sd[p + "intermediate.dense.weight"], sd[p + "intermediate.dense.bias"] = g.weight((F, W)), g.bias(F)
        sd[p + "output.dense.weight"], sd[p + "output.dense.bias"] = g.weight((W, F)), g.bias(W)
        sd[p + "output.LayerNorm.weight"], sd[p + "output.LayerNorm.bias"] = g.gamma(W), g.beta(W)
    sd["projection.linear1.weight"] = g.weight((D, W))
    sd["projection.linear2.weight"] = g.weight((D, D))
    sd["projection.layer_norm.weight"], sd["projection.layer_norm.bias"] = g.gamma(D), g.beta(D)
    return sd


def make_openclip_visual_state_dict(cfg, seed=12):
    """`model.visual.`-relative keys of open_clip's VisionTransformer (what `open_clip.create_model_and_transforms`
    returns for ViT-H-14; encoders/modules.py:321)."""
    g, sd = _Gen(seed), {}
    W, F, D, P = cfg["width"], cfg["mlp_dim"], cfg["d_proj"], cfg["patch"]
    tokens = (cfg["image"] // P) ** 2 + 1
    sd["conv1.weight"] = g.weight((W, 3, P, P))
    sd["class_embedding"] = g.normal((W,), 0.5)
    sd["positional_embedding"] = g.normal((tokens, W), 0.3)
    sd["ln_pre.weight"], sd["ln_pre.bias"] = g.gamma(W), g.beta(W)
    for i in range(cfg["layers"]):
        p = "transformer.resblocks.%d." % i
        sd[p + "ln_1.weight"], sd[p + "ln_1.bias"] = g.gamma(W), g.beta(W)
        sd[p + "attn.in_proj_weight"], sd[p + "attn.in_proj_bias"] = g.weight((3 * W, W), 1.5), g.bias(3 * W)
        sd[p + "attn.out_proj.weight"], sd[p + "attn.out_proj.bias"] = g.weight((W, W), 0.5), g.bias(W)
        sd[p + "ln_2.weight"], sd[p + "ln_2.bias"] = g.gamma(W), g.beta(W)
        sd[p + "mlp.c_fc.weight"], sd[p + "mlp.c_fc.bias"] = g.weight((F, W)), g.bias(F)
        sd[p + "mlp.c_proj.weight"], sd[p + "mlp.c_proj.bias"] = g.weight((W, F), 0.5), g.bias(W)
    sd["ln_post.weight"], sd["ln_post.bias"] = g.gamma(W), g.beta(W)
    sd["proj"] = g.normal((W, D), W ** -0.5)
    return sd


def make_openclip_text_state_dict(cfg, seed=13):
    """`model.`-relative keys of open_clip's CLIP text tower (token_embedding, positional_embedding, transformer, ln_final,
    text_projection)."""
    g, sd = _Gen(seed), {}
    W, F, D = cfg["width"], cfg["mlp_dim"], cfg["d_proj"]
    sd["token_embedding.weight"] = g.normal((cfg["vocab"], W), 0.5)
    sd["positional_embedding"] = g.normal((cfg["max_positions"], W), 0.3)
    for i in range(cfg["layers"]):
        p = "transformer.resblocks.%d." % i
        sd[p + "ln_1.weight"], sd[p + "ln_1.bias"] = g.gamma(W), g.beta(W)
        sd[p + "attn.in_proj_weight"], sd[p + "attn.in_proj_bias"] = g.weight((3 * W, W), 1.5), g.bias(3 * W)
        sd[p + "attn.out_proj.weight"], sd[p + "attn.out_proj.bias"] = g.weight((W, W), 0.5), g.bias(W)
        sd[p + "ln_2.weight"], sd[p + "ln_2.bias"] = g.gamma(W), g.beta(W)
        sd[p + "mlp.c_fc.weight"], sd[p + "mlp.c_fc.bias"] = g.weight((F, W)), g.bias(F)
        sd[p + "mlp.c_proj.weight"], sd[p + "mlp.c_proj.bias"] = g.weight((W, F), 0.5), g.bias(W)
    sd["ln_final.weight"], sd["ln_final.bias"] = g.gamma(W), g.beta(W)
    sd["text_projection"] = g.normal((W, D), W ** -0.5)
    return sd


def make_clap_audio_state_dict(cfg, seed=14):
    """`audio_encoder.`-relative keys of the CLAP checkpoint's audio branch (CLAP/clap.py:22-39, CLAP/audio.py:113-141):
    `base.*` = Cnn14 without its spectrogram / log-mel extractors' frozen buffers, `projection.*`."""
    g, sd = _Gen(seed), {}

    def bn(p, n):
        sd[p + ".weight"], sd[p + ".bias"] = g.gamma(n), g.beta(n)
        sd[p + ".running_mean"], sd[p + ".running_var"] = g.normal((n,), 0.2), 1.0 + g.normal((n,), 0.1).abs()
        sd[p + ".num_batches_tracked"] = torch.tensor(100)
    bn("base.bn0", cfg["mel_bins"])
    cin = 1
    for i, c in enumerate(cfg["channels"]):
        p = "base.conv_block%d." % (i + 1)
        sd[p + "conv1.weight"] = g.weight((c, cin, 3, 3), 1.4)
        sd[p + "conv2.weight"] = g.weight((c, c, 3, 3), 1.4)
        bn(p + "bn1", c)
        bn(p + "bn2", c)
        cin = c
    E, D = cfg["out_emb"], cfg["d_proj"]
    sd["base.fc1.weight"], sd["base.fc1.bias"] = g.weight((E, cin)), g.bias(E)
    sd["base.fc_audioset.weight"], sd["base.fc_audioset.bias"] = g.weight((cfg["classes_num"], E)), g.bias(cfg["classes_num"])
    sd["projection.linear1.weight"] = g.weight((D, E))
    sd["projection.linear2.weight"] = g.weight((D, D))
    sd["projection.layer_norm.weight"], sd["projection.layer_norm.bias"] = g.gamma(D), g.beta(D)
    return sd


def fold_weight_norm(sd):
    """weight_g / weight_v -> weight, as torch's remove_weight_norm: w = g * v / ||v||_(dims != 0)
    (NeuralSeq/modules/hifigan/hifigan.py:171-178; for ConvTranspose1d dim 0 is the in-channel axis)."""
    out = {}
    for k, v in sd.items():
        if k.endswith(".weight_g"):
            base = k[: -len(".weight_g")]
            vv = sd[base + ".weight_v"]
            norm = vv.reshape(vv.shape[0], -1).norm(dim=1).reshape(-1, *([1] * (vv.dim() - 1)))
            out[base + ".weight"] = vv * (v / norm)
        elif not k.endswith(".weight_v"):
            out[k] = v
    return out


def strip_prefix(sd, prefix):
    """Select the sub-dict under `prefix` of a full LatentDiffusion checkpoint
    (e.g. 'model.diffusion_model.' or 'first_stage_model.')."""
    n = len(prefix)
    return {k[n:]: v for k, v in sd.items() if k.startswith(prefix)}
