"""The Glow post-net of GenerSpeech and PortaSpeech run in reverse on the device -- AudioGPT's TTS_OOD and TTS tools' last stage
before the vocoder (NeuralSeq/modules/GenerSpeech/model/glow_modules.py::Glow, model/wavenet.py::WN, generspeech.py:233-260
run_post_glow; hparams as in modules/GenerSpeech/config/generspeech.yaml:83-92 and egs_bases/tts/ps_flow.yaml).

    glow = Glow(C.GENERSPEECH_POST_GLOW, state_dict=post_flow_sd)
    x, logdet = glow(z, x_mask, g=g, reverse=True)                      # the reference's call, device tensors
    post = PostGlow(C.GENERSPEECH_POST_GLOW, state_dict=post_flow_sd)
    mel = post.infer(ret['mel_out'], ret['decoder_inp'], ret['spk_embed'], ret['emo_embed'], ret['ref_prosody'])

The whole pass is one library call (maa_glow_reverse): the conditioning projections of every block and layer as one GEMM, the
gated dilated convolutions as implicit GEMMs, each block's coupling inverse, 4 x 4 channel mix and ActNorm as one row kernel.
torch transposes between the reference's [B, C, T] and the library's channels-last rows.

Built: inv_conv_type 'near', n_sqz 2, n_split 4, odd kernel_size, hidden_channels and in_channels multiples of 4, the reverse
direction.  Everything else is refused with the reason before a device is touched; p_dropout is not read (eval).  The rest of
GenerSpeech (MixStyle, the style adaptors and aligners, the pitch inpainter, the emotion and speaker encoders) and of PortaSpeech
(FVAE, encoder) is not here: their outputs are this class's inputs."""
import torch

from . import backend
from . import config as C
from . import weights as WT
from .backend import Context, default_precision
from ._lib import MaaError


def check_shared_wn(cfg, sd):
    """With share_wn_layers = n the blocks of a group run one WN: their in_layers / res_skip_layers must be equal tensors."""
    n = int(cfg.get("share_wn_layers", 0))
    if n <= 0:
        return
    for b in range(int(cfg["n_blocks"])):
        lead = b - b % n
        if lead == b:
            continue
        p, q = "flows.%d.wn." % (3 * b + 2), "flows.%d.wn." % (3 * lead + 2)
        for k in sorted(sd):
            if k.startswith(p) and not k.startswith(p + "cond_layer."):
                other = q + k[len(p):]
                if other not in sd or sd[other].shape != sd[k].shape or not torch.equal(sd[other].cpu(), sd[k].cpu()):
                    raise MaaError("Glow: share_wn_layers = %d but %s differs from %s: the blocks of a group share one WN, a state "
                                   "dict whose group members differ was not made with this configuration" % (n, k, other))


class Glow(object):
    """glow_modules.py:496-580 with the reference's call surface, reverse only: glow(z, x_mask, g=g, reverse=True,
    return_hiddens=False) with z [B, C, T], x_mask [B, 1, T] (None: all ones), g [B, gin, T] (None when gin_channels is 0) ->
    (x [B, C, 2 (T // 2)], logdet [B]) and, on request, hs: the 3 n_blocks flows' outputs [B, 2C, T // 2] in execution order.
    cfg: config.GENERSPEECH_POST_GLOW / PORTASPEECH_POST_GLOW; state_dict: the checkpoint's post_flow (a `model.post_flow.` or
    `post_flow.` prefix is stripped; weight-norm pairs or the plain weights store_inverse leaves), seeded random weights when None."""

    def __init__(self, cfg=None, device="cuda:0", state_dict=None, ctx=None, precision=None, seed=23):
        self.cfg = dict(cfg or C.GENERSPEECH_POST_GLOW)
        backend.glow_config(self.cfg)                  # refuses an unsupported configuration before a context is made
        sd = state_dict if state_dict is not None else WT.make_glow_state_dict(self.cfg, seed=seed)
        sd = WT.strip_prefix(sd, "model.post_flow.") or WT.strip_prefix(sd, "post_flow.") or sd
        check_shared_wn(self.cfg, sd)
        self.ctx = ctx or Context(device, precision=precision or default_precision())
        self.device = self.ctx.device
        self.net = backend.Glow(self.ctx, self.cfg, sd)

    @torch.no_grad()
    def forward(self, x, x_mask=None, g=None, reverse=False, return_hiddens=False):
        if not reverse:
            raise MaaError("Glow: reverse=False (the training direction, mel -> latent) is not built: only the inference pass "
                           "reverse=True runs on the device")
        if x.dim() != 3 or x.shape[1] != self.cfg["in_channels"]:
            raise MaaError("Glow: z %s is not [B, %d, T]" % (tuple(x.shape), self.cfg["in_channels"]))
        if x.shape[2] < 2:
            raise MaaError("Glow: T < 2 -- the squeeze pairs frames, T = %d leaves no row" % x.shape[2])
        rows = lambda t: t.to(self.device, torch.float32).transpose(1, 2).contiguous()          # noqa: E731
        mask = None if x_mask is None else x_mask.to(self.device, torch.float32).reshape(x.shape[0], x.shape[2]).contiguous()
        out, logdet, hs = self.net.reverse(rows(x), None if g is None else rows(g), mask, return_hiddens=return_hiddens)
        out = out.transpose(1, 2)
        if return_hiddens:
            return out, logdet, [h.transpose(1, 2) for h in hs]
        return out, logdet

    __call__ = forward

    def eval(self):
        return self

    def to(self, *args, **kwargs):
        return self


class PostGlow(object):
    """run_post_glow's inference branch (generspeech.py:233-243, 255-260): the conditioning is the channel concatenation
    [mel_out, decoder_inp, spk_embed over T, emo_embed over T, ref_prosody] (decoder_inp dropped when use_txt_cond is false), the
    mask all ones, the latent a draw of Normal(0, 1) on the host's global generator times noise_scale.  PortaSpeech's form,
    g = [mel_out, decoder_inp], is the same call without the three vectors."""

    def __init__(self, cfg=None, device="cuda:0", state_dict=None, ctx=None, precision=None, seed=23):
        self.cfg = dict(cfg or C.GENERSPEECH_POST_GLOW)
        self.post_flow = Glow(self.cfg, device=device, state_dict=state_dict, ctx=ctx, precision=precision, seed=seed)
        self.ctx, self.device = self.post_flow.ctx, self.post_flow.device

    def cond(self, mel_out, decoder_inp=None, spk_embed=None, emo_embed=None, ref_prosody=None):
        """g as channels-last rows [B, T, gin] on the device."""
        dev = lambda t: t.to(self.device, torch.float32)          # noqa: E731
        B, T = mel_out.shape[0], mel_out.shape[1]
        parts = [dev(mel_out)]
        if self.cfg.get("use_txt_cond", True):
            if decoder_inp is None:
                raise MaaError("PostGlow: use_txt_cond is true, so decoder_inp is part of the conditioning and must be given")
            parts.append(dev(decoder_inp))
        vectors = (spk_embed, emo_embed, ref_prosody)
        if any(v is not None for v in vectors):
            if any(v is None for v in vectors):
                raise MaaError("PostGlow: spk_embed, emo_embed and ref_prosody come together (GenerSpeech) or not at all (PortaSpeech)")
            parts += [dev(spk_embed).reshape(B, 1, -1).expand(B, T, -1), dev(emo_embed).reshape(B, 1, -1).expand(B, T, -1),
                      dev(ref_prosody)]
        g = torch.cat(parts, dim=2).contiguous()
        if g.shape[2] != self.cfg["gin_channels"]:
            raise MaaError("PostGlow: the conditioning has %d channels, gin_channels is %d" % (g.shape[2], self.cfg["gin_channels"]))
        return g

    @torch.no_grad()
    def infer(self, mel_out, decoder_inp=None, spk_embed=None, emo_embed=None, ref_prosody=None, z=None, noise_scale=None):
        """mel_out [B, T, 80], decoder_inp [B, T, hidden], spk_embed / emo_embed [B, 1, hidden], ref_prosody [B, T, hidden] (the
        reference's `ret` entries, channels-last) -> mel_out [B, 2 (T // 2), 80] on the device.  z [B, 80, T]: the latent in place of
        the draw."""
        B, T, M = mel_out.shape
        if T < 2:
            raise MaaError("PostGlow: T < 2 -- the squeeze pairs frames, T = %d leaves no row" % T)
        g = self.cond(mel_out, decoder_inp, spk_embed, emo_embed, ref_prosody)
        if z is None:
            scale = self.cfg["noise_scale"] if noise_scale is None else noise_scale
            z = torch.distributions.Normal(0, 1).sample((B, M, T)).to(self.device) * scale
        zr = z.to(self.device, torch.float32).transpose(1, 2).contiguous()
        x, _, _ = self.post_flow.net.reverse(zr, g, None, return_logdet=False)
        return x
