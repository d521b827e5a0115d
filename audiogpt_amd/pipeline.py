"""Make-An-Audio generation pipeline on one MI355X: DDIM, PLMS or ancestral DDPM (UNet) -> VAE decode -> clamp -> vocoder.

This is the body of the reference's `T2A.txt2audio` / `I2A.img2audio` / `Inpaint.inpaint`
(audio-chatgpt.py:158-183, 232-261, 500-528) between conditioning and waveform, run by
libaudiogpt_mi355x.  Batched over prompts: where the reference loops `vocoder.vocode(spec)` per sample
(audio-chatgpt.py:179-181) the vocoder here takes the whole batch (identical per-sample results).
"""
import numpy as np
import torch

from . import config as C
from . import weights as WT
from ._lib import MaaError
from .backend import Context, UNet, VAE, Vocoder, ddim_stochastic_encode


def make_beta_schedule_linear(timesteps, linear_start, linear_end):
    """util.py:21-25 ("linear"): linspace(sqrt(b0), sqrt(b1), T)**2 in fp64."""
    return np.linspace(linear_start ** 0.5, linear_end ** 0.5, timesteps, dtype=np.float64) ** 2


def alphas_cumprod_f32(timesteps, linear_start, linear_end):
    """ddpm.py:115-136: fp64 cumprod stored as an fp32 buffer."""
    betas = make_beta_schedule_linear(timesteps, linear_start, linear_end)
    return np.cumprod(1.0 - betas, axis=0).astype(np.float32)


def ddim_schedule(S, ac_f32):
    """util.py:46-74 ('uniform', eta = 0): (timesteps, alphas, alphas_prev) as the sampler's tables."""
    T = ac_f32.shape[0]
    c = T // S
    steps = np.asarray(list(range(0, T, c))) + 1
    alphas = ac_f32[steps]
    alphas_prev = np.asarray([ac_f32[0]] + ac_f32[steps[:-1]].tolist(), dtype=np.float32)
    return steps, alphas, alphas_prev


class MakeAnAudio:
    """UNet + VAE + vocoder replicas on one device."""

    def __init__(self, device="cuda:0", ldm=None, vocoder_cfg=None, unet_sd=None, vae_sd=None, vocoder_sd=None,
                 seeds=(0, 1, 2), with_encoder=False, precision="f32", stream=None):
        # stream: a torch.cuda.Stream this replica runs on (its library context shares it).  None: the library creates its
        # own blocking stream, which orders against PyTorch's legacy default stream -- simple, but every default-stream op
        # is then a barrier across ALL replicas of the device.  Several replicas side by side want one stream each.
        self.ldm = ldm or C.LDM_T2A
        self.vocoder_cfg = vocoder_cfg or C.HIFIGAN_16K
        self.precision = precision
        self.stream = stream
        self.ctx = Context(device, stream=stream, precision=precision)
        self.device = self.ctx.device
        unet_sd = unet_sd if unet_sd is not None else WT.make_unet_state_dict(self.ldm["unet"], seed=seeds[0])
        vae_sd = vae_sd if vae_sd is not None else WT.make_vae_state_dict(self.ldm["vae"], seed=seeds[1],
                                                                          with_encoder=with_encoder)
        vocoder_sd = vocoder_sd if vocoder_sd is not None else WT.make_vocoder_state_dict(self.vocoder_cfg, seed=seeds[2])
        self.unet = UNet(self.ctx, self.ldm["unet"], unet_sd)
        self.vae = VAE(self.ctx, self.ldm["vae"], vae_sd)
        self.has_encoder = any(k.startswith("encoder.") for k in vae_sd)
        self.vocoder = Vocoder(self.ctx, self.vocoder_cfg, vocoder_sd)
        self.scale_factor = float(self.ldm.get("scale_factor", 1.0))
        self.alphas_cumprod = alphas_cumprod_f32(self.ldm["timesteps"], self.ldm["linear_start"], self.ldm["linear_end"])
        self._ddpm_tables = None      # the ancestral sampler's schedule buffers, made on first use (sample_latents)

    # ---- stages ----------------------------------------------------------------------------------
    # The widest latent the chain takes.  The VAE decoder's mid-block attention (vae.cpp run_attn: one head as wide as the block,
    # 512, which the fused attention kernel does not take) runs as two batched GEMMs around a softmax over the [h w, h w] score
    # matrix of each sample, held in the workspace with its rows padded to a multiple of 4; the contraction engines address a
    # sample's matrix with 32-bit products of position and pitch (blocks.cpp attention_into, igemm_*.hip), so h w * pad4(h w)
    # must stay below 2^31: h w <= 46340, i.e. w <= 4634 at the models' h = 10 (4634 * 8 frames * 256 / 16 kHz = 593 s).
    MAX_LATENT_POSITIONS = 46340

    def check_latent_size(self, h, w):
        """Raises MaaError for a latent [*, *, h, w] larger than the VAE decoder's mid-block attention accepts
        (MAX_LATENT_POSITIONS = 46340 positions: w <= 4634 at h = 10); nothing is launched."""
        if int(h) * int(w) > self.MAX_LATENT_POSITIONS:
            raise MaaError("latent %d x %d has %d positions; the VAE decoder's mid-block attention takes at most %d (w <= %d at "
                           "h = %d)" % (h, w, int(h) * int(w), self.MAX_LATENT_POSITIONS, self.MAX_LATENT_POSITIONS // int(h), h))

    def sample_latents(self, x_T, cond=None, uncond=None, scale=1.0, S=100, concat=None, use_graph=True, sampler="ddim", split=None):
        """x_T -> x_0 over the S-step schedule: sampler "ddim" (DDIMSampler, S UNet evaluations) or "plms" (PLMSSampler,
        S + 1 evaluations); or sampler "ddpm", the model's own ancestral chain (LatentDiffusion_audio.p_sample_loop) over all
        `timesteps` (1000) DDPM steps with the model's clip_denoised=True -- S is ignored there.  Its per-step noise is drawn up
        front from torch's global generator on the device, in the reference's order (ldm/ddpm.py): timesteps * B * C * H * W * 4
        bytes, 100 MB for 8 T2A latents.  Guidance with "ddpm" is an extension (the reference's chain has none).
        split: the reference's `split_input_params` dictionary (ldm/split.py) for a latent wider than the
        model was trained on -- every evaluation runs on overlapping crops of `ks` and is stitched (ddpm_audio.py:572-654)."""
        if sampler not in ("ddim", "plms", "ddpm"):
            raise MaaError('sampler must be "ddim", "plms" or "ddpm", got %r' % (sampler,))
        kw = dict(split=split) if split is not None else {}
        if sampler == "ddpm":
            from .ldm.ddpm import schedule_buffers
            if self._ddpm_tables is None:
                self._ddpm_tables = schedule_buffers(self.ldm["timesteps"], self.ldm["linear_start"], self.ldm["linear_end"])
            n = self.ldm["timesteps"]
            noise_p = torch.stack([torch.randn(tuple(x_T.shape), device=self.device) for _ in range(n)])      # ddpm_audio.py:766
            return self.unet.ddpm_sample(x_T, self._ddpm_tables, n, cond=cond, uncond=uncond, scale=scale, concat=concat,
                                         noise_p=noise_p, use_graph=use_graph, **kw)
        steps, a, ap = ddim_schedule(S, self.alphas_cumprod)
        run = self.unet.plms_sample if sampler == "plms" else self.unet.ddim_sample
        return run(x_T, steps, a, ap, cond=cond, uncond=uncond, scale=scale, concat=concat, use_graph=use_graph, **kw)

    def decode(self, z):
        """decode_first_stage then the tools' clamp((x+1)/2, 0, 1) (audio-chatgpt.py:175-176) -> [B,80,T]."""
        return self.vae.decode_spec(z, self.scale_factor)      # (the clamp runs in the decoder's last pass: no torch arithmetic)

    def vocode(self, spec):
        return self.vocoder(spec)[:, 0]

    def generate_here(self, x_T, cond=None, uncond=None, scale=1.0, S=100, concat=None, use_graph=True, sampler="ddim", split=None):
        """generate() on the CURRENT torch stream, which must be this replica's stream when it has one (the caller orders
        inputs and outputs against other streams itself: bench.py's worker threads)."""
        self.check_latent_size(x_T.shape[-2], x_T.shape[-1])
        z = self.sample_latents(x_T, cond, uncond, scale, S, concat, use_graph, sampler=sampler, split=split)
        spec = self.decode(z)
        return self.vocode(spec), spec, z

    def generate(self, x_T, cond=None, uncond=None, scale=1.0, S=100, concat=None, use_graph=True, sampler="ddim", split=None):
        """x_T [B,4,h,w] -> (wav [B, T*hop], spec [B,80,T], z [B,4,h,w]); all on the device.  With a private stream the
        work is ordered after the caller's current stream on entry and the caller's stream after it on return.
        sampler: "ddim", "plms" or "ddpm" -- the model's ancestral chain over all its timesteps; S is ignored (sample_latents).
        split: long-form generation -- the reference's `split_input_params` dictionary (sample_latents); the sampler evaluates the
        UNet on crops of the training size, the VAE decode and the vocoder run on the whole width.  The widest latent the VAE's
        mid-block attention accepts is h * w <= 46340 positions (w <= 4634 at h = 10, about 593 s of audio: MAX_LATENT_POSITIONS
        above says why); a wider one raises MaaError before anything is launched."""
        self.check_latent_size(x_T.shape[-2], x_T.shape[-1])
        if self.stream is None:
            return self.generate_here(x_T, cond, uncond, scale, S, concat, use_graph, sampler=sampler, split=split)
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            out = self.generate_here(x_T, cond, uncond, scale, S, concat, use_graph, sampler=sampler, split=split)
        cur.wait_stream(self.stream)
        for t in out:
            t.record_stream(cur)
        return out

    def edit_here(self, mel, cond, uncond=None, scale=1.0, S=100, strength=0.5, noise=None, use_graph=True, split=None):
        """Text-guided editing of an existing recording (SDEdit, Make-An-Audio's img2img form): the mel's latent is noised
        part of the way down an S-step DDIM schedule and denoised under `cond`.  mel [B, 1, 80, T] in [-1, 1] (as
        Inpaint.make_batch_sd forms it) -> (wav [B, T*hop], spec [B, 80, T], z [B, 4, 10, T/8]), all on the device, on the
        CURRENT torch stream (as generate_here).
        The chain: VAE encode (moments) -> one kernel forming the posterior sample * scale_factor and noising it to DDIM
        index t_enc = int(strength * S) (DDIMSampler.stochastic_encode) -> the DDIM steps of indices t_enc - 1 .. 0
        (DDIMSampler.decode) -> VAE decode + clamp -> vocoder.  As in the reference's img2img, the noise level is that of
        index t_enc and the first denoising step is index t_enc - 1; strength must lie in [0, 1), so that t_enc < S (an
        S-step schedule has no index S); at t_enc = 0 the latent is noised at index 0 and no step runs.
        noise: None (the posterior noise, then the q_sample noise, drawn from the model's device generator) or the pair
        (n_post, n_q), each [B, 4, h, w].
        split: the reference's `split_input_params` dictionary for a recording longer than the model's training size (the
        denoising steps then run on overlapping crops, as generate's; the same width limit applies)."""
        if not self.has_encoder:
            raise MaaError("edit: the VAE has no encoder weights -- build MakeAnAudio with with_encoder=True (or a vae_sd with "
                           "encoder.* / quant_conv.*)")
        if not 0.0 <= float(strength) < 1.0:
            raise MaaError("edit: strength must lie in [0, 1), got %r" % (strength,))
        t_enc = int(float(strength) * S)
        mel = mel.detach().to(device=self.device, dtype=torch.float32).contiguous()
        if mel.dim() != 4 or mel.shape[1] != 1:
            raise MaaError("edit: mel must be [B, 1, n_mels, T], got %s" % (tuple(mel.shape),))
        self.check_latent_size(mel.shape[2] // 8, mel.shape[3] // 8)
        moments = self.vae.encode_moments(mel)
        B, C2, h, w = moments.shape
        shape = (B, C2 // 2, h, w)
        if noise is None:
            n_post = torch.randn(shape, device=self.device)      # posterior.sample() (distributions.py:35)
            n_q = torch.randn(shape, device=self.device)         # stochastic_encode's randn_like (ddim.py:238-239)
        else:
            n_post, n_q = noise
        steps, a, ap = ddim_schedule(S, self.alphas_cumprod)
        a_t = torch.from_numpy(a)
        z_enc = ddim_stochastic_encode(self.ctx, moments, t_enc, torch.sqrt(a_t), torch.sqrt(1.0 - a_t), n_q, moments=True,
                                       scale_factor=self.scale_factor, noise_post=n_post)
        kw = dict(split=split) if split is not None else {}
        z = self.unet.ddim_decode(z_enc, t_enc, steps, a, ap, cond=cond, uncond=uncond, scale=scale, use_graph=use_graph, **kw)
        spec = self.decode(z)
        return self.vocode(spec), spec, z

    def edit(self, mel, cond, uncond=None, scale=1.0, S=100, strength=0.5, noise=None, use_graph=True, split=None):
        """edit_here with generate()'s stream ordering: with a private stream the work is ordered after the caller's current
        stream on entry and the caller's stream after it on return."""
        if self.stream is None:
            return self.edit_here(mel, cond, uncond, scale, S, strength, noise, use_graph, split=split)
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            out = self.edit_here(mel, cond, uncond, scale, S, strength, noise, use_graph, split=split)
        cur.wait_stream(self.stream)
        for t in out:
            t.record_stream(cur)
        return out

    def audio_seconds(self, n_clips, frames):
        return n_clips * frames * self.vocoder.hop / float(self.vocoder_cfg["sampling_rate"])

    def close(self):
        for o in (self.unet, self.vae, self.vocoder, self.ctx):
            o.close()
