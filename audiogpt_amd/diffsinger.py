"""DiffSinger's shallow-diffusion sampler with the reference's Python surface, backed by the HIP library.

Inference subset of `GaussianDiffusion` (NeuralSeq/modules/diff/shallow_diffusion_tts.py:66-283) as the T2S tool drives
it (audio-chatgpt.py:298-339 -> NeuralSeq/inference/svs/ds_e2e.py): the part that costs the time is `denoise_fn` (DiffNet,
20 gated dilated residual layers) inside the sampling loop; the FastSpeech2(MIDI) front end (`self.fs2`) that turns tokens and
note features into the conditioning `decoder_inp`, `mel2ph` and the coarse mel runs on the device in front of it
(`FastSpeech2MIDI`, once per utterance).  Both loops of forward(infer=True) are here: the PLMS loop (`pndm_speedup`, K_step /
pndm_speedup evaluations per utterance, ds1000.yaml) and the ancestral chain every other shipped configuration takes
(K_step p_sample steps: popcs_ds_beta6.yaml, lj_ds_beta6.yaml, ds100_adj_rel.yaml, ds60_rel.yaml, ds1000-10dil.yaml).

    gd = GaussianDiffusion(C.DIFFSINGER_DS1000, device="cuda:0", state_dict=ckpt_denoise_fn_sd, spec_min=..., spec_max=...)
    mel = gd.infer(fs2_mel [B, T, 80], cond [B, 256, T])          # == ret['mel_out'] of forward(..., infer=True)

The tail of the e2e singing pipeline (NeuralSeq/inference/svs/ds_e2e.py:36-45, every shipped e2e configuration sets
`pe_enable`) runs on the device as well: `PitchExtractor` predicts f0 from the generated mel and the NSF HiFi-GAN takes both,
so the mel never leaves the device between the diffusion and the waveform.

    e2e = DiffSingerE2E(gd, hifigan.vocoder, pe=PitchExtractor(ctx=gd.ctx, state_dict=pe_ckpt_sd))
    wav = e2e.infer(fs2_mel, cond)                                # [1, B * T * hop], run_vocoder's shape

    e2e = DiffSingerE2E(gd, hifigan.vocoder, pe=..., fs2=FastSpeech2MIDI(ctx=gd.ctx, state_dict=ckpt_fs2_sd))
    wav = e2e.forward_model(txt_tokens, pitch_midi, midi_dur, is_slur)      # score -> waveform, no model on the host

The cascade configuration (NeuralSeq/inference/svs/ds_cascade.py, ds60_rel.yaml: use_pitch_embed, no PitchExtractor) predicts the
pitch in the front end and sings it: `FastSpeech2MIDICascade` adds the pitch branch to the front end, `DiffSingerCascade` hands its
f0 to the vocoder.

    cas = DiffSingerCascade(gd, hifigan.vocoder, FastSpeech2MIDICascade(ctx=gd.ctx, state_dict=ckpt_fs2_sd))
    wav = cas.forward_model(txt_tokens, pitch_midi, midi_dur, is_slur)      # f0=, uv=, mel2ph=: a caller's, else predicted

The configurations without use_midi -- DiffSpeech (lj_ds_beta6.yaml) and the original DiffSinger (popcs_ds_beta6.yaml) -- run the
plain `FastSpeech2` (energy branch and speaker embeddings included) in front of the same chain: `DiffSpeech`.

    tts = DiffSpeech(gd, hifigan.vocoder, FastSpeech2(ctx=gd.ctx, state_dict=ckpt_fs2_sd))
    wav = tts.forward_model(txt_tokens)                                     # spk_embed=, mel2ph=, f0=, uv=, energy=
"""
import numpy as np
import torch

from . import config as C
from . import weights as WT
from . import backend
from .backend import Context, DiffNet, default_precision

# sample_ddpm's default cap on the steps' noise buffer: n * B * M * T * 4 bytes per device call
NOISE_CAP_BYTES = 64 << 20


def linear_beta_schedule(timesteps, max_beta=0.01):
    """shallow_diffusion_tts.py:44-49."""
    return np.linspace(1e-4, max_beta, timesteps)


def cosine_beta_schedule(timesteps, s=0.008):
    """shallow_diffusion_tts.py:52-62 (https://openreview.net/forum?id=-NEXDKk8gZ)."""
    steps = timesteps + 1
    x = np.linspace(0, steps, steps)
    alphas_cumprod = np.cos(((x / steps) + s) / (1 + s) * np.pi * 0.5) ** 2
    alphas_cumprod = alphas_cumprod / alphas_cumprod[0]
    betas = 1 - (alphas_cumprod[1:] / alphas_cumprod[:-1])
    return np.clip(betas, a_min=0, a_max=0.999)


def extract(a, t, x_shape):
    """shallow_diffusion_tts.py:32-35."""
    b = t.shape[0]
    return a.gather(-1, t).reshape(b, *((1,) * (len(x_shape) - 1)))


def noise_like(shape, device, repeat=False):
    """shallow_diffusion_tts.py:38-41: one draw of `shape`, or one row drawn and repeated over the batch."""
    if repeat:
        return torch.randn((1, *shape[1:]), device=device).repeat(shape[0], *((1,) * (len(shape) - 1)))
    return torch.randn(shape, device=device)


# the buffers of __init__ (:103-123), in its order
SCHEDULE_BUFFERS = ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod",
                    "log_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod",
                    "posterior_variance", "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2")


def schedule_buffers(timesteps, schedule_type=None, max_beta=0.01, betas=None):
    """The twelve schedule buffers of GaussianDiffusion.__init__ (:82-123) as fp32 numpy arrays: float64 numpy, rounded once.
    betas given: used as they are; else schedule_type "linear" (1e-4 .. max_beta) or "cosine" (also when it is None: :85-88)."""
    if betas is not None:
        betas = betas.detach().cpu().numpy() if isinstance(betas, torch.Tensor) else np.asarray(betas)
    elif schedule_type is None or schedule_type == "cosine":
        betas = cosine_beta_schedule(timesteps)
    elif schedule_type == "linear":
        betas = linear_beta_schedule(timesteps, max_beta)
    else:
        raise KeyError("schedule_type %r: the reference has 'linear' and 'cosine'" % (schedule_type,))
    alphas = 1. - betas
    alphas_cumprod = np.cumprod(alphas, axis=0)
    alphas_cumprod_prev = np.append(1., alphas_cumprod[:-1])
    posterior_variance = betas * (1. - alphas_cumprod_prev) / (1. - alphas_cumprod)
    b = dict(
        betas=betas, alphas_cumprod=alphas_cumprod, alphas_cumprod_prev=alphas_cumprod_prev,
        sqrt_alphas_cumprod=np.sqrt(alphas_cumprod), sqrt_one_minus_alphas_cumprod=np.sqrt(1. - alphas_cumprod),
        log_one_minus_alphas_cumprod=np.log(1. - alphas_cumprod), sqrt_recip_alphas_cumprod=np.sqrt(1. / alphas_cumprod),
        sqrt_recipm1_alphas_cumprod=np.sqrt(1. / alphas_cumprod - 1), posterior_variance=posterior_variance,
        posterior_log_variance_clipped=np.log(np.maximum(posterior_variance, 1e-20)),
        posterior_mean_coef1=betas * np.sqrt(alphas_cumprod_prev) / (1. - alphas_cumprod),
        posterior_mean_coef2=(1. - alphas_cumprod_prev) * np.sqrt(alphas) / (1. - alphas_cumprod))
    return {k: torch.tensor(b[k], dtype=torch.float32).numpy() for k in SCHEDULE_BUFFERS}


class GaussianDiffusion(object):
    """cfg keys beside the denoiser's: timesteps, K_step, schedule_type ("linear" with max_beta, or "cosine": the reference's
    default when the key is absent), pndm_speedup (truthy: the PLMS loop; falsy or absent: the ancestral chain), gaussian_start.
    betas: an explicit schedule, as the reference's constructor takes it.  ctx / denoise_fn: an existing Context / DiffNet to use."""

    def __init__(self, cfg=None, device="cuda:0", state_dict=None, spec_min=None, spec_max=None, ctx=None, precision=None,
                 seed=7, betas=None, denoise_fn=None):
        self.cfg = dict(cfg or C.DIFFSINGER_DS1000)
        self.ctx = ctx or Context(device, precision=precision or default_precision())
        self.device = self.ctx.device
        self.mel_bins = self.cfg["in_dims"]
        self.K_step = int(self.cfg["K_step"])
        host = schedule_buffers(int(self.cfg["timesteps"]), self.cfg.get("schedule_type"), self.cfg.get("max_beta", 0.01), betas)
        self.num_timesteps = int(host["betas"].shape[0])
        for k in SCHEDULE_BUFFERS:                                                         # (:101-123: fp32 buffers)
            setattr(self, k, torch.from_numpy(host[k]).to(self.device))
        # sigma of p_sample (:166), by torch in fp32 from the fp32 buffer; with the four coefficients, the step's host tables
        sigma = (0.5 * torch.from_numpy(host["posterior_log_variance_clipped"])).exp().numpy()
        self._ddpm_tables = (host["sqrt_recip_alphas_cumprod"], host["sqrt_recipm1_alphas_cumprod"], host["posterior_mean_coef1"],
                             host["posterior_mean_coef2"], sigma)
        self._alphas_cumprod_host = host["alphas_cumprod"]
        m = self.mel_bins
        self.spec_min = torch.as_tensor(spec_min if spec_min is not None else [-6.0] * m, dtype=torch.float32, device=self.device)[None, None, :m]
        self.spec_max = torch.as_tensor(spec_max if spec_max is not None else [1.5] * m, dtype=torch.float32, device=self.device)[None, None, :m]
        if denoise_fn is None:
            sd = state_dict if state_dict is not None else WT.make_diffnet_state_dict(self.cfg, seed=seed)
            sd = WT.strip_prefix(sd, "denoise_fn.") or sd
            denoise_fn = DiffNet(self.ctx, self.cfg, sd)
        self.denoise_fn = denoise_fn

    def _t(self, t):
        return torch.as_tensor(t, device=self.device).long().reshape(-1)

    # ---- shallow_diffusion_tts.py:128-147
    def q_mean_variance(self, x_start, t):
        t = self._t(t)
        mean = extract(self.sqrt_alphas_cumprod, t, x_start.shape) * x_start
        variance = extract(1. - self.alphas_cumprod, t, x_start.shape)
        log_variance = extract(self.log_one_minus_alphas_cumprod, t, x_start.shape)
        return mean, variance, log_variance

    def predict_start_from_noise(self, x_t, t, noise):
        t = self._t(t)
        return (extract(self.sqrt_recip_alphas_cumprod, t, x_t.shape) * x_t -
                extract(self.sqrt_recipm1_alphas_cumprod, t, x_t.shape) * noise)

    def q_posterior(self, x_start, x_t, t):
        t = self._t(t)
        posterior_mean = (extract(self.posterior_mean_coef1, t, x_t.shape) * x_start +
                          extract(self.posterior_mean_coef2, t, x_t.shape) * x_t)
        posterior_variance = extract(self.posterior_variance, t, x_t.shape)
        posterior_log_variance_clipped = extract(self.posterior_log_variance_clipped, t, x_t.shape)
        return posterior_mean, posterior_variance, posterior_log_variance_clipped

    # ---- :149-166: the denoiser, then the fused step kernel (maa_ds_ddpm_update)
    @torch.no_grad()
    def p_mean_variance(self, x, t, cond, clip_denoised: bool):
        t = self._t(t)
        noise_pred = self.denoise_fn(x, t, cond)
        model_mean = self.denoise_fn.ddpm_update(x, noise_pred, t, self._ddpm_tables, torch.zeros_like(noise_pred), clip_denoised)
        return (model_mean, extract(self.posterior_variance, t, model_mean.shape),
                extract(self.posterior_log_variance_clipped, t, model_mean.shape))

    @torch.no_grad()
    def p_sample(self, x, t, cond, clip_denoised=True, repeat_noise=False):
        t = self._t(t)
        noise_pred = self.denoise_fn(x, t, cond)
        noise = noise_like(tuple(noise_pred.shape), self.device, repeat_noise)
        return self.denoise_fn.ddpm_update(x, noise_pred, t, self._ddpm_tables, noise, clip_denoised)

    # ---- :203-208, 279-283
    def q_sample(self, x_start, t, noise=None):
        if noise is None:
            noise = torch.randn_like(x_start)
        ex = lambda a: a[t].reshape(-1, 1, 1, 1)    # noqa: E731
        return ex(self.sqrt_alphas_cumprod) * x_start + ex(self.sqrt_one_minus_alphas_cumprod) * noise

    def norm_spec(self, x):
        return (x - self.spec_min) / (self.spec_max - self.spec_min) * 2 - 1

    def denorm_spec(self, x):
        return (x + 1) / 2 * (self.spec_max - self.spec_min) + self.spec_min

    # ---- :262-269 with :166-201, on the device
    def sample_plms(self, x, cond, K_step=None, interval=None, use_graph=True):
        """x [B, 1, M, T] at step K_step - 1 -> x_0."""
        K = self.K_step if K_step is None else int(K_step)
        iv = int(self.cfg["pndm_speedup"]) if interval is None else int(interval)
        return self.denoise_fn.plms_sample(x, cond, self._alphas_cumprod_host, K, iv, use_graph=use_graph)

    # ---- :269-271 with :159-166, on the device
    @torch.no_grad()
    def sample_ddpm(self, x, cond, K_step=None, noise_p=None, clip_denoised=True, use_graph=True, noise_cap_bytes=NOISE_CAP_BYTES):
        """The ancestral chain `for i in reversed(range(0, K_step)): x = p_sample(x, i, cond)`: x [B, 1, M, T] at step
        K_step - 1 -> x_0.  noise_p [K_step, B, 1, M, T]: the steps' draws in loop order; None draws them as the reference's loop
        does, one torch.randn of x's shape per step on the device from the global generator, the t = 0 draw included.

        The chain runs as consecutive device calls of n steps each (maa_ds_ddpm_sample(start, n)), n the largest count whose
        noise buffer n * B * M * T * 4 bytes stays within noise_cap_bytes (at least 1: a single step's draw is never split).
        The device loop equals its consecutive parts bit for bit and the draws are made one step at a time either way, so
        the cap changes neither the draws nor the result."""
        K = self.K_step if K_step is None else int(K_step)
        x = x.to(device=self.device, dtype=torch.float32)
        shape = tuple(x.shape)
        if noise_p is not None and tuple(noise_p.shape) != (K,) + shape:
            raise ValueError("sample_ddpm: noise_p %s is not [K_step = %d] + x %s" % (tuple(noise_p.shape), K, shape))
        chunk = max(1, int(noise_cap_bytes) // (4 * max(x.numel(), 1)))
        done = 0
        while done < K:
            n = min(chunk, K - done)
            if noise_p is not None:
                z = noise_p[done:done + n]
            else:
                z = torch.empty((n,) + shape, dtype=torch.float32, device=self.device)
                for k in range(n):
                    z[k] = torch.randn(shape, device=self.device)
            x = self.denoise_fn.ddpm_sample(x, cond, self._ddpm_tables, K - 1 - done, n, z, clip_denoised=clip_denoised,
                                            use_graph=use_graph)
            done += n
        return x

    def _ancestral(self):
        return not self.cfg.get("pndm_speedup")

    def _infer_x0(self, fs2_mels, cond, noise, gaussian_start, noise_start, noise_p, clip_denoised):
        fs2_mels = fs2_mels.to(device=self.device, dtype=torch.float32)
        x0 = self.norm_spec(fs2_mels).transpose(1, 2)[:, None, :, :]
        t = torch.tensor([self.K_step - 1], device=self.device).long()
        x = self.q_sample(x0, t, noise)
        if gaussian_start is None:
            gaussian_start = bool(self.cfg.get("gaussian_start"))
        if gaussian_start:
            shape = (cond.shape[0], 1, self.mel_bins, cond.shape[2])
            x = torch.randn(shape, device=self.device) if noise_start is None else noise_start.to(self.device).reshape(shape)
        if self._ancestral():
            x = self.sample_ddpm(x, cond, noise_p=noise_p, clip_denoised=clip_denoised)
        else:
            x = self.sample_plms(x, cond)
        return x[:, 0].transpose(1, 2)

    @torch.no_grad()
    def infer(self, fs2_mels, cond, noise=None, gaussian_start=None, mel2ph=None, noise_start=None, noise_p=None,
              clip_denoised=True):
        """The infer branch of forward (:244-276) after the FastSpeech2 front end: fs2_mels [B, T, M] (ret['mel_out'] of
        fs2), cond [B, H, T] (ret['decoder_inp'].transpose(1, 2)) -> mel_out [B, T, M]; with mel2ph [B, T] (singing) the
        frames that belong to no phoneme are zeroed (:273-274).  The loop is the PLMS one with a truthy cfg['pndm_speedup'], the
        ancestral chain (sample_ddpm) otherwise.  gaussian_start: None takes cfg['gaussian_start'].

        Draws, in the reference's order, each made on the device from torch's global generator unless given: `noise` of
        q_sample (made even when gaussian_start discards its result), `noise_start` [B, 1, M, T] with gaussian_start, then --
        ancestral chain only -- `noise_p` [K_step, B, 1, M, T], one draw per step in loop order."""
        out = self.denorm_spec(self._infer_x0(fs2_mels, cond, noise, gaussian_start, noise_start, noise_p, clip_denoised))
        if mel2ph is not None:
            out = out * (torch.as_tensor(mel2ph).to(out.device) > 0).float()[:, :, None]
        return out


class OfflineGaussianDiffusion(GaussianDiffusion):
    """shallow_diffusion_tts.py:292-324: the coarse mel comes with the batch (ref_mels[1]) and the loop is always the ancestral
    chain, whatever cfg['pndm_speedup'] says; mel2ph masks nothing here (:322-323)."""

    def _ancestral(self):
        return True

    @torch.no_grad()
    def infer(self, fs2_mels, cond, noise=None, gaussian_start=None, mel2ph=None, noise_start=None, noise_p=None,
              clip_denoised=True):
        return self.denorm_spec(self._infer_x0(fs2_mels, cond, noise, gaussian_start, noise_start, noise_p, clip_denoised))


class PitchExtractor(object):
    """modules/fastspeech/pe.py:119-149 with the reference's call surface: `pe(mel_out)['f0_denorm_pred']`.  cfg: the hparams
    it reads (config.PITCH_EXTRACTOR); state_dict: the checkpoint's (a `model.` prefix is stripped), seeded random weights when
    None.  ctx: an existing Context, e.g. the diffusion's, so the stages share one stream."""

    def __init__(self, cfg=None, device="cuda:0", state_dict=None, ctx=None, precision=None, seed=13):
        self.cfg = dict(cfg or C.PITCH_EXTRACTOR)
        backend.pe_config(self.cfg)                    # refuses an unsupported configuration before a context is made
        self.ctx = ctx or Context(device, precision=precision or default_precision())
        self.device = self.ctx.device
        sd = state_dict if state_dict is not None else WT.make_pe_state_dict(self.cfg, seed=seed)
        sd = WT.strip_prefix(sd, "model.") or sd
        self.net = backend.PitchExtractor(self.ctx, self.cfg, sd)

    @torch.no_grad()
    def forward(self, mel_input=None):
        """mel_input [B, T, n_mel_bins] -> {'pitch_pred' [B, T, 2], 'f0_denorm_pred' [B, T]}, device tensors."""
        pitch_pred, f0 = self.net.forward(mel_input)
        return {"pitch_pred": pitch_pred, "f0_denorm_pred": f0}

    __call__ = forward

    def eval(self):
        return self

    def to(self, *args, **kwargs):
        return self


class FastSpeech2MIDI(object):
    """modules/diffsinger_midi/fs2.py:46-118 with the reference's call surface: `fs2(txt_tokens, infer=True, pitch_midi=...,
    midi_dur=..., is_slur=...)` -> the reference's dict, device tensors.  cfg: the hparams it reads (config.FASTSPEECH2_MIDI);
    state_dict: the checkpoint's (a `model.fs2.` or `fs2.` prefix is stripped), seeded random weights when None.  ctx: an existing
    Context, e.g. the diffusion's, so the stages share one stream.

    The network runs as two device calls, encode (tokens -> encoder_out, durations) and decode (mel2ph -> decoder_inp, mel_out);
    T_mel = max_b sum(dur) sizes decode's outputs, so with predicted durations the B per-sample totals are read back between the
    two: the single device-to-host read per utterance.  With a caller's mel2ph there is none.

    The integer inputs are checked on the host, where preprocess_input leaves them (a tensor handed over on the device is copied
    back for that): tokens in [0, vocab_size), pitch_midi in [0, 300), is_slur in {0, 1}, a live token in every sample, a given
    mel2ph within [0, T_txt] with a frame per sample.  A sample whose predicted durations sum to 0 frames is refused: the
    reference's decoder has no visible key there and returns NaN."""

    def __init__(self, cfg=None, device="cuda:0", state_dict=None, ctx=None, precision=None, seed=17):
        self.cfg = dict(cfg or C.FASTSPEECH2_MIDI)
        backend.fs2_config(self.cfg)                   # refuses an unsupported configuration before a context is made
        self.ctx = ctx or Context(device, precision=precision or default_precision())
        self.device = self.ctx.device
        sd = state_dict if state_dict is not None else WT.make_fs2_state_dict(self.cfg, seed=seed)
        sd = WT.strip_prefix(sd, "model.fs2.") or WT.strip_prefix(sd, "fs2.") or sd
        self.net = backend.FastSpeech2MIDI(self.ctx, self.cfg, sd)

    def _check(self, txt_tokens, pitch_midi, is_slur, mel2ph):
        what = "FastSpeech2MIDI"
        tok = torch.as_tensor(txt_tokens).cpu()
        if tok.dim() != 2 or tok.shape[0] < 1 or tok.shape[1] < 1:
            raise ValueError("%s: txt_tokens %s is not [B, T_txt]" % (what, tuple(tok.shape)))
        V = int(self.cfg["vocab_size"])
        if int(tok.min()) < 0 or int(tok.max()) >= V:
            raise ValueError("%s: txt_tokens outside [0, vocab_size = %d): the token table has no such row" % (what, V))
        if not bool((tok > 0).any(dim=1).all()):
            raise ValueError("%s: a sample with no live token (all padding, token 0): its attention has no visible key" % what)
        if pitch_midi is None:
            raise ValueError("%s: pitch_midi is required (fs2.py:60)" % what)
        midi = torch.as_tensor(pitch_midi).cpu()
        if int(midi.min()) < 0 or int(midi.max()) >= 300:
            raise ValueError("%s: pitch_midi outside [0, 300): midi_embed has 300 rows" % what)
        if is_slur is not None:
            sl = torch.as_tensor(is_slur).cpu()
            if int(sl.min()) < 0 or int(sl.max()) > 1:
                raise ValueError("%s: is_slur outside {0, 1}: is_slur_embed has 2 rows" % what)
        if mel2ph is not None:
            m = torch.as_tensor(mel2ph).cpu()
            if m.dim() != 2 or m.shape[0] != tok.shape[0] or m.shape[1] < 1:
                raise ValueError("%s: mel2ph %s is not [B = %d, T_mel]" % (what, tuple(m.shape), tok.shape[0]))
            if int(m.min()) < 0 or int(m.max()) > tok.shape[1]:
                raise ValueError("%s: mel2ph outside [0, T_txt = %d]: a frame points at no token" % (what, tok.shape[1]))
            if not bool((m > 0).any(dim=1).all()):
                raise ValueError("%s: a sample whose mel2ph is all 0: no frame, its decoder has no visible key" % what)

    @torch.no_grad()
    def forward(self, txt_tokens, mel2ph=None, skip_decoder=False, infer=True, pitch_midi=None, midi_dur=None, is_slur=None):
        """-> {'decoder_inp' [B, T_mel, H], 'mel2ph' [B, T_mel] long, 'dur', 'mel_out' [B, T_mel, 80] unless skip_decoder}, and
        'dur_choice' [B, T_txt] long when mel2ph was predicted.  'dur' is the duration predictor's log-domain output: [B, T_txt, 1]
        when mel2ph was predicted, [B, T_txt] when it was given, as the reference returns it."""
        if not infer:
            raise ValueError("FastSpeech2MIDI: only infer=True is built (no dropout, no losses)")
        self._check(txt_tokens, pitch_midi, is_slur, mel2ph)
        enc, xs, dur, totals = self.net.encode(txt_tokens, pitch_midi, midi_dur, is_slur)
        ret = {}
        if mel2ph is None:
            tot = totals.cpu()                         # the one device-to-host read: T_mel sizes everything after it
            if int(tot.min()) < 1:
                raise ValueError("FastSpeech2MIDI: the predicted durations of sample %d sum to 0 frames: the reference's decoder "
                                 "returns NaN there" % int(tot.argmin()))
            m2p = self.net.length_regulate(dur, int(tot.max()))
            ret["dur"], ret["dur_choice"] = xs[:, :, None], dur.long()
        else:
            m2p = torch.as_tensor(mel2ph).to(device=self.device, dtype=torch.int32)
            ret["dur"] = xs
        ret["mel2ph"] = m2p.long()
        ret["decoder_inp"], mel_out = self.net.decode(enc, m2p, skip_decoder=skip_decoder)
        if not skip_decoder:
            ret["mel_out"] = mel_out
        return ret

    __call__ = forward

    def eval(self):
        return self

    def to(self, *args, **kwargs):
        return self


class FastSpeech2MIDICascade(FastSpeech2MIDI):
    """FastSpeech2MIDI with use_pitch_embed, as the cascade singing configuration runs it (inference/svs/ds_cascade.py over
    midi/cascade/opencs/ds60_rel.yaml; modules/fastspeech/fs2.py:125-132,174-220, pitch_type 'frame'): after the expand, a
    PitchPredictor reads the frames, denorm_f0 and f0_to_coarse pick a row of pitch_embed, and that row is added to decoder_inp
    before the decoder.  cfg: config.FASTSPEECH2_MIDI_CASCADE; state_dict: the reference's full FastSpeech2MIDI state dict (a
    `model.fs2.` or `fs2.` prefix is stripped), seeded random weights when None.

    Two handles on one context: a backend.FastSpeech2MIDI built from the cfg with use_pitch_embed cleared, and a backend.FS2Pitch.
    Device calls, in order: encode -> (the totals read, with predicted durations: still the single device-to-host read) ->
    length_regulate -> decode without the decoder -> the pitch branch -> run_decoder.

    f0 [B, T_mel] is the NORMALISED pitch the reference takes (log2 Hz with pitch_norm 'log'), uv [B, T_mel] its unvoiced flags
    (> 0: unvoiced); each may be None and is then predicted.  The reference zeroes the caller's f0 in place on padding frames
    (fs2.py:215-216); here the caller's tensors are only read."""

    def __init__(self, cfg=None, device="cuda:0", state_dict=None, ctx=None, precision=None, seed=17):
        self.cfg = dict(cfg or C.FASTSPEECH2_MIDI_CASCADE)
        if not self.cfg.get("use_pitch_embed"):
            raise backend.L.MaaError("FastSpeech2MIDICascade: use_pitch_embed is false in this configuration: that is FastSpeech2MIDI")
        inner = dict(self.cfg, use_pitch_embed=False)
        backend.fs2_pitch_config(self.cfg)             # both refuse an unsupported configuration before a context is made
        backend.fs2_config(inner)
        self.ctx = ctx or Context(device, precision=precision or default_precision())
        self.device = self.ctx.device
        sd = state_dict if state_dict is not None else WT.make_fs2_state_dict(self.cfg, seed=seed)
        sd = WT.strip_prefix(sd, "model.fs2.") or WT.strip_prefix(sd, "fs2.") or sd
        is_pitch = lambda k: k.startswith(("pitch_embed.", "pitch_predictor."))      # noqa: E731
        self.net = backend.FastSpeech2MIDI(self.ctx, inner, {k: v for k, v in sd.items() if not is_pitch(k)})
        self.pitch = backend.FS2Pitch(self.ctx, self.cfg, {k: v for k, v in sd.items() if is_pitch(k)})

    @torch.no_grad()
    def forward(self, txt_tokens, mel2ph=None, f0=None, uv=None, skip_decoder=False, infer=True, pitch_midi=None, midi_dur=None,
                is_slur=None):
        """-> FastSpeech2MIDI.forward's dict with decoder_inp carrying the pitch embedding, plus 'pitch_pred' [B, T_mel, 2] (value
        and voicing logit; the value is 0 on padding frames when f0 was predicted, as in the reference) and 'f0_denorm' [B, T_mel]
        (Hz; 0 on unvoiced and padding frames) -- what ds_cascade.py hands the NSF vocoder."""
        ret = super().forward(txt_tokens, mel2ph=mel2ph, skip_decoder=True, infer=infer, pitch_midi=pitch_midi, midi_dur=midi_dur,
                              is_slur=is_slur)
        B, T_mel = ret["mel2ph"].shape
        for name, t in (("f0", f0), ("uv", uv)):
            if t is not None and tuple(torch.as_tensor(t).shape) != (B, T_mel):
                raise ValueError("FastSpeech2MIDICascade: %s %s is not [B = %d, T_mel = %d]" % (name, tuple(torch.as_tensor(t).shape), B, T_mel))
        ret["decoder_inp"], ret["pitch_pred"], ret["f0_denorm"] = self.pitch.forward(ret["decoder_inp"], ret["mel2ph"], f0=f0, uv=uv)
        if not skip_decoder:
            ret["mel_out"] = self.net.run_decoder(ret["decoder_inp"], ret["mel2ph"])
        return ret

    __call__ = forward


class FastSpeech2(object):
    """modules/fastspeech/fs2.py:22-226 with the reference's call surface, inference only: `fs2(txt_tokens, mel2ph=None,
    spk_embed=None, ref_mels=None, f0=None, uv=None, energy=None, skip_decoder=False, spk_embed_dur_id=None, spk_embed_f0_id=None,
    infer=True)` -> the reference's dict, device tensors: 'dur', 'dur_choice' (predicted durations), 'mel2ph', 'pitch_pred' and
    'f0_denorm' (use_pitch_embed), 'energy_pred' (use_energy_embed), 'decoder_inp', 'mel_out' (unless skip_decoder).  This is the
    `fs2` of every configuration without use_midi: the TTS ones (config.FASTSPEECH2, FASTSPEECH2_LIBRITTS) and both *_ds_beta6
    chains.  state_dict: the checkpoint's (a `model.fs2.` or `fs2.` prefix is stripped), seeded random weights when None.

    Two handles on one context: a backend.FastSpeech2Plain (encoder with token-counted sinusoid positions, or rel_pos; speakers;
    the energy branch) and, with use_pitch_embed, a backend.FS2Pitch built from a cfg copy with the energy / speaker keys cleared.
    Device calls, in order: [speaker] -> encode -> (the totals read, with predicted durations: the single device-to-host read) ->
    length_regulate -> decode without the decoder -> [add_speaker] -> [the pitch branch] -> [finish] -> run_decoder.

    spk_embed: int ids [B] with use_spk_id (spk_embed_dur_id / spk_embed_f0_id too, read with use_split_spk_id only), a float
    [B, 256] vector with use_spk_embed.  f0 / uv as FastSpeech2MIDICascade takes them; energy [B, T_mel] >= 0 replaces the
    prediction.  Checked on the host, where the caller's preprocessing leaves them (a device tensor is copied back for that):
    tokens, speaker ids in [0, num_spk], mel2ph, energy >= 0.  The caller's f0, uv and energy are only read.

    One divergence: a NEGATIVE predicted energy raises IndexError in the reference (on any frame, padding included: the table is
    indexed with floor(64 e)); here such a frame takes row 0 of energy_embed.

    Not built, refused with the reason: pitch_type 'ph' / 'cwt', pitch_ar, use_bert, use_pos_embed false; the text front end
    (text -> txt_tokens) is the caller's."""

    def __init__(self, cfg=None, device="cuda:0", state_dict=None, ctx=None, precision=None, seed=19):
        self.cfg = dict(cfg or C.FASTSPEECH2)
        inner = dict(self.cfg, use_pitch_embed=False)
        backend.fs2_plain_config(inner)                # both refuse an unsupported configuration before a context is made
        self.use_pitch = bool(self.cfg.get("use_pitch_embed", False))
        pitch_cfg = dict(self.cfg, use_energy_embed=False, use_spk_id=False, use_spk_embed=False)
        if self.use_pitch:
            backend.fs2_pitch_config(pitch_cfg)
        self.use_energy = bool(self.cfg.get("use_energy_embed", False))
        self.spk_mode = "id" if self.cfg.get("use_spk_id") else "embed" if self.cfg.get("use_spk_embed") else None
        self.ctx = ctx or Context(device, precision=precision or default_precision())
        self.device = self.ctx.device
        sd = state_dict if state_dict is not None else WT.make_fs2_plain_state_dict(self.cfg, seed=seed)
        sd = WT.strip_prefix(sd, "model.fs2.") or WT.strip_prefix(sd, "fs2.") or sd
        is_pitch = lambda k: k.startswith(("pitch_embed.", "pitch_predictor."))      # noqa: E731
        self.net = backend.FastSpeech2Plain(self.ctx, inner, {k: v for k, v in sd.items() if not is_pitch(k)})
        self.pitch = backend.FS2Pitch(self.ctx, pitch_cfg, {k: v for k, v in sd.items() if is_pitch(k)}) if self.use_pitch else None

    def _check_tokens(self, txt_tokens, mel2ph):
        what = "FastSpeech2"
        tok = torch.as_tensor(txt_tokens).cpu()
        if tok.dim() != 2 or tok.shape[0] < 1 or tok.shape[1] < 1:
            raise ValueError("%s: txt_tokens %s is not [B, T_txt]" % (what, tuple(tok.shape)))
        V = int(self.cfg["vocab_size"])
        if int(tok.min()) < 0 or int(tok.max()) >= V:
            raise ValueError("%s: txt_tokens outside [0, vocab_size = %d): the token table has no such row" % (what, V))
        if not bool((tok > 0).any(dim=1).all()):
            raise ValueError("%s: a sample with no live token (all padding, token 0): its attention has no visible key" % what)
        if mel2ph is not None:
            m = torch.as_tensor(mel2ph).cpu()
            if m.dim() != 2 or m.shape[0] != tok.shape[0] or m.shape[1] < 1:
                raise ValueError("%s: mel2ph %s is not [B = %d, T_mel]" % (what, tuple(m.shape), tok.shape[0]))
            if int(m.min()) < 0 or int(m.max()) > tok.shape[1]:
                raise ValueError("%s: mel2ph outside [0, T_txt = %d]: a frame points at no token" % (what, tok.shape[1]))
            if not bool((m > 0).any(dim=1).all()):
                raise ValueError("%s: a sample whose mel2ph is all 0: no frame, its decoder has no visible key" % what)
        return int(tok.shape[0])

    def _speaker_ids(self, spk_embed, spk_embed_dur_id, spk_embed_f0_id, B):
        """The [3, B] ids of a use_spk_id model (fs2.py:99-104: the dur / f0 ids default to the speaker's), checked on the host."""
        what, n = "FastSpeech2", int(self.cfg["num_spk"])
        if spk_embed is None:
            raise ValueError("%s: use_spk_id needs spk_embed, the speaker ids [B]" % what)
        rows = []
        for name, t in (("spk_embed", spk_embed), ("spk_embed_dur_id", spk_embed_dur_id), ("spk_embed_f0_id", spk_embed_f0_id)):
            t = torch.as_tensor(spk_embed if t is None else t).cpu()
            if t.is_floating_point() or tuple(t.reshape(-1).shape) != (B,):
                raise ValueError("%s: %s %s %s is not integer ids [B = %d]" % (what, name, t.dtype, tuple(t.shape), B))
            if int(t.min()) < 0 or int(t.max()) > n:
                raise ValueError("%s: %s outside [0, num_spk = %d]: the speaker table has no such row" % (what, name, n))
            rows.append(t.reshape(-1).long())
        return torch.stack(rows)

    @torch.no_grad()
    def forward(self, txt_tokens, mel2ph=None, spk_embed=None, ref_mels=None, f0=None, uv=None, energy=None, skip_decoder=False,
                spk_embed_dur_id=None, spk_embed_f0_id=None, infer=True):
        if not infer:
            raise ValueError("FastSpeech2: only infer=True is built (no dropout, no losses)")
        B = self._check_tokens(txt_tokens, mel2ph)
        if energy is not None and self.use_energy and not bool((torch.as_tensor(energy).cpu() >= 0).all()):
            raise ValueError("FastSpeech2: energy below 0 (or NaN): energy_embed has no such row -- the reference raises IndexError")
        sp = None
        if self.spk_mode == "id":
            ids = self._speaker_ids(spk_embed, spk_embed_dur_id, spk_embed_f0_id, B)
            sp = self.net.speaker(ids=ids)
        elif self.spk_mode == "embed":
            if spk_embed is None or tuple(torch.as_tensor(spk_embed).shape) != (B, 256):
                raise ValueError("FastSpeech2: use_spk_embed needs spk_embed [B = %d, 256]" % B)
            sp = self.net.speaker(vec=spk_embed)
        enc, xs, dur, totals = self.net.encode(txt_tokens, spk_dur=sp[1] if sp is not None else None)
        ret = {}
        if mel2ph is None:
            tot = self._read_totals(totals)            # the one device-to-host read: T_mel sizes everything after it
            if int(tot.min()) < 1:
                raise ValueError("FastSpeech2: the predicted durations of sample %d sum to 0 frames: the reference's decoder "
                                 "returns NaN there" % int(tot.argmin()))
            m2p = self.net.length_regulate(dur, int(tot.max()))
            ret["dur"], ret["dur_choice"] = xs[:, :, None], dur.long()
        else:
            m2p = torch.as_tensor(mel2ph).to(device=self.device, dtype=torch.int32)
            ret["dur"] = xs
        ret["mel2ph"] = m2p.long()
        T_mel = int(m2p.shape[1])
        for name, t in (("f0", f0), ("uv", uv), ("energy", energy)):
            if t is not None and tuple(torch.as_tensor(t).shape) != (B, T_mel):
                raise ValueError("FastSpeech2: %s %s is not [B = %d, T_mel = %d]" % (name, tuple(torch.as_tensor(t).shape), B, T_mel))
        origin, _ = self.net.decode(enc, m2p, skip_decoder=True)
        pred_inp = self.net.add_speaker(origin, sp[2], m2p) if sp is not None else origin
        acc = origin
        if self.use_pitch:
            acc, ret["pitch_pred"], ret["f0_denorm"] = self.pitch.forward(origin, m2p, f0=f0, uv=uv,
                                                                         pred_inp=pred_inp if sp is not None else None)
        if self.use_energy or sp is not None:
            acc, energy_pred = self.net.finish(pred_inp, acc, m2p, energy=energy, spk=sp[0] if sp is not None else None)
            if self.use_energy:
                ret["energy_pred"] = energy_pred
        ret["decoder_inp"] = acc                       # (without energy and speakers the tail is acc * tgt = acc: no launch)
        if not skip_decoder:
            ret["mel_out"] = self.net.run_decoder(acc, m2p)
        return ret

    @staticmethod
    def _read_totals(totals):
        return totals.cpu()

    __call__ = forward

    def eval(self):
        return self

    def to(self, *args, **kwargs):
        return self


class DiffSingerE2E(object):
    """DiffSingerE2EInfer.forward_model (inference/svs/ds_e2e.py:22-45) with BaseSVSInfer.run_vocoder (base_svs_infer.py:61-70):
    score -> (fs2, when set) decoder_inp, mel2ph, coarse mel -> the diffusion's mel_out -> f0 (pe, when set) -> waveform.
    diffusion: a GaussianDiffusion; vocoder: a backend.Vocoder (forward / forward_f0) on the same device; use_nsf:
    hparams['use_nsf']; fs2: a FastSpeech2MIDI on the same device, needed by forward_model only."""

    def __init__(self, diffusion, vocoder, pe=None, use_nsf=True, fs2=None):
        self.diffusion, self.vocoder, self.pe, self.use_nsf, self.fs2 = diffusion, vocoder, pe, bool(use_nsf), fs2

    @torch.no_grad()
    def run_vocoder(self, c, f0=None, **draws):
        """c [B, T, 80], f0 [B, T] or None -> [1, B * T * hop].  The NSF branch runs only with f0 given and use_nsf; draws:
        SineGen's rand_ini / noise, passed to forward_f0."""
        c = c.transpose(2, 1)
        if f0 is not None and self.use_nsf:
            y = self.vocoder.forward_f0(c, f0, **draws).reshape(-1)
        else:
            y = self.vocoder.forward(c).reshape(-1)
        return y[None]

    @torch.no_grad()
    def mel_to_wav(self, mel_out, **draws):
        f0 = self.pe(mel_out)["f0_denorm_pred"] if self.pe is not None else None
        return self.run_vocoder(mel_out, f0=f0, **draws)

    @torch.no_grad()
    def infer(self, fs2_mels, cond, mel2ph=None, rand_ini=None, noise_sine=None, **kw):
        """diffusion.infer(fs2_mels, cond, mel2ph=mel2ph, **kw) followed by mel_to_wav.  rand_ini / noise_sine: SineGen's two draws
        (`noise` is q_sample's draw of diffusion.infer)."""
        mel_out = self.diffusion.infer(fs2_mels, cond, mel2ph=mel2ph, **kw)
        return self.mel_to_wav(mel_out, **self._sine_draws(rand_ini, noise_sine))

    @staticmethod
    def _sine_draws(rand_ini, noise_sine):
        draws = {}
        if rand_ini is not None:
            draws["rand_ini"] = rand_ini
        if noise_sine is not None:
            draws["noise"] = noise_sine
        return draws

    @torch.no_grad()
    def forward_model(self, txt_tokens, pitch_midi, midi_dur, is_slur, mel2ph=None, **draws):
        """Score -> [1, B * T_mel * hop]: the front end, then infer with cond = its decoder_inp as [B, H, T_mel] (a device
        transpose, no host round trip) and fs2_mels = its mel_out.  As shallow_diffusion_tts.py:273-276 the final mask uses the
        ARGUMENT mel2ph: predicted durations (mel2ph None) leave the mel unmasked.  draws: as infer takes them."""
        if self.fs2 is None:
            raise ValueError("DiffSingerE2E.forward_model needs the front end: pass fs2=FastSpeech2MIDI(...)")
        ret = self.fs2(txt_tokens, mel2ph=mel2ph, infer=True, pitch_midi=pitch_midi, midi_dur=midi_dur, is_slur=is_slur)
        return self.infer(ret["mel_out"], ret["decoder_inp"].transpose(1, 2), mel2ph=mel2ph, **draws)


class DiffSingerCascade(DiffSingerE2E):
    """DiffSingerCascadeInfer.forward_model (inference/svs/ds_cascade.py:22-34): the front end predicts the pitch itself
    (pe_enable false, no PitchExtractor), and its f0_denorm goes straight to the NSF vocoder with the diffusion's mel.
    diffusion / vocoder / use_nsf: as DiffSingerE2E, whose run_vocoder this shares; fs2: a FastSpeech2MIDICascade on the same
    device.  Nothing leaves the device between score and waveform except the durations' totals."""

    def __init__(self, diffusion, vocoder, fs2, use_nsf=True):
        super().__init__(diffusion, vocoder, pe=None, use_nsf=use_nsf, fs2=fs2)

    @torch.no_grad()
    def forward_model(self, txt_tokens, pitch_midi, midi_dur, is_slur, mel2ph=None, f0=None, uv=None, rand_ini=None, noise_sine=None,
                      **draws):
        """Score -> [1, B * T_mel * hop].  mel2ph / f0 / uv: a caller's, else predicted (FastSpeech2MIDICascade); the final mask
        of the diffusion uses the ARGUMENT mel2ph, as DiffSingerE2E.forward_model.  rand_ini / noise_sine: SineGen's two draws;
        draws: as GaussianDiffusion.infer takes them."""
        ret = self.fs2(txt_tokens, mel2ph=mel2ph, f0=f0, uv=uv, infer=True, pitch_midi=pitch_midi, midi_dur=midi_dur, is_slur=is_slur)
        mel_out = self.diffusion.infer(ret["mel_out"], ret["decoder_inp"].transpose(1, 2), mel2ph=mel2ph, **draws)
        return self.run_vocoder(mel_out, f0=ret["f0_denorm"], **self._sine_draws(rand_ini, noise_sine))


class DiffSpeech(DiffSingerE2E):
    """GaussianDiffusion.forward(infer=True) of the configurations without use_midi (shallow_diffusion_tts.py:236-277 over the
    plain FastSpeech2: lj_ds_beta6.yaml, popcs_ds_beta6.yaml) followed by run_vocoder: text tokens -> waveform with no model on
    the host.  diffusion: a GaussianDiffusion (config.DIFFSPEECH_LJ_BETA6, DIFFSINGER_POPCS_BETA6); vocoder / use_nsf: as
    DiffSingerE2E, whose run_vocoder this shares (with use_nsf the front end's f0_denorm goes to the NSF vocoder); fs2: a
    FastSpeech2 on the same device."""

    def __init__(self, diffusion, vocoder, fs2, use_nsf=False):
        super().__init__(diffusion, vocoder, pe=None, use_nsf=use_nsf, fs2=fs2)

    @torch.no_grad()
    def forward_model(self, txt_tokens, spk_embed=None, mel2ph=None, f0=None, uv=None, energy=None, rand_ini=None, noise_sine=None,
                      **draws):
        """Tokens -> [1, B * T_mel * hop].  spk_embed / mel2ph / f0 / uv / energy: as FastSpeech2.forward takes them; the final mask
        of the diffusion uses the ARGUMENT mel2ph (shallow_diffusion_tts.py:273-276), so predicted durations leave the mel unmasked.
        rand_ini / noise_sine: SineGen's two draws (use_nsf); draws: as GaussianDiffusion.infer takes them."""
        ret = self.fs2(txt_tokens, mel2ph=mel2ph, spk_embed=spk_embed, f0=f0, uv=uv, energy=energy, infer=True)
        mel_out = self.diffusion.infer(ret["mel_out"], ret["decoder_inp"].transpose(1, 2), mel2ph=mel2ph, **draws)
        f0_denorm = ret.get("f0_denorm") if self.use_nsf else None
        return self.run_vocoder(mel_out, f0=f0_denorm, **self._sine_draws(rand_ini, noise_sine))
