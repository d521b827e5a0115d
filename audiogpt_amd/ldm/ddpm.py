"""The model's own ancestral sampler: LatentDiffusion_audio's DDPM chain with the reference's method surface.

`AncestralSampling` carries `register_schedule`'s buffers (ldm/models/diffusion/ddpm.py:115-155) and the methods
`predict_start_from_noise`, `q_posterior` (ddpm.py:214-227), `p_mean_variance`, `p_sample`, `p_sample_loop`,
`progressive_denoising`, `sample` and `sample_log` (ddpm_audio.py:717-917) with the reference's signatures and defaults;
`LatentDiffusionAudio` (latent_diffusion.py) inherits it.

The chain runs `num_timesteps` (1000) model evaluations per clip, t = n - 1 .. 0.  Without host hooks the whole of it runs on the
device inside `maa_ddpm_sample`: one captured step -- the UNet and one fused kernel (x_recon, clamp, posterior mean, noise, the
mask blend AFTER the step, the logs) -- replayed n - 1 times.

RNG.  The reference draws from torch's global generator on the model's device inside its Python loop: `randn(shape)` for a missing
x_T, then per step `noise_like(x.shape)` in p_sample (ddpm_audio.py:766) and, with a mask, `randn_like(x0)` in q_sample
(:874 -> ddpm.py:273) -- also at t = 0, where the first is multiplied by zero.  The device loop makes the same draws up front in
that order, so a seeded call consumes the generator exactly as the reference does.  That costs n * B * C * H * W * 4 bytes per
noise tensor: 100 MB for the 1000 steps of 8 T2A latents [8, 4, 10, 78] (twice that with a mask).  `_step_noise=(noise_p,
noise_q)`, a keyword of this port for tests, supplies the draws instead ([n, B, C, H, W] each, loop order; noise_q None without a
mask).

Host hooks -- `callback(i)`, `img_callback(img, i)`, `quantize_denoised`, and progressive_denoising's `score_corrector` /
`corrector_kwargs` and `noise_dropout > 0` -- need host code between steps: such a call takes `_host_loop`, the reference's loop
one step per iteration over `apply_model` (maa_unet_forward) and `p_sample` (maa_ddpm_update), the hooks called where the
reference calls them.  There each step's noise is drawn lazily, where the reference draws it (after the model and the corrector,
before F.dropout; q_sample's draw after the step), so that a seeded call with hooks that draw random numbers themselves still
consumes the generator as the reference does.

Guidance.  The reference's ancestral path has none (p_sample evaluates apply_model(x, t, c) once), so these methods take none;
`backend.UNet.ddpm_sample` and `MakeAnAudio.generate(sampler="ddpm", uncond=..., scale=...)` accept it as an extension.
`shorten_cond_schedule=True` (num_timesteps_cond > 1: the conditioning itself is noised per step) raises NotImplementedError;
no Make-An-Audio config sets it.
"""
import numpy as np
import torch

from ..pipeline import make_beta_schedule_linear

SCHEDULE_BUFFERS = ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1", "posterior_mean_coef2",
                    "posterior_variance", "posterior_log_variance_clipped", "log_one_minus_alphas_cumprod")


def schedule_buffers(timesteps, linear_start, linear_end, v_posterior=0.0):
    """register_schedule (ddpm.py:115-155) for the "linear" schedule: every buffer formed in fp64 numpy from the fp64 betas and
    rounded once to fp32.  Returns {name: fp32 ndarray [timesteps]} with the reference's names."""
    betas = make_beta_schedule_linear(timesteps, linear_start, linear_end)
    alphas = 1.0 - betas
    ac = np.cumprod(alphas, axis=0)
    ac_prev = np.append(1.0, ac[:-1])
    var = (1 - v_posterior) * betas * (1.0 - ac_prev) / (1.0 - ac) + v_posterior * betas
    out = dict(
        betas=betas, alphas_cumprod=ac, alphas_cumprod_prev=ac_prev,
        sqrt_alphas_cumprod=np.sqrt(ac), sqrt_one_minus_alphas_cumprod=np.sqrt(1.0 - ac),
        log_one_minus_alphas_cumprod=np.log(1.0 - ac),
        sqrt_recip_alphas_cumprod=np.sqrt(1.0 / ac), sqrt_recipm1_alphas_cumprod=np.sqrt(1.0 / ac - 1),
        posterior_variance=var, posterior_log_variance_clipped=np.log(np.maximum(var, 1e-20)),
        posterior_mean_coef1=betas * np.sqrt(ac_prev) / (1.0 - ac),
        posterior_mean_coef2=(1.0 - ac_prev) * np.sqrt(alphas) / (1.0 - ac))
    return {k: v.astype(np.float32) for k, v in out.items()}


def _extract(a, t, x_shape):
    """util.py extract_into_tensor: a.gather(-1, t) shaped to broadcast over x."""
    return a.gather(-1, t).reshape((t.shape[0],) + (1,) * (len(x_shape) - 1))


def _slice_cond(cond, batch_size):
    """ddpm_audio.py:797-802 / :892-897: the conditioning cut to the batch."""
    if cond is None:
        return None
    if isinstance(cond, dict):
        return {k: cond[k][:batch_size] if not isinstance(cond[k], list) else [x[:batch_size] for x in cond[k]] for k in cond}
    return [c[:batch_size] for c in cond] if isinstance(cond, list) else cond[:batch_size]


class AncestralSampling(object):
    """Mixin over a model with `.device`, `.unet`, `.conditioning_key`, `.apply_model`, `.q_sample`, `.first_stage_model` and
    `split_params()` (LatentDiffusionAudio); register_ancestral_schedule() gives it the rest."""

    clip_denoised = True
    parameterization = "eps"
    v_posterior = 0.0
    shorten_cond_schedule = False
    log_every_t = 200

    def register_ancestral_schedule(self, timesteps, linear_start, linear_end):
        """The buffers of register_schedule the ancestral chain reads, as fp32 tensors on the model's device under the
        reference's names (the others -- betas, alphas_cumprod(_prev), sqrt_(one_minus_)alphas_cumprod -- are the owner's)."""
        bufs = schedule_buffers(timesteps, linear_start, linear_end, self.v_posterior)
        for name in SCHEDULE_BUFFERS:
            setattr(self, name, torch.from_numpy(bufs[name]).to(self.device))
        self._ddpm_host_tables = bufs          # what backend.UNet.ddpm_sample / ddpm_update hand to the library: read on the host
        return bufs

    # ---- ddpm.py:214-227 ---------------------------------------------------------------------------
    def predict_start_from_noise(self, x_t, t, noise):
        return (_extract(self.sqrt_recip_alphas_cumprod, t, x_t.shape) * x_t -
                _extract(self.sqrt_recipm1_alphas_cumprod, t, x_t.shape) * noise)

    def q_posterior(self, x_start, x_t, t):
        posterior_mean = (_extract(self.posterior_mean_coef1, t, x_t.shape) * x_start +
                          _extract(self.posterior_mean_coef2, t, x_t.shape) * x_t)
        posterior_variance = _extract(self.posterior_variance, t, x_t.shape)
        posterior_log_variance_clipped = _extract(self.posterior_log_variance_clipped, t, x_t.shape)
        return posterior_mean, posterior_variance, posterior_log_variance_clipped

    # ---- ddpm_audio.py:717-777 ---------------------------------------------------------------------
    def _model_out(self, x, c, t, return_codebook_ids, score_corrector, corrector_kwargs):
        if return_codebook_ids:
            raise DeprecationWarning("Support dropped.")          # ddpm_audio.py:758-759
        model_out = self.apply_model(x, t, c)
        if score_corrector is not None:
            assert self.parameterization == "eps"
            model_out = score_corrector.modify_score(self, model_out, x, t, c, **(corrector_kwargs or {}))
        return model_out

    def _update(self, x, model_out, t, noise, temperature, clip_denoised, quantize_denoised):
        """x_recon, the posterior mean and mean + (t != 0) exp(0.5 logvar) (noise temperature) of one step in one kernel
        (maa_ddpm_update).  quantize_denoised needs a VQ first stage between x_recon and the mean: Make-An-Audio's is the KL
        autoencoder, which has no `quantize` -- the reference raises the same AttributeError (ddpm_audio.py:739)."""
        if quantize_denoised:
            self.first_stage_model.quantize
            raise NotImplementedError("quantize_denoised needs a VQ first stage")
        return self.unet.ddpm_update(x, model_out.contiguous(), t, self, noise, temperature=temperature, clip_denoised=clip_denoised)

    def p_mean_variance(self, x, c, t, clip_denoised: bool, return_codebook_ids=False, quantize_denoised=False,
                        return_x0=False, score_corrector=None, corrector_kwargs=None):
        model_out = self._model_out(x, c, t, return_codebook_ids, score_corrector, corrector_kwargs)
        # (the mean is the update without its noise term)
        model_mean, x_recon = self._update(x, model_out, t, torch.zeros_like(x), 0.0, clip_denoised, quantize_denoised)
        var = _extract(self.posterior_variance, t, x.shape)
        logvar = _extract(self.posterior_log_variance_clipped, t, x.shape)
        if return_x0:
            return model_mean, var, logvar, x_recon
        return model_mean, var, logvar

    @torch.no_grad()
    def p_sample(self, x, c, t, clip_denoised=False, repeat_noise=False,
                 return_codebook_ids=False, quantize_denoised=False, return_x0=False,
                 temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None):
        """One ancestral step (t may differ per sample): the model, then maa_ddpm_update.  The noise is drawn where the
        reference draws it: after the model (and the corrector), before the dropout."""
        model_out = self._model_out(x, c, t, return_codebook_ids, score_corrector, corrector_kwargs)
        if repeat_noise:          # util.py noise_like: one draw repeated over the batch
            noise = torch.randn((1,) + tuple(x.shape[1:]), device=x.device).repeat(x.shape[0], *((1,) * (x.dim() - 1)))
        else:
            noise = torch.randn(x.shape, device=x.device)
        if noise_dropout > 0.:
            # the reference drops out noise * temperature (ddpm_audio.py:766-768); the scaling commutes with the dropout's mask
            noise = torch.nn.functional.dropout(noise * temperature, p=noise_dropout)
            temperature = 1.0
        x_prev, x_recon = self._update(x, model_out, t, noise, float(temperature), clip_denoised, quantize_denoised)
        if return_x0:
            return x_prev, x_recon
        return x_prev

    # ---- the loops ---------------------------------------------------------------------------------
    def _cond_tensor(self, cond):
        if isinstance(cond, dict):
            cond = cond["c_concat" if self.conditioning_key == "concat" else "c_crossattn"]
        if isinstance(cond, (list, tuple)):
            cond = torch.cat(list(cond), 1)
        return cond

    def _ancestral(self, cond, shape, x_T, n, log_every_t, mask, x0, temperature, hooks, step_noise):
        """Both loops' body.  Returns (img, x_T, logged x, logged x_recon).  hooks: dict of the host hooks given (empty: the device
        loop)."""
        if self.shorten_cond_schedule:
            raise NotImplementedError("shorten_cond_schedule (num_timesteps_cond > 1) noises the conditioning itself every step "
                                      "(ddpm_audio.py:865-868); no Make-An-Audio config sets it and the device loop keeps the "
                                      "conditioning's K/V fixed over the trajectory")
        if mask is not None:
            assert x0 is not None          # ddpm_audio.py:825, 860
        dev = self.device
        shape = tuple(int(s) for s in shape)
        img = torch.randn(shape, device=dev) if x_T is None else x_T.to(dev)
        x_T = img
        if hooks:
            return (x_T,) + self._host_loop(cond, img, n, log_every_t, mask, x0, temperature, step_noise=step_noise, **hooks)
        if step_noise is not None:
            noise_p, noise_q = step_noise
        else:
            npp, nq = [], []
            for _ in range(n):
                npp.append(torch.randn(shape, device=dev))                       # ddpm_audio.py:766
                if mask is not None:
                    nq.append(torch.randn(x0.shape, device=dev).expand(shape))   # :874 -> ddpm.py:273 randn_like(x0)
            noise_p = torch.stack(npp)
            noise_q = torch.stack(nq) if nq else None
        kw = dict(clip_denoised=self.clip_denoised, log_every_t=int(log_every_t), temperature=temperature)
        split = self.split_params() if hasattr(self, "split_params") else getattr(self, "split_input_params", None)
        if split is not None:
            kw["split"] = split
        kw["concat" if self.conditioning_key == "concat" else "cond"] = self._cond_tensor(cond)
        if mask is not None:
            kw.update(mask=mask, x0=x0, noise_q=noise_q)
        img, x_log, x0_log = self.unet.ddpm_sample(img, self, n, noise_p=noise_p, **kw)
        return x_T, img, list(x_log), list(x0_log)

    def _host_loop(self, cond, img, n, log_every_t, mask, x0, temperature, step_noise=None, callback=None, img_callback=None,
                   quantize_denoised=False, noise_dropout=0., score_corrector=None, corrector_kwargs=None):
        """p_sample_loop / progressive_denoising (ddpm_audio.py:812-832, 863-880) one step per iteration."""
        dev = self.device
        b = img.shape[0]
        x_log, x0_log = [], []
        for v, i in enumerate(reversed(range(0, n))):
            ts = torch.full((b,), i, device=dev, dtype=torch.long)
            temp = temperature[i] if np.ndim(temperature) != 0 else temperature
            if step_noise is not None:
                model_out = self._model_out(img, cond, ts, False, score_corrector, corrector_kwargs)
                noise = step_noise[0][v].to(dev)
                if noise_dropout > 0.:
                    noise, temp = torch.nn.functional.dropout(noise * temp, p=noise_dropout), 1.0
                img, x0_partial = self._update(img, model_out, ts, noise, float(temp), self.clip_denoised, quantize_denoised)
            else:
                img, x0_partial = self.p_sample(img, cond, ts, clip_denoised=self.clip_denoised,
                                                quantize_denoised=quantize_denoised, return_x0=True, temperature=temp,
                                                noise_dropout=noise_dropout, score_corrector=score_corrector,
                                                corrector_kwargs=corrector_kwargs)
            if mask is not None:
                nq = step_noise[1][v].to(dev) if step_noise is not None else None
                img_orig = self.q_sample(x0.to(dev), ts, noise=nq)
                img = img_orig * mask.to(dev) + (1. - mask.to(dev)) * img
            if i % log_every_t == 0 or i == n - 1:
                x_log.append(img)
                x0_log.append(x0_partial)
            if callback:
                callback(i)
            if img_callback:
                img_callback(img, i)
        return img, x_log, x0_log

    @torch.no_grad()
    def progressive_denoising(self, cond, shape, verbose=True, callback=None, quantize_denoised=False,
                              img_callback=None, mask=None, x0=None, temperature=1., noise_dropout=0.,
                              score_corrector=None, corrector_kwargs=None, batch_size=None, x_T=None, start_T=None,
                              log_every_t=None, _step_noise=None):
        """ddpm_audio.py:779-833: returns (img, the clamped x_recon of the logged steps).  temperature: a float or a list indexed
        by the timestep."""
        if not log_every_t:
            log_every_t = self.log_every_t
        timesteps = self.num_timesteps
        if batch_size is not None:
            shape = [batch_size] + list(shape)
        else:
            batch_size = shape[0]
        cond = _slice_cond(cond, batch_size)
        if start_T is not None:
            timesteps = min(timesteps, start_T)
        hooks = {}
        if callback is not None:
            hooks["callback"] = callback
        if img_callback is not None:
            hooks["img_callback"] = img_callback
        if quantize_denoised:
            hooks["quantize_denoised"] = True
        if score_corrector is not None:
            hooks.update(score_corrector=score_corrector, corrector_kwargs=corrector_kwargs)
        if noise_dropout > 0.:
            hooks["noise_dropout"] = noise_dropout
        _, img, _, x0_log = self._ancestral(cond, shape, x_T, timesteps, log_every_t, mask, x0, temperature, hooks, _step_noise)
        return img, x0_log

    @torch.no_grad()
    def p_sample_loop(self, cond, shape, return_intermediates=False,
                      x_T=None, verbose=True, callback=None, timesteps=None, quantize_denoised=False,
                      mask=None, x0=None, img_callback=None, start_T=None,
                      log_every_t=None, _step_noise=None):
        """ddpm_audio.py:835-884: t = n - 1 .. 0 with n = min(timesteps or num_timesteps, start_T); the intermediates are x_T and
        the latent after every logged step."""
        if not log_every_t:
            log_every_t = self.log_every_t
        if timesteps is None:
            timesteps = self.num_timesteps
        if start_T is not None:
            timesteps = min(timesteps, start_T)
        hooks = {}
        if callback is not None:
            hooks["callback"] = callback
        if img_callback is not None:
            hooks["img_callback"] = img_callback
        if quantize_denoised:
            hooks["quantize_denoised"] = True
        x_T, img, x_log, _ = self._ancestral(cond, shape, x_T, timesteps, log_every_t, mask, x0, 1.0, hooks, _step_noise)
        if return_intermediates:
            return img, [x_T] + x_log
        return img

    @torch.no_grad()
    def sample(self, cond, batch_size=16, return_intermediates=False, x_T=None,
               verbose=True, timesteps=None, quantize_denoised=False,
               mask=None, x0=None, shape=None, **kwargs):
        """ddpm_audio.py:886-902 (kwargs are ignored there too)."""
        if shape is None:
            shape = (batch_size, self.channels, self.mel_dim, self.mel_length)
        cond = _slice_cond(cond, batch_size)
        return self.p_sample_loop(cond, shape, return_intermediates=return_intermediates, x_T=x_T, verbose=verbose,
                                  timesteps=timesteps, quantize_denoised=quantize_denoised, mask=mask, x0=x0)

    @torch.no_grad()
    def sample_log(self, cond, batch_size, ddim, ddim_steps, **kwargs):
        """ddpm_audio.py:904-917."""
        if ddim:
            from .ddim import DDIMSampler
            shape = (self.channels, self.mel_dim, self.mel_length)
            samples, intermediates = DDIMSampler(self).sample(ddim_steps, batch_size, shape, cond, verbose=False, **kwargs)
        else:
            samples, intermediates = self.sample(cond=cond, batch_size=batch_size, return_intermediates=True, **kwargs)
        return samples, intermediates
