"""PLMSSampler with the reference's Python call signature, backed by the HIP library.

Drop-in for `ldm.models.diffusion.plms.PLMSSampler` (text_to_audio/Make_An_Audio/ldm/models/diffusion/plms.py), the second
sampler of Make-An-Audio's latent-diffusion package; it takes the place of `DDIMSampler` in the same call:

    sampler = PLMSSampler(model)
    samples, intermediates = sampler.sample(S=..., conditioning=c, batch_size=n, shape=[4, 10, 78], verbose=False,
                                            unconditional_guidance_scale=scale, unconditional_conditioning=uc,
                                            x_T=start_code)

The pseudo linear multistep trajectory runs on the device inside `maa_ldm_plms_sample`: step 0 is the pseudo improved Euler
step (two UNet evaluations), the later steps Adams-Bashforth of order up to 4 over the earlier steps' first evaluations
(plms.py:223-233); S steps make S + 1 evaluations.  Guidance, concat conditioning, `mask` / `x0` blending (plms.py:148-151) and
the `x_inter` / `pred_x0` logs every `log_every_t` steps (:163-165) are part of the device loop.  PLMS requires eta = 0
(plms.py:26-27), so the reference's per-update `noise_like` draws are multiplied by zero; they are still made, up front and in
the reference's order on the model's device (x_T if not given; per step the mask's `randn_like` in q_sample, then one draw per
update -- two at step 0), so a seeded caller's generator ends where the reference's does.  Only the q_sample draws go to the
device.

Host code inside the loop -- `score_corrector` / `corrector_kwargs`, `callback(i)` / `img_callback(pred_x0, i)`, `noise_dropout`
and `quantize_x0` -- takes `_host_loop` below: the reference's loop over `model.apply_model` (maa_unet_forward), e' formed
with torch in the reference's order and the update through `maa_ddim_update`.  A non-uniform discretisation raises
NotImplementedError, as the DDIM drop-in does.
"""
import numpy as np
import torch

from .ddim import DDIMSampler


class PLMSSampler(object):
    def __init__(self, model, schedule="linear", **kwargs):
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule
        self.device = model.device

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        """plms.py:25-56: DDIMSampler's tables with eta 0 (any other eta raises ValueError, as the reference)."""
        if ddim_eta != 0:
            raise ValueError('ddim_eta must be 0 for PLMS')
        DDIMSampler.make_schedule(self, ddim_num_steps, ddim_discretize=ddim_discretize, ddim_eta=0.0, verbose=verbose)

    @torch.no_grad()
    def sample(self,
               S,
               batch_size,
               shape,
               conditioning=None,
               callback=None,
               normals_sequence=None,
               img_callback=None,
               quantize_x0=False,
               eta=0.,
               mask=None,
               x0=None,
               temperature=1.,
               noise_dropout=0.,
               score_corrector=None,
               corrector_kwargs=None,
               verbose=True,
               x_T=None,
               log_every_t=100,
               unconditional_guidance_scale=1.,
               unconditional_conditioning=None,
               **kwargs
               ):
        if conditioning is not None and not isinstance(conditioning, dict):
            if conditioning.shape[0] != batch_size:
                print(f"Warning: Got {conditioning.shape[0]} conditionings but batch-size is {batch_size}")
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        Cc, H, W = shape
        size = (batch_size, Cc, H, W)
        if x_T is None:
            x_T = torch.randn(size, device=self.device)          # plms.py:128-129
        host_hooks = score_corrector is not None or quantize_x0 or callback is not None or img_callback is not None \
            or noise_dropout != 0.0
        if host_hooks:
            # (the loop draws in place, as the reference: dropout's own draws interleave with noise_like's)
            return self._host_loop(conditioning, x_T, callback=callback, img_callback=img_callback, quantize_denoised=quantize_x0,
                                   mask=mask, x0=x0, noise_dropout=noise_dropout, temperature=temperature,
                                   score_corrector=score_corrector, corrector_kwargs=corrector_kwargs, log_every_t=log_every_t,
                                   unconditional_guidance_scale=unconditional_guidance_scale,
                                   unconditional_conditioning=unconditional_conditioning)
        if mask is not None and x0 is None:
            raise AssertionError("mask needs x0")                # plms.py:149
        # the loop's draws in its order (plms.py:150 -> ddpm.py:273, then util.py:264-267 in each get_x_prev_and_pred_x0: two
        # at step 0, one after), made up front; only the q_sample ones enter the result (sigma = 0)
        nq = []
        for i in range(len(self.ddim_timesteps)):
            if mask is not None:
                nq.append(torch.randn(size, device=self.device))
            torch.randn(size, device=self.device)
            if i == 0:
                torch.randn(size, device=self.device)
        key = self.model.conditioning_key
        kw = dict(scale=float(unconditional_guidance_scale), log_every_t=int(log_every_t))
        if DDIMSampler._split(self) is not None:          # the model's split_input_params (ddpm_audio.py:572)
            kw["split"] = DDIMSampler._split(self)
        if key == "concat":
            kw["concat"] = conditioning          # cat([x, c], dim=1) inside the loop (ddpm.py:1404-1406)
        else:
            kw["cond"] = conditioning
            kw["uncond"] = unconditional_conditioning
        if mask is not None:
            steps = np.asarray(self.ddim_timesteps)
            kw.update(mask=mask, x0=x0, noise_q=torch.stack(nq),
                      sqrt_ac=self.model.sqrt_alphas_cumprod.detach().cpu().numpy()[steps],
                      sqrt_1mac=self.model.sqrt_one_minus_alphas_cumprod.detach().cpu().numpy()[steps])
        img, x_log, x0_log = self.model.unet.plms_sample(x_T, self.ddim_timesteps, self.ddim_alphas.numpy(),
                                                         self.ddim_alphas_prev, **kw)
        # plms.py:137, 163-165: the start point, then the logged steps
        intermediates = {"x_inter": [x_T] + list(x_log), "pred_x0": [x_T] + list(x0_log)}
        return img, intermediates

    def _host_loop(self, cond, x_T, callback, img_callback, quantize_denoised, mask, x0, noise_dropout, temperature,
                   score_corrector, corrector_kwargs, log_every_t, unconditional_guidance_scale, unconditional_conditioning):
        """plms_sampling + p_sample_plms (plms.py:115-236) one step per iteration, for the calls that put host code inside the
        loop.  Device work: the UNet passes (`apply_model` -> maa_unet_forward; the guided pass as one batch [uncond ; cond],
        plms.py:183-190) and the update (maa_ddim_update with the combined e', sigma 0); the CFG combine, e' and whatever the
        corrector does are torch arithmetic on the model's device in the reference's order, and the RNG draws are made where the
        reference makes them."""
        dev, unet, model = self.device, self.model.unet, self.model
        img = x_T.to(dev)
        b = img.shape[0]
        total = len(self.ddim_timesteps)
        alphas, alphas_prev = self.ddim_alphas.numpy(), np.asarray(self.ddim_alphas_prev, dtype=np.float32)
        somas = self.ddim_sqrt_one_minus_alphas.numpy()
        scale, uc = float(unconditional_guidance_scale), unconditional_conditioning
        time_range = np.flip(np.asarray(self.ddim_timesteps))

        def get_model_output(x, t):
            if uc is None or scale == 1.0:
                e_t = model.apply_model(x, t, cond)
            else:
                x_in, t_in = torch.cat([x] * 2), torch.cat([t] * 2)
                if isinstance(cond, dict):
                    c_in = {k: ([torch.cat([uc[k][j], cond[k][j]]) for j in range(len(cond[k]))] if isinstance(cond[k], list)
                                else torch.cat([uc[k], cond[k]])) for k in cond}
                elif isinstance(cond, list):
                    c_in = [torch.cat([uc[j], cond[j]]) for j in range(len(cond))]
                else:
                    c_in = torch.cat([uc.to(dev), cond.to(dev)])
                e_t_uncond, e_t = model.apply_model(x_in, t_in, c_in).chunk(2)
                e_t = e_t_uncond + scale * (e_t - e_t_uncond)
            if score_corrector is not None:
                assert getattr(model, "parameterization", "eps") == "eps"
                e_t = score_corrector.modify_score(model, e_t, x, t, cond, **(corrector_kwargs or {}))
            return e_t

        def get_x_prev_and_pred_x0(x, e_t, index):
            if quantize_denoised:
                # plms.py:213-214 needs a VQ first stage; Make-An-Audio's is the KL autoencoder, which has no `quantize` (the
                # reference raises the same AttributeError from this line)
                model.first_stage_model.quantize
            x_prev, pred_x0 = unet.ddim_update(x, e_t.contiguous(), None, 1.0, alphas[index], alphas_prev[index], 0.0, somas[index])
            noise = 0.0 * torch.randn(x.shape, device=dev) * temperature       # sigma_t = 0 (util.py:264-267)
            if noise_dropout > 0.0:
                noise = torch.nn.functional.dropout(noise, p=noise_dropout)
            return x_prev + noise, pred_x0

        intermediates = {"x_inter": [img], "pred_x0": [img]}
        old_eps = []
        for i, step in enumerate(time_range):
            index = total - i - 1
            ts = torch.full((b,), int(step), device=dev, dtype=torch.long)
            ts_next = torch.full((b,), int(time_range[min(i + 1, len(time_range) - 1)]), device=dev, dtype=torch.long)
            if mask is not None:
                assert x0 is not None
                img_orig = model.q_sample(x0.to(dev), ts)
                img = img_orig * mask.to(dev) + (1.0 - mask.to(dev)) * img
            e_t = get_model_output(img, ts)
            if len(old_eps) == 0:
                x_mid, _ = get_x_prev_and_pred_x0(img, e_t, index)
                e_t_next = get_model_output(x_mid, ts_next)
                e_t_prime = (e_t + e_t_next) / 2
            elif len(old_eps) == 1:
                e_t_prime = (3 * e_t - old_eps[-1]) / 2
            elif len(old_eps) == 2:
                e_t_prime = (23 * e_t - 16 * old_eps[-1] + 5 * old_eps[-2]) / 12
            else:
                e_t_prime = (55 * e_t - 59 * old_eps[-1] + 37 * old_eps[-2] - 9 * old_eps[-3]) / 24
            img, pred_x0 = get_x_prev_and_pred_x0(img, e_t_prime, index)
            old_eps.append(e_t)
            if len(old_eps) >= 4:
                old_eps.pop(0)
            if callback:
                callback(i)
            if img_callback:
                img_callback(pred_x0, i)
            if index % log_every_t == 0 or index == total - 1:
                intermediates["x_inter"].append(img)
                intermediates["pred_x0"].append(pred_x0)
        return img, intermediates
