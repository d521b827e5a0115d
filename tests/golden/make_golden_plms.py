"""Golden vectors of PLMS sampling from the REFERENCE's own PLMSSampler (run only where the reference checkout is available).

    python tests/golden/make_golden_plms.py     # needs the reference checkout (make_golden.REF); writes tests/golden/plms_*.npz

PLMSSampler.sample (text_to_audio/Make_An_Audio/ldm/models/diffusion/plms.py) runs on CPU fp32 through a minimal model shim (the
pattern of make_golden.py / make_golden_sdedit.py; LatentDiffusion itself needs pytorch_lightning), with the seeded weights of
`audiogpt_amd.weights`.  The reference's `register_buffer` moves every table to "cuda"; the subclass below overrides it to keep
them on the CPU -- the only change to the class.  Every sampling call is seeded; the noise tensors it draws are drawn again
from the same seed and stored (loop order), and so is the generator's next draw after `sample` returns, so the tests can check
the drop-in's RNG consumption without the reference.

    plms_t2a_s10             T2A UNet, latent [2, 4, 10, 78], S = 10, guidance 1.5, log_every_t 3 (samples and both logs)
    plms_t2a_orders          S = 1 (a single step: t_next == t) and S = 5 (Euler, AB2, AB3, AB4, AB4), latent [2, 4, 10, 32]
    plms_t2a_mask_s6         mask and x0 with the stored q_sample noise, S = 6 (seven steps), guidance 1.5, log_every_t 2
    plms_i2a_s4              I2A UNet (add_context_to_emb), 1-token context, guidance 3
    plms_inpaint_s4          inpaint UNet, concat conditioning, no guidance
    plms_t2a_host_hooks_s4   a deterministic score corrector (its calls' t recorded), callback and img_callback, guidance 1.5

The conditioning has COND_TOKENS tokens (the cross-attention takes any count; the tools' 77 would make the files large).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG                       # noqa: E402  (helpers and shims; not modified)
from make_golden import C, _cond               # noqa: E402

COND_TOKENS = 4
N_NEXT = 16          # how many values of the generator's next draw are stored


def _shim(unet, ldm):
    """The model surface PLMSSampler reads: the schedule buffers, q_sample (ddpm.py:272-275) and apply_model."""
    from ldm.modules.diffusionmodules.util import extract_into_tensor, make_beta_schedule
    concat = ldm["conditioning_key"] == "concat"

    class Shim:
        parameterization = "eps"            # asserted by p_sample_plms when a corrector is given

        def __init__(self):
            betas = make_beta_schedule("linear", ldm["timesteps"], ldm["linear_start"], ldm["linear_end"])
            ac = np.cumprod(1.0 - betas, axis=0)
            self.num_timesteps = ldm["timesteps"]
            self.betas = torch.tensor(betas, dtype=torch.float32)
            self.alphas_cumprod = torch.tensor(ac, dtype=torch.float32)
            self.alphas_cumprod_prev = torch.tensor(np.append(1.0, ac[:-1]), dtype=torch.float32)
            self.sqrt_alphas_cumprod = torch.tensor(np.sqrt(ac), dtype=torch.float32)
            self.sqrt_one_minus_alphas_cumprod = torch.tensor(np.sqrt(1.0 - ac), dtype=torch.float32)
            self.device = torch.device("cpu")

        def q_sample(self, x_start, t, noise=None):
            noise = torch.randn_like(x_start) if noise is None else noise
            return (extract_into_tensor(self.sqrt_alphas_cumprod, t, x_start.shape) * x_start +
                    extract_into_tensor(self.sqrt_one_minus_alphas_cumprod, t, x_start.shape) * noise)

        def apply_model(self, x, t, c):
            if concat:
                return unet(torch.cat([x] + [c], dim=1), t)          # ddpm.py:1404-1406
            return unet(x, t, context=c)

    return Shim()


def _sampler(unet, ldm=None):
    from ldm.models.diffusion.plms import PLMSSampler

    class CpuPLMSSampler(PLMSSampler):
        def register_buffer(self, name, attr):           # the reference's moves tensors to "cuda"; keep them on the CPU
            setattr(self, name, attr)

    shim = _shim(unet, ldm or C.LDM_T2A)
    return CpuPLMSSampler(shim), shim


def _draws(size, n_steps, masked, seed):
    """The reference loop's draws after x_T, repeated from the seed: per step randn_like(x0) in q_sample when masked, then one
    noise_like per update (two at step 0); and the generator's next draw after them."""
    torch.manual_seed(seed)
    nq = []
    for i in range(n_steps):
        if masked:
            nq.append(torch.randn(size))
        torch.randn(size)
        if i == 0:
            torch.randn(size)
    return nq, torch.randn(N_NEXT)


def _run(sampler, seed, **kw):
    torch.manual_seed(seed)
    with torch.no_grad():
        z, inter = sampler.sample(verbose=False, **kw)
    nxt = torch.randn(N_NEXT)
    return z, inter, nxt


def _tables(sampler):
    return dict(ddim_timesteps=np.asarray(sampler.ddim_timesteps), ddim_alphas=sampler.ddim_alphas.numpy(),
                ddim_alphas_prev=np.asarray(sampler.ddim_alphas_prev, dtype=np.float32),
                ddim_sqrt_one_minus_alphas=np.asarray(sampler.ddim_sqrt_one_minus_alphas, dtype=np.float32))


def _logs(inter):
    """The logged steps (x_inter / pred_x0 without their first entry, which is x_T itself: plms.py:137)."""
    return dict(x_log=np.stack([t.numpy() for t in inter["x_inter"][1:]]), x0_log=np.stack([t.numpy() for t in inter["pred_x0"][1:]]))


def t2a_case(name, unet, S=10, scale=1.5, log_every_t=3, seed=501, W=78):
    sampler, _ = _sampler(unet)
    B = 2
    x_T = torch.from_numpy(np.random.RandomState(58).randn(B, 4, 10, W)).float()
    c, uc = _cond(B, COND_TOKENS, 1240), _cond(B, COND_TOKENS, 1241)
    z, inter, nxt = _run(sampler, seed, S=S, conditioning=c, batch_size=B, shape=[4, 10, W], unconditional_guidance_scale=scale,
                         unconditional_conditioning=uc, x_T=x_T, log_every_t=log_every_t)
    _, nxt2 = _draws(x_T.shape, len(sampler.ddim_timesteps), False, seed)
    assert torch.equal(nxt, nxt2)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), x_T=x_T.numpy(), c=c.numpy(), uc=uc.numpy(), z=z.numpy(), **_logs(inter),
                        **_tables(sampler), next_draw=nxt.numpy(), S=S, scale=scale, log_every_t=log_every_t, seed=seed)
    print(name, "z std", float(z.std()), "logged", len(inter["x_inter"]))


def orders_case(name, unet, scale=1.5, seed=511, W=32):
    B = 2
    x_T = torch.from_numpy(np.random.RandomState(59).randn(B, 4, 10, W)).float()
    c, uc = _cond(B, COND_TOKENS, 1242), _cond(B, COND_TOKENS, 1243)
    out = dict(x_T=x_T.numpy(), c=c.numpy(), uc=uc.numpy(), scale=scale, seed=seed)
    for S in (1, 5):
        sampler, _ = _sampler(unet)
        z, inter, nxt = _run(sampler, seed, S=S, conditioning=c, batch_size=B, shape=[4, 10, W], unconditional_guidance_scale=scale,
                             unconditional_conditioning=uc, x_T=x_T, log_every_t=1)
        assert len(sampler.ddim_timesteps) == S
        out.update({f"z_s{S}": z.numpy(), f"x_log_s{S}": _logs(inter)["x_log"], f"x0_log_s{S}": _logs(inter)["x0_log"],
                    f"ddim_timesteps_s{S}": np.asarray(sampler.ddim_timesteps), f"next_draw_s{S}": nxt.numpy()})
        print(name, "S", S, "z std", float(z.std()))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)


def mask_case(name, unet, S=6, scale=1.5, log_every_t=2, seed=521, W=32):
    sampler, shim = _sampler(unet)
    B = 2
    x_T = torch.from_numpy(np.random.RandomState(60).randn(B, 4, 10, W)).float()
    g = torch.Generator().manual_seed(79)
    x0 = torch.randn(B, 4, 10, W, generator=g)
    mask = torch.zeros(B, 1, 10, W)
    mask[0, :, :, 5:17] = 1.0
    mask[1, :, 2:7, 20:] = 1.0
    c, uc = _cond(B, COND_TOKENS, 1244), _cond(B, COND_TOKENS, 1245)
    z, inter, nxt = _run(sampler, seed, S=S, conditioning=c, batch_size=B, shape=[4, 10, W], mask=mask, x0=x0,
                         unconditional_guidance_scale=scale, unconditional_conditioning=uc, x_T=x_T, log_every_t=log_every_t)
    nq, nxt2 = _draws(x_T.shape, len(sampler.ddim_timesteps), True, seed)
    assert torch.equal(nxt, nxt2)
    steps = np.asarray(sampler.ddim_timesteps)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), x_T=x_T.numpy(), x0=x0.numpy(), mask=mask.numpy(), c=c.numpy(),
                        uc=uc.numpy(), noise_q=torch.stack(nq).numpy(), z=z.numpy(), **_logs(inter), **_tables(sampler),
                        sqrt_ac=shim.sqrt_alphas_cumprod.numpy()[steps], sqrt_1mac=shim.sqrt_one_minus_alphas_cumprod.numpy()[steps],
                        next_draw=nxt.numpy(), S=S, scale=scale, log_every_t=log_every_t, seed=seed)
    print(name, "z std", float(z.std()), "steps", len(steps), "logged", len(inter["x_inter"]))


def variant_case(name, unet, ldm, S, scale, ctx_len=None, seed=531):
    """The other two tools' call patterns (make_golden.ddim_variant_case) with PLMS: inpaint -- concat conditioning, no guidance;
    I2A -- crossattn with a 1-token context and guidance 3 (the embedding is not hoisted: add_context_to_emb)."""
    sampler, _ = _sampler(unet, ldm)
    concat = ldm["conditioning_key"] == "concat"
    Cz, H, W = ldm["latent_shape"]
    x_T = torch.from_numpy(np.random.RandomState(61).randn(1, Cz, H, W)).float()
    out = dict(x_T=x_T.numpy(), S=S, scale=scale)
    if concat:
        g = torch.Generator().manual_seed(80)
        masked = torch.randn(1, Cz, H, W, generator=g)
        mask = torch.zeros(1, 1, H, W)
        mask[:, :, :, W // 3: W // 2] = 1.0
        c = torch.cat([masked * (1 - mask), mask], dim=1)
        out["c"] = c.numpy()
        kw = dict(conditioning=c)
    else:
        c, uc = _cond(1, ctx_len, 1246), _cond(1, ctx_len, 1247)
        out["c"], out["uc"] = c.numpy(), uc.numpy()
        kw = dict(conditioning=c, unconditional_guidance_scale=scale, unconditional_conditioning=uc)
    z, _, _ = _run(sampler, seed, S=S, batch_size=1, shape=[Cz, H, W], x_T=x_T, **kw)
    out["z"] = z.numpy()
    out["ddim_timesteps"] = np.asarray(sampler.ddim_timesteps)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print(name, "z std", float(z.std()))


def host_hooks_case(name, unet, S=4, scale=1.5, seed=541, W=32):
    """score_corrector (an affine map of (e_t, x), so that the result pins the call order and arguments; it records the t of
    each call: step 0 calls it twice, the second time at t_next), callback(i) and img_callback(pred_x0, i)."""
    sampler, shim = _sampler(unet)
    calls = []

    class Corrector:
        def modify_score(self, model, e_t, x, t, c, gain, shift):
            assert model is shim and t.dtype == torch.long and c.shape[0] == x.shape[0]
            calls.append(int(t[0]))
            return gain * e_t + shift * x * (t.float() / 1000.0).reshape(-1, 1, 1, 1)

    B = 2
    x_T = torch.from_numpy(np.random.RandomState(62).randn(B, 4, 10, W)).float()
    c, uc = _cond(B, COND_TOKENS, 1248), _cond(B, COND_TOKENS, 1249)
    seen, preds = [], []
    z, inter, nxt = _run(sampler, seed, S=S, conditioning=c, batch_size=B, shape=[4, 10, W], unconditional_guidance_scale=scale,
                         unconditional_conditioning=uc, x_T=x_T, log_every_t=3, score_corrector=Corrector(),
                         corrector_kwargs=dict(gain=0.9, shift=0.05), callback=seen.append,
                         img_callback=lambda p, i: preds.append((i, p.clone())))
    n = len(sampler.ddim_timesteps)
    assert seen == list(range(n)) and [i for i, _ in preds] == seen and len(calls) == n + 1
    _, nxt2 = _draws(x_T.shape, n, False, seed)
    assert torch.equal(nxt, nxt2)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), x_T=x_T.numpy(), c=c.numpy(), uc=uc.numpy(), z=z.numpy(),
                        pred_x0_steps=np.stack([p.numpy() for _, p in preds]), x_log=_logs(inter)["x_log"],
                        callback_i=np.asarray(seen), corrector_t=np.asarray(calls), next_draw=nxt.numpy(),
                        ddim_timesteps=np.asarray(sampler.ddim_timesteps), S=S, scale=scale, gain=0.9, shift=0.05, log_every_t=3,
                        seed=seed)
    print(name, "z std", float(z.std()), "corrector t", calls)


def main():
    torch.set_num_threads(8)
    MG._install_shims()
    unet = MG.unet_case("unet_t2a", C.UNET_T2A, 10, 78, 77, {}, save=False)
    t2a_case("plms_t2a_s10", unet)
    orders_case("plms_t2a_orders", unet)
    mask_case("plms_t2a_mask_s6", unet)
    host_hooks_case("plms_t2a_host_hooks_s4", unet)
    u_i2a = MG.unet_case("unet_i2a", C.UNET_I2A, 10, 78, 1, {}, seed=4, save=False)
    variant_case("plms_i2a_s4", u_i2a, C.LDM_I2A, 4, 3.0, ctx_len=1)
    u_inp = MG.unet_case("unet_inpaint", C.UNET_INPAINT, 10, 106, 0, {}, n=1, seed=5, save=False)
    variant_case("plms_inpaint_s4", u_inp, C.LDM_INPAINT, 4, 1.0)
    print("torch", torch.__version__)


if __name__ == "__main__":
    main()
