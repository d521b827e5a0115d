"""Golden vectors of text-guided editing (SDEdit) from the REFERENCE's own DDIMSampler (run in the build container only).

    python tests/golden/make_golden_sdedit.py     # needs /root/reference; writes tests/golden/sdedit_*.npz

DDIMSampler.stochastic_encode and DDIMSampler.decode (text_to_audio/Make_An_Audio/ldm/models/diffusion/ddim.py:227-261) run on
CPU fp32 through a minimal model shim (the pattern of make_golden.py; LatentDiffusion itself needs pytorch_lightning), with the
seeded weights of `audiogpt_amd.weights`.  Every noise tensor the reference draws is drawn again from the same seed and stored,
so the GPU tests need neither the device RNG nor the reference.

    sdedit_encode         stochastic_encode at B = 3, three different t, DDIM tables and use_original_steps=True
    sdedit_decode_s10     decode, T2A UNet, latent [2, 4, 10, 78], S = 10, t_start = 6, guidance 1.5, eta 0
    sdedit_decode_eta_s6  decode, latent [2, 4, 10, 32], S = 6 (seven DDIM steps), t_start = 4, guidance 1.5, eta 0.5
    sdedit_chain          mel [2, 1, 80, 48] -> Encoder + quant_conv -> DiagonalGaussianDistribution.sample() -> stochastic_encode
                          -> decode (S = 10, strength 0.6) -> post_quant_conv + Decoder -> clamp((x + 1) / 2) -> HiFi-GAN 16 kHz

The shapes are kept small so that each file stays a few hundred KB: the conditioning has COND_TOKENS tokens (the cross-attention
takes any count; the tools' 77 would be 1.2 MB per case) and the chain's clip is 48 frames (latent width 6), which every stage
of the chain supports.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG                       # noqa: E402  (helpers and shims; not modified)
from make_golden import C, WT, _cond           # noqa: E402

COND_TOKENS = 4


def _shim(unet, ldm):
    """The DDIM model shim of make_golden.py: the schedule buffers DDIMSampler reads and apply_model (crossattn path)."""
    from ldm.modules.diffusionmodules.util import make_beta_schedule

    class Shim:
        def __init__(self):
            betas = make_beta_schedule("linear", ldm["timesteps"], ldm["linear_start"], ldm["linear_end"])
            ac = np.cumprod(1.0 - betas, axis=0)
            self.num_timesteps = ldm["timesteps"]
            self.betas = torch.tensor(betas, dtype=torch.float32)
            self.alphas_cumprod = torch.tensor(ac, dtype=torch.float32)
            self.alphas_cumprod_prev = torch.tensor(np.append(1.0, ac[:-1]), dtype=torch.float32)
            self.device = torch.device("cpu")

        def apply_model(self, x, t, c):          # DiffusionWrapper crossattn path (ddpm.py:1407-1409)
            return unet(x, t, context=c)

    return Shim()


def _sampler(unet, S, eta=0.0):
    from ldm.models.diffusion.ddim import DDIMSampler
    sampler = DDIMSampler(_shim(unet, C.LDM_T2A))
    sampler.device = torch.device("cpu")
    sampler.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=False)
    return sampler


def encode_case(name, S=10):
    sampler = _sampler(None, S)
    g = torch.Generator().manual_seed(401)
    x0 = torch.randn(3, 4, 10, 78, generator=g)
    noise = torch.randn(3, 4, 10, 78, generator=g)
    t = torch.tensor([0, 4, S - 1], dtype=torch.long)
    t_orig = torch.tensor([0, 517, 999], dtype=torch.long)
    with torch.no_grad():
        out = sampler.stochastic_encode(x0, t, use_original_steps=False, noise=noise)
        out_orig = sampler.stochastic_encode(x0, t_orig, use_original_steps=True, noise=noise)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), x0=x0.numpy(), noise=noise.numpy(), t=t.numpy(), t_orig=t_orig.numpy(),
                        out=out.numpy(), out_orig=out_orig.numpy(),
                        sqrt_a=torch.sqrt(sampler.ddim_alphas).numpy(),
                        sqrt_1ma=np.asarray(sampler.ddim_sqrt_one_minus_alphas, dtype=np.float32),
                        sqrt_ac=sampler.sqrt_alphas_cumprod.numpy(), sqrt_1mac=sampler.sqrt_one_minus_alphas_cumprod.numpy(), S=S)
    print(name, "out std", float(out.std()), "out_orig std", float(out_orig.std()))


def decode_case(name, unet, S, t_start, scale=1.5, eta=0.0, seed=411, B=2, W=78):
    sampler = _sampler(unet, S, eta)
    x = torch.from_numpy(np.random.RandomState(57).randn(B, 4, 10, W)).float()
    c, uc = _cond(B, COND_TOKENS, 1234), _cond(B, COND_TOKENS, 1235)
    torch.manual_seed(seed)
    with torch.no_grad():
        z = sampler.decode(x, c, t_start, unconditional_guidance_scale=scale, unconditional_conditioning=uc)
    extra = {}
    if eta != 0.0:          # (with eta 0 the draws are multiplied by sigma = 0: they do not enter the result)
        torch.manual_seed(seed)
        extra["noise_p"] = torch.stack([torch.randn(x.shape) for _ in range(t_start)]).numpy()   # noise_like, loop order
    np.savez_compressed(os.path.join(HERE, name + ".npz"), x_latent=x.numpy(), c=c.numpy(), uc=uc.numpy(), z=z.numpy(),
                        **extra, ddim_timesteps=np.asarray(sampler.ddim_timesteps),
                        ddim_sigmas=np.asarray(sampler.ddim_sigmas, dtype=np.float64), S=S, t_start=t_start, scale=scale, eta=eta,
                        temperature=1.0, seed=seed)
    print(name, "z std", float(z.std()), "steps", len(sampler.ddim_timesteps))


def chain_case(name, unet, S=10, strength=0.6, scale=1.5, seed=421, T=48):
    from argparse import Namespace
    from ldm.modules.diffusionmodules.model import Decoder, Encoder
    from ldm.modules.distributions.distributions import DiagonalGaussianDistribution
    from vocoder.hifigan.modules import Generator
    dd, ldm, vcfg = C.VAE_DDCONFIG, C.LDM_T2A, C.HIFIGAN_16K
    kw = dict(ch=dd["ch"], out_ch=dd["out_ch"], ch_mult=tuple(dd["ch_mult"]), num_res_blocks=dd["num_res_blocks"],
              attn_resolutions=list(dd["attn_resolutions"]), in_channels=dd["in_channels"],
              resolution=dd["resolution"], z_channels=dd["z_channels"], double_z=dd["double_z"])
    dec, enc = Decoder(**kw).eval(), Encoder(**kw).eval()
    sd = WT.make_vae_state_dict(dd, seed=1, with_encoder=True)
    dec.load_state_dict(WT.strip_prefix(sd, "decoder."), strict=True)
    enc.load_state_dict(WT.strip_prefix(sd, "encoder."), strict=True)
    pq = torch.nn.Conv2d(dd["embed_dim"], dd["z_channels"], 1)
    qc = torch.nn.Conv2d(2 * dd["z_channels"], 2 * dd["embed_dim"], 1)
    pq.load_state_dict(WT.strip_prefix(sd, "post_quant_conv."))
    qc.load_state_dict(WT.strip_prefix(sd, "quant_conv."))
    gen = Generator(Namespace(**{k: (list(map(list, v)) if k == "resblock_dilation_sizes" else
                                     (list(v) if isinstance(v, tuple) else v)) for k, v in vcfg.items()})).eval()
    gen.load_state_dict(WT.make_vocoder_state_dict(vcfg, seed=2), strict=True)
    sampler = _sampler(unet, S)
    sf = float(ldm["scale_factor"])
    B = 2
    g = torch.Generator().manual_seed(431)
    mel_in = torch.rand(B, 1, 80, T, generator=g) * 2 - 1
    n_q = torch.randn(B, 4, 10, T // 8, generator=g)
    c, uc = _cond(B, COND_TOKENS, 1236), _cond(B, COND_TOKENS, 1237)
    t_enc = int(strength * S)
    with torch.no_grad():
        posterior = DiagonalGaussianDistribution(qc(enc(mel_in)))           # AutoencoderKL.encode (autoencoder.py:345-349)
        torch.manual_seed(seed)
        z0 = sf * posterior.sample()                                          # get_first_stage_encoding
        torch.manual_seed(seed)
        n_post = torch.randn(posterior.mean.shape)
        z_enc = sampler.stochastic_encode(z0, torch.tensor([t_enc] * B), noise=n_q)
        z = sampler.decode(z_enc, c, t_enc, unconditional_guidance_scale=scale, unconditional_conditioning=uc)
        mel = dec(pq(z / sf))                                                 # decode_first_stage (autoencoder.py:351-354)
        spec = torch.clamp((mel + 1.0) / 2.0, 0.0, 1.0)[:, 0]
        wav = gen(spec)[:, 0]
    np.savez_compressed(os.path.join(HERE, name + ".npz"), mel_in=mel_in.numpy(), n_post=n_post.numpy(), n_q=n_q.numpy(),
                        c=c.numpy(), uc=uc.numpy(), z0=z0.numpy(), z_enc=z_enc.numpy(), z=z.numpy(), spec=spec.numpy(),
                        wav=wav.numpy(), S=S, strength=strength, t_enc=t_enc, scale=scale)
    print(name, "z std", float(z.std()), "wav std", float(wav.std()))


def main():
    torch.set_num_threads(8)
    MG._install_shims()
    unet = MG.unet_case("unet_t2a", C.UNET_T2A, 10, 78, 77, {}, save=False)
    encode_case("sdedit_encode")
    decode_case("sdedit_decode_s10", unet, S=10, t_start=6)
    decode_case("sdedit_decode_eta_s6", unet, S=6, t_start=4, eta=0.5, seed=412, W=32)
    chain_case("sdedit_chain", unet)
    print("torch", torch.__version__)


if __name__ == "__main__":
    main()
