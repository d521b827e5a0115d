"""Text-guided editing (SDEdit) on the MI355X: DDIMSampler.stochastic_encode / decode and MakeAnAudio.edit_here against the
reference-generated goldens (tests/golden/make_golden_sdedit.py), and the bit-identical invariants of the device path.

Tolerances as the rest of the suite: stochastic_encode rel-max 1e-6; DDIM latent rel-max 1e-3 (test_ddim_10_steps_matches_reference);
mel-L1 on the [0, 1] mel and waveform RMS <= 1e-4."""
import numpy as np
import pytest
import torch

from audiogpt_amd import config as C
from audiogpt_amd import weights as WT
from tests.util import check, record

pytestmark = pytest.mark.gpu


def _t2a(precision):
    from audiogpt_amd.backend import Context, UNet
    ctx = Context("cuda:0", precision=precision)
    return ctx, UNet(ctx, C.UNET_T2A, WT.make_unet_state_dict(C.UNET_T2A, seed=0))


@pytest.fixture(scope="module")
def f32():
    ctx, unet = _t2a("f32")
    yield ctx, unet
    unet.close()
    ctx.close()


@pytest.fixture(scope="module", params=["f32", "bf16x3"])
def model(request, f32):
    """The T2A UNet in both precision modes (the f32 one is the `f32` fixture's)."""
    if request.param == "f32":
        yield f32
        return
    ctx, unet = _t2a(request.param)
    yield ctx, unet
    unet.close()
    ctx.close()


def _tables(S):
    from oracle import ddim as O
    ldm = C.LDM_T2A
    ac = O.alphas_cumprod(ldm["timesteps"], ldm["linear_start"], ldm["linear_end"])
    steps = O.ddim_timesteps(S, ldm["timesteps"])
    a, ap, _, _ = O.ddim_tables(ac, steps)
    return steps, a.numpy(), ap.numpy()


def _t(a):
    return torch.from_numpy(np.asarray(a))


def test_stochastic_encode_matches_reference(golden, f32):
    from audiogpt_amd.backend import ddim_stochastic_encode
    ctx, _ = f32
    g = golden("sdedit_encode")
    out = ddim_stochastic_encode(ctx, _t(g["x0"]), _t(g["t"]), g["sqrt_a"], g["sqrt_1ma"], _t(g["noise"]))
    check("sdedit_encode_ddim_vs_reference", out, g["out"], 1e-6)
    out = ddim_stochastic_encode(ctx, _t(g["x0"]), _t(g["t_orig"]), g["sqrt_ac"], g["sqrt_1mac"], _t(g["noise"]))
    check("sdedit_encode_orig_vs_reference", out, g["out_orig"], 1e-6)
    # one sample alone == the same sample inside the batch
    one = ddim_stochastic_encode(ctx, _t(g["x0"][1:2]), _t(g["t"][1:2]), g["sqrt_a"], g["sqrt_1ma"], _t(g["noise"][1:2]))
    full = ddim_stochastic_encode(ctx, _t(g["x0"]), _t(g["t"]), g["sqrt_a"], g["sqrt_1ma"], _t(g["noise"]))
    assert torch.equal(one.cpu(), full[1:2].cpu())


def test_stochastic_encode_entry_checks_t_on_the_device(golden, f32):
    """The C entry's own check (the Python helper checks first): an index past the table fails the call, nothing is read."""
    import ctypes
    from audiogpt_amd import _lib as L
    ctx, _ = f32
    g = golden("sdedit_encode")
    x = _t(g["x0"]).cuda()
    n = torch.empty_like(x)
    t = torch.tensor([0, 3, 10], dtype=torch.int32, device="cuda")
    tab = np.ascontiguousarray(g["sqrt_a"], dtype=np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    st = ctx.lib.maa_ddim_stochastic_encode(ctx.h, L.dptr(x), 0, 1.0, None, ctypes.c_void_p(t.data_ptr()), tab.ctypes.data_as(fp),
                                            tab.ctypes.data_as(fp), tab.shape[0], L.dptr(x), 3, 4, 10, 78, L.dptr(n))
    assert st < 0 and b"outside" in ctx.lib.maa_last_error()
    ctx.synchronize()


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("name", ["sdedit_decode_s10", "sdedit_decode_eta_s6"])
def test_decode_matches_reference(golden, model, name, use_graph):
    ctx, unet = model
    g = golden(name)
    S = int(g["S"])
    steps, a, ap = _tables(S)
    assert steps.tolist() == g["ddim_timesteps"].tolist()
    kw = {}
    if float(g["eta"]) != 0.0:
        kw = dict(sigmas=g["ddim_sigmas"].astype(np.float32), noise_p=_t(g["noise_p"]), temperature=float(g["temperature"]))
    z = unet.ddim_decode(_t(g["x_latent"]), int(g["t_start"]), steps, a, ap, cond=_t(g["c"]), uncond=_t(g["uc"]),
                         scale=float(g["scale"]), use_graph=use_graph, **kw)
    check(f"{name}_{ctx.precision}_graph{int(use_graph)}_vs_reference", z, g["z"], 1e-3)


def test_decode_graph_equals_eager_and_batch_invariant(golden, model):
    ctx, unet = model
    g = golden("sdedit_decode_eta_s6")
    S, k = int(g["S"]), int(g["t_start"])
    steps, a, ap = _tables(S)
    x, c, uc, z = _t(g["x_latent"]), _t(g["c"]), _t(g["uc"]), _t(g["noise_p"])
    kw = dict(sigmas=g["ddim_sigmas"].astype(np.float32), temperature=1.0)
    zg = unet.ddim_decode(x, k, steps, a, ap, cond=c, uncond=uc, scale=1.5, noise_p=z, use_graph=True, **kw).cpu()
    ze = unet.ddim_decode(x, k, steps, a, ap, cond=c, uncond=uc, scale=1.5, noise_p=z, use_graph=False, **kw).cpu()
    assert torch.equal(zg, ze), "decode: graph and eager differ"
    # sample 1 alone == sample 1 inside a batch of three
    xb, cb, ucb = torch.cat([x[1:2], x, x[1:2]]), torch.cat([c[1:2], c, c[1:2]]), torch.cat([uc[1:2], uc, uc[1:2]])
    zb_noise = torch.cat([z[:, 1:2], z, z[:, 1:2]], dim=1)
    zb = unet.ddim_decode(xb, k, steps, a, ap, cond=cb, uncond=ucb, scale=1.5, noise_p=zb_noise, **kw).cpu()
    z1 = unet.ddim_decode(x[1:2], k, steps, a, ap, cond=c[1:2], uncond=uc[1:2], scale=1.5, noise_p=z[:, 1:2], **kw).cpu()
    assert torch.equal(zb[0:1], z1) and torch.equal(zb[2:3], z1) and torch.equal(zb[1:3], zg)


@pytest.mark.parametrize("cfg", [True, False])
def test_decode_from_the_top_is_sample(golden, f32, cfg):
    ctx, unet = f32
    g = golden("ddim_t2a_s10")
    S = int(g["S"])
    steps, a, ap = _tables(S)
    kw = dict(cond=_t(g["c"]), uncond=_t(g["uc"]) if cfg else None, scale=float(g["scale"]) if cfg else 1.0)
    zs = unet.ddim_sample(_t(g["x_T"]), steps, a, ap, **kw).cpu()
    zd = unet.ddim_decode(_t(g["x_T"]), S, steps, a, ap, **kw).cpu()
    assert torch.equal(zs, zd), "decode(x_T, t_start=S) differs from sample(x_T)"
    if cfg:
        check("sdedit_decode_from_top_vs_reference", zd, g["z"], 1e-3)
    z0 = unet.ddim_decode(_t(g["x_T"]), 0, steps, a, ap, **kw).cpu()
    assert torch.equal(z0, _t(g["x_T"]).float())


def test_decode_is_the_tail_of_a_logged_sample(golden, f32):
    ctx, unet = f32
    g = golden("ddim_t2a_s10")
    S = int(g["S"])
    steps, a, ap = _tables(S)
    kw = dict(cond=_t(g["c"]), uncond=_t(g["uc"]), scale=float(g["scale"]))
    z, x_log, _ = unet.ddim_sample(_t(g["x_T"]), steps, a, ap, log_every_t=1, **kw)
    x_inter = [_t(g["x_T"]).float()] + [t.cpu() for t in x_log]
    for k in (1, 4, 7):
        zd = unet.ddim_decode(x_inter[S - k], k, steps, a, ap, **kw)
        assert torch.equal(zd.cpu(), z.cpu()), f"decode(x_inter[S - {k}], t_start={k}) differs from the sample's end"


def test_decode_after_sample_equals_decode_in_a_fresh_context(golden, f32):
    from audiogpt_amd.backend import Context, UNet
    ctx, unet = f32
    g = golden("sdedit_decode_s10")
    S, k = int(g["S"]), int(g["t_start"])
    steps, a, ap = _tables(S)
    kw = dict(cond=_t(g["c"]), uncond=_t(g["uc"]), scale=float(g["scale"]))
    unet.ddim_sample(_t(g["x_latent"]), steps, a, ap, **kw)            # leaves its step graph on the context
    z_after = unet.ddim_decode(_t(g["x_latent"]), k, steps, a, ap, **kw).cpu()
    ctx2 = Context("cuda:0", precision="f32")
    u2 = UNet(ctx2, C.UNET_T2A, WT.make_unet_state_dict(C.UNET_T2A, seed=0))
    z_fresh = u2.ddim_decode(_t(g["x_latent"]), k, steps, a, ap, **kw).cpu()
    u2.close()
    ctx2.close()
    assert torch.equal(z_after, z_fresh)


def test_decode_checks_its_arguments(golden, f32):
    from audiogpt_amd import _lib as L
    ctx, unet = f32
    g = golden("sdedit_decode_s10")
    steps, a, ap = _tables(10)
    with pytest.raises(L.MaaError, match="t_start"):
        unet.ddim_decode(_t(g["x_latent"]), 11, steps, a, ap, cond=_t(g["c"]))
    with pytest.raises(L.MaaError, match="noise_p"):
        unet.ddim_decode(_t(g["x_latent"]), 3, steps, a, ap, cond=_t(g["c"]), sigmas=np.ones(10, np.float32),
                         noise_p=torch.zeros(10, 2, 4, 10, 78))


@pytest.fixture(scope="module")
def edit_model():
    from audiogpt_amd.pipeline import MakeAnAudio
    m = MakeAnAudio("cuda:0", ldm=C.LDM_T2A, vocoder_cfg=C.HIFIGAN_16K, seeds=(0, 1, 2), with_encoder=True, precision="f32")
    yield m
    m.close()


def test_edit_here_matches_reference(golden, edit_model):
    g = golden("sdedit_chain")
    wav, spec, z = edit_model.edit_here(_t(g["mel_in"]), _t(g["c"]), _t(g["uc"]), scale=float(g["scale"]), S=int(g["S"]),
                                        strength=float(g["strength"]), noise=(_t(g["n_post"]), _t(g["n_q"])))
    check("sdedit_chain_z_vs_reference", z, g["z"], 1e-3)
    l1 = float((spec.cpu() - _t(g["spec"])).abs().mean())
    rms = float(((wav.cpu() - _t(g["wav"])) ** 2).mean().sqrt())
    record("sdedit_chain_vs_reference", mel_l1=l1, wav_rms=rms, tol=1e-4)
    assert l1 <= 1e-4 and rms <= 1e-4, (l1, rms)
    # edit() on the library's own stream gives the same
    wav2, spec2, z2 = edit_model.edit(_t(g["mel_in"]), _t(g["c"]), _t(g["uc"]), scale=float(g["scale"]), S=int(g["S"]),
                                      strength=float(g["strength"]), noise=(_t(g["n_post"]), _t(g["n_q"])))
    assert torch.equal(wav2.cpu(), wav.cpu()) and torch.equal(z2.cpu(), z.cpu())


def test_edit_checks_strength_and_encoder(golden, edit_model):
    from audiogpt_amd import _lib as L
    from audiogpt_amd.pipeline import MakeAnAudio
    g = golden("sdedit_chain")
    for s in (1.0, -0.1):
        with pytest.raises(L.MaaError, match="strength"):
            edit_model.edit_here(_t(g["mel_in"]), _t(g["c"]), S=10, strength=s)
    # strength 0: noised at index 0, no step runs
    _, _, z = edit_model.edit_here(_t(g["mel_in"]), _t(g["c"]), S=10, strength=0.0, noise=(_t(g["n_post"]), _t(g["n_q"])))
    assert torch.isfinite(z).all()
    m = MakeAnAudio("cuda:0", ldm=C.LDM_T2A, vocoder_cfg=C.HIFIGAN_16K, with_encoder=False, precision="f32")
    with pytest.raises(L.MaaError, match="encoder"):
        m.edit_here(_t(g["mel_in"]), _t(g["c"]), S=10, strength=0.5)
    m.close()


@pytest.fixture(scope="module")
def dropin():
    from audiogpt_amd.ldm.ddim import DDIMSampler
    from audiogpt_amd.ldm.latent_diffusion import LatentDiffusionAudio
    m = LatentDiffusionAudio(C.LDM_T2A, precision="f32")
    return m, DDIMSampler(m)


def test_fused_moments_prologue_equals_the_drop_in_chain(golden, edit_model, dropin):
    """encode_moments + the fused kernel == encode_first_stage -> get_first_stage_encoding (posterior noise given) ->
    DDIMSampler.stochastic_encode, bit for bit."""
    from audiogpt_amd.backend import ddim_stochastic_encode
    from audiogpt_amd.ldm.latent_diffusion import DiagonalGaussianDistribution
    model, sampler = dropin
    g = golden("sdedit_chain")
    sampler.make_schedule(int(g["S"]), verbose=False)
    t_enc = int(g["t_enc"])
    n_post, n_q = _t(g["n_post"]).cuda(), _t(g["n_q"]).cuda()
    moments = model.vae.encode_moments(_t(g["mel_in"]))
    post = model.encode_first_stage(_t(g["mel_in"]))
    assert isinstance(post, DiagonalGaussianDistribution)
    z0 = model.scale_factor * (post.mean + post.std * n_post)           # posterior.sample() with the given draw
    unfused = sampler.stochastic_encode(z0, torch.tensor([t_enc] * 2, device="cuda"), noise=n_q)
    fused = ddim_stochastic_encode(model.ctx, moments, t_enc, torch.sqrt(sampler.ddim_alphas), sampler.ddim_sqrt_one_minus_alphas,
                                   n_q, moments=True, scale_factor=model.scale_factor, noise_post=n_post)
    record("sdedit_fused_vs_unfused", max_abs=float((fused - unfused).abs().max()))
    assert torch.equal(fused.cpu(), unfused.cpu())
    check("sdedit_chain_z_enc_vs_reference", fused, g["z_enc"], 1e-4)


def test_drop_in_draws_as_the_reference(golden, dropin):
    """Seeded device generator: stochastic_encode(noise=None) + decode(t_start) leave it where 1 + t_start draws of the
    latent's shape leave it (the reference: randn_like in stochastic_encode, noise_like in every p_sample_ddim)."""
    model, sampler = dropin
    g = golden("sdedit_decode_s10")
    S, k = int(g["S"]), int(g["t_start"])
    sampler.make_schedule(S, verbose=False)
    x = _t(g["x_latent"]).cuda()
    torch.cuda.manual_seed(2024)
    z_enc = sampler.stochastic_encode(x, torch.tensor([k, k], device="cuda"))
    z = sampler.decode(z_enc, _t(g["c"]).cuda(), k, unconditional_guidance_scale=1.5, unconditional_conditioning=_t(g["uc"]).cuda())
    after = torch.cuda.get_rng_state()
    torch.cuda.manual_seed(2024)
    first = torch.randn(x.shape, device="cuda")
    for _ in range(k):
        torch.randn(x.shape, device="cuda")
    assert torch.equal(torch.cuda.get_rng_state(), after)
    assert torch.isfinite(z).all()
    # the draw the sampler used is the first of them
    ref = torch.sqrt(sampler.ddim_alphas)[k] * x.cpu() + sampler.ddim_sqrt_one_minus_alphas[k] * first.cpu()
    assert torch.equal(z_enc.cpu(), ref)
    # and decode itself matches the reference golden (eta 0: the draws do not enter)
    zd = sampler.decode(x, _t(g["c"]).cuda(), k, unconditional_guidance_scale=float(g["scale"]),
                        unconditional_conditioning=_t(g["uc"]).cuda())
    check("sdedit_dropin_decode_vs_reference", zd, g["z"], 1e-3)
