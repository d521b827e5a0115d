"""The model's own ancestral (DDPM) sampler on the MI355X: UNet.ddpm_sample (maa_ddpm_sample), UNet.ddpm_update
(maa_ddpm_update), LatentDiffusionAudio's p_sample / p_sample_loop and MakeAnAudio.generate(sampler="ddpm") against the goldens
made by the reference's own LatentDiffusion_audio methods (tests/golden/make_golden_ddpm.py), and the bit-identical invariants
of the device loop.

Tolerances as the rest of the suite: latents and logs rel-max 1e-3 (test_gpu_plms.py, the DDIM tests); the host-hook path 1e-3
(f32) / 2e-3 (bf16x3), as test_gpu_plms' host-hook test."""
import os

import numpy as np
import pytest
import torch

from audiogpt_amd import config as C
from audiogpt_amd import weights as WT
from audiogpt_amd.ldm.ddpm import schedule_buffers
from tests import split_ref as R
from tests.util import check

pytestmark = pytest.mark.gpu

SHORT8 = dict(C.LDM_T2A, timesteps=8, linear_start=0.00085 * 50, linear_end=0.0120 * 50)


def _tabs(ldm):
    return schedule_buffers(ldm["timesteps"], ldm["linear_start"], ldm["linear_end"])


def _unet(precision, cfg=C.UNET_T2A, seed=0):
    from audiogpt_amd.backend import Context, UNet
    ctx = Context("cuda:0", precision=precision)
    return ctx, UNet(ctx, cfg, WT.make_unet_state_dict(cfg, seed=seed))


@pytest.fixture(scope="module", params=["f32", "bf16x3"])
def model(request):
    ctx, unet = _unet(request.param)
    yield ctx, unet
    unet.close()
    ctx.close()


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _check_logs(tag, got, ref):
    assert tuple(got.shape) == tuple(ref.shape), (tag, got.shape, ref.shape)
    for i in range(ref.shape[0]):
        check(f"{tag}{i}", got[i], ref[i], 1e-3)


def test_short8_matches_reference_with_and_without_the_clamp(golden, model):
    """All 8 rows of the tables, t == 0's missing noise, the clamp (the reference's own x_recon is clamped at 42-84 % of its
    elements at the logged steps: clamp_share) and both logs."""
    ctx, unet = model
    g = golden("ddpm_t2a_short8")
    assert (float(g["linear_start"]), float(g["linear_end"])) == (SHORT8["linear_start"], SHORT8["linear_end"])
    assert any(0.01 <= s <= 0.99 for s in g["clamp_share"])
    tabs = _tabs(SHORT8)
    for clip, sfx in ((True, ""), (False, "_noclip")):
        z, x_log, x0_log = unet.ddpm_sample(_t(g["x_T"]), tabs, 8, cond=_t(g["c"]), noise_p=_t(g["noise_p"]), clip_denoised=clip,
                                            log_every_t=int(g["log_every_t"]))
        tag = f"ddpm_t2a_short8{sfx}_{ctx.precision}"
        check(tag + "_vs_reference", z, g["z" + sfx], 1e-3)
        _check_logs(tag + "_x_log", x_log, g["x_log" + sfx])
        if clip:
            _check_logs(tag + "_x0_log", x0_log, g["x0_log"])
            assert float(x0_log.abs().max()) == 1.0


def test_tail4_and_start_T_match_reference(golden, model):
    ctx, unet = model
    g = golden("ddpm_t2a_tail4")
    tabs = _tabs(C.LDM_T2A)
    for n, sfx in ((4, "_t4"), (3, "_start3")):
        z, x_log, _ = unet.ddpm_sample(_t(g["x_T"]), tabs, n, cond=_t(g["c"]), noise_p=_t(g["noise_p"][:n]), log_every_t=200)
        tag = f"ddpm_t2a_tail4{sfx}_{ctx.precision}"
        check(tag + "_vs_reference", z, g["z" + sfx], 1e-3)
        _check_logs(tag + "_x_log", x_log, g["x_log" + sfx])


def test_mask8_matches_reference_on_both_loops(golden, model):
    """The blend AFTER the step with the step's own t (also at t = 0), and progressive_denoising's per-timestep temperature."""
    ctx, unet = model
    g = golden("ddpm_t2a_mask8")
    tabs = _tabs(SHORT8)
    kw = dict(cond=_t(g["c"]), mask=_t(g["mask"]), x0=_t(g["x0"]), noise_p=_t(g["noise_p"]), noise_q=_t(g["noise_q"]),
              log_every_t=int(g["log_every_t"]))
    z, x_log, _ = unet.ddpm_sample(_t(g["x_T"]), tabs, 8, **kw)
    tag = f"ddpm_t2a_mask8_{ctx.precision}"
    check(tag + "_vs_reference", z, g["z"], 1e-3)
    _check_logs(tag + "_x_log", x_log, g["x_log"])
    zp, _, x0_log = unet.ddpm_sample(_t(g["x_T"]), tabs, 8, temperature=g["temperature"].tolist(), **kw)
    check(tag + "_progressive_vs_reference", zp, g["z_prog"], 1e-3)
    _check_logs(tag + "_progressive_x0_log", x0_log, g["x0_log_prog"])


def test_guided_short8_matches_the_reference_loop_over_a_guided_model(golden, model):
    ctx, unet = model
    g = golden("ddpm_guided_short8")
    z, x_log, _ = unet.ddpm_sample(_t(g["x_T"]), _tabs(SHORT8), 8, cond=_t(g["c"]), uncond=_t(g["uc"]), scale=float(g["scale"]),
                                   noise_p=_t(g["noise_p"]), log_every_t=int(g["log_every_t"]))
    tag = f"ddpm_guided_short8_{ctx.precision}"
    check(tag + "_vs_reference", z, g["z"], 1e-3)
    _check_logs(tag + "_x_log", x_log, g["x_log"])


def test_split_tail3_matches_reference(golden, model):
    ctx, unet = model
    g = golden("ddpm_split_tail3")
    n = int(g["n"])
    z = unet.ddpm_sample(_t(g["x_T"]), _tabs(C.LDM_T2A), n, cond=_t(g["c"]), noise_p=_t(g["noise_p"]), split=R.params("A"))
    check(f"ddpm_split_tail3_{ctx.precision}_vs_reference", z, g["z"], 1e-3)
    assert float(np.abs(g["z_whole"] - g["z"]).max()) > 1e-2          # (the control: without the crops the result differs)


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("name,cfg,ldm,seed", [("ddpm_i2a_tail3", C.UNET_I2A, C.LDM_I2A, 4),
                                               ("ddpm_inpaint_tail3", C.UNET_INPAINT, C.LDM_INPAINT, 5)])
def test_variants_match_reference(golden, precision, name, cfg, ldm, seed):
    """I2A: the embedding is not hoisted (add_context_to_emb); inpaint: concat conditioning."""
    ctx, unet = _unet(precision, cfg, seed)
    try:
        g = golden(name)
        kw = dict(concat=_t(g["c"])) if ldm["conditioning_key"] == "concat" else dict(cond=_t(g["c"]))
        z, x_log, _ = unet.ddpm_sample(_t(g["x_T"]), _tabs(ldm), int(g["n"]), noise_p=_t(g["noise_p"]),
                                       log_every_t=int(g["log_every_t"]), **kw)
        check(f"{name}_{precision}_vs_reference", z, g["z"], 1e-3)
        _check_logs(f"{name}_{precision}_x_log", x_log, g["x_log"])
    finally:
        unet.close()
        ctx.close()


@pytest.fixture(scope="module", params=["f32", "bf16x3"])
def ldm_model(request):
    from audiogpt_amd.ldm.latent_diffusion import LatentDiffusionAudio
    return LatentDiffusionAudio(C.LDM_T2A, device="cuda:0", precision=request.param)


def test_p_sample_matches_reference_at_four_timesteps(golden, ldm_model):
    """p_sample on a batch whose samples sit at t = [999, 500, 1, 0].  It draws its own noise from the device generator; the
    reference's result is moved to that draw: x_prev_ref + sd[t] (noise_here - noise_ref), sd = exp(0.5 logvar[t]), 0 at t = 0."""
    m = ldm_model
    g = golden("ddpm_p_sample_t")
    x, c, t = _t(g["x"]).cuda(), _t(g["c"]).cuda(), _t(g["t"]).cuda()
    torch.cuda.manual_seed(77)
    x_prev, x_recon = m.p_sample(x, c, t, clip_denoised=True, return_x0=True)
    torch.cuda.manual_seed(77)
    noise = torch.randn(x.shape, device="cuda").cpu().double()
    lv = m.posterior_log_variance_clipped.cpu().double()[g["t"]]
    sd = (torch.exp(0.5 * lv) * _t(g["t"] != 0).double()).reshape(-1, 1, 1, 1)
    want = _t(g["x_prev"]).double() + sd * (noise - _t(g["noise"]).double())
    check(f"ddpm_p_sample_t_{m.precision}_x_prev", x_prev, want, 1e-3)
    check(f"ddpm_p_sample_t_{m.precision}_x_recon", x_recon, g["x_recon"], 1e-3)
    # the same step with the reference's own draw, through the entry p_sample calls
    e = m.apply_model(x, t, c)
    x_prev2, x_recon2 = m.unet.ddpm_update(x, e, t, m, _t(g["noise"]))
    check(f"ddpm_update_t_{m.precision}_x_prev", x_prev2, g["x_prev"], 1e-3)
    assert torch.equal(x_recon2, x_recon)
    assert torch.equal(x_prev2[3], m.p_mean_variance(x, c, t, True)[0][3])          # t = 0: the mean alone


def test_host_hook_loop_matches_reference(golden, ldm_model):
    m = ldm_model
    g = golden("ddpm_t2a_tail4")
    seen = []
    z, inter = m.p_sample_loop(_t(g["c"]).cuda(), tuple(g["x_T"].shape), return_intermediates=True, x_T=_t(g["x_T"]).cuda(),
                               verbose=False, timesteps=4, img_callback=lambda img, i: seen.append((i, img.clone())),
                               _step_noise=(_t(g["noise_p"]).cuda(), None))
    tol = 2e-3 if m.precision == "bf16x3" else 1e-3
    assert [i for i, _ in seen] == [3, 2, 1, 0] and len(inter) == 1 + g["x_log_t4"].shape[0]
    check(f"ddpm_{m.precision}_host_hooks_z", z, g["z_t4"], tol)
    for i in range(g["x_log_t4"].shape[0]):
        check(f"ddpm_{m.precision}_host_hooks_x_log{i}", inter[i + 1], g["x_log_t4"][i], tol)
    assert torch.equal(seen[-1][1], z) and torch.equal(seen[0][1], inter[1])
    # the same call without the hook runs the device loop
    zd, interd = m.p_sample_loop(_t(g["c"]).cuda(), tuple(g["x_T"].shape), return_intermediates=True, x_T=_t(g["x_T"]).cuda(),
                                 verbose=False, timesteps=4, _step_noise=(_t(g["noise_p"]).cuda(), None))
    check(f"ddpm_{m.precision}_dropin_z", zd, g["z_t4"], 1e-3)
    assert len(interd) == len(inter) and torch.equal(interd[0].cpu(), _t(g["x_T"]))


def test_graph_eager_replay_lanes_shared_prefix_and_batch_are_bit_identical(golden, model):
    """On short8 with the mask, logs included: graph == eager == a second call on the kept graph; guided, one stream == two
    lanes == MAA_CFG_SHARED=0; a sample alone == the same sample in a batch of 2."""
    from audiogpt_amd.backend import reload_tuning
    ctx, unet = model
    g, gg = golden("ddpm_t2a_mask8"), golden("ddpm_guided_short8")
    tabs = _tabs(SHORT8)
    x, c, uc = _t(g["x_T"]), _t(g["c"]), _t(gg["uc"])
    kw = dict(mask=_t(g["mask"]), x0=_t(g["x0"]), noise_p=_t(g["noise_p"]).cuda(), noise_q=_t(g["noise_q"]).cuda(), log_every_t=2)
    plain = {mode: [t.cpu() for t in unet.ddpm_sample(x, tabs, 8, cond=c, use_graph=graph, **kw)]
             for mode, graph in (("eager", False), ("graph", True), ("again", True))}
    assert bool(torch.isfinite(plain["eager"][0]).all()) and float(plain["eager"][0].abs().max()) > 0
    for mode, v in plain.items():
        for i in range(3):
            assert torch.equal(v[i], plain["eager"][i]), (mode, i)
    guided = {}
    try:
        for shared in ("1", "0"):
            os.environ["MAA_CFG_SHARED"] = shared
            reload_tuning()
            for lanes in (False, True):
                ctx.set_cfg_split(lanes)
                for graph in (False, True, True):
                    r = unet.ddpm_sample(x, tabs, 8, cond=c, uncond=uc, scale=1.5, use_graph=graph, **kw)
                    guided[shared, lanes, graph, len(guided)] = [t.cpu() for t in r]
    finally:
        os.environ.pop("MAA_CFG_SHARED", None)
        reload_tuning()
        ctx.set_cfg_split(None)
    ref = guided["1", False, False, 0]
    assert not torch.equal(ref[0], plain["eager"][0])
    for k, v in guided.items():
        for i in range(3):
            assert torch.equal(v[i], ref[i]), (k, i)
    # sample 1 alone == sample 1 in the batch of 2 (unguided and guided)
    one = {k: (v[1:2] if k in ("mask", "x0") else v[:, 1:2].contiguous() if k.startswith("noise") else v) for k, v in kw.items()}
    z1 = unet.ddpm_sample(x[1:2], tabs, 8, cond=c[1:2], **one)
    for i in range(3):
        assert torch.equal(z1[i].cpu()[:, 0] if i else z1[i].cpu()[0], plain["eager"][i][:, 1] if i else plain["eager"][i][1]), i
    z1g = unet.ddpm_sample(x[1:2], tabs, 8, cond=c[1:2], uncond=uc[1:2], scale=1.5, **one)
    assert torch.equal(z1g[0].cpu()[0], ref[0][1])
    assert torch.equal(z1g[1].cpu()[:, 0], ref[1][:, 1]) and torch.equal(z1g[2].cpu()[:, 0], ref[2][:, 1])


def test_a_ddim_sample_between_two_ancestral_calls_changes_neither(golden):
    from oracle import ddim as O
    g = golden("ddpm_t2a_mask8")
    tabs = _tabs(SHORT8)
    ac = O.alphas_cumprod(1000, C.LDM_T2A["linear_start"], C.LDM_T2A["linear_end"])
    steps = O.ddim_timesteps(4, 1000)
    a, ap, _, _ = O.ddim_tables(ac, steps)
    x, c = _t(g["x_T"]), _t(g["c"])
    kw = dict(cond=c, mask=_t(g["mask"]), x0=_t(g["x0"]), noise_p=_t(g["noise_p"]).cuda(), noise_q=_t(g["noise_q"]).cuda(),
              log_every_t=2)
    ctx, unet = _unet("f32")
    ctx2, unet2 = _unet("f32")
    try:
        p1 = [t.cpu() for t in unet.ddpm_sample(x, tabs, 8, **kw)]
        d1 = unet.ddim_sample(x, steps, a.numpy(), ap.numpy(), cond=c).cpu()
        p2 = [t.cpu() for t in unet.ddpm_sample(x, tabs, 8, **kw)]
        d2 = unet.ddim_sample(x, steps, a.numpy(), ap.numpy(), cond=c).cpu()
        d_alone = unet2.ddim_sample(x, steps, a.numpy(), ap.numpy(), cond=c).cpu()
    finally:
        for o in (unet, ctx, unet2, ctx2):
            o.close()
    for i in range(3):
        assert torch.equal(p1[i], p2[i]), i
    assert torch.equal(d1, d2) and torch.equal(d1, d_alone) and not torch.equal(d1, p1[0])
    check("ddpm_around_ddim_vs_reference", p2[0], g["z"], 1e-3)


def test_long_chain_equals_its_two_halves():
    """The 1000-step schedule at a launch-bound size: t = 999 .. 0 in one call is bit-identical to t = 999 .. 500 followed by
    t = 499 .. 0 from its result with the matching slices of the same noise (the entry's (start, n) form), and finite."""
    ctx, unet = _unet("bf16x3")
    try:
        tabs = _tabs(C.LDM_T2A)
        g = torch.Generator().manual_seed(91)
        x = torch.randn(1, 4, 8, 16, generator=g)
        c = torch.nn.functional.layer_norm(torch.randn(1, 77, 1024, generator=g), (1024,))
        noise = torch.randn(1000, 1, 4, 8, 16, generator=g).cuda()
        full = unet.ddpm_sample(x, tabs, 1000, cond=c, noise_p=noise)
        half = unet.ddpm_sample(x, tabs, 500, cond=c, noise_p=noise[:500], start=999)
        both = unet.ddpm_sample(half, tabs, 500, cond=c, noise_p=noise[500:])
        assert bool(torch.isfinite(full).all()) and float(full.abs().max()) > 0
        assert not torch.equal(half, full) and torch.equal(both, full)
    finally:
        unet.close()
        ctx.close()


def test_generate_with_ddpm_is_sample_latents_then_vae_and_vocoder(golden):
    from audiogpt_amd import _lib as L
    from audiogpt_amd.pipeline import MakeAnAudio
    g = golden("ddpm_t2a_short8")
    m = MakeAnAudio("cuda:0", ldm=SHORT8, vocoder_cfg=C.HIFIGAN_16K, seeds=(0, 1, 2), precision="f32")
    try:
        x, c = _t(g["x_T"]), _t(g["c"])
        torch.cuda.manual_seed(5)
        wav, spec, z = m.generate(x, c, sampler="ddpm", S=3)          # (S is ignored: all 8 timesteps run)
        torch.cuda.manual_seed(5)
        z_ref = m.sample_latents(x, c, sampler="ddpm")
        torch.cuda.manual_seed(5)
        noise = torch.stack([torch.randn(tuple(x.shape), device="cuda") for _ in range(8)])
        z_loop = m.unet.ddpm_sample(x, _tabs(SHORT8), 8, cond=c, noise_p=noise)
        spec_ref = m.decode(z_ref)
        wav_ref = m.vocode(spec_ref)
        assert torch.equal(z.cpu(), z_ref.cpu()) and torch.equal(z.cpu(), z_loop.cpu())
        assert torch.equal(spec.cpu(), spec_ref.cpu()) and torch.equal(wav.cpu(), wav_ref.cpu())
        assert bool(torch.isfinite(wav).all())
        with pytest.raises(L.MaaError, match='"ddim", "plms" or "ddpm"'):
            m.generate(x, c, sampler="bogus")
    finally:
        m.close()
