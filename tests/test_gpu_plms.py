"""PLMS sampling on the MI355X: UNet.plms_sample (maa_ldm_plms_sample), PLMSSampler and MakeAnAudio.generate(sampler="plms")
against the goldens made by the reference's own PLMSSampler (tests/golden/make_golden_plms.py), and the bit-identical
invariants of the device loop.

Tolerances as the rest of the suite: DDIM / PLMS latent rel-max 1e-3; the host-hook path 1e-3 (f32) / 2e-3 (bf16x3), as
test_gpu_tools' DDIM host-hook test."""
import numpy as np
import pytest
import torch

from audiogpt_amd import config as C
from audiogpt_amd import weights as WT
from tests.util import check

pytestmark = pytest.mark.gpu


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


def _tables(S, ldm=C.LDM_T2A):
    from oracle import ddim as O
    ac = O.alphas_cumprod(ldm["timesteps"], ldm["linear_start"], ldm["linear_end"])
    steps = O.ddim_timesteps(S, ldm["timesteps"])
    a, ap, _, _ = O.ddim_tables(ac, steps)
    return steps, a.numpy(), ap.numpy()


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _check_logs(tag, x_log, x0_log, g, sfx=""):
    assert x_log.shape == g["x_log" + sfx].shape and x0_log.shape == g["x0_log" + sfx].shape
    for i in range(x_log.shape[0]):
        check(f"{tag}_x_log{i}", x_log[i], g["x_log" + sfx][i], 1e-3)
        check(f"{tag}_x0_log{i}", x0_log[i], g["x0_log" + sfx][i], 1e-3)


def test_plms_s10_matches_reference(golden, model):
    ctx, unet = model
    g = golden("plms_t2a_s10")
    steps, a, ap = _tables(int(g["S"]))
    assert steps.tolist() == g["ddim_timesteps"].tolist()
    z, x_log, x0_log = unet.plms_sample(_t(g["x_T"]), steps, a, ap, cond=_t(g["c"]), uncond=_t(g["uc"]), scale=float(g["scale"]),
                                        log_every_t=int(g["log_every_t"]))
    tag = f"plms_t2a_s10_{ctx.precision}"
    check(tag + "_vs_reference", z, g["z"], 1e-3)
    _check_logs(tag, x_log, x0_log, g)


def test_plms_orders_match_reference(golden, model):
    """S = 1 (the Euler pair alone, t_next == t) and S = 5 (Euler, AB2, AB3, AB4, AB4): every step's x_prev and pred_x0."""
    ctx, unet = model
    g = golden("plms_t2a_orders")
    for S in (1, 5):
        steps, a, ap = _tables(S)
        assert steps.tolist() == g[f"ddim_timesteps_s{S}"].tolist()
        z, x_log, x0_log = unet.plms_sample(_t(g["x_T"]), steps, a, ap, cond=_t(g["c"]), uncond=_t(g["uc"]),
                                            scale=float(g["scale"]), log_every_t=1)
        tag = f"plms_t2a_orders_s{S}_{ctx.precision}"
        check(tag + "_vs_reference", z, g[f"z_s{S}"], 1e-3)
        _check_logs(tag, x_log, x0_log, g, f"_s{S}")


def test_plms_mask_matches_reference(golden, model):
    ctx, unet = model
    g = golden("plms_t2a_mask_s6")
    steps, a, ap = _tables(int(g["S"]))
    assert steps.tolist() == g["ddim_timesteps"].tolist() and len(steps) == 7
    z, x_log, x0_log = unet.plms_sample(_t(g["x_T"]), steps, a, ap, cond=_t(g["c"]), uncond=_t(g["uc"]), scale=float(g["scale"]),
                                        mask=_t(g["mask"]), x0=_t(g["x0"]), noise_q=_t(g["noise_q"]), sqrt_ac=g["sqrt_ac"],
                                        sqrt_1mac=g["sqrt_1mac"], log_every_t=int(g["log_every_t"]))
    tag = f"plms_t2a_mask_s6_{ctx.precision}"
    check(tag + "_vs_reference", z, g["z"], 1e-3)
    _check_logs(tag, x_log, x0_log, g)


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("name,cfg,ldm,seed", [("plms_i2a_s4", C.UNET_I2A, C.LDM_I2A, 4),
                                               ("plms_inpaint_s4", C.UNET_INPAINT, C.LDM_INPAINT, 5)])
def test_plms_variants_match_reference(golden, precision, name, cfg, ldm, seed):
    """I2A: the embedding is not hoisted (add_context_to_emb), so the second evaluation of step 0 forms it from t_next itself;
    inpaint: concat conditioning, whose channels the Euler mid-point kernel leaves in place."""
    ctx, unet = _unet(precision, cfg, seed)
    try:
        g = golden(name)
        steps, a, ap = _tables(int(g["S"]), ldm)
        assert steps.tolist() == g["ddim_timesteps"].tolist()
        if ldm["conditioning_key"] == "concat":
            kw = dict(concat=_t(g["c"]))
        else:
            kw = dict(cond=_t(g["c"]), uncond=_t(g["uc"]), scale=float(g["scale"]))
        z = unet.plms_sample(_t(g["x_T"]), steps, a, ap, **kw)
        check(f"{name}_{precision}_vs_reference", z, g["z"], 1e-3)
    finally:
        unet.close()
        ctx.close()


def test_plms_graph_eager_replay_lanes_and_batch_are_bit_identical(golden, model):
    """Graph, eager and a second call on the kept graph; the CFG halves as one stream and as two lanes; a prompt alone and the
    same prompt inside a batch: all bit-identical, logs included."""
    ctx, unet = model
    g = golden("plms_t2a_mask_s6")
    steps, a, ap = _tables(int(g["S"]))
    x, c, uc = _t(g["x_T"]), _t(g["c"]), _t(g["uc"])
    m, x0, nq = _t(g["mask"]), _t(g["x0"]), _t(g["noise_q"])
    kw = dict(scale=float(g["scale"]), sqrt_ac=g["sqrt_ac"], sqrt_1mac=g["sqrt_1mac"], log_every_t=int(g["log_every_t"]))
    out = {}
    try:
        for lanes in (True, False):
            ctx.set_cfg_split(lanes)
            for mode, graph in (("eager", False), ("graph", True), ("again", True)):
                r = unet.plms_sample(x, steps, a, ap, cond=c, uncond=uc, mask=m, x0=x0, noise_q=nq, use_graph=graph, **kw)
                out[lanes, mode] = [t.cpu() for t in r]
    finally:
        ctx.set_cfg_split(None)
    ref = out[False, "eager"]
    assert bool(torch.isfinite(ref[0]).all()) and float(ref[0].abs().max()) > 0
    for k, v in out.items():
        for i in range(3):
            assert torch.equal(v[i], ref[i]), (k, i)
    # sample 1 alone == sample 1 inside a batch of three
    cat = lambda t: torch.cat([t[1:2], t, t[1:2]])
    zb = unet.plms_sample(cat(x), steps, a, ap, cond=cat(c), uncond=cat(uc), mask=cat(m), x0=cat(x0),
                          noise_q=torch.cat([nq[:, 1:2], nq, nq[:, 1:2]], dim=1), **kw)[0].cpu()
    z1 = unet.plms_sample(x[1:2], steps, a, ap, cond=c[1:2], uncond=uc[1:2], mask=m[1:2], x0=x0[1:2], noise_q=nq[:, 1:2], **kw)[0].cpu()
    assert torch.equal(zb[0:1], z1) and torch.equal(zb[2:3], z1) and torch.equal(zb[1:3], ref[0])


def test_ddim_then_plms_then_ddim_on_one_context(golden):
    """The two loops keep their step graphs apart: DDIM, PLMS, DDIM on one context gives the DDIM result twice and the PLMS
    result of a fresh context."""
    g = golden("plms_t2a_s10")
    S = int(g["S"])
    steps, a, ap = _tables(S)
    kw = dict(cond=_t(g["c"]), uncond=_t(g["uc"]), scale=float(g["scale"]))
    x = _t(g["x_T"])
    ctx, unet = _unet("f32")
    ctx2, unet2 = _unet("f32")
    try:
        d1 = unet.ddim_sample(x, steps, a, ap, **kw).cpu()
        p = unet.plms_sample(x, steps, a, ap, **kw).cpu()
        d2 = unet.ddim_sample(x, steps, a, ap, **kw).cpu()
        p2 = unet.plms_sample(x, steps, a, ap, **kw).cpu()
        p_alone = unet2.plms_sample(x, steps, a, ap, **kw).cpu()
    finally:
        for o in (unet, ctx, unet2, ctx2):
            o.close()
    assert torch.equal(d1, d2)
    assert torch.equal(p, p_alone) and torch.equal(p2, p_alone)
    assert not torch.equal(p, d1)
    check("plms_after_ddim_vs_reference", p, g["z"], 1e-3)


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_plms_sampler_host_hooks_match_reference(golden, precision):
    """score_corrector / callback / img_callback send PLMSSampler.sample to its host loop (apply_model + maa_ddim_update): the
    corrector is called S + 1 times (twice at step 0, the second time at t_next), every step's pred_x0, the logs and the result
    match the reference's run."""
    from audiogpt_amd.ldm.latent_diffusion import LatentDiffusionAudio
    from audiogpt_amd.ldm.plms import PLMSSampler
    g = golden("plms_t2a_host_hooks_s4")
    model = LatentDiffusionAudio(C.LDM_T2A, device="cuda:0", precision=precision)
    sampler = PLMSSampler(model)
    t = lambda k: torch.from_numpy(g[k]).cuda()
    gain, shift = float(g["gain"]), float(g["shift"])
    calls = []

    class Corrector:
        def modify_score(self, m, e_t, x, ts, c, gain, shift):
            assert m is model and ts.dtype == torch.long and c.shape[0] == x.shape[0]
            calls.append(int(ts[0]))
            return gain * e_t + shift * x * (ts.float() / 1000.0).reshape(-1, 1, 1, 1)

    seen, preds = [], []
    z, inter = sampler.sample(S=int(g["S"]), conditioning=t("c"), batch_size=2, shape=list(g["x_T"].shape[1:]), verbose=False,
                              unconditional_guidance_scale=float(g["scale"]), unconditional_conditioning=t("uc"), x_T=t("x_T"),
                              log_every_t=int(g["log_every_t"]), score_corrector=Corrector(),
                              corrector_kwargs=dict(gain=gain, shift=shift), callback=seen.append,
                              img_callback=lambda p, i: preds.append((i, p.clone())))
    n = len(g["ddim_timesteps"])
    assert seen == g["callback_i"].tolist() == [i for i, _ in preds]
    assert calls == g["corrector_t"].tolist() and len(calls) == n + 1
    tol = 2e-3 if precision == "bf16x3" else 1e-3
    for i, p in preds:
        check(f"plms_{precision}_host_hooks_pred_x0_{i}", p, g["pred_x0_steps"][i], tol)
    assert len(inter["x_inter"]) == g["x_log"].shape[0] + 1
    for i in range(g["x_log"].shape[0]):
        check(f"plms_{precision}_host_hooks_x_log{i}", inter["x_inter"][i + 1], g["x_log"][i], tol)
    check(f"plms_{precision}_host_hooks_z", z, g["z"], tol)
    with pytest.raises(AttributeError):          # the KL first stage has no quantize (plms.py:213-214), as in the reference
        sampler.sample(S=4, conditioning=t("c"), batch_size=2, shape=list(g["x_T"].shape[1:]), verbose=False, x_T=t("x_T"),
                       quantize_x0=True)


def test_plms_sampler_device_path_matches_reference_and_draws_as_the_reference(golden):
    """PLMSSampler.sample without host hooks runs the device loop: result and logs against the reference; a seeded device
    generator ends where the reference loop's draws (two at step 0, one per later step) leave it."""
    from audiogpt_amd.ldm.latent_diffusion import LatentDiffusionAudio
    from audiogpt_amd.ldm.plms import PLMSSampler
    g = golden("plms_t2a_s10")
    model = LatentDiffusionAudio(C.LDM_T2A, device="cuda:0", precision="f32")
    sampler = PLMSSampler(model)
    t = lambda k: torch.from_numpy(g[k]).cuda()
    shape = tuple(g["x_T"].shape)
    torch.cuda.manual_seed(2025)
    z, inter = sampler.sample(S=int(g["S"]), conditioning=t("c"), batch_size=2, shape=list(shape[1:]), verbose=False,
                              unconditional_guidance_scale=float(g["scale"]), unconditional_conditioning=t("uc"), x_T=t("x_T"),
                              log_every_t=int(g["log_every_t"]))
    after = torch.cuda.get_rng_state()
    torch.cuda.manual_seed(2025)
    for _ in range(len(g["ddim_timesteps"]) + 1):
        torch.randn(shape, device="cuda")
    assert torch.equal(torch.cuda.get_rng_state(), after)
    check("plms_dropin_z_vs_reference", z, g["z"], 1e-3)
    assert len(inter["x_inter"]) == g["x_log"].shape[0] + 1 and torch.equal(inter["x_inter"][0].cpu(), _t(g["x_T"]))
    for i in range(g["x_log"].shape[0]):
        check(f"plms_dropin_x_log{i}", inter["x_inter"][i + 1], g["x_log"][i], 1e-3)
        check(f"plms_dropin_x0_log{i}", inter["pred_x0"][i + 1], g["x0_log"][i], 1e-3)


def test_generate_with_plms_is_unet_plms_then_vae_and_vocoder(golden):
    from audiogpt_amd import _lib as L
    from audiogpt_amd.pipeline import MakeAnAudio, ddim_schedule
    g = golden("plms_t2a_s10")
    m = MakeAnAudio("cuda:0", ldm=C.LDM_T2A, vocoder_cfg=C.HIFIGAN_16K, seeds=(0, 1, 2), precision="f32")
    try:
        x, c, uc, scale, S = _t(g["x_T"]), _t(g["c"]), _t(g["uc"]), float(g["scale"]), 6
        wav, spec, z = m.generate(x, c, uc, scale, S, sampler="plms")
        steps, a, ap = ddim_schedule(S, m.alphas_cumprod)
        z_ref = m.unet.plms_sample(x, steps, a, ap, cond=c, uncond=uc, scale=scale)
        spec_ref = m.vae.decode_spec(z_ref, m.scale_factor)
        wav_ref = m.vocoder(spec_ref)[:, 0]
        assert torch.equal(z.cpu(), z_ref.cpu()) and torch.equal(spec.cpu(), spec_ref.cpu()) and torch.equal(wav.cpu(), wav_ref.cpu())
        z_ddim = m.generate(x, c, uc, scale, S)[2]
        assert torch.equal(z_ddim.cpu(), m.unet.ddim_sample(x, steps, a, ap, cond=c, uncond=uc, scale=scale).cpu())
        with pytest.raises(L.MaaError, match="sampler"):
            m.generate(x, c, uc, scale, S, sampler="dpm")
    finally:
        m.close()
