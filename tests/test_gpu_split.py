"""`split_input_params` on the MI355X: the unfold / fold kernels, maa_unet_forward_split, the three device loops, the host-hook
loop and MakeAnAudio.generate(split=...), against the reference's own apply_model / DDIMSampler / PLMSSampler run with the
attribute set (tests/golden/make_golden_split.py) and against the test-side restatement tests/split_ref.py.

Gates: the UNet's 1e-4 (f32) / 2e-4 (bf16x3) rel-max of test_gpu_models.py for one evaluation, the samplers' latent rel-max 1e-3,
the host-hook path 1e-3 (f32) / 2e-3 (bf16x3).  The stitch itself has a derived bound (split_ref.fold64):
|dev - ref64| <= (n + 2) 2^-24 (sum_l |w e|) / norm with n the number of crops covering the position."""
import os

import numpy as np
import pytest
import torch

from audiogpt_amd import config as C
from audiogpt_amd import weights as WT
from audiogpt_amd._lib import MaaError
from audiogpt_amd.ldm import split as SP
from tests import split_ref as R
from tests.util import check

pytestmark = pytest.mark.gpu

TAGS = [("A", False), ("B", False), ("B", True), ("C", False), ("D", False)]
UNET_TOL = {"f32": 1e-4, "bf16x3": 2e-4}
HOOK_TOL = {"f32": 1e-3, "bf16x3": 2e-3}


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _plan(case, tie=False):
    shape, _, _ = R.CASES[case]
    return SP.plan(R.params(case, tie), shape[2], shape[3], down=2)


@pytest.fixture(scope="module")
def ctx():
    from audiogpt_amd.backend import Context
    c = Context("cuda:0")
    yield c
    c.close()


@pytest.fixture(scope="module", params=["f32", "bf16x3"])
def ldm(request):
    """The model object of the tools with the seeded T2A weights of the goldens (UNet seed 0)."""
    from audiogpt_amd.ldm.latent_diffusion import LatentDiffusionAudio
    m = LatentDiffusionAudio(C.LDM_T2A, device="cuda:0", precision=request.param)
    yield m
    m.__dict__.pop("split_input_params", None)
    m.unet.close()
    m.vae.close()
    m.ctx.close()


def _within(name, dev, ref64, bound):
    d = (dev.detach().cpu().double() - ref64).abs()
    ratio = float((d / bound.clamp_min(1e-300)).max())
    print(f"{name}: max |dev - ref64| / bound = {ratio:.3f} (max abs err {float(d.max()):.3e})")
    assert bool(torch.isfinite(dev).all()) and bool((d <= bound).all()), f"{name}: exceeds the (n + 2) 2^-24 bound by x{ratio:.2f}"


@pytest.mark.parametrize("case", "ABCD")
def test_unfold_is_torch_unfold_bit_for_bit(ctx, case):
    shape, ks, stride = R.CASES[case]
    x = torch.randn(shape, generator=torch.Generator().manual_seed(11))
    z = ctx.op_unfold(x, ks, stride).cpu()
    assert torch.equal(z, R.unfold(x, ks, stride))
    x3 = torch.randn(3, 5, shape[2] + 1, shape[3] + 3, generator=torch.Generator().manual_seed(12))      # odd sizes: the scalar kernel
    ks3, st3 = (ks[0] - 1, ks[1] - 1), (2, 3)
    if (x3.shape[2] - ks3[0]) % 2 == 0 and (x3.shape[3] - ks3[1]) % 3 == 0:
        assert torch.equal(ctx.op_unfold(x3, ks3, st3).cpu(), R.unfold(x3, ks3, st3))


@pytest.mark.parametrize("case,tie", TAGS)
def test_fold_is_the_weighted_stitch_within_its_rounding_bound(ctx, case, tie):
    shape, ks, stride = R.CASES[case]
    p = _plan(case, tie)
    g = torch.Generator().manual_seed(21)
    crops = torch.randn(shape[0] * p.L, shape[1], *ks, generator=g)
    crops[(shape[0] * p.L) // 2] *= 1e4            # a wrong crop index cannot hide
    out = ctx.op_fold(crops, p.weight, shape[2:], ks, stride)
    ref, bound = R.fold64(crops, p.weight, shape[2:], ks, stride)
    _within(f"fold_{case}{'_tie' if tie else ''}", out, ref, bound)


def test_fold_scalar_path_on_sizes_that_are_no_multiple_of_four(ctx):
    ks, stride, size = (7, 15), (2, 3), (13, 39)          # Ly = 4, Lx = 9: up to 4 x 5 crops cover a position
    prm = dict(R.PARAMS, ks=ks, stride=stride)
    p = SP.plan(prm, *size)
    crops = torch.randn(2 * p.L, 3, *ks, generator=torch.Generator().manual_seed(22))
    crops[p.L + 3] *= 1e4
    ref, bound = R.fold64(crops, p.weight, size, ks, stride)
    _within("fold_odd", ctx.op_fold(crops, p.weight, size, ks, stride), ref, bound)


@pytest.mark.parametrize("case,tie", [("A", False), ("B", False), ("B", True)])
def test_forward_split_is_unfold_unet_per_crop_fold_and_matches_the_reference(golden, ldm, case, tie):
    g = golden("split_apply")
    _, ks, stride = R.CASES[case]
    tag = case + ("_tie" if tie else "")
    x, t, c = (_t(g[k + "_" + tag]).cuda() for k in ("x", "t", "c"))
    p = _plan(case, tie)
    unet, B = ldm.unet, x.shape[0]
    z = R.unfold(x, ks, stride)                                        # torch's unfold on the device
    zl = z.reshape(B, p.L, *z.shape[1:])
    per_crop = torch.stack([unet(zl[:, l].contiguous(), t, c) for l in range(p.L)], dim=1).reshape(z.shape[0], -1, *ks)
    batched = unet(z, t.repeat_interleave(p.L), c.repeat_interleave(p.L, dim=0))
    assert torch.equal(batched, per_crop), "the UNet is not batch-invariant over the crop rows"
    y = unet.forward_split(x, t, c, R.params(case, tie))
    ref, bound = R.fold64(per_crop, p.weight, x.shape[2:], ks, stride)
    _within(f"forward_split_{tag}_{ldm.precision}", y, ref, bound)
    check(f"forward_split_{tag}_{ldm.precision}_vs_reference", y, g["y_" + tag], UNET_TOL[ldm.precision])
    ldm.split_input_params = R.params(case, tie)
    try:
        assert torch.equal(ldm.apply_model(x, t, c), y)
    finally:
        del ldm.split_input_params
    assert not torch.equal(ldm.apply_model(x, t, c), y)          # without the attribute: the wide latent whole


def _sample_kw(g):
    return dict(S=int(g["S"]), conditioning=_t(g["c"]).cuda(), batch_size=g["x_T"].shape[0], shape=list(g["x_T"].shape[1:]),
                verbose=False, unconditional_guidance_scale=float(g["scale"]), unconditional_conditioning=_t(g["uc"]).cuda(),
                x_T=_t(g["x_T"]).cuda())


def _tables(S):
    from audiogpt_amd.pipeline import alphas_cumprod_f32, ddim_schedule
    ldm = C.LDM_T2A
    return ddim_schedule(S, alphas_cumprod_f32(ldm["timesteps"], ldm["linear_start"], ldm["linear_end"]))


def test_ddim_sampler_with_the_attribute_matches_the_reference_in_every_arrangement(golden, ldm):
    from audiogpt_amd.backend import reload_tuning
    from audiogpt_amd.ldm.ddim import DDIMSampler
    g = golden("split_ddim_a")
    sampler = DDIMSampler(ldm)
    tag = f"split_ddim_a_{ldm.precision}"
    whole, _ = sampler.sample(**_sample_kw(g))
    check(tag + "_whole_vs_reference", whole, g["z_whole"], 1e-3)
    ldm.split_input_params = R.params("A")
    try:
        z, _ = sampler.sample(**_sample_kw(g))
        assert sampler.ddim_timesteps.tolist() == g["ddim_timesteps"].tolist()
        check(tag + "_vs_reference", z, g["z"], 1e-3)
        z_eta, _ = sampler.sample(eta=float(g["eta"]), _step_noise=(None, _t(g["noise_p"]).cuda()), **_sample_kw(g))
        check(tag + "_eta_vs_reference", z_eta, g["z_eta"], 1e-3)
    finally:
        del ldm.split_input_params
    assert not torch.equal(z, whole)
    # graph / eager, two lanes / one stream, shared prefix on / off: bit-identical
    steps, a, ap = _tables(int(g["S"]))
    kw = dict(cond=_t(g["c"]), uncond=_t(g["uc"]), scale=float(g["scale"]), split=R.params("A"))
    out = {}
    try:
        for lanes in (True, False):
            ldm.ctx.set_cfg_split(lanes)
            for graph in (False, True, True):
                out[lanes, graph, len(out)] = ldm.unet.ddim_sample(_t(g["x_T"]), steps, a, ap, use_graph=graph, **kw).cpu()
        ldm.ctx.set_cfg_split(False)
        os.environ["MAA_CFG_SHARED"] = "0"
        reload_tuning()
        for graph in (False, True):
            out["unshared", graph] = ldm.unet.ddim_sample(_t(g["x_T"]), steps, a, ap, use_graph=graph, **kw).cpu()
    finally:
        os.environ.pop("MAA_CFG_SHARED", None)
        reload_tuning()
        ldm.ctx.set_cfg_split(None)
    for k, v in out.items():
        assert torch.equal(v, z.cpu()), k


def test_plms_sampler_with_the_attribute_matches_the_reference(golden, ldm):
    from audiogpt_amd.ldm.plms import PLMSSampler
    g = golden("split_ddim_a")
    ldm.split_input_params = R.params("A")
    try:
        z, _ = PLMSSampler(ldm).sample(**_sample_kw(g))
    finally:
        del ldm.split_input_params
    check(f"split_plms_a_{ldm.precision}_vs_reference", z, g["z_plms"], 1e-3)
    steps, a, ap = _tables(int(g["S"]))
    kw = dict(cond=_t(g["c"]), uncond=_t(g["uc"]), scale=float(g["scale"]), split=R.params("A"))
    ze = ldm.unet.plms_sample(_t(g["x_T"]), steps, a, ap, use_graph=False, **kw)
    assert torch.equal(ze, z)


def test_decode_after_sample_replays_the_split_step_and_matches_the_reference(golden, ldm):
    from audiogpt_amd.ldm.ddim import DDIMSampler
    g = golden("split_ddim_a")
    sampler = DDIMSampler(ldm)
    ldm.split_input_params = R.params("A")
    try:
        sampler.sample(**_sample_kw(g))
        kw = _sample_kw(g)
        zd = sampler.decode(_t(g["z"]).cuda(), kw["conditioning"], int(g["t_start"]),
                            unconditional_guidance_scale=kw["unconditional_guidance_scale"],
                            unconditional_conditioning=kw["unconditional_conditioning"])
    finally:
        del ldm.split_input_params
    check(f"split_decode_a_{ldm.precision}_vs_reference", zd, g["z_decode"], 1e-3)
    steps, a, ap = _tables(int(g["S"]))
    ze = ldm.unet.ddim_decode(_t(g["z"]), int(g["t_start"]), steps, a, ap, cond=_t(g["c"]), uncond=_t(g["uc"]),
                              scale=float(g["scale"]), split=R.params("A"), use_graph=False)
    assert torch.equal(ze, zd)


@pytest.mark.parametrize("first", ["split", "plain"])
def test_a_kept_step_graph_is_not_replayed_across_the_split(golden, first):
    """One context, the same shapes: a call with the split and a call without it must each capture their own step."""
    from audiogpt_amd.backend import Context, UNet
    g = golden("split_ddim_a")
    steps, a, ap = _tables(int(g["S"]))
    kw = dict(cond=_t(g["c"]), uncond=_t(g["uc"]), scale=float(g["scale"]))
    split = dict(split=R.params("A"))
    order = [split, {}] if first == "split" else [{}, split]
    made = []
    try:
        got = []
        for n in range(2):
            c = Context("cuda:0")
            made.append(c)
            u = UNet(c, C.UNET_T2A, WT.make_unet_state_dict(C.UNET_T2A, seed=0))
            made.append(u)
            if n == 0:
                u.ddim_sample(_t(g["x_T"]), steps, a, ap, **kw, **order[0])
            got.append(u.ddim_sample(_t(g["x_T"]), steps, a, ap, **kw, **order[1]).cpu())
    finally:
        for o in reversed(made):
            o.close()
    assert torch.equal(got[0], got[1])
    check("split_stale_" + first, got[0], g["z"] if order[1] else g["z_whole"], 1e-3)


def test_host_hook_loop_honours_the_attribute(golden, ldm):
    from audiogpt_amd.ldm.ddim import DDIMSampler
    g = golden("split_ddim_a")
    sampler = DDIMSampler(ldm)
    ldm.split_input_params = R.params("A")
    seen = []
    try:
        z_dev, _ = sampler.sample(**_sample_kw(g))
        z_host, _ = sampler.sample(img_callback=lambda p, i: seen.append(i), **_sample_kw(g))
    finally:
        del ldm.split_input_params
    assert seen == list(range(len(g["ddim_timesteps"])))
    check(f"split_host_loop_{ldm.precision}_vs_device_loop", z_host, z_dev, HOOK_TOL[ldm.precision])
    check(f"split_host_loop_{ldm.precision}_vs_reference", z_host, g["z"], HOOK_TOL[ldm.precision])


def test_generate_with_split_is_its_three_stages_and_refuses_too_wide_a_latent(golden):
    from audiogpt_amd.pipeline import MakeAnAudio
    g = golden("split_ddim_a")
    m = MakeAnAudio("cuda:0", ldm=C.LDM_T2A, vocoder_cfg=C.HIFIGAN_16K, seeds=(0, 1, 2), precision="f32")
    try:
        split = dict(R.PARAMS, ks=(10, 16), stride=(10, 8))
        x = torch.randn(1, 4, 10, 40, generator=torch.Generator().manual_seed(31))
        c, uc, scale, S = _t(g["c"])[:1], _t(g["uc"])[:1], 1.5, 2
        wav, spec, z = m.generate(x, c, uc, scale, S, split=split)
        assert tuple(wav.shape) == (1, 40 * 8 * m.vocoder.hop) and tuple(spec.shape) == (1, 80, 320)
        z_ref = m.sample_latents(x, c, uc, scale, S, split=split)
        spec_ref = m.decode(z_ref)
        wav_ref = m.vocode(spec_ref)
        assert torch.equal(z, z_ref) and torch.equal(spec, spec_ref) and torch.equal(wav, wav_ref)
        assert not torch.equal(z, m.sample_latents(x, c, uc, scale, S))
        launches = m.ctx.workspace_bytes()
        w_max = m.MAX_LATENT_POSITIONS // 10
        with pytest.raises(MaaError, match="mid-block attention"):
            m.generate(torch.zeros(1, 4, 10, w_max + 1), c, uc, scale, S, split=dict(R.PARAMS, ks=(10, 16), stride=(10, 1)))
        assert m.ctx.workspace_bytes() == launches
        m.check_latent_size(10, w_max)
    finally:
        m.close()


def test_concat_model_with_the_attribute_raises():
    from audiogpt_amd.ldm.ddim import DDIMSampler
    from audiogpt_amd.ldm.latent_diffusion import LatentDiffusionAudio
    m = LatentDiffusionAudio(C.LDM_INPAINT, device="cuda:0", precision="f32")
    try:
        m.split_input_params = R.params("A")
        x, cc = torch.zeros(1, 4, 8, 40), torch.zeros(1, 5, 8, 40)
        with pytest.raises(MaaError, match="concat"):
            m.apply_model(x, torch.zeros(1, dtype=torch.long), cc)
        with pytest.raises(MaaError, match="concat"):
            DDIMSampler(m).sample(S=4, batch_size=1, shape=[4, 8, 40], conditioning=cc, verbose=False, x_T=x)
        with pytest.raises(MaaError, match="concat"):
            m.unet.ddim_sample(x, *_tables(4), concat=cc, split=R.params("A"))
    finally:
        m.unet.close()
        m.vae.close()
        m.ctx.close()
