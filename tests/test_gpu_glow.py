"""The Glow post-net in reverse on the device (csrc/glow.cpp, glow.hip; audiogpt_amd/generspeech.py: Glow, PostGlow).

Golden: tests/golden/glow_*.npz and postglow_gs_t40.npz, the reference's own Glow class and run_post_glow on the CPU
(tests/golden/make_golden_glow.py); weights are WT.make_glow_state_dict(cfg, seed, coupling_gain) of the golden's stored values.
Gates: the project's one-evaluation gates, 1e-4 (f32) and 2e-4 (bf16x3) of max|reference|, on x, on every entry of hs -- which
localises a wrong channel map to its flow -- and on logdet.  Plain bf16 is recorded only."""
import numpy as np
import pytest
import torch

from tests import glow_ref as R
from tests.util import check, record, rel_err

pytestmark = pytest.mark.gpu

PRECISIONS = [("f32", 1e-4), ("bf16x3", 2e-4)]


@pytest.fixture(scope="module")
def models():
    """(precision, case) -> the reference-surface Glow of the case's weights; cases with the same weights share one handle."""
    from audiogpt_amd.backend import Context
    from audiogpt_amd.generspeech import Glow
    ctxs, made = {}, {}

    def get(precision, name):
        cfg, sd, g = R.load_case(name)
        key = (precision, tuple(g["cfg"]), int(g["weight_seed"]), float(g["coupling_gain"]))
        if key not in made:
            if precision not in ctxs:
                ctxs[precision] = Context("cuda:0", precision=precision)
            made[key] = Glow(cfg, state_dict=sd, ctx=ctxs[precision])
        return made[key], cfg, sd, g
    yield get
    for m in made.values():
        m.net.close()
    for c in ctxs.values():
        c.close()


def _inputs(g):
    t = lambda k: torch.from_numpy(g[k]).cuda() if k in g.files else None          # noqa: E731
    return t("z"), t("mask"), t("g")


def _run(glow, g, hiddens=True):
    z, mask, cond = _inputs(g)
    out = glow(z, mask, g=cond, reverse=True, return_hiddens=hiddens)
    return out[0].cpu(), out[1].cpu(), [h.cpu() for h in out[2]] if hiddens else None


@pytest.mark.parametrize("precision,tol", PRECISIONS)
@pytest.mark.parametrize("name", R.CASES)
def test_matches_reference(models, name, precision, tol):
    glow, cfg, sd, g = models(precision, name)
    x, logdet, hs = _run(glow, g)
    B, _, T = g["z"].shape
    assert x.shape == (B, cfg["in_channels"], 2 * (T // 2)) and logdet.shape == (B,) and len(hs) == 3 * cfg["n_blocks"]
    tag = "%s_%s" % (precision, name)
    for i, h in enumerate(hs):          # (first, so that a wrong channel map is reported at its flow)
        check("%s_hs%02d_vs_reference" % (tag, i), h, g["hs"][i], tol)
    check(tag + "_x_vs_reference", x, g["x"], tol)
    check(tag + "_logdet_vs_reference", logdet, g["logdet"], tol)
    # exact zeros on every masked frame, pairs the mask cuts included; the odd frame is not there at all
    live = torch.from_numpy(g["mask"])[:, 0, 1::2].repeat_interleave(2, dim=1)
    assert bool((x.transpose(1, 2)[live == 0] == 0).all())
    for h in hs:
        assert bool((h.transpose(1, 2)[live[:, ::2] == 0] == 0).all())


@pytest.mark.parametrize("name", ("glow_gs_b2_t37", "glow_variants_b2_t24", "glow_ps_t40"))
def test_plain_bf16_is_recorded(models, name):
    glow, cfg, sd, g = models("bf16", name)
    x, logdet, _ = _run(glow, g, hiddens=False)
    assert torch.isfinite(x).all() and torch.isfinite(logdet).all()
    record("bf16_%s_x_vs_reference" % name, rel_max=rel_err(x, g["x"])[0], recorded_only=True)
    record("bf16_%s_logdet_vs_reference" % name, rel_max=rel_err(logdet, g["logdet"])[0], recorded_only=True)


def test_masked_frames_are_exact_zeros_and_the_odd_frame_is_dropped(models):
    glow, cfg, sd, g = models("bf16x3", "glow_gs_b2_t37")
    x, logdet, _ = _run(glow, g, hiddens=False)
    assert x.shape == (2, 80, 36)          # 37 frames give 36
    assert bool((x[1, :, 20:] == 0).all())          # live length 21: frame 20's pair is cut by the mask
    assert bool((x[1, :, :20].abs().amax(0) > 0).all()) and bool((x[0].abs().amax(0) > 0).all())
    glow3, _, _, g3 = models("bf16x3", "glow_t3")
    assert _run(glow3, g3, hiddens=False)[0].shape == (1, g3["z"].shape[1], 2)


@pytest.mark.parametrize("precision,tol", PRECISIONS)
@pytest.mark.parametrize("name", ("glow_gs_b2_t37", "glow_narrow_b2_t300"))
def test_two_identical_calls_give_identical_bits(models, name, precision, tol):
    glow, cfg, sd, g = models(precision, name)
    a, b = _run(glow, g), _run(glow, g)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(p, q) for p, q in zip(a[2], b[2]))


@pytest.mark.parametrize("precision,tol", PRECISIONS)
@pytest.mark.parametrize("name", ("glow_gs_b2_t37", "glow_narrow_b2_t300"))
def test_a_sample_alone_matches_the_same_sample_in_the_ragged_batch(models, name, precision, tol):
    glow, cfg, sd, g = models(precision, name)
    z, mask, cond = _inputs(g)
    x, logdet = glow(z, mask, g=cond, reverse=True)
    for b in range(z.shape[0]):
        x1, logdet1 = glow(z[b:b + 1], mask[b:b + 1], g=cond[b:b + 1], reverse=True)
        scale = float(np.abs(g["x"]).max())
        assert float((x1 - x[b:b + 1]).abs().max()) <= tol * scale, b
        assert float((logdet1 - logdet[b:b + 1]).abs().max()) <= tol * float(np.abs(g["logdet"]).max()), b


def _postglow_inputs(g):
    return [torch.from_numpy(g[k]).cuda() for k in ("mel_out", "decoder_inp", "spk_embed", "emo_embed", "ref_prosody")]


@pytest.mark.parametrize("precision,tol", PRECISIONS)
def test_postglow_wrapper_matches_the_glow_class_and_the_reference(models, precision, tol):
    """run_post_glow's inference branch: the seeded host draw, the concatenated conditioning and an all-ones mask."""
    from audiogpt_amd.generspeech import PostGlow
    glow, cfg, sd, g = models(precision, "postglow_gs_t40")
    post = PostGlow.__new__(PostGlow)          # (around the module's handle: the same weights are not packed twice)
    post.cfg, post.post_flow, post.ctx, post.device = dict(cfg), glow, glow.ctx, glow.device
    parts = _postglow_inputs(g)
    torch.manual_seed(int(g["draw_seed"]))
    mel = post.infer(*parts)
    assert mel.shape == (1, 40, 80) and mel.is_cuda
    check("%s_postglow_gs_t40_vs_reference" % precision, mel.cpu(), g["x"], tol)
    given = post.infer(*parts, z=torch.from_numpy(g["z"]))
    assert torch.equal(given, mel)                                   # the draw is the golden's z
    cond = R.post_glow_cond(cfg, *[p.cpu() for p in parts])
    x, _ = glow(torch.from_numpy(g["z"]), torch.ones(1, 1, 40), g=cond, reverse=True)
    assert torch.equal(x.transpose(1, 2), mel)                        # an all-ones mask is no mask


@pytest.mark.parametrize("precision,tol", PRECISIONS)
def test_postglow_with_a_callers_z_matches_case_1(models, precision, tol):
    """Case 1's conditioning handed over in PortaSpeech's form, [mel_out | the other 1024 channels], with its z."""
    from audiogpt_amd.generspeech import PostGlow
    glow, cfg, sd, g = models(precision, "glow_gs_t40")
    post = PostGlow.__new__(PostGlow)
    post.cfg, post.post_flow, post.ctx, post.device = dict(cfg), glow, glow.ctx, glow.device
    cond = torch.from_numpy(g["g"]).transpose(1, 2)
    before = torch.get_rng_state()
    mel = post.infer(cond[:, :, :80], cond[:, :, 80:], z=torch.from_numpy(g["z"]))
    assert torch.equal(torch.get_rng_state(), before)
    check("%s_postglow_callers_z_vs_case_1" % precision, mel.cpu().transpose(1, 2), g["x"], tol)


def test_library_refusals_that_need_the_handle(models):
    from audiogpt_amd import _lib
    glow, cfg, sd, g = models("bf16x3", "glow_uncond_t16")
    z = torch.from_numpy(g["z"]).cuda().transpose(1, 2).contiguous()
    with pytest.raises(_lib.MaaError, match="g must be given exactly when"):
        glow.net.reverse(z, torch.zeros(1, 16, 8).cuda(), None)
    one, out = z[:, :1].contiguous(), torch.zeros_like(z)
    with glow.ctx.lock:          # past the Python check: the library's own refusal of a single frame
        st = glow.ctx.lib.maa_glow_reverse(glow.ctx.h, glow.net.h, _lib.dptr(one), None, None, 1, 1, _lib.dptr(out), None, None)
    assert st < 0 and b"T < 2" in glow.ctx.lib.maa_last_error() and not bool(out.any())
