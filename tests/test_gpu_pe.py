"""DiffSinger's PitchExtractor on the device (csrc/pitch_extractor.cpp, pitch.hip) and the e2e tail mel -> f0 -> NSF waveform
(audiogpt_amd/diffsinger.py: PitchExtractor, DiffSingerE2E).

Golden: tests/golden/pe_*.npz, the reference's own PitchExtractor on the CPU (tests/golden/make_golden_pe.py); weights are
WT.make_pe_state_dict(cfg, seed=13) with the generator's two linear-bias values.  Gates: the project's one-evaluation gates,
1e-4 (f32) and 2e-4 (bf16x3) of max|reference|, on mel_hidden and pitch_pred.  f0 is a threshold (voicing logit > 0) and an
exponential of pitch_pred, so it is held to what those gates imply: zero / non-zero as the reference except on frames whose
reference |logit| lies within gate * max|pitch_pred| of 0 (the generator asserts the goldens have at most 1 % of those, none
under 100 frames), voiced frames within ln 2 * gate * max|pitch_pred| * f0 ('log') or gate * max|pitch_pred| * f0_std
('standard'), padding frames exactly 0.

The waveform is compared with the CPU oracle fed the DEVICE's f0: the sine source integrates f0 over T * hop samples, so
rounding-level f0 differences move the top harmonics' phase by more than a waveform gate allows."""
import math

import numpy as np
import pytest
import torch

from audiogpt_amd import config as C
from audiogpt_amd import weights as WT
from tests import pe_ref as R
from tests.util import check

pytestmark = pytest.mark.gpu

PRECISIONS = [("f32", 1e-4), ("bf16x3", 2e-4)]


@pytest.fixture(scope="module")
def contexts():
    from audiogpt_amd.backend import Context
    made = {}

    def get(precision):
        if precision not in made:
            made[precision] = Context("cuda:0", precision=precision)
        return made[precision]
    yield get
    for ctx in made.values():
        ctx.close()


def _pe(ctx, cfg, sd):
    from audiogpt_amd.backend import PitchExtractor
    return PitchExtractor(ctx, cfg, sd)


@pytest.mark.parametrize("precision,tol", PRECISIONS)
@pytest.mark.parametrize("name,prefix", R.CASES)
def test_matches_reference(contexts, name, prefix, precision, tol):
    cfg, sd, g = R.load_case(name, prefix)
    pe = _pe(contexts(precision), cfg, sd)
    mel = torch.from_numpy(g["mel"])
    pp, f0, hidden = pe.forward(mel, return_hidden=True)
    pp, f0, hidden = pp.cpu(), f0.cpu(), hidden.cpu()
    pe.close()
    tag = "%s_pe_%s%s" % (precision, name[3:], prefix.rstrip("."))
    check(tag + "_mel_hidden_vs_reference", hidden, g["mel_hidden"], tol)
    check(tag + "_pitch_pred_vs_reference", pp, g["pitch_pred"], tol)
    ref_pp, ref_f0 = torch.from_numpy(g["pitch_pred"]), torch.from_numpy(g["f0_denorm_pred"])
    assert torch.isfinite(f0).all()
    margin = tol * float(ref_pp.abs().max())
    frames = ref_f0.numel()
    differ = (f0 == 0) != (ref_f0 == 0)
    near = ref_pp[..., 1].abs() <= margin
    print(tag, "frames", frames, "voiced", int((ref_f0 != 0).sum()), "zero/non-zero differs on", int(differ.sum()), "near the threshold", int(near.sum()))
    assert not bool((differ & ~near).any()), "voicing differs on a frame whose logit is clear of the threshold"
    assert int(differ.sum()) <= (frames // 100 if frames >= 100 else 0)
    pad = mel.abs().sum(-1) == 0
    assert bool((f0[pad] == 0).all())
    both = (f0 != 0) & (ref_f0 != 0)
    err = (f0 - ref_f0).abs()[both]
    bound = math.log(2) * margin * ref_f0[both].abs() if cfg["pitch_norm"] == "log" else torch.full_like(err, margin * cfg["f0_std"])
    if err.numel():
        print(tag, "f0 worst err / bound %.3f" % float((err / bound).max()))
    assert bool((err <= bound).all())


@pytest.mark.parametrize("precision,tol", PRECISIONS)
def test_batch_rows_are_independent(contexts, precision, tol):
    cfg, sd, g = R.load_case("pe_b3_t37")
    pe = _pe(contexts(precision), cfg, sd)
    mel = torch.from_numpy(g["mel"]).cuda()
    pp, f0, hidden = pe.forward(mel, return_hidden=True)
    for b in range(mel.shape[0]):
        pp1, f01, hidden1 = pe.forward(mel[b:b + 1], return_hidden=True)
        assert torch.equal(hidden1, hidden[b:b + 1]), b
        assert torch.equal(pp1, pp[b:b + 1]), b
        assert torch.equal(f01, f0[b:b + 1]), b
    pe.close()


@pytest.fixture(scope="module")
def nsf():
    cfg = C.HIFIGAN_NSF_24K
    return cfg, WT.make_vocoder_state_dict(cfg, seed=6), int(np.prod(cfg["upsample_rates"]))


@pytest.mark.parametrize("precision,tol", PRECISIONS)
def test_mel_to_wav_chain(contexts, nsf, precision, tol):
    from audiogpt_amd.backend import Vocoder
    from audiogpt_amd.diffsinger import DiffSingerE2E, PitchExtractor
    from oracle import nsf as N
    from oracle import vocoder as O_voc
    vcfg, vsd, hop = nsf
    cfg, sd, g = R.load_case("pe_cl0_b2_t37")
    ctx = contexts(precision)
    voc = Vocoder(ctx, vcfg, vsd)
    pe = PitchExtractor(cfg, state_dict=sd, ctx=ctx)
    assert pe.eval() is pe and pe.to("cuda:0") is pe
    mel = torch.from_numpy(g["mel"])
    B, T, _ = mel.shape
    rand_ini, noise = N.draw_source_noise(9, B, T * hop)
    e2e = DiffSingerE2E(None, voc, pe=pe)
    wav = e2e.mel_to_wav(mel.cuda(), rand_ini=rand_ini, noise=noise)
    assert tuple(wav.shape) == (1, B * T * hop)
    ret = pe(mel.cuda())
    assert set(ret) == {"pitch_pred", "f0_denorm_pred"} and ret["f0_denorm_pred"].is_cuda
    f0 = ret["f0_denorm_pred"]
    direct = voc.forward_f0(mel.cuda().transpose(1, 2), f0, rand_ini=rand_ini, noise=noise).reshape(1, -1)
    assert torch.equal(wav, direct)
    assert torch.equal(e2e.run_vocoder(mel.cuda(), f0=f0, rand_ini=rand_ini, noise=noise), direct)
    # the waveform against the CPU oracle on the device's own f0
    folded = O_voc.fold_weight_norm(vsd)
    with torch.no_grad():
        ref = N.hifigan_nsf_forward(folded, vcfg, mel.transpose(1, 2), f0.cpu(), rand_ini, noise)
    check(f"{precision}_pe_mel_to_wav_vs_oracle_on_device_f0", wav.cpu().reshape(-1), ref.reshape(-1), 2e-4)
    # the branches of run_vocoder (base_svs_infer.py:61-70)
    plain = voc.forward(mel.cuda().transpose(1, 2)).reshape(1, -1)
    assert torch.equal(DiffSingerE2E(None, voc, pe=pe, use_nsf=False).mel_to_wav(mel.cuda()), plain)
    assert torch.equal(DiffSingerE2E(None, voc, pe=None).mel_to_wav(mel.cuda()), plain)
    assert torch.equal(e2e.run_vocoder(mel.cuda()), plain)
    assert tuple(plain.shape) == (1, B * T * hop)
    with torch.no_grad():
        ref_plain = O_voc.hifigan_forward(folded, vcfg, mel.transpose(1, 2))
    check(f"{precision}_pe_run_vocoder_without_f0_vs_oracle", plain.cpu().reshape(-1), ref_plain.reshape(-1), 2e-4)
    voc.close()


def test_infer_end_to_end(contexts, nsf):
    from audiogpt_amd.backend import Vocoder
    from audiogpt_amd.diffsinger import DiffSingerE2E, GaussianDiffusion, PitchExtractor
    from oracle import nsf as N
    vcfg, vsd, hop = nsf
    ctx = contexts("bf16x3")
    cfg = dict(C.DIFFSINGER_POPCS_BETA6, K_step=4)
    gd = GaussianDiffusion(cfg, ctx=ctx)
    e2e = DiffSingerE2E(gd, Vocoder(ctx, vcfg, vsd), pe=PitchExtractor(ctx=ctx))
    B, T = 2, 33
    gen = torch.Generator().manual_seed(17)
    fs2 = torch.rand(B, T, 80, generator=gen) * 6.0 - 5.0
    cond = torch.randn(B, 256, T, generator=gen)
    noise = torch.randn(B, 1, 80, T, generator=gen)
    noise_p = torch.randn(4, B, 1, 80, T, generator=gen)
    mel2ph = torch.ones(B, T, dtype=torch.long)
    mel2ph[0, T - 4:] = 0
    rand_ini, noise_sine = N.draw_source_noise(3, B, T * hop)
    draws = dict(noise=noise.cuda(), noise_p=noise_p.cuda())
    wav = e2e.infer(fs2, cond.cuda(), mel2ph=mel2ph, rand_ini=rand_ini, noise_sine=noise_sine, **draws)
    assert tuple(wav.shape) == (1, B * T * hop) and wav.is_cuda and bool(torch.isfinite(wav).all())
    mel = gd.infer(fs2, cond.cuda(), mel2ph=mel2ph, **draws)
    assert mel.is_cuda and bool((mel[0, T - 4:] == 0).all())
    assert torch.equal(wav, e2e.mel_to_wav(mel, rand_ini=rand_ini, noise=noise_sine))
    f0 = e2e.pe(mel)["f0_denorm_pred"]
    assert bool((f0[0, T - 4:] == 0).all())          # the frames mel2ph zeroed are padding to the extractor
    e2e.vocoder.close()
