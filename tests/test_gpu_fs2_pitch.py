"""The FastSpeech2MIDI pitch branch on the device (csrc/fs2.cpp: FS2Pitch, run_decoder; fs2.hip: the pitch tail) and the cascade
chain score -> waveform (audiogpt_amd/diffsinger.py: FastSpeech2MIDICascade, DiffSingerCascade).

Reference: tests/golden/fs2_pitch_*.npz, the reference's own FastSpeech2MIDI with use_pitch_embed on the CPU
(tests/golden/make_golden_fs2_pitch.py); weights are WT.make_fs2_state_dict(cfg, seed=17) with the generator's duration bias
and pitch linear.  Gates: the project's one-evaluation gates, 1e-4 (f32) and 2e-4 (bf16x3) of max|reference|.  Integers: the
voicing exactly (the generator keeps every live logit clear of 0 by the bf16x3 gate); the coarse bin exactly on every frame the
generator did not flag and within +-1 on the flagged ones (their bin boundary lies within the gate of the prediction); with a
caller's f0, at bin centres, every bin exactly.  decoder_inp is compared on the rows whose bin is the reference's."""
import numpy as np
import pytest
import torch

from audiogpt_amd import config as C
from audiogpt_amd import weights as WT
from tests import fs2_pitch_ref as P
from tests import fs2_ref as R
from tests.util import check

pytestmark = pytest.mark.gpu

PRECISIONS = [("f32", 1e-4), ("bf16x3", 2e-4)]
PREDICTED = [c for c in P.CASES if c[0] not in P.GIVEN_F0]
GIVEN = [c for c in P.CASES if c[0] in P.GIVEN_F0]


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


def _is_pitch(k):
    return k.startswith(("pitch_embed.", "pitch_predictor."))


def _inner(ctx, cfg, sd):
    from audiogpt_amd.backend import FastSpeech2MIDI
    return FastSpeech2MIDI(ctx, dict(cfg, use_pitch_embed=False), {k: v for k, v in sd.items() if not _is_pitch(k)})


def _t(g, k):
    return torch.from_numpy(g[k]) if k in g else None


def _check_pitch(tag, g, tol, dec, pp, f0d, coarse):
    """The operator-level comparison of one forward with the golden g; coarse int [B, T_mel]."""
    dec, pp, f0d, coarse = dec.cpu(), pp.cpu(), f0d.cpu(), coarse.cpu().long()
    live, fl, ref_c = _t(g, "mel2ph") > 0, _t(g, "flagged"), _t(g, "coarse")
    check(tag + "_pitch_pred_vs_reference", pp, g["pitch_pred"], tol)
    if "uv_in" not in g:          # predicted voicing: exactly the reference's
        assert torch.equal((pp[..., 1] > 0)[live], (_t(g, "pitch_pred")[..., 1] > 0)[live]), tag
    off = _t(g, "f0_denorm") == 0          # unvoiced and padding frames
    assert bool(off[~live].all()) and bool((f0d[off] == 0).all()) and bool((f0d[~off] > 0).all()), tag
    check(tag + "_f0_denorm_vs_reference", f0d, g["f0_denorm"], tol)
    d = (coarse - ref_c).abs()
    print("%s: flagged %d of %d live, bins differing %d" % (tag, int(fl.sum()), int(live.sum()), int((d > 0).sum())))
    assert int(coarse.min()) >= 1 and int(coarse.max()) <= 255
    assert bool((d[~fl] == 0).all()) and int(d.max()) <= 1, tag
    rows = d == 0
    check(tag + "_decoder_inp_vs_reference", dec[rows], _t(g, "decoder_inp")[rows], tol)
    assert bool((dec[~live] == 0).all()) and bool((coarse[~live] == 1).all()), tag
    if "f0_in" in g:
        assert bool(rows.all()), tag


@pytest.mark.parametrize("precision,tol", PRECISIONS)
@pytest.mark.parametrize("name,prefix", P.CASES)
def test_pitch_branch_vs_reference(contexts, name, prefix, precision, tol):
    from audiogpt_amd.backend import FS2Pitch
    cfg, sd, g = P.load_case(name, prefix)
    net = FS2Pitch(contexts(precision), cfg, {k: v for k, v in sd.items() if _is_pitch(k)})
    f0 = _t(g, "f0_in").cuda() if "f0_in" in g else None
    uv = _t(g, "uv_in").cuda() if "uv_in" in g else None
    before = None if f0 is None else f0.clone()
    dec, pp, f0d, coarse = net.forward(_t(g, "decoder_inp_origin"), _t(g, "mel2ph"), f0=f0, uv=uv, return_coarse=True)
    assert dec.is_cuda and coarse.dtype == torch.int32 and tuple(pp.shape) == tuple(g["pitch_pred"].shape)
    _check_pitch("%s_fs2_pitch_%s%s" % (precision, name[10:], prefix.rstrip(".")), g, tol, dec, pp, f0d, coarse)
    if f0 is not None:
        assert torch.equal(f0, before)          # the caller's f0 is only read
    # without the optional output: the same three tensors
    again = net.forward(_t(g, "decoder_inp_origin"), _t(g, "mel2ph"), f0=f0, uv=uv)
    assert len(again) == 3 and all(torch.equal(a, b) for a, b in zip(again, (dec, pp, f0d)))
    net.close()


@pytest.mark.parametrize("precision,tol", PRECISIONS)
@pytest.mark.parametrize("name,prefix", P.CASES)
def test_run_decoder_vs_reference(contexts, name, prefix, precision, tol):
    """Fed the reference's decoder_inp: no dependence on a flagged bin, the predicted cases included."""
    cfg, sd, g = P.load_case(name, prefix)
    m = _inner(contexts(precision), cfg, sd)
    mel = m.run_decoder(_t(g, "decoder_inp"), _t(g, "mel2ph"))
    check("%s_fs2_run_decoder_%s%s" % (precision, name[10:], prefix.rstrip(".")), mel, g["mel_out"], tol)
    assert bool((mel.cpu()[_t(g, "mel2ph") == 0] == 0).all())
    m.close()


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("name,prefix", R.CASES)
def test_run_decoder_is_decodes_second_half(contexts, name, prefix, precision):
    from audiogpt_amd.backend import FastSpeech2MIDI
    cfg, sd, g = R.load_case(name, prefix)
    m = FastSpeech2MIDI(contexts(precision), cfg, sd)
    inp = R.inputs(g)
    enc = m.encode(inp["txt_tokens"], inp["pitch_midi"], inp["midi_dur"], inp["is_slur"])[0]
    dec_inp, mel = m.decode(enc, _t(g, "mel2ph"))
    assert torch.equal(m.run_decoder(dec_inp, _t(g, "mel2ph")), mel)
    m.close()


def _cascade(ctx, cfg, sd):
    from audiogpt_amd.diffsinger import FastSpeech2MIDICascade
    return FastSpeech2MIDICascade(cfg, state_dict=sd, ctx=ctx)


def _call(m, inp, **kw):
    return m(inp["txt_tokens"], mel2ph=inp["mel2ph"], f0=inp["f0"], uv=inp["uv"], infer=True, pitch_midi=inp["pitch_midi"],
             midi_dur=inp["midi_dur"], is_slur=inp["is_slur"], **kw)


@pytest.mark.parametrize("precision,tol", PRECISIONS)
@pytest.mark.parametrize("name,prefix", GIVEN)
def test_cascade_given_f0_matches_reference(contexts, name, prefix, precision, tol):
    cfg, sd, g = P.load_case(name, prefix)
    m = _cascade(contexts(precision), cfg, {"fs2." + k: v for k, v in sd.items()})          # (the checkpoint's prefix is accepted)
    assert m.eval() is m and m.to("cuda:0") is m
    inp = P.inputs(g)
    f0_before = inp["f0"].clone()
    ret = _call(m, inp)
    assert set(ret) == {"decoder_inp", "mel2ph", "dur", "pitch_pred", "f0_denorm", "mel_out"}
    assert all(t.is_cuda for t in ret.values()) and torch.equal(inp["f0"], f0_before)
    tag = "%s_fs2_cascade_%s" % (precision, name[10:])
    assert ret["mel2ph"].dtype == torch.long and torch.equal(ret["mel2ph"].cpu(), _t(g, "mel2ph")), tag
    B, T_mel = g["mel2ph"].shape
    assert tuple(ret["pitch_pred"].shape) == (B, T_mel, 2) and tuple(ret["f0_denorm"].shape) == (B, T_mel)
    check(tag + "_xs_vs_reference", ret["dur"], g["xs"], tol)
    check(tag + "_pitch_pred_vs_reference", ret["pitch_pred"], g["pitch_pred"], tol)
    check(tag + "_f0_denorm_vs_reference", ret["f0_denorm"], g["f0_denorm"], tol)
    assert torch.equal(ret["f0_denorm"].cpu() == 0, _t(g, "f0_denorm") == 0)
    check(tag + "_decoder_inp_vs_reference", ret["decoder_inp"], g["decoder_inp"], tol)
    check(tag + "_mel_out_vs_reference", ret["mel_out"], g["mel_out"], tol)
    off = _t(g, "mel2ph") == 0
    assert bool((ret["decoder_inp"].cpu()[off] == 0).all()) and bool((ret["mel_out"].cpu()[off] == 0).all())
    skip = _call(m, inp, skip_decoder=True)
    assert "mel_out" not in skip and torch.equal(skip["decoder_inp"], ret["decoder_inp"])
    with pytest.raises(ValueError, match="f0"):
        _call(m, dict(inp, f0=inp["f0"][:, :-1]))
    m.net.close(), m.pitch.close()


@pytest.mark.parametrize("precision,tol", PRECISIONS)
@pytest.mark.parametrize("name,prefix", PREDICTED)
def test_cascade_predicted_matches_reference(contexts, name, prefix, precision, tol):
    cfg, sd, g = P.load_case(name, prefix)
    m = _cascade(contexts(precision), cfg, sd)
    inp = P.inputs(g)
    ret = _call(m, inp)
    assert set(ret) == {"decoder_inp", "mel2ph", "dur", "dur_choice", "pitch_pred", "f0_denorm", "mel_out"}
    tag = "%s_fs2_cascade_%s%s" % (precision, name[10:], prefix.rstrip("."))
    # integers first: a wrong duration moves every frame after it
    assert torch.equal(ret["dur_choice"].cpu(), _t(g, "dur_choice")) and torch.equal(ret["mel2ph"].cpu(), _t(g, "mel2ph")), tag
    # the bins are not part of the reference's dict: the same two device calls by hand give them, and the same bits
    enc = m.net.encode(inp["txt_tokens"], inp["pitch_midi"], inp["midi_dur"], inp["is_slur"])[0]
    origin, _ = m.net.decode(enc, ret["mel2ph"], skip_decoder=True)
    dec, pp, f0d, coarse = m.pitch.forward(origin, ret["mel2ph"], return_coarse=True)
    assert torch.equal(dec, ret["decoder_inp"]) and torch.equal(pp, ret["pitch_pred"]) and torch.equal(f0d, ret["f0_denorm"])
    check(tag + "_origin_vs_reference", origin, g["decoder_inp_origin"], tol)
    _check_pitch(tag, g, tol, dec, pp, f0d, coarse)
    off = _t(g, "mel2ph") == 0
    assert bool(torch.isfinite(ret["mel_out"]).all()) and bool((ret["mel_out"].cpu()[off] == 0).all())
    assert torch.equal(ret["mel_out"], m.net.run_decoder(dec, ret["mel2ph"]))
    m.net.close(), m.pitch.close()


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_batch_rows_are_independent(contexts, precision):
    """A sample run alone at the batch's T_txt and T_mel (its padding kept, through a caller's mel2ph) equals its rows in the
    batch bit for bit.  A sample trimmed of its trailing frames is not expected to: the LayerNorm of a padding frame is its bias,
    which the predictor's next convolution carries into live frames."""
    cfg, sd, g = P.load_case("fs2_pitch_b2_t33")
    m = _cascade(contexts(precision), cfg, sd)
    inp = P.inputs(g)
    both = _call(m, inp)
    for b in range(inp["txt_tokens"].shape[0]):
        s = slice(b, b + 1)
        one = m(inp["txt_tokens"][s], mel2ph=both["mel2ph"][s], pitch_midi=inp["pitch_midi"][s], midi_dur=inp["midi_dur"][s],
                is_slur=inp["is_slur"][s])
        for k in ("decoder_inp", "pitch_pred", "f0_denorm", "mel_out"):
            assert torch.equal(one[k], both[k][s]), (b, k)
    m.net.close(), m.pitch.close()


def test_forward_model_end_to_end(contexts):
    from audiogpt_amd.backend import Vocoder
    from audiogpt_amd.diffsinger import DiffSingerCascade, GaussianDiffusion
    from oracle import nsf as N
    vcfg = C.HIFIGAN_NSF_24K
    hop = int(np.prod(vcfg["upsample_rates"]))
    ctx = contexts("bf16x3")
    cfg, sd, g = P.load_case("fs2_pitch_given_f0")
    gd = GaussianDiffusion(dict(C.DIFFSINGER_POPCS_BETA6, K_step=4), ctx=ctx)
    fs2 = _cascade(ctx, cfg, sd)
    voc = Vocoder(ctx, vcfg, WT.make_vocoder_state_dict(vcfg, seed=6))
    chain = DiffSingerCascade(gd, voc, fs2)
    inp = P.inputs(g)
    score = (inp["txt_tokens"], inp["pitch_midi"], inp["midi_dur"], inp["is_slur"])
    # ---- predicted durations, pitch and voicing
    ret = fs2(score[0], infer=True, pitch_midi=score[1], midi_dur=score[2], is_slur=score[3])
    B, T_mel = ret["mel2ph"].shape
    gen = torch.Generator().manual_seed(29)
    noise = torch.randn(B, 1, 80, T_mel, generator=gen).cuda()
    noise_p = torch.randn(4, B, 1, 80, T_mel, generator=gen).cuda()
    rand_ini, noise_sine = N.draw_source_noise(5, B, T_mel * hop)
    wav = chain.forward_model(*score, noise=noise, noise_p=noise_p, rand_ini=rand_ini, noise_sine=noise_sine)
    assert tuple(wav.shape) == (1, B * T_mel * hop) and wav.is_cuda and bool(torch.isfinite(wav).all())
    # the same pieces chained by hand; predicted durations leave the mel unmasked (the ARGUMENT mel2ph is None)
    mel = gd.infer(ret["mel_out"], ret["decoder_inp"].transpose(1, 2), mel2ph=None, noise=noise, noise_p=noise_p)
    assert bool((ret["f0_denorm"] > 0).any()) and bool((ret["f0_denorm"] == 0).any())
    by_hand = voc.forward_f0(mel.transpose(2, 1), ret["f0_denorm"], rand_ini=rand_ini, noise=noise_sine).reshape(-1)[None]
    assert torch.equal(wav, by_hand)
    # the model's f0 reaches the NSF source: without it the waveform is another
    assert not torch.equal(wav, chain.run_vocoder(mel, f0=None))
    assert not torch.equal(wav, chain.run_vocoder(mel, f0=ret["f0_denorm"] * 1.5, rand_ini=rand_ini, noise=noise_sine))
    # ---- a caller's mel2ph, f0 and uv: the final mask applies, and the caller's pitch is the one sung
    T2 = g["mel2ph_in"].shape[1]
    noise2, noise_p2 = noise[..., :T2].contiguous(), noise_p[..., :T2].contiguous()
    rand2, sine2 = N.draw_source_noise(7, B, T2 * hop)
    uv = (inp["f0"] < 7.0).float()
    wav2 = chain.forward_model(*score, mel2ph=inp["mel2ph"], f0=inp["f0"], uv=uv, noise=noise2, noise_p=noise_p2, rand_ini=rand2,
                               noise_sine=sine2)
    ret2 = fs2(score[0], mel2ph=inp["mel2ph"], f0=inp["f0"], uv=uv, pitch_midi=score[1], midi_dur=score[2], is_slur=score[3])
    mel2 = gd.infer(ret2["mel_out"], ret2["decoder_inp"].transpose(1, 2), mel2ph=inp["mel2ph"], noise=noise2, noise_p=noise_p2)
    assert bool((mel2.cpu()[inp["mel2ph"] == 0] == 0).all()) and bool((mel2.cpu()[inp["mel2ph"] > 0] != 0).any())
    assert torch.equal(wav2, chain.run_vocoder(mel2, f0=ret2["f0_denorm"], rand_ini=rand2, noise=sine2))
    assert tuple(wav2.shape) == (1, B * T2 * hop)
    voc.close()
    fs2.net.close(), fs2.pitch.close()
