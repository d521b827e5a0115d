"""The plain FastSpeech2 on the device (encoder with token-counted positions, speakers, energy branch, and the DiffSpeech chain
on top) against the goldens of the reference's own class (tests/golden/make_golden_fs2_plain.py), in f32 and bf16x3 at the
project's one-evaluation gates, 1e-4 / 2e-4 of max|reference|.  Integers -- durations, mel2ph, voicing, and the bins off the
frames the generator flagged -- are exact."""
import numpy as np
import pytest
import torch

from audiogpt_amd import config as C
from audiogpt_amd import weights as WT
from tests import fs2_pitch_ref as P
from tests import fs2_plain_ref as R
from tests.util import check

pytestmark = pytest.mark.gpu

PRECISIONS = [("f32", 1e-4), ("bf16x3", 2e-4)]
ENERGY_CASES = [c for c in R.CASES if c[0] in ("fs2_plain_energy_spk_b2_t33", "fs2_plain_given", "fs2_plain_short", "fs2_plain_ph384_b2_t9")]
SPEAKER_CASES = [("fs2_plain_energy_spk_b2_t33", ""), ("fs2_plain_given", ""), ("fs2_plain_short", "t4.")]


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


def _t(g, k):
    return torch.from_numpy(g[k]) if k in g else None


def _model(ctx, cfg, sd):
    from audiogpt_amd.diffsinger import FastSpeech2
    return FastSpeech2(cfg, state_dict=sd, ctx=ctx)


def _close(m):
    m.net.close()
    if m.pitch is not None:
        m.pitch.close()


def _tag(precision, what, name, prefix):
    return "%s_fs2_plain_%s_%s%s" % (precision, what, name[10:], prefix.rstrip("."))


@pytest.mark.parametrize("name,prefix", R.PREDICTED)
@pytest.mark.parametrize("precision,tol", PRECISIONS)
def test_encode_plain_vs_reference(contexts, precision, tol, name, prefix):
    """Fails on a port that indexes the positions instead of counting them (fs2_plain_b2_t33: token 11 of sample 0 is padding
    inside the sample) or applies the embedding scale twice."""
    cfg, sd, g = R.load_case(name, prefix)
    m = _model(contexts(precision), cfg, sd)
    tok = _t(g, "txt_tokens")
    spk_dur = _t(g, "spk")[1] if "spk" in g else None
    enc, xs, dur, totals = m.net.encode(tok, spk_dur=spk_dur)
    tag = _tag(precision, "encode", name, prefix)
    check(tag + "_encoder_out_vs_reference", enc, g["encoder_out"], tol)
    check(tag + "_xs_vs_reference", xs, g["xs"], tol)
    assert torch.equal(dur.cpu().long(), _t(g, "dur_choice")), tag
    assert torch.equal(totals.cpu().long(), (_t(g, "mel2ph") > 0).sum(-1)), tag
    m2p = m.net.length_regulate(dur, int(totals.max()))
    assert torch.equal(m2p.cpu().long(), _t(g, "mel2ph")), tag
    pad = tok == 0
    assert bool((enc.cpu()[pad] == 0).all()) and bool((xs.cpu()[pad] == 0).all()) and bool((dur.cpu()[pad] == 0).all())
    origin, none = m.net.decode(enc, m2p, skip_decoder=True)
    assert none is None
    check(tag + "_origin_vs_reference", origin, R.origin(g), tol)
    _close(m)


def test_encode_entries_refuse_the_other_handle(contexts):
    from audiogpt_amd import _lib, backend
    ctx = contexts("f32")
    cfg, sd, g = R.load_case("fs2_plain_relpos_b2_t9")
    plain = backend.FastSpeech2Plain(ctx, dict(cfg, use_pitch_embed=False), sd)
    tok = _t(g, "txt_tokens")
    with pytest.raises(_lib.MaaError, match="maa_fs2_encode_plain"):
        backend.FastSpeech2MIDI.encode(plain, tok, torch.ones_like(tok))
    mcfg = dict(C.FASTSPEECH2_MIDI, enc_layers=1, dec_layers=1)
    midi = backend.FastSpeech2MIDI(ctx, mcfg, WT.make_fs2_state_dict(mcfg, seed=17))
    with pytest.raises(_lib.MaaError, match="call maa_fs2_encode"):
        backend.FastSpeech2Plain.encode(midi, tok)
    with pytest.raises(_lib.MaaError, match="no speaker embedding"):
        plain.speaker(ids=torch.zeros(3, 2, dtype=torch.long))
    plain.close(), midi.close()


@pytest.mark.parametrize("name,prefix", SPEAKER_CASES)
@pytest.mark.parametrize("precision,tol", PRECISIONS)
def test_speaker_vs_reference(contexts, precision, tol, name, prefix):
    cfg, sd, g = R.load_case(name, prefix)
    m = _model(contexts(precision), cfg, sd)
    tag = _tag(precision, "speaker", name, prefix)
    if cfg["use_spk_id"]:
        out = m.net.speaker(ids=_t(g, "spk_ids"))
        assert torch.equal(out.cpu(), _t(g, "spk")), tag          # rows of a table: a copy
        both = m.net.speaker(ids=_t(g, "spk_ids"), vec=torch.zeros(g["spk_ids"].shape[1], 256))      # the handle's mode chooses
        assert torch.equal(both, out)
    else:
        out = m.net.speaker(vec=_t(g, "spk_vec"))
        check(tag + "_projection_vs_reference", out, g["spk"], tol)
        assert torch.equal(out[0], out[1]) and torch.equal(out[0], out[2])
    # the broadcast add and mask: exact in fp32 (one add, one product with 0 or 1)
    origin, m2p = R.origin(g), _t(g, "mel2ph")
    got = m.net.add_speaker(origin, _t(g, "spk")[2], m2p)
    want = (origin + _t(g, "spk")[2][:, None, :]) * (m2p > 0).float()[:, :, None]
    assert torch.equal(got.cpu(), want), tag
    _close(m)


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_pitch_forward_from_with_equal_inputs_is_pitch_forward(contexts, precision):
    """On an existing cascade case: the entry that separates the predictor's input from origin gives maa_fs2_pitch_forward's bits
    when both are the same values (a copy, since the outputs may alias neither)."""
    from audiogpt_amd.backend import FS2Pitch
    cfg, sd, g = P.load_case("fs2_pitch_b2_t33")
    pitch = FS2Pitch(contexts(precision), cfg, {k: v for k, v in sd.items() if k.startswith(("pitch_embed.", "pitch_predictor."))})
    origin, m2p = _t(g, "decoder_inp_origin").cuda(), _t(g, "mel2ph")
    a = pitch.forward(origin, m2p, return_coarse=True)
    b = pitch.forward(origin, m2p, return_coarse=True, pred_inp=origin.clone())
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    f0 = _t(g, "pitch_pred")[..., 0].contiguous()
    a = pitch.forward(origin, m2p, f0=f0)
    b = pitch.forward(origin, m2p, f0=f0, pred_inp=origin.clone())
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    pitch.close()


@pytest.mark.parametrize("precision,tol", PRECISIONS)
def test_pitch_forward_from_with_speakers_vs_reference(contexts, precision, tol):
    cfg, sd, g = R.load_case("fs2_plain_energy_spk_b2_t33")
    m = _model(contexts(precision), cfg, sd)
    origin, m2p = R.origin(g), _t(g, "mel2ph")
    live, fl = m2p > 0, _t(g, "flagged")
    pitch_inp = (origin + _t(g, "spk")[2][:, None, :]) * live.float()[:, :, None]
    dec, pp, f0d, coarse = m.pitch.forward(origin, m2p, return_coarse=True, pred_inp=pitch_inp)
    tag = "%s_fs2_plain_pitch_from_energy_spk" % precision
    check(tag + "_pitch_pred_vs_reference", pp, g["pitch_pred"], tol)
    check(tag + "_f0_denorm_vs_reference", f0d, g["f0_denorm"], tol)
    assert torch.equal((pp.cpu()[..., 1] > 0)[live], (_t(g, "pitch_pred")[..., 1] > 0)[live]), tag
    c = coarse.cpu().long()
    assert torch.equal(c[~fl], _t(g, "coarse")[~fl]) and int((c - _t(g, "coarse")).abs().max()) <= 1, tag
    # the row is added to ORIGIN, not to the predictor's input
    rows = c == _t(g, "coarse")
    want = (origin + sd["pitch_embed.weight"][_t(g, "coarse")]) * live.float()[:, :, None]
    assert torch.equal(dec.cpu()[rows], want[rows]), tag
    # ... and without the speaker the prediction is another
    _, pp0, _ = m.pitch.forward(origin, m2p)
    assert float((pp0.cpu() - _t(g, "pitch_pred")).abs().max()) > 100 * tol * float(np.abs(g["pitch_pred"]).max())
    _close(m)


@pytest.mark.parametrize("name,prefix", ENERGY_CASES)
@pytest.mark.parametrize("precision,tol", PRECISIONS)
def test_finish_vs_reference(contexts, precision, tol, name, prefix):
    """maa_fs2_finish fed the reference's decoder_inp so far and pitch_inp."""
    cfg, sd, g = R.load_case(name, prefix)
    m = _model(contexts(precision), cfg, sd)
    origin, m2p = R.origin(g), _t(g, "mel2ph")
    live, fl = m2p > 0, _t(g, "energy_flagged")
    spk = _t(g, "spk") if "spk" in g else None
    pitch_inp = origin if spk is None else (origin + spk[2][:, None, :]) * live.float()[:, :, None]
    acc = origin + sd["pitch_embed.weight"][_t(g, "coarse")]
    e_in = _t(g, "energy_in")
    before = None if e_in is None else e_in.clone()
    dec, e_pred, e_bin = m.net.finish(pitch_inp, acc, m2p, energy=e_in, spk=None if spk is None else spk[0], return_bin=True)
    assert before is None or torch.equal(e_in, before)
    tag = _tag(precision, "finish", name, prefix)
    check(tag + "_energy_pred_vs_reference", e_pred, g["energy_pred"], tol)
    b = e_bin.cpu().long()
    assert torch.equal(b[~fl], _t(g, "energy_bin")[~fl]) and int((b - _t(g, "energy_bin")).abs().max()) <= 1, tag
    if e_in is not None:
        assert torch.equal(b, _t(g, "energy_bin")), tag
    rows = b == _t(g, "energy_bin")
    ref = _t(g, "decoder_inp")
    err = float((dec.cpu() - ref)[rows].abs().max()) / float(ref.abs().max())
    print("%s: decoder_inp rel max %.3e on %d of %d rows" % (tag, err, int(rows.sum()), rows.numel()))
    assert err <= tol, tag
    assert bool((dec.cpu()[~live] == 0).all()), tag
    # a negative energy handed straight to the entry lands in bin 0 (the reference raises IndexError)
    neg = torch.full(tuple(m2p.shape), -0.75)
    dec0, _, bin0 = m.net.finish(pitch_inp, acc, m2p, energy=neg, spk=None if spk is None else spk[0], return_bin=True)
    assert bool((bin0 == 0).all())
    zero = m.net.finish(pitch_inp, acc, m2p, energy=torch.zeros(tuple(m2p.shape)), spk=None if spk is None else spk[0])[0]
    assert torch.equal(dec0, zero)
    _close(m)


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_finish_without_an_energy_branch_adds_the_speaker_alone(contexts, precision):
    cfg, sd, g = R.load_case("fs2_plain_energy_spk_b2_t33")
    cfg = dict(cfg, use_energy_embed=False)
    m = _model(contexts(precision), cfg, {k: v for k, v in sd.items() if not k.startswith("energy_")})
    origin, m2p = R.origin(g), _t(g, "mel2ph")
    acc = origin + sd["pitch_embed.weight"][_t(g, "coarse")]
    dec, e_pred = m.net.finish(None, acc, m2p, spk=_t(g, "spk")[0])
    assert e_pred is None
    assert torch.equal(dec.cpu(), (acc + _t(g, "spk")[0][:, None, :]) * (m2p > 0).float()[:, :, None])
    _close(m)


@pytest.mark.parametrize("name,prefix", R.CASES)
@pytest.mark.parametrize("precision,tol", PRECISIONS)
def test_forward_vs_reference(contexts, precision, tol, name, prefix):
    cfg, sd, g = R.load_case(name, prefix)
    m = _model(contexts(precision), cfg, sd)
    tok, kw = R.call_args(cfg, g)
    floats = {k: v.clone() for k, v in kw.items() if v is not None and v.is_floating_point()}
    ret = m(tok, **kw)
    assert all(torch.equal(kw[k], v) for k, v in floats.items())          # the caller's f0 / uv / energy are only read
    want = ["dur"] + (["dur_choice"] if "mel2ph_in" not in g else []) + ["mel2ph", "pitch_pred", "f0_denorm"]
    want += (["energy_pred"] if cfg["use_energy_embed"] else []) + ["decoder_inp", "mel_out"]
    assert list(ret) == want and all(t.is_cuda for t in ret.values())          # the reference's keys, in its order
    tag = _tag(precision, "forward", name, prefix)
    if "dur_choice" in g:
        assert torch.equal(ret["dur_choice"].cpu(), _t(g, "dur_choice")), tag
        assert tuple(ret["dur"].shape) == tuple(g["xs"].shape) + (1,)
    assert ret["mel2ph"].dtype == torch.long and torch.equal(ret["mel2ph"].cpu(), _t(g, "mel2ph")), tag
    check(tag + "_xs_vs_reference", ret["dur"].reshape(g["xs"].shape), g["xs"], tol)
    check(tag + "_pitch_pred_vs_reference", ret["pitch_pred"], g["pitch_pred"], tol)
    check(tag + "_f0_denorm_vs_reference", ret["f0_denorm"], g["f0_denorm"], tol)
    live = _t(g, "mel2ph") > 0
    if "uv_in" not in g:
        assert torch.equal((ret["pitch_pred"].cpu()[..., 1] > 0)[live], (_t(g, "pitch_pred")[..., 1] > 0)[live]), tag
    if cfg["use_energy_embed"]:
        check(tag + "_energy_pred_vs_reference", ret["energy_pred"], g["energy_pred"], tol)
    # decoder_inp on the rows no flagged bin touches; mel_out where the device took the reference's bins everywhere, else
    # through run_decoder from the reference's decoder_inp
    clear = ~_t(g, "flagged") & (~_t(g, "energy_flagged") if "energy_flagged" in g else True)
    ref = _t(g, "decoder_inp")
    dec = ret["decoder_inp"].cpu()
    bad = (dec - ref).abs().amax(-1) > tol * float(ref.abs().max())
    assert not bool((bad & clear).any()), (tag, int((bad & clear).sum()))
    assert bool((dec[~live] == 0).all()) and bool((ret["mel_out"].cpu()[~live] == 0).all())
    if not bool(bad.any()):
        check(tag + "_mel_out_vs_reference", ret["mel_out"], g["mel_out"], tol)
    else:
        check(tag + "_mel_out_from_reference_decoder_inp", m.net.run_decoder(ref, _t(g, "mel2ph")), g["mel_out"], tol)
    skip = m(tok, skip_decoder=True, **kw)
    assert "mel_out" not in skip and torch.equal(skip["decoder_inp"], ret["decoder_inp"])
    _close(m)


@pytest.mark.parametrize("name", ["fs2_plain_b2_t33", "fs2_plain_energy_spk_b2_t33"])
@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_batch_rows_are_independent(contexts, precision, name):
    """A sample run alone at the batch's T_txt and T_mel (its padding kept, through a caller's mel2ph) equals its rows in the
    batch bit for bit."""
    cfg, sd, g = R.load_case(name)
    m = _model(contexts(precision), cfg, sd)
    tok, kw = R.call_args(cfg, g)
    both = m(tok, **kw)
    for b in range(tok.shape[0]):
        s = slice(b, b + 1)
        one_kw = {k: (v[s] if v is not None else None) for k, v in kw.items()}
        one = m(tok[s], **dict(one_kw, mel2ph=both["mel2ph"][s]))
        for k in ("decoder_inp", "pitch_pred", "f0_denorm", "mel_out") + (("energy_pred",) if cfg["use_energy_embed"] else ()):
            assert torch.equal(one[k], both[k][s]), (b, k)
    _close(m)


def test_diffspeech_forward_model_is_its_three_stages(contexts, monkeypatch):
    """timesteps 100, K_step 4: forward_model equals fs2 -> GaussianDiffusion.infer -> run_vocoder called one after another, bit
    for bit, with one device-to-host read (the frame totals) with predicted durations and none with a caller's mel2ph."""
    from audiogpt_amd.backend import Vocoder
    from audiogpt_amd.diffsinger import DiffSpeech, FastSpeech2, GaussianDiffusion
    vcfg = C.HIFIGAN_NS_128
    hop = int(np.prod(vcfg["upsample_rates"]))
    ctx = contexts("bf16x3")
    cfg, sd, g = R.load_case("fs2_plain_given")
    gd = GaussianDiffusion(dict(C.DIFFSPEECH_LJ_BETA6, K_step=4), ctx=ctx)
    assert gd.num_timesteps == 100
    fs2 = _model(ctx, cfg, sd)
    voc = Vocoder(ctx, vcfg, WT.make_vocoder_state_dict(vcfg, seed=6))
    chain = DiffSpeech(gd, voc, fs2)
    reads = []
    real = FastSpeech2._read_totals
    monkeypatch.setattr(FastSpeech2, "_read_totals", staticmethod(lambda t: (reads.append(1), real(t))[1]))
    tok, kw = R.call_args(cfg, g)
    vec = kw["spk_embed"]
    # ---- everything predicted
    ret = fs2(tok, spk_embed=vec)
    assert len(reads) == 1
    B, T_mel = ret["mel2ph"].shape
    gen = torch.Generator().manual_seed(31)
    noise = torch.randn(B, 1, 80, T_mel, generator=gen).cuda()
    noise_p = torch.randn(4, B, 1, 80, T_mel, generator=gen).cuda()
    wav = chain.forward_model(tok, spk_embed=vec, noise=noise, noise_p=noise_p)
    assert len(reads) == 2
    assert tuple(wav.shape) == (1, B * T_mel * hop) and wav.is_cuda and bool(torch.isfinite(wav).all())
    mel = gd.infer(ret["mel_out"], ret["decoder_inp"].transpose(1, 2), mel2ph=None, noise=noise, noise_p=noise_p)
    assert torch.equal(wav, chain.run_vocoder(mel))
    # ---- a caller's mel2ph, f0, uv and energy: no read, and the final mask applies
    T2 = g["mel2ph_in"].shape[1]
    noise2, noise_p2 = torch.randn(B, 1, 80, T2, generator=gen).cuda(), torch.randn(4, B, 1, 80, T2, generator=gen).cuda()
    wav2 = chain.forward_model(tok, noise=noise2, noise_p=noise_p2, **kw)
    ret2 = fs2(tok, **kw)
    assert len(reads) == 2
    mel2 = gd.infer(ret2["mel_out"], ret2["decoder_inp"].transpose(1, 2), mel2ph=kw["mel2ph"], noise=noise2, noise_p=noise_p2)
    assert bool((mel2.cpu()[kw["mel2ph"] == 0] == 0).all()) and bool((mel2.cpu()[kw["mel2ph"] > 0] != 0).any())
    assert torch.equal(wav2, chain.run_vocoder(mel2)) and tuple(wav2.shape) == (1, B * T2 * hop)
    voc.close()
    _close(fs2)
