"""DiffSinger's FastSpeech2MIDI on the device (csrc/fs2.cpp, fs2.hip, the masked attention of flash_attn.hip / blocks.cpp) and
the whole chain score -> waveform (audiogpt_amd/diffsinger.py: FastSpeech2MIDI, DiffSingerE2E.forward_model).

Operator: maa_op_attention_masked at heads = 2, dh = 128 against float64 (tests/fs2_ref.py) under the operator gates of
tests/attn_ref.py (rel-max: f32 2e-5, bf16x3 2e-4, bf16 5e-2).

Model: tests/golden/fs2_*.npz, the reference's own FastSpeech2MIDI on the CPU (tests/golden/make_golden_fs2.py); weights are
WT.make_fs2_state_dict(cfg, seed=17) with the generator's duration bias.  Gates: the project's one-evaluation gates, 1e-4 (f32)
and 2e-4 (bf16x3) of max|reference|, on encoder_out, xs, decoder_inp and mel_out; dur_choice and mel2ph exactly (the generator
keeps every live token clear of a rounding boundary by the bf16x3 gate); padding rows exactly 0."""
import numpy as np
import pytest
import torch

from audiogpt_amd import config as C
from audiogpt_amd import weights as WT
from tests import attn_ref as A
from tests import fs2_ref as R
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


def _masked(ctx, q, k, v, hidden):
    """q / k / v [B, N, heads, dh] on the host, hidden [B, Nk] bool -> the operator's output [B, Nq, heads, dh] on the host."""
    B, Nq, heads, dh = q.shape
    Nk, Cc = k.shape[1], heads * dh
    qd, kd, vd = (t.reshape(B, -1, Cc).contiguous().cuda() for t in (q, k, v))
    out = torch.full((B, Nq, Cc), float("nan"), device="cuda")
    ctx.op_attention_masked(qd, Cc, dh, kd, Cc, dh, vd, Cc, dh, B, heads, dh, Nq, Nk, dh ** -0.5, out, Cc,
                            hidden.to(torch.float32).contiguous().cuda())
    return out.cpu().reshape(B, Nq, heads, dh)


@pytest.mark.parametrize("precision", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("N,B,case", R.OP_SHAPES)
def test_masked_attention_vs_float64(contexts, N, B, case, precision):
    q, k, v, hidden = R.op_inputs(N, B, case)
    got = _masked(contexts(precision), q, k, v, hidden)
    assert bool(torch.isfinite(got).all())
    ref = R.masked_attention_ref(q, k, v, R.OP_HEADS, R.OP_DH ** -0.5, hidden)
    check("%s_attention_masked_n%d_%s" % (precision, N, case), got, ref, A.GATE[precision])
    # exactly zero weight on hidden keys: the output does not depend on what they hold
    if bool(hidden.any()):
        k2, v2 = k.clone(), v.clone()
        for b in range(B):
            k2[b, hidden[b]] = 7.0
            v2[b, hidden[b]] = -1e4
        assert torch.equal(_masked(contexts(precision), q, k2, v2, hidden), got)


@pytest.mark.parametrize("precision", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("L", [70, 129])
def test_masked_attention_sharp_hidden_targets(contexts, L, precision):
    alpha = R.OP_DH ** -0.5
    q, k, v, hidden = R.sharp_hidden_qkv(2, R.OP_HEADS, R.OP_DH, L, alpha, 40 + L)
    got = _masked(contexts(precision), q, k, v, hidden)
    assert bool(torch.isfinite(got).all())
    check("%s_attention_masked_sharp_l%d" % (precision, L), got, R.masked_attention_ref(q, k, v, R.OP_HEADS, alpha, hidden), A.GATE[precision])


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_masked_attention_all_hidden_sample_is_zero(contexts, precision):
    """NaN in the reference and unreachable through the model; the operator writes zeros there and leaves the other sample alone."""
    N = 40
    q, k, v = A.random_qkv(2, R.OP_HEADS, R.OP_DH, N, N, 7)
    hidden = torch.zeros(2, N, dtype=torch.bool)
    hidden[1] = True
    got = _masked(contexts(precision), q, k, v, hidden)
    assert bool((got[1] == 0).all())
    ref = R.masked_attention_ref(q[:1], k[:1], v[:1], R.OP_HEADS, R.OP_DH ** -0.5, hidden[:1])
    check("%s_attention_masked_all_hidden_other_sample" % precision, got[:1], ref, A.GATE[precision])


def _fs2(ctx, cfg, sd):
    from audiogpt_amd.diffsinger import FastSpeech2MIDI
    return FastSpeech2MIDI(cfg, state_dict=sd, ctx=ctx)


@pytest.mark.parametrize("precision,tol", PRECISIONS)
@pytest.mark.parametrize("name,prefix", R.CASES)
def test_matches_reference(contexts, name, prefix, precision, tol):
    cfg, sd, g = R.load_case(name, prefix)
    m = _fs2(contexts(precision), cfg, {"fs2." + k: v for k, v in sd.items()})          # (the checkpoint's prefix is accepted)
    assert m.eval() is m and m.to("cuda:0") is m
    inp = R.inputs(g)
    ret = m(inp["txt_tokens"], mel2ph=inp["mel2ph"], infer=True, pitch_midi=inp["pitch_midi"], midi_dur=inp["midi_dur"],
            is_slur=inp["is_slur"])
    enc, xs, dur, _ = m.net.encode(inp["txt_tokens"], inp["pitch_midi"], inp["midi_dur"], inp["is_slur"])
    predicted = inp["mel2ph"] is None
    assert set(ret) == {"decoder_inp", "mel2ph", "dur", "mel_out"} | ({"dur_choice"} if predicted else set())
    assert all(t.is_cuda for t in ret.values())
    B, T = inp["txt_tokens"].shape
    assert tuple(ret["dur"].shape) == ((B, T, 1) if predicted else (B, T)) and ret["mel2ph"].dtype == torch.long
    assert torch.equal(ret["dur"].reshape(B, T), xs)
    tag = "%s_fs2_%s%s" % (precision, name[4:], prefix.rstrip("."))
    # integers first: a wrong duration moves every frame after it
    if predicted:
        assert ret["dur_choice"].dtype == torch.long
        assert torch.equal(ret["dur_choice"].cpu(), torch.from_numpy(g["dur_choice"])), tag
    assert torch.equal(ret["mel2ph"].cpu(), torch.from_numpy(g["mel2ph"])), tag
    check(tag + "_encoder_out_vs_reference", enc, g["encoder_out"], tol)
    check(tag + "_xs_vs_reference", xs, g["xs"], tol)
    check(tag + "_decoder_inp_vs_reference", ret["decoder_inp"], g["decoder_inp"], tol)
    check(tag + "_mel_out_vs_reference", ret["mel_out"], g["mel_out"], tol)
    pad = inp["txt_tokens"] == 0
    assert bool((enc.cpu()[pad] == 0).all()) and bool((xs.cpu()[pad] == 0).all())
    off = torch.from_numpy(g["mel2ph"]) == 0
    assert bool((ret["decoder_inp"].cpu()[off] == 0).all()) and bool((ret["mel_out"].cpu()[off] == 0).all())
    # skip_decoder: the same decoder_inp, no mel_out
    skip = m(inp["txt_tokens"], mel2ph=inp["mel2ph"], skip_decoder=True, pitch_midi=inp["pitch_midi"], midi_dur=inp["midi_dur"],
             is_slur=inp["is_slur"])
    assert "mel_out" not in skip and torch.equal(skip["decoder_inp"], ret["decoder_inp"])
    m.net.close()


@pytest.mark.parametrize("precision,tol", PRECISIONS)
def test_batch_rows_are_independent(contexts, precision, tol):
    """A sample run alone at the same T_txt (its padding kept) equals its rows in the batch bit for bit.  A sample trimmed of its
    padding is not expected to: the LayerNorm of a padding row is its bias, which the FFN convolution carries into live rows."""
    cfg, sd, g = R.load_case("fs2_b2_t33")
    m = _fs2(contexts(precision), cfg, sd)
    inp = R.inputs(g)
    kw = lambda s: dict(pitch_midi=inp["pitch_midi"][s], midi_dur=inp["midi_dur"][s], is_slur=inp["is_slur"][s])      # noqa: E731
    both = m(inp["txt_tokens"], **kw(slice(None)))
    for b in range(inp["txt_tokens"].shape[0]):
        one = m(inp["txt_tokens"][b:b + 1], **kw(slice(b, b + 1)))
        n = one["mel2ph"].shape[1]
        assert n == int((both["mel2ph"][b] > 0).sum())
        assert torch.equal(one["dur"], both["dur"][b:b + 1]) and torch.equal(one["dur_choice"], both["dur_choice"][b:b + 1])
        assert torch.equal(one["mel2ph"], both["mel2ph"][b:b + 1, :n])
        assert torch.equal(one["decoder_inp"], both["decoder_inp"][b:b + 1, :n])
        # the decoder alone at the batch's T_mel (trailing zero frames kept): bit for bit
        dec_inp, mel = m.net.decode(m.net.encode(inp["txt_tokens"][b:b + 1], **kw(slice(b, b + 1)))[0], both["mel2ph"][b:b + 1])
        assert torch.equal(dec_inp, both["decoder_inp"][b:b + 1]) and torch.equal(mel, both["mel_out"][b:b + 1])
    m.net.close()


def test_zero_frame_prediction_is_refused(contexts):
    cfg, sd, g = R.load_case("fs2_short", "t1.")
    sd = dict(sd)
    sd["dur_predictor.linear.weight"] = torch.zeros_like(sd["dur_predictor.linear.weight"])
    sd["dur_predictor.linear.bias"] = torch.tensor([-3.0])          # round(exp(-3) - 1) clamps to 0 frames
    m = _fs2(contexts("bf16x3"), cfg, sd)
    inp = R.inputs(g)
    with pytest.raises(ValueError, match="0 frames"):
        m(inp["txt_tokens"], pitch_midi=inp["pitch_midi"], midi_dur=inp["midi_dur"], is_slur=inp["is_slur"])
    m.net.close()


def test_forward_model_end_to_end(contexts):
    from audiogpt_amd.backend import Vocoder
    from audiogpt_amd.diffsinger import DiffSingerE2E, GaussianDiffusion, PitchExtractor
    from oracle import nsf as N
    vcfg = C.HIFIGAN_NSF_24K
    hop = int(np.prod(vcfg["upsample_rates"]))
    ctx = contexts("bf16x3")
    cfg, sd, g = R.load_case("fs2_b2_t33")
    gd = GaussianDiffusion(dict(C.DIFFSINGER_POPCS_BETA6, K_step=4), ctx=ctx)
    fs2 = _fs2(ctx, cfg, sd)
    e2e = DiffSingerE2E(gd, Vocoder(ctx, vcfg, WT.make_vocoder_state_dict(vcfg, seed=6)), pe=PitchExtractor(ctx=ctx), fs2=fs2)
    inp = R.inputs(g)
    B, T_mel = g["mel2ph"].shape
    gen = torch.Generator().manual_seed(23)
    noise = torch.randn(B, 1, 80, T_mel, generator=gen).cuda()
    noise_p = torch.randn(4, B, 1, 80, T_mel, generator=gen).cuda()
    rand_ini, noise_sine = N.draw_source_noise(5, B, T_mel * hop)
    score = (inp["txt_tokens"], inp["pitch_midi"], inp["midi_dur"], inp["is_slur"])
    wav = e2e.forward_model(*score, noise=noise, noise_p=noise_p, rand_ini=rand_ini, noise_sine=noise_sine)
    assert tuple(wav.shape) == (1, B * T_mel * hop) and wav.is_cuda and bool(torch.isfinite(wav).all())
    # the same pieces chained by hand; predicted durations leave the mel unmasked (the ARGUMENT mel2ph is None)
    ret = fs2(score[0], infer=True, pitch_midi=score[1], midi_dur=score[2], is_slur=score[3])
    mel = gd.infer(ret["mel_out"], ret["decoder_inp"].transpose(1, 2), mel2ph=None, noise=noise, noise_p=noise_p)
    assert bool((mel[1, int((ret["mel2ph"][1] > 0).sum()):] != 0).any())
    assert torch.equal(wav, e2e.mel_to_wav(mel, rand_ini=rand_ini, noise=noise_sine))
    # with the caller's mel2ph the final mask applies
    m2p = ret["mel2ph"]
    wav2 = e2e.forward_model(*score, mel2ph=m2p, noise=noise, noise_p=noise_p, rand_ini=rand_ini, noise_sine=noise_sine)
    mel2 = gd.infer(ret["mel_out"], ret["decoder_inp"].transpose(1, 2), mel2ph=m2p, noise=noise, noise_p=noise_p)
    assert bool((mel2[m2p == 0] == 0).all())
    assert torch.equal(wav2, e2e.mel_to_wav(mel2, rand_ini=rand_ini, noise=noise_sine))
    with pytest.raises(ValueError, match="fs2"):
        DiffSingerE2E(gd, e2e.vocoder).forward_model(*score)
    e2e.vocoder.close()
    fs2.net.close()
