"""The one-wave-per-row kernels of DiffSinger's sequence models as the models launch them (csrc/pitch.hip, fs2.hip and
row_device.h through maa_op_seq_rows, which forwards every argument of the library's internal launches), the growing sinusoid
table (csrc/seq_layers.cpp), and the same code at song length through the model handles: scans that go round more than once,
tables that grow, and grow again, every head width, GroupNorm statistics over samples of different scale, and the edges of the
row guards, the in-place forms, the frame mask and the clamps -- each against a float64 reference on the CPU (tests/seq_ref.py).

Tolerances of the operator tests are the project's operator gates, rel-max against float64: 1e-5 where the operation is a
LayerNorm or an elementwise affine, 2e-5 where a reduction follows it (the heads' dot products, the GroupNorm); integers and masks
exactly.  The long-sequence tests use the one-evaluation gates of the model tests, 1e-4 (f32) and 2e-4 (bf16x3) of
max|reference|.  tests/test_seq_ref.py shows on the CPU that torch's own fp32 kernels stay within half of the operator tolerances
on every input used here, and that the inputs keep the distance from a threshold that the exact comparisons rely on.

Every output of an operator call has 8 spare rows of a sentinel behind it, so that a store past the last row shows up with every
access still inside an allocation.

Findings that are not bugs:
  * gn_relu_res, T = 1, the first_frame placement: the planted group is constant, and torch's own fp32 GroupNorm is 4e-2 .. 7e-2 of
    max|ref| from float64 there (seq_ref.gn_compared); that group is compared on the all-zero sample only, where it is exact.
  * f0_to_coarse has no reference for f0 <= -700 Hz (the logarithm of a non-positive number); the kernel's contract there is bin 1,
    and the test stays above -700 Hz.
  * pos_add is held to the reference's fp32 table with every operation correctly rounded (seq_ref.sinusoid_table_rounded), not to
    torch's own fp32 evaluation of it: torch's exp leaves one to three of the 128 frequencies an ulp high, which ones depends on
    the host, and at row 1056 that is 1.2e-4 in the table.  Against torch's table on the device's host pos_add at T = 1100 was
    1.7e-5 of max|out| with the library's table (glibc's expf / sinf / cosf) within one fp32 ulp of the correctly rounded one; the
    1e-5 gate stands."""
import functools
import math

import pytest
import torch

from tests import fs2_pitch_ref as FP
from tests import fs2_ref as FS
from tests import pe_ref as PE
from tests import seq_ref as R
from tests.util import check

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -12345.0     # spare rows behind every output
PAD = 8
PRECISIONS = [("f32", 1e-4), ("bf16x3", 2e-4)]
F64 = torch.float64


@pytest.fixture(scope="module")
def contexts():
    from audiogpt_amd.backend import Context
    made = {}

    def get(precision):
        if precision not in made:
            made[precision] = Context(DEV, precision=precision)
        return made[precision]
    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def ctx(contexts):
    """The operator tests' context: the row kernels do not depend on the precision mode."""
    return contexts("f32")


def padded(rows, width, dtype=torch.float32, src=None):
    """A device buffer of rows + PAD rows of `width`, the spare rows a sentinel; `src` [rows, width] fills the front."""
    buf = torch.full(((rows + PAD) * width,), SENTINEL, dtype=dtype, device=DEV)
    if src is not None:
        buf[:rows * width] = src.reshape(-1).to(DEV)
    return buf


def taken(buf, rows, width):
    """The first `rows` rows on the CPU, after checking that the sentinel rows did not move."""
    t = buf.cpu()
    assert bool((t[rows * width:] == SENTINEL).all()), "store past the last output row"
    return t[:rows * width].reshape(rows, width) if width > 1 else t[:rows]


# ---------------------------------------------------------------------------------------------------- frame mask

@pytest.mark.parametrize("M", R.FM_BINS)
@pytest.mark.parametrize("rows", R.FM_ROWS)
def test_frame_mask(ctx, M, rows):
    for shift in range(len(R.FM_CONTENTS) if rows < len(R.FM_CONTENTS) else 1):
        x = R.frame_mask_input(M, rows, shift)
        ref = R.frame_mask_ref(x)
        xd = x.to(DEV)
        mask, hidden = padded(rows, 1), padded(rows, 1)
        ctx.op_seq_rows("frame_mask", xd, mask, M, rows=rows, out2=hidden)
        mask, hidden = taken(mask, rows, 1), taken(hidden, rows, 1)
        assert torch.equal(mask, ref), (shift, mask.tolist(), ref.tolist())
        assert torch.equal(hidden, 1.0 - ref)
        alone = padded(rows, 1)
        ctx.op_seq_rows("frame_mask", xd, alone, M, rows=rows)          # hidden null
        assert torch.equal(taken(alone, rows, 1), ref)


# ---------------------------------------------------------------------------------------------------- masked affine

@pytest.mark.parametrize("C", R.AM_C)
@pytest.mark.parametrize("rows", R.AM_ROWS)
@pytest.mark.parametrize("variant", (0, 1))
def test_affine_mask(ctx, C, rows, variant):
    x, scale, shift, mask = R.affine_mask_input(C, rows, variant)
    md = mask.to(DEV)
    for affine in (True, False):
        sc, sh = (scale, shift) if affine else (None, None)
        ref = R.affine_mask_ref(x, sc, sh, mask)
        out = padded(rows, C)
        ctx.op_seq_rows("affine_mask", x.to(DEV), out, C, rows=rows, mask=md, scale=sc, shift=sh)
        out = taken(out, rows, C)
        check("seq_affine_mask_C%d_r%d_v%d_%s" % (C, rows, variant, "affine" if affine else "mask"), out, ref, R.TOL_ROW)
        assert bool((out[mask == 0] == 0).all()), "a masked row is not +-0"
        inplace = padded(rows, C, src=x)
        ctx.op_seq_rows("affine_mask", inplace, inplace, C, rows=rows, mask=md, scale=sc, shift=sh)
        assert torch.equal(taken(inplace, rows, C).view(torch.int32), out.view(torch.int32)), "in place differs from out of place"


# ---------------------------------------------------------------------------------------------------- GroupNorm + ReLU + residual

def run_gn(ctx, y, res, groups, gamma, beta, inplace=False):
    B, T, C = y.shape
    out = padded(B * T, C, src=y if inplace else None)
    ctx.op_seq_rows("gn_relu_res", out if inplace else y.to(DEV), out, C, B=B, T=T, res=res.to(DEV), gamma=gamma, beta=beta,
                    groups=groups, eps=R.EPS)
    return taken(out, B * T, C).reshape(B, T, C)


@pytest.mark.parametrize("C,groups", R.GN_SHAPES)
@pytest.mark.parametrize("T", R.GN_T)
def test_gn_relu_res(ctx, C, groups, T):
    gamma, beta = R.gn_params(C)
    for case in R.GN_CASES:
        y, res = R.gn_input(C, groups, T, case)
        keep = R.gn_compared(C, groups, T, case)
        ref = R.gn_relu_res_ref(y, res, groups, gamma, beta)
        out = run_gn(ctx, y, res, groups, gamma, beta)
        name = "seq_gn_relu_res_C%d_g%d_T%d_%s" % (C, groups, T, case)
        check(name, out[..., keep], ref[..., keep], R.TOL_REDUCE)
        for b in range(R.GN_B):          # each sample against its own size: a table row of another sample cannot hide
            check("%s_b%d" % (name, b), out[b][..., keep], ref[b][..., keep], R.TOL_REDUCE)
        if case == "zero_sample":
            assert torch.equal(out[1], res[1] + torch.relu(beta)), "an all-zero sample is not res + relu(beta)"
        assert torch.equal(run_gn(ctx, y, res, groups, gamma, beta, inplace=True).view(torch.int32), out.view(torch.int32)), \
            "in place differs from out of place"
        for b in (0, R.GN_B - 1):
            one = run_gn(ctx, y[b:b + 1], res[b:b + 1], groups, gamma, beta)
            assert torch.equal(one[0].view(torch.int32), out[b].view(torch.int32)), "a sample alone differs from its rows in the batch"


# ---------------------------------------------------------------------------------------------------- positions + table gather

def run_pos_add(ctx, x, table_rows, with_pos=True):
    B, T, C = x.shape
    out = padded(B * T, C)
    pos = padded(B * T, 1, dtype=torch.int32) if with_pos else None
    ctx.op_seq_rows("pos_add", x.to(DEV), out, C, B=B, T=T, table_rows=table_rows, alpha=R.POS_ALPHA, pos=pos)
    return taken(out, B * T, C).reshape(B, T, C), taken(pos, B * T, 1).reshape(B, T).long() if with_pos else None


def check_pos_add(ctx, T, key, table_rows, tag):
    x = R.pos_input(T, key)
    ref_pos, ref = R.pos_add_ref(x, R.POS_ALPHA)
    out, pos = run_pos_add(ctx, x, table_rows)
    bad = torch.nonzero(pos != ref_pos)
    assert bad.numel() == 0, "positions differ first at (sample, frame) %s: %d for %d" % (
        bad[0].tolist(), int(pos[tuple(bad[0])]), int(ref_pos[tuple(bad[0])]))
    check("seq_pos_add_%s_T%d_%s" % (tag, T, key), out, ref, R.TOL_ROW)
    return out


@pytest.mark.parametrize("T", R.POS_T)
@pytest.mark.parametrize("key", sorted(R.POS_PATTERNS))
def test_pos_add(ctx, T, key):
    out = check_pos_add(ctx, T, key, R.POS_TABLE_ROWS, "rows%d" % R.POS_TABLE_ROWS)
    if T in (65, 513):          # the workspace buffer in place of d_pos: the same output
        again, _ = run_pos_add(ctx, R.pos_input(T, key), R.POS_TABLE_ROWS, with_pos=False)
        assert torch.equal(again, out)


@pytest.mark.parametrize("T", R.POS_GROW_T)
def test_pos_add_table_growth(ctx, T):
    """A table of 300 rows: T = 299 fits it (the positions reach 299), T = 300 is the first that needs row 300, so the table
    grows exactly when T + 1 > rows.  Then a short call on a fresh entry call."""
    for key in sorted(R.POS_PATTERNS):
        check_pos_add(ctx, T, key, R.POS_GROW_ROWS, "rows%d" % R.POS_GROW_ROWS)
    check_pos_add(ctx, 65, "a", R.POS_GROW_ROWS, "rows%d_after_T%d" % (R.POS_GROW_ROWS, T))


# ---------------------------------------------------------------------------------------------------- predictor heads

@pytest.mark.parametrize("C", R.HEAD_C)
@pytest.mark.parametrize("rows", R.HEAD_ROWS)
def test_pitch_head(ctx, C, rows):
    x, gamma, beta, w, bias, mask = R.head_input(C, rows, 2)
    ref = R.head_ref(x, gamma, beta, w, bias)
    margin = R.logit_margin(ref)
    xd, md = x.to(DEV), mask.to(DEV)
    live = mask != 0
    first = None
    for norm in (0, 1):
        for use_uv in (0, 1):
            pp, f0 = padded(rows, 2), padded(rows, 1)
            ctx.op_seq_rows("head", xd, pp, C, rows=rows, mask=md, gamma=gamma, beta=beta, w=w, bias=bias, eps=R.EPS, n_out=2,
                            pitch_norm=norm, f0_mean=R.F0_MEAN, f0_std=R.F0_STD, use_uv=use_uv, out2=f0)
            pp, f0 = taken(pp, rows, 2), taken(f0, rows, 1)
            name = "seq_pitch_head_C%d_r%d_n%d_uv%d" % (C, rows, norm, use_uv)
            check(name, pp, ref, R.TOL_REDUCE)
            first = pp if first is None else first
            assert torch.equal(pp, first), "pitch_pred depends on pitch_norm / use_uv"
            assert torch.isfinite(f0).all()
            ref_f0 = R.denorm_f0(ref, mask, norm, use_uv)
            off = ~live | ((ref[:, 1] > margin) if use_uv else torch.zeros_like(live))
            assert bool((f0[off] == 0).all()), name + ": f0 is not 0 on a masked or an unvoiced row"
            assert bool((ref_f0[off] == 0).all()) and bool((ref_f0[~off] != 0).all())
            err = (f0.double() - ref_f0).abs()[~off]
            bound = math.log(2) * margin * ref_f0[~off].abs() if norm == 0 else torch.full_like(err, margin * R.F0_STD)
            if err.numel():
                print(name, "f0 worst err / bound %.3f" % float((err / bound).max()))
            assert bool((err <= bound).all()), name


@pytest.mark.parametrize("C", R.HEAD_C)
@pytest.mark.parametrize("rows", R.HEAD_ROWS)
def test_duration_head(ctx, C, rows):
    x, gamma, beta, w, bias, mask = R.head_input(C, rows, 1)
    ref = R.head_ref(x, gamma, beta, w, bias)[:, 0] * mask.double()
    xs, dur = padded(rows, 1), padded(rows, 1, dtype=torch.int32)
    ctx.op_seq_rows("head", x.to(DEV), xs, C, rows=rows, mask=mask.to(DEV), gamma=gamma, beta=beta, w=w, bias=bias, eps=R.EPS,
                    n_out=1, dur=dur)
    xs, dur = taken(xs, rows, 1), taken(dur, rows, 1).long()
    check("seq_duration_head_C%d_r%d" % (C, rows), xs, ref, R.TOL_REDUCE)
    assert bool((xs[mask == 0] == 0).all()), "xs is not 0 on a masked row"
    want = R.out2dur(xs)          # float64 on the DEVICE's xs: the inputs keep exp(xs) - 1 clear of every half-integer
    assert torch.equal(dur, want), (dur.tolist(), want.tolist())
    assert torch.equal(dur, R.out2dur(ref))


# ---------------------------------------------------------------------------------------------------- long sequences: FastSpeech2MIDI

def small_fs2_cfg():
    """The golden's configuration and weights (the generator's duration bias included), cut to one encoder and one decoder layer."""
    cfg, sd, _ = FS.load_case("fs2_b2_t33")
    later = tuple("%s.layers.%d." % (s, i) for s in ("encoder", "decoder") for i in range(1, 8))
    return dict(cfg, enc_layers=1, dec_layers=1), {k: v for k, v in sd.items() if not k.startswith(later)}


@pytest.fixture(scope="module")
def fs2_handles(contexts):
    """FastSpeech2MIDI with the golden's weights (the generator's duration bias included), one encoder and one decoder layer."""
    from audiogpt_amd.backend import FastSpeech2MIDI
    made = {}

    def get(precision):
        if precision not in made:
            cfg, sd = small_fs2_cfg()
            made[precision] = FastSpeech2MIDI(contexts(precision), cfg, sd)
        return made[precision]
    yield get
    for m in made.values():
        m.close()


@pytest.mark.parametrize("T", R.LR_T)
def test_length_regulate_long(fs2_handles, T):
    """fs2_length_kernel alone: more than one scan step, a carry across them, trailing frames past the total."""
    m = fs2_handles("f32")
    dur = R.lr_dur()[:, :T].contiguous()
    total = int(dur.clamp_min(0).sum(1).max())
    for T_mel in sorted({max(total, 1), total + 37}):
        got = m.length_regulate(dur, T_mel).cpu().long()
        ref = R.length_regulate_ref(dur, T_mel)
        bad = torch.nonzero(got != ref)
        assert bad.numel() == 0, "T %d, T_mel %d: mel2ph differs first at %s" % (T, T_mel, bad[0].tolist())


@functools.lru_cache(maxsize=None)
def encode_reference():
    cfg, sd = small_fs2_cfg()
    tok, midi, mdur, slur = R.long_score(cfg, 2, 300, 270)
    enc, xs, dur = FS.encode(sd, cfg, tok, midi, mdur.double(), slur, dtype=F64)
    return (tok, midi, mdur, slur), enc, xs, dur


@pytest.mark.parametrize("precision,tol", PRECISIONS)
def test_encode_300_tokens(fs2_handles, precision, tol):
    m = fs2_handles(precision)
    (tok, midi, mdur, slur), ref_enc, ref_xs, ref_dur = encode_reference()
    enc, xs, dur, totals = m.encode(tok, midi, mdur, slur)
    enc, xs, dur, totals = enc.cpu(), xs.cpu(), dur.cpu().long(), totals.cpu().long()
    check("%s_seq_fs2_encode_T300_encoder_out" % precision, enc, ref_enc, tol)
    check("%s_seq_fs2_encode_T300_xs" % precision, xs, ref_xs, tol)
    pad = tok == 0
    assert bool((enc[pad] == 0).all()) and bool((xs[pad] == 0).all()) and bool((dur[pad] == 0).all())
    assert torch.equal(totals, dur.sum(1)), (totals.tolist(), dur.sum(1).tolist())
    print(precision, "durations differing from float64:", int((dur != ref_dur).sum()), "of", dur.numel(), "totals", totals.tolist())
    T_mel = int(totals.max())
    assert T_mel > 256
    assert torch.equal(m.length_regulate(dur, T_mel).cpu().long(), FS.length_regulate(dur))          # on the device's dur


def test_expand_long(fs2_handles):
    """decode(skip_decoder=True) is fs2_expand_kernel alone: exact rows of encoder_out, zeros where mel2ph is 0, and the rows of
    the clamped index where mel2ph is past T or negative (the kernel's stated contract)."""
    m = fs2_handles("f32")
    T, T_mel, H = 300, 1030, 256
    g = R.gen(850)
    enc = torch.randn(2, T, H, generator=g)
    m2p = torch.randint(0, T + 1, (2, T_mel), generator=g)
    m2p[0, 100:140] = 0
    m2p[1, 1000:] = 0
    m2p[0, 0], m2p[1, 1029 - 40] = T, 1
    dec, mel = m.decode(enc, m2p, skip_decoder=True)
    assert mel is None
    assert torch.equal(dec.cpu(), FS.expand(enc, m2p))
    wild = m2p.clone()
    wild[0, 5], wild[1, 7], wild[0, 1029], wild[1, 0] = T + 5, -1, T + 5, -1
    dec, _ = m.decode(enc, wild, skip_decoder=True)
    assert torch.equal(dec.cpu(), FS.expand(enc, wild.clamp(0, T)))


@functools.lru_cache(maxsize=None)
def decoder_reference(T_mel):
    cfg, sd = small_fs2_cfg()
    # a zero tail of one frame at the long lengths: the positions reach T_mel - 1, so T_mel = 2001 reads row 2000, a grown one
    x, m2p = R.decoder_input(T_mel, cfg["hidden_size"], 1 if T_mel > 1000 else T_mel // 4)
    return x, m2p, FS.run_decoder(sd, cfg, x, m2p, F64)


def check_decoder(tag, mel, T_mel, tol):
    _, m2p, ref = decoder_reference(T_mel)
    mel = mel.cpu()
    check(tag, mel, ref, tol)
    assert bool((mel[m2p == 0] == 0).all())


@pytest.mark.parametrize("precision,tol", PRECISIONS)
@pytest.mark.parametrize("T_mel", (1999, 2000, 2001))
def test_decoder_at_the_tables_edge(contexts, T_mel, precision, tol):
    """The decoder's table has 2000 rows: T_mel = 1999 is the last that fits, 2000 and 2001 make it grow.  A fresh handle each."""
    from audiogpt_amd.backend import FastSpeech2MIDI
    cfg, sd = small_fs2_cfg()
    m = FastSpeech2MIDI(contexts(precision), cfg, sd)
    x, m2p, _ = decoder_reference(T_mel)
    mel = m.run_decoder(x, m2p)
    check_decoder("%s_seq_fs2_run_decoder_T%d" % (precision, T_mel), mel, T_mel, tol)
    m.close()


@pytest.mark.parametrize("precision,tol", PRECISIONS)
def test_decoder_grows_twice_then_runs_short(contexts, precision, tol):
    """One handle: T_mel = 2001 (the first growth), 2600 (the second, past the slack of the first) and 129, issued back to back
    with no synchronisation in between, then compared."""
    from audiogpt_amd.backend import FastSpeech2MIDI
    cfg, sd = small_fs2_cfg()
    m = FastSpeech2MIDI(contexts(precision), cfg, sd)
    lengths = (2001, 2600, 129)
    inputs = [(x.to(DEV), p.to(DEV)) for x, p, _ in (decoder_reference(t) for t in lengths)]
    mels = [m.run_decoder(x, p) for x, p in inputs]
    for T_mel, mel in zip(lengths, mels):
        check_decoder("%s_seq_fs2_run_decoder_same_handle_T%d" % (precision, T_mel), mel, T_mel, tol)
    m.close()


def test_embedding_clamps(fs2_handles):
    """Token >= vocab_size, midi >= 300 and slur > 1 read the rows of the clamped ids: the same bits, all finite."""
    m = fs2_handles("f32")
    cfg, _, g = FS.load_case("fs2_b2_t33")
    inp = FS.inputs(g)
    tok, midi, slur = inp["txt_tokens"].clone(), inp["pitch_midi"].clone(), inp["is_slur"].clone()
    live = torch.nonzero(tok[0] != 0).flatten()[:3].tolist()
    tok[0, live[0]], midi[0, live[1]], slur[0, live[2]] = cfg["vocab_size"] + 5, 305, 3
    tok[1, 0], midi[1, 0], slur[1, 0] = cfg["vocab_size"], 300, 2
    wild = m.encode(tok, midi, inp["midi_dur"], slur)
    clamped = m.encode(tok.clamp_max(cfg["vocab_size"] - 1), midi.clamp_max(299), inp["midi_dur"], slur.clamp_max(1))
    for a, b in zip(wild, clamped):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------- long sequences: the pitch branch

def pitch_cfg(**over):
    cfg, sd, _ = FP.load_case("fs2_pitch_given_f0")
    return dict(cfg, **over), sd


def is_pitch(k):
    return k.startswith(("pitch_embed.", "pitch_predictor."))


def check_given_f0(contexts, precision, tol, T_mel):
    from audiogpt_amd.backend import FS2Pitch
    cfg, sd = pitch_cfg(pitch_norm="standard", f0_mean=0.0, f0_std=1.0)          # the caller's f0 is Hz
    net = FS2Pitch(contexts(precision), cfg, {k: v for k, v in sd.items() if is_pitch(k)})
    origin, m2p, f0, bins = R.pitch_given_f0(2, T_mel, cfg["hidden_size"])
    dec, pp, f0d, coarse = net.forward(origin, m2p, f0=f0, uv=torch.zeros_like(f0), return_coarse=True)
    dec, f0d, coarse = dec.cpu(), f0d.cpu(), coarse.cpu().long()
    net.close()
    live = m2p > 0
    bad = torch.nonzero(coarse != bins)
    assert bad.numel() == 0, "bins differ first at %s: %d for %d" % (bad[0].tolist(), int(coarse[tuple(bad[0])]), int(bins[tuple(bad[0])]))
    assert torch.equal(f0d, torch.where(live, f0, torch.zeros_like(f0)))
    ref = (origin.double() + sd["pitch_embed.weight"].double()[bins]) * live.double()[:, :, None]
    check("%s_seq_fs2_pitch_given_f0_T%d_decoder_inp" % (precision, T_mel), dec, ref, tol)
    assert bool((dec[~live] == 0).all()) and bool((coarse[~live] == 1).all())
    assert torch.isfinite(pp).all()


@pytest.mark.parametrize("precision,tol", PRECISIONS)
def test_pitch_branch_with_a_callers_f0_long(contexts, precision, tol):
    check_given_f0(contexts, precision, tol, 1100)


@pytest.mark.parametrize("precision,tol", PRECISIONS)
def test_pitch_branch_table_growth(contexts, precision, tol):
    """T_mel = 4096 needs 4097 rows of the predictor's table of 4096: it grows."""
    check_given_f0(contexts, precision, tol, 4096)


# ---------------------------------------------------------------------------------------------------- long sequences: PitchExtractor

@functools.lru_cache(maxsize=None)
def pe_reference(name, B, T, predictor_hidden=None):
    cfg, sd, g = PE.load_case(name)
    if predictor_hidden is not None:
        from audiogpt_amd import weights as WT
        bias = sd["pitch_predictor.linear.bias"]
        cfg = dict(cfg, predictor_hidden=predictor_hidden)
        sd = WT.make_pe_state_dict(cfg, seed=13)
        sd["pitch_predictor.linear.bias"] = bias
    mel = R.pe_long_mel(B, T) if T > 200 else torch.from_numpy(g["mel"])
    hidden, pp, f0 = PE.forward(sd, cfg, mel.double())
    return cfg, sd, mel, hidden, pp, f0


def check_pe(contexts, precision, tol, tag, name, B, T, predictor_hidden=None):
    """The rules of tests/test_gpu_pe.py: mel_hidden and pitch_pred at the gate; voicing as the reference except on frames whose
    reference logit lies within the gate of 0, at most 1 % of the frames; voiced frames within what the gate implies."""
    from audiogpt_amd.backend import PitchExtractor
    cfg, sd, mel, ref_hidden, ref_pp, ref_f0 = pe_reference(name, B, T, predictor_hidden)
    pe = PitchExtractor(contexts(precision), cfg, sd)
    pp, f0, hidden = pe.forward(mel, return_hidden=True)
    pp, f0, hidden = pp.cpu(), f0.cpu(), hidden.cpu()
    pe.close()
    check(tag + "_mel_hidden", hidden, ref_hidden, tol)
    check(tag + "_pitch_pred", pp, ref_pp, tol)
    assert torch.isfinite(f0).all()
    margin = tol * float(ref_pp.abs().max())
    frames = ref_f0.numel()
    differ = (f0 == 0) != (ref_f0 == 0)
    near = R.near_threshold(ref_pp, tol)
    print(tag, "frames", frames, "voiced", int((ref_f0 != 0).sum()), "zero/non-zero differs on", int(differ.sum()), "near the threshold", int(near.sum()))
    assert not bool((differ & ~near).any()), "voicing differs on a frame whose logit is clear of the threshold"
    assert int(differ.sum()) <= (frames // 100 if frames >= 100 else 0)
    assert bool((f0[mel.abs().sum(-1) == 0] == 0).all())
    both = (f0 != 0) & (ref_f0 != 0)
    err = (f0.double() - ref_f0).abs()[both]
    bound = math.log(2) * margin * ref_f0[both].abs() if cfg["pitch_norm"] == "log" else torch.full_like(err, margin * cfg["f0_std"])
    assert bool((err <= bound).all())


@pytest.mark.parametrize("precision,tol", PRECISIONS)
@pytest.mark.parametrize("name", ("pe_b3_t37", "pe_cl0_b2_t37"))          # conv_layers 2 and 0
def test_pitch_extractor_table_growth(contexts, name, precision, tol):
    """T = 4096 needs 4097 rows of the table of 4096: it grows; the positions cross sixteen scan steps."""
    check_pe(contexts, precision, tol, "%s_seq_%s_T4096" % (precision, name), name, 1, 4096)


@pytest.mark.parametrize("precision,tol", PRECISIONS)
@pytest.mark.parametrize("name", ("pe_b3_t37", "pe_cl0_b2_t37"))
def test_pitch_extractor_600_frames(contexts, name, precision, tol):
    check_pe(contexts, precision, tol, "%s_seq_%s_T600" % (precision, name), name, 2, 600)


# ---------------------------------------------------------------------------------------------------- predictor_hidden = 768: NR = 4 through the models

@pytest.mark.parametrize("precision,tol", PRECISIONS)
def test_pitch_extractor_predictor_768(contexts, precision, tol):
    check_pe(contexts, precision, tol, "%s_seq_pe_ph768" % precision, "pe_b3_t37", 3, 37, predictor_hidden=768)


@functools.lru_cache(maxsize=None)
def fs2_768_reference():
    from audiogpt_amd import weights as WT
    cfg, sd0, g = FS.load_case("fs2_b2_t33")
    cfg = dict(cfg, enc_layers=1, dec_layers=1, predictor_hidden=768)
    sd = WT.make_fs2_state_dict(cfg, seed=17)
    sd["dur_predictor.linear.bias"] = sd0["dur_predictor.linear.bias"]
    inp = FS.inputs(g)
    enc, xs, dur = FS.encode(sd, cfg, inp["txt_tokens"], inp["pitch_midi"], inp["midi_dur"].double(), inp["is_slur"], dtype=F64)
    return cfg, sd, inp, enc, xs, dur


@pytest.mark.parametrize("precision,tol", PRECISIONS)
def test_fs2_duration_predictor_768(contexts, precision, tol):
    from audiogpt_amd.backend import FastSpeech2MIDI
    cfg, sd, inp, ref_enc, ref_xs, ref_dur = fs2_768_reference()
    m = FastSpeech2MIDI(contexts(precision), cfg, sd)
    enc, xs, dur, totals = m.encode(inp["txt_tokens"], inp["pitch_midi"], inp["midi_dur"], inp["is_slur"])
    m.close()
    enc, xs, dur = enc.cpu(), xs.cpu(), dur.cpu().long()
    check("%s_seq_fs2_ph768_encoder_out" % precision, enc, ref_enc, tol)
    check("%s_seq_fs2_ph768_xs" % precision, xs, ref_xs, tol)
    clear = R.dur_clear(xs.double())          # float64 on the device's xs, where exp(xs) - 1 is clear of a half-integer
    assert torch.equal(dur[clear], R.out2dur(xs)[clear])
    assert bool((dur[inp["txt_tokens"] == 0] == 0).all()) and torch.equal(totals.cpu().long(), dur.sum(1))
    print(precision, "durations differing from float64:", int((dur != ref_dur).sum()), "of", dur.numel())


@functools.lru_cache(maxsize=None)
def pitch_768_reference():
    from audiogpt_amd import weights as WT
    cfg0, sd0, g = FP.load_case("fs2_pitch_b2_t33")
    cfg = dict(cfg0, predictor_hidden=768)
    sd = WT.make_fs2_state_dict(cfg, seed=17)
    sd["pitch_predictor.linear.bias"] = sd0["pitch_predictor.linear.bias"]
    origin, m2p = torch.from_numpy(g["decoder_inp_origin"]), torch.from_numpy(g["mel2ph"])
    pp = R.conv_predictor_ref(sd, "pitch_predictor.", origin, cfg["predictor_layers"], cfg["predictor_kernel"], 4096)
    return cfg, sd, origin, m2p, pp


@pytest.mark.parametrize("precision,tol", PRECISIONS)
def test_pitch_branch_predictor_768(contexts, precision, tol):
    from audiogpt_amd.backend import FS2Pitch
    cfg, sd, origin, m2p, ref_pp = pitch_768_reference()
    net = FS2Pitch(contexts(precision), cfg, {k: v for k, v in sd.items() if is_pitch(k)})
    dec, pp, f0d, coarse = net.forward(origin, m2p, return_coarse=True)
    net.close()
    pp, f0d, coarse, dec = pp.cpu(), f0d.cpu(), coarse.cpu().long(), dec.cpu()
    live = m2p > 0
    ref = ref_pp.clone()
    ref[..., 0] = ref[..., 0] * live.double()          # pitch_pred[..., 0] is 0 on a padding frame when f0 was predicted
    check("%s_seq_fs2_pitch_ph768_pitch_pred" % precision, pp, ref, tol)
    # the tail on the DEVICE's prediction: denorm_f0, the bin and the gather are then exact to fp32 rounding
    f_ref, c_ref, dec_ref = FP.tail(cfg, pp, origin, m2p.long(), sd["pitch_embed.weight"])
    margin = tol * float(ref.abs().max())
    clear = ref_pp[..., 1].abs() > margin
    assert torch.equal((pp[..., 1] > 0)[live & clear], (ref_pp[..., 1] > 0)[live & clear])
    assert bool((f0d[~live] == 0).all()) and bool((dec[~live] == 0).all()) and bool((coarse[~live] == 1).all())
    assert int((coarse - c_ref).abs().max()) <= 1
    same = coarse == c_ref
    print(precision, "bins differing from the fp32 tail on the device's prediction:", int((~same).sum()), "of", same.numel())
    assert int((~same).sum()) <= same.numel() // 100
    check("%s_seq_fs2_pitch_ph768_f0_denorm" % precision, f0d, f_ref, 1e-5)
    check("%s_seq_fs2_pitch_ph768_decoder_inp" % precision, dec[same], dec_ref[same], 1e-6)
