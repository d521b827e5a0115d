"""The row kernels of the Glow post-net run in reverse (csrc/glow.hip) and of the plain FastSpeech2 (csrc/fs2.hip) as the models
launch them, one launch at a time through maa_op_tts_rows, which forwards every argument of the library's internal launches; and
the same code at utterance length through the model handles.  The goldens of tests/test_gpu_glow.py and test_gpu_fs2_plain.py stop
at 33 tokens, 160-channel rows and 150 squeezed frames; here the channel loops go round a second time and end on a partial round,
the token scan crosses waves and 256-token rounds, the log-determinant sum goes round, every nullable argument is given and
null, and every output is held to a float64 reference on the CPU (tests/tts_rows_ref.py).

Gates of the operator tests are the project's operator gates, rel-max against float64: 1e-5 for elementwise work, 2e-5 where a
reduction follows (the energy head's dot product, rowld); integers, masks, copies and in-place / batch-invariance comparisons
exactly; the log-determinant sum at the rounding bound of its fixed order (tts_rows_ref.logdet_bound).  The two model-length tests
use the one-evaluation gates of the model tests, 1e-4 (f32) and 2e-4 (bf16x3) of max|reference|.  tests/test_tts_rows_ref.py
shows on the CPU that torch's own fp32 kernels stay within half of these gates on every input used here, and that the predicted
energies keep the distance from a bin edge that the exact comparison of the bins relies on.

Every output of an operator call has 8 spare rows of a sentinel behind it, so that a store past the last row shows up with every
access still inside an allocation.

Findings that are not bugs:
  * No gate had to move: torch's fp32 evaluation of the references is at most 5 % of its gate on these inputs, the block tail at
    |logs| = 3 and at the floor of log(1e-6 + sigmoid(.)) included (0.9 % and 4.9 % of 1e-5).
  * The block tail's exp(-logs) of ActNorm comes from the host; the reference takes the same fp32 array, so the comparison holds
    the kernel, not the host's exponential.
  * fs2_embed_plain reads row 0 of the table for a negative token but keeps the row live and counts it; the reference module has no
    negative tokens.  The test pins the clamp, as test_embedding_clamps does for the MIDI form."""
import functools

import pytest
import torch

from tests import fs2_plain_ref as FP
from tests import glow_ref as G
from tests import tts_rows_ref as R
from tests.test_gpu_seq_ops import DEV, PRECISIONS, padded, taken
from tests.util import check

pytestmark = pytest.mark.gpu

F64 = torch.float64
I32 = torch.int32


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


def bits(t):
    return t.contiguous().view(I32)


def dev(t, dtype=None):
    return None if t is None else (t if dtype is None else t.to(dtype)).contiguous().to(DEV)


# ---------------------------------------------------------------------------------------------------- squeeze

@pytest.mark.parametrize("C", R.SQ_C)
@pytest.mark.parametrize("T", R.SQ_T)
def test_glow_squeeze(ctx, C, T):
    Ts = T // 2
    for B in R.SQ_B:
        rows = B * Ts
        for masked in (False, True):
            z, mask = R.squeeze_input(C, T, B, masked)
            ref, ref_ms = R.squeeze_ref(z, mask)
            for with_mask_out in (True, False):
                out, ms = padded(rows, 2 * C), padded(rows, 1) if with_mask_out else None
                ctx.op_tts_rows("glow_squeeze", d_x=dev(z), d_mask=dev(mask), B=B, T=T, C=C, d_out=out, d_out2=ms)
                out = taken(out, rows, 2 * C)
                assert torch.isfinite(out).all(), "the odd last frame or a frame behind the mask was read into the output"
                assert torch.equal(out.double(), ref), (B, masked)
                if with_mask_out:
                    assert torch.equal(taken(ms, rows, 1).double(), ref_ms)


# ---------------------------------------------------------------------------------------------------- gate

@pytest.mark.parametrize("H", R.GATE_H)
@pytest.mark.parametrize("rows", R.GATE_ROWS)
def test_glow_gate(ctx, H, rows):
    y = R.gate_input(H, rows)
    out = padded(rows, H)
    ctx.op_tts_rows("glow_gate", d_x=dev(y), rows=rows, C=H, d_out=out)
    check("tts_glow_gate_H%d_r%d" % (H, rows), taken(out, rows, H), R.gate_ref(y), R.TOL_ROW)


# ---------------------------------------------------------------------------------------------------- WN residual

def run_wn(ctx, rs, mask, first, last, x, skip):
    """x / skip [rows, H] on the CPU (skip None: NaN, which a first call must not read) -> the two after the call."""
    rows, H = x.shape
    xd = padded(rows, H, src=x)
    sd = padded(rows, H, src=skip if skip is not None else torch.full((rows, H), float("nan")))
    ctx.op_tts_rows("glow_wn_residual", d_x=dev(rs), rows=rows, C=H, d_mask=dev(mask), first=first, last=last, d_out=xd, d_out2=sd)
    return taken(xd, rows, H), taken(sd, rows, H)


@pytest.mark.parametrize("H", R.WN_H)
@pytest.mark.parametrize("rows", R.WN_ROWS)
def test_glow_wn_residual(ctx, H, rows):
    x, rs, mask = R.wn_input(H, rows)
    off = mask == 0
    tag = "tts_glow_wn_residual_H%d_r%d" % (H, rows)
    # a first, a middle and a last layer, each fed the device's own state: the reference's three-layer bookkeeping
    x1, s1 = run_wn(ctx, rs[0], mask, 1, 0, x, None)
    rx1, rs1 = R.wn_step_ref(x, None, rs[0], mask, True, False)
    check(tag + "_first_x", x1, rx1, R.TOL_ROW)
    check(tag + "_first_skip", s1, rs1, R.TOL_ROW)
    x2, s2 = run_wn(ctx, rs[1], mask, 0, 0, x1, s1)
    rx2, rs2 = R.wn_step_ref(rx1, rs1, rs[1], mask, False, False)
    check(tag + "_middle_x", x2, rx2, R.TOL_ROW)
    check(tag + "_middle_skip", s2, rs2, R.TOL_ROW)
    x3, s3 = run_wn(ctx, rs[2], mask, 0, 1, x2, s2)
    _, rs3 = R.wn_step_ref(rx2, rs2, rs[2], mask, False, True)
    check(tag + "_last_skip", s3, rs3, R.TOL_ROW)
    assert torch.equal(bits(x3), bits(x2)), "the last layer touched x"
    # first and last at once: a WN of one layer
    x4, s4 = run_wn(ctx, rs[2], mask, 1, 1, x, None)
    check(tag + "_only_skip", s4, R.wn_step_ref(x, None, rs[2], mask, True, True)[1], R.TOL_ROW)
    assert torch.equal(bits(x4), bits(x))
    for t in (x1, x2, s3, s4):
        assert bool((t[off] == 0).all()), "a masked row is not exact zeros"


# ---------------------------------------------------------------------------------------------------- block tail

def run_bt(ctx, x, eo, mask, winv, an_bias, an_einv, C, sigmoid_scale, first, rowld=None, hiddens=True, inplace=False):
    rows = x.shape[0]
    out = padded(rows, 2 * C, src=x if inplace else None)
    ld = padded(rows, 1, src=rowld)
    hs = [padded(rows, 2 * C) if hiddens else None for _ in range(3)]
    ctx.op_tts_rows("glow_block_tail", d_x=out if inplace else dev(x), d_y=dev(eo), d_mask=dev(mask), rows=rows, C=C,
                    sigmoid_scale=sigmoid_scale, h_winv=winv, h_an_bias=an_bias, h_an_einv=an_einv, first=first, d_out=out, d_rowld=ld,
                    d_h_cpl=hs[0], d_h_inv=hs[1], d_h_act=hs[2])
    return taken(out, rows, 2 * C), taken(ld, rows, 1), [taken(h, rows, 2 * C) for h in hs] if hiddens else None


@pytest.mark.parametrize("C", R.BT_C)
@pytest.mark.parametrize("sigmoid_scale", (0, 1))
def test_glow_block_tail(ctx, C, sigmoid_scale):
    x, eo, mask, winv, an_bias, an_einv, planted = R.bt_input(C, sigmoid_scale)
    args = (x, eo, mask, winv, an_bias, an_einv, C, sigmoid_scale)
    r_cpl, r_inv, r_act, r_ld = R.bt_ref(x, eo, mask, winv, an_bias, an_einv, sigmoid_scale)
    off = mask == 0
    tag = "tts_glow_block_tail_C%d_ss%d" % (C, sigmoid_scale)
    out, ld, hs = run_bt(ctx, *args, first=1)
    check(tag + "_h_cpl", hs[0], r_cpl, R.TOL_ROW)
    assert torch.equal(hs[0][:, :C], x[:, :C]), "the coupling's first half is not a copy of x0"
    check(tag + "_h_inv", hs[1], r_inv, R.TOL_ROW)
    check(tag + "_h_act", hs[2], r_act, R.TOL_ROW)
    check(tag + "_out", out, r_act, R.TOL_ROW)
    assert torch.equal(bits(out), bits(hs[2]))
    check(tag + "_rowld_first", ld, r_ld, R.TOL_REDUCE)
    for t in [out] + hs:
        assert bool((t[off] == 0).all()), "a masked row is not exact zeros"
    assert bool((ld[off] == 0).all())
    # not first: rowld accumulates onto the planted values; hiddens null: the same out
    out2, ld2, _ = run_bt(ctx, *args, first=0, rowld=planted, hiddens=False)
    assert torch.equal(bits(out2), bits(out)), "out depends on the hiddens or on first"
    check(tag + "_rowld_accumulated", ld2, planted.double() + r_ld, R.TOL_REDUCE)
    assert torch.equal(bits(ld2[off]), bits(planted[off])), "a masked row's rowld moved"
    assert torch.equal(bits(ld2[~off]), bits(planted[~off] + ld[~off])), "rowld is not the planted value plus the row's sum"
    # in place
    out3, ld3, hs3 = run_bt(ctx, *args, first=1, inplace=True)
    assert torch.equal(bits(out3), bits(out)) and torch.equal(bits(ld3), bits(ld)), "in place differs from out of place"
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(hs3, hs))
    # a row alone
    for r in (0, 1, 2, R.BT_ROWS - 1):          # live, mask 0.5, masked, the last row
        one, ld1, _ = run_bt(ctx, x[r:r + 1], eo[r:r + 1], mask[r:r + 1], winv, an_bias, an_einv, C, sigmoid_scale, first=1, hiddens=False)
        assert torch.equal(bits(one[0]), bits(out[r])) and torch.equal(bits(ld1), bits(ld[r:r + 1])), "row %d alone differs" % r


# ---------------------------------------------------------------------------------------------------- log-determinant sum

@pytest.mark.parametrize("Ts", R.LD_TS)
@pytest.mark.parametrize("B", R.LD_B)
def test_glow_logdet(ctx, Ts, B):
    rowld, mask = R.logdet_input(Ts, B)
    ref, bound = R.logdet_ref(rowld, mask, R.LD_PER_LEN), R.logdet_bound(rowld, mask, R.LD_PER_LEN)
    got = []
    for _ in range(2):
        out = padded(B, 1)
        ctx.op_tts_rows("glow_logdet", d_x=dev(rowld), d_mask=dev(mask), B=B, T=Ts, alpha=R.LD_PER_LEN, d_out=out)
        got.append(taken(out, B, 1))
    err = (got[0].double() - ref).abs()
    print("tts_glow_logdet Ts %d B %d: worst err / bound %.3f" % (Ts, B, float((err / bound).max())))
    assert bool((err <= bound).all()), (err.tolist(), bound.tolist())
    assert torch.equal(bits(got[0]), bits(got[1])), "two calls differ"


# ---------------------------------------------------------------------------------------------------- token positions, embedding

def run_embed(ctx, tok, E, pe, scale, rel):
    B, T = tok.shape
    H = E.shape[1]
    x, nonpad, hidden = padded(B * T, H), padded(B * T, 1), padded(B * T, 1)
    ctx.op_tts_rows("fs2_embed_plain", d_tok=dev(tok, I32), h_table=E, vocab=E.shape[0], h_pe=pe, pe_rows=pe.shape[0], alpha=scale,
                    rel=rel, B=B, T=T, C=H, d_out=x, d_out2=nonpad, d_out3=hidden)
    return taken(x, B * T, H), taken(nonpad, B * T, 1), taken(hidden, B * T, 1)


@pytest.mark.parametrize("T", R.TP_T)
def test_fs2_token_positions(ctx, T):
    """A table whose row p holds p, a zero embedding and scale 1: the embedding's output is the counted position itself."""
    tok = R.positions_tokens(T)
    x, nonpad, hidden = run_embed(ctx, tok, torch.zeros(R.TP_VOCAB, 4), R.positions_table(T), 1.0, 0)
    want = FP.positions(tok.long())
    got = x.reshape(3, T, 4)
    for c in range(4):
        bad = torch.nonzero(got[..., c].long() != want)
        assert bad.numel() == 0, "positions differ first at (sample, token) %s: %d for %d" % (
            bad[0].tolist(), int(got[..., c][tuple(bad[0])]), int(want[tuple(bad[0])]))
    assert torch.equal(got[..., 0], want.float())
    live = (tok != 0).float().reshape(-1)
    assert torch.equal(nonpad, live) and torch.equal(hidden, 1.0 - live)


@pytest.mark.parametrize("H", R.EMB_H)
@pytest.mark.parametrize("rel", (0, 1))
def test_fs2_embed_plain(ctx, H, rel):
    tok, E, pe, scale = R.embed_input(H, rel)
    ref, live = R.embed_ref(tok, E, pe, scale, rel)
    x, nonpad, hidden = run_embed(ctx, tok, E, pe, scale, rel)
    check("tts_fs2_embed_plain_H%d_rel%d" % (H, rel), x, ref, R.TOL_ROW)
    assert torch.equal(nonpad.double(), live) and torch.equal(hidden.double(), 1.0 - live)
    assert bool((x[live == 0] == 0).all())
    # the clamped ids read the same rows: the same bits
    cl = tok.clamp(max=R.EMB_VOCAB - 1)
    again, _, _ = run_embed(ctx, torch.where(tok < 0, torch.full_like(tok, 1), cl), torch.cat([E[:1], E[:1], E[2:]]), pe, scale, rel)
    assert torch.equal(bits(again), bits(x)), "a token outside the vocabulary does not read the clamped row"


# ---------------------------------------------------------------------------------------------------- speakers

@pytest.mark.parametrize("H", R.SPK_H)
def test_fs2_add_speaker(ctx, H):
    x, spk, mask, m2p = R.add_speaker_input(H)
    rows = R.SPK_B * R.SPK_T
    for form, live in (("mask", mask != 0), ("mel2ph", m2p > 0)):
        out = padded(rows, H)
        ctx.op_tts_rows("fs2_add_speaker", d_x=dev(x), d_spk=dev(spk), B=R.SPK_B, T=R.SPK_T, C=H, d_out=out,
                        d_mask=dev(mask) if form == "mask" else None, d_mel2ph=dev(m2p) if form == "mel2ph" else None)
        out = taken(out, rows, H)
        check("tts_fs2_add_speaker_H%d_%s" % (H, form), out, R.add_speaker_ref(x, spk, live), R.TOL_ROW)
        assert bool((out[~live] == 0).all())


@pytest.mark.parametrize("H", R.SPK_H)
@pytest.mark.parametrize("B", R.GATHER_B)
def test_fs2_speaker_gather(ctx, H, B):
    tabs, ids = R.gather_input(H, B)
    for use_ids, split in ((True, 1), (True, 0), (False, 0), (False, 1)):
        out = padded(3 * B, H)
        ctx.op_tts_rows("fs2_speaker_gather", h_table=tabs[0], h_t1=tabs[1], h_t2=tabs[2], d_ids=dev(ids) if use_ids else None,
                        split=split, n_rows=R.GATHER_ROWS, B=B, C=H, d_out=out)
        want = R.gather_ref(tabs, ids if use_ids else None, split, B)
        assert torch.equal(bits(taken(out, 3 * B, H)), bits(want.reshape(3 * B, H))), (use_ids, split)


# ---------------------------------------------------------------------------------------------------- energy tail

def run_energy(ctx, x, head, m2p, energy, acc, table, spk, H, with_pred, with_bin):
    rows = acc.shape[0]
    out = padded(rows, H)
    pred = padded(rows, 1) if with_pred else None
    ebin = padded(rows, 1, dtype=I32) if with_bin else None
    kw = {}
    if x is not None:
        gamma, beta, w, bias = head
        kw = dict(d_x=dev(x), C=x.shape[1], h_gamma=gamma, h_beta=beta, h_w=w, h_bias=bias, eps=R.EPS, h_table=table)
    ctx.op_tts_rows("fs2_energy_tail", rows=rows, T=R.EN_T, H=H, d_mel2ph=dev(m2p), d_energy=dev(energy), d_y=dev(acc), d_spk=dev(spk),
                    d_energy_pred=pred, d_bin=ebin, d_out=out, **kw)
    return (taken(out, rows, H), taken(pred, rows, 1) if with_pred else None, taken(ebin, rows, 1).long() if with_bin else None)


@pytest.mark.parametrize("C", R.EN_C)
@pytest.mark.parametrize("H", R.EN_H)
def test_fs2_energy_tail(ctx, C, H):
    x, gamma, beta, w, bias = R.energy_head_input(C)
    head = (gamma, beta, w, bias)
    acc, table, spk, m2p = R.energy_rows_input(H)
    planted, planted_bins = R.energy_planted()
    ref_pred = R.energy_head_ref(x, gamma, beta, w, bias)
    ref_bins = R.energy_bin_ref(ref_pred)
    off = m2p <= 0
    tag = "tts_fs2_energy_tail_C%d_H%d" % (C, H)
    # ---- the predicted energy, with a speaker: every output
    dec, pred, ebin = run_energy(ctx, x, head, m2p, None, acc, table, spk, H, True, True)
    check(tag + "_energy_pred", pred, ref_pred, R.TOL_REDUCE)
    assert torch.equal(ebin, ref_bins), "bins differ on frames %s" % torch.nonzero(ebin != ref_bins).flatten().tolist()
    check(tag + "_predicted_spk", dec, R.energy_tail_ref(acc, ref_bins, table, spk, m2p), R.TOL_ROW)
    assert bool((dec[off] == 0).all())
    # ... energy_pred and energy_bin null: the same decoder_inp
    alone, _, _ = run_energy(ctx, x, head, m2p, None, acc, table, spk, H, False, False)
    assert torch.equal(bits(alone), bits(dec))
    # ---- a caller's energy at the bin edges, no speaker: the bins exactly, the prediction still returned
    dec, pred2, ebin = run_energy(ctx, x, head, m2p, planted, acc, table, None, H, True, True)
    assert torch.equal(ebin, planted_bins), "bins differ on frames %s" % torch.nonzero(ebin != planted_bins).flatten().tolist()
    assert torch.equal(bits(pred2), bits(pred))
    check(tag + "_given_nospk", dec, R.energy_tail_ref(acc, planted_bins, table, None, m2p), R.TOL_ROW)
    # ... with the speaker and without energy_pred
    dec, _, ebin = run_energy(ctx, x, head, m2p, planted, acc, table, spk, H, False, True)
    assert torch.equal(ebin, planted_bins)
    check(tag + "_given_spk", dec, R.energy_tail_ref(acc, planted_bins, table, spk, m2p), R.TOL_ROW)
    assert bool((dec[off] == 0).all())
    # ---- no energy branch (x null): the speaker add and the mask alone, and the mask alone
    if C == R.EN_C[0]:
        for s in (spk, None):
            dec, _, _ = run_energy(ctx, None, None, m2p, None, acc, table, s, H, False, False)
            check(tag + "_no_branch_%s" % ("spk" if s is not None else "nospk"), dec, R.energy_tail_ref(acc, None, table, s, m2p), R.TOL_ROW)
            assert bool((dec[off] == 0).all())
        assert torch.equal(bits(dec[~off]), bits(acc[~off]))


# ---------------------------------------------------------------------------------------------------- tgt mask

@pytest.mark.parametrize("rows", R.TGT_ROWS)
def test_fs2_tgt_mask(ctx, rows):
    m2p = R.tgt_input(rows)
    out = padded(rows, 1)
    ctx.op_tts_rows("fs2_tgt_mask", d_mel2ph=dev(m2p), rows=rows, d_out=out)
    assert torch.equal(taken(out, rows, 1), (m2p > 0).float())


# ---------------------------------------------------------------------------------------------------- model lengths

@functools.lru_cache(maxsize=None)
def plain_reference(T):
    cfg, sd = R.plain_cfg()
    tok = R.plain_tokens(T, cfg["vocab_size"])
    return (cfg, sd, tok) + R.plain_encode_ref(sd, cfg, tok, F64)


@pytest.mark.parametrize("precision,tol", PRECISIONS)
@pytest.mark.parametrize("T", R.PLAIN_T)
def test_plain_encode_long(contexts, T, precision, tol):
    """encode at 300 and 600 tokens with padding inside the samples: the token scan crosses waves and 256-token rounds."""
    from audiogpt_amd.diffsinger import FastSpeech2
    cfg, sd, tok, ref_enc, ref_xs, ref_dur = plain_reference(T)
    m = FastSpeech2(cfg, state_dict=sd, ctx=contexts(precision))
    enc, xs, dur, totals = m.net.encode(tok)
    enc, xs, dur, totals = enc.cpu(), xs.cpu(), dur.cpu().long(), totals.cpu().long()
    m.net.close()
    if m.pitch is not None:
        m.pitch.close()
    check("%s_tts_fs2_plain_encode_T%d_encoder_out" % (precision, T), enc, ref_enc, tol)
    check("%s_tts_fs2_plain_encode_T%d_xs" % (precision, T), xs, ref_xs, tol)
    pad = tok == 0
    assert bool((enc[pad] == 0).all()) and bool((xs[pad] == 0).all()) and bool((dur[pad] == 0).all())
    assert torch.equal(totals, dur.sum(1))
    print(precision, "T", T, "durations differing from float64:", int((dur != ref_dur).sum()), "of", dur.numel())


@functools.lru_cache(maxsize=None)
def glow_reference():
    cfg, sd, z, mask, cond = R.glow_long_case()
    x, logdet = G.glow_reverse(sd, cfg, z.double(), mask, cond)
    return cfg, sd, z, mask, cond, x, logdet


@pytest.mark.parametrize("precision,tol", PRECISIONS)
def test_glow_601_frames(contexts, precision, tol):
    """The narrow configuration at T = 601, a ragged batch of two: 300 squeezed rows per sample, so the log-determinant sum goes
    round, and the odd frame is dropped."""
    from audiogpt_amd.generspeech import Glow
    cfg, sd, z, mask, cond, ref_x, ref_logdet = glow_reference()
    glow = Glow(cfg, state_dict=sd, ctx=contexts(precision))
    x, logdet = glow(z.to(DEV), mask.to(DEV), g=None if cond is None else cond.to(DEV), reverse=True)
    x, logdet = x.cpu(), logdet.cpu()
    glow.net.close()
    assert x.shape == (2, cfg["in_channels"], 600)
    check("%s_tts_glow_T601_x" % precision, x, ref_x, tol)
    check("%s_tts_glow_T601_logdet" % precision, logdet, ref_logdet, tol)
    assert bool((x[1, :, 410:] == 0).all()) and bool((x[1, :, :410].abs().amax(0) > 0).all())
