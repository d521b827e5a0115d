"""tests/seq_ref.py on the CPU, no library: for every input tests/test_gpu_seq_ops.py uses, torch's own fp32 evaluation of each
reference stays within HALF of the tolerance the GPU test applies to the kernels, the integer references agree between fp32 and
fp64 evaluation, the inputs keep the distance from a threshold that the GPU test's exact comparisons rely on, and make_positions /
length_regulate equal a plain Python loop."""
import math

import numpy as np
import pytest
import torch

from tests import fs2_pitch_ref as FP
from tests import fs2_ref as FS
from tests import norm_ref as N
from tests import pe_ref as PE
from tests import seq_ref as R

F32, F64 = torch.float32, torch.float64


def half(got, ref, tol, what):
    r = N.rel_max(got, ref)
    assert r <= tol / 2, "%s: torch fp32 is %.3e from float64, more than half of %.1e" % (what, r, tol)
    return r


# ---- frame mask

@pytest.mark.parametrize("M", R.FM_BINS)
@pytest.mark.parametrize("rows", R.FM_ROWS)
def test_frame_mask_references_agree(M, rows):
    seen = set()
    for shift in range(len(R.FM_CONTENTS)):
        x = R.frame_mask_input(M, rows, shift)
        m = R.frame_mask_ref(x)
        assert torch.equal(m, R.frame_mask_ref(x, F32)) and torch.equal(m, R.frame_mask_bits(x))
        for r in range(rows):
            kind = R.FM_CONTENTS[(r + shift) % len(R.FM_CONTENTS)]
            seen.add(kind)
            assert float(m[r]) == (0.0 if kind in ("zeros", "neg_zeros") else 1.0), kind
            if kind in ("bin0", "bin_last", "last_lane", "denormal"):
                assert int((x[r] != 0).sum()) == 1
    assert seen == set(R.FM_CONTENTS)
    assert torch.signbit(R.frame_mask_input(M, 2)[1]).all()          # the -0.0 row is -0.0
    assert (M - 4) // 4 == M // 4 - 1 and M - 4 != M - 1             # last_lane: the last lane that holds bins, not the last bin


# ---- masked affine

@pytest.mark.parametrize("C", R.AM_C)
@pytest.mark.parametrize("rows", R.AM_ROWS)
@pytest.mark.parametrize("variant", (0, 1))
def test_affine_mask_fp32_within_half(C, rows, variant):
    x, scale, shift, mask = R.affine_mask_input(C, rows, variant)
    for sc, sh in ((scale, shift), (None, None)):
        ref = R.affine_mask_ref(x, sc, sh, mask)
        got = R.affine_mask_ref(x, sc, sh, mask, F32)
        assert torch.isfinite(got).all()
        half(got, ref, R.TOL_ROW, "affine_mask")
        assert bool((got[mask == 0] == 0).all()) and bool((ref[mask == 0] == 0).all())
    if variant == 0:
        assert float(mask[0]) == 0 and float(mask[-1]) == 0 and float(x.abs().max()) > 0.99 * R.HUGE
        assert rows < 5 or (float(mask[3]) == 0 and float(mask[1]) == 1)


# ---- GroupNorm + ReLU + residual

@pytest.mark.parametrize("C,groups", R.GN_SHAPES)
@pytest.mark.parametrize("T", R.GN_T)
def test_gn_relu_res_fp32_within_half(C, groups, T):
    gamma, beta = R.gn_params(C)
    for case in R.GN_CASES:
        y, res = R.gn_input(C, groups, T, case)
        keep = R.gn_compared(C, groups, T, case)
        ref = R.gn_relu_res_ref(y, res, groups, gamma, beta)[..., keep]
        got = R.gn_relu_res_ref(y, res, groups, gamma, beta, dtype=F32)[..., keep]
        assert bool(keep.all()) or (T == 1 and case == "first_frame" and int((~keep).sum()) == C // groups)
        half(got, ref, R.TOL_REDUCE, "gn_relu_res %s" % case)
        for b in range(R.GN_B):
            half(got[b], ref[b], R.TOL_REDUCE, "gn_relu_res %s sample %d" % (case, b))
        if case == "zero_sample":
            assert torch.equal(ref[1], res[1].double() + torch.relu(beta).double()) and torch.equal(got[1], res[1] + torch.relu(beta))
    y, _ = R.gn_input(C, groups, T, "plain")
    spread = [float(y[b].std()) if y[b].numel() > 1 else 0.0 for b in range(R.GN_B)]
    assert T * C < 64 or spread[1] > 5 * spread[0] > 25 * spread[2], spread          # the samples differ in scale


# ---- positions and the table gather

@pytest.mark.parametrize("T", R.POS_T + R.POS_GROW_T)
@pytest.mark.parametrize("key", sorted(R.POS_PATTERNS))
def test_pos_add_reference(T, key):
    x = R.pos_input(T, key)
    pos, ref = R.pos_add_ref(x, R.POS_ALPHA)
    pos32, got = R.pos_add_ref(x, R.POS_ALPHA, F32)
    assert torch.equal(pos, pos32) and torch.equal(pos, PE.make_positions(x[..., 0].double()))
    half(got, ref, R.TOL_ROW, "pos_add")
    if T <= 257:
        assert torch.equal(pos, R.make_positions_loop(x[..., 0]))
    assert int(pos.max()) <= T and int(pos.min()) == 0 or key == "a" and T < 6
    for b, pattern in enumerate(R.POS_PATTERNS[key]):
        live = R.channel0_live(T, pattern)
        assert torch.equal(x[b, :, 0] != 0, live)
        assert int(pos[b].max()) == int(live.sum())
    if key == "b":
        assert int(pos[0].max()) == 0 and pos[1].tolist() == [0] * (T - 1) + [1] and not bool(x[0].any())


def test_torch_table_is_the_rounded_table_up_to_one_frequency_ulp():
    """pe_ref.sinusoid_table (torch's fp32 exp / sin / cos) against seq_ref.sinusoid_table_rounded: every frequency within one
    ulp, and every entry within what that allows -- the angle p * freq moves by at most two of its own ulps, is rounded once,
    and the sine once more.  Where torch's frequencies are the rounded ones the two tables agree to one ulp of 1."""
    rows, dim = 2601, R.POS_C
    half = dim // 2
    ours, theirs = R.sinusoid_table_rounded(rows, dim), PE.sinusoid_table(rows, dim)
    arg = torch.arange(half, dtype=torch.float) * -(math.log(10000) / (half - 1))
    freq, tfreq = arg.double().exp().float(), arg.exp()
    ulp = torch.from_numpy(np.spacing(freq.numpy()))
    assert bool(((tfreq - freq).abs() <= ulp).all())
    ang = torch.arange(rows, dtype=torch.float).unsqueeze(1) * freq.unsqueeze(0)
    bound = 3.0 * torch.from_numpy(np.spacing(ang.numpy())).double() + 1.2e-7
    d = (ours.double() - theirs.double()).abs()
    assert bool((d <= torch.cat([bound, bound], dim=1)).all()), float(d.max())
    same = torch.cat([tfreq == freq, tfreq == freq])
    assert float(d[:, same].max()) <= 1.2e-7
    assert not bool(ours[0].any()) and float((ours[1:, :half] ** 2 + ours[1:, half:] ** 2 - 1).abs().max()) < 3e-7


def test_pos_patterns_straddle_the_scan_steps():
    live = R.channel0_live(1100, "holes")
    assert not live[63] and not live[64] and live[60] and live[67] and not live[255] and not live[256] and live[249] and live[259]
    assert R.POS_GROW_T[0] + 1 == R.POS_GROW_ROWS and R.POS_GROW_T[1] + 1 > R.POS_GROW_ROWS          # growth exactly from T = 300 on
    assert max(R.POS_T) + 1 <= R.POS_TABLE_ROWS


# ---- heads

@pytest.mark.parametrize("C", R.HEAD_C)
@pytest.mark.parametrize("rows", R.HEAD_ROWS)
def test_pitch_head_reference(C, rows):
    x, gamma, beta, w, bias, mask = R.head_input(C, rows, 2)
    assert float(x.min()) >= 0
    ref = R.head_ref(x, gamma, beta, w, bias)
    got = R.head_ref(x, gamma, beta, w, bias, F32)
    half(got, ref, R.TOL_REDUCE, "pitch head")
    assert R.pitch_head_clear(ref, mask)
    live = mask != 0
    assert torch.equal((got[:, 1] > 0)[live], (ref[:, 1] > 0)[live])          # the voicing: fp32 and fp64 agree
    for norm in (0, 1):
        for use_uv in (0, 1):
            f64, f32 = R.denorm_f0(ref, mask, norm, use_uv), R.denorm_f0(got, mask, norm, use_uv, F32)
            assert torch.equal(f64 == 0, f32 == 0) and bool((f64[~live] == 0).all())
    if rows > 2:
        assert torch.allclose(ref[1], (beta.double() @ w.double().T) + bias.double(), rtol=0, atol=1e-12)          # the constant row
        assert float(x[2].max()) == R.HEAD_LARGE
    if rows == 130:
        assert bool((ref[live, 1] > 0).any()) and bool((ref[live, 1] < 0).any())


@pytest.mark.parametrize("C", R.HEAD_C)
@pytest.mark.parametrize("rows", R.HEAD_ROWS)
def test_duration_head_reference(C, rows):
    x, gamma, beta, w, bias, mask = R.head_input(C, rows, 1)
    ref = R.head_ref(x, gamma, beta, w, bias)[:, 0] * mask.double()
    got = R.head_ref(x, gamma, beta, w, bias, F32)[:, 0] * mask
    half(got, ref, R.TOL_REDUCE, "duration head")
    assert R.dur_head_clear(ref)
    assert torch.equal(R.out2dur(ref), R.out2dur(got))          # fp32 and fp64 agree on every duration
    assert torch.equal(R.out2dur(got), torch.clamp(torch.round(got.exp() - 1.0), min=0).long())          # and fp32 arithmetic too
    assert bool((R.out2dur(ref)[mask == 0] == 0).all())
    if rows == 130:
        d = R.out2dur(ref)
        assert int(d.min()) == 0 and 10 <= int(d.max()) <= 60, (int(d.min()), int(d.max()))


# ---- the long sequences

def test_length_regulate_equals_a_loop():
    dur = R.lr_dur()
    assert int(dur.min()) < 0 and int(dur.max()) == 8 and not bool(dur[0, 500:].any()) and int((dur[1] != 0).sum()) == 1
    for T in R.LR_T:
        d = dur[:, :T] if T < 600 else dur
        total = int(d.clamp_min(0).sum(1).max())
        for T_mel in sorted({max(total, 1), total + 37}):
            ref = R.length_regulate_ref(d, T_mel)
            assert torch.equal(ref, R.length_regulate_loop(d, T_mel)), (T, T_mel)
            assert int(ref.max()) <= T
    assert bool((R.length_regulate_ref(dur, 4000)[:, -37:] == 0).all())


def test_bin_centres_map_exactly_in_fp32():
    hz = R.bin_centres()
    k = torch.arange(1, 256)
    assert torch.equal(FP.f0_to_coarse(hz.float()), k)
    off = (R.coarse_position(hz.float(), F32).double() - k.double()).abs()
    assert float(off.max()) <= 5e-5, float(off.max())
    assert float((R.coarse_position(hz) - k.double()).abs().max()) <= 1e-9
    for f0, b in R.EDGE_F0:
        assert int(FP.f0_to_coarse(torch.tensor([f0]))[0]) == b, f0
    for T_mel in (1100, 4096):
        origin, m2p, f0, bins = R.pitch_given_f0(2, T_mel, 256)
        live = m2p > 0
        assert torch.equal(FP.f0_to_coarse(f0.clone())[live], bins[live]) and bool((bins[~live] == 1).all())
        assert set(bins[live].tolist()) == set(range(1, 256)) and not bool(origin[~live].any())


PE_LONG = (("pe_b3_t37", 1, 4096), ("pe_b3_t37", 2, 600), ("pe_cl0_b2_t37", 1, 4096), ("pe_cl0_b2_t37", 2, 600))


@pytest.mark.parametrize("name,B,T", PE_LONG)
def test_pe_long_inputs_have_few_near_threshold_frames(name, B, T):
    cfg, sd, _ = PE.load_case(name)
    mel = R.pe_long_mel(B, T)
    assert not bool(mel[:, 300:340].any()) and not bool(mel[B - 1, T - T // 10:].any())
    _, pp, f0 = PE.forward(sd, cfg, mel.double())
    near = int(R.near_threshold(pp, 2e-4).sum())
    print(name, B, T, "near-threshold frames", near, "of", B * T, "voiced", int((f0 != 0).sum()))
    assert near <= B * T // 100
    assert bool((f0 != 0).any()) and bool((f0[mel.abs().sum(-1) == 0] == 0).all())


def test_decoder_half_is_forwards_second_half():
    """fs2_ref.decode / run_decoder, factored out of forward, on a golden: the same tensors."""
    cfg, sd, g = FS.load_case("fs2_b2_t33")
    out = FS.forward(sd, cfg, **FS.inputs(g))
    again = FS.decode(sd, cfg, out["encoder_out"], out["mel2ph"])
    assert torch.equal(again["decoder_inp"], out["decoder_inp"]) and torch.equal(again["mel_out"], out["mel_out"])
    assert torch.equal(FS.run_decoder(sd, cfg, out["decoder_inp"], out["mel2ph"]), out["mel_out"])
